"""nx_zstd_next_frame, the walker a ZstdDecoder handle runs on its cumulation: skippable frames, and for a
Zstandard frame its size, flags and an output bound, the content size when the header has it, else the most
its blocks can regenerate.  No entropy work, no GPU."""
import ctypes as C
import os
import subprocess

import pytest

import zstd_checksum_inputs as K
import zstd_decode_inputs as I
import zstd_frames as Z
import zstd_handbuilt as HB

pa = pytest.importorskip("pyarrow")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nx_zstd_next_frame", "nx_zstd_decode_host_ex", "nx_zstd_decode_batch_ex", "nx_zstd_decoder_new", "nx_zstd_decoder_free",
         "nx_zstd_decoder_decode", "nx_zstd_decoder_stats")


@pytest.fixture(scope="module")
def B():
    from netty_amd import batch
    return batch


@pytest.mark.parametrize("payload", [b"", b"hello"])
def test_skippable_frames(B, payload):
    for nibble in (0, 7, 15):
        f = K.skippable(payload, nibble)
        assert len(f) == 8 + len(payload)
        for more in (b"", I.TRAILING, f):
            assert B.zstd_next_frame(f + more) == (0, B.ZSTD_KIND_SKIPPABLE, len(f), 0, 0), (nibble, more)
        for k in range(len(f)):
            assert B.zstd_next_frame(f[:k])[0] == K.TRUNCATED, (nibble, k)
    assert B.zstd_next_frame(b"\x60\x2a\x4d\x18" + bytes(4))[0] == -84  # 0x184D2A60 is no skippable magic
    assert B.zstd_next_frame(b"\x50\x2b")[0] == -84


def test_out_bound_is_the_content_size_when_the_header_has_it(B, oracle):
    for c in I.libzstd_frames(oracle):
        for data in (c.frame, c.frame + I.TRAILING):
            st, kind, fb, bound, flags = B.zstd_next_frame(data)
            assert (st, kind, fb, bound) == (0, B.ZSTD_KIND_FRAME, len(c.frame), c.n), (c.kind, c.n, c.level)
            assert (0, fb, c.n, flags) == B.zstd_frame_info(data)
    for name, f, want in K.cases(oracle):  # the checksum's four bytes are counted
        if name != "handbuilt_no_content_size":
            assert B.zstd_next_frame(f)[:4] == (0, B.ZSTD_KIND_FRAME, len(f), len(want)), name
            assert B.zstd_next_frame(f)[4] & B.ZSTD_FRAME_CHECKSUM


def test_out_bound_without_a_content_size_covers_what_the_frame_regenerates(B, oracle):
    looser = 0
    for c in I.libzstd_frames(oracle):
        f = K.without_content_size(c.frame)
        if c.n <= 5000 or c.level == 3:
            assert I.unzstd(f, c.n) == c.data  # the re-headed frame is still libzstd's frame
        zf = Z.parse_frame(f)
        assert zf.content_size is None and zf.end == len(f)
        st, kind, fb, bound, flags = B.zstd_next_frame(f)
        assert (st, kind, fb) == (0, B.ZSTD_KIND_FRAME, len(f)), (c.kind, c.n, c.level)
        assert (0, fb, None, flags) == B.zstd_frame_info(f)
        assert c.n <= bound, (c.kind, c.n, c.level, bound)
        window = 1 << (10 + (zf.window_descriptor >> 3))
        assert bound == sum(min(window, 131072) if b.type == Z.COMPRESSED else b.size for b in zf.blocks)
        looser += bound > c.n
    assert looser >= 50  # the bound is not the content size in disguise (Raw and RLE blocks are exact, Compressed are not)


def test_out_bound_is_exact_for_raw_and_rle_blocks(B):
    blocks = [("raw", b"abc" * 100), ("rle", 0x55, 1000), ("raw", b""), ("rle", 1, 1), ("raw", bytes(range(200)))]
    f, want = HB.build(blocks, single=False, window_descriptor=0x20, with_size=False)
    assert Z.parse_frame(f).content_size is None
    assert B.zstd_next_frame(f) == (0, B.ZSTD_KIND_FRAME, len(f), len(want), 0x20 << 8)
    for name, (f, want) in HB.cases().items():
        zf = Z.parse_frame(f)
        st, kind, fb, bound, flags = B.zstd_next_frame(f)
        assert (st, kind, fb) == (0, B.ZSTD_KIND_FRAME, len(f)), name
        if zf.content_size is not None or Z.regenerated_size(zf) is not None:
            assert bound == len(want), name
        else:
            assert bound >= len(want), name
    f, want = HB.cases()["no_content_size"]  # a Raw block of 300 bytes and a Compressed block under a 16 KiB window
    assert B.zstd_next_frame(f)[3] == 300 + 16384


def test_errors_are_those_of_frame_info(B, oracle):
    for name, (f, status) in HB.malformed().items():
        if name == "skippable_magic":  # the one difference: this walker knows skippable frames
            assert B.zstd_next_frame(f) == (0, B.ZSTD_KIND_SKIPPABLE, len(f), 0, 0)
            assert B.zstd_frame_info(f)[0] == status
            continue
        assert B.zstd_next_frame(f)[0] == B.zstd_frame_info(f)[0], name
    for f, _ in I.small_frames(oracle)[:3] + [HB.malformed()["checksum_flag"]]:
        for k in range(len(f)):
            assert B.zstd_next_frame(f[:k])[0] == K.TRUNCATED, (len(f), k)


def test_argument_checks():
    from netty_amd import _lib
    L = _lib.load()
    k, fb, ob, fl = C.c_uint32(7), C.c_uint64(7), C.c_uint64(7), C.c_uint32(7)
    refs = [C.byref(k), C.byref(fb), C.byref(ob), C.byref(fl)]
    assert L.nx_zstd_next_frame(None, 4, *refs) == K.INVALID_ARG
    for i in range(4):
        a = list(refs)
        a[i] = None
        assert L.nx_zstd_next_frame(b"abcd", 4, *a) == K.INVALID_ARG, i
    assert L.nx_zstd_next_frame(None, 0, *refs) == K.TRUNCATED
    assert (k.value, fb.value, ob.value, fl.value) == (7, 7, 7, 7)


def test_exported_and_declared():
    from netty_amd import _lib
    L = _lib.load()
    so = os.path.join(ROOT, "netty_amd", "libnetty_amd.so")
    syms = {l.split()[-1] for l in subprocess.check_output(["nm", "-D", "--defined-only", so], text=True).splitlines() if l.strip()}
    header = open(os.path.join(ROOT, "include", "netty_amd.h")).read()
    for name in NAMES:
        assert name in syms and name in _lib.EXPORTED and name + "(" in header, name
    assert "NX_ZSTD_DECODE_VERIFY_CHECKSUM 1u" in header
    assert L.nx_zstd_decoder_new(-1) is None  # checkPositiveOrZero: refused before any device is looked at
