"""nx_zstd_frame_info, the host frame walker, against tests/zstd_frames.py (itself pinned on libzstd's
frames), and the exported / declared / argument checks of the three Zstandard decoder entry points, which
answer before any GPU call.  No GPU."""
import ctypes as C
import os
import subprocess

import pytest

import zstd_decode_inputs as I
import zstd_frames as Z
import zstd_handbuilt as HB

pa = pytest.importorskip("pyarrow")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, TRUNCATED, CHECKSUM_UNSUPPORTED = -100, -85, -83
NAMES = ("nx_zstd_decode_batch", "nx_zstd_frame_info", "nx_zstd_decode_host")


@pytest.fixture(scope="module")
def B():
    from netty_amd import batch
    return batch


def _agrees(B, frame, data):
    f = Z.parse_frame(frame)
    st, end, size, flags = B.zstd_frame_info(data)
    assert st == 0 and end == f.end and size == f.content_size
    assert bool(flags & B.ZSTD_FRAME_SINGLE_SEGMENT) == f.single_segment
    assert bool(flags & B.ZSTD_FRAME_CHECKSUM) == f.checksum
    assert (flags >> 8) == (f.window_descriptor or 0)


def test_agrees_with_the_frame_reader(B, oracle):
    for c in I.libzstd_frames(oracle):
        _agrees(B, c.frame, c.frame)
        _agrees(B, c.frame, c.frame + I.TRAILING)
    for f, _ in HB.cases().values():
        _agrees(B, f, f)
    with_checksum, status = HB.malformed()["checksum_flag"]  # walked, its four bytes counted; the decoders refuse it
    assert status == CHECKSUM_UNSUPPORTED
    _agrees(B, with_checksum, with_checksum)


def test_need_more_input_at_every_proper_prefix(B, oracle):
    for f, _ in I.small_frames(oracle)[:3] + [HB.malformed()["checksum_flag"]]:
        for k in range(len(f)):
            assert B.zstd_frame_info(f[:k])[0] == TRUNCATED, (len(f), k)
        assert B.zstd_frame_info(f)[:2] == (0, len(f))


def test_first_frame_of_two(B, oracle):
    (a, _), (b, _) = I.small_frames(oracle)[0], I.small_frames(oracle)[3]
    assert B.zstd_frame_info(a + b)[:2] == (0, len(a))
    assert B.zstd_frame_info((a + b)[len(a):])[:2] == (0, len(b))


def test_header_errors(B):
    bad = HB.malformed()
    for name in ("dictionary_id", "reserved_bit", "block_type_3", "skippable_magic", "unknown_magic", "window_too_large",
                 "content_too_large", "block_above_window", "truncated"):
        frame, want = bad[name]
        assert B.zstd_frame_info(frame)[0] == want, name


def test_exported_and_declared():
    from netty_amd import _lib
    L = _lib.load()
    so = os.path.join(ROOT, "netty_amd", "libnetty_amd.so")
    syms = {l.split()[-1] for l in subprocess.check_output(["nm", "-D", "--defined-only", so], text=True).splitlines() if l.strip()}
    header = open(os.path.join(ROOT, "include", "netty_amd.h")).read()
    for name in NAMES:
        assert name in syms and name in _lib.EXPORTED and name + "(" in header
        assert getattr(L, name).restype is C.c_int32


def test_decode_batch_argument_checks():
    from netty_amd import _lib
    L = _lib.load()
    p = C.c_void_p(0x1000)  # never dereferenced: every case below is answered first
    args = [p] * 9
    assert L.nx_zstd_decode_batch(*([None] * 9), 0, None) == 0  # n = 0: nothing to do, nothing looked at
    for k in range(9):
        a = list(args)
        a[k] = None
        assert L.nx_zstd_decode_batch(*a, 1, None) == INVALID_ARG, k


def test_host_entries_argument_checks():
    from netty_amd import _lib
    L = _lib.load()
    fb, cs, fl = C.c_uint64(7), C.c_uint64(7), C.c_uint32(7)
    assert L.nx_zstd_frame_info(None, 4, C.byref(fb), C.byref(cs), C.byref(fl)) == INVALID_ARG
    assert L.nx_zstd_frame_info(b"abcd", 4, None, C.byref(cs), C.byref(fl)) == INVALID_ARG
    assert L.nx_zstd_frame_info(None, 0, C.byref(fb), C.byref(cs), C.byref(fl)) == TRUNCATED
    assert (fb.value, cs.value, fl.value) == (7, 7, 7)
    ol, co = C.c_size_t(0), C.c_size_t(0)
    assert L.nx_zstd_decode_host(None, 4, None, 0, C.byref(ol), C.byref(co)) == INVALID_ARG
    assert L.nx_zstd_decode_host(b"abcd", 4, None, 0, None, C.byref(co)) == INVALID_ARG
    for code in range(-87, -80):
        assert _lib.status_string(code) != "unknown status"
