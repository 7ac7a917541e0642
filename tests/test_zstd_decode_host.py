"""nx_zstd_decode_host, the CPU run of the decoder's format core (csrc/zstd_decode_core.hpp), against
libzstd through pyarrow: frames libzstd wrote must regenerate their sources, hand-built frames must
regenerate what libzstd regenerates from them (which pins the generator and its model), and malformed
frames get their statuses with nothing written outside the output slot.  No GPU."""
import ctypes as C

import pytest

import zstd_decode_inputs as I
import zstd_frames as Z
import zstd_handbuilt as HB

pa = pytest.importorskip("pyarrow")

OK = 0
GUARD = I.GUARD


@pytest.fixture(scope="module")
def L():
    from netty_amd import _lib
    return _lib.load()


def _decode(L, frame, cap):
    """(status, output, consumed); the slot lies between guards, which must come back untouched"""
    buf = (C.c_uint8 * (cap + 2 * GUARD)).from_buffer(bytearray(b"\xa5" * (cap + 2 * GUARD)))
    ol, co = C.c_size_t(0), C.c_size_t(0)
    st = L.nx_zstd_decode_host(frame, len(frame), C.byref(buf, GUARD), cap, C.byref(ol), C.byref(co))
    raw = bytes(buf)
    assert ol.value <= cap
    assert raw[:GUARD] == b"\xa5" * GUARD and raw[GUARD + ol.value:] == b"\xa5" * (cap - ol.value + GUARD), "bytes outside the output changed"
    return st, raw[GUARD:GUARD + ol.value], co.value


def test_libzstd_corpus(L, oracle):
    for c in I.libzstd_frames(oracle):
        what = (c.kind, c.n, c.level)
        st, out, used = _decode(L, c.frame, c.n)
        assert (st, used) == (OK, len(c.frame)), what
        assert out == c.data, what


def test_trailing_bytes_are_left_alone(L, oracle):
    for c in I.libzstd_frames(oracle):
        if c.n > 131073:
            continue
        st, out, used = _decode(L, c.frame + I.TRAILING, c.n)
        assert (st, used) == (OK, len(c.frame)) and out == c.data, (c.kind, c.n, c.level)
    for name, (f, want) in HB.cases().items():
        st, out, used = _decode(L, f + I.TRAILING, len(want))
        assert (st, used) == (OK, len(f)) and out == want, name


def test_handbuilt_generator_is_pinned_by_libzstd():
    for name, (f, want) in HB.cases().items():
        assert I.unzstd(f, len(want)) == want, name


def test_handbuilt_frames(L):
    for name, (f, want) in HB.cases().items():
        st, out, used = _decode(L, f, len(want) + 3)
        assert (st, used) == (OK, len(f)), (name, st)
        assert out == want, name


def test_handbuilt_frames_cover_what_libzstd_did_not_emit():
    hb = HB.cases()
    cs = I.census([f for f, _ in hb.values()])
    assert ("lit", Z.LIT_RLE) in cs["flags"] and ("lit", Z.LIT_RAW) in cs["flags"]
    assert {("mode", i, Z.SEQ_RLE) for i in range(3)} <= cs["flags"]
    assert {"nseq0", "nseq_1b", "nseq_2b", "nseq_3b"} <= cs["flags"]
    assert Z.parse_frame(hb["no_content_size"][0]).content_size is None
    f = Z.parse_frame(hb["window_below_content"][0])
    assert not f.single_segment and f.window_descriptor == 0 and f.content_size > 1024
    assert [(b.type, b.size) for b in Z.parse_frame(hb["empty_raw_block"][0]).blocks] == [(Z.RAW, 0)]
    assert [Z.parse_frame(hb[f"nseq_{n}"][0]).blocks[1].nseq for n in (127, 128, 0x7EFF, 0x7F00)] == [127, 128, 0x7EFF, 0x7F00]


def test_every_truncation_fails(L, oracle):
    for f, want in I.small_frames(oracle):
        assert _decode(L, f, len(want))[0] == OK
        for k in range(len(f)):
            st, out, used = _decode(L, f[:k], len(want) + 8)
            assert st != OK and used == 0, (len(f), k, st)
            assert want.startswith(out), (len(f), k)


@pytest.mark.parametrize("name", sorted(HB.malformed()))
def test_limit_cases(L, name):
    frame, want = HB.malformed()[name]
    st, out, used = _decode(L, frame, 4096)
    assert st == want and used == 0, (name, st)


def test_output_capacity(L, oracle):
    for f, want in I.small_frames(oracle):
        st, out, used = _decode(L, f, len(want) - 1)
        assert st == -87 and used == 0, st


def test_mutations_agree_with_libzstd_where_both_accept(L, oracle):
    for f in I.mutations(oracle):
        st, out, used = _decode(L, f, 4096)
        if st != OK:
            continue
        try:
            lib = I.unzstd(f, len(out))
        except Exception:
            continue
        assert lib == out


def test_corpus_census(oracle):
    """the features the decoder tests rely on, so that another pyarrow cannot silently thin the corpus"""
    cs = I.census([c.frame for c in I.libzstd_frames(oracle)])
    fl = cs["flags"]
    assert cs["frames"] == 300
    assert cs["multi_block"] >= 60 and cs["windowed"] >= 1 and cs["treeless_blocks"] >= 10, cs
    assert {("block", Z.RAW), ("block", Z.RLE), ("block", Z.COMPRESSED)} <= fl
    assert {("lit", Z.LIT_RAW), ("lit", Z.LIT_COMPRESSED), ("lit", Z.LIT_TREELESS)} <= fl
    assert {("streams", 1), ("streams", 4), ("tree", "fse")} <= fl
    for which in range(3):
        assert {("mode", which, Z.SEQ_PREDEFINED), ("mode", which, Z.SEQ_FSE), ("mode", which, Z.SEQ_REPEAT)} <= fl, which
    assert {"nseq0", "nseq_1b", "nseq_2b"} <= fl
    ent = I.entropy_census([c.frame for c in I.libzstd_frames(oracle)])   # printed only: what libzstd chose to emit
    for key in ("ll_log", "of_log", "ml_log", "hw_log", "ll_minus", "of_minus", "ml_minus", "tree_weights", "lit_format"):
        print(key, sorted(x[1] for x in ent if isinstance(x, tuple) and x[0] == key))
    print("zero-run flag chains", sorted({x[1] for x in ent if isinstance(x, tuple) and x[0].endswith("_flags")}))
