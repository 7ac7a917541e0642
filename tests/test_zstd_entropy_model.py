"""The generated Zstandard frames of tests/zstd_entropy.py (real FSE and Huffman coding at the format's
edges) on the CPU: libzstd, through pyarrow, pins the generator and its model on every case; then
nx_zstd_decode_host must regenerate the same bytes; a census read from the frames' bytes by the independent
reader (tests/zstd_frames.py) asserts that the cases hold what they are named for; and every single-bit
flip of the tables and every truncation of two small frames goes through the host decoder.  No GPU."""
import pytest

import zstd_decode_inputs as I
import zstd_entropy as E
import zstd_frames as Z
from test_zstd_decode_host import L, _decode  # noqa: F401  (the fixture, and the decode between guards)

pa = pytest.importorskip("pyarrow")

OK, OUTPUT_FULL = 0, -87


def test_libzstd_pins_the_generator():
    assert len(E.REFUSED_BY_LIBZSTD) <= 3 and set(E.REFUSED_BY_LIBZSTD) <= set(E.cases())
    assert all(isinstance(r, str) and r and "\n" not in r for r in E.REFUSED_BY_LIBZSTD.values())
    for name, (f, want) in E.cases().items():
        if name not in E.REFUSED_BY_LIBZSTD:
            assert I.unzstd(f, len(want)) == want, name
    print(f"{len(E.cases())} generated cases, {len(E.REFUSED_BY_LIBZSTD)} of them refused by libzstd")


def test_host_decoder_on_every_case(L):
    for name, (f, want) in E.cases().items():
        st, out, used = _decode(L, f, len(want))
        assert (st, used) == (OK, len(f)), (name, st, used)
        assert out == want, name
        st, out, used = _decode(L, f, len(want) - 1)
        assert (st, used) == (OUTPUT_FULL, 0), (name, st)


def test_census_from_the_bytes():
    """every item the cases are there for, as the independent reader finds it in the frames"""
    c = E.cases()
    fl = I.entropy_census([f for f, _ in c.values()])
    # accuracy logs at both ends
    assert {("ll_log", 5), ("of_log", 5), ("ml_log", 5), ("ll_log", 9), ("of_log", 8), ("ml_log", 9), ("hw_log", 5), ("hw_log", 6)} <= fl
    for n in ("ll", "of", "ml"):
        assert any((n + "_minus", k) in fl for k in (3, 4)), n                  # several "less than 1" symbols
        assert {(n + "_flags", ch) for ch in ((0,), (1,), (2,), (3, 0), (3, 1), (3, 3, 1))} <= fl, n
        assert (n + "_size_minus_1", 1) in fl and (n + "_symbols", 2) in fl, n
    assert {("ll_top", 35), ("ml_top", 52), ("of_top", 31)} <= fl                # a zero run reaches the last symbol
    lz = Z.parse_frame(c["fse_zero_run_to_last"][0], entropy=True).blocks[1]
    assert [len(lz.dists[w].probs) for w in range(3)] == [36, 32, 53]
    assert [lz.dists[w].probs[-2] for w in range(3)] == [0, 0, 0]
    assert {("live_nseq", n) for n in (63, 64, 65, 128, 129)} <= fl
    # modes
    assert {("repeat_after", w, m) for w in range(3) for m in (Z.SEQ_PREDEFINED, Z.SEQ_RLE, Z.SEQ_FSE)} <= fl
    assert {("mode", w, Z.SEQ_REPEAT) for w in range(3)} <= I.census([f for f, _ in c.values()])["flags"]
    assert {("modes", (2, 0, 1)), ("modes", (0, 1, 2)), ("modes", (1, 2, 0))} <= fl
    assert {("rle_sym", 0, 35), ("rle_sym", 2, 52), ("rle_sym", 1, 16)} <= fl
    assert "tables_across_nseq0" in fl
    chain = Z.parse_frame(c["repeat_chain"][0]).blocks
    assert [(b.type, b.nseq and b.modes) for b in chain[1:]] == [(2, (2, 2, 2)), (0, None), (2, (3, 3, 3)), (2, 0), (2, (3, 3, 3))]
    # the widest sequence
    wide = Z.parse_frame(c["widest_sequence"][0], entropy=True).blocks
    assert [(b.type, b.size) for b in wide[:33]] == [(Z.RLE, 131072)] * 33 and len(wide) == 34
    w = wide[33]
    assert w.nseq == 2 and w.lit_regen == 131071
    assert [(w.dists[k].log, w.dists[k].top, w.dists[k].probs[-1]) for k in range(3)] == [(9, 35, -1), (8, 22, -1), (9, 52, -1)]
    # Huffman trees
    assert {("tree", "direct"), ("tree", "fse"), ("hw_minus", 3)} <= fl
    assert {("tree_weights", n) for n in (1, 2, 3, 128)} <= fl
    # streams
    assert {("lit_format", k) for k in range(4)} <= fl
    assert {("lit_regen", 1, n) for n in (1, 2, 1023)} <= fl
    assert {("lit_regen", 4, n) for n in (6, 7, 8, 9, 1023, 16383, 131072)} <= fl
    full = Z.parse_frame(c["lit4_format3_131072"][0]).blocks[0]
    assert (full.lit_format, full.nseq) == (3, 0)
    assert {("stream_end_01", 1), ("stream_end_01", 4), "seq_end_01", "weights_end_01"} <= fl
    # Treeless
    assert ("treeless_after", frozenset()) in fl
    assert ("treeless_after", frozenset({("lit", Z.LIT_RAW), ("lit", Z.LIT_RLE), ("block", Z.RAW)})) in fl
    assert {("treeless_streams", 4, 1), ("treeless_streams", 1, 4)} <= fl
    # everything at once
    ev = [Z.parse_frame(c[f"everything_{k}"][0]) for k in range(4)]
    assert all(3 <= len(f.blocks) <= 7 for f in ev)
    assert not ev[3].single_segment and ev[3].content_size is None


def test_generator_fails_loudly():
    with pytest.raises(AssertionError, match="probability 0"):
        E.fse_states(E.fse_table(5, [16, 0, 16]), [0, 1, 2])
    with pytest.raises(AssertionError, match="no weight"):
        E.huf_stream(E.huf_codes([1, 0, 1]), bytes([0, 1]))
    with pytest.raises(AssertionError, match="do not fit"):
        E.lit_header(2, 1, 1024, 10)
    with pytest.raises(AssertionError):
        E.write_distribution(5, [16, 15])


def test_targeted_corruption(L):
    """every bit of the tables flipped, every truncation: nothing outside the slot (the guards of _decode),
    truncations fail with a prefix of the output, and what both decoders accept they decode alike"""
    for f, want in E.corruption_frames():
        assert I.unzstd(f, len(want)) == want
        assert _decode(L, f, len(want))[:2] == (OK, want)
        for k in range(len(f)):
            st, out, used = _decode(L, f[:k], len(want) + 8)
            assert st != OK and used == 0, (len(f), k, st)
            assert want.startswith(out), (len(f), k)
    here = lib = both = neither = total = 0
    for f0, want in E.corruption_frames():
        for f in E.flips_of(f0):
            st, out, used = _decode(L, f, 4096)
            assert (used == len(f)) == (st == OK)
            try:
                ref = I.unzstd(f, len(want))  # (the header, which no flip touches, holds libzstd to this size)
            except Exception:
                ref = None
            total += 1
            here += st == OK
            lib += ref is not None
            both += st == OK and ref is not None
            neither += st != OK and ref is None
            if st == OK and ref is not None:
                assert ref == out
    print(f"{total} bit flips: {here} accepted by the host decoder, {lib} by libzstd, {both} by both, {neither} by neither")
    assert both >= 1 and neither >= 1


def test_stale_state_batch_on_the_host(L):
    """the frames of the GPU test of state left between a wave's frames: alone, the Treeless-first and the
    Repeat_Mode-first frame are refused; behind the first frame's blocks the same bodies decode"""
    batch, after_first = E.stale_state_batch()
    got = [_decode(L, f, 8192) for f, _ in batch]
    assert [g[0] for g in got] == [OK, -86, -86, OK, OK]
    assert [got[k][1] for k in (0, 3, 4)] == [batch[k][1] for k in (0, 3, 4)]
    for f in after_first:
        st, out, used = _decode(L, f, 8192)
        assert st == -86 and len(out) > len(batch[0][1]), (st, len(out))  # past every block: only the content size is off
    wide = [Z.parse_frame(batch[k][0], entropy=True).blocks[1] for k in (0, 3)]
    assert [[b.dists[w].log for w in range(3)] for b in wide] == [[9, 8, 9], [5, 5, 5]]
    assert [(b.tree_weights, len(Z.parse_frame(batch[k][0]).blocks)) for b, k in zip(wide, (0, 3))] == [(11, 2), (1, 2)]
    assert [Z.parse_frame(batch[k][0]).blocks[0].lit_type for k in (1, 2)] == [Z.LIT_TREELESS, Z.LIT_RAW]
    assert Z.parse_frame(batch[2][0]).blocks[0].modes == (Z.SEQ_REPEAT,) * 3
