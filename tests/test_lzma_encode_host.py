"""CPU tests of nx_lzma_encode_host, the format core the kernels run.  Two checkers, neither the project's code:
liblzma through Python's lzma (FORMAT_ALONE) and tests/lzma_model.py, which also lists the packets."""
import collections
import lzma
import random

import pytest

import lzma_inputs as I
import lzma_model as M

NX_ERR_LZMA_PROPS, NX_ERR_LZMA_DICT_SIZE, NX_ERR_LZMA_ENCODE_FULL = -140, -141, -143


@pytest.fixture(scope="module")
def B():
    from netty_amd import batch
    return batch


def liblzma_check(stream, data, end_marker):
    """liblzma decodes the stream to the data, reaches eof and leaves nothing; with junk appended, exactly the junk"""
    if end_marker:  # this liblzma refuses a known size together with an end marker
        stream = stream[:5] + b"\xff" * 8 + stream[13:]
    for junk in (b"", b"JUNK"):
        d = lzma.LZMADecompressor(format=lzma.FORMAT_ALONE)
        assert d.decompress(stream + junk) == data
        assert d.eof and d.unused_data == junk


def check_stream(B, stream, data, lc, lp, pb, dict_size, end_marker):
    assert stream[0] == (pb * 5 + lp) * 9 + lc
    assert stream[1:5] == dict_size.to_bytes(4, "little")
    assert stream[5:13] == len(data).to_bytes(8, "little")
    assert len(stream) <= B.lzma_max_compressed_length(len(data))
    out, packets = M.decode(stream)
    assert out == data
    assert (packets[-1][0] == M.END_MARKER if packets else False) == bool(end_marker)
    for kind, n, dist in packets:
        assert dist <= max(dict_size, 0), (kind, n, dist)
    if lc + lp <= 4:
        liblzma_check(stream, data, end_marker)
    return packets


@pytest.fixture(scope="module")
def streams(B, oracle):
    """every item at the default settings, once: (name, data, stream, packets)"""
    out = []
    for name, data in I.items(oracle):
        st, s = B.lzma_encode_host(data)
        assert st == 0, name
        out.append((name, data, s, check_stream(B, s, data, 3, 0, 2, 65536, False)))
    return out


def test_default_settings_every_item(streams):
    assert len(streams) == len(I.directed()) + 2


def test_empty_is_eighteen_bytes(B):
    st, s = B.lzma_encode_host(b"")
    assert st == 0 and s == bytes([0x5D, 0, 0, 1, 0]) + bytes(8) + bytes(5)


@pytest.mark.parametrize("lc,lp,pb", I.PROPS + I.PROPS_MODEL_ONLY)
@pytest.mark.parametrize("end_marker", [False, True])
def test_properties_and_end_marker(B, lc, lp, pb, end_marker):
    for name, data in I.directed():
        if len(data) > 11000:
            continue  # the model decoder is Python: the long items ran at the default settings
        st, s = B.lzma_encode_host(data, lc, lp, pb, 65536, end_marker)
        assert st == 0, name
        check_stream(B, s, data, lc, lp, pb, 65536, end_marker)


def test_end_marker_on_long_items(B):
    for name, data in I.directed():
        if len(data) > 11000:
            st, s = B.lzma_encode_host(data, end_marker=True)
            assert st == 0, name
            liblzma_check(s, data, True)


@pytest.mark.parametrize("name,data,dict_size", I.dict_cases(), ids=[c[0] for c in I.dict_cases()])
def test_dictionary_size_bounds_every_distance(B, name, data, dict_size):
    st, s = B.lzma_encode_host(data, dict_size=dict_size)
    assert st == 0
    packets = check_stream(B, s, data, 3, 0, 2, dict_size, False)
    if dict_size == 0:
        assert {k for k, _, _ in packets} == {M.LIT}
    if name == "rep65537_dict65536":
        assert not any(dist == 65537 for _, _, dist in packets)


def test_a_repetition_within_the_dictionary_is_found(B):
    data = I.far_copy(65536, 16)
    st, s = B.lzma_encode_host(data)
    assert (M.MATCH, 16, 65536) in check_stream(B, s, data, 3, 0, 2, 65536, False)


def test_census(streams):
    """the directed inputs make the coder write every kind of packet it can (a missing kind fails)"""
    kinds = collections.Counter()
    len_class, dist_class = set(), set()
    for name, data, s, packets in streams:
        for kind, n, dist in packets:
            kinds[kind] += 1
            if kind == M.MATCH:
                len_class.add("low" if n < 10 else "mid" if n < 18 else "high")
                dist_class.add("slot" if dist - 1 < 4 else "tree" if dist - 1 < 128 else "direct")
    for kind in (M.LIT, M.MATCHED_LIT, M.MATCH, M.REP0, M.REP1, M.REP2, M.REP3):
        assert kinds[kind] > 0, kind
    assert len_class == {"low", "mid", "high"}
    assert dist_class == {"slot", "tree", "direct"}


def test_expected_packets(streams):
    by = {name: packets for name, _, _, packets in streams}
    for d in I.DISTANCES[1:]:
        assert any(k == M.MATCH and dist == d for k, _, dist in by["dist%d" % d]), d
    for n in I.MATCH_LENGTHS:
        assert (M.MATCH, n, 300) in by["mlen%d" % n], n
    # a run: one literal, then rep0 packets of at most 273 bytes, a one-byte tail as a matched literal
    assert by["run273"] == [(M.LIT, 1, 0), (M.REP0, 272, 1)]
    assert by["run274"] == [(M.LIT, 1, 0), (M.REP0, 273, 1)]
    assert by["run277"] == [(M.LIT, 1, 0), (M.REP0, 273, 1), (M.REP0, 3, 1)]
    assert by["run546"] == [(M.LIT, 1, 0), (M.REP0, 273, 1), (M.REP0, 272, 1)]


def test_long_run_compresses(streams):
    s = {name: s for name, _, s, _ in streams}["run65536"]
    assert len(s) < 4096  # about 241 rep0 packets: a literal-only coder cannot pass


def test_carry_through_pending_ff(B):
    data = I.rand(I.CARRY_SEED, I.CARRY_LEN)
    st, s, stats = B.lzma_encode_host(data, stats=True)
    assert st == 0 and stats["carries"] >= 1 and stats["max_carry_ff"] >= 1
    assert stats["literals"] + stats["matched_literals"] + stats["matches"] + sum(stats["reps"]) == len(M.decode(s)[1])


@pytest.mark.parametrize("name", ["len0", "len1", "run277", "dist129", "cycle4", "random1000", "carry"])
def test_one_byte_short_is_full_and_guards_stay(B, name):
    data = dict(I.directed())[name]
    st, s = B.lzma_encode_host(data)
    st2, s2, guard = B.lzma_encode_host(data, out_cap=len(s) - 1, guard=16)
    assert st2 == NX_ERR_LZMA_ENCODE_FULL and guard == b"\xa5" * 16
    st3, s3, guard = B.lzma_encode_host(data, out_cap=len(s), guard=16)
    assert st3 == 0 and s3 == s and guard == b"\xa5" * 16


def test_argument_codes(B):
    for lc, lp, pb in [(9, 0, 0), (-1, 0, 0), (0, 5, 0), (0, -1, 0), (0, 0, 5), (0, 0, -1)]:
        assert B.lzma_encode_host(b"x", lc, lp, pb)[0] == NX_ERR_LZMA_PROPS
    assert B.lzma_encode_host(b"x", dict_size=-1)[0] == NX_ERR_LZMA_DICT_SIZE
    assert B.lzma_max_compressed_length(0) == 141 and B.lzma_max_compressed_length(65536) == 13 + 65536 + 21845 + 128
