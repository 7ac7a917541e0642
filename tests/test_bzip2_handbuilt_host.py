"""CPU tests of the bzip2 decoder on hand-built streams (tests/bzip2_handbuilt.py).  The model decoder
(tests/bzip2_model.py) is first held against libbz2 on everything libbz2 can judge: the streams and mutants of
bzip2_streams.py, then every hand-built case inside libbz2's limits.  nx_bzip2_decode_host must then equal the
model on every case, status, bytes and consumed length."""
import pytest

import bzip2_handbuilt as H
import bzip2_model as M
import bzip2_streams as S


@pytest.fixture(scope="module")
def B():
    from netty_amd import batch
    return batch


@pytest.fixture(scope="module")
def all_cases(B):
    return H.cases(B.bzip2_decode_chains()) + (H.big_case(),)


def test_model_equals_libbz2_on_libbz2_streams(oracle):
    for v in S.valid_streams(oracle):
        assert M.decode(v.stream, len(v.data)) == (M.OK, v.data, v.consumed), v.name
        assert S.libbz2(v.stream) == ("ok", v.data, v.consumed), v.name
    for m in S.mutants(oracle):
        verdict, data, consumed = S.libbz2(m.stream)
        st, out, used = M.decode(m.stream, 1 << 21)  # libbz2 has no cap
        assert (st == M.OK) == (verdict == "ok"), (m.name, st, verdict)
        assert (st == M.TRUNCATED) == (verdict == "more"), (m.name, st, verdict)
        if st == M.OK:
            assert (out, used) == (data, consumed), m.name
        assert M.decode(m.stream, m.cap)[0] == m.status, m.name


def test_model_equals_libbz2_on_handbuilt_cases(all_cases):
    valid = confirmed = 0
    for c in all_cases:
        verdict, data, consumed = S.libbz2(c.stream)
        valid += c.status == M.OK
        if c.verdict == "outside":
            # a condition, not a measurement: only the named classes, and libbz2 does refuse them
            assert H.OUTSIDE[c.name] in H.OUTSIDE_CLASSES, c.name
            assert verdict == "error", c.name
            continue
        assert c.name not in H.OUTSIDE
        assert verdict == c.verdict, (c.name, verdict)
        if verdict == "ok" and c.status == M.OK:
            assert (data, consumed) == (c.data, c.consumed), c.name
            confirmed += 1
        if c.status == M.OK:
            assert verdict == "ok", c.name  # a valid case inside libbz2's limits decodes there too
    assert set(H.OUTSIDE.values()) <= set(H.OUTSIDE_CLASSES)
    assert valid >= 300 and 4 * confirmed >= 3 * valid, (confirmed, valid)


def test_groups_mix_valid_and_invalid(B):
    kc = B.bzip2_decode_chains()
    for g in H.GROUPS:
        sts = {c.status for c in H.group(kc, g)}
        assert M.OK in sts and len(sts) > 1, g
    names = {c.name for c in H.cases(kc)}
    assert len(names) == len(H.cases(kc))


def test_expected_statuses_the_issue_names(B):
    by = {c.name: c for c in H.cases(B.bzip2_decode_chains())}
    want = {"len_walk_to0": M.CODE, "len_walk_to24": M.CODE, "incomplete_unused_not_sent": M.OK, "sel_18002": M.OK,
            "sel_18003": M.SELECTORS, "sel_one_too_few": M.DECODING_BLOCK, "sel_index_at_table_count": M.DECODING_BLOCK,
            "fill_100000_by_run": M.OK, "fill_100000_by_symbol": M.OK, "fill_100001_by_run": M.BLOCK_EXCEEDS,
            "fill_100001_by_symbol": M.BLOCK_EXCEEDS, "blocks40": M.OK, "blocks40_cap_zero": M.OUTPUT_FULL,
            "blocks40_cap_total_minus_1": M.OUTPUT_FULL, "walk_n5000_a256_wrong_crc": M.BLOCK_CRC, "len_longest23": M.OK,
            "run_wrap_31_digits": M.BLOCK_EXCEEDS, "run_wrap_to_5": M.OK}
    for name, st in want.items():
        assert by[name].status == st, (name, by[name].status)
    assert H.big_case().status == M.OK and len(H.big_case().data) == 1440000


def test_forty_blocks_cover_every_bit_phase_and_caps(B):
    texts, specs, stream, positions = H.multi_block()
    assert len(texts) == 40 and {p % 8 for p in positions} == set(range(8))
    assert S.find_magics(stream)[0] == list(positions)
    by = {c.name: c for c in H.cases(B.bzip2_decode_chains()) if c.group == "streams"}
    total = sum(len(t) for t in texts)
    assert by["blocks40"].cap == total and by["blocks40"].data == b"".join(texts)
    edge = by["blocks40_cap_block_edge"]
    assert (edge.status, edge.data) == (M.OUTPUT_FULL, texts[0] + texts[1])
    inside = by["blocks40_cap_inside_block2"]
    assert (inside.status, inside.data) == (M.OUTPUT_FULL, texts[0] + texts[1])
    assert by["blocks40_cap_inside_block1"].data == texts[0]
    assert by["blocks40_cap_total_minus_1"].data == b"".join(texts[:39])
    assert by["blocks40_tail"].consumed == len(stream) and by["blocks40_tail"].status == M.OK


def test_host_decoder_equals_model(B, all_cases):
    for c in all_cases:
        got = B.bzip2_decode_host(c.stream, c.cap)
        assert (got[0], got[2], len(got[1])) == (c.status, c.consumed, len(c.data)), c.name
        assert got[1] == c.data, c.name
