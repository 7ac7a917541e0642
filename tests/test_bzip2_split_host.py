"""CPU tests of the split bzip2 decode's host forms: nx_bzip2_scan_host (every block and end-of-stream magic at
every bit position), nx_bzip2_decode_block_host (one block at a bit position) and nx_bzip2_decode_split_host
(scan, per-candidate decode, stitch), which must equal nx_bzip2_decode_host on every stream the decoder tests
have, decoys (tests/bzip2_decoys.py) included."""
import bz2

import pytest

import bzip2_decoys as D
import bzip2_handbuilt as H
import bzip2_streams as S

DECODE_BLOCKS = -128  # NX_ERR_BZIP2_DECODE_BLOCKS


@pytest.fixture(scope="module")
def B():
    from netty_amd import batch
    return batch


def _scan_equals_find_magics(B, data):
    blocks, ends = S.find_magics(data)
    want = sorted([(p, False) for p in blocks] + [(p, True) for p in ends])
    assert B.bzip2_scan_host(data) == want
    return want


def test_scan_forty_blocks(B):
    texts, specs, stream, positions = H.multi_block()
    got = _scan_equals_find_magics(B, stream)
    assert [p for p, e in got if not e] == list(positions)
    assert [e for p, e in got] == [False] * 40 + [True]
    end = got[-1][0]
    for k in range(1, 8):  # the stream behind a prefix of k bits, in whole bytes
        n = (len(stream) * 8 + k + 7) // 8
        shifted = (int.from_bytes(stream, "big") << (n * 8 - len(stream) * 8 - k)).to_bytes(n, "big")
        got = _scan_equals_find_magics(B, shifted)
        assert got == [(p + k, False) for p in positions] + [(end + k, True)]
    assert B.bzip2_scan_host(b"") == [] and B.bzip2_scan_host(stream[:5]) == []
    assert B.bzip2_scan_host(stream[:9]) == [] and B.bzip2_scan_host(stream[:10]) == [(32, False)]  # a magic needs its six bytes


def test_scan_decoys(B):
    for name, stream, true, decoy_b, decoy_e, data in D.streams():
        got = _scan_equals_find_magics(B, stream)
        assert set(decoy_b) <= {p for p, e in got if not e} and set(decoy_e) <= {p for p, e in got if e}, name


def test_block_by_block(B):
    texts, specs, stream, positions = H.multi_block()
    ends = list(positions[1:]) + [S.find_magics(stream)[1][0]]
    for i, p in enumerate(positions):
        st, out, info = B.bzip2_decode_block_host(stream, p, 1, 1 << 16)
        assert (st, out) == (S.OK, texts[i]), i
        assert info["end_bit"] == ends[i] and info["final_len"] == len(texts[i]), i
        assert info["stored_crc"] == info["computed_crc"] == specs[i].crc, i
        assert 1 <= info["pre_len"] <= 100000, i
        for off in (-1, 1):  # one bit off: no magic there
            assert B.bzip2_decode_block_host(stream, p + off, 1, 1 << 16)[0] == S.BLOCK_HEADER, i
    assert B.bzip2_decode_block_host(stream, ends[-1], 1, 16)[0] == S.BLOCK_HEADER  # the end magic is no block
    assert B.bzip2_decode_block_host(stream, 8 * len(stream) - 8, 1, 16)[0] == S.TRUNCATED
    assert B.bzip2_decode_block_host(stream, 8 * len(stream) + 800, 1, 16)[0] == S.TRUNCATED
    assert B.bzip2_decode_block_host(stream, positions[39], 1, len(texts[39]) - 1)[0] == S.OUTPUT_FULL
    assert B.bzip2_decode_block_host(stream[:positions[20] // 8 + 12], positions[20], 1, 1 << 16)[0] == S.TRUNCATED


def _equal(B, stream, cap, name):
    want = B.bzip2_decode_host(stream, cap)
    got = B.bzip2_decode_split_host(stream, cap)
    assert got[:3] == want, name
    return got


def test_split_equals_serial_on_libbz2_streams(B, oracle):
    for v in S.valid_streams(oracle):
        got = _equal(B, v.stream, len(v.data), v.name)
        assert got[:3] == (S.OK, v.data, v.consumed), v.name
    for m in S.mutants(oracle):
        assert _equal(B, m.stream, m.cap, m.name)[0] == m.status, m.name
    for i, (s, cap) in enumerate(S.fuzz_set()):
        _equal(B, s, cap, i)


def test_split_equals_serial_on_handbuilt_cases(B):
    for c in H.cases(B.bzip2_decode_chains()):
        got = _equal(B, c.stream, c.cap, c.name)
        assert (got[0], got[1], got[2]) == (c.status, c.data, c.consumed), c.name
    by = {c.name: c for c in H.group(B.bzip2_decode_chains(), "streams")}
    for name, blocks in (("blocks40", 40), ("blocks40_tail", 40), ("blocks40_cut_in_block33", 33), ("blocks40_block35_wrong_crc", 35),
                         ("blocks40_wrong_stream_crc", 40), ("blocks40_cap_block_edge", 2), ("blocks40_cap_zero", 0), ("no_blocks", 0)):
        assert B.bzip2_decode_split_host(by[name].stream, by[name].cap)[3] == blocks, name


def test_decoys(B):
    for name, stream, true, decoy_b, decoy_e, data in D.streams():
        assert decoy_b or decoy_e
        got = _equal(B, stream, len(data), name)
        assert got[:2] == (S.OK, data) and got[3] == len(true), name  # the chain counts the true blocks only
        assert S.libbz2(stream)[:2] == ("ok", data), name
        assert bz2.BZ2Decompressor().decompress(stream) == data


def test_max_blocks(B):
    texts, specs, stream, positions = H.multi_block()
    cap = sum(len(t) for t in texts)
    assert B.bzip2_decode_split_host(stream, cap, max_blocks=41)[0] == S.OK
    assert B.bzip2_decode_split_host(stream, cap, max_blocks=40) == (DECODE_BLOCKS, b"", 0, 0)
