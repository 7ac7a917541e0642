"""CPU tests of the bzip2 format core through nx_bzip2_decode_host: streams libbz2 wrote (Python's bz2) must
decode to libbz2's bytes, output length and consumed length; every hand-mutated stream is first shown to
libbz2, whose verdict the test asserts, and must then get its exact status."""
import bz2

import pytest

import bzip2_streams as S


@pytest.fixture(scope="module")
def B():
    from netty_amd import batch
    return batch


def test_valid_streams_equal_libbz2(B, oracle):
    for v in S.valid_streams(oracle):
        verdict, data, consumed = S.libbz2(v.stream)
        assert (verdict, data, consumed) == ("ok", v.data, v.consumed), v.name
        st, out, used = B.bzip2_decode_host(v.stream, len(v.data))
        assert st == S.OK, (v.name, st)
        assert out == data, v.name
        assert used == consumed, (v.name, used, consumed)
        if v.ntables:
            assert S.first_block_fields(v.stream).ntables_value == v.ntables, v.name


def test_multi_block_streams_have_bit_aligned_blocks(oracle):
    v = next(v for v in S.valid_streams(oracle) if v.name == "text250k_l1")
    blocks, ends = S.find_magics(v.stream[:v.consumed])
    assert len(blocks) == 3 and len(ends) == 1
    assert any(b % 8 for b in blocks[1:])  # a later block starts inside a byte


def test_mutants_get_their_status(B, oracle):
    for m in S.mutants(oracle):
        assert S.libbz2(m.stream)[0] == m.libbz2, m.name
        st, out, used = B.bzip2_decode_host(m.stream, m.cap)
        assert st == m.status, (m.name, st)
        assert used == 0 and len(out) <= m.cap, m.name


def test_status_strings(B):
    from netty_amd import _lib
    assert _lib.status_string(S.BLOCK_CRC) == "block CRC error"
    assert _lib.status_string(S.STREAM_ID).startswith("Unexpected stream identifier contents")
    assert all(_lib.status_string(c) for c in S.BZIP2_CODES)


def test_error_keeps_completed_blocks(B, oracle):
    """On an error out_len is the bytes of the blocks completed before it."""
    v = next(v for v in S.valid_streams(oracle) if v.name == "text250k_l1")
    blocks, _ = S.find_magics(v.stream[:v.consumed])
    bad = S.flip_bit(v.stream, blocks[2] + 48 + 3)  # the third block's CRC
    assert S.libbz2(bad)[0] == "error"
    st, out, used = B.bzip2_decode_host(bad, len(v.data))
    assert st == S.BLOCK_CRC and used == 0
    assert 0 < len(out) < len(v.data) and out == v.data[:len(out)]
    assert len(out) > 150000


def test_start_pointer_moved(B, oracle):
    """A start pointer in range but wrong: the walk spells another rotation, which the block CRC refuses
    (or, for a rotation with the same bytes, accepts), as libbz2 does."""
    for s, cap in S.start_moved(oracle):
        st, out, _ = B.bzip2_decode_host(s, cap)
        verdict, data, _ = S.libbz2(s)
        assert st in (S.OK, S.BLOCK_CRC)
        assert (st == S.OK) == (verdict == "ok")
        if st == S.OK:
            assert out == data


def test_mutation_fuzz(B):
    both = 0
    for s, cap in S.fuzz_set():
        st, out, used = B.bzip2_decode_host(s, cap)
        assert st == S.OK or st in S.BZIP2_CODES, st
        verdict, data, consumed = S.libbz2(s)
        if st == S.OK and verdict == "ok":
            assert out == data and used == consumed
            both += 1
    assert both > 0  # some changes land in padding or after the stream
