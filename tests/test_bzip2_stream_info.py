"""CPU tests of nx_bzip2_stream_info: what the first 14 bytes of a stream say."""
import bz2

import pytest

import bzip2_streams as S


@pytest.fixture(scope="module")
def B():
    from netty_amd import batch
    return batch


def test_levels_and_first_block_crc(B):
    for lv in range(1, 10):
        s = bz2.compress(b"stream info %d" % lv, lv)
        st, level, crc, empty = B.bzip2_stream_info(s)
        assert (st, level, empty) == (S.OK, lv, False)
        assert crc == S.get_bits(s, 80, 32)
        assert B.bzip2_stream_info(s[:14]) == (st, level, crc, empty)  # the first 14 bytes are enough


def test_empty_stream(B):
    s = bz2.compress(b"")
    assert len(s) == 14
    assert B.bzip2_stream_info(s) == (S.OK, 9, 0, True)


def test_truncated_below_14_bytes(B):
    s = bz2.compress(b"abc")
    for k in range(14):
        assert B.bzip2_stream_info(s[:k])[0] == S.TRUNCATED
    assert B.bzip2_stream_info(b"XYZ1" + s[4:13])[0] == S.TRUNCATED  # not even a wrong magic is judged early


def test_header_errors(B):
    s = bz2.compress(b"abc")
    assert B.bzip2_stream_info(b"BZx" + s[3:])[0] == S.STREAM_ID
    assert B.bzip2_stream_info(s[:3] + b"0" + s[4:])[0] == S.BLOCK_SIZE
    assert B.bzip2_stream_info(s[:3] + b":" + s[4:])[0] == S.BLOCK_SIZE
    assert B.bzip2_stream_info(S.flip_bit(s, 40))[0] == S.BLOCK_HEADER
