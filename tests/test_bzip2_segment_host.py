"""CPU tests of the bzip2 split path's host forms: the planner (nx_bzip2_plan_host, nx_bzip2_plan_resume_host)
against the Python restatement of the block filling in bzip2_encode_inputs, and nx_bzip2_encode_segment_host
against the one-shot host stream (nx_bzip2_encode_host, which test_bzip2_encode_host.py holds against libbz2):
a stream written in segments is the one-shot stream, bit for bit."""
import bz2

import pytest

import bzip2_encode_inputs as I
import bzip2_split_inputs as X
import bzip2_streams as S


@pytest.fixture(scope="module")
def B():
    from netty_amd import batch
    return batch


def test_blocks_bound(B):
    assert B.bzip2_blocks_bound(0, 1) == 0 and B.bzip2_blocks_bound(5, 0) == 0 and B.bzip2_blocks_bound(5, 10) == 0
    for level in (1, 9):
        for n in (1, 99994, 99995, 100000, 250000, 10 ** 7):
            assert B.bzip2_blocks_bound(n, level) == (n + n // 4) // (level * 100000 - 5) + 1


def test_planner_equals_block_slices(B, oracle):
    for it in I.items(oracle) + X.run_straddles() + (X.three_blocks(), I.full_block(oracle)):
        st, cuts = B.bzip2_plan_host(it.data, it.level)
        assert st == I.OK and cuts == X.cuts_of(it.data, it.level), it.name
        assert len(cuts) <= B.bzip2_blocks_bound(len(it.data), it.level), it.name
    names = {it.name for it in I.items(oracle)}
    assert set(I.BOUNDARY_NAMES) <= names
    for run in (254, 255, 256, 510):  # the runs do reach over the limit
        assert any(len(X.cuts_of(it.data, 1)) == 2 for it in X.run_straddles() if it.name.startswith(f"straddle{run}_"))
    assert B.bzip2_plan_host(b"x", 0)[0] == I.LEVEL and B.bzip2_plan_host(b"x", 10)[0] == I.LEVEL


def _resumed(B, data, level, points):
    """The cuts of `data` fed to the resumable planner in the writes that `points` cut it into."""
    state, cuts, at = [0, 0, 0], [], 0
    for p in list(points) + [len(data)]:
        st, c = B.bzip2_plan_host(data[at:p], level, state=state, close=p == len(data))
        assert st == I.OK
        cuts += [at + v for v in c]
        at = p
    return cuts


def test_planner_resumes_at_every_split_point(B):
    it = X.three_blocks()
    want = X.cuts_of(it.data, 1)
    assert len(want) == 3
    # the state saved and restored after every single byte: every split point of the input at once
    assert _resumed(B, it.data, 1, range(1, len(it.data))) == want
    # and two writes, cut at and round every block boundary and at both ends
    for c in want[:2]:
        for p in range(c - 3, c + 4):
            assert _resumed(B, it.data, 1, [p]) == want, p
    for p in (0, 1, len(it.data) - 1, len(it.data)):
        assert _resumed(B, it.data, 1, [p]) == want, p
    # a block closes as soon as it is full: the write that ends on a cut reports it, the next one does not
    state = [0, 0, 0]
    assert B.bzip2_plan_host(it.data[:want[0]], 1, state=state, close=False) == (I.OK, [want[0]]) and state[:2] == [0, 0]
    assert B.bzip2_plan_host(it.data[:want[0] - 1], 1, state=[0, 0, 0], close=False) == (I.OK, [])


def test_segment_behind_every_carry(B, oracle):
    it = X.small_stream_item(oracle)
    st, stream = B.bzip2_encode_host(it.data, it.level)
    assert st == I.OK and bz2.decompress(stream) == it.data
    crc_in = 0x1234ABCD  # the stream CRC of the blocks before: the footer's CRC folds this block's into it
    block_crc = I.bzip2_crc(it.data)
    assert int.from_bytes(X.pack_bits(X.bits_of(stream, X.end_magic_bit(stream) + 48, X.end_magic_bit(stream) + 80)), "big") == block_crc
    for count in range(32):
        carry = X.CARRY_PATTERN & ((1 << count) - 1)
        st, got, seg = B.bzip2_encode_segment_host(it.data, it.level, (X.SEG_LAST, carry, count, 0))
        assert st == I.OK and got == X.carried(stream, count), count
        assert seg[1:] == (0, 0, block_crc), count
        st, got2, seg = B.bzip2_encode_segment_host(it.data, it.level, (X.SEG_LAST, carry, count, crc_in))
        want_crc = I.combined_crc([block_crc]) ^ (((crc_in << 1) | (crc_in >> 31)) & 0xFFFFFFFF)
        assert st == I.OK and seg[3] == want_crc and got2[:-11] == got[:-11], count
    assert B.bzip2_encode_segment_host(it.data, it.level, (X.SEG_LAST, 0, 32, 0))[0] == -100
    assert B.bzip2_encode_segment_host(it.data, 0, (X.SEG_LAST, 0, 0, 0))[0] == I.LEVEL
    short = B.bzip2_encode_segment_host(it.data, it.level, (X.SEG_LAST, 0, 0, 0), out_cap=len(X.carried(stream, 0)) - 1)
    assert short[0] == I.ENCODE_FULL and short[1] == b""
    # no data at all: the header and the footer
    assert B.bzip2_encode_segment_host(b"", 9, (X.SEG_FIRST | X.SEG_LAST, 0, 0, 0))[:2] == (I.OK, bz2.compress(b""))
    assert B.bzip2_encode_segment_host(b"", 4, (X.SEG_FIRST, 0, 0, 0)) == (I.OK, b"BZh4", (X.SEG_FIRST, 0, 0, 0))


def test_whole_stream_in_three_segments(B):
    it = X.three_blocks()
    st, stream = X.three_blocks_stream(B)
    assert st == I.OK and bz2.decompress(stream) == it.data
    cuts = X.cuts_of(it.data, 1)
    seg, out, at = (X.SEG_FIRST, 0, 0, 0), b"", 0
    for k, c in enumerate(cuts):
        flags = (X.SEG_FIRST if k == 0 else 0) | (X.SEG_LAST if k == 2 else 0)
        st, piece, seg = B.bzip2_encode_segment_host(it.data[at:c], 1, (flags,) + tuple(seg[1:]))
        assert st == I.OK
        if k < 2:
            assert len(piece) % 4 == 0 and seg[2] < 32
            assert out + piece == stream[:len(out) + len(piece)]
        out, at = out + piece, c
    assert out == stream
    assert seg[3] == I.combined_crc([I.bzip2_crc(s) for s in I.block_slices(it.data, 1)])
    # two blocks in one segment, then the last
    st, a, seg = B.bzip2_encode_segment_host(it.data[:cuts[1]], 1, (X.SEG_FIRST, 0, 0, 0))
    st2, b, _ = B.bzip2_encode_segment_host(it.data[cuts[1]:], 1, (X.SEG_LAST,) + tuple(seg[1:]))
    assert (st, st2) == (I.OK, I.OK) and a + b == stream


def test_phase_coverage(B):
    """The second block of the phase inputs starts at every bit phase of a byte in the host streams: a condition
    on the inputs that the GPU splice test relies on."""
    phases = set()
    for it, (st, stream) in zip(X.phase_items(), X.phase_streams(B)):
        assert st == I.OK and 100000 < len(it.data) < 100100, it.name
        assert len(I.block_slices(it.data, 1)) == 2, it.name
        # the first block alone as a FIRST segment without LAST: its bits are the header's 32 and the block's
        cut = X.cuts_of(it.data, 1)[0]
        st, piece, seg = B.bzip2_encode_segment_host(it.data[:cut], 1, (X.SEG_FIRST, 0, 0, 0))
        start = 8 * len(piece) + seg[2]
        assert st == I.OK and X.bits_of(stream, start, start + 48) == format(S.BLOCK_MAGIC, "048b"), it.name
        phases.add(start % 8)
    assert phases == set(range(8)), sorted(phases)
