"""The inputs of the bzip2 split-path tests (nx_bzip2_encode_batch_split, nx_bzip2_encode_segment_host and the
Bzip2Encoder handle), beside those of bzip2_encode_inputs.  Seeded; built once per process.  Also the bit-level
helpers the tests compute expected bytes with."""
import functools
import random

import bzip2_encode_inputs as I
import bzip2_streams as S

BLOCKS = -127  # NX_ERR_BZIP2_ENCODE_BLOCKS
SEG_FIRST, SEG_LAST = 1, 2
LIMIT1 = 100000 - 6  # blockLengthLimit at level 1
CARRY_PATTERN = 0x5A3C96E1  # the carry sweep's bits: the low k of it, for k carried bits


def _rb(r, n):
    return bytes(r.getrandbits(8) for _ in range(n))


# Two-block random inputs at level 1: the first block takes a little under 100 000 bytes, so where the second one
# starts in the stream differs from seed to seed.  test_bzip2_segment_host.test_phase_coverage asserts that the
# host streams put the second block at every bit phase of a byte: the GPU splice test relies on that.
PHASE_SEEDS = (100, 101, 102, 104, 110, 111, 115, 116, 122, 128, 130, 139)  # chosen so that the condition holds


@functools.lru_cache(maxsize=None)
def phase_items():
    return tuple(I.Item(f"phase{seed}", _rb(random.Random(seed), 100040 + seed % 7), 1) for seed in PHASE_SEEDS)


@functools.lru_cache(maxsize=None)
def phase_streams(B):
    return tuple(B.bzip2_encode_host(it.data, it.level) for it in phase_items())


@functools.lru_cache(maxsize=None)
def run_straddles():
    """Runs of 254 / 255 / 256 / 510 equal bytes that reach over the block limit at level 1, at several distances."""
    r = random.Random(77)
    out = []
    for run in (254, 255, 256, 510):
        for before in (LIMIT1 - 300, LIMIT1 - 4, LIMIT1 - 3, LIMIT1 - 1, LIMIT1, LIMIT1 + 1):
            head = _rb(r, before).replace(b"\x7a", b"\x7b")  # no byte of the run's value next to it by accident
            out.append(I.Item(f"straddle{run}_{before}", head + b"\x7a" * run + _rb(r, 50), 1))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def three_blocks():
    """A 3-block level-1 stream: random bytes with runs mixed in, so that cuts fall in and next to runs."""
    r = random.Random(4242)
    parts, block_bytes = [], 0  # about 2.3 blocks' worth after the first run-length stage
    while block_bytes < 230000:
        if r.random() < 0.8:
            parts.append(_rb(r, r.randrange(1, 400)))
            block_bytes += len(parts[-1])
        else:
            run = r.randrange(2, 600)
            parts.append(bytes([r.getrandbits(8)]) * run)
            block_bytes += 5 * (run // 255) + min(run % 255, 5)
    data = b"".join(parts)
    assert len(I.block_slices(data, 1)) == 3
    return I.Item("three_blocks", data, 1)


@functools.lru_cache(maxsize=None)
def three_blocks_stream(B):
    return B.bzip2_encode_host(three_blocks().data, 1)


@functools.lru_cache(maxsize=None)
def five_blocks():
    r = random.Random(99)
    return I.Item("five_blocks", _rb(r, 450000), 1)


def small_stream_item(oracle):
    return I.Item("seg_small", oracle.textgen_chunk(11, 3000), 1)


def cuts_of(data: bytes, level: int):
    """The input end of every block, from bzip2_encode_inputs.block_slices."""
    out, at = [], 0
    for s in I.block_slices(data, level):
        at += len(s)
        out.append(at)
    return out


def end_magic_bit(stream: bytes) -> int:
    """The bit where the stream's end magic starts: the last place the pattern occurs, 80 bits and at most 7
    bits of padding before the end."""
    v, n = int.from_bytes(stream, "big"), 8 * len(stream)
    for pad in range(8):
        at = n - 80 - pad
        if at >= 0 and (v >> (n - at - 48)) & ((1 << 48) - 1) == S.END_MAGIC:
            return at
    raise AssertionError("no end magic")


def bits_of(stream: bytes, start: int, end: int) -> str:
    return bin(int.from_bytes(stream, "big") | (1 << (8 * len(stream))))[3:][start:end]


def pack_bits(bits: str) -> bytes:
    bits += "0" * (-len(bits) % 8)
    return int(bits, 2).to_bytes(len(bits) // 8, "big") if bits else b""


def carried(stream: bytes, count: int) -> bytes:
    """What a LAST segment that continues behind `count` carried bits of CARRY_PATTERN must write, given the
    one-shot stream of the same input: the carry, then the stream's bits behind its 32-bit header."""
    carry = format(CARRY_PATTERN & ((1 << count) - 1), f"0{count}b") if count else ""
    return pack_bits(carry + bits_of(stream, 32, end_magic_bit(stream) + 80))
