"""The inputs of the bzip2 encoder tests, shared by the CPU tests (nx_bzip2_encode_host) and the GPU tests
(nx_bzip2_encode_batch): the smallest shapes at which each stage can go wrong.  Seeded; built once per process.
Also a Python restatement of Bzip2BlockCompressor's write / writeRun / isFull, which says where a stream's
blocks are cut, and bzip2's CRC."""
import functools
import random
from dataclasses import dataclass

OK, LEVEL, ENCODE_FULL = 0, -125, -126


@dataclass(frozen=True)
class Item:
    name: str
    data: bytes
    level: int
    kind: str = ""  # "periodic": equal rotations; "text" / "random": the size comparison's inputs


def fibonacci_word(n: int) -> bytes:
    a, b = b"a", b"ab"
    while len(b) < n:
        a, b = b, b + a
    return b[:n]


@functools.lru_cache(maxsize=None)
def items(oracle):
    """Every input but the full-size block."""
    r = random.Random(20261020)
    rb = lambda n: bytes(r.getrandbits(8) for _ in range(n))
    out = [Item("empty", b"", 9)]
    out += [Item(f"rand{n}", rb(n), 9) for n in (1, 2, 3, 4, 5, 63, 64, 65)]
    out.append(Item("all256", bytes(range(256)), 9))
    out += [Item(f"run{n}", b"x" * n, 9, "periodic") for n in (3, 4, 5, 254, 255, 256, 259, 260, 510, 1000)]
    out += [Item("count0", b"\x00" * 4, 9, "periodic"), Item("count1", b"\x01" * 5, 9, "periodic"), Item("count0then1", b"\x00" * 4 + b"\x01", 9)]
    out += [Item("hello10", b"hello world" * 10, 9, "periodic"), Item("ab500", b"ab" * 500, 9, "periodic"),
            Item("a5000", b"a" * 5000, 9, "periodic"), Item("abc333ab", b"abc" * 333 + b"ab", 9)]
    out += [Item("fib90k", fibonacci_word(90000), 1), Item("ab49000", b"ab" * 49000, 1, "periodic"),
            Item("two95k", bytes(r.choice(b"ab") for _ in range(95000)), 1)]
    out += [Item(f"tables{n}", rb(n), 1, "random") for n in (100, 400, 1000, 2000, 5000)]
    out += [Item(f"text30k_l{lv}", oracle.textgen_chunk(7, 30000), lv, "text") for lv in range(1, 10)]
    out += [Item(f"edge{n}", rb(n), 1) for n in range(99993, 100003)]
    out.append(Item("run_over_limit", rb(99990) + b"z" * 300, 1))
    out.append(Item("text250k_l1", oracle.textgen_chunk(7, 250000), 1))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def full_block(oracle):
    """One full-size block: two blocks at level 9."""
    return Item("text1m_l9", oracle.textgen_chunk(7, 1000000), 9)


BOUNDARY_NAMES = tuple(f"edge{n}" for n in range(99993, 100003)) + ("run_over_limit", "text250k_l1")


def block_slices(data: bytes, level: int):
    """The input bytes of each block, by Bzip2BlockCompressor.write / writeRun / isFull and Bzip2Encoder's loop: a
    byte is accepted while blockLength <= blockSize - 6, runs are cut at 255, a run of four or more is five bytes,
    and closing a block flushes the pending run."""
    limit = level * 100000 - 6
    out, start, length, run, cur = [], 0, 0, 0, -1
    flush = lambda k: k if k < 4 else 5
    i = 0
    while i < len(data):
        if length > limit:  # write() refuses: the block is closed with its pending run
            out.append(data[start:i])
            start, length, run, cur = i, 0, 0, -1
            continue
        v = data[i]
        if run == 0:
            cur, run = v, 1
        elif v != cur:
            length += flush(run)
            cur, run = v, 1
        elif run == 254:
            length += 5
            run = 0
        else:
            run += 1
        i += 1
    if start < len(data):
        out.append(data[start:])
    return out


@functools.lru_cache(maxsize=None)
def _crc_table():
    t = []
    for i in range(256):
        c = i << 24
        for _ in range(8):
            c = ((c << 1) ^ 0x04C11DB7) & 0xFFFFFFFF if c & 0x80000000 else (c << 1) & 0xFFFFFFFF
        t.append(c)
    return t


def bzip2_crc(data: bytes) -> int:
    t, c = _crc_table(), 0xFFFFFFFF
    for b in data:
        c = ((c << 8) & 0xFFFFFFFF) ^ t[(c >> 24) ^ b]
    return c ^ 0xFFFFFFFF


def combined_crc(crcs) -> int:
    c = 0
    for b in crcs:
        c = (((c << 1) | (c >> 31)) & 0xFFFFFFFF) ^ b
    return c


@functools.lru_cache(maxsize=None)
def host_streams(B, oracle):
    """nx_bzip2_encode_host's (status, stream) of every item, computed once."""
    return tuple(B.bzip2_encode_host(it.data, it.level) for it in items(oracle))
