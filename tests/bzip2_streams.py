"""The inputs of the bzip2 decoder tests, shared by the CPU tests (nx_bzip2_decode_host) and the GPU tests
(nx_bzip2_decode_batch): streams Python's bz2 (libbz2) wrote, a bit-level reader that finds the block and
end-of-stream magics and the fields of a stream's first block, bit patchers, and the mutated streams of the
hostile-input tests with the status each must get and what libbz2 says about it.  Seeded; built once per
process."""
import bz2
import functools
import random
from dataclasses import dataclass

OK = 0
(STREAM_ID, BLOCK_SIZE, STREAM_CRC, BLOCK_HEADER, HUFFMAN_GROUPS, ALPHABET, SELECTORS, DECODING_BLOCK, CODE, BLOCK_EXCEEDS,
 START_POINTER, BLOCK_CRC, TRUNCATED, OUTPUT_FULL, RANDOMISED) = range(-110, -125, -1)
BZIP2_CODES = set(range(-124, -109))
BLOCK_MAGIC, END_MAGIC = 0x314159265359, 0x177245385090
GUARD = 64


# ------------------------------------------------------------------ bits
def get_bits(data: bytes, at: int, n: int) -> int:
    """n bits of data from bit `at`, most significant first."""
    v = int.from_bytes(data[at // 8:(at + n + 7) // 8 + 1], "big")
    total = (len(data[at // 8:(at + n + 7) // 8 + 1])) * 8
    return (v >> (total - (at % 8) - n)) & ((1 << n) - 1)


def put_bits(data: bytes, at: int, n: int, value: int) -> bytes:
    """data with the n bits at bit `at` replaced by value."""
    b = bytearray(data)
    for k in range(n):
        p = at + k
        bit = (value >> (n - 1 - k)) & 1
        b[p // 8] = (b[p // 8] & ~(0x80 >> (p % 8))) | ((0x80 >> (p % 8)) if bit else 0)
    return bytes(b)


def flip_bit(data: bytes, at: int) -> bytes:
    return put_bits(data, at, 1, get_bits(data, at, 1) ^ 1)


def find_magics(data: bytes):
    """Bit positions of every 48-bit block magic and end-of-stream magic in data, by a scan of every bit
    position: ([block positions], [end positions])."""
    v = int.from_bytes(data, "big")
    total = len(data) * 8
    blocks, ends = [], []
    mask = (1 << 48) - 1
    for at in range(0, total - 47):
        w = (v >> (total - at - 48)) & mask
        if w == BLOCK_MAGIC:
            blocks.append(at)
        elif w == END_MAGIC:
            ends.append(at)
    return blocks, ends


@dataclass
class Fields:
    """Bit positions of the fields of a stream's first block (the block starts at bit 32)."""
    crc: int
    randomised: int
    start: int
    in_use16: int
    ntables: int
    nsel: int
    ntables_value: int
    nsel_value: int


def first_block_fields(stream: bytes) -> Fields:
    assert get_bits(stream, 32, 48) == BLOCK_MAGIC
    in_use16 = 32 + 48 + 32 + 1 + 24
    maps = bin(get_bits(stream, in_use16, 16)).count("1")
    ntables = in_use16 + 16 + 16 * maps
    return Fields(crc=80, randomised=112, start=113, in_use16=in_use16, ntables=ntables, nsel=ntables + 3,
                  ntables_value=get_bits(stream, ntables, 3), nsel_value=get_bits(stream, ntables + 3, 15))


def libbz2(stream: bytes):
    """What libbz2 says about stream: ("ok", bytes, consumed), ("more", b"", 0) when it wants more input, or
    ("error", b"", 0)."""
    d = bz2.BZ2Decompressor()
    try:
        out = d.decompress(stream)
    except (OSError, ValueError, EOFError):
        return "error", b"", 0
    if not d.eof:
        return "more", b"", 0
    return "ok", out, len(stream) - len(d.unused_data)


# ------------------------------------------------------------------ valid streams
@dataclass
class Valid:
    name: str
    data: bytes
    stream: bytes       # the first stream and whatever follows it
    consumed: int       # bytes of the first stream
    level: int
    ntables: int = 0    # of its first block, where the test asserts it


def _rle1_length(data: bytes) -> int:
    """Bytes of data after bzip2's first run-length stage (a block's length when it fits one block)."""
    n, i = 0, 0
    while i < len(data):
        j = i
        while j < len(data) and data[j] == data[i] and j - i < 255:
            j += 1
        n += j - i if j - i < 4 else 5
        i = j
    return n


@functools.lru_cache(maxsize=None)
def _text(oracle_mod, n):
    return oracle_mod.textgen_chunk(7, n)


def valid_streams(oracle):
    return _valid_streams(oracle)


@functools.lru_cache(maxsize=None)
def _valid_streams(oracle):
    rng = random.Random(20261020)
    out = []

    def add(name, data, level=9, tail=b"", ntables=0):
        s = bz2.compress(data, level)
        out.append(Valid(name, data, s + tail, len(s), level, ntables))

    add("empty", b"")
    for n in (1, 2, 63, 64, 65):
        add(f"bytes{n}", rng.randbytes(n))
    add("all256", bytes(range(256)))
    for n in (4, 5, 259, 260, 1000):
        add(f"run{n}", b"r" * n)
    add("period", b"hello world" * 10)  # a periodic block: its inverse BWT has ten cycles
    for n, t in ((100, 2), (400, 3), (1000, 4), (2000, 5), (5000, 6)):
        add(f"random{n}", rng.randbytes(n), level=1, ntables=t)
    text = _text(oracle, 1000000)
    add("text250k_l1", text[:250000], level=1)
    add("text1m_l9", text, level=9)
    for lv in range(1, 10):
        add(f"level{lv}", text[:30000], level=lv)
    add("two_streams", text[:3000], tail=bz2.compress(b"second stream"))
    add("junk_after", text[3000:5000], tail=b"junk after the stream \x31\x41\x59")
    return tuple(out)


# ------------------------------------------------------------------ mutated streams
@dataclass
class Mutant:
    name: str
    stream: bytes
    cap: int
    status: int
    libbz2: str  # "ok", "more" or "error": asserted before the case is used


def mutants(oracle):
    return _mutants(oracle)


@functools.lru_cache(maxsize=None)
def _mutants(oracle):
    rng = random.Random(77)
    text = _text(oracle, 1000000)[:2000]  # no run of four equal bytes: the block is 2000 bytes long
    assert _rle1_length(text) == len(text)
    s = bz2.compress(text, 9)
    F = first_block_fields(s)
    blocks, ends = find_magics(s)
    assert blocks[0] == 32 and len(ends) == 1
    cap = len(text)
    out = []

    def add(name, stream, status, lib, cap=cap):
        out.append(Mutant(name, stream, cap, status, lib))

    add("magic3", s[:2] + b"x" + s[3:], STREAM_ID, "error")
    add("level0", s[:3] + b"0" + s[4:], BLOCK_SIZE, "error")
    add("level_colon", s[:3] + b":" + s[4:], BLOCK_SIZE, "error")
    add("block_magic", flip_bit(s, 32 + 5), BLOCK_HEADER, "error")
    for k in (0, 17, 31):
        add(f"block_crc_bit{k}", flip_bit(s, F.crc + k), BLOCK_CRC, "error")
    add("stream_crc", flip_bit(s, ends[0] + 48 + 9), STREAM_CRC, "error")
    add("randomised", put_bits(s, F.randomised, 1, 1), RANDOMISED, "error")
    add("start_at_length", put_bits(s, F.start, 24, len(text)), START_POINTER, "error")
    add("start_max", put_bits(s, F.start, 24, (1 << 24) - 1), START_POINTER, "error")
    for t in (0, 1, 7):
        add(f"ntables{t}", put_bits(s, F.ntables, 3, t), HUFFMAN_GROUPS, "error")
    add("nsel0", put_bits(s, F.nsel, 15, 0), SELECTORS, "error")
    big = bz2.compress(rng.randbytes(150000), 9)
    add("exceeds", big[:3] + b"1" + big[4:], BLOCK_EXCEEDS, "error", cap=150000)
    add("cap_short", s, OUTPUT_FULL, "ok", cap=cap - 1)
    for name, data in (("p_empty", b""), ("p_small", b"abracadabra"), ("p_run", b"z" * 300 + b"y")):
        ps = bz2.compress(data, 9)
        for k in range(len(ps)):
            add(f"{name}_{k}", ps[:k], TRUNCATED, "more", cap=len(data))
    return tuple(out)


def start_moved(oracle):
    """Streams whose start pointer is patched to another valid index."""
    text = _text(oracle, 1000000)[:2000]
    s = bz2.compress(text, 9)
    F = first_block_fields(s)
    sp = get_bits(s, F.start, 24)
    return [(put_bits(s, F.start, 24, v), len(text)) for v in ((sp + 1) % len(text), 0 if sp else 1, len(text) - 1 if sp != len(text) - 1 else 7)]


@functools.lru_cache(maxsize=None)
def fuzz_set():
    """300 single-bit and single-byte changes over small streams: (stream, cap)."""
    rng = random.Random(300)
    bases = []
    for k in range(6):
        data = bytes(rng.choice(b"abcdefgh \n") for _ in range(rng.randrange(20, 400))) + bytes(rng.randrange(256) for _ in range(k * 9))
        if k % 2:
            data += b"q" * rng.randrange(4, 300)
        bases.append((bz2.compress(data, 1 + k) + b"tail" * 3, len(data)))  # a change in the tail leaves the stream whole
    out = []
    for i in range(300):
        s, n = bases[i % len(bases)]
        b = bytearray(s)
        at = rng.randrange(len(b))
        if i % 2:
            b[at] ^= 1 << rng.randrange(8)
        else:
            b[at] = rng.randrange(256)
        out.append((bytes(b), n + 64))
    return tuple(out)
