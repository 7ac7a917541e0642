"""Inputs of the LZMA encoder tests (no GPU needed to build them): the smallest shapes at which the coder can
go wrong.  Each is (name, bytes); items(oracle) adds the oracle generator's text."""
import functools
import random

# A short random input whose coding (default settings, no end marker) propagates a carry through a pending
# 0xFF byte: found by searching seeds with nx_lzma_encode_host's stats (max_carry_ff >= 1); the host test
# asserts that it still does.
CARRY_SEED, CARRY_LEN = 0, 200

PROPS = [(3, 0, 2), (0, 0, 0), (4, 0, 0), (0, 4, 4), (1, 3, 1)]  # liblzma and the model decoder
PROPS_MODEL_ONLY = [(8, 4, 4), (3, 2, 0)]                     # lc + lp > 4: the model decoder alone

RUNS = [272, 273, 274, 277, 546, 65536]
DISTANCES = [1, 2, 3, 4, 5, 96, 127, 128, 129, 4097, 65535, 65536]
MATCH_LENGTHS = [4, 9, 10, 17, 18, 273]
RANDOM_LENGTHS = [1, 200, 500, 1000, 10000, 65536]


def rand(seed, n):
    return random.Random(seed).randbytes(n)


def near_copy(dist, length):
    """a random head, then `length` bytes that repeat at distance `dist` (periodic where length > dist), then a
    byte that ends the repetition"""
    d = bytearray(rand(1000 + dist, max(dist, 8)))
    for _ in range(length):
        d.append(d[-dist])
    d.append(d[-dist] ^ 0x55)
    return bytes(d + rand(7, 6))


def far_copy(dist, length):
    """`length` random non-zero bytes, zeros, and the same bytes again `dist` after their first place: the zeros
    share one table entry, so the first copy's entries survive any distance"""
    r = random.Random(dist * 1000 + length)
    m = bytes(r.randrange(1, 256) for _ in range(length))
    assert dist >= length + 1
    return m + bytes(dist - length) + m + b"\x01\x02\x03"


def cycle(distances, blocks=24, block=8):
    """blocks of `block` bytes, block k repeating what lies distances[k % len] back: the distances alternate,
    so all but the last used come from the rep list (two distances: rep1, three: rep2, four: rep3)"""
    d = bytearray(rand(len(distances), max(distances) + 16))
    for k in range(blocks):
        dist = distances[k % len(distances)]
        for _ in range(block):
            d.append(d[-dist])
        d.append(d[-dist] ^ 0xFF)  # ends the repetition
    return bytes(d)


@functools.lru_cache(maxsize=None)
def directed():
    out = [("len%d" % n, b"lzma!"[:n]) for n in range(6)]
    out += [("run%d" % n, b"z" * n) for n in RUNS]
    out += [("period4", b"abcd" * 120), ("period5", b"abcde" * 100)]
    out += [("dist%d" % d, near_copy(d, 6) if d < 8 else far_copy(d, 8)) for d in DISTANCES]
    out += [("mlen%d" % n, far_copy(300, n)) for n in MATCH_LENGTHS]
    out += [("cycle2", cycle((100, 230))), ("cycle3", cycle((100, 230, 370))), ("cycle4", cycle((100, 230, 370, 510)))]
    out += [("random%d" % n, rand(n, n)) for n in RANDOM_LENGTHS]
    out += [("carry", rand(CARRY_SEED, CARRY_LEN))]
    return tuple(out)


def items(oracle):
    return directed() + (("text30k", oracle.textgen_chunk(7, 30000)), ("text200k", oracle.textgen_chunk(7, 200000)))


def dict_cases():
    """(name, bytes, dict_size): a repetition at distance 32 against dictionaries of 0, 1 and 16, and one at
    65537 against 65536: no packet may reach past the dictionary"""
    rep32 = rand(32, 32) * 6
    return [("rep32_dict%d" % s, rep32, s) for s in (0, 1, 16)] + [("rep65537_dict65536", far_copy(65537, 16), 65536)]
