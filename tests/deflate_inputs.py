"""Crafted inputs for the structure tests of the deflate encoder (tests/test_gpu_deflate_structure.py):
chunks of at most 64 KiB built so that the encoder's own tokens reach one named path.  Pure Python and
seeded: the same seed gives the same bytes (tests/test_deflate_blocks.py).

The three `*_fib` inputs aim a Fibonacci frequency profile, whose Huffman tree is a chain, at one of the
three codes, so that its unlimited depth passes the limit (15 bits, 7 for the code-length code) and the
encoder has to fold the code back.  Whether it did is for the test to assert from the parsed tokens."""
import random

FIB = [1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597, 2584]
PREFIX = 2200


def _append_unit(d, rng, length, lo, hi):
    """one unit: a `length`-byte copy of the bytes some lo <= dist <= hi back, chosen so that the
    source's first 4 bytes do not occur again before the copy (a matcher that keeps the latest
    position of a 4-gram finds this source), then 4 fresh bytes, the first unlike the source's
    continuation (so the match ends where the copy does)"""
    p = len(d)
    for _ in range(64):
        dist = rng.randrange(max(lo, length), hi + 1)
        src = p - dist
        d += d[src:src + length]
        if d.find(d[src:src + 4], src + 1, p + 3) < 0:
            break
        del d[p:]
    else:
        raise AssertionError("no distance with a unique source")
    fresh = bytearray(rng.randbytes(4))
    if fresh[0] == d[src + length]:
        fresh[0] ^= 0x55
    d += fresh


def dist_fib(seed):
    """Distance codes 4..21 with Fibonacci frequencies, the most frequent at the smallest distance:
    2200 random bytes, then 6764 units of a 4-byte copy and 4 fresh bytes.  56 312 bytes."""
    rng = random.Random(seed)
    from deflate_blocks import DIST_BASE
    codes = [4 + i for i, f in enumerate(reversed(FIB)) for _ in range(f)]
    rng.shuffle(codes)
    d = bytearray(rng.randbytes(PREFIX))
    for c in codes:
        _append_unit(d, rng, 4, DIST_BASE[c], DIST_BASE[c + 1] - 1)
    return bytes(d)


def len_fib(seed, ncodes=15, fresh=32):
    """Length codes 258.. (lengths 4, 5, ...) with Fibonacci frequencies, the most frequent the
    shortest, among uniformly random literals: 1596 units of a copy of the code's base length from 300
    to 2048 bytes back and 32 fresh bytes.  The chain of rare length codes (and the end of block) hangs
    below the 256 literals' own 8 levels, and it is the literals' frequency (some 200 each) that sets how
    many codes the chain holds before it reaches them: 4 fresh bytes per unit, as in dist_fib, leave
    the unlimited depth at 13 to 15 for any size up to 64 KiB.  Some 62 300 bytes."""
    rng = random.Random(seed)
    from deflate_blocks import LEN_BASE
    lengths = [LEN_BASE[1 + i] for i, f in enumerate(reversed(FIB[:ncodes])) for _ in range(f)]
    rng.shuffle(lengths)
    d = bytearray(rng.randbytes(PREFIX))
    for length in lengths:
        _append_unit(d, rng, length, 300, 2048)
        d += rng.randbytes(fresh - 4)
    return bytes(d)


def cl_fib(seed):
    """Literals only, code lengths with a long-tailed profile: triples (x, 40 + i // 108, 148 + i % 108)
    with x from 16 symbols of Fibonacci frequencies.  Every 4-byte window holds one (i // 108, i % 108)
    pair whole, so none repeats.  7749 bytes."""
    rng = random.Random(seed)
    xs = [s for s, f in enumerate(FIB[:16]) for _ in range(f)]
    rng.shuffle(xs)
    return bytes(b for i, x in enumerate(xs) for b in (x, 40 + i // 108, 148 + i % 108))


def two_symbol(seed, n):
    return bytes(b"ab"[b & 1] for b in random.Random(seed).randbytes(n))


def inner_repeat(seed):
    """W + F + W[100:200] + tail, all random: one repeat of 100 bytes whose source starts inside W;
    returns (bytes, position of the repeat, its distance)"""
    rng = random.Random(seed)
    w, f, tail = rng.randbytes(300), rng.randbytes(500), rng.randbytes(8)
    return w + f + w[100:200] + tail, len(w) + len(f), len(w) + len(f) - 100


def inner_of_match(seed):
    """W + F + W + G + W[100:200] + tail: the second W is coded as matches, so the latest entry of
    W[100:104] is a position inside a match, and the last repeat is found there (at distance
    len(W) + len(G) - 100) only if those positions were entered; returns (bytes, position of the
    last repeat, that distance)"""
    rng = random.Random(seed)
    w, f, g, tail = rng.randbytes(300), rng.randbytes(500), rng.randbytes(400), rng.randbytes(8)
    return w + f + w + g + w[100:200] + tail, 2 * len(w) + len(f) + len(g), len(w) + len(g) - 100


def full_slot(seed):
    """8 KiB of two-symbol data (many short matches), random bytes up to 65 536 (one token each: the
    token slot fills), the last 600 bytes a 300-byte random marker placed twice"""
    rng = random.Random(seed)
    m = rng.randbytes(300)
    head = two_symbol(seed + 1, 8192)
    return head + rng.randbytes(65536 - len(head) - 600) + m + m


def stamp_pair(seed):
    """two 200-byte inputs sharing five 8-byte pieces at different positions, unlike elsewhere: a table
    entry left by one would offer the other a candidate whose bytes differ"""
    rng = random.Random(seed)
    pieces = [rng.randbytes(8) for _ in range(5)]
    a, b = bytearray(rng.randbytes(200)), bytearray(rng.randbytes(200))
    for i, pc in enumerate(pieces):
        a[10 + 36 * i:18 + 36 * i] = pc
        b[150 - 30 * i:158 - 30 * i] = pc
    # each repeats its own first piece once, so that both have a match of their own as well
    a[190:198] = pieces[0]
    b[190:198] = pieces[4]
    return bytes(a), bytes(b)


def stamp_plant(seed):
    """(planter, victim): two unlike 200-byte inputs holding the same six 4-byte pieces, the victim's
    each 12 bytes later than the planter's.  A table entry of the planter's that the victim meets under
    the same stamp is taken for a match whose first four bytes were never compared with the victim's."""
    rng = random.Random(seed)
    c, v = bytearray(rng.randbytes(200)), bytearray(rng.randbytes(200))
    for k in range(6):
        g = rng.randbytes(4)
        c[8 + 30 * k:12 + 30 * k] = g
        v[20 + 30 * k:24 + 30 * k] = g
    return bytes(c), bytes(v)


GENERATORS = {
    "stamp_plant": lambda s: b"".join(stamp_plant(s)),
    "dist_fib": lambda s: dist_fib(s),
    "len_fib": lambda s: len_fib(s),
    "cl_fib": lambda s: cl_fib(s),
    "two_symbol": lambda s: two_symbol(s, 700),
    "inner_repeat": lambda s: inner_repeat(s)[0],
    "inner_of_match": lambda s: inner_of_match(s)[0],
    "full_slot": lambda s: full_slot(s),
    "stamp_pair": lambda s: b"".join(stamp_pair(s)),
}
