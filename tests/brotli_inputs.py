"""Inputs of the Brotli encoder tests (no GPU needed to build them): named items, each chosen for a place the
encoder can go wrong.  Each is (name, bytes); items(oracle) adds the oracle generator's text."""
import functools
import random

LGWINS = [10, 16, 22, 24]
INSERT_BOUNDARIES = [5, 6, 129, 130, 2113, 2114, 6209, 6210, 22594]  # the insert-length codes' edges
COPY_BOUNDARIES = [9, 10, 133, 134, 2117, 2118]                       # the copy-length codes' edges


def rand(seed, n):
    return random.Random(seed).randbytes(n)


def few(k, n=600):
    """n bytes over k distinct values in no order a matcher can use for long"""
    r = random.Random(k)
    return bytes(r.choices(b"ETAOIN"[:k], k=n))


def skewed4():
    """16 literals with counts 9, 4, 2, 1 and no four bytes twice, then copies of them: the simple code of
    lengths 1, 2, 3, 3 (few(4) gives 2, 2, 2, 2)"""
    return b"aaabbaabcaacabda" * 6


def fibonacci(nsym=18):
    """18 byte values with Fibonacci counts, each followed by three bytes of a scrambled counter that keep the
    matcher from finding anything: the literal code's unlimited Huffman depth is 17"""
    counts, a, b = [], 1, 1
    for _ in range(nsym):
        counts.append(a)
        a, b = b, a + b
    lits = []
    for v, c in enumerate(counts):
        lits += [65 + v] * c
    random.Random(24).shuffle(lits)
    out = bytearray()
    for i, lit in enumerate(lits):
        c = (i * 2654435761) % 8000
        out += bytes([lit, 0x80 + c % 20, 0xA0 + (c // 20) % 20, 0xC0 + c // 400])
    return bytes(out)


PAD = bytes(3000)  # a run that makes the compressed form of a meta-block the smaller one


def insert_then_repeat(n):
    """n random bytes that hold no match, a repeat of their first bytes, and the pad"""
    d = rand(n, n)
    return d + d[:min(n, 40)] + PAD


def repeat_of(length):
    """a random block of `length` non-zero bytes, a gap, the block again, a byte that ends the repeat, and the pad"""
    r = random.Random(length)
    m = bytes(r.randrange(1, 256) for _ in range(length))
    return m + b"\xfe" * 7 + m + b"\xff\x01\x02" + PAD


def far_repeat():
    """200 KiB whose second half repeats a block first seen more than 65 536 bytes earlier, across meta-blocks"""
    block = rand(5, 20000)
    filler = bytes(random.Random(6).choices(b"0123456789", k=102400 - 20000))
    second = bytes(random.Random(8).choices(b"abcdef", k=102400 - 20000))
    return block + filler + second[:40000] + block + second[40000:]


def ring():
    """records of 24 bytes whose fields repeat at the same few distances over and over: ring and implicit commands"""
    r = random.Random(9)
    out = bytearray(rand(10, 24))
    for _ in range(80):
        rec = bytearray(out[-24:])
        rec[r.randrange(24)] = r.randrange(256)
        rec[r.randrange(24)] = r.randrange(256)
        out += rec
    return bytes(out)


def window10():
    """data repeating 2 000 bytes back: at lgwin 10 no copy may reach it (1 008 is the farthest)"""
    d = rand(11, 2000)
    return d + d + d[:500]


@functools.lru_cache(maxsize=None)
def directed():
    out = [("len%d" % n, b"br!"[:n]) for n in range(4)]
    out += [("run%d" % n, b"z" * n) for n in (65535, 65536, 65537)]
    out += [("few%d" % k, few(k)) for k in range(1, 6)] + [("skewed4", skewed4())]
    out += [("fibonacci", fibonacci())]
    out += [("random70000", rand(70000, 70000))]
    out += [("insert%d" % n, insert_then_repeat(n)) for n in INSERT_BOUNDARIES]
    out += [("copy%d" % n, repeat_of(n)) for n in COPY_BOUNDARIES]
    out += [("far", far_repeat()), ("ring", ring()), ("window10", window10())]
    return tuple(out)


def items(oracle):
    return directed() + tuple(("text%d" % n, oracle.textgen_chunk(3, n)) for n in (300, 5000, 65536))


def ratio_set(oracle):
    """the three text items and 16 text chunks of 64 KiB"""
    return [oracle.textgen_chunk(3, n) for n in (300, 5000, 65536)] + [oracle.textgen_chunk(100 + k, 65536) for k in range(16)]
