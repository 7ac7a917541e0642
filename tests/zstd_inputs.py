"""Inputs of the Zstandard encoder tests (no GPU needed to build them)."""
import random


def skewed(rng, n, symbols=64, base=0x30, rate=0.12):
    """bytes of a `symbols`-letter alphabet, geometrically skewed, in which no four bytes recur (a byte
    that would complete a repeat is drawn again): Huffman gains and a 4-byte matcher finds nothing,
    so the literal count is n"""
    out, seen = bytearray(), set()
    while len(out) < n:
        b = base + min(symbols - 1, int(rng.expovariate(rate)))
        g = bytes(out[-3:]) + bytes([b])
        if len(g) == 4 and g in seen:
            continue
        seen.add(g)
        out.append(b)
    return bytes(out)


def high(rng, n):
    """values 144..255, skewed: the last symbol is above 127, so the direct weight form cannot describe the tree"""
    return bytes(144 + min(111, int(rng.expovariate(0.06))) for _ in range(n))


def periodic(rng, n, period):
    base = rng.randbytes(min(n, period))
    return (base * (n // len(base) + 1))[:n]


def markers(seed, k, gap, lead=40, mlen=8):
    """random bytes with one marker and k repeats of it, each `gap` bytes after the last: k sequences of
    one literal-length code (lead + gap and gap - mlen share it for the gaps used), one match length,
    one distance"""
    rng = random.Random(seed)
    m = rng.randbytes(mlen)
    out = bytearray(rng.randbytes(lead))
    for _ in range(k + 1):
        out += m + rng.randbytes(gap - mlen)
    return bytes(out)


def recur(seed, n, src, dst, length):
    """n random bytes whose `length` bytes at src recur at dst"""
    d = bytearray(random.Random(seed).randbytes(n))
    d[dst:dst + length] = d[src:src + length]
    return bytes(d)
