"""tests/deflate_blocks.py, pinned without a GPU: the block reader against the real zlib's streams (every
block type, sync-flushed and finished), its refusals on hand-made bad streams, package-merge against
the plain Huffman cost, and the crafted inputs of tests/deflate_inputs.py for determinism."""
import random
import zlib

import pytest

import deflate_blocks as D
import deflate_inputs as I

SIZES = [1, 2, 3, 100, 4097, 70000]  # 70 000: more than one stored block, and distances up to the window


def _data(kind, n):
    rng = random.Random(n * 7 + len(kind))
    if kind == "text":
        words = [bytes(rng.choice(b"etaoinshrdlu") for _ in range(rng.randrange(2, 9))) for _ in range(200)]
        out = bytearray()
        while len(out) < n:
            out += rng.choice(words) + b" "
        return bytes(out[:n])
    if kind == "zeros":
        return bytes(n)
    if kind == "random":
        return rng.randbytes(n)
    return I.two_symbol(n, n)


STREAMS = [(kind, n, level, strategy, finish)
           for kind in ("text", "zeros", "random", "two")
           for n in SIZES
           for level in (0, 1, 6, 9)
           for strategy in (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY)
           for finish in (False, True)]


def test_reader_against_zlib():
    types = set()
    for kind, n, level, strategy, finish in STREAMS:
        data = _data(kind, n)
        z = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
        x = z.compress(data) + z.flush(zlib.Z_FINISH if finish else zlib.Z_SYNC_FLUSH)
        what = (kind, n, level, strategy, finish)
        blocks = D.read_blocks(x)
        assert D.replay(blocks) == data, what
        assert (blocks[-1].end + 7) // 8 == len(x), what
        assert bool(blocks[-1].bfinal) == finish and not any(b.bfinal for b in blocks[:-1]), what
        for a, b in zip(blocks, blocks[1:]):
            assert b.start == a.end, what
        if not finish:
            assert blocks[-1].btype == 0 and blocks[-1].len == 0 and x[-4:] == b"\0\0\xff\xff", what
        if level == 0:
            assert {b.btype for b in blocks} == {0}, what
        elif strategy == zlib.Z_FIXED:
            # Z_FIXED rules out dynamic blocks only: zlib still stores what the fixed code would grow
            # (random bytes), and its sync flush itself is an empty stored block
            body = {b.btype for b in (blocks if finish else blocks[:-1])}
            assert body == {1} if kind != "random" else body <= {0, 1}, what
        for b in blocks:
            types.add(b.btype)
            if b.btype == 0:
                assert b.len == len(b.payload) and b.tokens is None
                continue
            assert b.header_bits + b.symbol_bits == b.bits
            lf, df = D.token_frequencies(b.tokens)
            if b.btype == 1:
                assert b.header_bits == 3 and b.symbol_bits == D.fixed_cost(b.tokens), what
                continue
            assert len(b.lit_lens) == b.hlit and len(b.dist_lens) == b.hdist and len(b.cl_lens) == 19
            assert 4 <= b.hclen <= 19 and b.repeats <= {16, 17, 18}
            x_bits = sum(D.LEN_EXTRA[s - 257] * f for s, f in enumerate(lf) if s > 256) + sum(D.DIST_EXTRA[s] * f for s, f in enumerate(df))
            lens_l, lens_d = b.lit_lens + [0] * 30, b.dist_lens + [0] * 30
            assert b.symbol_bits == x_bits + sum(f * lens_l[s] for s, f in enumerate(lf)) + sum(f * lens_d[s] for s, f in enumerate(df)), what
            assert D.kraft(b.lit_lens)[0] == D.kraft(b.lit_lens)[1], what
    assert types == {0, 1, 2}


def test_reader_sees_repeat_symbols():
    z = zlib.compressobj(6, zlib.DEFLATED, -15)
    blocks = D.read_blocks(z.compress(_data("text", 4097)) + z.flush())
    assert blocks[0].btype == 2 and blocks[0].repeats


def _pack(fields):
    """bytes of (value, bit count) fields, least significant bit first"""
    acc = n = 0
    for v, b in fields:
        acc |= v << n
        n += b
    return acc.to_bytes((n + 7) // 8, "little")


def _dynamic_header(cl_lens_in_order):
    return [(1, 1), (2, 2), (0, 5), (0, 5), (len(cl_lens_in_order) - 4, 4)] + [(l, 3) for l in cl_lens_in_order]


def test_reader_refuses_what_the_rfc_forbids():
    with pytest.raises(D.DeflateError, match="over-subscribed"):
        D.read_blocks(_pack(_dynamic_header([1, 1, 1, 0]) + [(0, 64)]))  # three one-bit codes
    with pytest.raises(D.DeflateError, match="incomplete"):
        D.read_blocks(_pack(_dynamic_header([1, 2, 0, 0]) + [(0, 64)]))
    # a code-length code of two one-bit codes, for the lengths 0 (bit 0) and 1 (bit 1); 257 + 1 lengths
    order = [0] * 19
    order[D.CL_ORDER.index(0)] = order[D.CL_ORDER.index(1)] = 1
    hdr = _dynamic_header(order)
    with pytest.raises(D.DeflateError, match="literal/length code: over-subscribed"):
        D.read_blocks(_pack(hdr + [(1, 1)] * 258 + [(0, 64)]))  # 257 one-bit literal/length codes
    with pytest.raises(D.DeflateError, match="literal/length code: incomplete"):
        D.read_blocks(_pack(hdr + [(0, 1)] * 256 + [(1, 1), (0, 1)] + [(0, 64)]))  # the end of block alone
    with pytest.raises(D.DeflateError, match="no code for the end of block"):
        D.read_blocks(_pack(hdr + [(1, 1)] * 2 + [(0, 1)] * 256 + [(0, 64)]))
    one = D.read_blocks(_pack(hdr + [(1, 1)] + [(0, 1)] * 255 + [(1, 1), (1, 1)] + [(0, 1), (1, 1)]))  # literal 0, end
    assert one[0].dist_lens == [1] and D.replay(one) == b"\0"  # the single one-bit distance code is allowed
    # fixed blocks: literal 'a' (0x30 + 97, 8 bits, most significant first), then length 3 (symbol 257:
    # 0000001) at distance 2 (code 1, 5 bits: 00001 -> reversed 10000) with one byte before it
    lit_a = int(format(0x30 + 97, "08b")[::-1], 2)
    bad = [(0, 1), (1, 2), (lit_a, 8), (0b1000000, 7), (0b10000, 5), (0, 7)]
    with pytest.raises(D.DeflateError, match="distance 2 with 1 bytes"):
        D.read_blocks(_pack(bad))
    good = [(1, 1), (1, 2), (lit_a, 8), (0b1000000, 7), (0b00000, 5), (0, 7)]
    assert D.replay(D.read_blocks(_pack(good))) == b"aaaa"
    for sym, what in ((286, "length symbol 286"), (287, "length symbol 287")):
        code = int(format(0xC0 + sym - 280, "08b")[::-1], 2)
        with pytest.raises(D.DeflateError, match=what):
            D.read_blocks(_pack([(1, 1), (1, 2), (lit_a, 8), (code, 8), (0, 32)]))
    for dsym in (30, 31):
        code = int(format(dsym, "05b")[::-1], 2)
        with pytest.raises(D.DeflateError, match=f"distance symbol {dsym}"):
            D.read_blocks(_pack([(1, 1), (1, 2), (lit_a, 8), (0b1000000, 7), (code, 5), (0, 32)]))
    with pytest.raises(D.DeflateError, match="NLEN"):
        D.read_blocks(b"\x00\x02\x00\xfd\xfe" + b"ab")
    assert D.replay(D.read_blocks(b"\x01\x02\x00\xfd\xff" + b"ab")) == b"ab"
    with pytest.raises(D.DeflateError, match="ends inside"):
        D.read_blocks(b"\x01\x02\x00\xfd\xff" + b"a")
    with pytest.raises(D.DeflateError, match="block type 3"):
        D.read_blocks(b"\x07")


def test_cost_references():
    assert D.huffman_cost([5, 0, 0]) == (0, 0) and D.huffman_cost([]) == (0, 0)
    assert D.huffman_cost([1, 1]) == (2, 1) and D.huffman_cost([1, 1, 2, 4]) == (1 * 3 + 1 * 3 + 2 * 2 + 4, 3)
    assert D.limited_cost([1, 1, 2, 4], 2) == 16 and D.limited_cost([1, 1, 2, 4], 3) == 14
    assert D.stored_cost(0) == 0 and D.stored_cost(1) == 48 and D.stored_cost(65535) == 8 * 65540
    assert D.stored_cost(65536) == 8 * (65536 + 10)
    assert D.fixed_cost([]) == 7
    assert D.fixed_cost([("lit", 0), ("lit", 143), ("lit", 144), ("lit", 255)]) == 7 + 8 + 8 + 9 + 9
    # length 3: symbol 257 (7 bits); 11: 265 (7 + 1 extra); 115: 280 (8 + 4); 258: 285 (8); distances 1
    # (code 0), 5 (code 4, 1 extra), 32768 (code 29, 13 extra)
    assert D.fixed_cost([("match", 3, 1), ("match", 11, 5), ("match", 115, 32768), ("match", 258, 4)]) == 7 + (7 + 5) + (8 + 6) + (12 + 18) + (8 + 5)
    assert D.length_symbol(257) == (284, 5) and D.length_symbol(258) == (285, 0) and D.distance_symbol(24577) == (29, 13)
    with pytest.raises(ValueError):
        D.limited_cost([1] * 5, 2)
    rng = random.Random(1951)
    seen = {True: 0, False: 0}
    for trial in range(300):
        n = rng.randrange(2, 287)
        shape = trial % 3
        if shape == 0:
            f = [rng.randrange(1, 1000) for _ in range(n)]
        elif shape == 1:
            f = [int(rng.paretovariate(0.6)) for _ in range(n)]   # long tails: deep trees
        else:
            f = [max(1, int(1.5 ** rng.randrange(0, 30))) for _ in range(n)]
        rng.shuffle(f)
        for maxbits in (15, 9 if n <= 512 else 15):
            h = D.huffman_cost(f)
            lim = D.limited_cost(f, maxbits)
            seen[h.depth <= maxbits] += 1
            if h.depth <= maxbits:
                assert lim == h.cost, (trial, maxbits)
            else:
                assert lim >= h.cost, (trial, maxbits)
    assert seen[True] > 50 and seen[False] > 50  # both sides of the limit were tried
    assert D.limited_cost([7] * 128, 7) == 7 * 7 * 128
    fib = I.FIB + [4181, 6765]
    assert len(fib) == 20
    h = D.huffman_cost(fib)
    assert h.depth == 19 and D.limited_cost(fib, 15) > h.cost and D.limited_cost(fib, 19) == h.cost


def test_crafted_inputs_are_deterministic():
    for name, gen in I.GENERATORS.items():
        a = gen(3)
        assert a == gen(3) and 0 < len(a) <= 65536, name
        assert a != gen(4), name
    assert len(I.dist_fib(3)) == 56312 and len(I.cl_fib(3)) == 7749
    d = I.cl_fib(3)
    assert len({d[i:i + 4] for i in range(len(d) - 3)}) == len(d) - 3  # no 4-byte window repeats: no matches
    assert len(I.full_slot(3)) == 65536 and I.full_slot(3)[-300:] == I.full_slot(3)[-600:-300]
    a, b = I.stamp_pair(3)
    assert len(a) == len(b) == 200 and sum(x != y for x, y in zip(a, b)) > 150
    shared = {a[i:i + 4] for i in range(197)} & {b[i:i + 4] for i in range(197)}
    assert len(shared) >= 20 and all(a.find(g) != b.find(g) for g in shared)
