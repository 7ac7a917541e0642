"""GPU tests of the deflate encoder's structure: what tests/test_gpu_deflate.py's inflate check cannot
see.  Every output is first held to that contract (zlib inflates it to the chunk, it ends 00 00 FF FF),
then read block by block with tests/deflate_blocks.py (pinned to the real zlib in
tests/test_deflate_blocks.py) and held to the properties csrc/deflate.hip documents: one block per
chunk in the cheapest of the three encodings by exact bit count, complete codes that are optimal
whenever the optimum fits the length limit, trimmed counts, no repeat symbols, and the matcher's
promises (inner positions entered, matches clipped at 258 bytes / the chunk end / the window, literals
once the token slot is full).  Token choice and tie-breaking stay free: the codes are judged by cost
against the textbook Huffman construction and package-merge, never against the kernel's arithmetic.

The three `*_fib` inputs (tests/deflate_inputs.py) reach the fold-back of over-long codes in
build_lengths, one per code, and each test asserts from the parsed output that it did (the unlimited
Huffman depth of the frequencies it counted exceeds the limit).  The literal/length case needs 32 fresh
bytes per unit, not the 4 of the distance case: with 4 its depth stays at 13 to 15 at any size up to 64 KiB."""
import random
import time
import zlib

import pytest

import deflate_blocks as D
import deflate_inputs as I
from test_gpu_deflate import _check_block_run, _contents, _encode

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TOKEN_SLOT = 49148
# The most the fold-back of over-long codes may cost over the optimal length-limited code
# (package-merge), as a fraction of it: the largest excess measured on the MI355X over the three *_fib
# inputs and the handler message (deflate encode), rounded up to the next 0.1 %.  Every one
# measured 0 (the fold-back met package-merge's cost: 17 595, 586 and 454 906 bits, each 2 or 3 over the
# unlimited Huffman cost), so the figure is 0: on these inputs the folded code is optimal.
LIMIT_EXCESS = 0.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def B():
    from netty_amd import batch
    return batch


def _parse(chunk, out, what):
    _check_block_run(chunk, out, what)
    blocks = D.read_blocks(out)
    assert D.replay(blocks) == chunk, what
    assert blocks[-1].end == 8 * len(out), what
    assert not any(b.bfinal for b in blocks), what
    return blocks


def _padded(freqs):
    """the frequencies with the documented padding: symbols 0 and/or 1 are added (as if seen once)
    until two symbols occur"""
    f = list(freqs)
    for s in (0, 1):
        if sum(1 for x in f if x) < 2 and f[s] == 0:
            f[s] = 1
    return f


def _check_code(lens, freqs, maxbits, what):
    """one emitted code against the frequencies it was built for; returns (unlimited depth, excess over
    the optimal limited cost as a fraction, or None where the limit was not reached)"""
    f = _padded(freqs)
    lens = list(lens) + [0] * (len(f) - len(lens))
    assert max(lens) <= maxbits, what
    total, unit = D.kraft(lens)
    assert total == unit, (what, total, unit)
    assert [s for s, l in enumerate(lens) if l] == [s for s, x in enumerate(f) if x], what
    cost = sum(x * l for x, l in zip(f, lens))
    best = D.huffman_cost(f)
    if best.depth <= maxbits:
        assert cost == best.cost, (what, cost, best)
        return best.depth, None
    lim = D.limited_cost(f, maxbits)
    excess = (cost - lim) / lim
    print(f"deflate length limit: {what}: unlimited depth {best.depth} over {maxbits}, cost {cost} against "
          f"package-merge {lim} (Huffman {best.cost}): excess {excess:.6f}")
    assert cost >= lim, (what, cost, lim)
    assert excess <= LIMIT_EXCESS, (what, cost, lim)
    return best.depth, excess


def _check_huffman_block(blk, n, what):
    """code properties and block choice of one emitted Huffman block over n bytes; returns the
    unlimited depths {"lit": .., "dist": .., "cl": ..} of a dynamic block's frequencies"""
    assert blk.bits < D.stored_cost(n), what
    lf, df = D.token_frequencies(blk.tokens)
    if blk.btype == 1:
        assert blk.bits == 3 + D.fixed_cost(blk.tokens), what
        # fixed was no worse than any dynamic block could have been: the optimal codes' symbol bits
        # and the dearest header there is (19 + 316 lengths of 7 bits) bound the dynamic form from above
        extra = sum(D.LEN_EXTRA[s - 257] * x for s, x in enumerate(lf) if s > 256) + sum(D.DIST_EXTRA[s] * x for s, x in enumerate(df))
        dearest = 17 + 3 * 19 + 7 * 316 + D.limited_cost(_padded(lf), 15) + D.limited_cost(_padded(df), 15) + extra
        assert blk.bits <= dearest, (what, blk.bits, dearest)
        return None
    assert blk.btype == 2, what
    assert blk.bits < 3 + D.fixed_cost(blk.tokens), what
    assert not blk.repeats, what
    depth = {}
    depth["lit"] = _check_code(blk.lit_lens, lf, 15, (what, "literal/length"))[0]
    depth["dist"] = _check_code(blk.dist_lens, df, 15, (what, "distance"))[0]
    assert blk.lit_lens[-1] and blk.dist_lens[-1], what  # hlit - 1 and hdist - 1 are the last used symbols
    cf = [0] * 19
    for l in blk.lit_lens + blk.dist_lens:
        cf[l] += 1
    depth["cl"] = _check_code(blk.cl_lens, cf, 7, (what, "code-length"))[0]
    in_order = [blk.cl_lens[s] for s in D.CL_ORDER]
    assert blk.hclen == max(4, max(i + 1 for i, l in enumerate(in_order) if l)), what
    assert blk.header_bits == 17 + 3 * blk.hclen + sum(cf[l] * blk.cl_lens[l] for l in range(19)), what
    return depth


def _check_chunk(chunk, out, what):
    """shape of one non-empty chunk's output: one block (ceil(n / 65535) stored ones) and the empty
    stored block; returns (the block or None when stored, a dynamic block's depths)"""
    n = len(chunk)
    blocks = _parse(chunk, out, what)
    last = blocks[-1]
    assert last.btype == 0 and last.len == 0, what
    if blocks[0].btype == 0:
        assert [b.btype for b in blocks] == [0] * (-(-n // 65535) + 1), what
        assert [b.len for b in blocks[:-1]] == [min(65535, n - o) for o in range(0, n, 65535)], what
        assert len(out) == D.stored_cost(n) // 8 + 5, what
        return None, None
    assert len(blocks) == 2, what
    return blocks[0], _check_huffman_block(blocks[0], n, what)


@pytest.fixture(scope="module")
def corpus(B, dev, oracle):
    """the corpus of tests/test_gpu_deflate.py at level 6, one launch, parsed once:
    {(kind, n): (chunk, out, block or None, depths)}"""
    cases = _contents(oracle)
    outs, st = _encode(B, dev, [c for _, _, c in cases])
    assert st == [0] * len(cases)
    return {(k, n): (c, o) + _check_chunk(c, o, (k, n)) for (k, n, c), o in zip(cases, outs)}


CRAFTED = {
    "dist_fib": lambda: I.dist_fib(4),
    "cl_fib": lambda: I.cl_fib(1),
    "len_fib": lambda: I.len_fib(2),
    "inner_repeat": lambda: I.inner_repeat(1)[0],
    "inner_of_match": lambda: I.inner_of_match(1)[0],
    "full_slot": lambda: I.full_slot(1),
    "zeros1000": lambda: bytes(1000),
    "two700": lambda: I.two_symbol(7, 700),
}


@pytest.fixture(scope="module")
def crafted(B, dev):
    """the crafted inputs at level 6, one launch: {name: (chunk, out, block or None, depths)}"""
    chunks = {k: f() for k, f in CRAFTED.items()}
    chunks.update({f"zeros{n}": bytes(n) for n in range(5, 13)})
    outs, st = _encode(B, dev, list(chunks.values()))
    assert st == [0] * len(chunks)
    return {k: (c, o) + _check_chunk(c, o, k) for (k, c), o in zip(chunks.items(), outs)}


def _matches(blk):
    return [t for t in blk.tokens if t[0] == "match"]


def test_shape_codes_and_block_choice_on_the_corpus(corpus):
    """the fixture has held every chunk to the shape, the code properties and the block choice; here:
    which encoding the three landmark chunks got, and that all three occur"""
    assert corpus[("random", 65536)][2] is None  # stored
    assert corpus[("text", 65536)][2].btype == 2
    c, o, blk, _ = corpus[("text", 1)]
    assert blk.btype == 1
    kinds = {None if blk is None else blk.btype for _, _, blk, _ in corpus.values()}
    assert kinds == {None, 1, 2}


def test_single_byte_is_a_fixed_block(B, dev):
    outs, st = _encode(B, dev, [b"x"])
    blk, _ = _check_chunk(b"x", outs[0], "x")
    assert st == [0] and blk.btype == 1 and blk.tokens == [("lit", ord("x"))]


def test_codes_and_block_choice_on_the_crafted_inputs(crafted):
    assert all(blk is not None for _, _, blk, _ in crafted.values())
    assert {k for k, (_, _, blk, _) in crafted.items() if blk.btype == 2} >= {"dist_fib", "cl_fib", "len_fib", "full_slot", "two700"}
    # fewer than two distance symbols: the documented padding gives symbols 0 and 1 one bit each
    blk = crafted["cl_fib"][2]
    assert _matches(blk) == [] and blk.dist_lens == [1, 1]
    blk = crafted["zeros1000"][2]
    if blk.btype == 2:
        assert blk.dist_lens == [1, 1]


def test_length_limit_distance_code(crafted):
    """witness: the distance frequencies of the parsed tokens need more than 15 bits unlimited"""
    _, _, blk, depth = crafted["dist_fib"]
    assert len(_matches(blk)) > 6700
    assert depth["dist"] > 15, depth


def test_length_limit_code_length_code(crafted):
    """witness: the frequencies of the transmitted code lengths need more than 7 bits unlimited"""
    _, _, blk, depth = crafted["cl_fib"]
    assert _matches(blk) == []
    assert depth["cl"] > 7, depth


def test_length_limit_literal_length_code(crafted):
    """witness: the literal/length frequencies of the parsed tokens need more than 15 bits unlimited"""
    _, _, blk, depth = crafted["len_fib"]
    assert depth["lit"] > 15, depth


def _covering(blk, pos):
    """the token that covers byte `pos` of the block's output, and where it starts"""
    at = 0
    for t in blk.tokens:
        size = 1 if t[0] == "lit" else t[1]
        if at + size > pos:
            return t, at
        at += size
    raise AssertionError(pos)


def test_matcher_finds_a_repeat_of_inner_bytes(crafted):
    for name, (_, pos, dist) in (("inner_repeat", I.inner_repeat(1)), ("inner_of_match", I.inner_of_match(1))):
        blk = crafted[name][2]
        t, at = _covering(blk, pos)
        assert at == pos and t[0] == "match" and t[2] == dist, (name, t, at)
        assert 100 <= t[1] <= 108, (name, t)  # the 100 bytes, and the tail's where it agrees by chance
    # inner_of_match: the source 600 back lies inside the match that coded the second W; the first W,
    # 1400 back, is what a matcher that entered only probed positions would have found
    blk = crafted["inner_of_match"][2]
    assert _covering(blk, 900)[0][0] == "match" and _covering(blk, 900)[1] < 900


def test_matches_are_clipped_at_258_and_at_the_chunk_end(crafted):
    blk = crafted["zeros1000"][2]
    m = _matches(blk)
    assert {t[2] for t in m} == {1} and max(t[1] for t in m) == 258
    assert [t[1] for t in m].count(258) == 3
    assert sum(t[1] for t in m) + sum(1 for t in blk.tokens if t[0] == "lit") == 1000
    for n in range(5, 13):
        blk = crafted[f"zeros{n}"][2]
        assert sum(1 if t[0] == "lit" else t[1] for t in blk.tokens) == n, n
        assert _matches(blk), n


def test_matches_at_the_window_edge_from_tokens(corpus):
    at = [t for t in _matches(corpus[("mark32768", 65536)][2]) if t[2] == 32768]
    assert at and max(t[1] for t in at) >= 190  # the 200-byte marker's repeat
    assert [t for t in _matches(corpus[("mark32769", 65536)][2]) if t[2] >= 32768] == []
    for (kind, n), (_, _, blk, _) in corpus.items():
        if blk is not None:
            assert all(3 <= t[1] <= 258 and 1 <= t[2] <= 32768 for t in _matches(blk)), (kind, n)


def test_full_token_slot_after_matches(crafted):
    blk = crafted["full_slot"][2]
    slots, before, after = 0, 0, []
    for t in blk.tokens:
        if slots >= TOKEN_SLOT:
            after.append(t)
        else:
            before += t[0] == "match"
        slots += 1 if t[0] == "lit" else 2
    assert slots > TOKEN_SLOT and before >= 100, (slots, before)   # witness: the slot filled, after matches
    assert len(after) > 600 and all(t[0] == "lit" for t in after)  # the marker's repeat included


def test_output_placement_at_every_offset_in_a_line(B, dev, oracle):
    chunks = [I.two_symbol(7, 700), oracle.textgen_chunk(311, 30)]
    caps = [B.deflate_max_compressed_length(len(c)) for c in chunks]
    offs, cur = [], 0
    for k in range(256):
        cur += 128                                # a guard
        cur += (k % 128 - cur) % 128              # then the slot, at k % 128 within its line
        offs.append(cur)
        cur += caps[k // 128]
    total = cur + 128
    inp, off, ln = B.pack([chunks[k // 128] for k in range(256)], dev)
    out = torch.full((total,), 0xA5, dtype=torch.uint8, device=dev)
    ooff = torch.tensor(offs, dtype=torch.int64, device=dev)
    olen, st = B.deflate_encode(inp, off, ln, out, ooff, level=6)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0] * 256
    assert sorted({o % 128 for o in offs[:128]}) == list(range(128)) == sorted({o % 128 for o in offs[128:]})
    h, ol = out.cpu().numpy().tobytes(), olen.cpu().tolist()
    outs = [h[o:o + w] for o, w in zip(offs, ol)]
    for j, chunk in enumerate(chunks):
        blk, _ = _check_chunk(chunk, outs[128 * j], j)
        assert all(o == outs[128 * j] for o in outs[128 * j:128 * j + 128]), j
        assert j == 1 or blk.btype == 2
    assert len(outs[128]) < 128
    # the guards on both sides of every slot, and the unused rest of every slot
    end = 0
    for o, w in zip(offs, ol):
        assert o - end >= 128 and h[end:o] == b"\xa5" * (o - end), o
        end = o + w
    assert total - end >= 128 and h[end:] == b"\xa5" * (total - end)


def test_stamp_wrap_over_many_calls(B, dev):
    """One stamp per sub-batch and 65 534 stamps between two zeroings of the tables, so 65 600 calls
    pass the wrap once wherever the stamp stood.  Call 0 plants entries (the planter of
    deflate_inputs.stamp_plant), the calls after it alternate the two inputs of stamp_pair in both
    table slots, and call 65 534, which has call 0's stamp again if the counter restarts, encodes the
    victim: an entry that outlived the wrap is a match whose first four bytes were never compared.
    Every 1024th call and the 200 calls around 65 534 are checked: each output inflates to its input
    and equals the first output for the same input.  Measured on the MI355X: 14.9 s for the 65 600
    calls (some 230 us a call, host-bound); the design has no cheaper route to the wrap."""
    from netty_amd import JdkZlibEncoder
    a, b = I.stamp_pair(1)
    c, v = I.stamp_plant(1)
    batches = {"ab": [a, b], "ba": [b, a], "plant": [c, c], "victim": [v, v]}
    packed = {k: B.pack(x, dev) for k, x in batches.items()}
    cap = B.deflate_max_compressed_length(200)
    out, ooff = B.out_slots([cap, cap], dev)
    oo = ooff.cpu().tolist()
    holder = JdkZlibEncoder()  # holds the deflate workspace, and with it the stamp, for the duration
    first = {}
    calls = 65600
    t0 = time.perf_counter()
    try:
        for i in range(calls):
            k = "plant" if i == 0 else "victim" if i in (65534, calls - 1) else "ab" if i % 2 else "ba"
            inp, off, ln = packed[k]
            olen, st = B.deflate_encode(inp, off, ln, out, ooff, level=6)
            if i % 1024 and abs(i - 65534) > 100 and i != calls - 1:
                continue
            h, ol = out.cpu().numpy().tobytes(), olen.cpu().tolist()
            assert st.cpu().tolist() == [0, 0], i
            got = [h[o:o + w] for o, w in zip(oo, ol)]
            for chunk, g in zip(batches[k], got):
                _check_block_run(chunk, g, (i, k))
            assert first.setdefault(k, got) == got, (i, k)
        torch.cuda.synchronize()
    finally:
        holder.close()
    print(f"deflate stamp wrap: {calls} calls in {time.perf_counter() - t0:.1f} s")
    assert set(first) == set(batches)


def test_handler_message_is_slices_of_block_runs(oracle):
    from netty_amd import JdkZlibEncoder, ZlibWrapper
    msg = oracle.textgen_chunk(79, 150000) + bytes(20000) + random.Random(9).randbytes(30000)
    enc = JdkZlibEncoder(ZlibWrapper.GZIP, 6)
    wire = enc.encode(msg) + enc.finish_encode()
    enc.close()
    assert zlib.decompress(wire, 31) == msg
    blocks = D.read_blocks(wire[10:-8])
    assert D.replay(blocks) == msg and (blocks[-1].end + 7) // 8 == len(wire) - 18
    closing = blocks.pop()
    assert closing.bfinal == 1 and closing.btype == 1 and closing.tokens == [] and closing.bits == 10
    assert wire[-10:-8] == b"\x03\x00" and closing.start == 8 * (len(wire) - 20)
    assert not any(b.bfinal for b in blocks)
    # the empty stored block closes each slice; a slice's run stands alone (no distance reaches the
    # slice before it) and has the shape of a chunk's output
    ends = [blk.end // 8 for blk in blocks if blk.btype == 0 and blk.len == 0]
    assert len(ends) == 4 and ends[-1] == blocks[-1].end // 8
    kinds = []
    for i, (lo, hi) in enumerate(zip([0] + ends, ends)):
        blk, _ = _check_chunk(msg[65536 * i:65536 * (i + 1)], wire[10 + lo:10 + hi], ("slice", i))
        kinds.append(None if blk is None else blk.btype)
    assert kinds == [2, 2, 2, None]  # text, text, text then zeros then random, 3392 random bytes
