"""GPU tests of the deflate encoder's history prefix (nx_deflate_encode_batch_ex).  The checker is the
machine's zlib: a chunk's output inflates to the chunk with the prefix as preset dictionary, and its tokens
are read from stored_block(prefix) + output (tests/deflate_prefix_inputs.py, pinned on the CPU by
tests/test_deflate_prefix_inputs.py)."""
import random
import zlib

import pytest

import deflate_prefix_inputs as P

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GUARD = 0xA5
INVALID_ARG = -100


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def B():
    from netty_amd import batch
    return batch


def _encode(B, dev, cases, level=6, prefix_lens=None, offs=None, arena=None, no_prefix=False):
    """one launch over (prefix, chunk) cases, each prefix right in front of its chunk in the arena (or the
    given arena / offsets / prefix lengths); returns (outputs, statuses) after checking the guard bytes
    around every output slot"""
    if arena is None:
        buf, offs = bytearray(), []
        for prefix, chunk in cases:
            buf += bytes(-len(buf) % 16 + len(buf) % 3)  # three alignments
            buf += prefix
            offs.append(len(buf))
            buf += chunk
        arena = bytes(buf) + bytes(16)
    if prefix_lens is None:
        prefix_lens = [len(p) for p, _ in cases]
    inp = torch.frombuffer(bytearray(arena), dtype=torch.uint8).to(dev)
    off = torch.tensor(offs, dtype=torch.int64, device=dev)
    ln = torch.tensor([len(c) for _, c in cases], dtype=torch.int32, device=dev)
    pl = None if no_prefix else torch.tensor(prefix_lens, dtype=torch.int32, device=dev)
    caps = [B.deflate_max_compressed_length(len(c)) for _, c in cases]
    slots = [16 + cap + 16 for cap in caps]  # guard bytes before and after
    out, ooff = B.out_slots(slots, dev, align=1)
    out.fill_(GUARD)
    olen, st = B.deflate_encode(inp, off, ln, out, ooff + 16, level=level, prefix_len=pl)
    torch.cuda.synchronize()
    outh, oo, ol = out.cpu().numpy().tobytes(), ooff.cpu().tolist(), olen.cpu().tolist()
    res = []
    for o, w, cap in zip(oo, ol, caps):
        assert 0 <= w <= cap, (w, cap)
        assert outh[o:o + 16] == bytes([GUARD]) * 16
        assert outh[o + 16 + w:o + 32 + cap] == bytes([GUARD]) * (cap - w + 16)
        res.append(outh[o + 16:o + 16 + w])
    return res, st.cpu().tolist()


def _check(prefix, chunk, out, what):
    assert P.inflate_with(prefix, out) == chunk, what
    assert out[-4:] == b"\0\0\xff\xff", what


@pytest.mark.parametrize("level", [0, 1, 6])
def test_no_prefix_is_the_plain_entry_point(B, dev, level):
    cases = [(b"", c) for c in P.mixed_chunks()]
    assert len(cases) == 32
    plain, st0 = _encode(B, dev, cases, level=level, no_prefix=True)
    zeros, st1 = _encode(B, dev, cases, level=level)
    assert st0 == st1 == [0] * 32
    assert zeros == plain
    for (_, c), o in zip(cases, plain):
        assert (o == b"") if not c else (zlib.decompressobj(-15).decompress(o) == c)


@pytest.fixture(scope="module")
def round_trips(B, dev):
    cases = P.round_trip_cases()
    outs, st = _encode(B, dev, cases)
    return cases, outs, st


def test_round_trips(round_trips):
    cases, outs, st = round_trips
    assert st == [0] * len(cases)
    assert {len(p) for p, _ in cases} == set(P.PREFIX_LENS)
    for (prefix, chunk), out in zip(cases, outs):
        _check(prefix, chunk, out, (len(prefix), len(chunk)))


def test_prefix_is_matched_not_emitted(round_trips):
    """a text chunk with 32 KiB of the same text before it: the output inflates to the chunk alone, and the
    zero chunks behind a zero prefix open with a match into it"""
    cases, outs, _ = round_trips
    for (prefix, chunk), out in zip(cases, outs):
        if prefix and not any(prefix) and len(chunk) >= 4:
            assert P.chunk_tokens(prefix, out)[0][0] == "match", (len(prefix), len(chunk))


def test_fuzz(B, dev):
    cases = P.fuzz_cases()
    outs, st = _encode(B, dev, cases)
    assert st == [0] * len(cases)
    for i, ((prefix, chunk), out) in enumerate(zip(cases, outs)):
        _check(prefix, chunk, out, i)
    # the prefixes are used: fewer bytes than the same chunks without them
    bare, _ = _encode(B, dev, cases, prefix_lens=[0] * len(cases))
    assert sum(map(len, outs)) < sum(map(len, bare))


def test_level_zero_ignores_the_prefix(B, dev):
    cases = [c for c in P.round_trip_cases() if len(c[1]) <= 259]
    outs, st = _encode(B, dev, cases, level=0)
    assert st == [0] * len(cases)
    for (prefix, chunk), out in zip(cases, outs):
        assert len(out) == B.deflate_max_compressed_length(len(chunk))
        assert zlib.decompressobj(-15).decompress(out) == chunk


def test_empty_chunk_with_a_prefix_writes_nothing(B, dev):
    cases = [(b"abcdefgh" * 4, b""), (b"abcdefgh" * 4, b"abcdefgh"), (b"x", b"")]
    outs, st = _encode(B, dev, cases)
    assert st == [0, 0, 0] and outs[0] == b"" and outs[2] == b""
    _check(*cases[1], outs[1], "neighbour")


# ------------------------------------------------------------------------------ reach
@pytest.fixture(scope="module")
def reach(B, dev):
    cases = P.reach_cases()
    outs, st = _encode(B, dev, [(p, c) for p, c, _ in cases.values()])
    assert st == [0] * len(cases)
    return {name: (p, c, want, P.chunk_tokens(p, o), o) for (name, (p, c, want)), o in zip(cases.items(), outs)}


@pytest.mark.parametrize("name", ["dist32768", "boundary", "dist1", "dist1_len1"])
def test_reach_first_token(reach, name):
    prefix, chunk, want, toks, out = reach[name]
    _check(prefix, chunk, out, name)
    assert toks[0] == want[1], name


def test_reach_never_beyond_the_window(reach):
    prefix, chunk, want, toks, out = reach["dist32769"]
    _check(prefix, chunk, out, "dist32769")  # zlib refuses a distance of 32769
    assert toks[:want[2]] == [("lit", b) for b in chunk[:want[2]]]
    assert all(t[0] == "lit" or t[2] <= P.MAX_DIST for t in toks)


def test_copy_of_a_slot_clean_prefix_is_matches_only(reach):
    prefix, chunk, _, toks, out = reach["copy"]
    _check(prefix, chunk, out, "copy")
    assert toks and all(t[0] == "match" for t in toks)
    assert all(t[2] == len(prefix) for t in toks) and sum(t[1] for t in toks) == len(chunk)


# ------------------------------------------------------------------------------ isolation
def test_chunks_never_see_each_others_prefix(B, dev):
    """two chunks with the same bytes, one behind its own copy and one behind other bytes: the second finds
    nothing of the first's prefix (its tokens are those of the chunk encoded alone)"""
    clean, other = P.slot_clean(1024, 77), P.slot_clean(1024, 78)
    outs, st = _encode(B, dev, [(clean, clean), (other, clean), (b"", clean)])
    assert st == [0, 0, 0]
    for prefix, out in zip((clean, other, b""), outs):
        _check(prefix, clean, out, "isolation")
    assert all(t[0] == "match" for t in P.chunk_tokens(clean, outs[0]))
    assert all(clean[i:i + 4] not in other + clean[:i + 3] for i in range(len(clean) - 3))  # nothing to find elsewhere
    assert P.chunk_tokens(other, outs[1]) == P.chunk_tokens(b"", outs[2]) == [("lit", b) for b in clean]


def test_sub_batches_do_not_leak_prefix_entries(B, dev):
    """more chunks than one launch has slots for (as test_gpu_deflate.py::test_sub_batches_reuse_slots forces
    it): a slot's later chunk has no prefix and the same bytes as the earlier chunk's prefix; an entry left
    over from that prefix would give a distance before the chunk's start, which zlib refuses"""
    rng = random.Random(6)
    n = 256 * 16 * 2 + 37
    bodies = [bytes(rng.choice(b"abc") for _ in range(40 + i % 23)) for i in range(n)]
    cases = [(bodies[(i * 7) % n][:32], bodies[i]) if i % 2 == 0 else (b"", bodies[i]) for i in range(n)]
    outs, st = _encode(B, dev, cases)
    assert st == [0] * n
    for i, ((prefix, chunk), out) in enumerate(zip(cases, outs)):
        _check(prefix, chunk, out, i)


# ------------------------------------------------------------------------------ limits
def test_limits_fail_alone(B, dev):
    rng = random.Random(8)
    big = bytes(rng.choice(b"abcd") for _ in range(32769 + 65536))
    good = b"neighbour " * 30
    arena = good + big + good + bytes(16)
    a = len(good)
    # (offset, length, prefix_len)
    rows = [(0, len(good), 0),
            (a + 32769, 100, 32769),                       # prefix over the window
            (a + 32768, 100, 32768),                       # the largest prefix: fine
            (a + 32768, 65536 - 32768 + 1, 32768),         # prefix + length = 65537
            (a + 1000, 64536, 1000),                       # prefix + length = 65536: fine
            (5, 20, 6),                                    # prefix_len > in_off
            (a + len(big), len(good), len(good))]          # a neighbour with a prefix
    cases = [(arena[o - min(p, o):o], arena[o:o + n]) for o, n, p in rows]
    for level in (6, 0):
        outs, st = _encode(B, dev, cases, level=level, arena=arena, offs=[r[0] for r in rows], prefix_lens=[r[2] for r in rows])
        assert st == [0, INVALID_ARG, 0, INVALID_ARG, 0, INVALID_ARG, 0], level
        for i in (1, 3, 5):
            assert outs[i] == b""
        for i in (0, 2, 4, 6):
            o, n, p = rows[i]
            _check(arena[o - p:o] if level else b"", arena[o:o + n], outs[i], (level, i))


# ------------------------------------------------------------------------------ independence and size
def test_stream_cut_into_prefixed_chunks(B, dev):
    stream = P.repeated_stream()
    cuts = P.stream_chunks(stream)
    cases = [(stream[o - p:o], stream[o:o + n]) for o, n, p in cuts]
    outs, st = _encode(B, dev, cases, arena=stream + bytes(16), offs=[c[0] for c in cuts], prefix_lens=[c[2] for c in cuts])
    assert st == [0] * len(cuts)
    d = zlib.decompressobj(-15)
    assert d.decompress(b"".join(outs) + b"\x03\x00") == stream and d.eof
    bare, st = _encode(B, dev, cases, arena=stream + bytes(16), offs=[c[0] for c in cuts], prefix_lens=[0] * len(cuts))
    assert st == [0] * len(cuts)
    print(f"prefixed {sum(map(len, outs))} bytes, without {sum(map(len, bare))}")
    assert sum(map(len, outs)) < sum(map(len, bare))
