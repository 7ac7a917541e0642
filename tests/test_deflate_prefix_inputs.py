"""The inputs and yardsticks of the history-prefix and preset-dictionary tests (tests/
deflate_prefix_inputs.py), pinned on the machine's zlib.  No GPU and none of the project's code."""
import zlib

import pytest

import deflate_prefix_inputs as P
from deflate_blocks import read_blocks


def _zlib_chunk(chunk, prefix, level=1):
    z = zlib.compressobj(level, zlib.DEFLATED, -15, zdict=prefix) if prefix else zlib.compressobj(level, zlib.DEFLATED, -15)
    return z.compress(chunk) + z.flush(zlib.Z_SYNC_FLUSH)


def test_stored_block_plus_chunk_reads_as_prefix_plus_chunk():
    """the reading the token assertions rest on: zlib inflates stored_block(prefix) + (a chunk deflated with
    that prefix as dictionary) to prefix + chunk, and the block reader sees the chunk's tokens with distances
    that reach into the prefix"""
    for prefix, chunk in P.round_trip_cases()[::7] + P.fuzz_cases(40):
        out = _zlib_chunk(chunk, prefix, 6)
        d = zlib.decompressobj(-15)
        assert d.decompress(P.stored_block(prefix) + out) == prefix + chunk
        assert P.inflate_with(prefix, out) == chunk
        toks = P.chunk_tokens(prefix, out)
        assert sum(1 if t[0] == "lit" else t[1] for t in toks) == len(chunk)
    prefix = P.RUN * 3
    toks = P.chunk_tokens(prefix, _zlib_chunk(P.RUN, prefix, 6))
    assert toks == [("match", len(P.RUN), len(P.RUN))]  # a distance that only the stored block satisfies
    assert len(read_blocks(P.stored_block(bytes(32768)) + b"\x03\x00")) == 2  # the longest prefix is one block


def test_slot_function_and_clean_bytes():
    assert P.slot(bytes(4)) == 0 and P.slot(b"\x01\0\0\0") == 2654435761 >> 20
    for n, seed in ((1024, 77), (2048, 9)):
        d = P.slot_clean(n, seed)
        assert len(d) == n and d == P.slot_clean(n, seed)  # seeded
        flat = d + d[:3]
        slots = [P.slot(flat[q:q + 4]) for q in range(n)]
        assert len(set(slots)) == n  # no two words share a slot, the three that wrap included


def test_reach_cases_keep_their_slots():
    for name, (flat, src, probe) in P.reach_sources().items():
        assert flat[src:src + 4] == flat[probe:probe + 4], name
        assert P.slot_kept(flat, src, probe), name
    cases = P.reach_cases()
    prefix, chunk, _ = cases["dist32768"]
    assert len(prefix) == 32768 and chunk.startswith(prefix[:40]) and len(set(P.RUN)) == len(P.RUN)
    prefix, chunk, _ = cases["dist32769"]
    assert (prefix + chunk).find(P.RUN, 1) == 32769  # the only earlier copy is one byte out of reach
    prefix, chunk, _ = cases["copy"]
    assert prefix == chunk and len(prefix) == 1024
    for name, (prefix, chunk, _) in cases.items():  # zlib agrees that every case is encodable with its prefix
        assert P.inflate_with(prefix, _zlib_chunk(chunk, prefix)) == chunk, name


def test_zlib_shows_the_same_reach():
    """zlib itself, given the prefix as dictionary, opens the chunk with a match into it (it enters no
    dictionary shorter than its minimum match, so the 1-byte prefix is not asked of it), and its distances
    never pass 32768"""
    cases = P.reach_cases()
    for name in ("boundary", "dist1"):
        prefix, chunk, want = cases[name]
        assert P.chunk_tokens(prefix, _zlib_chunk(chunk, prefix, 6))[0][0] == "match", name
    prefix, chunk, _ = cases["dist32769"]
    toks = P.chunk_tokens(prefix, _zlib_chunk(chunk, prefix, 9))
    assert all(t[0] == "lit" or t[2] <= P.MAX_DIST for t in toks)


@pytest.mark.parametrize("level", [0, 1, 6, 9, -1])
def test_header_expectations(level):
    """what the encoder handle's first bytes are compared with: FDICT and DICTID for every non-empty
    dictionary, the plain header for the empty one"""
    plain = P.zlib_header(level, None)
    assert len(plain) == 2 and plain[0] == 0x78 and int.from_bytes(plain, "big") % 31 == 0 and not plain[1] & 0x20
    for n in P.DICT_LENS:
        d = P.dictionary(n)
        h = P.zlib_header(level, d)
        if n == 0:
            assert h == plain
            continue
        assert len(h) == 6 and h[0] == 0x78 and h[1] & 0x20 and int.from_bytes(h[:2], "big") % 31 == 0
        assert h[1] & 0xC0 == plain[1] & 0xC0
        assert h[2:] == zlib.adler32(d).to_bytes(4, "big")  # of the whole dictionary, beyond 32 KiB too
    far, msg = P.far_dictionary()
    assert len(far) == 40000 and far.find(msg) + len(msg) < 40000 - 32768


def test_size_directions():
    """zlib level 1 shows the direction the GPU tests assert: prefixes make the repeated stream smaller, and a
    dictionary makes a message drawn from it smaller"""
    stream = P.repeated_stream()
    cuts = P.stream_chunks(stream)
    assert [c[2] for c in cuts] == [0, 32768]
    with_prefix = sum(len(_zlib_chunk(stream[o:o + n], stream[o - p:o])) for o, n, p in cuts)
    without = sum(len(_zlib_chunk(stream[o:o + n], b"")) for o, n, p in cuts)
    assert with_prefix < without
    d = P.slot_clean(2048, 9)
    z = zlib.compressobj(1, zdict=d)
    assert len(z.compress(d) + z.flush()) < len(zlib.compress(d, 1))


def test_fuzz_is_seeded_and_shares_substrings():
    a, b = P.fuzz_cases(), P.fuzz_cases()
    assert a == b and len(a) == 200
    for prefix, chunk in a:
        assert prefix and chunk[:min(4, len(prefix))] in prefix  # every chunk opens with bytes of its prefix
    assert sum(len(p) >= 4 for p, _ in a) > 100
    assert all(1 <= len(c) and len(p) + len(c) <= P.MAX_CHUNK for p, c in a)
