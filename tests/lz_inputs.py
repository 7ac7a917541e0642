"""Seeded inputs that aim the four LZ encoders (FastLZ level 1/2, LZF, LZ4 fast, Snappy) at their
boundary paths.  Pure Python: the same seed gives the same bytes (tests/test_lz_inputs.py), and no
oracle or kernel is used to build them.

The unit is `repeat`: a short random head, a source of `length` bytes, a gap, then a copy of the source
`dist` bytes after it and fresh bytes whose first one breaks the match.  The encoders keep the latest
position per hash slot, so the copy is found only if nothing between the source and the copy lands in
the source's slot and the source's first bytes occur nowhere else; `repeat` restates each codec's hash
to check both and draws again until they hold.  Long gaps are a run of one byte: an encoder codes it
as a few long matches and enters almost none of its positions, so a far source survives (and Snappy's
and LZ4's growing search step is reset right before the copy).

A family is a function of a seed that returns Cases: the bytes, and what the encoder's tokens must
show for the family to have reached its path (`want` tokens starting at position `at`, `lits`
positions that must stay literals).  tests/test_lz_inputs.py asserts that on the oracle's output;
tests/test_gpu_alt_encode_edges.py runs the bytes through the kernels."""
import random
from collections import namedtuple

CODECS = ("fastlz1", "fastlz2", "lzf", "lz4", "snappy")

# data: the chunk.  want: tokens (lz_tokens form without the form field; None is a wildcard) that must
# follow one another, the first starting at output position `at` (None: anywhere).  lits: positions no
# match may cover; no further match at want's distance follows the wanted ones.  only: `want` holds every
# match of the chunk (so the literals before and after it are counted exactly).  end: the output position
# at which the chunk's last match must end.
Case = namedtuple("Case", "data at want lits only end", defaults=(None, (), (), False, None))

_WORDS = [b"netty", b"channel", b"buffer", b"handler", b"codec", b"the", b"of", b"pipeline", b"event", b"loop",
          b"write", b"read", b"flush", b"byte", b"frame", b"and", b"to", b"in", b"compression", b"stream"]


def text(rng, n):
    out = bytearray()
    while len(out) < n:
        out += rng.choice(_WORDS) + rng.choice([b" ", b" ", b", ", b".\n", b"-"])
    return bytes(out[:n])


def quad(rng, n, base=b"acgt"):
    """n bytes of a 4-symbol alphabet: full of short matches"""
    return bytes(base[b & 3] for b in rng.randbytes(n))


def filler(seed):
    """a small chunk unlike every other seed's: 60..70 bytes of a 4-symbol alphabet"""
    rng = random.Random(0xF111E5 + seed)
    return quad(rng, rng.randrange(60, 71))


# ---- the encoders' hash slots, restated (to keep a source's slot free, not to predict output) ----
def _i32(x):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >= 1 << 31 else x


def _slot_fastlz(d, o, n):
    def u16(i):
        return d[i] if i + 1 >= n else d[i] | (d[i + 1] << 8)
    v = u16(o)
    return (v ^ u16(o + 1) ^ (v >> 3)) & 8191


def _slot_lzf(d, o, n):
    return (_i32(int.from_bytes(d[o:o + 3], "big") * 57321) >> 9) & 16383


def _slot_lz4(d, o, n):
    if n >= 65547:  # byU32: LZ4_hash5
        return (((int.from_bytes(d[o:o + 8], "little") << 24) & (2**64 - 1)) * 889523592379 & (2**64 - 1)) >> 52
    return ((int.from_bytes(d[o:o + 4], "little") * 2654435761) & 0xFFFFFFFF) >> 19


def _slot_snappy(d, o, n):
    hts = 1
    while hts < n and hts < 16384:
        hts <<= 1
    return ((int.from_bytes(d[o:o + 4], "big") * 0x1E35A7BD) & 0xFFFFFFFF) >> (32 - hts.bit_length() + 1)


# per codec: hash function and the bytes it hashes (LZF's rolling value holds the byte BEFORE the position
# too, but its hash keeps bits 9..22 of the product, which that byte does not reach)
_MATCHER = {"fastlz1": (_slot_fastlz, 3), "fastlz2": (_slot_fastlz, 3), "lzf": (_slot_lzf, 3),
            "lz4": (_slot_lz4, 4), "snappy": (_slot_snappy, 4)}

# bytes before the chunk's end at which a match that could go on must stop: FastLZ's ipBound (n - 2, and
# the last compared byte is not coded), LZF's `inEnd - ip + 2` cap on the length (inEnd = n - 4), LZ4's
# LASTLITERALS; Snappy matches to the last byte
END_MARGIN = {"fastlz1": 3, "fastlz2": 3, "lzf": 2, "lz4": 5, "snappy": 0}


def _source(rng, length):
    """`length` bytes an encoder enters few positions of when long: 16 random bytes, then a period
    of 251"""
    if length <= 600:
        return rng.randbytes(length)
    per = rng.randbytes(251)
    return rng.randbytes(16) + (per * (length // 251 + 1))[:length - 16]


def _gap(rng, g, random_gap):
    if g <= 200 or random_gap:
        return rng.randbytes(g)
    r1, r2 = rng.randbytes(4), rng.randbytes(4)
    if g > 20000:  # a far source: some text first, so that the chunk is not one run alone
        r1 += text(rng, 3000)
    x = next(b for b in range(256) if b not in (r1[-1], r2[0]))
    return r1 + bytes([x]) * (g - len(r1) - 4) + r2


def _unique_before(d, pos, width):
    """the `width` bytes at pos occur nowhere before pos"""
    return d.find(d[pos:pos + width], 0, pos + width - 1) < 0


def repeat(rng, codec, length, dist, head=6, tail=20, random_gap=False):
    """head + source + gap + copy + tail, the copy `dist` after the source.  Returns (bytes,
    position of the copy).  dist < length gives an overlapping match on data of period dist."""
    slot, width = _MATCHER[codec]
    for _ in range(400):
        d = bytearray(rng.randbytes(head))
        src = len(d)
        if dist >= length:
            s = _source(rng, length)
            d += s + _gap(rng, dist - length, random_gap) + s
        else:
            per = rng.randbytes(dist)
            d += per + (per * (length // dist + 1))[:length]
        p = src + dist
        t = bytearray(rng.randbytes(tail))
        if t and t[0] == d[src + length]:
            t[0] ^= 0x55
        d += t
        if src and d[src - 1] == d[p - 1]:
            continue
        total = len(d)
        # the first bytes of the source and of the copy (and of the positions just before them, where
        # a match would swallow the anchor) occur nowhere earlier
        if not all(_unique_before(d, q, width) for q in range(max(src - width + 1, 0), src + 1)):
            continue
        if d.find(d[p:p + width], 0, p + width - 1) != src:
            continue
        if any(d.find(d[q:q + width], 0, q + width - 1) >= 0 for q in range(p - width + 1, p)):
            continue
        want = slot(d, src, total)
        if any(slot(d, q, total) == want for q in range(src + 1, p) if q + 8 <= total):
            continue
        return bytes(d), p
    raise AssertionError(f"{codec}: no draw with a free slot for length {length} at {dist}")


def _m(length, dist):
    return ("match", length, dist)


def _hit(rng, codec, length, dist, want=None, only=False, **kw):
    """a Case whose chunk holds one repeat, found as `want` (default: one match of length at dist)"""
    d, at = repeat(rng, codec, length, dist, **kw)
    return Case(d, at, [_m(length, dist)] if want is None else want, (), only)


def _miss(rng, codec, length, dist, **kw):
    """a Case whose repeat must NOT be taken: its first position stays a literal"""
    d, at = repeat(rng, codec, length, dist, **kw)
    return Case(d, None, [], (at,), False)


# ---- families for every codec ----
SWEEP = list(range(0, 41)) + list(range(59, 69))


def short_lengths(seed, codec):
    """Every length 0..40 and 59..68 as text, random bytes and zeros: the encoders' minimum lengths
    (FastLZ 4 and 13, LZF 16, LZ4 13, Snappy 15) and the first literal-run splits."""
    rng = random.Random(seed)
    return [Case(f(n)) for n in SWEEP for f in (lambda n: text(rng, n), rng.randbytes, bytes)]


def match_to_end(seed, codec):
    """A copy that runs to the last byte, 70 bytes after its source, in chunks of 116, 117, .. 140 bytes:
    the end of the match moves through every position of the word / byte hand-over, and the match
    stops where the encoder's end margin stops it (END_MARGIN: FastLZ's ipBound, LZF's
    `inEnd - ip + 2` cap on the match length, LZ4's last 5 literals, Snappy's last byte)."""
    rng = random.Random(seed)
    out = []
    for j in range(25):
        d, _ = repeat(rng, codec, 40 + j, 70, tail=0)
        out.append(Case(d, None, [("match", None, 70)], end=len(d) - END_MARGIN[codec]))
    return out


def mismatch_near_end(seed, codec):
    """The same with the match broken 0..16 bytes before the end of the chunk."""
    rng = random.Random(seed)
    out = []
    for k in range(17):
        d, _ = repeat(rng, codec, 40, 70, tail=k)
        out.append(Case(d, None, [("match", None, 70)]))
    return out


def periodic(seed, codec):
    """Periods 1, 2, 3, 4, 7 and 8 (overlapping matches, FastLZ's run shortcut), 300 and 2000 bytes."""
    rng = random.Random(seed)
    out = []
    for per in (1, 2, 3, 4, 7, 8):
        unit = bytes(rng.sample(range(256), per))
        for n in (300, 2000):
            out.append(Case(rng.randbytes(5) + (unit * (n // per + 1))[:n] + rng.randbytes(17), None, [("match", None, per)]))
    return out


COMMON = {"short_lengths": short_lengths, "match_to_end": match_to_end, "mismatch_near_end": mismatch_near_end,
          "periodic": periodic}


# ---- FastLZ ----
FLZ_FAR = 8191  # real distances from here take 5 equal bytes at level 2, from 8192 the far form


def _flz_split(length):
    """the tokens of a level-1 match: 262-byte pieces while more than 264 bytes are left"""
    b, out = length - 2, []
    while b > 262:
        out.append(262)
        b -= 262
    return out + [b + 2]


def flz_distances(seed, codec):
    """Distances 1, 2, 255..257 and 8189..8193: level 1 takes a candidate up to 8190 back and none
    beyond; level 2 codes up to 8191 in the near form and 8192 on in the far form (8447: far bytes
    0, 255), up to 65000."""
    rng = random.Random(seed)
    out = []
    for dist in (1, 2, 255, 256, 257, 8189, 8190, 8191, 8192, 8193):
        if codec == "fastlz1" and dist >= FLZ_FAR:
            out.append(_miss(rng, codec, 20, dist))
        else:
            out.append(_hit(rng, codec, 20, dist))
    if codec == "fastlz2":
        out += [_hit(rng, codec, 20, dist) for dist in (8446, 8447, 16383, 40000, 65000)]
    return out


def flz_lengths(seed, codec):
    """Lengths 3..10 at distance 300; at level 2 also 9000 back, where 3 and 4 equal bytes are not
    enough (the 4th or 5th byte differs: a literal) and 5 are."""
    rng = random.Random(seed)
    out = [_hit(rng, codec, n, 300) for n in range(3, 11)]
    if codec == "fastlz2":
        out += [_miss(rng, codec, n, 9000) for n in (3, 4)]
        out += [_hit(rng, codec, n, 9000) for n in range(5, 11)]
    return out


def flz_long(seed, codec):
    """Level 1: 264, 265, 266, 526, 527 and 1000 bytes, which the 262-byte splitting loop leaves
    with remainders 0, 1 and 2.  Level 2: 9, 10, 263, 264, 265 and 519 bytes (no, one and two 255
    length bytes, each with remainder 0 on one side) and 20 000."""
    rng = random.Random(seed)
    if codec == "fastlz1":
        return [_hit(rng, codec, n, n + 300, want=[_m(k, n + 300) for k in _flz_split(n)])
                for n in (264, 265, 266, 526, 527, 1000)]
    return [_hit(rng, codec, n, n + 300) for n in (9, 10, 263, 264, 265, 519, 20000)]


def flz_runs(seed, codec):
    """Runs of one byte ending 0..12 bytes before the chunk's end and of 30..39 bytes: the level-2 run
    shortcut's word loop, its byte loop near the end, and ipBound."""
    rng = random.Random(seed)
    out = []
    for k in range(13):
        out.append(Case(rng.randbytes(5) + b"r" * 60 + bytes(rng.randrange(97) for _ in range(k)), None, [("match", None, 1)]))
    for m in range(30, 40):
        out.append(Case(rng.randbytes(5) + b"q" * m + rng.randbytes(20), None, [("match", None, 1)]))
    return out


def flz_position0(seed, codec):
    """A repeat of the chunk's first bytes: the candidate is position 0, which is also what an unwritten
    slot reads as (distance == anchor)."""
    rng = random.Random(seed)
    return [_hit(rng, codec, n, dist, head=0) for n, dist in ((8, 30), (12, 200), (5, 8189))]


def flz_u16(seed, codec):
    """Chunks for the readU16 quirk's limits (len, len - 1, len // 2, 1, 0): the hash of every
    position at and after the limit reads single bytes."""
    rng = random.Random(seed)
    return [Case(text(rng, 700)), Case(quad(rng, 300)), Case(rng.randbytes(100)), Case(bytes(50)),
            Case(repeat(rng, codec, 30, 200)[0]), Case(quad(rng, 64) * 5), Case(text(rng, 13)), Case(text(rng, 12))]


def flz_literal_runs(seed, codec):
    """Exactly 31, 32, 33, 64 and 65 literals before a match and after the last one: the run header
    written when a run fills (copy == MAX_COPY) and taken back when no literal follows (op--)."""
    rng = random.Random(seed)
    out = []
    for k in (31, 32, 33, 64, 65):
        out.append(_hit(rng, codec, 5, k - 6, random_gap=True, only=True))            # the match starts at k
        out.append(_hit(rng, codec, 5, 40, tail=k, random_gap=True, only=True))       # k literals close the chunk
    return out


FASTLZ = {"flz_distances": flz_distances, "flz_lengths": flz_lengths, "flz_long": flz_long, "flz_runs": flz_runs,
          "flz_position0": flz_position0, "flz_u16": flz_u16, "flz_literal_runs": flz_literal_runs}


def fastlz_limits(n):
    """the u16_limit values of the readU16 quirk for a chunk of n bytes"""
    return [n, n - 1, n // 2, 1, 0]


# ---- LZF ----
def lzf_offsets(seed, codec):
    """Offsets 1, 256, 257, 8191 and 8192 (MAX_OFF, inclusive) match; 8193 does not."""
    rng = random.Random(seed)
    return [_hit(rng, codec, 20, d) for d in (1, 256, 257, 8191, 8192)] + [_miss(rng, codec, 20, 8193)]


def lzf_lengths(seed, codec):
    """Lengths 3, 8 and 9 (the short / long token split at len - 2 < 7), 10, 263 and 264 (MAX_REF); 265
    and 600, which the cap cuts into chained matches of 264."""
    rng = random.Random(seed)
    out = [_hit(rng, codec, n, n + 300) for n in (3, 8, 9, 10, 263, 264)]
    out.append(_hit(rng, codec, 265, 565, want=[_m(264, 565)]))
    out.append(_hit(rng, codec, 600, 900, want=[_m(264, 900), _m(264, 900), _m(72, 900)]))
    return out


def lzf_chunk_sizes(seed, codec):
    """15, 16 and 17 bytes (encode_chunk compresses from 16), compressible and not."""
    rng = random.Random(seed)
    return [Case(f(n)) for n in (15, 16, 17) for f in (bytes, rng.randbytes, lambda n: (b"abc" * 6)[:n])]


# (seed, n) found on the CPU with the restated encoder: bodies of n - 3, n - 2 and n - 1 bytes, on
# each side of `clen + 7 < n + 5` (the first is kept, the other two fall back to a raw chunk)
LZF_THRESHOLD = ((3, 24), (11, 24), (0, 24), (5, 40), (0, 40), (7, 40), (8, 64), (2, 64), (0, 64))


def lzf_threshold_input(seed, n):
    """n random bytes holding one repeat of 3..8 bytes, 9 bytes back at position 12"""
    rng = random.Random(seed)
    d = bytearray(rng.randbytes(n))
    k = rng.randrange(3, 9)
    d[12:12 + k] = d[3:3 + k]
    return bytes(d)


def lzf_threshold(seed, codec):
    """Bodies one byte under, at and over the length at which a compressed chunk is kept
    (clen + 2 in {n - 1, n, n + 1})."""
    return [Case(lzf_threshold_input(s, n)) for s, n in LZF_THRESHOLD]


def lzf_literal_runs(seed, codec):
    """31, 32 and 33 literals before a match and in the tail: the run header at MAX_LIT."""
    rng = random.Random(seed)
    out = []
    for k in (31, 32, 33):
        out.append(_hit(rng, codec, 5, k - 6, random_gap=True, only=True))        # the match starts at k
        out.append(_hit(rng, codec, 5, 40, tail=k, random_gap=True, only=True))
    return out


def lzf_signed(seed, codec):
    """Bytes >= 0x80 in the first two positions of the chunk and after a match (first2 reads the first
    byte signed)."""
    rng = random.Random(seed)
    out = [Case(quad(rng, 300, bytes([0x80, 0xFF, 0xC3, 0x9A]))), Case(bytes([0xFF]) * 40), Case(bytes([0x80, 0xFF]) * 30)]
    for _ in range(3):
        d, at = repeat(rng, codec, 12, 60)
        out.append(Case(bytes(b | 0x80 for b in d), None, [("match", None, 60)]))
    return out


LZF = {"lzf_offsets": lzf_offsets, "lzf_lengths": lzf_lengths, "lzf_chunk_sizes": lzf_chunk_sizes,
       "lzf_threshold": lzf_threshold, "lzf_literal_runs": lzf_literal_runs, "lzf_signed": lzf_signed}


# ---- LZ4 fast ----
def lz4_min_lengths(seed, codec):
    """12, 13 and 14 bytes: below LZ4_minLength (13) a block is literals only."""
    rng = random.Random(seed)
    return [Case(f(n)) for n in (12, 13, 14) for f in (bytes, rng.randbytes, lambda n: (b"ab" * 8)[:n])]


def lz4_table_limit(seed, codec):
    """65 546, 65 547 and 65 548 bytes, the only inputs above 64 KiB: the byU16 table below
    LZ4_64Klimit, the byU32 one from it on.  Four chunks repeat their first bytes as far back as
    their end margin allows: 65 534 back (byU16), 65 535 back (byU32, taken) and 65 536 back (byU32,
    too far); a gap of text would overwrite the source's slot, so most of theirs is one run.  Then one
    chunk of plain text at each of the three lengths, with no token aimed at: the two table forms on
    64 KiB of varied data."""
    rng = random.Random(seed)
    a, _ = repeat(rng, codec, 6, 65534, head=0, tail=6)
    b, _ = repeat(rng, codec, 6, 65535, head=0, tail=6)
    c, _ = repeat(rng, codec, 6, 65535, head=1, tail=6)
    e, at = repeat(rng, codec, 6, 65536, head=0, tail=6)
    assert [len(x) for x in (a, b, c, e)] == [65546, 65547, 65548, 65548]
    return [Case(a, 65534, [_m(6, 65534)]), Case(b, 65535, [_m(6, 65535)]), Case(c, 65536, [_m(6, 65535)]),
            Case(e, None, [], (at,))] + [Case(text(rng, n)) for n in (65546, 65547, 65548)]


def lz4_end_margin(seed, codec):
    """A match ending exactly 5 and 6 bytes before the end, and copies that go on to the end (cut at
    n - 5); one starting 12 and one 11 bytes before the end (the latter is past MFLIMIT: literals)."""
    rng = random.Random(seed)
    out = [_hit(rng, codec, 10, 30, tail=5), _hit(rng, codec, 10, 30, tail=6)]
    for cut in (0, 1, 4):
        d, at = repeat(rng, codec, 20, 30, tail=cut)
        out.append(Case(d, at, [_m(len(d) - 5 - at, 30)]))
    out.append(_hit(rng, codec, 7, 30, tail=5))
    out.append(_miss(rng, codec, 6, 30, tail=5))
    return out


def lz4_lengths(seed, codec):
    """Match lengths 4, 18 (token 14), 19 (15, extension 0), 20, 273, 274 (extension 255, 0) and 275."""
    rng = random.Random(seed)
    return [_hit(rng, codec, n, n + 300) for n in (4, 18, 19, 20, 273, 274, 275)]


def lz4_literal_runs(seed, codec):
    """Literal runs of 14, 15 (extension 0), 16, 269, 270 (extension 255, 0) and 271 before a match."""
    rng = random.Random(seed)
    return [_hit(rng, codec, 8, k - 6, random_gap=True, only=True) for k in (14, 15, 16, 269, 270, 271)]


def lz4_skip(seed, codec):
    """3000 incompressible bytes, then 300 of them again: the search step has grown to dozens of bytes
    when the repeat comes."""
    rng = random.Random(seed)
    r = rng.randbytes(3000)
    return [Case(r + r[100:400] + rng.randbytes(30), None, [("match", None, 2900)])]


LZ4 = {"lz4_min_lengths": lz4_min_lengths, "lz4_table_limit": lz4_table_limit, "lz4_end_margin": lz4_end_margin,
       "lz4_lengths": lz4_lengths, "lz4_literal_runs": lz4_literal_runs, "lz4_skip": lz4_skip}


# ---- Snappy ----
def _snappy_copies(length):
    """Snappy.encodeCopy: 64-byte copies while 68 or more are left, a 60-byte one above 64, the rest"""
    out = []
    while length >= 68:
        out.append(64)
        length -= 64
    if length > 64:
        out.append(60)
        length -= 60
    return out + [length]


def snappy_offsets(seed, codec):
    """Offsets 2047 (the last 1-byte-offset copy), 2048 and 2049, and 65 531, the largest there is: a
    65 536-byte chunk repeats its first 4 bytes at the last position the encoder searches (n - 5)."""
    rng = random.Random(seed)
    out = [_hit(rng, codec, 8, d) for d in (2047, 2048, 2049)]
    out.append(_hit(rng, codec, 4, 65531, head=0, tail=1))
    return out


def snappy_lengths(seed, codec):
    """Copy lengths 4, 11 (1-byte offset), 12, 60, 64, 65, 67 (60 + rest), 68, 128 and 130 (64s first)."""
    rng = random.Random(seed)
    return [_hit(rng, codec, n, n + 300, want=[_m(k, n + 300) for k in _snappy_copies(n)])
            for n in (4, 11, 12, 60, 64, 65, 67, 68, 128, 130)]


def snappy_table_steps(seed, codec):
    """Input lengths on both sides of every hash-table size the encoder takes (the next power of two of
    the length, at most 16 384) and of MIN_COMPRESSIBLE_BYTES."""
    rng = random.Random(seed)
    return [Case(quad(rng, n)) for k in range(4, 15) for n in (1 << k, (1 << k) + 1)] + [Case(quad(rng, n)) for n in (14, 15)]


def snappy_margin(seed, codec):
    """The end of the search: a 4-byte repeat at n - 5 is taken, one at n - 4 is not, and a match that
    began earlier runs to the last byte.  (MIN_COMPRESSIBLE_BYTES, the 15-byte limit, is on the input
    length: snappy_table_steps and short_lengths hold 14 and 15 bytes.)"""
    rng = random.Random(seed)
    e, at2 = repeat(rng, codec, 20, 24, tail=0)
    return [_hit(rng, codec, 4, 20, tail=1), _miss(rng, codec, 4, 20, tail=0), Case(e, at2, [_m(20, 24)])]


def snappy_literals(seed, codec):
    """One literal of 17 and 60 bytes (length in the tag), 61 and 256 (one length byte), 257 and 4096
    (two): the classes of test_snappy_literal_length_classes a 64 KiB chunk can reach."""
    rng = random.Random(seed)
    return [Case(rng.randbytes(n)) for n in (17, 60, 61, 256, 257, 4096)]


SNAPPY = {"snappy_offsets": snappy_offsets, "snappy_lengths": snappy_lengths, "snappy_table_steps": snappy_table_steps,
          "snappy_margin": snappy_margin, "snappy_literals": snappy_literals}

GENERATORS = {"fastlz1": {**COMMON, **FASTLZ}, "fastlz2": {**COMMON, **FASTLZ}, "lzf": {**COMMON, **LZF},
              "lz4": {**COMMON, **LZ4}, "snappy": {**COMMON, **SNAPPY}}


def family(codec, name, seed=1):
    return GENERATORS[codec][name](seed, codec)


def all_cases(codec, seed=1):
    """every family's cases of a codec, in order: [(family name, Case)]"""
    return [(name, c) for name in GENERATORS[codec] for c in family(codec, name, seed)]


# ---- planter / victim pairs ----
def plant_pair(seed):
    """(planter, victim): two unlike inputs of 200..400 bytes holding the same eight 6-byte pieces, the
    victim's each 12 bytes later than the planter's.  Each piece occurs once in each, so neither has a
    match of its own there: a victim that took a table entry the planter left (same slot, same bytes,
    a position 12 back) would emit a match the oracle does not."""
    rng = random.Random(0x57A3 + seed)
    c, v = bytearray(rng.randbytes(rng.randrange(260, 401))), bytearray(rng.randbytes(rng.randrange(260, 401)))
    for k in range(8):
        g = rng.randbytes(6)
        c[8 + 30 * k:14 + 30 * k] = g
        v[20 + 30 * k:26 + 30 * k] = g
    return bytes(c), bytes(v)
