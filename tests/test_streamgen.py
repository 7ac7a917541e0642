"""The generated valid streams of tests/streamgen.py, pinned without a GPU: for every case set the
GPU grammar tests use, the builder's expected bytes (its own LZ77 byte loop) must equal what the
oracle's restatement of the reference decoder produces, with status OK and the whole stream
consumed; no case may be rejected.  Where pyarrow is present, its libsnappy and liblz4 (`lz4_raw`)
must decode the Snappy and LZ4 cases to the same bytes: two decoders that share nothing with the
generator."""
import pytest

import streamgen as G

ALT_NAMES = sorted(G.ALT)


def test_builders_on_hand_checked_streams():
    """Every form once, against bytes worked out by hand from the format descriptions."""
    L, C = G.literal, G.copy
    s, w = G.snappy([L(b"abcde", 63), C(5, 4, 1), C(2, 3, 2), C(9, 2, 4), L(b"z", 60)], preamble_pad=3)
    assert s == bytes([0x8F, 0x80, 0x00, 63 << 2, 4, 0, 0, 0]) + b"abcde" + bytes([0x01, 5, 0x02 | 2 << 2, 2, 0, 0x03 | 1 << 2, 9, 0, 0, 0,
                                                                                    60 << 2, 0]) + b"z"
    assert w == b"abcdeabcdcdcdez"
    s, w = G.lz4([L(b"ab"), C(2, 4), C(1, 19), L(b"x" * 15)])
    assert s == bytes([0x20]) + b"ab" + bytes([2, 0, 0x0F, 1, 0, 0, 0xF0, 0]) + b"x" * 15
    assert w == b"ab" + b"abab" + b"b" * 19 + b"x" * 15
    s, w = G.lzf([L(b"abc"), C(3, 3), C(1, 9)])
    assert s == bytes([2]) + b"abc" + bytes([0x20, 2, 0xE0, 0, 0]) and w == b"abcabc" + b"c" * 9
    s, w = G.fastlz([L(b"abc"), C(3, 3), C(1, 9)], 1)
    assert s == bytes([2]) + b"abc" + bytes([0x20, 2, 0xE0, 0, 0]) and w == b"abcabc" + b"c" * 9
    s, w = G.fastlz([L(bytes(8192)), C(8192, 3), C(8191, 9 + 255)], 2)
    assert s[0] == 0x20 | 31 and s[-8:] == bytes([0x3F, 0xFF, 0, 0, 0xFF, 0xFF, 0, 0xFE]) and len(w) == 8192 + 3 + 264


@pytest.mark.parametrize("name", ["overlap_grid", "ring_sweep", "edges", "chains", "straddles", "walk", "large"])
def test_snappy_sets_decode_by_the_oracle(oracle, name):
    cases = G.snappy_sets()[name]
    assert cases
    rejected = []
    for i, (s, want) in enumerate(cases):
        st, out, cons = oracle.snappy_decode(s, 1 << 24)
        if st != 0 or out != want or cons != len(s):
            rejected.append((i, st, cons, len(s), len(out), len(want)))
    assert not rejected, rejected[:5]


def test_snappy_sets_cover_the_forms():
    """The sets hold what no project encoder emits: COPY_4 at every offset range, copies under 4 bytes,
    literal codes 62 / 63, non-minimal literal fields, padded preambles, offsets above 65535."""
    S = G.snappy_sets()
    seen = set()
    for name in S:
        for s, want in S[name][:40] + S[name][-4:]:
            p, v, sh = 0, 0, 0
            while True:
                v |= (s[p] & 0x7F) << sh
                sh += 7
                p += 1
                if not s[p - 1] & 0x80:
                    break
            assert v == len(want)
            if p > 1 and v < 1 << (7 * (p - 1)):
                seen.add("padded_preamble")
            while p < len(s):
                t = s[p]
                if t & 3 == 0:
                    code = t >> 2
                    nb = max(0, code - 59)
                    n = (int.from_bytes(s[p + 1:p + 1 + nb], "little") if nb else code) + 1
                    seen.add(f"lit{min(code, 59)}" if code < 60 else f"lit{code}")
                    if nb and (n <= 60 or n - 1 < 1 << (8 * (nb - 1))):
                        seen.add("non_minimal_literal")
                    p += 1 + nb + n
                elif t & 3 == 1:
                    seen.add("copy1")
                    p += 2
                elif t & 3 == 2:
                    seen.add("copy2_short" if (t >> 2) + 1 < 4 else "copy2")
                    p += 3
                else:
                    off = int.from_bytes(s[p + 1:p + 5], "little")
                    seen.add("copy4_near" if off < 2048 else ("copy4_far" if off > 65535 else "copy4"))
                    if (t >> 2) + 1 < 4:
                        seen.add("copy4_short")
                    p += 5
            assert p == len(s)
    assert seen >= {"padded_preamble", "non_minimal_literal", "lit59", "lit60", "lit61", "lit62", "lit63", "copy1", "copy2",
                    "copy2_short", "copy4", "copy4_near", "copy4_far", "copy4_short"}, seen


@pytest.mark.parametrize("name", ALT_NAMES)
def test_alt_sets_decode_by_the_oracle(oracle, name):
    rejected, n = [], 0
    for sname, cases in G.alt_sets(name).items():
        assert cases
        for i, (s, want) in enumerate(cases):
            n += 1
            if name == "lz4":
                st, out = oracle.lz4_decompress(s, len(want))
                ok = st == 0 and out == want
                # (consumed: the oracle takes a block only if its last sequence ends on the last input byte)
                ok = ok and oracle.lz4_decompress(s + b"\x00", len(want))[0] != 0
                ok = ok and oracle.lz4_decompress(s[:-1], len(want))[0] != 0
            elif name == "lzf":
                st, out = oracle.lzf_decode_chunk(s, len(want))
                ok = st == 0 and out == want and oracle.lzf_decode_chunk(s[:-1], len(want))[0] != 0
            else:
                r, out = oracle.fastlz_decompress(s, len(want))
                ok = r == len(want) and out == want and oracle.fastlz_decompress(s[:-1], len(want))[0] != len(want)
            if not ok:
                rejected.append((sname, i, len(s), len(want)))
    assert n > 500 and not rejected, rejected[:5]


def test_snappy_sets_decode_by_libsnappy():
    pa = pytest.importorskip("pyarrow")
    codec = pa.Codec("snappy")
    for name, cases in G.snappy_sets().items():
        for i, (s, want) in enumerate(cases):
            got = codec.decompress(s, decompressed_size=len(want)).to_pybytes()
            assert got == want, (name, i)


def test_lz4_sets_decode_by_liblz4():
    """(`lz4_short_tails` is left out: liblz4 wants a block's last five bytes to be literals, the
    reference's decoder and the oracle do not.)"""
    pa = pytest.importorskip("pyarrow")
    codec = pa.Codec("lz4_raw")
    for name, cases in G.alt_sets("lz4").items():
        if name == "lz4_short_tails":
            continue
        for i, (s, want) in enumerate(cases):
            got = codec.decompress(s, decompressed_size=len(want)).to_pybytes()
            assert got == want, (name, i)
