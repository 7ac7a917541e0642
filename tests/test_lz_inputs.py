"""The edge-directed inputs of tests/lz_inputs.py, on the CPU: they are deterministic, the oracle's
output on every one parses (tests/lz_tokens.py) and decodes to the input, each family reaches the path
it names (read from the parsed tokens: a family that misses its target fails here), and the oracle
equals its pins on them: the second restatements of FastLZ and LZF, liblz4 for LZ4, and libsnappy's
decoder for Snappy."""
import pytest

import lz_inputs
import lz_tokens
from test_fastlz_restatement import fastlz_compress_py
from test_oracle_kat import _LzfEncoderPy

CODECS = lz_inputs.CODECS
FAMILIES = [(c, f) for c in CODECS for f in lz_inputs.GENERATORS[c]]


def encode(oracle, codec, data, u16_limit=None):
    if codec.startswith("fastlz"):
        return oracle.fastlz_compress(data, int(codec[-1]), u16_limit=len(data) if u16_limit is None else u16_limit)
    return {"lzf": oracle.lzf_encode_chunk, "lz4": oracle.lz4_compress, "snappy": oracle.snappy_encode}[codec](data)


def parse(codec, blob):
    """(tokens without the form field, tokens, decoded bytes)"""
    if codec.startswith("fastlz"):
        level, toks, out = lz_tokens.fastlz(blob)
        assert len(out) < 4 or level == int(codec[-1])  # under 4 bytes: one literal run, no level bit
    elif codec == "lzf":
        _, toks, out = lz_tokens.lzf_chunk(blob)
    else:
        toks, out = getattr(lz_tokens, codec)(blob)
    return [t[:3] if t[0] == "match" else t[:2] for t in toks], toks, out


def tokens(oracle, codec, data):
    """parse() of the oracle's output for data.  LZF: the chunk is parsed and must decode to the input,
    but the tokens are the compressed body's, which a chunk that falls back to raw does not show"""
    toks, full, out = parse(codec, encode(oracle, codec, data))
    assert out == data, (codec, len(data))
    if codec == "lzf" and len(data) >= 16:
        full, out = lz_tokens.lzf_body(oracle.lzf_compress_body(data))
        assert out == data, (codec, len(data))
        toks = full
    return toks, full


def _same(tok, want):
    return len(tok) == len(want) and all(w is None or w == t for t, w in zip(tok, want))


def check_case(case, toks):
    """the tokens show what the Case says its input reaches"""
    placed = lz_tokens.positions(toks)
    for pos in case.lits:
        assert not any(t[0] == "match" and p <= pos < p + t[1] for p, t in placed), (pos, toks)
    if case.want:
        starts = [i for i, (p, t) in enumerate(placed) if _same(t, case.want[0]) and (case.at is None or p == case.at)]
        assert starts, (case.at, case.want, toks)
        i = starts[0]
        got = [t for _, t in placed[i:i + len(case.want)]]
        assert len(got) == len(case.want) and all(_same(t, w) for t, w in zip(got, case.want)), (case.want, got)
        if case.at is not None and i + len(case.want) < len(placed):
            nxt = placed[i + len(case.want)][1]
            assert not (nxt[0] == "match" and nxt[2] == case.want[-1][2]), ("the match goes on", nxt)
    if case.end is not None:
        ends = [p + t[1] for p, t in placed if t[0] == "match"]
        assert ends and ends[-1] == case.end, (case.end, ends[-1:], len(case.data))
    if case.only:
        assert [t for t in toks if t[0] == "match"] == [tuple(w) for w in case.want], toks


@pytest.fixture(scope="module")
def parsed(oracle):
    """codec -> family -> [(Case, tokens, form tokens)], encoded by the oracle once"""
    res = {}
    for codec, fam in FAMILIES:
        rows = []
        for case in lz_inputs.family(codec, fam):
            toks, full = tokens(oracle, codec, case.data)
            rows.append((case, toks, full))
        res.setdefault(codec, {})[fam] = rows
    return res


def test_inputs_are_deterministic():
    for codec, fam in FAMILIES:
        a, b = lz_inputs.family(codec, fam, 5), lz_inputs.family(codec, fam, 5)
        assert a == b and a, (codec, fam)
        assert [c.data for c in a] != [c.data for c in lz_inputs.family(codec, fam, 6)] or fam == "lzf_threshold", (codec, fam)
    assert lz_inputs.plant_pair(3) == lz_inputs.plant_pair(3) != lz_inputs.plant_pair(4)
    assert lz_inputs.filler(3) == lz_inputs.filler(3) != lz_inputs.filler(4)


def test_every_family_has_a_docstring():
    for codec, fam in FAMILIES:
        assert lz_inputs.GENERATORS[codec][fam].__doc__, fam


@pytest.mark.parametrize("codec,fam", FAMILIES)
def test_round_trip_and_coverage(parsed, codec, fam):
    """The oracle's output decodes to the input (asserted where it is parsed) and shows the family's
    path."""
    rows = parsed[codec][fam]
    assert rows
    for case, toks, _ in rows:
        check_case(case, toks)


@pytest.mark.parametrize("codec", CODECS)
def test_match_to_end_lengths_are_consecutive(parsed, codec):
    """25 consecutive chunk lengths, each with its last match ending at the encoder's end margin
    (check_case holds every case to its `end`)."""
    rows = parsed[codec]["match_to_end"]
    assert [len(c.data) for c, _, _ in rows] == list(range(116, 141))
    assert all(c.end == len(c.data) - lz_inputs.END_MARGIN[codec] for c, _, _ in rows)


def _forms(rows):
    return [t for _, _, full in rows for t in full]


def test_fastlz_forms_reached(parsed):
    """What the per-case tokens cannot say: level 2 used the far form from 8192 on and the near form
    up to 8191, and a level-1 265-byte match is a 262-byte token and a 3-byte one."""
    far = {t[2]: t[3] for t in _forms(parsed["fastlz2"]["flz_distances"]) if t[0] == "match" and t[2] > 1}
    assert far[8191] is False and far[8192] is True and far[8447] is True and far[65000] is True and far[257] is False
    assert not any(t[0] == "match" and t[3] for t in _forms(parsed["fastlz1"]["flz_distances"]))
    assert ("match", 262, 565, False) in _forms(parsed["fastlz1"]["flz_long"])
    assert ("match", 20000, 20300, True) in _forms(parsed["fastlz2"]["flz_long"])
    assert any(t[:2] == ("match", 5) and t[3] for t in _forms(parsed["fastlz2"]["flz_lengths"]))
    for level in ("fastlz1", "fastlz2"):  # literal runs of exactly 32 and of 32 + 1
        runs = [[t[1] for t in toks if t[0] == "lit"] for _, toks, _ in parsed[level]["flz_literal_runs"]]
        assert [32] in [r[:1] for r in runs] and any(r[-2:] == [32, 1] for r in runs) and any(r[-2:] == [32, 32] for r in runs)


def test_lzf_forms_reached(parsed, oracle):
    """Offset 8192 is taken and 8193 is not; the threshold inputs sit on both sides of
    clen + 7 < n + 5; 15 bytes are raw, 16 zeros compressed."""
    offs = {t[2] for _, toks, _ in parsed["lzf"]["lzf_offsets"] for t in toks if t[0] == "match"}
    assert 8192 in offs and 8193 not in offs and 1 in offs
    seen = set()
    for case, _, _ in parsed["lzf"]["lzf_threshold"]:
        n, clen = len(case.data), len(oracle.lzf_compress_body(case.data))
        seen.add(clen + 2 - n)
        assert oracle.lzf_encode_chunk(case.data)[2] == (1 if clen + 2 < n else 0)
    assert seen == {-1, 0, 1}
    kinds = {(len(c.data), oracle.lzf_encode_chunk(c.data)[2]) for c, _, _ in parsed["lzf"]["lzf_chunk_sizes"]}
    assert (15, 0) in kinds and (15, 1) not in kinds and (16, 1) in kinds and (16, 0) in kinds
    assert all(c.data[0] >= 0x80 and c.data[1] >= 0x80 for c, _, _ in parsed["lzf"]["lzf_signed"])


def test_lz4_forms_reached(parsed):
    """A match of 274 bytes (length bytes 255, 0) and a literal run of 270 (the same), and the
    table form on each side of 65 547."""
    assert ("match", 274, 574) in [t for _, toks, _ in parsed["lz4"]["lz4_lengths"] for t in toks]
    assert ("lit", 270) in [t for _, toks, _ in parsed["lz4"]["lz4_literal_runs"] for t in toks]
    assert sorted(len(c.data) for c, _, _ in parsed["lz4"]["lz4_table_limit"]) == [65546, 65546, 65547, 65547, 65548, 65548, 65548]


def test_snappy_forms_reached(parsed):
    """1-byte-offset copies up to 2047 and 2-byte-offset ones from 2048; each literal length class."""
    kinds = {t[2]: t[3] for t in _forms(parsed["snappy"]["snappy_offsets"]) if t[0] == "match" and t[1] in (4, 8)}
    assert kinds[2047] == "copy1" and kinds[2048] == "copy2" and kinds[2049] == "copy2" and kinds[65531] == "copy2"
    lens = {t[1]: t[3] for t in _forms(parsed["snappy"]["snappy_lengths"]) if t[0] == "match" and t[2] > 1}
    assert lens[11] == "copy1" and lens[12] == "copy2" and lens[4] == "copy1"
    lits = {(t[1], t[2]) for t in _forms(parsed["snappy"]["snappy_literals"])}
    assert lits == {(17, "lit0"), (60, "lit0"), (61, "lit1"), (256, "lit1"), (257, "lit2"), (4096, "lit2")}


def test_plant_pairs_share_pieces_the_victim_has_once():
    for seed in range(40):
        c, v = lz_inputs.plant_pair(seed)
        assert 200 <= len(c) <= 400 and 200 <= len(v) <= 400 and c != v
        for k in range(8):
            g = v[20 + 30 * k:26 + 30 * k]
            assert c[8 + 30 * k:14 + 30 * k] == g
            for w in range(3):  # no 4-byte piece of it occurs earlier in the victim
                assert v.find(g[w:w + 4]) == 20 + 30 * k + w


@pytest.mark.parametrize("codec", ["fastlz1", "fastlz2", "lzf", "lz4"])
def test_plant_pair_victims_have_no_match_at_the_pieces(oracle, codec):
    """On its own a victim codes every shared piece as literals: a match there on the GPU would be a
    table entry of the planter's."""
    for seed in range(40):
        _, v = lz_inputs.plant_pair(seed)
        toks, _ = tokens(oracle, codec, v)
        check_case(lz_inputs.Case(v, None, [], tuple(20 + 30 * k + 1 for k in range(8))), toks)


@pytest.mark.parametrize("level", [1, 2])
def test_fastlz_restatements_agree_on_the_families(oracle, level):
    """oracle.fastlz_compress == fastlz_compress_py on every chunk of every FastLZ family, at each of
    the readU16 quirk's limits (len, len - 1, len // 2, 1, 0)."""
    for fam, case in lz_inputs.all_cases(f"fastlz{level}"):
        for lim in lz_inputs.fastlz_limits(len(case.data)):
            assert oracle.fastlz_compress(case.data, level, u16_limit=lim) == fastlz_compress_py(case.data, level, u16_limit=lim), \
                (fam, len(case.data), lim)


def test_lzf_restatements_agree_on_the_families(oracle):
    for fam, case in lz_inputs.all_cases("lzf"):
        if len(case.data) >= 4:  # tryCompress reads two bytes before it looks at the length
            assert oracle.lzf_compress_body(case.data) == _LzfEncoderPy()._try_compress(case.data, 0, len(case.data)), \
                (fam, len(case.data))


def test_lz4_families_equal_liblz4(oracle):
    """the availability condition of test_oracle_kat.py::test_lz4_compress_equals_liblz4"""
    pa = pytest.importorskip("pyarrow")
    z = pa.Codec("lz4_raw")
    for fam, case in lz_inputs.all_cases("lz4"):
        if case.data:
            assert oracle.lz4_compress(case.data) == z.compress(case.data).to_pybytes(), (fam, len(case.data))


def test_snappy_families_decode_with_libsnappy(oracle):
    """the availability condition of test_oracle_kat.py::test_snappy_blocks_decode_with_libsnappy"""
    pa = pytest.importorskip("pyarrow")
    sn = pa.Codec("snappy")
    for fam, case in lz_inputs.all_cases("snappy"):
        if case.data:
            enc = oracle.snappy_encode(case.data)
            assert sn.decompress(enc, decompressed_size=len(case.data)).to_pybytes() == case.data, (fam, len(case.data))


def test_parsers_reject_malformed():
    for f, blob in ((lz_tokens.fastlz, bytes([0x40])), (lz_tokens.fastlz, bytes([0x00, 0x41, 0x20, 0x05])),
                    (lz_tokens.fastlz, bytes([0x05, 1, 2])), (lz_tokens.lzf_body, bytes([0x20, 0x05])),
                    (lz_tokens.lzf_chunk, b"ZX\x00\x00\x00"), (lz_tokens.lzf_chunk, b"ZV\x00\x00\x02a"),
                    (lz_tokens.lz4, bytes([0x10, 0x41, 0x05, 0x00])), (lz_tokens.lz4, bytes([0x11, 0x41])),
                    (lz_tokens.lz4, bytes([0x10, 0x41, 0x01, 0x00, 0x00])),
                    (lz_tokens.snappy, bytes([5, 0x00, 0x41])), (lz_tokens.snappy, bytes([4, 0x01, 0x09]))):
        with pytest.raises(lz_tokens.Malformed):
            f(blob)
