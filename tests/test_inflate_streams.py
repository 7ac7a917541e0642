"""The inflate tests' inputs are what they claim, under zlib alone (no GPU): every crafted valid
stream ends cleanly, every crafted invalid one fails with exactly the expected zlib message, the
split-point stream has the blocks and the far copy it is meant to have, the JdkZlibTest fixture
holds its two members, and the fuzz corpus exercises all three outcomes."""
import gzip
import os
import zlib

import pytest

import inflate_streams as IS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_stops_before_an_incomplete_symbol():
    z = zlib.compress(b"hello world hello world", 6)[2:-4]
    r = IS.reference(z[:10], bytewise=True)
    assert r == IS.reference(z[:10]) and r.out == zlib.decompressobj(-15).decompress(z[:10])
    assert r.kind == "need" and b"hello world hello world".startswith(r.out) and 0 < len(r.out) < 23
    r = IS.reference(z + b"junk")
    assert r.kind == "end" and r.out == b"hello world hello world" and r.consumed == len(z)


def test_crafted_valid_streams_end_under_zlib():
    S = IS.crafted_valid()
    assert len(S) >= 13
    for name, z in S.items():
        r = IS.reference(z)
        assert r.kind == "end" and r.consumed == len(z), (name, r.kind, r.text)
        assert len(z) > 70000 or r == IS.reference(z, bytewise=True), name
        assert zlib.decompress(z, -15) == r.out, name
    assert [len(IS.reference(S[f"stored_{n}"]).out) for n in (0, 1, 65535)] == [0, 1, 65535]
    assert IS.reference(S["rle_distance_1"]).out == b"x" * 517 + b"yyyy"
    assert len(IS.reference(S["fixed_all_bases"]).out) > 32768 + sum(IS.LEN_BASE)
    assert IS.reference(S["no_distance_code"]).out == b"only literals really" * 9


def test_crafted_invalid_streams_fail_with_the_expected_message():
    E = IS.crafted_invalid()
    texts = {t for _, t in E.values()}
    assert texts == {"invalid block type", "invalid stored block lengths", "too many length or distance symbols",
                     "invalid code lengths set", "invalid bit length repeat", "invalid code -- missing end-of-block",
                     "invalid literal/lengths set", "invalid distances set", "invalid literal/length code",
                     "invalid distance code", "invalid distance too far back"}
    for name, (z, text) in E.items():
        r = IS.reference(z, bytewise=True)
        assert r == IS.reference(z), name
        with pytest.raises(zlib.error, match=text):  # Python's own binding agrees
            zlib.decompressobj(-15).decompress(z)
        assert r.kind == "error" and r.text == text, (name, r.kind, r.text)
        if name != "distance_too_far":
            assert r.out.startswith(b"before the error "), name
    assert IS.reference(E["litlen_code_286"][0]).out == b"before the error ab"
    assert IS.reference(E["distance_too_far"][0]).out == b"ab"


def test_split_stream_shape():
    z = IS.split_stream()
    assert 2000 <= len(z) <= 3000
    r = IS.reference(z)
    assert r.kind == "end" and r.consumed == len(z) and len(r.out) > 32768 + 2000
    assert r.out[32768:32768 + 358] == r.out[:358]  # the copies at distance 32768


def test_multiple_gz_fixture():
    raw = open(os.path.join(ROOT, "tests", "golden", "multiple.gz"), "rb").read()
    assert len(raw) == 46
    first = zlib.decompressobj(31)
    assert first.decompress(raw) == b"a" and first.eof
    assert gzip.decompress(first.unused_data) == b"b"
    assert gzip.decompress(raw) == b"ab"


def test_fuzz_corpus_covers_every_outcome():
    corpus = IS.fuzz_corpus()
    assert len(corpus) == IS.N_FUZZ == 600
    assert all(len(z) <= 3100 for z, _ in corpus)
    for kind in ("end", "need", "error"):
        share = sum(1 for _, r in corpus if r.kind == kind) / len(corpus)
        assert share >= 0.05, (kind, share)
    assert len({r.text for _, r in corpus if r.kind == "error"}) >= 5
