"""CPU tests of the Brotli encoder's format core through nx_brotli_encode_host: libbrotli (pyarrow) and the model
decoder of tests/brotli_model.py decode every stream to the item, the stream ends where it says, the size bound
holds, a short buffer is refused without a byte past it, and the census over the whole set still shows every
feature the encoder is meant to emit."""
import pytest

import brotli_inputs as I
import brotli_model as M

pa = pytest.importorskip("pyarrow")

NX_ERR_INVALID_ARG, NX_ERR_BROTLI_LGWIN, NX_ERR_BROTLI_ENCODE_FULL = -100, -151, -153
# Measured on the CPU with this test's own loop: the host encoder's 371 183 bytes over ratio_set divided by
# libbrotli quality 1's 370 414 through pyarrow 25.0.0 are RATIO_MEASURED.  The encoder is deterministic; the margin
# is for another libbrotli inside another pyarrow.
RATIO_MEASURED = 1.0021
RATIO_BAR = RATIO_MEASURED + 0.05


@pytest.fixture(scope="module")
def codec():
    return pa.Codec("brotli")


@pytest.fixture(scope="module")
def B():
    from netty_amd import batch
    return batch


@pytest.fixture(scope="module")
def items(oracle):
    return I.items(oracle)


@pytest.fixture(scope="module")
def encoded(B, items):
    """(stream, stats) of every item at every window, computed once"""
    out = {}
    for name, data in items:
        for lg in I.LGWINS:
            st, s, stats = B.brotli_encode_host(data, lgwin=lg, stats=True)
            assert st == 0, (name, lg)
            out[name, lg] = (s, stats)
    return out


def test_libbrotli_decodes_every_item_at_every_window(codec, items, encoded):
    for name, data in items:
        for lg in I.LGWINS:
            s = encoded[name, lg][0]
            assert codec.decompress(s, decompressed_size=len(data)).to_pybytes() == data, (name, lg)


def test_every_stream_ends_exactly_at_its_end(items, encoded):
    for name, data in items:
        for lg in I.LGWINS:
            s = encoded[name, lg][0]
            out, census = M.decode(s + b"\x55")
            assert out == data and census["last"] and census["consumed"] == len(s), (name, lg)
            assert census["lgwin"] == lg
            if len(s) > 1:
                with pytest.raises(M.BrotliError):
                    M.decode(s[:-1])


def test_no_distance_passes_the_window(B, codec, items, encoded):
    for name, data in items:
        for lg in I.LGWINS:
            census = M.decode(encoded[name, lg][0])[1]
            assert census["max_distance"] <= (1 << lg) - 16, (name, lg)
    data = dict(I.directed())["window10"]
    s = encoded["window10", 10][0]
    assert codec.decompress(s, decompressed_size=len(data)).to_pybytes() == data
    assert M.decode(s)[1]["max_distance"] <= 1008
    assert M.decode(encoded["window10", 16][0])[1]["max_distance"] == 2000  # the repeat is there to be found


def test_size_bound(B, items, encoded):
    for n, want in [(0, 3), (1, 8), (65536, 65536 + 7), (65537, 65537 + 11), (200000, 200000 + 19)]:
        assert B.brotli_max_compressed_length(n) == want
    for name, data in items:
        for lg in I.LGWINS:
            assert len(encoded[name, lg][0]) <= B.brotli_max_compressed_length(len(data)), (name, lg)
    # the worst case: nothing to find, two meta-blocks
    assert encoded["random70000", 22][1]["uncompressed_blocks"] == 2


def test_out_cap_one_byte_short(B, items, encoded):
    for name, data in items:
        s = encoded[name, 22][0]
        st, out, guard = B.brotli_encode_host(data, lgwin=22, out_cap=len(s) - 1, guard=16)
        assert (st, out, guard) == (NX_ERR_BROTLI_ENCODE_FULL, b"", b"\xa5" * 16), name
        st, out, guard = B.brotli_encode_host(data, lgwin=22, out_cap=len(s), guard=16)
        assert (st, out, guard) == (0, s, b"\xa5" * 16), name


def test_census_shows_every_feature(items, encoded):
    total = {"simple": [0] * 4, "select": [0, 0]}
    keys = ("compressed_blocks", "uncompressed_blocks", "ring_copies", "implicit_copies", "split_copies", "complex_codes", "limited_codes")
    for k in keys:
        total[k] = 0
    deepest = longest = far_code = continued = ignored = 0
    for name, _ in items:
        s, stats = encoded[name, 22]
        census = M.decode(s)[1]
        for k in keys:
            total[k] += stats[k]
        for i in range(4):
            total["simple"][i] += stats["simple_codes"][i]
            assert stats["simple_codes"][i] == census["simple"][i], name
        assert stats["complex_codes"] == census["complex"] and stats["compressed_blocks"] == census["compressed"], name
        assert stats["uncompressed_blocks"] == census["uncompressed"] and stats["commands"] == census["commands"], name
        assert stats["literals"] == census["literals"] and stats["implicit_copies"] == census["implicit"], name
        assert stats["ring_copies"] == census["ring"], name
        total["select"][0] += census["tree_select"][0]
        total["select"][1] += census["tree_select"][1]
        deepest = max(deepest, stats["max_depth_unlimited"])
        longest = max(longest, census["max_code_length"])
        far_code = max(far_code, census["max_distance_code"])
        continued += census["continued"]
        ignored += census["ignored_copy"]
    assert all(total["simple"]), total          # NSYM 1, 2, 3 and 4
    assert all(total["select"]), total          # both 4-symbol shapes
    assert all(total[k] for k in keys), total   # complex and limited codes, both block kinds, ring, implicit, a cut copy
    assert deepest > 15 >= longest              # a code that needed limiting, and no length over 15
    assert far_code >= 16 + 2 * 15              # a distance over 65 536: 16 or more extra bits
    assert continued and ignored                # a copy going on in the next block; a block ending in literals
    assert encoded["run65537", 22][1]["split_copies"] == 1


def test_bad_arguments(B):
    for lg in (-2, 0, 9, 25, 30):
        assert B.brotli_encode_host(b"abc", lgwin=lg)[0] == NX_ERR_BROTLI_LGWIN
    assert B.brotli_encode_host(b"abc", lgwin=-1) == B.brotli_encode_host(b"abc", lgwin=22)
    assert B.brotli_encode_host(b"", lgwin=22) == (0, b"\x3b") and B.brotli_encode_host(b"", lgwin=16) == (0, b"\x06")


def test_ratio_against_libbrotli_quality_1(B, oracle):
    q1 = pa.Codec("brotli", compression_level=1)
    ours = theirs = 0
    for data in I.ratio_set(oracle):
        st, s = B.brotli_encode_host(data)
        assert st == 0
        ours += len(s)
        theirs += len(q1.compress(data).to_pybytes())
    print("host encoder %d bytes, libbrotli quality 1 %d bytes, ratio %.4f" % (ours, theirs, ours / theirs))
    assert ours / theirs <= RATIO_BAR
