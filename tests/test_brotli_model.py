"""Pins tests/brotli_model.py: on libbrotli's own streams that stay inside its subset, on the host encoder's
stream of every item (where it must regenerate what libbrotli regenerates), and on hand-built uncompressed, flush
and final blocks.  The last two tests below need no encoder: they pin the test helper itself and would pass
without the feature; the first one, and every other new test file, does not."""
import pytest

import brotli_inputs as I
import brotli_model as M

pa = pytest.importorskip("pyarrow")


@pytest.fixture(scope="module")
def codec():
    return pa.Codec("brotli")


@pytest.fixture(scope="module")
def B():
    from netty_amd import batch
    return batch


def lib(codec, s, n):
    return codec.decompress(s, decompressed_size=n).to_pybytes()


def test_model_regenerates_what_libbrotli_regenerates(B, codec, oracle):
    for name, data in I.items(oracle):
        st, s = B.brotli_encode_host(data)
        assert st == 0
        out, census = M.decode(s)
        assert out == lib(codec, s, len(data)) == data, name
        assert census["last"] and census["consumed"] == len(s), name


def test_hand_built_blocks(codec):
    raw = b"hello, raw"
    # lgwin 16 (one 0 bit), then ISLAST 0, MNIBBLES 0, MLEN - 1 = 9 in 16 bits, ISUNCOMPRESSED 1: 21 bits, padded to 24
    head = (0 | 0 << 1 | 0 << 2 | (len(raw) - 1) << 4 | 1 << 20).to_bytes(3, "little")
    stream = head + raw + b"\x06" + b"\x03"  # the block, the flush marker, the final block
    out, census = M.decode(stream)
    assert out == raw == lib(codec, stream, len(raw))
    assert (census["uncompressed"], census["metadata"], census["compressed"], census["lgwin"]) == (1, 1, 0, 16)
    assert census["consumed"] == len(stream)
    assert M.decode(b"\x3b")[0] == b"" and M.decode(b"\x3b")[1]["lgwin"] == 22
    # an open end is a prefix of a handle's writes, not a stream
    assert M.decode(head + raw + b"\x06", allow_open_end=True)[0] == raw
    with pytest.raises(M.Truncated):
        M.decode(head + raw + b"\x06")
    with pytest.raises(M.Truncated):
        M.decode(head + raw[:-1])
    with pytest.raises(Exception):
        lib(codec, head + raw[:-1], len(raw))
    with pytest.raises(M.BrotliError):
        M.decode(head + raw + b"\x0e" + b"\x03")  # the reserved bit of a metadata block


def test_model_reads_libbrotli_streams_inside_the_subset(codec):
    """quality 0 and 1 write one block type and no context map; a stream that leaves the subset or uses the static
    dictionary is reported, never misread"""
    read = 0
    for q in (0, 1):
        c = pa.Codec("brotli", compression_level=q)
        for data in (b"abcabcabcabd" * 50, bytes(range(256)) * 8, I.few(3), I.rand(5, 3000)):
            s = c.compress(data).to_pybytes()
            try:
                out, census = M.decode(s)
            except M.BrotliError as e:
                assert "subset" in str(e) or "dictionary" in str(e), e
                continue
            assert out == data and census["consumed"] == len(s)
            read += 1
    assert read >= 4
