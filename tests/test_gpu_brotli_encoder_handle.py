"""GPU tests of the BrotliEncoder handle (nx_brotli_encoder_*, handlers.BrotliEncoder): one stream over many
writes, every write flushed, so that any prefix of the writes plus the byte 0x03 is a complete stream."""
import random

import pytest

import brotli_model as M

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
pa = pytest.importorskip("pyarrow")


@pytest.fixture(scope="module")
def H():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    import netty_amd
    return netty_amd


def lib(s, n):
    return pa.Codec("brotli").decompress(s, decompressed_size=n).to_pybytes()


def writes(oracle):
    return [oracle.textgen_chunk(4, 3000), b"", random.Random(3).randbytes(2000), b"q", oracle.textgen_chunk(5, 70000)]


@pytest.mark.parametrize("window", [-1, 16, 10])
def test_sequence_of_writes(H, oracle, window):
    e = H.BrotliEncoder(window=window)
    stream, plain = b"", b""
    for w in writes(oracle):
        out = e.encode(w)
        if not w:
            assert out == b""  # an unreadable message: nothing, and nothing changes
            continue
        stream += out
        plain += w
        assert lib(stream + b"\x03", len(plain)) == plain
        got, census = M.decode(stream + b"\x03")
        assert got == plain and census["consumed"] == len(stream) + 1 and census["metadata"] >= 1
        assert M.decode(stream, allow_open_end=True)[0] == plain  # whole bytes: the prefix ends on a block boundary
    assert not e.is_closed()
    tail = e.finish_encode()
    assert tail == b"\x03" and e.is_closed()
    assert lib(stream + tail, len(plain)) == plain
    census = M.decode(stream + tail)[1]
    assert census["lgwin"] == (22 if window == -1 else window) and census["metadata"] == 4
    assert e.finish_encode() == b""          # a second close writes nothing
    assert e.encode(b"late") == b""          # a write after close: an empty buffer and no error
    e.close()


def test_close_on_a_fresh_handle(H):
    for window, want in ((-1, b"\x3b"), (16, b"\x06"), (10, b"\xa1\x01")):
        e = H.BrotliEncoder(window=window)
        assert e.encode(b"") == b""
        tail = e.finish_encode()
        assert tail == want and M.decode(tail)[0] == b"" and lib(tail, 0) == b""
        assert e.finish_encode() == b"" and e.encode(b"x") == b""
        e.close()


def test_writes_equal_the_batch_encoder_but_for_the_ending(H, oracle):
    """a first write is the batch stream with the flush marker where the last block would be"""
    from netty_amd import batch as B
    data = oracle.textgen_chunk(6, 5000)
    e = H.BrotliEncoder()
    out = e.encode(data)
    whole = B.brotli_encode_host(data)[1]
    assert M.decode(out + b"\x03")[0] == data
    assert out[:len(whole) - 2] == whole[:len(whole) - 2]
    e.close()


def test_constructor_ranges(H):
    from netty_amd import _lib
    L = _lib.load()
    for q in (-2, 12):
        with pytest.raises(ValueError, match="quality"):
            H.BrotliEncoder(quality=q)
        assert L.nx_brotli_encoder_check(q, -1, 1) == -150 and not L.nx_brotli_encoder_new(q, -1, 1)
    for w in (-2, 0, 9, 25):
        with pytest.raises(ValueError, match="lgwin"):
            H.BrotliEncoder(window=w)
        assert L.nx_brotli_encoder_check(4, w, 1) == -151 and not L.nx_brotli_encoder_new(4, w, 1)
    for m in (-1, 3):
        with pytest.raises(ValueError, match="mode"):
            H.BrotliEncoder(mode=m)
        assert L.nx_brotli_encoder_check(4, -1, m) == -152 and not L.nx_brotli_encoder_new(4, -1, m)
    # quality and mode are checked and change nothing
    outs = set()
    for q, m in ((-1, 0), (0, 1), (11, 2), (4, 1)):
        e = H.BrotliEncoder(quality=q, window=24, mode=m)
        outs.add(e.encode(b"the same bytes, the same bytes"))
        e.close()
    assert len(outs) == 1


def test_batch_equals_host(oracle):
    from netty_amd import batch as B
    dev = torch.device("cuda:0")
    chunks = [oracle.textgen_chunk(k, n) for k, n in ((1, 100), (2, 4000), (3, 66000))] + [b""]
    inp, off, ln = B.pack(chunks, dev, align=1, pad=16)
    caps = [B.brotli_max_compressed_length(len(c)) for c in chunks]
    out, ooff = B.out_slots(caps, dev, align=1)
    olen, st = B.brotli_encode(inp, off, ln, out, ooff, torch.tensor(caps, dtype=torch.int32))
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0] * len(chunks)
    outh = out.cpu().numpy().tobytes()
    for c, o, w in zip(chunks, ooff.cpu().tolist(), olen.cpu().tolist()):
        assert outh[o:o + w] == B.brotli_encode_host(c)[1]
