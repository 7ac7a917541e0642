"""GPU tests of handlers.LzmaFrameEncoder in the shape of the reference's LzmaFrameEncoderTest: a message cut into
writes of 0-49 bytes gives one stream per write, which liblzma decodes to that write's bytes."""
import lzma
import random

import pytest

import lzma_model as M

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def nx():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    import netty_amd
    return netty_amd


def _unlzma(stream):
    d = lzma.LZMADecompressor(format=lzma.FORMAT_ALONE)
    out = d.decompress(stream)
    assert d.eof and d.unused_data == b""
    return out


@pytest.mark.parametrize("kind", ["text", "random"])
def test_writes_of_random_sizes(nx, oracle, kind):
    data = oracle.textgen_chunk(3, 4096) if kind == "text" else random.Random(5).randbytes(4096)
    rng = random.Random(7)
    enc = nx.LzmaFrameEncoder()
    got, pos, writes = bytearray(), 0, 0
    while pos < len(data):
        n = min(rng.randrange(50), len(data) - pos)
        s = enc.encode(data[pos:pos + n])
        assert s[:13] == bytes([0x5D]) + (65536).to_bytes(4, "little") + n.to_bytes(8, "little")
        piece = _unlzma(s)
        assert piece == data[pos:pos + n]
        got += piece
        pos += n
        writes += 1
    enc.close()
    assert bytes(got) == data and writes > 100


def test_empty_write_is_eighteen_bytes(nx):
    enc = nx.LzmaFrameEncoder()
    assert enc.encode(b"") == bytes([0x5D, 0, 0, 1, 0]) + bytes(8) + bytes(5)
    assert enc.write(b"") == enc.encode(b"")  # no state between writes
    enc.close()


def test_handle_writes_the_host_bytes(nx):
    from netty_amd import batch as B
    data = b"one stream per write, " * 40
    for kw, args in [(dict(), ()), (dict(lc=0, lp=2, pb=1), (0, 2, 1)), (dict(dictionary_size=64), (3, 0, 2, 64)),
                     (dict(end_marker_mode=True, num_fast_bytes=273), (3, 0, 2, 65536, True))]:
        enc = nx.LzmaFrameEncoder(**kw)
        assert enc.encode(data) == B.lzma_encode_host(data, *args)[1]
        enc.close()


@pytest.mark.parametrize("kw,msg", [
    (dict(lc=9), "lc: 9 (expected: 0-8)"), (dict(lc=-1), "lc: -1 (expected: 0-8)"),
    (dict(lp=5), "lp: 5 (expected: 0-4)"), (dict(pb=5), "pb: 5 (expected: 0-4)"), (dict(pb=-2), "pb: -2 (expected: 0-4)"),
    (dict(dictionary_size=-1), "dictionarySize: -1 (expected: 0+)"),
    (dict(num_fast_bytes=4), "numFastBytes: 4 (expected: 5-273)"), (dict(num_fast_bytes=274), "numFastBytes: 274 (expected: 5-273)"),
])
def test_constructor_messages(nx, kw, msg):
    with pytest.raises(ValueError) as e:
        nx.LzmaFrameEncoder(**kw)
    assert str(e.value) == msg


def test_native_constructor_codes(nx):
    from netty_amd import _lib
    L = _lib.load()
    assert L.nx_lzma_frame_encoder_check(9, 0, 0, 0, 32) == -140
    assert L.nx_lzma_frame_encoder_check(3, 0, 2, -1, 32) == -141
    assert L.nx_lzma_frame_encoder_check(3, 0, 2, 0, 4) == -142
    assert L.nx_lzma_frame_encoder_check(8, 4, 4, 0, 273) == 0
    assert not L.nx_lzma_frame_encoder_new(3, 0, 5, 65536, 0, 32)
    assert "lc" in _lib.status_string(-140) and "dictionarySize" in _lib.status_string(-141)
    assert "numFastBytes" in _lib.status_string(-142) and "LZMA" in _lib.status_string(-143)


def test_lc_eight_round_trips_through_the_model_decoder(nx, oracle):
    data = oracle.textgen_chunk(3, 3000)
    enc = nx.LzmaFrameEncoder(lc=8, lp=0, pb=2)
    s = enc.encode(data)
    enc.close()
    assert M.parse_header(s) == (8, 0, 2, 65536, len(data))
    out, packets = M.decode(s)
    assert out == data and any(k == M.MATCH for k, _, _ in packets)
