"""GPU tests of the ZstdEncoder handle (ZstdEncoder.java:90-193).  The checker is libzstd through
pyarrow's streaming reader, which reads concatenated frames as one stream."""
import random

import pytest

import zstd_frames as Z

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
pa = pytest.importorskip("pyarrow")


@pytest.fixture(scope="module")
def H():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from netty_amd import handlers
    return handlers


def _unzstd_stream(data):
    if not data:
        return b""
    return pa.CompressedInputStream(pa.BufferReader(data), "zstd").read()


def _bound(n):
    return n + (n >> 8) + ((131072 - n) >> 11 if n < 131072 else 0)


def test_constructor_refusals(H):
    for kw in (dict(compression_level=23), dict(compression_level=-131073), dict(block_size=0), dict(block_size=-1),
               dict(max_encode_size=0), dict(max_encode_size=-7)):
        with pytest.raises(ValueError):
            H.ZstdEncoder(**kw)
    from netty_amd import _lib
    L = _lib.load()
    for args in ((23, 65536, 1 << 25), (-131073, 65536, 1 << 25), (3, 0, 1 << 25), (3, 65536, 0)):
        assert not L.nx_zstd_encoder_new(*args)
    e = H.ZstdEncoder()
    assert (e.compression_level, e.block_size, e.max_encode_size) == (3, 1 << 16, 1 << 25)
    e.close()
    for level in (-131072, 22):
        H.ZstdEncoder(level).close()


@pytest.mark.parametrize("block_size", [64, 4096, 65536, 200_000])
def test_random_slices_round_trip(H, oracle, block_size):
    rng = random.Random(block_size)
    total = {64: 3000, 4096: 40_000, 65536: 300_000, 200_000: 650_000}[block_size]
    data = b"".join(oracle.textgen_chunk(k, 65536) for k in range(-(-total // 65536)))[:total]
    e = H.ZstdEncoder(block_size=block_size)
    out, p, fed = bytearray(), 0, 0
    while p < len(data):
        k = min(len(data) - p, rng.choice((1, 7, block_size // 3 + 1, block_size, 2 * block_size + 5)))
        got = e.encode(data[p:p + k])
        before, fed = fed, fed + k
        if before // block_size == fed // block_size:
            assert got == b""  # nothing is emitted before a block fills
        else:
            assert got != b""
        out += got
        p += k
    out += e.flush()
    assert e.flush() == b""  # nothing pending
    e.close()
    frames = Z.parse_frames(bytes(out))
    assert sum(f.content_size for f in frames) == len(data)
    assert all(f.content_size <= 65536 for f in frames)
    # a block is cut into 64 KiB slices, each its own frame: 4 frames per block of 200 000 bytes, else one
    full, rest = divmod(total, block_size)
    assert len(frames) == full * -(-block_size // 65536) + -(-rest // 65536)
    assert _unzstd_stream(bytes(out)) == data


def test_flush_with_nothing_pending_and_close_drops(H):
    e = H.ZstdEncoder(block_size=1000)
    assert e.flush() == b""
    assert e.encode(b"x" * 999) == b""
    e.close()  # handlerRemoved: the buffered bytes are dropped
    e.close()
    e = H.ZstdEncoder(block_size=1000)
    assert e.encode(b"y" * 400) == b""
    out = e.flush()
    assert _unzstd_stream(out) == b"y" * 400
    e.close()


def test_max_encode_size(H):
    bs, n = 4096, 10_000
    need = 2 * _bound(bs) + _bound(n - 2 * bs)
    data = random.Random(2).randbytes(n)
    e = H.ZstdEncoder(block_size=bs, max_encode_size=need - 1)
    assert e.encode(data[:100]) == b""
    with pytest.raises(H.EncoderException) as ei:
        e.encode(data[100:])
    assert str(ei.value) == f"requested encode buffer size ({need} bytes) exceeds the maximum allowable size ({need - 1} bytes)"
    # the handle is unchanged: the 100 bytes are still pending, and a message that fits goes through
    out = e.encode(data[100:bs]) + e.flush()
    assert _unzstd_stream(out) == data[:bs]
    e.close()
    e = H.ZstdEncoder(block_size=bs, max_encode_size=need)
    out = e.encode(data) + e.flush()
    assert _unzstd_stream(out) == data
    e.close()
    e = H.ZstdEncoder(block_size=bs, max_encode_size=_bound(50) - 1)
    assert e.encode(b"q" * 49) == b""  # 49 pending bytes fit (the bound falls with n below 128 KiB's slope)
    e.close()


def test_embedded_channel(H, oracle):
    data = oracle.textgen_chunk(1, 100_000)
    enc = H.ZstdEncoder(block_size=32768)
    ch = H.EmbeddedChannel(enc)
    assert ch.write_outbound(data[:50_000], data[50_000:])
    out = b""
    while (m := ch.read_outbound()) is not None:
        out += m
    out += enc.flush()
    assert _unzstd_stream(out) == data
    assert ch.finish() is False
    enc.close()
