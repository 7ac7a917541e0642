"""GPU tests of the ZstdDecoder handle (handlers.ZstdDecoder over nx_zstd_decoder_*): whole frames out of a
cumulation fed in any pieces, skippable frames, content checksums, maximumAllocationSize, the CORRUPTED
state.  Expected outputs are the sources libzstd compressed (tests/zstd_decode_inputs.py)."""
import pytest

import zstd_checksum_inputs as K
import zstd_decode_inputs as I
import zstd_frames as Z
import zstd_handbuilt as HB

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
pa = pytest.importorskip("pyarrow")
pytest.importorskip("xxhash")


@pytest.fixture(scope="module")
def H():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from netty_amd import handlers
    return handlers


@pytest.fixture(scope="module")
def parts(oracle):
    """the stream of the split tests as (bytes, what they regenerate): a skippable frame, a small frame, an
    empty frame, a checksummed frame, a frame without content size"""
    by = {(c.kind, c.n, c.level): c for c in I.libzstd_frames(oracle)}
    small, summed, unsized = by["text", 300, 3], by["skew", 1024, 19], by["two", 1024, 3]
    empty = pa.Codec("zstd").compress(b"").to_pybytes()
    assert Z.parse_frame(empty).content_size == 0
    return [(K.skippable(b"skip me", 3), b""), (small.frame, small.data), (empty, b""),
            (K.with_checksum(summed.frame, summed.data), summed.data), (K.without_content_size(unsized.frame), unsized.data)]


def _decoder(H, *a):
    return H.ZstdDecoder(*a)


def _feed(d, stream, cuts, parts):
    """feed stream[cuts[i-1]:cuts[i]] call by call; after each call what has been delivered is exactly the
    output of the frames that are complete, and the cumulation holds the bytes of the unfinished frame"""
    ends, at = [0], 0
    for f, _ in parts:
        at += len(f)
        ends.append(at)
    got, prev = b"", 0
    for cut in list(cuts) + [len(stream)]:
        if cut == prev:
            continue
        msgs = d.channel_read(stream[prev:cut])
        assert all(msgs), "an empty message was delivered"
        got += b"".join(msgs)
        prev = cut
        done = max(k for k, e in enumerate(ends) if e <= cut)
        assert got == b"".join(w for _, w in parts[:done]), (cut, done)
        assert d.readable_bytes() == cut - ends[done], cut
    return got


def test_round_trip_with_the_encoder(H):
    msg = bytes(range(256)) * 2 + b"netty on the gpu " * 11  # 699 bytes: three blocks of 256
    enc = H.EmbeddedChannel(H.ZstdEncoder(block_size=256))
    enc.write_outbound(msg)
    wire = enc.read_outbound() + enc.handler.flush()
    assert [f.content_size for f in Z.parse_frames(wire)] == [256, 256, 187]
    d = _decoder(H)
    try:
        ch = H.EmbeddedChannel(d)
        assert ch.write_inbound(wire)
        out = []
        while (m := ch.read_inbound()) is not None:
            out.append(m)
        assert b"".join(out) == msg and [len(m) for m in out] == [256, 256, 187]
        assert d.readable_bytes() == 0
    finally:
        d.close()
        enc.handler.close()


def test_stream_in_any_pieces(H, parts):
    stream = b"".join(f for f, _ in parts)
    want = b"".join(w for _, w in parts)
    bounds, at = [], 0
    for f, _ in parts:
        at += len(f)
        bounds.append(at)
    ways = [[], list(range(1, len(stream)))]  # whole; one byte per call
    ways += [[b + k] for b in bounds[:-1] for k in (-1, 0, 1)] + [[bounds[-1] - 1]]
    ways.append([b - 1 for b in bounds])
    for cuts in ways:
        d = _decoder(H)
        try:
            assert _feed(d, stream, cuts, parts) == want, cuts[:4]
        finally:
            d.close()


def test_maximum_allocation_size(H, oracle):
    c = next(c for c in I.libzstd_frames(oracle) if (c.kind, c.n, c.level) == ("text", 300, 3))
    for size, lens in ((0, [300]), (1, [1] * 300), (100, [100, 100, 100]), (128, [128, 128, 44]), (300, [300]), (1 << 20, [300])):
        d = _decoder(H, size)
        try:
            msgs = d.channel_read(c.frame + c.frame)
            assert [len(m) for m in msgs] == lens + lens, size
            assert b"".join(msgs) == c.data + c.data
        finally:
            d.close()
    d = _decoder(H)  # the default: 4 MiB
    try:
        assert d.maximum_allocation_size == 4 * 1024 * 1024
        big = next(c for c in I.libzstd_frames(oracle) if (c.kind, c.n, c.level) == ("text", 1048576, 1))
        assert d.channel_read(big.frame) == [big.data]
    finally:
        d.close()


def test_constructor_refuses_a_negative_size(H):
    with pytest.raises(ValueError, match="maximumAllocationSize"):
        H.ZstdDecoder(-1)


def _bad_frames(oracle):
    c = next(c for c in I.libzstd_frames(oracle) if (c.kind, c.n, c.level) == ("skew", 1024, 19))
    m = HB.malformed()
    return {"wrong_checksum": (K.wrong_checksum(K.with_checksum(c.frame, c.data), 1, 6), -88, "Restored data doesn't match checksum"),
            "corrupt_block": (m["offset_beyond"][0], -86, "Data corruption detected"),
            "unknown_magic": (m["unknown_magic"][0], -84, "Unknown frame descriptor"),
            "window_too_large": (m["window_too_large"][0], -81, "Frame requires too much memory for decoding"),
            "dictionary_id": (m["dictionary_id"][0], -82, "Dictionary mismatch")}


@pytest.mark.parametrize("which", ["wrong_checksum", "corrupt_block", "unknown_magic", "window_too_large", "dictionary_id"])
def test_failure_delivers_what_came_before_and_corrupts_the_decoder(H, oracle, which):
    bad, status, text = _bad_frames(oracle)[which]
    good = next(c for c in I.libzstd_frames(oracle) if (c.kind, c.n, c.level) == ("text", 300, 3))
    d = _decoder(H)
    try:
        with pytest.raises(H.DecompressionException) as e:
            d.channel_read(good.frame + bad + good.frame)
        assert str(e.value) == text and e.value.status == status
        assert e.value.decoded == [good.data]
        for more in (good.frame, b"anything", good.frame + good.frame):  # CORRUPTED: swallowed, nothing comes out
            assert d.channel_read(more) == [] and d.readable_bytes() == 0
    finally:
        d.close()


def test_failure_in_a_later_call(H, oracle):
    bad, status, text = _bad_frames(oracle)["wrong_checksum"]
    good = next(c for c in I.libzstd_frames(oracle) if (c.kind, c.n, c.level) == ("text", 300, 3))
    d = _decoder(H)
    try:
        assert d.channel_read(good.frame + bad[:-1]) == [good.data]
        assert d.readable_bytes() == len(bad) - 1
        with pytest.raises(H.DecompressionException, match="checksum") as e:
            d.channel_read(bad[-1:] + good.frame)
        assert e.value.decoded == [] and e.value.status == status
        assert d.channel_read(good.frame) == []
    finally:
        d.close()


def test_all_frames_of_a_read_are_one_launch(H, oracle):
    a, b = [c for c in I.libzstd_frames(oracle) if c.level == 3 and c.n == 5000 and c.kind in ("text", "skew")]
    d = _decoder(H, 0)
    try:
        assert d.stats() == {"launches": 0, "frames": 0}
        assert d.channel_read(a.frame + K.skippable(b"between") + b.frame + a.frame[:10]) == [a.data, b.data]
        assert d.stats() == {"launches": 1, "frames": 2}
        assert d.channel_read(a.frame[10:20]) == [] and d.readable_bytes() == 20  # no frame completed: no launch
        assert d.stats() == {"launches": 1, "frames": 2}
        assert d.channel_read(a.frame[20:] + b.frame + K.skippable(b"") + a.frame + b.frame) == [a.data, b.data, a.data, b.data]
        assert d.stats() == {"launches": 2, "frames": 6}
        assert d.channel_read(K.skippable(b"only this")) == [] and d.readable_bytes() == 0
        assert d.stats() == {"launches": 2, "frames": 6}
    finally:
        d.close()
