"""GPU tests of the Bzip2Encoder handle (Bzip2Encoder.java:96-228 over nx_bzip2_encode_batch_split).  The stream
is a function of the concatenated input alone, so every way of slicing an input into writes must give the
one-shot host stream (nx_bzip2_encode_host, held against libbz2 by the CPU tests), and each call must hand over
what the reference's bit writer has completed by then: whole 32-bit words."""
import bz2

import pytest

import bzip2_encode_inputs as I
import bzip2_split_inputs as X

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def H():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from netty_amd import handlers
    return handlers


@pytest.fixture(scope="module")
def B():
    from netty_amd import batch
    return batch


@pytest.fixture(scope="module")
def words_by_cut(B):
    """The 32-bit words of the one-shot stream complete once 0, 1, 2 blocks are closed (the header is word 0):
    from the segment encoder on the host, one block at a time."""
    it = X.three_blocks()
    cuts, seg, done, at, words = X.cuts_of(it.data, 1), (X.SEG_FIRST, 0, 0, 0), 0, 0, []
    for k, c in enumerate(cuts[:2]):
        st, piece, seg = B.bzip2_encode_segment_host(it.data[at:c], 1, ((X.SEG_FIRST if k == 0 else 0),) + tuple(seg[1:]))
        assert st == I.OK
        done, at = done + len(piece), c
        words.append(done // 4)
    return [1] + words


def _splits(cuts, n):
    c0, c1 = cuts[0], cuts[1]
    return {
        "one write": [n],
        "single bytes round the first cut": [c0 - 2, c0 - 1, c0, c0 + 1, c0 + 2, n],
        "an empty write": [1000, 1000, c1 + 5, c1 + 5, n],
        "a write holding two cuts": [c0 - 10, c1 + 10, n],
        "a write ending exactly on a cut": [c0, c1, n],
    }


@pytest.mark.parametrize("name", list(_splits([10, 20], 30)))
def test_splits_of_one_input(H, B, words_by_cut, name):
    it = X.three_blocks()
    st, stream = X.three_blocks_stream(B)
    cuts = X.cuts_of(it.data, 1)
    points = _splits(cuts, len(it.data))[name]
    e = H.Bzip2Encoder(1)
    out, at, handed = b"", 0, 0
    for k, p in enumerate(points):
        piece = e.encode(it.data[at:p])
        # a block closes in the write whose last byte fills it: the blocks closed once the input up to p is in
        closed = sum(1 for c in cuts[:2] if c <= p)
        want_words = words_by_cut[closed]
        assert len(piece) == 4 * (want_words - handed), (name, k, p)
        out, at, handed = out + piece, p, want_words
    assert not e.is_closed()
    out += e.finish_encode()
    assert e.is_closed() and st == I.OK and out == stream and bz2.decompress(out) == it.data
    # one launch per write that closed blocks, however many it closed, and one for the close
    writes_closing = len({min(p for p in points if p >= c) for c in cuts[:2]})
    assert e.launches() == writes_closing + 1, name
    e.close()


def test_two_blocks_closed_by_one_write_is_one_launch(H, B):
    it = X.three_blocks()
    cuts = X.cuts_of(it.data, 1)
    e = H.Bzip2Encoder(1)
    assert e.encode(it.data[:100]) == b"BZh1" and e.launches() == 0
    piece = e.encode(it.data[100:cuts[1] + 1])
    assert len(piece) % 4 == 0 and len(piece) > 100000 and e.launches() == 1  # two blocks, one split call
    assert e.encode(it.data[cuts[1] + 1:]) == b"" and e.launches() == 1  # the third block stays open
    assert piece + e.finish_encode() == X.three_blocks_stream(B)[1][4:] and e.launches() == 2
    e.close()


def test_empty_stream_close_and_errors(H):
    e = H.Bzip2Encoder()
    assert e.block_size_multiplier == 9 and not e.is_closed()
    assert e.encode(b"") == b"BZh9" and e.encode(b"") == b""
    assert e.finish_encode() == bz2.compress(b"")[4:] and len(bz2.compress(b"")) == 14
    assert e.is_closed() and e.finish_encode() == b"" and e.is_closed()
    assert e.encode(b"passed through") == b"passed through" and e.encode(b"") == b""
    e.close()
    e = H.Bzip2Encoder(3)  # never written to: the whole empty stream
    assert e.finish_encode() == bz2.compress(b"", 3) and e.finish_encode() == b""
    e.close()
    L = __import__("netty_amd._lib", fromlist=["load"]).load()
    assert not L.nx_bzip2_encoder_new(0) and not L.nx_bzip2_encoder_new(10)
    for bad in (0, 10, -1):
        with pytest.raises(ValueError, match="expected: 1-9"):
            H.Bzip2Encoder(bad)


def test_embedded_channel(H, oracle):
    text = oracle.textgen_chunk(3, 50000)
    enc = H.Bzip2Encoder(1)
    ch = H.EmbeddedChannel(enc)
    assert ch.write_outbound(text[:20000], text[20000:])
    out = b""
    while (m := ch.read_outbound()) is not None:
        out += m
    out += enc.finish_encode()
    assert bz2.decompress(out) == text
    enc.close()
