"""GPU tests of handlers.Bzip2Decoder (nx_bzip2_decoder_*): the 40-block stream of tests/bzip2_handbuilt.py fed
whole and in pieces, decoy streams (tests/bzip2_decoys.py) fed byte by byte, the failing and truncated variants,
the header's two messages, and the round trip from handlers.Bzip2Encoder."""
import random

import pytest

import bzip2_decoys as D
import bzip2_handbuilt as H
import bzip2_streams as S

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def N():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    import netty_amd
    return netty_amd


@pytest.fixture(scope="module")
def forty(N):
    texts, specs, stream, positions = H.multi_block()
    blocks, ends = S.find_magics(stream)
    assert blocks == list(positions) and len(ends) == 1  # no decoy: the condition of "every block attempted once"
    from netty_amd import batch
    by = {c.name: c for c in H.group(batch.bzip2_decode_chains(), "streams")}
    return list(texts), stream, positions, by


def _feed(N, stream, cuts):
    """The messages of a fresh decoder fed stream[cuts[k-1]:cuts[k]] in turn, and the decoder."""
    d = N.Bzip2Decoder()
    out, last = [], 0
    for c in list(cuts) + [len(stream)]:
        if c > last:
            out += d.channel_read(stream[last:c])
            last = c
    return out, d


def test_one_call(N, forty):
    texts, stream, positions, by = forty
    out, d = _feed(N, stream, [])
    assert out == texts and d.is_closed() and d.readable_bytes() == 0
    assert d.stats() == {"launches": 1, "blocks_attempted": 40, "blocks_emitted": 40}
    assert d.channel_read(b"more bytes after the end") == [] and d.readable_bytes() == 0  # :328-330


@pytest.mark.parametrize("piece", [1, 7, 64, "magics"])
def test_pieces(N, forty, piece):
    texts, stream, positions, by = forty
    if piece == "magics":
        cuts = sorted({p // 8 + k for p in positions for k in (-1, 0, 1)})
    else:
        cuts = list(range(piece, len(stream), piece))
    out, d = _feed(N, stream, cuts)
    assert out == texts and d.is_closed() and d.readable_bytes() == 0
    st = d.stats()
    assert st["blocks_attempted"] == 40 and st["blocks_emitted"] == 40 and st["launches"] <= 41


def test_decoys_byte_by_byte(N):
    for name, stream, true, decoy_b, decoy_e, data in D.streams():
        out, d = _feed(N, stream, range(1, len(stream)))
        assert b"".join(out) == data and len(out) == len(true) and d.is_closed(), name
        assert len(true) <= d.stats()["blocks_attempted"] <= len(true) + len(decoy_b) + len(decoy_e), (name, d.stats())
        whole, d2 = _feed(N, stream, [])
        assert whole == out and d2.stats()["blocks_attempted"] == len(true), name


def test_failures_and_tails(N, forty):
    texts, stream, positions, by = forty
    out, d = _feed(N, by["blocks40_cut_in_block33"].stream, [])
    assert out == texts[:33] and not d.is_closed() and d.readable_bytes() > 0
    assert d.channel_read(b"") == [] and d.stats()["blocks_attempted"] == 33  # the waiting block is not attempted
    d = N.Bzip2Decoder()
    with pytest.raises(N.DecompressionException, match="^block CRC error$") as e:
        d.channel_read(by["blocks40_block35_wrong_crc"].stream)
    assert e.value.decoded == texts[:35] and e.value.status == S.BLOCK_CRC
    assert d.channel_read(stream) == [] and d.readable_bytes() == 0 and not d.is_closed()  # input discarded
    d = N.Bzip2Decoder()
    with pytest.raises(N.DecompressionException, match="^stream CRC error$") as e:
        d.channel_read(by["blocks40_wrong_stream_crc"].stream)
    assert e.value.decoded == texts
    d = N.Bzip2Decoder()
    with pytest.raises(N.DecompressionException, match="^Unexpected stream identifier contents. Mismatched bzip2 protocol version\\?$"):
        d.channel_read(b"BZx1" + stream[4:])
    d = N.Bzip2Decoder()
    assert d.channel_read(b"BZ") == []
    with pytest.raises(N.DecompressionException, match="^block size is invalid$"):
        d.channel_read(b"h0" + stream[4:])
    d = N.Bzip2Decoder()
    with pytest.raises(N.DecompressionException, match="^bad block header$"):
        d.channel_read(stream[:4] + b"\x00" * 16)
    out, d = _feed(N, by["no_blocks"].stream, [])
    assert out == [] and d.is_closed()
    out, d = _feed(N, by["blocks40_tail"].stream, [])
    assert out == texts and d.is_closed() and d.readable_bytes() == 0  # the trailing bytes are consumed and ignored


def test_runs_that_outgrow_the_first_slot(N):
    """Blocks that expand far beyond their declared size in the final stage: the handle repeats the sequence with a
    larger output slot and delivers the same bytes."""
    import bz2
    data = b"\x00" * 3000000 + b"tail"
    out, d = _feed(N, bz2.compress(data, 1), [])
    assert b"".join(out) == data and d.is_closed() and d.stats()["launches"] >= 2


def test_embedded_channel_and_round_trip(N, oracle):
    rng = random.Random(41)
    text = oracle.textgen_chunk(3, 260000)
    enc = N.EmbeddedChannel(N.Bzip2Encoder(1))
    at = 0
    while at < len(text):  # several writes; three blocks at level 1
        k = rng.randrange(1, 90000)
        enc.write_outbound(text[at:at + k])
        at += k
    wire = b""
    while (m := enc.read_outbound()) is not None:
        wire += m
    wire += enc.handler.finish_encode()
    dec = N.EmbeddedChannel(N.Bzip2Decoder())
    at = 0
    while at < len(wire):  # arbitrary pieces
        k = rng.choice((1, 2, 5, 100, 4000, 30000))
        dec.write_inbound(wire[at:at + k])
        at += k
    got = b""
    while (m := dec.read_inbound()) is not None:
        got += m
    assert got == text and dec.handler.is_closed()
    assert dec.handler.stats()["blocks_emitted"] == dec.handler.stats()["blocks_attempted"] >= 3
