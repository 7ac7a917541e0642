"""Preset dictionaries: JdkZlibEncoder(level, dictionary), JdkZlibDecoder(dictionary) and both as batcher
jobs.  The yardstick is the machine's zlib (zlib.compressobj / decompressobj with zdict), never the code under
test; the batcher's results are compared with the synchronous handles', ticket by ticket.  Inputs from
tests/deflate_prefix_inputs.py (pinned by tests/test_deflate_prefix_inputs.py)."""
import random
import zlib

import pytest

import deflate_prefix_inputs as P
import inflate_streams as IS

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DICT_MISMATCH = -77
TEXT = IS.big_text(200000, seed=12)


@pytest.fixture(scope="module")
def H():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from netty_amd import handlers
    return handlers


def _messages(tail):
    rng = random.Random(tail)
    sizes = [1, 65536 - tail, 65536 - tail + 1, 70000, 300, 5000]
    return [TEXT[a:a + n] for n in sizes for a in [rng.randrange(0, len(TEXT) - n)]]


def _encode_stream(enc, msgs):
    wire = b"".join(enc.encode(m) for m in msgs)
    return wire + enc.finish_encode()


# ------------------------------------------------------------------------------ encoder
@pytest.mark.parametrize("n", P.DICT_LENS)
def test_encoder_stream(H, n):
    d = P.dictionary(n)
    tail = min(n, 32768)
    for level in ((0, 1, 6, 9, -1) if n in (0, 100, 32768) else (6,)):
        msgs = _messages(tail)
        enc = H.JdkZlibEncoder(compression_level=level, dictionary=d)
        first = enc.encode(msgs[0])
        want = P.zlib_header(level, d)
        assert len(want) == (6 if n else 2) and first[:len(want)] == want, (n, level)
        wire = first
        for k, m in enumerate(msgs[1:], 2):
            wire += enc.encode(m)
            if k in (2, 3):  # the sync-flush property across the first slice's cut
                z = zlib.decompressobj(zdict=d)
                assert z.decompress(wire) == b"".join(msgs[:k]) and not z.eof, (n, level, k)
        wire += enc.finish_encode()
        data = b"".join(msgs)
        z = zlib.decompressobj(zdict=d)
        assert z.decompress(wire) == data and z.eof and z.unused_data == b"", (n, level)
        assert wire[-4:] == zlib.adler32(data).to_bytes(4, "big")
        assert enc.encode(b"after close") == b"after close" and enc.finish_encode() == b""
        enc.close()


@pytest.mark.parametrize("n", P.DICT_LENS)
def test_encoder_close_with_nothing_written(H, n):
    d = P.dictionary(n)
    enc = H.JdkZlibEncoder(compression_level=6, dictionary=d)
    assert enc.encode(b"") == b""
    out = enc.finish_encode()
    assert out == P.zlib_header(6, d) + b"\x03\x00" + (1).to_bytes(4, "big")
    z = zlib.decompressobj(zdict=d)
    assert z.decompress(out) == b"" and z.eof
    enc.close()


def test_far_text_of_a_long_dictionary_still_round_trips(H):
    d, msg = P.far_dictionary()
    enc = H.JdkZlibEncoder(dictionary=d)
    wire = _encode_stream(enc, [msg, msg])
    assert wire[:6] == P.zlib_header(6, d)
    z = zlib.decompressobj(zdict=d)
    assert z.decompress(wire) == msg + msg and z.eof
    enc.close()


def test_the_dictionary_helps(H):
    d = P.slot_clean(2048, 9)
    with_d, without = H.JdkZlibEncoder(compression_level=6, dictionary=d), H.JdkZlibEncoder(compression_level=6)
    a, b = _encode_stream(with_d, [d]), _encode_stream(without, [d])
    assert zlib.decompressobj(zdict=d).decompress(a) == d and zlib.decompress(b) == d
    print(f"2 KiB drawn from its dictionary: {len(a)} bytes against {len(b)} without")
    assert len(a) < len(b)
    with_d.close()
    without.close()


def test_constructors_refuse_what_the_reference_refuses(H):
    from netty_amd import _lib
    L = _lib.load()
    assert not L.nx_zlib_encoder_new_dict(6, None, 0) and not L.nx_zlib_decoder_new_dict(None, 0, 0)
    assert not L.nx_zlib_encoder_new_dict(10, b"abc", 3) and not L.nx_zlib_decoder_new_dict(b"abc", 3, -1)
    for w in (H.ZlibWrapper.GZIP, H.ZlibWrapper.NONE):
        with pytest.raises(ValueError):
            H.JdkZlibEncoder(w, 6, dictionary=b"abc")
        with pytest.raises(ValueError):
            H.JdkZlibDecoder(w, dictionary=b"abc")
    with pytest.raises(ValueError):
        H.JdkZlibDecoder(H.ZlibWrapper.ZLIB, decompress_concatenated=True, dictionary=b"abc")


# ------------------------------------------------------------------------------ decoder
def _zstream(data, d, level=6):
    c = zlib.compressobj(level, zdict=d) if d is not None else zlib.compressobj(level)
    return c.compress(data) + c.flush()


@pytest.mark.parametrize("n,level", [(1, 1), (3, 6), (100, 9), (32768, 6), (40000, 1)])
def test_decoder_reads_zlib_streams(H, n, level):
    d = P.dictionary(n)
    data = (d[-2000:] + TEXT[:3000] + d[:1500]) * 2
    z = _zstream(data, d, level)
    assert z[1] & 0x20
    for step in (len(z), 7, 1):
        if step == 1:
            z1 = _zstream(data[:600], d, level)
            dec, got = H.JdkZlibDecoder(dictionary=d), b""
            for i in range(len(z1)):
                got += b"".join(dec.channel_read(z1[i:i + 1]))
            assert got == data[:600] and dec.is_closed()
        else:
            dec = H.JdkZlibDecoder(dictionary=d)
            got = b"".join(b"".join(dec.channel_read(z[i:i + step])) for i in range(0, len(z), step))
            assert got == data and dec.is_closed(), (n, step)
        dec.close()


def test_decoder_without_fdict_and_max_allocation(H):
    d = P.dictionary(100)
    dec = H.JdkZlibDecoder(dictionary=d)
    assert b"".join(dec.channel_read(zlib.compress(TEXT[:5000]))) == TEXT[:5000] and dec.is_closed()
    dec.close()
    # max_allocation behaves as without a dictionary
    for make, stream in ((lambda m: H.JdkZlibDecoder(max_allocation=m, dictionary=d), _zstream(TEXT[:5000], d)),
                         (lambda m: H.JdkZlibDecoder(max_allocation=m), zlib.compress(TEXT[:5000]))):
        ok = make(5000)
        assert ok.channel_read(stream) == [TEXT[:5000]]
        small = make(4999)
        with pytest.raises(H.DecompressionException, match="Decompression buffer has reached maximum size: 4999"):
            small.channel_read(stream)
        assert small.is_closed()


def test_wrong_dictionary(H):
    d, other = P.dictionary(100), P.dictionary(100, seed=6)
    z = _zstream(TEXT[:5000], d)
    with pytest.raises(zlib.error):
        zlib.decompressobj(zdict=other).decompress(z)
    dec = H.JdkZlibDecoder(dictionary=other)
    with pytest.raises(H.DecoderException) as e:
        dec.channel_read(z)
    assert not isinstance(e.value, H.DecompressionException) and e.value.status == DICT_MISMATCH and e.value.decoded == []
    assert dec.channel_read(z) == [] and dec.readable_bytes() == 0  # later reads are skipped
    # without a dictionary the stream still fails as before
    with pytest.raises(H.DecompressionException, match="unable to set dictionary as non was specified"):
        H.JdkZlibDecoder().channel_read(z)


def _crafted(d, dist):
    """a zlib stream whose first token is a match of 3 bytes at `dist`, then the Adler32 of what that gives"""
    bw = IS.BitWriter()
    IS.fixed(bw, [(3, dist)], final=True)
    window = bytearray(d)
    for _ in range(3):
        window.append(window[-dist] if dist <= len(window) else 0)
    return P.zlib_header(6, d) + bw.done() + zlib.adler32(bytes(window[len(d):])).to_bytes(4, "big")


@pytest.mark.parametrize("n", [1, 32768])
def test_crafted_first_match_into_the_dictionary(H, n):
    d = P.dictionary(n) if n > 1 else b"q"
    good, bad = _crafted(d, n), _crafted(d, n + 1)
    want = zlib.decompressobj(zdict=d).decompress(good)
    assert want == (d[:3] if n >= 3 else d * 3)
    dec = H.JdkZlibDecoder(dictionary=d)
    assert b"".join(dec.channel_read(good)) == want and dec.is_closed()
    if n < 32768:  # (a distance of 32769 does not exist in deflate)
        with pytest.raises(zlib.error, match="invalid distance too far back"):
            zlib.decompressobj(zdict=d).decompress(bad)
        dec = H.JdkZlibDecoder(dictionary=d)
        with pytest.raises(H.DecompressionException, match="decompression failure") as e:
            dec.channel_read(bad)
        assert e.value.status == -70 and H._lib.status_string(-70) == "invalid distance too far back"


# ------------------------------------------------------------------------------ batcher
def test_batcher_channels_with_and_without_dictionaries(H):
    rng = random.Random(4)
    dicts = [P.dictionary(100), P.dictionary(32768), P.dictionary(40000), None]
    levels = [6, 1, 9, 0, 6, -1, 1, 6]
    chans = []
    for c in range(8):
        d = dicts[c % 4]
        make = lambda d=d, lv=levels[c]: H.JdkZlibEncoder(compression_level=lv, dictionary=d)
        sizes = [(300, 70000), (40000, 1), (65536 - 100, 2000), (5, 140000)][c % 4]
        msgs = []
        for n in sizes:
            src = d if d is not None and n <= len(d) and c % 2 else TEXT
            a = rng.randrange(0, len(src) - n + 1)
            msgs.append(src[a:a + n])
        chans.append((d, make, msgs))
    b = H.Batcher()
    encs = [make() for _, make, _ in chans]
    tickets = [[] for _ in chans]
    for r in range(2):  # two flushes of encode jobs, then the closes
        for i, (d, make, msgs) in enumerate(chans):
            tickets[i].append(b.submit_encode(encs[i], msgs[r]))
        b.flush()
    for i in range(len(chans)):
        tickets[i].append(b.submit_encode(encs[i], b"", op=2))
    b.flush()
    streams = []
    for i, (d, make, msgs) in enumerate(chans):
        s = make()
        want = [s.encode(msgs[0]), s.encode(msgs[1]), s.finish_encode()]
        got = []
        for t in tickets[i]:
            b.wait(t)
            got.append(b"".join(b.result(t)))
        assert got == want, i
        wire = b"".join(got)
        z = zlib.decompressobj(zdict=d) if d is not None else zlib.decompressobj()
        assert z.decompress(wire) == msgs[0] + msgs[1] and z.eof, i
        assert wire[:2] == P.zlib_header(levels[i], d)[:2] and bool(wire[1] & 0x20) == (d is not None)
        streams.append(wire)
        s.close()
    # the streams through decoder jobs, two submits each; channel 2 has the wrong dictionary
    decs = [H.JdkZlibDecoder(dictionary=(dicts[0] if i == 2 else d)) if (d is not None or i == 2) else H.JdkZlibDecoder()
            for i, (d, _, _) in enumerate(chans)]
    dt = [[] for _ in chans]
    for half in range(2):
        for i, wire in enumerate(streams):
            cut = 3 if i % 2 else len(wire) // 2  # (a cut inside the header on the odd channels)
            dt[i].append(b.submit_decode(decs[i], wire[:cut] if half == 0 else wire[cut:]))
        b.flush()
    for i, (d, _, msgs) in enumerate(chans):
        got, failed = b"", None
        for t in dt[i]:
            b.wait(t)
            try:
                got += b"".join(b.result(t))
            except H.DecoderException as e:
                failed = e
        if i == 2:
            assert failed is not None and failed.status == DICT_MISMATCH and not isinstance(failed, H.DecompressionException)
            assert got == b""
        else:
            assert failed is None and got == msgs[0] + msgs[1] and decs[i].is_closed(), i
    for h in encs + decs:
        h.close()
