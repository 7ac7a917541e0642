"""JdkZlibEncoder / JdkZlibDecoder as batcher jobs (include/netty_amd.h section 3, DESIGN.md §4 "zlib jobs
on the batcher").  The references are the synchronous handles and Python's zlib, never the batcher path:
per ticket an encoder job's bytes equal a fresh synchronous handle's for the same call sequence, and a
decoder job's messages, status, error text and is_closed() equal those of the k-th channel_read of a fresh
synchronous decoder fed the same slices."""
import gzip
import random
import zlib

import pytest

import inflate_streams as IS

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def H():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from netty_amd import handlers
    return handlers


WBITS = {"ZLIB": 15, "GZIP": 31, "NONE": -15}
TEXT = IS.big_text(200000, seed=11)


def _data(rng, n, text=None):
    if text is None:
        text = rng.random() < 0.7
    if text:
        at = rng.randrange(0, len(TEXT) - n + 1)
        return TEXT[at:at + n]
    return rng.randbytes(n)


def _msgs(rng, k):  # the size mix of tests/test_gpu_batcher_alt.py::_msgs
    return [_data(rng, rng.choice((0, 1, rng.randint(2, 40), rng.randint(100, 5000), rng.randint(20000, 140000)))) for _ in range(k)]


def _deflate(data, wbits, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, wbits)
    return c.compress(data) + c.flush()


def _cut(rng, z, forced=()):
    """1-6 slices of z; `forced` cut points (inside a header, trailer, footer) are kept when they fit"""
    k = rng.randint(1, 6)
    cuts = sorted(set([c for c in forced if 0 < c < len(z)][:k - 1] + [rng.randrange(1, len(z)) for _ in range(rng.randint(0, k - 1))]))[:k - 1]
    edges = [0] + sorted(cuts) + [len(z)]
    return [z[a:b] for a, b in zip(edges, edges[1:]) if b > a]


def _sync_calls(H, make, slices):
    """what the k-th channel_read of a fresh synchronous decoder gives: (bytes, status, text, bytes decoded before the
    failure, closed)"""
    d = make()
    out = []
    for s in slices:
        try:
            out.append((b"".join(d.channel_read(s)), 0, None, None, d.is_closed()))
        except H.DecompressionException as e:
            out.append((None, e.status, str(e), b"".join(e.decoded), d.is_closed()))
    return out


def _ticket(H, b, d, t):
    b.wait(t)
    try:
        return (b"".join(b.result(t)), 0, None, None, d.is_closed())
    except H.DecompressionException as e:
        return (None, e.status, str(e), b"".join(e.decoded), d.is_closed())


# ------------------------------------------------------------------------------------------ 1. encoder jobs
def test_encoder_jobs_equal_the_synchronous_handle(H):
    rng = random.Random(1)
    b = H.Batcher()
    chans = []
    for c in range(24):
        wrapper, level = ("ZLIB", "GZIP", "NONE")[c % 3], (0, 6)[(c // 3) % 2]
        msgs = _msgs(rng, rng.randint(1, 5))
        if c == 0:
            msgs[0] = _data(rng, 140000)  # three slices
        if c == 1:
            msgs[0] = _data(rng, 70000)   # two
        calls = [(m, 0) for m in msgs]
        if c % 2:
            calls[-1] = (msgs[-1], 2)  # the last message closes
        else:
            calls.append((b"", 2))     # an empty close job
        calls.append((b"after the close", 0))  # passes through
        chans.append((wrapper, level, H.JdkZlibEncoder(H.ZlibWrapper[wrapper], level), calls, []))
    for r in range(max(len(ch[3]) for ch in chans)):
        for wrapper, level, e, calls, tickets in chans:
            if r < len(calls):
                tickets.append(b.submit_encode(e, calls[r][0], op=calls[r][1]))
        if r % 3 == 2:
            b.flush()
    b.flush()
    slices = set()
    for wrapper, level, e, calls, tickets in chans:
        s = H.JdkZlibEncoder(H.ZlibWrapper[wrapper], level)
        stream = b""
        for (m, op), t in zip(calls, tickets):
            b.wait(t)
            res = b.result(t)
            assert len(res) == 1
            want = s.encode(m) + (s.finish_encode() if op == 2 else b"")
            assert res[0] == want, (wrapper, level, len(m), op)
            stream += res[0]
            slices.add(-(-len(m) // 65536))
        assert stream.endswith(b"after the close")
        z = zlib.decompressobj(WBITS[wrapper])
        assert z.decompress(stream[:-len(b"after the close")]) == b"".join(m for m, _ in calls[:-1]) and z.eof
    assert {1, 2, 3} <= slices


# ------------------------------------------------------------------------------------------ 2. decoder jobs
def _decoder_channels(H, rng):
    """32 channels: (make decoder, slices)"""
    chans = []
    for c in range(32):
        kind = ("ZLIB", "GZIP2", "NONE", "ZON")[c % 4]
        level = (0, 1, 6, 9)[(c // 4) % 4]
        data = _data(rng, rng.choice((0, 1, 37, 3000, 70000)), text=c % 8 < 6)
        forced = []
        if kind == "ZLIB" or (kind == "ZON" and c % 8 == 3):
            z = _deflate(data, 15, level)
            forced = [1, len(z) - 2, len(z) - 4]  # inside the header, the trailer
            make = (lambda: H.JdkZlibDecoder(H.ZlibWrapper.ZLIB)) if kind == "ZLIB" else (lambda: H.JdkZlibDecoder(H.ZlibWrapper.ZLIB_OR_NONE))
        elif kind == "GZIP2":
            z1 = _deflate(data, 31, level)
            z = z1 + _deflate(_data(rng, 500), 31, level)
            forced = [5, len(z1) - 3, len(z1) + 4, len(z) - 5]  # the header, the footer, the second member's header, its footer
            make = lambda: H.JdkZlibDecoder(H.ZlibWrapper.GZIP, True)
        else:
            z = _deflate(data, -15, level)
            make = (lambda: H.JdkZlibDecoder(H.ZlibWrapper.NONE)) if kind == "NONE" else (lambda: H.JdkZlibDecoder(H.ZlibWrapper.ZLIB_OR_NONE))
        rng.shuffle(forced)
        slices = _cut(rng, z, forced)
        if c % 5 == 0 and len(z) > 3:
            slices = [z[:1], z[1:2], z[2:]]  # 1-byte slices
        chans.append((make, slices))
    return chans


@pytest.fixture(scope="module")
def decoder_cases(H):
    chans = _decoder_channels(H, random.Random(2))
    return chans, [_sync_calls(H, make, slices) for make, slices in chans]


@pytest.mark.parametrize("mode", ["all_before_the_first_flush", "flush_without_wait"])
def test_decoder_jobs_per_ticket_equivalence(H, decoder_cases, mode):
    chans, want = decoder_cases
    b = H.Batcher()
    decs = [make() for make, _ in chans]
    tickets = [[] for _ in chans]
    for r in range(max(len(s) for _, s in chans)):
        for c, (_, slices) in enumerate(chans):
            if r < len(slices):
                tickets[c].append(b.submit_decode(decs[c], slices[r]))
        if mode == "flush_without_wait":
            b.flush()
    b.flush()
    for c, d in enumerate(decs):
        for k, t in enumerate(tickets[c]):
            got = _ticket(H, b, d, t)
            assert got[:4] == want[c][k][:4], (c, k)
            # a later ticket of the channel may be complete already (a held job that needed no body step), so the
            # handle is closed no later than the synchronous one, and equally closed after the last ticket
            assert got[4] >= want[c][k][4] and (k + 1 < len(tickets[c]) or got[4] == want[c][k][4]), (c, k)
        assert d.readable_bytes() == 0


# ------------------------------------------------------------------------------------------ 3. continuation
def test_a_job_larger_than_any_output_room_continues(H):
    big = bytes(3 << 20) + TEXT[:1000]
    small = [TEXT[100 * i:100 * i + 100] for i in range(8)]
    b = H.Batcher()
    f0 = b.stats()["flushes"]
    dbig = H.JdkZlibDecoder(H.ZlibWrapper.ZLIB)
    z = zlib.compress(big)
    assert len(z) < 16384
    tb = b.submit_decode(dbig, z)
    ds = [H.JdkZlibDecoder(H.ZlibWrapper.ZLIB) for _ in small]
    ts = [b.submit_decode(d, zlib.compress(m)) for d, m in zip(ds, small)]
    b.flush()
    assert b.stats()["flushes"] == f0 + 1
    b.wait(ts[0])  # applies the first flush (and launches the big job's next round)
    for d, t, m in zip(ds, ts, small):  # the small ones are complete after the first flush: no further wait
        assert b.poll(t) and b.result(t) == [m] and d.is_closed()
    b.wait(tb)
    assert b.stats()["flushes"] > f0 + 1
    assert b"".join(b.result(tb)) == big and dbig.is_closed()


# ------------------------------------------------------------------------------------------ 4. history
@pytest.mark.parametrize("interleaved", [False, True])
def test_matches_reach_into_the_carried_history(H, interleaved):
    rng = random.Random(4)
    data = rng.randbytes(30000) * 4
    z = _deflate(data, 15, 9)
    assert len(z) < 32000  # the repeats are matches at distance 30 000, about 1 000 bytes at the end
    cuts = [len(z) // 3, len(z) - 500]  # the third job holds only such matches, the second mostly literals
    parts = [z[:cuts[0]], z[cuts[0]:cuts[1]], z[cuts[1]:]]
    other = rng.randbytes(20000) * 3
    zo = _deflate(other, 31, 9)
    oparts = [zo[:len(zo) // 3], zo[len(zo) // 3:len(zo) - 300], zo[len(zo) - 300:]]
    b = H.Batcher()
    d, do = H.JdkZlibDecoder(H.ZlibWrapper.ZLIB), H.JdkZlibDecoder(H.ZlibWrapper.GZIP)
    got, goto = b"", b""
    for p, po in zip(parts, oparts):
        to = b.submit_decode(do, po) if interleaved else None
        t = b.submit_decode(d, p)
        b.flush()
        b.wait(t)
        got += b"".join(b.result(t))
        if interleaved:
            b.wait(to)
            goto += b"".join(b.result(to))
    assert got == data and d.is_closed()
    if interleaved:
        assert goto == other and do.is_closed()


# ------------------------------------------------------------------------------------------ 5. failures
def _failing_streams():
    out = [(name, "NONE", z) for name, (z, _) in sorted(IS.crafted_invalid().items())]
    good = zlib.compress(TEXT[:3000])
    out.append(("adler_mismatch", "ZLIB", good[:-1] + bytes([good[-1] ^ 1])))
    gz = gzip.compress(TEXT[:3000])
    out.append(("gzip_crc_mismatch", "GZIP", gz[:-8] + bytes([gz[-8] ^ 1]) + gz[-7:]))
    c = zlib.compressobj(6, zlib.DEFLATED, 15, zdict=b"dictionary")
    out.append(("fdict", "ZLIB", c.compress(TEXT[:3000]) + c.flush()))
    return out


def test_failures_equal_the_synchronous_handle(H):
    cases = _failing_streams()
    b = H.Batcher()
    decs, tickets, others = [], [], []
    for name, wrapper, z in cases:
        d = H.JdkZlibDecoder(H.ZlibWrapper[wrapper])
        decs.append(d)
        tickets.append((b.submit_decode(d, z), b.submit_decode(d, b"more bytes")))
        o = H.JdkZlibDecoder(H.ZlibWrapper.ZLIB)  # a healthy neighbour in the same batch
        others.append((o, b.submit_decode(o, zlib.compress(name.encode() * 50)), name.encode() * 50))
    b.flush()
    for (name, wrapper, z), d, (t1, t2) in zip(cases, decs, tickets):
        (want,) = _sync_calls(H, lambda: H.JdkZlibDecoder(H.ZlibWrapper[wrapper]), [z])
        assert want[1] != 0, name
        assert _ticket(H, b, d, t1) == want, name
        b.wait(t2)
        assert b.result(t2) == [], name  # skips what follows
    for o, t, m in others:
        b.wait(t)
        assert b"".join(b.result(t)) == m and o.is_closed()


def test_max_allocation(H):
    z = zlib.compress(TEXT[:5000])
    make = lambda: H.JdkZlibDecoder(H.ZlibWrapper.ZLIB, False, 1000)
    (want,) = _sync_calls(H, make, [z])
    assert want[2].startswith("Decompression buffer has reached maximum size: 1000") and want[3] == b"" and want[4]
    b = H.Batcher()
    d = make()
    assert _ticket(H, b, d, b.submit_decode(d, z)) == want
    d = H.JdkZlibDecoder(H.ZlibWrapper.ZLIB, False, 5000)  # within the limit: one message
    t = b.submit_decode(d, z)
    b.wait(t)
    assert b.result(t) == [TEXT[:5000]] and d.is_closed()


# ------------------------------------------------------------------------------------------ 6. launches
def test_launches_per_flush_do_not_depend_on_the_number_of_jobs(H):
    b = H.Batcher()
    b.reserve(1 << 6)  # the deflate workspace up front
    msg = TEXT[:2000]
    z = zlib.compress(msg)

    def decode_flush(n):
        ds = [H.JdkZlibDecoder(H.ZlibWrapper.ZLIB) for _ in range(n)]
        l0 = b.stats()["launches"]
        ts = [b.submit_decode(d, z) for d in ds]
        b.flush()
        grown = b.stats()["launches"] - l0
        for t in ts:
            b.wait(t)
            assert b.result(t) == [msg]
        return grown

    def encode_flush(n):
        es = [H.JdkZlibEncoder(H.ZlibWrapper.GZIP, 6) for _ in range(n)]
        l0 = b.stats()["launches"]
        ts = [b.submit_encode(e, msg, op=2) for e in es]
        b.flush()
        grown = b.stats()["launches"] - l0
        for t in ts:
            b.wait(t)
            assert gzip.decompress(b.result(t)[0]) == msg
        return grown

    assert decode_flush(4) == decode_flush(64) > 0
    assert encode_flush(4) == encode_flush(64) > 0


# ------------------------------------------------------------------------------------------ 7. mixed batch
def test_one_flush_of_snappy_lz4_and_zlib_jobs(H):
    b = H.Batcher()
    msg = TEXT[:50000]
    se, le, ze = H.SnappyFrameEncoder(), H.Lz4FrameEncoder(), H.JdkZlibEncoder(H.ZlibWrapper.ZLIB, 6)
    snappy_frames = H.SnappyFrameEncoder().encode(msg)
    lz4_frames = H.Lz4FrameEncoder()
    lz4_bytes = lz4_frames.encode(msg) + lz4_frames.finish_encode()
    sd, ld, zd = H.SnappyFrameDecoder(), H.Lz4FrameDecoder(), H.JdkZlibDecoder(H.ZlibWrapper.ZLIB)
    f0 = b.stats()["flushes"]
    t = {"se": b.submit_encode(se, msg), "le": b.submit_encode(le, msg, op=2), "ze": b.submit_encode(ze, msg, op=2),
         "sd": b.submit_decode(sd, snappy_frames), "ld": b.submit_decode(ld, lz4_bytes), "zd": b.submit_decode(zd, zlib.compress(msg))}
    b.flush()
    got = {}
    for k, v in t.items():
        b.wait(v)
        got[k] = b"".join(b.result(v))
    assert b.stats()["flushes"] == f0 + 1
    assert got["se"] == snappy_frames and got["le"] == lz4_bytes
    assert zlib.decompress(got["ze"]) == msg
    s = H.JdkZlibEncoder(H.ZlibWrapper.ZLIB, 6)
    assert got["ze"] == s.encode(msg) + s.finish_encode()
    assert got["sd"] == got["ld"] == got["zd"] == msg


# ------------------------------------------------------------------------------------------ 8. lifetime
def test_handles_closed_between_submit_and_flush(H):
    b = H.Batcher()
    msg = TEXT[:70000]
    e, d = H.JdkZlibEncoder(H.ZlibWrapper.GZIP, 6), H.JdkZlibDecoder(H.ZlibWrapper.GZIP)
    te = b.submit_encode(e, msg, op=2)
    td = b.submit_decode(d, gzip.compress(msg))
    e.close()
    d.close()
    b.flush()
    b.wait(te)
    b.wait(td)
    assert gzip.decompress(b.result(te)[0]) == msg
    assert b"".join(b.result(td)) == msg


def test_synchronous_calls_on_batcher_handles(H):
    b = H.Batcher()
    d = H.JdkZlibDecoder(H.ZlibWrapper.ZLIB)
    t = b.submit_decode(d, zlib.compress(b"abc"))
    with pytest.raises(RuntimeError):
        d.channel_read(b"x")
    b.wait(t)
    assert b.result(t) == [b"abc"]
    with pytest.raises(RuntimeError):  # a batcher decoder stays a batcher decoder
        d.channel_read(b"x")
    e, s = H.JdkZlibEncoder(H.ZlibWrapper.ZLIB, 6), H.JdkZlibEncoder(H.ZlibWrapper.ZLIB, 6)
    a, c = TEXT[:3000], TEXT[3000:9000]
    t = b.submit_encode(e, a)
    with pytest.raises(H.CompressionException):
        e.encode(c)
    with pytest.raises(H.CompressionException):
        e.finish_encode()
    b.wait(t)
    first = b.result(t)[0]
    assert first == s.encode(a)
    rest = e.encode(c) + e.finish_encode()  # the same stream goes on
    assert rest == s.encode(c) + s.finish_encode()
    assert zlib.decompress(first + rest) == a + c
