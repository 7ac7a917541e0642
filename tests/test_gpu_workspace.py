"""GPU tests of the shared device workspaces (csrc/workspace.hpp, include/netty_amd.h NX_WS_*): one
encoder table workspace and one decoder record workspace per device, shared by every stream, held by
batchers and handles from creation, never grown inside a flush, freed with their last owner.

The reference allocates its tables per call (Snappy.java:187-211); these tests pin the resource
behaviour of the GPU replacement, and that a batch capped to a held workspace (a grid narrower than
the batch) still yields the oracle's bytes."""
import gc

import pytest
import torch

pytestmark = pytest.mark.gpu

MiB = 1 << 20


@pytest.fixture(scope="module")
def nx():
    import netty_amd
    return netty_amd


@pytest.fixture(scope="module")
def B():
    from netty_amd import batch
    return batch


def _free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def _collect(B):
    gc.collect()  # handles of earlier tests release their share in __del__
    B.workspaces_trim()


def test_handles_hold_and_release(nx, B):
    _collect(B)
    makers = {
        B.WS_SNAPPY_ENC: lambda: nx.SnappyFrameEncoder(),
        B.WS_DEC_RECORDS: lambda: nx.SnappyFrameDecoder(True),
        B.WS_LZ4_ENC: lambda: nx.Lz4FrameEncoder(),
        B.WS_FASTLZ_ENC: lambda: nx.FastLzFrameEncoder(),
        B.WS_LZF_ENC: lambda: nx.LzfEncoder(),
    }
    for kind, mk in makers.items():
        b0, o0 = B.workspace_info(kind)
        h1, h2 = mk(), mk()
        b1, o1 = B.workspace_info(kind)
        assert o1 == o0 + 2 and b1 > 0 and b1 >= b0, kind
        h1.close()
        assert B.workspace_info(kind) == (b1, o0 + 1), kind  # the second holder keeps it
        h2.close()
        b2, o2 = B.workspace_info(kind)
        assert o2 == o0, kind
        if o0 == 0:
            assert b2 == 0, kind  # the last owner frees it


def test_standalone_growth_kept_until_trim(nx, B):
    _collect(B)
    _, owners = B.workspace_info(B.WS_SNAPPY_ENC)
    if owners:
        pytest.skip("a live handle of another test holds the workspace")
    dev = torch.device("cuda:0")
    chunks = [b"standalone %d " % i * 9 for i in range(2000)]
    inp, off, ln = B.pack(chunks, dev, align=1)
    out, ooff = B.out_slots([B.snappy_max_compressed_length(len(c)) for c in chunks], dev)
    olen, st = B.snappy_encode(inp, off, ln, out, ooff)
    torch.cuda.synchronize()
    assert int((st != 0).sum()) == 0
    b1, o1 = B.workspace_info(B.WS_SNAPPY_ENC)
    assert b1 > 0 and o1 == 0  # grown on demand, kept for the next standalone call
    B.workspaces_trim()
    assert B.workspace_info(B.WS_SNAPPY_ENC) == (0, 0)


def test_handle_message_beyond_its_reservation(nx, B, oracle):
    """A handle holds 1024 table slots; a 1100-slice message runs on that grid (some waves encode two
    slices in turn) without growing it, and its bytes equal the oracle's."""
    _collect(B)
    e = nx.SnappyFrameEncoder()
    held, _ = B.workspace_info(B.WS_SNAPPY_ENC)
    msg = b"".join(oracle.textgen_chunk(900 + i, 32767) for i in range(1100))
    got = e.encode(msg)
    want, _ = oracle.snappy_frame_encode(msg)
    assert got == want
    assert B.workspace_info(B.WS_SNAPPY_ENC)[0] == held
    e.close()


# One stream of 1025 blocks per decoder: 1024 small compressed blocks, then one valid block of more
# records than a record slot holds (16384), which the record parse leaves to the lane-serial decoder.
_SERIAL_MATCHES = 21000


def _small(i):
    return b"netty %04d channel pipeline " % i * 2  # 58 bytes: every codec compresses them


def _lz4_stream(oracle):
    blocks = [oracle.lz4_frame_encode(_small(i), close=False) for i in range(1024)]
    assert all(b[8] & 0xF0 == 0x20 for b in blocks)  # compressed
    # 'a', then _SERIAL_MATCHES four-byte matches at distance 1, then the five last literals
    body = b"\x10a\x01\x00" + b"\x00\x01\x00" * (_SERIAL_MATCHES - 1) + b"\x50aaaaa"
    n = 1 + 4 * _SERIAL_MATCHES + 5
    last = oracle.LZ4_MAGIC + bytes([0x20 | 7]) + len(body).to_bytes(4, "little") + n.to_bytes(4, "little") + bytes(4)
    return b"".join(blocks) + last + body, n


def _fastlz_stream(oracle):
    blocks = [oracle.fastlz_frame_encode(_small(i)) for i in range(1024)]
    assert all(b[3] == 0x01 for b in blocks)  # compressed, no checksum
    body = bytes([0, ord("a")]) + bytes([1 << 5, 0]) * _SERIAL_MATCHES  # test_gpu_fastlz_lzf._fastlz_many_matches
    n = 1 + 3 * _SERIAL_MATCHES
    return b"".join(blocks) + b"FLZ\x01" + len(body).to_bytes(2, "big") + n.to_bytes(2, "big") + body, n


def _lzf_stream(oracle):
    blocks = [oracle.lzf_frame_encode(_small(i)) for i in range(1024)]
    assert all(b[:3] == b"ZV\x01" for b in blocks)  # compressed
    body = bytes([0, ord("a")]) + bytes([0x20, 0]) * _SERIAL_MATCHES  # as test_lzf_decode_record_path_edges
    n = 1 + 3 * _SERIAL_MATCHES
    return b"".join(blocks) + b"ZV\x01" + len(body).to_bytes(2, "big") + n.to_bytes(2, "big") + body, n


@pytest.mark.parametrize("codec", ["lz4", "fastlz", "lzf"])
def test_decoder_call_beyond_its_record_slots(nx, B, oracle, codec):
    """A decoder handle holds 1024 record slots; one call with 1025 blocks runs in sub-batches of 1024
    and 1 without growing them.  The lone block of the second sub-batch is one the record parse leaves
    to the codec's lane-serial decoder, so that runs with base 1024.  The oracle's messages, in order."""
    from oracle import frame_decoders as F
    _collect(B)
    stream, n_last = {"lz4": _lz4_stream, "fastlz": _fastlz_stream, "lzf": _lzf_stream}[codec](oracle)
    want, err = F.run({"lz4": lambda: F.Lz4FrameDecoder(False), "fastlz": lambda: F.FastLzFrameDecoder(False),
                       "lzf": F.LzfDecoder}[codec](), [stream])
    assert err is None and len(want) == 1025 and want[0] == _small(0) and want[-1] == b"a" * n_last
    d = {"lz4": lambda: nx.Lz4FrameDecoder(False), "fastlz": lambda: nx.FastLzFrameDecoder(False), "lzf": nx.LzfDecoder}[codec]()
    held, _ = B.workspace_info(B.WS_DEC_RECORDS)
    assert d.channel_read(stream) == want
    assert B.workspace_info(B.WS_DEC_RECORDS)[0] == held
    d.close()


@pytest.mark.parametrize("codec", ["lzf", "fastlz", "lz4", "lz4hc"])
def test_encoder_message_beyond_its_table_slots(nx, B, oracle, codec):
    """An encoder handle holds 1024 table slots; a message of 1025 units runs on that grid without
    growing it, so one wave encodes two units in turn (the second with the next stamp), and its bytes
    equal the oracle's.  A unit is the largest chunk of LZF and FastLZ, the smallest block of LZ4."""
    _collect(B)
    unit = 64 if codec.startswith("lz4") else 65535
    msg = b"".join(oracle.textgen_chunk(900 + i, unit) for i in range(1025))
    if codec == "lzf":
        e, kind, want = nx.LzfEncoder(), B.WS_LZF_ENC, oracle.lzf_frame_encode(msg)
    elif codec == "fastlz":
        e, kind, want = nx.FastLzFrameEncoder(), B.WS_FASTLZ_ENC, oracle.fastlz_frame_encode(msg)
    else:
        high = codec == "lz4hc"
        e, kind = nx.Lz4FrameEncoder(unit, high_compressor=high), B.WS_LZ4HC_ENC if high else B.WS_LZ4_ENC
        want = oracle.lz4_frame_encode(msg, block_size=unit, close=False, high=high)
    held, _ = B.workspace_info(kind)
    assert held > 0
    assert e.encode(msg) == want
    assert B.workspace_info(kind)[0] == held
    e.close()


def test_batcher_large_flushes_on_all_streams_one_workspace(nx, B, oracle):
    """Eight flushes of 16 500 encoder slices each (two on each of the batcher's four streams, all in
    flight together) and two 16 500-chunk decoder jobs: the workspaces reserved by nx_batcher_reserve
    are the only ones (no growth during the flushes, device memory grows by less than one workspace),
    every job's bytes equal the oracle's, and nx_batcher_free returns the memory."""
    _collect(B)
    enc = nx.SnappyFrameEncoder()
    dec = nx.SnappyFrameDecoder(True)
    free0 = _free_bytes()
    e0, eo0 = B.workspace_info(B.WS_SNAPPY_ENC)
    d0, do0 = B.workspace_info(B.WS_DEC_RECORDS)
    b = nx.Batcher()
    # a batcher holds a workspace from its first submit that needs it, or from reserve()
    assert B.workspace_info(B.WS_SNAPPY_ENC)[1] == eo0 and B.workspace_info(B.WS_DEC_RECORDS)[1] == do0
    b.reserve((1 << B.WS_SNAPPY_ENC) | (1 << B.WS_DEC_RECORDS))
    e1, eo1 = B.workspace_info(B.WS_SNAPPY_ENC)
    d1, do1 = B.workspace_info(B.WS_DEC_RECORDS)
    assert (eo1, do1) == (eo0 + 1, do0 + 1)
    assert e1 >= e0 and d1 >= d0
    free1 = _free_bytes()

    n = 16500
    msgs = [oracle.textgen_chunk(70000 + i, 19 + (i * 37) % 300) for i in range(n)]
    stream = bytearray()
    for i, m in enumerate(msgs):
        stream += oracle.snappy_frame_encode(m, started=i > 0)[0]
    stream = bytes(stream)
    tickets = []
    for f in range(8):
        ts = [b.submit_encode(enc, m) for m in msgs]
        td = b.submit_decode(dec, stream) if f in (0, 5) else None
        b.flush()
        tickets.append((ts, td))
    assert b.stats()["flushes"] == 8
    for f, (ts, td) in enumerate(tickets):
        for j, (t, m) in enumerate(zip(ts, msgs)):
            b.wait(t)
            want = oracle.snappy_frame_encode(m, started=f > 0 or j > 0)[0]
            assert b.result(t) == [want], (f, j)
        if td is not None:
            b.wait(td)
            assert b.result(td) == msgs, f
    assert B.workspace_info(B.WS_SNAPPY_ENC) == (e1, eo1)  # never grown inside a flush
    assert B.workspace_info(B.WS_DEC_RECORDS) == (d1, do1)
    free2 = _free_bytes()
    assert free1 - free2 < max(e1, 64 * MiB), (free1 - free2) / MiB
    b.close()
    enc.close()
    dec.close()
    _, eo3 = B.workspace_info(B.WS_SNAPPY_ENC)
    _, do3 = B.workspace_info(B.WS_DEC_RECORDS)
    assert (eo3, do3) == (eo0 - 1, do0 - 1)  # the batcher's and the two handles' shares returned
    free3 = _free_bytes()
    assert free3 >= free0 - 64 * MiB, (free0 - free3) / MiB


def test_record_part_leases_overlap_streams(nx, B, oracle):
    """(The parse/expand pair: below 32 768 frames "auto" takes the fused decoder, which uses no
    record workspace.)  The decoder's record workspace is leased by part (a ring of frame slots): batches on different
    streams take disjoint slots and run together, a batch that wraps onto slots still in use waits
    for their batch.  Twelve decodes over four streams, launched back to back with no host sync,
    against a 3000-slot workspace (three 1000-frame batches fit, the fourth reuses the first's
    slots): every frame decodes to its source bytes."""
    _collect(B)
    _, owners = B.workspace_info(B.WS_DEC_RECORDS)
    if owners:
        pytest.skip("a live handle of another test holds the workspace")
    dev = torch.device("cuda:0")
    L = 4096
    src = torch.empty(3000 * L, dtype=torch.uint8, device=dev)
    B.textgen(src, 0, 3000, L)
    off = torch.arange(3000, dtype=torch.int64, device=dev) * L
    ln = torch.full((3000,), L, dtype=torch.int32, device=dev)
    cap = (B.snappy_max_compressed_length(L) + 15) // 16 * 16
    enc = torch.empty(3000 * cap, dtype=torch.uint8, device=dev)
    eoff = torch.arange(3000, dtype=torch.int64, device=dev) * cap
    elen, est = B.snappy_encode(src, off, ln, enc, eoff)
    dec = torch.zeros_like(src)
    r = B.snappy_decode(enc, eoff, elen, dec, off, variant="pair")  # grows the workspace to 3000 slots
    torch.cuda.synchronize()
    assert int((est != 0).sum()) == 0 and int((r["status"] != 0).sum()) == 0 and torch.equal(dec, src)
    assert B.workspace_info(B.WS_DEC_RECORDS)[0] >= 3000 * 16384 * 4
    streams = [torch.cuda.Stream(dev) for _ in range(4)]
    bufs = [torch.zeros_like(src) for _ in range(12)]
    torch.cuda.synchronize()  # the zero fills (default stream) are done before the side streams write
    outs = []
    for k in range(12):
        part = slice(1000 * (k % 3), 1000 * (k % 3 + 1))
        o = bufs[k]
        with torch.cuda.stream(streams[k % 4]):
            res = B.snappy_decode(enc, eoff[part], elen[part], o, off[part], variant="pair")
        outs.append((part, o, res, streams[k % 4]))
    torch.cuda.synchronize()
    for part, o, res, s in outs:
        a, b = part.start * L, part.stop * L
        assert int((res["status"] != 0).sum()) == 0
        assert torch.equal(o[a:b], src[a:b]), part
    B.workspaces_trim()


def test_trim_after_batchers_and_handles_are_freed(nx, B, oracle):
    """Workspace events recorded on a batcher's or a handle's own stream are forgotten when that
    stream is destroyed (ws_forget_stream): a later trim, grow or lease never waits on an event
    whose stream is gone (round 5, profiles/r05/s6-s7: nx_workspaces_trim failed with "operation not
    permitted when stream is capturing" after earlier tests' batchers were freed).  LZ4 frames decode
    through the record workspace (k_parse_lz4 + the expander) on the batcher's and the handle's
    streams; each round frees both, then trims."""
    data = oracle.textgen_chunk(5, 300000)
    enc = nx.Lz4FrameEncoder(65536)
    framed = enc.encode(data) + enc.finish_encode()
    for _ in range(12):
        b = nx.Batcher()
        d = nx.Lz4FrameDecoder(True)
        t = b.submit_decode(d, framed)
        b.flush()
        b.wait(t)
        assert b"".join(b.result(t)) == data
        h = nx.Lz4FrameDecoder(True)
        assert b"".join(h.channel_read(framed)) == data
        del b, d, h
        _collect(B)
        B.workspaces_trim()
        _, owners = B.workspace_info(B.WS_DEC_RECORDS)
        assert owners == 0


def test_encoder_reserve_under_a_byte_cap(nx, B, oracle):
    """VERDICT r5 item 5 (the reference decodes under an allocator memory limit,
    AbstractIntegrationTest.java:193-255): nx_snappy_encoder_reserve_ex caps the Snappy table workspace;
    a standalone batch larger than the cap runs on the capped lanes in more launches, never grows it,
    and its bytes equal the oracle's; the placement held at most the default peak (half the device)."""
    _collect(B)
    _, owners = B.workspace_info(B.WS_SNAPPY_ENC)
    if owners:
        pytest.skip("a live handle of another test holds the workspace")
    B.workspace_placement_config(0, 0)  # the defaults (bench.py lifts them in its own process)
    lanes = 20480  # above the one-chunk-per-wave form: dense launches of at most 20 480 chunks
    cap = lanes * 128 * 1024 + 12345
    got_bytes, peak = B.snappy_encoder_reserve(70000, cap)
    assert got_bytes == lanes * 128 * 1024
    total = torch.cuda.mem_get_info()[1]
    assert got_bytes <= peak <= total // 2
    dev = torch.device("cuda:0")
    n = 50000
    chunks = [oracle.textgen_chunk(5000 + (i % 97), 300 + (i % 97) * 37) for i in range(n)]
    inp, off, ln = B.pack(chunks, dev, align=1)
    out, ooff = B.out_slots([B.snappy_max_compressed_length(len(c)) for c in chunks], dev)
    olen, st = B.snappy_encode(inp, off, ln, out, ooff)
    torch.cuda.synchronize()
    assert int((st != 0).sum()) == 0
    assert B.workspace_info(B.WS_SNAPPY_ENC)[0] == got_bytes  # not grown past the cap
    outh, oo, ol = out.cpu().numpy().tobytes(), ooff.cpu().tolist(), olen.cpu().tolist()
    want = {}
    for i in list(range(0, n, 211)) + list(range(n - 300, n)):
        k = i % 97
        if k not in want:
            want[k] = oracle.snappy_encode(chunks[i])
        assert outh[oo[i]:oo[i] + ol[i]] == want[k], i
    # a reserve above the cap is refused while the capped workspace lives; trim lifts the cap
    from netty_amd import _lib
    assert _lib.load().nx_snappy_encoder_reserve_ex(70000, cap // 2, None, None, None) != 0
    B.workspaces_trim()
    assert B.workspace_info(B.WS_SNAPPY_ENC) == (0, 0)
