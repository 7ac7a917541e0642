"""GPU tests of the deflate encoder (nx_deflate_encode_batch, nx_crc32_batch, JdkZlibEncoder).  The
checker is Python's zlib / gzip (the real zlib), never the project's own code: every chunk's output
must be a valid, byte-aligned, non-final run of deflate blocks that inflates to the chunk."""
import gzip
import random
import zlib

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LENGTHS = [1, 2, 3, 4, 5, 257, 258, 259, 260, 32767, 32768, 32769, 65535, 65536]
SYNC = b"\0\0\xff\xff"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def B():
    from netty_amd import batch
    return batch


def _periodic(rng, n, period):
    base = rng.randbytes(min(n, period))
    return (base * (n // len(base) + 1))[:n]


def _marked(n, dist):
    """zeros with one 200-byte random marker and its repeat `dist` bytes later: the only match the
    repeat can find is at exactly that distance (the zeros between hash to one table slot, not the
    marker's), and it saves some 200 literals"""
    d = bytearray(n)
    m = bytes(b | 1 for b in random.Random(200).randbytes(200))
    for p in (100, 100 + dist):
        if p + len(m) <= n:
            d[p:p + len(m)] = m
    return bytes(d)


def _contents(oracle):
    rng = random.Random(1951)
    kinds = {
        "text": lambda n: oracle.textgen_chunk(300 + n % 97, n),
        "random": lambda n: rng.randbytes(n),
        "zero": lambda n: bytes(n),
        "period32768": lambda n: _periodic(rng, n, 32768),
        "period32769": lambda n: _periodic(rng, n, 32769),
        "high": lambda n: bytes(144 + b % 112 for b in rng.randbytes(n)),
        "two": lambda n: bytes(b"ab"[b & 1] for b in rng.randbytes(n)),
        "mark32768": lambda n: _marked(n, 32768),
        "mark32769": lambda n: _marked(n, 32769),
    }
    return [(k, n, f(n)) for k, f in kinds.items() for n in LENGTHS]


def _encode(B, dev, chunks, level=6, in_offsets=None, out_align=1):
    """one launch over `chunks`; returns (out bytes per chunk, status list)"""
    if in_offsets is None:
        inp, off, ln = B.pack(chunks, dev, align=16)
    else:
        buf = bytearray(max(o + len(c) for o, c in zip(in_offsets, chunks)) + 16)
        for o, c in zip(in_offsets, chunks):
            buf[o:o + len(c)] = c
        inp = torch.frombuffer(buf, dtype=torch.uint8).to(dev)
        off = torch.tensor(in_offsets, dtype=torch.int64, device=dev)
        ln = torch.tensor([len(c) for c in chunks], dtype=torch.int32, device=dev)
    caps = [B.deflate_max_compressed_length(len(c)) for c in chunks]
    out, ooff = B.out_slots(caps, dev, align=out_align)
    out.fill_(0xA5)
    olen, st = B.deflate_encode(inp, off, ln, out, ooff, level=level)
    torch.cuda.synchronize()
    outh, oo, ol = out.cpu().numpy().tobytes(), ooff.cpu().tolist(), olen.cpu().tolist()
    res = []
    for o, w, cap in zip(oo, ol, caps):
        assert 0 <= w <= cap, (w, cap)
        assert outh[o + w:o + cap] == b"\xa5" * (cap - w)  # nothing written past the reported length
        res.append(outh[o:o + w])
    return res, st.cpu().tolist()


def _check_block_run(chunk, out, what):
    d = zlib.decompressobj(-15)
    assert d.decompress(out) == chunk, what
    assert d.unused_data == b"" and d.eof is False, what
    assert out[-4:] == SYNC, what
    assert len(out) <= len(chunk) + 5 * -(-len(chunk) // 65535) + 5, what


@pytest.fixture(scope="module")
def sweep(B, dev, oracle):
    """the block-validity corpus, encoded once at level 6 into unaligned output slots"""
    cases = _contents(oracle)
    outs, st = _encode(B, dev, [c for _, _, c in cases])
    return cases, outs, st


def test_block_validity(sweep):
    cases, outs, st = sweep
    assert st == [0] * len(cases)
    for (kind, n, chunk), out in zip(cases, outs):
        _check_block_run(chunk, out, (kind, n))


def test_alignment_and_independence(sweep):
    cases, outs, _ = sweep
    d = zlib.decompressobj(-15)
    got = d.decompress(b"".join(outs) + b"\x03\x00")
    assert got == b"".join(c for _, _, c in cases)
    assert d.eof is True and d.unused_data == b""


def test_matches_at_the_window_edge(sweep):
    """a repeat exactly 32768 bytes back is coded as a match (the output is shorter than the same chunk
    with the repeat one byte farther, which must stay literals)"""
    cases, outs, _ = sweep
    size = {(k, n): len(o) for (k, n, _), o in zip(cases, outs)}
    assert size[("mark32768", 65536)] + 100 < size[("mark32769", 65536)]


def test_empty_chunk_and_level_zero(B, dev, sweep):
    cases = sweep[0]
    chunks = [b""] + [c for k, _, c in cases if k in ("text", "zero")]
    outs, st = _encode(B, dev, chunks, level=0)
    assert st == [0] * len(chunks) and outs[0] == b""
    for c, o in zip(chunks[1:], outs[1:]):
        assert len(o) == B.deflate_max_compressed_length(len(c)), len(c)  # stored blocks: exactly the bound
        _check_block_run(c, o, ("level0", len(c)))
    outs6, st6 = _encode(B, dev, [b"", b"x", b""])
    assert st6 == [0, 0, 0] and outs6[0] == b"" and outs6[2] == b""


def test_levels_and_oversize(B, dev):
    data = [b"netty " * 500, bytes(65537)]
    inp, off, ln = B.pack(data, dev)
    out, ooff = B.out_slots([70000, 70000], dev)
    for level in (-1, 1, 9):
        olen, st = B.deflate_encode(inp, off, ln, out, ooff, level=level)
        torch.cuda.synchronize()
        assert st.cpu().tolist() == [0, -100] and olen.cpu().tolist()[1] == 0  # NX_ERR_INVALID_ARG per chunk
        w = olen.cpu().tolist()[0]
        _check_block_run(data[0], out.cpu().numpy().tobytes()[:w], level)
    for level in (-2, 10):
        with pytest.raises(RuntimeError):
            B.deflate_encode(inp, off, ln, out, ooff, level=level)


def test_small_fuzz(B, dev):
    rng = random.Random(300)
    chunks, offs, cur = [], [], 0
    for i in range(300):
        n = rng.randrange(0, 701)
        alpha = bytes(rng.sample(range(256), rng.randrange(1, 5)))
        chunks.append(bytes(rng.choice(alpha) for _ in range(n)))
        offs.append((cur + 15) // 16 * 16 + i % 3)  # three input alignments
        cur = offs[-1] + n
    outs, st = _encode(B, dev, chunks, in_offsets=offs)
    assert st == [0] * 300
    for i, (c, o) in enumerate(zip(chunks, outs)):
        if c:
            _check_block_run(c, o, i)
        else:
            assert o == b""
    d = zlib.decompressobj(-15)
    assert d.decompress(b"".join(outs) + b"\x03\x00") == b"".join(chunks) and d.eof


def test_sub_batches_reuse_slots(B, dev):
    """more chunks than one launch has slots for (the small-batch form runs one chunk per wave on a
    bounded number of waves): every sub-batch's tokens are its own"""
    rng = random.Random(5)
    n = 256 * 16 * 2 + 37  # over twice the waves of any device up to 256 CUs
    chunks = [bytes(rng.choice(b"abc") for _ in range(40 + i % 23)) for i in range(n)]
    outs, st = _encode(B, dev, chunks)
    assert st == [0] * n
    d = zlib.decompressobj(-15)
    assert d.decompress(b"".join(outs) + b"\x03\x00") == b"".join(chunks) and d.eof


def test_checksums(B, dev):
    rng = random.Random(32)
    lens = [0, 1, 15, 16, 17, 8191, 8192, 8193, 65536]
    chunks, offs, cur = [], [], 0
    for n in lens:
        for a in range(16):
            chunks.append(rng.randbytes(n))
            offs.append((cur + 15) // 16 * 16 + a)
            cur = offs[-1] + n
    buf = bytearray(cur + 16)
    for o, c in zip(offs, chunks):
        buf[o:o + len(c)] = c
    inp = torch.frombuffer(buf, dtype=torch.uint8).to(dev)
    off = torch.tensor(offs, dtype=torch.int64, device=dev)
    ln = torch.tensor([len(c) for c in chunks], dtype=torch.int32, device=dev)
    crc = [v & 0xFFFFFFFF for v in B.crc32(inp, off, ln).cpu().tolist()]
    adl = [v & 0xFFFFFFFF for v in B.adler32(inp, off, ln).cpu().tolist()]
    assert crc == [zlib.crc32(c) for c in chunks]
    assert adl == [zlib.adler32(c) for c in chunks]
    # the masked CRC32C of the same launch geometry is untouched by the second table set
    from netty_amd import _lib
    assert _lib.load().nx_crc32_combine(crc[-2], crc[-1], 65536) == zlib.crc32(chunks[-2] + chunks[-1])


def test_ratio_against_zlib_level_1(B, dev, oracle):
    """16 text chunks: each smaller than stored, and in total within 1.10 x zlib level 1 per chunk with
    a sync flush (a single-probe greedy matcher with dynamic Huffman codes modelled at 0.93-0.97 of
    it; fixed Huffman alone sits at 1.18-1.24 and fails this)."""
    chunks = [oracle.textgen_chunk(1000 + i, 65536) for i in range(16)]
    outs, st = _encode(B, dev, chunks, out_align=16)
    assert st == [0] * 16
    ref = 0
    for c, o in zip(chunks, outs):
        _check_block_run(c, o, "ratio")
        assert len(o) < B.deflate_max_compressed_length(65536)
        z = zlib.compressobj(1, zlib.DEFLATED, -15)
        ref += len(z.compress(c) + z.flush(zlib.Z_SYNC_FLUSH))
    total = sum(len(o) for o in outs)
    print(f"deflate ratio: {total} bytes against zlib level 1 {ref} = {total / ref:.4f}")
    assert total <= 1.10 * ref, (total, ref)


GZIP_HEADER = bytes([0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 0])
WBITS = {0: 15, 1: 31, 2: -15}


@pytest.fixture(scope="module")
def messages(oracle):
    return [b"", b"z", oracle.textgen_chunk(77, 70000), oracle.textgen_chunk(78, 150000) + bytes(20000) + random.Random(9).randbytes(30000)]


@pytest.mark.parametrize("wrapper", [0, 1, 2])
@pytest.mark.parametrize("level", [0, 1, 6, 9])
def test_handler_stream(wrapper, level, messages):
    from netty_amd import EmbeddedChannel, JdkZlibEncoder, ZlibWrapper
    enc = JdkZlibEncoder(ZlibWrapper(wrapper), level)
    ch = EmbeddedChannel(enc)
    assert [len(m) for m in messages] == [0, 1, 70000, 200000]
    wire, data = b"", b""
    for m in messages:
        ch.write_outbound(m)
        piece = ch.read_outbound()
        if not m:
            assert piece == b""  # nothing, not even the header
        wire += piece
        data += m
        d = zlib.decompressobj(WBITS[wrapper])
        assert d.decompress(wire) == data  # the sync-flush property
        assert d.eof is False and d.unused_data == b""
    wire += enc.finish_encode()
    d = zlib.decompressobj(WBITS[wrapper])
    assert d.decompress(wire) == data and d.eof is True and d.unused_data == b""
    if wrapper == 1:
        assert gzip.decompress(wire) == data
        assert wire[:10] == GZIP_HEADER
        assert wire[-8:] == zlib.crc32(data).to_bytes(4, "little") + (len(data) % 2**32).to_bytes(4, "little")
    elif wrapper == 0:
        assert wire[:2] == zlib.compress(b"", level)[:2]
        assert wire[-4:] == zlib.adler32(data).to_bytes(4, "big")
    else:
        assert wire[-2:] == b"\x03\x00"
    assert enc.encode(b"after close") == b"after close" and enc.finish_encode() == b""
    enc.close()


def test_handler_close_with_nothing_written():
    from netty_amd import JdkZlibEncoder, ZlibWrapper
    want = {ZlibWrapper.ZLIB: zlib.compress(b"", 6), ZlibWrapper.GZIP: GZIP_HEADER + b"\x03\x00" + bytes(8),
            ZlibWrapper.NONE: b"\x03\x00"}
    assert want[ZlibWrapper.ZLIB] == bytes.fromhex("789c030000000001")
    for w, expect in want.items():
        enc = JdkZlibEncoder(w)
        assert enc.encode(b"") == b""
        assert enc.finish_encode() == expect
        assert enc.encode(b"x") == b"x" and enc.finish_encode() == b""
        enc.close()


def test_handler_refuses_what_the_reference_refuses():
    from netty_amd import JdkZlibEncoder, ZlibWrapper, _lib
    with pytest.raises(ValueError):
        JdkZlibEncoder(ZlibWrapper.ZLIB_OR_NONE)
    for level in (-2, 10):
        with pytest.raises(ValueError):
            JdkZlibEncoder(ZlibWrapper.GZIP, level)
    L = _lib.load()
    assert not L.nx_zlib_encoder_new(3, 6) and not L.nx_zlib_encoder_new(0, -2) and not L.nx_zlib_encoder_new(1, 10)


def test_handles_hold_the_workspace(B):
    from netty_amd import JdkZlibEncoder, ZlibWrapper
    _, o0 = B.workspace_info(B.WS_DEFLATE_ENC)
    a, b = JdkZlibEncoder(), JdkZlibEncoder(ZlibWrapper.GZIP, 1)
    bytes_held, o1 = B.workspace_info(B.WS_DEFLATE_ENC)
    assert o1 == o0 + 2 and bytes_held >= 1024 * 128 * 1024
    assert a.encode(b"hello hello hello")  # runs on the held slots
    assert B.workspace_info(B.WS_DEFLATE_ENC) == (bytes_held, o1)
    a.close()
    b.close()
    assert B.workspace_info(B.WS_DEFLATE_ENC)[1] == o0
