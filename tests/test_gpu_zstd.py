"""GPU tests of the Zstandard frame encoder (nx_zstd_encode_batch).  The checker is libzstd through
pyarrow, never the project's own code: every chunk's output must be one complete frame that libzstd
decodes to the chunk; structure is asserted from headers parsed by tests/zstd_frames.py."""
import random

import pytest

import zstd_frames as Z
import zstd_inputs as I

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
pa = pytest.importorskip("pyarrow")

LENGTHS = [1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 65535, 65536]
NX_ERR_INVALID_ARG = -100
# total of 16 text chunks of 64 KiB against libzstd level 1, measured on the MI355X plus
# 5 % of itself, rounded up to two decimals
SIZE_RATIO_MEASURED = 1.0499  # 348 191 bytes against libzstd's 331 649
SIZE_RATIO_BAR = 1.11       # 1.0499 * 1.05 = 1.1024


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def B():
    from netty_amd import batch
    return batch


def _unzstd(frame, n):
    return pa.Codec("zstd").decompress(frame, decompressed_size=n).to_pybytes()


def _encode(B, dev, chunks, level=3, in_offsets=None, out_align=1, caps=None):
    """one launch over `chunks` into slots pre-filled with 0xA5; returns (frame per chunk, status list)"""
    if in_offsets is None:
        inp, off, ln = B.pack(chunks, dev, align=16)
    else:
        buf = bytearray(max(o + len(c) for o, c in zip(in_offsets, chunks)) + 16)
        for o, c in zip(in_offsets, chunks):
            buf[o:o + len(c)] = c
        inp = torch.frombuffer(buf, dtype=torch.uint8).to(dev)
        off = torch.tensor(in_offsets, dtype=torch.int64, device=dev)
        ln = torch.tensor([len(c) for c in chunks], dtype=torch.int32, device=dev)
    caps = caps or [B.zstd_max_compressed_length(len(c)) for c in chunks]
    out, ooff = B.out_slots(caps, dev, align=out_align)
    out.fill_(0xA5)
    olen, st = B.zstd_encode(inp, off, ln, out, ooff, level=level)
    torch.cuda.synchronize()
    outh, oo, ol = out.cpu().numpy().tobytes(), ooff.cpu().tolist(), olen.cpu().tolist()
    res = []
    for o, w, cap in zip(oo, ol, caps):
        assert 0 <= w <= cap, (w, cap)
        assert outh[o + w:o + cap] == b"\xa5" * (cap - w)  # guard bytes: nothing past the reported length
        res.append(outh[o:o + w])
    return res, st.cpu().tolist()


def _check_frame(chunk, out, what):
    n = len(chunk)
    f = Z.parse_frame(out)
    assert f.end == len(out), what
    assert f.single_segment and not f.checksum and f.dict_id == 0 and f.content_size == n, what
    assert f.fcs_bytes == (1 if n <= 255 else 2), what
    assert len(f.blocks) == 1 and f.blocks[0].last, what
    assert _unzstd(out, n) == chunk, what
    assert len(out) <= n + (n >> 8) + ((131072 - n) >> 11), what
    assert len(out) <= n + 3 + f.header, what  # never larger than its Raw-block frame
    return f.blocks[0]


def _contents(oracle):
    rng = random.Random(8878)
    kinds = {
        "text": lambda n: oracle.textgen_chunk(300 + n % 97, n),
        "random": lambda n: rng.randbytes(n),
        "zero": lambda n: bytes(n),
        "high": lambda n: I.high(rng, n),
        "two": lambda n: bytes(b"ab"[b & 1] for b in rng.randbytes(n)),
        "period": lambda n: I.periodic(rng, n, 7),
    }
    return [(k, n, f(n)) for k, f in kinds.items() for n in LENGTHS]


@pytest.fixture(scope="module")
def sweep(B, dev, oracle):
    """content kinds x lengths, encoded in one launch into unaligned output slots"""
    cases = _contents(oracle)
    outs, st = _encode(B, dev, [c for _, _, c in cases])
    return cases, outs, st


def test_frames_decode_and_block_choice(sweep):
    cases, outs, st = sweep
    assert st == [0] * len(cases)
    for (kind, n, chunk), out in zip(cases, outs):
        b = _check_frame(chunk, out, (kind, n))
        if kind == "random" or n == 1:
            assert b.type == Z.RAW, (kind, n)
        elif kind == "zero":
            assert b.type == Z.RLE and b.size == n, (kind, n)
        if kind == "text" and n == 65536:
            assert b.type == Z.COMPRESSED and b.lit_type == Z.LIT_COMPRESSED, (kind, n)
        if kind == "high" and n == 65536:  # the last symbol is above 127: only FSE weights can describe the tree
            assert b.type == Z.COMPRESSED and b.lit_type == Z.LIT_COMPRESSED and b.tree == "fse", (kind, n)
        if kind == "period" and n == 65536:
            # 10 of frame and block header, 8 of literals, 2 of sequence header, 5 of bitstream; a 258 cap needs 254 sequences
            assert len(out) <= 40, len(out)


def test_sequence_modes(sweep, B, dev):
    cases, outs, _ = sweep
    modes = [Z.parse_frame(o).blocks[0].modes for (k, n, _), o in zip(cases, outs) if k == "text"]
    assert any(m and Z.SEQ_FSE in m for m in modes), modes
    chunk = I.markers(11, 20, 200)  # 20 sequences of one literal-length code, one match length, one distance
    (out,), st = _encode(B, dev, [chunk])
    b = _check_frame(chunk, out, "markers")
    # all three codes are constant over the chunk's sequences, literal lengths (modes[0]) included
    assert st == [0] and b.nseq == 20 and b.modes == (Z.SEQ_RLE, Z.SEQ_RLE, Z.SEQ_RLE), (b.nseq, b.modes)


def test_literals_size_formats(B, dev):
    lens = list(range(1016, 1033)) + list(range(16376, 16393))
    chunks = [I.skewed(random.Random(n), n) for n in lens]
    outs, st = _encode(B, dev, chunks)
    assert st == [0] * len(lens)
    seen = {}
    for c, o in zip(chunks, outs):
        b = _check_frame(c, o, len(c))
        assert b.type == Z.COMPRESSED and b.lit_type == Z.LIT_COMPRESSED, len(c)
        assert b.lit_streams == (1 if b.lit_regen <= 1023 else 4), (len(c), b.lit_regen, b.lit_streams)
        assert b.lit_format == (0 if b.lit_regen <= 1023 else 2 if b.lit_regen <= 16383 else 3), (len(c), b.lit_regen, b.lit_format)
        assert b.lit_header + b.lit_comp + b.seq_header <= b.size
        seen[b.lit_regen] = b
    for edge in (1023, 16383):  # literal counts on both sides of each format's limit
        assert any(r <= edge for r in seen if r > edge - 10) and any(r > edge for r in seen if r <= edge + 10), sorted(seen)
    assert 1023 in seen and 1024 in seen and 16383 in seen and 16384 in seen, sorted(seen)


def test_number_of_sequences_forms(B, dev):
    chunks = [I.markers(5, k, 64, lead=8) for k in (100, 127, 128, 140)] + [I.skewed(random.Random(3), 300)]
    outs, st = _encode(B, dev, chunks)
    assert st == [0] * len(chunks)
    counts = [_check_frame(c, o, len(c)).nseq for c, o in zip(chunks, outs)]
    assert all(x is not None for x in counts), counts  # every one a Compressed block
    assert 0 in counts and any(0 < x <= 127 for x in counts) and any(x >= 128 for x in counts), counts
    for c, o in zip(chunks, outs):
        b = Z.parse_frame(o).blocks[0]
        assert b.seq_header == (1 if b.nseq == 0 else 2 if b.nseq < 128 else 3), (b.nseq, b.seq_header)


def test_reach_is_the_whole_chunk(B, dev):
    n = 65536
    chunks = [I.recur(9, n, 0, d, 400) for d in (65000, 32768, 32769)]
    outs, st = _encode(B, dev, chunks)
    assert st == [0, 0, 0]
    for c, o, d in zip(chunks, outs, (65000, 32768, 32769)):
        _check_frame(c, o, d)
        assert len(o) < n - 300, (d, len(o))  # 400 literals saved, less a few header bytes


def test_oversized_chunk_fails_alone(B, dev):
    rng = random.Random(4)
    chunks = [rng.randbytes(500) * 3, bytes(65537), b"neighbour " * 40]
    caps = [B.zstd_max_compressed_length(len(c)) for c in chunks]
    outs, st = _encode(B, dev, chunks, caps=caps)
    assert st == [0, NX_ERR_INVALID_ARG, 0] and outs[1] == b""
    for i in (0, 2):
        _check_frame(chunks[i], outs[i], i)


def test_empty_chunk_writes_nothing_and_levels(B, dev):
    outs, st = _encode(B, dev, [b"", b"abc" * 50])
    assert st == [0, 0] and outs[0] == b""
    ref = outs[1]
    for level in (-131072, -5, 0, 1, 22):  # every level the one matcher
        outs, st = _encode(B, dev, [b"abc" * 50], level=level)
        assert st == [0] and outs[0] == ref
    for level in (-131073, 23):
        with pytest.raises(RuntimeError):
            _encode(B, dev, [b"abc"], level=level)


def test_unaligned_offsets(B, dev, oracle):
    text = oracle.textgen_chunk(5, 3000)
    chunks = [text[i:i + 900 + i] for i in range(16)]
    in_off = [i * 4096 + (i * 7 + 1) % 16 for i in range(16)]  # unaligned inputs
    caps = [B.zstd_max_compressed_length(len(c)) + i for i, c in enumerate(chunks)]  # out_off walks through every residue mod 16
    outs, st = _encode(B, dev, chunks, in_offsets=in_off, out_align=1, caps=caps)
    assert st == [0] * 16
    for c, o in zip(chunks, outs):
        _check_frame(c, o, len(c))
    ref, _ = _encode(B, dev, chunks)
    assert outs == ref  # the bytes do not depend on where the chunk or its slot lies
    for r in range(16):
        one, st1 = _encode(B, dev, [b"", chunks[3]], caps=[r, B.zstd_max_compressed_length(len(chunks[3]))], out_align=1)
        assert one[1] == ref[3], r


def test_grid_forms_agree(B, dev, oracle):
    base = [oracle.textgen_chunk(k, 200 + 37 * (k % 5)) for k in range(70)]
    one, _ = _encode(B, dev, base[:1])
    spread, st70 = _encode(B, dev, base)
    many = [base[k % 70] for k in range(16385)]
    dense, stn = _encode(B, dev, many)
    assert st70 == [0] * 70 and stn == [0] * 16385
    assert one[0] == spread[0]
    assert all(dense[k] == spread[k % 70] for k in range(16385))
    for c, o in zip(base, spread):
        _check_frame(c, o, len(c))


def test_size_against_libzstd_level_1(B, dev, oracle):
    chunks = [oracle.textgen_chunk(k, 65536) for k in range(16)]
    outs, st = _encode(B, dev, chunks)
    assert st == [0] * 16
    for c, o in zip(chunks, outs):
        b = _check_frame(c, o, "text")
        assert b.lit_type == Z.LIT_COMPRESSED  # not a silent fall back to raw literals
    ours = sum(len(o) for o in outs)
    lib = sum(len(pa.Codec("zstd", compression_level=1).compress(c).to_pybytes()) for c in chunks)
    ratio = ours / lib
    print(f"zstd size: ours {ours} libzstd-1 {lib} ratio {ratio:.4f}")
    assert SIZE_RATIO_BAR is not None, f"measured ratio {ratio:.4f}: the bar is not set"
    assert ratio <= SIZE_RATIO_BAR, (ratio, SIZE_RATIO_BAR)
