"""Device-resident batch API (thin wrappers over the C-ABI batch kernels).

All tensors are torch tensors on the same HIP device; torch is used only as the device
allocator / stream provider.  Chunk i is ``data[off[i] : off[i] + length[i]]``.  Calls are
asynchronous on torch's current stream.
"""
from __future__ import annotations

import torch

from . import _lib


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _chk(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed: {rc} ({_lib.status_string(rc)})")


# Shared device workspaces (include/netty_amd.h NX_WS_*; csrc/workspace.hpp)
WS_SNAPPY_ENC, WS_LZ4_ENC, WS_FASTLZ_ENC, WS_LZF_ENC, WS_DEC_RECORDS, WS_LZ4HC_ENC, WS_DEFLATE_ENC, WS_ZSTD_ENC, WS_ZSTD_DEC, WS_BZIP2_DEC, WS_BZIP2_ENC, WS_LZMA_ENC, WS_BROTLI_ENC, WS_BROTLI_DEC = range(14)


def workspace_info(kind: int) -> tuple[int, int]:
    """(bytes, owners) of the current device's workspace of `kind`."""
    import ctypes as C
    b, o = C.c_uint64(0), C.c_int32(0)
    _chk(_lib.load().nx_workspace_info(kind, C.byref(b), C.byref(o)), "nx_workspace_info")
    return b.value, o.value


def workspaces_trim():
    """Free the current device's workspaces that no batcher or handle holds."""
    _chk(_lib.load().nx_workspaces_trim(), "nx_workspaces_trim")


def snappy_encoder_reserve(max_chunks: int, max_bytes: int = 0) -> tuple[int, int]:
    """nx_snappy_encoder_reserve_ex: place the Snappy table workspace now, capped at max_bytes for good
    (0: no cap).  Returns (workspace bytes, most bytes its placement held at once)."""
    import ctypes as C
    b, p = C.c_uint64(0), C.c_uint64(0)
    _chk(_lib.load().nx_snappy_encoder_reserve_ex(max_chunks, max_bytes, _stream(), C.byref(b), C.byref(p)),
         "nx_snappy_encoder_reserve_ex")
    return b.value, p.value


def workspace_placement_config(peak_bytes: int = 0, max_candidates: int = 0):
    """nx_workspace_placement_config: the bytes a large workspace's placement candidates may hold at once
    (0: half the device; 2**64 - 1: all but 8 GiB free) and the candidates drawn in all (0: 24)."""
    _chk(_lib.load().nx_workspace_placement_config(peak_bytes, max_candidates), "nx_workspace_placement_config")


def snappy_max_compressed_length(n: int) -> int:
    return _lib.load().nx_snappy_max_compressed_length(n)


def fastlz_max_compressed_length(n: int) -> int:
    return _lib.load().nx_fastlz_max_compressed_length(n)


def lzf_max_compressed_length(n: int) -> int:
    return _lib.load().nx_lzf_max_compressed_length(n)


def snappy_encode(inp, in_off, in_len, out, out_off, out_len=None, status=None):
    """Snappy.encode per chunk (Snappy.java:82-165).  Returns (out_len, status) int tensors."""
    n = in_len.numel()
    dev = inp.device
    out_len = torch.empty(n, dtype=torch.int32, device=dev) if out_len is None else out_len
    status = torch.empty(n, dtype=torch.int32, device=dev) if status is None else status
    _chk(_lib.load().nx_snappy_encode_batch(_ptr(inp), _ptr(in_off), _ptr(in_len), _ptr(out), _ptr(out_off), _ptr(out_len),
                                            _ptr(status), n, _stream()), "nx_snappy_encode_batch")
    return out_len, status


def snappy_decode(inp, in_off, in_len, out, out_off, out_cap=None, expected_crc=None, want_crc=False, consumed=False,
                  out_len=None, status=None, variant="auto", fn=None):
    """Snappy.decode per chunk (+ fused masked-CRC32C verify).  Returns dict of tensors.

    variant: "auto" (the fused decoder up to 32768 frames, the parse/expand pair above), "pair" (always
    the parse/expand kernel pair) or "fused" (always the single-kernel wave decoder), same contract; fn: another entry point of that contract (the tests' lane-per-chunk cross-check kernel)."""
    n = in_len.numel()
    dev = inp.device
    out_len = torch.empty(n, dtype=torch.int32, device=dev) if out_len is None else out_len
    status = torch.empty(n, dtype=torch.int32, device=dev) if status is None else status
    cons = torch.empty(n, dtype=torch.int32, device=dev) if consumed else None
    crc = torch.empty(n, dtype=torch.int32, device=dev) if want_crc else None
    lib = _lib.load()
    if fn is None:
        fn = {"auto": lib.nx_snappy_decode_batch, "fused": lib.nx_snappy_decode_batch_fused,
              "pair": lib.nx_snappy_decode_batch_pair}[variant]
    _chk(fn(_ptr(inp), _ptr(in_off), _ptr(in_len), _ptr(out), _ptr(out_off), _ptr(out_cap), _ptr(out_len), _ptr(cons),
            _ptr(status), _ptr(expected_crc), _ptr(crc), n, _stream()), "nx_snappy_decode_batch")
    return {"out_len": out_len, "status": status, "consumed": cons, "crc": crc}


def snappy_frame_scan(inp, in_off, in_len, state, cap: int):
    """SnappyFrameDecoder's chunk walk over device cumulations (nx_snappy_frame_scan_batch).

    in_off / in_len: int64 tensors (one cumulation per stream); state: int32 tensor, updated in place
    (started | corrupted << 1 | numBytesToSkip << 8).  Returns a dict of tensors: consumed, status,
    counts [compressed, uncompressed, claims], and the list arrays data_off, data_len, masked_crc,
    stream, seq (compressed entries at [0, counts[0]), uncompressed at [cap - counts[1], cap))."""
    n = in_len.numel()
    dev = inp.device
    c = max(int(cap), 1)
    r = {"consumed": torch.empty(n, dtype=torch.int64, device=dev),
         "status": torch.empty(n, dtype=torch.int32, device=dev),
         "data_off": torch.empty(c, dtype=torch.int64, device=dev),
         "data_len": torch.empty(c, dtype=torch.int32, device=dev),
         "masked_crc": torch.empty(c, dtype=torch.int32, device=dev),
         "stream": torch.empty(c, dtype=torch.int32, device=dev),
         "seq": torch.empty(c, dtype=torch.int32, device=dev),
         "counts": torch.empty(3, dtype=torch.int32, device=dev)}
    _chk(_lib.load().nx_snappy_frame_scan_batch(_ptr(inp), _ptr(in_off), _ptr(in_len), _ptr(state), _ptr(r["consumed"]),
                                                _ptr(r["status"]), _ptr(r["data_off"]), _ptr(r["data_len"]),
                                                _ptr(r["masked_crc"]), _ptr(r["stream"]), _ptr(r["seq"]), _ptr(r["counts"]),
                                                int(cap), n, _stream()), "nx_snappy_frame_scan_batch")
    return r


def snappy_frame_scan_long(inp, length: int, state, cap: int, offset: int = 0):
    """The segmented walk of ONE long cumulation inp[offset, offset + length) (nx_snappy_frame_scan_long);
    state: a one-element int32 tensor, updated in place.  Same result dict as snappy_frame_scan with
    n = 1 (data_off relative to inp[offset])."""
    dev = inp.device
    c = max(int(cap), 1)
    r = {"consumed": torch.empty(1, dtype=torch.int64, device=dev),
         "status": torch.empty(1, dtype=torch.int32, device=dev),
         "data_off": torch.empty(c, dtype=torch.int64, device=dev),
         "data_len": torch.empty(c, dtype=torch.int32, device=dev),
         "masked_crc": torch.empty(c, dtype=torch.int32, device=dev),
         "stream": torch.empty(c, dtype=torch.int32, device=dev),
         "seq": torch.empty(c, dtype=torch.int32, device=dev),
         "counts": torch.empty(3, dtype=torch.int32, device=dev)}
    _chk(_lib.load().nx_snappy_frame_scan_long(_ptr(inp) + int(offset), int(length), _ptr(state), _ptr(r["consumed"]),
                                               _ptr(r["status"]), _ptr(r["data_off"]), _ptr(r["data_len"]),
                                               _ptr(r["masked_crc"]), _ptr(r["stream"]), _ptr(r["seq"]), _ptr(r["counts"]),
                                               int(cap), _stream()), "nx_snappy_frame_scan_long")
    return r


def crc32c_masked(inp, off, length, out=None):
    """Snappy.calculateChecksum per chunk (Snappy.java:668-676)."""
    n = length.numel()
    out = torch.empty(n, dtype=torch.int32, device=inp.device) if out is None else out
    _chk(_lib.load().nx_crc32c_masked_batch(_ptr(inp), _ptr(off), _ptr(length), _ptr(out), n, _stream()),
         "nx_crc32c_masked_batch")
    return out


def fastlz_compress(inp, in_off, in_len, out, out_off, level=None, u16_limit=None):
    n = in_len.numel()
    dev = inp.device
    out_len = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    _chk(_lib.load().nx_fastlz_compress_batch(_ptr(inp), _ptr(in_off), _ptr(in_len), _ptr(out), _ptr(out_off), _ptr(out_len),
                                              _ptr(level), _ptr(u16_limit), _ptr(status), n, _stream()),
         "nx_fastlz_compress_batch")
    return out_len, status


def fastlz_decompress(inp, in_off, in_len, out, out_off, out_len_limit, in_avail=None):
    n = in_len.numel()
    res = torch.empty(n, dtype=torch.int32, device=inp.device)
    _chk(_lib.load().nx_fastlz_decompress_batch(_ptr(inp), _ptr(in_off), _ptr(in_len), _ptr(in_avail), _ptr(out),
                                                _ptr(out_off), _ptr(out_len_limit), _ptr(res), n, _stream()),
         "nx_fastlz_decompress_batch")
    return res


def adler32(inp, off, length):
    n = length.numel()
    out = torch.empty(n, dtype=torch.int32, device=inp.device)
    _chk(_lib.load().nx_adler32_batch(_ptr(inp), _ptr(off), _ptr(length), _ptr(out), n, _stream()), "nx_adler32_batch")
    return out


def crc32(inp, off, length, out=None):
    """java.util.zip.CRC32 per chunk (nx_crc32_batch)."""
    n = length.numel()
    out = torch.empty(n, dtype=torch.int32, device=inp.device) if out is None else out
    _chk(_lib.load().nx_crc32_batch(_ptr(inp), _ptr(off), _ptr(length), _ptr(out), n, _stream()), "nx_crc32_batch")
    return out


def deflate_max_compressed_length(n: int) -> int:
    return _lib.load().nx_deflate_max_compressed_length(n)


def deflate_encode(inp, in_off, in_len, out, out_off, level: int = 6, prefix_len=None):
    """Raw deflate with a sync flush per chunk of at most 65536 bytes (nx_deflate_encode_batch): slots
    of deflate_max_compressed_length bytes; level as java.util.zip.Deflater.  prefix_len (an int32 tensor;
    nx_deflate_encode_batch_ex): chunk i may match into the prefix_len[i] <= 32768 bytes before it in inp,
    prefix_len[i] + in_len[i] <= 65536.  Returns (out_len, status)."""
    n = in_len.numel()
    dev = inp.device
    out_len = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    if prefix_len is None:
        _chk(_lib.load().nx_deflate_encode_batch(_ptr(inp), _ptr(in_off), _ptr(in_len), _ptr(out), _ptr(out_off), _ptr(out_len),
                                                 _ptr(status), n, int(level), _stream()), "nx_deflate_encode_batch")
    else:
        assert prefix_len.numel() == n and prefix_len.dtype == torch.int32
        _chk(_lib.load().nx_deflate_encode_batch_ex(_ptr(inp), _ptr(in_off), _ptr(in_len), _ptr(prefix_len), _ptr(out),
                                                    _ptr(out_off), _ptr(out_len), _ptr(status), n, int(level), _stream()),
             "nx_deflate_encode_batch_ex")
    return out_len, status


def zstd_max_compressed_length(n: int) -> int:
    return _lib.load().nx_zstd_max_compressed_length(n)


def zstd_encode(inp, in_off, in_len, out, out_off, level: int = 3):
    """One complete Zstandard frame per chunk of at most 65536 bytes (nx_zstd_encode_batch): slots of
    zstd_max_compressed_length bytes; level as libzstd (-131072..22, every one the one matcher).
    Returns (out_len, status)."""
    n = in_len.numel()
    dev = inp.device
    out_len = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    _chk(_lib.load().nx_zstd_encode_batch(_ptr(inp), _ptr(in_off), _ptr(in_len), _ptr(out), _ptr(out_off), _ptr(out_len),
                                          _ptr(status), n, int(level), _stream()), "nx_zstd_encode_batch")
    return out_len, status


ZSTD_FRAME_SINGLE_SEGMENT, ZSTD_FRAME_CHECKSUM = 1, 2
ZSTD_CONTENT_SIZE_UNKNOWN = 2 ** 64 - 1


ZSTD_DECODE_VERIFY_CHECKSUM = 1
ZSTD_KIND_FRAME, ZSTD_KIND_SKIPPABLE = 0, 1


def zstd_decode(inp, in_off, in_len, out, out_off, out_cap, verify_checksum: bool = False):
    """One complete Zstandard frame per item (nx_zstd_decode_batch): item i starts at inp[in_off[i]], bytes
    after its frame inside in_len[i] are left alone; it regenerates into out[out_off[i] : + out_cap[i]].
    Returns (consumed, out_len, status): the frame's compressed size, the regenerated size (on an error,
    what was written before it) and 0 or one NX_ERR_ZSTD_* code per item.  verify_checksum
    (nx_zstd_decode_batch_ex, NX_ZSTD_DECODE_VERIFY_CHECKSUM): a frame with a content checksum is decoded
    and its XXH64 verified in the same launch (a mismatch is NX_ERR_ZSTD_CHECKSUM, -88) instead of refused."""
    n = in_len.numel()
    dev = inp.device
    consumed = torch.empty(n, dtype=torch.int32, device=dev)
    out_len = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    if not verify_checksum:
        _chk(_lib.load().nx_zstd_decode_batch(_ptr(inp), _ptr(in_off), _ptr(in_len), _ptr(out), _ptr(out_off), _ptr(out_cap),
                                              _ptr(consumed), _ptr(out_len), _ptr(status), n, _stream()), "nx_zstd_decode_batch")
    else:
        _chk(_lib.load().nx_zstd_decode_batch_ex(_ptr(inp), _ptr(in_off), _ptr(in_len), _ptr(out), _ptr(out_off), _ptr(out_cap),
                                                 _ptr(consumed), _ptr(out_len), _ptr(status), n, ZSTD_DECODE_VERIFY_CHECKSUM,
                                                 _stream()), "nx_zstd_decode_batch_ex")
    return consumed, out_len, status


def zstd_decoder_reserve(max_frames: int):
    """nx_zstd_decoder_reserve: size the decoder's literals workspace for max_frames frames in flight now and
    cap it there until workspaces_trim()."""
    _chk(_lib.load().nx_zstd_decoder_reserve(int(max_frames), _stream()), "nx_zstd_decoder_reserve")


def zstd_frame_info(data: bytes):
    """nx_zstd_frame_info on host bytes: (status, frame_bytes, content_size, flags) of the first frame of
    `data`; content_size is None when the frame does not carry it; status NX_ERR_ZSTD_TRUNCATED (-85) when
    `data` ends inside the frame.  flags: ZSTD_FRAME_SINGLE_SEGMENT | ZSTD_FRAME_CHECKSUM | Window_Descriptor << 8."""
    import ctypes as C
    fb, cs, fl = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
    data = bytes(data)
    st = _lib.load().nx_zstd_frame_info(data, len(data), C.byref(fb), C.byref(cs), C.byref(fl))
    if st != 0:
        return st, 0, None, 0
    return 0, fb.value, None if cs.value == ZSTD_CONTENT_SIZE_UNKNOWN else cs.value, fl.value


def zstd_next_frame(data: bytes):
    """nx_zstd_next_frame on host bytes: (status, kind, frame_bytes, out_bound, flags) of the first frame of
    `data`, a Zstandard frame (ZSTD_KIND_FRAME; out_bound: a size its output always fits, the content size
    when the header has it) or a skippable one (ZSTD_KIND_SKIPPABLE; out_bound 0); status
    NX_ERR_ZSTD_TRUNCATED (-85) when `data` ends inside it."""
    import ctypes as C
    kind, fb, ob, fl = C.c_uint32(0), C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
    data = bytes(data)
    st = _lib.load().nx_zstd_next_frame(data, len(data), C.byref(kind), C.byref(fb), C.byref(ob), C.byref(fl))
    if st != 0:
        return st, 0, 0, 0, 0
    return 0, kind.value, fb.value, ob.value, fl.value


def bzip2_decode(inp, in_off, in_len, out, out_off, out_cap, split: bool = False, max_blocks=None):
    """One complete bzip2 stream per item (nx_bzip2_decode_batch): item i starts at inp[in_off[i]], only its
    first stream is decoded and bytes after it inside in_len[i] are left alone; it decodes into
    out[out_off[i] : + out_cap[i]].  Returns (out_len, consumed, status): the decoded size (on an error, the
    bytes of the blocks completed before it), the stream's compressed size and 0 or one NX_ERR_BZIP2_* code
    (-110 .. -124) per item.  A block with the randomised bit set is refused (NX_ERR_BZIP2_RANDOMISED, -124).

    split=True takes nx_bzip2_decode_batch_split: the same results item for item, a stream's blocks on several
    waves, and a fourth tensor, every item's chain length (the blocks that decoded).  max_blocks is the most
    candidates (block and end-of-stream magics, decoys included) the call lists over all items; an item whose
    candidates fall beyond it gets NX_ERR_BZIP2_DECODE_BLOCKS (-128).  The default runs bzip2_scan first and
    reads the count back, which synchronises; a caller that knows a bound passes it and the call does not."""
    n = in_len.numel()
    dev = inp.device
    out_len = torch.empty(n, dtype=torch.int32, device=dev)
    consumed = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    if not split:
        _chk(_lib.load().nx_bzip2_decode_batch(_ptr(inp), _ptr(in_off), _ptr(in_len), _ptr(out), _ptr(out_off), _ptr(out_cap),
                                               _ptr(out_len), _ptr(consumed), _ptr(status), n, _stream()), "nx_bzip2_decode_batch")
        return out_len, consumed, status
    if max_blocks is None:
        # a generous list for the pre-scan; should an item overflow even that, say so instead of passing it on
        _, _, count, sst = bzip2_scan(inp, in_off, in_len, max_blocks=int(in_len.sum().item()) // 6 + n + 1)
        if int((sst != 0).sum().item()):
            raise RuntimeError("bzip2_decode(split=True): the pre-scan's list overflowed; pass max_blocks")
        max_blocks = int(count.sum().item())
    blocks = torch.empty(n, dtype=torch.int32, device=dev)
    _chk(_lib.load().nx_bzip2_decode_batch_split(_ptr(inp), _ptr(in_off), _ptr(in_len), _ptr(out), _ptr(out_off), _ptr(out_cap),
                                                 _ptr(out_len), _ptr(consumed), _ptr(status), n, int(max_blocks), _ptr(blocks), _stream()),
         "nx_bzip2_decode_batch_split")
    return out_len, consumed, status, blocks


def bzip2_scan(inp, in_off, in_len, max_blocks: int):
    """nx_bzip2_scan_batch: every bit position of every item at which the block magic or the end-of-stream
    magic stands.  Returns (positions, first, count, status): item i's candidates are
    positions[first[i] : first[i] + count[i]] in ascending order, int64 with the sign bit (BZIP2_CAND_END) set for
    the end magic; status is 0, or NX_ERR_BZIP2_DECODE_BLOCKS (-128) with count 0 for an item whose candidates do
    not fit what is left of max_blocks."""
    n = in_len.numel()
    dev = inp.device
    positions = torch.zeros(max(int(max_blocks), 1), dtype=torch.int64, device=dev)
    first = torch.empty(n, dtype=torch.int32, device=dev)
    count = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    _chk(_lib.load().nx_bzip2_scan_batch(_ptr(inp), _ptr(in_off), _ptr(in_len), n, int(max_blocks), _ptr(positions), _ptr(first),
                                         _ptr(count), _ptr(status), _stream()), "nx_bzip2_scan_batch")
    return positions, first, count, status


BZIP2_CAND_END = -(1 << 63)  # NX_BZIP2_CAND_END as the sign bit of an int64 position


def bzip2_scan_host(data: bytes):
    """nx_bzip2_scan_host on host bytes: [(bit position, is_end)] of every magic in `data`, ascending (not a
    product path)."""
    import ctypes as C
    data = bytes(data)
    cnt = C.c_size_t(0)
    L = _lib.load()
    L.nx_bzip2_scan_host(data, len(data), None, 0, C.byref(cnt))
    pos = (C.c_uint64 * max(cnt.value, 1))()
    _chk(L.nx_bzip2_scan_host(data, len(data), pos, cnt.value, C.byref(cnt)), "nx_bzip2_scan_host")
    return [(v & ((1 << 63) - 1), bool(v >> 63)) for v in pos[:cnt.value]]


def bzip2_decode_block_host(data: bytes, bit_pos: int, level: int, out_cap: int):
    """nx_bzip2_decode_block_host on host bytes: the one block whose magic stands at bit_pos of a stream at
    `level`.  Returns (status, bytes, info) with info = dict(end_bit, pre_len, final_len, stored_crc,
    computed_crc) (not a product path)."""
    import ctypes as C
    data = bytes(data)
    buf = C.create_string_buffer(max(int(out_cap), 1))
    info = _lib.Bzip2BlockInfo()
    st = _lib.load().nx_bzip2_decode_block_host(data, len(data), int(bit_pos), int(level), C.cast(buf, C.c_void_p), int(out_cap),
                                                C.byref(info))
    got = buf.raw[:info.final_len] if st == 0 else b""
    return st, got, {k: getattr(info, k) for k in ("end_bit", "pre_len", "final_len", "stored_crc", "computed_crc")}


def bzip2_decode_split_host(data: bytes, out_cap: int, max_blocks=None):
    """nx_bzip2_decode_split_host on host bytes: (status, decoded bytes, consumed, blocks) of the first stream of
    `data` by scan, per-candidate decode and stitch on the CPU (not a product path); max_blocks defaults to no
    limit."""
    import ctypes as C
    data = bytes(data)
    buf = C.create_string_buffer(max(int(out_cap), 1))
    ol, cs, nb = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    mb = (1 << 62) if max_blocks is None else int(max_blocks)
    st = _lib.load().nx_bzip2_decode_split_host(data, len(data), C.cast(buf, C.c_void_p), int(out_cap), C.byref(ol), C.byref(cs), mb,
                                                C.byref(nb))
    return st, buf.raw[:ol.value], cs.value, nb.value


def bzip2_decoder_reserve(max_streams: int):
    """nx_bzip2_decoder_reserve: size the decoder's block workspace for max_streams streams in flight now and
    cap it there until workspaces_trim()."""
    _chk(_lib.load().nx_bzip2_decoder_reserve(int(max_streams), _stream()), "nx_bzip2_decoder_reserve")


def bzip2_decode_chains() -> int:
    """nx_bzip2_decode_chains: the sublists the kernel splits a block's inverse BWT walk into."""
    return _lib.load().nx_bzip2_decode_chains()


def bzip2_decode_host(data: bytes, out_cap: int):
    """nx_bzip2_decode_host on host bytes: (status, decoded bytes, consumed) of the first stream of `data`, by
    the kernel's format functions on the CPU (the tests' second opinion, not a product path)."""
    import ctypes as C
    data = bytes(data)
    buf = C.create_string_buffer(max(int(out_cap), 1))
    ol, cs = C.c_size_t(0), C.c_size_t(0)
    st = _lib.load().nx_bzip2_decode_host(data, len(data), C.cast(buf, C.c_void_p), int(out_cap), C.byref(ol), C.byref(cs))
    return st, buf.raw[:ol.value], cs.value


def brotli_decode(inp, in_off, in_len, out, out_off, out_cap):
    """One complete Brotli stream (RFC 7932) per item (nx_brotli_decode_batch): item i starts at inp[in_off[i]],
    bytes after its end inside in_len[i] are left alone; it decodes into out[out_off[i] : + out_cap[i]].  Returns
    (out_len, consumed, status): the decoded size (on an error, what was written before it), the stream's size
    through the byte that holds its last bit (0 on an error) and 0 or one NX_ERR_BROTLI_* code (-154 .. -171) per
    item, libbrotli's format errors one for one plus TRUNCATED (-170) and OUTPUT_FULL (-171)."""
    n = in_len.numel()
    dev = inp.device
    out_len = torch.empty(n, dtype=torch.int32, device=dev)
    consumed = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    _chk(_lib.load().nx_brotli_decode_batch(_ptr(inp), _ptr(in_off), _ptr(in_len), _ptr(out), _ptr(out_off), _ptr(out_cap),
                                            _ptr(out_len), _ptr(consumed), _ptr(status), n, _stream()), "nx_brotli_decode_batch")
    return out_len, consumed, status


def brotli_decoder_reserve(max_streams: int):
    """nx_brotli_decoder_reserve: size the decoder's tree workspace for max_streams streams in flight now and
    cap it there until workspaces_trim()."""
    _chk(_lib.load().nx_brotli_decoder_reserve(int(max_streams), _stream()), "nx_brotli_decoder_reserve")


def brotli_decode_host(data: bytes, out_cap: int, stats: bool = False):
    """nx_brotli_decode_host on host bytes: (status, decoded bytes, consumed) of the first stream of `data`, by
    the kernel's format functions on the CPU (the tests' second opinion, not a product path); with stats=True a
    fourth element, the nx_brotli_decode_stats census as a dict (arrays as lists)."""
    import ctypes as C
    data = bytes(data)
    buf = C.create_string_buffer(max(int(out_cap), 1))
    ol, cs = C.c_size_t(0), C.c_size_t(0)
    census = _lib.BrotliDecodeStats()
    st = _lib.load().nx_brotli_decode_host(data, len(data), C.cast(buf, C.c_void_p), int(out_cap), C.byref(ol), C.byref(cs),
                                           C.byref(census) if stats else None)
    if not stats:
        return st, buf.raw[:ol.value], cs.value
    d = {}
    for name, _ in census._fields_:
        v = getattr(census, name)
        d[name] = v if isinstance(v, int) else list(v)
    return st, buf.raw[:ol.value], cs.value, d


def brotli_transform_word(transform: int, word: bytes):
    """nx_brotli_transform_word: `word` (4..24 bytes) under transform 0..120 of RFC 7932 Appendix B."""
    import ctypes as C
    out = C.create_string_buffer(40)
    n = _lib.load().nx_brotli_transform_word(int(transform), bytes(word), len(word), C.cast(out, C.c_void_p))
    if n < 0:
        raise ValueError(f"nx_brotli_transform_word: {_lib.status_string(n)}")
    return out.raw[:n]


def brotli_dictionary() -> bytes:
    """nx_brotli_dictionary: the static dictionary of RFC 7932 Appendix A."""
    import ctypes as C
    size = C.c_size_t(0)
    p = _lib.load().nx_brotli_dictionary(C.byref(size))
    return C.string_at(p, size.value)


def bzip2_stream_info(data: bytes):
    """nx_bzip2_stream_info on host bytes: (status, level, first_block_crc, is_empty) from the first 14 bytes
    of `data`; status NX_ERR_BZIP2_TRUNCATED (-122) while fewer are there."""
    import ctypes as C
    data = bytes(data)
    lv, crc, em = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    st = _lib.load().nx_bzip2_stream_info(data, len(data), C.byref(lv), C.byref(crc), C.byref(em))
    if st != 0:
        return st, 0, 0, False
    return 0, lv.value, crc.value, bool(em.value)


def bzip2_max_compressed_length(n: int, level: int = 9) -> int:
    """nx_bzip2_max_compressed_length: a derived upper bound of the stream of an n-byte item at `level` (0 for
    a level outside 1..9)."""
    return _lib.load().nx_bzip2_max_compressed_length(int(n), int(level))


BZIP2_SEG_FIRST, BZIP2_SEG_LAST = 1, 2


def bzip2_encode(inp, in_off, in_len, out, out_off, out_cap, level: int = 9, split: bool = False, max_blocks=None, seg=None):
    """One bzip2 stream per item (nx_bzip2_encode_batch): item i = inp[in_off[i] : + in_len[i]] becomes what
    Bzip2Encoder writes for one encode(in) and close() at block size level x 100 000, in
    out[out_off[i] : + out_cap[i]] (slots may start at any byte; nothing is written outside them).  Returns
    (out_len, status): the stream's size and 0 or NX_ERR_BZIP2_ENCODE_FULL (-126) per item.  A level outside
    1..9 raises (NX_ERR_BZIP2_LEVEL, -125).
    split=True takes nx_bzip2_encode_batch_split: the same bytes, a stream's blocks on several workgroups.
    max_blocks is the most blocks the call lists (default: the sum of bzip2_blocks_bound over in_len, which
    reads in_len back); items beyond it get NX_ERR_BZIP2_ENCODE_BLOCKS (-127).  seg, split only: an int32 or
    uint32 device tensor of n x 4 (flags, carry_bits, carry_count, crc), read and written: the items are
    segments of streams (include/netty_amd.h)."""
    n = in_len.numel()
    dev = inp.device
    out_len = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    if not split:
        if max_blocks is not None or seg is not None:
            raise ValueError("max_blocks and seg belong to split=True")
        _chk(_lib.load().nx_bzip2_encode_batch(_ptr(inp), _ptr(in_off), _ptr(in_len), _ptr(out), _ptr(out_off), _ptr(out_cap),
                                               _ptr(out_len), _ptr(status), n, int(level), _stream()), "nx_bzip2_encode_batch")
        return out_len, status
    if max_blocks is None:
        max_blocks = sum(bzip2_blocks_bound(v, level) for v in in_len.cpu().tolist()) if 1 <= level <= 9 else 0
    if seg is not None and (seg.numel() != 4 * n or seg.element_size() != 4 or not seg.is_contiguous()):
        raise ValueError("seg: n x 4 32-bit values")
    _chk(_lib.load().nx_bzip2_encode_batch_split(_ptr(inp), _ptr(in_off), _ptr(in_len), _ptr(out), _ptr(out_off), _ptr(out_cap),
                                                 _ptr(out_len), _ptr(status), n, int(level), int(max_blocks), _ptr(seg), _stream()),
         "nx_bzip2_encode_batch_split")
    return out_len, status


def bzip2_blocks_bound(n: int, level: int = 9) -> int:
    """nx_bzip2_blocks_bound: the blocks of an n-byte item at `level`, at most (0 for n = 0)."""
    return _lib.load().nx_bzip2_blocks_bound(int(n), int(level))


def bzip2_plan(inp, in_off, in_len, level: int = 9):
    """nx_bzip2_plan_batch: the planner's launch alone; returns the int32 tensor of every item's block count."""
    n = in_len.numel()
    counts = torch.empty(n, dtype=torch.int32, device=inp.device)
    _chk(_lib.load().nx_bzip2_plan_batch(_ptr(inp), _ptr(in_off), _ptr(in_len), _ptr(counts), n, int(level), _stream()),
         "nx_bzip2_plan_batch")
    return counts


def bzip2_plan_host(data: bytes, level: int = 9, state=None, close: bool = True):
    """nx_bzip2_plan_host on host bytes: (status, cuts), the input end of every block of `data`.  With `state`
    (a list of three ints, updated in place; [0, 0, 0] at a stream's start) it is nx_bzip2_plan_resume_host: the
    planner continues from that state, and close=False leaves the open block open."""
    import ctypes as C
    data = bytes(data)
    L = _lib.load()
    cap = L.nx_bzip2_blocks_bound(len(data), int(level)) + 2
    cuts = (C.c_uint64 * cap)()
    cnt = C.c_size_t(0)
    if state is None:
        st = L.nx_bzip2_plan_host(data, len(data), int(level), cuts, cap, C.byref(cnt))
    else:
        s = (C.c_uint32 * 3)(*state)
        st = L.nx_bzip2_plan_resume_host(data, len(data), int(level), s, int(bool(close)), cuts, cap, C.byref(cnt))
        state[:] = list(s)
    return st, list(cuts[:min(cnt.value, cap)])


def bzip2_encode_segment_host(data: bytes, level: int, seg, out_cap=None):
    """nx_bzip2_encode_segment_host on host bytes: `data` is whole blocks of a stream, seg = (flags, carry_bits,
    carry_count, crc).  Returns (status, bytes, seg after)."""
    import ctypes as C
    data = bytes(data)
    cap = bzip2_max_compressed_length(len(data), level) + 8 if out_cap is None else int(out_cap)
    buf = C.create_string_buffer(max(cap, 1))
    ol = C.c_size_t(0)
    s = (C.c_uint32 * 4)(*seg)
    st = _lib.load().nx_bzip2_encode_segment_host(data, len(data), int(level), s, C.cast(buf, C.c_void_p), cap, C.byref(ol))
    return st, buf.raw[:ol.value], tuple(s)


def bzip2_encoder_reserve(max_streams: int, level: int = 9):
    """nx_bzip2_encoder_reserve: size the encoder's workspace for max_streams streams in flight at `level` now
    and cap it there until workspaces_trim()."""
    _chk(_lib.load().nx_bzip2_encoder_reserve(int(max_streams), int(level), _stream()), "nx_bzip2_encoder_reserve")


def bzip2_encoder_slot_bytes(level: int = 9) -> int:
    """nx_bzip2_encoder_slot_bytes: the workspace bytes of one stream in flight at `level`."""
    return _lib.load().nx_bzip2_encoder_slot_bytes(int(level))


def bzip2_encode_host(data: bytes, level: int = 9, out_cap=None):
    """nx_bzip2_encode_host on host bytes: (status, stream) of one item, by the kernel's format functions on the
    CPU (the tests' second opinion, not a product path); out_cap defaults to bzip2_max_compressed_length."""
    import ctypes as C
    data = bytes(data)
    cap = bzip2_max_compressed_length(len(data), level) if out_cap is None else int(out_cap)
    buf = C.create_string_buffer(max(cap, 1))
    ol = C.c_size_t(0)
    st = _lib.load().nx_bzip2_encode_host(data, len(data), int(level), C.cast(buf, C.c_void_p), cap, C.byref(ol))
    return st, buf.raw[:ol.value]


def lzma_max_compressed_length(n: int) -> int:
    """nx_lzma_max_compressed_length: 13 + n + n / 3 + 128, the LZMA SDK's allowance (not a proven bound)."""
    return _lib.load().nx_lzma_max_compressed_length(int(n))


def lzma_encode(inp, in_off, in_len, out, out_off, out_cap, lc: int = 3, lp: int = 0, pb: int = 2, dict_size: int = 65536,
                end_marker: bool = False):
    """One LZMA stream per item (nx_lzma_encode_batch): item i = inp[in_off[i] : + in_len[i]] becomes what
    LzmaFrameEncoder writes for one encode(in), header and payload, in out[out_off[i] : + out_cap[i]].  Returns
    (out_len, status): the stream's size and 0 or NX_ERR_LZMA_ENCODE_FULL (-143) per item.  out_cap is copied
    into out_len, which the call takes as capacities.  lc + lp > 4 raises (NX_ERR_LZMA_PROPS); the call reads
    in_len back, so it synchronises the current stream."""
    n = in_len.numel()
    dev = inp.device
    out_len = out_cap.to(device=dev, dtype=torch.int32, copy=True)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    _chk(_lib.load().nx_lzma_encode_batch(_ptr(inp), _ptr(in_off), _ptr(in_len), _ptr(out), _ptr(out_off), _ptr(out_len), _ptr(status),
                                          n, int(lc), int(lp), int(pb), int(dict_size), int(bool(end_marker)), _stream()),
         "nx_lzma_encode_batch")
    return out_len, status


def lzma_encode_host(data: bytes, lc: int = 3, lp: int = 0, pb: int = 2, dict_size: int = 65536, end_marker: bool = False,
                     out_cap=None, stats: bool = False, guard: int = 0):
    """nx_lzma_encode_host on host bytes: (status, stream) of one item, by the kernels' format functions on the
    CPU, for every lc, lp, pb; out_cap defaults to lzma_max_compressed_length.  stats=True appends the
    nx_lzma_encode_stats as a dict; guard > 0 appends the `guard` bytes behind out_cap (0xA5 before the call)."""
    import ctypes as C
    data = bytes(data)
    cap = lzma_max_compressed_length(len(data)) if out_cap is None else int(out_cap)
    buf = C.create_string_buffer(b"\xa5" * (cap + guard + 1), cap + guard + 1)
    S = _lib.LzmaEncodeStats()
    r = _lib.load().nx_lzma_encode_host(data, len(data), int(lc), int(lp), int(pb), int(dict_size), int(bool(end_marker)),
                                        C.cast(buf, C.c_void_p), cap, C.byref(S) if stats else None)
    res = [0 if r >= 0 else int(r), buf.raw[:r] if r >= 0 else b""]
    if stats:
        res.append({"literals": S.literals, "matched_literals": S.matched_literals, "matches": S.matches, "short_reps": S.short_reps,
                    "reps": list(S.reps), "carries": S.carries, "max_pending_ff": S.max_pending_ff, "max_carry_ff": S.max_carry_ff})
    if guard:
        res.append(buf.raw[cap:cap + guard])
    return tuple(res)


def brotli_max_compressed_length(n: int) -> int:
    """nx_brotli_max_compressed_length: n + 4 * ceil(n / 65536) + 3, a proven bound (csrc/brotli_encode_core.hpp)."""
    return _lib.load().nx_brotli_max_compressed_length(int(n))


def brotli_encode(inp, in_off, in_len, out, out_off, out_cap, lgwin: int = -1):
    """One Brotli stream per item (nx_brotli_encode_batch): item i = inp[in_off[i] : + in_len[i]] becomes a complete
    RFC 7932 stream in out[out_off[i] : + out_cap[i]].  Returns (out_len, status): the stream's size and 0 or
    NX_ERR_BROTLI_ENCODE_FULL (-153) per item.  out_cap is copied into out_len, which the call takes as
    capacities.  lgwin outside -1 and 10-24 raises; the call reads in_len back, so it synchronises the current
    stream."""
    n = in_len.numel()
    dev = inp.device
    out_len = out_cap.to(device=dev, dtype=torch.int32, copy=True)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    _chk(_lib.load().nx_brotli_encode_batch(_ptr(inp), _ptr(in_off), _ptr(in_len), _ptr(out), _ptr(out_off), _ptr(out_len), _ptr(status),
                                            n, int(lgwin), _stream()),
         "nx_brotli_encode_batch")
    return out_len, status


def brotli_encode_host(data: bytes, lgwin: int = -1, out_cap=None, stats: bool = False, guard: int = 0):
    """nx_brotli_encode_host on host bytes: (status, stream) of one item, by the kernels' format functions on the
    CPU; out_cap defaults to brotli_max_compressed_length.  stats=True appends the nx_brotli_encode_stats as a
    dict; guard > 0 appends the `guard` bytes behind out_cap (0xA5 before the call)."""
    import ctypes as C
    data = bytes(data)
    cap = brotli_max_compressed_length(len(data)) if out_cap is None else int(out_cap)
    buf = C.create_string_buffer(b"\xa5" * (cap + guard + 1), cap + guard + 1)
    S = _lib.BrotliEncodeStats()
    r = _lib.load().nx_brotli_encode_host(data, len(data), int(lgwin), C.cast(buf, C.c_void_p), cap, C.byref(S) if stats else None)
    res = [0 if r >= 0 else int(r), buf.raw[:r] if r >= 0 else b""]
    if stats:
        res.append({k: (list(getattr(S, k)) if k == "simple_codes" else getattr(S, k)) for k, _ in S._fields_})
    if guard:
        res.append(buf.raw[cap:cap + guard])
    return tuple(res)


INFLATE_STATE_BYTES = 512
INFLATE_NEED_INPUT, INFLATE_OUTPUT_FULL = 2, 3


def inflate(inp, in_off, in_len, out, out_off, hist_len, out_cap, state):
    """Resumable raw inflate per stream (nx_inflate_batch).  Stream i reads inp[in_off[i] : + in_len[i]];
    its window is out[out_off[i]:], whose first hist_len[i] bytes are its last output and which takes
    at most out_cap[i] new bytes after them; state is a uint8 tensor of INFLATE_STATE_BYTES per
    stream (zeros at the start of a stream), updated in place.  Returns (consumed, out_len, status):
    status 0 at the end of the stream, INFLATE_NEED_INPUT, INFLATE_OUTPUT_FULL or zlib's error."""
    n = in_len.numel()
    dev = inp.device
    assert state.numel() >= n * INFLATE_STATE_BYTES and state.dtype == torch.uint8
    consumed = torch.empty(n, dtype=torch.int32, device=dev)
    out_len = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    _chk(_lib.load().nx_inflate_batch(_ptr(inp), _ptr(in_off), _ptr(in_len), _ptr(out), _ptr(out_off), _ptr(hist_len),
                                      _ptr(out_cap), _ptr(state), _ptr(consumed), _ptr(out_len), _ptr(status), n, _stream()),
         "nx_inflate_batch")
    return consumed, out_len, status


def lzf_encode(inp, in_off, in_len, out, out_off):
    n = in_len.numel()
    dev = inp.device
    out_len = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    _chk(_lib.load().nx_lzf_encode_batch(_ptr(inp), _ptr(in_off), _ptr(in_len), _ptr(out), _ptr(out_off), _ptr(out_len),
                                         _ptr(status), n, _stream()), "nx_lzf_encode_batch")
    return out_len, status


def lzf_decode(inp, in_off, in_len, out, out_off, out_len):
    n = in_len.numel()
    status = torch.empty(n, dtype=torch.int32, device=inp.device)
    _chk(_lib.load().nx_lzf_decode_batch(_ptr(inp), _ptr(in_off), _ptr(in_len), _ptr(out), _ptr(out_off), _ptr(out_len),
                                         _ptr(status), n, _stream()), "nx_lzf_decode_batch")
    return status


def lz4_max_compressed_length(n: int) -> int:
    return _lib.load().nx_lz4_max_compressed_length(n)


def lz4_encode(inp, in_off, in_len, out, out_off, high: bool = False):
    """LZ4 block encode per chunk (nx_lz4_encode_batch; high: lz4-java's highCompressor(), liblz4's
    LZ4_compress_HC level 9, nx_lz4hc_encode_batch).  Returns (out_len, status)."""
    n = in_len.numel()
    dev = inp.device
    out_len = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    name = "nx_lz4hc_encode_batch" if high else "nx_lz4_encode_batch"
    _chk(getattr(_lib.load(), name)(_ptr(inp), _ptr(in_off), _ptr(in_len), _ptr(out), _ptr(out_off), _ptr(out_len),
                                    _ptr(status), n, _stream()), name)
    return out_len, status


def lz4_decode(inp, in_off, in_len, out, out_off, out_len):
    """LZ4 block decode per chunk to exactly out_len[i] bytes (nx_lz4_decode_batch).  Returns status."""
    n = in_len.numel()
    status = torch.empty(n, dtype=torch.int32, device=inp.device)
    _chk(_lib.load().nx_lz4_decode_batch(_ptr(inp), _ptr(in_off), _ptr(in_len), _ptr(out), _ptr(out_off), _ptr(out_len),
                                         _ptr(status), n, _stream()), "nx_lz4_decode_batch")
    return status


LZ4_DEFAULT_SEED = 0x9747B28C  # Lz4Constants.java:70


def xxhash32(inp, off, length, seed: int = LZ4_DEFAULT_SEED, out=None):
    """XXH32 per block (nx_xxhash32_batch), unmasked; Lz4XXHash32.getValue() is this & 0x0FFFFFFF."""
    n = length.numel()
    out = torch.empty(n, dtype=torch.int32, device=inp.device) if out is None else out
    _chk(_lib.load().nx_xxhash32_batch(_ptr(inp), _ptr(off), _ptr(length), seed & 0xFFFFFFFF, _ptr(out), n, _stream()),
         "nx_xxhash32_batch")
    return out


def lz4_frame_encode(inp, in_off, in_len, out, out_off, compression_level: int = 6, high: bool = False):
    """Lz4FrameEncoder.flushBufferedData per block (nx_lz4_frame_encode_batch_ex): header + block in each
    out slot (capacity 21 + lz4_max_compressed_length); high = the highCompressor flag.
    Returns (out_len, status)."""
    n = in_len.numel()
    dev = inp.device
    out_len = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    _chk(_lib.load().nx_lz4_frame_encode_batch_ex(_ptr(inp), _ptr(in_off), _ptr(in_len), _ptr(out), _ptr(out_off),
                                                  _ptr(out_len), int(compression_level), int(bool(high)), _ptr(status), n,
                                                  _stream()),
         "nx_lz4_frame_encode_batch_ex")
    return out_len, status


def lz4_frame_scan(inp, in_off, in_len, state, cap: int):
    """Lz4FrameDecoder's block walk over device cumulations (nx_lz4_frame_scan_batch).  state: int32
    tensor (finished | corrupted << 1), updated in place.  Returns a dict of tensors: consumed, status,
    counts [compressed, non-compressed, claims] and the list arrays data_off, comp_len, decomp_len,
    checksum, stream, seq (compressed at [0, counts[0]), non-compressed at [cap - counts[1], cap))."""
    n = in_len.numel()
    dev = inp.device
    c = max(int(cap), 1)
    r = {"consumed": torch.empty(n, dtype=torch.int64, device=dev),
         "status": torch.empty(n, dtype=torch.int32, device=dev),
         "data_off": torch.empty(c, dtype=torch.int64, device=dev),
         "comp_len": torch.empty(c, dtype=torch.int32, device=dev),
         "decomp_len": torch.empty(c, dtype=torch.int32, device=dev),
         "checksum": torch.empty(c, dtype=torch.int32, device=dev),
         "stream": torch.empty(c, dtype=torch.int32, device=dev),
         "seq": torch.empty(c, dtype=torch.int32, device=dev),
         "counts": torch.empty(3, dtype=torch.int32, device=dev)}
    _chk(_lib.load().nx_lz4_frame_scan_batch(_ptr(inp), _ptr(in_off), _ptr(in_len), _ptr(state), _ptr(r["consumed"]),
                                             _ptr(r["status"]), _ptr(r["data_off"]), _ptr(r["comp_len"]),
                                             _ptr(r["decomp_len"]), _ptr(r["checksum"]), _ptr(r["stream"]), _ptr(r["seq"]),
                                             _ptr(r["counts"]), int(cap), n, _stream()), "nx_lz4_frame_scan_batch")
    return r


def lz4_frame_decode(inp, scan: dict, cap: int, validate_checksums: bool = True):
    """The data half of Lz4FrameDecoder.decode (Lz4FrameDecoder.java:184-229) for the blocks a scan listed:
    compressed blocks are decoded into one output buffer (slots packed by decomp_len), non-compressed
    blocks stay where they are in `inp` (Java's retainedSlice, :197-199).  With validate_checksums the
    masked XXH32 of every block's bytes is compared with its header (:226-228).
    Returns {"compressed": (out, out_off, status), "raw": (data_off, len, status)} over the two list ranges."""
    nc, nu = (int(v) for v in scan["counts"][:2].tolist())
    dev = inp.device
    dl = scan["decomp_len"][:nc].to(torch.int64)
    out_off = torch.cumsum(dl, 0) - dl
    total = int(dl.sum().item()) if nc else 0
    out = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
    st_c = lz4_decode(inp, scan["data_off"][:nc], scan["comp_len"][:nc], out, out_off, scan["decomp_len"][:nc]) if nc \
        else torch.empty(0, dtype=torch.int32, device=dev)
    lo = cap - nu
    r_off, r_len = scan["data_off"][lo:cap], scan["decomp_len"][lo:cap]
    st_u = torch.zeros(nu, dtype=torch.int32, device=dev)
    if validate_checksums:
        bad = torch.tensor(-56, dtype=torch.int32, device=dev)  # NX_ERR_LZ4_CHECKSUM_MISMATCH
        if nc:
            hc = xxhash32(out, out_off, scan["decomp_len"][:nc]) & 0x0FFFFFFF
            st_c = torch.where((st_c == 0) & (hc != scan["checksum"][:nc]), bad, st_c)
        if nu:
            hu = xxhash32(inp, r_off, r_len) & 0x0FFFFFFF
            st_u = torch.where(hu != scan["checksum"][lo:cap], bad, st_u)
    return {"compressed": (out, out_off, st_c), "raw": (r_off, r_len, st_u)}


def textgen(out, first_chunk: int, n_chunks: int, chunk_len: int):
    """Fill out[k*chunk_len:(k+1)*chunk_len] with text-like chunk first_chunk+k."""
    _chk(_lib.load().nx_textgen_device(_ptr(out), first_chunk, n_chunks, chunk_len, _stream()), "nx_textgen_device")
    return out


def gather(src, src_off, length, dst=None, dst_off=None):
    """Pack chunk i = src[src_off[i] : +length[i]] contiguously (nx_pack_batch).  dst_off defaults
    to the exclusive scan of length.  Returns (dst, dst_off)."""
    n = length.numel()
    if dst_off is None:
        dst_off = torch.zeros(n, dtype=torch.int64, device=src.device)
        if n > 1:
            torch.cumsum(length[:-1].to(torch.int64), 0, out=dst_off[1:])
    if dst is None:
        total = int((dst_off[-1] + length[-1].to(torch.int64)).item()) if n else 0
        dst = torch.empty(max(total, 1), dtype=torch.uint8, device=src.device)
    _chk(_lib.load().nx_pack_batch(_ptr(src), _ptr(src_off), _ptr(length), _ptr(dst), _ptr(dst_off), n, _stream()),
         "nx_pack_batch")
    return dst, dst_off


def pack(chunks: list[bytes], device, align: int = 16, pad: int = 0):
    """Pack host chunks into one device tensor; returns (data, off[int64], len[int32])."""
    offs, cur = [], 0
    for c in chunks:
        offs.append(cur)
        cur += (len(c) + align - 1) // align * align
    buf = bytearray(cur + pad + 16)
    for o, c in zip(offs, chunks):
        buf[o:o + len(c)] = c
    data = torch.frombuffer(buf, dtype=torch.uint8).to(device)  # buf is a fresh bytearray, copied by .to()
    off = torch.tensor(offs, dtype=torch.int64, device=device)
    ln = torch.tensor([len(c) for c in chunks], dtype=torch.int32, device=device)
    return data, off, ln


def out_slots(lengths: list[int], device, align: int = 16):
    offs, cur = [], 0
    for n in lengths:
        offs.append(cur)
        cur += (n + align - 1) // align * align
    data = torch.zeros(cur + 16, dtype=torch.uint8, device=device)
    return data, torch.tensor(offs, dtype=torch.int64, device=device)
