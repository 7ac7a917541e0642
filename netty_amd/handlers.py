"""Netty's codec-compression handler API over the GPU path.

Mirrors the public surface of the reference handlers (same names, constructor options,
encode/decode contracts and error behaviour):

* ``SnappyFrameEncoder()`` / ``SnappyFrameEncoder.snappy_encoder_with_jumbo_frames()``
  — SnappyFrameEncoder.java:60-117
* ``SnappyFrameDecoder(validate_checksums=False)`` — SnappyFrameDecoder.java:67-231
* ``FastLzFrameEncoder(level=0, checksum=False)`` — FastLzFrameEncoder.java:58-172
* ``FastLzFrameDecoder(validate_checksums=False)`` — FastLzFrameDecoder.java:90-207
* ``LzfEncoder(compress_threshold=16)`` / ``LzfDecoder()`` — LzfEncoder.java / LzfDecoder.java

Encoders follow ``MessageToByteEncoder.write`` (MessageToByteEncoder.java:99-131): one call per
outbound message, empty output replaced by an empty buffer.  Decoders follow
``ByteToMessageDecoder.channelRead`` (ByteToMessageDecoder.java:286-341): inbound bytes are
cumulated, ``decode`` runs until it stops making progress, consumed bytes are discarded, and a
failure raises ``DecompressionException`` and leaves the decoder corrupted (all later input is
skipped).  The per-chunk work runs in libnetty_amd.so (HIP kernels); headers are parsed by the
native host layer exactly as the Java decode() does.
"""
from __future__ import annotations

import ctypes as C
import enum

from . import _lib


class DecoderException(Exception):
    """io.netty.handler.codec.DecoderException"""


class EncoderException(Exception):
    """io.netty.handler.codec.EncoderException"""


class DecompressionException(DecoderException):
    """DecompressionException.java:23"""


class IllegalStateException(Exception):
    """java.lang.IllegalStateException (Lz4FrameEncoder.encode after close, Lz4FrameEncoder.java:233-239)"""


class CompressionException(EncoderException):
    """CompressionException.java:23"""


def _new(handle, what):
    if not handle:
        raise RuntimeError(f"{what}: native handle creation failed (no GPU visible, or invalid options); "
                           f"the HIP path has no CPU fallback")
    return handle


class _Encoder:
    """MessageToByteEncoder<ByteBuf> template (MessageToByteEncoder.java:99-160)."""

    _free = None

    def encode(self, data: bytes) -> bytes:  # pragma: no cover - overridden
        raise NotImplementedError

    def write(self, msg) -> bytes:
        return self.encode(bytes(msg))

    def close(self):
        if getattr(self, "_h", None):
            getattr(_lib.load(), self._free)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Decoder:
    """ByteToMessageDecoder template (ByteToMessageDecoder.java:286-341, callDecode :464-517)."""

    _free = None
    _decode_fn = None

    def __init__(self):
        self._cum = bytearray()

    def channel_read(self, data) -> list[bytes]:
        L = _lib.load()
        self._cum += bytes(data)
        buf = bytes(self._cum)
        consumed = C.c_size_t(0)
        msgs = C.POINTER(_lib.NxMsg)()
        nmsg = C.c_size_t(0)
        err = C.c_char_p()
        rc = getattr(L, self._decode_fn)(self._h, buf, len(buf), C.byref(consumed), C.byref(msgs), C.byref(nmsg),
                                         C.byref(err))
        out = [C.string_at(msgs[i].data, msgs[i].len) if msgs[i].len else b"" for i in range(nmsg.value)]
        del self._cum[:consumed.value]
        if rc != 0:
            if rc in (-100, -101, -102, -103):
                raise RuntimeError(f"{type(self).__name__}: native failure {rc} ({_lib.status_string(rc)})")
            msg = err.value.decode() if err.value else _lib.status_string(rc)
            # a ByteBuf failure (IndexOutOfBounds / IllegalArgument) reaches the pipeline as the
            # DecoderException ByteToMessageDecoder wraps it in (ByteToMessageDecoder.java:297-300)
            e = DecoderException(msg) if msg.startswith("java.lang.") else DecompressionException(msg)
            e.decoded = out  # messages fired before the failing chunk
            e.status = rc
            raise e
        return out

    def readable_bytes(self) -> int:
        return len(self._cum)

    def close(self):
        if getattr(self, "_h", None):
            getattr(_lib.load(), self._free)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------------------------------------------- Snappy
class SnappyFrameEncoder(_Encoder):
    """SnappyFrameEncoder.java:29-153 — 32767-byte slices (65535 with jumbo frames)."""

    _free = "nx_snappy_frame_encoder_free"

    def __init__(self, jumbo: bool = False):
        self._h = _new(_lib.load().nx_snappy_frame_encoder_new(1 if jumbo else 0), "SnappyFrameEncoder")

    @classmethod
    def snappy_encoder_with_jumbo_frames(cls) -> "SnappyFrameEncoder":
        return cls(jumbo=True)

    def encode(self, data: bytes) -> bytes:
        L = _lib.load()
        cap = L.nx_snappy_frame_max_encoded_length(len(data))
        out = (C.c_uint8 * max(cap, 1))()
        n = L.nx_snappy_frame_encoder_encode(self._h, data, len(data), out, cap)
        if n < 0:
            raise CompressionException(_lib.status_string(n))
        return bytes(out[:n])


class SnappyFrameDecoder(_Decoder):
    """SnappyFrameDecoder.java:37-259 (validateChecksums defaults to false, :67-69)."""

    _free = "nx_snappy_frame_decoder_free"
    _decode_fn = "nx_snappy_frame_decoder_decode"

    def __init__(self, validate_checksums: bool = False):
        super().__init__()
        self._h = _new(_lib.load().nx_snappy_frame_decoder_new(1 if validate_checksums else 0), "SnappyFrameDecoder")


# Deprecated aliases kept by the reference (SnappyFramedEncoder.java:22, SnappyFramedDecoder.java:22)
SnappyFramedEncoder = SnappyFrameEncoder
SnappyFramedDecoder = SnappyFrameDecoder


# ------------------------------------------------------------------------------------- FastLZ
LEVEL_AUTO, LEVEL_1, LEVEL_2 = 0, 1, 2


class FastLzFrameEncoder(_Encoder):
    """FastLzFrameEncoder.java:45-173.  ``reader_index`` of encode() reproduces the readU16 quirk."""

    _free = "nx_fastlz_frame_encoder_free"

    def __init__(self, level: int = LEVEL_AUTO, checksum: bool = False):
        if level not in (LEVEL_AUTO, LEVEL_1, LEVEL_2):
            raise ValueError(f"level: {level} (expected: {LEVEL_AUTO} or {LEVEL_1} or {LEVEL_2})")
        self._h = _new(_lib.load().nx_fastlz_frame_encoder_new(level, 1 if checksum else 0), "FastLzFrameEncoder")

    def encode(self, data: bytes, reader_index: int = 0, buffer: bytes | None = None) -> bytes:
        """Encode ``data``; if ``buffer``/``reader_index`` are given, data = buffer[reader_index:]."""
        L = _lib.load()
        if buffer is None:
            buffer, reader_index = bytes(reader_index) + bytes(data), reader_index
        n = len(buffer) - reader_index
        cap = L.nx_fastlz_frame_max_encoded_length(n)
        out = (C.c_uint8 * max(cap, 1))()
        r = L.nx_fastlz_frame_encoder_encode(self._h, bytes(buffer), reader_index, n, out, cap)
        if r < 0:
            raise CompressionException(_lib.status_string(r))
        return bytes(out[:r])


class FastLzFrameDecoder(_Decoder):
    """FastLzFrameDecoder.java:36-208."""

    _free = "nx_fastlz_frame_decoder_free"
    _decode_fn = "nx_fastlz_frame_decoder_decode"

    def __init__(self, validate_checksums: bool = False):
        super().__init__()
        self._h = _new(_lib.load().nx_fastlz_frame_decoder_new(1 if validate_checksums else 0), "FastLzFrameDecoder")


# ------------------------------------------------------------------------------------- LZF
class LzfEncoder(_Encoder):
    """LzfEncoder.java:36-253: LzfEncoder(totalLength = MAX_CHUNK_LEN, compressThreshold = 16)
    (:111-166).  total_length is validated as the reference does and does not change the bytes
    (include/netty_amd.h, nx_lzf_encoder_new_ex)."""

    _free = "nx_lzf_encoder_free"
    MAX_CHUNK_LEN = 65535  # LZFChunk.MAX_CHUNK_LEN
    MIN_BLOCK_TO_COMPRESS = 16  # LzfEncoder.java:42

    def __init__(self, compress_threshold: int = 16, total_length: int = MAX_CHUNK_LEN):
        if total_length < 16 or total_length > 65535:  # :147-150
            raise ValueError(f"totalLength: {total_length} (expected: 16-65535)")
        if compress_threshold < 16:  # :152-156
            raise ValueError(f"compressThreshold:{compress_threshold} expected >=16")
        self._h = _new(_lib.load().nx_lzf_encoder_new_ex(total_length, compress_threshold), "LzfEncoder")

    def encode(self, data: bytes) -> bytes:
        L = _lib.load()
        cap = L.nx_lzf_frame_max_encoded_length(len(data))
        out = (C.c_uint8 * max(cap, 1))()
        r = L.nx_lzf_encoder_encode(self._h, data, len(data), out, cap)
        if r < 0:
            raise CompressionException(_lib.status_string(r))
        return bytes(out[:r])


class LzfDecoder(_Decoder):
    """LzfDecoder.java:40-242."""

    _free = "nx_lzf_decoder_free"
    _decode_fn = "nx_lzf_decoder_decode"

    def __init__(self):
        super().__init__()
        self._h = _new(_lib.load().nx_lzf_decoder_new(), "LzfDecoder")


class Lz4FrameEncoder(_Encoder):
    """Lz4FrameEncoder.java:61-403 (XXHash32 seed 0x9747b28c).  high_compressor selects lz4-java's
    highCompressor() (liblz4 LZ4_compress_HC level 9) over fastCompressor() (:121-125,161-163);
    max_encode_size is the maxEncodeSize constructor argument (:150-170, default Integer.MAX_VALUE).
    encode() returns the full blocks it flushed (a partial block stays buffered, :231-248); flush()
    writes the partial block (:296-304); finish_encode() = close(): flush + end block (:306-330).
    encode() and flush() raise EncoderException when the pending bytes' output would exceed
    max_encode_size (allocateBuffer, :190-214), leaving the encoder unchanged."""

    _free = "nx_lz4_frame_encoder_free"
    MAX_ENCODE_SIZE = (1 << 31) - 1  # DEFAULT_MAX_ENCODE_SIZE (:68)

    def __init__(self, block_size: int = 1 << 16, high_compressor: bool = False, max_encode_size: int = MAX_ENCODE_SIZE):
        if not 64 <= block_size <= 1 << 25:
            raise ValueError(f"blockSize: {block_size} (expected: 64-{1 << 25})")
        if max_encode_size <= 0:  # ObjectUtil.checkPositive (:168)
            raise ValueError(f"maxEncodeSize : {max_encode_size} (expected: > 0)")
        self.block_size = block_size
        self.high_compressor = bool(high_compressor)
        self.max_encode_size = int(max_encode_size)
        self._h = _new(_lib.load().nx_lz4_frame_encoder_new_ex(block_size, int(self.high_compressor), self.max_encode_size),
                       "Lz4FrameEncoder")

    def _out(self, n: int):
        cap = _lib.load().nx_lz4_frame_max_encoded_length(n, self.block_size)
        return (C.c_uint8 * cap)(), cap

    def raise_for(self, r):
        """the reference's exception for a handle status: NX_ERR_LZ4_ENCODE_SIZE (-58) is allocateBuffer's
        EncoderException, NX_ERR_LZ4_ENCODE_FINISHED (-59) encode's IllegalStateException after close"""
        if r == -58:
            raise EncoderException(_lib.load().nx_lz4_frame_encoder_error(self._h).decode())
        if r == -59:
            raise IllegalStateException(_lib.load().nx_lz4_frame_encoder_error(self._h).decode())

    def _ret(self, r, out) -> bytes:
        self.raise_for(r)
        if r < 0:
            raise CompressionException(_lib.status_string(r))
        return bytes(out[:r])

    def encode(self, data: bytes) -> bytes:
        out, cap = self._out(len(data) + self.block_size)
        return self._ret(_lib.load().nx_lz4_frame_encoder_encode(self._h, data, len(data), out, cap), out)

    def flush(self) -> bytes:
        out, cap = self._out(self.block_size)
        return self._ret(_lib.load().nx_lz4_frame_encoder_flush(self._h, out, cap), out)

    def finish_encode(self) -> bytes:
        out, cap = self._out(self.block_size)
        return self._ret(_lib.load().nx_lz4_frame_encoder_close(self._h, out, cap), out)


class ZstdEncoder(_Encoder):
    """ZstdEncoder.java:90-193 over the GPU Zstandard frame encoder.  encode() returns the frames of the
    blocks it filled (a partial block stays buffered, :134-143), flush() the frame of the pending bytes
    (:171-178; nothing when nothing is pending).  Each block of block_size bytes is one complete frame
    (a block over 64 KiB: consecutive frames of 64 KiB slices), which any Zstandard decoder reads as one
    stream; the bytes differ from zstd-jni's.  Every level runs the one matcher.  encode() and flush()
    raise EncoderException when the pending bytes' compressBound sum exceeds max_encode_size
    (allocateBuffer, :105-122), leaving the encoder unchanged.  There is no finish: close() drops
    buffered bytes as handlerRemoved does (:187-193)."""

    _free = "nx_zstd_encoder_free"
    MIN_COMPRESSION_LEVEL, MAX_COMPRESSION_LEVEL = -131072, 22  # Zstd.minCompressionLevel() / maxCompressionLevel()
    MAX_BLOCK_SIZE = 1 << 25  # ZstdConstants.java:40: 1 << (3 + 7) + 0x0F, 32 MiB by operator precedence

    def __init__(self, compression_level: int = 3, block_size: int = 1 << 16, max_encode_size: int = MAX_BLOCK_SIZE):
        if not self.MIN_COMPRESSION_LEVEL <= compression_level <= self.MAX_COMPRESSION_LEVEL:  # ObjectUtil.checkInRange (:92-93)
            raise ValueError(f"compressionLevel: {compression_level} (expected: {self.MIN_COMPRESSION_LEVEL}-{self.MAX_COMPRESSION_LEVEL})")
        if block_size <= 0:  # ObjectUtil.checkPositive (:94)
            raise ValueError(f"blockSize : {block_size} (expected: > 0)")
        if max_encode_size <= 0:  # (:95)
            raise ValueError(f"maxEncodeSize : {max_encode_size} (expected: > 0)")
        self.compression_level = int(compression_level)
        self.block_size = int(block_size)
        self.max_encode_size = int(max_encode_size)
        self._h = _new(_lib.load().nx_zstd_encoder_new(self.compression_level, self.block_size, self.max_encode_size), "ZstdEncoder")

    def _out(self, n: int):
        cap = _lib.load().nx_zstd_max_encoded_length(n, self.block_size)
        return (C.c_uint8 * cap)(), cap

    def _ret(self, r, out) -> bytes:
        if r == -80:  # NX_ERR_ZSTD_ENCODE_SIZE: allocateBuffer's EncoderException
            raise EncoderException(_lib.load().nx_zstd_encoder_error(self._h).decode())
        if r < 0:
            raise CompressionException(_lib.status_string(r))
        return bytes(out[:r])

    def encode(self, data: bytes) -> bytes:
        out, cap = self._out(len(data) + self.block_size)
        return self._ret(_lib.load().nx_zstd_encoder_encode(self._h, data, len(data), out, cap), out)

    def flush(self) -> bytes:
        out, cap = self._out(self.block_size)
        return self._ret(_lib.load().nx_zstd_encoder_flush(self._h, out, cap), out)


class LzmaFrameEncoder(_Encoder):
    """LzmaFrameEncoder.java:97-213 over the GPU LZMA encoder.  Every encode() returns one complete stream: the
    13 header bytes (properties, dictionary size, the exact length) and the payload coded from a fresh model;
    an empty write gives 18 bytes.  Nothing is kept between writes and close() writes nothing.  The
    reference's shorter constructors, LzmaFrameEncoder(), (lc, lp, pb), (dictionarySize) and (lc, lp, pb,
    dictionarySize), are the keyword defaults.  num_fast_bytes is checked and does not change the bytes (it
    steers lzma-java's optimal parser; this encoder parses greedily).  lc + lp > 4 is accepted as the reference
    accepts it (it logs a warning: current decoder libraries refuse such streams) and is encoded on the host by
    the same format code, since the kernel keeps the model in LDS."""

    _free = "nx_lzma_frame_encoder_free"
    MIN_FAST_BYTES, MAX_FAST_BYTES = 5, 273  # LzmaFrameEncoder.java:45-50

    def __init__(self, lc: int = 3, lp: int = 0, pb: int = 2, dictionary_size: int = 65536, end_marker_mode: bool = False,
                 num_fast_bytes: int = 32):
        if lc < 0 or lc > 8:  # :139-141
            raise ValueError(f"lc: {lc} (expected: 0-8)")
        if lp < 0 or lp > 4:  # :142-144
            raise ValueError(f"lp: {lp} (expected: 0-4)")
        if pb < 0 or pb > 4:  # :145-147
            raise ValueError(f"pb: {pb} (expected: 0-4)")
        if dictionary_size < 0:  # :157-159
            raise ValueError(f"dictionarySize: {dictionary_size} (expected: 0+)")
        if num_fast_bytes < self.MIN_FAST_BYTES or num_fast_bytes > self.MAX_FAST_BYTES:  # :160-164
            raise ValueError(f"numFastBytes: {num_fast_bytes} (expected: {self.MIN_FAST_BYTES}-{self.MAX_FAST_BYTES})")
        self.lc, self.lp, self.pb = int(lc), int(lp), int(pb)
        self.dictionary_size = int(dictionary_size)
        self.end_marker_mode = bool(end_marker_mode)
        self.num_fast_bytes = int(num_fast_bytes)
        self._h = _new(_lib.load().nx_lzma_frame_encoder_new(self.lc, self.lp, self.pb, self.dictionary_size, int(self.end_marker_mode),
                                                             self.num_fast_bytes), "LzmaFrameEncoder")

    def encode(self, data: bytes) -> bytes:
        cap = _lib.load().nx_lzma_frame_max_encoded_length(len(data))
        out = (C.c_uint8 * cap)()
        r = _lib.load().nx_lzma_frame_encoder_encode(self._h, data, len(data), out, cap)
        if r < 0:
            err = _lib.load().nx_lzma_frame_encoder_error(self._h)
            raise CompressionException(err.decode() if err else _lib.status_string(r))
        return bytes(out[:r])


class BrotliEncoder(_Encoder):
    """BrotliEncoder.java:47-230 over the GPU Brotli encoder: one stream per channel, every write compressed and
    flushed.  encode() of an empty message returns b"" and changes nothing; any other returns whole bytes that
    end in libbrotli's flush marker (the first begin with the WBITS header), so the writes so far plus b"\\x03"
    are always a complete stream.  finish_encode() (the handler's close) returns the last block (after the header, if
    nothing was written), a second one b"", and encode() after it b"" as the reference's allocateBuffer does.  quality (-1, 0-11),
    window (-1, 10-24) and mode are brotli4j's Encoder.Parameters with BrotliOptions.DEFAULT as defaults; quality
    and mode are checked and do not change the bytes (this encoder parses greedily).  Copies do not reach into
    earlier writes."""

    _free = "nx_brotli_encoder_free"
    GENERIC, TEXT, FONT = 0, 1, 2  # Encoder.Mode

    def __init__(self, quality: int = 4, window: int = -1, mode: int = 1):
        if quality < -1 or quality > 11:
            raise ValueError("quality should be in range [0, 11], or -1")
        if window != -1 and (window < 10 or window > 24):
            raise ValueError("lgwin should be in range [10, 24], or -1")
        if mode not in (self.GENERIC, self.TEXT, self.FONT):
            raise ValueError("mode should be GENERIC, TEXT or FONT")
        self.quality, self.window, self.mode = int(quality), int(window), int(mode)
        self._h = _new(_lib.load().nx_brotli_encoder_new(self.quality, self.window, self.mode), "BrotliEncoder")

    def _ret_or_raise(self, r, out):
        if r < 0:
            err = _lib.load().nx_brotli_encoder_error(self._h)
            raise CompressionException(err.decode() if err else _lib.status_string(r))
        return bytes(out[:r])

    def encode(self, data: bytes) -> bytes:
        cap = _lib.load().nx_brotli_encoder_max_encoded_length(len(data))
        out = (C.c_uint8 * cap)()
        return self._ret_or_raise(_lib.load().nx_brotli_encoder_encode(self._h, data, len(data), out, cap), out)

    def finish_encode(self) -> bytes:
        out = (C.c_uint8 * 8)()
        return self._ret_or_raise(_lib.load().nx_brotli_encoder_close(self._h, out, 8), out)

    def is_closed(self) -> bool:
        return bool(_lib.load().nx_brotli_encoder_is_closed(self._h))


class Bzip2Encoder(_Encoder):
    """Bzip2Encoder.java:96-228 over the GPU bzip2 encoder's split path: one stream over any number of writes,
    the same bytes however the writes slice the input.  The first encode() writes "BZh" and the level digit;
    a write that closes k blocks encodes them in one launch on k workgroups and returns the 32-bit words they
    complete (a block that is not full yet stays in host memory); finish_encode() = close(): the open block,
    the footer and the padding, after which encode() passes its input through (:107-110) and a second
    finish_encode() returns nothing.  finish_encode() on an encoder that was never written to returns the
    whole 14-byte empty stream (the Java writes the footer alone)."""

    _free = "nx_bzip2_encoder_free"
    MIN_BLOCK_SIZE, MAX_BLOCK_SIZE = 1, 9  # Bzip2Constants.java

    def __init__(self, block_size_multiplier: int = MAX_BLOCK_SIZE):
        if not self.MIN_BLOCK_SIZE <= block_size_multiplier <= self.MAX_BLOCK_SIZE:  # :98-101
            raise ValueError(f"blockSizeMultiplier: {block_size_multiplier} (expected: 1-9)")
        self.block_size_multiplier = int(block_size_multiplier)
        self._h = _new(_lib.load().nx_bzip2_encoder_new(self.block_size_multiplier), "Bzip2Encoder")

    def _out(self, n: int):
        cap = _lib.load().nx_bzip2_encoder_max_encoded_length(self._h, n)
        return (C.c_uint8 * max(cap, 1))(), cap

    @staticmethod
    def _ret(r, out) -> bytes:
        if r < 0:
            raise CompressionException(_lib.status_string(r))
        return bytes(out[:r])

    def encode(self, data: bytes) -> bytes:
        out, cap = self._out(len(data))
        return self._ret(_lib.load().nx_bzip2_encoder_encode(self._h, data, len(data), out, cap), out)

    def finish_encode(self) -> bytes:
        out, cap = self._out(0)
        return self._ret(_lib.load().nx_bzip2_encoder_close(self._h, out, cap), out)

    def is_closed(self) -> bool:
        """Bzip2Encoder.isClosed() (:166-168)"""
        return bool(_lib.load().nx_bzip2_encoder_is_closed(self._h))

    def launches(self) -> int:
        """nx_bzip2_encoder_launches: the split-path calls made so far (one per write that closes blocks)"""
        return _lib.load().nx_bzip2_encoder_launches(self._h)


class Bzip2Decoder(_Decoder):
    """Bzip2Decoder.java:93-343 over the GPU bzip2 decoder's split path (nx_bzip2_decoder_*): the stream as the
    channel delivers it, one message per block.  A read uploads the cumulation, scans it for block and
    end-of-stream magics and decodes every block that has a later magic behind it in one launch sequence, a
    block per wave; a block still arriving waits in the cumulation (readable_bytes(), a whole compressed block
    at most: the reference decodes inside a partial block, this handle does not).  After the end-of-stream
    marker is_closed() is true and further input is swallowed (:328-330).  The first failing block raises
    DecompressionException with the reference's text (its code as .status, the messages of the blocks before
    it as .decoded); afterwards input is swallowed too, a state the reference does not have.  Randomised
    blocks are refused."""

    _free = "nx_bzip2_decoder_free"
    _decode_fn = "nx_bzip2_decoder_decode"

    def __init__(self):
        super().__init__()
        self._h = _new(_lib.load().nx_bzip2_decoder_new(), "Bzip2Decoder")

    def is_closed(self) -> bool:
        """the end-of-stream marker has been read and its stream CRC checked (State.EOF)"""
        return bool(_lib.load().nx_bzip2_decoder_is_closed(self._h))

    def stats(self) -> dict:
        """launch sequences made so far, chain blocks attempted and blocks emitted"""
        a, b, c = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _lib.load().nx_bzip2_decoder_stats(self._h, C.byref(a), C.byref(b), C.byref(c))
        return {"launches": a.value, "blocks_attempted": b.value, "blocks_emitted": c.value}


class ZstdDecoder(_Decoder):
    """ZstdDecoder.java:59-122 over the GPU Zstandard frame decoder (nx_zstd_decoder_*).  Every complete
    frame of a read is decoded in one launch, content checksums verified (XXH64) and skippable frames
    stepped over; the concatenation of the messages is libzstd's output for the complete frames received
    so far.  With maximum_allocation_size > 0 no message is longer than that (a longer frame is cut into
    several, :99-110), with 0 a frame is one message; an empty frame fires none.  Unlike the reference,
    a frame is emitted when it is whole: a partial frame waits in the cumulation (readable_bytes()).
    The first bad frame raises DecompressionException with libzstd's text (its code as .status, the
    messages of the frames before it as .decoded); afterwards input is swallowed (State.CORRUPTED)."""

    _free = "nx_zstd_decoder_free"
    _decode_fn = "nx_zstd_decoder_decode"

    def __init__(self, maximum_allocation_size: int = 4 * 1024 * 1024):
        super().__init__()
        if maximum_allocation_size < 0:  # ObjectUtil.checkPositiveOrZero (:64)
            raise ValueError(f"maximumAllocationSize : {maximum_allocation_size} (expected: >= 0)")
        self.maximum_allocation_size = int(maximum_allocation_size)
        self._h = _new(_lib.load().nx_zstd_decoder_new(self.maximum_allocation_size), "ZstdDecoder")

    def stats(self) -> dict:
        """batch launches made so far and the frames they held (one launch per read that completes a frame)"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        _lib.load().nx_zstd_decoder_stats(self._h, C.byref(a), C.byref(b))
        return {"launches": a.value, "frames": b.value}


class ZlibWrapper(enum.IntEnum):
    """ZlibWrapper.java:21-40 (the ordinals the C-ABI takes)"""
    ZLIB = 0
    GZIP = 1
    NONE = 2
    ZLIB_OR_NONE = 3


class JdkZlibEncoder(_Encoder):
    """JdkZlibEncoder.java:123-137,214-276,308-340 over the GPU deflate encoder.  encode() writes the
    header once and the message as sync-flushed deflate blocks (64 KiB slices of one batch), so the
    bytes written so far always inflate to the input so far; finish_encode() writes the final block
    and the wrapper's trailer, after which encode() passes its input through (:215-218).  Levels 1-9
    and -1 run one matcher (sizes near zlib level 1), level 0 writes stored blocks; the bytes differ
    from the JDK's and inflate to the same data.  ZLIB_OR_NONE and levels outside -1..9 are refused
    as the reference's constructor refuses them (:124-132).  dictionary: JdkZlibEncoder(level, dictionary)
    (:149-177), ZLIB only: the header carries FDICT and the dictionary's Adler32, and the stream's first
    slice may match into the dictionary's last 32 KiB."""

    _free = "nx_zlib_encoder_free"

    def __init__(self, wrapper: ZlibWrapper = ZlibWrapper.ZLIB, compression_level: int = 6, dictionary: bytes | None = None):
        wrapper = ZlibWrapper(wrapper)
        if not -1 <= compression_level <= 9:
            raise ValueError(f"compressionLevel: {compression_level} (expected: -1-9)")
        if wrapper == ZlibWrapper.ZLIB_OR_NONE:
            raise ValueError(f"wrapper '{wrapper.name}' is not allowed for compression.")
        self.wrapper = wrapper
        self.compression_level = int(compression_level)
        if dictionary is None:
            self._h = _new(_lib.load().nx_zlib_encoder_new(int(wrapper), self.compression_level), "JdkZlibEncoder")
            return
        if wrapper != ZlibWrapper.ZLIB:  # the dictionary constructors take no wrapper (:173)
            raise ValueError(f"a preset dictionary needs ZlibWrapper.ZLIB, not '{wrapper.name}'")
        dictionary = bytes(dictionary)
        self._h = _new(_lib.load().nx_zlib_encoder_new_dict(self.compression_level, dictionary, len(dictionary)), "JdkZlibEncoder")

    @staticmethod
    def _ret(r, out) -> bytes:
        if r < 0:
            raise CompressionException(_lib.status_string(r))
        return bytes(out[:r])

    def encode(self, data: bytes) -> bytes:
        L = _lib.load()
        cap = L.nx_zlib_max_encoded_length(len(data))
        out = (C.c_uint8 * cap)()
        return self._ret(L.nx_zlib_encoder_encode(self._h, data, len(data), out, cap), out)

    def finish_encode(self) -> bytes:
        out = (C.c_uint8 * 32)()
        return self._ret(_lib.load().nx_zlib_encoder_close(self._h, out, 32), out)


class JdkZlibDecoder(_Decoder):
    """JdkZlibDecoder.java:117-160,198-314 over the GPU inflater (nx_zlib_decoder_*): ZLIB, GZIP (every
    header field, optionally concatenated members), NONE and ZLIB_OR_NONE, maxAllocation as
    ZlibDecoder.java:49,62-84.  The concatenation of the messages is zlib's output for the bytes
    received so far (the boundaries are this decoder's own); with max_allocation > 0 a read delivers
    one message of at most that many bytes or fails with "Decompression buffer has reached maximum
    size".  A data error raises DecompressionException("decompression failure") with the inflater's
    code as .status.  dictionary: JdkZlibDecoder(dictionary, maxAllocation) (:96-111), ZLIB and not
    concatenated; a stream whose DICTID is not the dictionary's raises DecoderException."""

    _free = "nx_zlib_decoder_free"
    _decode_fn = "nx_zlib_decoder_decode"

    def __init__(self, wrapper: ZlibWrapper = ZlibWrapper.ZLIB, decompress_concatenated: bool = False, max_allocation: int = 0,
                 dictionary: bytes | None = None):
        super().__init__()
        if max_allocation < 0:  # ObjectUtil.checkPositiveOrZero (ZlibDecoder.java:49)
            raise ValueError(f"maxAllocation : {max_allocation} (expected: >= 0)")
        self.wrapper = ZlibWrapper(wrapper)
        if dictionary is not None:
            if self.wrapper != ZlibWrapper.ZLIB or decompress_concatenated:  # the dictionary constructors take neither (:97,110)
                raise ValueError("a preset dictionary needs ZlibWrapper.ZLIB and decompress_concatenated = False")
            dictionary = bytes(dictionary)
            self._h = _new(_lib.load().nx_zlib_decoder_new_dict(dictionary, len(dictionary), int(max_allocation)), "JdkZlibDecoder")
            return
        self._h = _new(_lib.load().nx_zlib_decoder_new(int(self.wrapper), int(bool(decompress_concatenated)), int(max_allocation)),
                       "JdkZlibDecoder")

    def is_closed(self) -> bool:
        """ZlibDecoder.isClosed(): the end of the compressed stream has been reached"""
        return bool(_lib.load().nx_zlib_decoder_is_closed(self._h))


class Lz4FrameDecoder(_Decoder):
    """Lz4FrameDecoder.java:36-277 (validateChecksums default false, :100-102)."""

    _free = "nx_lz4_frame_decoder_free"
    _decode_fn = "nx_lz4_frame_decoder_decode"

    def __init__(self, validate_checksums: bool = False):
        super().__init__()
        self._h = _new(_lib.load().nx_lz4_frame_decoder_new(int(validate_checksums)), "Lz4FrameDecoder")


# ------------------------------------------------------------------------------------- harness
class EmbeddedChannel:
    """The subset of io.netty.channel.embedded.EmbeddedChannel the codec tests use
    (EmbeddedChannel.java:337-483): one handler, outbound/inbound message queues."""

    def __init__(self, handler):
        self.handler = handler
        self._outbound: list[bytes] = []
        self._inbound: list[bytes] = []

    def write_outbound(self, *msgs) -> bool:
        for m in msgs:
            # MessageToByteEncoder.write: empty output is replaced by EMPTY_BUFFER (:112-117)
            self._outbound.append(self.handler.write(m))
        return bool(self._outbound)

    def write_inbound(self, *msgs) -> bool:
        for m in msgs:
            self._inbound.extend(self.handler.channel_read(m))
        return bool(self._inbound)

    def read_outbound(self):
        return self._outbound.pop(0) if self._outbound else None

    def read_inbound(self):
        return self._inbound.pop(0) if self._inbound else None

    def finish(self) -> bool:
        return bool(self._outbound or self._inbound)


class Batcher:
    """Asynchronous cross-channel batching executor (include/netty_amd.h section 3, csrc/batcher.cpp):
    encode()/decode() calls of many SnappyFrameEncoder / SnappyFrameDecoder instances become jobs of
    one GPU launch per flush().  submit_* never touches the GPU; poll() never blocks."""

    def __init__(self, flush_bytes: int = 0):
        self._h = _new(_lib.load().nx_batcher_new(), "Batcher")
        if flush_bytes:
            self.set_flush_bytes(flush_bytes)

    def set_flush_bytes(self, n: int):
        """Auto-flush once the collecting batch holds n input bytes (0 = only flush())."""
        _lib.load().nx_batcher_set_flush_bytes(self._h, n)

    def close(self):
        if self._h:
            _lib.load().nx_batcher_free(self._h)
            self._h = None

    __del__ = close

    def reserve(self, kinds: int = 0x1F):
        """Hold the device workspaces of the given kinds now (bit NX_WS_* per kind; default all), so no
        submit pays for them (nx_batcher_reserve)."""
        r = _lib.load().nx_batcher_reserve(self._h, kinds)
        if r != 0:
            raise RuntimeError(f"nx_batcher_reserve: {_lib.status_string(r)}")

    def reserve_arenas(self, nbatches: int, staging_bytes: int, out_bytes: int):
        """Size the pinned arenas now (nx_batcher_reserve_arenas): submits then never allocate."""
        r = _lib.load().nx_batcher_reserve_arenas(self._h, nbatches, staging_bytes, out_bytes)
        if r != 0:
            raise RuntimeError(f"nx_batcher_reserve_arenas: {_lib.status_string(r)}")

    def arena_stats(self) -> dict:
        a, n = C.c_uint64(0), C.c_uint64(0)
        k = C.c_uint32(0)
        _lib.load().nx_batcher_arena_stats(self._h, C.byref(a), C.byref(n), C.byref(k))
        return {"allocs": a.value, "bytes": n.value, "batches": k.value}

    def _ticket(self, t, what):
        if t < 0:
            raise RuntimeError(f"{what}: {_lib.status_string(t)}")
        return t

    def submit_encode(self, encoder, data, registered_ptr: int | None = None, reader_index: int = 0, op: int = 0) -> int:
        """encode() of any encoder handler as a job: SnappyFrameEncoder (with registered_ptr, an address
        inside memory passed to register(), the bytes are DMA'd from there at flush and must stay valid
        until completion), FastLzFrameEncoder (``reader_index`` as in encode()), LzfEncoder,
        Lz4FrameEncoder (``op`` 0 encode, 1 encode + flush, 2 encode + close), JdkZlibEncoder (``op`` 0
        encode, 2 encode + finish_encode).  Any other handle is a TypeError."""
        L = _lib.load()
        if isinstance(encoder, FastLzFrameEncoder):
            buf = bytes(reader_index) + bytes(data)
            return self._ticket(L.nx_fastlz_frame_encoder_submit(encoder._h, self._h, buf, reader_index, len(data)),
                                "nx_fastlz_frame_encoder_submit")
        if isinstance(encoder, LzfEncoder):
            buf = bytes(data)
            return self._ticket(L.nx_lzf_encoder_submit(encoder._h, self._h, buf, len(buf)), "nx_lzf_encoder_submit")
        if isinstance(encoder, Lz4FrameEncoder):
            buf = bytes(data)
            t = L.nx_lz4_frame_encoder_submit(encoder._h, self._h, buf, len(buf), op)
            encoder.raise_for(t)
            return self._ticket(t, "nx_lz4_frame_encoder_submit")
        if isinstance(encoder, JdkZlibEncoder):
            buf = bytes(data)
            return self._ticket(L.nx_zlib_encoder_submit(encoder._h, self._h, buf, len(buf), op), "nx_zlib_encoder_submit")
        if not isinstance(encoder, SnappyFrameEncoder):
            raise TypeError(f"Batcher.submit_encode: {type(encoder).__name__} is not an encoder handler of this package")
        if registered_ptr is not None:
            t = L.nx_snappy_frame_encoder_submit(encoder._h, self._h, C.c_void_p(registered_ptr), len(data), 1)
        else:
            buf = bytes(data)
            t = L.nx_snappy_frame_encoder_submit(encoder._h, self._h, buf, len(buf), 0)
        if t < 0:
            raise RuntimeError(f"nx_snappy_frame_encoder_submit: {_lib.status_string(t)}")
        return t

    _DECODE_SUBMIT = {"SnappyFrameDecoder": "nx_snappy_frame_decoder_submit",
                      "FastLzFrameDecoder": "nx_fastlz_frame_decoder_submit",
                      "LzfDecoder": "nx_lzf_decoder_submit",
                      "Lz4FrameDecoder": "nx_lz4_frame_decoder_submit",
                      "JdkZlibDecoder": "nx_zlib_decoder_submit"}

    def submit_decode(self, decoder, data) -> int:
        """decode() of any decoder handler over its cumulation + data as a job; the consumed bytes leave
        the cumulation now (ByteToMessageDecoder.channelRead)."""
        L = _lib.load()
        fn = next((v for k, v in self._DECODE_SUBMIT.items() if any(c.__name__ == k for c in type(decoder).__mro__)), None)
        if fn is None:
            raise TypeError(f"Batcher.submit_decode: {type(decoder).__name__} is not a decoder handler of this package")
        decoder._cum += bytes(data)
        buf = bytes(decoder._cum)
        consumed = C.c_size_t(0)
        t = self._ticket(getattr(L, fn)(decoder._h, self._h, buf, len(buf), C.byref(consumed)), fn)
        del decoder._cum[:consumed.value]
        return t

    def submit_decode_registered(self, decoder: "SnappyFrameDecoder", ptr: int, n: int) -> tuple[int, int]:
        """SnappyFrameDecoder.decode over a cumulation the caller holds in registered memory
        (register()): nothing is copied; bytes [ptr, ptr + consumed) must stay valid until the job
        completes.  Returns (ticket, consumed); the caller discards the consumed bytes afterwards."""
        consumed = C.c_size_t(0)
        t = _lib.load().nx_snappy_frame_decoder_submit_registered(decoder._h, self._h, C.c_void_p(ptr), n, C.byref(consumed))
        if t < 0:
            raise RuntimeError(f"nx_snappy_frame_decoder_submit_registered: {_lib.status_string(t)}")
        return t, consumed.value

    def flush(self):
        r = _lib.load().nx_batcher_flush(self._h)
        if r != 0:
            raise RuntimeError(f"nx_batcher_flush: {_lib.status_string(r)}")

    def poll(self, ticket: int) -> bool:
        r = _lib.load().nx_batcher_poll(self._h, ticket)
        if r < 0:
            raise RuntimeError(f"nx_batcher_poll: {_lib.status_string(r)}")
        return r == 1

    def wait(self, ticket: int):
        r = _lib.load().nx_batcher_wait(self._h, ticket)
        if r != 0:
            raise RuntimeError(f"nx_batcher_wait: {_lib.status_string(r)}")

    def result(self, ticket: int, release: bool = True):
        """The job's messages (list of bytes); a failed decoder job raises like decode() would, with
        the messages decoded before the failure attached as .decoded."""
        L = _lib.load()
        msgs = C.POINTER(_lib.NxMsg)()
        n = C.c_size_t(0)
        err = C.c_char_p()
        rc = L.nx_batcher_result(self._h, ticket, C.byref(msgs), C.byref(n), C.byref(err))
        out = [C.string_at(msgs[i].data, msgs[i].len) if msgs[i].len else b"" for i in range(n.value)]
        if release:
            L.nx_batcher_release(self._h, ticket)
        if rc != 0:
            if rc in (-100, -101, -102, -103):
                raise RuntimeError(f"Batcher: native failure {rc} ({_lib.status_string(rc)})")
            msg = err.value.decode() if err.value else _lib.status_string(rc)
            e = DecoderException(msg) if msg.startswith("java.lang.") else DecompressionException(msg)
            e.decoded = out
            e.status = rc
            raise e
        return out

    def stats(self) -> dict:
        f, l_, c = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _lib.load().nx_batcher_stats(self._h, C.byref(f), C.byref(l_), C.byref(c))
        df, db = C.c_uint64(0), C.c_uint64(0)
        _lib.load().nx_batcher_dma_stats(self._h, C.byref(df), C.byref(db))
        return {"flushes": f.value, "launches": l_.value, "chunks": c.value, "dma_flushes": df.value, "dma_bytes": db.value}

    @staticmethod
    def register(ptr: int, n: int):
        r = _lib.load().nx_host_register(C.c_void_p(ptr), n)
        if r != 0:
            raise RuntimeError(f"nx_host_register: {_lib.status_string(r)}")

    @staticmethod
    def unregister(ptr: int):
        _lib.load().nx_host_unregister(C.c_void_p(ptr))
