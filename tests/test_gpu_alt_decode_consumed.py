"""The synchronous FastLZ / LZF / LZ4 frame decoders through the C-ABI on calls that fail or skip:
the messages before the failure, the status, the error text (against oracle/frame_decoders.py) and
`consumed`, the reader index the call leaves behind.  Every expected offset is worked out from the
block layouts:

  FastLZ  'F' 'L' 'Z' options [checksum 4] chunkLength 2 [originalLength 2]   6 / 8 bytes, 10 / 12 with a checksum
  LZF     'Z' 'V' type chunkLength 2 [originalLength 2]                        5 / 7 bytes
  LZ4     magic 8, token 1, compressedLength 4, decompressedLength 4, checksum 4   21 bytes

A block that fails to decode, and a FastLZ block whose checksum mismatches, leave the reader at the
block's payload (the Java decoders read the headers into their state and throw before skipping the
payload); an LZ4 checksum mismatch is found after the payload was skipped; a bad magic leaves the reader
behind the magic bytes read.
"""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

NX_ERR_FASTLZ_LENGTH_MISMATCH, NX_ERR_FASTLZ_CRC_MISMATCH = -22, -23
NX_ERR_LZF_CORRUPT, NX_ERR_FRAME_CORRUPT = -30, -40
NX_ERR_LZ4_BAD_MAGIC, NX_ERR_LZ4_CHECKSUM_MISMATCH = -51, -56
NX_ERR_INVALID_ARG = -100


@pytest.fixture(scope="module")
def L():
    from netty_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def F():
    from oracle import frame_decoders
    return frame_decoders


@pytest.fixture(scope="module")
def text(oracle):
    """Two messages every codec compresses and one below FastLZ's MIN_LENGTH_TO_COMPRESSION (32)."""
    return oracle.textgen_chunk(1, 300), oracle.textgen_chunk(2, 400), oracle.textgen_chunk(3, 20)


class Dec:
    """One native decoder handle."""

    def __init__(self, L, codec, validate=False):
        self.L, self.codec = L, codec
        self.fn = getattr(L, {"fastlz": "nx_fastlz_frame_decoder_decode", "lzf": "nx_lzf_decoder_decode",
                              "lz4": "nx_lz4_frame_decoder_decode"}[codec])
        if codec == "lzf":
            self.h = L.nx_lzf_decoder_new()
        else:
            self.h = getattr(L, f"nx_{codec}_frame_decoder_new")(int(validate))
        assert self.h

    def decode(self, data):
        """(status, consumed, messages, error text)"""
        from netty_amd import _lib
        consumed, n = C.c_size_t(12345), C.c_size_t(12345)
        msgs, err = C.POINTER(_lib.NxMsg)(), C.c_char_p()
        rc = self.fn(self.h, data, len(data), C.byref(consumed), C.byref(msgs), C.byref(n), C.byref(err))
        out = [C.string_at(msgs[i].data, msgs[i].len) for i in range(n.value)]
        return rc, consumed.value, out, err.value.decode() if err.value else None

    def close(self):
        free = "nx_lzf_decoder_free" if self.codec == "lzf" else f"nx_{self.codec}_frame_decoder_free"
        getattr(self.L, free)(self.h)


@pytest.fixture
def dec(L):
    made = []

    def make(codec, validate=False):
        made.append(Dec(L, codec, validate))
        return made[-1]

    yield make
    for d in made:
        d.close()


def _oracle(F, codec, validate, stream):
    d = {"fastlz": lambda: F.FastLzFrameDecoder(validate), "lzf": F.LzfDecoder,
         "lz4": lambda: F.Lz4FrameDecoder(validate)}[codec]()
    msgs, err = F.run(d, [stream])
    return msgs, err[1] if err else None


def _patch(stream, at, fn):
    b = bytearray(stream)
    b[at] = fn(b[at]) & 0xFF
    return bytes(b)


def _fails(F, dec, codec, validate, stream, status, consumed, first):
    """One failing call: the first message, status, oracle's text, consumed; then the corrupted
    decoder skips whatever comes next."""
    want_msgs, want_err = _oracle(F, codec, validate, stream)
    assert want_msgs == [first] and want_err
    d = dec(codec, validate)
    rc, used, msgs, err = d.decode(stream)
    assert msgs == [first]
    assert rc == status
    assert err == want_err
    assert used == consumed
    rest = stream[used:] + b"\x00" * 7
    assert d.decode(rest) == (0, len(rest), [], None)  # CORRUPTED: everything is skipped
    return err


# ------------------------------------------------------------------------------------- FastLZ
def _flz(oracle, data, checksum):
    blk = oracle.fastlz_frame_encode(data, 0, checksum)
    comp = len(data) >= 32
    assert blk[:3] == b"FLZ" and blk[3] == (0x01 if comp else 0) | (0x10 if checksum else 0)
    hdr = 4 + (4 if checksum else 0) + 2 + (2 if comp else 0)
    assert len(blk) == hdr + int.from_bytes(blk[hdr - (4 if comp else 2):hdr - (2 if comp else 0)], "big")  # one block
    return blk, hdr


def test_fastlz_block_failure(oracle, F, dec, text):
    a, _ = _flz(oracle, text[0], False)
    b, hdr = _flz(oracle, text[1], False)
    assert hdr == 8
    s = _patch(a + b, len(a) + 7, lambda v: v + 1)  # originalLength + 1 (400 -> 401: no carry)
    err = _fails(F, dec, "fastlz", False, s, NX_ERR_FASTLZ_LENGTH_MISMATCH, len(a) + 8, text[0])
    assert err == "stream corrupted: originalLength(401) and actual length(400) mismatch"


@pytest.mark.parametrize("second", [1, 2], ids=["compressed", "raw"])
def test_fastlz_checksum_mismatch(oracle, F, dec, text, second):
    a, _ = _flz(oracle, text[0], True)
    b, hdr = _flz(oracle, text[second], True)
    assert hdr == (12 if second == 1 else 10)
    s = _patch(a + b, len(a) + 7, lambda v: v ^ 0x01)  # the checksum's low byte
    err = _fails(F, dec, "fastlz", True, s, NX_ERR_FASTLZ_CRC_MISMATCH, len(a) + hdr, text[0])
    assert err.startswith("stream corrupted: mismatching checksum: ")


def test_fastlz_walk_error(oracle, F, dec, text):
    a, _ = _flz(oracle, text[0], False)
    b, _ = _flz(oracle, text[1], False)
    s = _patch(a + b, len(a) + 1, lambda v: v ^ 0x20)  # 'L' -> 'l'
    # readUnsignedMedium() has read the three magic bytes when decode() throws
    err = _fails(F, dec, "fastlz", False, s, NX_ERR_FRAME_CORRUPT, len(a) + 3, text[0])
    assert err == "unexpected block identifier"


# ------------------------------------------------------------------------------------- LZF
def _lzf(oracle, data):
    blk = oracle.lzf_frame_encode(data)
    assert blk[:3] == b"ZV\x01" and len(blk) == 7 + int.from_bytes(blk[3:5], "big")  # one compressed block
    return blk


def test_lzf_block_failure(oracle, F, dec, text):
    a, b = _lzf(oracle, text[0]), _lzf(oracle, text[1])
    s = _patch(a + b, len(a) + 6, lambda v: v + 1)  # originalLength + 1 (400 -> 401: no carry)
    err = _fails(F, dec, "lzf", False, s, NX_ERR_LZF_CORRUPT, len(a) + 7, text[0])
    assert err == F.LZF_CORRUPT_MSG


def test_lzf_walk_error(oracle, F, dec, text):
    a, b = _lzf(oracle, text[0]), _lzf(oracle, text[1])
    s = _patch(a + b, len(a) + 1, lambda v: v ^ 0x20)  # 'V' -> 'v'
    # readUnsignedShort() has read the two magic bytes when decode() throws
    err = _fails(F, dec, "lzf", False, s, NX_ERR_FRAME_CORRUPT, len(a) + 2, text[0])
    assert err == "unexpected block identifier"


# ------------------------------------------------------------------------------------- LZ4
def _lz4(oracle, data):
    blk = oracle.lz4_frame_encode(data, close=False)
    assert blk[:8] == oracle.LZ4_MAGIC and blk[8] & 0xF0 == 0x20  # one compressed block
    assert len(blk) == 21 + int.from_bytes(blk[9:13], "little")
    return blk


def test_lz4_checksum_mismatch(oracle, F, dec, text):
    a, b = _lz4(oracle, text[0]), _lz4(oracle, text[1])
    s = _patch(a + b, len(a) + 17, lambda v: v ^ 0x01)  # the checksum's low byte
    # the payload is skipped before the checksum is compared (Lz4FrameDecoder.java:222-228)
    err = _fails(F, dec, "lz4", True, s, NX_ERR_LZ4_CHECKSUM_MISMATCH, len(a) + len(b), text[0])
    assert err.startswith("stream corrupted: mismatching checksum: ")


def test_lz4_checksum_not_validated(oracle, F, dec, text):
    a, b = _lz4(oracle, text[0]), _lz4(oracle, text[1])
    s = _patch(a + b, len(a) + 17, lambda v: v ^ 0x01)
    assert _oracle(F, "lz4", False, s) == ([text[0], text[1]], None)
    assert dec("lz4", False).decode(s) == (0, len(s), [text[0], text[1]], None)


def test_lz4_finished_stream_skips(oracle, F, dec, text):
    s = oracle.lz4_frame_encode(text[0], close=True)
    assert len(s) == len(_lz4(oracle, text[0])) + 21  # the block and the end block
    d = dec("lz4", True)
    assert d.decode(s) == (0, len(s), [text[0]], None)
    junk = oracle.java_random_bytes(11, 30)
    assert d.decode(junk) == (0, 30, [], None)  # FINISHED (Lz4FrameDecoder.java:250-254)


def test_lz4_walk_error_then_skips(oracle, F, dec, text):
    a, b = _lz4(oracle, text[0]), _lz4(oracle, text[1])
    s = _patch(a + b, len(a) + 2, lambda v: v ^ 0x01)  # '4' -> '5'
    # the eight magic bytes are read (readLong) when decode() throws
    err = _fails(F, dec, "lz4", False, s, NX_ERR_LZ4_BAD_MAGIC, len(a) + 8, text[0])
    assert err == "unexpected block identifier"


# ------------------------------------------------------------------------------------- arguments
@pytest.mark.parametrize("codec", ["fastlz", "lzf", "lz4"])
def test_null_out_pointer_is_invalid_arg(oracle, dec, text, codec):
    from netty_amd import _lib
    enc = {"fastlz": lambda m: _flz(oracle, m, False)[0], "lzf": lambda m: _lzf(oracle, m),
           "lz4": lambda m: _lz4(oracle, m)}[codec]
    s = enc(text[0]) + enc(text[1])
    d = dec(codec)
    consumed, n = C.c_size_t(0), C.c_size_t(0)
    msgs, err = C.POINTER(_lib.NxMsg)(), C.c_char_p()
    full = [C.byref(consumed), C.byref(msgs), C.byref(n)]
    for k in range(3):
        args = full[:k] + [None] + full[k + 1:]
        assert d.fn(d.h, s, len(s), *args, C.byref(err)) == NX_ERR_INVALID_ARG
    assert d.decode(s) == (0, len(s), [text[0], text[1]], None)  # the refused calls changed nothing


ENTRY_POINTS = {  # every synchronous decoder's decode(): its handle and one good stream of `data`
    "snappy": (lambda H: H.SnappyFrameDecoder(True), lambda o, d: o.snappy_frame_encode(d)[0]),
    "fastlz": (lambda H: H.FastLzFrameDecoder(True), lambda o, d: o.fastlz_frame_encode(d, 0, True)),
    "lzf": (lambda H: H.LzfDecoder(), lambda o, d: o.lzf_frame_encode(d)),
    "lz4": (lambda H: H.Lz4FrameDecoder(True), lambda o, d: o.lz4_frame_encode(d)),
    "zstd": (lambda H: H.ZstdDecoder(0), lambda o, d: __import__("pyarrow").Codec("zstd").compress(d).to_pybytes()),
    "zlib": (lambda H: H.JdkZlibDecoder(), lambda o, d: __import__("zlib").compress(d)),
    "bzip2": (lambda H: H.Bzip2Decoder(), lambda o, d: __import__("bz2").compress(d, 1)),
}


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_null_arguments_of_every_decoder(L, oracle, text, name):
    """Null consumed, msgs or n_msgs: NX_ERR_INVALID_ARG and nothing changes; null err_msg is accepted, and the
    handle that refused three calls then decodes a good stream as a fresh handle does."""
    from netty_amd import _lib, handlers as H
    make, enc = ENTRY_POINTS[name]
    s = enc(oracle, text[0] + text[1])

    def decode(d, err_arg):
        consumed, n, msgs = C.c_size_t(12345), C.c_size_t(12345), C.POINTER(_lib.NxMsg)()
        rc = getattr(L, d._decode_fn)(d._h, s, len(s), C.byref(consumed), C.byref(msgs), C.byref(n), err_arg)
        return rc, consumed.value, [C.string_at(msgs[i].data, msgs[i].len) for i in range(n.value)]

    d, fresh = make(H), make(H)
    try:
        consumed, n, msgs, err = C.c_size_t(0), C.c_size_t(0), C.POINTER(_lib.NxMsg)(), C.c_char_p()
        full = [C.byref(consumed), C.byref(msgs), C.byref(n)]
        for k in range(3):
            args = full[:k] + [None] + full[k + 1:]
            assert getattr(L, d._decode_fn)(d._h, s, len(s), *args, C.byref(err)) == NX_ERR_INVALID_ARG
        want = decode(fresh, C.byref(err))
        assert want[:2] == (0, len(s)) and b"".join(want[2]) == text[0] + text[1] and err.value is None
        assert decode(d, None) == want
    finally:
        d.close()
        fresh.close()
