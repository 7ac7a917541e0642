"""JdkZlibDecoder on the MI355X: the cases of ZlibTest / JdkZlibTest (codec-compression/src/test/java/
io/netty/handler/codec/compression/), read like the Java, with Python's zlib and gzip as the other side."""
import gzip
import os
import random
import struct
import zlib

import pytest

import inflate_streams as IS

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BYTES_SMALL = IS.big_text(256, seed=3)
BYTES_LARGE = IS.big_text(1024 * 1024, seed=4)


@pytest.fixture(scope="module")
def H():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from netty_amd import handlers
    return handlers


def _zlib_side(H, wrapper, data, level=6):
    wbits = {H.ZlibWrapper.ZLIB: 15, H.ZlibWrapper.GZIP: 31, H.ZlibWrapper.NONE: -15}[wrapper]
    c = zlib.compressobj(level, zlib.DEFLATED, wbits)
    return c.compress(data) + c.flush()


def _read_all(ch):
    out = bytearray()
    while (m := ch.read_inbound()) is not None:
        out += m
    return bytes(out)


@pytest.mark.parametrize("wrapper", ["ZLIB", "GZIP", "NONE"])
@pytest.mark.parametrize("data", [b"", BYTES_SMALL, BYTES_LARGE], ids=["empty", "small", "large"])
def test_round_trips(H, wrapper, data):
    """ZlibTest.testZLIB / testGZIP / testNONE: this project's encoder and zlib's, into the decoder"""
    w = H.ZlibWrapper[wrapper]
    enc = H.JdkZlibEncoder(w)
    ours = enc.encode(data[:len(data) // 2]) + enc.encode(data[len(data) // 2:]) + enc.finish_encode()
    for z in (ours, _zlib_side(H, w, data)):
        ch = H.EmbeddedChannel(H.JdkZlibDecoder(w))
        ch.write_inbound(z)
        assert _read_all(ch) == data
        assert ch.handler.is_closed() and ch.handler.readable_bytes() == 0


def test_zlib_or_none(H):
    """ZlibTest.testZLIB_OR_NONE / 2 / JdkZlibTest.testZLIB_OR_NONE3"""
    for w in (H.ZlibWrapper.ZLIB, H.ZlibWrapper.NONE):
        ch = H.EmbeddedChannel(H.JdkZlibDecoder(H.ZlibWrapper.ZLIB_OR_NONE))
        z = _zlib_side(H, w, BYTES_SMALL)
        ch.write_inbound(z[:1])  # the decision needs two bytes
        assert ch.read_inbound() is None
        ch.write_inbound(z[1:])
        assert _read_all(ch) == BYTES_SMALL and ch.handler.is_closed()
    ch = H.EmbeddedChannel(H.JdkZlibDecoder(H.ZlibWrapper.ZLIB_OR_NONE))
    with pytest.raises(H.DecompressionException, match="^decompression failure$"):
        ch.write_inbound(_zlib_side(H, H.ZlibWrapper.GZIP, BYTES_SMALL))


def test_multiple_gz(H):
    """JdkZlibTest.testConcatenatedStreamsReadFirstOnly / ReadFully / ReadFullyWhenFragmented"""
    raw = open(os.path.join(ROOT, "tests", "golden", "multiple.gz"), "rb").read()
    ch = H.EmbeddedChannel(H.JdkZlibDecoder(H.ZlibWrapper.GZIP))
    ch.write_inbound(raw)
    assert _read_all(ch) == b"a" and ch.handler.is_closed()
    ch = H.EmbeddedChannel(H.JdkZlibDecoder(H.ZlibWrapper.GZIP, True))
    ch.write_inbound(raw)
    assert _read_all(ch) == b"ab" and not ch.handler.is_closed()
    ch = H.EmbeddedChannel(H.JdkZlibDecoder(H.ZlibWrapper.GZIP, True))
    for b in raw:
        ch.write_inbound(bytes([b]))
    assert _read_all(ch) == b"ab"


def test_header_follows_footer_split_before_the_end(H):
    """JdkZlibTest.testDecodeWithHeaderFollowingFooter: two members, the last byte in a second read"""
    a, b = IS.big_text(1024, seed=11), IS.big_text(1024, seed=12)
    z = gzip.compress(a) + gzip.compress(b)
    ch = H.EmbeddedChannel(H.JdkZlibDecoder(H.ZlibWrapper.GZIP, True))
    ch.write_inbound(z[:-1])
    ch.write_inbound(z[-1:])
    assert _read_all(ch) == a + b


def test_footer_mismatches(H):
    """JdkZlibTest.testGZIP3-style footers: the CRC and the ISIZE checks, with Java's formatting"""
    z = bytearray(gzip.compress(BYTES_SMALL))
    crc, isize = struct.unpack("<II", z[-8:])
    bad = bytes(z[:-8]) + struct.pack("<II", crc ^ 0x80000001, isize)
    ch = H.EmbeddedChannel(H.JdkZlibDecoder(H.ZlibWrapper.GZIP))
    with pytest.raises(H.DecompressionException) as e:
        ch.write_inbound(bad)
    assert str(e.value) == f"CRC value mismatch. Expected: {crc ^ 0x80000001}, Got: {crc}" and e.value.decoded == [BYTES_SMALL]
    bad = bytes(z[:-8]) + struct.pack("<II", crc, 0xFFFFFFFE)
    ch = H.EmbeddedChannel(H.JdkZlibDecoder(H.ZlibWrapper.GZIP))
    with pytest.raises(H.DecompressionException) as e:
        ch.write_inbound(bad[:-3])
        ch.write_inbound(bad[-3:])  # the footer is read only once all 8 bytes are there
    assert str(e.value) == f"Number of bytes mismatch. Expected: -2, Got: {len(BYTES_SMALL)}"


def _gzip_with(flags, extra=b"", name=b"", comment=b"", body=BYTES_SMALL, bad_hcrc=False):
    h = bytes([31, 139, 8, flags, 1, 2, 3, 4, 0, 3])
    if flags & 4:
        h += struct.pack("<H", len(extra)) + extra
    if flags & 8:
        h += name + b"\0"
    if flags & 16:
        h += comment + b"\0"
    if flags & 2:
        h += struct.pack("<H", (zlib.crc32(h) & 0xFFFF) ^ (1 if bad_hcrc else 0))
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    return h + c.compress(body) + c.flush() + struct.pack("<II", zlib.crc32(body), len(body))


@pytest.mark.parametrize("flags", [2, 4, 8, 16, 2 | 4 | 8 | 16], ids=["FHCRC", "FEXTRA", "FNAME", "FCOMMENT", "all"])
def test_gzip_header_fields(H, flags):
    """every optional header field, whole and byte by byte.  The reference ORs the FEXTRA length into
    an xlen of -1 (JdkZlibDecoder.java:393), so it never skips the field: an empty one decodes."""
    z = _gzip_with(flags, name=b"file.txt", comment=b"a comment")
    assert gzip.decompress(z) == BYTES_SMALL
    ch = H.EmbeddedChannel(H.JdkZlibDecoder(H.ZlibWrapper.GZIP))
    ch.write_inbound(z)
    assert _read_all(ch) == BYTES_SMALL and ch.handler.is_closed()
    ch = H.EmbeddedChannel(H.JdkZlibDecoder(H.ZlibWrapper.GZIP))
    for b in z:
        ch.write_inbound(bytes([b]))
    assert _read_all(ch) == BYTES_SMALL and ch.handler.is_closed()


def test_gzip_header_errors(H):
    for z, msg in ((b"\x1e" + gzip.compress(b"x")[1:], "Input is not in the GZIP format"),
                   (bytes([31, 139, 7]) + gzip.compress(b"x")[3:], "Unsupported compression method 7 in the GZIP header"),
                   (bytes([31, 139, 8, 0x20]) + gzip.compress(b"x")[4:], "Reserved flags are set in the GZIP header")):
        ch = H.EmbeddedChannel(H.JdkZlibDecoder(H.ZlibWrapper.GZIP))
        with pytest.raises(H.DecompressionException) as e:
            ch.write_inbound(z)
        assert str(e.value) == msg
    z = _gzip_with(2, bad_hcrc=True)
    want = zlib.crc32(z[:10]) & 0xFFFF
    ch = H.EmbeddedChannel(H.JdkZlibDecoder(H.ZlibWrapper.GZIP))
    with pytest.raises(H.DecompressionException) as e:
        ch.write_inbound(z)
    assert str(e.value) == f"CRC16 value mismatch. Expected: {want ^ 1}, Got: {want}"
    # a non-empty FEXTRA field stays in front of the deflate data (the xlen quirk): 0x07 = a final block of type 3
    ch = H.EmbeddedChannel(H.JdkZlibDecoder(H.ZlibWrapper.GZIP))
    with pytest.raises(H.DecompressionException) as e:
        ch.write_inbound(_gzip_with(4, extra=b"\x07\x00\x00\x00"))
    assert str(e.value) == "decompression failure" and H._lib.status_string(e.value.status) == "invalid block type"


def test_zlib_wrapper_errors(H):
    good = zlib.compress(BYTES_SMALL)
    def head(cmf):  # the FLG byte (no FDICT) that makes the pair a multiple of 31
        return bytes([cmf, (31 - cmf * 256 % 31) % 31])

    cases = [(bytes([0x78, 0x9D]) + good[2:], "incorrect header check"),
             (head(0x77) + good[2:], "unknown compression method"),
             (head(0x88) + good[2:], "invalid window size"),
             (good[:-1] + bytes([good[-1] ^ 1]), "incorrect data check")]
    for z, text in cases:
        assert (z[0] * 256 + z[1]) % 31 == (1 if text == "incorrect header check" else 0)
        with pytest.raises(zlib.error, match=text):
            zlib.decompress(z)
        ch = H.EmbeddedChannel(H.JdkZlibDecoder(H.ZlibWrapper.ZLIB))
        with pytest.raises(H.DecompressionException) as e:
            ch.write_inbound(z)
        assert str(e.value) == "decompression failure" and H._lib.status_string(e.value.status) == text
        assert not ch.handler.is_closed()
    c = zlib.compressobj(6, zlib.DEFLATED, 15, zdict=b"dictionary")
    ch = H.EmbeddedChannel(H.JdkZlibDecoder(H.ZlibWrapper.ZLIB))
    with pytest.raises(H.DecompressionException, match="unable to set dictionary as non was specified"):
        ch.write_inbound(c.compress(BYTES_SMALL) + c.flush())
    # the stream is finished only once the trailer has verified
    ch = H.EmbeddedChannel(H.JdkZlibDecoder(H.ZlibWrapper.ZLIB))
    ch.write_inbound(good[:-2])
    assert _read_all(ch) == BYTES_SMALL and not ch.handler.is_closed()
    ch.write_inbound(good[-2:])
    assert ch.handler.is_closed()


def test_max_allocation(H):
    """ZlibTest.testMaxAllocation: a 1024-byte limit against a larger stream"""
    with pytest.raises(ValueError):
        H.JdkZlibDecoder(H.ZlibWrapper.ZLIB, False, -1)
    z = zlib.compress(bytes(64 * 1024))
    ch = H.EmbeddedChannel(H.JdkZlibDecoder(H.ZlibWrapper.ZLIB, False, 1024))
    with pytest.raises(H.DecompressionException) as e:
        ch.write_inbound(z)
    assert str(e.value).startswith("Decompression buffer has reached maximum size: 1024")
    assert ch.handler.is_closed() and e.value.decoded == [] and ch.read_inbound() is None
    # within the limit: one message per read, a stream of exactly the limit succeeds
    z = zlib.compress(BYTES_LARGE[:1024])
    ch = H.EmbeddedChannel(H.JdkZlibDecoder(H.ZlibWrapper.ZLIB, False, 1024))
    ch.write_inbound(z)
    assert ch.read_inbound() == BYTES_LARGE[:1024] and ch.read_inbound() is None and ch.handler.is_closed()


def test_bytes_after_the_end_are_skipped(H):
    for w in (H.ZlibWrapper.ZLIB, H.ZlibWrapper.GZIP, H.ZlibWrapper.NONE):
        ch = H.EmbeddedChannel(H.JdkZlibDecoder(w))
        ch.write_inbound(_zlib_side(H, w, BYTES_SMALL) + b"trailing junk")
        ch.write_inbound(b"more of it")
        assert _read_all(ch) == BYTES_SMALL and ch.handler.is_closed() and ch.handler.readable_bytes() == 0


def test_input_after_a_failure_is_skipped(H):
    """A parity difference: Java's decoder keeps its state after a DecompressionException
    and throws again on the next read; this handle raises once, then drops what follows and stays open."""
    good = _zlib_side(H, H.ZlibWrapper.NONE, BYTES_SMALL)
    bad_zlib = zlib.compress(BYTES_SMALL)
    bad_zlib = bad_zlib[:-1] + bytes([bad_zlib[-1] ^ 1])                    # a wrapper error (Adler32)
    bad_gzip = bytearray(gzip.compress(BYTES_SMALL))
    bad_gzip[-8] ^= 1                                                       # a wrapper error (CRC32)
    bad_raw = IS.crafted_invalid()["block_type"][0]                         # a data error from the device
    for w, bad in ((H.ZlibWrapper.ZLIB, bad_zlib), (H.ZlibWrapper.GZIP, bytes(bad_gzip)), (H.ZlibWrapper.NONE, bad_raw)):
        ch = H.EmbeddedChannel(H.JdkZlibDecoder(w))
        with pytest.raises(H.DecompressionException):
            ch.write_inbound(bad)
        _read_all(ch)
        for more in (_zlib_side(H, w, BYTES_SMALL), good, b"\x00" * 100):
            ch.write_inbound(more)  # no second exception, and nothing decoded
            assert ch.read_inbound() is None and ch.handler.readable_bytes() == 0
        assert not ch.handler.is_closed()


def test_random_slices_of_a_3mb_stream(H):
    rng = random.Random(3)
    data = IS.big_text(2 * 1024 * 1024, seed=5) + bytes(rng.getrandbits(8) for _ in range(256 * 1024)) + IS.big_text(768 * 1024, seed=6)
    z = gzip.compress(data, 6)
    ref = zlib.decompressobj(31)
    ch = H.EmbeddedChannel(H.JdkZlibDecoder(H.ZlibWrapper.GZIP))
    at, want, got = 0, bytearray(), bytearray()
    while at < len(z):
        k = rng.randint(1, 70000)
        want += ref.decompress(z[at:at + k])
        ch.write_inbound(z[at:at + k])
        got += _read_all(ch)
        at += k
        assert len(got) == len(want), at
    assert bytes(got) == data == bytes(want) and ch.handler.is_closed()
