"""Inputs of the content-checksum and frame-walker tests, shared by the CPU and the GPU files: frames with
a Content_Checksum made from frames without one (bit 2 of the Frame_Header_Descriptor set, the low 32 bits
of XXH64 of the content appended little-endian; tests/test_zstd_checksum_host.py pins that on libzstd),
frames re-headed without a Frame_Content_Size, and skippable frames.  Built once per process."""
import struct

import zstd_decode_inputs as I
import zstd_frames as Z
import zstd_handbuilt as HB

# every tail path of XXH64 (8-, 4- and 1-byte steps), the path under 32 bytes, whole stripes, and 64 KiB
RAW_SIZES = (0, 1, 3, 4, 5, 7, 8, 9, 31, 32, 33, 63, 64, 65, 95, 96, 127, 65536)
VERIFY = 1
OK, UNSUPPORTED, TRUNCATED, CHECKSUM, INVALID_ARG = 0, -83, -85, -88, -100


def checksum_of(content):
    import xxhash
    return struct.pack("<I", xxhash.xxh64(content, seed=0).intdigest() & 0xFFFFFFFF)


def with_checksum(frame, content):
    """`frame` (one frame, no checksum) with the Content_Checksum flag set and the checksum appended"""
    assert not frame[4] & 4
    return frame[:4] + bytes([frame[4] | 4]) + frame[5:] + checksum_of(content)


def _bytes(seed, n):
    import random
    return random.Random(seed).randbytes(n)


def raw_frame(content):
    """one Raw block (sizes up to 128 KiB), single-segment, with checksum"""
    return with_checksum(HB.frame_header(len(content)) + HB.raw_block(content, True), content)


_CACHE = {}


def cases(oracle):
    """(name, frame, content) of every valid checksummed frame of the tests: the Raw-block sizes, a
    two-block frame (the hash spans blocks), a hand-built frame with sequences and without content size,
    and 20 of libzstd's frames"""
    if "cases" not in _CACHE:
        out = [(f"raw_{n}", raw_frame(c), c) for n in RAW_SIZES for c in [_bytes(100 + n, n)]]
        a, b = _bytes(7, 45), _bytes(8, 100)
        two = HB.frame_header(len(a) + 13 + len(b)) + HB.raw_block(a, False) + HB.rle_block(0x41, 13, False) + HB.raw_block(b, True)
        out.append(("three_blocks", with_checksum(two, a + b"A" * 13 + b), a + b"A" * 13 + b))
        f, want = HB.cases()["no_content_size"]
        out.append(("handbuilt_no_content_size", with_checksum(f, want), want))
        picked = [c for c in I.libzstd_frames(oracle)
                  if c.level == 3 and c.n in (5, 300, 5000, 65536, 131073) and c.kind in ("text", "random", "zero", "skew")]
        assert len(picked) == 20
        out += [(f"libzstd_{c.kind}_{c.n}", with_checksum(c.frame, c.data), c.data) for c in picked]
        _CACHE["cases"] = out
    return _CACHE["cases"]


def wrong_checksum(frame, byte=0, bit=0):
    """the checksummed `frame` with one bit of checksum byte `byte` flipped"""
    f = bytearray(frame)
    f[len(f) - 4 + byte] ^= 1 << bit
    return bytes(f)


def without_content_size(frame):
    """`frame` (libzstd's, no checksum) under a header with a window descriptor and no Frame_Content_Size:
    the smallest power-of-two window of 1 KiB or more that holds the content, so every block still fits"""
    f = Z.parse_frame(frame)
    assert f.end == len(frame) and f.dict_id == 0 and not f.checksum and f.content_size is not None
    e = 0
    while (1 << (10 + e)) < f.content_size:
        e += 1
    return Z.MAGIC + bytes([0x00, e << 3]) + frame[f.header:]


def skippable(payload, nibble=0):
    return bytes([0x50 | nibble, 0x2A, 0x4D, 0x18]) + struct.pack("<I", len(payload)) + payload


def host_decode(L, frame, cap, flags):
    """nx_zstd_decode_host_ex: (status, output, consumed); the slot lies between guards that must survive"""
    import ctypes as C
    G = I.GUARD
    buf = (C.c_uint8 * (cap + 2 * G)).from_buffer(bytearray(b"\xa5" * (cap + 2 * G)))
    ol, co = C.c_size_t(0), C.c_size_t(0)
    st = L.nx_zstd_decode_host_ex(frame, len(frame), C.byref(buf, G), cap, C.byref(ol), C.byref(co), flags)
    raw = bytes(buf)
    assert ol.value <= cap
    assert raw[:G] == b"\xa5" * G and raw[G + ol.value:] == b"\xa5" * (cap - ol.value + G), "bytes outside the output changed"
    return st, raw[G:G + ol.value], co.value
