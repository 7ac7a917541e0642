"""Fixed, seeded read sequences through every synchronous decoder handle: what
scripts/record_decoder_messages.py records (tests/golden/decoder_messages.json) and
tests/test_gpu_decoder_messages.py replays.  The shapes sit where the handles' shared call frame and
staging can go wrong: no item, one item list empty and the other not, a stream cut between and inside its
parts, a failure after delivered messages, a read after the failure.

No stream comes from the code under test: the committed oracle's frame encoders write the Snappy, FastLZ,
LZF and LZ4 streams, the standard library's zlib and bz2 theirs, libzstd (zstd_decode_inputs) and
zstd_handbuilt the Zstandard frames.  Payloads are handler_sequences.mixed of at most 200 000 bytes, but
for the two cases that need more output than one launch holds.

A case is (name, make, reads).  make(H) builds the handle from netty_amd.handlers; reads() builds the list
of byte strings handed to channel_read in turn (built on first use: listing the cases needs no oracle).
run(H, case) returns the record of the whole sequence."""
import bz2
import functools
import hashlib
import random
import zlib

import handler_sequences as S

mixed = S.mixed


def _oracle():
    from oracle import pyoracle
    pyoracle.build()
    return pyoracle


def _rand(seed, n):
    return random.Random(0xDEC + seed).randbytes(n)


def _patch(stream, at, fn):
    b = bytearray(stream)
    b[at] = fn(b[at]) & 0xFF
    return bytes(b)


def _thirds(s):
    a, b = len(s) // 3, 2 * len(s) // 3
    return [s[:a], s[a:b], s[b:]]


# ------------------------------------------------------------------------------------- Snappy
SNAPPY_HEADER = b"\xff\x06\x00\x00sNaPpY"


def _snappy_raw(data):
    """an uncompressed chunk: type 1, length, masked CRC32C, the bytes"""
    return b"\x01" + (len(data) + 4).to_bytes(3, "little") + _oracle().snappy_checksum(data).to_bytes(4, "little") + data


def _snappy_chunks(data):
    """the chunks SnappyFrameEncoder writes for data, without the stream header"""
    out, at, chunks = _oracle().snappy_frame_encode(data, started=True)[0], 0, []
    while at < len(out):
        n = 4 + int.from_bytes(out[at + 1:at + 4], "little")
        chunks.append(out[at:at + n])
        at += n
    return chunks


def _snappy_cases():
    def both():  # a compressed chunk and the raw chunk of the 10 bytes left over
        c = _snappy_chunks(mixed(1001, 32767 + 10))
        assert [x[0] for x in c] == [0, 1]
        return c

    def comp3():
        c = _snappy_chunks(mixed(1002, 70000))
        assert [x[0] for x in c] == [0, 0, 0]
        return c

    def cut_inside():
        c = both() + comp3()[2:]
        s = SNAPPY_HEADER + b"".join(c)
        h = len(SNAPPY_HEADER) + 2                        # two bytes into the first chunk's header
        b = len(SNAPPY_HEADER) + len(c[0]) + len(c[1]) + 100  # inside the third chunk's body
        return [s[:h], s[h:b], s[b:]]

    def bad_crc(kind):  # a good message, then a chunk of `kind` whose stored CRC has one bit flipped, then a read after it
        good, bad = comp3()[2], (comp3()[1] if kind == 0 else _snappy_raw(mixed(1003, 500)))
        assert bad[0] == kind
        return [SNAPPY_HEADER + good + _patch(bad, 4, lambda v: v ^ 1), good]

    shapes = {
        "header_alone": lambda: [SNAPPY_HEADER],
        "raw_only": lambda: [SNAPPY_HEADER + _snappy_raw(mixed(1004, 300)) + _snappy_raw(mixed(1005, 5000))],
        "compressed_only": lambda: [SNAPPY_HEADER + b"".join(comp3())],
        "both_kinds": lambda: [SNAPPY_HEADER + b"".join(both())],
        "under_18_bytes": lambda: [_oracle().snappy_frame_encode(mixed(1006, 17))[0]],
        "cut_at_chunks": lambda: [SNAPPY_HEADER] + both() + comp3(),
        "cut_inside": cut_inside,
        "skippable": lambda: [SNAPPY_HEADER + b"\x80\x05\x00\x00hello" + b"".join(both())],
        "crc_mismatch_compressed": lambda: bad_crc(0),
        "crc_mismatch_raw": lambda: bad_crc(1),
    }
    return [(f"snappy/validate{v}/{name}", lambda H, v=v: H.SnappyFrameDecoder(bool(v)), reads)
            for v in (0, 1) for name, reads in shapes.items()]


# ------------------------------------------------------------------------------------- FastLZ / LZF / LZ4
def _alt_cases():
    text = lambda k: mixed(1100 + k, 60000)
    out = []

    def add(codec, variant, make, enc, zero_block, damage, walk, tail=None):
        """enc(data) is one message's blocks; damage and walk patch the second of two blocks"""
        def after_good(fn):
            def reads():
                a, b = enc(text(1)), enc(text(2))
                return [a + fn(a, b), enc(text(3))]  # the failure after a good message, then a read after it
            return reads

        shapes = {
            "compressed_only": lambda: [enc(text(1)) + enc(text(2)) + enc(text(3))],
            "raw_only": lambda: [enc(_rand(1, 40000)) + enc(_rand(2, 30000))],
            "mixed": lambda: [enc(text(1)) + enc(_rand(3, 40000)) + enc(text(2)) + enc(_rand(4, 100))],
            "damaged_block": after_good(damage),
            "walk_error": after_good(walk),
        }
        if zero_block:
            shapes["zero_length_block"] = lambda: [enc(text(1)) + zero_block + enc(text(2))]
        if tail:
            shapes.update(tail)
        out.extend((f"{codec}/{variant}/{name}", make, reads) for name, reads in shapes.items())

    O = _oracle
    for cks, val in ((0, 0), (1, 0), (1, 1)):
        enc = lambda d, c=cks: O().fastlz_frame_encode(d, 0, bool(c))
        hdr = 4 + 4 * cks  # up to chunkLength; originalLength's low byte is at hdr + 3
        add("fastlz", f"checksum{cks}_validate{val}", lambda H, v=val: H.FastLzFrameDecoder(bool(v)), enc, b"FLZ\x00\x00\x00",
            lambda a, b, h=hdr: _patch(b, h + 3, lambda v: v + 1 if v < 255 else v - 1),
            lambda a, b: _patch(b, 1, lambda v: v ^ 0x20),
            # the next block's first five bytes stand behind the frame: the decoder's readable bytes go on past its block
            {"trailing_bytes": lambda e=enc: [e(text(1)) + e(text(2))[:5], e(text(2))[5:]]})
    add("lzf", "plain", lambda H: H.LzfDecoder(), lambda d: O().lzf_frame_encode(d), b"ZV\x00\x00\x00",
        lambda a, b: _patch(b, 6, lambda v: v + 1 if v < 255 else v - 1), lambda a, b: _patch(b, 1, lambda v: v ^ 0x20))
    for val in (0, 1):
        enc = lambda d: O().lz4_frame_encode(d, close=False)
        add("lz4", f"validate{val}", lambda H, v=val: H.Lz4FrameDecoder(bool(v)), enc, None,
            lambda a, b: _patch(b, 13, lambda v: v + 1 if v < 255 else v - 1),  # decompressedLength off by one
            lambda a, b: _patch(b, 2, lambda v: v ^ 1),
            {"checksum_mismatch": lambda e=enc: [e(text(1)) + _patch(e(text(2)), 17, lambda v: v ^ 1), e(text(3))],
             "end_block_then_junk": lambda: [O().lz4_frame_encode(text(1), close=True) + _rand(5, 30), _rand(6, 50)]})
    return out


# ------------------------------------------------------------------------------------- Zstd
def _zstd_frame(kind, n, level):
    import zstd_decode_inputs
    for c in zstd_decode_inputs.libzstd_frames(_oracle()):
        if (c.kind, c.n, c.level) == (kind, n, level):
            return c.frame
    raise KeyError((kind, n, level))


def _zstd_cases():
    import zstd_handbuilt as HB
    f1 = lambda: _zstd_frame("text", 5000, 3)
    f2 = lambda: _zstd_frame("skew", 1024, 19)
    f3 = lambda: _zstd_frame("text", 65536, 3)
    skip = b"\x53\x2a\x4d\x18" + (9).to_bytes(4, "little") + b"skippable"
    bad = lambda: HB.malformed()["content_size_larger"][0]
    make = lambda m: (lambda H: H.ZstdDecoder(m))
    out = [
        ("zstd/one_frame", make(0), lambda: [f1()]),
        ("zstd/frames_and_skippable", make(0), lambda: [f1() + skip + f2() + f3()]),
        ("zstd/three_reads", make(0), lambda: _thirds(f3())),
        ("zstd/empty_frame", make(0), lambda: [HB.cases()["empty_raw_block"][0], f1()]),
        ("zstd/bad_after_good_one_read", make(0), lambda: [f1() + bad() + f2(), f1()]),
        ("zstd/bad_in_later_read", make(0), lambda: [f1(), bad(), f1()]),
    ]
    out += [(f"zstd/maximum_allocation_size{m}", make(m), lambda: [f1()]) for m in (0, 1000, 1 << 20)]
    return out


# ------------------------------------------------------------------------------------- zlib
def _deflate(data, wbits, **kw):
    c = zlib.compressobj(6, zlib.DEFLATED, wbits, **kw)
    return c.compress(data) + c.flush()


def _gzip_all_fields(data):
    """a member whose header has FEXTRA (an empty field), FNAME, FCOMMENT and FHCRC"""
    h = b"\x1f\x8b\x08\x1e" + bytes(4) + b"\x00\x03" + b"\x00\x00" + b"name.txt\x00" + b"a comment\x00"
    h += (zlib.crc32(h) & 0xFFFF).to_bytes(2, "little")
    return h, _deflate(data, -15) + zlib.crc32(data).to_bytes(4, "little") + (len(data) & 0xFFFFFFFF).to_bytes(4, "little")


def _zlib_cases():
    data = lambda: mixed(1300, 100000)
    big = lambda: mixed(1301, 200000) * 11  # 2 200 000 bytes: three output chunks of one read
    dic = lambda: mixed(1302, 5000)
    with_dict = lambda: _deflate(dic()[1000:4000] + mixed(1303, 20000), 15, zdict=dic())

    def split_header():
        h, rest = _gzip_all_fields(data())
        return [h[i:i + 1] for i in range(len(h))] + [rest]

    def data_error():  # 64 bytes of 0xFF well behind the first output chunks
        s = bytearray(_deflate(big(), 15))
        at = len(s) * 9 // 10
        s[at:at + 64] = b"\xff" * 64
        return [bytes(s), b"after"]

    Z = lambda w, **kw: (lambda H: H.JdkZlibDecoder(H.ZlibWrapper[w], **kw))
    two = lambda: _deflate(data(), 31) + _deflate(mixed(1304, 3000), 31)
    return [
        ("zlib/ZLIB", Z("ZLIB"), lambda: [_deflate(data(), 15), b"behind the stream"]),
        ("zlib/GZIP", Z("GZIP"), lambda: [_deflate(data(), 31)]),
        ("zlib/NONE", Z("NONE"), lambda: [_deflate(data(), -15)]),
        ("zlib/ZLIB_OR_NONE/zlib", Z("ZLIB_OR_NONE"), lambda: [_deflate(data(), 15)]),
        ("zlib/ZLIB_OR_NONE/none", Z("ZLIB_OR_NONE"), lambda: [_deflate(data(), -15)]),
        ("zlib/gzip_header_byte_by_byte", Z("GZIP"), split_header),
        ("zlib/concatenated_on", Z("GZIP", decompress_concatenated=True), lambda: [two()]),
        ("zlib/concatenated_off", Z("GZIP"), lambda: [two()]),
        ("zlib/several_chunks", Z("ZLIB"), lambda: [_deflate(big(), 15)]),
        ("zlib/three_reads", Z("GZIP"), lambda: _thirds(_deflate(data(), 31))),
        ("zlib/dictionary_right", lambda H: H.JdkZlibDecoder(dictionary=dic()), lambda: [with_dict()]),
        ("zlib/dictionary_wrong", lambda H: H.JdkZlibDecoder(dictionary=dic()[:-1]), lambda: [with_dict(), b"after"]),
        ("zlib/dictionary_missing", Z("ZLIB"), lambda: [with_dict()]),
        ("zlib/max_allocation_reached", Z("ZLIB", max_allocation=1000), lambda: [_deflate(mixed(1305, 5000), 15), b"after"]),
        ("zlib/max_allocation_holds", Z("ZLIB", max_allocation=8000), lambda: [_deflate(mixed(1305, 5000), 15)]),
        ("zlib/data_error_after_output", Z("ZLIB"), data_error),
        ("zlib/bad_trailer/zlib", Z("ZLIB"), lambda: [_patch(_deflate(data(), 15), -1, lambda v: v ^ 1), b"after"]),
        ("zlib/bad_trailer/gzip_crc", Z("GZIP"), lambda: [_patch(_deflate(data(), 31), -8, lambda v: v ^ 1), b"after"]),
        ("zlib/bad_trailer/gzip_length", Z("GZIP"), lambda: [_patch(_deflate(data(), 31), -4, lambda v: v ^ 1), b"after"]),
    ]


# ------------------------------------------------------------------------------------- Bzip2
def bzip2_magics(stream):
    """bit positions of the block magics and of the end magics of stream (a search of its bit string:
    bzip2_streams.find_magics, which tries every position with big-integer shifts, takes minutes on 100 KB)"""
    bits = bin(int.from_bytes(b"\x01" + stream, "big"))[3:]
    found = []
    for magic in (0x314159265359, 0x177245385090):
        pat, at, hits = format(magic, "048b"), 0, []
        while (at := bits.find(pat, at)) >= 0:
            hits.append(at)
            at += 1
        found.append(hits)
    return found


GROW_STREAM_BYTES = 600000  # zero bytes through bz2.compress(.., 1): one block that decodes to more than the first slot


def _bzip2_cases():
    import bzip2_streams as BS
    one = lambda: bz2.compress(mixed(1400, 50000), 1)
    two = lambda: bz2.compress(mixed(1401, 150000), 1)

    def second_block_crc():
        s = two()
        blocks, ends = bzip2_magics(s)
        assert len(blocks) == 2 and len(ends) == 1
        return [BS.flip_bit(s, blocks[1] + 48 + 7), b"after"]

    make = lambda H: H.Bzip2Decoder()
    return [(f"bzip2/{name}", make, reads) for name, reads in {
        "header_3_then_rest": lambda: [one()[:3], one()[3:]],
        "empty_stream": lambda: [bz2.compress(b"", 1)],
        "one_block": lambda: [one()],
        "two_blocks": lambda: [two()],
        "three_reads": lambda: _thirds(one()),
        "bytes_after_end": lambda: [one() + b"behind the end marker", b"more"],
        "second_block_crc": second_block_crc,
        "bad_magic": lambda: [BS.flip_bit(one(), 32 + 5), b"after"],
        "bad_stream_header": lambda: [b"BZx1" + one()[4:], b"after"],
        "grow_and_retry": lambda: [bz2.compress(bytes(GROW_STREAM_BYTES), 1)],
    }.items()]


def cases():
    return _snappy_cases() + _alt_cases() + _zstd_cases() + _zlib_cases() + _bzip2_cases()


@functools.lru_cache(maxsize=None)
def _reads_by_name(name):
    return {c[0]: c[2] for c in cases()}[name]()


def reads(case):
    """the case's reads, built once per process"""
    return _reads_by_name(case[0])


def digest(pieces):
    return [{"sha256": hashlib.sha256(p).hexdigest(), "len": len(p)} for p in pieces]


def run(H, case):
    """Each read's messages (SHA-256 and length) or its exception (class, .status, text, the digests of
    .decoded), the bytes left in the cumulation after it, and is_closed() and stats() at the end where the
    handle has them."""
    d = case[1](H)
    rec = {"reads": []}
    try:
        for data in reads(case):
            try:
                r = {"msgs": digest(d.channel_read(data))}
            except Exception as e:  # noqa: BLE001 - whatever the handle raises is what is recorded
                r = {"error": {"class": type(e).__name__, "status": getattr(e, "status", None), "text": str(e),
                               "decoded": digest(getattr(e, "decoded", []))}}
            r["readable"] = d.readable_bytes()
            rec["reads"].append(r)
        if hasattr(d, "is_closed"):
            rec["closed"] = d.is_closed()
        if hasattr(d, "stats"):
            rec["stats"] = d.stats()
    finally:
        d.close()
    return rec


def input_digest(case):
    """one hash over a case's reads and their lengths, so that a drifting generator is told apart from drifting output"""
    h = hashlib.sha256()
    for data in reads(case):
        h.update(len(data).to_bytes(8, "little"))
        h.update(data)
    return h.hexdigest()
