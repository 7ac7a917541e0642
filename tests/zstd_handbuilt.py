"""Hand-built Zstandard frames for the decoder tests: what libzstd's encoder does not emit.  Compressed
blocks carry Raw or RLE literals and all three sequence codes in RLE mode, so the sequence bitstream holds
nothing but extra bits and no FSE encoder is needed.  A Python model (run_sequences) computes the expected
output; tests/test_zstd_decode_host.py first pins both against libzstd.  Also the malformed frames of the
limit cases, each one change away from a valid frame."""
from dataclasses import dataclass

MAGIC = b"\x28\xb5\x2f\xfd"

# RFC 8878 3.1.1.3.2.1.1: (baseline, extra bits) per literal-length and match-length code
LL = [(c, 0) for c in range(16)] + [(16, 1), (18, 1), (20, 1), (22, 1), (24, 2), (28, 2), (32, 3), (40, 3), (48, 4), (64, 6),
                                    (128, 7), (256, 8), (512, 9), (1024, 10), (2048, 11), (4096, 12), (8192, 13), (16384, 14),
                                    (32768, 15), (65536, 16)]
ML = [(c + 3, 0) for c in range(32)] + [(35, 1), (37, 1), (39, 1), (41, 1), (43, 2), (47, 2), (51, 3), (59, 3), (67, 4), (83, 4),
                                        (99, 5), (131, 7), (259, 8), (515, 9), (1027, 10), (2051, 11), (4099, 12), (8195, 13),
                                        (16387, 14), (32771, 15), (65539, 16)]
assert len(LL) == 36 and len(ML) == 53


def frame_header(content_size=None, single=True, window_descriptor=None, descriptor_or=0, dict_id=None):
    """single: a single-segment header with content_size in its smallest field; else a window descriptor and,
    when content_size is given, its smallest field of 2 bytes or more"""
    if single:
        code, n = (0, 1) if content_size < 256 else (1, 2) if content_size < 65536 + 256 else (2, 4)
        d = (code << 6) | 0x20
        fcs = (content_size - (256 if n == 2 else 0)).to_bytes(n, "little")
        wd = b""
    else:
        wd = bytes([window_descriptor])
        if content_size is None:
            d, fcs = 0, b""
        else:
            code, n = (1, 2) if 256 <= content_size < 65536 + 256 else (2, 4)
            d = code << 6
            fcs = (content_size - (256 if n == 2 else 0)).to_bytes(n, "little")
    did = b""
    if dict_id is not None:
        d |= 1
        did = bytes([dict_id])
    return MAGIC + bytes([d | descriptor_or]) + wd + did + fcs


def block_header(last, btype, size):
    return ((size << 3) | (btype << 1) | int(last)).to_bytes(3, "little")


def raw_block(data, last):
    return block_header(last, 0, len(data)) + data


def rle_block(byte, n, last):
    return block_header(last, 1, n) + bytes([byte])


def literals_section(lits):
    """lits: bytes (Raw literals) or ('rle', byte, n)"""
    ltype, n = (1, lits[2]) if isinstance(lits, tuple) else (0, len(lits))
    if n < 32:
        h = bytes([(n << 3) | ltype])
    elif n < 4096:
        h = ((n << 4) | (1 << 2) | ltype).to_bytes(2, "little")
    else:
        h = ((n << 4) | (3 << 2) | ltype).to_bytes(3, "little")
    return h + (bytes([lits[1]]) if ltype else lits)


def nseq_field(n):
    if n < 128:
        return bytes([n])
    if n < 0x7F00:
        return bytes([(n >> 8) + 128, n & 255])
    return b"\xff" + (n - 0x7F00).to_bytes(2, "little")


@dataclass
class Seqs:
    """one block's sequences: the three codes (all RLE mode) and per sequence the three extra-bit values"""
    ll_code: int
    of_code: int
    ml_code: int
    extra: list  # (literal-length extra, match-length extra, offset extra)

    def decoded(self):
        """(literal length, match length, offset value) per sequence"""
        return [(LL[self.ll_code][0] + a, ML[self.ml_code][0] + b, (1 << self.of_code) + c) for a, b, c in self.extra]


def sequences_section(s, modes=0x54):
    """modes 0x54: RLE for literal lengths, offsets and match lengths"""
    if s is None or not s.extra:
        return b"\x00"
    acc, nb = 0, 0
    for a, b, c in reversed(s.extra):  # read backwards: offset, match length, literal length of sequence 0 first
        for v, w in ((a, LL[s.ll_code][1]), (b, ML[s.ml_code][1]), (c, s.of_code)):
            assert 0 <= v < (1 << w) or (w == 0 and v == 0)
            acc |= v << nb
            nb += w
    acc |= 1 << nb  # the padding marker
    stream = acc.to_bytes(nb // 8 + 1, "little")
    return nseq_field(len(s.extra)) + bytes([modes, s.ll_code, s.of_code, s.ml_code]) + stream


def compressed_block(lits, s, last, modes=0x54):
    body = literals_section(lits) + sequences_section(s, modes)
    return block_header(last, 2, len(body)) + body


def run_sequences(out, lits, s, rep):
    """the model: append the block's output to `out` (bytearray), update rep (list of 3) in place"""
    lits = bytes([lits[1]]) * lits[2] if isinstance(lits, tuple) else lits
    at = 0
    for ll, ml, ov in (s.decoded() if s else []):
        out += lits[at:at + ll]
        at += ll
        if ov > 3:
            off = ov - 3
            rep[:] = [off, rep[0], rep[1]]
        else:
            idx = ov + (1 if ll == 0 else 0)
            if idx == 1:
                off = rep[0]
            elif idx == 2:
                off = rep[1]
                rep[:] = [off, rep[0], rep[2]]
            elif idx == 3:
                off = rep[2]
                rep[:] = [off, rep[0], rep[1]]
            else:
                off = rep[0] - 1
                rep[:] = [off, rep[0], rep[1]]
        assert 0 < off <= len(out), (off, len(out))
        for _ in range(ml):
            out.append(out[-off])
    out += lits[at:]


def build(blocks, single=True, window_descriptor=None, with_size=True, **hdr):
    """blocks: ('raw', bytes) | ('rle', byte, n) | ('seq', lits, Seqs or None) | ('ent', lits, sequences, coding):
    a block of tests/zstd_entropy.py's encoder, Huffman and FSE coded as `coding` says.  Returns (frame, expected)."""
    out, rep, body, enc = bytearray(), [1, 4, 8], b"", None
    for i, b in enumerate(blocks):
        last = i == len(blocks) - 1
        if b[0] == "ent":
            if enc is None:
                import zstd_entropy
                enc = zstd_entropy.BlockEncoder()  # one per frame: it holds the tables Repeat_Mode and Treeless reuse
            run_sequences(out, b[1], b[2], rep)
            body += enc.block(b[1], b[2], b[3], last)
        elif b[0] == "raw":
            out += b[1]
            body += raw_block(b[1], last)
        elif b[0] == "rle":
            out += bytes([b[1]]) * b[2]
            body += rle_block(b[1], b[2], last)
        else:
            run_sequences(out, b[1], b[2], rep)
            body += compressed_block(b[1], b[2], last)
    h = frame_header(len(out) if with_size else None, single, window_descriptor, **hdr)
    return h + body, bytes(out)


def _lits(seed, n):
    import random
    return random.Random(seed).randbytes(n)


def cases():
    """name -> (frame, expected output)"""
    c = {}
    # literal-length code 22: 32..39 (3 bits); offset code 4: values 16..31 = offsets 13..28; match length 8
    setup = ("seq", _lits(1, 3 * 36 + 5), Seqs(22, 4, 5, [(4, 0, 0), (0, 0, 7), (7, 0, 15)]))
    # literal length 0: offset value 1 is repeat 2 (swap), 2 is repeat 3, 3 is repeat 1 minus 1
    c["repeat_ll0_code0"] = build([setup, ("seq", b"", Seqs(0, 0, 4, [(0, 0, 0)] * 5))])
    c["repeat_ll0_code1"] = build([setup, ("seq", b"tail", Seqs(0, 1, 2, [(0, 0, 0), (0, 0, 1), (0, 0, 1), (0, 0, 0), (0, 0, 1)]))])
    # literal length 3: value 1 is repeat 1, 2 is repeat 2, 3 is repeat 3
    c["repeat_ll3_code0"] = build([setup, ("seq", _lits(2, 3 * 4 + 2), Seqs(3, 0, 9, [(0, 0, 0)] * 4))])
    c["repeat_ll3_code1"] = build([setup, ("seq", _lits(3, 3 * 6), Seqs(3, 1, 1, [(0, 0, 0), (0, 0, 1), (0, 0, 1), (0, 0, 0), (0, 0, 0), (0, 0, 1)]))])
    # the initial history (1, 4, 8) used directly: 9 literals first
    c["repeat_initial"] = build([("seq", _lits(4, 9 * 3 + 1), Seqs(9, 1, 0, [(0, 0, 0), (0, 0, 1), (0, 0, 0)]))])
    # the history crosses a Raw block and two Compressed blocks
    c["repeat_across_blocks"] = build([setup, ("raw", _lits(5, 20)), ("seq", b"", Seqs(0, 0, 0, [(0, 0, 0)] * 3)),
                                       ("seq", _lits(6, 10), Seqs(5, 0, 3, [(0, 0, 0), (0, 0, 0)]))])
    # overlapping matches longer than 64 bytes: match-length code 43 is 131..258 (7 bits)
    c["overlap_offset1"] = build([("seq", b"Q" + _lits(7, 6), Seqs(1, 2, 43, [(0, 100, 0)]))])         # offset value 4: offset 1
    c["overlap_offset7"] = build([("seq", _lits(8, 7 + 5), Seqs(7, 3, 43, [(0, 127, 2)]))])            # offset value 10: offset 7
    c["overlap_offset7_long"] = build([("seq", _lits(9, 2 * 7), Seqs(7, 3, 46, [(0, 1000, 2), (0, 3, 2)]))])
    # RLE literals
    c["rle_literals"] = build([("seq", ("rle", 0x5A, 40), Seqs(16, 2, 2, [(0, 0, 3), (1, 0, 2)]))])
    c["rle_literals_long"] = build([("seq", ("rle", 0x33, 5000), Seqs(27, 5, 38, [(100, 5, 17), (200, 0, 0)]))])
    # the three forms of the sequence count; literal length 0, match length 3, repeat offsets
    for n in (127, 128, 0x7EFF, 0x7F00):
        c[f"nseq_{n}"] = build([("raw", _lits(10 + n, 16)), ("seq", b"", Seqs(0, 0, 0, [(0, 0, 0)] * n))])
    # no Frame_Content_Size (so a window descriptor: 0x20 is 16 KiB)
    c["no_content_size"] = build([("raw", _lits(20, 300)), ("seq", _lits(21, 33), Seqs(16, 6, 3, [(0, 0, 5), (1, 0, 60)]))],
                                 single=False, window_descriptor=0x20, with_size=False)
    # a window (1 KiB) smaller than the content: blocks of at most 1 KiB
    c["window_below_content"] = build([("raw", _lits(22, 1024)), ("rle", 7, 1000), ("seq", _lits(23, 600), Seqs(25, 9, 40, [(30, 3, 100), (0, 15, 400)])),
                                       ("raw", _lits(24, 500))], single=False, window_descriptor=0)
    c["empty_raw_block"] = build([("raw", b"")])
    c["zero_sequences"] = build([("seq", _lits(25, 77), None), ("seq", ("rle", 9, 3), None)])
    return c


def malformed():
    """name -> (frame, the status it must get); each is one change away from a valid frame"""
    WINDOW, DICT, CHECKSUM, MAGIC_, TRUNC, CORRUPT = -81, -82, -83, -84, -85, -86
    lits = _lits(30, 40)
    s = Seqs(16, 3, 2, [(0, 0, 3), (1, 0, 2)])
    good, want = build([("seq", lits, s)])
    body = good[6:]
    m = {}
    m["checksum_flag"] = (frame_header(len(want), descriptor_or=0x04) + body + b"\x00\x00\x00\x00", CHECKSUM)
    m["dictionary_id"] = (frame_header(len(want), dict_id=5) + body, DICT)
    m["reserved_bit"] = (frame_header(len(want), descriptor_or=0x08) + body, CORRUPT)
    m["block_type_3"] = (frame_header(3) + block_header(True, 3, 3) + b"abc", CORRUPT)
    m["content_size_larger"] = (frame_header(len(want) + 1) + body, CORRUPT)
    m["content_size_smaller"] = (frame_header(len(want) - 1) + body, CORRUPT)
    # Treeless literals (type 3, one stream, regenerated 4, compressed 2) in a frame's first block
    treeless = ((4 << 4) | (2 << 14) | 3).to_bytes(3, "little") + b"\x01\x01" + b"\x00"
    m["treeless_first"] = (frame_header(4, single=False, window_descriptor=0) + block_header(True, 2, len(treeless)) + treeless, CORRUPT)
    rep_body = literals_section(lits) + sequences_section(s, modes=0xFC)
    m["repeat_mode_first"] = (frame_header(len(want)) + block_header(True, 2, len(rep_body)) + rep_body, CORRUPT)
    far = literals_section(lits) + sequences_section(Seqs(2, 3, 0, [(0, 0, 0)]))  # 2 literals, then offset 5
    m["offset_beyond"] = (frame_header(43, single=False, window_descriptor=0) + block_header(True, 2, len(far)) + far, CORRUPT)
    m["skippable_magic"] = (b"\x50\x2a\x4d\x18" + b"\x04\x00\x00\x00abcd", MAGIC_)
    m["unknown_magic"] = (b"\x29" + good[1:], MAGIC_)
    m["window_too_large"] = (MAGIC + bytes([0x00, (18 << 3)]) + raw_block(b"abc", True), WINDOW)  # 2^28
    m["content_too_large"] = (MAGIC + bytes([0xA0]) + (1 << 28).to_bytes(4, "little") + raw_block(b"abc", True), WINDOW)
    m["block_above_window"] = (frame_header(5) + raw_block(b"abcdef", True), CORRUPT)
    m["truncated"] = (good[:-1], TRUNC)
    return m
