"""Deflate streams for the inflate tests, and zlib as their reference.

Crafted streams are written with an LSB-first bit writer that emits arbitrary RFC 1951 blocks (stored,
fixed, dynamic with any header), so they reach corners no encoder of this project or zlib produces;
one crafted stream per error site of zlib's inflate(); a seeded corpus of damaged valid streams.
`reference()` is what the GPU inflater must reproduce: Python's zlib (the library
java.util.zip.Inflater wraps).  Everything is built once per process.
"""
import ctypes as C
import ctypes.util
import functools
import random
import zlib
from collections import namedtuple

# ------------------------------------------------------------------------------------ reference
Outcome = namedtuple("Outcome", "kind out text consumed")  # kind: "end" | "need" | "error"


class _ZStream(C.Structure):
    _fields_ = [("next_in", C.c_void_p), ("avail_in", C.c_uint), ("total_in", C.c_ulong), ("next_out", C.c_void_p),
                ("avail_out", C.c_uint), ("total_out", C.c_ulong), ("msg", C.c_char_p), ("state", C.c_void_p),
                ("zalloc", C.c_void_p), ("zfree", C.c_void_p), ("opaque", C.c_void_p), ("data_type", C.c_int),
                ("adler", C.c_ulong), ("reserved", C.c_ulong)]


@functools.lru_cache(maxsize=None)
def _libz():
    """the libz Python's zlib module runs on (the same version), through its C interface"""
    L = C.CDLL(C.util.find_library("z"))
    L.zlibVersion.restype = C.c_char_p
    assert L.zlibVersion().decode() == zlib.ZLIB_RUNTIME_VERSION
    L.inflateInit2_.argtypes = [C.POINTER(_ZStream), C.c_int, C.c_char_p, C.c_int]
    L.inflate.argtypes = [C.POINTER(_ZStream), C.c_int]
    L.inflateEnd.argtypes = [C.POINTER(_ZStream)]
    return L


def reference(stream: bytes, wbits: int = -15, bytewise: bool = False) -> Outcome:
    """zlib's inflate() over the stream, whole or (bytewise) fed byte by byte: the output and whether
    the stream ended (consumed = bytes up to the end of the final block), wants more input, or failed
    (text = zlib's message, out = every byte of the symbols before the error).  Python's zlib module
    drops the output of a failing call, so this drives the same libz through its C interface."""
    L = _libz()
    zs = _ZStream()
    assert L.inflateInit2_(C.byref(zs), wbits, L.zlibVersion(), C.sizeof(_ZStream)) == 0
    src = C.create_string_buffer(stream, max(len(stream), 1))
    buf = C.create_string_buffer(1 << 16)
    out = bytearray()
    try:
        step = 1 if bytewise else max(len(stream), 1)
        for at in range(0, len(stream), step):
            zs.next_in = C.addressof(src) + at
            zs.avail_in = min(step, len(stream) - at)
            while True:
                zs.next_out = C.addressof(buf)
                zs.avail_out = len(buf)
                rc = L.inflate(C.byref(zs), 0)
                out += buf.raw[:len(buf) - zs.avail_out]
                if rc == 1:  # Z_STREAM_END
                    return Outcome("end", bytes(out), None, zs.total_in)
                if rc == -3:  # Z_DATA_ERROR
                    return Outcome("error", bytes(out), zs.msg.decode(), None)
                assert rc in (0, -5), rc  # Z_OK, Z_BUF_ERROR (no progress possible)
                if zs.avail_out:
                    break
        return Outcome("need", bytes(out), None, None)
    finally:
        L.inflateEnd(C.byref(zs))


# ------------------------------------------------------------------------------------ bit writer
class BitWriter:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, v: int, n: int):
        """n bits of v, least significant first (header fields, extra bits)"""
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, code: int, length: int):
        """a Huffman code, most significant bit first"""
        for k in range(length - 1, -1, -1):
            self.bits((code >> k) & 1, 1)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def raw(self, b: bytes):
        assert self.n == 0
        self.out += b

    def done(self) -> bytes:
        self.align()
        return bytes(self.out)


def canonical(lens: dict) -> dict:
    """{symbol: length} -> {symbol: (code, length)} by RFC 1951 3.2.2"""
    codes, code = {}, 0
    for bl in range(1, 16):
        for s in sorted(k for k, v in lens.items() if v == bl):
            codes[s] = (code, bl)
            code += 1
        code <<= 1
    return codes


def complete_lengths(symbols) -> dict:
    """a complete code over the symbols (two or more): lengths k - 1 and k"""
    syms = sorted(symbols)
    assert len(set(syms)) == len(syms)
    n = len(syms)
    assert n >= 2
    k = (n - 1).bit_length()
    short = (1 << k) - n
    return {s: (k - 1 if i < short else k) for i, s in enumerate(syms)}


LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def len_sym(length):
    i = 28 if length == 258 else max(k for k in range(28) if LEN_BASE[k] <= length)
    return 257 + i, LEN_EXTRA[i], length - LEN_BASE[i]


def dist_sym(dist):
    i = max(k for k in range(30) if DIST_BASE[k] <= dist)
    return i, DIST_EXTRA[i], dist - DIST_BASE[i]


FIXED_LIT = canonical({s: (8 if s < 144 else 9 if s < 256 else 7 if s < 280 else 8) for s in range(288)})
FIXED_DIST = canonical({s: 5 for s in range(32)})


def tokens(bw: BitWriter, toks, lit, dist, eob=True):
    """toks: ints (literals) and (length, distance) pairs, in the codes `lit` / `dist`"""
    for t in toks:
        if isinstance(t, int):
            bw.code(*lit[t])
        else:
            s, eb, ev = len_sym(t[0])
            bw.code(*lit[s])
            bw.bits(ev, eb)
            s, eb, ev = dist_sym(t[1])
            bw.code(*dist[s])
            bw.bits(ev, eb)
    if eob:
        bw.code(*lit[256])


def stored(bw: BitWriter, data: bytes, final=False):
    bw.bits(1 if final else 0, 1)
    bw.bits(0, 2)
    bw.align()
    bw.raw(len(data).to_bytes(2, "little") + (len(data) ^ 0xFFFF).to_bytes(2, "little") + data)


def fixed(bw: BitWriter, toks, final=False, eob=True):
    bw.bits(1 if final else 0, 1)
    bw.bits(1, 2)
    tokens(bw, toks, FIXED_LIT, FIXED_DIST, eob)


# code-length code used by the crafted dynamic headers: complete over all 19 symbols
CL_LENS = {s: (4 if s < 13 else 5) for s in range(19)}


def rle(lens):
    """greedy run-length coding of a length list into code-length symbols (sym, extra value)"""
    out, i = [], 0
    while i < len(lens):
        v, j = lens[i], i
        while j < len(lens) and lens[j] == v:
            j += 1
        run = j - i
        if v == 0 and run >= 3:
            r = min(run, 138)
            out.append((18, r - 11) if r >= 11 else (17, r - 3))
            i += r
        elif v != 0 and run >= 4:
            out.append((v, 0))
            r = min(run - 1, 6)
            out.append((16, r - 3))
            i += 1 + r
        else:
            out.append((v, 0))
            i += 1
    return out


def dyn_header(bw: BitWriter, final, nl, nd, cl_syms, cl_lens=None, hclen=19):
    cl_lens = CL_LENS if cl_lens is None else cl_lens
    bw.bits(1 if final else 0, 1)
    bw.bits(2, 2)
    bw.bits(nl - 257, 5)
    bw.bits(nd - 1, 5)
    bw.bits(hclen - 4, 4)
    for k in range(hclen):
        bw.bits(cl_lens.get(CL_ORDER[k], 0), 3)
    cl = canonical(cl_lens)
    for s, ev in cl_syms:
        bw.code(*cl[s])
        if s >= 16:
            bw.bits(ev, {16: 2, 17: 3, 18: 7}[s])


def dynamic(bw: BitWriter, toks, lit_lens: dict, dist_lens: dict, final=False, nl=None, nd=None, eob=True):
    nl = max(257, max(lit_lens) + 1) if nl is None else nl
    nd = max(1, max(dist_lens) + 1 if dist_lens else 1) if nd is None else nd
    lens = [lit_lens.get(s, 0) for s in range(nl)] + [dist_lens.get(s, 0) for s in range(nd)]
    dyn_header(bw, final, nl, nd, rle(lens))
    tokens(bw, toks, canonical(lit_lens), canonical(dist_lens), eob)


def _text(rng, n):
    words = ["netty", "channel", "buffer", "pipeline", "handler", "codec", "frame", "the", "of", "and", "a", "inflate",
             "window", "stream", "block", "0123456789", "\n", "GET /index.html HTTP/1.1\r\n", "Content-Encoding: gzip\r\n"]
    out = bytearray()
    while len(out) < n:
        out += rng.choice(words).encode() + (b" " if rng.random() < 0.8 else b"")
        if rng.random() < 0.05:
            out += bytes(rng.getrandbits(8) for _ in range(rng.randint(1, 6)))
    return bytes(out[:n])


def _chain_lengths(symbols):
    """lengths 1, 2, ..., 14, 15, 15 over sixteen symbols: a complete code that reaches 15 bits"""
    assert len(symbols) == 16
    return {s: min(i + 1, 15) for i, s in enumerate(symbols)}


# ------------------------------------------------------------------------------------ crafted, valid
@functools.lru_cache(maxsize=None)
def crafted_valid() -> dict:
    rng = random.Random(1951)
    S = {}

    for n in (0, 1, 65535):
        bw = BitWriter()
        stored(bw, bytes(rng.getrandbits(8) for _ in range(n)), final=True)
        S[f"stored_{n}"] = bw.done()

    # a fixed block with every length base and every distance base, after 32 KiB of history
    bw = BitWriter()
    stored(bw, _text(rng, 32768 + 300))
    toks = [ord("q")]
    toks += [(LEN_BASE[i], 1 + 37 * i) for i in range(29)]
    toks += [(3 + (i % 5), DIST_BASE[i]) for i in range(30)]
    toks += [(258, 32768), (LEN_BASE[27] + 31, DIST_BASE[29] + 8191)]  # the largest extra-bit values
    fixed(bw, toks, final=True)
    S["fixed_all_bases"] = bw.done()

    bw = BitWriter()
    fixed(bw, [ord("x"), (258, 1), (258, 1), ord("y"), (3, 1)], final=True)
    S["rle_distance_1"] = bw.done()

    bw = BitWriter()
    toks = list(b"abcdefg")
    for d in range(2, 8):
        toks += [(3, d), (d + 1, d), (64 + d, d), (65, d), (258, d), ord("A") + d]
    fixed(bw, toks, final=True)
    S["overlap_2_to_7"] = bw.done()

    # a dynamic block whose literal/length and distance codes both reach 15 bits
    lit_syms = [ord(c) for c in "etaoinshrdlucm"] + [256, 257 + 9]
    lit = _chain_lengths(lit_syms)
    dist = _chain_lengths(list(range(16)))
    bw = BitWriter()
    toks = [rng.choice(lit_syms[:14]) for _ in range(400)]
    for k in range(16):
        toks += [ord("e"), (13 + (k & 1), DIST_BASE[k]), lit_syms[13 - (k % 14)]]
    dynamic(bw, toks, lit, dist, final=True)
    S["dynamic_15_bit_codes"] = bw.done()

    # repeat symbols that run across the literal/distance boundary
    bw = BitWriter()  # 16: 2,2,2 | 2,2,2,2
    lit = {ord("a"): 3, ord("b"): 4, 256: 4, 257: 2, 258: 2, 259: 2}
    dynamic(bw, [ord("a"), ord("b"), ord("a"), (3, 2), (4, 1), (5, 3), ord("b"), (3, 4)], lit, {0: 2, 1: 2, 2: 2, 3: 2},
            final=True, nl=260, nd=4)
    S["repeat_16_across_boundary"] = bw.done()
    bw = BitWriter()  # 17: 0,0,0,0 | 0,0,0 then 1
    lit = {ord("a"): 1, ord("b"): 2, 256: 3, 257: 3}
    dynamic(bw, [ord("a"), ord("b"), ord("a"), ord("b"), (3, 4), ord("a")], lit, {3: 1}, final=True, nl=262, nd=4)
    S["repeat_17_across_boundary"] = bw.done()
    bw = BitWriter()  # 18: ten zeros | five zeros then 1
    dynamic(bw, list(b"abababab") + [(3, 7), (3, 8), ord("b")], lit, {5: 1}, final=True, nl=268, nd=6)
    S["repeat_18_across_boundary"] = bw.done()

    bw = BitWriter()  # one distance code (an incomplete code zlib accepts: a single one-bit code)
    lit = complete_lengths([ord("x"), ord("y"), ord("z"), 256, 257, 258, 264, 285])
    dynamic(bw, list(b"xyzzy") + [(3, 1), (4, 1), (10, 1), (258, 1), ord("x")], lit, {0: 1}, final=True)
    S["single_distance_code"] = bw.done()

    bw = BitWriter()  # no distance code at all, literals only
    lit = complete_lengths(sorted(set(b"only literals really")) + [256])
    dynamic(bw, list(b"only literals really") * 9, {**lit}, {}, final=True)
    S["no_distance_code"] = bw.done()

    bw = BitWriter()  # 300 blocks of mixed types
    lit = complete_lengths(sorted(set(b"mixed blocks")) + [256, 257, 258, 260])
    dist = complete_lengths([0, 1, 2, 3, 4, 9])
    for b in range(300):
        final = b == 299
        if b % 3 == 0:
            stored(bw, _text(rng, b % 41), final=final)
        elif b % 3 == 1:
            fixed(bw, list(_text(rng, 5 + b % 23)) + ([(3 + b % 30, 1 + b % 17)] if b > 3 else []), final=final)
        else:
            toks = [rng.choice(list(b"mixed blocks")) for _ in range(3 + b % 19)] + [(3, 1), (4, 2 + b % 3), (6, 5 + b % 2)]
            dynamic(bw, toks, lit, dist, final=final)
    S["mixed_300_blocks"] = bw.done()
    return S


# ------------------------------------------------------------------------------------ crafted, invalid
@functools.lru_cache(maxsize=None)
def crafted_invalid() -> dict:
    """name -> (stream, zlib's message); most begin with output, so the bytes before the error count"""
    E = {}

    def start():
        bw = BitWriter()
        fixed(bw, list(b"before the error "))
        return bw

    bw = start()
    bw.bits(1, 1)
    bw.bits(3, 2)
    bw.bits(0, 16)
    E["block_type"] = (bw.done(), "invalid block type")

    bw = start()
    bw.bits(0, 3)
    bw.align()
    bw.raw(bytes([5, 0, 5, 0]) + b"12345")
    E["stored_lengths"] = (bw.done(), "invalid stored block lengths")

    bw = start()
    bw.bits(0, 1)
    bw.bits(2, 2)
    bw.bits(30, 5)  # HLIT = 287
    bw.bits(0, 5)
    bw.bits(0, 4)
    bw.bits(0, 64)
    E["too_many_symbols"] = (bw.done(), "too many length or distance symbols")

    bw = start()
    bw.bits(0, 1)
    bw.bits(2, 2)
    bw.bits(0, 5)
    bw.bits(31, 5)  # HDIST = 32
    bw.bits(0, 4)
    bw.bits(0, 64)
    E["too_many_distance_symbols"] = (bw.done(), "too many length or distance symbols")

    bw = start()  # three code-length codes of one bit: over-subscribed
    dyn_header(bw, False, 257, 1, [], cl_lens={16: 1, 17: 1, 18: 1}, hclen=4)
    bw.bits(0, 64)
    E["code_lengths_over"] = (bw.done(), "invalid code lengths set")

    bw = start()  # one code-length code of two bits: incomplete
    dyn_header(bw, False, 257, 1, [], cl_lens={0: 2}, hclen=4)
    bw.bits(0, 64)
    E["code_lengths_incomplete"] = (bw.done(), "invalid code lengths set")

    bw = start()  # repeat-previous with no previous length
    dyn_header(bw, False, 257, 1, [(16, 0)])
    bw.bits(0, 64)
    E["repeat_without_previous"] = (bw.done(), "invalid bit length repeat")

    bw = start()  # a zero run past the last length
    dyn_header(bw, False, 257, 1, [(18, 127), (18, 110)])
    bw.bits(0, 64)
    E["repeat_past_end"] = (bw.done(), "invalid bit length repeat")

    bw = start()  # no code for end-of-block
    lens = [0] * 258
    lens[65] = lens[66] = 1
    dyn_header(bw, False, 257, 1, rle(lens))
    bw.bits(0, 64)
    E["missing_end_of_block"] = (bw.done(), "invalid code -- missing end-of-block")

    bw = start()  # a code-length code with no codes at all: every length reads as 0 (inftrees.c)
    dyn_header(bw, False, 257, 1, [], cl_lens={}, hclen=4)
    bw.bits(0, 400)
    E["empty_code_length_code"] = (bw.done(), "invalid code -- missing end-of-block")

    bw = start()  # three literal/length codes of one bit
    lens = [0] * 258
    lens[65] = lens[66] = lens[256] = 1
    dyn_header(bw, False, 257, 1, rle(lens))
    bw.bits(0, 64)
    E["litlen_set_over"] = (bw.done(), "invalid literal/lengths set")

    bw = start()  # two literal/length codes of two bits: incomplete and longer than one bit
    lens = [0] * 258
    lens[65] = lens[256] = 2
    dyn_header(bw, False, 257, 1, rle(lens))
    bw.bits(0, 64)
    E["litlen_set_incomplete"] = (bw.done(), "invalid literal/lengths set")

    bw = start()  # a complete literal/length code, two distance codes of two bits
    lens = [0] * 257 + [2, 2]
    lens[65] = lens[256] = 1
    dyn_header(bw, False, 257, 2, rle(lens))
    bw.bits(0, 64)
    E["distance_set_incomplete"] = (bw.done(), "invalid distances set")

    bw = start()
    lens = [0] * 257 + [1, 1, 1]
    lens[65] = lens[256] = 1
    dyn_header(bw, False, 257, 3, rle(lens))
    bw.bits(0, 64)
    E["distance_set_over"] = (bw.done(), "invalid distances set")

    bw = start()  # the fixed code's unused literal/length symbol 286
    fixed(bw, list(b"ab"), eob=False)
    bw.code(*FIXED_LIT[286])
    bw.bits(0, 32)
    E["litlen_code_286"] = (bw.done(), "invalid literal/length code")

    bw = start()  # a one-bit incomplete literal/length code, the unassigned bit
    lens = [0] * 258
    lens[256] = 1
    dyn_header(bw, False, 257, 1, rle(lens))
    bw.bits(1, 1)
    bw.bits(0, 32)
    E["litlen_code_unassigned"] = (bw.done(), "invalid literal/length code")

    bw = start()  # the fixed code's unused distance symbol 30
    fixed(bw, list(b"ab"), eob=False)
    bw.code(*FIXED_LIT[257])
    bw.code(*FIXED_DIST[30])
    bw.bits(0, 32)
    E["distance_code_30"] = (bw.done(), "invalid distance code")

    bw = start()  # a block without distance codes that uses a length
    lit = complete_lengths([ord("a"), 256, 257, 258])
    dynamic(bw, [ord("a")], lit, {}, eob=False)
    bw.code(*canonical(lit)[257])
    bw.bits(0, 32)
    E["distance_code_none"] = (bw.done(), "invalid distance code")

    bw = start()  # a single one-bit distance code, the other bit
    dynamic(bw, [ord("a"), (3, 1)], lit, {0: 1}, eob=False)
    bw.code(*canonical(lit)[257])
    bw.bits(1, 1)
    bw.bits(0, 32)
    E["distance_code_unassigned"] = (bw.done(), "invalid distance code")

    bw = BitWriter()  # a copy from before the start of the stream
    fixed(bw, list(b"ab") + [(3, 3)], final=True)
    E["distance_too_far"] = (bw.done(), "invalid distance too far back")

    bw = start()  # 17 bytes of output, then distance 18
    fixed(bw, [(10, 18)], final=True)
    E["distance_too_far_by_one"] = (bw.done(), "invalid distance too far back")
    return E


# ------------------------------------------------------------------------------------ the split-point stream
@functools.lru_cache(maxsize=None)
def split_stream() -> bytes:
    """About 2.5 KB with stored, fixed and dynamic blocks and a copy at distance 32768."""
    rng = random.Random(32768)
    bw = BitWriter()
    fixed(bw, [ord("A")] + [(258, 1)] * 126 + list(_text(rng, 259)))  # 1 + 32508 + 259 = 32768 bytes
    fixed(bw, [(258, 32768), (100, 32768), ord("!")])
    text = _text(rng, 700)
    lit = complete_lengths(sorted(set(text)) + [256, 257, 260, 270, 285])
    dist = complete_lengths([0, 4, 10, 20, 29])
    toks = list(text[:350]) + [(3, 1), (6, 5), (24, DIST_BASE[10] + 3), (258, DIST_BASE[20] + 77), (3, DIST_BASE[29] + 8000)] + \
        list(text[350:])
    dynamic(bw, toks, lit, dist)
    stored(bw, _text(rng, 1100))
    stored(bw, b"")
    fixed(bw, list(b"the end") + [(7, 7), (258, 32768)], final=True)
    return bw.done()


# ------------------------------------------------------------------------------------ fuzz corpus
N_FUZZ = 600
FUZZ_SEED = 20261019


def damage(rng, blk: bytes) -> bytes:
    """the damage of tests/test_gpu_decode_fuzz.py"""
    b = bytearray(blk)
    kind = rng.randrange(6)
    if not b:
        return bytes(rng.getrandbits(8) for _ in range(rng.randint(1, 16)))
    if kind == 0:  # overwrite 1-3 bytes
        for _ in range(rng.randint(1, 3)):
            b[rng.randrange(len(b))] = rng.getrandbits(8)
    elif kind == 1:  # overwrite a byte near the start
        b[rng.randrange(min(len(b), 8))] = rng.getrandbits(8)
    elif kind == 2:  # remove a run
        a = rng.randrange(len(b))
        del b[a:a + rng.randint(1, 12)]
    elif kind == 3:  # repeat a run
        a = rng.randrange(len(b))
        b[a:a] = b[a:a + rng.randint(1, 12)]
    elif kind == 4:  # cut short
        del b[rng.randrange(len(b)):]
    else:  # junk appended
        b += bytes(rng.getrandbits(8) for _ in range(rng.randint(1, 40)))
    return bytes(b)


def _valid_stream(rng, style: int) -> bytes:
    """a raw deflate stream of 200 to 3000 bytes: zlib at level 1 / 6 / 9, or sync-flushed non-final
    blocks ending in 00 00 FF FF (the shape of this project's encoder output), with or without the
    final empty block"""
    for _ in range(64):
        payload = _text(rng, rng.randint(600, 9000)) if rng.random() < 0.7 else \
            bytes(rng.getrandbits(8) for _ in range(rng.randint(200, 2900)))
        if style < 3:
            c = zlib.compressobj((1, 6, 9)[style], zlib.DEFLATED, -15)
            z = c.compress(payload) + c.flush()
        else:
            c = zlib.compressobj(1, zlib.DEFLATED, -15)
            cut = len(payload) // 2
            z = c.compress(payload[:cut]) + c.flush(zlib.Z_SYNC_FLUSH) + c.compress(payload[cut:]) + c.flush(zlib.Z_SYNC_FLUSH)
            assert z.endswith(b"\x00\x00\xff\xff")
            if style == 4:
                z += b"\x03\x00"
        if 200 <= len(z) <= 3000:
            return z
    raise AssertionError("no stream of the wanted size")


@functools.lru_cache(maxsize=None)
def fuzz_corpus():
    """[(damaged stream, zlib's Outcome)]; one stream in six stays undamaged"""
    rng = random.Random(FUZZ_SEED)
    out = []
    for i in range(N_FUZZ):
        z = _valid_stream(rng, i % 5)
        if i % 6:
            z = damage(rng, z)
        out.append((z, reference(z)))
    return out


@functools.lru_cache(maxsize=None)
def big_text(n: int, seed: int = 7) -> bytes:
    return _text(random.Random(seed), n)
