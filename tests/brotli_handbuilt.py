"""Hand-built Brotli streams: what libbrotli's encoder cannot be made to emit, written bit by bit from RFC 7932.

VALID is [(name, stream, plain)]; the writer models the output itself (literals, copies, dictionary words under
the transforms of brotli_transforms.py), so `plain` is made by no decoder.  INVALID is [(name, stream, code name)]:
one complete stream per status code of the decoder.  The tests hold both lists against libbrotli as well.
"""
import os

from brotli_transforms import TRANSFORMS

_DICT_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "netty_amd", "csrc", "brotli_dictionary.bin")
NDBITS = [0, 0, 0, 0, 10, 10, 11, 11, 10, 10, 10, 10, 10, 9, 9, 8, 7, 7, 8, 7, 7, 6, 6, 5, 5]
DOFFSET = [0] * 26
for _i in range(25):
    DOFFSET[_i + 1] = DOFFSET[_i] + ((_i << NDBITS[_i]) if NDBITS[_i] else 0)
_dictionary = None


def dictionary() -> bytes:
    global _dictionary
    if _dictionary is None:
        with open(_DICT_PATH, "rb") as f:
            _dictionary = f.read()
    return _dictionary


def _upper(b: bytearray, i: int) -> int:
    if b[i] < 0xC0:
        if 97 <= b[i] <= 122:
            b[i] ^= 32
        return 1
    if b[i] < 0xE0:
        if i + 1 < len(b):
            b[i + 1] ^= 32
        return 2
    if i + 2 < len(b):
        b[i + 2] ^= 5
    return 3


def transform(t: int, word: bytes) -> bytes:
    pre, ty, suf = TRANSFORMS[t]
    w = bytearray(word)
    if 1 <= ty <= 9:
        w = w[:max(len(w) - ty, 0)]
    elif ty >= 12:
        w = w[ty - 11:]
    if ty == 10:
        _upper(w, 0)
    elif ty == 11:
        i = 0
        while i < len(w):
            i += _upper(w, i)
    return pre + bytes(w) + suf


class Bits:
    def __init__(self):
        self.v = 0
        self.n = 0

    def put(self, val, nbits):
        assert 0 <= val < (1 << nbits) or nbits == 0
        self.v |= val << self.n
        self.n += nbits

    def code(self, c):  # a prefix code word: its first bit first
        val, length = c
        for i in range(length - 1, -1, -1):
            self.put((val >> i) & 1, 1)

    def pad(self, fill=0):
        while self.n % 8:
            self.put(fill, 1)

    def raw(self, data):
        assert self.n % 8 == 0
        for x in data:
            self.put(x, 8)

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


def wbits(w: Bits, lg: int):
    if lg == 16:
        w.put(0, 1)
    elif lg == 17:
        w.put(1, 7)
    elif lg >= 18:
        w.put(1, 1)
        w.put(lg - 17, 3)
    else:
        w.put(1, 4)
        w.put(lg - 8, 3)


def varlen8(w: Bits, v: int):
    if v == 0:
        w.put(0, 1)
        return
    w.put(1, 1)
    n = v.bit_length() - 1
    w.put(n, 3)
    w.put(v - (1 << n), n)


def canonical(lens: dict) -> dict:
    """symbol -> (code, length); one symbol takes no bits."""
    if len(lens) == 1:
        return {s: (0, 0) for s in lens}
    out, code, prev = {}, 0, 0
    for length, s in sorted((l, s) for s, l in lens.items()):
        code <<= length - prev
        prev = length
        out[s] = (code, length)
        code += 1
    return out


def simple_code(w: Bits, abits: int, syms, shape=0) -> dict:
    w.put(1, 2)
    w.put(len(syms) - 1, 2)
    for s in syms:
        w.put(s, abits)
    n = len(syms)
    if n == 4:
        w.put(shape, 1)
    lens = {1: [0], 2: [1, 1], 3: [1, 2, 2], 4: [1, 2, 3, 3] if shape else [2, 2, 2, 2]}[n]
    if n == 1:
        return {syms[0]: (0, 0)}
    return canonical(dict(zip(syms, lens)))


_CL_ORDER = [1, 2, 3, 4, 0, 5, 17, 6, 16, 7, 8, 9, 10, 11, 12, 13, 14, 15]
_CL_CODE = {0: (0b00, 2), 4: (0b01, 2), 3: (0b10, 2), 2: (0b011, 3), 1: (0b0111, 4), 5: (0b1111, 4)}


def balanced(syms) -> dict:
    """Lengths of a complete code over syms (at least two): depth d - 1 for the first 2^d - k, d for the rest."""
    k = len(syms)
    d = max((k - 1).bit_length(), 1)
    short = (1 << d) - k
    return {s: (d - 1 if i < short else d) for i, s in enumerate(sorted(syms))}


def complex_code(w: Bits, alpha: int, lens: dict, cl_lens=None) -> dict:
    """A complex prefix code with HSKIP 0 and no repeat codes; lens: symbol -> length (others 0).  The writer stops
    where the decoder stops reading (space used up), so over- and under-subscribed codes can be written too."""
    w.put(0, 2)
    used = sorted({lens.get(s, 0) for s in range(alpha)})
    if cl_lens is None:
        cl_lens = {used[0]: 1} if len(used) == 1 else balanced(used)
    space, num = 32, 0
    for s in _CL_ORDER:
        v = cl_lens.get(s, 0)
        val, n = _CL_CODE[v]
        w.put(val, n)
        if v:
            space -= 32 >> v
            num += 1
            if space <= 0:
                break
    if not (num == 1 or space == 0):
        return {}  # CL_SPACE: the decoder stops here
    cl = canonical({s: l for s, l in cl_lens.items() if l})
    space = 32768
    for s in range(alpha):
        l = lens.get(s, 0)
        w.code(cl[l])
        if l:
            space -= 32768 >> l
        if space == 0:
            break
    return canonical({s: l for s, l in lens.items() if l})


def auto_code(w: Bits, alpha: int, syms, kind=None) -> dict:
    """A code over the used symbols: simple for up to four (kind = ('simple', shape) forces the shape), else complex."""
    syms = sorted(set(syms)) or [0]
    abits = max((alpha - 1).bit_length(), 1)
    if len(syms) <= 4 and (kind is None or kind[0] == "simple"):
        return simple_code(w, abits, syms, kind[1] if kind else 0)
    if len(syms) == 1:
        syms = syms + [syms[0] + 1 if syms[0] + 1 < alpha else 0]
    return complex_code(w, alpha, balanced(syms))


_INS_BASE = [0, 1, 2, 3, 4, 5, 6, 8, 10, 14, 18, 26, 34, 50, 66, 98, 130, 194, 322, 578, 1090, 2114, 6210, 22594]
_INS_BITS = [0, 0, 0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 7, 8, 9, 10, 12, 14, 24]
_CPY_BASE = [2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 14, 18, 22, 30, 38, 54, 70, 102, 134, 198, 326, 582, 1094, 2118]
_CPY_BITS = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 7, 8, 9, 10, 24]
_CELL = {(0, 0): 2, (0, 1): 3, (1, 0): 4, (1, 1): 5, (0, 2): 6, (2, 0): 7, (1, 2): 8, (2, 1): 9, (2, 2): 10}


def _code_of(base, v):
    return max(i for i in range(24) if base[i] <= v)


def command_symbol(ins: int, cpy: int, implicit: bool):
    ic, cc = _code_of(_INS_BASE, ins), _code_of(_CPY_BASE, cpy)
    cell = (0 if cc < 8 else 1) if implicit else _CELL[(ic >> 3, cc >> 3)]
    assert not implicit or (ic < 8 and cc < 16)
    sym = cell * 64 + ((ic & 7) << 3) + (cc & 7)
    return sym, (ins - _INS_BASE[ic], _INS_BITS[ic]), (cpy - _CPY_BASE[cc], _CPY_BITS[cc])


def direct_distance(d: int):
    """The distance symbol and extra bits of distance d at NPOSTFIX 0, NDIRECT 0."""
    v = d + 3
    nbits = v.bit_length() - 2
    prefix = (v >> nbits) & 1
    return 16 + 2 * (nbits - 1) + prefix, v - ((2 + prefix) << nbits), nbits


def _context(mode, p1, p2):
    if mode == 0:
        return p1 & 63
    if mode == 1:
        return p1 >> 2
    raise NotImplementedError


def meta_block_header(w: Bits, mlen: int, last: bool, nibbles=None):
    w.put(1 if last else 0, 1)
    if last:
        w.put(0, 1)
    n = nibbles or max(4, ((mlen - 1).bit_length() + 3) // 4)
    w.put(n - 4, 2)
    for i in range(n):
        w.put(((mlen - 1) >> (4 * i)) & 15, 4)
    if not last:
        w.put(0, 1)


def compressed(w: Bits, out: bytearray, ring: list, cmds, last: bool, lgwin=22, mode=2, two_trees=False, lit_kind=None, mlen=None):
    """One compressed meta-block of one block type per category.  cmds: dicts with lits (bytes), copy (length or
    None), and one of dist (a distance, coded directly), ring (a distance symbol 0..15), implicit (True) or word
    ((transform, index): a dictionary reference of `copy` letters).  Models the output into `out` and the ring.
    two_trees: two literal trees chosen by the context's lowest bit (modes 0 and 1 only)."""
    sim, lit_syms, cmd_syms, dist_syms, ops = bytearray(out), [set(), set()], set(), set(), []
    rg = list(ring)
    for c in cmds:
        lits, cpy = c.get("lits", b""), c.get("copy")
        tl = []
        for b in lits:
            p1, p2 = (sim[-1] if sim else 0), (sim[-2] if len(sim) > 1 else 0)
            t = (_context(mode, p1, p2) & 1) if two_trees else 0
            lit_syms[t].add(b)
            tl.append((t, b))
            sim.append(b)
        implicit = bool(c.get("implicit"))
        sym, iex, cex = command_symbol(len(lits), cpy if cpy else 2, implicit)
        cmd_syms.add(sym)
        dop = None
        if cpy:
            maxd = min(len(sim), (1 << lgwin) - 16)
            if implicit:
                d = rg[-1]
            elif "ring" in c:
                k = c["ring"]
                if k == 0:
                    d = rg[-1]
                elif k < 4:
                    d = rg[-1 - k]
                else:
                    d = rg[-1 if k < 10 else -2] + [-1, 1, -2, 2, -3, 3][(k - 4) % 6]
                dop = (k, 0, 0)
            elif "word" in c:
                t, idx = c["word"]
                d = maxd + 1 + ((t << NDBITS[cpy]) | idx)
                dop = direct_distance(d)
            else:
                d = c["dist"]
                dop = direct_distance(d)
            if dop:
                dist_syms.add(dop[0])
            if "word" in c:
                t, idx = c["word"]
                at = DOFFSET[cpy] + idx * cpy
                sim += transform(t, dictionary()[at:at + cpy])
            elif c.get("raw_copy", True) and 0 < d <= maxd:
                for _ in range(cpy):
                    sim.append(sim[-d])
                if not implicit and c.get("ring") != 0:
                    rg.append(d)
        ops.append((tl, sym, iex, cex, dop))
    meta_block_header(w, mlen if mlen is not None else len(sim) - len(out), last)
    w.put(0, 3)  # NBLTYPESL, NBLTYPESI, NBLTYPESD = 1
    w.put(0, 6)  # NPOSTFIX 0, NDIRECT 0
    w.put(mode, 2)
    if two_trees:
        varlen8(w, 1)  # NTREESL = 2
        w.put(0, 1)    # no RLE
        cm = simple_code(w, 1, [0, 1])
        for ctx in range(64):
            w.code(cm[ctx & 1])
        w.put(0, 1)    # no inverse move-to-front
    else:
        varlen8(w, 0)
    varlen8(w, 0)  # NTREESD = 1
    lit_codes = [auto_code(w, 256, lit_syms[t], lit_kind) for t in range(2 if two_trees else 1)]
    cmd_code = auto_code(w, 704, cmd_syms)
    dist_code = auto_code(w, 64, dist_syms)
    for tl, sym, iex, cex, dop in ops:
        w.code(cmd_code[sym])
        w.put(*iex)
        w.put(*cex)
        for t, b in tl:
            w.code(lit_codes[t][b])
        if dop:
            w.code(dist_code[dop[0]])
            w.put(dop[1], dop[2])
    out[:] = sim
    ring[:] = rg


def _stream(lgwin=22):
    w = Bits()
    wbits(w, lgwin)
    return w, bytearray(), [16, 15, 11, 4]


def _finish(w: Bits):
    w.pad()
    return w.bytes()


def _valid():
    v = []
    for name, mode in (("lsb6", 0), ("msb6", 1)):
        w, out, ring = _stream()
        text = b"abcabcabdabd" + bytes(range(60, 76)) + b"\x00\xff\x80\x7f"
        compressed(w, out, ring, [dict(lits=text, copy=6, dist=5), dict(lits=b"zy", copy=3, implicit=True)], False, mode=mode, two_trees=True)
        compressed(w, out, ring, [dict(lits=b"qrs", copy=4, dist=3), dict(lits=b"ab")], True, mode=mode, two_trees=True)
        v.append(("context-" + name, _finish(w), bytes(out)))
    # a metadata meta-block with a skip of 5 bytes, then a last metadata block of none would end the stream too
    w, out, ring = _stream(16)
    w.put(0, 1)      # ISLAST 0
    w.put(3, 2)      # MNIBBLES 0: metadata
    w.put(0, 1)      # reserved
    w.put(1, 2)      # MSKIPBYTES 1
    w.put(4, 8)      # MSKIPLEN - 1
    w.pad()
    w.raw(b"\xffskip")
    compressed(w, out, ring, [dict(lits=b"after metadata")], True, lgwin=16)
    v.append(("metadata-skip", _finish(w), bytes(out)))
    # simple codes of 1, 2, 3 and 4 symbols, both four-symbol shapes, one meta-block each
    w, out, ring = _stream(10)
    sets = [(b"aaaa", None), (b"abab", None), (b"abcabc", None), (b"abcdabcd", ("simple", 0)), (b"dcbaabcd", ("simple", 1))]
    for i, (t, kind) in enumerate(sets):
        compressed(w, out, ring, [dict(lits=t, copy=2, dist=1)], i == len(sets) - 1, lgwin=10, lit_kind=kind)
    v.append(("simple-codes", _finish(w), bytes(out)))
    # every transform, on words of every length
    w, out, ring = _stream()
    cmds = [dict(copy=4 + t % 21, word=(t, (37 * t + 5) % (1 << NDBITS[4 + t % 21]))) for t in range(121)]
    cmds += [dict(lits=b" ", copy=n, word=(44, 3)) for n in range(4, 25)]
    compressed(w, out, ring, cmds, True)
    v.append(("all-transforms", _finish(w), bytes(out)))
    # every distance symbol of the ring
    w, out, ring = _stream()
    cmds = [dict(lits=bytes(range(48, 48 + 40)))]
    for k in range(16):
        cmds += [dict(lits=b"x", copy=2, dist=20), dict(lits=b"y", copy=3, dist=24), dict(lits=b"z", copy=2 + k % 4, ring=k)]
    cmds[0]["copy"] = 2
    cmds[0]["dist"] = 7
    compressed(w, out, ring, cmds, True)
    v.append(("ring-codes", _finish(w), bytes(out)))
    return v


def _to_first_code(w: Bits, mlen=4):
    """A last compressed meta-block up to its first prefix code (the literal tree): one block type, one tree."""
    meta_block_header(w, mlen, True)
    w.put(0, 3)
    w.put(0, 6)
    w.put(2, 2)
    varlen8(w, 0)
    varlen8(w, 0)


def _invalid():
    bad = []

    def add(name, code, w, tail=8):
        w.pad()
        bad.append((name, w.bytes() + bytes(tail), code))  # zero bytes behind, so nothing ends the input early

    w, _, _ = _stream()
    w.put(0, 1)
    w.put(1, 2)  # five nibbles
    for nib in (1, 0, 0, 0, 0):
        w.put(nib, 4)
    add("exuberant-nibble", "EXUBERANT_NIBBLE", w)
    w, _, _ = _stream()
    w.put(0, 1)
    w.put(3, 2)
    w.put(1, 1)
    add("reserved-bit", "RESERVED", w)
    w, _, _ = _stream()
    w.put(0, 1)
    w.put(3, 2)
    w.put(0, 1)
    w.put(2, 2)
    w.put(5, 8)
    w.put(0, 8)
    add("exuberant-meta-nibble", "EXUBERANT_META_NIBBLE", w)
    w, _, _ = _stream()
    _to_first_code(w)
    simple_code(w, 8, [65])
    w.put(1, 2)
    w.put(0, 2)
    w.put(1000, 10)  # a command symbol above 703
    add("simple-alphabet", "SIMPLE_HUFFMAN_ALPHABET", w)
    w, _, _ = _stream()
    _to_first_code(w)
    w.put(1, 2)
    w.put(1, 2)
    w.put(65, 8)
    w.put(65, 8)
    add("simple-same", "SIMPLE_HUFFMAN_SAME", w)
    w, _, _ = _stream()
    _to_first_code(w)
    complex_code(w, 256, {65: 1, 66: 1}, cl_lens={1: 1, 2: 2, 3: 1})
    add("cl-space-over", "CL_SPACE", w)
    w, _, _ = _stream()
    _to_first_code(w)
    complex_code(w, 256, {65: 1, 66: 1}, cl_lens={1: 2, 2: 2})
    add("cl-space-under", "CL_SPACE", w)
    w, _, _ = _stream()
    _to_first_code(w)
    w.put(0, 2)
    for v_ in (1, 2, 2):  # code lengths 1, 2 and 3 of the code-length code; the rest 0
        w.put(*_CL_CODE[v_])
    cl = canonical({1: 1, 2: 2, 3: 2})
    for l in (1, 2, 1) + (3,) * 253:  # 1/2 + 1/4 + 1/2: over-subscribed; the decoder reads on to the alphabet's end
        w.code(cl[l])
    add("huffman-space-over", "HUFFMAN_SPACE", w)
    w2, _, _ = _stream()
    _to_first_code(w2)
    w2.put(0, 2)
    w2.put(*_CL_CODE[1])  # symbol 1: length 1
    w2.put(*_CL_CODE[0])  # 2
    w2.put(*_CL_CODE[0])  # 3
    w2.put(*_CL_CODE[0])  # 4
    w2.put(*_CL_CODE[1])  # symbol 0: length 1: complete
    cl2 = canonical({1: 1, 0: 1})
    for l in (1,) + (0,) * 255:  # one code of length 1 and nothing else: under-subscribed
        w2.code(cl2[l])
    add("huffman-space-under", "HUFFMAN_SPACE", w2)
    w, _, _ = _stream()
    meta_block_header(w, 4, True)
    w.put(0, 3)
    w.put(0, 6)
    w.put(2, 2)
    varlen8(w, 1)  # NTREESL = 2
    w.put(1, 1)
    w.put(5, 4)    # RLEMAX 6
    simple_code(w, 3, [6])
    w.put(1, 6)    # 64 + 1 zeros in a map of 64
    add("context-map-repeat", "CONTEXT_MAP_REPEAT", w)
    w, out, ring = _stream()
    compressed(w, out, ring, [dict(lits=b"abcdef")], True, mlen=4)
    add("insert-past-mlen", "BLOCK_LENGTH_2", w)
    w, out, ring = _stream()
    compressed(w, out, ring, [dict(lits=b"ab", copy=8, dist=1)], True, mlen=5)
    add("copy-past-mlen", "BLOCK_LENGTH_2", w)
    # An over-run whose bytes reach the end of libbrotli's ring buffer is BLOCK_LENGTH_1.  The ring is the window,
    # halved while the half holds the position plus MLEN, 1024 at least: 1024 bytes here, 65536 in the third.
    a = b"a"
    w, out, ring = _stream(10)
    compressed(w, out, ring, [dict(lits=a * 1040)], True, lgwin=10, mlen=1030)
    add("insert-reaches-ring-end", "BLOCK_LENGTH_1", w)
    w, out, ring = _stream(10)
    compressed(w, out, ring, [dict(lits=a * 1020, copy=20, dist=1)], True, lgwin=10, mlen=1030)
    add("copy-reaches-ring-end", "BLOCK_LENGTH_1", w)
    w, out, ring = _stream(16)
    compressed(w, out, ring, [dict(lits=a * 65520, copy=40, dist=1)], True, lgwin=16, mlen=65530)
    add("copy-reaches-ring-end-64k", "BLOCK_LENGTH_1", w)
    w, out, ring = _stream(10)
    compressed(w, out, ring, [dict(lits=a * 1020, copy=4, word=(0, 7))], True, lgwin=10, mlen=1022)
    add("word-reaches-ring-end", "BLOCK_LENGTH_1", w)
    w, out, ring = _stream(22)  # the ring stays at 1024 after a first meta-block of 1000 bytes
    compressed(w, out, ring, [dict(lits=a * 1000)], False)
    compressed(w, out, ring, [dict(lits=a * 30)], True, mlen=20)
    add("insert-reaches-ring-end-second-block", "BLOCK_LENGTH_1", w)
    w, out, ring = _stream(22)
    compressed(w, out, ring, [dict(lits=a * 1000)], False)
    compressed(w, out, ring, [dict(lits=a * 23)], True, mlen=20)
    add("insert-short-of-ring-end-second-block", "BLOCK_LENGTH_2", w)
    w, out, ring = _stream(10)  # the ring at the window's size wraps: 2649 + 444 literals stand at 21, and 21 + 799 < 1024
    for n in (821, 1422, 406):
        compressed(w, out, ring, [dict(lits=a * n)], False, lgwin=10)
    compressed(w, out, ring, [dict(lits=a * 444, copy=799, dist=1)], True, lgwin=10, mlen=845)
    add("copy-past-mlen-after-wrap", "BLOCK_LENGTH_2", w)
    w, out, ring = _stream()
    compressed(w, out, ring, [dict(lits=b"a", copy=4, dist=1 + 1 + (121 << 10), raw_copy=False)], True, mlen=9)
    add("transform-121", "TRANSFORM", w)
    for n in (3, 25):
        w, out, ring = _stream()
        compressed(w, out, ring, [dict(lits=b"a", copy=n, dist=100, raw_copy=False)], True, mlen=1 + n)
        add("dictionary-length-%d" % n, "DICTIONARY", w)
    w = Bits()
    w.put(0x11, 7)
    add("large-window", "WINDOW_BITS", w)
    w, _, _ = _stream(16)
    w.put(0, 1)
    w.put(0, 2)
    for nib in (3, 0, 0, 0):
        w.put(nib, 4)
    w.put(1, 1)  # ISUNCOMPRESSED
    assert w.n % 8
    w.pad(1)
    w.raw(b"abcd")
    w.put(3, 2)
    add("padding-uncompressed", "PADDING_1", w)
    w, _, _ = _stream()
    w.put(0, 1)
    w.put(3, 2)
    w.put(0, 1)
    w.put(0, 2)
    w.pad(1)
    w.put(3, 2)
    add("padding-metadata", "PADDING_1", w)
    w, out, ring = _stream()
    compressed(w, out, ring, [dict(lits=b"abc")], True)
    assert w.n % 8
    w.pad(1)
    add("padding-end", "PADDING_2", w, tail=0)
    w, out, ring = _stream()
    compressed(w, out, ring, [dict(lits=b"abcd", copy=2, ring=8), dict(lits=b"e", copy=2, ring=4, raw_copy=False)], True, mlen=11)
    add("distance-zero", "DISTANCE", w)
    return bad


VALID = _valid()
INVALID = _invalid()
