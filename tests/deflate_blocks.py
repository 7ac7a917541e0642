"""A plain RFC 1951 block reader and three small cost references, for the tests of the deflate
encoder (tests/test_gpu_deflate_structure.py).  Pure Python, no project code: tests/test_deflate_blocks.py
pins it to the real zlib's output on the CPU.

`read_blocks(raw)` walks a raw deflate stream and returns one `Block` per block, raising `DeflateError`
on anything the RFC forbids; `replay(blocks)` returns the bytes the blocks stand for.  A stream need not
end in a final block: reading stops after a block with BFINAL set, or at the end of `raw` when that is
where a block ends (a sync-flushed piece ends in an empty stored block, on a byte boundary).

`huffman_cost`, `limited_cost`, `fixed_cost` and `stored_cost` are the yardsticks the structure tests
hold the encoder's codes and block choice to."""
import heapq
from collections import namedtuple
from dataclasses import dataclass, field


class DeflateError(ValueError):
    pass


LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT_LENS = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST_LENS = [5] * 32


@dataclass
class Block:
    bfinal: int
    btype: int
    start: int                     # bit offset of the BFINAL bit
    end: int = 0                   # bit offset after the block's last bit (a stored block's last byte)
    len: int = None                # stored: LEN
    payload: bytes = None          # stored: the bytes
    tokens: list = None            # Huffman: ("lit", b) / ("match", length, distance), without the end of block
    hlit: int = None               # dynamic: counts as sent (HLIT + 257, HDIST + 1, HCLEN + 4)
    hdist: int = None
    hclen: int = None
    cl_lens: list = None           # dynamic: the 19 code-length-code lengths, by symbol
    lit_lens: list = None          # dynamic: the hlit literal/length code lengths
    dist_lens: list = None         # dynamic: the hdist distance code lengths
    repeats: set = field(default_factory=set)  # dynamic: which of 16, 17, 18 occurred in the header
    header_bits: int = None        # Huffman: the 3 block bits (and a dynamic block's code description)
    symbol_bits: int = None        # Huffman: the tokens and the end of block

    @property
    def bits(self):
        return self.end - self.start


def kraft(lens):
    """(sum of 2^-len over the non-zero lengths, as an integer count of 2^-maxlen units), 2^maxlen"""
    used = [l for l in lens if l]
    if not used:
        return 0, 1
    m = max(used)
    return sum(1 << (m - l) for l in used), 1 << m


def _decode_table(lens, what, one_bit_ok=False, empty_ok=False):
    """(table indexed by the next maxlen stream bits -> (symbol, length) or None, maxlen) of the canonical
    code of RFC 1951 section 3.2.2; raises unless the code is complete"""
    total, unit = kraft(lens)
    if total == 0:
        if empty_ok:
            return [None], 0
        raise DeflateError(f"{what}: no code at all")
    if total > unit:
        raise DeflateError(f"{what}: over-subscribed code")
    if total < unit and not (one_bit_ok and [l for l in lens if l] == [1]):
        raise DeflateError(f"{what}: incomplete code")
    maxlen = max(lens)
    count = [0] * (maxlen + 2)
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * (maxlen + 2), 0
    for b in range(1, maxlen + 1):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    table = [None] * (1 << maxlen)
    for sym, l in enumerate(lens):
        if not l:
            continue
        c = nxt[l]
        nxt[l] += 1
        r = int(format(c, f"0{l}b")[::-1], 2)  # Huffman codes go out most significant bit first
        for k in range(r, 1 << maxlen, 1 << l):
            table[k] = (sym, l)
    return table, maxlen


class _Bits:
    def __init__(self, raw):
        self.raw = raw
        self.nbits = 8 * len(raw)
        self.pos = 0
        self._base = 0   # a window of the stream as a small integer: shifts of the whole stream would
        self._win = 0    # cost its length each
        self._wbits = 0

    def _refill(self, pos):
        b = pos >> 3
        chunk = self.raw[b:b + 512]
        self._base = 8 * b
        self._win = int.from_bytes(chunk, "little")
        self._wbits = 8 * len(chunk)

    def peek(self, n):
        """the next n bits, least significant first; bits past the end read as zero"""
        p = self.pos - self._base
        if p < 0 or p + n > self._wbits:
            self._refill(self.pos)
            p = self.pos - self._base
        return (self._win >> p) & ((1 << n) - 1)

    def skip(self, n):
        self.pos += n
        if self.pos > self.nbits:
            raise DeflateError("the stream ends inside a block")

    def take(self, n):
        v = self.peek(n)
        self.skip(n)
        return v

    def symbol(self, table, maxlen, what):
        e = table[self.peek(maxlen)]
        if e is None:
            raise DeflateError(f"{what}: bits that are no code")
        self.skip(e[1])
        return e[0]


def _read_dynamic_header(bits, blk):
    blk.hlit, blk.hdist, blk.hclen = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
    if blk.hlit > 286:
        raise DeflateError(f"HLIT of {blk.hlit} codes")
    if blk.hdist > 30:
        raise DeflateError(f"HDIST of {blk.hdist} codes")
    blk.cl_lens = [0] * 19
    for i in range(blk.hclen):
        blk.cl_lens[CL_ORDER[i]] = bits.take(3)
    table, maxlen = _decode_table(blk.cl_lens, "code-length code")
    lens, want = [], blk.hlit + blk.hdist
    while len(lens) < want:
        s = bits.symbol(table, maxlen, "code-length code")
        if s < 16:
            lens.append(s)
            continue
        blk.repeats.add(s)
        if s == 16:
            if not lens:
                raise DeflateError("repeat of a previous length that does not exist")
            lens += [lens[-1]] * (3 + bits.take(2))
        elif s == 17:
            lens += [0] * (3 + bits.take(3))
        else:
            lens += [0] * (11 + bits.take(7))
        if len(lens) > want:
            raise DeflateError("a repeat runs past the last code length")
    blk.lit_lens, blk.dist_lens = lens[:blk.hlit], lens[blk.hlit:]
    if blk.lit_lens[256] == 0:
        raise DeflateError("no code for the end of block")


def read_blocks(raw):
    bits, blocks, produced = _Bits(bytes(raw)), [], 0
    while True:
        blk = Block(bfinal=0, btype=0, start=bits.pos)
        blk.bfinal, blk.btype = bits.take(1), bits.take(2)
        if blk.btype == 3:
            raise DeflateError("block type 3")
        if blk.btype == 0:
            bits.skip(-bits.pos % 8)
            blk.len, nlen = bits.take(16), bits.take(16)
            if blk.len ^ nlen != 0xFFFF:
                raise DeflateError(f"LEN {blk.len:#x} against NLEN {nlen:#x}")
            b = bits.pos >> 3
            bits.skip(8 * blk.len)
            blk.payload = bits.raw[b:b + blk.len]
            produced += blk.len
        else:
            if blk.btype == 2:
                _read_dynamic_header(bits, blk)
                lit_lens, dist_lens = blk.lit_lens, blk.dist_lens
            else:
                lit_lens, dist_lens = FIXED_LIT_LENS, FIXED_DIST_LENS
            lt, lmax = _decode_table(lit_lens, "literal/length code")
            dt, dmax = _decode_table(dist_lens, "distance code", one_bit_ok=True, empty_ok=True)
            blk.header_bits = bits.pos - blk.start
            blk.tokens = toks = []
            while True:
                s = bits.symbol(lt, lmax, "literal/length code")
                if s < 256:
                    toks.append(("lit", s))
                    produced += 1
                elif s == 256:
                    break
                elif s > 285:
                    raise DeflateError(f"length symbol {s}")
                else:
                    length = LEN_BASE[s - 257] + bits.take(LEN_EXTRA[s - 257])
                    if dmax == 0:
                        raise DeflateError("a match in a block without distance codes")
                    d = bits.symbol(dt, dmax, "distance code")
                    if d > 29:
                        raise DeflateError(f"distance symbol {d}")
                    dist = DIST_BASE[d] + bits.take(DIST_EXTRA[d])
                    if dist > produced:
                        raise DeflateError(f"distance {dist} with {produced} bytes before it")
                    toks.append(("match", length, dist))
                    produced += length
            blk.symbol_bits = bits.pos - blk.start - blk.header_bits
        blk.end = bits.pos
        blocks.append(blk)
        if blk.bfinal or bits.pos == bits.nbits:
            return blocks


def replay(blocks):
    out = bytearray()
    for blk in blocks:
        if blk.btype == 0:
            out += blk.payload
            continue
        for t in blk.tokens:
            if t[0] == "lit":
                out.append(t[1])
            else:
                _, length, dist = t
                if dist > len(out):
                    raise DeflateError(f"distance {dist} with {len(out)} bytes before it")
                if dist >= length:
                    out += out[len(out) - dist:len(out) - dist + length]
                else:
                    for _ in range(length):
                        out.append(out[-dist])
    return bytes(out)


# ------------------------------------------------------------------------------------- symbols
def length_symbol(length):
    """(literal/length symbol 257..285, extra bits) of a match length 3..258"""
    for c in range(28, -1, -1):
        if length >= LEN_BASE[c]:
            return 257 + c, LEN_EXTRA[c]


def distance_symbol(dist):
    """(distance symbol 0..29, extra bits) of a distance 1..32768"""
    for c in range(29, -1, -1):
        if dist >= DIST_BASE[c]:
            return c, DIST_EXTRA[c]


def token_frequencies(tokens):
    """(286 literal/length frequencies with the end of block counted once, 30 distance frequencies)"""
    lf, df = [0] * 286, [0] * 30
    lf[256] = 1
    for t in tokens:
        if t[0] == "lit":
            lf[t[1]] += 1
        else:
            lf[length_symbol(t[1])[0]] += 1
            df[distance_symbol(t[2])[0]] += 1
    return lf, df


# ---------------------------------------------------------------------------------------- costs
HuffmanCost = namedtuple("HuffmanCost", "cost depth")


def huffman_cost(freqs):
    """The optimal prefix code's cost sum(f * len) over the non-zero frequencies, and the depth of the
    tree the textbook construction builds (repeatedly join the two lightest; among equal weights the
    shallower).  Fewer than two symbols cost nothing at depth 0."""
    heap = [(f, 0) for f in freqs if f]
    heapq.heapify(heap)
    cost = 0
    while len(heap) > 1:
        f0, d0 = heapq.heappop(heap)
        f1, d1 = heapq.heappop(heap)
        cost += f0 + f1
        heapq.heappush(heap, (f0 + f1, max(d0, d1) + 1))
    return HuffmanCost(cost, heap[0][1] if heap else 0)


def limited_cost(freqs, maxbits):
    """The least sum(f * len) of a prefix code with no length over maxbits, by package-merge (Larmore
    and Hirschberg): a code's cost is the total weight of the 2n - 2 lightest items of the last of
    maxbits lists, each the leaves merged with the pairs of the list before."""
    leaves = sorted(f for f in freqs if f)
    n = len(leaves)
    if n < 2:
        return 0
    if n > 1 << maxbits:
        raise ValueError(f"{n} symbols do not fit {maxbits} bits")
    items = leaves
    for _ in range(maxbits - 1):
        packages = [items[i] + items[i + 1] for i in range(0, len(items) - 1, 2)]
        items = sorted(leaves + packages)
    return sum(items[:2 * n - 2])


def fixed_cost(tokens):
    """Bits of the tokens and the end of block under the fixed code (RFC 1951 section 3.2.6), without
    the 3 block bits."""
    bits = 7
    for t in tokens:
        if t[0] == "lit":
            bits += FIXED_LIT_LENS[t[1]]
        else:
            s, x = length_symbol(t[1])
            bits += FIXED_LIT_LENS[s] + x + 5 + distance_symbol(t[2])[1]
    return bits


def stored_cost(n):
    """Bits of n bytes in stored blocks of at most 65535 (section 3.2.4), counted from a byte boundary."""
    return 8 * (n + 5 * -(-n // 65535))
