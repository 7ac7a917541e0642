"""A bzip2 stream writer that takes every field explicitly, and a plain reference decoder of the same format.

The writer emits what it is told: the level, and per block the start pointer, the symbol-use set, the table
count, the selector list, each table's code lengths (with detours in their delta coding), the symbol
sequence as symbols (RUNA, RUNB, move-to-front indices + 1, the end-of-block symbol, or raw bits) and the
stored CRC.  Nothing is derived from data unless the caller asks the convenience layer for it (symbols of a
BWT column, the column of a text by a naive rotation sort, CRCs filled in from the model).

The decoder is the model the hand-built cases get their expectations from.  It is written from the format and
from Bzip2Decoder.java, Bzip2BlockDecompressor.java and Bzip2HuffmanStageDecoder.java: an ordinary tt array,
a serial walk, Java `int` arithmetic made explicit with masks.  Where the Java would throw an unchecked
array-index exception the model gives the status the decoder's header names for it; where the Java waits for
more input the model answers TRUNCATED: missing bits read as zeros, and any verdict reached after a bit past
the end was consumed is TRUNCATED.  No project imports."""
from dataclasses import dataclass

from bzip2_encode_inputs import bzip2_crc, combined_crc

OK = 0
(STREAM_ID, BLOCK_SIZE, STREAM_CRC, BLOCK_HEADER, HUFFMAN_GROUPS, ALPHABET, SELECTORS, DECODING_BLOCK, CODE, BLOCK_EXCEEDS,
 START_POINTER, BLOCK_CRC, TRUNCATED, OUTPUT_FULL, RANDOMISED) = range(-110, -125, -1)
BLOCK_MAGIC, END_MAGIC = 0x314159265359, 0x177245385090
RUNA, RUNB = 0, 1
MAX_LEN = 23          # HUFFMAN_DECODE_MAX_CODE_LENGTH
MAX_ALPHA = 258       # HUFFMAN_MAX_ALPHABET_SIZE
MAX_SELECTORS = 18002
GROUP = 50            # HUFFMAN_GROUP_RUN_LENGTH
M32 = 0xFFFFFFFF


def s32(x: int) -> int:
    """x as a Java int."""
    x &= M32
    return x - (1 << 32) if x & 0x80000000 else x


# ------------------------------------------------------------------ canonical codes, the Java's construction
def code_tables(lens):
    """(minimum, limit, base, symbols) as createHuffmanDecodingTables builds them
    (Bzip2HuffmanStageDecoder.java:126-163), for any lengths in 1..23, complete or not: `code` runs on as a
    Java int, so an over-subscribed set wraps where the Java wraps."""
    mn, mx = min(lens), max(lens)
    cum = [0] * (MAX_LEN + 3)  # cum[i]: symbols with a length below i
    for ln in lens:
        cum[ln + 1] += 1
    for i in range(1, MAX_LEN + 3):
        cum[i] += cum[i - 1]
    limit, base = [0] * (MAX_LEN + 1), cum[:MAX_LEN + 2]
    code = 0
    for i in range(mn, mx + 1):
        first = code
        code = s32(code + cum[i + 1] - cum[i])
        base[i] = s32(first - cum[i])
        limit[i] = s32(code - 1)
        code = s32(code << 1)
    syms = [s for bl in range(mn, mx + 1) for s in range(len(lens)) if lens[s] == bl]
    return mn, limit, base, syms + [0] * (MAX_ALPHA - len(syms))


def symbol_codes(lens):
    """[(code, length)] per symbol: the first code of a length is the `base` of the loop at
    Bzip2HuffmanStageDecoder.java:148-154 (the value before tableBases[i] is subtracted), the codes of one
    length follow in symbol order.  For a complete or incomplete set these are the canonical codes; for an
    over-subscribed one the low `length` bits are what a writer can send, and the model says what they mean."""
    mn, limit, base, _ = code_tables(lens)
    rank, out = {}, []
    cum = {bl: sum(1 for x in lens if x < bl) for bl in set(lens)}
    for ln in lens:
        k = rank.get(ln, 0)
        rank[ln] = k + 1
        out.append(((base[ln] + cum[ln] + k) & ((1 << ln) - 1), ln))
    return out


# ------------------------------------------------------------------ writer
class BitWriter:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, value: int, bits: int):
        self.acc = (self.acc << bits) | (value & ((1 << bits) - 1))
        self.n += bits
        while self.n >= 8:
            self.n -= 8
            self.out.append((self.acc >> self.n) & 0xFF)
        self.acc &= (1 << self.n) - 1

    @property
    def bit_length(self):
        return len(self.out) * 8 + self.n

    def finish(self, pad_ones=False) -> bytes:
        if self.n:
            k = 8 - self.n
            self.put((1 << k) - 1 if pad_ones else 0, k)
        return bytes(self.out)


@dataclass
class BlockSpec:
    """One block, field by field.  selectors: table numbers, any count (the count field is their number);
    selector_mtf, when given, is the list of unary move-to-front indices sent instead.  lengths: per table a
    list with one item per alphabet entry, an int or a sequence of waypoints the delta coding walks through
    one step at a time before it settles on the last; a table may be (first, items) to set the 5-bit start
    value apart.  symbols: ints, or (value, bits) for raw bits in place of a code."""
    start: int
    used: list
    ntables: int
    selectors: list
    lengths: list
    symbols: list
    crc: int = 0
    randomised: int = 0
    selector_mtf: list = None
    magic: int = BLOCK_MAGIC


def _final_lengths(table):
    items = table[1] if isinstance(table, tuple) else table
    return [it if isinstance(it, int) else it[-1] for it in items]


def write_block(w: BitWriter, b: BlockSpec):
    w.put(b.magic, 48)
    w.put(b.crc, 32)
    w.put(b.randomised, 1)
    w.put(b.start, 24)
    used = set(b.used)
    rows = [sum(0x8000 >> j for j in range(16) if i * 16 + j in used) for i in range(16)]
    w.put(sum(0x8000 >> i for i in range(16) if rows[i]), 16)
    for m in rows:
        if m:
            w.put(m, 16)
    w.put(b.ntables, 3)
    if b.selector_mtf is not None:
        idxs = list(b.selector_mtf)
    else:
        order, idxs = list(range(6)), []
        for t in b.selectors:
            k = order.index(t)
            idxs.append(k)
            order.insert(0, order.pop(k))
    w.put(len(idxs), 15)
    for k in idxs:
        w.put((1 << (k + 1)) - 2, k + 1)  # k ones and a zero
    for table in b.lengths:
        first, items = table if isinstance(table, tuple) else (None, table)
        cur = None
        for it in items:
            way = [it] if isinstance(it, int) else list(it)
            if cur is None:
                cur = way[0] if first is None else first
                w.put(cur, 5)
            for target in way:
                while cur != target:
                    w.put(0b11 if target < cur else 0b10, 2)
                    cur += -1 if target < cur else 1
            w.put(0, 1)
    finals = [_final_lengths(t) for t in b.lengths]
    if any(not 1 <= ln <= MAX_LEN for f in finals for ln in f):
        return  # the decoder stops at the lengths
    codes = [symbol_codes(f) for f in finals]
    sel = list(b.selectors)
    pos = 0
    for s in b.symbols:
        if isinstance(s, tuple):
            w.put(*s)
            pos += 1  # raw bits stand for one symbol of their group
            continue
        t = sel[min(pos // GROUP, len(sel) - 1)] if sel else 0
        w.put(*codes[min(t, len(codes) - 1)][s])
        pos += 1


def write_stream(level, blocks, *, stream_crc=None, pad_ones=False, tail=b"", end=True, positions=None) -> bytes:
    """"BZh", the level character, the blocks, the end magic with the combined CRC of the blocks' stored CRCs
    (or stream_crc), padding, tail.  positions, a list, receives the bit position of every block magic."""
    w = BitWriter()
    for ch in b"BZh" + (level if isinstance(level, bytes) else str(level).encode()):
        w.put(ch, 8)
    for b in blocks:
        if positions is not None:
            positions.append(w.bit_length)
        write_block(w, b)
    if end:
        w.put(END_MAGIC, 48)
        w.put(combined_crc([b.crc for b in blocks]) if stream_crc is None else stream_crc, 32)
    return w.finish(pad_ones) + tail


# ------------------------------------------------------------------ convenience layer
def run_digits(n: int):
    """The run symbols that spell n >= 1: bijective base two, least significant digit first."""
    out = []
    while n > 0:
        if n & 1:
            out.append(RUNA)
            n = (n - 1) >> 1
        else:
            out.append(RUNB)
            n = (n - 2) >> 1
    return out


def column_symbols(column: bytes, used=None):
    """(used, symbols) of a BWT column: move-to-front indices over the sorted values in use, zero runs as run
    symbols, the end-of-block symbol last."""
    used = sorted(set(column)) if used is None else list(used)
    order, out, run = list(used), [], 0
    for v in column:
        k = order.index(v)
        if k == 0:
            run += 1
            continue
        out += run_digits(run)
        run = 0
        out.append(k + 1)
        order.insert(0, order.pop(k))
    out += run_digits(run)
    out.append(len(used) + 1)
    return used, out


def flat_lengths(alpha: int):
    """A complete code over alpha >= 2 symbols with lengths that differ by at most one."""
    top = max(1, (alpha - 1).bit_length())
    short = (1 << top) - alpha
    return [top - 1] * short + [top] * (alpha - short) if top > 1 else [1] * alpha


def groups_of(symbols) -> int:
    return max(1, -(-len(symbols) // GROUP))


def column_block(column: bytes, start: int, **over) -> BlockSpec:
    used, symbols = column_symbols(column, over.pop("used", None))
    symbols = over.pop("symbols", symbols)
    spec = dict(start=start, used=used, ntables=2, selectors=[0] * groups_of(symbols), lengths=[flat_lengths(len(used) + 2)] * 2,
                symbols=symbols)
    spec.update(over)
    if "lengths" not in over and spec["ntables"] != 2:
        spec["lengths"] = [flat_lengths(len(used) + 2)] * spec["ntables"]
    return BlockSpec(**spec)


def bwt(text: bytes):
    """(column, start pointer) of text by a naive sort of its rotations (ties by position)."""
    n, dd = len(text), text + text
    rot = sorted(range(n), key=lambda i: dd[i:i + n])
    return bytes(dd[i + n - 1] for i in rot), rot.index(0)


def rle1(data: bytes) -> bytes:
    """bzip2's first run-length stage: four equal bytes and a count of up to 251 more."""
    out, i = bytearray(), 0
    while i < len(data):
        j = i
        while j < len(data) and data[j] == data[i] and j - i < 255:
            j += 1
        out += data[i:i + min(j - i, 4)]
        if j - i >= 4:
            out.append(j - i - 4)
        i = j
    return bytes(out)


def text_block(pre: bytes, **over) -> BlockSpec:
    """The block whose inverse BWT spells pre (the bytes before the final run-length stage)."""
    column, start = bwt(pre)
    return column_block(column, over.pop("start", start), **over)


def seal(level, blocks, **kw) -> bytes:
    """write_stream after every block's stored CRC has been set to what the model computes for it."""
    trace = []
    decode(write_stream(level, blocks), 1 << 30, check_crc=False, trace=trace)
    for b, c in zip(blocks, trace):
        b.crc = c
    return write_stream(level, blocks, **kw)


def cycles(column: bytes):
    """The cycles of j -> tt[j] >> 8 for this column, as lists of tt positions in walk order."""
    ptr = sorted(range(len(column)), key=column.__getitem__)
    seen, out = [False] * len(column), []
    for s in range(len(column)):
        if seen[s]:
            continue
        cyc, j = [], s
        while not seen[j]:
            seen[j] = True
            cyc.append(j)
            j = ptr[j]
        out.append(cyc)
    return out


# ------------------------------------------------------------------ model decoder
class _Fail(Exception):
    def __init__(self, code):
        self.code = code


class _Bits:
    def __init__(self, data: bytes, pos: int):
        self.d, self.end, self.pos = data, len(data) * 8, pos

    def peek(self, k: int) -> int:  # k <= 32; zeros past the end
        at = self.pos >> 3
        v = int.from_bytes(self.d[at:at + 5].ljust(5, b"\0"), "big")
        return (v >> (40 - (self.pos & 7) - k)) & ((1 << k) - 1)

    def read(self, k: int) -> int:
        v = self.peek(k)
        self.pos += k
        return v

    @property
    def over(self) -> bool:
        return self.pos > self.end

    def need(self):
        if self.over:
            raise _Fail(TRUNCATED)


def _block(r: _Bits, block_size: int):
    # Bzip2Decoder.java:147-290
    randomised, start, in16 = r.read(1), r.read(24), r.read(16)
    r.need()
    if randomised:
        raise _Fail(RANDOMISED)  # the decoder under test carries no randomisation table
    symmap = []
    for i in range(16):
        if in16 & (0x8000 >> i):
            m = r.read(16)
            symmap += [i * 16 + j for j in range(16) if m & (0x8000 >> j)]
    nsym = len(symmap)
    symmap += [0] * (256 - nsym)  # huffmanSymbolMap is a fresh array per block
    eob, alpha = nsym + 1, nsym + 2
    ntables = r.read(3)
    r.need()
    if not 2 <= ntables <= 6:
        raise _Fail(HUFFMAN_GROUPS)
    nsel = r.read(15)
    r.need()
    if not 1 <= nsel <= MAX_SELECTORS:
        raise _Fail(SELECTORS)
    order, sels = list(range(6)), []
    for _ in range(nsel):
        k = 0
        while k < ntables and r.read(1):
            k += 1
        r.need()
        if k >= ntables:  # Java: an index into arrays of ntables rows
            raise _Fail(DECODING_BLOCK)
        order.insert(0, order.pop(k))
        sels.append(order[0])
    tables = []
    for _ in range(ntables):
        ln, lens = r.read(5), []
        for _ in range(alpha):
            while True:
                r.need()
                if not 1 <= ln <= MAX_LEN:  # Java: stored unchecked, an array index later
                    raise _Fail(CODE)
                if not r.read(1):
                    break
                ln += -1 if r.read(1) else 1
            lens.append(ln)
        r.need()
        tables.append(code_tables(lens))
    # Bzip2BlockDecompressor.decodeHuffmanData with Bzip2HuffmanStageDecoder.nextSymbol
    mtf, bwt_col = list(range(256)), bytearray()
    rc, ri, mv, gpos, gidx = 0, 1, 0, -1, -1  # rc, ri: Java ints
    while True:
        gpos += 1
        if gpos % GROUP == 0:
            gidx += 1
            if gidx == nsel:
                raise _Fail(DECODING_BLOCK)
            mn, limit, base, syms = tables[sels[gidx]]
        w = r.peek(MAX_LEN)
        for ln in range(mn, MAX_LEN + 1):
            code = w >> (MAX_LEN - ln)
            if code <= limit[ln]:
                r.pos += ln
                r.need()
                idx = code - base[ln]
                if not 0 <= idx < MAX_ALPHA:  # Java: tableSymbols[idx] out of range
                    raise _Fail(CODE)
                sym = syms[idx]
                break
        else:
            r.pos += MAX_LEN + 1  # the loop reads one more bit before it gives up
            r.need()
            raise _Fail(CODE)
        if sym == RUNA:
            rc, ri = s32(rc + ri), s32(ri << 1)
        elif sym == RUNB:
            rc, ri = s32(rc + (ri << 1)), s32(ri << 1)
        else:
            if rc > 0:
                # (Java adds two ints here; a sum past 2^31 would wrap and the copy loop leave the array:
                # an unchecked exception, for which the declared-size error stands)
                if len(bwt_col) + rc > block_size:
                    raise _Fail(BLOCK_EXCEEDS)
                bwt_col += bytes([symmap[mv]]) * rc
                rc, ri = 0, 1
            if sym == eob:
                break
            if len(bwt_col) >= block_size:
                raise _Fail(BLOCK_EXCEEDS)
            mv = mtf.pop(sym - 1)
            mtf.insert(0, mv)
            bwt_col.append(symmap[mv])
    n = len(bwt_col)
    if start >= n:
        raise _Fail(START_POINTER)
    # initialiseInverseBWT, decodeNextBWTByte
    ptr = sorted(range(n), key=bwt_col.__getitem__)  # stable: tt[k] = (ptr[k] << 8) | sorted byte k
    first = sorted(bwt_col)
    pre, j = bytearray(n), start
    for i in range(n):
        pre[i] = first[j]
        j = ptr[j]
    # read(): after four equal bytes the next byte is a repeat count.  At the block's end the Java takes it all
    # the same (Bzip2BlockDecompressor.java:297 asks decodeNextBWTByte without looking at bwtBytesDecoded),
    # which leaves bwtBytesDecoded past bwtBlockLength, so line 283 never sees the end again and the output
    # grows until an unchecked exception; libbz2 calls such a block corrupt.  missing: that happened.
    out, last, acc, i, missing = bytearray(), -1, 0, 0, False
    while i < n:
        b = pre[i]
        i += 1
        out.append(b)
        if b != last:
            last, acc = b, 1
        else:
            acc += 1
            if acc == 4:
                acc = 0
                if i < n:
                    out += bytes([b]) * pre[i]
                    i += 1
                else:
                    missing = True
    return bytes(out), missing


def decode(stream: bytes, cap: int, *, check_crc=True, trace=None):
    """(status, bytes, consumed) of the first stream of `stream` with room for cap bytes: on an error the
    bytes of the blocks completed before it and consumed 0.  check_crc=False takes every CRC as right;
    trace, a list, receives each block's computed CRC."""
    out = bytearray()
    r = _Bits(stream, 32)
    try:
        if len(stream) < 4:
            raise _Fail(TRUNCATED)
        if stream[:3] != b"BZh":
            raise _Fail(STREAM_ID)
        level = (stream[3] - 256 if stream[3] > 127 else stream[3]) - ord("0")  # readByte() is signed
        if not 1 <= level <= 9:
            raise _Fail(BLOCK_SIZE)
        stream_crc = 0
        while True:
            magic, stored = (r.read(24) << 24) | r.read(24), r.read(32)
            r.need()
            if magic == END_MAGIC:
                if check_crc and stored != stream_crc:
                    raise _Fail(STREAM_CRC)
                return OK, bytes(out), (r.pos + 7) // 8
            if magic != BLOCK_MAGIC:
                raise _Fail(BLOCK_HEADER)
            data, missing = _block(r, level * 100000)
            if len(out) + len(data) > cap:
                raise _Fail(OUTPUT_FULL)
            if missing:  # met after the block's last byte has gone out
                raise _Fail(DECODING_BLOCK)
            crc = bzip2_crc(data)
            if trace is not None:
                trace.append(crc)
            if check_crc and crc != stored:
                raise _Fail(BLOCK_CRC)
            out += data
            stream_crc = combined_crc([stream_crc, crc])  # (streamCRC << 1 | streamCRC >>> 31) ^ blockCRC
    except _Fail as f:
        return f.code, bytes(out), 0
