"""A Python encoder model for full Zstandard blocks, written from RFC 8878: FSE (distribution writer,
decoding-table build, backward-bitstream encoder for interleaved states), Huffman (canonical codes from
weights, tree descriptions as direct or FSE-compressed weights, 1 and 4 streams with the jump table) and a
block encoder that keeps the previous tables across blocks for Repeat_Mode and Treeless literals.  It emits
what libzstd's encoder never chooses: accuracy logs at both ends, "less than 1" cells, zero-run flag chains,
every size format, streams that end on a byte boundary.  The output model is zstd_handbuilt.run_sequences;
tests/test_zstd_entropy_model.py pins every case on libzstd.  The generator asserts instead of emitting
something else: a used symbol with probability 0, a literal without a weight, a size that does not fit."""
import random
from dataclasses import dataclass

import zstd_handbuilt as HB

LL, ML = HB.LL, HB.ML
MAX_LOG = (9, 8, 9)      # literal lengths, offsets, match lengths
MAX_SYMS = (36, 32, 53)
HW_MAX_LOG = 6
# RFC 8878 3.1.1.3.2.2: the predefined distributions (accuracy logs 6, 5, 6)
PREDEFINED = ((6, [4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1]),
              (5, [1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1]),
              (6, [1, 4, 3, 2, 2, 2, 2, 2, 2] + [1] * 37 + [-1] * 7))
assert [sum(abs(p) for p in d) for _, d in PREDEFINED] == [64, 32, 64] and len(PREDEFINED[2][1]) == 53

# cases libzstd refuses although the RFC allows them: name -> reason (at most three; for these only the
# host decoder and the kernel have to agree)
REFUSED_BY_LIBZSTD = {}


def highbit(v):
    return v.bit_length() - 1


# ---- bit writers ----
class ForwardBits:
    """little-endian bit fields in reading order (FSE distributions)"""

    def __init__(self):
        self.acc = self.n = 0

    def put(self, v, k):
        assert 0 <= v < (1 << k), (v, k)
        self.acc |= v << self.n
        self.n += k

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def back_stream(reads):
    """reads: (value, bits) in the order the decoder reads them.  A backward stream is written in the
    reverse order, and ends with the padding marker, a single 1 bit above the last field written."""
    buf, acc, n = bytearray(), 0, 0
    for v, k in reversed(reads):
        assert 0 <= v < (1 << k) or (k == 0 and v == 0), (v, k)
        acc |= v << n
        n += k
        if n >= 64:
            buf += (acc & 0xFFFFFFFFFFFFFFFF).to_bytes(8, "little")
            acc >>= 64
            n -= 64
    acc |= 1 << n
    return bytes(buf) + acc.to_bytes(n // 8 + 1, "little")


# ---- FSE ----
def write_distribution(log, probs):
    """probs[s] in -1, 0, 1..: the caller's zeros are the zero runs.  Sums to 2^log exactly."""
    assert log >= 5
    w = ForwardBits()
    w.put(log - 5, 4)
    remaining, i = 1 << log, 0
    while remaining > 0:
        assert i < len(probs), "the distribution does not reach the table size"
        p = probs[i]
        assert -1 <= p <= remaining, (i, p, remaining)
        v, r = p + 1, remaining + 1          # v in [0, r]: r + 1 values
        bits = highbit(r) + 1
        low = (1 << (bits - 1)) - 1
        short = (1 << bits) - 1 - r          # this many values take bits - 1 bits
        if v < short:
            w.put(v, bits - 1)
        elif v <= low:
            w.put(v, bits)
        else:
            w.put(v + short, bits)
        remaining -= abs(p)
        i += 1
        if p == 0:                            # 2-bit flags: how many more zeros follow; 3 means another flag
            z = 0
            while i + z < len(probs) and probs[i + z] == 0:
                z += 1
            assert i + z < len(probs), "a zero run ends the distribution"
            i += z
            while z >= 3:
                w.put(3, 2)
                z -= 3
            w.put(z, 2)
    assert all(p == 0 for p in probs[i:]), "probabilities after the table is full"
    return w.bytes()


def fse_table(log, probs):
    """the decoding table: per state (symbol, bits to read, baseline)"""
    size = 1 << log
    assert sum(abs(p) for p in probs) == size
    sym, high = [None] * size, size
    for s, p in enumerate(probs):
        if p == -1:
            high -= 1
            sym[high] = s
    step, pos = (size >> 1) + (size >> 3) + 3, 0
    for s, p in enumerate(probs):
        for _ in range(max(p, 0)):
            sym[pos] = s
            pos = (pos + step) & (size - 1)
            while pos >= high:
                pos = (pos + step) & (size - 1)
    assert pos == 0 and None not in sym
    nxt = [1 if p == -1 else p for p in probs]
    cells = []
    for s in sym:
        x = nxt[s]
        nxt[s] += 1
        nb = log - highbit(x)
        cells.append((s, nb, (x << nb) - size))
    return cells


def fse_states(table, symbols, last_reads_bits=False):
    """the state the decoder is in at each symbol: the last is free (the lowest state of its symbol, or the
    lowest that reads bits), each earlier one is the state of its symbol whose range holds its successor"""
    by = {}
    for st, (s, nb, base) in enumerate(table):
        by.setdefault(s, []).append(st)
    for s in symbols:
        assert s in by, f"symbol {s} has probability 0"
    last = [st for st in by[symbols[-1]] if table[st][1] > 0 or not last_reads_bits]
    assert last, "the stream's end needs a state that reads bits"
    states = [last[0]]
    for s in reversed(symbols[:-1]):
        nx = states[-1]
        hit = [st for st in by[s] if table[st][2] <= nx < table[st][2] + (1 << table[st][1])]
        assert len(hit) == 1
        states.append(hit[0])
    return states[::-1]


def update(table, states, i):
    """(value, bits) the decoder reads to go from state i to state i + 1"""
    _, nb, base = table[states[i]]
    return states[i + 1] - base, nb


# ---- sequences ----
class Triples:
    """a block's sequences as (literal length, match length, offset value): what run_sequences runs"""

    def __init__(self, t):
        self.t = list(t)

    def decoded(self):
        return self.t

    def __bool__(self):
        return bool(self.t)


def split(ll, ml, ov):
    """((code, extra value, extra bits)) for literal length, offset and match length"""
    lc = max(c for c in range(36) if LL[c][0] <= ll)
    mc = max(c for c in range(53) if ML[c][0] <= ml)
    oc = highbit(ov)
    assert ll - LL[lc][0] < (1 << LL[lc][1]) or ll == LL[lc][0]
    assert ml - ML[mc][0] < (1 << ML[mc][1]) or ml == ML[mc][0]
    return (lc, ll - LL[lc][0], LL[lc][1]), (oc, ov - (1 << oc), oc), (mc, ml - ML[mc][0], ML[mc][1])


PRE, RLE, REP = ("pre",), ("rle",), ("rep",)


def FSE(log, probs):
    return ("fse", log, list(probs))


class BlockEncoder:
    """Compressed blocks of one frame; remembers what the decoder will hold for Repeat_Mode and Treeless."""

    def __init__(self):
        self.seq = [None, None, None]   # (log, table) per code
        self.huf = None                 # symbol -> (code, bits)

    def sequences(self, triples, modes):
        if not triples:
            return b"\x00"
        codes = [split(*t) for t in triples]
        head = HB.nseq_field(len(triples)) + bytes([(_MODE[modes[0][0]] << 6) | (_MODE[modes[1][0]] << 4) | (_MODE[modes[2][0]] << 2)])
        chains = []
        for which, mode in enumerate(modes):
            syms = [c[which][0] for c in codes]
            assert max(syms) < MAX_SYMS[which]
            if mode[0] == "pre":
                log, probs = PREDEFINED[which]
                self.seq[which] = (log, fse_table(log, probs))
            elif mode[0] == "rle":
                assert len(set(syms)) == 1, "RLE mode codes one symbol"
                self.seq[which] = (0, [(syms[0], 0, 0)])
                head += bytes([syms[0]])
            elif mode[0] == "fse":
                _, log, probs = mode
                assert log <= MAX_LOG[which] and len(probs) <= MAX_SYMS[which]
                head += write_distribution(log, probs)
                self.seq[which] = (log, fse_table(log, probs))
            else:
                assert self.seq[which] is not None, "Repeat_Mode without a previous table"
            chains.append(fse_states(self.seq[which][1], syms))
        tab = [t for _, t in self.seq]
        reads = [(chains[w][0], self.seq[w][0]) for w in range(3)]        # initial states: literal length, offset, match length
        for i, (l, o, m) in enumerate(codes):
            reads += [(o[1], o[2]), (m[1], m[2]), (l[1], l[2])]           # extra bits: offset, match length, literal length
            if i + 1 < len(codes):
                reads += [update(tab[w], chains[w], i) for w in (0, 2, 1)]  # updates: literal length, match length, offset
        return head + back_stream(reads)

    def literals(self, lits, coding):
        if coding is None:
            return HB.literals_section(lits)
        if isinstance(coding, Huf):
            desc, self.huf = coding.description(), huf_codes(coding.weights)
        else:
            assert self.huf is not None, "Treeless literals without a previous tree"
            desc = b""
        body = desc + huf_streams(self.huf, lits, coding.streams)
        fmt = coding.fmt if coding.fmt is not None else 0 if coding.streams == 1 else \
            1 if max(len(lits), len(body)) < 1024 else 2 if max(len(lits), len(body)) < 16384 else 3
        assert (fmt == 0) == (coding.streams == 1)
        return lit_header(2 if isinstance(coding, Huf) else 3, fmt, len(lits), len(body)) + body

    def block(self, lits, seqs, coding, last):
        body = self.literals(lits, coding.get("lit")) + self.sequences(seqs.decoded() if seqs else [], coding.get("modes", (PRE, PRE, PRE)))
        assert len(body) <= 131072, "Block_Size above Block_Maximum_Size"
        return HB.block_header(last, 2, len(body)) + body


_MODE = {"pre": 0, "rle": 1, "fse": 2, "rep": 3}


# ---- Huffman ----
def implied_weight(weights):
    """the weight the decoder deduces for the symbol after weights[]: it completes the next power of two"""
    total = sum(1 << (w - 1) for w in weights if w)
    assert total > 0
    left = (1 << (highbit(total) + 1)) - total
    assert left & (left - 1) == 0, "the weights cannot be completed by one symbol"
    return highbit(left) + 1


def huf_codes(weights):
    """weights of symbols 0..n-1, the last one implied: symbol -> (code, bits), as the RFC assigns them
    (from the lowest weight, symbols in natural order, codes in sequence)"""
    assert weights[-1] == implied_weight(weights[:-1]), "the last weight is not the implied one"
    depth = highbit(sum(1 << (w - 1) for w in weights if w))
    assert 1 <= depth <= 11 and max(weights) <= depth
    codes, code = {}, 0
    for w in range(1, depth + 1):
        for s, sw in enumerate(weights):
            if sw == w:
                codes[s] = (code, depth + 1 - w)
                code += 1
        assert code % 2 == 0 or w == depth
        code >>= 1
    assert code == 1 and len(weights) <= 256
    return codes


@dataclass
class Huf:
    """Compressed literals: weights (all symbols, the last implied), tree form 'direct' or ('fse', log, probs
    over weight values), 1 or 4 streams, size format (None: the smallest that fits)"""
    weights: list
    tree: object = "direct"
    streams: int = 1
    fmt: int = None

    def description(self):
        sent = self.weights[:-1]
        if self.tree == "direct":
            assert 1 <= len(sent) <= 128
            nib = sent + [0] * (len(sent) & 1)
            return bytes([127 + len(sent)]) + bytes((nib[i] << 4) | nib[i + 1] for i in range(0, len(nib), 2))
        _, log, probs = self.tree
        assert log <= HW_MAX_LOG and len(sent) >= 2
        table = fse_table(log, probs)
        a, b = fse_states(table, sent[0::2], True), fse_states(table, sent[1::2], True)
        reads = [(a[0], log), (b[0], log)]
        for i in range(len(sent) - 2):      # the last symbol of each state is read off without an update:
            ch = b if i & 1 else a          # the update after the last but one runs past the stream's start
            reads.append(update(table, ch, i >> 1))
        body = write_distribution(log, probs) + back_stream(reads)
        assert len(body) < 128, "FSE-compressed weights take at most 127 bytes"
        return bytes([len(body)]) + body


@dataclass
class Treeless:
    streams: int = 1
    fmt: int = None


def huf_stream(codes, lits):
    for s in lits:
        assert s in codes, f"literal {s} has no weight"
    return back_stream([codes[s] for s in lits])


def huf_streams(codes, lits, streams):
    assert len(lits) > 0
    if streams == 1:
        return huf_stream(codes, lits)
    assert len(lits) >= 6
    seg = (len(lits) + 3) >> 2
    assert 3 * seg <= len(lits)
    parts = [huf_stream(codes, lits[k * seg:(k + 1) * seg]) for k in range(3)] + [huf_stream(codes, lits[3 * seg:])]
    assert all(len(p) < 65536 for p in parts[:3])
    return b"".join(len(p).to_bytes(2, "little") for p in parts[:3]) + b"".join(parts)


def lit_header(ltype, fmt, regen, comp):
    bits = (10, 10, 14, 18)[fmt]
    assert regen < (1 << bits) and comp < (1 << bits), "the sizes do not fit the size format"
    return (ltype | (fmt << 2) | (regen << 4) | (comp << (4 + bits))).to_bytes((3, 3, 4, 5)[fmt], "little")


# ---- composing frames ----
def resolve_offset(ov, ll, rep):
    """(offset, repeat history after it) of an offset value, or None where it resolves to 0"""
    if ov > 3:
        return ov - 3, [ov - 3, rep[0], rep[1]]
    idx = ov + (ll == 0)
    if idx == 1:
        return rep[0], list(rep)
    if idx == 2:
        return rep[1], [rep[1], rep[0], rep[2]]
    off = rep[2] if idx == 3 else rep[0] - 1
    return (off, [off, rep[0], rep[1]]) if off else None


def spread(log, syms, minus=()):
    """a distribution over syms (ascending): those in `minus` get -1, the others share the rest evenly"""
    plain = [s for s in syms if s not in minus]
    rest = (1 << log) - len(minus)
    assert plain and rest >= len(plain)
    probs = [0] * (max(syms) + 1)
    for s in minus:
        probs[s] = -1
    for k, s in enumerate(plain):
        probs[s] = rest // len(plain) + (k < rest % len(plain))
    return probs


def draw(rng, probs, n, never=()):
    """n symbols: every one with a probability (but `never`) at least once, the rest by their weights;
    the codes of 32768 bytes and more once only, so that a block stays a block"""
    used = [s for s, p in enumerate(probs) if p and s not in never]
    assert n >= len(used)
    again = [s for s in used if s < 34]
    out = used + rng.choices(again, [abs(probs[s]) for s in again], k=n - len(used))
    rng.shuffle(out)
    return out


def lits_for(rng, weights, n):
    """n literals over the symbols that have a weight, likelier the shorter their code, each at least once if n allows"""
    used = [s for s, w in enumerate(weights) if w]
    out = used[:n] + rng.choices(used, [1 << weights[s] for s in used], k=max(0, n - len(used)))
    rng.shuffle(out)
    return bytes(out)


class Plan:
    """composes a frame block by block, tracking the position and the repeat offsets so that the
    sequences it draws are valid"""

    def __init__(self, seed):
        self.rng = random.Random(seed)
        self.pos, self.rep, self.blocks, self.weights = 0, [1, 4, 8], [], None

    def raw(self, n):
        self.blocks.append(("raw", self.rng.randbytes(n)))
        self.pos += n
        return self

    def rle(self, byte, n):
        self.blocks.append(("rle", byte, n))
        self.pos += n
        return self

    def seqs(self, codes):
        """codes: (literal-length code, offset code, match-length code) per sequence; the extra bits are random"""
        out = []
        for lc, oc, mc in codes:
            for _ in range(200):
                ll = LL[lc][0] + self.rng.getrandbits(min(LL[lc][1], 12))  # (the widest fields: _widest)
                ml = ML[mc][0] + self.rng.getrandbits(min(ML[mc][1], 12))
                ov = (1 << oc) + self.rng.getrandbits(oc)
                r = resolve_offset(ov, ll, self.rep)
                if r and r[0] <= self.pos + ll:
                    break
            else:
                raise AssertionError(f"no valid offset for code {oc} at {self.pos}")
            self.rep = r[1]
            self.pos += ll + ml
            out.append((ll, ml, ov))
        return out

    def ent(self, codes=(), lit=None, modes=(PRE, PRE, PRE), tail=0, triples=None, rle_lits=None):
        """a Compressed block: sequences from codes (or given as triples), `tail` literals after the last"""
        if triples is None:
            triples = self.seqs(codes)
        else:
            for ll, ml, ov in triples:
                self.rep = resolve_offset(ov, ll, self.rep)[1]
                self.pos += ll + ml
        n = sum(t[0] for t in triples) + tail
        self.pos += tail
        if isinstance(lit, Huf):
            self.weights = lit.weights
        if lit is not None:
            lits = lits_for(self.rng, self.weights, n)
        elif rle_lits is not None:
            lits = ("rle", rle_lits, n)
        else:
            lits = self.rng.randbytes(n)
        self.blocks.append(("ent", lits, Triples(triples), {"lit": lit, "modes": modes}))
        return self

    def build(self, **kw):
        import zstd_frames as Z
        frame, want = HB.build(self.blocks, **kw)
        f = Z.parse_frame(frame)
        window = len(want) if f.single_segment else (1 << (10 + (f.window_descriptor >> 3))) * (8 + (f.window_descriptor & 7)) // 8
        assert all(b.size <= min(window, 131072) for b in f.blocks), "a block above Block_Maximum_Size"
        return frame, want


# symbol sets that keep a block small: literal lengths up to 39, offsets below 1024, match lengths up to 66
LLS, OFS, MLS = [0, 1, 2, 3, 5, 8, 16, 20, 22], [0, 1, 2, 3, 5, 7, 9], [0, 1, 2, 5, 10, 32, 36, 39]
DEPTH11 = [1, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11]


def _fse_block(p, dists, n, never=((), (), ()), **kw):
    """one block with all three codes FSE-compressed, n sequences that use every symbol of dists"""
    cols = [draw(p.rng, d[2], n, nv) for d, nv in zip(dists, never)]
    return p.ent(list(zip(*cols)), modes=tuple(dists), **kw)


def _fse_cases(c):
    def one(name, seed, dists, n=60, history=1024, never=((), (), ())):
        c[name] = _fse_block(Plan(seed).raw(history), dists, n, never, tail=7).build()

    one("fse_log5", 100, (FSE(5, spread(5, LLS)), FSE(5, spread(5, OFS)), FSE(5, spread(5, MLS))))
    one("fse_log_max", 101, (FSE(9, spread(9, LLS)), FSE(8, spread(8, OFS)), FSE(9, spread(9, MLS))), n=200)
    one("fse_less_than_one", 102, (FSE(6, spread(6, LLS, (1, 8, 22))), FSE(6, spread(6, OFS, (0, 5, 9))), FSE(7, spread(7, MLS, (2, 10, 36, 39)))))
    for k in (1, 2, 3, 4, 7):   # symbols 0, 1 and 3 + k: a zero and k more between them
        d = spread(6, [0, 1, 3 + k])
        one(f"fse_zero_run_{k}", 110 + k, (FSE(6, d), FSE(6, d), FSE(6, d)), n=40, history=4096)
    one("fse_two_symbols", 120, (FSE(6, spread(6, [3, 17])), FSE(5, spread(5, [2, 6])), FSE(7, spread(7, [0, 33]))), n=40)
    # one symbol on size - 1 cells beside one "less than 1" symbol: the big symbol's states read 0 bits or 1
    one("fse_size_minus_1", 121, (FSE(5, [31, -1]), FSE(5, [0, 0, 31, 0, -1]), FSE(6, [-1, 0, 0, 63])), n=40)
    # the highest symbols, 35 and 52, in two blocks: either alone takes more than half a block's output
    p = Plan(122).raw(1024)
    _fse_block(p, (FSE(6, spread(6, [0, 1, 2, 3, 20, 35], (35,))), FSE(6, spread(6, OFS)), FSE(6, spread(6, MLS + [52], (52,)))), 40, ((), (), (52,)))
    _fse_block(p, (FSE(6, spread(6, LLS + [35], (35,))), FSE(6, spread(6, OFS)), FSE(6, spread(6, [0, 1, 2, 40, 52], (52,)))), 40, ((35,), (), ()), tail=3)
    c["fse_top_symbol"] = p.build()
    # zero runs that reach the last symbol of each alphabet (offset code 31 has a cell and is never used:
    # it would need 2 GiB of history)
    p = Plan(123).raw(1024)
    _fse_block(p, (FSE(6, spread(6, [0, 1, 35], (35,))), FSE(5, spread(5, [0, 1, 2, 3, 31], (31,))), FSE(6, spread(6, [0, 1, 52], (52,)))), 40,
               ((), (31,), (52,)))
    _fse_block(p, (FSE(6, spread(6, [0, 1, 35], (35,))), FSE(5, spread(5, [0, 1, 2, 3, 31], (31,))), FSE(6, spread(6, [0, 1, 52], (52,)))), 40,
               ((35,), (31,), ()))
    c["fse_zero_run_to_last"] = p.build()
    # the tile of 64 sequences crossed with live states and extra bits in every field
    for n in (63, 64, 65, 128, 129):
        one(f"tile_{n}", 130 + n, (FSE(6, spread(6, [16, 17, 18, 20, 22, 23])), FSE(6, spread(6, [3, 4, 5, 7, 9])), FSE(7, spread(7, [32, 33, 36, 38, 40]))), n=n)


def _mode_cases(c):
    sets = ([16, 17, 20, 25], [3, 5, 8], [4, 33, 38])
    fse = tuple(FSE(6, spread(6, s)) for s in sets)
    for name, first in (("pre", (PRE,) * 3), ("rle", (RLE,) * 3), ("fse", fse)):
        p = Plan(200 + len(c)).raw(1024)
        pick = (lambda n: [(17, 5, 33)] * n) if name == "rle" else (lambda n: [tuple(p.rng.choice(s) for s in sets) for _ in range(n)])
        p.ent(pick(30), modes=first).ent(pick(70), modes=(REP,) * 3, tail=5)
        c[f"repeat_after_{name}"] = p.build()
    # Repeat across a Raw block and a Compressed block without sequences
    p = Plan(210).raw(1024)
    pick = lambda n: [tuple(p.rng.choice(s) for s in sets) for _ in range(n)]
    p.ent(pick(40), modes=fse).raw(100).ent(pick(20), modes=(REP,) * 3).ent((), tail=50).ent(pick(66), modes=(REP,) * 3, tail=1)
    c["repeat_chain"] = p.build()
    # RLE mode with the highest symbols: 35 and 52, a block each; the offset code is the highest the
    # history of this frame reaches (16)
    p = Plan(211).raw(1024)
    p.ent([(35, 3, 0)], modes=(RLE,) * 3, tail=2).ent([(0, 16, 52)], modes=(RLE,) * 3)
    c["rle_top_symbols"] = p.build()
    p = Plan(212).raw(1024)
    for rot in range(3):
        modes = [fse[w] if (w + rot) % 3 == 0 else PRE if (w + rot) % 3 == 1 else RLE for w in range(3)]
        codes = [tuple((17, 5, 33)[w] if modes[w] is RLE else p.rng.choice(sets[w]) for w in range(3)) for _ in range(50)]
        p.ent(codes, modes=tuple(modes), tail=rot)
    c["mixed_modes"] = p.build()


def _widest(c):
    """One sequence with the most bits the format allows within the decoder's limits: literal-length code 35
    and match-length code 52 with all 16 extra bits set, offset code 22 with its low 18 extra bits set (the
    most this history of 33 RLE blocks reaches), and, because a second sequence follows, state updates of
    9, 8 and 9 bits from "less than 1" cells of log-9/8/9 tables.  Offset code 22 is the ceiling chosen
    here so that the frame stays a few MiB; kMaxWindow would allow codes up to 27.  131071 Raw literals do
    not fit a block, so the literals are Huffman-compressed."""
    p = Plan(300)
    for k in range(33):
        p.rle(k + 1, 131072)
    ll, ml = 65536 + 65535, 65539 + 65535
    ov = (1 << 22) + (1 << 18) - 1
    assert ov - 3 <= p.pos + ll
    zeros = lambda n: [0] * n
    modes = (FSE(9, [511] + zeros(34) + [-1]), FSE(8, [255] + zeros(21) + [-1]), FSE(9, [511] + zeros(51) + [-1]))
    p.ent(triples=[(ll, ml, ov), (0, 3, 1)], lit=Huf([1, 1, 1, 1], streams=4, fmt=3), modes=modes)
    c["widest_sequence"] = p.build()


def _huffman_cases(c):
    def one(name, seed, huf, n=300, seq=True):
        huf.streams, huf.fmt = (1, None) if n < 900 else (4, 2)
        p = Plan(seed).raw(64)
        codes = [(p.rng.choice(LLS), p.rng.choice(OFS[:4]), p.rng.choice(MLS)) for _ in range(12)] if seq else ()
        c[name] = p.ent(codes, lit=huf, tail=n).build()

    rng = random.Random(400)
    one("huf_direct_1", 401, Huf([1, 1]), n=40, seq=False)                        # depth 1, the implied weight equals it
    one("huf_direct_2", 402, Huf([1, 1, 2]), n=40)
    one("huf_direct_3", 403, Huf([1, 1, 2, 3]), n=40)
    one("huf_direct_128", 404, Huf([1] * 128 + [8]), n=600)
    one("huf_holes", 405, Huf([0] * 65 + [3, 0, 0, 1, 0, 2, 0, 0, 0, 1, 4, 0, 5]), n=200)   # weight-0 symbols between used ones
    one("huf_depth1_holes", 406, Huf([1, 0, 0, 1]), n=33, seq=False)
    one("huf_depth11_last_is_depth", 407, Huf(DEPTH11), n=3000)                  # the implied weight is 11
    one("huf_depth11_last_is_1", 408, Huf(DEPTH11[::-1]), n=3000)                # the implied weight is 1
    # FSE-compressed weights: 30 sent (the stream ends on the first state), 31 sent (on the second)
    w30 = _complete(shuffled_base(rng, {1: 14, 2: 11, 3: 4, 4: 1}))
    one("huf_fse_log5_even", 409, Huf(w30, tree=_hw_dist(5, w30)), n=500)
    w31 = _complete(shuffled_base(rng, {1: 16, 2: 11, 3: 2, 4: 2}))
    one("huf_fse_log6_odd", 410, Huf(w31, tree=_hw_dist(6, w31)), n=500)
    wm = _complete(shuffled_base(rng, {0: 1, 1: 12, 2: 10, 3: 8, 5: 1, 6: 1}))
    one("huf_fse_less_than_one", 411, Huf(wm, tree=_hw_dist(6, wm, minus=(0, 5, 6))), n=500)
    w129 = _complete(shuffled_base(rng, {1: 66, 2: 63}))
    one("huf_fse_129", 412, Huf(w129, tree=_hw_dist(6, w129)), n=2000)
    w255 = _complete(shuffled_base(rng, {1: 126, 2: 129}))                        # symbol 255 is the implied one
    one("huf_fse_255", 413, Huf(w255, tree=_hw_dist(6, w255)), n=4000)
    wd = DEPTH11[:-1] + [10, 0, 0]
    rng.shuffle(wd)
    wd = _complete(wd)
    one("huf_fse_depth11", 414, Huf(wd, tree=_hw_dist(6, wd)), n=3000)


def shuffled_base(rng, counts):
    ws = [w for w, k in counts.items() for _ in range(k)]
    rng.shuffle(ws)
    return ws


def _complete(sent):
    return sent + [implied_weight(sent)]


def _hw_dist(log, weights, minus=()):
    """a distribution for the sent weights: cells in proportion to their counts, `minus` as "less than 1" """
    sent = weights[:-1]
    count = {w: sent.count(w) for w in set(sent)}
    plain = sorted(w for w in count if w not in minus)
    rest = (1 << log) - len(minus)
    total = sum(count[w] for w in plain)
    probs = [0] * (max(count) + 1)
    for w in minus:
        assert w in count
        probs[w] = -1
    for w in plain:
        probs[w] = max(1, count[w] * rest // total)
    probs[max(plain, key=lambda w: probs[w])] += rest - sum(probs[w] for w in plain)
    assert all(probs[w] > 0 for w in plain)
    return ("fse", log, probs)


def _stream_cases(c):
    def one(name, seed, huf, n):
        # (a window of 1 KiB where the content is smaller than the block that carries it)
        c[name] = Plan(seed).ent((), lit=huf, tail=n).build(**(dict(single=False, window_descriptor=0) if n < 100 else {}))

    w = [3, 1, 2, 0, 1, 4, 5]
    for n in (1, 2, 1023):
        one(f"lit1_{n}", 500 + n, Huf(w, streams=1), n)
    for n in (6, 7, 8, 9):
        one(f"lit4_{n}", 510 + n, Huf(w, streams=4, fmt=1), n)
    one("lit4_format1_1023", 520, Huf(w, streams=4, fmt=1), 1023)
    one("lit4_format2_16383", 521, Huf(w, streams=4, fmt=2), 16383)
    one("lit4_format3_131072", 522, Huf(DEPTH11, streams=4, fmt=3), 131072)   # a full block without sequences
    # depth 1: a bit a literal, so 8 literals a stream fill whole bytes and the stream's last byte is the marker alone
    one("lit1_ends_on_a_byte", 523, Huf([1, 1], streams=1), 16)
    one("lit4_ends_on_a_byte", 524, Huf([1, 1], streams=4, fmt=1), 32)
    # the sequence bitstream and the weight bitstream ending on a byte boundary: found by search over seeds
    for seed in range(1000):
        p = Plan(5000 + seed).raw(1024)
        f, want = p.ent([(p.rng.choice(LLS), p.rng.choice(OFS), p.rng.choice(MLS)) for _ in range(20)],
                        modes=(FSE(6, spread(6, LLS)), FSE(5, spread(5, OFS)), FSE(6, spread(6, MLS)))).build()
        if f[-1] == 1:
            c["seq_ends_on_a_byte"] = (f, want)
            break
    for seed in range(1000):
        rng = random.Random(6000 + seed)
        ws = _complete(shuffled_base(rng, {1: 14, 2: 11, 3: 4, 4: 1}))
        huf = Huf(ws, tree=_hw_dist(5, ws))
        if huf.description()[-1] == 1:
            one("weights_end_on_a_byte", 6000 + seed, huf, 100)
            break
    assert "seq_ends_on_a_byte" in c and "weights_end_on_a_byte" in c


def _treeless_cases(c):
    w = [2, 0, 1, 3, 1, 4, 5]
    some = lambda p, n: [(p.rng.choice(LLS), p.rng.choice(OFS[:4]), p.rng.choice(MLS)) for _ in range(n)]
    p = Plan(600).raw(64)
    c["treeless_direct"] = p.ent(some(p, 8), lit=Huf(w), tail=90).ent(some(p, 8), lit=Treeless(), tail=70).build()
    p = Plan(601).raw(64)
    p.ent(some(p, 8), lit=Huf(w), tail=90).ent(some(p, 5), tail=20).ent(some(p, 5), rle_lits=0x41, tail=9).raw(33)
    c["treeless_after_others"] = p.ent(some(p, 8), lit=Treeless(), tail=70).build()
    p = Plan(602).raw(64)
    c["treeless_1_after_4"] = p.ent(some(p, 8), lit=Huf(w, streams=4, fmt=1), tail=200).ent(some(p, 8), lit=Treeless(1), tail=50).build()
    # Huffman literals, then a frame that ends in an overlapping match (offset 2, 300 bytes)
    c["huffman_then_overlap"] = Plan(604).raw(64).ent(triples=[(20, 5, 30), (10, 300, 5)], lit=Huf(w, streams=4, fmt=1)).build()
    p = Plan(603).raw(64)
    c["treeless_4_after_1"] = p.ent(some(p, 8), lit=Huf(w, streams=1), tail=50).ent(some(p, 8), lit=Treeless(4, 1), tail=200).build()


def _everything(c):
    """multi-block frames, each block drawn from the kinds above by a seeded choice"""
    sets = (LLS, OFS, MLS)

    def block(p, k, first):
        rng = p.rng
        codes = [tuple(rng.choice(s) for s in sets) for _ in range(rng.choice((5, 64, 70)))]
        fse = tuple(FSE(lg, spread(lg, s, tuple(rng.sample(s, 2)))) for lg, s in zip((rng.choice((5, 9)), rng.choice((5, 8)), rng.choice((6, 9))), sets))
        kind = rng.randrange(6)
        huf = Huf(_complete(shuffled_base(rng, {0: 3, 1: 10, 2: 7, 3: 4, 4: 2})), streams=rng.choice((1, 4)))
        if huf.streams == 4:
            huf.fmt = rng.choice((1, 2))
        if rng.random() < 0.5:
            huf.tree = _hw_dist(rng.choice((5, 6)), huf.weights)
        if first or kind == 0:
            p.ent(codes, lit=huf, modes=fse, tail=rng.randrange(9, 300))
        elif kind == 1:
            p.ent(codes, lit=Treeless(rng.choice((1, 4))), modes=(REP,) * 3, tail=rng.randrange(9, 300))
        elif kind == 2:
            p.raw(rng.randrange(1, 200))
        elif kind == 3:
            p.ent((), lit=Treeless(1), tail=rng.randrange(1, 100))
        elif kind == 4:
            p.ent(codes, modes=(fse[0], REP, PRE), tail=3)
        else:
            p.ent(codes, rle_lits=rng.randrange(256), modes=(REP, fse[1], REP))

    for k in range(4):
        p = Plan(700 + k).raw(1024)
        for b in range(3 + (k + p.rng.randrange(2)) % 4):
            block(p, k, b == 0)
        # the last of them has a window (1 MiB) and no content size
        c[f"everything_{k}"] = p.build(single=False, window_descriptor=0x50, with_size=False) if k == 3 else p.build()


_CACHE, _OTHER = {}, {}


def cases():
    """name -> (frame, expected output): built once per process"""
    if not _CACHE:
        c = {}
        _fse_cases(c)
        _mode_cases(c)
        _widest(c)
        _huffman_cases(c)
        _stream_cases(c)
        _treeless_cases(c)
        _everything(c)
        _CACHE.update(c)
    return _CACHE


# ---- targeted corruption ----
def corruption_frames():
    """two small frames: three FSE tables, FSE-compressed weights and four streams; direct weights and a
    second block in Repeat_Mode with Treeless literals"""
    if "corruption" not in _OTHER:
        rng = random.Random(800)
        w = _complete(shuffled_base(rng, {1: 14, 2: 11, 3: 4, 4: 1}))
        some = lambda p, n: [(p.rng.choice(LLS), p.rng.choice(OFS[:5]), p.rng.choice(MLS)) for _ in range(n)]
        fse = (FSE(6, spread(6, LLS, (22,))), FSE(5, spread(5, OFS[:5])), FSE(6, spread(6, MLS, (39,))))
        p = Plan(801).raw(32)
        a = p.ent(some(p, 14), lit=Huf(w, tree=_hw_dist(5, w), streams=4, fmt=1), modes=fse, tail=40).build()
        p = Plan(802).raw(32)
        b = p.ent(some(p, 10), lit=Huf([2, 0, 1, 3, 1, 4, 5]), modes=fse, tail=30) \
             .ent(some(p, 10), lit=Treeless(), modes=(REP,) * 3, tail=25).build()
        _OTHER["corruption"] = [a, b]
    return _OTHER["corruption"]


def flips_of(f):
    """every single-bit flip of every byte of the frame's distributions, tree descriptions and jump table"""
    import zstd_frames as Z
    out = []
    for blk in Z.parse_frame(f, entropy=True).blocks:
        if blk.type == Z.COMPRESSED:
            for lo, hi in blk.tables:
                for k in range(lo, hi):
                    for bit in range(8):
                        g = bytearray(f)
                        g[k] ^= 1 << bit
                        out.append(bytes(g))
    return out


def bit_flips():
    return [g for f, _ in corruption_frames() for g in flips_of(f)]


def truncations():
    return [f[:k] for f, _ in corruption_frames() for k in range(len(f))]


def stale_state_batch():
    """Five frames for one wave of the kernel to take in order: (frame, expected output or None where the
    frame must be refused), and the two refused frames' bodies behind the first frame's blocks, as frames
    that must decode.  1: tables of logs 9, 8, 9 and a tree of depth 11.  2: a Treeless first block, 3: a
    Repeat_Mode first block, both encoded with what frame 1 leaves behind.  4: logs 5 and a tree of depth 1.
    5: frame 1 again."""
    if "stale" not in _OTHER:
        some = lambda p, n, ofs: [(16, 2, 0)] + [(p.rng.choice(LLS), p.rng.choice(ofs), p.rng.choice(MLS)) for _ in range(n)]
        big = (FSE(9, spread(9, LLS)), FSE(8, spread(8, OFS)), FSE(9, spread(9, MLS)))
        small = (FSE(5, spread(5, LLS)), FSE(5, spread(5, OFS)), FSE(5, spread(5, MLS)))
        p1 = Plan(900).raw(1024)
        p1.ent(some(p1, 70, OFS), lit=Huf(DEPTH11, streams=4, fmt=2), modes=big, tail=200)
        first = p1.build()
        p4 = Plan(903).raw(1024)
        fourth = p4.ent(some(p4, 70, OFS), lit=Huf([1, 1], streams=4, fmt=2), modes=small, tail=200).build()
        refused, after_first = [], []
        for seed in (901, 902):
            p = Plan(seed)
            p.weights = DEPTH11
            if seed == 901:
                p.ent((), lit=Treeless(1), tail=150)
            else:
                p.ent(some(p, 40, OFS[:4]), modes=(REP,) * 3, tail=5)   # offsets of 12 bytes at most: valid on their own
            enc = BlockEncoder()
            enc.block(*p1.blocks[1][1:], False)      # the encoder as after frame 1
            kind, lits, seqs, coding = p.blocks[0]
            body = enc.block(lits, seqs, coding, True)
            out = bytearray()
            HB.run_sequences(out, lits, seqs, [1, 4, 8])
            refused.append((HB.frame_header(len(out), single=False, window_descriptor=0x10) + body, None))
            # behind frame 1's blocks the same body decodes (the repeat offsets there are frame 1's: only the status)
            after_first.append(first[0][:-len(_last_block(first[0]))] + _not_last(_last_block(first[0])) + body)
        _OTHER["stale"] = ([first, refused[0], refused[1], fourth, first], after_first)
    return _OTHER["stale"]


def _last_block(frame):
    import zstd_frames as Z
    f = Z.parse_frame(frame)
    return frame[f.end - 3 - f.blocks[-1].content:f.end]


def _not_last(block):
    return bytes([block[0] & 0xFE]) + block[1:]


def write_frames(path):
    """the input of scripts/asan/zstd_entropy_fuzz.cpp: per frame a 4-byte length, a flag byte (1: also
    truncate it and flip its bits) and the frame"""
    with open(path, "wb") as fp:
        for flag, frames in ((1, corruption_frames()), (0, list(cases().values()))):
            for f, _ in frames:
                fp.write(len(f).to_bytes(4, "little") + bytes([flag]) + f)


if __name__ == "__main__":
    import sys
    import zstd_entropy  # the module zstd_handbuilt.build imports, so that its classes are the same ones
    zstd_entropy.write_frames(sys.argv[1])
