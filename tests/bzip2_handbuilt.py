"""Hand-built bzip2 streams libbz2's encoder never writes, for the decoder tests on the CPU
(nx_bzip2_decode_host) and the GPU (nx_bzip2_decode_batch): every field set through bzip2_model's writer.
A case is (name, stream, cap, status, data, consumed, verdict): the expectations come from bzip2_model.decode,
never from the code under test; verdict is what libbz2 says about the stream ("ok", "error", "more"), or
"outside" where libbz2's documented limits exclude it (OUTSIDE names the class and the reason).  Seeded;
built once per process.  kc is the kernel's chain count (bzip2_decode_chains())."""
import bz2
import functools
import random
from dataclasses import dataclass, replace

import bzip2_model as M
from bzip2_model import RUNA, RUNB

GROUPS = ("huffman", "runs", "walk", "final", "streams")
TILE = 1024      # the decoder's LDS tile: symbol decode and final stage
RLE_INLINE = 16  # final-stage runs below this are written in place

# The classes a case may be "outside" for, and why libbz2 cannot be asked.
OUTSIDE_CLASSES = {
    "len21_23": "libbz2 refuses a code length above 20 on every value the delta coding takes; the Java goes to 23",
    "run_wrap": "libbz2 refuses a run counter past 2 Mi; the Java's int counter and increment wrap",
}
# name -> class of every "outside" case (filled while the cases are built)
OUTSIDE = {}
# Cases the model takes otherwise than libbz2, with libbz2's verdict as observed with the libbz2 behind
# Python's bz2 here (BZ2_bzlibVersion() = "1.0.8, 13-Jul-2019"):
#   alpha_none_*     with no byte value in use the end-of-block symbol is 1, which the Java takes for RUNB before
#                    it compares with end-of-block: the block cannot end and the input runs out (TRUNCATED);
#                    libbz2 refuses an empty symbol map outright.
# sel_18003 (18003 selectors on a small block) is "incorrect selectors number" in the Java and an error for this
# libbz2 too; 1.0.6 took any count and upstream 1.0.8 reads and drops the selectors past 18002, so the verdict
# is the one observed, not a property of the format.
LIBBZ2_DIFFERS = {"alpha_none_eob": "error", "alpha_none_runa": "error"}


@dataclass(frozen=True)
class Case:
    group: str
    name: str
    stream: bytes
    cap: int
    status: int
    data: bytes
    consumed: int
    verdict: str


class _Cases:
    def __init__(self):
        self.out, self.names = [], set()

    def add_sealed(self, group, name, level, blocks):
        """add(seal(level, blocks)) with one run of the model in place of two: the decode that finds the CRCs
        is the decode of the sealed stream, whose CRCs are then right."""
        trace = []
        natural = M.decode(M.write_stream(level, blocks), 1 << 30, check_crc=False, trace=trace)
        for b, c in zip(blocks, trace):
            b.crc = c
        self.add(group, name, M.write_stream(level, blocks), natural=natural)

    def add(self, group, name, stream, cap=None, outside=None, natural=None):
        assert name not in self.names, name
        self.names.add(name)
        st, data, used = natural or M.decode(stream, 1 << 30)
        if cap is None:
            cap = len(data) if st == M.OK else len(data) + 4096
        verdict = {M.OK: "ok", M.TRUNCATED: "more"}.get(st, "error")  # libbz2 has no cap: of the uncapped decode
        if cap < len(data) or st != M.OK:
            st, data, used = M.decode(stream, cap)
        if outside:
            OUTSIDE[name] = outside
            verdict = "outside"
        verdict = LIBBZ2_DIFFERS.get(name, verdict)
        self.out.append(Case(group, name, stream, cap, st, data, used, verdict))


def _no_runs(rng, n, values, avoid=None):
    """n bytes over values with no two neighbours equal, the last one not `avoid`."""
    out = bytearray()
    while len(out) < n:
        v = rng.choice(values)
        if (out and out[-1] == v) or (len(out) == n - 1 and v == avoid):
            continue
        out.append(v)
    return bytes(out)


def complete_lengths(alpha, longest):
    """A complete code over alpha symbols whose longest code has `longest` bits, lengths ascending: a spine
    with one leaf per depth and two at the bottom, then the shallowest leaves split until there are alpha."""
    lens = list(range(1, longest)) + [longest, longest]
    assert alpha >= len(lens)
    while len(lens) < alpha:
        lens.sort()
        k = next(i for i, x in enumerate(lens) if x < longest)
        lens[k:k + 1] = [lens[k] + 1, lens[k] + 1]
    return sorted(lens)


# ------------------------------------------------------------------ Huffman stage
def _huffman(C):
    rng = random.Random(1)
    g = "huffman"
    values = list(range(40, 70))  # 30 byte values: an alphabet of 32

    def column(n):  # n - 1 bytes with every value and no run: n symbols with the end-of-block symbol
        c = bytes(values) + _no_runs(rng, n - 31, values)
        while c[29] == c[30]:
            c = bytes(values) + _no_runs(rng, n - 31, values)
        assert len(M.column_symbols(c)[1]) == n
        return c

    col = column(60)
    start = max(M.cycles(col), key=len)[0]
    alpha = 32
    flat = M.flat_lengths(alpha)

    def one(name, lengths, outside=None, **over):
        C.add(g, name, M.seal(1, [M.column_block(col, start, lengths=lengths, **over)]), outside=outside)

    # code lengths: the end-of-block symbol and the last value get the longest code
    for longest in (17, 18, 20, 21, 23):
        one(f"len_longest{longest}", [complete_lengths(alpha, longest)] * 2, outside="len21_23" if longest > 20 else None)
    one("len_all23_but_two", [[1, 2] + [23] * (alpha - 2)] * 2, outside="len21_23")
    one("len_all20_but_two", [[1, 2] + [20] * (alpha - 2)] * 2)
    one("len_min1", [complete_lengths(alpha, 6)[::-1], complete_lengths(alpha, 6)])  # the first value's code is one bit long
    walk = list(flat)
    walk[3] = (1, 23, flat[3])
    one("len_walk_1_23", [walk, flat], outside="len21_23")
    walk20 = list(flat)
    walk20[3] = (1, 20, 1, flat[3])
    one("len_walk_1_20", [walk20, flat])
    for name, way in (("len_walk_to0", (0, 5)), ("len_walk_to24", (24, 5))):
        bad = list(flat)
        bad[7] = way
        one(name, [flat, bad])
    one("len_first0", [(0, [(1, 5)] + flat[1:]), flat])
    one("len_first24", [flat, (24, [(23, 5)] + flat[1:])])
    one("len_first31", [(31, flat), flat])
    # incomplete and over-subscribed sets, on alphabets of three and four
    one_col = b"\x07" * 5
    inc = dict(lengths=[[2, 2, 2]] * 2)  # codes 00, 01, 10: 11 is no code
    C.add(g, "incomplete_unused_not_sent", M.seal(1, [M.column_block(one_col, 0, **inc)]))
    C.add(g, "incomplete_unused_sent",
          M.seal(1, [M.column_block(one_col, 0, symbols=[RUNA, (0b11, 2), RUNA, 2], selectors=[0], **inc)]))
    # lengths 2, 2, 1, 1 (Kraft sum 1.5): both one-bit codes match, so only symbol 2 and end-of-block can be sent
    two = bytes([9, 8] * 6)  # used 8, 9: every byte is move-to-front index 1, symbol 2
    C.add(g, "oversubscribed", M.seal(1, [M.column_block(two, 0, lengths=[[2, 2, 1, 1]] * 2)]))
    C.add(g, "oversubscribed_23", M.seal(1, [M.column_block(two, 0, lengths=[[23, 23, 1, 1]] * 2)]), outside="len21_23")
    # table counts and selectors
    spine = complete_lengths(alpha, 20)
    for nt in (2, 3, 4, 5, 6):
        one(f"tables{nt}", [flat] + [[5] * alpha] * (nt - 2) + [spine[::-1]], ntables=nt, selectors=[0, nt - 1])
    col300 = column(300)
    rot = [flat[t:] + flat[:t] for t in range(0, 30, 5)]
    C.add(g, "tables6_selector_mtf_max", M.seal(1, [M.column_block(col300, 7, ntables=6, lengths=rot, selectors=[5, 4, 3, 2, 1, 0])]))
    one("sel_one_more", [flat, spine], selectors=[1, 0, 1])
    one("sel_18002", [flat, spine], selectors=[1, 0] + [1, 0] * 9000)
    one("sel_18003", [flat, spine], selectors=[1, 0] + [1, 0] * 9000 + [1])
    one("sel_one_too_few", [flat, spine], selectors=[1])
    one("sel_index_at_table_count", [flat, spine], selectors=[0, 0], selector_mtf=[0, 2])
    one("sel_index_at_table_count6", [flat] * 6, ntables=6, selectors=[0, 0], selector_mtf=[5, 6])
    for n in (50, 51):
        c = column(n)
        C.add(g, f"symbols{n}", M.seal(1, [M.column_block(c, n // 2, lengths=[flat, spine], selectors=[1, 0][:M.groups_of(range(n))])]))
    # alphabets
    C.add(g, "alpha_one_value", M.seal(1, [M.column_block(b"\x80" * 3, 2)]))
    all256 = list(range(256))
    C.add(g, "alpha_256_index255", M.seal(1, [M.column_block(b"", 30, used=all256, symbols=[256] * 59 + [257], selectors=[0, 1])]))
    none = dict(used=[], lengths=[[1, 1]] * 2, selectors=[0])
    C.add(g, "alpha_none_eob", M.seal(1, [M.column_block(b"", 0, symbols=[1], **none)]))
    C.add(g, "alpha_none_runa", M.seal(1, [M.column_block(b"", 0, symbols=[RUNA, 1], **none)]))
    C.add(g, "alpha_00_ff", M.seal(1, [M.column_block(bytes([0, 255, 255, 0, 0, 0, 255, 0, 255, 255, 255, 255, 0]), 4)]))


# ------------------------------------------------------------------ runs in the BWT column
def _runs(C):
    g = "runs"
    rng = random.Random(2)

    def col(prefix, run, tail):
        return _no_runs(rng, prefix, [1, 2, 3]) + b"\x00" * run + tail

    for run in (1023, 1024, 1025):
        # at offset 0; ending at the first and the second tile edge; starting one byte before a tile edge
        for prefix in sorted({0, TILE - run, 2 * TILE - run, TILE - 1} - {-1}):
            for tname, tail in (("eob", b""), ("sym", b"\x01")):
                C.add(g, f"run{run}_at{prefix}_{tname}", M.seal(1, [M.column_block(col(prefix, run, tail), prefix // 2, used=[0, 1, 2, 3])]))
    C.add(g, "two_runs_back_to_back", M.seal(1, [M.column_block(col(5, 1025, b"\x02") + b"\x00" * 1024 + b"\x01", 3, used=[0, 1, 2, 3])]))
    assert M.run_digits(1023) == [RUNA] * 10 and M.run_digits(2046) == [RUNB] * 10
    C.add(g, "run_all_runa_1023", M.seal(1, [M.column_block(b"\x05" * 1023 + b"\x06", 1000)]))  # the most RUNA digits a value can take
    C.add(g, "run_all_runb_2046", M.seal(1, [M.column_block(b"\x05" * 2046 + b"\x06", 1000)]))
    # a level-1 block filled to exactly 100000, and one byte past it
    C.add(g, "fill_100000_by_run", M.seal(1, [M.column_block(b"\x01" + b"\x00" * 99999, 50000)]))
    C.add(g, "fill_100000_by_symbol", M.seal(1, [M.column_block(b"\x00" * 99999 + b"\x01", 50000)]))
    C.add(g, "fill_100001_by_run", M.seal(1, [M.column_block(b"\x01" + b"\x00" * 100000, 50000)]))
    C.add(g, "fill_100001_by_symbol", M.seal(1, [M.column_block(b"\x00" * 100000 + b"\x01", 50000)]))
    # run counters that wrap: the Java adds and shifts ints
    tail = [2, RUNA, RUNA, 3, 4]  # used 1, 2: a symbol, a run of three, a symbol, the end
    for k in (31, 32, 33):
        sy = [RUNA] * k + tail
        C.add(g, f"run_wrap_{k}_digits", M.seal(1, [M.column_block(b"", 0, used=[1, 2, 3], symbols=sy, selectors=[0] * M.groups_of(sy))]),
              outside="run_wrap")
    digits = M.run_digits((1 << 31) + 5)
    assert len(digits) == 31
    sy = digits + [RUNA] + tail  # 2^31 + 5 + 2^31: five, as an int
    C.add(g, "run_wrap_to_5", M.seal(1, [M.column_block(b"", 0, used=[1, 2, 3], symbols=sy, selectors=[0])]), outside="run_wrap")


def _run900000(C):
    C.add("runs", "run_900000_level9", M.seal(9, [M.column_block(b"\x04" * 900000, 0)]))


# ------------------------------------------------------------------ columns that are no text's transform
def walk_columns(kc):
    """[(name, column)]: random columns over alphabets of 1, 2, 3 and 256 values."""
    rng = random.Random(3)
    out = []
    for n in (63, 64, 65, kc - 1, kc, kc + 1, 4 * kc + 7, 5000):
        for a in (1, 2, 3, 256):
            out.append((f"n{n}_a{a}", bytes(rng.randrange(a) * (255 // max(a - 1, 1)) if a < 256 else rng.randrange(256) for _ in range(n))))
    return out


def walk_starts(column, kc):
    """{label: start pointer} from the cycle decomposition of the column's permutation."""
    n = len(column)
    cyc = M.cycles(column)
    by_len = {}
    for c in cyc:
        by_len.setdefault(len(c), c)
    want = {}
    for ln in (1, 2, 63, 64, 65):
        if ln in by_len:
            want[f"cycle{ln}"] = by_len[ln][len(by_len[ln]) // 2]
    half = min(cyc, key=lambda c: abs(len(c) - n // 2))
    want["cycle_half"] = half[len(half) // 3]
    longest = max(cyc, key=len)
    want["cycle_longest"] = longest[-1]
    want["first"], want["last"] = 0, n - 1
    chains = min(n, kc)
    want["chain_start"] = (chains // 2) * n // chains
    want["after_chain_start"] = min(want["chain_start"] + 1, n - 1)
    seen, out = set(), {}
    for label, s in want.items():
        if s not in seen:
            seen.add(s)
            out[label] = s
    return out


def _walk(C, kc):
    g = "walk"
    for cname, column in walk_columns(kc):
        base = M.column_block(column, 0)
        for label, s in walk_starts(column, kc).items():
            b = replace(base, start=s)
            C.add_sealed(g, f"walk_{cname}_{label}", 1, [b])
            if label == "cycle_longest":
                b.crc ^= 1 << (s % 32)
                C.add(g, f"walk_{cname}_wrong_crc", M.write_stream(1, [b]), cap=C.out[-1].cap)
    for n in (1, 64, kc, 5000):  # the identity: every chain closes on itself
        C.add(g, f"walk_one_value_n{n}", M.seal(1, [M.column_block(b"\x5a" * n, n // 2)]))
        C.add(g, f"walk_one_value_n{n}_last", M.seal(1, [M.column_block(b"\x5a" * n, n - 1)]))


# ------------------------------------------------------------------ final stage and CRC fold
COUNTS = (0, 1, RLE_INLINE - 1, RLE_INLINE, RLE_INLINE + 1, 255)


def _filler(n):
    return (b"bcd" * (n // 3 + 1))[:n]  # no runs, no "a"


def _final(C):
    g = "final"
    for c in COUNTS:
        # source tiles: the fourth equal byte at pre-RLE offset e, its count byte at e + 1
        for e in (TILE - 2, TILE - 1, TILE, TILE + 1):
            pre = _filler(e - 3) + b"aaaa" + bytes([c]) + b"xyz"
            C.add(g, f"count{c}_fourth_at{e}", M.seal(1, [M.text_block(pre)]))
        # output tiles: the run fills the tile exactly, or overflows it by one, or by all of itself
        for over in sorted({0, 1, c}):
            if over > c:
                continue
            pre = _filler(TILE - 4 - c + over) + b"aaaa" + bytes([c]) + b"xyz"
            C.add(g, f"count{c}_overflow{over}", M.seal(1, [M.text_block(pre)]))
    # a block that ends right after four equal bytes, with no count byte
    for e in (3, TILE - 2, TILE - 1, TILE, TILE + 1):
        pre = _filler(e - 3) + b"aaaa"
        C.add(g, f"no_count_fourth_at{e}_last", M.seal(1, [M.text_block(pre)]))
        # the next block starts with the byte the run ended on
        C.add(g, f"no_count_fourth_at{e}_then_block", M.seal(1, [M.text_block(pre), M.text_block(b"aaa second block")]))
    # total outputs around the lanes' sixteen bytes and the tile: the last flush_out sees 0, 1 and 1024 bytes
    rng = random.Random(4)
    for n in (0, 1, 15, 16, 17, 1007, 1009, 1023, 1024, 1025, 1039, 1041, 2048, 2049):
        C.add(g, f"total{n}", bz2.compress(_no_runs(rng, n, list(range(97, 123))), 1))
    # 1024 after the final stage by way of a run: the last tile is exactly full, then nothing is left
    C.add(g, "total1024_by_run", bz2.compress(b"q" * 1000 + _no_runs(rng, 24, [1, 2, 3]), 1))


# ------------------------------------------------------------------ streams
@functools.lru_cache(maxsize=None)
def multi_block():
    """(blocks' texts, block specs, stream, bit positions of the block magics) of the 40-block stream.
    Every fifth block ends on three equal bytes and the next starts with three more of them;
    every block ends in a run symbol or not by chance, and uses its own set of byte values."""
    rng = random.Random(5)
    specs = []
    for i in range(40):
        n = 1 + (i * 37) % 300 if i else 1
        n = 300 if i == 39 else n
        values = rng.sample(range(256), rng.randrange(1, 6)) + [0x61]
        text = bytearray(rng.choice(values) for _ in range(n))
        if i % 3 == 1:
            text[n // 2:n // 2] = bytes([values[0]]) * rng.randrange(4, 300)
            del text[300:]
        pre = bytearray(M.rle1(bytes(text)))
        if i % 5 == 0:
            pre += b"\x62aaa"  # ends on three equal bytes; the next block starts with the same three
        elif i % 5 == 1:
            pre[:0] = b"aaa"
        specs.append(M.text_block(bytes(pre), ntables=2 + i % 5))
    positions = []
    stream = M.seal(1, specs, positions=positions)
    texts = []
    for b in specs:
        st, data, _ = M.decode(M.write_stream(1, [b]), 1 << 20)
        assert st == M.OK
        texts.append(data)
    return tuple(texts), tuple(specs), stream, tuple(positions)


def _streams(C):
    g = "streams"
    texts, specs, stream, positions = multi_block()
    total = sum(len(t) for t in texts)
    C.add(g, "blocks40", stream)
    for i, b in enumerate(specs):
        C.add(g, f"blocks40_block{i}_alone", M.write_stream(1, [b]))
    l0, l1 = len(texts[0]), len(texts[1])
    for name, cap in (("total_minus_1", total - 1), ("inside_block1", l0 + l1 // 2), ("inside_block2", l0 + l1 + 1), ("block_edge", l0 + l1),
                      ("zero", 0)):
        C.add(g, f"blocks40_cap_{name}", stream, cap=cap)
    C.add(g, "blocks40_tail", M.write_stream(1, list(specs), tail=b"BZh9 trailing bytes \x17\x72\x45"))
    C.add(g, "blocks40_pad_ones", M.write_stream(1, list(specs[:7]), pad_ones=True))
    C.add(g, "blocks40_pad_ones_tail", M.write_stream(1, list(specs[:6]), pad_ones=True, tail=b"\xff" * 5))
    C.add(g, "blocks40_wrong_stream_crc", M.write_stream(1, list(specs), stream_crc=0))
    C.add(g, "blocks40_cut_in_block33", stream[:positions[33] // 8 + 20])
    bad = list(specs)
    bad[35] = M.BlockSpec(**{**bad[35].__dict__, "crc": bad[35].crc ^ 0x8000})
    C.add(g, "blocks40_block35_wrong_crc", M.write_stream(1, bad))
    C.add(g, "no_blocks", M.write_stream(4, []))


@functools.lru_cache(maxsize=None)
def group(kc, name):
    """The cases of one group, built when first asked for."""
    C = _Cases()
    {"huffman": _huffman, "runs": _runs, "walk": lambda c: _walk(c, kc), "final": _final, "streams": _streams}[name](C)
    return tuple(C.out)


def cases(kc):
    return tuple(c for g in GROUPS for c in group(kc, g))


@functools.lru_cache(maxsize=None)
def big_case():
    """The one level-9 block of 900000 equal bytes written as one run, apart from the rest for its size."""
    C = _Cases()
    _run900000(C)
    return C.out[0]
