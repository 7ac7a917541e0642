"""Seeded builders of VALID compressed streams that none of the project's encoders emits.

A decoder's contract is the format, not what one encoder writes.  Each builder here takes a list of
ops, ``literal(data, form)`` and ``copy(offset, length, form)``, and returns ``(stream, expected)``:
the stream in the codec's format, every op written in the form asked for, and the bytes it must
decode to.  The expected bytes come from `model()`, the obvious LZ77 byte loop below; it is the
plain reference of the decode tests and shares no code with ``oracle/`` or the kernels.

Formats (as their decoders read them):
  * Snappy block: varint preamble (padded up to Java's 4 bytes), literal codes 0-59 / 60-63 (a
    length may sit in a wider field than it needs), COPY_1 (length 4-11, offset 1-2047), COPY_2 and
    COPY_4 (length 1-64, any offset the field holds).
  * LZ4 block: token, 255-byte length extensions, offsets 1-65535, matches of 4 bytes and more;
    the block ends with a literal-only sequence.
  * LZF chunk body: literal runs 1-32, matches 3-8 (short) and 9-264 (long), distance 1-8192.
  * FastLZ level 1 / 2: literal runs 1-32 (the block starts with one), matches 3-8 (short), 9-264
    (level 1) or 9 and up (level 2, 255-byte extensions), distance 1-8192 (level 1), 1-8191 and the
    far form 8192-73727 (level 2).

The `*_sets()` functions build the named case sets that both tests/test_streamgen.py (CPU: builder
vs the oracle's decoders and, where present, libsnappy / liblz4) and tests/test_gpu_decode_grammar.py
(GPU) use; they are seeded and cached, so both see the same bytes.
"""
import functools
import random

# ------------------------------------------------------------------------------------------ ops


def literal(data, form=None):
    return ("L", bytes(data), form)


def copy(offset, length, form=None):
    return ("C", int(offset), int(length), form)


def model(ops) -> bytes:
    """What the ops decode to: literals appended, copies byte by byte from `offset` back."""
    out = bytearray()
    for op in ops:
        if op[0] == "L":
            out += op[1]
        else:
            _, off, ln, _ = op
            assert 1 <= off <= len(out) and ln >= 1, (off, ln, len(out))
            for _ in range(ln):
                out.append(out[-off])
    return bytes(out)


def _out_len(ops) -> int:
    return sum(len(op[1]) if op[0] == "L" else op[2] for op in ops)


def n_records(ops) -> int:
    """Records the GPU parsers emit for these ops: one per 64 output bytes of every op."""
    return sum((len(op[1]) + 63) // 64 if op[0] == "L" else (op[2] + 63) // 64 for op in ops)


# ------------------------------------------------------------------------------------------ Snappy


def _varint(v, pad=0):
    b = bytearray()
    while v >= 0x80:
        b.append((v & 0x7F) | 0x80)
        v >>= 7
    b.append(v)
    while len(b) < pad:  # non-minimal: continuation bits and zero groups
        b[-1] |= 0x80
        b.append(0)
    assert len(b) <= 4, "Java's readPreamble stops at 4 bytes"
    return bytes(b)


def snappy_literal_forms(n):
    """The literal codes that can carry a literal of n bytes (code < 60: the length itself)."""
    forms = [n - 1] if n <= 60 else []
    return forms + [60 + k for k in range(4) if n - 1 < 1 << (8 * (k + 1))]


def snappy_copy_forms(offset, length):
    forms = []
    if 4 <= length <= 11 and offset < 2048:
        forms.append(1)
    if length <= 64 and offset < 65536:
        forms.append(2)
    if length <= 64:
        forms.append(4)
    return forms


def snappy_op(op) -> bytes:
    if op[0] == "L":
        _, data, form = op
        n = len(data)
        assert n >= 1
        if form is None:
            form = snappy_literal_forms(n)[0]
        assert form == n - 1 if form < 60 else form <= 63 and n - 1 < 1 << (8 * (form - 59)), (n, form)
        if form < 60:
            return bytes([form << 2]) + data
        return bytes([form << 2]) + (n - 1).to_bytes(form - 59, "little") + data
    _, off, ln, form = op
    if form is None:
        form = snappy_copy_forms(off, ln)[0]
    assert 1 <= ln <= 64 and off >= 1 and (form == 4 or (form == 2 and off < 65536) or (form == 1 and 4 <= ln <= 11 and off < 2048)), op
    if form == 1:
        return bytes([1 | ((ln - 4) << 2) | ((off >> 8) << 5), off & 0xFF])
    if form == 2:
        return bytes([2 | ((ln - 1) << 2)]) + off.to_bytes(2, "little")
    return bytes([3 | ((ln - 1) << 2)]) + off.to_bytes(4, "little")


def snappy(ops, preamble_pad=0):
    want = model(ops)
    return _varint(len(want), preamble_pad) + b"".join(snappy_op(op) for op in ops), want


# ------------------------------------------------------------------------------------------ LZ4 block


def _lz4_ext(v):
    """The extension bytes of a length field whose nibble is 15 (v = length - 15 >= 0)."""
    return bytes([255]) * (v // 255) + bytes([v % 255])


def lz4(ops):
    """Consecutive literals join into one run; every copy closes a sequence (its literal run may be
    empty); the literals after the last copy, possibly none, are the block's last sequence."""
    out, lit = bytearray(), bytearray()

    def seq(match):
        ml = match[2] - 4 if match else 0
        out.append((min(len(lit), 15) << 4) | min(ml, 15))
        if len(lit) >= 15:
            out.extend(_lz4_ext(len(lit) - 15))
        out.extend(lit)
        if match:
            out.extend(match[1].to_bytes(2, "little"))
            if ml >= 15:
                out.extend(_lz4_ext(ml - 15))
        lit.clear()

    for op in ops:
        if op[0] == "L":
            lit += op[1]
        else:
            assert op[2] >= 4 and 1 <= op[1] <= 65535, op
            seq(op)
    seq(None)
    return bytes(out), model(ops)


# ------------------------------------------------------------------------------------------ LZF chunk body


def _runs32(data):
    for i in range(0, len(data), 32):
        yield data[i:i + 32]


def lzf(ops):
    out = bytearray()
    for op in ops:
        if op[0] == "L":
            for r in _runs32(op[1]):
                out.append(len(r) - 1)
                out += r
        else:
            _, off, ln, _ = op
            assert 3 <= ln <= 264 and 1 <= off <= 8192, op
            d = off - 1
            if ln <= 8:
                out += bytes([((ln - 2) << 5) | (d >> 8), d & 0xFF])
            else:
                out += bytes([(7 << 5) | (d >> 8), ln - 9, d & 0xFF])
    return bytes(out), model(ops)


# ------------------------------------------------------------------------------------------ FastLZ

FASTLZ_FAR = 8191  # level 2: a match this far back and beyond takes the far-distance form


def fastlz_max_offset(level):
    return 8192 if level == 1 else FASTLZ_FAR + 1 + 65535


def fastlz_max_length(level):
    return 264 if level == 1 else 1 << 20


def fastlz(ops, level):
    assert ops and ops[0][0] == "L", "a FastLZ block starts with a literal run"
    out = bytearray()
    for op in ops:
        if op[0] == "L":
            for r in _runs32(op[1]):
                out.append(len(r) - 1)
                out += r
            continue
        _, off, ln, _ = op
        assert 3 <= ln <= fastlz_max_length(level) and 1 <= off <= fastlz_max_offset(level), op
        far = level == 2 and off > FASTLZ_FAR
        d = FASTLZ_FAR if far else off - 1
        if ln <= 8:
            out.append(((ln - 2) << 5) | (d >> 8))
        else:
            out.append((7 << 5) | (d >> 8))
            ext = ln - 9
            if level == 1:
                out.append(ext)
            else:
                out += bytes([255]) * (ext // 255) + bytes([ext % 255])
        out.append(d & 0xFF)
        if far:
            out += (off - FASTLZ_FAR - 1).to_bytes(2, "big")
    out[0] |= (level - 1) << 5
    return bytes(out), model(ops)


# ------------------------------------------------------------------------------------------ case sets

# the offsets where the decoders change path: the output ring (2048 bytes, and the 4096 of the
# alternative build) bracketed by one 256-byte pass on either side, and the ends of the offset fields
RING_OFFSETS = list(range(1780, 2057)) + list(range(3830, 4105))
FIELD_OFFSETS = [8191, 8192, 32767, 32768, 65535]
HOT_OFFSETS = list(range(1, 69)) + RING_OFFSETS + FIELD_OFFSETS
SWEEP_LENGTHS = [1, 3, 4, 5, 63, 64]
SWEEP_K = [0, 1, 31, 62, 63, 64, 65]


def _rb(rng, n):
    return rng.randbytes(n)


def _phase_fill(rng, pos, phase, k=0):
    """A literal of 1-4 bytes after which, and after k more one-byte records, output position & 3 == phase."""
    n = (phase - k - pos - 1) % 4 + 1
    return literal(_rb(rng, n))


def _one_byte_records(rng, k, pos):
    """k records of one output byte each: literals and, once there is history, length-1 copies."""
    ops, data = [], _rb(rng, 2 * k)
    for i in range(k):
        if i % 3 == 2 and pos + i >= 70:
            ops.append(("C", 1 + data[i] % 70, 1, 2 + 2 * (data[k + i] & 1)))
        else:
            ops.append(("L", data[i:i + 1], (0, 0, 60, 61, 62, 63)[data[k + i] % 6]))
    return ops


def _snappy_walk(rng, total, hot=0.7):
    """Random ops of every form that decode to exactly `total` bytes."""
    ops, pos = [], 0
    while pos < total:
        room = total - pos
        if pos == 0 or rng.random() < 0.4:
            n = min(room, rng.choice((1, 1, 2, 3, 4, 5, 7, 8, 16, 59, 60, 61, 64, 65, 100, 255, 256, 257, 300, 1000)))
            n = rng.randint(1, n)
            ops.append(literal(_rb(rng, n), rng.choice(snappy_literal_forms(n))))
            pos += n
        else:
            if rng.random() < hot:
                cand = [o for o in (rng.choice(HOT_OFFSETS) for _ in range(4)) if o <= pos]
                off = cand[0] if cand else rng.randint(1, pos)
            else:
                off = rng.randint(1, pos)
            ln = min(room, rng.randint(1, 64))
            ops.append(copy(off, ln, rng.choice(snappy_copy_forms(off, ln))))
            pos += ln
    return ops


def _fill_input(rng, gap):
    """Literals whose encoded size is exactly `gap` bytes (0, or 2 and more)."""
    assert gap == 0 or gap >= 2, gap
    ops = []
    while gap:
        take = gap if gap <= 61 else (61 if gap - 61 >= 2 else gap - 2)
        ops.append(literal(_rb(rng, take - 1)))
        gap -= take
    return ops


def _enc_len(ops):
    return sum(len(snappy_op(op)) for op in ops)


@functools.lru_cache(maxsize=None)
def snappy_sets():
    """name -> list of (stream, expected).  Every frame but the ones of `large` holds at most
    65536 bytes and fewer than 16384 records (so the record path, not its fallback, decodes it)."""
    sets = {}

    # overlap grid: offset 1..68 x length 1..64 x COPY_2 / COPY_4 (/ COPY_1) x output phase 0..3
    rng = random.Random(0x5A01)
    grid = []
    for off in range(1, 69):
        for phase in range(4):
            ops, pos = [literal(_rb(rng, 68))], 68
            for ln in range(1, 65):
                for form in (1, 2, 4):
                    if form not in snappy_copy_forms(off, ln):
                        continue
                    f = _phase_fill(rng, pos, phase)
                    ops += [f, copy(off, ln, form)]
                    pos += len(f[1]) + ln
            grid.append(snappy(ops))
    sets["overlap_grid"] = grid

    # ring boundary sweep: every offset around the ring sizes, random history, k one-byte records first
    rng = random.Random(0x5A02)
    sweep = []
    def sweep_items(ops, pos, chunk, ln, phase, k):
        for off in chunk:
            f = _phase_fill(rng, pos, phase, k)
            pos += len(f[1])
            ops.append(f)
            ops += _one_byte_records(rng, k, pos)
            pos += k
            ops.append(copy(off, ln, rng.choice(snappy_copy_forms(off, ln))))
            pos += ln
        return pos

    for ln in SWEEP_LENGTHS:
        for phase in range(4):
            for k in SWEEP_K:
                per = max(1, 6000 // (k + 2))
                for i in range(0, len(RING_OFFSETS), per):
                    chunk = RING_OFFSETS[i:i + per]
                    hist = max(chunk) + rng.randint(0, 300)
                    ops = _snappy_walk(rng, hist, hot=0.2)
                    pos = sweep_items(ops, hist, chunk, ln, phase, k)
                    assert pos <= 65536 and n_records(ops) < 16384
                    sweep.append(snappy(ops))
            # the ends of the offset fields (65535 needs a frame above 64 KiB: in `large`), every k in one frame
            hist = 32768 + rng.randint(0, 300)
            ops, pos = [literal(_rb(rng, hist), 62)], hist
            for k in SWEEP_K:
                pos = sweep_items(ops, pos, FIELD_OFFSETS[:4], ln, phase, k)
            assert pos <= 65536 and n_records(ops) < 16384
            sweep.append(snappy(ops))
    sets["ring_sweep"] = sweep

    # flush and stage edges
    rng = random.Random(0x5A03)
    edges = []
    for j in (1, 2, 3, 4, 5, 8):  # output: an op ending at 512 j - 1, 512 j, 512 j + 1
        for d in (-1, 0, 1):
            for ln in (1, 4, 9, 64):
                for kind in "LCF":
                    T = 512 * j + d
                    ops = _snappy_walk(rng, T - ln)
                    if kind == "L":
                        ops.append(literal(_rb(rng, ln), rng.choice(snappy_literal_forms(ln))))
                    else:
                        off = rng.choice([o for o in (1, 3, 60, 200, T - ln) if o <= T - ln])
                        ops.append(copy(off, ln, rng.choice(snappy_copy_forms(off, ln))))
                    if kind != "F":  # "F": the copy is the frame's last op
                        ops += _snappy_walk(rng, rng.randint(1, 40))
                    edges.append(snappy(ops))
    for unit in (512, 1024):  # input: a tag ending at unit j - 1, unit j, unit j + 1 (3-byte preamble)
        for j in (1, 2, 3):
            for d in (-1, 0, 1):
                for kind in ("L1", "L9", "C2", "C4", "C1"):
                    T = unit * j + d
                    ops = [literal(_rb(rng, 300), 61)]  # 3 + 300 input bytes
                    last = {"L1": literal(_rb(rng, 1)), "L9": literal(_rb(rng, 9), 61), "C2": copy(250, 7, 2),
                            "C4": copy(2, 33, 4), "C1": copy(299, 11, 1)}[kind]
                    ops += _fill_input(rng, T - 3 - _enc_len(ops) - _enc_len([last]))
                    ops.append(last)
                    assert 3 + _enc_len(ops) == T
                    edges.append(snappy(ops + _snappy_walk(rng, 30), preamble_pad=3))
                    if d == 0:  # and as the frame's last tag
                        edges.append(snappy(ops, preamble_pad=3))
    for total in (7, 8, 9, 511, 512, 513, 2047, 2048, 2049, 4096, 65536):
        for _ in range(3):
            edges.append(snappy(_snappy_walk(rng, total), preamble_pad=rng.choice((0, 0, 3, 4))))
    sets["edges"] = edges

    # dependency chains: back-to-back copies of 4 bytes, every piece waiting for the one before
    rng = random.Random(0x5A04)
    chains = []
    for off in (1, 2, 3, 4, 5, 8, 60, 63, 64):
        for phase in range(4):
            for form in (1, 2, 4):
                n = rng.choice((70, 128, 129, 200))
                chains.append(snappy([literal(_rb(rng, 64 + phase))] + [copy(off, 4, form)] * n))
    sets["chains"] = chains

    # tag-window straddles: multi-byte tags starting at input byte 59..64 mod 64
    rng = random.Random(0x5A05)
    strad = []
    tags = [copy(70, 9, 4), copy(100, 64, 4), copy(90, 5, 2), literal(_rb(rng, 7), 60), literal(_rb(rng, 9), 61),
            literal(_rb(rng, 61), 62), literal(_rb(rng, 5), 63)]
    for base in (128, 448, 512, 960, 1024, 2048):
        for start in range(59, 65):
            for tag in tags:
                ops = [literal(_rb(rng, 120), 60)]  # with the 3-byte preamble: 3 + 2 + 120 input bytes
                ops += _fill_input(rng, base + start - 3 - _enc_len(ops))
                assert 3 + _enc_len(ops) == base + start  # the tag starts at input byte `start` mod 64
                ops += [tag] * 3 + _snappy_walk(rng, 50)
                strad.append(snappy(ops, preamble_pad=3))
    sets["straddles"] = strad

    # mixed random walk
    rng = random.Random(0x5A06)
    sets["walk"] = [snappy(_snappy_walk(rng, rng.choice((rng.randint(100, 2000), rng.randint(100, 20000)))),
                           preamble_pad=rng.choice((0, 0, 0, 2, 3, 4))) for _ in range(200)]

    # large out_cap: output above 65536 bytes, COPY_4 offsets 65535 / 65536 / 65537 / output - 1; the
    # last frame has more than 16384 records (the pair path hands it to the fused decoder)
    rng = random.Random(0x5A07)
    large = []
    for total in (65537, 70000, 200000, 1200000 + 11):
        if total == 65537:
            ops = [literal(_rb(rng, 65500), 62), literal(_rb(rng, 35)), copy(65535, 1, 4), copy(65536, 1, 4)]
        else:
            ops, pos = [literal(_rb(rng, 65537), 63)], 65537
            for off in (65535, 65536, 65537):
                for ln in SWEEP_LENGTHS:
                    for phase in range(4):
                        for k in (0, 1, 63):
                            if total == 70000 and (k == 63 or off == 65535):
                                continue  # (the 70 000-byte frame has no room for all of them)
                            f = _phase_fill(rng, pos, phase, k)
                            ops += [f] + _one_byte_records(rng, k, pos + len(f[1]))
                            ops.append(copy(off, ln, 4 if off > 65535 else rng.choice((2, 4))))
                            pos += len(f[1]) + k + ln
            if total == 200000:  # the ring sweep's offset 65535, at every length, phase and k
                for ln in SWEEP_LENGTHS:
                    for phase in range(4):
                        for k in SWEEP_K:
                            f = _phase_fill(rng, pos, phase, k)
                            ops += [f] + _one_byte_records(rng, k, pos + len(f[1])) + [copy(65535, ln, rng.choice((2, 4)))]
                            pos += len(f[1]) + k + ln
            while pos < total - 400:
                if total > 1000000 and rng.random() < 0.8:  # short ops: many records
                    n = rng.randint(1, 3)
                    if rng.random() < 0.5:
                        ops.append(literal(_rb(rng, n), rng.choice(snappy_literal_forms(n))))
                    else:
                        ops.append(copy(rng.choice([o for o in (1, 2, 5, 2047, 2048, 2049, 65536, 100000, pos) if o <= pos]), n, 4))
                elif rng.random() < 0.7:
                    n = rng.randint(1, 64)
                    ops.append(copy(rng.choice([o for o in (pos, pos - 1, 65535, 65536, 65537, 99999, rng.randint(1, pos)) if o <= pos]), n, 4))
                else:
                    n = rng.randint(1, 320)
                    ops.append(literal(_rb(rng, n), 63))
                pos += n
            if total > 1000000:
                assert n_records(ops) > 16384
            ops.append(literal(_rb(rng, total - pos - 1)))
            ops.append(copy(total - 1, 1, 4))  # offset = output - 1: the frame's first byte
        s, w = snappy(ops)
        assert len(w) == total, (len(w), total)
        large.append((s, w))
    sets["large"] = large
    return sets


# -------- LZ4 / LZF / FastLZ: the same ideas scaled to each format

ALT_LONG = [65, 127, 128, 129, 264, 1000, 5000]
ALT_LONG_OFFSETS = [1, 63, 64, 65, 70, 300, 2049]


class _Alt:
    def __init__(self, name, build, minlen, maxlen, maxoff, lit_split, first_literal):
        self.name, self.build, self.minlen, self.maxlen, self.maxoff = name, build, minlen, maxlen, maxoff
        self.lit_split = lit_split  # literal runs are cut at this many bytes (None: length extensions)
        self.first_literal = first_literal


ALT = {
    "lz4": _Alt("lz4", lz4, 4, 1 << 20, 65535, None, False),
    "lzf": _Alt("lzf", lzf, 3, 264, 8192, 32, False),
    "fastlz1": _Alt("fastlz1", lambda ops: fastlz(ops, 1), 3, 264, 8192, 32, True),
    "fastlz2": _Alt("fastlz2", lambda ops: fastlz(ops, 2), 3, 1 << 20, 8192 + 65535, 32, True),
}

LZ4_TAIL = 12  # liblz4 takes a block only if it ends with literals and no earlier run ends within 12 bytes of the output's end


def _alt_finish(c, rng, ops):
    if c.name == "lz4":
        ops = ops + [literal(_rb(rng, LZ4_TAIL))]
    return c.build(ops)


def _alt_walk(c, rng, total, hot=0.7):
    ops, pos = [], 0
    hot_offsets = [o for o in HOT_OFFSETS + [c.maxoff, c.maxoff - 1, 8190, 8191, 8192, 8193] if o <= c.maxoff]
    while pos < total:
        if pos == 0 or rng.random() < 0.4:
            n = rng.randint(1, rng.choice((1, 2, 4, 14, 15, 16, 31, 32, 33, 64, 65, 270, 300)))
            ops.append(literal(_rb(rng, n)))
        else:
            off = rng.choice(hot_offsets) if rng.random() < hot else rng.randint(1, min(pos, c.maxoff))
            if off > pos:
                off = rng.randint(1, min(pos, c.maxoff))
            n = rng.randint(c.minlen, min(c.maxlen, rng.choice((8, 9, 18, 19, 20, 64, 65, 130, 264, 300, 700))))
            ops.append(copy(off, n))
        pos += n
    return ops


@functools.lru_cache(maxsize=None)
def alt_sets(name):
    """name of a codec of ALT -> {set name: list of (stream, expected)}."""
    c = ALT[name]
    sets = {}
    seed = {"lz4": 0x1400, "lzf": 0x1F00, "fastlz1": 0xF100, "fastlz2": 0xF200}[name]

    # overlap grid: offset 1..68 x every length up to 64 (and the first long ones) x output phase
    rng = random.Random(seed + 1)
    grid = []
    for off in range(1, 69):
        for phase in range(4):
            ops, pos = [literal(_rb(rng, 68))], 68
            for ln in list(range(c.minlen, 65)) + [65, 66, 67, 68, 69, 127, 128, 129]:
                f = _phase_fill(rng, pos, phase)
                ops += [f, copy(off, ln)]
                pos += len(f[1]) + ln
            grid.append(_alt_finish(c, rng, ops))
    sets["overlap_grid"] = grid

    # offset sweep around the ring sizes and at the ends of each offset form
    rng = random.Random(seed + 2)
    sweep = []
    field = sorted({o for o in (8190, 8191, 8192, 8193, 8194, 32767, 32768, 65535, c.maxoff - 1, c.maxoff) if o <= c.maxoff})
    kb1 = 1 + (c.minlen if c.name == "lz4" else 0)  # output bytes of one short record (LZ4: a literal closed by a minimum match)

    def sweep_items(ops, pos, chunk, ln, phase, k):
        for off in chunk:
            f = _phase_fill(rng, pos, phase, k * kb1)
            ops.append(f)
            pos += len(f[1])
            for _ in range(k):
                ops.append(literal(_rb(rng, 1)))
                if c.name == "lz4":
                    ops.append(copy(rng.randint(1, 64), c.minlen))
            ops.append(copy(off, ln))
            pos += k * kb1 + ln
        return pos

    for ln in (c.minlen, c.minlen + 1, 8, 9, 63, 64, 65):
        for phase in range(4):
            for k in (0, 1, 63):
                per = max(1, 6000 // (2 * k + 3))
                for i in range(0, len(RING_OFFSETS), per):
                    chunk = RING_OFFSETS[i:i + per]
                    ops = _alt_walk(c, rng, max(chunk) + rng.randint(0, 200), hot=0.2)
                    sweep_items(ops, _out_len(ops), chunk, ln, phase, k)
                    assert n_records(ops) < 16384
                    sweep.append(_alt_finish(c, rng, ops))
            hist = max(field) + rng.randint(0, 200)
            ops, pos = [literal(_rb(rng, hist))], hist
            for k in (0, 1, 63):
                pos = sweep_items(ops, pos, field, ln, phase, k)
            assert n_records(ops) < 16384
            sweep.append(_alt_finish(c, rng, ops))
    sets["offset_sweep"] = sweep

    # long matches: a record of a split match copies what the records before it produced
    rng = random.Random(seed + 3)
    longs = []
    for off in ALT_LONG_OFFSETS:
        for phase in range(4):
            ops, pos = [literal(_rb(rng, 2049))], 2049
            for ln in ALT_LONG:
                if ln > c.maxlen:
                    continue
                f = _phase_fill(rng, pos, phase)
                ops += [f, copy(off, ln)]
                pos += len(f[1]) + ln
            longs.append(_alt_finish(c, rng, ops))
    sets["long_matches"] = longs

    # length-extension edges
    rng = random.Random(seed + 4)
    ext = []
    if c.name == "lz4":
        vals = [14, 15, 16, 15 + 254, 15 + 255, 15 + 256, 19 + 254, 19 + 255, 19 + 256, 15 + 510, 15 + 511, 19 + 510, 15 + 765, 19 + 765]
        lit_lens, match_lens = [0, 1] + vals, [4, 5, 18] + vals + [v + 4 for v in vals]
    else:
        lit_lens = [1, 2, 31, 32, 33, 63, 64, 65, 96, 97]
        match_lens = [m for m in (3, 4, 7, 8, 9, 10, 263, 264, 265, 9 + 254, 9 + 255, 9 + 256, 9 + 510, 9 + 511, 9 + 765, 5000)
                      if m <= c.maxlen]
    for off in (1, 2, 7, 64, 301):
        ops = [literal(_rb(rng, 400))]
        for n in lit_lens:
            for m in (match_lens[0], match_lens[-1]):
                ops += ([literal(_rb(rng, n))] if n else []) + [copy(off, m)]
        for m in match_lens:
            for n in (lit_lens[0], 1, lit_lens[-1]):
                ops += ([literal(_rb(rng, n))] if n else []) + [copy(off, m)]
        ext.append(_alt_finish(c, rng, ops))
    if c.name == "lz4":  # how a block may end: a last sequence with no literals, one, or a few
        for tail in (0, 1, 4, 5, 11):
            ops = [literal(_rb(rng, 40)), copy(13, 20)] + ([literal(_rb(rng, tail))] if tail else [])
            sets.setdefault("lz4_short_tails", []).append(c.build(ops))
    sets["length_edges"] = ext

    # mixed random walk
    rng = random.Random(seed + 5)
    sets["walk"] = [_alt_finish(c, rng, _alt_walk(c, rng, rng.choice((rng.randint(100, 2000), rng.randint(100, 20000)))))
                    for _ in range(100)]

    # more than 16384 records: the block goes to the codec's lane-serial decoder
    rng = random.Random(seed + 6)
    many = []
    for _ in range(2):
        ops, pos = [literal(_rb(rng, 100))], 100
        while len(ops) <= 16384 + 100:  # every op here is one record
            ops += [literal(_rb(rng, rng.randint(1, 3))), copy(rng.choice((1, 2, 3, 64, 99, min(pos, 2049))), rng.randint(c.minlen, 9))]
            pos += len(ops[-2][1]) + ops[-1][2]
        assert n_records(ops) > 16384
        many.append(_alt_finish(c, rng, ops))
    sets["many_records"] = many
    return sets
