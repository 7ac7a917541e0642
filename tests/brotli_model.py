"""A Brotli decoder for the subset the project's encoder writes, written from RFC 7932 and from nothing in
netty_amd/csrc: one block type per category, NPOSTFIX = NDIRECT = 0, one literal and one distance tree, no static
dictionary.  Inside that subset it is complete (simple and complex prefix codes, every distance code 0-63,
uncompressed and metadata meta-blocks) and strict: anything outside it, a reserved bit, non-zero padding, a copy
past MLEN or a distance beyond the window raises BrotliError.  decode() returns (bytes, census); the census says
what the stream used, so tests can assert that the encoder still emits every feature."""

INSERT_BASE = [0, 1, 2, 3, 4, 5, 6, 8, 10, 14, 18, 26, 34, 50, 66, 98, 130, 194, 322, 578, 1090, 2114, 6210, 22594]
INSERT_EXTRA = [0, 0, 0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 7, 8, 9, 10, 12, 14, 24]
COPY_BASE = [2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 14, 18, 22, 30, 38, 54, 70, 102, 134, 198, 326, 582, 1094, 2118]
COPY_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 7, 8, 9, 10, 24]
# insert-and-copy symbol >> 6 -> (first insert code, first copy code); cells 0 and 1 imply distance code 0
CELLS = [(0, 0), (0, 8), (0, 0), (0, 8), (8, 0), (8, 8), (0, 16), (16, 0), (8, 16), (16, 8), (16, 16)]
CL_ORDER = [1, 2, 3, 4, 0, 5, 17, 6, 16, 7, 8, 9, 10, 11, 12, 13, 14, 15]


class BrotliError(Exception):
    pass


class Truncated(BrotliError):
    pass


class Bits:
    def __init__(self, data):
        self.d, self.pos = bytes(data), 0

    def bits(self, n):
        v = 0
        for i in range(n):
            if self.pos >= 8 * len(self.d):
                raise Truncated("the stream ends inside a meta-block")
            v |= ((self.d[self.pos >> 3] >> (self.pos & 7)) & 1) << i
            self.pos += 1
        return v

    def align(self):
        while self.pos & 7:
            if self.bits(1):
                raise BrotliError("non-zero padding bit")


class Code:
    """a prefix code from (symbol, length) pairs: canonical, by (length, symbol), read most significant bit first"""

    def __init__(self, lengths):
        used = sorted((l, s) for s, l in enumerate(lengths) if l)
        self.table, self.single = {}, None
        if len(used) == 1:
            self.single = used[0][1]
            return
        code, prev = 0, used[0][0]
        for l, s in used:
            code <<= l - prev
            prev = l
            self.table[(l, code)] = s
            code += 1
        if code != 1 << prev:
            raise BrotliError("prefix code is not complete")

    def read(self, br):
        if self.single is not None:
            return self.single
        code = 0
        for l in range(1, 16):
            code = (code << 1) | br.bits(1)
            s = self.table.get((l, code))
            if s is not None:
                return s
        raise BrotliError("no such code word")


def read_code(br, alphabet, census):
    hskip = br.bits(2)
    lengths = [0] * alphabet
    if hskip == 1:
        nsym = br.bits(2) + 1
        abits = (alphabet - 1).bit_length()
        syms = [br.bits(abits) for _ in range(nsym)]
        if len(set(syms)) != nsym or max(syms) >= alphabet:
            raise BrotliError("simple code symbols")
        shape = [[0], [1, 1], [1, 2, 2], None][nsym - 1]
        if nsym == 4:
            select = br.bits(1)
            shape = [1, 2, 3, 3] if select else [2, 2, 2, 2]
            census["tree_select"][select] += 1
        if nsym == 1:
            census["simple"][0] += 1
            lengths[syms[0]] = 1  # any length: a code of one symbol takes no bits
            return Code(lengths)
        for s, l in zip(syms, shape):
            lengths[s] = l
        census["simple"][nsym - 1] += 1
        census["max_code_length"] = max(census["max_code_length"], max(shape))
        return Code(lengths)
    cl = [0] * 18
    space, num = 32, 0
    for i in range(hskip, 18):
        x = br.bits(2)  # the fixed code of 0..5: 00, 0111, 011, 10, 01, 1111 read right to left
        v = {0: 0, 1: 4, 2: 3}.get(x)
        if v is None:
            v = 2 if br.bits(1) == 0 else (1 if br.bits(1) == 0 else 5)
        cl[CL_ORDER[i]] = v
        if v:
            space -= 32 >> v
            num += 1
            if space <= 0:
                break
    if not (num == 1 or space == 0):
        raise BrotliError("code-length code is not complete")
    clcode = Code(cl)
    i, prev, repeat, repeat_len, space = 0, 8, 0, 0, 32768
    while i < alphabet and space > 0:
        s = clcode.read(br)
        if s < 16:
            lengths[i] = s
            i += 1
            repeat = 0
            if s:
                prev = s
                space -= 32768 >> s
        else:
            extra = 2 if s == 16 else 3
            new_len = prev if s == 16 else 0
            if repeat_len != new_len:
                repeat, repeat_len = 0, new_len
            old = repeat
            if repeat > 0:
                repeat = (repeat - 2) << extra
            repeat += br.bits(extra) + 3
            delta = repeat - old
            if i + delta > alphabet:
                raise BrotliError("repeat past the alphabet")
            for k in range(delta):
                lengths[i + k] = new_len
            i += delta
            if new_len:
                space -= delta * (32768 >> new_len)
    if space != 0:
        raise BrotliError("prefix code is not complete")
    census["complex"] += 1
    census["max_code_length"] = max(census["max_code_length"], max(lengths))
    return Code(lengths)


def read_count(br):
    """the 1..256 variable-length code of NBLTYPES and NTREES"""
    if br.bits(1) == 0:
        return 1
    n = br.bits(3)
    return (1 << n) + 1 + br.bits(n)


def new_census():
    return {"compressed": 0, "uncompressed": 0, "metadata": 0, "simple": [0, 0, 0, 0], "tree_select": [0, 0], "complex": 0,
            "max_code_length": 0, "commands": 0, "literals": 0, "ring": 0, "implicit": 0, "continued": 0, "ignored_copy": 0,
            "max_distance": 0, "max_distance_code": 0, "window": 0, "lgwin": 0, "consumed": 0, "last": False}


def decode(data, allow_open_end=False):
    """(bytes, census).  allow_open_end: stop without error where the data ends at a meta-block boundary (a prefix
    of a handle's writes); otherwise the stream must reach its last meta-block."""
    br = Bits(data)
    census = new_census()
    if br.bits(1) == 0:
        lgwin = 16
    else:
        n = br.bits(3)
        if n:
            lgwin = 17 + n
        else:
            n = br.bits(3)
            if n == 1:
                raise BrotliError("large-window stream")
            lgwin = 17 if n == 0 else 8 + n
    census["lgwin"], census["window"] = lgwin, (1 << lgwin) - 16
    out = bytearray()
    ring = [4, 11, 15, 16]  # the last distance first
    while True:
        if allow_open_end and br.pos % 8 == 0 and br.pos == 8 * len(data):
            break
        last = br.bits(1)
        if last and br.bits(1):
            census["last"] = True
            break
        nib = br.bits(2)
        if nib == 3:
            if last:
                raise BrotliError("metadata in a last meta-block")
            if br.bits(1):
                raise BrotliError("reserved bit")
            skip_bytes = br.bits(2)
            skip = br.bits(8 * skip_bytes) + 1 if skip_bytes else 0
            if skip_bytes > 1 and (skip - 1) >> (8 * (skip_bytes - 1)) == 0:
                raise BrotliError("MSKIPLEN not minimal")
            br.align()
            if br.pos // 8 + skip > len(data):
                raise Truncated("metadata")
            br.pos += 8 * skip
            census["metadata"] += 1
            continue
        nib += 4
        mlen = br.bits(4 * nib) + 1
        if nib > 4 and (mlen - 1) >> (4 * (nib - 1)) == 0:
            raise BrotliError("MLEN not minimal")
        if not last and br.bits(1):
            br.align()
            at = br.pos // 8
            if at + mlen > len(data):
                raise Truncated("uncompressed meta-block")
            out += data[at:at + mlen]
            br.pos += 8 * mlen
            census["uncompressed"] += 1
            continue
        for what in "LID":
            if read_count(br) != 1:
                raise BrotliError("NBLTYPES%s > 1 is outside the subset" % what)
        if br.bits(2) != 0 or br.bits(4) != 0:
            raise BrotliError("NPOSTFIX / NDIRECT outside the subset")
        br.bits(2)  # the context mode of the one literal block type
        if read_count(br) != 1 or read_count(br) != 1:
            raise BrotliError("NTREES > 1 is outside the subset")
        lit, cmd, dist = read_code(br, 256, census), read_code(br, 704, census), read_code(br, 64, census)
        census["compressed"] += 1
        end, first = len(out) + mlen, True
        while len(out) < end:
            c = cmd.read(br)
            ibase, cbase = CELLS[c >> 6]
            icode, ccode = ibase + ((c >> 3) & 7), cbase + (c & 7)
            ins = INSERT_BASE[icode] + br.bits(INSERT_EXTRA[icode])
            cp = COPY_BASE[ccode] + br.bits(COPY_EXTRA[ccode])
            census["commands"] += 1
            if len(out) + ins > end:
                raise BrotliError("literals past MLEN")
            for _ in range(ins):
                out.append(lit.read(br))
            census["literals"] += ins
            if len(out) == end:
                census["ignored_copy"] += 1
                break
            if c < 128:
                dcode = 0
                census["implicit"] += 1
            else:
                dcode = dist.read(br)
                census["ring"] += dcode < 16
            if dcode < 16:
                d = ring[[0, 1, 2, 3, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1][dcode]] + [0, 0, 0, 0, -1, 1, -2, 2, -3, 3, -1, 1, -2, 2, -3, 3][dcode]
                if d <= 0:
                    raise BrotliError("distance <= 0")
            else:
                nb = 1 + ((dcode - 16) >> 1)
                d = ((2 + ((dcode - 16) & 1)) << nb) - 4 + br.bits(nb) + 1
            census["max_distance_code"] = max(census["max_distance_code"], dcode)
            if d > min(len(out), census["window"]):
                raise BrotliError("distance %d beyond min(position %d, window %d): a dictionary reference" % (d, len(out), census["window"]))
            if len(out) + cp > end:
                raise BrotliError("copy past MLEN")
            if first and ins == 0 and dcode == 0:
                census["continued"] += 1  # a meta-block that opens by going on with the last distance: a cut copy
            if dcode != 0:
                ring = [d] + ring[:3]
            census["max_distance"] = max(census["max_distance"], d)
            for _ in range(cp):
                out.append(out[-d])
            first = False
    if census["last"]:
        br.align()
    census["consumed"] = br.pos // 8
    return bytes(out), census
