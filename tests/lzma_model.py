"""A pure-Python decoder of the LZMA "alone" container (13 header bytes and an LZMA payload), written from the
format's specification for the tests: any lc, lp, pb, and the checks lzma-java's decoder makes.  decode()
returns the bytes and the packet list; it raises LzmaError where the stream is not a valid one that ends
exactly at its last byte."""

LIT, MATCHED_LIT, MATCH, SHORT_REP, REP0, REP1, REP2, REP3, END_MARKER = (
    "lit", "matched_lit", "match", "short_rep", "rep0", "rep1", "rep2", "rep3", "end_marker")


class LzmaError(Exception):
    pass


class _Rc:
    def __init__(self, data, pos):
        self.d, self.p = data, pos
        if len(data) < pos + 5:
            raise LzmaError("truncated: the range coder's first five bytes")
        if data[pos] != 0:
            raise LzmaError("the payload's first byte is not 0")
        self.code = int.from_bytes(data[pos + 1:pos + 5], "big")
        self.range = 0xFFFFFFFF
        self.p = pos + 5

    def _norm(self):
        if self.range < (1 << 24):
            if self.p >= len(self.d):
                raise LzmaError("truncated payload")
            self.range = (self.range << 8) & 0xFFFFFFFF
            self.code = ((self.code << 8) | self.d[self.p]) & 0xFFFFFFFF
            self.p += 1

    def bit(self, probs, i):
        self._norm()
        v = probs[i]
        bound = (self.range >> 11) * v
        if self.code < bound:
            self.range = bound
            probs[i] = v + ((2048 - v) >> 5)
            return 0
        self.code -= bound
        self.range -= bound
        probs[i] = v - (v >> 5)
        return 1

    def direct(self, n):
        r = 0
        for _ in range(n):
            self._norm()
            self.range >>= 1
            b = 1 if self.code >= self.range else 0
            if b:
                self.code -= self.range
            r = (r << 1) | b
        return r

    def tree(self, probs, base, n):
        m = 1
        for _ in range(n):
            m = (m << 1) | self.bit(probs, base + m)
        return m - (1 << n)

    def rtree(self, probs, base, n):
        m, r = 1, 0
        for i in range(n):
            b = self.bit(probs, base + m)
            m = (m << 1) | b
            r |= b << i
        return r


def _len(rc, p, base, ps):
    # {choice, choice2, low[16][8], mid[16][8], high[256]}
    if rc.bit(p, base) == 0:
        return 2 + rc.tree(p, base + 2 + ps * 8, 3)
    if rc.bit(p, base + 1) == 0:
        return 10 + rc.tree(p, base + 2 + 128 + ps * 8, 3)
    return 18 + rc.tree(p, base + 2 + 256, 8)


def parse_header(stream):
    if len(stream) < 13:
        raise LzmaError("truncated header")
    props = stream[0]
    if props >= 9 * 5 * 5:
        raise LzmaError("properties byte out of range")
    lc, lp, pb = props % 9, props // 9 % 5, props // 45
    return lc, lp, pb, int.from_bytes(stream[1:5], "little"), int.from_bytes(stream[5:13], "little")


def decode(stream):
    """(bytes, packets) of one stream; packets are (kind, length, distance) with distance 0 for literals."""
    stream = bytes(stream)
    lc, lp, pb, dict_size, size = parse_header(stream)
    known = size != 0xFFFFFFFFFFFFFFFF
    window = max(dict_size, 1)
    # one flat model; the offsets are this file's own
    IS_MATCH, IS_REP, G0, G1, G2, REP0_LONG = 0, 192, 204, 216, 228, 240
    POS_SLOT, SPEC, ALIGN, LEN, REP_LEN, LITERAL = 432, 688, 816, 832, 1346, 1860
    p = [1024] * (LITERAL + (0x300 << (lc + lp)))
    rc = _Rc(stream, 13)
    out = bytearray()
    packets = []
    state, rep = 0, [0, 0, 0, 0]
    ended = False

    def check_dist(d0):
        if d0 >= len(out) or d0 >= window:
            raise LzmaError("distance %d beyond the %d bytes produced or the dictionary of %d" % (d0 + 1, len(out), window))

    def copy(d0, n):
        if known and len(out) + n > size:
            raise LzmaError("a match runs past the stated length")
        for _ in range(n):
            out.append(out[-d0 - 1])

    while True:
        if known and len(out) == size:
            # the end marker may still follow: it does iff bytes remain once the coder has normalised
            saved = (rc.range, rc.code, rc.p)
            rc._norm()
            if rc.p == len(stream):
                break
            rc.range, rc.code, rc.p = saved
        ps = len(out) & ((1 << pb) - 1)
        if rc.bit(p, IS_MATCH + (state << 4) + ps) == 0:
            if known and len(out) >= size:
                raise LzmaError("a literal past the stated length")
            prev = out[-1] if out else 0
            base = LITERAL + 0x300 * (((len(out) & ((1 << lp) - 1)) << lc) + (prev >> (8 - lc)))
            sym = 1
            if state >= 7:
                mb = out[-rep[0] - 1]
                while sym < 0x100:
                    mbit = (mb >> 7) & 1
                    mb = (mb << 1) & 0xFF
                    b = rc.bit(p, base + ((1 + mbit) << 8) + sym)
                    sym = (sym << 1) | b
                    if mbit != b:
                        break
            while sym < 0x100:
                sym = (sym << 1) | rc.bit(p, base + sym)
            out.append(sym & 0xFF)
            packets.append((MATCHED_LIT if state >= 7 else LIT, 1, 0))
            state = 0 if state < 4 else state - 3 if state < 10 else state - 6
            continue
        if rc.bit(p, IS_REP + state) == 0:
            n = _len(rc, p, LEN, ps)
            state = 7 if state < 7 else 10
            slot = rc.tree(p, POS_SLOT + min(n - 2, 3) * 64, 6)
            d0 = slot
            if slot >= 4:
                fb = (slot >> 1) - 1
                d0 = (2 | (slot & 1)) << fb
                if slot < 14:
                    d0 += rc.rtree(p, SPEC + d0 - slot - 1, fb)
                else:
                    d0 += rc.direct(fb - 4) << 4
                    d0 += rc.rtree(p, ALIGN, 4)
            if d0 == 0xFFFFFFFF:
                packets.append((END_MARKER, n, 0))
                ended = True
                break
            rep = [d0, rep[0], rep[1], rep[2]]
            check_dist(d0)
            copy(d0, n)
            packets.append((MATCH, n, d0 + 1))
            continue
        if not out:
            raise LzmaError("a rep match with nothing produced")
        if rc.bit(p, G0 + state) == 0:
            if rc.bit(p, REP0_LONG + (state << 4) + ps) == 0:
                check_dist(rep[0])
                state = 9 if state < 7 else 11
                copy(rep[0], 1)
                packets.append((SHORT_REP, 1, rep[0] + 1))
                continue
            idx = 0
        else:
            if rc.bit(p, G1 + state) == 0:
                idx = 1
            else:
                idx = 2 + rc.bit(p, G2 + state)
            d = rep.pop(idx)
            rep.insert(0, d)
        n = _len(rc, p, REP_LEN, ps)
        state = 8 if state < 7 else 11
        check_dist(rep[0])
        copy(rep[0], n)
        packets.append(((REP0, REP1, REP2, REP3)[idx], n, rep[0] + 1))
    if known and len(out) != size:
        raise LzmaError("the stream ends after %d of %d bytes" % (len(out), size))
    if not known and not ended:
        raise LzmaError("no end marker in a stream of unknown length")
    rc._norm()  # the decoder normalises once more after the last packet (lzma-java, liblzma)
    if rc.code != 0:
        raise LzmaError("the range coder's code word is not zero at the end")
    if rc.p != len(stream):
        raise LzmaError("the stream ends at byte %d of %d" % (rc.p, len(stream)))
    return bytes(out), packets
