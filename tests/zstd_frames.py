"""A reader of Zstandard frame structure for the tests: frame header, block headers, the literals-section
header, the first byte of a Huffman tree description and the sequences header.  With entropy=True also
the FSE distributions (accuracy log, probabilities, zero-run flags), the form and size of a tree description
and where each bitstream ends.  It decodes no bitstream; sizes it parses must add up, and it raises
ValueError where they cannot."""
from dataclasses import dataclass, field

MAGIC = b"\x28\xb5\x2f\xfd"
RAW, RLE, COMPRESSED = 0, 1, 2
LIT_RAW, LIT_RLE, LIT_COMPRESSED, LIT_TREELESS = 0, 1, 2, 3
SEQ_PREDEFINED, SEQ_RLE, SEQ_FSE, SEQ_REPEAT = 0, 1, 2, 3


@dataclass
class Block:
    last: bool
    type: int
    size: int            # Block_Size: the content's bytes, or the regenerated size of an RLE block
    content: int         # bytes the block occupies after its header
    lit_type: int = None
    lit_format: int = None
    lit_header: int = None
    lit_regen: int = None
    lit_comp: int = None  # bytes after the literals header (Raw: regen, RLE: 1)
    lit_streams: int = None
    tree: str = None      # 'direct' or 'fse' (Compressed literals only)
    tree_byte: int = None
    nseq: int = None
    seq_header: int = None
    modes: tuple = None   # (literal lengths, offsets, match lengths)
    # with entropy=True:
    tree_weights: int = None   # direct weights: how many are sent
    tree_dist: object = None   # FSE-compressed weights: their Dist
    tree_bytes: int = None     # the whole description (0 for Treeless)
    weights_end: int = None    # FSE-compressed weights: the last byte of their bitstream
    stream_ends: list = None   # the last byte of each literals stream
    dists: dict = None         # which -> Dist, for the codes in FSE mode
    rle_syms: dict = None      # which -> symbol, for the codes in RLE mode
    seq_end: int = None        # the last byte of the sequence bitstream
    tables: list = None        # (start, end) in the input of the tree description, the jump table and every code's table


@dataclass
class Dist:
    log: int
    probs: list       # -1 = "less than 1"
    flags: list       # one tuple of 2-bit repeat flags per probability 0 read
    size: int         # bytes

    @property
    def minus(self):
        return sum(p == -1 for p in self.probs)

    @property
    def top(self):
        return len(self.probs) - 1


def read_distribution(b, p, end, max_syms):
    """the FSE distribution at b[p:end): RFC 8878 4.1.1"""
    at = 0

    def take(k):
        nonlocal at
        if p * 8 + at + k > end * 8:
            raise ValueError("distribution runs past its section")
        v = (int.from_bytes(b[p:end], "little") >> at) & ((1 << k) - 1)
        at += k
        return v

    log = take(4) + 5
    left, probs, flags = 1 << log, [], []
    while left > 0:
        if len(probs) >= max_syms:
            raise ValueError("more symbols than the alphabet")
        width = (left + 1).bit_length()          # left + 2 values in `width` bits, the lowest ones in one fewer
        spare = (1 << width) - (left + 2)
        v = take(width - 1)
        if v >= spare:
            v |= take(1) << (width - 1)
            if v >= 1 << (width - 1):
                v -= spare
        left -= abs(v - 1)
        if left < 0:
            raise ValueError("probabilities above the table size")
        probs.append(v - 1)
        if v == 1:
            chain = []
            while True:
                chain.append(take(2))
                probs += [0] * chain[-1]
                if chain[-1] != 3:
                    break
            flags.append(tuple(chain))
    if len(probs) > max_syms:
        raise ValueError("more symbols than the alphabet")
    return Dist(log, probs, flags, (at + 7) // 8)


@dataclass
class Frame:
    start: int
    end: int
    header: int
    single_segment: bool
    window_descriptor: int   # None when Single_Segment
    dict_id: int
    content_size: int        # None when absent
    fcs_bytes: int
    checksum: bool
    blocks: list = field(default_factory=list)


def _le(b, p, n):
    if p + n > len(b):
        raise ValueError("truncated")
    return int.from_bytes(b[p:p + n], "little")


def parse_compressed_block(b, p, size, blk, entropy=False):
    end = p + size
    b0 = _le(b, p, 1)
    blk.lit_type, blk.lit_format = b0 & 3, (b0 >> 2) & 3
    if blk.lit_type in (LIT_RAW, LIT_RLE):
        h = {0: 1, 2: 1, 1: 2, 3: 3}[blk.lit_format]
        v = _le(b, p, h)
        blk.lit_regen = v >> 3 if h == 1 else v >> 4
        blk.lit_comp = blk.lit_regen if blk.lit_type == LIT_RAW else 1
        blk.lit_streams = 0
    else:
        h = {0: 3, 1: 3, 2: 4, 3: 5}[blk.lit_format]
        bits = {0: 10, 1: 10, 2: 14, 3: 18}[blk.lit_format]
        v = _le(b, p, h) >> 4
        blk.lit_regen, blk.lit_comp = v & ((1 << bits) - 1), v >> bits
        blk.lit_streams = 1 if blk.lit_format == 0 else 4
        if blk.lit_type == LIT_COMPRESSED:
            blk.tree_byte = _le(b, p + h, 1)
            blk.tree = "fse" if blk.tree_byte < 128 else "direct"
    blk.lit_header = h
    q = p + h + blk.lit_comp
    if q > end:
        raise ValueError("literals section runs past its block")
    if entropy and blk.lit_type >= LIT_COMPRESSED:
        t = p + h
        blk.tree_bytes, blk.tables = 0, []
        if blk.tree == "direct":
            blk.tree_weights = blk.tree_byte - 127
            blk.tree_bytes = 1 + (blk.tree_weights + 1) // 2
        elif blk.tree == "fse":
            blk.tree_bytes = 1 + blk.tree_byte
            blk.tree_dist = read_distribution(b, t + 1, t + blk.tree_bytes, 256)
            blk.weights_end = b[t + blk.tree_bytes - 1]
        if blk.tree_bytes:
            blk.tables.append((t, t + blk.tree_bytes))
        t += blk.tree_bytes
        if blk.lit_streams == 4:
            sizes = [_le(b, t + 2 * k, 2) for k in range(3)]
            blk.tables.append((t, t + 6))
            t += 6
            sizes.append(q - t - sum(sizes))
        else:
            sizes = [q - t]
        if min(sizes) < 1:
            raise ValueError("an empty literals stream")
        blk.stream_ends = []
        for n in sizes:
            t += n
            blk.stream_ends.append(b[t - 1])
    if q == end:
        raise ValueError("no sequences section")
    s0 = _le(b, q, 1)
    if s0 == 0:
        blk.nseq, blk.seq_header = 0, 1
        if q + 1 != end:
            raise ValueError("bytes after an empty sequences section")
        return
    if s0 < 128:
        blk.nseq, n = s0, 1
    elif s0 < 255:
        blk.nseq, n = ((s0 - 128) << 8) + _le(b, q + 1, 1), 2
    else:
        blk.nseq, n = _le(b, q + 1, 2) + 0x7F00, 3
    m = _le(b, q + n, 1)
    if m & 3:
        raise ValueError("reserved mode bits")
    blk.modes = (m >> 6, (m >> 4) & 3, (m >> 2) & 3)
    blk.seq_header = n + 1
    if q + n + 1 > end:
        raise ValueError("sequences header runs past its block")
    if entropy:
        t = q + n + 1
        blk.dists, blk.rle_syms, blk.tables = {}, {}, blk.tables or []
        for which, mode in enumerate(blk.modes):
            t0 = t
            if mode == SEQ_RLE:
                blk.rle_syms[which] = _le(b, t, 1)
                t += 1
            elif mode == SEQ_FSE:
                blk.dists[which] = read_distribution(b, t, end, (36, 32, 53)[which])
                t += blk.dists[which].size
            if t > t0:
                blk.tables.append((t0, t))
        if t >= end:
            raise ValueError("no sequence bitstream")
        blk.seq_end = b[end - 1]


def parse_frame(b, p=0, entropy=False):
    if b[p:p + 4] != MAGIC:
        raise ValueError("bad magic")
    fhd = _le(b, p + 4, 1)
    if fhd & 0x08:
        raise ValueError("reserved descriptor bit")
    single = bool(fhd & 0x20)
    q = p + 5
    wd = None
    if not single:
        wd = _le(b, q, 1)
        q += 1
    dn = (0, 1, 2, 4)[fhd & 3]
    did = _le(b, q, dn) if dn else 0
    q += dn
    fn = (1 if single else 0, 2, 4, 8)[fhd >> 6]
    fcs = None
    if fn:
        fcs = _le(b, q, fn) + (256 if fn == 2 else 0)
    q += fn
    f = Frame(p, 0, q - p, single, wd, did, fcs, fn, bool(fhd & 4))
    while True:
        h = _le(b, q, 3)
        blk = Block(bool(h & 1), (h >> 1) & 3, h >> 3, 0)
        if blk.type == 3:
            raise ValueError("reserved block type")
        blk.content = 1 if blk.type == RLE else blk.size
        q += 3
        if q + blk.content > len(b):
            raise ValueError("block runs past the input")
        if blk.type == COMPRESSED:
            parse_compressed_block(b, q, blk.size, blk, entropy)
        q += blk.content
        f.blocks.append(blk)
        if blk.last:
            break
    if f.checksum:
        _le(b, q, 4)
        q += 4
    f.end = q
    return f


def parse_frames(b):
    """every frame of b, which must be nothing but frames"""
    out, p = [], 0
    while p < len(b):
        out.append(parse_frame(b, p))
        p = out[-1].end
    return out


def regenerated_size(f):
    """bytes the frame's Raw and RLE blocks regenerate (a Compressed block's needs its sequences: None)"""
    if any(k.type == COMPRESSED for k in f.blocks):
        return None
    return sum(k.size for k in f.blocks)
