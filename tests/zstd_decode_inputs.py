"""The corpus of the Zstandard decoder tests, shared by the CPU tests (nx_zstd_decode_host) and the GPU
tests (nx_zstd_decode_batch): frames libzstd wrote (through pyarrow) over a grid of levels, content
kinds and lengths, plus the truncations, limit cases and mutations of the hostile-input tests.  Seeded;
built once per process."""
import functools
import random
from dataclasses import dataclass

import zstd_frames as Z
import zstd_handbuilt as HB

LEVELS = (-5, 1, 3, 9, 19)
LENGTHS = (1, 5, 300, 1024, 5000, 65536, 131072, 131073, 300000, 1048576)
KINDS = ("text", "random", "zero", "two", "period7", "skew")
TRAILING = b"\x28\xb5\x2f\xfd\x00"  # five bytes after a frame: the start of another
GUARD = 64


@dataclass
class Case:
    kind: str
    n: int
    level: int
    data: bytes
    frame: bytes


def _content(oracle, rng, kind, n):
    if kind == "text":
        return oracle.textgen_chunk(7, n)
    if kind == "random":
        return rng.randbytes(n)
    if kind == "zero":
        return bytes(n)
    if kind == "two":
        return bytes(rng.randbytes(n).translate(bytes(b"ab"[b & 1] for b in range(256))))
    if kind == "period7":
        return (rng.randbytes(7) * (n // 7 + 1))[:n]
    return bytes(min(255, int(rng.expovariate(0.05))) for _ in range(n))  # a skewed exponential byte distribution


_CACHE = {}


def libzstd_frames(oracle):
    """every (level, kind, length) of the grid as a Case, in a fixed order"""
    if "frames" not in _CACHE:
        import pyarrow as pa
        rng = random.Random(5)
        contents = [(k, n, _content(oracle, rng, k, n)) for n in LENGTHS for k in KINDS]
        _CACHE["frames"] = [Case(k, n, lvl, d, pa.Codec("zstd", compression_level=lvl).compress(d).to_pybytes())
                            for lvl in LEVELS for k, n, d in contents]
    return _CACHE["frames"]


def unzstd(frame, n):
    """libzstd's decode of a frame that regenerates n bytes (raises on anything else)"""
    import pyarrow as pa
    return pa.Codec("zstd").decompress(frame, decompressed_size=n).to_pybytes()


def small_frames(oracle):
    """six small frames for the truncation and mutation tests: three of libzstd's (Compressed blocks with
    Huffman literals and FSE tables, a Raw block, an RLE block) and three hand-built"""
    by = {(c.kind, c.n, c.level): c for c in libzstd_frames(oracle)}
    hb = HB.cases()
    return [(by["text", 300, 3].frame, by["text", 300, 3].data),
            (by["skew", 1024, 19].frame, by["skew", 1024, 19].data),
            (by["zero", 300, 1].frame, by["zero", 300, 1].data),
            hb["repeat_ll0_code1"], hb["rle_literals"], hb["no_content_size"]]


def truncations(oracle):
    """every proper prefix of the six small frames"""
    return [f[:k] for f, _ in small_frames(oracle) for k in range(len(f))]


def mutations(oracle, count=256, seed=77):
    """`count` single-byte mutations of two small frames (one of libzstd's, one hand-built), at seeded positions"""
    rng = random.Random(seed)
    src = [small_frames(oracle)[1][0], small_frames(oracle)[3][0]]
    out = []
    for i in range(count):
        f = bytearray(src[i & 1])
        at = rng.randrange(len(f))
        f[at] ^= rng.randrange(1, 256)
        out.append(bytes(f))
    return out


@functools.lru_cache(maxsize=None)
def _census_of(frames):
    seen = {"frames": len(frames), "multi_block": 0, "windowed": 0, "treeless_blocks": 0}
    flags = set()
    for fr in frames:
        f = Z.parse_frame(fr)
        assert f.end == len(fr)
        seen["multi_block"] += len(f.blocks) > 1
        seen["windowed"] += not f.single_segment
        for b in f.blocks:
            flags.add(("block", b.type))
            if b.type != Z.COMPRESSED:
                continue
            flags.add(("lit", b.lit_type))
            seen["treeless_blocks"] += b.lit_type == Z.LIT_TREELESS
            if b.lit_type >= 2:
                flags.add(("streams", b.lit_streams))
            if b.tree:
                flags.add(("tree", b.tree))
            if b.nseq == 0:
                flags.add("nseq0")
            else:
                flags.add("nseq_1b" if b.nseq < 128 else "nseq_2b" if b.nseq < 0x7F00 else "nseq_3b")
                for i, m in enumerate(b.modes):
                    flags.add(("mode", i, m))
    seen["flags"] = flags
    return seen


def census(frames):
    """what the frames exercise, from their headers (tests/zstd_frames.py)"""
    return _census_of(tuple(frames))


def entropy_census(frames):
    """what the frames' entropy tables exercise, read from their bytes (tests/zstd_frames.py, entropy=True):
    a set of flags such as ("ll_log", 9), ("of_minus", 3), ("ml_flags", (3, 1)), ("tree_weights", 128),
    ("repeat_after", which, mode), ("live_nseq", 65)"""
    flags = set()
    names = ("ll", "of", "ml")
    for fr in frames:
        f = Z.parse_frame(fr, entropy=True)
        assert f.end == len(fr)
        held = [None, None, None]   # the mode that built the table a Repeat_Mode block would reuse
        since_tree = None           # what came since the last tree description
        tree_streams = None
        for b in f.blocks:
            if b.type != Z.COMPRESSED:
                if since_tree is not None:
                    since_tree.add(("block", b.type))
                continue
            if b.lit_type >= Z.LIT_COMPRESSED:
                flags.add(("lit_format", b.lit_format))
                flags.add(("lit_regen", b.lit_streams, b.lit_regen))
                if 1 in b.stream_ends:
                    flags.add(("stream_end_01", b.lit_streams))
            if b.lit_type == Z.LIT_COMPRESSED:
                flags.add(("tree", b.tree))
                if b.tree == "direct":
                    flags.add(("tree_weights", b.tree_weights))
                else:
                    d = b.tree_dist
                    flags.update({("hw_log", d.log), ("hw_minus", d.minus)})
                    if b.weights_end == 1:
                        flags.add("weights_end_01")
                since_tree, tree_streams = set(), b.lit_streams
            elif b.lit_type == Z.LIT_TREELESS:
                flags.add(("treeless_after", frozenset(since_tree)))
                flags.add(("treeless_streams", tree_streams, b.lit_streams))
            elif since_tree is not None:
                since_tree.add(("lit", b.lit_type))
            if not b.nseq:
                if any(held):
                    flags.add("tables_across_nseq0")
                continue
            for which, mode in enumerate(b.modes):
                if mode == Z.SEQ_REPEAT:
                    flags.add(("repeat_after", which, held[which]))
                else:
                    held[which] = mode
            for which, sym in b.rle_syms.items():
                flags.add(("rle_sym", which, sym))
            for which, d in b.dists.items():
                n = names[which]
                flags.update({(n + "_log", d.log), (n + "_minus", d.minus), (n + "_top", d.top), (n + "_symbols", sum(p != 0 for p in d.probs))})
                flags.update((n + "_flags", c) for c in d.flags)
                if (1 << d.log) - 1 in d.probs:
                    flags.add((n + "_size_minus_1", d.minus))
            if len(b.dists) == 3 and min(d.log for d in b.dists.values()) >= 6:
                flags.add(("live_nseq", b.nseq))
            flags.add(("modes", b.modes))
            if b.seq_end == 1:
                flags.add("seq_end_01")
    return flags
