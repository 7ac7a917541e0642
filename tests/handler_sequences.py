"""Fixed, seeded write sequences through every encoder handle: what scripts/record_handler_bytes.py
records (tests/golden/handler_bytes.json) and tests/test_gpu_handler_bytes.py replays.  The sizes sit
where the handles' shared staging can go wrong: one item, an item boundary on either side, a block
buffer one byte short of, at and past a block, several items of one launch.  No message is over
200 000 bytes; every one is text and random bytes mixed (lz_inputs.text, Random.randbytes).

A case is (name, make, ops).  make(H) builds the handle from netty_amd.handlers; an op is
("write", bytes), ("write_at", buffer, reader_index) for FastLZ, ("flush",) or ("close",).
run(H, case) returns what each op returned, in order."""
import hashlib
import random

import lz_inputs

SNAPPY_SLICES = (32767, 65535)  # SnappyFrameEncoder's slice, plain and with jumbo frames


def mixed(seed, n):
    """n bytes: runs of word text and of random bytes, 50..3000 bytes each"""
    rng = random.Random(0x5E9 + seed)
    out = bytearray()
    while len(out) < n:
        k = rng.randrange(50, 3000)
        out += lz_inputs.text(rng, k) if rng.random() < 0.6 else rng.randbytes(k)
    return bytes(out[:n])


def _writes(seed, sizes):
    return [("write", mixed(seed + i, n)) for i, n in enumerate(sizes)]


def _buffer_edges(seed, bs):
    """Block-buffer writes for Lz4FrameEncoder and ZstdEncoder: have + n = bs - 1, bs and bs + 1, and a
    write of several blocks onto a buffer holding bs - 1 (3 bs + 7 bytes where that is at most 200 000,
    bs + 7 otherwise: two blocks close either way)."""
    big = 3 * bs + 7 if 3 * bs + 7 <= 200000 else bs + 7
    sizes = [10, bs - 11,      # the buffer holds bs - 1
             big,              # closes every block but the last 6 bytes
             bs - 6,           # have + n = bs
             5, bs - 4,        # have + n = bs + 1
             20]               # 21 bytes stay
    return _writes(seed, sizes)


def cases():
    out = []
    for jumbo, sl in enumerate(SNAPPY_SLICES):
        sizes = [17, 18, 19, sl - 1, sl, sl + 1, 2 * sl + 5]  # one handle: the stream header comes once
        out.append((f"snappy/slice{sl}", lambda H, j=jumbo: H.SnappyFrameEncoder(jumbo=bool(j)), _writes(100 + jumbo, sizes)))
    for level in (0, 1, 2):
        for cks in (False, True):
            out.append((f"fastlz/level{level}/checksum{int(cks)}", lambda H, l=level, c=cks: H.FastLzFrameEncoder(l, c),
                        _writes(200 + level, [1, 31, 32, 65535, 65536, 131071])))
    out.append(("fastlz/reader_index", lambda H: H.FastLzFrameEncoder(1, True), [("write_at", mixed(210, 70100), 100)]))
    out.append(("fastlz/incompressible", lambda H: H.FastLzFrameEncoder(0, False),
                [("write", random.Random(211).randbytes(40000))]))
    out.append(("lzf/below_threshold", lambda H: H.LzfEncoder(compress_threshold=1000), _writes(300, [0, 999])))
    out.append(("lzf/chunks", lambda H: H.LzfEncoder(), _writes(310, [65535, 65536, 140000])))
    for bs in (64, 4096):
        for high in (False, True):
            ops = _buffer_edges(400 + bs, bs) + [("flush",), ("write", mixed(420, 30)), ("close",),
                                                 ("write", mixed(421, 2 * bs + 40))]  # after close: passes through
            out.append((f"lz4/bs{bs}/high{int(high)}", lambda H, b=bs, h=high: H.Lz4FrameEncoder(b, h), ops))
    for bs in (64, 65536, 100000):  # 100 000: a block is two 64 KiB slices
        ops = [("flush",)] + _buffer_edges(500 + bs, bs) + [("flush",), ("flush",)]
        out.append((f"zstd/bs{bs}", lambda H, b=bs: H.ZstdEncoder(3, b), ops))
    for w in ("ZLIB", "GZIP", "NONE"):
        out.append((f"zlib/{w}", lambda H, w=w: H.JdkZlibEncoder(H.ZlibWrapper[w], 6), _writes(600, [1, 65536, 65537]) + [("close",)]))
    out.append(("zlib/dictionary", lambda H: H.JdkZlibEncoder(H.ZlibWrapper.ZLIB, 6, dictionary=mixed(610, 5000)),
                [("write", mixed(610, 5000)[1000:4000] + mixed(611, 70000)), ("write", mixed(612, 3000)), ("close",)]))
    # level 1 closes a block every 99 994 bytes of these (runs are rare): 0, 1 and 2 blocks close
    out.append(("bzip2/writes", lambda H: H.Bzip2Encoder(1), _writes(700, [50000, 100000, 200000]) + [("close",)]))
    out.append(("bzip2/never_written", lambda H: H.Bzip2Encoder(1), [("close",)]))
    return out


def run(H, case):
    _, make, ops = case
    e = make(H)
    got = []
    try:
        for op in ops:
            if op[0] == "write":
                got.append(e.encode(op[1]))
            elif op[0] == "write_at":
                got.append(e.encode(b"", reader_index=op[2], buffer=op[1]))
            elif op[0] == "flush":
                got.append(e.flush())
            else:
                got.append(e.finish_encode())
    finally:
        e.close()
    return got


def digest(pieces):
    return [{"sha256": hashlib.sha256(p).hexdigest(), "len": len(p)} for p in pieces]


def input_digest(case):
    """one hash over a case's input bytes, so that a drifting generator is told apart from drifting output"""
    h = hashlib.sha256()
    for op in case[2]:
        if len(op) > 1:
            h.update(op[1])
    return h.hexdigest()
