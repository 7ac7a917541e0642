#!/usr/bin/env python3
"""Wall time and API work of one 1 MiB encode() on each of the seven synchronous encoder handles
(Bzip2 at level 1), or with --decoders of one decode() of the stream of that 1 MiB on each of the seven
decoder handles.  Needs a GPU.

    python scripts/measure_handlers.py [--decoders] [--lib libnetty_amd.so] [--steps 15] [--warmup 3]
        one JSON line: the median wall time of the call per handle, in microseconds
    python scripts/measure_handlers.py [--decoders] --once NAME [--lib ...]
        one handle, one call and nothing else: the program to put behind `rocprofv3 --hip-trace
        --kernel-trace --memory-copy-trace -- ` when the call's copies, syncs, allocations and launches
        are counted (scripts/count_handler_api.py reads the traces)"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

N = 1 << 20
# name: (the handle, its encode entry point); the call goes to the C ABI with one output buffer made
# beforehand, so that the Python wrapper's own copies are not in the time
HANDLES = {
    "snappy": (lambda H: H.SnappyFrameEncoder(), "nx_snappy_frame_encoder_encode"),
    "fastlz": (lambda H: H.FastLzFrameEncoder(1, True), "nx_fastlz_frame_encoder_encode"),
    "lzf": (lambda H: H.LzfEncoder(), "nx_lzf_encoder_encode"),
    "lz4": (lambda H: H.Lz4FrameEncoder(1 << 16), "nx_lz4_frame_encoder_encode"),
    "zstd": (lambda H: H.ZstdEncoder(3, 1 << 16), "nx_zstd_encoder_encode"),
    "zlib": (lambda H: H.JdkZlibEncoder(H.ZlibWrapper.ZLIB, 6), "nx_zlib_encoder_encode"),
    "bzip2": (lambda H: H.Bzip2Encoder(1), "nx_bzip2_encoder_encode"),
}
CAP = 4 << 20  # above every handle's bound for 1 MiB (Bzip2's includes an open block of up to 100 000 bytes)

# --decoders.  name: (the handle, its stream of `data`): the streams come from the oracle's frame encoders, the
# standard library and libzstd, and are built before anything is timed.  One handle takes every call where the stream lets it
# (LZ4's is left without its end block for that); zlib and Bzip2 close at their stream's end, so each of their
# calls has a fresh handle, made outside the time.
FRESH = ("zlib", "bzip2")
DECODERS = {
    "snappy": (lambda H: H.SnappyFrameDecoder(True), lambda O, d: O.snappy_frame_encode(d)[0]),
    "fastlz": (lambda H: H.FastLzFrameDecoder(True), lambda O, d: O.fastlz_frame_encode(d, 0, True)),
    "lzf": (lambda H: H.LzfDecoder(), lambda O, d: O.lzf_frame_encode(d)),
    "lz4": (lambda H: H.Lz4FrameDecoder(True), lambda O, d: O.lz4_frame_encode(d, close=False)),
    "zstd": (lambda H: H.ZstdDecoder(0), lambda O, d: _zstd(d)),
    "zlib": (lambda H: H.JdkZlibDecoder(H.ZlibWrapper.ZLIB), lambda O, d: __import__("zlib").compress(d, 6)),
    "bzip2": (lambda H: H.Bzip2Decoder(), lambda O, d: __import__("bz2").compress(d, 1)),
}


def _zstd(data):  # libzstd, as tests/zstd_decode_inputs.py reaches it; frames of 128 KiB, so that a call has several items
    import pyarrow as pa
    c = pa.Codec("zstd", compression_level=3)
    return b"".join(c.compress(data[i:i + (1 << 17)]).to_pybytes() for i in range(0, len(data), 1 << 17))


def decode(L, _lib, d, stream):
    """one decode() of the whole stream through the C ABI: (seconds, bytes delivered)"""
    import ctypes as C
    consumed, n = C.c_size_t(0), C.c_size_t(0)
    msgs, err = C.POINTER(_lib.NxMsg)(), C.c_char_p()
    f = getattr(L, d._decode_fn)
    t0 = time.perf_counter()
    rc = f(d._h, stream, len(stream), C.byref(consumed), C.byref(msgs), C.byref(n), C.byref(err))
    t = time.perf_counter() - t0
    if rc != 0 or consumed.value != len(stream):
        raise RuntimeError(f"{type(d).__name__}: decode returned {rc}, consumed {consumed.value} of {len(stream)}")
    return t, sum(msgs[i].len for i in range(n.value))


def main_decoders(a, H, _lib, L, data):
    from oracle import pyoracle as O
    O.build()
    names = [a.once] if a.once else list(DECODERS)
    streams = {k: DECODERS[k][1](O, data) for k in names}
    if a.once:
        d = DECODERS[a.once][0](H)
        _, got = decode(L, _lib, d, streams[a.once])
        d.close()
        print(json.dumps({"handle": a.once, "bytes_in": len(streams[a.once]), "bytes_out": got}))
        return
    med = {}
    for name in names:
        ts, d = [], None
        for k in range(a.warmup + a.steps):
            if d is None or name in FRESH:
                if d:
                    d.close()
                d = DECODERS[name][0](H)
            t, got = decode(L, _lib, d, streams[name])
            if got != N:
                raise RuntimeError(f"{name}: {got} bytes delivered")
            if k >= a.warmup:
                ts.append(t)
        d.close()
        med[name] = round(statistics.median(ts) * 1e6, 1)
    print(json.dumps({"lib": _lib.LIB_PATH, "decoders": True, "bytes_out": N, "steps": a.steps, "median_us": med}))


def encode(L, name, e, data, out):
    f = getattr(L, HANDLES[name][1])
    r = f(e._h, data, 0, len(data), out, CAP) if name == "fastlz" else f(e._h, data, len(data), out, CAP)
    if r < 0:
        raise RuntimeError(f"{name}: encode failed with {r}")
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib")
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--once", choices=sorted(HANDLES))
    ap.add_argument("--decoders", action="store_true", help="the decoder handles' decode() instead of the encoders' encode()")
    a = ap.parse_args()
    if a.lib:  # the package's own import loads the tree's library: stand in for it, so that only a.lib is loaded
        import types
        pkg = types.ModuleType("netty_amd")
        pkg.__path__ = [os.path.join(ROOT, "netty_amd")]
        sys.modules["netty_amd"] = pkg
    from netty_amd import _lib
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    from netty_amd import handlers as H
    import handler_sequences as S

    import ctypes
    L = _lib.load()
    data = S.mixed(900, N)
    if a.decoders:
        return main_decoders(a, H, _lib, L, data)
    out = (ctypes.c_uint8 * CAP)()
    if a.once:
        e = HANDLES[a.once][0](H)
        print(json.dumps({"handle": a.once, "bytes_in": N, "bytes_out": encode(L, a.once, e, data, out)}))
        e.close()
        return
    med = {}
    for name, (make, _) in HANDLES.items():
        e = make(H)
        for _ in range(a.warmup):
            encode(L, name, e, data, out)
        ts = []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            encode(L, name, e, data, out)
            ts.append(time.perf_counter() - t0)
        e.close()
        med[name] = round(statistics.median(ts) * 1e6, 1)
    print(json.dumps({"lib": _lib.LIB_PATH, "bytes_in": N, "steps": a.steps, "median_us": med}))


if __name__ == "__main__":
    main()
