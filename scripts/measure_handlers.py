#!/usr/bin/env python3
"""Wall time and API work of one 1 MiB encode() on each of the seven synchronous encoder handles
(Bzip2 at level 1).  Needs a GPU.

    python scripts/measure_handlers.py [--lib libnetty_amd.so] [--steps 15] [--warmup 3]
        one JSON line: the median wall time of the call per handle, in microseconds
    python scripts/measure_handlers.py --once NAME [--lib ...]
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
