#!/usr/bin/env python3
"""Rate of batch.bzip2_encode (nx_bzip2_encode_batch) on text, next to libbz2 (Python's bz2) on 16 host threads.

Two batches of k_textgen text at level 9: (a) 4 096 items of 64 KiB, (b) 256 items of 900 000 bytes.  Steps, each
a fresh child process under its own `timeout` (the parent never touches the GPU; the first failing step ends the
run):
  gpu_a, gpu_b    device-resident encode: HIP events around batch.bzip2_encode, 1 warm-up call and 3 timed, every
                  output stream round-tripped through bz2.decompress on 16 threads.
  host_a, host_b  bz2.compress of the same items on 16 threads (the module releases the GIL), best of 3.
--step runs one step.  To separate the sort from the rest, copy a variant of the library built with
scripts/build_lib_variant.sh sortonly -DNX_BZIP2_ENC_SORT_ONLY (the kernel stops a block after its rotation sort)
over netty_amd/libnetty_amd.so and run --step gpu_a / gpu_b with --sort-only, which skips the round trip: that
time is the first run-length stage, the CRC and the sort.  Prints one JSON line per step.
DESIGN.md section 4 "Bzip2 encode" records the figures.
"""
import argparse
import bz2
import json
import os
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BATCH = {"a": (4096, 65536), "b": (256, 900000)}
STEP_LIMIT_S = {"gpu_a": 300, "gpu_b": 300, "host_a": 240, "host_b": 240}
LEVEL = 9


def step_gpu(which, sort_only):
    import torch
    from netty_amd import batch as B
    n, L = BATCH[which]
    dev = torch.device("cuda:0")
    src = torch.empty(n * L, dtype=torch.uint8, device=dev)
    B.textgen(src, 0, n, L)
    off = torch.arange(n, dtype=torch.int64, device=dev) * L
    ln = torch.full((n,), L, dtype=torch.int32, device=dev)
    cap = (B.bzip2_max_compressed_length(L, LEVEL) + 15) // 16 * 16
    out = torch.empty(n * cap, dtype=torch.uint8, device=dev)
    ooff = torch.arange(n, dtype=torch.int64, device=dev) * cap
    caps = torch.full((n,), cap, dtype=torch.int32, device=dev)
    ms = []
    for it in range(4):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        olen, st = B.bzip2_encode(src, off, ln, out, ooff, caps, LEVEL)
        b.record()
        torch.cuda.synchronize()
        if it >= 1:
            ms.append(a.elapsed_time(b))
    assert int((st != 0).sum()) == 0, "bzip2_encode reported a status"
    lens = olen.cpu().tolist()
    if not sort_only:
        host, enc = src.cpu().numpy().tobytes(), out.cpu().numpy().tobytes()
        with ThreadPoolExecutor(16) as ex:
            ok = list(ex.map(lambda k: bz2.decompress(enc[k * cap:k * cap + lens[k]]) == host[k * L:(k + 1) * L], range(n)))
        assert all(ok), "a stream does not decompress to its item"
    best = min(ms)
    print(json.dumps({"step": "gpu_" + which, "sort_only": sort_only, "items": n, "bytes_each": L, "level": LEVEL,
                      "compressed_bytes": sum(lens), "ms": [round(x, 3) for x in ms], "in_gib_s": round(n * L / 2**30 / (best / 1e3), 3)}))


def step_host(which):
    from oracle import pyoracle as O
    O.build()
    n, L = BATCH[which]
    chunks = [O.textgen_chunk(k, L) for k in range(n)]

    def run(part):
        return sum(len(bz2.compress(c, LEVEL)) for c in part)

    parts = [chunks[k::16] for k in range(16)]
    best = None
    for _ in range(3):
        t = time.perf_counter()
        with ThreadPoolExecutor(16) as ex:
            total = sum(ex.map(run, parts))
        dt = time.perf_counter() - t
        best = dt if best is None or dt < best else best
    print(json.dumps({"step": "host_" + which, "items": n, "bytes_each": L, "level": LEVEL, "threads": 16, "compressed_bytes": total,
                      "s": round(best, 4), "in_gib_s": round(n * L / 2**30 / best, 3)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=list(STEP_LIMIT_S))
    ap.add_argument("--sort-only", action="store_true")
    a = ap.parse_args()
    if a.step:
        return step_host(a.step[-1]) if a.step.startswith("host") else step_gpu(a.step[-1], a.sort_only)
    for s, limit in STEP_LIMIT_S.items():
        rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", s]).returncode
        if rc != 0:
            sys.exit(f"step {s} ended with status {rc}: nothing more is started")


if __name__ == "__main__":
    main()
