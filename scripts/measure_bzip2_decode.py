#!/usr/bin/env python3
"""Rate of batch.bzip2_decode (nx_bzip2_decode_batch) on text, next to libbz2 (Python's bz2) on 16 host threads.

Two batches of k_textgen text compressed by libbz2 at level 9: (a) 4 096 streams of 64 KiB, (b) 256 streams
of 900 000 bytes.  Steps, each a fresh child process under its own `timeout` (the parent never touches the
GPU; the first failing step ends the run):
  gpu_a, gpu_b    device-resident decode: HIP events around batch.bzip2_decode, 1 warm-up call and 3 timed,
                  output checked against the source.
  host_a, host_b  bz2.decompress of the same streams on 16 threads (the module releases the GIL), best of 3.
--step runs one step.  For the A/B of the split walk, copy a variant of the library (scripts/build_lib_variant.sh
with -DNX_BZIP2_CHAINS_PER_LANE=k or -DNX_BZIP2_SINGLE_CHAIN) over netty_amd/libnetty_amd.so and run --step gpu_b:
the line carries the build's chain count.  Prints one JSON line per step.
DESIGN.md section 4 "Bzip2 decode" records the figures.
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
STEP_LIMIT_S = {"gpu_a": 300, "gpu_b": 420, "host_a": 240, "host_b": 240}


def _compress(chunks):
    with ThreadPoolExecutor(16) as ex:
        return list(ex.map(lambda c: bz2.compress(c, 9), chunks))


def step_gpu(which):
    import torch
    from netty_amd import batch as B
    n, L = BATCH[which]
    dev = torch.device("cuda:0")
    src = torch.empty(n * L, dtype=torch.uint8, device=dev)
    B.textgen(src, 0, n, L)
    host = src.cpu().numpy().tobytes()
    enc, eoff, elen = B.pack(_compress([host[k * L:(k + 1) * L] for k in range(n)]), dev)
    off = torch.arange(n, dtype=torch.int64, device=dev) * L
    cap = torch.full((n,), L, dtype=torch.int32, device=dev)
    dec = torch.empty(n * L, dtype=torch.uint8, device=dev)
    ms = []
    for it in range(4):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        olen, cons, st = B.bzip2_decode(enc, eoff, elen, dec, off, cap)
        b.record()
        torch.cuda.synchronize()
        if it >= 1:
            ms.append(a.elapsed_time(b))
    assert int((olen != L).sum()) == 0 and int((st != 0).sum()) == 0, "bzip2_decode did not produce every stream"
    assert torch.equal(cons, elen), "consumed differs from the stream lengths"
    assert torch.equal(dec, src), "bzip2_decode output differs from the source"
    best = min(ms)
    print(json.dumps({"step": "gpu_" + which, "chains": B.bzip2_decode_chains(), "streams": n, "bytes_each": L,
                      "compressed_bytes": int(elen.sum()), "ms": [round(x, 3) for x in ms],
                      "out_gib_s": round(n * L / 2**30 / (best / 1e3), 3)}))


def step_host(which):
    from oracle import pyoracle as O
    O.build()
    n, L = BATCH[which]
    zs = _compress([O.textgen_chunk(k, L) for k in range(n)])

    def run(part):
        return sum(len(bz2.decompress(z)) for z in part)

    parts = [zs[k::16] for k in range(16)]
    best = None
    for _ in range(3):
        t = time.perf_counter()
        with ThreadPoolExecutor(16) as ex:
            total = sum(ex.map(run, parts))
        dt = time.perf_counter() - t
        best = dt if best is None or dt < best else best
    assert total == n * L
    print(json.dumps({"step": "host_" + which, "streams": n, "bytes_each": L, "threads": 16, "s": round(best, 4),
                      "out_gib_s": round(n * L / 2**30 / best, 3)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=list(STEP_LIMIT_S))
    a = ap.parse_args()
    if a.step:
        return step_host(a.step[-1]) if a.step.startswith("host") else step_gpu(a.step[-1])
    for s, limit in STEP_LIMIT_S.items():
        rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", s]).returncode
        if rc != 0:
            sys.exit(f"step {s} ended with status {rc}: nothing more is started")


if __name__ == "__main__":
    main()
