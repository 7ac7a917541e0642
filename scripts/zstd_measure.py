#!/usr/bin/env python3
"""Zstandard encoder measurement (DESIGN.md §4 "Zstandard encode"): 32 768 x 64 KiB k_textgen chunks.

  python scripts/zstd_measure.py            runs every step, each a child process under its own timeout
  python scripts/zstd_measure.py time       HIP events, 2 warm-up and 5 timed calls: batch.zstd_encode and
                                            batch.deflate_encode on the same chunks in one process; output sizes
  python scripts/zstd_measure.py libzstd    libzstd levels 1 and 3 on 16 host threads over the first 4 096 chunks
  python scripts/zstd_measure.py trace      the time step under rocprofv3 --kernel-trace --stats: the per-pass split
"""
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, L = 32768, 65536


def _chunks(n):
    import torch
    from netty_amd import batch as B
    dev = torch.device("cuda:0")
    src = torch.empty(n * L, dtype=torch.uint8, device=dev)
    B.textgen(src, 0, n, L)
    off = torch.arange(n, dtype=torch.int64, device=dev) * L
    ln = torch.full((n,), L, dtype=torch.int32, device=dev)
    return torch, B, dev, src, off, ln


def step_time(calls=5, warm=2):
    torch, B, dev, src, off, ln = _chunks(N)
    for name, enc, bound in (("zstd", B.zstd_encode, B.zstd_max_compressed_length), ("deflate", B.deflate_encode, B.deflate_max_compressed_length)):
        cap = (bound(L) + 15) // 16 * 16
        out = torch.empty(N * cap, dtype=torch.uint8, device=dev)
        ooff = torch.arange(N, dtype=torch.int64, device=dev) * cap
        ms = []
        for i in range(warm + calls):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            olen, st = enc(src, off, ln, out, ooff)
            b.record()
            torch.cuda.synchronize()
            if i >= warm:
                ms.append(a.elapsed_time(b))
        assert int((st != 0).sum()) == 0
        med = sorted(ms)[len(ms) // 2]
        print(f"{name}: ms per launch sequence {['%.2f' % m for m in ms]} median {med:.2f}  {N * L / 2**30 / (med / 1e3):.1f} GiB/s of input  "
              f"output {int(olen.sum())} bytes ({int(olen.sum()) / (N * L):.4f} of input)", flush=True)
        del out


def step_libzstd(n=4096, threads=16):
    import pyarrow as pa
    from concurrent.futures import ThreadPoolExecutor
    torch, B, dev, src, off, ln = _chunks(n)
    host = src.cpu().numpy().tobytes()
    chunks = [host[i * L:(i + 1) * L] for i in range(n)]
    for level in (1, 3):
        codec = pa.Codec("zstd", compression_level=level)
        with ThreadPoolExecutor(threads) as ex:
            t0 = time.perf_counter()
            sizes = list(ex.map(lambda c: len(codec.compress(c)), chunks))
            dt = time.perf_counter() - t0
        print(f"libzstd level {level}, {threads} host threads, {n} chunks: {dt * 1e3:.0f} ms  {n * L / 2**30 / dt:.2f} GiB/s  "
              f"output {sum(sizes)} bytes ({sum(sizes) / (n * L):.4f} of input)", flush=True)


def main():
    step = sys.argv[1] if len(sys.argv) > 1 else "all"
    if step == "time":
        return step_time()
    if step == "libzstd":
        return step_libzstd()
    me = os.path.abspath(__file__)
    out = tempfile.mkdtemp(prefix="zstd_trace_")
    steps = [([sys.executable, me, "time"], 300), ([sys.executable, me, "libzstd"], 300),
             (["rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "zstd", "--output-format", "csv", "--", sys.executable, me, "time"], 420)]
    if step == "trace":
        steps = steps[2:]
    for cmd, limit in steps:
        # `timeout` ends the step's whole tree, the child that holds the GPU included
        r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=ROOT, env=dict(os.environ), stdout=None if "rocprofv3" not in cmd[0] else subprocess.DEVNULL)
        if r.returncode != 0:  # a failed step ends the run: nothing more is started on the GPU
            sys.exit(r.returncode)
    stats = [os.path.join(d, f) for d, _, fs in os.walk(out) for f in fs if f.endswith("kernel_stats.csv")]
    for p in stats:
        for line in open(p):
            if "zstd" in line or "deflate" in line or line.startswith('"Name"'):
                print(line.rstrip())


if __name__ == "__main__":
    main()
