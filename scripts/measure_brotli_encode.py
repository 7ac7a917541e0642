#!/usr/bin/env python3
"""Rate and ratio of batch.brotli_encode (nx_brotli_encode_batch) on text, next to libbrotli on the host.

Steps, each a fresh child process under its own `timeout` (the parent never touches the GPU; the first failing
step ends the run):
  gpu_1024, gpu_4096  device-resident encode of that many items of 64 KiB of k_textgen text at lgwin 22: HIP events
                  around batch.brotli_encode, 1 warm-up call and 3 timed; 64 streams spread over the batch are
                  decoded by libbrotli (pyarrow) and compared.  The share of each pass is read from
                  `rocprofv3 --kernel-trace --stats -- python scripts/measure_brotli_encode.py --step gpu_1024`
                  The call launches both passes itself, so events around it time their sum; the split per pass
                  comes from that kernel trace and not from events (step `passes` prints it from the trace's CSV).
  passes          that kernel trace, run and read: the average time of each pass per call.
  ratio           the compressed size of 256 of those items next to libbrotli quality 1 through pyarrow on the
                  same bytes, and libbrotli's own time for them on 16 host threads.
--step runs one step.  Prints one JSON line per step.  DESIGN.md "Brotli encode" records the figures.
"""
import argparse
import json
import os
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
L = 65536
STEP_LIMIT_S = {"gpu_1024": 240, "gpu_4096": 300, "ratio": 240, "passes": 300}


def _text(n):
    import torch
    from netty_amd import batch as B
    dev = torch.device("cuda:0")
    src = torch.empty(n * L, dtype=torch.uint8, device=dev)
    B.textgen(src, 0, n, L)
    off = torch.arange(n, dtype=torch.int64, device=dev) * L
    ln = torch.full((n,), L, dtype=torch.int32, device=dev)
    return torch, B, dev, src, off, ln


def _slots(torch, dev, n, cap):
    cap = (cap + 15) // 16 * 16
    return (torch.empty(n * cap, dtype=torch.uint8, device=dev), torch.arange(n, dtype=torch.int64, device=dev) * cap,
            torch.full((n,), cap, dtype=torch.int32, device=dev), cap)


def step_gpu(n):
    import pyarrow as pa
    torch, B, dev, src, off, ln = _text(n)
    out, ooff, caps, cap = _slots(torch, dev, n, B.brotli_max_compressed_length(L))
    ms = []
    for it in range(4):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        olen, st = B.brotli_encode(src, off, ln, out, ooff, caps)
        b.record()
        torch.cuda.synchronize()
        if it >= 1:
            ms.append(a.elapsed_time(b))
    assert int((st != 0).sum()) == 0, "brotli_encode reported a status"
    lens = olen.cpu().tolist()
    codec = pa.Codec("brotli")
    for k in range(0, n, max(1, n // 64)):
        item = src[k * L:(k + 1) * L].cpu().numpy().tobytes()
        s = out[k * cap:k * cap + lens[k]].cpu().numpy().tobytes()
        assert codec.decompress(s, decompressed_size=L).to_pybytes() == item, "a stream does not decode to its item"
    best = min(ms)
    print(json.dumps({"step": "gpu_%d" % n, "items": n, "bytes_each": L, "compressed_bytes": sum(lens), "ms": [round(x, 3) for x in ms],
                      "in_gib_s": round(n * L / 2**30 / (best / 1e3), 3), "ratio": round(n * L / sum(lens), 4)}))


def step_ratio():
    import pyarrow as pa
    n = 256
    torch, B, dev, src, off, ln = _text(n)
    out, ooff, caps, _ = _slots(torch, dev, n, B.brotli_max_compressed_length(L))
    olen, st = B.brotli_encode(src, off, ln, out, ooff, caps)
    torch.cuda.synchronize()
    assert int((st != 0).sum()) == 0
    host = src.cpu().numpy().tobytes()
    items = [host[k * L:(k + 1) * L] for k in range(n)]
    q1 = pa.Codec("brotli", compression_level=1)

    def one(d):
        return len(q1.compress(d).to_pybytes())  # pyarrow releases the GIL inside the codec
    with ThreadPoolExecutor(16) as ex:
        list(ex.map(one, items[:16]))
        t = time.perf_counter()
        sizes = list(ex.map(one, items))
        dt = time.perf_counter() - t
    res = {"step": "ratio", "items": n, "bytes_each": L, "brotli_gpu": int(olen.sum().item()), "libbrotli_q1": sum(sizes),
           "libbrotli_q1_16_threads_ms": round(dt * 1e3, 2), "libbrotli_q1_16_threads_gib_s": round(n * L / 2**30 / dt, 3)}
    res["gpu_over_libbrotli"] = round(res["brotli_gpu"] / res["libbrotli_q1"], 4)
    for k in ("brotli_gpu", "libbrotli_q1"):
        res[k + "_ratio"] = round(n * L / res[k], 4)
    print(json.dumps(res))


def step_passes():
    """the kernel trace of the gpu_1024 step (four calls): average time of each pass per call.  This process opens no GPU."""
    import csv
    import glob
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "rp", "--", sys.executable,
                        os.path.abspath(__file__), "--step", "gpu_1024"], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL,
                       timeout=STEP_LIMIT_S["passes"] - 20)
        res = {"step": "passes", "items": 1024}
        for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                for k, name in (("k_brotli_match", "k_seq_match<nx::brotli"), ("k_brotli_emit", "k_brotli_emit")):
                    if name in row["Name"]:
                        res[k + "_ms"] = round(float(row["AverageNs"]) / 1e6, 3)
                        res[k + "_calls"] = int(row["Calls"])
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=list(STEP_LIMIT_S))
    a = ap.parse_args()
    if a.step:
        return step_ratio() if a.step == "ratio" else step_passes() if a.step == "passes" else step_gpu(int(a.step[4:]))
    for s, limit in STEP_LIMIT_S.items():
        rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", s]).returncode
        if rc != 0:
            sys.exit(f"step {s} ended with status {rc}: nothing more is started")


if __name__ == "__main__":
    main()
