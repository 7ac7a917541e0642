#!/usr/bin/env python3
"""Times nx_brotli_decode_batch on the fixture's text streams replicated to a few thousand items, and pyarrow's
libbrotli (one thread) on the same streams on the same host.  Prints one JSON line.  Both sides are timed the same
way: `--warmup` untimed passes, then the median of `--reps` passes over all items.  A device pass is one
batch.brotli_decode call between two events, which includes that call's three small result allocations (from
torch's caching allocator after the warm-up); a libbrotli pass is wall time over one Codec.decompress per item.
Outputs are checked once against the plain texts."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import pyarrow as pa
    import torch

    import brotli_decode_inputs as I
    from netty_amd import batch as B

    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    base = [(s, I.plain(c)) for c, s in I.load() if c["kind"] == "text" and c["size"] >= 1000]
    items = [base[i % len(base)] for i in range(a.items)]
    dev = torch.device("cuda:0")
    inp, off, ln = B.pack([s for s, _ in items], dev, align=1, pad=16)
    out, ooff = B.out_slots([len(p) for _, p in items], dev, align=1)
    caps = torch.tensor([len(p) for _, p in items], dtype=torch.int32, device=dev)
    times = []
    for k in range(a.warmup + a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        olen, used, st = B.brotli_decode(inp, off, ln, out, ooff, caps)
        e1.record()
        torch.cuda.synchronize()
        if k >= a.warmup:
            times.append(e0.elapsed_time(e1))
    assert int((st != 0).sum()) == 0
    raw, oo = out.cpu().numpy().tobytes(), ooff.cpu().tolist()
    for (s, p), o in list(zip(items, oo))[::97]:
        assert raw[o:o + len(p)] == p
    times.sort()
    gpu_ms = times[len(times) // 2]
    codec = pa.Codec("brotli")
    cpu = []
    for k in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        for s, p in items:
            codec.decompress(s, decompressed_size=len(p))
        if k >= a.warmup:
            cpu.append((time.perf_counter() - t0) * 1e3)
    cpu.sort()
    cpu_ms = cpu[len(cpu) // 2]
    out_bytes = sum(len(p) for _, p in items)
    print(json.dumps({"items": a.items, "in_bytes": sum(len(s) for s, _ in items), "out_bytes": out_bytes, "gpu_ms_median": round(gpu_ms, 3),
                      "gpu_ms_min": round(times[0], 3), "gpu_ms_max": round(times[-1], 3), "gpu_out_MBps": round(out_bytes / gpu_ms / 1e3, 1),
                      "libbrotli_1thread_ms_median": round(cpu_ms, 3), "libbrotli_ms_min": round(cpu[0], 3), "libbrotli_ms_max": round(cpu[-1], 3), "libbrotli_out_MBps": round(out_bytes / cpu_ms / 1e3, 1)}))


if __name__ == "__main__":
    main()
