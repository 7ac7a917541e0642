#!/usr/bin/env python3
"""Time of the bzip2 encoder's split path (nx_bzip2_encode_batch_split) next to the per-stream kernel
(nx_bzip2_encode_batch) on the same input in the same run, k_textgen text at level 9.

Steps, each a fresh child process under its own `timeout` (the parent never touches the GPU; the first failing
step ends the run):
  a  one stream of 16 full blocks (16 x 899 990 bytes as one item): both paths.
  b  4 096 items of 64 KiB, one block each: both paths, which shows what the plan and the splice cost when
     there is nothing to split.
  c  the planner's launch alone (nx_bzip2_plan_batch) on the input of a.
HIP events around each call, 1 warm-up call and 3 timed, best of three; every stream of a and b is round-tripped
through bz2.decompress on 16 threads and the two paths' bytes are compared.  --step runs one step.  Prints one
JSON line per step.  DESIGN.md section 4 "Bzip2 encode, split" records the figures.
"""
import argparse
import bz2
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BATCH = {"a": (1, 16 * 899990), "b": (4096, 65536), "c": (1, 16 * 899990)}  # a block takes a byte while it holds <= 899 994
TEXT = {"a": (16, 899990), "b": (4096, 65536), "c": (16, 899990)}           # the k_textgen chunks that fill the input
STEP_LIMIT_S = {"a": 420, "b": 300, "c": 120}
LEVEL = 9


def timed(fn):
    import torch
    ms = []
    for it in range(4):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        torch.cuda.synchronize()
        if it >= 1:
            ms.append(a.elapsed_time(b))
    return r, [round(x, 3) for x in ms]


def step(which):
    import torch
    from netty_amd import batch as B
    n, L = BATCH[which]
    dev = torch.device("cuda:0")
    src = torch.empty(n * L, dtype=torch.uint8, device=dev)
    B.textgen(src, 0, *TEXT[which])
    off = torch.arange(n, dtype=torch.int64, device=dev) * L
    ln = torch.full((n,), L, dtype=torch.int32, device=dev)
    if which == "c":
        counts, ms = timed(lambda: B.bzip2_plan(src, off, ln, LEVEL))
        print(json.dumps({"step": "c", "items": n, "bytes_each": L, "level": LEVEL, "blocks": counts.cpu().tolist(), "ms": ms,
                          "in_gib_s": round(n * L / 2**30 / (min(ms) / 1e3), 3)}))
        return
    cap = (B.bzip2_max_compressed_length(L, LEVEL) + 15) // 16 * 16
    ooff = torch.arange(n, dtype=torch.int64, device=dev) * cap
    caps = torch.full((n,), cap, dtype=torch.int32, device=dev)
    max_blocks = n * B.bzip2_blocks_bound(L, LEVEL)
    host = src.cpu().numpy().tobytes()
    res = {}
    for path in ("split", "stream"):
        out = torch.empty(n * cap, dtype=torch.uint8, device=dev)
        kw = {"split": True, "max_blocks": max_blocks} if path == "split" else {}
        (olen, st), ms = timed(lambda: B.bzip2_encode(src, off, ln, out, ooff, caps, LEVEL, **kw))
        assert int((st != 0).sum()) == 0, "bzip2_encode reported a status"
        lens, enc = olen.cpu().tolist(), out.cpu().numpy().tobytes()
        with ThreadPoolExecutor(16) as ex:
            ok = list(ex.map(lambda k: bz2.decompress(enc[k * cap:k * cap + lens[k]]) == host[k * L:(k + 1) * L], range(n)))
        assert all(ok), "a stream does not decompress to its item"
        res[path] = (ms, [enc[k * cap:k * cap + lens[k]] for k in range(n)])
    assert res["split"][1] == res["stream"][1], "the two paths' bytes differ"
    best = {p: min(res[p][0]) for p in res}
    print(json.dumps({"step": which, "items": n, "bytes_each": L, "level": LEVEL, "max_blocks": max_blocks,
                      "compressed_bytes": sum(map(len, res["split"][1])), "split_ms": res["split"][0], "stream_ms": res["stream"][0],
                      "speedup": round(best["stream"] / best["split"], 2), "split_in_gib_s": round(n * L / 2**30 / (best["split"] / 1e3), 3)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=list(STEP_LIMIT_S))
    a = ap.parse_args()
    if a.step:
        return step(a.step)
    for s, limit in STEP_LIMIT_S.items():
        rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", s]).returncode
        if rc != 0:
            sys.exit(f"step {s} ended with status {rc}: nothing more is started")


if __name__ == "__main__":
    main()
