#!/usr/bin/env python3
"""batch.bzip2_decode (nx_bzip2_decode_batch, the serial call) next to batch.bzip2_decode(split=True)
(nx_bzip2_decode_batch_split) in one GPU visit, and the scan alone.

Four batches of k_textgen text compressed by libbz2 at level 9: (a) 4 096 streams of 64 KiB, (b) 256 streams of
900 000 bytes, (c) 8 streams of 32 MiB, (d) one stream of 64 MiB.  Each step is a fresh child process under its
own `timeout` (the parent never touches the GPU; the first failing step ends the run).  A step times, with HIP
events, 1 warm-up call and 3 timed calls of the serial call, the split call (max_blocks given, so the call does
not synchronise) and nx_bzip2_scan_batch, and checks every output against the source; the step "handle" times
one handlers.Bzip2Decoder call on (d) from host bytes to messages (wall time).  --step runs one step.
Prints one JSON line per step.  DESIGN.md "Bzip2 decode, split" records the figures.
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
BATCH = {"a": (4096, 65536), "b": (256, 900000), "c": (8, 32 << 20), "d": (1, 64 << 20)}
STEP_LIMIT_S = {"a": 300, "b": 420, "c": 600, "d": 900, "handle": 420}
PIECE = 8 << 20  # textgen runs over pieces of this size


def _timed(torch, fn):
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
    if L <= PIECE:
        B.textgen(src, 0, n, L)
    else:
        B.textgen(src, 0, n * L // PIECE, PIECE)
    host = src.cpu().numpy().tobytes()
    with ThreadPoolExecutor(16) as ex:
        zs = list(ex.map(lambda k: bz2.compress(host[k * L:(k + 1) * L], 9), range(n)))
    enc, eoff, elen = B.pack(zs, dev)
    off = torch.arange(n, dtype=torch.int64, device=dev) * L
    cap = torch.full((n,), L, dtype=torch.int32, device=dev)
    total = int(B.bzip2_scan(enc, eoff, elen, max_blocks=int(elen.sum()) // 6 + 1)[2].sum())
    out = {"step": which, "streams": n, "bytes_each": L, "compressed_bytes": int(elen.sum()), "candidates": total}

    def check(r, dec):
        assert int((r[0] != L).sum()) == 0 and int((r[2] != 0).sum()) == 0, "not every stream decoded"
        assert torch.equal(r[1], elen) and torch.equal(dec, src), "output differs from the source"

    for name, kw in (("serial", {}), ("split", {"split": True, "max_blocks": total})):
        dec = torch.zeros(n * L, dtype=torch.uint8, device=dev)
        r, ms = _timed(torch, lambda: B.bzip2_decode(enc, eoff, elen, dec, off, cap, **kw))
        check(r, dec)
        out[name + "_ms"] = ms
        out[name + "_out_gib_s"] = round(n * L / 2**30 / (min(ms) / 1e3), 3)
        if name == "split":
            out["blocks"] = int(r[3].sum())
    _, ms = _timed(torch, lambda: B.bzip2_scan(enc, eoff, elen, max_blocks=total))
    out["scan_ms"] = ms
    out["scan_in_gb_s"] = round(int(elen.sum()) / 1e9 / (min(ms) / 1e3), 2)
    print(json.dumps(out))


def step_handle():
    """One handlers.Bzip2Decoder call on (d): host bytes in, messages out (upload, scan, one decode sequence, two
    copies back), wall time; a fresh handle per call, 1 warm-up and 3 timed."""
    import time
    import torch
    from netty_amd import batch as B
    from netty_amd import handlers as Hd
    n, L = BATCH["d"]
    src = torch.empty(n * L, dtype=torch.uint8, device=torch.device("cuda:0"))
    B.textgen(src, 0, n * L // PIECE, PIECE)
    host = src.cpu().numpy().tobytes()
    z = bz2.compress(host, 9)
    ms = []
    for it in range(4):
        d = Hd.Bzip2Decoder()
        t = time.perf_counter()
        out = d.channel_read(z)
        dt = (time.perf_counter() - t) * 1e3
        assert b"".join(out) == host and d.is_closed(), "the handle's messages differ from the source"
        st = d.stats()
        d.close()
        if it >= 1:
            ms.append(round(dt, 3))
    print(json.dumps({"step": "handle", "bytes": L, "compressed_bytes": len(z), "wall_ms": ms, "stats": st,
                      "out_gib_s": round(L / 2**30 / (min(ms) / 1e3), 3)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=list(STEP_LIMIT_S))
    a = ap.parse_args()
    if a.step:
        return step_handle() if a.step == "handle" else step(a.step)
    for s, limit in STEP_LIMIT_S.items():
        rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", s]).returncode
        if rc != 0:
            sys.exit(f"step {s} ended with status {rc}: nothing more is started")


if __name__ == "__main__":
    main()
