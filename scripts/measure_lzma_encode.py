#!/usr/bin/env python3
"""Rate and ratio of batch.lzma_encode (nx_lzma_encode_batch) on text, and its worst expansion on random bytes.

Steps, each a fresh child process under its own `timeout` (the parent never touches the GPU; the first failing
step ends the run):
  gpu_4096, gpu_65536  device-resident encode of that many items of 64 KiB of k_textgen text at the default
                  settings: HIP events around batch.lzma_encode, 1 warm-up call and 3 timed; 64 streams spread over
                  the batch are decoded by liblzma (Python's lzma) and compared.  The share of each pass is read from
                  `rocprofv3 --kernel-trace --stats -- python scripts/measure_lzma_encode.py --step gpu_4096`.
  ratio           the compressed size of 256 of those items next to liblzma preset 0 on the host and to this
                  project's JdkZlibEncoder (batch.deflate_encode, level 6) and ZstdEncoder (batch.zstd_encode,
                  level 3) on the same bytes.
  random          the worst expansion over random items of 1 .. 65 536 bytes beside the n / 3 + 128 allowance.
--step runs one step.  Prints one JSON line per step.  DESIGN.md "LZMA encode" records the figures.
"""
import argparse
import json
import lzma
import os
import random
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
L = 65536
STEP_LIMIT_S = {"gpu_4096": 240, "gpu_65536": 420, "ratio": 240, "random": 240}


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
    torch, B, dev, src, off, ln = _text(n)
    out, ooff, caps, cap = _slots(torch, dev, n, B.lzma_max_compressed_length(L))
    ms = []
    for it in range(4):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        olen, st = B.lzma_encode(src, off, ln, out, ooff, caps)
        b.record()
        torch.cuda.synchronize()
        if it >= 1:
            ms.append(a.elapsed_time(b))
    assert int((st != 0).sum()) == 0, "lzma_encode reported a status"
    lens = olen.cpu().tolist()
    for k in range(0, n, max(1, n // 64)):
        item = src[k * L:(k + 1) * L].cpu().numpy().tobytes()
        s = out[k * cap:k * cap + lens[k]].cpu().numpy().tobytes()
        d = lzma.LZMADecompressor(format=lzma.FORMAT_ALONE)
        assert d.decompress(s) == item and d.eof and d.unused_data == b"", "a stream does not decode to its item"
    best = min(ms)
    print(json.dumps({"step": "gpu_%d" % n, "items": n, "bytes_each": L, "compressed_bytes": sum(lens), "ms": [round(x, 3) for x in ms],
                      "in_gib_s": round(n * L / 2**30 / (best / 1e3), 3), "ratio": round(n * L / sum(lens), 4)}))


def step_ratio():
    n = 256
    torch, B, dev, src, off, ln = _text(n)
    res = {"step": "ratio", "items": n, "bytes_each": L}
    out, ooff, caps, _ = _slots(torch, dev, n, B.lzma_max_compressed_length(L))
    olen, st = B.lzma_encode(src, off, ln, out, ooff, caps)
    assert int((st != 0).sum()) == 0
    res["lzma_gpu"] = int(olen.sum().item())
    out, ooff, _, _ = _slots(torch, dev, n, B.zstd_max_compressed_length(L))
    olen, st = B.zstd_encode(src, off, ln, out, ooff, level=3)
    assert int((st != 0).sum()) == 0
    res["zstd_gpu"] = int(olen.sum().item())
    out, ooff, _, _ = _slots(torch, dev, n, B.deflate_max_compressed_length(L))
    olen, st = B.deflate_encode(src, off, ln, out, ooff, level=6)
    assert int((st != 0).sum()) == 0
    res["deflate_gpu"] = int(olen.sum().item())
    torch.cuda.synchronize()
    host = src.cpu().numpy().tobytes()
    res["liblzma_preset0"] = sum(len(lzma.compress(host[k * L:(k + 1) * L], format=lzma.FORMAT_ALONE, preset=0)) for k in range(n))
    for k in ("lzma_gpu", "zstd_gpu", "deflate_gpu", "liblzma_preset0"):
        res[k + "_ratio"] = round(n * L / res[k], 4)
    print(json.dumps(res))


def step_random():
    import torch
    from netty_amd import batch as B
    dev = torch.device("cuda:0")
    r = random.Random(1)
    sizes = [1, 2, 5, 13, 50, 200, 500, 1000, 4096, 10000, 65536] * 8
    chunks = [r.randbytes(s) for s in sizes]
    inp, off, ln = B.pack(chunks, dev)
    caps = [B.lzma_max_compressed_length(len(c)) for c in chunks]
    out, ooff = B.out_slots(caps, dev)
    olen, st = B.lzma_encode(inp, off, ln, out, ooff, torch.tensor(caps, dtype=torch.int32))
    torch.cuda.synchronize()
    assert int((st != 0).sum()) == 0
    worst = {}
    for s, w in zip(sizes, olen.cpu().tolist()):
        worst[s] = max(worst.get(s, 0), w - 13 - s)  # bytes the payload adds to the item
    print(json.dumps({"step": "random", "payload_minus_item_bytes": worst, "allowance": {s: s // 3 + 128 for s in worst},
                      "worst_percent_64k": round(100.0 * worst[65536] / 65536, 3)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=list(STEP_LIMIT_S))
    a = ap.parse_args()
    if a.step:
        return step_ratio() if a.step == "ratio" else step_random() if a.step == "random" else step_gpu(int(a.step[4:]))
    for s, limit in STEP_LIMIT_S.items():
        rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", s]).returncode
        if rc != 0:
            sys.exit(f"step {s} ended with status {rc}: nothing more is started")


if __name__ == "__main__":
    main()
