#!/usr/bin/env python3
"""Rate of batch.zstd_decode (nx_zstd_decode_batch) on text chunks, next to libzstd on 16 host threads.

Steps, each a fresh child process under its own `timeout` (the parent never touches the GPU; the
first failing step ends the run):
  gpu_encoder  n x 64 KiB k_textgen chunks as the project's encoder wrote them, then decoded: HIP events
               around batch.zstd_decode, 2 warm-up calls and 5 timed, output checked against the source.
  gpu_encoder_checksum
               the same frames with a content checksum each (the Content_Checksum flag set, the low 32 bits of
               XXH64 of the chunk appended), decoded with verify_checksum=True: what verification costs.
  gpu_libzstd3 the first `sample` chunks compressed by libzstd level 3 on the host, decoded the same way.
  host         libzstd's own decode of the same `sample` level-3 frames on 16 threads.
Prints one JSON line per step.  DESIGN.md section 4 "Zstandard decode" records the figures.
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
STEP_LIMIT_S = {"gpu_encoder": 240, "gpu_encoder_checksum": 300, "gpu_libzstd3": 180, "host": 180}


def _time_decode(B, torch, enc, eoff, elen, n, dev, src, verify=False):
    off = torch.arange(n, dtype=torch.int64, device=dev) * L
    dec = torch.empty(n * L, dtype=torch.uint8, device=dev)
    cap = torch.full((n,), L, dtype=torch.int32, device=dev)
    ms = []
    for it in range(7):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        cons, olen, st = B.zstd_decode(enc, eoff, elen, dec, off, cap, verify_checksum=True) if verify else \
            B.zstd_decode(enc, eoff, elen, dec, off, cap)
        b.record()
        torch.cuda.synchronize()
        if it >= 2:
            ms.append(a.elapsed_time(b))
    assert int((olen != L).sum()) == 0 and int((st != 0).sum()) == 0, "zstd_decode did not produce every chunk"
    assert torch.equal(cons, elen), "consumed differs from the frame lengths"
    assert torch.equal(dec, src), "zstd_decode output differs from the source"
    return ms


def _level3(chunks):
    import pyarrow as pa
    codec = pa.Codec("zstd", compression_level=3)
    with ThreadPoolExecutor(16) as ex:
        return list(ex.map(lambda c: codec.compress(c).to_pybytes(), chunks))


def _add_checksums(torch, enc, eoff, elen, slot, src, n):
    """make every frame of enc a checksummed one, in place; returns the new lengths"""
    import numpy as np
    import xxhash
    host = src.cpu().numpy()
    sums = np.array([xxhash.xxh64_intdigest(host[k * L:(k + 1) * L]) & 0xFFFFFFFF for k in range(n)], dtype="<u4")
    assert int(elen.max()) + 4 <= slot
    enc[eoff + 4] |= 4  # Frame_Header_Descriptor bit 2
    at = (eoff + elen.to(torch.int64))[:, None] + torch.arange(4, device=enc.device)[None, :]
    enc[at] = torch.from_numpy(sums.view(np.uint8).reshape(n, 4)).to(enc.device)
    return elen + 4


def step_gpu(n, sample, which):
    import torch
    from netty_amd import batch as B
    dev = torch.device("cuda:0")
    n = sample if which == "gpu_libzstd3" else n
    src = torch.empty(n * L, dtype=torch.uint8, device=dev)
    B.textgen(src, 0, n, L)
    if which != "gpu_libzstd3":
        off = torch.arange(n, dtype=torch.int64, device=dev) * L
        ln = torch.full((n,), L, dtype=torch.int32, device=dev)
        slot = (B.zstd_max_compressed_length(L) + 127) // 128 * 128
        enc = torch.empty(n * slot, dtype=torch.uint8, device=dev)
        eoff = torch.arange(n, dtype=torch.int64, device=dev) * slot
        elen, est = B.zstd_encode(src, off, ln, enc, eoff)
        torch.cuda.synchronize()
        assert int((est != 0).sum()) == 0
        if which == "gpu_encoder_checksum":
            elen = _add_checksums(torch, enc, eoff, elen, slot, src, n)
    else:
        host = src.cpu().numpy().tobytes()
        enc, eoff, elen = B.pack(_level3([host[k * L:(k + 1) * L] for k in range(n)]), dev)
    comp = int(elen.sum())
    ms = _time_decode(B, torch, enc, eoff, elen, n, dev, src, verify=which == "gpu_encoder_checksum")
    best = min(ms)
    print(json.dumps({"step": which, "chunks": n, "compressed_bytes": comp, "ms": [round(x, 3) for x in ms],
                      "out_gib_s": round(n * L / 2**30 / (best / 1e3), 3)}))


def step_host(sample):
    import pyarrow as pa
    from oracle import pyoracle as O
    O.build()
    zs = _level3([O.textgen_chunk(k, L) for k in range(sample)])
    codec = pa.Codec("zstd")

    def run(part):
        return sum(len(codec.decompress(z, decompressed_size=L)) for z in part)

    parts = [zs[k::16] for k in range(16)]
    best = None
    for _ in range(3):
        t = time.perf_counter()
        with ThreadPoolExecutor(16) as ex:
            total = sum(ex.map(run, parts))
        dt = time.perf_counter() - t
        best = dt if best is None or dt < best else best
    assert total == sample * L
    print(json.dumps({"step": "host", "chunks": sample, "threads": 16, "s": round(best, 4),
                      "out_gib_s": round(sample * L / 2**30 / best, 3)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=32768)
    ap.add_argument("--sample", type=int, default=4096)
    ap.add_argument("--step", choices=list(STEP_LIMIT_S))
    a = ap.parse_args()
    if a.step == "host":
        return step_host(a.sample)
    if a.step:
        return step_gpu(a.chunks, a.sample, a.step)
    for s, limit in STEP_LIMIT_S.items():
        rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", s,
                             "--chunks", str(a.chunks), "--sample", str(a.sample)]).returncode
        if rc != 0:
            sys.exit(f"step {s} ended with status {rc}: nothing more is started")


if __name__ == "__main__":
    main()
