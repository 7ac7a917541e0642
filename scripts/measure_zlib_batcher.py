#!/usr/bin/env python3
"""JdkZlibEncoder / JdkZlibDecoder as batcher jobs, host memory to host memory, next to the same messages
through the synchronous handles.

One 64 KiB k_textgen message per channel, at each channel count.  Steps, each a fresh child process under
its own `timeout` (the parent never touches the GPU; the first failing step ends the run):
  enc_batcher   one encoder job per channel, one flush, wait for every ticket
  enc_sync      the same messages through JdkZlibEncoder.encode, one call per channel
  dec_batcher   zlib level-6 streams of the messages, one decoder job per channel, one flush and its
                continuations; reports the flush rounds the tickets took
  dec_sync      the same streams through JdkZlibDecoder.channel_read
A step times submit .. last result through the Python binding, its per-ticket ctypes calls and copies
included (handles and the first-use workspaces are made before the clock starts), checks every output, and
prints one JSON line.  A batcher step runs a warm-up pass with its own handles and two timed ones; a
synchronous step, at ~24 ms per encode and ~9 ms per read, warms up on 8 channels and times one pass.  The baselines are
the synchronous handles and DESIGN.md's kernel-only figures (24.98 GiB/s deflate, 19.1 GiB/s inflate);
DESIGN.md section 4 "zlib jobs on the batcher" records the figures.
"""
import argparse
import json
import os
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
L = 65536
STEPS = ("enc_batcher", "enc_sync", "dec_batcher", "dec_sync")
STEP_LIMIT_S = 300


def _messages(n):
    import torch
    from netty_amd import batch as B
    src = torch.empty(n * L, dtype=torch.uint8, device="cuda:0")
    B.textgen(src, 0, n, L)
    host = src.cpu().numpy().tobytes()
    return [host[k * L:(k + 1) * L] for k in range(n)]


def step(which, n):
    from netty_amd import handlers as H
    msgs = _messages(n)
    enc = which.startswith("enc")
    inputs = msgs if enc else [zlib.compress(m, 6) for m in msgs]
    _all_msgs, _all_inputs = msgs, inputs
    best, rounds = None, None
    batched = which.endswith("batcher")
    for it in range(3 if batched else 2):  # a warm-up pass, then the timed ones
        if not batched:
            msgs, inputs = (_all_msgs[:8], _all_inputs[:8]) if it == 0 else (_all_msgs, _all_inputs)
        hs = [H.JdkZlibEncoder(H.ZlibWrapper.ZLIB, 6) if enc else H.JdkZlibDecoder(H.ZlibWrapper.ZLIB) for _ in range(len(msgs))]
        b = H.Batcher() if batched else None
        if b and enc:
            b.reserve(1 << 6)
        f0 = b.stats()["flushes"] if b else 0
        t0 = time.perf_counter()
        if b:
            ts = [b.submit_encode(h, x) if enc else b.submit_decode(h, x) for h, x in zip(hs, inputs)]
            b.flush()
            outs = []
            for t in ts:
                b.wait(t)
                outs.append(b"".join(b.result(t)))
        elif enc:
            outs = [h.encode(x) for h, x in zip(hs, inputs)]
        else:
            outs = [b"".join(h.channel_read(x)) for h, x in zip(hs, inputs)]
        dt = time.perf_counter() - t0
        if b:
            rounds = b.stats()["flushes"] - f0
        for m, o in zip(msgs, outs):
            if enc:
                assert zlib.decompressobj(15).decompress(o) == m, "encoder output does not inflate to the message"
            else:
                assert o == m, "decoder output differs from the message"
        for h in hs:
            h.close()
        if b:
            b.close()
        if it and (best is None or dt < best):
            best = dt
    line = {"step": which, "channels": n, "bytes": n * L, "s": round(best, 5), "gib_s": round(n * L / 2**30 / best, 3)}
    if rounds is not None:
        line["flush_rounds"] = rounds
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--step", choices=STEPS)
    a = ap.parse_args()
    if a.step:
        return step(a.step, a.channels[0])
    for n in a.channels:
        for s in STEPS:
            rc = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--step", s,
                                 "--channels", str(n)]).returncode
            if rc != 0:
                sys.exit(f"step {s} at {n} channels ended with status {rc}: nothing more is started")


if __name__ == "__main__":
    main()
