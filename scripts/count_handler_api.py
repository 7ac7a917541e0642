#!/usr/bin/env python3
"""Count what one encode() call of a handle asks of the runtime, from the CSV traces of

    rocprofv3 --hip-trace --kernel-trace --memory-copy-trace --output-format csv -d DIR/NAME -o t -- \\
        python scripts/measure_handlers.py --once NAME

    python scripts/count_handler_api.py DIR      one JSON line: per NAME the counts below

hipMemcpyAsync by direction (the memory-copy trace's records), hipStreamSynchronize, hipMalloc and
kernel launches of the whole process: the handle's construction is in them, the same on both sides
of a comparison."""
import csv
import glob
import json
import os
import sys


def rows(d, suffix):
    out = []
    for p in glob.glob(os.path.join(d, "**", "*" + suffix), recursive=True):
        with open(p, newline="") as f:
            out += list(csv.DictReader(f))
    return out


def main():
    top = sys.argv[1]
    res = {}
    for name in sorted(os.listdir(top)):
        d = os.path.join(top, name)
        if not os.path.isdir(d):
            continue
        api = [r["Function"] for r in rows(d, "hip_api_trace.csv")]
        c = {"hipMemcpyAsync": api.count("hipMemcpyAsync"), "hipStreamSynchronize": api.count("hipStreamSynchronize"),
             "hipMalloc": api.count("hipMalloc"), "kernels": len(rows(d, "kernel_trace.csv"))}
        for r in rows(d, "memory_copy_trace.csv"):
            k = "copy_" + r["Direction"].replace("MEMORY_COPY_", "").lower()
            c[k] = c.get(k, 0) + 1
        res[name] = c
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
