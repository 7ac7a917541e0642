"""Writes the input file of scripts/asan/bzip2_host_fuzz.cpp: the bzip2 tests' valid streams, every proper
prefix of the small ones, the mutated streams and the mutation fuzz, as records of (u32 length, u32 output
capacity, bytes).  Usage: python scripts/asan/bzip2_host_fuzz_inputs.py OUT.bin"""
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import bzip2_streams as S  # noqa: E402
from oracle import pyoracle  # noqa: E402


def main(path):
    pyoracle.build()
    recs = []
    for v in S.valid_streams(pyoracle):
        recs.append((v.stream, len(v.data)))
        if len(v.stream) <= 4096:
            recs += [(v.stream[:k], len(v.data)) for k in range(len(v.stream))]
    recs += [(m.stream, m.cap) for m in S.mutants(pyoracle)]
    recs += list(S.fuzz_set())
    with open(path, "wb") as f:
        for s, cap in recs:
            f.write(struct.pack("<II", len(s), cap) + s)
    print(f"{len(recs)} records")


if __name__ == "__main__":
    main(sys.argv[1])
