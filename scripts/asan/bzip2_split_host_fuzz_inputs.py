#!/usr/bin/env python3
"""Writes the input file of scripts/asan/bzip2_split_host_fuzz.cpp: the 40-block stream of the decoder tests, its
failing variants, the decoy streams (tests/bzip2_decoys.py) and 200 single-bit and single-byte mutants of them
(the recipe of bzip2_streams.fuzz_set), as records of a u32 length, a u32 output capacity and the bytes."""
import os
import random
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bzip2_decoys as D  # noqa: E402
import bzip2_handbuilt as H  # noqa: E402


def main(path):
    texts, specs, stream, positions = H.multi_block()
    bases = [(stream, sum(len(t) for t in texts))]
    bases += [(c.stream, c.cap) for c in H.group(512, "streams") if not c.name.endswith("_alone")]
    bases += [(d[1], len(d[5])) for d in D.streams()]
    rng = random.Random(200)
    recs = list(bases)
    for i in range(200):
        s, cap = bases[i % len(bases)]
        b = bytearray(s)
        at = rng.randrange(len(b))
        if i % 2:
            b[at] ^= 1 << rng.randrange(8)
        else:
            b[at] = rng.randrange(256)
        recs.append((bytes(b), cap + 64))
    with open(path, "wb") as f:
        for s, cap in recs:
            f.write(struct.pack("<II", len(s), cap) + s)
    print(f"{len(recs)} records, {len(bases)} bases")


if __name__ == "__main__":
    main(sys.argv[1])
