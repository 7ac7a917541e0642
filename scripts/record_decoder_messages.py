#!/usr/bin/env python3
"""Record what every synchronous decoder handle delivers for the read sequences of
tests/decoder_sequences.py: per read the SHA-256 and length of each message (or the exception) and the
bytes left in the cumulation, and is_closed() and stats() at the end, into
tests/golden/decoder_messages.json, which tests/test_gpu_decoder_messages.py compares a later build
against.  Run it on the commit whose behaviour is to be kept (a GPU is needed):

    python scripts/record_decoder_messages.py [--lib path/to/libnetty_amd.so] [--out file.json]

Every sequence runs twice, on two fresh handles; a case whose two runs differ is not recorded (it is
listed under "unstable" instead, and the script exits with status 1)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", help="the library to record from (default: the tree's netty_amd/libnetty_amd.so)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "decoder_messages.json"))
    a = ap.parse_args()
    if a.lib:  # the package's own import loads the tree's library: stand in for it, so that only a.lib is loaded
        import types
        pkg = types.ModuleType("netty_amd")
        pkg.__path__ = [os.path.join(ROOT, "netty_amd")]
        sys.modules["netty_amd"] = pkg
    from netty_amd import _lib
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    from netty_amd import handlers as H
    import decoder_sequences as S

    rec, unstable = {}, []
    for case in S.cases():
        first, second = S.run(H, case), S.run(H, case)
        if first != second:
            unstable.append(case[0])
            continue
        rec[case[0]] = {"input_sha256": S.input_digest(case), **first}
    with open(a.out, "w") as f:
        json.dump({"cases": rec, "unstable": unstable}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(rec)} cases, {len(unstable)} unstable {unstable}")
    return 1 if unstable else 0


if __name__ == "__main__":
    sys.exit(main())
