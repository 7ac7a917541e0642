"""The bytes of nx_lzma_encode_host and nx_brotli_encode_host, pinned: SHA-256 of every stream against
tests/golden/encode_host_digests.json.  The GPU tests hold the kernels to the host encoders, and both run the
same matcher, so a change that moves both would pass them all; this test is what notices it.

The digests were recorded from the commit that added the Brotli encoder.  A change that means to move the bytes
regenerates them with `python tests/test_encode_host_digests.py` and says so."""
import hashlib
import json
import os

import brotli_inputs as BI
import lzma_inputs as LI

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encode_host_digests.json")


def digest(result):
    status, stream = result[0], result[1]
    assert status == 0
    return hashlib.sha256(stream).hexdigest()


def compute(B, oracle):
    out = {}
    for lc, lp, pb in LI.PROPS:
        for end_marker in (False, True):
            for name, data in LI.items(oracle):
                key = "lzma/lc%d_lp%d_pb%d_em%d/%s" % (lc, lp, pb, end_marker, name)
                out[key] = digest(B.lzma_encode_host(data, lc, lp, pb, 65536, end_marker))
    for name, data, dict_size in LI.dict_cases():
        out["lzma/dict/%s" % name] = digest(B.lzma_encode_host(data, dict_size=dict_size))
    for lgwin in BI.LGWINS:
        for name, data in BI.items(oracle):
            out["brotli/lgwin%d/%s" % (lgwin, name)] = digest(B.brotli_encode_host(data, lgwin))
    return out


def test_host_encoder_bytes_are_the_recorded_ones(oracle):
    from netty_amd import batch as B
    with open(GOLDEN) as f:
        want = json.load(f)
    got = compute(B, oracle)
    assert sorted(got) == sorted(want)
    moved = [k for k in want if got[k] != want[k]]
    assert not moved, moved


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from netty_amd import batch
    from oracle import pyoracle
    pyoracle.build()
    with open(GOLDEN, "w") as f:
        json.dump(compute(batch, pyoracle), f, indent=0, sort_keys=True)
        f.write("\n")
