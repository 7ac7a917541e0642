"""The bytes every synchronous encoder handle returns, call by call, against a recording
(tests/golden/handler_bytes.json, written by scripts/record_handler_bytes.py from the commit before the
handles' launch staging was folded into nx::h::EncodeItems), and what the handles do when the caller's
buffer is too small.  The write sequences are in handler_sequences.py."""
import ctypes as C
import json
import os

import pytest

import handler_sequences as S

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

INVALID_ARG = -100  # NX_ERR_INVALID_ARG
CASES = S.cases()


@pytest.fixture(scope="module")
def H():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from netty_amd import handlers
    return handlers


@pytest.fixture(scope="module")
def L():
    from netty_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "handler_bytes.json")) as f:
        return json.load(f)


def test_every_case_is_recorded(golden):
    assert golden["unstable"] == []
    assert sorted(golden["cases"]) == sorted(c[0] for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_recorded_bytes(H, golden, case):
    want = golden["cases"][case[0]]
    assert S.input_digest(case) == want["input_sha256"], "the inputs differ from the recorded run's"
    got = S.digest(S.run(H, case))
    assert [g["len"] for g in got] == [w["len"] for w in want["calls"]]
    assert got == want["calls"]


# ---- capacity: straight through the C ABI, so that out_cap can be chosen
def _call(fn, h, data, cap, fill=0xAA):
    out = (C.c_uint8 * max(cap, 1)).from_buffer_copy(bytes([fill]) * max(cap, 1))
    r = fn(h, data, len(data), out, cap)
    return r, bytes(out)


@pytest.mark.parametrize("codec", ["lz4", "zstd"])
def test_block_buffer_survives_a_failed_flush(H, L, codec):
    """A handle holding a partial buffer takes a write that closes two blocks with one byte too little room:
    NX_ERR_INVALID_ARG, and the same write again with room returns what a twin handle returned."""
    bs = 4096
    make = (lambda: H.Lz4FrameEncoder(bs)) if codec == "lz4" else (lambda: H.ZstdEncoder(3, bs))
    fn = L.nx_lz4_frame_encoder_encode if codec == "lz4" else L.nx_zstd_encoder_encode
    part, big, room = S.mixed(800, 100), S.mixed(801, 2 * bs), 4 * bs + 4096
    e, twin = make(), make()
    try:
        for x in (e, twin):
            assert _call(fn, x._h, part, room)[0] == 0
        n, want = _call(fn, twin._h, big, room)
        assert n > 0
        r, out = _call(fn, e._h, big, n - 1)
        assert r == INVALID_ARG
        r, out = _call(fn, e._h, big, room)
        assert r == n and out[:n] == want[:n]
        assert e.flush() == twin.flush()  # and the same 100 bytes stay buffered
    finally:
        e.close()
        twin.close()


def _short_cases(H, L):
    fl = L.nx_fastlz_frame_encoder_encode
    return {
        "snappy": (lambda: H.SnappyFrameEncoder(), L.nx_snappy_frame_encoder_encode, L.nx_snappy_frame_max_encoded_length),
        "fastlz": (lambda: H.FastLzFrameEncoder(1, True), lambda h, d, n, o, c: fl(h, d, 0, n, o, c), L.nx_fastlz_frame_max_encoded_length),
        "lzf": (lambda: H.LzfEncoder(), L.nx_lzf_encoder_encode, L.nx_lzf_frame_max_encoded_length),
        "zlib": (lambda: H.JdkZlibEncoder(H.ZlibWrapper.ZLIB, 6), L.nx_zlib_encoder_encode, L.nx_zlib_max_encoded_length),
    }


@pytest.mark.parametrize("codec", ["snappy", "fastlz", "lzf", "zlib"])
def test_short_buffer_is_refused_untouched(H, L, codec):
    """out_cap one below the handle's bound: NX_ERR_INVALID_ARG, not a byte written, and the handle goes on as
    a twin that never saw the call (Snappy's stream header, zlib's header are still to come)."""
    make, fn, bound = _short_cases(H, L)[codec]
    data = S.mixed(810, 70000)
    cap = bound(len(data))
    e, twin = make(), make()
    try:
        r, out = _call(fn, e._h, data, cap - 1)
        assert r == INVALID_ARG
        assert out == b"\xaa" * (cap - 1)
        n, want = _call(fn, twin._h, data, cap)
        r, out = _call(fn, e._h, data, cap)
        assert n > 0 and r == n and out[:n] == want[:n]
    finally:
        e.close()
        twin.close()
