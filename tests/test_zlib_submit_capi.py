"""nx_zlib_encoder_submit / nx_zlib_decoder_submit without a GPU: the library exports them, _lib declares
them, and their argument checks answer before any GPU call (so NULL handles are enough to reach them)."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = -100
SUBMITS = ("nx_zlib_encoder_submit", "nx_zlib_decoder_submit")


@pytest.fixture(scope="module")
def L():
    from netty_amd import _lib
    return _lib.load()


def test_exported_and_declared(L):
    from netty_amd import _lib
    so = os.path.join(ROOT, "netty_amd", "libnetty_amd.so")
    syms = {l.split()[-1] for l in subprocess.check_output(["nm", "-D", "--defined-only", so], text=True).splitlines() if l.strip()}
    header = open(os.path.join(ROOT, "include", "netty_amd.h")).read()
    for name in SUBMITS:
        assert name in syms and name in _lib.EXPORTED and name + "(" in header
        assert getattr(L, name).restype is C.c_int64


def test_encoder_submit_argument_checks(L):
    h = C.c_void_p(0x1000)  # never dereferenced: every case below fails its check first
    buf = b"abc"
    assert L.nx_zlib_encoder_submit(None, h, buf, 3, 0) == INVALID_ARG
    assert L.nx_zlib_encoder_submit(h, None, buf, 3, 0) == INVALID_ARG
    assert L.nx_zlib_encoder_submit(h, h, None, 3, 0) == INVALID_ARG
    for op in (1, 3, -1):
        assert L.nx_zlib_encoder_submit(h, h, buf, 3, op) == INVALID_ARG


def test_decoder_submit_argument_checks(L):
    h = C.c_void_p(0x1000)
    buf = b"abc"
    consumed = C.c_size_t(7)
    assert L.nx_zlib_decoder_submit(None, h, buf, 3, C.byref(consumed)) == INVALID_ARG
    assert L.nx_zlib_decoder_submit(h, None, buf, 3, C.byref(consumed)) == INVALID_ARG
    assert L.nx_zlib_decoder_submit(h, h, None, 3, C.byref(consumed)) == INVALID_ARG
    assert L.nx_zlib_decoder_submit(h, h, buf, 3, None) == INVALID_ARG
    assert consumed.value == 7


def test_batcher_refuses_unknown_handles():
    """an unknown handle never reaches a native function (it used to fall through to the Snappy submit, or
    die with StopIteration)"""
    from netty_amd import handlers as H
    b = H.Batcher.__new__(H.Batcher)  # no native batcher: the type check comes first
    b._h = None
    with pytest.raises(TypeError):
        b.submit_encode(object(), b"x")
    with pytest.raises(TypeError):
        b.submit_decode(object(), b"x")
