#!/usr/bin/env python3
"""Writes tests/golden/brotli_libbrotli_streams.json: the cases of tests/brotli_decode_inputs.py encoded by
libbrotli's own encoder (libbrotlienc.so.1.0.9 through ctypes), each verified with libbrotli's own decoder
before it is written.  The fixture holds the streams, not the plain texts (the tests regenerate those).

    python3 tests/golden/make_brotli_libbrotli_streams.py
"""
import base64
import ctypes as C
import ctypes.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import brotli_decode_inputs as I  # noqa: E402

PROCESS, FLUSH, FINISH = 0, 1, 2
PARAM_MODE, PARAM_QUALITY, PARAM_LGWIN = 0, 1, 2


def _lib(name):
    path = ctypes.util.find_library(name) or "lib%s.so.1" % name
    return C.CDLL(path)


enc = _lib("brotlienc")
dec = _lib("brotlidec")
enc.BrotliEncoderCreateInstance.restype = C.c_void_p
enc.BrotliEncoderCreateInstance.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
enc.BrotliEncoderSetParameter.argtypes = [C.c_void_p, C.c_int, C.c_uint32]
enc.BrotliEncoderDestroyInstance.argtypes = [C.c_void_p]
enc.BrotliEncoderCompressStream.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                            C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
enc.BrotliEncoderIsFinished.argtypes = [C.c_void_p]
dec.BrotliDecoderDecompress.argtypes = [C.c_size_t, C.c_char_p, C.POINTER(C.c_size_t), C.c_char_p]


def encode(data: bytes, quality: int, lgwin: int, mode: int, flush_at=None) -> bytes:
    s = enc.BrotliEncoderCreateInstance(None, None, None)
    assert s
    for p, v in ((PARAM_MODE, mode), (PARAM_QUALITY, quality), (PARAM_LGWIN, lgwin)):
        assert enc.BrotliEncoderSetParameter(s, p, v) == 1
    cap = len(data) + (len(data) >> 2) + 1024
    outbuf = C.create_string_buffer(cap)
    next_out = C.c_void_p(C.addressof(outbuf))
    avail_out = C.c_size_t(cap)
    parts = [(data, FINISH)] if flush_at is None else [(data[:flush_at], FLUSH), (data[flush_at:], FINISH)]
    for chunk, op in parts:
        inbuf = C.create_string_buffer(chunk, len(chunk) + 1)
        next_in = C.c_void_p(C.addressof(inbuf))
        avail_in = C.c_size_t(len(chunk))
        while True:
            assert enc.BrotliEncoderCompressStream(s, op, C.byref(avail_in), C.byref(next_in), C.byref(avail_out), C.byref(next_out), None) == 1
            if avail_in.value == 0 and (op == FLUSH or enc.BrotliEncoderIsFinished(s)):
                break
    assert enc.BrotliEncoderIsFinished(s)
    enc.BrotliEncoderDestroyInstance(s)
    return outbuf.raw[:cap - avail_out.value]


def decode(stream: bytes, size: int) -> bytes:
    out = C.create_string_buffer(size + 1)
    n = C.c_size_t(size + 1)
    assert dec.BrotliDecoderDecompress(len(stream), stream, C.byref(n), out) == 1, "libbrotli refuses its own stream"
    return out.raw[:n.value]


def main():
    streams = []
    for c in I.CASES:
        data = I.plain(c)
        s = encode(data, c["quality"], c["lgwin"], I.MODES[c["mode"]], c.get("flush_at"))
        assert decode(s, len(data)) == data, c["name"]
        d = dict(c)
        d["stream"] = base64.b64encode(s).decode()
        streams.append(d)
    doc = {"encoder": "libbrotlienc 1.0.9", "streams": streams}
    with open(I.GOLDEN, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d streams, %d bytes" % (len(streams), os.path.getsize(I.GOLDEN)))


if __name__ == "__main__":
    main()
