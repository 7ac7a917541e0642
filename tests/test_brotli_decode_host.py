"""nx_brotli_decode_host, the CPU run of the Brotli decoder's format core (csrc/brotli_decode_core.hpp), against
libbrotli: its encoder made the fixture's streams, its decoder (through pyarrow, and through ctypes for the error
codes) says what every stream holds.  Also the dictionary, the transforms, the census of what
the stream set exercises, this library's own encoder, and one run of the host code under ASan and UBSan as a
stand-alone program.  No GPU."""
import ctypes as C
import ctypes.util
import os
import random
import subprocess
import zlib

import pytest

import brotli_decode_streams as S
import brotli_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK = 0
GUARD = S.GUARD


@pytest.fixture(scope="module")
def B():
    from netty_amd import batch
    return batch


@pytest.fixture(scope="module")
def L():
    from netty_amd import _lib
    return _lib.load()


def _cdll(name):
    path = ctypes.util.find_library(name)
    if not path:
        pytest.skip("lib%s is not installed" % name)
    return C.CDLL(path)


def _decode(L, stream, cap):
    """(status, output, consumed); the slot lies between guards, which must come back untouched"""
    buf = (C.c_uint8 * (cap + 2 * GUARD)).from_buffer(bytearray(b"\xa5" * (cap + 2 * GUARD)))
    ol, co = C.c_size_t(0), C.c_size_t(0)
    st = L.nx_brotli_decode_host(stream, len(stream), C.byref(buf, GUARD), cap, C.byref(ol), C.byref(co), None)
    raw = bytes(buf)
    assert raw[:GUARD] == b"\xa5" * GUARD and raw[GUARD + cap:] == b"\xa5" * GUARD, "a byte was written outside the slot"
    assert ol.value <= cap
    return st, raw[GUARD:GUARD + ol.value], co.value


def test_dictionary(B):
    d = B.brotli_dictionary()
    assert len(d) == 122784
    assert zlib.crc32(d) == 0x5136CB04


def test_transforms_match_libbrotli(B):
    com = _cdll("brotlicommon")
    com.BrotliGetTransforms.restype = C.c_void_p
    com.BrotliTransformDictionaryWord.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_void_p, C.c_int]
    tr = com.BrotliGetTransforms()
    rng = random.Random(7)
    d = B.brotli_dictionary()
    for n in range(4, 25):
        words = [bytes(rng.randrange(256) for _ in range(n)), bytes(rng.choice(b"abcxyzABZ \xc3\xa9\xe2\x82\xac") for _ in range(n)), d[1000 * n:1001 * n]]
        for w in words:
            for t in range(121):
                dst = C.create_string_buffer(64)
                k = com.BrotliTransformDictionaryWord(dst, w, n, tr, t)
                assert B.brotli_transform_word(t, w) == dst.raw[:k], (t, w)


def test_valid_streams(L):
    for name, s, plain in S.valid():
        st, out, used = _decode(L, s, len(plain))
        assert (st, used) == (OK, len(s)), name
        assert out == plain, name
        st, out, used = _decode(L, s + b"\x9c\xff\x00\x37\x01", len(plain) + 3)
        assert (st, used, out) == (OK, len(s), plain), name


def test_valid_streams_pyarrow():
    """libbrotli's decoder, through pyarrow, makes the same plain text of every valid stream, the empty ones too."""
    import pyarrow as pa
    for name, s, plain in S.valid():
        assert pa.CompressedInputStream(pa.BufferReader(s), "brotli").read() == plain, name


def _libbrotli_error(dec, stream):
    st = dec.BrotliDecoderCreateInstance(None, None, None)
    ib = C.create_string_buffer(stream, len(stream) + 1)
    ni, ai = C.c_void_p(C.addressof(ib)), C.c_size_t(len(stream))
    ob = C.create_string_buffer(1 << 16)
    no, ao = C.c_void_p(C.addressof(ob)), C.c_size_t(1 << 16)
    r = dec.BrotliDecoderDecompressStream(st, C.byref(ai), C.byref(ni), C.byref(ao), C.byref(no), None)
    code = dec.BrotliDecoderGetErrorCode(st)
    dec.BrotliDecoderDestroyInstance(st)
    return r, code


def test_invalid_streams_host(L):
    want = set(S.CODES) - {"TRUNCATED", "OUTPUT_FULL"}
    assert {c for _, _, c in __import__("brotli_handbuilt").INVALID} == want
    for name, s, code in S.invalid():
        st, _, used = _decode(L, s, 66000)
        assert (st, used) == (code, 0), name


def test_invalid_streams_libbrotli():
    dec = _cdll("brotlidec")
    dec.BrotliDecoderCreateInstance.restype = C.c_void_p
    dec.BrotliDecoderCreateInstance.argtypes = [C.c_void_p] * 3
    dec.BrotliDecoderDestroyInstance.argtypes = [C.c_void_p]
    dec.BrotliDecoderGetErrorCode.argtypes = [C.c_void_p]
    dec.BrotliDecoderDecompressStream.argtypes = [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                                  C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    for name, s, code in __import__("brotli_handbuilt").INVALID:
        r, err = _libbrotli_error(dec, s)
        assert (r, err) == (0, S.LIBBROTLI[code]), name
    for name, s, _ in S.valid()[-6:]:  # and it accepts the hand-built valid ones
        assert _libbrotli_error(dec, s) == (1, 1), name


def test_truncated(L):
    for name, s in S.cuts():
        st, _, used = _decode(L, s, 80000)
        assert (st, used) == (S.CODES["TRUNCATED"], 0), name


def test_output_full(L):
    for name, s, cap in S.small_caps():
        st, _, used = _decode(L, s, cap)
        assert (st, used) == (S.CODES["OUTPUT_FULL"], 0), name


def test_census(B):
    """The stream set exercises everything the census lists: a condition, not a measurement."""
    total = None
    for name, s, plain in S.valid():
        st, _, _, c = B.brotli_decode_host(s, len(plain), stats=True)
        assert st == OK, name
        if total is None:
            total = c
            continue
        for k, v in c.items():
            if isinstance(v, list):
                total[k] = [max(a, b) if k.startswith("max_") else (a | b if k == "transforms" else a + b) for a, b in zip(total[k], v)]
            elif k.startswith("max_"):
                total[k] = max(total[k], v)
            elif k in ("context_modes", "ring_codes", "simple_four_shapes"):
                total[k] |= v
            else:
                total[k] += v
    print(total)
    for k in ("mb_compressed", "mb_uncompressed", "mb_metadata", "mb_empty_last", "metadata_skipped", "cmap_rle_runs", "cmap_imtf",
              "max_npostfix", "max_ndirect", "complex_codes", "repeat_16", "repeat_17", "dict_refs"):
        assert total[k] > 0, k
    assert all(v > 1 for v in total["max_nbltypes"]), total["max_nbltypes"]
    assert total["max_ntrees_l"] > 1 and total["max_ntrees_d"] > 1
    assert total["context_modes"] == 0xF
    assert all(v > 0 for v in total["simple_codes"]) and total["simple_four_shapes"] == 3
    assert total["ring_codes"] == 0xFFFF
    assert total["transforms"] == [0xFFFFFFFF] * 3 + [(1 << 25) - 1]


def test_own_encoder_round_trip(B, L):
    """nx_brotli_encode_host's streams at every window decode back to their inputs."""
    items = [(n, d) for n, d in brotli_inputs.directed() if n in ("len0", "len3", "few3", "fibonacci", "insert130", "copy134", "far", "ring", "window10")]
    assert len(items) == 9
    for lgwin in range(10, 25):
        for name, data in items:
            est, s = B.brotli_encode_host(data, lgwin=lgwin)
            assert est == 0
            st, dec, used = _decode(L, s, len(data))
            assert (st, used) == (OK, len(s)) and dec == data, (name, lgwin)


def test_host_sanitizers(tmp_path):
    """The host decoder as a stand-alone program under ASan and UBSan, over every stream of the set, the cuts
    and the small capacities: exit 0 and no report."""
    cxx = next((c for c in ("g++", "c++", "clang++") if subprocess.run(["which", c], capture_output=True).returncode == 0), None)
    if not cxx:
        pytest.skip("no host C++ compiler")
    items = [(s, len(p) + 8) for _, s, p in S.valid()] + [(s, 64) for _, s, _ in S.invalid()]
    items += [(s, 80000) for _, s in S.cuts()] + [(s, cap) for _, s, cap in S.small_caps()]
    path = tmp_path / "streams.bin"
    with open(path, "wb") as f:
        for s, cap in items:
            f.write(len(s).to_bytes(4, "little") + cap.to_bytes(4, "little") + s)
    main = tmp_path / "main.cpp"
    main.write_text(
        '#include <stdio.h>\n#include <stdint.h>\n#include <stdlib.h>\n#include <vector>\n#include "netty_amd.h"\n'
        'int main(int argc, char** argv) {\n    FILE* f = fopen(argv[1], "rb");\n    if (!f) return 2;\n    uint32_t h[2];\n    unsigned n = 0;\n'
        '    while (fread(h, 4, 2, f) == 2) {\n        std::vector<uint8_t> in(h[0]), out(h[1]);\n'
        '        if (h[0] && fread(in.data(), 1, h[0], f) != h[0]) return 3;\n        size_t ol = 0, co = 0;\n        nx_brotli_decode_stats st;\n'
        '        nx_brotli_decode_host(in.data(), in.size(), out.data(), out.size(), &ol, &co, &st);\n        if (ol > out.size()) return 4;\n        ++n;\n    }\n'
        '    printf("%u streams\\n", n);\n    return 0;\n}\n')
    exe = tmp_path / "brotli_decode_host_san"
    src = os.path.join(ROOT, "netty_amd", "csrc", "brotli_decode_host.cpp")
    dict_path = os.path.join(ROOT, "netty_amd", "csrc", "brotli_dictionary.bin")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                           '-DNX_BROTLI_DICT_PATH="%s"' % dict_path, str(main), src, "-o", str(exe)])
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip() == "%d streams" % len(items)
