"""Content checksums on the host: XXH64 of csrc/zstd_decode_core.hpp through nx_zstd_decode_host_ex with
NX_ZSTD_DECODE_VERIFY_CHECKSUM, against frames whose checksum xxhash computed and libzstd accepts.  The
generator is pinned first: libzstd (through pyarrow) decodes every checksummed frame of the tests and
rejects it after one flipped checksum bit.  No GPU."""
import pytest

import zstd_checksum_inputs as K
import zstd_decode_inputs as I
import zstd_handbuilt as HB

pa = pytest.importorskip("pyarrow")
pytest.importorskip("xxhash")


@pytest.fixture(scope="module")
def L():
    from netty_amd import _lib
    return _lib.load()


def test_checksum_generator_is_pinned_by_libzstd(oracle):
    for name, f, want in K.cases(oracle):
        assert f[4] & 4, name
        assert I.unzstd(f, len(want)) == want, name
        with pytest.raises(Exception):
            I.unzstd(K.wrong_checksum(f, byte=len(want) % 4, bit=len(want) % 8), len(want))


def test_raw_block_sizes_cover_every_tail_path(L, oracle):
    got = {name: K.host_decode(L, f, len(want), K.VERIFY) for name, f, want in K.cases(oracle) if name.startswith("raw_")}
    assert len(got) == len(K.RAW_SIZES) == 18
    for name, f, want in K.cases(oracle):
        if name in got:
            assert got[name] == (K.OK, want, len(f)), name


def test_checksummed_frames(L, oracle):
    """the hash spans blocks; libzstd's frames; a frame without content size; consumed counts the four bytes"""
    for name, f, want in K.cases(oracle):
        assert K.host_decode(L, f, len(want), K.VERIFY) == (K.OK, want, len(f)), name
        assert K.host_decode(L, f + I.TRAILING, len(want) + 5, K.VERIFY) == (K.OK, want, len(f)), name


def test_each_checksum_byte_is_compared(L, oracle):
    for name, f, want in K.cases(oracle):
        for byte in range(4):
            st, out, used = K.host_decode(L, K.wrong_checksum(f, byte, bit=(byte * 3 + len(want)) % 8), len(want), K.VERIFY)
            assert (st, used) == (K.CHECKSUM, 0) and out == want, (name, byte, st)


def test_checksum_cut_short(L, oracle):
    for name, f, want in K.cases(oracle):
        for cut in range(1, 5):
            st, out, used = K.host_decode(L, f[:-cut], len(want), K.VERIFY)
            assert (st, used) == (K.TRUNCATED, 0) and out == want, (name, cut, st)


def test_without_the_flag_a_checksummed_frame_is_refused(L, oracle):
    import ctypes as C
    for name, f, want in K.cases(oracle):
        assert K.host_decode(L, f, len(want), 0) == (K.UNSUPPORTED, b"", 0), name
        ol, co = C.c_size_t(0), C.c_size_t(0)
        out = (C.c_uint8 * (len(want) + 1))()
        assert L.nx_zstd_decode_host(f, len(f), out, len(want), C.byref(ol), C.byref(co)) == K.UNSUPPORTED, name


def test_frames_without_a_checksum_are_unaffected(L, oracle):
    for c in I.libzstd_frames(oracle):
        if c.n <= 5000:
            assert K.host_decode(L, c.frame, c.n, K.VERIFY) == (K.OK, c.data, len(c.frame)), (c.kind, c.n, c.level)
    for name, (f, want) in HB.cases().items():
        assert K.host_decode(L, f, len(want), K.VERIFY) == (K.OK, want, len(f)), name
    for name, (f, status) in HB.malformed().items():
        if name != "checksum_flag":
            assert K.host_decode(L, f, 4096, K.VERIFY)[0] == status, name
    f, _ = HB.malformed()["checksum_flag"]  # four zero bytes are not its checksum
    assert K.host_decode(L, f, 4096, K.VERIFY)[0] == K.CHECKSUM


def test_unknown_flag_bits(L, oracle):
    name, f, want = K.cases(oracle)[5]
    for flags in (2, 3, 0x80000000, 0x80000001):
        assert K.host_decode(L, f, len(want), flags) == (K.INVALID_ARG, b"", 0), flags
    assert L.nx_zstd_decode_batch_ex(*([None] * 9), 0, 2, None) == K.INVALID_ARG  # answered before anything is looked at
    assert L.nx_zstd_decode_batch_ex(*([None] * 9), 0, 1, None) == K.OK


def test_status_string():
    from netty_amd import _lib
    assert _lib.status_string(K.CHECKSUM) == "Restored data doesn't match checksum"
