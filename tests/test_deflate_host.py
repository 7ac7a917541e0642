"""Host-only checks of the deflate encoder's C-ABI (no GPU): the output bound and the checksum combine
helpers, against Python's zlib."""
import random
import zlib


def _lib():
    from netty_amd import _lib
    return _lib.load()


def test_deflate_length_bound():
    L = _lib()
    for n in (0, 1, 65535, 65536):
        assert L.nx_deflate_max_compressed_length(n) == n + 5 * -(-n // 65535) + 5, n


def test_checksum_combine_against_zlib():
    L = _lib()
    rng = random.Random(11)
    for k in range(200):
        la = 0 if k % 17 == 0 else rng.randrange(0, 5000)
        lb = 0 if k % 13 == 0 else rng.randrange(0, 5000)
        a, b = rng.randbytes(la), rng.randbytes(lb)
        assert L.nx_crc32_combine(zlib.crc32(a), zlib.crc32(b), lb) == zlib.crc32(a + b), (la, lb)
        assert L.nx_adler32_combine(zlib.adler32(a), zlib.adler32(b), lb) == zlib.adler32(a + b), (la, lb)


def test_checksum_combine_long_second_half():
    """len_b up to 2^33 by arithmetic on short data: a run of 2^k zero bytes is two runs of 2^(k-1),
    so its checksums follow from the combine itself, and appending it in one step must equal
    appending its halves one after the other (checked against zlib while the run is short)."""
    L = _lib()
    a = bytes(range(1, 200))
    ca, aa = zlib.crc32(a), zlib.adler32(a)
    zc, za, n = zlib.crc32(b"\0"), zlib.adler32(b"\0"), 1  # checksums of n zero bytes
    for k in range(34):
        if n <= 1 << 16:
            assert zc == zlib.crc32(bytes(n)) and za == zlib.adler32(bytes(n))
            assert L.nx_crc32_combine(ca, zc, n) == zlib.crc32(a + bytes(n))
            assert L.nx_adler32_combine(aa, za, n) == zlib.adler32(a + bytes(n))
        if k:  # a || 0^n in one step == (a || 0^(n/2)) || 0^(n/2)
            assert L.nx_crc32_combine(ca, zc, n) == L.nx_crc32_combine(L.nx_crc32_combine(ca, hc, n // 2), hc, n // 2)
            assert L.nx_adler32_combine(aa, za, n) == L.nx_adler32_combine(L.nx_adler32_combine(aa, ha, n // 2), ha, n // 2)
        hc, ha = zc, za
        zc, za, n = L.nx_crc32_combine(zc, zc, n), L.nx_adler32_combine(za, za, n), 2 * n
    assert n == 1 << 34
    # Adler32 of 2^33 zero bytes in closed form: s1 = 1, s2 = 2^33 mod 65521
    assert ha == ((1 << 33) % 65521) << 16 | 1


def test_python_names():
    import netty_amd
    from netty_amd import batch
    assert netty_amd.ZlibWrapper.GZIP == 1 and netty_amd.JdkZlibEncoder is not None
    assert batch.WS_DEFLATE_ENC == 6 and batch.deflate_max_compressed_length(65536) == 65536 + 15
