"""One flush that holds every kind of batcher job at once (include/netty_amd.h section 3): Snappy encoder
and decoder jobs (copied and registered inputs, validating and not), FastLZ / LZF / LZ4 encoder jobs and
FastLZ / LZF / LZ4 decoder jobs (checksums validated, and for one FastLZ decoder not), submitted interleaved into one batch, so
that every array of the flush's upload, every codec launch list and every result region is populated
together.  Two decoder inputs fail (a Snappy chunk with a wrong stored CRC, a damaged LZ4 block) between
jobs that pass.  Every job's result equals that of a fresh synchronous handle of the same kind fed the
same calls: the bytes, and for the failing jobs the status and the message text."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nx():
    import netty_amd
    return netty_amd


def _sync(call):
    """(messages, status, error text, exception type) of one synchronous handle call"""
    try:
        out = call()
    except Exception as e:  # a DecoderException carries the status and what decode() fired before failing
        return list(e.decoded), e.status, str(e), type(e)
    return (out if isinstance(out, list) else [out]), 0, None, None


def _job(nx, b, t):
    """the same of batcher job t, with the status and text nx_batcher_result returns"""
    from netty_amd import _lib
    msgs, n, err = C.POINTER(_lib.NxMsg)(), C.c_size_t(0), C.c_char_p()
    b.wait(t)
    rc = _lib.load().nx_batcher_result(b._h, t, C.byref(msgs), C.byref(n), C.byref(err))
    text = err.value.decode() if err.value else None
    try:
        return b.result(t), rc, text, None
    except nx.DecoderException as e:
        return e.decoded, rc, text, type(e)


def test_one_flush_with_every_kind_of_job(nx, oracle):
    seeds = iter(range(1, 1000))

    def text(n):
        return oracle.textgen_chunk(next(seeds), n)

    def msgs(*lens):  # every third message incompressible
        return [oracle.java_random_bytes(s, n) if s % 3 == 0 else oracle.textgen_chunk(s, n)
                for n, s in zip(lens, seeds)]

    def frames(enc, ms, after=lambda e: b""):
        return [enc.encode(m) + after(enc) for m in ms]

    def flushed(e):
        return e.flush()

    # Lengths: 17 is below SnappyFrameEncoder's MIN_COMPRESSIBLE_LENGTH (an uncompressed chunk), 19 above
    # it; 70 001 bytes are three Snappy slices (two with jumbo frames) and two 65 536-byte LZ4 blocks.
    # ---- decoder inputs, made by synchronous encoders
    sn_a = frames(nx.SnappyFrameEncoder(), msgs(301, 17, 70001, 0, 19))
    sn_b = frames(nx.SnappyFrameEncoder(jumbo=True), msgs(70001, 1, 5003))
    sn_c = frames(nx.SnappyFrameEncoder(), msgs(19, 5003, 17, 301))
    sn_bad = frames(nx.SnappyFrameEncoder(), [text(5003), text(301), text(19)])
    bad = bytearray(sn_bad[1])  # [type][len u24][masked crc LE][payload]: a wrong stored CRC
    assert bad[0] == 0x00  # a compressed chunk
    bad[5] ^= 0x40
    sn_bad[1] = bytes(bad)
    flz_s = frames(nx.FastLzFrameEncoder(1, True), msgs(301, 0, 70001, 17))
    flz_t = frames(nx.FastLzFrameEncoder(2, True), msgs(19, 5003, 1))
    lzf_s = frames(nx.LzfEncoder(), msgs(5003, 1, 70001, 19))
    lzf_t = frames(nx.LzfEncoder(100), msgs(17, 301, 0))  # a non-compressed block, then a compressed one
    lz4_s = frames(nx.Lz4FrameEncoder(1 << 16), msgs(70001, 17, 301, 0), after=flushed)
    lz4_bad = frames(nx.Lz4FrameEncoder(4096), [text(301), text(5003), text(19)], after=flushed)
    bad = bytearray(lz4_bad[1])  # its first 4096-byte block: a 21-byte header, then the compressed bytes
    assert bad[:8] == b"LZ4Block" and bad[8] & 0xF0 == 0x20  # BLOCK_TYPE_COMPRESSED
    bad[21 + 40] ^= 0xFF
    lz4_bad[1] = bytes(bad)

    # registered memory: one encoder input, and one decoder's reads (each a whole number of chunks)
    reg_in = text(70001)
    cells = [reg_in] + sn_c
    size = sum((len(c) + 15) & ~15 for c in cells) + 16
    arena = (C.c_uint8 * size)()
    base, addr, pos = C.addressof(arena), {}, 0
    for c in cells:
        C.memmove(base + pos, c, len(c))
        addr[id(c)] = base + pos
        pos += (len(c) + 15) & ~15

    b = nx.Batcher()
    chans = []  # (synchronous call, batcher submit, inputs)

    def enc(make, ins):
        s, e = make(), make()

        def sub(m):
            return b.submit_encode(e, m, registered_ptr=addr[id(m)]) if m is reg_in else b.submit_encode(e, m)
        chans.append((s.encode, sub, ins))

    def lz4(block, high, ins):  # encode + flush per message
        s, e = (nx.Lz4FrameEncoder(block, high_compressor=high) for _ in range(2))
        chans.append((lambda m: s.encode(m) + s.flush(), lambda m: b.submit_encode(e, m, op=1), ins))

    def dec(make, ins, registered=False):
        s, d = make(), make()

        def sub(m):
            if not registered:
                return b.submit_decode(d, m)
            t, consumed = b.submit_decode_registered(d, addr[id(m)], len(m))
            assert consumed == len(m)
            return t
        chans.append((s.channel_read, sub, ins))

    # The high-compressor LZ4 channel comes first, and the codec's launches go by (level, compressor) in
    # rising order: the flush's LZ4 list is a real permutation of the submit order.
    lz4(4096, True, msgs(5003, 17, 70001))
    enc(nx.SnappyFrameEncoder, msgs(19, 70001, 0, 17))
    dec(lambda: nx.SnappyFrameDecoder(True), sn_a)
    enc(lambda: nx.FastLzFrameEncoder(1, True), msgs(301, 70001, 1))
    dec(lambda: nx.FastLzFrameDecoder(True), flz_s)
    enc(lambda: nx.LzfEncoder(100), msgs(17, 301, 99, 70001))  # below and above its threshold
    dec(lambda: nx.SnappyFrameDecoder(True), sn_bad)  # passes, fails (CRC), delivers nothing
    lz4(1 << 16, False, msgs(70001, 0, 301))
    enc(nx.SnappyFrameEncoder, [reg_in] + msgs(1, 5003))
    dec(nx.LzfDecoder, lzf_s)
    enc(lambda: nx.FastLzFrameEncoder(2, False), msgs(5003, 19, 0))
    dec(lambda: nx.SnappyFrameDecoder(False), sn_b)
    dec(lambda: nx.Lz4FrameDecoder(True), lz4_bad)  # passes, fails (damaged block), delivers nothing
    enc(lambda: nx.LzfEncoder(16), msgs(19, 5003, 0))
    dec(lambda: nx.FastLzFrameDecoder(False), flz_t)  # the blocks carry checksums; this decoder ignores them
    dec(lambda: nx.SnappyFrameDecoder(True), sn_c, registered=True)
    lz4(4096, True, msgs(301, 19))
    dec(lambda: nx.Lz4FrameDecoder(True), lz4_s)
    dec(nx.LzfDecoder, lzf_t)
    enc(nx.SnappyFrameEncoder, msgs(17, 301, 5003))

    nx.Batcher.register(base, size)
    try:
        tickets = [[] for _ in chans]
        for r in range(max(len(ins) for _, _, ins in chans)):  # round-robin: the channels' jobs interleave
            for c, (_, sub, ins) in enumerate(chans):
                if r < len(ins):
                    tickets[c].append(sub(ins[r]))
        assert b.stats()["flushes"] == 0
        b.flush()
        failed = []
        for c, (sync, _, ins) in enumerate(chans):
            for r, (m, t) in enumerate(zip(ins, tickets[c])):
                want, got = _sync(lambda: sync(m)), _job(nx, b, t)
                assert got == want, (c, r)
                if want[1] != 0:
                    failed.append((c, r))
        assert failed == [(6, 1), (12, 1)]
        assert b.stats()["flushes"] == 1
    finally:
        nx.Batcher.unregister(base)
