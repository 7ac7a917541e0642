"""GPU tests of the bzip2 decoder (nx_bzip2_decode_batch).  The checker is libbz2 through Python's bz2: valid
streams must decode to libbz2's bytes.  nx_bzip2_decode_host is the second opinion on malformed input: the
kernel and the host decoder run the same format functions, so status, out_len and consumed must agree item
for item.  Every mutated input here is one the host decoder answers with a status
(tests/test_bzip2_decode_host.py); the GPU run checks equality."""
import bz2
import random

import pytest

import bzip2_streams as S

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GUARD = S.GUARD


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def B():
    from netty_amd import batch
    return batch


def _decode(B, dev, streams, caps):
    """One launch.  Streams are packed back to back; item i's slot has caps[i] bytes between guards of GUARD
    bytes of 0xA5 and a third of the slots start at odd addresses.  Returns (out_len, consumed, status,
    outputs) with the guards checked: on an error the slot beyond out_len may have been written, the guards not."""
    buf, offs = bytearray(), []
    for s in streams:
        offs.append(len(buf))
        buf += s
    buf += b"\x00" * 16
    ooffs, cur = [], 0
    for i, c in enumerate(caps):
        cur += GUARD + (1 if i % 3 == 1 else 0)
        ooffs.append(cur)
        cur += c
    cur += GUARD
    inp = torch.frombuffer(buf, dtype=torch.uint8).to(dev)
    out = torch.full((cur,), 0xA5, dtype=torch.uint8, device=dev)
    t = lambda v, dt: torch.tensor(v, dtype=dt, device=dev)
    out_len, consumed, status = B.bzip2_decode(inp, t(offs, torch.int64), t([len(s) for s in streams], torch.int32), out,
                                               t(ooffs, torch.int64), t(caps, torch.int32))
    torch.cuda.synchronize()
    outa = out.cpu().numpy()
    out_len, consumed, status = out_len.cpu().tolist(), consumed.cpu().tolist(), status.cpu().tolist()
    res = []
    for i, (o, c, w) in enumerate(zip(ooffs, caps, out_len)):
        assert 0 <= w <= c, (i, w, c)
        res.append(outa[o:o + w].tobytes())
        outa[o:o + c] = 0xA5
    changed = (outa != 0xA5).nonzero()[0]  # every byte outside the slots
    assert changed.size == 0, f"a guard byte changed, first at {int(changed[0])}"
    return out_len, consumed, status, res


def _equal_host(B, streams, caps, got):
    out_len, consumed, status, res = got
    for i, (s, c) in enumerate(zip(streams, caps)):
        st, out, used = B.bzip2_decode_host(s, c)
        assert (status[i], out_len[i], consumed[i]) == (st, len(out), used), i
        if st == S.OK:
            assert res[i] == out, i


def test_batch_call_exists(B):
    assert callable(B.bzip2_decode) and B.bzip2_decode_chains() >= 1


def test_valid_and_mutated_streams(B, dev, oracle):
    valid, bad = S.valid_streams(oracle), S.mutants(oracle)
    streams = [v.stream for v in valid] + [m.stream for m in bad]
    caps = [len(v.data) for v in valid] + [m.cap for m in bad]
    got = _decode(B, dev, streams, caps)
    out_len, consumed, status, res = got
    for i, v in enumerate(valid):
        assert status[i] == S.OK, (v.name, status[i])
        assert res[i] == v.data, v.name  # libbz2's bytes (tests/test_bzip2_decode_host.py holds v.data against it)
        assert consumed[i] == v.consumed, v.name
    for k, m in enumerate(bad):
        assert status[len(valid) + k] == m.status, (m.name, status[len(valid) + k])
    _equal_host(B, streams, caps, got)


def test_chain_edges(B, dev):
    """Blocks of n pre-RLE bytes around the lane count and the chain count, and periodic ones (several cycles)."""
    kc = B.bzip2_decode_chains()
    rng = random.Random(5)
    datas = []
    for n in sorted({1, 2, 63, 64, 65, kc - 1, kc, kc + 1} - {0}):
        d = bytes(rng.randrange(256) for _ in range(n))
        while S._rle1_length(d) != n:  # no run of four: the block has n bytes
            d = bytes(rng.randrange(256) for _ in range(n))
        datas.append(d)
    datas += [b"ab" * (kc + 3), b"x" * 518, b"hello world" * 100]
    streams = [bz2.compress(d) for d in datas]
    out_len, consumed, status, res = _decode(B, dev, streams, [len(d) for d in datas])
    for i, d in enumerate(datas):
        assert (status[i], res[i], consumed[i]) == (S.OK, d, len(streams[i])), (i, len(d))


def test_start_pointer_moved(B, dev, oracle):
    moved = S.start_moved(oracle)
    streams, caps = [s for s, _ in moved], [c for _, c in moved]
    got = _decode(B, dev, streams, caps)
    assert all(st in (S.OK, S.BLOCK_CRC) for st in got[2])
    _equal_host(B, streams, caps, got)


def test_slot_reuse(B, dev, oracle):
    """Nine streams of different sizes on two slots: the ring of slots and a wave's loop over several streams."""
    B.workspaces_trim()
    B.bzip2_decoder_reserve(2)
    try:
        assert B.workspace_info(B.WS_BZIP2_DEC)[0] == 2 * (6 * 900000 + 256)
        text = oracle.textgen_chunk(3, 120000)
        datas = [text[:n] for n in (120000, 1, 70000, 333, 5000, 64, 99999, 2, 40000)]
        streams = [bz2.compress(d, 1 + i) for i, d in enumerate(datas)]
        for _ in range(2):
            out_len, consumed, status, res = _decode(B, dev, streams, [len(d) for d in datas])
            assert status == [S.OK] * 9 and res == datas
    finally:
        B.workspaces_trim()


def test_mutation_fuzz(B, dev):
    fz = S.fuzz_set()
    streams, caps = [s for s, _ in fz], [c for _, c in fz]
    _equal_host(B, streams, caps, _decode(B, dev, streams, caps))
