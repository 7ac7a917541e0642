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

from bzip2_gpu import decode as _decode, equal_host as _equal_host  # noqa: E402  (after torch is known to be there)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def B():
    from netty_amd import batch
    return batch


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
