"""GPU tests of the split bzip2 decode (nx_bzip2_scan_batch, nx_bzip2_decode_batch_split): item for item it
must equal the serial call nx_bzip2_decode_batch in status, out_len, consumed and out[:out_len], on valid,
mutated, fuzzed and hand-built streams and on streams with decoy magics, and equal nx_bzip2_decode_split_host."""
import bz2

import pytest

import bzip2_decoys as D
import bzip2_handbuilt as H
import bzip2_model as M
import bzip2_streams as S

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import bzip2_gpu as G  # noqa: E402  (after torch is known to be there)

DECODE_BLOCKS = -128  # NX_ERR_BZIP2_DECODE_BLOCKS
SLOT = 6 * 900000 + 256


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def B():
    from netty_amd import batch
    return batch


class _Split:
    """netty_amd.batch with bzip2_decode taking the split path, for bzip2_gpu.decode's one launch over guarded
    slots; keeps the chain lengths of the last call."""

    def __init__(self, B, max_blocks=None):
        self.B, self.max_blocks, self.blocks = B, max_blocks, None

    def bzip2_decode(self, *a):
        out_len, consumed, status, blocks = self.B.bzip2_decode(*a, split=True, max_blocks=self.max_blocks)
        self.blocks = blocks
        return out_len, consumed, status


def _both(B, dev, streams, caps, max_blocks=None, host=True):
    """The serial and the split call on the same batch: equal in status, out_len, consumed and bytes.  Returns
    the split call's results and chain lengths."""
    want = G.decode(B, dev, streams, caps)
    sp = _Split(B, max_blocks)
    got = G.decode(sp, dev, streams, caps)
    blocks = sp.blocks.cpu().tolist()
    for i in range(len(streams)):
        assert (got[2][i], got[0][i], got[1][i]) == (want[2][i], want[0][i], want[1][i]), i
        assert got[3][i] == want[3][i], i
    if host:
        for i, (s, c) in enumerate(zip(streams, caps)):
            st, out, used, nb = B.bzip2_decode_split_host(s, c)
            assert (got[2][i], got[3][i], got[1][i], blocks[i]) == (st, out, used, nb), i
    return got, blocks


def test_scan(B, dev):
    texts, specs, stream, positions = H.multi_block()
    items = [stream, b"", stream[:9], D.streams()[2][1], b"\x00" * 700 + stream, stream[:10]]
    buf, offs = bytearray(), []
    for s in items:
        offs.append(len(buf))
        buf += s + b"\x31\x41\x59"  # bytes between the items belong to none
    t = lambda v, dt: torch.tensor(v, dtype=dt, device=dev)
    inp = torch.frombuffer(buf, dtype=torch.uint8).to(dev)
    pos, first, count, status = B.bzip2_scan(inp, t(offs, torch.int64), t([len(s) for s in items], torch.int32), max_blocks=200)
    pos, first, count, status = pos.cpu().tolist(), first.cpu().tolist(), count.cpu().tolist(), status.cpu().tolist()
    at = 0
    for i, s in enumerate(items):
        want = [p | (B.BZIP2_CAND_END if e else 0) for p, e in B.bzip2_scan_host(s)]
        assert (status[i], first[i], count[i]) == (0, at, len(want)), i
        assert pos[at:at + len(want)] == want, i
        at += len(want)
    assert count[0] == 41 and count[4] == 41 and count[5] == 1


@pytest.mark.parametrize("which", ["valid", "mutants", "fuzz", "decoys"])
def test_equals_serial(B, dev, oracle, which):
    if which == "valid":
        vs = S.valid_streams(oracle)
        streams, caps = [v.stream for v in vs], [len(v.data) for v in vs]
    elif which == "mutants":
        ms = S.mutants(oracle)
        streams, caps = [m.stream for m in ms], [m.cap for m in ms]
    elif which == "fuzz":
        streams, caps = [s for s, c in S.fuzz_set()], [c for s, c in S.fuzz_set()]
    else:
        streams, caps = [d[1] for d in D.streams()], [len(d[5]) for d in D.streams()]
    got, blocks = _both(B, dev, streams, caps)
    if which == "valid":
        for i, v in enumerate(S.valid_streams(oracle)):
            assert (got[2][i], got[3][i], got[1][i]) == (S.OK, v.data, v.consumed), v.name
    if which == "decoys":
        for i, d in enumerate(D.streams()):
            assert (got[2][i], got[3][i], blocks[i]) == (S.OK, d[5], len(d[2])), d[0]
            assert bz2.BZ2Decompressor().decompress(d[1]) == d[5]


@pytest.mark.parametrize("group", H.GROUPS)
def test_handbuilt_group(B, dev, group):
    cases = H.group(B.bzip2_decode_chains(), group)
    got, blocks = _both(B, dev, [c.stream for c in cases], [c.cap for c in cases])
    for i, c in enumerate(cases):
        assert (got[2][i], got[0][i], got[1][i]) == (c.status, len(c.data), c.consumed), c.name
        assert got[3][i] == c.data, c.name
    if group == "streams":
        by = {c.name: blocks[i] for i, c in enumerate(cases)}
        want = {"blocks40": 40, "blocks40_tail": 40, "blocks40_cut_in_block33": 33, "blocks40_block35_wrong_crc": 35,
                "blocks40_wrong_stream_crc": 40, "blocks40_cap_block_edge": 2, "blocks40_cap_inside_block1": 1, "blocks40_cap_inside_block2": 2,
                "blocks40_cap_total_minus_1": 39, "blocks40_cap_zero": 0, "no_blocks": 0}
        assert {k: by[k] for k in want} == want


def test_rounds_on_two_slots(B, dev):
    """Three copies of the 40-block stream, 123 candidates, on two slots: 62 rounds, twice in a row."""
    texts, specs, stream, positions = H.multi_block()
    cap = sum(len(t) for t in texts)
    B.workspaces_trim()
    B.bzip2_decoder_reserve(2)
    try:
        assert B.workspace_info(B.WS_BZIP2_DEC)[0] == 2 * SLOT
        for _ in range(2):
            got, blocks = _both(B, dev, [stream] * 3, [cap] * 3, max_blocks=123, host=False)
            assert got[2] == [S.OK] * 3 and blocks == [40] * 3 and got[3] == [b"".join(texts)] * 3
        assert B.workspace_info(B.WS_BZIP2_DEC)[0] == 2 * SLOT
    finally:
        B.workspaces_trim()


def test_max_blocks(B, dev):
    """max_blocks below an item's candidate count: the new status for that item, its neighbours decode."""
    texts, specs, stream, positions = H.multi_block()
    cap = sum(len(t) for t in texts)
    small = bz2.compress(b"a small neighbour", 1)
    sp = _Split(B, max_blocks=40)
    got = G.decode(sp, dev, [small, stream, small], [32, cap, 32])
    assert got[2] == [S.OK, DECODE_BLOCKS, S.OK] and got[0] == [17, 0, 17] and got[1] == [len(small), 0, len(small)]
    assert got[3][0] == b"a small neighbour" == got[3][2]
    sp = _Split(B, max_blocks=45)
    got = G.decode(sp, dev, [small, stream, small], [32, cap, 32])
    assert got[2] == [S.OK] * 3 and got[3][1] == b"".join(texts) and sp.blocks.cpu().tolist() == [1, 40, 1]


def test_full_size_slots(B, dev, oracle):
    """2.0 MB of text at level 9: three blocks, slots filled to the last byte.  That stream is 392 KB, so its bit
    positions stay below 2^23; a second item, half of it random bytes, is 1.4 MB and carries them past it."""
    import random
    text = oracle.textgen_chunk(11, 2000000)
    mixed = text[:1000000] + random.Random(9).randbytes(1000000)
    datas = [text, mixed]
    streams = [bz2.compress(d, 9) for d in datas]
    got, nb = _both(B, dev, streams, [len(d) for d in datas], host=False)
    assert nb == [3, 3] and got[2] == [S.OK] * 2
    for i in range(2):
        assert got[3][i] == datas[i] == bz2.decompress(streams[i]), i
    t = lambda v, dt: torch.tensor(v, dtype=dt, device=dev)
    inp = torch.frombuffer(bytearray(streams[1]), dtype=torch.uint8).to(dev)
    pos, first, count, status = B.bzip2_scan(inp, t([0], torch.int64), t([len(streams[1])], torch.int32), max_blocks=64)
    pos = pos.cpu().tolist()[:int(count[0])]
    assert int(status[0]) == 0 and int(count[0]) >= 4
    assert max(p & ~B.BZIP2_CAND_END for p in pos) > 1 << 23


def test_chain_edge_sizes(B, dev):
    """Blocks of 1, 2, 63, 64, 65, kc - 1, kc, kc + 1 pre-RLE bytes and periodic texts, one block each, in one stream."""
    kc = B.bzip2_decode_chains()
    pres = [bytes((7 * i + k) % 251 for i in range(n)) for k, n in enumerate((1, 2, 63, 64, 65, kc - 1, kc, kc + 1))]
    pres += [b"hello world" * 10, b"ab" * 300, b"xyz" * (kc // 3 + 5)]
    blocks = [M.text_block(p) for p in pres]
    stream = M.seal(1, blocks)
    st, data, used = M.decode(stream, 1 << 20)
    assert st == M.OK and used == len(stream)
    cut = stream[:-11]  # the end marker and a byte of the last block are missing
    got, nb = _both(B, dev, [stream, cut], [len(data), len(data)])
    assert (got[2][0], got[3][0], nb[0]) == (S.OK, data, len(pres))
    assert (got[2][1], got[3][1], nb[1]) == (S.TRUNCATED, data[:len(data) - len(pres[-1])], len(pres) - 1)
