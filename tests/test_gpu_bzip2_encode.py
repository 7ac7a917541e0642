"""GPU tests of the bzip2 encoder (nx_bzip2_encode_batch).  The checker is nx_bzip2_encode_host, which the CPU
tests (tests/test_bzip2_encode_host.py) hold against libbz2: the kernel and the host encoder run the same format
functions and the same rotation order, so status, out_len and the bytes must agree item for item."""
import bz2
import random

import pytest

import bzip2_encode_inputs as I
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


def _encode(B, dev, datas, caps, level):
    """One launch.  Items are packed back to back; item i's slot has caps[i] bytes between guards of GUARD bytes
    of 0xA5 and a third of the slots start at odd addresses (the scheme of test_gpu_bzip2_decode._decode).
    Returns (out_len, status, outputs) with every byte outside the slots checked."""
    buf, offs = bytearray(), []
    for s in datas:
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
    out_len, status = B.bzip2_encode(inp, t(offs, torch.int64), t([len(s) for s in datas], torch.int32), out, t(ooffs, torch.int64),
                                     t(caps, torch.int32), level)
    torch.cuda.synchronize()
    outa = out.cpu().numpy()
    out_len, status = out_len.cpu().tolist(), status.cpu().tolist()
    res = []
    for i, (o, c, w) in enumerate(zip(ooffs, caps, out_len)):
        assert 0 <= w <= c, (i, w, c)
        res.append(outa[o:o + w].tobytes())
        outa[o:o + c] = 0xA5
    changed = (outa != 0xA5).nonzero()[0]  # every byte outside the slots
    assert changed.size == 0, f"a byte outside the slots changed, first at {int(changed[0])}"
    return out_len, status, res


@pytest.fixture(scope="module")
def launches(B, dev, oracle):
    """All inputs but the full-size block, one launch per level used: {level: (items, host results, gpu results)}."""
    items, host = I.items(oracle), I.host_streams(B, oracle)
    out = {}
    for level in sorted({it.level for it in items}):
        idx = [i for i, it in enumerate(items) if it.level == level]
        datas = [items[i].data for i in idx]
        caps = [B.bzip2_max_compressed_length(len(d), level) for d in datas]
        out[level] = ([items[i] for i in idx], [host[i] for i in idx], _encode(B, dev, datas, caps, level), caps)
    return out


def test_gpu_equals_host(B, dev, launches):
    for level, (items, host, (out_len, status, res), caps) in launches.items():
        for i, it in enumerate(items):
            st, stream = host[i]
            assert (status[i], out_len[i]) == (st, len(stream)) and st == I.OK, (it.name, status[i], out_len[i], st, len(stream))
            assert res[i] == stream, it.name
    # determinism: a second launch of one level gives identical bytes
    items, _, first, caps = launches[1]
    again = _encode(B, dev, [it.data for it in items], caps, 1)
    assert again == first


def test_round_trip_on_the_gpu(B, dev, launches):
    for level, (items, _, (out_len, status, res), _) in launches.items():
        buf, offs = bytearray(), []
        for s in res:
            offs.append(len(buf))
            buf += s
        buf += b"\x00" * 16
        caps = [max(len(it.data), 1) for it in items]
        ooffs = [sum(caps[:i]) for i in range(len(caps))]
        inp = torch.frombuffer(buf, dtype=torch.uint8).to(dev)
        out = torch.zeros(sum(caps) + 1, dtype=torch.uint8, device=dev)
        t = lambda v, dt: torch.tensor(v, dtype=dt, device=dev)
        dl, consumed, dst = B.bzip2_decode(inp, t(offs, torch.int64), t([len(s) for s in res], torch.int32), out, t(ooffs, torch.int64),
                                           t(caps, torch.int32))
        torch.cuda.synchronize()
        outa = out.cpu().numpy()
        assert dst.cpu().tolist() == [S.OK] * len(items)
        assert consumed.cpu().tolist() == [len(s) for s in res]
        for i, (it, w) in enumerate(zip(items, dl.cpu().tolist())):
            assert outa[ooffs[i]:ooffs[i] + w].tobytes() == it.data, it.name


def test_slots_in_turn(B, dev):
    B.workspaces_trim()
    B.bzip2_encoder_reserve(4, 1)
    r = random.Random(5)
    datas = [bytes(r.getrandbits(8) for _ in range(r.randrange(0, 3001))) for _ in range(20)]
    datas[3] = b""
    caps = [B.bzip2_max_compressed_length(len(d), 1) for d in datas]
    out_len, status, res = _encode(B, dev, datas, caps, 1)
    for i, d in enumerate(datas):
        assert (status[i], res[i]) == B.bzip2_encode_host(d, 1), i
    assert B.workspace_info(B.WS_BZIP2_ENC)[0] == 4 * B.bzip2_encoder_slot_bytes(1)
    B.workspaces_trim()
    assert B.workspace_info(B.WS_BZIP2_ENC)[0] == 0


def test_mixed_statuses_in_one_launch(B, dev, oracle):
    text = oracle.textgen_chunk(7, 3000)
    st, stream = B.bzip2_encode_host(text, 9)
    assert st == I.OK
    out_len, status, res = _encode(B, dev, [text, text, b""], [len(stream), len(stream) - 1, 14], 9)
    assert status == [I.OK, I.ENCODE_FULL, I.OK]  # _encode has checked the short slot's neighbours
    assert res[0] == stream and out_len[1] == 0 and res[2] == bz2.compress(b"")


def test_full_block(B, dev, oracle):
    it = I.full_block(oracle)
    st, stream = B.bzip2_encode_host(it.data, it.level)
    assert st == I.OK
    out_len, status, res = _encode(B, dev, [it.data], [B.bzip2_max_compressed_length(len(it.data), it.level)], it.level)
    assert status == [I.OK] and res[0] == stream
    assert bz2.decompress(res[0]) == it.data
