"""GPU tests of the bzip2 encoder's split path (nx_bzip2_encode_batch_split: a planner, one workgroup per block,
a bit splice).  The checker is the host encoder: nx_bzip2_encode_host for whole streams, which the split path must
equal byte for byte as nx_bzip2_encode_batch does, and nx_bzip2_encode_segment_host for segments (both held
against libbz2 and against each other by the CPU tests)."""
import bz2

import numpy as np
import pytest

import bzip2_encode_inputs as I
import bzip2_split_inputs as X
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


def _encode(B, dev, datas, caps, level, max_blocks=None, seg=None):
    """One split launch.  Items are packed back to back; item i's slot has caps[i] bytes between guards of GUARD
    bytes of 0xA5 and every slot starts at an odd address.  Returns (out_len, status, outputs, seg after) with
    every byte outside the slots checked."""
    buf, offs = bytearray(), []
    for s in datas:
        offs.append(len(buf))
        buf += s
    buf += b"\x00" * 16
    ooffs, cur = [], 0
    for c in caps:
        cur += GUARD
        cur += 1 - cur % 2
        ooffs.append(cur)
        cur += c
    cur += GUARD
    inp = torch.frombuffer(buf, dtype=torch.uint8).to(dev)
    out = torch.full((cur,), 0xA5, dtype=torch.uint8, device=dev)
    t = lambda v, dt: torch.tensor(v, dtype=dt, device=dev)
    segt = None if seg is None else torch.from_numpy(np.array(seg, dtype=np.uint32).view(np.int32)).to(dev)
    out_len, status = B.bzip2_encode(inp, t(offs, torch.int64), t([len(s) for s in datas], torch.int32), out, t(ooffs, torch.int64),
                                     t(caps, torch.int32), level, split=True, max_blocks=max_blocks, seg=segt)
    torch.cuda.synchronize()
    outa = out.cpu().numpy()
    out_len, status = out_len.cpu().tolist(), status.cpu().tolist()
    res = []
    for i, (o, c, w) in enumerate(zip(ooffs, caps, out_len)):
        assert o % 2 == 1 and 0 <= w <= c, (i, o, w, c)
        res.append(outa[o:o + w].tobytes())
        outa[o:o + c] = 0xA5
    changed = (outa != 0xA5).nonzero()[0]  # every byte outside the slots
    assert changed.size == 0, f"a byte outside the slots changed, first at {int(changed[0])}"
    after = None if segt is None else [tuple(v & 0xFFFFFFFF for v in row) for row in segt.cpu().tolist()]
    return out_len, status, res, after


def _check(items, host, got):
    out_len, status, res, _ = got
    for i, it in enumerate(items):
        st, stream = host[i]
        assert st == I.OK and (status[i], out_len[i]) == (st, len(stream)), (it.name, status[i], out_len[i], len(stream))
        assert res[i] == stream, it.name


def test_split_equals_host(B, dev, oracle):
    items, host = I.items(oracle), I.host_streams(B, oracle)
    for level in sorted({it.level for it in items}):
        idx = [i for i, it in enumerate(items) if it.level == level]
        datas = [items[i].data for i in idx]
        caps = [B.bzip2_max_compressed_length(len(d), level) for d in datas]
        _check([items[i] for i in idx], [host[i] for i in idx], _encode(B, dev, datas, caps, level))


def test_split_phases(B, dev):
    """Second blocks that land at every bit phase of a byte (test_bzip2_segment_host.test_phase_coverage)."""
    items = X.phase_items()
    caps = [B.bzip2_max_compressed_length(len(it.data), 1) for it in items]
    _check(items, X.phase_streams(B), _encode(B, dev, [it.data for it in items], caps, 1))


def test_split_full_block(B, dev, oracle):
    it = I.full_block(oracle)
    host = B.bzip2_encode_host(it.data, it.level)
    got = _encode(B, dev, [it.data], [B.bzip2_max_compressed_length(len(it.data), it.level)], it.level)
    _check([it], [host], got)
    assert bz2.decompress(got[2][0]) == it.data


def test_rounds(B, dev):
    """More jobs than slots: the workspace is capped at two units, so a stream's blocks straddle rounds."""
    B.workspaces_trim()
    B.bzip2_encoder_reserve(2, 1)
    try:
        five, three = X.five_blocks(), X.three_blocks()
        assert len(I.block_slices(five.data, 1)) == 5
        datas = [three.data[:5000], five.data, b"", five.data[:70000], three.data[1000:31000]]
        caps = [B.bzip2_max_compressed_length(len(d), 1) for d in datas]
        got = _encode(B, dev, datas, caps, 1)
        assert B.workspace_info(B.WS_BZIP2_ENC)[0] == 2 * B.bzip2_encoder_slot_bytes(1)
        for i, d in enumerate(datas):
            assert (got[1][i], got[2][i]) == B.bzip2_encode_host(d, 1), i
    finally:
        B.workspaces_trim()
    assert B.workspace_info(B.WS_BZIP2_ENC)[0] == 0


def test_statuses_in_one_launch(B, dev, oracle):
    text = oracle.textgen_chunk(7, 3000)
    st, stream = B.bzip2_encode_host(text, 1)
    assert st == I.OK
    out_len, status, res, _ = _encode(B, dev, [text, text, b"", text], [len(stream), len(stream) - 1, 14, len(stream) + 5], 1)
    assert status == [I.OK, I.ENCODE_FULL, I.OK, I.OK]  # _encode has checked the short slot's neighbours
    assert res[0] == stream and out_len[1] == 0 and res[2] == bz2.compress(b"", 1) and res[3] == stream
    # max_blocks below the true count of 4 blocks: the late items fail, an empty item has no block to list
    two = X.phase_items()[0]
    st2, stream2 = X.phase_streams(B)[0]
    datas = [text, two.data, b"", text]
    caps = [B.bzip2_max_compressed_length(len(d), 1) for d in datas]
    out_len, status, res, _ = _encode(B, dev, datas, caps, 1, max_blocks=2)
    assert status == [I.OK, X.BLOCKS, I.OK, X.BLOCKS] and out_len[1] == out_len[3] == 0
    assert res[0] == stream and res[2] == bz2.compress(b"", 1)
    out_len, status, res, _ = _encode(B, dev, datas, caps, 1, max_blocks=4)
    assert status == [I.OK] * 4 and res[1] == stream2 and res[3] == stream


def test_empty_batch_and_levels(B, dev):
    L = __import__("netty_amd._lib", fromlist=["load"]).load()
    assert L.nx_bzip2_encode_batch_split(None, None, None, None, None, None, None, None, 0, 1, 0, None, None) == I.OK
    assert L.nx_bzip2_encode_batch_split(None, None, None, None, None, None, None, None, 0, 0, 0, None, None) == I.LEVEL
    for level in (0, 10):
        with pytest.raises(RuntimeError, match=str(I.LEVEL)):
            _encode(B, dev, [b"abc"], [64], level, max_blocks=1)


def test_segments_behind_every_carry(B, dev, oracle):
    """The CPU test's carry sweep as 32 items of one launch, against nx_bzip2_encode_segment_host; then a
    stream in three segments with the carry and the CRC threaded through."""
    it = X.small_stream_item(oracle)
    segs = [(X.SEG_LAST, X.CARRY_PATTERN & ((1 << c) - 1), c, 0x1234ABCD) for c in range(32)]
    want = [B.bzip2_encode_segment_host(it.data, 1, s) for s in segs]
    cap = B.bzip2_max_compressed_length(len(it.data), 1) + 8
    out_len, status, res, after = _encode(B, dev, [it.data] * 32, [cap] * 32, 1, seg=segs)
    for c in range(32):
        assert (status[c], res[c]) == want[c][:2] and after[c] == want[c][2], c
    three, (st, stream) = X.three_blocks(), X.three_blocks_stream(B)
    cuts = X.cuts_of(three.data, 1)
    seg, out = (X.SEG_FIRST, 0, 0, 0), b""
    for k, (a, b) in enumerate(zip([0, cuts[0]], [cuts[0], len(three.data)])):  # one block, then two with the footer
        seg = ((X.SEG_FIRST, X.SEG_LAST)[k],) + tuple(seg[1:])
        want = B.bzip2_encode_segment_host(three.data[a:b], 1, seg)
        out_len, status, res, after = _encode(B, dev, [three.data[a:b]], [len(three.data)], 1, seg=[seg])
        assert (status[0], res[0], after[0]) == want, k
        assert k == 1 or (len(res[0]) % 4 == 0 and after[0][2] < 32)
        seg, out = after[0], out + res[0]
    assert st == I.OK and out == stream
