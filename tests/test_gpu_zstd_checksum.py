"""GPU tests of content-checksum verification in k_zstd_decode (batch.zstd_decode(verify_checksum=True),
nx_zstd_decode_batch_ex).  The frames and their checksums are those tests/test_zstd_checksum_host.py pins on
libzstd; nx_zstd_decode_host_ex, which that file checks, is the item-by-item second opinion here."""
import pytest

import zstd_checksum_inputs as K
import zstd_decode_inputs as I

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
pa = pytest.importorskip("pyarrow")
pytest.importorskip("xxhash")

GUARD = I.GUARD


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def B():
    from netty_amd import batch
    return batch


@pytest.fixture(scope="module")
def L():
    from netty_amd import _lib
    return _lib.load()


def _launch(B, dev, frames, caps, verify, in_res=None, out_res=None):
    """One launch.  Frame i starts at an input offset that is in_res[i] mod 8 and its slot of caps[i] bytes at
    an output offset that is out_res[i] mod 8 (default: i mod 8 and 3 i mod 8), slots GUARD bytes or more
    apart, everything pre-filled with 0xA5.  Returns per item (status, output, consumed); no byte outside
    the reported outputs may have changed."""
    n = len(frames)
    in_res = in_res or [i % 8 for i in range(n)]
    out_res = out_res or [3 * i % 8 for i in range(n)]
    buf, offs = bytearray(), []
    for f, r in zip(frames, in_res):
        buf += b"\x00" * ((r - len(buf)) % 8)
        offs.append(len(buf))
        buf += f
    buf += b"\x00" * 16
    ooffs, cur = [], 0
    for c, r in zip(caps, out_res):
        cur += GUARD
        cur += (r - cur) % 8
        ooffs.append(cur)
        cur += c
    cur += GUARD
    assert [o % 8 for o in offs] == list(in_res) and [o % 8 for o in ooffs] == list(out_res)
    inp = torch.frombuffer(buf, dtype=torch.uint8).to(dev)
    out = torch.full((cur,), 0xA5, dtype=torch.uint8, device=dev)
    t = lambda v, dt: torch.tensor(v, dtype=dt, device=dev)
    consumed, out_len, status = B.zstd_decode(inp, t(offs, torch.int64), t([len(f) for f in frames], torch.int32), out,
                                              t(ooffs, torch.int64), t(caps, torch.int32), verify_checksum=verify)
    torch.cuda.synchronize()
    outa = out.cpu().numpy()
    res = []
    for o, c, w, st, co in zip(ooffs, caps, out_len.cpu().tolist(), status.cpu().tolist(), consumed.cpu().tolist()):
        assert 0 <= w <= c, (w, c)
        res.append((st, outa[o:o + w].tobytes(), co))
        outa[o:o + w] = 0xA5
    changed = (outa != 0xA5).nonzero()[0]
    assert changed.size == 0, f"bytes outside the reported output changed, first at {int(changed[0])}"
    return res


def test_every_case_agrees_with_the_host_decoder(B, dev, L, oracle):
    """the valid frames, each with every checksum byte flipped and with its checksum cut short, in one batch"""
    frames, caps, want = [], [], []
    for name, f, data in K.cases(oracle):
        variants = [f] + [K.wrong_checksum(f, b, bit=(b * 3 + len(data)) % 8) for b in range(4)] + [f[:-c] for c in range(1, 5)]
        for v, st in zip(variants, [K.OK] + [K.CHECKSUM] * 4 + [K.TRUNCATED] * 4):
            frames.append(v)
            caps.append(len(data))
            want.append((st, data, len(f) if st == K.OK else 0))
    got = _launch(B, dev, frames, caps, True)
    for i, (f, c) in enumerate(zip(frames, caps)):
        assert got[i] == want[i], (i, got[i][0], want[i][0])
        if i % 9 < 2 or i % 9 == 5:  # the second opinion on one variant of each kind
            assert got[i] == K.host_decode(L, f, c, K.VERIFY), i


def test_every_alignment_of_input_and_output(B, dev, oracle):
    by = {name: (f, data) for name, f, data in K.cases(oracle)}
    for name in ("raw_127", "libzstd_text_5000"):
        f, data = by[name]
        res = [(i, o) for i in range(8) for o in range(8)]
        got = _launch(B, dev, [f] * 64, [len(data)] * 64, True, [i for i, _ in res], [o for _, o in res])
        assert got == [(K.OK, data, len(f))] * 64, name
        bad = K.wrong_checksum(f, 2, 5)
        got = _launch(B, dev, [bad] * 64, [len(data)] * 64, True, [i for i, _ in res], [o for _, o in res])
        assert got == [(K.CHECKSUM, data, 0)] * 64, name


def test_mixed_batch(B, dev, oracle):
    """checksummed, plain and wrong-checksum frames side by side: statuses are per item, neighbours intact"""
    plain = [(c.frame, c.data) for c in I.libzstd_frames(oracle) if c.level == 3 and c.n in (300, 5000, 65536)]
    frames, caps, want = [], [], []
    for k, (name, f, data) in enumerate(K.cases(oracle)):
        pf, pd = plain[k % len(plain)]
        for v, d, st, used in ((f, data, K.OK, len(f)), (pf, pd, K.OK, len(pf)), (K.wrong_checksum(f, k % 4, k % 8), data, K.CHECKSUM, 0)):
            frames.append(v)
            caps.append(len(d) + k % 5)
            want.append((st, d, used))
    assert _launch(B, dev, frames, caps, True) == want


def test_without_verify_checksum_the_frame_is_refused(B, dev, oracle):
    cs = K.cases(oracle)
    got = _launch(B, dev, [f for _, f, _ in cs], [len(d) for _, _, d in cs], False)
    assert got == [(K.UNSUPPORTED, b"", 0)] * len(cs)
