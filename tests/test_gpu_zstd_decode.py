"""GPU tests of the Zstandard frame decoder (nx_zstd_decode_batch).  The checker is libzstd through pyarrow:
the corpus frames are libzstd's own and must regenerate their sources; the hand-built frames are judged by
a Python model that tests/test_zstd_decode_host.py pins against libzstd.  nx_zstd_decode_host is the second
opinion on malformed input: the kernel and the host decoder run the same format functions, so their
statuses must agree byte for byte of input."""
import ctypes as C
import random

import pytest

import zstd_decode_inputs as I
import zstd_handbuilt as HB

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
pa = pytest.importorskip("pyarrow")

OK, TRUNCATED, CORRUPT, OUTPUT_FULL = 0, -85, -86, -87
GUARD = I.GUARD


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def B():
    from netty_amd import batch
    return batch


def _decode(B, dev, frames, caps, in_lens=None, odd=True, pad_between=0):
    """One launch.  Frames are packed back to back (pad_between bytes apart); item i's slot has caps[i] bytes
    between guards of GUARD bytes, everything pre-filled with 0xA5, and a third of the slots start at odd
    addresses.  Returns (consumed, out_len, status, outputs) with the guards checked."""
    buf, offs = bytearray(), []
    for f in frames:
        offs.append(len(buf))
        buf += f + b"\x00" * pad_between
    total = len(buf)
    buf += b"\x00" * 16
    in_lens = in_lens or [len(f) for f in frames]
    assert all(o + l <= total for o, l in zip(offs, in_lens))
    ooffs, cur = [], 0
    for i, c in enumerate(caps):
        cur += GUARD + (1 if odd and i % 3 == 1 else 0)
        ooffs.append(cur)
        cur += c
    cur += GUARD
    inp = torch.frombuffer(buf, dtype=torch.uint8).to(dev)
    out = torch.full((cur,), 0xA5, dtype=torch.uint8, device=dev)
    t = lambda v, dt: torch.tensor(v, dtype=dt, device=dev)
    consumed, out_len, status = B.zstd_decode(inp, t(offs, torch.int64), t(in_lens, torch.int32), out, t(ooffs, torch.int64),
                                              t(caps, torch.int32))
    torch.cuda.synchronize()
    outa = out.cpu().numpy()
    consumed, out_len, status = consumed.cpu().tolist(), out_len.cpu().tolist(), status.cpu().tolist()
    res = []
    for i, (o, c, w) in enumerate(zip(ooffs, caps, out_len)):
        assert 0 <= w <= c, (i, w, c)
        res.append(outa[o:o + w].tobytes())
        outa[o:o + w] = 0xA5
    changed = (outa != 0xA5).nonzero()[0]  # every byte outside [out_off, out_off + out_len) of some item
    assert changed.size == 0, f"bytes outside the reported output changed, first at {int(changed[0])}"
    return consumed, out_len, status, res


def _host(frame, cap):
    from netty_amd import _lib
    L = _lib.load()
    out = (C.c_uint8 * (cap + 1))()
    ol, co = C.c_size_t(0), C.c_size_t(0)
    st = L.nx_zstd_decode_host(frame, len(frame), out, cap, C.byref(ol), C.byref(co))
    return st, bytes(out[:ol.value])


def test_libzstd_corpus(B, dev, oracle):
    cases = I.libzstd_frames(oracle)
    consumed, out_len, status, outs = _decode(B, dev, [c.frame for c in cases], [c.n for c in cases])
    for c, co, ol, st, o in zip(cases, consumed, out_len, status, outs):
        what = (c.kind, c.n, c.level)
        assert st == OK and co == len(c.frame) and ol == c.n, (what, st, co, ol)
        assert o == c.data, what


def test_handbuilt_frames(B, dev):
    hb = HB.cases()
    frames = [f for f, _ in hb.values()]
    consumed, out_len, status, outs = _decode(B, dev, frames, [len(w) + 3 for _, w in hb.values()])
    for (name, (f, want)), co, st, o in zip(hb.items(), consumed, status, outs):
        assert st == OK and co == len(f), (name, st, co)
        assert o == want, name


def test_round_trip_with_the_encoder(B, dev, oracle):
    import test_gpu_zstd as E
    chunks = [c for _, _, c in E._contents(oracle)]
    frames, st = E._encode(B, dev, chunks)
    assert st == [0] * len(chunks)
    consumed, out_len, status, outs = _decode(B, dev, frames, [len(c) for c in chunks])
    assert status == [OK] * len(chunks)
    assert consumed == [len(f) for f in frames]
    assert outs == chunks


@pytest.mark.parametrize("n", [1, 65])
def test_batch_shapes(B, dev, oracle, n):
    cases = [c for c in I.libzstd_frames(oracle) if c.n <= 5000][:65]
    cases = [cases[k % len(cases)] for k in range(n)]
    consumed, out_len, status, outs = _decode(B, dev, [c.frame for c in cases], [c.n for c in cases])
    assert status == [OK] * n and outs == [c.data for c in cases]


def test_batch_larger_than_the_workspace(B, dev, oracle):
    """three slots of literals for 65 frames: a wave decodes its frames in turn through one slot"""
    cases = [c for c in I.libzstd_frames(oracle) if c.n <= 5000][:65]
    torch.cuda.synchronize()
    B.workspaces_trim()
    try:
        B.zstd_decoder_reserve(3)
        assert B.workspace_info(B.WS_ZSTD_DEC)[0] == 3 * 131072
        consumed, out_len, status, outs = _decode(B, dev, [c.frame for c in cases], [c.n for c in cases])
        assert B.workspace_info(B.WS_ZSTD_DEC)[0] == 3 * 131072
    finally:
        torch.cuda.synchronize()
        B.workspaces_trim()
    assert status == [OK] * len(cases) and outs == [c.data for c in cases]
    assert consumed == [len(c.frame) for c in cases]


def test_input_placement(B, dev, oracle):
    """frames back to back, each item's in_len reaching over the next frame: consumed is the first frame only"""
    cases = [c for c in I.libzstd_frames(oracle) if c.n in (300, 1024, 5000)][:24]
    frames = [c.frame for c in cases]
    lens = [len(f) + (len(frames[i + 1]) if i + 1 < len(frames) else 0) for i, f in enumerate(frames)]
    consumed, out_len, status, outs = _decode(B, dev, frames, [c.n for c in cases], in_lens=lens)
    assert status == [OK] * len(cases)
    assert consumed == [len(f) for f in frames]
    assert outs == [c.data for c in cases]


def test_hostile_truncations_and_limits(B, dev, oracle):
    bad = I.truncations(oracle) + [f for f, _ in HB.malformed().values()]
    cap = 4096
    consumed, out_len, status, outs = _decode(B, dev, bad, [cap] * len(bad), pad_between=1)
    for f, st, o in zip(bad, status, outs):
        hs, ho = _host(f, cap)
        assert st != OK and st == hs and o == ho, (len(f), st, hs)
    want = [w for _, w in HB.malformed().values()]
    assert status[-len(want):] == want


def test_hostile_mutations(B, dev, oracle):
    bad = I.mutations(oracle)
    cap = 4096
    consumed, out_len, status, outs = _decode(B, dev, bad, [cap] * len(bad))
    both = 0
    for f, st, o in zip(bad, status, outs):
        hs, ho = _host(f, cap)
        assert st == hs and o == ho, (st, hs)
        if st == OK:
            try:
                lib = I.unzstd(f, len(o))
            except Exception:
                continue
            assert lib == o
            both += 1
    print(f"mutations: {sum(s == OK for s in status)} accepted here, {both} of them by libzstd too")


def test_output_capacity(B, dev, oracle):
    cases = [c for c in I.libzstd_frames(oracle) if c.n in (300, 5000, 131073) and c.level == 3]
    hb = [HB.cases()[k] for k in ("overlap_offset7_long", "rle_literals", "zero_sequences")]
    frames = [c.frame for c in cases] + [f for f, _ in hb]
    sizes = [c.n for c in cases] + [len(w) for _, w in hb]
    consumed, out_len, status, outs = _decode(B, dev, frames, [n - 1 for n in sizes])  # _decode checks the guards
    assert status == [OUTPUT_FULL] * len(frames), status
    assert consumed == [0] * len(frames)
