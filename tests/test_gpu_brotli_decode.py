"""GPU tests of the Brotli stream decoder (nx_brotli_decode_batch).  The oracle is libbrotli: the fixture's
streams are its encoder's and must regenerate their plain texts; nx_brotli_decode_host, which
tests/test_brotli_decode_host.py holds against libbrotli's decoder, is the second opinion item for item: the
kernel and the host decoder run the same format functions, so status, sizes and bytes must agree."""
import pytest

import brotli_decode_streams as S
import brotli_inputs

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

OK = 0
GUARD = S.GUARD


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def B():
    from netty_amd import batch
    return batch


_host = {}


def host(B, stream, cap):
    key = (stream, cap)
    if key not in _host:
        _host[key] = B.brotli_decode_host(stream, cap)
    return _host[key]


def decode(B, dev, streams, caps):
    """One launch.  Item i's slot has caps[i] bytes behind a guard of GUARD bytes (slots at odd addresses too),
    everything pre-filled with 0xA5.  Returns [(status, output, consumed)] with the guards checked."""
    inp, off, ln = B.pack(streams, dev, align=1, pad=16)
    out, ooff = B.out_slots([c + GUARD for c in caps] + [GUARD], dev, align=1)
    out.fill_(0xA5)
    ooff = ooff[:-1] + GUARD
    cap_t = torch.tensor(caps, dtype=torch.int32, device=dev)
    olen, used, st = B.brotli_decode(inp, off, ln, out, ooff, cap_t)
    torch.cuda.synchronize()
    raw, oo = out.cpu().numpy().tobytes(), ooff.cpu().tolist()
    res = []
    for o, cap, w, u, s in zip(oo, caps, olen.cpu().tolist(), used.cpu().tolist(), st.cpu().tolist()):
        assert 0 <= w <= cap
        assert raw[o - GUARD:o] == b"\xa5" * GUARD and raw[o + cap:o + cap + GUARD] == b"\xa5" * GUARD, "a byte outside the slot"
        res.append((s, raw[o:o + w], u))
    return res


def test_all_streams_in_one_batch(B, dev):
    valid, invalid = S.valid(), S.invalid()
    streams = [s for _, s, _ in valid] + [s for _, s, _ in invalid]
    caps = [len(p) + (i % 3) for i, (_, _, p) in enumerate(valid)] + [66000] * len(invalid)
    order = list(range(len(streams)))
    order = order[::2] + order[1::2]  # valid and invalid mixed
    res = decode(B, dev, [streams[i] for i in order], [caps[i] for i in order])
    for k, i in enumerate(order):
        assert res[k] == host(B, streams[i], caps[i]), i
        if i < len(valid):
            assert res[k] == (OK, valid[i][2], len(streams[i])), valid[i][0]
        else:
            assert res[k][0] == invalid[i - len(valid)][2] and res[k][2] == 0, invalid[i - len(valid)][0]


def _small(k):
    return [(n, s, p) for n, s, p in S.valid() if 0 < len(p) <= 4200][:k]


def test_batch_shapes(B, dev):
    v = _small(5)
    empty = next((n, s, p) for n, s, p in S.valid() if not p)
    assert decode(B, dev, [v[0][1]], [len(v[0][2])]) == [(OK, v[0][2], len(v[0][1]))]
    three = [v[1], empty, v[2]]
    assert decode(B, dev, [s for _, s, _ in three], [len(p) for _, _, p in three]) == [(OK, p, len(s)) for _, s, p in three]
    assert decode(B, dev, [v[3][1] + b"\x00\xffafter"], [len(v[3][2]) + 5]) == [(OK, v[3][2], len(v[3][1]))]


def test_reserve_reuses_slots_and_trim(B, dev):
    v = _small(5)
    want = [(OK, p, len(s)) for _, s, p in v]
    B.workspaces_trim()
    B.brotli_decoder_reserve(2)
    assert decode(B, dev, [s for _, s, _ in v], [len(p) for _, _, p in v]) == want
    assert B.workspace_info(B.WS_BROTLI_DEC)[0] == 2 * 802304
    B.workspaces_trim()
    assert B.workspace_info(B.WS_BROTLI_DEC)[0] == 0
    B.brotli_decoder_reserve(2)
    assert decode(B, dev, [s for _, s, _ in v], [len(p) for _, _, p in v]) == want
    B.workspaces_trim()


@pytest.mark.parametrize("lgwin", [10, -1])
def test_round_trip_with_own_encoder(B, dev, lgwin):
    items = [d for _, d in brotli_inputs.directed()]
    inp, off, ln = B.pack(items, dev, align=1, pad=16)
    caps = [B.brotli_max_compressed_length(len(d)) for d in items]
    enc, eoff = B.out_slots(caps, dev, align=1)
    elen, est = B.brotli_encode(inp, off, ln, enc, eoff, torch.tensor(caps, dtype=torch.int32), lgwin=lgwin)
    assert int((est != 0).sum()) == 0
    out, ooff = B.out_slots([len(d) + GUARD for d in items], dev, align=1)
    out.fill_(0xA5)
    cap_t = torch.tensor([len(d) for d in items], dtype=torch.int32, device=dev)
    olen, used, st = B.brotli_decode(enc, eoff, elen, out, ooff, cap_t)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [OK] * len(items)
    assert used.cpu().tolist() == elen.cpu().tolist()
    raw = out.cpu().numpy().tobytes()
    for o, d, w in zip(ooff.cpu().tolist(), items, olen.cpu().tolist()):
        assert w == len(d) and raw[o:o + w] == d and raw[o + w:o + w + GUARD] == b"\xa5" * GUARD


def test_truncated_and_output_full(B, dev):
    cuts, caps = S.cuts(), S.small_caps()
    streams = [s for _, s in cuts] + [s for _, s, _ in caps]
    cap_list = [80000 if len(s) > 4000 else 9000 for _, s in cuts] + [c for _, _, c in caps]
    res = decode(B, dev, streams, cap_list)
    for k, (name, s) in enumerate(cuts):
        assert (res[k][0], res[k][2]) == (S.CODES["TRUNCATED"], 0), name
        assert res[k] == host(B, s, cap_list[k]), name
    for k, (name, s, cap) in enumerate(caps, len(cuts)):
        assert (res[k][0], res[k][2]) == (S.CODES["OUTPUT_FULL"], 0), name
        assert res[k] == host(B, s, cap), name
