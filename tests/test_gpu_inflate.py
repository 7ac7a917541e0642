"""nx_inflate_batch on the MI355X against zlib (tests/inflate_streams.py): crafted valid and invalid
streams, every split point of a stream with resume, output-full resume, grid edges and input
alignments, store bounds, the damaged-stream corpus, and the round trip with the project's encoder."""
import random
import zlib

import pytest

import inflate_streams as IS

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NEED, FULL = 2, 3
GUARD = 64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def B():
    from netty_amd import batch
    return batch


def _text_of(status):
    from netty_amd import _lib
    return _lib.status_string(status)


class Run:
    """One batch call over host streams: every output slot is `hist + cap` bytes between two guards
    of 64 bytes of 0xA5, which must be intact afterwards."""

    def __init__(self, B, dev, streams, caps, hists=None, state=None, align=16, shift=0):
        n = len(streams)
        hists = [b""] * n if hists is None else hists
        self.n, self.caps, self.hists = n, caps, hists
        inp, off, ln = B.pack([bytes(shift) + s for s in streams], dev, align=align)
        off = off + shift
        ln = ln - shift
        slots, cur = [], 0
        for h, c in zip(hists, caps):
            cur += GUARD
            slots.append(cur)
            cur += (len(h) + c + 15) // 16 * 16 + GUARD
        host = bytearray(b"\xA5" * (cur + 16))
        for o, h in zip(slots, hists):
            host[o:o + len(h)] = h
        self.before = bytes(host)
        out = torch.frombuffer(host, dtype=torch.uint8).to(dev)
        self.slots = slots
        self.state = torch.zeros(n * B.INFLATE_STATE_BYTES, dtype=torch.uint8, device=dev) if state is None else state
        cons, olen, st = B.inflate(inp, off, ln, out, torch.tensor(slots, dtype=torch.int64, device=dev),
                                   torch.tensor([len(h) for h in hists], dtype=torch.int32, device=dev),
                                   torch.tensor(caps, dtype=torch.int32, device=dev), self.state)
        torch.cuda.synchronize()
        self.consumed, self.out_len, self.status = cons.cpu().tolist(), olen.cpu().tolist(), st.cpu().tolist()
        self.host = out.cpu().numpy().tobytes()

    def out(self, i):
        o = self.slots[i] + len(self.hists[i])
        return self.host[o:o + self.out_len[i]]

    def check_bounds(self):
        """nothing but [hist, hist + out_len) of each slot changed"""
        got = bytearray(self.host)
        for i in range(self.n):
            assert 0 <= self.out_len[i] <= self.caps[i], i
            o = self.slots[i] + len(self.hists[i])
            got[o:o + self.out_len[i]] = self.before[o:o + self.out_len[i]]
        assert bytes(got) == self.before, "a store left its stream's output range"


def test_crafted_valid_streams(dev, B):
    S = IS.crafted_valid()
    names = list(S)
    refs = [IS.reference(S[k]) for k in names]
    r = Run(B, dev, [S[k] + b"\x55\xAA" for k in names], [len(x.out) + 300 for x in refs])
    for i, k in enumerate(names):
        assert r.status[i] == 0, (k, r.status[i], _text_of(r.status[i]))
        assert r.out(i) == refs[i].out, k
        assert r.consumed[i] == refs[i].consumed and r.out_len[i] == len(refs[i].out), k
    r.check_bounds()


def test_crafted_invalid_streams(dev, B):
    E = IS.crafted_invalid()
    names = list(E)
    refs = [IS.reference(E[k][0]) for k in names]
    r = Run(B, dev, [E[k][0] for k in names], [len(x.out) + 600 for x in refs])
    for i, k in enumerate(names):
        assert r.status[i] <= -60 and _text_of(r.status[i]) == E[k][1] == refs[i].text, (k, r.status[i])
        assert r.out(i) == refs[i].out, k
    r.check_bounds()
    # a failed stream stays failed
    again = Run(B, dev, [b"\x03\x00"] * len(names), [64] * len(names), state=r.state)
    assert again.status == r.status and not any(again.out_len) and not any(again.consumed)


def test_every_split_point_and_resume(dev, B):
    z = IS.split_stream()
    whole = IS.reference(z).out
    n = len(z)
    first = Run(B, dev, [z[:k] for k in range(n)], [len(whole) + 16] * n)
    d_out = []
    for k in range(n):
        d = zlib.decompressobj(-15)
        d_out.append(d.decompress(z[:k]))
        assert first.status[k] == NEED, (k, first.status[k])
        assert first.out(k) == d_out[k], k
        assert first.consumed[k] <= k
    first.check_bounds()
    # the rest of each stream, the history slid to at most 32 KiB, the saved state
    rest = [z[first.consumed[k]:] for k in range(n)]
    hists = [d_out[k][-32768:] for k in range(n)]
    second = Run(B, dev, rest, [len(whole) - len(d_out[k]) + 16 for k in range(n)], hists=hists, state=first.state)
    for k in range(n):
        assert second.status[k] == 0, (k, second.status[k], _text_of(second.status[k]))
        assert d_out[k] + second.out(k) == whole, k
        assert first.consumed[k] + second.consumed[k] == n, k
    second.check_bounds()


@pytest.mark.parametrize("cap", [258, 259, 1000])
def test_output_full_resume(dev, B, cap):
    data = IS.big_text(200_000)
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    z = c.compress(data) + c.flush()
    # the loop runs on the device: one stream per pass would be ~800 launches, so the passes of eight
    # streams (the same stream at eight phases of the first cap) share a launch
    lanes = 8
    first_caps = [cap + 31 * j for j in range(lanes)]
    outs = [bytearray() for _ in range(lanes)]
    pos = [0] * lanes
    state = torch.zeros(lanes * B.INFLATE_STATE_BYTES, dtype=torch.uint8, device=dev)
    done = [False] * lanes
    for it in range(3 * 200_000 // cap + 8):
        caps = [first_caps[j] if it == 0 else cap for j in range(lanes)]
        r = Run(B, dev, [z[pos[j]:pos[j] + 4096] for j in range(lanes)], caps, hists=[bytes(o[-32768:]) for o in outs], state=state)
        state = r.state
        for j in range(lanes):
            if done[j]:
                assert r.status[j] == 0 and r.out_len[j] == 0 and r.consumed[j] == 0
                continue
            # 4096 bytes of input hold far more than 1000 bytes of this text's output
            assert r.status[j] in (0, FULL), (it, j, r.status[j])
            assert r.out_len[j] > caps[j] - 258 or r.status[j] == 0, (it, j)  # stops only when the next symbol does not fit
            outs[j] += r.out(j)
            pos[j] += r.consumed[j]
            done[j] = r.status[j] == 0
        if it < 3:
            r.check_bounds()
        if all(done):
            break
    assert all(done) and all(bytes(o) == data for o in outs) and all(p == len(z) for p in pos)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 5000])
def test_grid_edges_and_alignments(dev, B, n):
    rng = random.Random(n)
    pool = []
    for k in range(24):
        payload = IS.big_text(rng.choice((0, 1, 7, 300, 2000, 9000)), seed=k) if k % 4 else bytes(rng.getrandbits(8) for _ in range(k * 9))
        c = zlib.compressobj(rng.choice((0, 1, 6, 9)), zlib.DEFLATED, -15)
        pool.append((c.compress(payload) + c.flush(), payload))
    pool.append((b"", b""))
    for shift in range(16):
        pick = [pool[rng.randrange(len(pool))] for _ in range(n)]
        r = Run(B, dev, [p[0] for p in pick], [len(p[1]) + 8 for p in pick], shift=shift)
        for i, (z, payload) in enumerate(pick):
            assert r.status[i] == (0 if z else NEED), (shift, i, r.status[i])
            assert r.out(i) == payload and r.consumed[i] == len(z), (shift, i)
        r.check_bounds()


def test_fuzz_corpus(dev, B):
    corpus = IS.fuzz_corpus()
    r = Run(B, dev, [z for z, _ in corpus], [len(ref.out) + 700 for _, ref in corpus])
    for i, (z, ref) in enumerate(corpus):
        kind = "end" if r.status[i] == 0 else "need" if r.status[i] == NEED else "error" if r.status[i] <= -60 else "?"
        assert kind == ref.kind, (i, r.status[i], ref.kind, ref.text)
        assert r.out(i) == ref.out, (i, kind)
        if kind == "error":
            assert _text_of(r.status[i]) == ref.text, i
        if kind == "end":
            assert r.consumed[i] == ref.consumed, i
    r.check_bounds()


def test_round_trip_with_the_project_encoder(dev, B):
    n, L = 64, 65536
    src = torch.empty(n * L, dtype=torch.uint8, device=dev)
    B.textgen(src, 9000, n, L)
    lens = [L - 97 * k for k in range(n)]
    off = torch.arange(n, dtype=torch.int64, device=dev) * L
    ln = torch.tensor(lens, dtype=torch.int32, device=dev)
    cap = (B.deflate_max_compressed_length(L) + 127) // 128 * 128
    enc = torch.empty(n * cap, dtype=torch.uint8, device=dev)
    eoff = torch.arange(n, dtype=torch.int64, device=dev) * cap
    elen, est = B.deflate_encode(src, off, ln, enc, eoff)
    torch.cuda.synchronize()
    assert int((est != 0).sum()) == 0
    host, eh, el = src.cpu().numpy().tobytes(), enc.cpu().numpy().tobytes(), elen.cpu().tolist()
    chunks = [host[k * L:k * L + lens[k]] for k in range(n)]
    stream = b"".join(eh[k * cap:k * cap + el[k]] for k in range(n)) + b"\x03\x00"
    want = b"".join(chunks)
    r = Run(B, dev, [stream, stream[:-2]], [len(want) + 1, len(want)])
    assert r.status == [0, NEED] and r.consumed == [len(stream), len(stream) - 2]
    assert r.out(0) == want and r.out(1) == want
    r.check_bounds()
