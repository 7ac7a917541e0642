"""GPU tests of the Brotli encoder (nx_brotli_encode_batch): every stream must equal nx_brotli_encode_host's byte
for byte (tests/test_brotli_encode_host.py checks those against libbrotli and the model decoder), with the
statuses and lengths, in batches of 1, of 65 and of every item mixed; nothing may be written outside a slot."""
import pytest

import brotli_inputs as I

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NX_ERR_INVALID_ARG, NX_ERR_BROTLI_LGWIN, NX_ERR_BROTLI_ENCODE_FULL = -100, -151, -153
GUARD = 32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def B():
    from netty_amd import batch
    return batch


@pytest.fixture(scope="module")
def items(oracle):
    return I.items(oracle)


@pytest.fixture(scope="module")
def host(B, items):
    """the host encoder's stream of every item at the default window, computed once"""
    out = {"len0": B.brotli_encode_host(b"")[1]}
    for name, data in items:
        st, s = B.brotli_encode_host(data)
        assert st == 0
        out[name] = s
    return out


def encode(B, dev, chunks, caps=None, **kw):
    """one call over `chunks` into slots pre-filled with 0xA5, GUARD bytes between slots; returns
    [(status, stream)] after checking that nothing outside [slot, slot + out_len) was written"""
    inp, off, ln = B.pack(chunks, dev, align=1, pad=16)
    caps = caps or [B.brotli_max_compressed_length(len(c)) for c in chunks]
    out, ooff = B.out_slots([c + GUARD for c in caps], dev, align=1)
    out.fill_(0xA5)
    olen, st = B.brotli_encode(inp, off, ln, out, ooff, torch.tensor(caps, dtype=torch.int32), **kw)
    torch.cuda.synchronize()
    outh, oo, ol, sl = out.cpu().numpy().tobytes(), ooff.cpu().tolist(), olen.cpu().tolist(), st.cpu().tolist()
    res = []
    for o, w, cap, s in zip(oo, ol, caps, sl):
        assert 0 <= w <= cap, (w, cap)
        assert outh[o + cap:o + cap + GUARD] == b"\xa5" * GUARD  # the guard bytes between slots
        if s == 0:
            assert outh[o + w:o + cap] == b"\xa5" * (cap - w)  # nothing past the reported length
        else:
            assert w == 0
        res.append((s, outh[o:o + w]))
    return res


def test_batches_of_one(B, dev, items, host):
    for name, data in items:
        assert encode(B, dev, [data]) == [(0, host[name])], name


def test_batch_of_65(B, dev, items, host):
    small = [(n, d) for n, d in items if len(d) <= 3300]
    pick = [small[i % len(small)] for i in range(65)]
    pick[20] = pick[40] = ("len0", b"")
    res = encode(B, dev, [d for _, d in pick])
    for (name, _), r in zip(pick, res):
        assert r == (0, host[name]), name


def test_all_items_mixed_with_empty_items(B, dev, items, host):
    pick = list(items)
    pick[5:5] = [("len0", b"")] * 3
    res = encode(B, dev, [d for _, d in pick])
    for (name, _), r in zip(pick, res):
        assert r == (0, host[name]), name


@pytest.mark.parametrize("lgwin", [10, 24])
def test_windows(B, dev, items, lgwin):
    pick = list(items)
    res = encode(B, dev, [d for _, d in pick], lgwin=lgwin)
    for (name, data), r in zip(pick, res):
        assert r == (0, B.brotli_encode_host(data, lgwin=lgwin)[1]), name


def test_one_mebibyte_beside_one_byte_items(B, dev, oracle):
    pa = pytest.importorskip("pyarrow")
    big = oracle.textgen_chunk(9, 1 << 20)
    chunks = [b"a", big, b"b", b""]
    res = encode(B, dev, chunks)
    for c, (st, s) in zip(chunks, res):
        assert st == 0 and s == B.brotli_encode_host(c)[1]
        assert pa.Codec("brotli").decompress(s, decompressed_size=len(c)).to_pybytes() == c


def test_the_arena_grows_and_is_used_again(B, dev, oracle):
    """a fresh workspace, 1-byte items, then an item that needs a larger arena, then the small call on the grown one"""
    B.workspaces_trim()
    small, big = [b"a", b"b", b"c"], [oracle.textgen_chunk(9, 1 << 20)]
    for chunks in (small, big, small):
        for c, r in zip(chunks, encode(B, dev, chunks)):
            assert r == (0, B.brotli_encode_host(c)[1])


def test_undersized_slots(B, dev, items, host):
    pick = [(n, d) for n, d in items if len(d) <= 30000][:27]
    caps, short = [], set()
    for i, (name, data) in enumerate(pick):
        full = B.brotli_max_compressed_length(len(data))
        if i % 3 == 1:
            short.add(i)
            caps.append([len(host[name]) - 1, 2, 0, len(host[name]) // 2][(i // 3) % 4])
        else:
            caps.append(len(host[name]) if i % 3 == 2 else full)  # an exact fit is not a short slot
    res = encode(B, dev, [d for _, d in pick], caps=caps)
    for i, ((name, _), r) in enumerate(zip(pick, res)):
        assert r == ((NX_ERR_BROTLI_ENCODE_FULL, b"") if i in short else (0, host[name])), name


def test_bad_window_is_refused_before_any_launch(B, dev):
    for lgwin in (-2, 9, 25):
        with pytest.raises(RuntimeError, match=str(NX_ERR_BROTLI_LGWIN)):
            encode(B, dev, [b"abc"], lgwin=lgwin)


def test_two_calls_on_one_workspace(B, dev, items, host):
    """the second call's items land on the first call's table slots: only this call's stamp counts"""
    a = [(n, d) for n, d in items if n.startswith(("copy", "ring", "few"))]
    b = list(reversed([(n, d) for n, d in items if n.startswith(("insert", "skewed", "window", "text3", "text5"))]))[:len(a)]
    for pick in (a, b, a):
        res = encode(B, dev, [d for _, d in pick])
        for (name, _), r in zip(pick, res):
            assert r == (0, host[name]), name


def test_item_over_the_cap_by_value_only(B, dev, host):
    """in_len says 256 MiB + 1 and no such buffer exists: the item is refused and nothing of it is read"""
    inp, off, ln = B.pack([b"abc", b"hello hello hello", b""], dev, align=1, pad=16)
    ln[1] = (256 << 20) + 1
    caps = [64, 64, 64]
    out, ooff = B.out_slots([c + GUARD for c in caps], dev, align=1)
    out.fill_(0xA5)
    olen, st = B.brotli_encode(inp, off, ln, out, ooff, torch.tensor(caps, dtype=torch.int32))
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0, NX_ERR_INVALID_ARG, 0]
    ol, oo, outh = olen.cpu().tolist(), ooff.cpu().tolist(), out.cpu().numpy().tobytes()
    assert ol[1] == 0 and outh[oo[1]:oo[1] + 64 + GUARD] == b"\xa5" * (64 + GUARD)
    assert outh[oo[0]:oo[0] + ol[0]] == B.brotli_encode_host(b"abc")[1] and outh[oo[2]:oo[2] + ol[2]] == host["len0"]
