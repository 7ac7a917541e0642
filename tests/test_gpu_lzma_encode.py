"""GPU tests of the LZMA encoder (nx_lzma_encode_batch): every stream must equal nx_lzma_encode_host's byte for
byte (tests/test_lzma_encode_host.py checks those against liblzma and the model decoder), with the statuses and
lengths, in batches of 1, of 65 and of every item mixed; nothing may be written outside a slot."""
import lzma

import pytest

import lzma_inputs as I

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NX_ERR_LZMA_PROPS, NX_ERR_LZMA_ENCODE_FULL = -140, -143
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
    """the host encoder's stream of every item at the default settings, computed once"""
    out = {}
    for name, data in items:
        st, s = B.lzma_encode_host(data)
        assert st == 0
        out[name] = s
    return out


def encode(B, dev, chunks, caps=None, **kw):
    """one call over `chunks` into slots pre-filled with 0xA5, GUARD bytes between slots; returns
    [(status, stream)] after checking that nothing outside [slot, slot + out_len) was written"""
    inp, off, ln = B.pack(chunks, dev, align=1, pad=16)
    caps = caps or [B.lzma_max_compressed_length(len(c)) for c in chunks]
    out, ooff = B.out_slots([c + GUARD for c in caps], dev, align=1)
    out.fill_(0xA5)
    olen, st = B.lzma_encode(inp, off, ln, out, ooff, torch.tensor(caps, dtype=torch.int32), **kw)
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
        if name in ("text200k", "random65536", "run65536"):
            continue  # they run in the mixed batch
        assert encode(B, dev, [data]) == [(0, host[name])], name


def test_batch_of_65(B, dev, items, host):
    small = [(n, d) for n, d in items if len(d) <= 1100]
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


@pytest.mark.parametrize("lc,lp,pb", I.PROPS[1:])
@pytest.mark.parametrize("end_marker", [False, True])
def test_properties_and_end_marker(B, dev, lc, lp, pb, end_marker):
    pick = [(n, d) for n, d in I.directed() if len(d) <= 11000]
    res = encode(B, dev, [d for _, d in pick], lc=lc, lp=lp, pb=pb, end_marker=end_marker)
    for (name, data), r in zip(pick, res):
        assert r == (0, B.lzma_encode_host(data, lc, lp, pb, 65536, end_marker)[1]), name


@pytest.mark.parametrize("name,data,dict_size", I.dict_cases(), ids=[c[0] for c in I.dict_cases()])
def test_dictionary_sizes(B, dev, name, data, dict_size):
    assert encode(B, dev, [data], dict_size=dict_size) == [(0, B.lzma_encode_host(data, dict_size=dict_size)[1])]


def test_one_mebibyte_beside_one_byte_items(B, dev, oracle):
    big = oracle.textgen_chunk(9, 1 << 20)
    chunks = [b"a", big, b"b", b""]
    res = encode(B, dev, chunks)
    for c, (st, s) in zip(chunks, res):
        assert st == 0 and s == B.lzma_encode_host(c)[1]
        d = lzma.LZMADecompressor(format=lzma.FORMAT_ALONE)
        assert d.decompress(s) == c and d.eof and d.unused_data == b""


def test_the_arena_grows_and_is_used_again(B, dev, oracle):
    """a fresh workspace, 1-byte items, then an item that needs a larger arena, then the small call on the grown one"""
    B.workspaces_trim()
    small, big = [b"a", b"b", b"c"], [oracle.textgen_chunk(9, 1 << 20)]
    for chunks in (small, big, small):
        for c, r in zip(chunks, encode(B, dev, chunks)):
            assert r == (0, B.lzma_encode_host(c)[1])


def test_undersized_slots(B, dev, items, host):
    pick = [(n, d) for n, d in items if len(d) <= 11000][:24]
    caps, short = [], set()
    for i, (name, data) in enumerate(pick):
        full = B.lzma_max_compressed_length(len(data))
        if i % 3 == 1:
            short.add(i)
            caps.append([len(host[name]) - 1, 12, 0, len(host[name]) // 2][(i // 3) % 4])
        else:
            caps.append(len(host[name]) if i % 3 == 2 else full)  # an exact fit is not a short slot
    res = encode(B, dev, [d for _, d in pick], caps=caps)
    for i, ((name, _), r) in enumerate(zip(pick, res)):
        assert r == ((NX_ERR_LZMA_ENCODE_FULL, b"") if i in short else (0, host[name])), name


def test_lc_plus_lp_over_four_is_refused(B, dev):
    for lc, lp in [(3, 2), (8, 4), (4, 1)]:
        with pytest.raises(RuntimeError, match=str(NX_ERR_LZMA_PROPS)):
            encode(B, dev, [b"abc"], lc=lc, lp=lp)


def test_two_calls_on_one_workspace(B, dev, items, host):
    """the second call's items land on the first call's table slots and models: stamps and re-initialisation"""
    a = [(n, d) for n, d in items if n.startswith(("dist", "cycle", "period"))]
    b = list(reversed([(n, d) for n, d in items if n.startswith(("mlen", "run2", "run5", "random1", "random2"))]))[:len(a)]
    for pick in (a, b, a):
        res = encode(B, dev, [d for _, d in pick])
        for (name, _), r in zip(pick, res):
            assert r == (0, host[name]), name
