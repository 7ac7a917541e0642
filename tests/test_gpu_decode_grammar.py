"""GPU decoders on generated VALID streams that none of the project's encoders emits.

tests/streamgen.py builds the streams from op lists in every form the formats allow (Snappy COPY_4,
copies under 4 bytes, literal codes 62 / 63, wider-than-needed literal fields, padded preambles,
offsets above 65535; LZ4 / LZF / FastLZ length extensions, long matches, every offset form) and
states what they decode to with its own byte loop.  Every check here is three-way: the GPU's bytes,
out_len, consumed, status and CRC against the builder's expectation and against the oracle's
decoder, which tests/test_streamgen.py pins to the builder on the CPU.  The whole output buffer is
compared, slot gaps included, so a store outside a frame's [0, out_len) fails too.

Which set covers what (tests/streamgen.py `snappy_sets` / `alt_sets`):
  overlap_grid   offset 1..68 x length 1..64 x COPY_1/2/4 x output phase 0..3
  ring_sweep     every offset in [1780, 2056] and [3830, 4104] and 8191 / 8192 / 32767 / 32768 (65535:
                 in the 200 000-byte frame of `large`), lengths 1 3 4 5 63 64, phases 0..3, k one-byte
                 records first (k = 0 1 31 62 63 64 65), random history
  edges          ops ending at / one short of / one past output 512 j and input 512 j, 1024 j; frames of
                 7 8 9 511 512 513 2047 2048 2049 4096 65536 bytes
  chains         70-200 back-to-back 4-byte copies at offsets 1 2 3 4 5 8 60 63 64
  straddles      5-byte COPY_4, 3-byte COPY_2 and 2-5-byte literal headers starting at input byte 59..64 mod 64
  large          65 537, 70 000, 200 000 and 1 200 011 bytes of output (the last: above 16384 records, the
                 pair path's fused fallback), COPY_4 offsets 65535 / 65536 / 65537 / output - 1
  walk           200 frames of 100 B - 20 KB drawing every form, 70 % of the offsets from the lists above
The ring sweep and the walk run with input and output slots packed at alignment 1 and 16, CRC
requested (the byte-store flush and its CRC fold); the other sets at (16, 16) and (1, 1).
"""
import base64
import json
import os
import zlib

import pytest

import streamgen as G

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

VARIANTS = ["auto", "pair", "fused", "naive"]
ALIGNS = [(16, 16), (1, 1), (1, 16), (16, 1)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def B():
    from netty_amd import batch
    return batch


_ORACLE = {}


def _snappy_oracle(oracle, name):
    """Per case of a Snappy set, once per module: the oracle's (status, bytes, consumed) at out_cap
    2^24, checked against the builder, and the masked CRC32C of the bytes."""
    if name not in _ORACLE:
        rows = []
        for s, want in G.snappy_sets()[name]:
            st, out, cons = oracle.snappy_decode(s, 1 << 24)
            assert (st, out, cons) == (0, want, len(s)), name
            rows.append(oracle.snappy_checksum(want))
        _ORACLE[name] = rows
    return _ORACLE[name]


def _decode_snappy(dev, B, naive_decode, cases, crcs, variant, in_align, out_align, caps=None):
    """Decode (stream, expected) cases in one batch and compare everything.  caps: out_cap per frame
    (None: frames up to 65536 bytes get the exact length and no out_cap array in turn)."""
    streams = [s for s, _ in cases]
    wants = [w for _, w in cases]
    inp, off, ln = B.pack(streams, dev, align=in_align)
    out, ooff = B.out_slots([len(w) for w in wants], dev, align=out_align)
    cap = None if caps is None else torch.tensor(caps, dtype=torch.int32, device=dev)
    exp = torch.tensor(crcs, dtype=torch.int64).to(torch.int32).to(dev)
    r = B.snappy_decode(inp, off, ln, out, ooff, out_cap=cap, expected_crc=exp, want_crc=True, consumed=True,
                        variant="auto" if variant == "naive" else variant, fn=naive_decode if variant == "naive" else None)
    torch.cuda.synchronize()
    st, olen, cons = r["status"].cpu().tolist(), r["out_len"].cpu().tolist(), r["consumed"].cpu().tolist()
    crc = [x & 0xFFFFFFFF for x in r["crc"].cpu().tolist()]
    got, oo = out.cpu().numpy().tobytes(), ooff.cpu().tolist()
    tag = (variant, in_align, out_align)
    for i, w in enumerate(wants):
        assert st[i] == 0, (tag, i, st[i])
        assert olen[i] == len(w), (tag, i, olen[i], len(w))
        assert cons[i] == len(streams[i]), (tag, i, cons[i], len(streams[i]))
        if got[oo[i]:oo[i] + len(w)] != w:
            g = got[oo[i]:oo[i] + len(w)]
            first = next(k for k in range(len(w)) if g[k] != w[k])
            raise AssertionError((tag, i, "first wrong byte", first, "of", len(w), g[first:first + 8].hex(), w[first:first + 8].hex()))
        assert crc[i] == crcs[i], (tag, i, hex(crc[i]), hex(crcs[i]))
    want_buf = bytearray(len(got))
    for o, w in zip(oo, wants):
        want_buf[o:o + len(w)] = w
    assert got == bytes(want_buf), (tag, "bytes stored outside a frame's output")


def _exact_or_default_caps(cases):
    """out_cap per frame: the exact output length for every second frame, Java's 65536 for the others."""
    return [len(w) if i % 2 else 65536 for i, (_, w) in enumerate(cases)]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", ["overlap_grid", "edges", "chains", "straddles"])
def test_snappy_small_sets(dev, B, oracle, naive_decode, name, variant):
    """Overlap grid; flush and stage edges; dependency chains (a pass of 64 pieces that each wait for
    the one before needs 64 rounds, the round guard's limit: bytes and status are still the
    oracle's); tag-window straddles.  Slots at alignment 16 without out_cap, then at alignment 1 with
    out_cap exact or 65536."""
    cases, crcs = G.snappy_sets()[name], _snappy_oracle(oracle, name)
    _decode_snappy(dev, B, naive_decode, cases, crcs, variant, 16, 16)
    _decode_snappy(dev, B, naive_decode, cases, crcs, variant, 1, 1, caps=_exact_or_default_caps(cases))


@pytest.mark.parametrize("in_align,out_align", ALIGNS)
@pytest.mark.parametrize("variant", VARIANTS)
def test_snappy_ring_sweep(dev, B, oracle, naive_decode, variant, in_align, out_align):
    """Copies whose offset brackets the output ring (and the 4096-byte ring of the alternative build)
    by one 256-byte pass, and the ends of the offset fields: the near / far switch of the expander,
    its unaligned far load and, at output alignment 1, the byte-store flush with its CRC fold."""
    cases, crcs = G.snappy_sets()["ring_sweep"], _snappy_oracle(oracle, "ring_sweep")
    _decode_snappy(dev, B, naive_decode, cases, crcs, variant, in_align, out_align,
                   caps=_exact_or_default_caps(cases) if in_align == 1 else None)


@pytest.mark.parametrize("in_align,out_align", ALIGNS)
@pytest.mark.parametrize("variant", VARIANTS)
def test_snappy_mixed_walk(dev, B, oracle, naive_decode, variant, in_align, out_align):
    cases, crcs = G.snappy_sets()["walk"], _snappy_oracle(oracle, "walk")
    _decode_snappy(dev, B, naive_decode, cases, crcs, variant, in_align, out_align,
                   caps=_exact_or_default_caps(cases) if out_align == 1 else None)


@pytest.mark.parametrize("variant", VARIANTS)
def test_snappy_large_out_cap(dev, B, oracle, naive_decode, variant):
    """Frames above 65536 bytes of output, reachable only through out_cap: the exact length and 2^24
    decode; 2^20 decodes all but the 1.2 MB frame; length - 1 gives the oracle's overflow status with
    nothing written.  Alignment 1 for the exact caps: a frame's neighbours sit right beside it."""
    cases, crcs = G.snappy_sets()["large"], _snappy_oracle(oracle, "large")
    _decode_snappy(dev, B, naive_decode, cases, crcs, variant, 16, 16, caps=[1 << 24] * len(cases))
    _decode_snappy(dev, B, naive_decode, cases, crcs, variant, 1, 1, caps=[len(w) for _, w in cases])
    small = [(c, k) for c, k in zip(cases, crcs) if len(c[1]) <= 1 << 20]
    _decode_snappy(dev, B, naive_decode, [c for c, _ in small], [k for _, k in small], variant, 1, 16, caps=[1 << 20] * len(small))
    # caps below the preamble: every frame overflows before its first tag, as the oracle says
    streams = [s for s, _ in cases] * 2
    caps = [len(w) - 1 for _, w in cases] + [min(len(w) - 1, 1 << 20) for _, w in cases]
    inp, off, ln = B.pack(streams, dev, align=1)
    out, ooff = B.out_slots([16] * len(streams), dev)
    r = B.snappy_decode(inp, off, ln, out, ooff, out_cap=torch.tensor(caps, dtype=torch.int32, device=dev), want_crc=True,
                        consumed=True, variant="auto" if variant == "naive" else variant, fn=naive_decode if variant == "naive" else None)
    torch.cuda.synchronize()
    for i, s in enumerate(streams):
        wst, wout, wcons = oracle.snappy_decode(s, caps[i])
        assert wst != 0 and wout == b""
        assert (int(r["status"][i]), int(r["out_len"][i]), int(r["consumed"][i])) == (wst, 0, wcons), (variant, i)
    assert int(out.count_nonzero()) == 0


# ---------------------------------------------------------------------------- LZ4 / LZF / FastLZ


def _alt_oracle(oracle, name):
    key = "alt:" + name
    if key not in _ORACLE:
        cases = [c for _, v in sorted(G.alt_sets(name).items()) for c in v]
        for s, want in cases:
            if name == "lz4":
                assert oracle.lz4_decompress(s, len(want)) == (0, want)
            elif name == "lzf":
                assert oracle.lzf_decode_chunk(s, len(want)) == (0, want)
            else:
                assert oracle.fastlz_decompress(s, len(want)) == (len(want), want)
        _ORACLE[key] = cases
    return _ORACLE[key]


@pytest.mark.parametrize("in_align,out_align", ALIGNS)
@pytest.mark.parametrize("name", sorted(G.ALT))
def test_alt_codec_sets(dev, B, oracle, name, in_align, out_align):
    """Every set of `alt_sets(name)` in one batch through the codec's batch entry point: the overlap
    grid, the offset sweeps around 2048 / 4096 and at each offset form's ends (LZ4 65535; LZF and
    FastLZ level 1 8192; level 2 8191 / 8192 / 8193 and the far form's 73727), long matches that the
    parsers split into 64-byte records, the length-extension edge values and a random walk, decoded
    by the record path; and the two `many_records` blocks, whose more than 16384 records leave them
    to the codec's lane-serial decoder.  That is the only way a valid block reaches the lane-serial
    decoders (records.hpp: an error, a read past the block's end, or too many records), so of the
    generated forms they see short literals and short matches at a few offsets, no more."""
    cases = _alt_oracle(oracle, name)
    streams, wants = [s for s, _ in cases], [w for _, w in cases]
    inp, off, ln = B.pack(streams, dev, align=in_align)
    out, ooff = B.out_slots([len(w) for w in wants], dev, align=out_align)
    olen = torch.tensor([len(w) for w in wants], dtype=torch.int32, device=dev)
    if name == "lz4":
        res, ok = B.lz4_decode(inp, off, ln, out, ooff, olen), [0] * len(cases)
    elif name == "lzf":
        res, ok = B.lzf_decode(inp, off, ln, out, ooff, olen), [0] * len(cases)
    else:
        res, ok = B.fastlz_decompress(inp, off, ln, out, ooff, olen), [len(w) for w in wants]
    torch.cuda.synchronize()
    res = res.cpu().tolist()
    got, oo = out.cpu().numpy().tobytes(), ooff.cpu().tolist()
    tag = (name, in_align, out_align)
    for i, w in enumerate(wants):
        assert res[i] == ok[i], (tag, i, res[i], ok[i])
        if got[oo[i]:oo[i] + len(w)] != w:
            g = got[oo[i]:oo[i] + len(w)]
            first = next(k for k in range(len(w)) if g[k] != w[k])
            raise AssertionError((tag, i, "first wrong byte", first, "of", len(w), g[first:first + 8].hex(), w[first:first + 8].hex()))
    want_buf = bytearray(len(got))
    for o, w in zip(oo, wants):
        want_buf[o:o + len(w)] = w
    assert got == bytes(want_buf), (tag, "bytes stored outside a block's output")


# ---------------------------------------------------------------------------- a foreign encoder's streams


@pytest.fixture(scope="module")
def foreign():
    """tests/golden/foreign_streams.json (make_golden.py): inputs and their libsnappy / liblz4 streams."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "foreign_streams.json")) as f:
        doc = json.load(f)
    return [{"name": c["name"], "input": zlib.decompress(base64.b64decode(c["input_zlib"])),
             "snappy": base64.b64decode(c["snappy"]), "lz4": base64.b64decode(c["lz4"])} for c in doc["cases"]]


@pytest.mark.parametrize("variant", VARIANTS)
def test_snappy_decodes_libsnappy_streams(dev, B, oracle, naive_decode, foreign, variant):
    cases = [(c["snappy"], c["input"]) for c in foreign]
    crcs = [oracle.snappy_checksum(w) for _, w in cases]
    _decode_snappy(dev, B, naive_decode, cases, crcs, variant, 1, 1)


def test_lz4_decodes_liblz4_streams(dev, B, foreign):
    wants = [c["input"] for c in foreign]
    inp, off, ln = B.pack([c["lz4"] for c in foreign], dev, align=1)
    out, ooff = B.out_slots([len(w) for w in wants], dev, align=1)
    st = B.lz4_decode(inp, off, ln, out, ooff, torch.tensor([len(w) for w in wants], dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0] * len(wants)
    assert out.cpu().numpy().tobytes()[:sum(len(w) for w in wants)] == b"".join(wants)
