"""GPU tests of k_zstd_decode on the generated frames of tests/zstd_entropy.py: real FSE and Huffman coding
at the format's edges, which tests/test_zstd_entropy_model.py pins on libzstd.  nx_zstd_decode_host is the
second opinion on the corrupted frames, item by item."""
import pytest

import zstd_checksum_inputs as K
import zstd_entropy as E
from test_gpu_zstd_decode import B, _decode, _host, dev  # noqa: F401  (fixtures; guards, 0xA5 fill, odd slots)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

OK, CORRUPT, OUTPUT_FULL = 0, -86, -87


def test_every_case_in_one_launch(B, dev):
    c = E.cases()
    consumed, out_len, status, outs = _decode(B, dev, [f for f, _ in c.values()], [len(w) for _, w in c.values()])
    for (name, (f, want)), co, st, o in zip(c.items(), consumed, status, outs):
        assert st == OK and co == len(f), (name, st, co)
        assert o == want, name


def test_every_case_one_byte_short(B, dev):
    c = E.cases()
    consumed, out_len, status, outs = _decode(B, dev, [f for f, _ in c.values()], [len(w) - 1 for _, w in c.values()])  # _decode checks the guards
    assert status == [OUTPUT_FULL] * len(c), [n for n, s in zip(c, status) if s != OUTPUT_FULL]
    assert consumed == [0] * len(c)


def test_targeted_corruption(B, dev):
    bad = E.bit_flips() + E.truncations()
    cap = 4096
    consumed, out_len, status, outs = _decode(B, dev, bad, [cap] * len(bad), pad_between=1)
    for i, (f, st, o) in enumerate(zip(bad, status, outs)):
        hs, ho = _host(f, cap)
        assert st == hs and o == ho, (i, len(f), st, hs)
    print(f"{len(bad)} corrupted frames, {sum(s == OK for s in status)} accepted")


def test_state_left_by_the_previous_frame_of_a_wave(B, dev):
    """one workspace slot, so one wave decodes all five in order: what the first leaves in LDS must not
    make a Treeless or Repeat_Mode first block decodable"""
    batch, _ = E.stale_state_batch()
    frames = [f for f, _ in batch]
    cap = 8192
    alone = [_host(f, cap) for f in frames]
    assert [s for s, _ in alone] == [OK, CORRUPT, CORRUPT, OK, OK]
    torch.cuda.synchronize()
    B.workspaces_trim()
    try:
        B.zstd_decoder_reserve(1)
        assert B.workspace_info(B.WS_ZSTD_DEC)[0] == 131072
        consumed, out_len, status, outs = _decode(B, dev, frames, [cap] * 5)
    finally:
        torch.cuda.synchronize()
        B.workspaces_trim()
    assert status == [OK, CORRUPT, CORRUPT, OK, OK]
    assert outs == [o for _, o in alone]
    assert [outs[k] for k in (0, 3, 4)] == [batch[k][1] for k in (0, 3, 4)]
    assert consumed == [len(frames[0]), 0, 0, len(frames[3]), len(frames[4])]


def test_checksum_over_huffman_literals_and_long_matches(B, dev):
    """the checksum reads back what the Huffman path and long matches wrote in the same launch"""
    pytest.importorskip("xxhash")
    from test_gpu_zstd_checksum import _launch
    c = E.cases()
    frames, caps, want = [], [], []
    for k, name in enumerate(("lit4_format2_16383", "huffman_then_overlap", "widest_sequence")):
        f, data = c[name]
        g = K.with_checksum(f, data)
        frames += [g, K.wrong_checksum(g, k, 2 * k + 1)]
        caps += [len(data)] * 2
        want += [(OK, data, len(g)), (K.CHECKSUM, data, 0)]
    assert _launch(B, dev, frames, caps, True) == want
