"""GPU tests of the bzip2 decoder (nx_bzip2_decode_batch) on hand-built streams (tests/bzip2_handbuilt.py):
one launch per group of cases, valid and invalid items mixed.  Every item must equal the model decoder
(tests/bzip2_model.py) in status, out_len and consumed, and in bytes when it decodes, and must equal
nx_bzip2_decode_host item for item.  tests/test_bzip2_handbuilt_host.py holds the model against libbz2."""
import pytest

import bzip2_handbuilt as H
import bzip2_streams as S

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from bzip2_gpu import decode, equal_host  # noqa: E402  (after torch is known to be there)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def B():
    from netty_amd import batch
    return batch


def _run(B, dev, cases):
    streams, caps = [c.stream for c in cases], [c.cap for c in cases]
    got = decode(B, dev, streams, caps)
    out_len, consumed, status, res = got
    for i, c in enumerate(cases):
        assert (status[i], out_len[i], consumed[i]) == (c.status, len(c.data), c.consumed), c.name
        if c.status == S.OK:
            assert res[i] == c.data, c.name
    equal_host(B, streams, caps, got)


@pytest.mark.parametrize("group", H.GROUPS)
def test_group(B, dev, group):
    cases = H.group(B.bzip2_decode_chains(), group)
    sts = {c.status for c in cases}
    assert S.OK in sts and len(sts) > 1  # valid and invalid items in one launch
    _run(B, dev, cases)


def test_run_of_900000(B, dev):
    """One level-9 block of 900000 equal bytes as a single run, between an invalid and a small valid item."""
    by = {c.name: c for c in H.group(B.bzip2_decode_chains(), "runs")}
    _run(B, dev, [by["fill_100001_by_run"], H.big_case(), by["run1025_at0_sym"]])


def test_walk_on_two_slots(B, dev):
    """The walk group on two slots, long and short blocks in turn, twice: a slot's flagged entries and the pre-RLE
    bytes of a longer block must not show in the shorter one that follows on it."""
    cases = sorted(H.group(B.bzip2_decode_chains(), "walk"), key=lambda c: len(c.stream))
    half = len(cases) // 2
    longs, shorts = cases[half:][::-1], cases[:half]
    order = []  # a wave takes items blockIdx, blockIdx + 2, ...: two long, two short, so each slot sees long, short, long, short
    for k in range(0, half, 2):
        order += longs[k:k + 2] + shorts[k:k + 2]
    B.workspaces_trim()
    B.bzip2_decoder_reserve(2)
    try:
        assert B.workspace_info(B.WS_BZIP2_DEC)[0] == 2 * (6 * 900000 + 256)
        for _ in range(2):
            _run(B, dev, order)
    finally:
        B.workspaces_trim()
