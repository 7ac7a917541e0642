"""What every synchronous decoder handle delivers, read by read, against a recording
(tests/golden/decoder_messages.json, written by scripts/record_decoder_messages.py from the commit before
the decode bodies were folded into nx::h::DecodeCall, DecodeItems and ParamBlock): each message's SHA-256
and length or the exception, the bytes left in the cumulation, is_closed() and stats().  The read
sequences are in decoder_sequences.py."""
import bz2
import json
import os

import pytest

import bzip2_streams
import decoder_sequences as S

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CASES = S.cases()


@pytest.fixture(scope="module")
def H():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from netty_amd import handlers
    return handlers


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decoder_messages.json")) as f:
        return json.load(f)


def test_every_case_is_recorded(golden):
    assert golden["unstable"] == []
    assert sorted(golden["cases"]) == sorted(c[0] for c in CASES)


def test_grow_stream_is_one_block(golden):
    """the stream of bzip2/grow_and_retry: one level-1 block that decodes to more than the first output slot
    (count x 100 000 + 65 536 bytes), so the recorded two launches are the retry"""
    blocks, ends = bzip2_streams.find_magics(bz2.compress(bytes(S.GROW_STREAM_BYTES), 1))
    assert len(blocks) == 1 and len(ends) == 1
    assert S.GROW_STREAM_BYTES > 1 * 100000 + 65536
    assert golden["cases"]["bzip2/grow_and_retry"]["stats"]["launches"] == 2


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_recorded_messages(H, golden, case):
    want = dict(golden["cases"][case[0]])
    assert S.input_digest(case) == want.pop("input_sha256"), "the inputs differ from the recorded run's"
    assert S.run(H, case) == want
