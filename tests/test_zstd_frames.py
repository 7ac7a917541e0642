"""The Zstandard header reader (tests/zstd_frames.py) pinned on frames libzstd writes through pyarrow."""
import random

import pytest

import zstd_frames as Z

pa = pytest.importorskip("pyarrow")


def _text(n):
    rng = random.Random(8878)
    words = [bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz") for _ in range(rng.randrange(2, 9))) for _ in range(400)]
    return b" ".join(rng.choice(words) for _ in range(n // 3 + 2))[:n]


def _stream(data):
    """libzstd's streaming compressor: no pledged size, so a window descriptor and no content size"""
    sink = pa.BufferOutputStream()
    with pa.CompressedOutputStream(sink, "zstd") as out:
        out.write(data)
    return sink.getvalue().to_pybytes()


CONTENTS = {"text": _text(300_000), "zeros": bytes(300_000), "random": random.Random(1).randbytes(300_000)}


def _check_blocks(f, frame, kind, data):
    assert f.start == 0 and f.end == len(frame)  # every parsed size adds up to the frame length
    assert f.header + sum(3 + k.content for k in f.blocks) + (4 if f.checksum else 0) == len(frame)
    assert len(f.blocks) >= 3 and f.blocks[-1].last and not any(k.last for k in f.blocks[:-1])
    assert f.content_size in (None, len(data))
    for k in f.blocks:
        if k.type == Z.COMPRESSED:
            assert k.lit_header + k.lit_comp + k.seq_header <= k.size
            assert k.lit_regen <= 131072
    if kind == "random":
        assert all(k.type == Z.RAW for k in f.blocks) and Z.regenerated_size(f) == len(data)
    if kind == "zeros":
        assert all(k.type in (Z.RLE, Z.COMPRESSED) for k in f.blocks)
    if kind == "text":
        comp = [k for k in f.blocks if k.type == Z.COMPRESSED]
        assert len(comp) == len(f.blocks)
        assert comp[0].lit_type == Z.LIT_COMPRESSED and comp[0].tree in ("direct", "fse") and comp[0].lit_streams == 4
        assert all(k.nseq > 0 and k.modes is not None for k in comp)
        # later blocks reuse the first one's tables: treeless literals or repeat modes
        assert any(k.lit_type == Z.LIT_TREELESS or Z.SEQ_REPEAT in k.modes for k in comp[1:])


@pytest.mark.parametrize("level", [1, 3])
@pytest.mark.parametrize("kind", list(CONTENTS))
def test_reader_on_libzstd_frames(kind, level):
    """one-shot frames at the level: single segment, a 4-byte content size, several blocks"""
    data = CONTENTS[kind]
    frame = pa.Codec("zstd", compression_level=level).compress(data).to_pybytes()
    (f,) = Z.parse_frames(frame)
    assert f.single_segment and f.window_descriptor is None and (f.content_size, f.fcs_bytes) == (len(data), 4)
    _check_blocks(f, frame, kind, data)


@pytest.mark.parametrize("kind", list(CONTENTS))
def test_reader_on_libzstd_stream_frames(kind):
    """streamed frames (the stream wrapper takes no level: libzstd at its default): a window descriptor"""
    data = CONTENTS[kind]
    frame = _stream(data)
    assert pa.Codec("zstd").decompress(frame, decompressed_size=len(data)).to_pybytes() == data
    (f,) = Z.parse_frames(frame)
    assert not f.single_segment and f.window_descriptor is not None
    _check_blocks(f, frame, kind, data)


def test_reader_small_frames():
    for n in (0, 1, 255, 256, 257, 70_000):
        data = _text(n)
        frame = pa.Codec("zstd", compression_level=1).compress(data).to_pybytes()
        (f,) = Z.parse_frames(frame)
        assert f.end == len(frame) and f.content_size in (None, n)
        if f.single_segment and f.content_size is not None:
            assert f.fcs_bytes == (1 if n < 256 else 2 if n < 65792 else 4)


def test_reader_refuses_damage():
    frame = pa.Codec("zstd", compression_level=1).compress(_text(5000)).to_pybytes()
    with pytest.raises(ValueError):
        Z.parse_frame(b"\x27" + frame[1:])
    with pytest.raises(ValueError):
        Z.parse_frame(frame[:-5])
    two = Z.parse_frames(frame + frame)
    assert [f.end for f in two] == [len(frame), 2 * len(frame)]
