"""tests/lzma_model.py pinned against streams liblzma wrote (Python's lzma, FORMAT_ALONE): it must decode them to
the input for several lc, lp, pb, and refuse them with a byte cut off or appended."""
import lzma
import random

import pytest

import lzma_model as M

PROPS = [(3, 0, 2), (0, 0, 0), (4, 0, 0), (0, 4, 4), (1, 3, 1), (2, 2, 3)]


def _inputs():
    r = random.Random(11)
    return [b"", b"a", b"hello hello hello hello hello", bytes(r.randrange(97, 101) for _ in range(5000)), r.randbytes(300),
            b"ab" * 4000, b"q" * 1000]


@pytest.mark.parametrize("lc,lp,pb", PROPS)
def test_model_decodes_liblzma_streams(lc, lp, pb):
    kinds = set()
    for d in _inputs():
        s = lzma.compress(d, format=lzma.FORMAT_ALONE,
                          filters=[{"id": lzma.FILTER_LZMA1, "lc": lc, "lp": lp, "pb": pb, "dict_size": 4096}])
        assert M.parse_header(s)[:4] == (lc, lp, pb, 4096)
        out, packets = M.decode(s)
        assert out == d
        assert sum(n for kind, n, _ in packets if kind != M.END_MARKER) == len(d)
        kinds |= {k for k, _, _ in packets}
        for bad in (s[:-1], s + b"\0"):
            with pytest.raises(M.LzmaError):
                M.decode(bad)
    assert {M.LIT, M.MATCHED_LIT, M.MATCH, M.REP0, M.END_MARKER} <= kinds  # liblzma writes unknown size and a marker
