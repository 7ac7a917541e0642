"""Streams whose bytes hold a block or end-of-stream magic that starts no block (decoys), for the tests of the
split bzip2 decode (nx_bzip2_scan_*, nx_bzip2_decode_split_host, nx_bzip2_decode_batch_split, Bzip2Decoder).

In the payload: a block over 254 byte values has an alphabet of 256 symbols, and with flat 8-bit lengths the
canonical code of symbol s is the byte s, so the symbol bits can spell anything but the end-of-block symbol 255.
A magic laid over six whole symbols stands at the symbol stream's own bit alignment; laid over seven symbols
with `shift` free bits in front it stands `shift` bits further.  The builder reads the alignment off the written
stream and picks the shifts so that one decoy is byte-aligned and one stands at an odd bit offset.
In the tail: a block magic in the bytes after the end of the stream.
Every stream is sealed by the model (bzip2_model.seal) and the model's decode is the expectation."""
import functools

import bzip2_model as M
import bzip2_streams as S

USED = list(range(1, 255))  # 254 byte values: symbols 0 .. 255, all with 8-bit codes
FILL = [2, 3, 4, 5, 6, 7, 8, 9]


def _spell(magic: int, shift: int):
    """The symbols whose 8-bit codes hold `magic` from bit `shift` (0..7) of the first one."""
    if shift == 0:
        return list(magic.to_bytes(6, "big"))
    for lead in range(1 << shift):
        for trail in range(1 << (8 - shift)):
            v = (((lead << 48) | magic) << (8 - shift)) | trail
            sy = list(v.to_bytes(7, "big"))
            if 255 not in sy and sy[0] >= 2 and sy[-1] >= 2:
                return sy
    raise AssertionError("no spelling")


def _block(parts):
    symbols = []
    for p in parts:
        symbols += FILL + p
    symbols += FILL + [255]
    assert 255 not in symbols[:-1]
    return M.column_block(b"", 0, used=USED, symbols=symbols, selectors=[0] * M.groups_of(symbols), lengths=[M.flat_lengths(256)] * 2)


def _payload_block(magic: int, kind: int, lead_blocks):
    """A block whose symbol bits spell `magic` byte-aligned and at an odd bit offset, behind lead_blocks."""
    true = []
    probe = M.seal(1, lead_blocks + [_block([_spell(magic, 0), _spell(magic, 0)])], positions=true)
    found = [p for p in S.find_magics(probe)[kind] if p not in true]
    if kind == 1:
        found = found[:-1]  # the last end magic is the stream's own
    assert len(found) == 2 and (found[1] - found[0]) % 8 == 0, found
    a = found[0] % 8
    s_even, s_odd = (-a) % 8, (1 - a) % 8
    return _block([_spell(magic, s_even), _spell(magic, s_odd)])


@functools.lru_cache(maxsize=None)
def streams():
    """((name, stream, true block positions, decoy block positions, decoy end positions), ...); every stream
    decodes (the model says so) and every decoy is where find_magics sees it."""
    text = [M.text_block(b"first block of the decoy stream " * 3), M.text_block(b"the block behind the decoys, aaaa\x05 with a run")]
    out = []
    blk = _payload_block(S.BLOCK_MAGIC, 0, [text[0]])
    end = _payload_block(S.END_MAGIC, 1, [text[0]])
    for name, blocks, tail in (("payload_block_magic", [text[0], blk, text[1]], b""),
                               ("payload_end_magic", [text[0], end, text[1]], b""),
                               ("payload_both", [blk, text[0], end, text[1]], b""),
                               ("tail_block_magic", [text[0], text[1]], b"xy" + S.BLOCK_MAGIC.to_bytes(6, "big") + b"\x00\x01\x02 tail"),
                               ("tail_shifted_magic", [text[0], text[1]],
                                ((S.BLOCK_MAGIC << 5) | 0x15).to_bytes(7, "big") + bytes(range(40)))):
        true = []
        stream = M.seal(1, list(blocks), positions=true, tail=tail)
        st, data, used = M.decode(stream, 1 << 20)
        assert st == M.OK and used == len(stream) - len(tail)
        fb, fe = S.find_magics(stream)
        decoy_b = [p for p in fb if p not in true]
        ends_in_stream = [p for p in fe if p < 8 * used]
        decoy_e = ends_in_stream[:-1] + [p for p in fe if p >= 8 * used]
        assert set(true) <= set(fb)
        out.append((name, stream, tuple(true), tuple(decoy_b), tuple(decoy_e), data))
    by = {o[0]: o for o in out}
    for name, nb, ne in (("payload_block_magic", 2, 0), ("payload_end_magic", 0, 2), ("payload_both", 2, 2), ("tail_block_magic", 1, 0),
                         ("tail_shifted_magic", 1, 0)):
        assert (len(by[name][3]), len(by[name][4])) == (nb, ne), (name, by[name][3], by[name][4])
    for name in ("payload_block_magic", "payload_end_magic"):
        d = by[name][3] or by[name][4]
        assert d[0] % 8 == 0 and d[1] % 2 == 1, (name, d)
    return tuple(out)
