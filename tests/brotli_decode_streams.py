"""The streams the Brotli decoder's tests share: libbrotli's fixture and the hand-built set, valid and invalid,
the truncation cuts and the too-small capacities, each with what the decoder must say."""
import brotli_decode_inputs as I
import brotli_handbuilt as HB

GUARD = 64
CODES = {name: -154 - i for i, name in enumerate(
    ["EXUBERANT_NIBBLE", "RESERVED", "EXUBERANT_META_NIBBLE", "SIMPLE_HUFFMAN_ALPHABET", "SIMPLE_HUFFMAN_SAME", "CL_SPACE", "HUFFMAN_SPACE",
     "CONTEXT_MAP_REPEAT", "BLOCK_LENGTH_1", "BLOCK_LENGTH_2", "TRANSFORM", "DICTIONARY", "WINDOW_BITS", "PADDING_1", "PADDING_2", "DISTANCE",
     "TRUNCATED", "OUTPUT_FULL"])}
LIBBROTLI = {name: -1 - i for i, name in enumerate(list(CODES)[:16])}  # BROTLI_DECODER_ERROR_FORMAT_*
_cache = {}


def valid():
    """[(name, stream, plain)]: the fixture (plain texts regenerated) and the hand-built streams."""
    if "valid" not in _cache:
        _cache["valid"] = [(c["name"], s, I.plain(c)) for c, s in I.load()] + list(HB.VALID)
    return _cache["valid"]


def invalid():
    """[(name, stream, status)]"""
    return [(n, s, CODES[c]) for n, s, c in HB.INVALID]


def cuts():
    """[(name, cut stream)]: every valid stream cut after its first byte, in the middle and before its last byte."""
    out = []
    for name, s, _ in valid():
        for at in sorted({1, len(s) // 2, len(s) - 1}):
            if 0 < at < len(s):
                out.append(("%s@%d" % (name, at), s[:at]))
    return out


def small_caps():
    """[(name, stream, cap)]: capacities one byte short, half and zero, for valid streams with output."""
    out = []
    for name, s, p in valid():
        if p and len(p) <= 8192:
            for cap in sorted({len(p) - 1, len(p) // 2, 0}):
                out.append(("%s/cap%d" % (name, cap), s, cap))
    return out
