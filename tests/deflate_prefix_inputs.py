"""Inputs and yardsticks for the deflate encoder's history prefix (nx_deflate_encode_batch_ex) and the
preset-dictionary handles.  Pure Python: no kernel and no oracle builds them; tests/
test_deflate_prefix_inputs.py pins every one of them on the machine's zlib, the GPU tests run them.

A case is (prefix, chunk): the chunk is encoded with the prefix as history.  Its output alone is not a
deflate stream (its distances reach before its first byte), so the tokens are read from
stored_block(prefix) + output: one non-final stored block puts the prefix into the reader's window (and
into zlib's), and the chunk's own blocks follow it byte-aligned.

The matcher keeps one position per hash slot, the latest.  A case that relies on a source position
restates the slot function to check that nothing entered between the source and the probe lands in the
source's slot (slot_kept); the restatement keeps slots free, it predicts no output."""
import random
import zlib

from deflate_blocks import read_blocks
from lz_inputs import text

MAX_DIST = 32768
MAX_CHUNK = 65536
PREFIX_LENS = [0, 1, 3, 4, 5, 255, 32767, 32768]
CHUNK_LENS = [1, 3, 4, 5, 259]           # and 65536 - prefix_len
DICT_LENS = [0, 1, 2, 3, 100, 32768, 32769, 40000]


def slot(w: bytes) -> int:
    """k_deflate_match's table slot of the 4 bytes w"""
    return ((int.from_bytes(w[:4], "little") * 2654435761) & 0xFFFFFFFF) >> 20


def slot_kept(flat: bytes, src: int, probe: int) -> bool:
    """no position in (src, probe) of flat shares the slot of the word at src: a probe at `probe` for that
    word finds src (every position below the probe is entered, by a probe or by a plain store)"""
    s = slot(flat[src:src + 4])
    return all(slot(flat[q:q + 4]) != s for q in range(src + 1, probe) if q + 4 <= len(flat))


def stored_block(data: bytes) -> bytes:
    """one non-final stored block holding data (nothing for no data)"""
    assert len(data) <= 65535
    if not data:
        return b""
    return b"\x00" + len(data).to_bytes(2, "little") + (len(data) ^ 0xFFFF).to_bytes(2, "little") + data


def chunk_tokens(prefix: bytes, out: bytes):
    """the tokens of a chunk's output, in order (a stored block's bytes as literals)"""
    blocks = read_blocks(stored_block(prefix) + out + b"\x03\x00")
    toks = []
    for blk in blocks[1 if prefix else 0:]:
        if blk.btype == 0:
            toks += [("lit", b) for b in blk.payload]
        else:
            toks += blk.tokens
    return toks


def inflate_with(prefix: bytes, out: bytes) -> bytes:
    """zlib's reading of a chunk's output with the prefix as preset dictionary"""
    d = zlib.decompressobj(-15, zdict=prefix) if prefix else zlib.decompressobj(-15)
    got = d.decompress(out)
    assert d.unused_data == b"" and d.eof is False
    return got


def slot_clean(n: int, seed: int, wrap: int = 3) -> bytes:
    """n bytes whose 4-byte words (those that wrap into the first `wrap` bytes included: a copy of the bytes
    may follow them) all lie in different slots"""
    rng = random.Random(seed)
    while True:
        d = bytearray(rng.randbytes(4))
        used = {slot(d)}
        while len(d) < n:
            for _ in range(64):
                b = rng.randrange(256)
                s = slot(bytes(d[-3:]) + bytes([b]))
                if s not in used:
                    used.add(s)
                    d.append(b)
                    break
            else:
                break
        if len(d) < n:
            continue
        tail = [slot((bytes(d) + bytes(d[:wrap]))[q:q + 4]) for q in range(n - 3, n - 3 + wrap)]
        if len(set(tail)) == wrap and not used & set(tail):
            return bytes(d)


def run_then_zeros(run: bytes, n: int) -> bytes:
    """a prefix that is one distinctive run followed by zero filler"""
    return run + bytes(n - len(run))


RUN = bytes(range(0x41, 0x41 + 40))  # 40 different bytes: no word of it repeats


def reach_cases() -> dict:
    """name -> (prefix, chunk, expectation).  Expectations: ("first", token) the chunk's first token;
    ("literals", a, b) chunk bytes [a, b) are all literal tokens and no distance exceeds 32768;
    ("matches_only",) no literal token at all."""
    period = b"abcdefgh"
    clean = slot_clean(1024, 77)
    return {
        "dist32768": (run_then_zeros(RUN, MAX_DIST), RUN + b"\xff" * 8, ("first", ("match", len(RUN), MAX_DIST))),
        "dist32769": (run_then_zeros(RUN, MAX_DIST), b"\xfe" + RUN + b"\xff" * 8, ("literals", 0, 1 + len(RUN))),
        "boundary": (period * 8, (period * 40)[:300], ("first", ("match", 258, 8))),
        "dist1": (b"bcda", b"a" * 300, ("first", ("match", 258, 1))),
        "dist1_len1": (b"a", b"a" * 300, ("first", ("match", 258, 1))),
        "copy": (clean, clean, ("matches_only",)),
    }


def reach_sources() -> dict:
    """name -> (flat bytes, source position, probe position) the case relies on"""
    c = reach_cases()
    out = {}
    for name, src in (("dist32768", 0), ("boundary", 56), ("dist1", 3), ("dist1_len1", 0)):
        prefix, chunk, _ = c[name]
        out[name] = (prefix + chunk, src, len(prefix))
    return out


def mixed_chunks(seed: int = 11, n: int = 32):
    """chunks of text, zeros, random bytes and short alphabets, 0..65536 bytes, for the parity check"""
    rng = random.Random(seed)
    kinds = [lambda k: text(rng, k), lambda k: bytes(k), lambda k: rng.randbytes(k),
             lambda k: bytes(rng.choice(b"ab") for _ in range(k))]
    lens = [0, 1, 3, 4, 5, 259, 4096, 65535, 65536]
    return [kinds[i % 4](lens[i % len(lens)] if i < 2 * len(lens) else rng.randrange(0, 3000)) for i in range(n)]


def round_trip_cases():
    """(prefix, chunk) for every prefix length x chunk length x content"""
    rng = random.Random(1951)
    contents = {"text": lambda k: text(rng, k), "zero": lambda k: bytes(k), "random": lambda k: rng.randbytes(k)}
    cases = []
    for p in PREFIX_LENS:
        for c in CHUNK_LENS + [MAX_CHUNK - p]:
            for name, f in contents.items():
                whole = f(p + c)
                cases.append((whole[:p], whole[p:]))
    return cases


def fuzz_cases(n: int = 200, seed: int = 20261020):
    """chunks with a random prefix that shares substrings with the chunk"""
    rng = random.Random(seed)
    cases = []
    for _ in range(n):
        p = rng.choice([1, 2, 3, 4, 7, 64, 700, 5000, 20000])
        prefix = text(rng, p) if rng.random() < 0.5 else bytes(rng.choice(b"abcd") for _ in range(p))
        chunk = bytearray()
        for k in range(rng.randrange(1, 12)):
            if k == 0 or rng.random() < 0.6:  # (the first piece always comes from the prefix)
                a = rng.randrange(max(1, len(prefix) - 3))
                chunk += prefix[a:a + rng.randrange(4, 300)]
            else:
                chunk += rng.randbytes(rng.randrange(0, 40))
        cases.append((prefix, bytes(chunk) or b"x"))
    return cases


def repeated_stream():
    """a text whose second half repeats its first (32 KiB each), to be cut into 32 KiB chunks that take what
    precedes them (at most 32 KiB) as prefix"""
    x = text(random.Random(3), 32768)
    return x * 2


def stream_chunks(stream: bytes, cut: int = 32768):
    """(in_off, length, prefix_len) of the stream's chunks"""
    return [(o, min(cut, len(stream) - o), min(MAX_DIST, o)) for o in range(0, len(stream), cut)]


# ------------------------------------------------------------------------------ dictionaries
def dictionary(n: int, seed: int = 5) -> bytes:
    return text(random.Random(seed + n), n)


def far_dictionary() -> tuple:
    """a 40000-byte dictionary whose only text is its first 7 KiB (out of the window's reach: 40000 - 32768 =
    7232), the rest random bytes; and a message drawn from that text"""
    rng = random.Random(40000)
    head = text(rng, 7168)
    return head + rng.randbytes(40000 - len(head)), head[100:2100]


def zlib_header(level: int, d: bytes) -> bytes:
    """the bytes zlib's deflate() writes before the first block for this level and dictionary"""
    z = zlib.compressobj(level, zdict=d) if d is not None else zlib.compressobj(level)
    out = z.compress(b"x") + z.flush(zlib.Z_SYNC_FLUSH)
    return out[:6 if d else 2]
