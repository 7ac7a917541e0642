"""Parsers of the four LZ block formats the alt encoders and the Snappy encoder emit: each returns the
token list and the decoded bytes, and raises Malformed on anything the format does not allow.  Pure
Python, no oracle and no kernel: tests/test_lz_inputs.py reads from the tokens which path of an
encoder an input reached, and tests/test_gpu_alt_encode_edges.py names the chunk that differs.

Tokens are ("lit", n) and ("match", length, distance), with one more field where a format has forms:
FastLZ matches end with True for the level-2 far form, Snappy tokens with the tag kind ("lit0" ..
"lit4" by the count of extra length bytes, "copy1", "copy2", "copy4")."""
from streamgen import FASTLZ_FAR


class Malformed(ValueError):
    pass


def _need(cond, what):
    if not cond:
        raise Malformed(what)


def _copy(out, length, distance):
    _need(0 < distance <= len(out), f"distance {distance} at output {len(out)}")
    start = len(out) - distance
    for i in range(length):  # byte by byte: an overlapping copy repeats its period
        out.append(out[start + i])


def fastlz(block: bytes):
    """A FastLZ block (FastLz.java:409-543); returns (level, tokens, bytes).  The empty block is the
    empty input's."""
    if not block:
        return 1, [], b""
    level = (block[0] >> 5) + 1
    _need(level in (1, 2), f"level {level}")
    toks, out, ip, ctrl = [], bytearray(), 1, block[0] & 31
    while True:
        if ctrl >= 32:
            length, hi = (ctrl >> 5) - 1, ctrl & 31
            if length == 6:
                while True:
                    _need(ip < len(block), "length byte past the block")
                    c = block[ip]
                    ip += 1
                    length += c
                    if level == 1 or c != 255:
                        break
            _need(ip < len(block), "distance byte past the block")
            c = block[ip]
            ip += 1
            far = level == 2 and c == 255 and hi == 31
            if far:
                _need(ip + 2 <= len(block), "far distance past the block")
                dist = ((block[ip] << 8) | block[ip + 1]) + FASTLZ_FAR
                ip += 2
            else:
                dist = (hi << 8) | c
            _copy(out, length + 3, dist + 1)
            toks.append(("match", length + 3, dist + 1, far))
        else:
            n = ctrl + 1
            _need(ip + n <= len(block), "literal run past the block")
            out += block[ip:ip + n]
            ip += n
            toks.append(("lit", n))
        if ip >= len(block):
            break
        ctrl = block[ip]
        ip += 1
    return level, toks, bytes(out)


def lzf_body(body: bytes):
    """The body of a compressed LZF chunk (liblzf format); returns (tokens, bytes)."""
    toks, out, ip = [], bytearray(), 0
    while ip < len(body):
        ctrl = body[ip]
        ip += 1
        if ctrl < 32:
            n = ctrl + 1
            _need(ip + n <= len(body), "literal run past the body")
            out += body[ip:ip + n]
            ip += n
            toks.append(("lit", n))
            continue
        length = ctrl >> 5
        if length == 7:
            _need(ip < len(body), "length byte past the body")
            length += body[ip]
            ip += 1
        _need(ip < len(body), "offset byte past the body")
        dist = ((ctrl & 31) << 8) + body[ip] + 1
        ip += 1
        _copy(out, length + 2, dist)
        toks.append(("match", length + 2, dist))
    return toks, bytes(out)


def lzf_chunk(chunk: bytes):
    """One 'ZV' chunk; returns (type, tokens, bytes): type 0 is a raw chunk, one ("lit", n)."""
    _need(len(chunk) >= 5 and chunk[:2] == b"ZV" and chunk[2] in (0, 1), "chunk header")
    if chunk[2] == 0:
        n = int.from_bytes(chunk[3:5], "big")
        _need(len(chunk) == 5 + n, "raw chunk length")
        return 0, [("lit", n)] if n else [], chunk[5:]
    _need(len(chunk) >= 7, "chunk header")
    clen, ulen = int.from_bytes(chunk[3:5], "big"), int.from_bytes(chunk[5:7], "big")
    _need(len(chunk) == 7 + clen, "compressed chunk length")
    toks, out = lzf_body(chunk[7:])
    _need(len(out) == ulen, "decoded length")
    return 1, toks, out


def _lz4_len(block, ip, v):
    if v == 15:
        while True:
            _need(ip < len(block), "length byte past the block")
            c = block[ip]
            ip += 1
            v += c
            if c != 255:
                break
    return v, ip


def lz4(block: bytes):
    """An LZ4 block, with the end-of-block rules of the format (the last sequence is literals only,
    the last 5 bytes are literals, the last match starts 12 bytes or more before the end); returns
    (tokens, bytes).  A literal run of 0 is kept as ("lit", 0): it is a token of the format."""
    toks, out, ip = [], bytearray(), 0
    _need(len(block) > 0, "empty block")
    last_match_start = None
    while True:
        _need(ip < len(block), "token past the block")
        t = block[ip]
        ip += 1
        n, ip = _lz4_len(block, ip, t >> 4)
        _need(ip + n <= len(block), "literals past the block")
        out += block[ip:ip + n]
        ip += n
        toks.append(("lit", n))
        if ip == len(block):
            _need(t & 15 == 0, "match length in the last token")
            break
        _need(ip + 2 <= len(block), "offset past the block")
        dist = block[ip] | (block[ip + 1] << 8)
        ip += 2
        m, ip = _lz4_len(block, ip, t & 15)
        last_match_start = len(out)
        _copy(out, m + 4, dist)
        toks.append(("match", m + 4, dist))
    if last_match_start is not None:
        _need(toks[-1][1] >= 5, "fewer than 5 last literals")
        _need(len(out) - last_match_start >= 12, "a match within 12 bytes of the end")
    return toks, bytes(out)


def snappy(block: bytes):
    """A Snappy block (preamble and elements); returns (tokens, bytes)."""
    ip, want, shift = 0, 0, 0
    while True:
        _need(ip < len(block) and shift <= 28, "preamble")
        c = block[ip]
        ip += 1
        want |= (c & 0x7F) << shift
        shift += 7
        if not c & 0x80:
            break
    toks, out = [], bytearray()
    while ip < len(block):
        tag = block[ip]
        ip += 1
        kind = tag & 3
        if kind == 0:
            n, extra = (tag >> 2) + 1, 0
            if n > 60:
                extra = n - 60
                _need(ip + extra <= len(block), "literal length past the block")
                n = int.from_bytes(block[ip:ip + extra], "little") + 1
                ip += extra
            _need(ip + n <= len(block), "literal past the block")
            out += block[ip:ip + n]
            ip += n
            toks.append(("lit", n, f"lit{extra}"))
            continue
        if kind == 1:
            _need(ip < len(block), "offset past the block")
            length, dist, name = 4 + ((tag >> 2) & 7), ((tag >> 5) << 8) | block[ip], "copy1"
            ip += 1
        else:
            nb = 2 if kind == 2 else 4
            _need(ip + nb <= len(block), "offset past the block")
            length, dist, name = (tag >> 2) + 1, int.from_bytes(block[ip:ip + nb], "little"), f"copy{nb}"
            ip += nb
        _copy(out, length, dist)
        toks.append(("match", length, dist, name))
    _need(len(out) == want, f"decoded {len(out)}, preamble {want}")
    return toks, bytes(out)


def positions(toks):
    """the tokens with the output position each starts at: [(pos, token)]"""
    res, pos = [], 0
    for t in toks:
        res.append((pos, t))
        pos += t[1]
    return res
