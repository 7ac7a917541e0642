"""The plain texts behind tests/golden/brotli_libbrotli_streams.json and the fixture's loader.

The fixture holds libbrotli's streams only; every plain text is regenerated here from (kind, size, seed), so
the tests compare a decode with bytes no decoder made.  tests/golden/make_brotli_libbrotli_streams.py writes the
fixture from the same CASES list.
"""
import base64
import json
import os
import random

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "brotli_libbrotli_streams.json")

_WORDS = (
    "the of and to in that is was for with as his on be at by this had not are but from or have an they which one you were her "
    "all she there would their we him been has when who will more no if out so said what up its about into than them can only "
    "other new some could time these two may then do first any my now such like our over man me even most made after also did "
    "many before must through years where much your way well down should because each just those people how too little state "
    "good very make world still own see men work long get here between both life being under never day same another know while "
    "last might us great old year off come since against go came right used take three government information international "
    "development university different national important children available following education including services although "
    "community something research president business possible together however children American company history general"
).split()


def text(n: int, seed: int) -> bytes:
    """English-like text: sentences of common words, which libbrotli finds in the static dictionary."""
    rng = random.Random(seed)
    out = []
    size = 0
    while size < n:
        k = rng.randint(4, 14)
        ws = [rng.choice(_WORDS) for _ in range(k)]
        ws[0] = ws[0].capitalize()
        s = " ".join(ws) + rng.choice([". ", ", ", ".\n", "? ", "; "])
        out.append(s)
        size += len(s)
    return "".join(out).encode()[:n]


def binary(n: int, seed: int) -> bytes:
    """Repetitive binary data: records with counters, a few repeating fields and some noise."""
    rng = random.Random(seed)
    out = bytearray()
    tags = [bytes(rng.randrange(256) for _ in range(rng.randint(3, 9))) for _ in range(6)]
    i = 0
    while len(out) < n:
        out += (i * 7).to_bytes(4, "little") + tags[i % 3] + bytes([0, 0, 0xFF, i & 0xFF])
        if rng.random() < 0.3:
            out += tags[3 + rng.randrange(3)] * rng.randint(1, 4)
        if rng.random() < 0.2:
            out += bytes(rng.randrange(256) for _ in range(rng.randint(1, 6)))
        i += 1
    return bytes(out[:n])


def noise(n: int, seed: int) -> bytes:
    rng = random.Random(seed)
    return bytes(rng.randrange(256) for _ in range(n))


def mixed(n: int, seed: int) -> bytes:
    """Text and binary stretches in turn, for a stream of several meta-blocks."""
    rng = random.Random(seed)
    out = bytearray()
    k = 0
    while len(out) < n:
        m = rng.randint(2000, 9000)
        out += text(m, seed * 100 + k) if k % 3 != 2 else binary(m, seed * 100 + k)
        k += 1
    return bytes(out[:n])


KINDS = {"text": text, "binary": binary, "noise": noise, "mixed": mixed}
MODES = {"GENERIC": 0, "TEXT": 1, "FONT": 2}


def plain(case: dict) -> bytes:
    return KINDS[case["kind"]](case["size"], case["seed"])


def _cases():
    cs = []
    lg_a, lg_b = (10, 16, 22, 24), (22, 24, 10, 16)
    md_a, md_b = ("GENERIC", "TEXT", "FONT"), ("FONT", "GENERIC", "TEXT")
    for q in range(12):
        cs.append(dict(kind="text", size=3000 + 17 * q, seed=100 + q, quality=q, lgwin=lg_a[q % 4], mode=md_a[q % 3]))
        cs.append(dict(kind="binary", size=4000 + 13 * q, seed=200 + q, quality=q, lgwin=lg_b[q % 4], mode=md_b[q % 3]))
    cs.append(dict(kind="noise", size=1500, seed=1, quality=5, lgwin=22, mode="GENERIC"))
    cs.append(dict(kind="noise", size=700, seed=2, quality=0, lgwin=16, mode="GENERIC"))
    cs.append(dict(kind="text", size=0, seed=0, quality=5, lgwin=22, mode="GENERIC"))
    cs.append(dict(kind="text", size=0, seed=0, quality=0, lgwin=10, mode="TEXT"))
    cs.append(dict(kind="text", size=1, seed=3, quality=11, lgwin=24, mode="TEXT"))
    cs.append(dict(kind="binary", size=1, seed=4, quality=1, lgwin=16, mode="FONT"))
    cs.append(dict(kind="mixed", size=70000, seed=5, quality=5, lgwin=16, mode="GENERIC"))
    cs.append(dict(kind="mixed", size=70001, seed=6, quality=10, lgwin=22, mode="FONT"))
    cs.append(dict(kind="text", size=3072, seed=7, quality=6, lgwin=10, mode="TEXT"))
    cs.append(dict(kind="text", size=3072, seed=8, quality=11, lgwin=10, mode="GENERIC"))
    cs.append(dict(kind="text", size=8192, seed=9, quality=9, lgwin=22, mode="TEXT"))
    cs.append(dict(kind="text", size=2500, seed=10, quality=4, lgwin=22, mode="TEXT", flush_at=1200))
    for i, c in enumerate(cs):
        c["name"] = "%02d-%s-%d-q%d-w%d-%s%s" % (i, c["kind"], c["size"], c["quality"], c["lgwin"], c["mode"].lower(),
                                                "-flush" if "flush_at" in c else "")
    return cs


CASES = _cases()


def load():
    """[(case, stream bytes)] of the committed fixture."""
    with open(GOLDEN) as f:
        doc = json.load(f)
    return [(c, base64.b64decode(c["stream"])) for c in doc["streams"]]
