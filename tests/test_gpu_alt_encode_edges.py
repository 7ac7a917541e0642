"""The LZ encoder kernels (FastLZ level 1/2, LZF, LZ4 fast, Snappy) on the edge-directed inputs of
tests/lz_inputs.py, bit-exact against the oracle: every chunk has status 0 and the oracle's bytes, at
every input / output alignment, in both launch forms (one chunk per wave up to 16 384 chunks, one per
lane above; Snappy through all of its forms), and with hash tables that hold another chunk's entries:
planter / victim pairs (lz_inputs.plant_pair) in consecutive calls of the same geometry and in the
consecutive chunks of one lane.  tests/test_lz_inputs.py shows on the CPU that each family reaches
the path it names and that the oracle equals its pins there; Adler32 is compared with zlib.adler32
at the slot, block and alignment edges of k_adler32.

Not covered: the wrap of the encoders' 16-bit stamp counter (ws_lane_launch zeroes the tables before
a stamp would reach 65 535).  Reaching it takes some 65 534 calls per codec, about 15 s each on an
MI355X as the deflate encoder's wrap test measured, which is too much for this suite."""
import random
import zlib

import pytest

import lz_inputs

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ALT = ("fastlz1", "fastlz2", "lzf", "lz4")  # the lane-per-chunk encoders (workspace.hpp ws_lane_launch)
LANE_FORM_N = 16385                         # above nx_common.hpp kSpreadMaxChunks: one chunk per lane
SPREAD_MAX_N = 16384                        # the largest batch that runs one chunk per wave


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def B():
    from netty_amd import batch
    return batch


class Want:
    """the oracle's bytes per (codec, chunk, u16_limit), computed once per module"""

    def __init__(self, oracle):
        self.oracle, self.memo = oracle, {}

    def __call__(self, codec, data, lim=None):
        key = (codec, data, lim)
        if key not in self.memo:
            o = self.oracle
            if codec.startswith("fastlz"):
                self.memo[key] = o.fastlz_compress(data, int(codec[-1]), u16_limit=len(data) if lim is None else lim)
            else:
                self.memo[key] = {"lzf": o.lzf_encode_chunk, "lz4": o.lz4_compress, "snappy": o.snappy_encode}[codec](data)
        return self.memo[key]


@pytest.fixture(scope="module")
def want(oracle):
    return Want(oracle)


@pytest.fixture(scope="module")
def families():
    """codec -> (chunks, u16 limits or None): every family's chunks, built once.  FastLZ takes each
    chunk with u16_limit = its length and again with each of the readU16 quirk's other limits."""
    res = {}
    for codec in lz_inputs.CODECS:
        cases = lz_inputs.all_cases(codec)
        chunks, lims = [c.data for _, c in cases], None
        if codec.startswith("fastlz"):
            lims = [len(c) for c in chunks]
            for _, case in cases:
                for lim in lz_inputs.fastlz_limits(len(case.data))[1:]:
                    chunks.append(case.data)
                    lims.append(lim)
        res[codec] = (chunks, lims)
    return res


@pytest.fixture(scope="module")
def fillers():
    return [lz_inputs.filler(i) for i in range(LANE_FORM_N)]


@pytest.fixture(scope="module")
def pairs():
    return [lz_inputs.plant_pair(i) for i in range(LANE_FORM_N)]


def _capacity(B, codec, n):
    if codec.startswith("fastlz"):
        return B.fastlz_max_compressed_length(n)
    return {"lzf": B.lzf_max_compressed_length, "lz4": B.lz4_max_compressed_length,
            "snappy": lambda n: B.snappy_max_compressed_length(n) + 1}[codec](n)


def encode(B, dev, codec, chunks, lims=None, in_align=16, out_align=16):
    """one batch call; returns the output bytes per chunk (status 0 asserted for every chunk)"""
    inp, off, ln = B.pack(chunks, dev, align=in_align)
    out, ooff = B.out_slots([_capacity(B, codec, len(c)) for c in chunks], dev, align=out_align)
    if codec.startswith("fastlz"):
        lv = torch.full((len(chunks),), int(codec[-1]), dtype=torch.int32, device=dev)
        lim = torch.tensor([len(c) for c in chunks] if lims is None else lims, dtype=torch.int32, device=dev)
        olen, st = B.fastlz_compress(inp, off, ln, out, ooff, level=lv, u16_limit=lim)
    else:
        olen, st = {"lzf": B.lzf_encode, "lz4": B.lz4_encode, "snappy": B.snappy_encode}[codec](inp, off, ln, out, ooff)
    torch.cuda.synchronize()
    assert int((st != 0).sum()) == 0, codec
    h, oo, ol = out.cpu().numpy().tobytes(), ooff.cpu().tolist(), olen.cpu().tolist()
    return [h[o:o + n] for o, n in zip(oo, ol)]


def check(got, want, codec, chunks, lims, idx):
    for i in idx:
        lim = None if lims is None else lims[i]
        assert got[i] == want(codec, chunks[i], lim), (codec, i, len(chunks[i]), lim)


@pytest.mark.parametrize("in_align,out_align", [(16, 16), (16, 4), (16, 1), (1, 16), (1, 4), (1, 1)])
@pytest.mark.parametrize("codec", lz_inputs.CODECS)
def test_edge_families(dev, B, want, families, codec, in_align, out_align):
    """All families of a codec in one batch, at chunk starts aligned to 16 bytes and packed, and
    output slots aligned to 16, 4 and 1."""
    chunks, lims = families[codec]
    got = encode(B, dev, codec, chunks, lims, in_align, out_align)
    check(got, want, codec, chunks, lims, range(len(chunks)))


def _scattered(chunks, lims, fillers, n, seed):
    """a batch of n: the family chunks (a seeded sample when n is smaller) at seeded positions among
    distinct fillers; returns (batch, limits, family positions, 64 sampled filler positions)"""
    rng = random.Random(seed)
    take = list(range(len(chunks))) if len(chunks) <= n else sorted(rng.sample(range(len(chunks)), n))
    pos = sorted(rng.sample(range(n), len(take)))
    batch = list(fillers[:n])
    bl = [len(c) for c in batch]
    for p, k in zip(pos, take):
        batch[p] = chunks[k]
        bl[p] = len(chunks[k]) if lims is None else lims[k]
    rest = sorted(set(range(n)) - set(pos))
    return batch, (None if lims is None else bl), pos, rng.sample(rest, min(64, len(rest)))


@pytest.mark.parametrize("codec", ALT)
def test_edge_families_lane_form(dev, B, want, families, fillers, codec):
    """The same chunks scattered through a batch of 16 385, which runs one chunk per lane: every
    family chunk and 64 of the (distinct, compressible) fillers around them."""
    chunks, lims = families[codec]
    batch, bl, pos, sample = _scattered(chunks, lims, fillers, LANE_FORM_N, 7)
    got = encode(B, dev, codec, batch, bl, in_align=1, out_align=1)
    check(got, want, codec, batch, bl, pos + sample)


@pytest.mark.parametrize("n", [1, 7, 256, 257, 4097, 16384, 16385])
def test_snappy_edge_families_every_form(dev, B, want, families, fillers, n):
    """Snappy's families through the batch sizes of test_gpu_snappy.py::
    test_snappy_encode_batch_size_forms (the LDS form, the wave-per-chunk form, the dense form)."""
    chunks, _ = families["snappy"]
    batch, _, pos, sample = _scattered(chunks, None, fillers, n, n)
    got = encode(B, dev, "snappy", batch, None, in_align=1, out_align=1)
    check(got, want, "snappy", batch, None, pos + sample)


@pytest.mark.parametrize("n", [1, 64, LANE_FORM_N])
@pytest.mark.parametrize("codec", ALT)
def test_tables_isolated_across_calls(dev, B, want, pairs, codec, n):
    """One call encodes n planters, the next call of the same n (the same launch geometry: lane t
    meets the table planter t left) their victims, a third the planters again: every chunk of the
    second and third call equals the oracle's."""
    planters, victims = [p for p, _ in pairs[:n]], [v for _, v in pairs[:n]]
    encode(B, dev, codec, planters)
    got = encode(B, dev, codec, victims)
    check(got, want, codec, victims, None, range(n))
    got = encode(B, dev, codec, planters)
    check(got, want, codec, planters, None, range(n))


@pytest.mark.parametrize("codec", ALT)
def test_tables_isolated_within_a_call(dev, B, want, pairs, fillers, codec):
    """A table that serves two chunks of one launch.  Up to 16 384 chunks run one per wave on
    min(n, CUs * waves per CU) waves (workspace.hip ws_want / ws_grid), wave t taking chunks t,
    t + waves, ...  Waves per CU is a build option (workspace.hpp kWsSpec), so the test does not
    assume it: in one batch of 16 384 it places, for EVERY value w at which a wave takes two chunks
    (CUs * w <= 8192), eight planters at positions i and their victims at i + CUs * w, among distinct
    fillers.  Whatever w the library was built with, eight waves meet a planter and then its victim;
    the second batch swaps the two.  With more than 8192 waves no wave takes two chunks in this form,
    and the lane form reuses a table only above CUs * waves * 64 chunks (262 144 by default), beyond
    what a test here should launch: there the consecutive calls of test_tables_isolated_across_calls
    stand in."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    ws = range(1, SPREAD_MAX_N // (2 * cus) + 1)
    assert len(ws) >= 1 and 8 * len(ws) <= cus
    first, second = {}, {}
    for k, w in enumerate(ws):
        for j in range(8):
            i, (planter, victim) = 8 * k + j, pairs[8 * k + j]
            first[i], first[i + cus * w] = planter, victim
            second[i], second[i + cus * w] = victim, planter
    assert len(first) == 16 * len(ws)  # no two pairs share a position
    for placed in (first, second):
        batch = [placed.get(i, fillers[i]) for i in range(SPREAD_MAX_N)]
        got = encode(B, dev, codec, batch, None, in_align=1, out_align=1)
        check(got, want, codec, batch, None, sorted(placed) + list(range(3, SPREAD_MAX_N, 257)))


def test_adler32_slot_block_and_alignment_edges(dev, B):
    """k_adler32 reads 1 KiB blocks of 16-byte lane slots, realigning a misaligned chunk over five
    dwords, and ends with a byte tail: lengths 0..40, around the 1 KiB block edge, around 2 KiB and
    65 535, of random bytes, zeros and 0xFF (the largest sums), at every start address mod 16; the last
    chunk ends at the last byte of the buffer."""
    rng = random.Random(23)
    lengths = list(range(0, 41)) + list(range(1008, 1041)) + [2047, 2048, 2049, 65535]
    buf, offs, lens, wants = bytearray(), [], [], []
    for n in lengths:
        for data in (rng.randbytes(n), bytes(n), b"\xff" * n):
            w = zlib.adler32(data)
            for s in range(16):
                pos = (len(buf) + 15) // 16 * 16 + s
                buf.extend(bytes(pos - len(buf)))
                offs.append(pos)
                lens.append(n)
                wants.append(w)
                buf.extend(data)
    assert offs[-1] + lens[-1] == len(buf) and lens[-1] == 65535 and offs[-1] % 16 == 15
    inp = torch.frombuffer(buf, dtype=torch.uint8).to(dev)
    off = torch.tensor(offs, dtype=torch.int64, device=dev)
    ln = torch.tensor(lens, dtype=torch.int32, device=dev)
    got = [x & 0xFFFFFFFF for x in B.adler32(inp, off, ln).cpu().tolist()]
    bad = [(lens[i], offs[i] % 16) for i in range(len(got)) if got[i] != wants[i]]
    assert not bad, bad[:10]
