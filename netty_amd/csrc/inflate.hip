// inflate.hip — RFC 1951 inflater over a batch of independent streams, resumable at symbol
// granularity (nx_inflate_batch; replaces Inflater.inflate as JdkZlibDecoder.java:254-296 calls it).
//
// One wave per stream (a block is one wave).  The serial chain is the symbol decode, kept
// wave-uniform: the 32 stream bits at the read position come out of a 256-byte input window the
// wave holds in registers (lane i = dword i, two v_readlane), the canonical Huffman decode has
// lane l test code length l + 1 (first code / count / symbol offset of that length live in lane l's
// registers) and a ballot pick the shortest hit, and the symbol is one LDS read.  The block's code
// is built by the whole wave: count per length (LDS atomics), first code per length, then the
// symbol array by ballot ranks.  Bytes are written by the whole wave: literals collect in a
// register (lane k = the k-th pending literal) and leave as one store of up to 64 bytes; a match
// is copied 64 bytes per step, an overlapping one (distance < length) by reading source byte
// k mod distance, so every source byte lies before the match.  A 4 KiB LDS ring mirrors the bytes
// this call produced and serves copies that reach at most kRingReach back; older sources (the
// caller's history, earlier output of this call) are read from HBM after the wave's own stores
// have been waited for (s_waitcnt vmcnt(0)), with loads that bypass the vector L1: the discipline
// of the Snappy expander's far copies.
//
// Nothing is assumed about the input: every loop is bounded by in_len, out_cap or a format
// constant (NX_ERR_INTERNAL is the guard), bits past in_len read as zero and are never loaded, a
// symbol is taken only when all its bits are present and its output fits, and no store leaves
// [hist_len, hist_len + out_cap) of the stream's window.  zlib's inflate() is followed error site
// by error site, in its order of checks (inflate.c, inftrees.c of zlib 1.2.11).
#include <hip/hip_runtime.h>
#include "../../include/netty_amd.h"
#include "nx_common.hpp"

namespace nx {
namespace inflate {

constexpr uint32_t kRing = 4096;
constexpr uint32_t kRingReach = kRing - 320;  // a match writes up to 258 bytes ahead of its source window
constexpr uint32_t kMaxIn = 1u << 27;         // input bytes one call looks at (bit positions and the guard stay in 32 bits)
constexpr uint32_t kMaxOut = 1u << 30;        // output bytes one call writes
constexpr uint32_t kMaxHist = 32768;

enum Phase : uint32_t { kHeader = 0, kStored = 1, kHuff = 2, kDone = 3, kFailed = 4 };

// NX_INFLATE_STATE_BYTES per stream; all zero = the start of a raw deflate stream
struct State {
    uint32_t phase;
    uint32_t bfinal;
    uint32_t bitoff;       // 0..7 into the first unconsumed byte
    uint32_t stored_left;  // kStored: bytes of the stored block still to copy
    uint32_t nlen, ndist;  // kHuff: symbols of the block's two codes
    uint32_t btype;        // kHuff: 1 fixed, 2 dynamic
    int32_t err;           // kFailed: the status every later call returns
    uint64_t total_out;
    uint32_t pad0[6];
    uint8_t lens[320];     // kHuff, dynamic: the code lengths (literal/length, then distance)
    uint8_t pad1[128];
};
static_assert(sizeof(State) == NX_INFLATE_STATE_BYTES, "state layout");

struct WaveLds {
    uint8_t ring[kRing];
    uint8_t lens[320];
    uint32_t cnt[16];
    uint16_t symL[288];
    uint16_t symD[32];
    uint16_t symC[20];
};

// A canonical code: lane l holds, for code length l + 1, the first code, the number of codes and
// the position of its first symbol in the symbol array (lanes 15.. hold an empty length).
struct Code {
    uint32_t first, count, offs;
};

__device__ const uint8_t kClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint32_t rdlane(uint32_t v, uint32_t l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)l); }
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The compressed input: a window of 64 dwords in registers, bits past `ilen` bytes are zero.
struct Bits {
    const uint8_t* src;
    uint32_t ilen;
    uint32_t w;    // this lane's dword of the window
    uint32_t wdw;  // the window's first dword
    int lane;
    __device__ __forceinline__ void load(uint32_t dw) {
        wdw = dw;
        const uint32_t b = (dw + (uint32_t)lane) * 4u;
        uint32_t v = 0;
        if (b + 4u <= ilen) {
            __builtin_memcpy(&v, src + b, 4);
        } else {
            for (uint32_t i = 0; i < 4u; ++i)
                if (b + i < ilen) v |= (uint32_t)src[b + i] << (8u * i);
        }
        w = v;
    }
    // the 32 bits from bit position p on (p <= 8 * ilen)
    __device__ __forceinline__ uint32_t peek(uint32_t p) {
        const uint32_t dw = p >> 5;
        if (dw < wdw || dw - wdw > 62u) load(dw);
        const uint32_t j = dw - wdw;
        const uint64_t v = ((uint64_t)rdlane(w, j + 1u) << 32) | rdlane(w, j);
        return (uint32_t)(v >> (p & 31u));
    }
};

// Build the canonical code of lens[0, nsym) (values 0..15) into `c` and `sym`.  *over = the lengths
// over-subscribe the code space, *left = unused code space (incomplete when > 0), *mx = longest length.
__device__ void build_code(WaveLds& L, const uint8_t* lens, uint32_t nsym, uint16_t* sym, Code& c, int lane, bool* over,
                           int32_t* left, uint32_t* mx) {
    wave_sync();
    if (lane < 16) L.cnt[lane] = 0;
    wave_sync();
    for (uint32_t s = (uint32_t)lane; s < nsym; s += 64u) atomicAdd(&L.cnt[lens[s] & 15u], 1u);
    wave_sync();
    uint32_t code = 0, acc = 0, prev = 0, m = 0;
    int32_t lf = 1;
    bool ov = false;
    c.first = c.count = c.offs = 0;
    for (uint32_t j = 1; j <= 15u; ++j) {
        const uint32_t nj = uni(L.cnt[j]);
        code = (code + prev) << 1;
        if ((uint32_t)lane + 1u == j) {
            c.first = code;
            c.count = nj;
            c.offs = acc;
        }
        acc += nj;
        prev = nj;
        if (!ov) {
            lf = (lf << 1) - (int32_t)nj;
            if (lf < 0) ov = true;
        }
        if (nj) m = j;
    }
    *over = ov;
    *left = lf;
    *mx = m;
    if (ov) return;
    uint32_t run = c.offs;  // lane j - 1: the next symbol slot of length j
    for (uint32_t base = 0; base < nsym; base += 64u) {
        const uint32_t s = base + (uint32_t)lane;
        const uint32_t l = s < nsym ? (lens[s] & 15u) : 0u;
        for (uint32_t j = 1; j <= m; ++j) {
            const uint64_t mask = __ballot(l == j);
            if (mask == 0) continue;
            const uint32_t start = rdlane(run, j - 1u);
            if (l == j) sym[start + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = (uint16_t)s;
            if ((uint32_t)lane + 1u == j) run += (uint32_t)__popcll(mask);
        }
    }
    wave_sync();
}

// One symbol of code `c` from the 32 stream bits `bits` (first bit = bit 0): the symbol and its
// length, or -1 when no code of up to 15 bits matches (possible only in an incomplete code).
__device__ __forceinline__ int32_t decode_sym(const Code& c, const uint16_t* sym, uint32_t bits, int lane, uint32_t* len) {
    const uint32_t rev = __brev(bits);
    const uint32_t code = lane < 15 ? rev >> (31 - lane) : 0u;
    const uint32_t idx = code - c.first;
    const uint64_t m = __ballot(idx < c.count);
    if (m == 0) return -1;
    const uint32_t l = (uint32_t)__ffsll((unsigned long long)m) - 1u;
    *len = l + 1u;
    return (int32_t)uni(sym[rdlane(c.offs + idx, l)]);
}

__device__ __forceinline__ void fixed_lens(WaveLds& L, int lane) {
    for (uint32_t s = (uint32_t)lane; s < 320u; s += 64u)
        L.lens[s] = (uint8_t)(s < 144u ? 8u : s < 256u ? 9u : s < 280u ? 7u : s < 288u ? 8u : 5u);
}

__device__ void inflate_stream(WaveLds& L, const uint8_t* __restrict__ src, uint32_t in_len, uint8_t* win, uint32_t hist,
                               uint32_t out_cap, State* S, uint32_t* consumed, uint32_t* out_len, int32_t* status, int lane) {
    uint32_t phase = uni(S->phase);
    auto leave = [&](int32_t st) {
        if (lane == 0) {
            *consumed = 0;
            *out_len = 0;
            *status = st;
        }
    };
    if (phase == kDone) return leave(NX_OK);
    if (phase == kFailed) return leave((int32_t)uni((uint32_t)S->err));
    if (phase > kFailed || hist > kMaxHist) return leave(NX_ERR_INVALID_ARG);
    if (in_len == 0u) return leave(NX_INFLATE_NEED_INPUT);  // (the saved bit offset has no byte to point into)

    Bits B{src, in_len < kMaxIn ? in_len : kMaxIn, 0u, 0u, lane};
    const uint32_t nbits = B.ilen * 8u;
    B.load(0);
    uint32_t p = uni(S->bitoff) & 7u;
    uint32_t bfinal = uni(S->bfinal) & 1u, stored_left = uni(S->stored_left) & 0xffffu;
    uint32_t nlen = uni(S->nlen), ndist = uni(S->ndist), btype = uni(S->btype);
    uint32_t pos = hist;  // window position after the last byte produced (pending literals included)
    const uint32_t end = hist + (out_cap < kMaxOut ? out_cap : kMaxOut);
    uint32_t ring_lo = hist;  // the ring holds window bytes [max(ring_lo, pos - kRing), pos)
    uint32_t npend = 0, pend = 0;
    Code CL{0, 0, 0}, CD{0, 0, 0};
    bool over;
    int32_t left;
    uint32_t mx;

    if (phase == kHuff) {  // the block's codes again, from the saved lengths
        if (btype == 1u) {
            fixed_lens(L, lane);
            nlen = 288u;
            ndist = 32u;
        } else {
            if (btype != 2u || nlen > 286u || ndist > 30u) return leave(NX_ERR_INVALID_ARG);
            for (uint32_t s = (uint32_t)lane; s < nlen + ndist; s += 64u) L.lens[s] = S->lens[s];
        }
        build_code(L, L.lens, nlen, L.symL, CL, lane, &over, &left, &mx);
        if (over) return leave(NX_ERR_INVALID_ARG);
        build_code(L, L.lens + nlen, ndist, L.symD, CD, lane, &over, &left, &mx);
        if (over) return leave(NX_ERR_INVALID_ARG);
    }

    auto flush_lits = [&]() {
        if (npend) {
            const uint32_t at = pos - npend + (uint32_t)lane;
            if ((uint32_t)lane < npend) {
                win[at] = (uint8_t)pend;
                L.ring[at & (kRing - 1u)] = (uint8_t)pend;
            }
            npend = 0;
        }
    };

    int32_t st = NX_ERR_INTERNAL;
    // every pass consumes at least one bit or ends the call, but for a stored block's body after its header
    uint32_t guard = 16u * B.ilen + 16u;
    for (;;) {
        if (guard-- == 0u) break;
        if (phase == kHeader) {
            if (nbits - p < 3u) { st = NX_INFLATE_NEED_INPUT; break; }
            const uint32_t h = B.peek(p);
            const uint32_t bf = h & 1u, type = (h >> 1) & 3u;
            if (type == 3u) { st = NX_ERR_INFLATE_BLOCK_TYPE; break; }
            if (type == 0u) {
                const uint32_t q = (p + 3u + 7u) & ~7u;
                if (q + 32u > nbits) { st = NX_INFLATE_NEED_INPUT; break; }
                const uint32_t v = B.peek(q);
                if ((v & 0xffffu) != ((v >> 16) ^ 0xffffu)) { st = NX_ERR_INFLATE_STORED_LENGTHS; break; }
                bfinal = bf;
                stored_left = v & 0xffffu;
                p = q + 32u;
                phase = kStored;
                continue;
            }
            if (type == 1u) {
                wave_sync();
                fixed_lens(L, lane);
                nlen = 288u;
                ndist = 32u;
                build_code(L, L.lens, nlen, L.symL, CL, lane, &over, &left, &mx);
                build_code(L, L.lens + nlen, ndist, L.symD, CD, lane, &over, &left, &mx);
                bfinal = bf;
                btype = 1u;
                p += 3u;
                phase = kHuff;
                continue;
            }
            // a dynamic block's header: nothing is kept of it until all of it is present
            uint32_t q = p + 3u;
            if (q + 14u > nbits) { st = NX_INFLATE_NEED_INPUT; break; }
            uint32_t v = B.peek(q);
            const uint32_t nl = (v & 31u) + 257u, nd = ((v >> 5) & 31u) + 1u, nc = ((v >> 10) & 15u) + 4u;
            q += 14u;
            if (nl > 286u || nd > 30u) { st = NX_ERR_INFLATE_TOO_MANY_SYMBOLS; break; }
            if (q + 3u * nc > nbits) { st = NX_INFLATE_NEED_INPUT; break; }
            {
                const uint64_t v64 = ((uint64_t)B.peek(q + 32u) << 32) | B.peek(q);
                wave_sync();
                if (lane < 19) L.lens[lane] = 0;
                wave_sync();
                if ((uint32_t)lane < nc) L.lens[kClOrder[lane]] = (uint8_t)((v64 >> (3u * (uint32_t)lane)) & 7u);
            }
            q += 3u * nc;
            Code CC{0, 0, 0};
            uint32_t cmx;
            build_code(L, L.lens, 19u, L.symC, CC, lane, &over, &left, &cmx);
            if (over || (left > 0 && cmx != 0u)) { st = NX_ERR_INFLATE_CODE_LENGTHS; break; }
            const uint32_t total = nl + nd;
            uint32_t have = 0, last = 0, dguard = total + 1u;
            int32_t hs = 0;
            while (have < total) {
                if (dguard-- == 0u) { hs = NX_ERR_INTERNAL; break; }
                if (q >= nbits) { hs = NX_INFLATE_NEED_INPUT; break; }
                v = B.peek(q);
                uint32_t cl = 1u;
                int32_t sym = 0;  // a code-length code with no codes reads every entry as one bit, length 0 (inftrees.c)
                if (cmx != 0u) sym = decode_sym(CC, L.symC, v, lane, &cl);
                if (sym < 0) { hs = NX_ERR_INTERNAL; break; }
                if (sym < 16) {
                    if (q + cl > nbits) { hs = NX_INFLATE_NEED_INPUT; break; }
                    if (lane == 0) L.lens[have] = (uint8_t)sym;
                    have += 1u;
                    last = (uint32_t)sym;
                    q += cl;
                    continue;
                }
                const uint32_t eb = sym == 16 ? 2u : sym == 17 ? 3u : 7u;
                if (q + cl + eb > nbits) { hs = NX_INFLATE_NEED_INPUT; break; }
                if (sym == 16 && have == 0u) { hs = NX_ERR_INFLATE_BIT_LENGTH_REPEAT; break; }
                const uint32_t rep = (sym == 18 ? 11u : 3u) + ((v >> cl) & ((1u << eb) - 1u));
                const uint32_t val = sym == 16 ? last : 0u;
                if (have + rep > total) { hs = NX_ERR_INFLATE_BIT_LENGTH_REPEAT; break; }
                for (uint32_t k = (uint32_t)lane; k < rep; k += 64u) L.lens[have + k] = (uint8_t)val;
                have += rep;
                last = val;
                q += cl + eb;
            }
            if (hs != 0) { st = hs; break; }
            wave_sync();
            if (uni(L.lens[256]) == 0u) { st = NX_ERR_INFLATE_MISSING_EOB; break; }
            build_code(L, L.lens, nl, L.symL, CL, lane, &over, &left, &mx);
            if (over || (left > 0 && mx != 1u)) { st = NX_ERR_INFLATE_LITLEN_SET; break; }
            build_code(L, L.lens + nl, nd, L.symD, CD, lane, &over, &left, &mx);
            if (over || (left > 0 && mx > 1u)) { st = NX_ERR_INFLATE_DIST_SET; break; }
            bfinal = bf;
            btype = 2u;
            nlen = nl;
            ndist = nd;
            p = q;
            phase = kHuff;
            continue;
        }
        if (phase == kStored) {
            if (stored_left == 0u) {
                if (bfinal) { phase = kDone; st = NX_OK; break; }
                phase = kHeader;
                continue;
            }
            const uint32_t bp = p >> 3, avail = B.ilen - bp, room = end - pos;
            if (avail == 0u) { st = NX_INFLATE_NEED_INPUT; break; }
            if (room == 0u) { st = NX_INFLATE_OUTPUT_FULL; break; }
            uint32_t nc = stored_left < avail ? stored_left : avail;
            nc = nc < room ? nc : room;
            flush_lits();
            for (uint32_t k = (uint32_t)lane; k < nc; k += 64u) win[pos + k] = src[bp + k];
            pos += nc;
            ring_lo = pos;  // stored bytes are not mirrored in the ring
            p += 8u * nc;
            stored_left -= nc;
            continue;
        }
        // kHuff: one symbol
        if (p >= nbits) { st = NX_INFLATE_NEED_INPUT; break; }
        const uint32_t v = B.peek(p);
        uint32_t l1 = 0;
        const int32_t sym = decode_sym(CL, L.symL, v, lane, &l1);
        if (sym < 0) { st = NX_ERR_INFLATE_LITLEN_CODE; break; }
        if (p + l1 > nbits) { st = NX_INFLATE_NEED_INPUT; break; }
        if (sym < 256) {
            if (pos >= end) { st = NX_INFLATE_OUTPUT_FULL; break; }
            if ((uint32_t)lane == npend) pend = (uint32_t)sym;
            npend += 1u;
            pos += 1u;
            p += l1;
            if (npend == 64u) flush_lits();
            continue;
        }
        if (sym == 256) {
            p += l1;
            if (bfinal) { phase = kDone; st = NX_OK; break; }
            phase = kHeader;
            continue;
        }
        if (sym >= 286) { st = NX_ERR_INFLATE_LITLEN_CODE; break; }
        const uint32_t li = (uint32_t)sym - 257u;
        const uint32_t lext = li < 8u || li == 28u ? 0u : (li >> 2) - 1u;
        const uint32_t lbase = li < 8u ? 3u + li : li == 28u ? 258u : 3u + ((4u + (li & 3u)) << lext);
        uint32_t q = p + l1 + lext;
        if (q >= nbits) { st = NX_INFLATE_NEED_INPUT; break; }  // the extra bits and a bit of the distance code
        const uint32_t len = lbase + ((v >> l1) & ((1u << lext) - 1u));
        const uint32_t v2 = B.peek(q);
        uint32_t l2 = 0;
        const int32_t dsym = decode_sym(CD, L.symD, v2, lane, &l2);
        if (dsym < 0) { st = NX_ERR_INFLATE_DIST_CODE; break; }
        if (q + l2 > nbits) { st = NX_INFLATE_NEED_INPUT; break; }
        if (dsym >= 30) { st = NX_ERR_INFLATE_DIST_CODE; break; }
        const uint32_t di = (uint32_t)dsym;
        const uint32_t dext = di < 4u ? 0u : (di >> 1) - 1u;
        const uint32_t dbase = di < 4u ? 1u + di : 1u + ((2u + (di & 1u)) << dext);
        if (q + l2 + dext > nbits) { st = NX_INFLATE_NEED_INPUT; break; }
        const uint32_t dist = dbase + ((v2 >> l2) & ((1u << dext) - 1u));
        q += l2 + dext;
        if (dist > pos) { st = NX_ERR_INFLATE_DISTANCE_TOO_FAR; break; }
        if (len > end - pos) { st = NX_INFLATE_OUTPUT_FULL; break; }
        flush_lits();
        const bool near = dist <= kRingReach && pos - dist >= ring_lo;
        if (near)
            wave_sync();
        else
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the wave's own earlier stores have landed
        const uint32_t s0 = pos - dist;
        for (uint32_t k0 = 0; k0 < len; k0 += 64u) {
            const uint32_t k = k0 + (uint32_t)lane;
            if (k < len) {
                const uint32_t sp = s0 + (dist < len ? k % dist : k);  // an overlapping copy repeats its first `dist` bytes
                const uint32_t b = near ? (uint32_t)L.ring[sp & (kRing - 1u)]
                                        : (uint32_t)__hip_atomic_load(win + sp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                win[pos + k] = (uint8_t)b;
                L.ring[(pos + k) & (kRing - 1u)] = (uint8_t)b;
            }
        }
        pos += len;
        p = q;
    }
    flush_lits();
    if (st == NX_OK) p = (p + 7u) & ~7u;  // the end of the stream: up to the next byte, as zlib leaves it
    wave_sync();
    if (phase == kHuff && btype == 2u && st >= 0)
        for (uint32_t s = (uint32_t)lane; s < nlen + ndist; s += 64u) S->lens[s] = L.lens[s];
    if (lane == 0) {
        S->phase = st < 0 ? (uint32_t)kFailed : phase;
        S->bfinal = bfinal;
        S->bitoff = st == NX_OK ? 0u : (p & 7u);
        S->stored_left = stored_left;
        S->nlen = nlen;
        S->ndist = ndist;
        S->btype = btype;
        S->err = st < 0 ? st : 0;
        S->total_out += (uint64_t)(pos - hist);
        *consumed = p >> 3;
        *out_len = pos - hist;
        *status = st;
    }
}

__global__ void __launch_bounds__(64) k_inflate(const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off,
                                                const uint32_t* __restrict__ in_len, uint8_t* out,
                                                const uint64_t* __restrict__ out_off, const uint32_t* __restrict__ hist_len,
                                                const uint32_t* __restrict__ out_cap, uint8_t* state, uint32_t* consumed,
                                                uint32_t* out_len, int32_t* status, uint32_t n) {
    __shared__ WaveLds L;
    const int lane = (int)threadIdx.x;
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        inflate_stream(L, in + in_off[i], uni(in_len[i]), out + out_off[i], uni(hist_len[i]), uni(out_cap[i]),
                       reinterpret_cast<State*>(state + (size_t)i * NX_INFLATE_STATE_BYTES), consumed + i, out_len + i,
                       status + i, lane);
        wave_sync();
    }
}

}  // namespace inflate
}  // namespace nx

extern "C" int32_t nx_inflate_batch(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint8_t* out,
                                    const uint64_t* out_off, const uint32_t* hist_len, const uint32_t* out_cap, uint8_t* state,
                                    uint32_t* consumed, uint32_t* out_len, int32_t* status, uint32_t n, void* stream) {
    if (n == 0) return NX_OK;
    if (!in || !in_off || !in_len || !out || !out_off || !hist_len || !out_cap || !state || !consumed || !out_len || !status)
        return NX_ERR_INVALID_ARG;
    NX_CLEAR_STALE_ERROR();
    const unsigned grid = n < (1u << 20) ? n : (1u << 20);
    hipLaunchKernelGGL(nx::inflate::k_inflate, dim3(grid), dim3(64), 0, (hipStream_t)stream, in, in_off, in_len, out, out_off,
                       hist_len, out_cap, state, consumed, out_len, status, n);
    NX_HIP_CHECK(hipGetLastError());
    return NX_OK;
}
