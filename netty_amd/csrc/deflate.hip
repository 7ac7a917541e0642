// deflate.hip — RFC 1951 deflate encoder for JdkZlibEncoder (JdkZlibEncoder.java:214-276), two passes
// over independent chunks of up to 64 KiB.
//
// Every encode() of the reference ends in Z_SYNC_FLUSH, so a message's output is byte-aligned and
// ends in an empty stored block; a deflate stream may be built from pieces closed that way.  A chunk's
// output here is one such piece: one block (BFINAL = 0) in the cheapest of the three encodings by exact
// bit count (stored, fixed Huffman, dynamic Huffman), then the empty stored block 00 00 FF FF.
//
//   pass 1, k_deflate_match, one lane per chunk (the lane grid of the other alt encoders): greedy
//     single-probe LZ77, a stamped 64-bit hash entry carrying the position's 4 bytes, one exchange per
//     probed position, stamps instead of clearing.  It writes 16-bit tokens to the chunk's slot:
//       0x0000 | byte        a literal
//       0x0100 | (len - 3)   a match length 3..258, followed by
//       0x8000 | (dist - 1)  its distance 1..32768
//     so every token says what it is and pass 2 codes each one on its own lane.
//   pass 2, k_deflate_emit, one wave per chunk: histogram of the 286 + 30 symbols in LDS, the two
//     length-limited codes (sort by rank counting across the wave, two-queue Huffman merge, lengths
//     over 15 folded back by moving codes between lengths), the code-length code, the exact cost of
//     the three encodings, then the bits: each lane codes one token, a wave prefix sum over the bit
//     lengths gives its bit offset, and the words are ORed into an LDS ring that is stored to the
//     output in whole 128-byte units.
//
// Per chunk the workspace holds 128 KiB: 4096 hash entries (32 KiB) and 96 KiB of tokens.  A chunk
// that fills the token slot (49 148 tokens: at most a quarter of it can still follow, and it found
// few matches) has its remaining bytes coded as literals, which pass 2 reads from the input.
#include "nx_common.hpp"
#include "workspace.hpp"

namespace nx {
namespace deflate {

constexpr uint32_t kMaxChunk = 65536;
constexpr uint32_t kHashLog = 12;
constexpr uint32_t kSlotBytes = 128u << 10;
constexpr uint32_t kTokOff = (1u << kHashLog) * 8u;              // the token area follows the hash table
constexpr uint32_t kTokCap = (kSlotBytes - kTokOff - 8u) / 2u;   // after its two-word header {tokens, tail}
constexpr uint32_t kMaxMatch = 258, kMaxDist = 32768;
constexpr uint32_t kLit = 288, kDistBase = 288, kSyms = 320;     // symbol tables: 288 literal/length slots, then 32 distance slots

// ---------------------------------------------------------------------------------------- pass 1
//
// PREFIX: `in` is the chunk's history followed by the chunk, one flat range of n = pre + length bytes
// (at most 65536, so a position still fits the entry's 16 bits).  The pre history positions are entered
// first (plain stores in rising order: a slot keeps the nearest occurrence; the last three read their
// word across the boundary), then matching starts at pre.  Tokens and the literal tail are the chunk's
// own: a distance may reach into the history, nothing else refers to it.
template <bool PREFIX>
__device__ __forceinline__ void match_chunk(const uint8_t* __restrict__ in, uint32_t n, uint32_t pre, uint64_t* __restrict__ table,
                                            uint32_t* __restrict__ hdr, uint32_t stamp) {
    uint32_t* tok32 = hdr + 2;
    const uint32_t stag = stamp << 16;
    uint32_t nt = 0, pend = 0, ip = 0;
    if (PREFIX) {
        for (uint32_t q = 0; q < pre && q + 4u <= n; ++q) {
            const uint32_t wq = ld32(in + q);
            __hip_atomic_store(table + ((wq * 2654435761u) >> (32u - kHashLog)), ((uint64_t)(stag | q) << 32) | wq,
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        ip = pre;
    }
#define NX_PUT_TOKEN(t)                                      \
    do {                                                     \
        if (nt & 1u) tok32[nt >> 1] = pend | ((t) << 16);    \
        else pend = (t);                                     \
        ++nt;                                                \
    } while (0)
    while (ip + 4u <= n && nt + 2u <= kTokCap) {
        const uint32_t w = ld32(in + ip);
        const uint32_t h = (w * 2654435761u) >> (32u - kHashLog);
        const uint64_t e = __hip_atomic_exchange(table + h, ((uint64_t)(stag | ip) << 32) | w, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t hi = (uint32_t)(e >> 32), cand = hi & 0xFFFFu;
        if ((hi & 0xFFFF0000u) == stag && (uint32_t)e == w && ip - cand <= kMaxDist) {
            const uint32_t maxlen = n - ip < kMaxMatch ? n - ip : kMaxMatch;
            uint32_t len = 4;
            for (;;) {
                if (len + 4u > maxlen) {
                    while (len < maxlen && in[ip + len] == in[cand + len]) ++len;
                    break;
                }
                const uint32_t x = ld32(in + ip + len) ^ ld32(in + cand + len);
                if (x) {
                    len += (uint32_t)__builtin_ctz(x) >> 3;
                    break;
                }
                len += 4;
            }
            NX_PUT_TOKEN(0x100u | (len - 3u));
            NX_PUT_TOKEN(0x8000u | (ip - cand - 1u));
            // the positions inside the match are entered too (no probe: plain stores), so that a
            // later repeat of its inner bytes finds them
            const uint32_t end = ip + len;
            for (uint32_t q = ip + 1; q < end && q + 4u <= n; ++q) {
                const uint32_t wq = ld32(in + q);
                __hip_atomic_store(table + ((wq * 2654435761u) >> (32u - kHashLog)), ((uint64_t)(stag | q) << 32) | wq,
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            ip = end;
        } else {
            NX_PUT_TOKEN(w & 0xFFu);
            ++ip;
        }
    }
#undef NX_PUT_TOKEN
    if (nt & 1u) tok32[nt >> 1] = pend;
    hdr[0] = nt;
    hdr[1] = PREFIX ? ip - pre : ip;  // the chunk's bytes from here on are literals pass 2 reads from the input
}

template <bool SPREAD>
__global__ void __launch_bounds__(256) k_deflate_match(const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off,
                                                       const uint32_t* __restrict__ in_len, uint32_t n,
                                                       uint8_t* __restrict__ workspace, uint32_t stamp) {
    uint32_t tid, nthreads;
    if (!chunk_slot<SPREAD>(tid, nthreads)) return;
    if (tid >= n) return;  // one chunk per slot: its tokens stay there for pass 2
    const uint32_t len = in_len[tid];
    if (len == 0 || len > kMaxChunk) return;
    uint8_t* slot = workspace + (size_t)tid * kSlotBytes;
    match_chunk<false>(in + in_off[tid], len, 0u, reinterpret_cast<uint64_t*>(slot), reinterpret_cast<uint32_t*>(slot + kTokOff), stamp);
}

// A chunk's history must lie in the arena, fit the window and leave its positions 16 bits.
__device__ __forceinline__ bool prefix_ok(uint32_t pre, uint32_t len, uint64_t off) {
    return pre <= kMaxDist && pre + len <= kMaxChunk && pre <= off;
}

// The same with a history prefix per chunk: the prefix_len[i] bytes before in_off[i] (nx_deflate_encode_batch_ex).
template <bool SPREAD>
__global__ void __launch_bounds__(256) k_deflate_match_prefix(const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off,
                                                              const uint32_t* __restrict__ in_len,
                                                              const uint32_t* __restrict__ prefix_len, uint32_t n,
                                                              uint8_t* __restrict__ workspace, uint32_t stamp) {
    uint32_t tid, nthreads;
    if (!chunk_slot<SPREAD>(tid, nthreads)) return;
    if (tid >= n) return;
    const uint32_t len = in_len[tid], pre = prefix_len[tid];
    const uint64_t off = in_off[tid];
    if (len == 0 || len > kMaxChunk || !prefix_ok(pre, len, off)) return;
    uint8_t* slot = workspace + (size_t)tid * kSlotBytes;
    match_chunk<true>(in + (off - pre), pre + len, pre, reinterpret_cast<uint64_t*>(slot), reinterpret_cast<uint32_t*>(slot + kTokOff),
                      stamp);
}

// ---------------------------------------------------------------------------------------- pass 2
struct Lds {
    uint32_t freq[kSyms];   // literal/length 0..285 (286, 287 stay 0), distance at kDistBase
    uint32_t code[kSyms];   // bit-reversed code | bits << 16
    uint8_t lens[kSyms];
    uint32_t cl_freq[20], cl_code[20];
    uint8_t cl_lens[20];
    uint16_t order[kLit], parent[2 * kLit], dep[2 * kLit];  // tree building
    uint32_t nfreq[2 * kLit];
    uint32_t cnt[16], nxt[16];
    uint32_t acc[8];
    uint32_t ring[128];     // 512 bytes of output bits: four 128-byte units
};

__device__ const uint8_t kClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

__device__ __forceinline__ uint32_t len_code(uint32_t l) {  // l = length - 3 -> code index 0..28 (symbol 257 + code)
    if (l < 8u) return l;
    if (l == 255u) return 28u;
    const uint32_t k = 31u - (uint32_t)__builtin_clz(l);
    return 4u * (k - 1u) + ((l >> (k - 2u)) & 3u);
}
__device__ __forceinline__ uint32_t len_extra(uint32_t c) { return c < 8u || c == 28u ? 0u : (c >> 2) - 1u; }
__device__ __forceinline__ uint32_t dist_code(uint32_t d) {  // d = distance - 1 -> code 0..29
    if (d < 4u) return d;
    const uint32_t k = 31u - (uint32_t)__builtin_clz(d);
    return 2u * k + ((d >> (k - 1u)) & 1u);
}
__device__ __forceinline__ uint32_t dist_extra(uint32_t c) { return c < 4u ? 0u : (c >> 1) - 1u; }
__device__ __forceinline__ uint32_t fixed_len(uint32_t s) { return s < 144u ? 8u : s < 256u ? 9u : s < 280u ? 7u : 8u; }

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t x, uint32_t lane) {
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    return x;
}

// Code lengths of at most maxbits for the nsym frequencies (at least two symbols get a length, so the
// code is always complete).  All 64 lanes call it.
__device__ void build_lengths(Lds& L, const uint32_t* freq, uint32_t nsym, uint32_t maxbits, uint8_t* lens, uint32_t lane) {
    if (lane == 0) L.acc[0] = 0;
    __syncthreads();
    uint32_t mine = 0;
    for (uint32_t s = lane; s < nsym; s += 64u) {
        lens[s] = 0;
        mine += freq[s] != 0u;
    }
    if (mine) atomicAdd(&L.acc[0], mine);
    __syncthreads();
    uint32_t used = L.acc[0];
    uint32_t add0 = 0, add1 = 0;
    if (used < 2u && freq[0] == 0u) {
        add0 = 1;
        ++used;
    }
    if (used < 2u && freq[1] == 0u) {
        add1 = 1;
        ++used;
    }
    // ascending by (frequency, symbol): a symbol's rank is the number of used symbols before it
    for (uint32_t s = lane; s < nsym; s += 64u) {
        const uint32_t fs = freq[s] + (s == 0u ? add0 : s == 1u ? add1 : 0u);
        if (fs == 0u) continue;
        uint32_t r = 0;
        for (uint32_t t = 0; t < nsym; ++t) {
            const uint32_t ft = freq[t] + (t == 0u ? add0 : t == 1u ? add1 : 0u);
            r += (ft != 0u) & ((ft < fs) | ((ft == fs) & (t < s)));
        }
        L.order[r] = (uint16_t)s;
        L.nfreq[r] = fs;
    }
    __syncthreads();
    if (lane == 0) {
        // two-queue Huffman merge: leaves [0, used) ascending, internal nodes [used, 2 * used - 1) in
        // the order they are made (ascending too); a node's parent has a higher index
        const uint32_t total = 2u * used - 1u;
        uint32_t a = 0, b = used;
        for (uint32_t nn = used; nn < total; ++nn) {
            uint32_t p0, p1;
            if (a < used && (b >= nn || L.nfreq[a] <= L.nfreq[b])) p0 = a++;
            else p0 = b++;
            if (a < used && (b >= nn || L.nfreq[a] <= L.nfreq[b])) p1 = a++;
            else p1 = b++;
            L.nfreq[nn] = L.nfreq[p0] + L.nfreq[p1];
            L.parent[p0] = (uint16_t)nn;
            L.parent[p1] = (uint16_t)nn;
        }
        for (uint32_t i = 0; i < 16u; ++i) L.cnt[i] = 0;
        L.dep[total - 1u] = 0;
        for (uint32_t i = total - 1u; i-- > 0u;) {
            const uint32_t d = (uint32_t)L.dep[L.parent[i]] + 1u;
            L.dep[i] = (uint16_t)d;
            if (i < used) L.cnt[d < maxbits ? d : maxbits] += 1u;
        }
        // lengths over maxbits were folded into maxbits, which overfills the code space by `tot -
        // 2^maxbits` units: each round frees one by moving a maxbits code up beside a shorter code
        // that goes one level down
        uint32_t tot = 0;
        for (uint32_t i = 1; i <= maxbits; ++i) tot += L.cnt[i] << (maxbits - i);
        while (tot > (1u << maxbits)) {
            L.cnt[maxbits] -= 1u;
            for (uint32_t i = maxbits - 1u; i >= 1u; --i)
                if (L.cnt[i]) {
                    L.cnt[i] -= 1u;
                    L.cnt[i + 1u] += 2u;
                    break;
                }
            --tot;
        }
        uint32_t idx = 0;  // the rarest symbols take the longest codes
        for (uint32_t b2 = maxbits; b2 >= 1u; --b2)
            for (uint32_t j = L.cnt[b2]; j > 0u; --j) lens[L.order[idx++]] = (uint8_t)b2;
    }
    __syncthreads();
}

// Canonical codes (RFC 1951 §3.2.2) for lens[0, nsym), stored bit-reversed (Huffman codes go out most
// significant bit first) with the length in the high half.
__device__ void assign_codes(Lds& L, const uint8_t* lens, uint32_t nsym, uint32_t* codes, uint32_t lane) {
    if (lane == 0) {
        for (uint32_t i = 0; i < 16u; ++i) L.cnt[i] = 0;
        for (uint32_t s = 0; s < nsym; ++s) L.cnt[lens[s]] += 1u;
        L.cnt[0] = 0;
        uint32_t c = 0;
        for (uint32_t b = 1; b < 16u; ++b) {
            c = (c + L.cnt[b - 1u]) << 1;
            L.nxt[b] = c;
        }
        for (uint32_t s = 0; s < nsym; ++s) {
            const uint32_t l = lens[s];
            uint32_t v = 0;
            if (l) {
                const uint32_t cd = L.nxt[l];
                L.nxt[l] = cd + 1u;
                v = (__brev(cd) >> (32u - l)) | (l << 16);
            }
            codes[s] = v;
        }
    }
    __syncthreads();
}

// The output bit stream of one chunk.  Bit positions count from `origin`, the 128-byte line holding
// the chunk's first output byte, so that whole units are stored as aligned lines.
struct BitOut {
    uint32_t* ring;
    uint8_t* origin;
    uint32_t lead;     // the chunk's first byte within its line
    uint32_t cur;      // next bit
    uint32_t flushed;  // bits below this are in global memory (a multiple of 1024)
};

__device__ __forceinline__ void flush_units(BitOut& o, uint32_t lane) {
    while (o.cur - o.flushed >= 1024u) {
        const uint32_t ub = o.flushed >> 3, w0 = (ub >> 2) & 127u;
        if (ub >= o.lead) {
            if (lane < 32u) {
                reinterpret_cast<uint32_t*>(o.origin + ub)[lane] = o.ring[w0 + lane];
                o.ring[w0 + lane] = 0;
            }
        } else {  // the first line: only the bytes from the chunk's start on
            for (uint32_t b = lane; b < 128u; b += 64u)
                if (ub + b >= o.lead) o.origin[ub + b] = (uint8_t)(o.ring[w0 + (b >> 2)] >> (8u * (b & 3u)));
            __syncthreads();
            if (lane < 32u) o.ring[w0 + lane] = 0;
        }
        o.flushed += 1024u;
        __syncthreads();
    }
}

// Every lane appends nb <= 28 bits (v, least significant first) in lane order; all 64 lanes call it.
__device__ __forceinline__ void emit(BitOut& o, uint32_t v, uint32_t nb, uint32_t lane) {
    const uint32_t incl = wave_incl_scan(nb, lane);
    const uint32_t total = __shfl(incl, 63);
    if (nb) {
        const uint32_t at = o.cur + incl - nb, sh = at & 31u, w = (at >> 5) & 127u;
        atomicOr(&o.ring[w], v << sh);
        if (sh + nb > 32u) atomicOr(&o.ring[(w + 1u) & 127u], v >> (32u - sh));
    }
    o.cur += total;
    __syncthreads();
    flush_units(o, lane);
}

// The bytes not yet stored, up to the (byte-aligned) end; leaves the ring zeroed for the next chunk.
__device__ __forceinline__ void finish_bits(BitOut& o, uint32_t lane) {
    const uint32_t end = o.cur >> 3;
    for (uint32_t b = (o.flushed >> 3) + lane; b < end; b += 64u)
        if (b >= o.lead) o.origin[b] = (uint8_t)(o.ring[(b >> 2) & 127u] >> (8u * (b & 3u)));
    __syncthreads();
    o.ring[lane] = 0;
    o.ring[lane + 64u] = 0;
    __syncthreads();
}

// One chunk by one wave (a block of 64): returns the bytes written.  (A template so that each of the two
// kernels below has an instance of its own, inlined as into its one caller.)
template <bool PREFIX>
__device__ uint32_t emit_chunk(Lds& L, const uint8_t* __restrict__ in, uint32_t n, const uint32_t* __restrict__ hdr,
                               uint8_t* __restrict__ dst, bool stored_only, uint32_t lane) {
    const uint32_t nblk = (n + 65534u) / 65535u;
    bool stored = stored_only;
    uint32_t nt = 0, tail = 0, ne = 0, hlit = 0, hdist = 0, hclen = 0;
    bool dyn = false;
    const uint16_t* tok = reinterpret_cast<const uint16_t*>(hdr + 2);
    if (!stored) {
        nt = hdr[0];
        tail = hdr[1];
        ne = nt + (n - tail);
        for (uint32_t s = lane; s < kSyms; s += 64u) L.freq[s] = 0;
        if (lane < 20u) L.cl_freq[lane] = 0;
        if (lane < 8u) L.acc[lane] = 0;
        __syncthreads();
        for (uint32_t k = lane; k < ne; k += 64u) {
            const uint32_t t = k < nt ? tok[k] : in[tail + (k - nt)];
            const uint32_t s = t < 0x100u ? t : t < 0x8000u ? 257u + len_code(t & 0xFFu) : kDistBase + dist_code(t & 0x7FFFu);
            atomicAdd(&L.freq[s], 1u);
        }
        if (lane == 0) L.freq[256] = 1;  // end of block
        __syncthreads();
        build_lengths(L, L.freq, 286u, 15u, L.lens, lane);
        build_lengths(L, L.freq + kDistBase, 30u, 15u, L.lens + kDistBase, lane);
        if (lane < 2u) L.lens[286u + lane] = 0;
        if (lane < 2u) L.lens[kDistBase + 30u + lane] = 0;
        __syncthreads();
        // bits of the symbols under both codes, and the last used symbol of each alphabet
        uint32_t dbits = 0, fbits = 0, top_l = 0, top_d = 0;
        for (uint32_t s = lane; s < 286u; s += 64u) {
            const uint32_t f = L.freq[s], x = s > 256u ? len_extra(s - 257u) : 0u;
            dbits += f * (L.lens[s] + x);
            fbits += f * (fixed_len(s) + x);
            if (L.lens[s]) top_l = s;
        }
        if (lane < 30u) {
            const uint32_t f = L.freq[kDistBase + lane], x = dist_extra(lane);
            dbits += f * (L.lens[kDistBase + lane] + x);
            fbits += f * (5u + x);
            if (L.lens[kDistBase + lane]) top_d = lane;
        }
        atomicAdd(&L.acc[1], dbits);
        atomicAdd(&L.acc[2], fbits);
        atomicMax(&L.acc[3], top_l);
        atomicMax(&L.acc[4], top_d);
        __syncthreads();
        hlit = L.acc[3] + 1u;  // >= 257: the end-of-block symbol always has a length
        hdist = L.acc[4] + 1u;
        // the code-length code over the hlit + hdist lengths, sent one by one (no repeat symbols)
        for (uint32_t i = lane; i < hlit + hdist; i += 64u) atomicAdd(&L.cl_freq[i < hlit ? L.lens[i] : L.lens[kDistBase + i - hlit]], 1u);
        __syncthreads();
        build_lengths(L, L.cl_freq, 19u, 7u, L.cl_lens, lane);
        assign_codes(L, L.cl_lens, 19u, L.cl_code, lane);
        if (lane < 19u) {
            atomicAdd(&L.acc[5], L.cl_freq[lane] * L.cl_lens[lane]);
            if (L.cl_lens[kClOrder[lane]]) atomicMax(&L.acc[6], lane + 1u);
        }
        __syncthreads();
        hclen = L.acc[6] < 4u ? 4u : L.acc[6];
        const uint32_t dyn_bits = 3u + 14u + 3u * hclen + L.acc[5] + L.acc[1], fix_bits = 3u + L.acc[2];
        dyn = dyn_bits < fix_bits;
        stored = 8u * (n + 5u * nblk) <= (dyn ? dyn_bits : fix_bits);
    }
    if (stored) {
        uint32_t pos = 0;
        for (uint32_t off = 0; off < n; off += 65535u) {
            const uint32_t len = n - off < 65535u ? n - off : 65535u;
            if (lane < 5u) dst[pos + lane] = lane == 0u ? 0u : (uint8_t)((lane < 3u ? len : ~len) >> (8u * ((lane - 1u) & 1u)));
            for (uint32_t i = lane; i < len; i += 64u) dst[pos + 5u + i] = in[off + i];
            pos += 5u + len;
        }
        if (lane < 5u) dst[pos + lane] = lane < 3u ? 0u : 0xFFu;
        return pos + 5u;
    }
    if (!dyn) {
        for (uint32_t s = lane; s < kLit; s += 64u) L.lens[s] = (uint8_t)fixed_len(s);
        if (lane < 32u) L.lens[kDistBase + lane] = lane < 30u ? 5u : 0u;
        __syncthreads();
    }
    assign_codes(L, L.lens, kLit, L.code, lane);
    assign_codes(L, L.lens + kDistBase, 32u, L.code + kDistBase, lane);
    BitOut o;
    o.ring = L.ring;
    o.lead = (uint32_t)((uintptr_t)dst & 127u);
    o.origin = dst - o.lead;
    o.cur = o.lead * 8u;
    o.flushed = 0;
    if (dyn) {
        uint32_t v = 0, nb = 0;
        if (lane == 0u) v = 4u, nb = 3u;  // BFINAL 0, BTYPE 10
        else if (lane == 1u) v = hlit - 257u, nb = 5u;
        else if (lane == 2u) v = hdist - 1u, nb = 5u;
        else if (lane == 3u) v = hclen - 4u, nb = 4u;
        else if (lane < 4u + hclen) v = L.cl_lens[kClOrder[lane - 4u]], nb = 3u;
        emit(o, v, nb, lane);
        for (uint32_t base = 0; base < hlit + hdist; base += 64u) {
            const uint32_t i = base + lane;
            v = nb = 0;
            if (i < hlit + hdist) {
                const uint32_t c = L.cl_code[i < hlit ? L.lens[i] : L.lens[kDistBase + i - hlit]];
                v = c & 0xFFFFu;
                nb = c >> 16;
            }
            emit(o, v, nb, lane);
        }
    } else {
        emit(o, 2u, lane == 0u ? 3u : 0u, lane);  // BFINAL 0, BTYPE 01
    }
    for (uint32_t base = 0; base < ne; base += 64u) {
        const uint32_t k = base + lane;
        uint32_t v = 0, nb = 0;
        if (k < ne) {
            const uint32_t t = k < nt ? tok[k] : in[tail + (k - nt)];
            if (t < 0x100u) {
                const uint32_t c = L.code[t];
                v = c & 0xFFFFu;
                nb = c >> 16;
            } else if (t < 0x8000u) {
                const uint32_t l = t & 0xFFu, lc = len_code(l), x = len_extra(lc), c = L.code[257u + lc];
                nb = c >> 16;
                v = (c & 0xFFFFu) | ((l & ((1u << x) - 1u)) << nb);
                nb += x;
            } else {
                const uint32_t d = t & 0x7FFFu, dc = dist_code(d), x = dist_extra(dc), c = L.code[kDistBase + dc];
                nb = c >> 16;
                v = (c & 0xFFFFu) | ((d & ((1u << x) - 1u)) << nb);
                nb += x;
            }
        }
        emit(o, v, nb, lane);
    }
    {   // end of block, then the empty stored block: 000, zeros up to the byte, 00 00 FF FF
        const uint32_t eob = L.code[256], eb = eob >> 16;
        uint32_t v = 0, nb = 0;
        if (lane == 0u) v = eob & 0xFFFFu, nb = eb;
        else if (lane == 1u) nb = 3u + ((8u - ((o.cur + eb + 3u) & 7u)) & 7u);
        else if (lane == 2u) nb = 16u;
        else if (lane == 3u) v = 0xFFFFu, nb = 16u;
        emit(o, v, nb, lane);
    }
    finish_bits(o, lane);
    return (o.cur >> 3) - o.lead;
}

__global__ void __launch_bounds__(64) k_deflate_emit(const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off,
                                                     const uint32_t* __restrict__ in_len, uint8_t* __restrict__ out,
                                                     const uint64_t* __restrict__ out_off, uint32_t* __restrict__ out_len,
                                                     int32_t* __restrict__ status, uint32_t n, const uint8_t* __restrict__ workspace,
                                                     uint32_t stored_only) {
    __shared__ Lds L;
    const uint32_t lane = threadIdx.x;
    L.ring[lane] = 0;
    L.ring[lane + 64u] = 0;
    __syncthreads();
    for (uint32_t c = blockIdx.x; c < n; c += gridDim.x) {
        const uint32_t len = in_len[c];
        uint32_t w = 0;
        if (len != 0u && len <= kMaxChunk)
            w = emit_chunk<false>(L, in + in_off[c], len, reinterpret_cast<const uint32_t*>(workspace + (size_t)c * kSlotBytes + kTokOff),
                           out + out_off[c], stored_only != 0u, lane);
        if (lane == 0u) {
            out_len[c] = w;
            status[c] = len <= kMaxChunk ? NX_OK : NX_ERR_INVALID_ARG;
        }
        __syncthreads();
    }
}

// Pass 2 beside k_deflate_match_prefix: a chunk whose prefix breaks a limit writes nothing and fails
// alone (pass 1 left its slot alone).  The prefix itself is never read here.
__global__ void __launch_bounds__(64) k_deflate_emit_prefix(const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off,
                                                            const uint32_t* __restrict__ in_len,
                                                            const uint32_t* __restrict__ prefix_len, uint8_t* __restrict__ out,
                                                            const uint64_t* __restrict__ out_off, uint32_t* __restrict__ out_len,
                                                            int32_t* __restrict__ status, uint32_t n,
                                                            const uint8_t* __restrict__ workspace, uint32_t stored_only) {
    __shared__ Lds L;
    const uint32_t lane = threadIdx.x;
    L.ring[lane] = 0;
    L.ring[lane + 64u] = 0;
    __syncthreads();
    for (uint32_t c = blockIdx.x; c < n; c += gridDim.x) {
        const uint32_t len = in_len[c];
        const bool ok = len <= kMaxChunk && prefix_ok(prefix_len[c], len, in_off[c]);
        uint32_t w = 0;
        if (len != 0u && ok)
            w = emit_chunk<true>(L, in + in_off[c], len, reinterpret_cast<const uint32_t*>(workspace + (size_t)c * kSlotBytes + kTokOff),
                           out + out_off[c], stored_only != 0u, lane);
        if (lane == 0u) {
            out_len[c] = w;
            status[c] = ok ? NX_OK : NX_ERR_INVALID_ARG;
        }
        __syncthreads();
    }
}

}  // namespace deflate
}  // namespace nx

namespace {
constexpr nx::WsPairSpec kPair = {nx::WsKind::DeflateEnc, 0xFFFFu, 0};  // 16-bit stamps, as many slots as the grid asks for
constexpr nx::WsSpec kSpec = nx::kWsSpec[(int)nx::WsKind::DeflateEnc];
static_assert(((size_t)kSpec.entry_bytes << kSpec.lg) == nx::deflate::kSlotBytes, "deflate slot geometry");
static_assert(nx::deflate::kTokCap * 2u + 8u + nx::deflate::kTokOff <= nx::deflate::kSlotBytes, "deflate token area");
}  // namespace

// The stored encoding's size, which no chunk's output exceeds: 5 bytes per stored block of up to
// 65535 bytes and the closing empty block.
extern "C" size_t nx_deflate_max_compressed_length(size_t n) { return n + 5 * ((n + 65534) / 65535) + 5; }

// Replaces Deflater.deflate(..., SYNC_FLUSH) as JdkZlibEncoder.encode calls it (JdkZlibEncoder.java:
// 256-276, 308-340) for n independent chunks of at most 65536 bytes: chunk i's output is a
// byte-aligned run of non-final deflate blocks ending in 00 00 FF FF (nothing for an empty chunk).
// level as java.util.zip.Deflater: 0 stored blocks, 1..9 and -1 the one matcher.
//
// prefix_len (nx_deflate_encode_batch_ex; NULL: none, the kernels of nx_deflate_encode_batch): chunk i's
// history is the prefix_len[i] bytes before in_off[i], which matches may refer to and which are never
// emitted (what deflateSetDictionary gives zlib's matcher).
namespace {
int32_t deflate_encode(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, const uint32_t* prefix_len, uint8_t* out,
                       const uint64_t* out_off, uint32_t* out_len, int32_t* status, uint32_t n, int32_t level, void* stream) {
    NX_CLEAR_STALE_ERROR();
    if (level < -1 || level > 9) return NX_ERR_INVALID_ARG;
    if (n == 0) return NX_OK;
    if (!in || !in_off || !in_len || !out || !out_off || !out_len || !status) return NX_ERR_INVALID_ARG;
    const hipStream_t st = (hipStream_t)stream;
    using namespace nx::deflate;
    // a slot holds one chunk's tokens from pass 1 to pass 2; level 0 stores, and runs no matcher
    return nx::ws_pair_launch(
        kPair, n, st, 16u, nullptr, level != 0,
        [&](uint32_t base, uint32_t m, const nx::LaneGrid& g, nx::SharedWs& W, uint32_t stamp) {
            uint8_t* ws = static_cast<uint8_t*>(W.p);
            if (prefix_len) {
                auto* k = g.spread ? k_deflate_match_prefix<true> : k_deflate_match_prefix<false>;
                hipLaunchKernelGGL(k, dim3(g.grid), dim3(g.block), 0, st, in, in_off + base, in_len + base, prefix_len + base, m, ws, stamp);
            } else {
                auto* k = g.spread ? k_deflate_match<true> : k_deflate_match<false>;
                hipLaunchKernelGGL(k, dim3(g.grid), dim3(g.block), 0, st, in, in_off + base, in_len + base, m, ws, stamp);
            }
        },
        [&](uint32_t base, uint32_t m, unsigned waves, nx::SharedWs& W) {
            uint8_t* ws = static_cast<uint8_t*>(W.p);
            if (prefix_len)
                hipLaunchKernelGGL(k_deflate_emit_prefix, dim3(waves), dim3(64), 0, st, in, in_off + base, in_len + base, prefix_len + base,
                                   out, out_off + base, out_len + base, status + base, m, ws, level == 0 ? 1u : 0u);
            else
                hipLaunchKernelGGL(k_deflate_emit, dim3(waves), dim3(64), 0, st, in, in_off + base, in_len + base, out, out_off + base,
                                   out_len + base, status + base, m, ws, level == 0 ? 1u : 0u);
        });
}
}  // namespace

extern "C" int32_t nx_deflate_encode_batch(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint8_t* out,
                                           const uint64_t* out_off, uint32_t* out_len, int32_t* status, uint32_t n, int32_t level,
                                           void* stream) {
    return deflate_encode(in, in_off, in_len, nullptr, out, out_off, out_len, status, n, level, stream);
}

extern "C" int32_t nx_deflate_encode_batch_ex(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len,
                                              const uint32_t* prefix_len, uint8_t* out, const uint64_t* out_off, uint32_t* out_len,
                                              int32_t* status, uint32_t n, int32_t level, void* stream) {
    return deflate_encode(in, in_off, in_len, prefix_len, out, out_off, out_len, status, n, level, stream);
}
