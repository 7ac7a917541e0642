// zstd.hip — Zstandard frame encoder for ZstdEncoder (ZstdEncoder.java:128-168), two passes over
// independent chunks of up to 64 KiB.
//
// The reference compresses each full block buffer with one Zstd.compress call: one complete frame per
// block.  A chunk's output here is one such frame: magic, a single-segment header with the exact content
// size (no checksum, no dictionary ID), and ONE last block in the cheapest of Raw, RLE and Compressed by
// exact byte count.  The bytes are this encoder's own (zstd-jni's matcher is not restated); libzstd
// decodes them to the input.
//
//   pass 1, k_zstd_match, one lane per chunk (the lane grid of the other alt encoders): greedy
//     single-probe LZ77 over 4-byte hashes, a stamped 64-bit entry carrying the position's 4 bytes, one
//     exchange per probed position.  Minimum match 4, reach and length the whole chunk.  It writes to
//     the chunk's slot the literal bytes (packed, staged four to a word) and one 64-bit word per
//     sequence (literal run | match length << 16 | distance << 32), staged two to a 16-byte store.
//   pass 2, k_zstd_emit, one wave per chunk: the literals section in the cheapest of Raw, RLE and
//     Huffman (codes of at most 11 bits; the tree as direct 4-bit weights or FSE-compressed weights,
//     whichever is smaller; 1 stream up to 1023 literals, else 4), the sequences section with each of
//     the three codes in the cheapest of Predefined, RLE and FSE_Compressed, every size known before a
//     bit goes out.  The three FSE state chains are walked by three lanes, 64 sequences at a time, which
//     record (value, bit count) per step in LDS; all lanes then place the fields with a wave prefix sum.
//
// Per chunk the workspace holds 512 KiB: 32 768 hash entries (256 KiB: a single-probe table keeps a
// position only until another lands on its entry, so a match 65 000 random bytes back is found only
// while the table is not much smaller than the chunk), a two-word header {sequences, literals},
// 64 KiB of literals and up to 16 384 sequences (128 KiB).
#include "nx_common.hpp"
#include "workspace.hpp"

namespace nx {
namespace zstd {

constexpr uint32_t kMaxChunk = 65536;
constexpr uint32_t kHashLog = 15;
constexpr uint32_t kSlotBytes = 512u << 10;
constexpr uint32_t kHdrOff = (1u << kHashLog) * 8u;  // {sequences, literals} follow the hash table
constexpr uint32_t kLitOff = kHdrOff + 16u;
constexpr uint32_t kSeqOff = kLitOff + kMaxChunk;
constexpr uint32_t kSeqCap = kMaxChunk / 4u;  // a sequence takes at least four bytes of the chunk
constexpr uint32_t kHufMaxBits = 11;

// ---------------------------------------------------------------------------------------- pass 1
__device__ __forceinline__ void match_chunk(const uint8_t* __restrict__ in, uint32_t n, uint8_t* __restrict__ slot, uint32_t stamp) {
    uint64_t* table = reinterpret_cast<uint64_t*>(slot);
    uint32_t* hdr = reinterpret_cast<uint32_t*>(slot + kHdrOff);
    uint32_t* lit32 = reinterpret_cast<uint32_t*>(slot + kLitOff);
    uint64_t* seq = reinterpret_cast<uint64_t*>(slot + kSeqOff);
    const uint32_t stag = stamp << 16;
    uint32_t nl = 0, pend = 0, ns = 0, ip = 0, run0 = 0, plo = 0, phi = 0;
#define NX_PUT_LIT(b)                               \
    do {                                            \
        pend |= (uint32_t)(b) << (8u * (nl & 3u));  \
        if ((nl & 3u) == 3u) {                      \
            lit32[nl >> 2] = pend;                  \
            pend = 0;                               \
        }                                           \
        ++nl;                                       \
    } while (0)
    while (ip + 4u <= n && ns < kSeqCap) {
        const uint32_t w = ld32(in + ip);
        const uint32_t h = (w * 2654435761u) >> (32u - kHashLog);
        const uint64_t e = __hip_atomic_exchange(table + h, ((uint64_t)(stag | ip) << 32) | w, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t hi = (uint32_t)(e >> 32), cand = hi & 0xFFFFu;
        if ((hi & 0xFFFF0000u) == stag && (uint32_t)e == w && cand < ip) {
            const uint32_t maxlen = n - ip;  // a match runs to the chunk's end
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
            // sequences leave two to an aligned 16-byte store, as the literals leave four to a word
            const uint32_t slo = (nl - run0) | (len << 16), shi = ip - cand;
            if (ns & 1u) *reinterpret_cast<uint4*>(seq + ns - 1u) = make_uint4(plo, phi, slo, shi);
            else plo = slo, phi = shi;
            ++ns;
            run0 = nl;
            const uint32_t end = ip + len;
            for (uint32_t q = ip + 1; q < end && q + 4u <= n; ++q) {
                const uint32_t wq = ld32(in + q);
                __hip_atomic_store(table + ((wq * 2654435761u) >> (32u - kHashLog)), ((uint64_t)(stag | q) << 32) | wq,
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            ip = end;
        } else {
            NX_PUT_LIT(w & 0xFFu);
            ++ip;
        }
    }
    for (; ip < n; ++ip) NX_PUT_LIT(in[ip]);
#undef NX_PUT_LIT
    if (nl & 3u) lit32[nl >> 2] = pend;
    if (ns & 1u) seq[ns - 1u] = ((uint64_t)phi << 32) | plo;
    hdr[0] = ns;
    hdr[1] = nl;
}

template <bool SPREAD>
__global__ void __launch_bounds__(256) k_zstd_match(const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off,
                                                    const uint32_t* __restrict__ in_len, uint32_t n, uint8_t* __restrict__ workspace,
                                                    uint32_t stamp) {
    uint32_t tid, nthreads;
    if (!chunk_slot<SPREAD>(tid, nthreads)) return;
    if (tid >= n) return;  // one chunk per slot: its literals and sequences stay there for pass 2
    const uint32_t len = in_len[tid];
    if (len == 0 || len > kMaxChunk) return;
    match_chunk(in + in_off[tid], len, workspace + (size_t)tid * kSlotBytes, stamp);
}

// ---------------------------------------------------------------------------------------- pass 2
// An FSE encoding table (zstd's FSE_buildCTable): next-state table and per-symbol deltas.
struct Fse {
    uint16_t st[512];
    uint32_t dnb[64];
    int32_t dfs[64];
    uint16_t first[64];  // the symbol's smallest state: where a chain starts
    uint16_t cum[65];
    uint32_t log;
};

struct Lds {
    Fse T[7];  // 0..2 predefined LL, OF, ML; 3..5 this chunk's LL, OF, ML; 6 the Huffman weights
    uint8_t tsym[3][512];
    int16_t norm[3][64];
    uint32_t cnt[3][64];
    uint8_t desc[3][72];   // table descriptions of LL, OF, ML
    uint32_t dlen[3];
    uint8_t wdesc[272];    // the Huffman tree description
    uint32_t freq[256];
    uint16_t code[256];
    uint8_t lens[256];
    uint16_t order[256], parent[512], dep[512];
    uint32_t nfreq[512];
    uint32_t hcnt[16], nxt[16];
    uint32_t wcnt[16];     // histogram of the Huffman weights
    uint32_t acc[16];
    uint32_t sb[4], mode[4];  // Huffman stream bytes; the modes of LL, OF, ML
    uint8_t tcode[3][64];  // a tile's codes, in write order
    uint32_t fv[3][64];    // the chain's fields of the tile
    uint8_t fnb[3][64];
    uint32_t ring[256];    // 1 KiB of output bits: eight 128-byte units
};

__device__ const int8_t kDefNorm[3][53] = {
    {4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1},
    {1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1},
    {1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
     1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1}};
__device__ const uint8_t kDefSyms[3] = {36, 29, 53}, kDefLog[3] = {6, 5, 6}, kMaxLog[3] = {9, 8, 9};
__device__ const uint8_t kLLBits[36] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1,
                                        1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
__device__ const uint8_t kMLBits[53] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                                        0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};

__device__ __forceinline__ uint32_t hb(uint32_t x) { return 31u - (uint32_t)__builtin_clz(x); }
__device__ __forceinline__ uint32_t ll_code(uint32_t v) {
    if (v < 16u) return v;
    if (v < 24u) return 16u + ((v - 16u) >> 1);
    if (v < 32u) return 20u + ((v - 24u) >> 2);
    if (v < 48u) return 22u + ((v - 32u) >> 3);
    if (v < 64u) return 24u;
    return hb(v) + 19u;
}
__device__ __forceinline__ uint32_t ml_code(uint32_t b) {  // b = match length - 3
    if (b < 32u) return b;
    if (b < 40u) return 32u + ((b - 32u) >> 1);
    if (b < 48u) return 36u + ((b - 40u) >> 2);
    if (b < 64u) return 38u + ((b - 48u) >> 3);
    if (b < 96u) return 40u + ((b - 64u) >> 4);
    if (b < 128u) return 42u;
    return hb(b) + 36u;
}

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t x, uint32_t lane) {
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    return x;
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t x, uint32_t lane) { return __shfl(wave_incl_scan(x, lane), 63); }

// The accuracy log for `total` symbols of which `present` are distinct.
__device__ __forceinline__ uint32_t pick_log(uint32_t total, uint32_t present, uint32_t maxlog) {
    uint32_t l = hb(total > 2u ? total - 1u : 1u);
    l = l > 7u ? l - 2u : 5u;
    if (l > maxlog) l = maxlog;
    while ((1u << l) < 2u * present && l < maxlog) ++l;
    return l;
}

// Counts to probabilities that sum to 2^log: a present symbol whose share is below one cell gets -1
// ("less than 1", one cell at the table's end); the rest goes to, or comes from, the largest.  One lane.
__device__ void fse_normalize(const uint32_t* cnt, uint32_t nsym, uint32_t total, uint32_t log, int16_t* norm) {
    const uint32_t size = 1u << log;
    uint32_t sum = 0;
    for (uint32_t s = 0; s < nsym; ++s) {
        int32_t p = 0;
        if (cnt[s]) {
            p = (int32_t)(((uint64_t)cnt[s] << log) / total);
            if (p < 1) p = -1;
            sum += (uint32_t)(p < 0 ? 1 : p);
        }
        norm[s] = (int16_t)p;
    }
    for (;;) {
        uint32_t big = 0;
        for (uint32_t s = 1; s < nsym; ++s)
            if (norm[s] > norm[big]) big = s;
        if (sum <= size) {
            norm[big] = (int16_t)(norm[big] + (int32_t)(size - sum));
            return;
        }
        if (norm[big] <= 1) return;  // cannot happen while 2^log >= 2 * present (pick_log)
        norm[big] = (int16_t)(norm[big] - 1);
        --sum;
    }
}

// zstd's FSE_buildCTable for norm[0, nsym).  One lane; tsym is its scratch of 2^log bytes.
template <class N>
__device__ void fse_build(Fse& T, const N* norm, uint32_t nsym, uint32_t log, uint8_t* tsym) {
    const uint32_t size = 1u << log, step = (size >> 1) + (size >> 3) + 3u, mask = size - 1u;
    uint32_t high = size - 1u, c = 0;
    for (uint32_t s = 0; s < nsym; ++s) {
        T.cum[s] = (uint16_t)c;
        const int32_t p = norm[s];
        if (p == -1) {
            tsym[high--] = (uint8_t)s;
            c += 1u;
        } else {
            c += (uint32_t)p;
        }
    }
    T.cum[nsym] = (uint16_t)c;
    uint32_t pos = 0;
    for (uint32_t s = 0; s < nsym; ++s)
        for (int32_t i = 0; i < (int32_t)norm[s]; ++i) {
            tsym[pos] = (uint8_t)s;
            pos = (pos + step) & mask;
            while (pos > high) pos = (pos + step) & mask;
        }
    for (uint32_t u = 0; u < size; ++u) {
        const uint32_t s = tsym[u];
        T.st[T.cum[s]] = (uint16_t)(size + u);
        T.cum[s] = (uint16_t)(T.cum[s] + 1u);
    }
    uint32_t total = 0;
    for (uint32_t s = 0; s < nsym; ++s) {
        const int32_t p = norm[s];
        if (p == 0) {
            T.dnb[s] = ((log + 1u) << 16) - size;
            T.dfs[s] = 0;
            T.first[s] = 0;
            continue;
        }
        const uint32_t a = (uint32_t)(p < 0 ? 1 : p);
        if (a == 1u) {
            T.dnb[s] = (log << 16) - size;
            T.dfs[s] = (int32_t)total - 1;
        } else {
            const uint32_t mb = log - hb(a - 1u);
            T.dnb[s] = (mb << 16) - (a << mb);
            T.dfs[s] = (int32_t)total - (int32_t)a;
        }
        T.first[s] = T.st[T.cum[s] - a];
        total += a;
    }
    T.log = log;
}

// zstd's FSE_writeNCount: the table description of norm[0, nsym) into out; returns its bytes.  One lane.
__device__ uint32_t fse_write_ncount(const int16_t* norm, uint32_t nsym, uint32_t log, uint8_t* out) {
    uint64_t acc = log - 5u;
    uint32_t nbits = 4, w = 0;
    const int32_t size = 1 << log;
    int32_t remaining = size + 1, threshold = size;
    uint32_t nb = log + 1u, sym = 0;
    bool prev0 = false;
#define NX_NC_PUT(v, k)                  \
    do {                                 \
        acc |= (uint64_t)(v) << nbits;   \
        nbits += (k);                    \
        while (nbits >= 8u) {            \
            out[w++] = (uint8_t)acc;     \
            acc >>= 8;                   \
            nbits -= 8u;                 \
        }                                \
    } while (0)
    while (sym < nsym && remaining > 1) {
        if (prev0) {
            uint32_t start = sym;
            while (sym < nsym && norm[sym] == 0) ++sym;
            if (sym == nsym) break;
            while (sym >= start + 24u) {
                start += 24u;
                NX_NC_PUT(0xFFFFu, 16u);
            }
            while (sym >= start + 3u) {
                start += 3u;
                NX_NC_PUT(3u, 2u);
            }
            NX_NC_PUT(sym - start, 2u);
        }
        int32_t c = norm[sym++];
        const int32_t mx = (2 * threshold - 1) - remaining;
        remaining -= c < 0 ? -c : c;
        ++c;
        if (c >= threshold) c += mx;
        NX_NC_PUT((uint32_t)c, nb - (c < mx ? 1u : 0u));
        prev0 = c == 1;
        if (remaining < 1) break;
        while (remaining < threshold) {
            --nb;
            threshold >>= 1;
        }
    }
    if (nbits) out[w++] = (uint8_t)acc;
#undef NX_NC_PUT
    return w;
}

// Code lengths of at most maxbits for freq[0, 256), of which at least two are used (k_deflate_emit's
// scheme: rank sort across the wave, two-queue merge, lengths over the limit folded back).  All lanes.
__device__ void build_lengths(Lds& L, uint32_t used, uint32_t maxbits, uint32_t lane) {
    for (uint32_t s = lane; s < 256u; s += 64u) {
        L.lens[s] = 0;
        const uint32_t fs = L.freq[s];
        if (fs == 0u) continue;
        uint32_t r = 0;
        for (uint32_t t = 0; t < 256u; ++t) {
            const uint32_t ft = L.freq[t];
            r += (ft != 0u) & ((ft < fs) | ((ft == fs) & (t < s)));
        }
        L.order[r] = (uint16_t)s;
        L.nfreq[r] = fs;
    }
    __syncthreads();
    if (lane == 0) {
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
        for (uint32_t i = 0; i < 16u; ++i) L.hcnt[i] = 0;
        L.dep[total - 1u] = 0;
        for (uint32_t i = total - 1u; i-- > 0u;) {
            const uint32_t d = (uint32_t)L.dep[L.parent[i]] + 1u;
            L.dep[i] = (uint16_t)d;
            if (i < used) L.hcnt[d < maxbits ? d : maxbits] += 1u;
        }
        uint32_t tot = 0;
        for (uint32_t i = 1; i <= maxbits; ++i) tot += L.hcnt[i] << (maxbits - i);
        while (tot > (1u << maxbits)) {
            L.hcnt[maxbits] -= 1u;
            for (uint32_t i = maxbits - 1u; i >= 1u; --i)
                if (L.hcnt[i]) {
                    L.hcnt[i] -= 1u;
                    L.hcnt[i + 1u] += 2u;
                    break;
                }
            --tot;
        }
        uint32_t idx = 0;  // the rarest symbols take the longest codes
        for (uint32_t b2 = maxbits; b2 >= 1u; --b2)
            for (uint32_t j = L.hcnt[b2]; j > 0u; --j) L.lens[L.order[idx++]] = (uint8_t)b2;
        // Zstandard's codes: values rise from 0 at the longest length in symbol order, halved at each
        // shorter length (hcnt still holds the count per length)
        uint32_t c = 0;
        for (uint32_t l = maxbits; l >= 1u; --l) {
            L.nxt[l] = c;
            c = (c + L.hcnt[l]) >> 1;
        }
        for (uint32_t s = 0; s < 256u; ++s) {
            const uint32_t l = L.lens[s];
            if (l) L.code[s] = (uint16_t)(L.nxt[l]++);
        }
    }
    __syncthreads();
}

// The Huffman tree description into L.wdesc, the smaller of the direct and the FSE form; returns its
// bytes (0: neither form can carry this tree).  maxsym: the last used symbol; mb: the longest length.  Lane 0.
__device__ uint32_t tree_desc(Lds& L, uint32_t maxsym, uint32_t mb) {
    const uint32_t count = maxsym;  // weights listed: symbols below the last, whose weight is implied
#define NX_W(s) (L.lens[s] ? mb + 1u - L.lens[s] : 0u)
    const uint32_t direct = count <= 128u ? 1u + (count + 1u) / 2u : 0u;
    uint32_t fse = 0;
    if (count >= 2u) {
        uint32_t* cnt = L.wcnt;  // (not L.cnt: the sequence histograms accumulate there)
        for (uint32_t i = 0; i < 16u; ++i) cnt[i] = 0;
        for (uint32_t s = 0; s < count; ++s) cnt[NX_W(s)] += 1u;
        uint32_t present = 0, top = 0;
        for (uint32_t i = 0; i < 13u; ++i)
            if (cnt[i]) {
                ++present;
                top = i;
            }
        if (present >= 2u) {
            const uint32_t log = pick_log(count, present, 6u);
            fse_normalize(cnt, top + 1u, count, log, L.norm[0]);
            Fse& T = L.T[6];
            fse_build(T, L.norm[0], top + 1u, log, L.tsym[0]);
            uint8_t* out = L.wdesc + 1;
            uint32_t w = fse_write_ncount(L.norm[0], top + 1u, log, out);
            // two interleaved states: symbol i belongs to state i & 1, the last two start them
            uint32_t st0 = T.first[NX_W(count - 1u)], st1 = T.first[NX_W(count - 2u)];
            if ((count - 1u) & 1u) {
                const uint32_t t = st0;
                st0 = st1;
                st1 = t;
            }
            uint64_t acc = 0;
            uint32_t nbits = 0;
            for (uint32_t i = count - 2u; i-- > 0u;) {
                const uint32_t sym = NX_W(i), s0 = (i & 1u) ? st1 : st0, nb = (s0 + T.dnb[sym]) >> 16;
                acc |= (uint64_t)(s0 & ((1u << nb) - 1u)) << nbits;
                nbits += nb;
                const uint32_t s1 = T.st[(s0 >> nb) + T.dfs[sym]];
                if (i & 1u) st1 = s1;
                else st0 = s1;
                while (nbits >= 8u) {
                    out[w++] = (uint8_t)acc;
                    acc >>= 8;
                    nbits -= 8u;
                }
            }
            acc |= (uint64_t)(st1 - (1u << log)) << nbits;
            nbits += log;
            acc |= (uint64_t)(st0 - (1u << log)) << nbits;
            nbits += log;
            acc |= (uint64_t)1 << nbits;
            nbits += 1u;
            while (nbits > 0u) {
                out[w++] = (uint8_t)acc;
                acc >>= 8;
                nbits = nbits > 8u ? nbits - 8u : 0u;
            }
            if (w < 128u) {
                L.wdesc[0] = (uint8_t)w;
                fse = 1u + w;
            }
        }
    }
    if (direct && (!fse || direct <= fse)) {
        L.wdesc[0] = (uint8_t)(127u + count);
        for (uint32_t i = 0; i < count; i += 2u) L.wdesc[1u + i / 2u] = (uint8_t)((NX_W(i) << 4) | (i + 1u < count ? NX_W(i + 1u) : 0u));
        return direct;
    }
#undef NX_W
    return fse;
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
        const uint32_t ub = o.flushed >> 3, w0 = (ub >> 2) & 255u;
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

__device__ __forceinline__ void put_bits(uint32_t* ring, uint32_t at, uint64_t v, uint32_t nb) {  // nb <= 64, v below 2^nb
    if (!nb) return;
    const uint32_t sh = at & 31u, w = (at >> 5) & 255u;
    atomicOr(&ring[w], (uint32_t)(v << sh));
    if (sh + nb > 32u) {
        atomicOr(&ring[(w + 1u) & 255u], (uint32_t)(v >> (32u - sh)));
        if (sh + nb > 64u) atomicOr(&ring[(w + 2u) & 255u], (uint32_t)(v >> (64u - sh)));
    }
}

// Every lane appends a (na <= 32 bits) then b (nb <= 48 bits), least significant first, in lane order;
// all 64 lanes call it.  At most 64 * 80 bits a call: with the unit still open that stays inside the ring.
__device__ __forceinline__ void emit2(BitOut& o, uint32_t a, uint32_t na, uint64_t b, uint32_t nb, uint32_t lane) {
    const uint32_t incl = wave_incl_scan(na + nb, lane);
    const uint32_t total = __shfl(incl, 63);
    const uint32_t at = o.cur + incl - (na + nb);
    put_bits(o.ring, at, a, na);
    put_bits(o.ring, at + na, b, nb);
    o.cur += total;
    __syncthreads();
    flush_units(o, lane);
}
__device__ __forceinline__ void emit(BitOut& o, uint32_t v, uint32_t nb, uint32_t lane) { emit2(o, v, nb, 0, 0, lane); }

// n bytes of p (LDS or global), 64 a call
template <class P>
__device__ __forceinline__ void emit_bytes(BitOut& o, P p, uint32_t n, uint32_t lane) {
    for (uint32_t base = 0; base < n; base += 64u) {
        const uint32_t i = base + lane;
        emit(o, i < n ? p[i] : 0u, i < n ? 8u : 0u, lane);
    }
}

__device__ __forceinline__ void finish_bits(BitOut& o, uint32_t lane) {
    const uint32_t end = o.cur >> 3;
    for (uint32_t b = (o.flushed >> 3) + lane; b < end; b += 64u)
        if (b >= o.lead) o.origin[b] = (uint8_t)(o.ring[(b >> 2) & 255u] >> (8u * (b & 3u)));
    __syncthreads();
    for (uint32_t i = lane; i < 256u; i += 64u) o.ring[i] = 0;
    __syncthreads();
}

__device__ __forceinline__ uint32_t raw_lit_hdr(uint32_t n) { return n < 32u ? 1u : n < 4096u ? 2u : 3u; }

// A tile of up to 64 sequences, from index hi - 1 down: lane j takes sequence hi - 1 - j (the order the
// bitstream is written in) and leaves its three codes in L.tcode.
__device__ __forceinline__ uint64_t load_tile(Lds& L, const uint64_t* seq, uint32_t hi, uint32_t cnt, uint32_t lane) {
    uint64_t q = 0;
    if (lane < cnt) {
        q = seq[hi - 1u - lane];
        const uint32_t ll = (uint32_t)q & 0xFFFFu, ml = ((uint32_t)q >> 16) & 0xFFFFu, of = (uint32_t)(q >> 32) + 3u;
        L.tcode[0][lane] = (uint8_t)ll_code(ll);
        L.tcode[1][lane] = (uint8_t)hb(of);
        L.tcode[2][lane] = (uint8_t)ml_code(ml - 3u);
    }
    return q;
}

// One chain over a tile: lane's table T (null: an RLE code, no bits), code row k.  Returns the bits.
template <bool RECORD>
__device__ __forceinline__ uint32_t walk_tile(Lds& L, const Fse* T, uint32_t k, uint32_t& state, uint32_t cnt, bool first_tile) {
    uint32_t bits = 0;
    for (uint32_t j = 0; j < cnt; ++j) {
        uint32_t v = 0, nb = 0;
        if (T) {
            const uint32_t c = L.tcode[k][j];
            if (first_tile && j == 0u) {
                state = T->first[c];
            } else {
                nb = (state + T->dnb[c]) >> 16;
                v = state & ((1u << nb) - 1u);
                state = T->st[(state >> nb) + T->dfs[c]];
            }
        }
        bits += nb;
        if (RECORD) {
            L.fv[k][j] = v;
            L.fnb[k][j] = (uint8_t)nb;
        }
    }
    return bits;
}

// One chunk by one wave (a block of 64): returns the bytes written (0 with *bad set: the sizes worked
// out before the bits disagree with the bits, which is a bug).
__device__ uint32_t emit_chunk(Lds& L, const uint8_t* __restrict__ in, uint32_t n, const uint8_t* __restrict__ slot,
                               uint8_t* __restrict__ dst, uint32_t lane, bool* bad) {
    const uint32_t* hdr = reinterpret_cast<const uint32_t*>(slot + kHdrOff);
    const uint8_t* lit = slot + kLitOff;
    const uint64_t* seq = reinterpret_cast<const uint64_t*>(slot + kSeqOff);
    const uint32_t ns = hdr[0], nl = hdr[1];
    const uint32_t fh = n < 256u ? 6u : 7u;  // magic, descriptor, content size

    for (uint32_t s = lane; s < 256u; s += 64u) L.freq[s] = 0;
    for (uint32_t s = lane; s < 192u; s += 64u) L.cnt[s / 64u][s % 64u] = 0;
    if (lane < 16u) L.acc[lane] = 0;
    __syncthreads();
    for (uint32_t k = lane; k < nl; k += 64u) atomicAdd(&L.freq[lit[k]], 1u);
    __syncthreads();
    {
        uint32_t used = 0, top = 0;
        for (uint32_t s = lane; s < 256u; s += 64u)
            if (L.freq[s]) {
                ++used;
                top = s;
            }
        if (used) {
            atomicAdd(&L.acc[0], used);
            atomicMax(&L.acc[1], top);
        }
    }
    __syncthreads();
    const uint32_t used = L.acc[0], maxsym = L.acc[1];

    // ---- the whole chunk one byte: an RLE block
    bool rle_block = false;
    if (n >= 2u) {
        if (ns == 0u) rle_block = used == 1u;
        else if (ns == 1u && nl == 1u) rle_block = seq[0] == ((uint64_t)(1u | ((n - 1u) << 16)) | ((uint64_t)1 << 32));
    }
    uint32_t lit_mode = 0, lit_bytes = raw_lit_hdr(nl) + nl;  // the literals section: 0 Raw, 1 RLE, 2 Huffman
    uint32_t tdesc = 0, lhdr = 0, q4 = 0;
    uint32_t seq_bytes = 1, nsh = 1, seq_bits = 0;
    if (!rle_block) {
        if (used == 1u && raw_lit_hdr(nl) + 1u < lit_bytes) {
            lit_mode = 1;
            lit_bytes = raw_lit_hdr(nl) + 1u;
        }
        if (used >= 2u) {
            build_lengths(L, used, kHufMaxBits, lane);
            if (lane == 0) {
                uint32_t mb = 0;
                for (uint32_t l = 1; l <= kHufMaxBits; ++l)
                    if (L.hcnt[l]) mb = l;
                L.acc[2] = tree_desc(L, maxsym, mb);
            }
            __syncthreads();
            tdesc = L.acc[2];
            const uint32_t nstreams = nl <= 1023u ? 1u : 4u;
            q4 = nstreams == 1u ? nl : (nl + 3u) / 4u;
            uint32_t total = 0;
            for (uint32_t s = 0; s < nstreams; ++s) {
                const uint32_t a = s * q4, b = s == nstreams - 1u ? nl : a + q4;
                uint32_t bits = 0;
                for (uint32_t k = a + lane; k < b; k += 64u) bits += L.lens[lit[k]];
                const uint32_t sb = wave_sum(bits, lane) / 8u + 1u;
                if (lane == 0) L.sb[s] = sb;
                total += sb;
            }
            lhdr = nl <= 1023u ? 3u : nl <= 16383u ? 4u : 5u;
            const uint32_t hb_ = lhdr + tdesc + (nstreams == 4u ? 6u : 0u) + total;
            if (tdesc && hb_ < lit_bytes) {
                lit_mode = 2;
                lit_bytes = hb_;
            }
        }
        // ---- the sequences section
        if (ns) {
            uint32_t xbits = 0;
            for (uint32_t hi = ns; hi > 0u;) {
                const uint32_t cnt = hi < 64u ? hi : 64u;
                load_tile(L, seq, hi, cnt, lane);
                if (lane < cnt) {
                    const uint32_t a = L.tcode[0][lane], b = L.tcode[1][lane], c = L.tcode[2][lane];
                    atomicAdd(&L.cnt[0][a], 1u);
                    atomicAdd(&L.cnt[1][b], 1u);
                    atomicAdd(&L.cnt[2][c], 1u);
                    xbits += kLLBits[a] + b + kMLBits[c];
                }
                hi -= cnt;
            }
            xbits = wave_sum(xbits, lane);
            __syncthreads();
            if (lane < 3u) {  // this chunk's three tables, side by side
                const uint32_t k = lane, nsym = kDefSyms[k];
                uint32_t present = 0, top = 0;
                for (uint32_t s = 0; s < nsym; ++s)
                    if (L.cnt[k][s]) {
                        ++present;
                        top = s;
                    }
                L.acc[4u + k] = present;
                L.acc[7u + k] = top;
                L.dlen[k] = 0;
                if (present >= 2u) {
                    const uint32_t log = pick_log(ns, present, kMaxLog[k]);
                    fse_normalize(L.cnt[k], top + 1u, ns, log, L.norm[k]);
                    fse_build(L.T[3u + k], L.norm[k], top + 1u, log, L.tsym[k]);
                    L.dlen[k] = fse_write_ncount(L.norm[k], top + 1u, log, L.desc[k]);
                }
            }
            __syncthreads();
            // the exact bits of every candidate: lanes 0..2 walk the predefined tables, 3..5 this chunk's
            {
                const uint32_t k = lane % 3u;
                const Fse* T = lane < 3u ? &L.T[lane] : lane < 6u && L.acc[4u + k] >= 2u ? &L.T[lane] : nullptr;
                uint32_t state = 0, bits = 0;
                for (uint32_t hi = ns; hi > 0u;) {
                    const uint32_t cnt = hi < 64u ? hi : 64u;
                    __syncthreads();
                    load_tile(L, seq, hi, cnt, lane);
                    __syncthreads();
                    if (lane < 6u) bits += walk_tile<false>(L, T, k, state, cnt, hi == ns);
                    hi -= cnt;
                }
                if (lane < 6u) L.acc[10u + lane] = bits + (T ? T->log : 0u);
                __syncthreads();
            }
            seq_bits = xbits + 1u;
            uint32_t dsum = 0;
            for (uint32_t k = 0; k < 3u; ++k) {
                uint32_t best = L.acc[10u + k], md = 0;  // Predefined, then RLE, then FSE_Compressed: ties to the simpler
                if (L.acc[4u + k] == 1u && 8u < best) {
                    best = 8u;
                    md = 1;
                }
                if (L.acc[4u + k] >= 2u && L.acc[13u + k] + 8u * L.dlen[k] < best) {
                    best = L.acc[13u + k] + 8u * L.dlen[k];
                    md = 2;
                }
                if (lane == 0) L.mode[k] = md;
                if (md == 1u) dsum += 1u;
                else if (md == 2u) {
                    dsum += L.dlen[k];
                    seq_bits += L.acc[13u + k];
                } else {
                    seq_bits += L.acc[10u + k];
                }
            }
            nsh = ns < 128u ? 1u : ns < 0x7F00u ? 2u : 3u;
            seq_bytes = nsh + 1u + dsum + (seq_bits + 7u) / 8u;
        }
    }
    __syncthreads();
    const uint32_t block = lit_bytes + seq_bytes;
    const bool raw_block = !rle_block && block >= n;

    // ---- frame header and block header, then a Raw or RLE block's content, as plain bytes
    const uint32_t bsize = rle_block ? n : raw_block ? n : block;
    const uint32_t btype = rle_block ? 1u : raw_block ? 0u : 2u;
    const uint32_t bh = 1u | (btype << 1) | (bsize << 3);
    uint32_t hbyte = 0;
    if (lane < 4u) hbyte = 0xFD2FB528u >> (8u * lane);
    else if (lane == 4u) hbyte = n < 256u ? 0x20u : 0x60u;
    else if (lane < fh) hbyte = n < 256u ? n : (n - 256u) >> (8u * (lane - 5u));
    else if (lane < fh + 3u) hbyte = bh >> (8u * (lane - fh));
    hbyte &= 0xFFu;
    if (rle_block || raw_block) {
        if (lane < fh + 3u) dst[lane] = (uint8_t)hbyte;
        if (rle_block) {
            if (lane == 0) dst[fh + 3u] = in[0];
            return fh + 4u;
        }
        for (uint32_t i = lane; i < n; i += 64u) dst[fh + 3u + i] = in[i];
        return fh + 3u + n;
    }

    BitOut o;
    o.ring = L.ring;
    o.lead = (uint32_t)((uintptr_t)dst & 127u);
    o.origin = dst - o.lead;
    o.cur = o.lead * 8u;
    o.flushed = 0;
    emit(o, hbyte, lane < fh + 3u ? 8u : 0u, lane);
    // ---- literals
    if (lit_mode < 2u) {
        const uint32_t h = raw_lit_hdr(nl);
        const uint32_t hv = h == 1u ? lit_mode | (nl << 3) : h == 2u ? lit_mode | 4u | (nl << 4) : lit_mode | 12u | (nl << 4);
        emit(o, hv, lane == 0u ? 8u * h : 0u, lane);
        if (lit_mode == 1u) {
            emit(o, lit[0], lane == 0u ? 8u : 0u, lane);
        } else {
            for (uint32_t base = 0; base < nl; base += 256u) {  // four bytes a lane
                const uint32_t i = base + 4u * lane;
                uint32_t v = 0, k = 0;
                for (; k < 4u && i + k < nl; ++k) v |= (uint32_t)lit[i + k] << (8u * k);
                emit(o, v, 8u * k, lane);
            }
        }
    } else {
        const uint32_t nstreams = nl <= 1023u ? 1u : 4u;
        const uint32_t comp = lit_bytes - lhdr;
        uint64_t hv;
        if (lhdr == 3u) hv = 2u | ((nstreams == 4u ? 1u : 0u) << 2) | (nl << 4) | ((uint64_t)comp << 14);
        else if (lhdr == 4u) hv = 2u | (2u << 2) | (nl << 4) | ((uint64_t)comp << 18);
        else hv = 2u | (3u << 2) | (nl << 4) | ((uint64_t)comp << 22);
        emit2(o, 0, 0, hv, lane == 0u ? 8u * lhdr : 0u, lane);
        emit_bytes(o, L.wdesc, tdesc, lane);
        if (nstreams == 4u) emit(o, lane < 3u ? L.sb[lane] : 0u, lane < 3u ? 16u : 0u, lane);
        for (uint32_t s = 0; s < nstreams; ++s) {
            const uint32_t a = s * q4, b = s == nstreams - 1u ? nl : a + q4;
            for (uint32_t hi = b; hi > a;) {  // each lane codes one literal, the stream's last first
                const uint32_t cnt = hi - a < 64u ? hi - a : 64u;
                uint32_t v = 0, nb = 0;
                if (lane < cnt) {
                    const uint32_t c = lit[hi - 1u - lane];
                    v = L.code[c];
                    nb = L.lens[c];
                }
                emit(o, v, nb, lane);
                hi -= cnt;
            }
            emit(o, 1u, lane == 0u ? 1u + ((8u - ((o.cur + 1u) & 7u)) & 7u) : 0u, lane);  // the closing bit, zeros up to the byte
        }
    }
    // ---- sequences
    if (ns == 0u) {
        emit(o, 0u, lane == 0u ? 8u : 0u, lane);
    } else {
        const uint32_t nv = nsh == 1u ? ns : nsh == 2u ? (((ns >> 8) + 128u) | ((ns & 255u) << 8)) : (255u | ((ns - 0x7F00u) << 8));
        emit(o, lane == 0u ? nv : (L.mode[0] << 6) | (L.mode[1] << 4) | (L.mode[2] << 2), lane == 0u ? 8u * nsh : lane == 1u ? 8u : 0u, lane);
        for (uint32_t k = 0; k < 3u; ++k) {
            if (L.mode[k] == 1u) emit(o, L.acc[7u + k], lane == 0u ? 8u : 0u, lane);
            else if (L.mode[k] == 2u) emit_bytes(o, L.desc[k], L.dlen[k], lane);
        }
        const Fse* T = nullptr;
        if (lane < 3u && L.mode[lane] != 1u) T = &L.T[L.mode[lane] == 2u ? 3u + lane : lane];
        uint32_t state = 0;
        for (uint32_t hi = ns; hi > 0u;) {
            const uint32_t cnt = hi < 64u ? hi : 64u;
            const uint64_t q = load_tile(L, seq, hi, cnt, lane);
            __syncthreads();
            if (lane < 3u) walk_tile<true>(L, T, lane, state, cnt, hi == ns);
            __syncthreads();
            uint32_t a = 0, na = 0, nb = 0;
            uint64_t b = 0;
            if (lane < cnt) {
                // the state bits in the order offset, match length, literal length; then the extra bits
                // in the order literal length, match length, offset
                a = L.fv[1][lane];
                na = L.fnb[1][lane];
                a |= L.fv[2][lane] << na;
                na += L.fnb[2][lane];
                a |= L.fv[0][lane] << na;
                na += L.fnb[0][lane];
                const uint32_t ll = (uint32_t)q & 0xFFFFu, mlb = (((uint32_t)q >> 16) & 0xFFFFu) - 3u, of = (uint32_t)(q >> 32) + 3u;
                const uint32_t cl = L.tcode[0][lane], co = L.tcode[1][lane], cm = L.tcode[2][lane];
                const uint32_t xl = kLLBits[cl], xm = kMLBits[cm];
                b = ll & ((1u << xl) - 1u);
                b |= (uint64_t)(mlb & ((1u << xm) - 1u)) << xl;
                b |= (uint64_t)(of & ((1u << co) - 1u)) << (xl + xm);
                nb = xl + xm + co;
            }
            emit2(o, a, na, b, nb, lane);
            hi -= cnt;
        }
        {   // the final states: match length, offset, literal length; then the closing bit
            const uint32_t slog = T ? T->log : 0u, sval = T ? state - (1u << slog) : 0u;
            const uint32_t src = lane < 3u ? 2u - lane : 0u;
            uint32_t v = __shfl(sval, src), nb = __shfl(slog, src);
            const uint32_t sbits = __shfl(slog, 0) + __shfl(slog, 1) + __shfl(slog, 2);
            if (lane == 3u) v = 1u, nb = 1u + ((8u - ((o.cur + sbits + 1u) & 7u)) & 7u);
            else if (lane > 3u) v = nb = 0;
            emit(o, v, nb, lane);
        }
    }
    finish_bits(o, lane);
    const uint32_t wrote = (o.cur >> 3) - o.lead;
    if (wrote != fh + 3u + block) *bad = true;
    return wrote;
}

__global__ void __launch_bounds__(64) k_zstd_emit(const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off,
                                                  const uint32_t* __restrict__ in_len, uint8_t* __restrict__ out,
                                                  const uint64_t* __restrict__ out_off, uint32_t* __restrict__ out_len,
                                                  int32_t* __restrict__ status, uint32_t n, const uint8_t* __restrict__ workspace) {
    __shared__ Lds L;
    const uint32_t lane = threadIdx.x;
    for (uint32_t i = lane; i < 256u; i += 64u) L.ring[i] = 0;
    if (lane < 3u) fse_build(L.T[lane], kDefNorm[lane], kDefSyms[lane], kDefLog[lane], L.tsym[lane]);
    __syncthreads();
    for (uint32_t c = blockIdx.x; c < n; c += gridDim.x) {
        const uint32_t len = in_len[c];
        uint32_t w = 0;
        bool bad = false;
        if (len != 0u && len <= kMaxChunk)
            w = emit_chunk(L, in + in_off[c], len, workspace + (size_t)c * kSlotBytes, out + out_off[c], lane, &bad);
        if (lane == 0u) {
            out_len[c] = bad ? 0u : w;
            status[c] = len > kMaxChunk ? NX_ERR_INVALID_ARG : bad ? NX_ERR_INTERNAL : NX_OK;
        }
        __syncthreads();
    }
}

}  // namespace zstd
}  // namespace nx

namespace {
// Stamps are 16 bits.  Most slots the standalone entry grows the workspace to: 32 768 (16 GiB), a larger batch
// runs in sub-batches; that many lanes are where the table request rate saturates, so nothing is lost.
constexpr nx::WsPairSpec kPair = {nx::WsKind::ZstdEnc, 0xFFFFu, 32768};
constexpr nx::WsSpec kSpec = nx::kWsSpec[(int)nx::WsKind::ZstdEnc];
static_assert(((size_t)kSpec.entry_bytes << kSpec.lg) == nx::zstd::kSlotBytes, "zstd slot geometry");
static_assert(nx::zstd::kSeqOff % 16u == 0 && nx::zstd::kSeqOff + nx::zstd::kSeqCap * 8u <= nx::zstd::kSlotBytes, "zstd sequence area");
}  // namespace

// ZSTD_compressBound, which Zstd.compressBound returns (ZstdEncoder.java:116,152).
extern "C" size_t nx_zstd_max_compressed_length(size_t n) {
    return n + (n >> 8) + (n < ((size_t)128 << 10) ? (((size_t)128 << 10) - n) >> 11 : 0);
}

// Replaces Zstd.compress(dst, src, level) as ZstdEncoder.flushBufferedData calls it (ZstdEncoder.java:
// 146-168) for n independent chunks of at most 65536 bytes: chunk i's output is one complete Zstandard
// frame (nothing for an empty chunk).  level as libzstd: -131072..22, every one the one matcher.
extern "C" int32_t nx_zstd_encode_batch(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint8_t* out,
                                        const uint64_t* out_off, uint32_t* out_len, int32_t* status, uint32_t n, int32_t level,
                                        void* stream) {
    NX_CLEAR_STALE_ERROR();
    if (level < -131072 || level > 22) return NX_ERR_INVALID_ARG;
    if (n == 0) return NX_OK;
    if (!in || !in_off || !in_len || !out || !out_off || !out_len || !status) return NX_ERR_INVALID_ARG;
    const hipStream_t st = (hipStream_t)stream;
    // a slot holds one chunk's literals and sequences from pass 1 to pass 2
    return nx::ws_pair_launch(
        kPair, n, st, 8u, nullptr, true,
        [&](uint32_t base, uint32_t m, const nx::LaneGrid& g, nx::SharedWs& W, uint32_t stamp) {
            auto* k = g.spread ? nx::zstd::k_zstd_match<true> : nx::zstd::k_zstd_match<false>;
            hipLaunchKernelGGL(k, dim3(g.grid), dim3(g.block), 0, st, in, in_off + base, in_len + base, m, static_cast<uint8_t*>(W.p), stamp);
        },
        [&](uint32_t base, uint32_t m, unsigned waves, nx::SharedWs& W) {
            hipLaunchKernelGGL(nx::zstd::k_zstd_emit, dim3(waves), dim3(64), 0, st, in, in_off + base, in_len + base, out, out_off + base,
                               out_len + base, status + base, m, static_cast<uint8_t*>(W.p));
        });
}
