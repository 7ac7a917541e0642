// bzip2_encode.hip — bzip2 encoder over a batch of items (nx_bzip2_encode_batch; what Bzip2Encoder.java writes
// for one encode(in) followed by close(), one stream per item).
//
// One workgroup of kThreads lanes (kWaves waves) per stream; a stream's blocks are done one after another by
// that workgroup and the bit position carries over the block boundary.  The format logic is
// bzip2_encode_core.hpp, the same functions the host encoder runs.  Per block:
//   1. SERIAL, lane 0: the first run-length stage, the block CRC and block filling, from LDS tiles of the input
//      that the workgroup loads, into the slot's block bytes;
//   2. the Burrows-Wheeler transform: a sort of the block's n cyclic rotations by prefix doubling.  The first
//      sort is by two bytes; every round then doubles the compared length h: the list (sa[j] - h) mod n is
//      already in the order of the second half, and a stable least-significant-digit radix sort by the rank of
//      the first half (8 bits a pass, so 1..3 passes for ranks below n) finishes the round.  A pass gives every
//      wave one contiguous chunk of the list: the waves count their chunks' digits into per-wave histograms in
//      LDS, a scan over (digit, wave) turns them into places, and each wave scatters its chunk 64 entries a
//      step in order, a lane's place among the step's lanes with the same digit coming from ballots over the
//      digit's bits (bzip2_decode.hip's merged-pointer step), which keeps the pass stable.  New ranks are the
//      first place of each group of equal pairs: a flag per entry, the last flagged place carried along each
//      chunk and across the chunks.  Rounds end when every rank is its own or h reaches n: at most
//      ceil(log2 n) of them, whatever the block holds (periodic and Fibonacci-word blocks take the rounds of
//      their length, no comparison ever follows a match).  Rotations still tied then are equal, and one more
//      sort of 0..n-1 by rank puts them in index order; the start pointer is the row of rotation 0;
//   3. SERIAL, lane 0: the move-to-front list and RUNA/RUNB, from LDS tiles of the transformed bytes;
//   4. the Huffman stage: seeds on lane 0; four passes in which every lane searches its 50-symbol groups'
//      cheapest table and adds their symbols to the table's frequencies with LDS integer atomics (sums that do
//      not depend on order), the 6 x 258 sort keys are ranked one a lane, and the length allocator runs
//      SERIAL on one lane per table (six waves); canonical codes the same way;
//   5. bit writing into the slot's zeroed staging words: lane 0 writes the block's head (magic .. code
//      lengths), every lane then counts the bits of its run of groups, a scan over the lanes gives each its bit
//      position, and the lanes emit their groups side by side, OR-ing words with atomics; the staged whole bytes
//      are copied to the caller's slot (which may start at any address and is never written past out_cap),
//      and the bits of the last, incomplete byte start the next block's staging.
// Barriers are __syncthreads() of the one workgroup; no workgroup waits for another.  Every loop is bounded by
// the block length, the item length or the round bound.  Staged words are read back with agent-scope loads,
// past the vector L1, since the atomics that wrote them went to L2.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "../../include/netty_amd.h"
#include "nx_common.hpp"
#include "workspace.hpp"
#include "bzip2_encode_core.hpp"

namespace nx {
namespace bz2e {

constexpr uint32_t kThreads = 1024, kWaves = kThreads / 64u;
constexpr uint32_t kTile = 4096;  // bytes per LDS tile of the serial stages

// a stream's slot at level L (L units of kBzip2EncUnitBytes): arrays of A = the block size + 64, rounded up to 64
struct SlotLayout {
    size_t A;
    __host__ __device__ explicit SlotLayout(uint32_t level) : A(((size_t)level * kBaseBlock + 64u + 63u) / 64u * 64u) {}
    __host__ __device__ size_t blk() const { return 0; }
    __host__ __device__ size_t bwt() const { return A; }
    __host__ __device__ size_t la() const { return 2u * A; }
    __host__ __device__ size_t lb() const { return 6u * A; }
    __host__ __device__ size_t ra() const { return 10u * A; }
    __host__ __device__ size_t rb() const { return 14u * A; }
    __host__ __device__ size_t mtf() const { return 18u * A; }  // A >= n + 1 symbols of two bytes
    __host__ __device__ size_t stg() const { return 20u * A; }  // 3 A bytes
    __host__ __device__ size_t end() const { return 23u * A; }
};
constexpr size_t staged_bytes_bound(uint32_t level) { return (size_t)((block_bits_bound((uint64_t)level * kBaseBlock) + 40u) / 32u + 2u) * 4u; }
static_assert(staged_bytes_bound(1) <= 3u * 100096u && staged_bytes_bound(9) <= 3u * 900096u, "a block's bits fit the staging words");
static_assert(23u * (900000u + 128u) <= 9u * kBzip2EncUnitBytes && 23u * (100000u + 128u) <= kBzip2EncUnitBytes, "slot layout");

struct EncLds {
    uint32_t crc_table[256];
    uint32_t hist[kWaves][256];  // a radix pass's places; the lanes' bit counts in stage 5
    uint32_t dbase[256];
    uint32_t chunk_last[kWaves];
    uint32_t mail[16];
    uint8_t tile[kTile];
    Rle1 R;
    Mtf2 M;
    uint8_t lens[kMaxTables][kMaxAlpha];
    uint32_t codes[kMaxTables][kMaxAlpha];
    uint32_t tfreq[kMaxTables][kMaxAlpha];
    int32_t merged[kMaxTables][kMaxAlpha], sorted[kMaxTables][kMaxAlpha];
    uint8_t sel[kMaxSelectors + 2];
};
static_assert(kThreads * 2u <= kWaves * 256u, "the lanes' 64-bit bit counts fit hist");

constexpr uint32_t kNone = 0xffffffffu;
__device__ __forceinline__ uint32_t load_l2(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

struct Chunk {
    uint32_t c0, c1;
};
__device__ __forceinline__ Chunk wave_chunk(uint32_t n, uint32_t wave) {
    const uint32_t per = ((n + kWaves - 1u) / kWaves + 63u) / 64u * 64u;
    const uint32_t c0 = wave * per < n ? wave * per : n;
    return {c0, c0 + per < n ? c0 + per : n};
}

// dst = src in the order of (key[src[j]] >> shift) & 255, stable.  Ends with a barrier.
__device__ void radix_pass(EncLds& L, const uint32_t* src, uint32_t* dst, const uint32_t* key, uint32_t shift, uint32_t n) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const Chunk c = wave_chunk(n, wave);
    for (uint32_t k = tid; k < kWaves * 256u; k += kThreads) (&L.hist[0][0])[k] = 0;
    __syncthreads();
    for (uint32_t j = c.c0 + lane; j < c.c1; j += 64u) atomicAdd(&L.hist[wave][(key[src[j]] >> shift) & 255u], 1u);
    __syncthreads();
    if (tid < 256u) {  // a digit's places: the waves' chunks in order
        uint32_t acc = 0;
        for (uint32_t w = 0; w < kWaves; ++w) {
            const uint32_t t = L.hist[w][tid];
            L.hist[w][tid] = acc;
            acc += t;
        }
        L.dbase[tid] = acc;
    }
    __syncthreads();
    if (tid == 0u) {
        uint32_t acc = 0;
        for (uint32_t d = 0; d < 256u; ++d) {
            const uint32_t t = L.dbase[d];
            L.dbase[d] = acc;
            acc += t;
        }
    }
    __syncthreads();
    for (uint32_t j0 = c.c0; j0 < c.c1; j0 += 64u) {  // uniform in the wave
        const uint32_t j = j0 + lane;
        const bool on = j < c.c1;
        const uint32_t v = on ? src[j] : 0u;
        const uint32_t d = on ? (key[v] >> shift) & 255u : 0u;
        uint64_t same = __ballot(on);
#pragma unroll
        for (uint32_t bit = 0; bit < 8u; ++bit) {
            const bool one = (d >> bit) & 1u;
            const uint64_t ones = __ballot(on && one);
            same &= one ? ones : ~ones;
        }
        const uint32_t rank = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
        const uint32_t at = on ? L.hist[wave][d] + L.dbase[d] : 0u;  // at + rank < n: the places count these digits
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (on && rank == 0u) L.hist[wave][d] += (uint32_t)__popcll(same);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (on) dst[at + rank] = v;
    }
    __syncthreads();
}

// nr[sa[j]] = the first place of sa[j]'s group (equal key, and with h equal key at distance h); tmp[0, n) is
// scratch.  Returns the number of groups.  Ends with a barrier.
__device__ uint32_t rerank(EncLds& L, const uint32_t* sa, const uint32_t* key, uint32_t* nr, uint32_t* tmp, uint32_t h, uint32_t n) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const Chunk c = wave_chunk(n, wave);
    if (tid == 0u) L.mail[8] = 0;
    __syncthreads();
    uint32_t carry = kNone, heads = 0;
    for (uint32_t j0 = c.c0; j0 < c.c1; j0 += 64u) {
        const uint32_t j = j0 + lane;
        const bool on = j < c.c1;
        bool flag = false;
        if (on) {
            const uint32_t a = sa[j], b = j ? sa[j - 1u] : 0u;
            flag = j == 0u || key[a] != key[b];
            if (!flag && h) {
                const uint32_t a2 = a + h >= n ? a + h - n : a + h, b2 = b + h >= n ? b + h - n : b + h;
                flag = key[a2] != key[b2];
            }
        }
        const uint64_t F = __ballot(flag);
        const uint64_t below = F & (lane == 63u ? ~0ull : ((2ull << lane) - 1ull));  // flags at or before this lane
        const uint32_t head = below ? j0 + 63u - (uint32_t)__clzll(below) : carry;
        if (on) tmp[j] = head;
        if (F) carry = j0 + 63u - (uint32_t)__clzll(F);
        heads += (uint32_t)__popcll(F);
    }
    if (lane == 0u) {
        L.chunk_last[wave] = carry;
        atomicAdd(&L.mail[8], heads);
    }
    __syncthreads();
    uint32_t before = kNone;  // the last head of the chunks before this one (place 0 is a head)
    for (uint32_t w = 0; w < wave; ++w) before = L.chunk_last[w] != kNone ? L.chunk_last[w] : before;
    for (uint32_t j = c.c0 + lane; j < c.c1; j += 64u) {
        const uint32_t hd = tmp[j];  // this lane's own store
        nr[sa[j]] = hd != kNone ? hd : before;
    }
    const uint32_t groups = L.mail[8];
    __syncthreads();
    return groups;
}

// Stage 2.  bwt[0, n) = the last column of the sorted rotations of blk[0, n); returns the row of rotation 0.
__device__ uint32_t block_sort(EncLds& L, const uint8_t* blk, uint8_t* bwt, uint32_t* la, uint32_t* lb, uint32_t* ra, uint32_t* rb,
                               uint32_t n) {
    const uint32_t tid = threadIdx.x;
    uint32_t *src = la, *dst = lb, *rk = ra, *nr = rb;
    const uint32_t passes = n <= 256u ? 1u : n <= 65536u ? 2u : 3u;
    for (uint32_t i = tid; i < n; i += kThreads) {
        src[i] = i;
        rk[i] = ((uint32_t)blk[i] << 8) | blk[i + 1u == n ? 0u : i + 1u];
    }
    __syncthreads();
    for (uint32_t p = 0; p < 2u; ++p) {
        radix_pass(L, src, dst, rk, 8u * p, n);
        uint32_t* t = src;
        src = dst;
        dst = t;
    }
    uint32_t groups = rerank(L, src, rk, nr, dst, 0, n);
    {
        uint32_t* t = rk;
        rk = nr;
        nr = t;
    }
    for (uint32_t h = 2; groups < n && h < n; h *= 2u) {  // at most ceil(log2 n) rounds
        for (uint32_t j = tid; j < n; j += kThreads) {
            const uint32_t v = src[j];
            dst[j] = v >= h ? v - h : v + n - h;
        }
        __syncthreads();
        uint32_t* t = src;
        src = dst;
        dst = t;
        for (uint32_t p = 0; p < passes; ++p) {
            radix_pass(L, src, dst, rk, 8u * p, n);
            t = src;
            src = dst;
            dst = t;
        }
        groups = rerank(L, src, rk, nr, dst, h, n);
        t = rk;
        rk = nr;
        nr = t;
    }
    if (groups < n) {  // equal rotations: by index
        for (uint32_t i = tid; i < n; i += kThreads) src[i] = i;
        __syncthreads();
        for (uint32_t p = 0; p < passes; ++p) {
            radix_pass(L, src, dst, rk, 8u * p, n);
            uint32_t* t = src;
            src = dst;
            dst = t;
        }
    }
    for (uint32_t j = tid; j < n; j += kThreads) {
        const uint32_t v = src[j];
        bwt[j] = blk[v ? v - 1u : n - 1u];
        if (v == 0u) L.mail[9] = j;
    }
    __syncthreads();
    return L.mail[9];
}

// Stage 4: L.lens, L.codes and L.sel from the symbols; returns the table count.
__device__ uint32_t huffman_tables(EncLds& L, const uint16_t* mtf, uint32_t mtf_len, uint32_t alpha) {
    const uint32_t tid = threadIdx.x;
    const uint32_t tables = select_table_count(mtf_len), groups = (mtf_len + kGroup - 1u) / kGroup;
    if (tid == 0u) huffman_seeds(L.lens, L.M.freq, alpha, mtf_len, tables);
    for (uint32_t pass = 0; pass < kPasses; ++pass) {
        for (uint32_t k = tid; k < kMaxTables * kMaxAlpha; k += kThreads) (&L.tfreq[0][0])[k] = 0;
        __syncthreads();
        for (uint32_t g = tid; g < groups; g += kThreads) {
            const uint32_t s = g * kGroup, cnt = mtf_len - s < kGroup ? mtf_len - s : kGroup;
            const uint32_t best = group_best_table(L.lens, mtf + s, cnt, tables);
            for (uint32_t i = 0; i < cnt; ++i) atomicAdd(&L.tfreq[best][mtf[s + i]], 1u);
            L.sel[g] = (uint8_t)best;  // the last pass's stay
        }
        __syncthreads();
        for (uint32_t k = tid; k < tables * alpha; k += kThreads) {
            const uint32_t t = k / alpha;
            lengths_sort_one(L.tfreq[t], alpha, k - t * alpha, L.merged[t], L.sorted[t]);
        }
        __syncthreads();
        if ((tid & 63u) == 0u && (tid >> 6) < tables) ha_allocate(L.sorted[tid >> 6], (int32_t)alpha, (int32_t)kEncMaxCodeLen);
        __syncthreads();
        for (uint32_t k = tid; k < tables * alpha; k += kThreads) {
            const uint32_t t = k / alpha;
            lengths_unsort_one(L.merged[t], L.sorted[t], k - t * alpha, L.lens[t]);
        }
        __syncthreads();
    }
    if ((tid & 63u) == 0u && (tid >> 6) < tables) assign_codes(L.lens[tid >> 6], alpha, L.codes[tid >> 6]);
    __syncthreads();
    return tables;
}

// What is staged so far, to the output.  mail[0..2]: the carried bits, their count, and whether the stream
// header is still to be written; mail[3]: the status.  Uniform.
struct Out {
    uint8_t* p;
    uint32_t cap, pos;
};
// zero the first `words` staging words, then lane 0 starts a writer over them with the header or the carried bits
__device__ void begin_piece(EncLds& L, uint32_t* stg, size_t words, uint32_t level, BitWriter& b) {
    for (size_t k = threadIdx.x; k < words; k += kThreads) stg[k] = 0;
    __syncthreads();
    if (threadIdx.x == 0u) {
        bw_init(b, stg, 0);
        if (L.mail[2]) {
            bw_put(b, 24, 0x425a68u);  // "BZh" (Bzip2Encoder.java:115-117)
            bw_put(b, 8, '0' + level);
            L.mail[2] = 0;
        }
        bw_put(b, L.mail[1], L.mail[0]);
    }
}
// the whole bytes of `bits` staged bits (all of them, zero-padded, when last) to the output; the rest is carried
__device__ int32_t end_piece(EncLds& L, const uint32_t* stg, Out& O, uint64_t bits, bool last) {
    const uint32_t bytes = last ? (uint32_t)((bits + 7u) / 8u) : (uint32_t)(bits / 8u);
    __syncthreads();  // the writers' atomics have been issued; an atomic load of a word comes after them at L2
    if (bytes > O.cap - O.pos) return NX_ERR_BZIP2_ENCODE_FULL;
    for (uint32_t w = threadIdx.x; w * 4u < bytes; w += kThreads) {
        const uint32_t v = load_l2(stg + w);
        for (uint32_t k = 0; k < 4u && w * 4u + k < bytes; ++k) O.p[O.pos + w * 4u + k] = (uint8_t)(v >> (8u * k));
    }
    if (threadIdx.x == 0u) {
        const uint32_t cn = last ? 0u : (uint32_t)(bits & 7u);
        L.mail[1] = cn;
        L.mail[0] = cn ? ((load_l2(stg + bytes / 4u) >> (8u * (bytes & 3u))) & 0xffu) >> (8u - cn) : 0u;
    }
    O.pos += bytes;
    __syncthreads();
    return NX_OK;
}

// Bzip2BlockCompressor.close for the block lane 0 has filled (L.R, blk).
__device__ int32_t encode_block(EncLds& L, uint8_t* slot, const SlotLayout& S, uint32_t level, Out& O, uint32_t* crc_out) {
    const uint32_t tid = threadIdx.x;
    uint8_t* blk = slot + S.blk();
    uint8_t* bwt = slot + S.bwt();
    uint16_t* mtf = reinterpret_cast<uint16_t*>(slot + S.mtf());
    uint32_t* stg = reinterpret_cast<uint32_t*>(slot + S.stg());
    if (tid == 0u) rle1_close(L.R, blk, L.crc_table);
    __syncthreads();
    const uint32_t n = L.R.len, crc = ~L.R.crc;
    const uint32_t start = block_sort(L, blk, bwt, reinterpret_cast<uint32_t*>(slot + S.la()), reinterpret_cast<uint32_t*>(slot + S.lb()),
                                      reinterpret_cast<uint32_t*>(slot + S.ra()), reinterpret_cast<uint32_t*>(slot + S.rb()), n);
#ifdef NX_BZIP2_ENC_SORT_ONLY  // build option (scripts/build_lib_variant.sh): stop after the sort, to time it alone
    *crc_out = crc + start;
    return NX_OK;
#endif
    // 3: move-to-front and the run symbols
    if (tid == 0u) mtf2_init(L.M, L.R.present);
    for (uint32_t i0 = 0; i0 < n; i0 += kTile) {
        const uint32_t m = n - i0 < kTile ? n - i0 : kTile;
        __syncthreads();
        for (uint32_t k = tid; k < m; k += kThreads) L.tile[k] = bwt[i0 + k];
        __syncthreads();
        if (tid == 0u) mtf2_step(L.M, L.tile, m, mtf);
    }
    if (tid == 0u) L.mail[10] = mtf2_finish(L.M, mtf);
    __syncthreads();
    const uint32_t mtf_len = L.mail[10], alpha = L.M.eob + 1u, groups = (mtf_len + kGroup - 1u) / kGroup;
    // 4
    const uint32_t tables = huffman_tables(L, mtf, mtf_len, alpha);
    // 5
    BitWriter b;
    begin_piece(L, stg, (size_t)((block_bits_bound(n) + 40u) / 32u + 2u), level, b);
    if (tid == 0u) {
        write_block_head(b, crc, start, L.R.present, tables, L.sel, groups, L.lens, alpha);
        bw_flush(b);
        L.mail[11] = (uint32_t)bw_bits(b);  // below 2^32: a block's head is a few tens of kilobytes
    }
    uint64_t* part = reinterpret_cast<uint64_t*>(&L.hist[0][0]);
    const uint32_t per = (groups + kThreads - 1u) / kThreads;  // a lane's run of groups
    const uint32_t g0 = tid * per < groups ? tid * per : groups, g1 = g0 + per < groups ? g0 + per : groups;
    part[tid] = emit_groups(nullptr, mtf, mtf_len, L.sel, L.codes, g0, g1);
    __syncthreads();
    if (tid == 0u) {
        uint64_t acc = L.mail[11];
        for (uint32_t t = 0; t < kThreads; ++t) {
            const uint64_t v = part[t];
            part[t] = acc;
            acc += v;
        }
        L.mail[12] = (uint32_t)acc;
        L.mail[13] = (uint32_t)(acc >> 32);
    }
    __syncthreads();
    if (g0 < g1) {
        BitWriter e;
        bw_init(e, stg, part[tid]);
        emit_groups(&e, mtf, mtf_len, L.sel, L.codes, g0, g1);
        bw_flush(e);
    }
    *crc_out = crc;
    const uint64_t bits = ((uint64_t)L.mail[13] << 32) | L.mail[12];
    return end_piece(L, stg, O, bits, false);
}

__device__ void encode_stream(EncLds& L, const uint8_t* in, uint32_t len, uint8_t* slot, const SlotLayout& S, uint32_t level, Out& O,
                              uint32_t* out_len, int32_t* status) {
    const uint32_t tid = threadIdx.x;
    uint8_t* blk = slot + S.blk();
    uint32_t* stg = reinterpret_cast<uint32_t*>(slot + S.stg());
    __syncthreads();
    if (tid == 0u) {
        L.mail[0] = 0;
        L.mail[1] = 0;
        L.mail[2] = 1;
        rle1_init(L.R, level * kBaseBlock);
    }
    uint32_t stream_crc = 0, pos = 0;
    int32_t st = NX_OK;
    // 1: Bzip2Encoder.java:112-148; every pass takes input bytes or closes a block that holds some
    for (;;) {
        const uint32_t m = len - pos < kTile ? len - pos : kTile;
        __syncthreads();
        for (uint32_t k = tid; k < m; k += kThreads) L.tile[k] = in[pos + k];
        __syncthreads();
        if (tid == 0u) {
            uint32_t used = 0;
            while (used < m && rle1_write(L.R, blk, L.crc_table, L.tile[used])) used += 1u;
            L.mail[4] = used;
            L.mail[5] = rle1_empty(L.R) ? 0u : 1u;
        }
        __syncthreads();
        const uint32_t used = L.mail[4];
        pos += used;
        if (used == m && pos < len) continue;  // the tile went in whole and there is more
        if (L.mail[5]) {                       // the block refused a byte, or the input has ended: Bzip2Encoder.java:154-161
            uint32_t crc = 0;
            st = encode_block(L, slot, S, level, O, &crc);
            if (st != NX_OK) break;
            stream_crc = bz2d::crc_combine_stream(stream_crc, crc);
            if (tid == 0u) rle1_init(L.R, level * kBaseBlock);
        }
        if (pos == len) break;
    }
    if (st == NX_OK) {  // Bzip2Encoder.java:220-223
        BitWriter b;
        begin_piece(L, stg, 8, level, b);
        uint64_t bits = 0;
        if (tid == 0u) {
            bw_put(b, 24, bz2d::kEndMagicHi);
            bw_put(b, 24, bz2d::kEndMagicLo);
            bw_put(b, 32, stream_crc);
            bw_flush(b);
            L.mail[12] = (uint32_t)bw_bits(b);
        }
        __syncthreads();
        bits = L.mail[12];
        st = end_piece(L, stg, O, bits, true);
    }
    if (tid == 0u) {
        *out_len = st == NX_OK ? O.pos : 0u;
        *status = st;
    }
}

__global__ void __launch_bounds__(kThreads) k_bzip2_encode(const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off,
                                                           const uint32_t* __restrict__ in_len, uint8_t* out,
                                                           const uint64_t* __restrict__ out_off, const uint32_t* __restrict__ out_cap,
                                                           uint8_t* ws, uint32_t* out_len, int32_t* status, uint32_t n, uint32_t level) {
    __shared__ EncLds L;
    const SlotLayout S(level);
    uint8_t* slot = ws + (size_t)blockIdx.x * level * kBzip2EncUnitBytes;
    for (uint32_t i = threadIdx.x; i < 256u; i += kThreads) L.crc_table[i] = bz2d::crc_table_entry(i);
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        Out O = {out + out_off[i], out_cap[i], 0};
        encode_stream(L, in + in_off[i], in_len[i], slot, S, level, O, out_len + i, status + i);
        __syncthreads();
    }
}

}  // namespace bz2e
}  // namespace nx

extern "C" uint64_t nx_bzip2_encoder_slot_bytes(int32_t level) { return level < 1 || level > 9 ? 0u : (uint64_t)level * nx::kBzip2EncUnitBytes; }

extern "C" int32_t nx_bzip2_encode_batch(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint8_t* out,
                                         const uint64_t* out_off, const uint32_t* out_cap, uint32_t* out_len, int32_t* status, uint32_t n,
                                         int32_t level, void* stream) {
    if (level < 1 || level > 9) return NX_ERR_BZIP2_LEVEL;  // Bzip2Encoder.java:98-101
    if (n == 0) return NX_OK;
    if (!in || !in_off || !in_len || !out || !out_off || !out_cap || !out_len || !status) return NX_ERR_INVALID_ARG;
    NX_CLEAR_STALE_ERROR();
    int dev = 0, cus = 256;
    NX_HIP_CHECK(hipGetDevice(&dev));
    NX_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    hipStream_t st = (hipStream_t)stream;
    nx::WsLease lease(nx::WsKind::Bzip2Enc, dev, st);
    // the workspace counts units of one level's worth; a stream takes `level` of them, one workgroup per CU
    const size_t streams = std::min<size_t>(n, (size_t)cus * nx::kBzip2EncGroupsPerCu);
    nx::SharedWs& W = lease.ws();
    if (W.cap && W.cap < (size_t)level) W.cap = (size_t)level;  // a reserve at a lower level: room for one stream of this one
    size_t first = 0, count = 0;
    NX_HIP_CHECK(lease.acquire_part(streams * (size_t)level, &first, &count));
    if (count < (size_t)level) return NX_ERR_INVALID_ARG;  // a workspace its owner holds below one slot of this level
    uint8_t* ws = static_cast<uint8_t*>(W.p) + first * nx::kBzip2EncUnitBytes;
    hipLaunchKernelGGL(nx::bz2e::k_bzip2_encode, dim3((unsigned)(count / (size_t)level)), dim3(nx::bz2e::kThreads), 0, st, in, in_off, in_len,
                       out, out_off, out_cap, ws, out_len, status, n, (uint32_t)level);
    NX_HIP_CHECK(hipGetLastError());
    return NX_OK;
}

// Size the workspace now: slots for max_streams streams in flight at `level`, and never more until
// nx_workspaces_trim; a batch of more streams runs on those slots, a workgroup taking several streams in turn.
extern "C" int32_t nx_bzip2_encoder_reserve(uint32_t max_streams, int32_t level, void* stream) {
    if (level < 1 || level > 9) return NX_ERR_BZIP2_LEVEL;
    if (max_streams == 0 || max_streams > 0xffffffffu / 9u) return NX_ERR_INVALID_ARG;
    const uint32_t units = max_streams * (uint32_t)level;
    int dev = 0;
    NX_HIP_CHECK(hipGetDevice(&dev));
    nx::SharedWs& W = nx::shared_ws(nx::WsKind::Bzip2Enc, dev);
    {
        std::lock_guard<std::mutex> lk(W.mu);
        if (W.p && W.slots > units) return NX_ERR_INVALID_ARG;  // already larger than the cap: trim first
        W.cap = units;
    }
    const int32_t r = nx::ws_hold(nx::WsKind::Bzip2Enc, dev, units, (hipStream_t)stream);
    if (r != NX_OK) return r;
    {
        std::lock_guard<std::mutex> lk(W.mu);
        W.kept = true;
    }
    nx::ws_unhold(nx::WsKind::Bzip2Enc, dev);
    return NX_OK;
}
