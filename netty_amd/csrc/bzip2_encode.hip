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

// Bzip2BlockCompressor.close for the block lane 0 has filled (L.R, blk), up to its bits in the staging words
// (behind the header or the carried bits that begin_piece finds in the mail); returns the staged bits.
__device__ uint64_t stage_block(EncLds& L, uint8_t* slot, const SlotLayout& S, uint32_t level, uint32_t* crc_out) {
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
    return 0;
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
    return ((uint64_t)L.mail[13] << 32) | L.mail[12];
}
__device__ int32_t encode_block(EncLds& L, uint8_t* slot, const SlotLayout& S, uint32_t level, Out& O, uint32_t* crc_out) {
    const uint64_t bits = stage_block(L, slot, S, level, crc_out);
#ifdef NX_BZIP2_ENC_SORT_ONLY
    return NX_OK;
#endif
    return end_piece(L, reinterpret_cast<const uint32_t*>(slot + S.stg()), O, bits, false);
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

// ------------------------------------------------------------------ the split path (nx_bzip2_encode_batch_split)
// A stream's blocks are independent once their cut points are known, apart from the bit offset where each one
// lands.  k_bzip2_plan finds the cuts (twice: once to count every item's blocks, and after k_bzip2_plan_scan has
// turned the counts into each item's first job, once more to write the job list); k_bzip2_encode_blocks encodes
// a round of jobs, one workgroup and one workspace slot each, from bit 0 of the slot's staging;
// k_bzip2_splice gathers the round's staged bits into the callers' slots and carries each stream's bit position,
// sub-word carry, CRC and status to the next round in ItemSt.  The launches are ordered by the one stream; no
// workgroup waits for another, and every loop is bounded by an item's length, a round's jobs or the item count.
struct ItemSt {  // per item, in the call's plan arrays
    uint32_t cnt, first;  // its blocks, and the job index of the first (saturated)
    uint32_t pos;         // bytes of its output slot written so far
    uint32_t carry, carry_n;  // the bits, fewer than 32, that follow them
    uint32_t crc;             // the stream CRC over the blocks spliced so far
    int32_t status;
    uint32_t flags;  // NX_BZIP2_SEG_*
};
struct Job {
    uint32_t item, begin, end;  // the block's input range in its item
    uint32_t bits, crc;         // of the encoded block
    int32_t status;
    uint32_t pad[2];
};
static_assert(sizeof(ItemSt) == 32 && sizeof(Job) == 32, "the plan arrays' layout");
constexpr uint32_t kMaxRound = 1024;  // jobs per round, at most: k_bzip2_splice's list of parts is in LDS
constexpr uint32_t kPlanStep = 64;    // bytes the planner's wave takes at a time
// A step of kPlanStep bytes grows the block by at most 5 (the pending run) + 5 for every 4 bytes: while the
// block stays this far below its limit no byte of the step can fill it.
constexpr uint32_t kPlanMargin = 5u + 5u * (kPlanStep / 4u) + 11u;

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (uint32_t d = 32; d > 0u; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// One wave per item.  The state (plan_byte's) is uniform.  Far from the block's limit a step is counted
// wave-wide: a lane that starts a run adds the bytes of the run that ended before it (5 for every 255 of its
// length and plan_run_bytes of the rest, the pending run included when it reaches back before the step), and
// the step's last run stays pending modulo 255.  Near the limit the step's bytes go through plan_byte one at a
// time, every lane alike, and a full block is closed where the reference closes it.
template <bool kWrite>
__global__ void __launch_bounds__(64) k_bzip2_plan(const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off,
                                                  const uint32_t* __restrict__ in_len, ItemSt* items, Job* jobs, uint32_t level,
                                                  uint32_t max_blocks) {
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    const uint8_t* p = in + in_off[i];
    const uint32_t len = in_len[i], limit = level * kBaseBlock - 6u;
    const uint32_t first = kWrite ? items[i].first : 0u;
    Plan P;
    plan_init(P);
    uint32_t count = 0, begin = 0;
    auto cut = [&](uint32_t end) {
        if (kWrite && lane == 0u && (uint64_t)first + count < max_blocks) {
            Job& J = jobs[first + count];
            J.item = i;
            J.begin = begin;
            J.end = end;
            J.bits = 0;
            J.crc = 0;
            J.status = NX_OK;
        }
        count += 1u;
        begin = end;
        plan_init(P);
    };
    for (uint32_t pos = 0; pos < len; pos += kPlanStep) {
        const uint32_t m = len - pos < kPlanStep ? len - pos : kPlanStep;
        const bool on = lane < m;
        const uint32_t v = on ? p[pos + lane] : 0u;
        if (P.len + kPlanMargin <= limit) {
            const uint32_t prev = __shfl_up(v, 1);
            const bool head = on && (lane == 0u ? (P.run == 0u || v != P.cur) : v != prev);
            const uint64_t H = __ballot(head);
            const uint64_t below = H & ((1ull << lane) - 1ull);
            const uint32_t r = below ? lane - (63u - (uint32_t)__clzll(below)) : P.run + lane;
            const uint32_t add = wave_sum(head ? 5u * (r / 255u) + plan_run_bytes(r % 255u) : 0u);
            const uint32_t tail = H ? m - (63u - (uint32_t)__clzll(H)) : P.run + m;
            P.len += add + 5u * (tail / 255u);
            P.run = tail % 255u;
            P.cur = __shfl(v, m - 1u);
        } else {
            for (uint32_t k = 0; k < m; ++k) {
                plan_byte(P, __shfl(v, k));
                if (plan_full(P, limit)) cut(pos + k + 1u);
            }
        }
    }
    if (!plan_empty(P)) cut(len);
    if (!kWrite && lane == 0u) items[i].cnt = count;
}

// One workgroup: every item's first job from the counts, its state from its segment, and the jobs listed.
__global__ void __launch_bounds__(kThreads) k_bzip2_plan_scan(ItemSt* items, uint32_t* njobs, const nx_bzip2_seg* seg, uint32_t* out_len,
                                                              int32_t* status, uint32_t n, uint32_t max_blocks) {
    __shared__ uint64_t wsum[kWaves];
    __shared__ uint64_t total;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (tid == 0u) total = 0;
    __syncthreads();
    for (uint32_t base = 0; base < n; base += kThreads) {
        const uint32_t i = base + tid;
        const uint32_t c = i < n ? items[i].cnt : 0u;
        uint64_t x = c;  // inclusive over the wave
#pragma unroll
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint32_t lo = __shfl_up((uint32_t)x, d), hi = __shfl_up((uint32_t)(x >> 32), d);
            if (lane >= d) x += ((uint64_t)hi << 32) | lo;
        }
        if (lane == 63u) wsum[wave] = x;
        __syncthreads();
        uint64_t before = total;
        for (uint32_t w = 0; w < wave; ++w) before += wsum[w];
        if (i < n) {
            const uint64_t f = before + x - c;
            ItemSt& I = items[i];
            const bool fits = c == 0u || f + c <= max_blocks;  // an item without blocks lists none
            const uint32_t flags = seg ? seg[i].flags : (NX_BZIP2_SEG_FIRST | NX_BZIP2_SEG_LAST);
            const bool cont = seg && !(flags & NX_BZIP2_SEG_FIRST);
            I.first = f < 0xffffffffull ? (uint32_t)f : 0xffffffffu;
            I.pos = 0;
            I.carry = cont ? seg[i].carry_bits : 0u;
            I.carry_n = cont ? seg[i].carry_count : 0u;
            I.crc = cont ? seg[i].crc : 0u;
            I.flags = flags;
            I.status = !fits ? NX_ERR_BZIP2_ENCODE_BLOCKS : I.carry_n >= 32u ? NX_ERR_INVALID_ARG : NX_OK;
            out_len[i] = 0;
            status[i] = I.status;
        }
        __syncthreads();
        if (tid == kThreads - 1u) total = before + x;
        __syncthreads();
    }
    if (tid == 0u) *njobs = total < max_blocks ? (uint32_t)total : max_blocks;
}

// One workgroup per job of the round: block `base_job + blockIdx.x` of the list, in slot blockIdx.x.
__global__ void __launch_bounds__(kThreads) k_bzip2_encode_blocks(const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off,
                                                                  const ItemSt* items, Job* jobs, const uint32_t* njobs, uint8_t* ws,
                                                                  uint32_t base_job, uint32_t level) {
    __shared__ EncLds L;
    const uint32_t tid = threadIdx.x, job = base_job + blockIdx.x;
    if (job >= *njobs) return;
    Job& J = jobs[job];
    if (items[J.item].status != NX_OK) return;  // the item has failed: the splice passes it over
    const SlotLayout S(level);
    uint8_t* slot = ws + (size_t)blockIdx.x * level * kBzip2EncUnitBytes;
    uint8_t* blk = slot + S.blk();
    const uint8_t* src = in + in_off[J.item];
    const uint32_t begin = J.begin, end = J.end;
    for (uint32_t k = tid; k < 256u; k += kThreads) L.crc_table[k] = bz2d::crc_table_entry(k);
    if (tid == 0u) {
        L.mail[0] = L.mail[1] = L.mail[2] = 0;  // no header, nothing carried: the block starts at bit 0
        L.mail[6] = 0;
        rle1_init(L.R, level * kBaseBlock);
    }
    // 1: the job's range goes in whole and closes as one block, or the plan and the block filler disagree
    for (uint32_t pos = begin; pos < end; pos += kTile) {
        const uint32_t m = end - pos < kTile ? end - pos : kTile;
        __syncthreads();
        for (uint32_t k = tid; k < m; k += kThreads) L.tile[k] = src[pos + k];
        __syncthreads();
        if (tid == 0u && L.mail[6] == 0u) {
            uint32_t used = 0;
            while (used < m && rle1_write(L.R, blk, L.crc_table, L.tile[used])) used += 1u;
            if (used < m) L.mail[6] = 1;
        }
    }
    __syncthreads();
    if (L.mail[6] || rle1_empty(L.R)) {
        if (tid == 0u) J.status = NX_ERR_INTERNAL;
        return;
    }
    uint32_t crc = 0;
    const uint64_t bits = stage_block(L, slot, S, level, &crc);
    if (tid == 0u) {
        J.bits = (uint32_t)bits;  // below 2^32: block_bits_bound of 900 000 bytes
        J.crc = crc;
    }
}

// One workgroup per item: the item's blocks of this round, behind the carried bits (or the stream header) and,
// when the stream ends here, before the footer, gathered into the item's output slot.  Lane 0 lists the parts
// and their destination bits in LDS; every lane then makes whole destination bytes from one or two parts
// (splice_source) and stores each once.  Staged words are read with agent-scope loads, as end_piece reads them.
__global__ void __launch_bounds__(kThreads) k_bzip2_splice(ItemSt* items, const Job* jobs, const uint32_t* njobs, const uint8_t* ws, uint8_t* out,
                                                           const uint64_t* __restrict__ out_off, const uint32_t* __restrict__ out_cap,
                                                           uint32_t* out_len, int32_t* status, nx_bzip2_seg* seg, uint32_t level,
                                                           uint32_t base_job, uint32_t round_jobs) {
    constexpr uint16_t kHead = 0xfffe, kFoot = 0xffff;
    __shared__ uint64_t start[kMaxRound + 3];
    __shared__ uint16_t kind[kMaxRound + 2];
    __shared__ uint32_t head_bytes[2], foot_bytes[3];  // the bytes in order, as the staging words hold them
    __shared__ uint32_t sh_parts, sh_bytes, sh_crc;
    __shared__ int32_t sh_status;
    const uint32_t i = blockIdx.x, tid = threadIdx.x;
    ItemSt& I = items[i];
    const uint64_t first = I.first, cnt = I.cnt, lo = base_job, hi = (uint64_t)base_job + round_jobs;
    const uint64_t listed = *njobs;
    const bool starts = cnt ? (first >= lo && first < hi) : base_job == 0u;
    const bool finishes = cnt ? (first + cnt - 1u >= lo && first + cnt - 1u < hi) : base_job == 0u;
    const uint64_t j0 = first > lo ? first : lo, j1e = first + cnt < hi ? first + cnt : hi, j1 = j1e < listed ? j1e : listed;
    if (!starts && !finishes && j1 <= j0) return;
    if (I.status != NX_OK) return;  // reported when it failed
    const uint32_t pos = I.pos, flags = I.flags;
    const bool fin = finishes && (flags & NX_BZIP2_SEG_LAST);
    const SlotLayout S(level);
    if (tid == 0u) {
        const bool header = starts && (flags & NX_BZIP2_SEG_FIRST);
        const uint32_t hn = header ? 32u : I.carry_n, hv = header ? (0x425a6800u | ('0' + level)) : I.carry;
        uint32_t k = 0, crc = I.crc;
        uint64_t bit = 0;
        int32_t st = NX_OK;
        if (hn) {
            head_bytes[0] = __builtin_bswap32(hv << (32u - hn));
            head_bytes[1] = 0;
            kind[k] = kHead;
            start[k++] = 0;
            bit = hn;
        }
        for (uint64_t j = j0; j < j1; ++j) {  // at most round_jobs <= kMaxRound
            const Job& J = jobs[j];
            if (J.status != NX_OK && st == NX_OK) st = J.status;
            kind[k] = (uint16_t)(j - lo);
            start[k++] = bit;
            bit += J.bits;
            crc = bz2d::crc_combine_stream(crc, J.crc);
        }
        if (fin) {  // Bzip2Encoder.java:220-223
            foot_bytes[0] = __builtin_bswap32((bz2d::kEndMagicHi << 8) | (bz2d::kEndMagicLo >> 16));
            foot_bytes[1] = __builtin_bswap32((bz2d::kEndMagicLo << 16) | (crc >> 16));
            foot_bytes[2] = __builtin_bswap32(crc << 16);
            kind[k] = kFoot;
            start[k++] = bit;
            bit += 80u;
        }
        start[k] = bit;
        const uint64_t bytes = fin ? (bit + 7u) / 8u : bit / 32u * 4u;
        if (st == NX_OK && bytes > out_cap[i] - pos) st = NX_ERR_BZIP2_ENCODE_FULL;
        sh_parts = k;
        sh_bytes = st == NX_OK ? (uint32_t)bytes : 0u;
        sh_crc = crc;
        sh_status = st;
    }
    __syncthreads();
    const uint32_t parts = sh_parts, bytes = sh_bytes;
    if (sh_status != NX_OK) {
        if (tid == 0u) {
            I.status = sh_status;
            out_len[i] = 0;
            status[i] = sh_status;
        }
        return;
    }
    auto part_byte = [&](uint32_t part, uint64_t b) -> uint32_t {
        const uint16_t kd = kind[part];
        if (kd == kHead) return b < 8u ? (head_bytes[b >> 2] >> (8u * (b & 3u))) & 0xffu : 0u;
        if (kd == kFoot) return b < 12u ? (foot_bytes[b >> 2] >> (8u * (b & 3u))) & 0xffu : 0u;
        const uint32_t* stg = reinterpret_cast<const uint32_t*>(ws + (size_t)kd * level * kBzip2EncUnitBytes + S.stg());
        return (load_l2(stg + (b >> 2)) >> (8u * (b & 3u))) & 0xffu;
    };
    auto gather = [&](uint64_t byte) -> uint32_t {
        if (parts == 0u) return 0u;
        const SpliceSrc s = splice_source(start, parts, byte);
        if (s.part >= parts) return 0u;
        uint32_t v = splice_read8([&](uint64_t b) { return part_byte(s.part, b); }, s.off);
        if (s.have < 8u && s.part + 1u < parts) v |= splice_read8([&](uint64_t b) { return part_byte(s.part + 1u, b); }, 0) >> s.have;
        return v;
    };
    uint8_t* dst = out + out_off[i] + pos;
    for (uint32_t b = tid; b < bytes; b += kThreads) dst[b] = (uint8_t)gather(b);
    if (tid == 0u) {
        const uint32_t cn = fin ? 0u : (uint32_t)(start[parts] - (uint64_t)bytes * 8u);  // below 32
        const uint32_t w = (gather(bytes) << 24) | (gather(bytes + 1ull) << 16) | (gather(bytes + 2ull) << 8) | gather(bytes + 3ull);
        const uint32_t carry = cn ? w >> (32u - cn) : 0u;
        I.pos = pos + bytes;
        I.carry = carry;
        I.carry_n = cn;
        I.crc = sh_crc;
        if (finishes) {
            out_len[i] = pos + bytes;
            status[i] = NX_OK;
            if (seg) {
                seg[i].carry_bits = carry;
                seg[i].carry_count = cn;
                seg[i].crc = sh_crc;
            }
        }
    }
}

}  // namespace bz2e
}  // namespace nx

extern "C" int32_t nx_bzip2_encode_batch_split(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint8_t* out,
                                               const uint64_t* out_off, const uint32_t* out_cap, uint32_t* out_len, int32_t* status,
                                               uint32_t n, int32_t level, uint32_t max_blocks, nx_bzip2_seg* seg, void* stream) {
    using namespace nx::bz2e;
    if (level < 1 || level > 9) return NX_ERR_BZIP2_LEVEL;  // Bzip2Encoder.java:98-101
    if (n == 0) return NX_OK;
    if (!in || !in_off || !in_len || !out || !out_off || !out_cap || !out_len || !status) return NX_ERR_INVALID_ARG;
    NX_CLEAR_STALE_ERROR();
    int dev = 0, cus = 256;
    NX_HIP_CHECK(hipGetDevice(&dev));
    NX_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    hipStream_t st = (hipStream_t)stream;
    nx::WsLease lease(nx::WsKind::Bzip2Enc, dev, st);
    // the plan arrays (a job count, n ItemSt, max_blocks Job) in whole units ahead of the slots
    const size_t unit = nx::kBzip2EncUnitBytes;
    const size_t plan_units = (64u + sizeof(ItemSt) * (size_t)n + sizeof(Job) * (size_t)max_blocks + unit - 1u) / unit;
    const size_t want_slots = std::min<size_t>({std::max<size_t>(max_blocks, 1u), (size_t)cus * nx::kBzip2EncGroupsPerCu, kMaxRound});
    const size_t need = plan_units + (size_t)level;
    nx::SharedWs& W = lease.ws();
    if (W.cap && W.cap < need) W.cap = need;  // a reserve below one slot of this level and the plan arrays
    size_t first = 0, count = 0;
    NX_HIP_CHECK(lease.acquire_part(plan_units + want_slots * (size_t)level, &first, &count));
    if (count < need) return NX_ERR_INVALID_ARG;  // a workspace its owner holds below that
    uint8_t* base = static_cast<uint8_t*>(W.p) + first * unit;
    uint32_t* njobs = reinterpret_cast<uint32_t*>(base);
    ItemSt* items = reinterpret_cast<ItemSt*>(base + 64u);
    Job* jobs = reinterpret_cast<Job*>(base + 64u + sizeof(ItemSt) * (size_t)n);
    uint8_t* ws = base + plan_units * unit;
    const uint32_t slots = (uint32_t)std::min<size_t>((count - plan_units) / (size_t)level, kMaxRound);
    hipLaunchKernelGGL(k_bzip2_plan<false>, dim3(n), dim3(64), 0, st, in, in_off, in_len, items, jobs, (uint32_t)level, max_blocks);
    hipLaunchKernelGGL(k_bzip2_plan_scan, dim3(1), dim3(kThreads), 0, st, items, njobs, seg, out_len, status, n, max_blocks);
    hipLaunchKernelGGL(k_bzip2_plan<true>, dim3(n), dim3(64), 0, st, in, in_off, in_len, items, jobs, (uint32_t)level, max_blocks);
    NX_HIP_CHECK(hipGetLastError());
    // rounds of at most `slots` jobs; a round's staging lives until its splice, and the launches are in stream order
    for (uint64_t b = 0; b == 0u || b < max_blocks; b += slots) {
        const uint32_t round = (uint32_t)std::min<uint64_t>(slots, max_blocks - b);
        if (round)
            hipLaunchKernelGGL(k_bzip2_encode_blocks, dim3(round), dim3(kThreads), 0, st, in, in_off, items, jobs, njobs, ws, (uint32_t)b,
                               (uint32_t)level);
        hipLaunchKernelGGL(k_bzip2_splice, dim3(n), dim3(kThreads), 0, st, items, jobs, njobs, ws, out, out_off, out_cap, out_len, status, seg,
                           (uint32_t)level, (uint32_t)b, slots);
        NX_HIP_CHECK(hipGetLastError());
    }
    return NX_OK;
}

// the planner alone (scripts/measure_bzip2_split.py times it): counts[i] = the blocks of item i
extern "C" int32_t nx_bzip2_plan_batch(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint32_t* counts, uint32_t n,
                                       int32_t level, void* stream) {
    using namespace nx::bz2e;
    if (level < 1 || level > 9) return NX_ERR_BZIP2_LEVEL;
    if (n == 0) return NX_OK;
    if (!in || !in_off || !in_len || !counts) return NX_ERR_INVALID_ARG;
    NX_CLEAR_STALE_ERROR();
    int dev = 0;
    NX_HIP_CHECK(hipGetDevice(&dev));
    hipStream_t st = (hipStream_t)stream;
    nx::WsLease lease(nx::WsKind::Bzip2Enc, dev, st);
    const size_t unit = nx::kBzip2EncUnitBytes, plan_units = (sizeof(ItemSt) * (size_t)n + unit - 1u) / unit;
    nx::SharedWs& W = lease.ws();
    if (W.cap && W.cap < plan_units) W.cap = plan_units;
    size_t first = 0, count = 0;
    NX_HIP_CHECK(lease.acquire_part(plan_units, &first, &count));
    if (count < plan_units) return NX_ERR_INVALID_ARG;
    ItemSt* items = reinterpret_cast<ItemSt*>(static_cast<uint8_t*>(W.p) + first * unit);
    hipLaunchKernelGGL(k_bzip2_plan<false>, dim3(n), dim3(64), 0, st, in, in_off, in_len, items, (Job*)nullptr, (uint32_t)level, 0u);
    NX_HIP_CHECK(hipGetLastError());
    NX_HIP_CHECK(hipMemcpy2DAsync(counts, 4, &items[0].cnt, sizeof(ItemSt), 4, n, hipMemcpyDeviceToDevice, st));
    return NX_OK;
}

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
