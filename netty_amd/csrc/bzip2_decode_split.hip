// bzip2_decode_split.hip — the bzip2 decoder with a stream's blocks on a wave each (nx_bzip2_scan_batch,
// nx_bzip2_decode_batch_split): the mirror image of bzip2_encode.hip's split path.  bzip2 blocks are
// independent once their first bit is known, and each starts with a 48-bit magic.
//
//   k_bzip2_scan<false>   one wave per (item, segment), 64 segments an item: every lane takes a window of eight
//                         bytes plus the six behind them and tests its 64 bit positions for both magics
//                         (scan_window); the wave counts its segment's candidates.
//   k_bzip2_scan_place    one wave: an exclusive scan of the segments' counts, item after item, gives every
//                         segment its place in the list; an item whose candidates do not fit what is left of
//                         max_blocks gets NX_ERR_BZIP2_DECODE_BLOCKS and no place, and the next item goes on
//                         from where the one before it ended.
//   k_bzip2_scan<true>    the same scan again, emitting: a lane's rank inside its wave step is a prefix sum
//                         over the lanes, so the list is in position order whatever the scheduling.
//   k_bzip2_begin         one lane per item: the stream header and the chain's start, bit 32, or the SplitStart the
//                         Bzip2Decoder handle gives (bzip2_decode_split.hpp): a stream still arriving, whose blocks
//                         the front attempts only once a later candidate stands behind them (split_attempt).
// then, in rounds of `slots` candidates in list order:
//   k_bzip2_front         one wave per candidate: block_front from the candidate's bit position into the
//                         wave's slot, then the length the final run-length stage will give (rle_length over
//                         LDS tiles of the pre-RLE bytes); records status, end bit, both lengths, the stored CRC.
//   k_bzip2_stitch        one lane per item: split_stitch extends the chain over the candidates that have a
//                         front result.
//   k_bzip2_back          one wave per member: block_back from the slot to the member's output offset.
// and k_bzip2_finish, one lane per item: split_finish.
// Kernel boundaries are the only synchronisation between waves: a wave reads what other waves wrote only in a
// later launch.  Every loop is bounded by the input or the declared block size (the core's and
// bzip2_decode_wave.hpp's), every load stays inside the item, the slot or the call's lists, and the back checks
// every output tile against [off, cap) of the item as the serial kernel does.  A decoy candidate decodes
// under the same bounds as any corrupt block; its result is never read.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "../../include/netty_amd.h"
#include "nx_common.hpp"
#include "workspace.hpp"
#include "bzip2_decode_core.hpp"
#include "bzip2_decode_wave.hpp"
#include "bzip2_decode_split.hpp"

namespace nx {
namespace bz2d {

constexpr uint32_t kNoPlace = 0xffffffffu;
static_assert(NX_BZIP2_CAND_END == kCandEnd, "the header's kind flag is the core's");

// inclusive prefix sum over the wave's lanes
__device__ __forceinline__ uint32_t wave_inclusive(uint32_t v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)v, d);
        if (lane >= d) v += o;
    }
    return v;
}

template <bool kEmit>
__global__ void __launch_bounds__(64) k_bzip2_scan(const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off,
                                                   const uint32_t* __restrict__ in_len, uint32_t* seg_count,
                                                   const uint32_t* __restrict__ seg_place, uint64_t* positions, uint32_t* cand_item,
                                                   uint32_t n) {
    const int lane = (int)threadIdx.x;
    const uint64_t jobs = (uint64_t)n * kScanSegments;
    for (uint64_t job = blockIdx.x; job < jobs; job += gridDim.x) {
        const uint32_t i = (uint32_t)(job / kScanSegments), s = (uint32_t)(job % kScanSegments);
        const uint32_t len = in_len[i];
        const uint8_t* p = in + in_off[i];
        const uint64_t seg = scan_segment_bytes(len);
        const uint64_t a = s * seg, b = a + seg < len ? a + seg : len;
        uint32_t place = 0;
        if (kEmit) {
            place = seg_place[job];
            if (place == kNoPlace) continue;
        }
        uint32_t running = 0;
        for (uint64_t w0 = a; w0 < b; w0 += 64u * kScanWindow) {  // (a >= b: an empty segment)
            const uint64_t b0 = w0 + (uint64_t)kScanWindow * (uint32_t)lane;
            uint64_t blk = 0, end = 0;
            if (b0 < b) scan_window(p, len, b0, &blk, &end);
            const uint32_t c = (uint32_t)__popcll(blk | end);
            if (__ballot(c != 0u) == 0ull) continue;
            const uint32_t incl = wave_inclusive(c, lane);
            if (kEmit) {
                uint32_t at = place + running + incl - c;
                for (uint64_t m = blk | end; m != 0ull; m &= m - 1ull) {
                    const uint32_t k = (uint32_t)__builtin_ctzll(m);
                    positions[at] = (8ull * b0 + k) | ((end >> k) & 1ull ? kCandEnd : 0ull);
                    cand_item[at] = i;
                    at += 1u;
                }
            }
            running += (uint32_t)__shfl((int)incl, 63);
        }
        if (!kEmit && lane == 0) seg_count[job] = running;
    }
}

__global__ void __launch_bounds__(64) k_bzip2_scan_place(const uint32_t* __restrict__ seg_count, uint32_t* seg_place, uint32_t* first,
                                                         uint32_t* count, int32_t* status, uint32_t* total, uint32_t n,
                                                         uint32_t max_blocks) {
    const int lane = (int)threadIdx.x;
    uint32_t base = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t c = seg_count[(size_t)i * kScanSegments + (uint32_t)lane];
        const uint32_t incl = wave_inclusive(c, lane);
        const uint32_t sum = (uint32_t)__shfl((int)incl, 63);  // at most 8 x in_len: below 2^32 only for items below 512 MiB
        const bool fits = sum <= max_blocks - base;
        seg_place[(size_t)i * kScanSegments + (uint32_t)lane] = fits ? base + incl - c : kNoPlace;
        if (lane == 0) {
            first[i] = base;
            count[i] = fits ? sum : 0u;
            status[i] = fits ? NX_OK : NX_ERR_BZIP2_DECODE_BLOCKS;
        }
        if (fits) base += sum;
    }
    if (lane == 0) *total = base;
}

__global__ void __launch_bounds__(64) k_bzip2_begin(const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off,
                                                    const uint32_t* __restrict__ in_len, const int32_t* __restrict__ scan_status,
                                                    const SplitStart* __restrict__ start, SplitItem* items, uint32_t n) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    SplitItem I;
    SplitStart s0;
    if (start) s0 = start[i];
    split_begin(I, in + in_off[i], in_len[i], start ? &s0 : nullptr);
    if (scan_status[i] != NX_OK) I.status = scan_status[i];
    items[i] = I;
}

// the candidate of this wave in the round that starts at list index `base`, or false
__device__ __forceinline__ bool round_candidate(const uint32_t* total, uint32_t base, uint32_t* g) {
    *g = base + blockIdx.x;
    return *g >= base && *g < *total;
}

__global__ void __launch_bounds__(64) k_bzip2_front(const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off,
                                                    const uint32_t* __restrict__ in_len, uint8_t* ws,
                                                    const uint64_t* __restrict__ positions, const uint32_t* __restrict__ cand_item,
                                                    const uint32_t* __restrict__ first, const uint32_t* __restrict__ count,
                                                    const SplitItem* __restrict__ items, CandResult* res,
                                                    const uint32_t* __restrict__ total, uint32_t base) {
    __shared__ WaveLds L;
    const int lane = (int)threadIdx.x;
    uint32_t g = 0;
    if (!round_candidate(total, base, &g)) return;
    const uint64_t pos = positions[g];
    if (pos & kCandEnd) return;
    const uint32_t i = cand_item[g];
    if (items[i].status != kChainOpen) return;  // the chain has ended (or never began): nothing reads this candidate
    if (!split_attempt(items[i], pos & kCandPos, first[i] + count[i] - 1u - g)) {  // a stream still arriving
        if (lane == 0) {
            CandResult c = {};
            c.status = kNotAttempted;
            res[g] = c;
        }
        return;
    }
    const uint32_t level = items[i].level;
    const uint8_t* p = in + in_off[i];
    const uint32_t n = uni(in_len[i]);
    uint8_t* slot = ws + (size_t)blockIdx.x * kBzip2DecSlotBytes;
    if (lane == 0) {
        br_init_bitpos(L.B.br, p, n, (pos & kCandPos) + 48u);
        L.B.crc = br_bits(L.B.br, 32);
        L.B.block_size = level * kBaseBlock;
        L.mail[5] = L.B.br.over;
    }
    wave_sync();
    uint32_t pre_len = 0;
    int32_t st = uni(L.mail[5]) ? NX_ERR_BZIP2_TRUNCATED : block_front(L, slot, &pre_len, lane);
    uint32_t final_len = 0;
    if (st == NX_OK) {  // the length of the final stage's output, tile by tile on lane 0
        const uint32_t* pre32 = reinterpret_cast<const uint32_t*>(slot + kOffPre);
        wave_sync();
        if (lane == 0) rle_init(L.R);
        for (uint32_t i0 = 0; i0 < pre_len; i0 += kTile) {
            const uint32_t m = pre_len - i0 < kTile ? pre_len - i0 : kTile;
            wave_sync();
            for (uint32_t w = (uint32_t)lane; w < (m + 3u) / 4u; w += 64u) L.rle.src[w] = load_own32(pre32 + i0 / 4u + w);
            wave_sync();
            if (lane == 0) final_len += rle_length(L.R, reinterpret_cast<const uint8_t*>(L.rle.src), m);
        }
    }
    if (lane == 0) {
        CandResult c;
        c.end_bit = st == NX_OK ? br_bitpos(L.B.br) : 0ull;
        c.status = st;
        c.pre_len = pre_len;
        c.final_len = final_len;
        c.crc = L.B.crc;
        c.member = 0;
        c.off = 0;
        c.back_status = NX_OK;
        c.crc_got = 0;
        res[g] = c;
    }
}

__global__ void __launch_bounds__(64) k_bzip2_stitch(const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off,
                                                     const uint32_t* __restrict__ in_len, const uint32_t* __restrict__ out_cap,
                                                     const uint64_t* __restrict__ positions, const uint32_t* __restrict__ first,
                                                     const uint32_t* __restrict__ count, SplitItem* items, CandResult* res, uint32_t n,
                                                     uint32_t ready_end) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    SplitItem I = items[i];
    if (I.status != kChainOpen) return;
    const uint32_t f = first[i], c = count[i];
    const uint32_t ready = ready_end <= f ? 0u : ready_end - f < c ? ready_end - f : c;
    split_stitch(I, in + in_off[i], in_len[i], out_cap[i], positions + f, res + f, c, ready);
    items[i] = I;
}

__global__ void __launch_bounds__(64) k_bzip2_back(uint8_t* out, const uint64_t* __restrict__ out_off,
                                                   const uint32_t* __restrict__ out_cap, const uint8_t* ws,
                                                   const uint32_t* __restrict__ cand_item, CandResult* res,
                                                   const uint32_t* __restrict__ total, uint32_t base) {
    __shared__ WaveLds L;
    const int lane = (int)threadIdx.x;
    uint32_t g = 0;
    if (!round_candidate(total, base, &g)) return;
    if (!res[g].member) return;
    const uint32_t i = cand_item[g];
    const uint32_t off = uni(res[g].off), cap = uni(out_cap[i]);  // off <= cap (split_stitch)
    for (uint32_t k = (uint32_t)lane; k < 256u; k += 64u) L.crc_table[k] = crc_table_entry(k);
    if (lane == 0) crc_shift_init(L.shift);
    wave_sync();
    uint32_t produced = 0;
    const int32_t st = block_back(L, ws + (size_t)blockIdx.x * kBzip2DecSlotBytes + kOffPre, uni(res[g].pre_len), uni(res[g].crc),
                                  out + out_off[i] + off, cap - off, &produced, lane);
    if (lane == 0) res[g].back_status = st;
}

__global__ void __launch_bounds__(64) k_bzip2_finish(const uint32_t* __restrict__ first, const uint32_t* __restrict__ count,
                                                     const SplitItem* __restrict__ items, const CandResult* __restrict__ res,
                                                     uint32_t* out_len, uint32_t* consumed, int32_t* status, uint32_t* blocks, uint32_t n) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    int32_t st = NX_OK;
    uint32_t ol = 0, cs = 0, nb = 0;
    split_finish(items[i], res + first[i], count[i], &st, &ol, &cs, &nb);
    status[i] = st;
    out_len[i] = ol;
    consumed[i] = cs;
    if (blocks) blocks[i] = nb;
}

static size_t up(size_t v) { return (v + 255u) / 256u * 256u; }
// The lists of one call laid out from `mem` (nullptr: sizes only); returns their bytes.  decode: the chain
// lists follow the scan's, in one piece from S.first to the end of S.res.
size_t split_lists_layout(SplitLists& S, void* mem, uint32_t n, uint32_t max_blocks, bool decode) {
    const size_t segs = (size_t)n * kScanSegments;
    const size_t b_seg = up(4u * segs), b_n = up(4u * (size_t)n), b_pos = up(8u * (size_t)max_blocks + 8u),
                 b_ci = up(4u * (size_t)max_blocks + 4u), b_items = up(sizeof(SplitItem) * (size_t)n),
                 b_res = up(sizeof(CandResult) * ((size_t)max_blocks + 1u));
    uint8_t* q = static_cast<uint8_t*>(mem);
    auto take = [&](size_t b) {
        uint8_t* r = q;
        q += b;
        return r;
    };
    S.mem = mem;
    S.seg_count = reinterpret_cast<uint32_t*>(take(b_seg));
    S.seg_place = reinterpret_cast<uint32_t*>(take(b_seg));
    S.total = reinterpret_cast<uint32_t*>(take(256));
    S.cand_item = reinterpret_cast<uint32_t*>(take(b_ci));
    if (decode) {
        S.first = reinterpret_cast<uint32_t*>(take(b_n));
        S.count = reinterpret_cast<uint32_t*>(take(b_n));
        S.scan_status = reinterpret_cast<int32_t*>(take(b_n));
        S.positions = reinterpret_cast<uint64_t*>(take(b_pos));
        S.items = reinterpret_cast<SplitItem*>(take(b_items));
        S.res = reinterpret_cast<CandResult*>(take(b_res));
        S.res_bytes = b_res;
    }
    return (size_t)(q - static_cast<uint8_t*>(mem));
}
static hipError_t lists_alloc(SplitLists& S, uint32_t n, uint32_t max_blocks, bool decode, hipStream_t st) {
    SplitLists sizes;
    void* mem = nullptr;
    const hipError_t e = hipMallocAsync(&mem, split_lists_layout(sizes, nullptr, n, max_blocks, decode), st);
    if (e == hipSuccess) split_lists_layout(S, mem, n, max_blocks, decode);
    return e;
}

static int32_t scan_launch(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint32_t n, uint32_t max_blocks,
                           SplitLists& S, int cus, hipStream_t st) {
    const uint64_t jobs = (uint64_t)n * kScanSegments;
    const unsigned grid = (unsigned)std::min<uint64_t>(jobs, (uint64_t)cus * 64u);
    hipLaunchKernelGGL(k_bzip2_scan<false>, dim3(grid), dim3(64), 0, st, in, in_off, in_len, S.seg_count, S.seg_place, S.positions,
                       S.cand_item, n);
    NX_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_bzip2_scan_place, dim3(1), dim3(64), 0, st, S.seg_count, S.seg_place, S.first, S.count, S.scan_status, S.total, n,
                       max_blocks);
    NX_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_bzip2_scan<true>, dim3(grid), dim3(64), 0, st, in, in_off, in_len, S.seg_count, S.seg_place, S.positions,
                       S.cand_item, n);
    NX_HIP_CHECK(hipGetLastError());
    return NX_OK;
}

}  // namespace bz2d
}  // namespace nx

extern "C" int32_t nx_bzip2_scan_batch(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint32_t n, uint32_t max_blocks,
                                       uint64_t* positions, uint32_t* first, uint32_t* count, int32_t* status, void* stream) {
    using namespace nx::bz2d;
    if (n == 0) return NX_OK;
    if (!in || !in_off || !in_len || (!positions && max_blocks) || !first || !count || !status) return NX_ERR_INVALID_ARG;
    NX_CLEAR_STALE_ERROR();
    int dev = 0, cus = 256;
    NX_HIP_CHECK(hipGetDevice(&dev));
    NX_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    hipStream_t st = (hipStream_t)stream;
    SplitLists S;
    NX_HIP_CHECK(lists_alloc(S, n, max_blocks, false, st));
    S.positions = positions;
    S.first = first;
    S.count = count;
    S.scan_status = status;
    const int32_t r = scan_launch(in, in_off, in_len, n, max_blocks, S, cus, st);
    NX_HIP_CHECK(hipFreeAsync(S.mem, st));
    return r;
}

namespace nx {
namespace bz2d {
int32_t decode_split_launch(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint8_t* out, const uint64_t* out_off,
                            const uint32_t* out_cap, uint32_t* out_len, uint32_t* consumed, int32_t* status, uint32_t n,
                            uint32_t max_blocks, uint32_t* blocks, const SplitStart* start, void* lists_mem, hipStream_t st) {
    NX_CLEAR_STALE_ERROR();
    int dev = 0, cus = 256;
    NX_HIP_CHECK(hipGetDevice(&dev));
    NX_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    SplitLists S;
    if (lists_mem) split_lists_layout(S, lists_mem, n, max_blocks, true);
    else NX_HIP_CHECK(lists_alloc(S, n, max_blocks, true, st));
    // a candidate no front reaches is no member
    int32_t r = hipMemsetAsync(S.res, 0, S.res_bytes, st) == hipSuccess ? NX_OK : NX_ERR_HIP;
    if (r == NX_OK) r = scan_launch(in, in_off, in_len, n, max_blocks, S, cus, st);
    const unsigned per_item = (n + 63u) / 64u;
    if (r == NX_OK) {
        hipLaunchKernelGGL(k_bzip2_begin, dim3(per_item), dim3(64), 0, st, in, in_off, in_len, S.scan_status, start, S.items, n);
        r = hipGetLastError() == hipSuccess ? NX_OK : NX_ERR_HIP;
    }
    if (r == NX_OK && max_blocks != 0u) {
        nx::WsLease lease(nx::WsKind::Bzip2Dec, dev, st);
        size_t first = 0, slots = 0;  // one slot per candidate of a round
        hipError_t e = lease.acquire_part(nx::ws_want(nx::WsKind::Bzip2Dec, max_blocks, cus), &first, &slots);
        if (e != hipSuccess || slots == 0) {
            r = NX_ERR_HIP;
        } else {
            uint8_t* ws = static_cast<uint8_t*>(lease.ws().p) + first * nx::kBzip2DecSlotBytes;
            for (uint64_t base = 0; base < max_blocks && r == NX_OK; base += slots) {
                const uint32_t ready_end = (uint32_t)std::min<uint64_t>(base + slots, max_blocks);
                const unsigned grid = (unsigned)(ready_end - base);
                hipLaunchKernelGGL(k_bzip2_front, dim3(grid), dim3(64), 0, st, in, in_off, in_len, ws, S.positions, S.cand_item, S.first,
                                   S.count, S.items, S.res, S.total, (uint32_t)base);
                hipLaunchKernelGGL(k_bzip2_stitch, dim3(per_item), dim3(64), 0, st, in, in_off, in_len, out_cap, S.positions, S.first,
                                   S.count, S.items, S.res, n, ready_end);
                hipLaunchKernelGGL(k_bzip2_back, dim3(grid), dim3(64), 0, st, out, out_off, out_cap, ws, S.cand_item, S.res, S.total,
                                   (uint32_t)base);
                r = hipGetLastError() == hipSuccess ? NX_OK : NX_ERR_HIP;
            }
        }
    } else if (r == NX_OK) {  // no list at all: the chains end where they begin
        hipLaunchKernelGGL(k_bzip2_stitch, dim3(per_item), dim3(64), 0, st, in, in_off, in_len, out_cap, S.positions, S.first, S.count,
                           S.items, S.res, n, 0u);
        r = hipGetLastError() == hipSuccess ? NX_OK : NX_ERR_HIP;
    }
    if (r == NX_OK) {
        hipLaunchKernelGGL(k_bzip2_finish, dim3(per_item), dim3(64), 0, st, S.first, S.count, S.items, S.res, out_len, consumed, status,
                           blocks, n);
        r = hipGetLastError() == hipSuccess ? NX_OK : NX_ERR_HIP;
    }
    const hipError_t fe = lists_mem ? hipSuccess : hipFreeAsync(S.mem, st);
    return r != NX_OK ? r : fe == hipSuccess ? NX_OK : NX_ERR_HIP;
}
}  // namespace bz2d
}  // namespace nx

extern "C" int32_t nx_bzip2_decode_batch_split(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint8_t* out,
                                               const uint64_t* out_off, const uint32_t* out_cap, uint32_t* out_len, uint32_t* consumed,
                                               int32_t* status, uint32_t n, uint32_t max_blocks, uint32_t* blocks, void* stream) {
    if (n == 0) return NX_OK;
    if (!in || !in_off || !in_len || !out || !out_off || !out_cap || !out_len || !consumed || !status) return NX_ERR_INVALID_ARG;
    return nx::bz2d::decode_split_launch(in, in_off, in_len, out, out_off, out_cap, out_len, consumed, status, n, max_blocks, blocks, nullptr,
                                         nullptr, (hipStream_t)stream);
}
