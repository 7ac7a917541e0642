// lzma.hip — LZMA stream encoder for LzmaFrameEncoder (LzmaFrameEncoder.java:177-186), two passes over
// independent items of any length up to kMaxItem.
//
// Every item becomes one complete stream: the reference's 13 header bytes (properties, dictionary size,
// the exact length) and an LZMA payload coded from a freshly initialised model, closed by the end marker
// if asked and by the range coder's five flush bytes.  The payload bytes are this encoder's own
// (lzma-java's BT4 optimal parser is not restated): liblzma decodes them to the input.  The format, the
// matcher's rule and the packet coders are in lzma_encode_core.hpp, which nx_lzma_encode_host runs on the
// CPU: the kernels write the host's bytes.
//
//   pass 1, k_lzma_match, one lane per item on the lane grid of the other alt encoders: match_item over
//     a stamped hash table of 65 536 entries (stamp << 32 | position; positions are 32-bit, an item is not
//     limited to 64 KiB) in the item's workspace slot.  It writes one 64-bit word per sequence (literal run,
//     length, distance) to the item's area of the sequence arena.  Literal bytes are not packed beside
//     them: an LZMA literal is coded under the byte before it and, after a match, against the byte at rep0,
//     both of which live in the input, so pass 2 reads the input in place.
//   pass 2, k_lzma_code, one wave per item, the item's whole probability model in LDS (1848 +
//     (0x300 << (lc + lp)) 16-bit entries: 15.6 KiB at lc = 3, lp = 0 and 27.6 KiB at lc + lp = 4) beside
//     1 KiB of staged output.  All lanes initialise the model; lane 0 runs the packet coders of the core
//     over it, one packet after another, into the stage; all lanes store the staged bytes as 16-byte
//     pieces of whole 128-byte lines.  (Why the packet step is not spread over the lanes: DESIGN.md "LZMA encode".)
//     Every output byte is checked against the slot's capacity before it is staged or stored.
//
// The sequence arena is one allocation per device beside the NX_WS_LZMA_ENC tables: an item of n bytes
// takes 16 + 8 * seq_cap(n) bytes of it (a sequence covers at least two bytes).  The host reads in_len
// back, lays the areas out and cuts the batch into launch pairs whose items fit the table slots and
// kArenaMax bytes of arena; a call therefore synchronises its stream once, before its first launch.
#include <algorithm>
#include <vector>
#include "lzma_encode_core.hpp"
#include "nx_common.hpp"
#include "workspace.hpp"

namespace nx {
namespace lzma {

constexpr uint32_t kMaxItem = 256u << 20;
constexpr uint32_t kSlotBytes = 8u << kHashLog;
constexpr uint32_t kStageBytes = 1024, kLine = 128, kCtrlBytes = 16;
__host__ __device__ inline size_t area_bytes(size_t n) { return (16u + 8u * seq_cap(n) + 15u) & ~(size_t)15; }
inline uint32_t code_lds_bytes(uint32_t lc, uint32_t lp) { return kStageBytes + kCtrlBytes + 2u * model_probs(lc, lp); }

// ---------------------------------------------------------------------------------------- pass 1
template <bool SPREAD>
__global__ void __launch_bounds__(256) k_lzma_match(const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off,
                                                    const uint32_t* __restrict__ in_len, uint32_t n, uint8_t* __restrict__ tables,
                                                    uint32_t stamp, uint8_t* __restrict__ arena, const uint64_t* __restrict__ aoff,
                                                    uint32_t dict_size) {
    uint32_t tid, nthreads;
    if (!chunk_slot<SPREAD>(tid, nthreads)) return;
    if (tid >= n) return;  // one item per slot: its sequences stay in the arena for pass 2
    const uint32_t len = in_len[tid];
    uint64_t* area = reinterpret_cast<uint64_t*>(arena + aoff[tid]);
    uint32_t ns = ~0u;
    if (len <= kMaxItem)
        ns = match_item(in + in_off[tid], len, dict_size, reinterpret_cast<uint64_t*>(tables + (size_t)tid * kSlotBytes), stamp, area + 2,
                        seq_cap(len));
    area[0] = ns;
}

// ---------------------------------------------------------------------------------------- pass 2
// The item's output bytes.  Positions count from `origin`, the 128-byte line holding the slot's first byte;
// bytes [flushed, at) that lie within kStageBytes of `flushed` are in the LDS ring, everything below
// `flushed` and any byte beyond the ring (a long run of pending 0xFF bytes leaving at once) is in global memory.
struct StageSink {
    uint8_t* ring;
    uint8_t* origin;
    uint32_t at, flushed, end;  // end: the slot's capacity as a position
    bool full;
    __device__ __forceinline__ void put(uint8_t b) {
        if (at >= end) {
            full = true;
            return;
        }
        if (at - flushed < kStageBytes) ring[at & (kStageBytes - 1u)] = b;
        else origin[at] = b;
        ++at;
    }
};

// All lanes: store the ring's bytes [from, to) (to - from <= kStageBytes), 16 bytes a lane where a piece is whole.
__device__ __forceinline__ void flush_ring(const uint8_t* ring, uint8_t* origin, uint32_t from, uint32_t to, uint32_t lane) {
    for (uint32_t c = (from & ~15u) + lane * 16u; c < to; c += 64u * 16u) {
        const uint32_t lo = c < from ? from : c, hi = c + 16u < to ? c + 16u : to;
        if (hi - lo == 16u) {
            *reinterpret_cast<uint4*>(origin + c) = *reinterpret_cast<const uint4*>(ring + (c & (kStageBytes - 1u)));
        } else {
            for (uint32_t b = lo; b < hi; ++b) origin[b] = ring[b & (kStageBytes - 1u)];
        }
    }
}

__global__ void __launch_bounds__(64) k_lzma_code(const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off,
                                                  const uint32_t* __restrict__ in_len, uint8_t* __restrict__ out,
                                                  const uint64_t* __restrict__ out_off, uint32_t* __restrict__ out_len,
                                                  int32_t* __restrict__ status, uint32_t n, const uint8_t* __restrict__ arena,
                                                  const uint64_t* __restrict__ aoff, Params P) {
    extern __shared__ __align__(16) uint8_t smem[];
    uint8_t* ring = smem;
    volatile uint32_t* ctrl = reinterpret_cast<volatile uint32_t*>(smem + kStageBytes);
    uint16_t* probs = reinterpret_cast<uint16_t*>(smem + kStageBytes + kCtrlBytes);
    const uint32_t lane = threadIdx.x;
    const uint32_t nprobs = model_probs(P.lc, P.lp);
    for (uint32_t c = blockIdx.x; c < n; c += gridDim.x) {
        const uint32_t len = in_len[c], cap = out_len[c] < 0xFFFFFF00u ? out_len[c] : 0xFFFFFF00u;
        const uint64_t* area = reinterpret_cast<const uint64_t*>(arena + aoff[c]);
        const uint32_t ns = (uint32_t)area[0];
        if (ns == ~0u) {  // uniform: an item over kMaxItem, or a sequence area that would have been passed (a bug)
            if (lane == 0u) {
                out_len[c] = 0;
                status[c] = len > kMaxItem ? NX_ERR_INVALID_ARG : NX_ERR_INTERNAL;
            }
            continue;
        }
        for (uint32_t i = lane; i < nprobs / 2u; i += 64u) reinterpret_cast<uint32_t*>(probs)[i] = kProbInit | (kProbInit << 16);
        __syncthreads();
        uint8_t* dst = out + out_off[c];
        const uint32_t lead = (uint32_t)((uintptr_t)dst & (kLine - 1u));
        uint8_t* origin = dst - lead;
        StageSink sink = {ring, origin, lead, lead, lead + cap, false};
        Coder<StageSink> C;
        uint64_t steps = max_steps(len, ns);
        if (lane == 0u) {
            C.init(probs, &sink, nullptr, in + in_off[c], len, area + 2, ns, P);
            uint8_t hdr[kHeaderBytes];
            write_header(hdr, P, len);
            for (uint32_t i = 0; i < kHeaderBytes; ++i) sink.put(hdr[i]);
        }
        uint32_t flushed = lead, flags = 0, at = lead;
        // a round stages at least one packet and at most the ring; the rounds are bounded by the steps
        for (uint64_t round = 0; round <= max_steps(len, ns) + 1u && !flags; ++round) {
            if (lane == 0u) {
                while (!C.done && !sink.full && steps != 0u && sink.at - sink.flushed < kStageBytes - kLine) {
                    C.step();
                    --steps;
                }
                ctrl[0] = sink.at;
                ctrl[1] = (C.done ? 1u : 0u) | (sink.full ? 2u : 0u) | (!C.done && !sink.full && steps == 0u ? 4u : 0u);
            }
            __syncthreads();
            at = ctrl[0];
            flags = ctrl[1];
            // beyond the ring the bytes went straight to global memory: the whole ring leaves, and everything
            // below `at` is stored then; else whole lines leave, and the rest with the last round
            const bool over = at - flushed >= kStageBytes;
            const uint32_t staged_end = over ? flushed + kStageBytes : at;
            const uint32_t to = flags || over ? staged_end : (staged_end & ~(kLine - 1u));
            if (to > flushed) {
                flush_ring(ring, origin, flushed, to, lane);
                flushed = over ? at : to;
            }
            if (lane == 0u) sink.flushed = flushed;
            __syncthreads();
        }
        if (lane == 0u) {
            const bool ok = flags == 1u;
            out_len[c] = ok ? at - lead : 0u;
            status[c] = ok ? NX_OK : (flags & 2u) ? NX_ERR_LZMA_ENCODE_FULL : NX_ERR_INTERNAL;
        }
        __syncthreads();
    }
}

// The sequence arena of a device: grown under the NX_WS_LZMA_ENC lease, dropped with that workspace.
struct Arena {
    uint8_t* p = nullptr;
    size_t bytes = 0;
};
static Arena g_arena[64];

}  // namespace lzma

void lzma_arena_drop(int dev) {
    lzma::Arena& A = lzma::g_arena[dev < 0 || dev >= 64 ? 0 : dev];
    if (A.p) (void)hipFree(A.p);
    A.p = nullptr;
    A.bytes = 0;
}
}  // namespace nx

namespace {
constexpr uint32_t kMaxStamp = 0xFFFFFFF0u;
// Most table slots the standalone entry grows the workspace to (8 GiB); a larger batch runs in sub-batches.
constexpr size_t kMaxSlots = 16384;
// Most arena bytes the sequence areas of one launch pair take, unless one item alone takes more.
constexpr size_t kArenaMax = (size_t)4 << 30;
constexpr nx::WsSpec kSpec = nx::kWsSpec[(int)nx::WsKind::LzmaEnc];
static_assert(((size_t)kSpec.entry_bytes << kSpec.lg) == nx::lzma::kSlotBytes, "lzma slot geometry");
}  // namespace

// One LZMA stream per item (netty_amd.h).
extern "C" int32_t nx_lzma_encode_batch(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint8_t* out,
                                        const uint64_t* out_off, uint32_t* out_len, int32_t* status, uint32_t n, int32_t lc, int32_t lp,
                                        int32_t pb, int32_t dict_size, int32_t end_marker, void* stream) {
    using namespace nx::lzma;
    NX_CLEAR_STALE_ERROR();
    if (lc < 0 || lc > 8 || lp < 0 || lp > 4 || pb < 0 || pb > 4 || lc + lp > 4) return NX_ERR_LZMA_PROPS;
    if (dict_size < 0) return NX_ERR_LZMA_DICT_SIZE;
    if (n == 0) return NX_OK;
    if (!in_off || !in_len || !out || !out_off || !out_len || !status) return NX_ERR_INVALID_ARG;
    const hipStream_t st = (hipStream_t)stream;
    int dev = 0, cus = 256;
    NX_HIP_CHECK(hipGetDevice(&dev));
    NX_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    nx::WsLease lease(nx::WsKind::LzmaEnc, dev, st);
    const size_t want = nx::ws_want(nx::WsKind::LzmaEnc, n, cus);
    NX_HIP_CHECK(lease.acquire(want < kMaxSlots ? want : kMaxSlots));
    nx::SharedWs& W = lease.ws();
    uint8_t* ws = static_cast<uint8_t*>(W.p);
    // the lengths, on the host: the stream has waited for the workspace's earlier users, so after this
    // synchronisation nothing reads the arena any more
    std::vector<uint32_t> len(n);
    NX_HIP_CHECK(hipMemcpyAsync(len.data(), in_len, (size_t)n * 4u, hipMemcpyDefault, st));
    NX_HIP_CHECK(hipStreamSynchronize(st));
    // launch pairs: as many items as the grid has slots, cut where the areas pass kArenaMax
    struct Pair {
        uint32_t base, m;
        nx::LaneGrid g;
    };
    std::vector<Pair> pairs;
    std::vector<uint64_t> aoff(n);
    const size_t head = ((size_t)n * 8u + 127u) & ~(size_t)127;
    size_t need = 0;
    for (uint32_t base = 0; base < n;) {
        const uint32_t left = n - base;
        const nx::LaneGrid g = nx::ws_grid(nx::WsKind::LzmaEnc, left, cus, W.slots < kMaxSlots ? W.slots : kMaxSlots);
        const uint32_t most = (uint32_t)(left < g.slots ? left : g.slots);
        size_t used = 0;
        uint32_t m = 0;
        for (; m < most; ++m) {
            const size_t a = area_bytes(len[base + m] <= kMaxItem ? len[base + m] : 0u);
            if (m && used + a > kArenaMax) break;
            aoff[base + m] = head + used;
            used += a;
        }
        need = std::max(need, used);
        pairs.push_back({base, m, g});
        base += m;
    }
    Arena& A = g_arena[dev < 0 || dev >= 64 ? 0 : dev];
    if (A.bytes < head + need) {
        nx::lzma_arena_drop(dev);
        NX_HIP_CHECK(hipMalloc(&A.p, head + need));
        A.bytes = head + need;
    }
    NX_HIP_CHECK(hipMemcpy(A.p, aoff.data(), (size_t)n * 8u, hipMemcpyHostToDevice));
    const uint64_t* d_aoff = reinterpret_cast<const uint64_t*>(A.p);
    const Params P = {(uint32_t)lc, (uint32_t)lp, (uint32_t)pb, (uint32_t)dict_size, end_marker ? 1u : 0u};
    const uint32_t lds = code_lds_bytes(P.lc, P.lp);
    // as many waves per CU as models fit the 160 KiB of LDS, at most 8 (two per SIMD)
    const unsigned per_cu = std::min<unsigned>(8u, (160u << 10) / lds);
    for (const Pair& pr : pairs) {
        const uint32_t base = pr.base, m = pr.m;
        if (W.stamp + 1u >= kMaxStamp) {
            NX_HIP_CHECK(hipMemsetAsync(W.p, 0, W.slots * (size_t)kSlotBytes, st));
            W.stamp = 0;
        }
        W.stamp += 1u;
        if (pr.g.spread)
            hipLaunchKernelGGL(k_lzma_match<true>, dim3(pr.g.grid), dim3(pr.g.block), 0, st, in, in_off + base, in_len + base, m, ws,
                               W.stamp, A.p, d_aoff + base, P.dict_size);
        else
            hipLaunchKernelGGL(k_lzma_match<false>, dim3(pr.g.grid), dim3(pr.g.block), 0, st, in, in_off + base, in_len + base, m, ws,
                               W.stamp, A.p, d_aoff + base, P.dict_size);
        NX_HIP_CHECK(hipGetLastError());
        const unsigned waves = (unsigned)cus * per_cu;
        hipLaunchKernelGGL(k_lzma_code, dim3(m < waves ? m : waves), dim3(64), lds, st, in, in_off + base, in_len + base, out,
                           out_off + base, out_len + base, status + base, m, A.p, d_aoff + base, P);
        NX_HIP_CHECK(hipGetLastError());
    }
    return NX_OK;
}
