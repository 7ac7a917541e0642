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
//   pass 1, k_seq_match<Match> (seq_stage.hpp), one lane per item on the lane grid of the other alt encoders: match_item over
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
// The sequence arena is the side allocation of the NX_WS_LZMA_ENC workspace, freed whenever its tables are:
// an item of n bytes takes 16 + 8 * seq_cap(n) bytes of it (a sequence covers at least two bytes).  The host
// reads in_len back, lays the areas out and cuts the batch into launch pairs whose items fit the table slots
// and kWsAreaMax bytes of arena (WsAreaCut, workspace.hpp); a call therefore synchronises its stream once,
// before its first launch.
#include <algorithm>
#include "lzma_encode_core.hpp"
#include "nx_common.hpp"
#include "seq_stage.hpp"
#include "workspace.hpp"

namespace nx {
namespace lzma {

constexpr uint32_t kMaxItem = 256u << 20;
constexpr uint32_t kSlotBytes = 8u << kHashLog;
constexpr uint32_t kStageBytes = 1024, kLine = kSeqLine, kCtrlBytes = 16;
inline uint32_t code_lds_bytes(uint32_t lc, uint32_t lp) { return kStageBytes + kCtrlBytes + 2u * model_probs(lc, lp); }

// pass 1: k_seq_match's codec; its parameter is the dictionary size
struct Match {
    static constexpr uint32_t kMaxItem = lzma::kMaxItem, kSlotBytes = lzma::kSlotBytes;
    static __device__ __forceinline__ size_t seq_cap(size_t n) { return lzma::seq_cap(n); }
    static __device__ __forceinline__ uint32_t match_item(const uint8_t* in, uint32_t n, uint32_t dict_size, uint64_t* table, uint32_t stamp,
                                                          uint64_t* seq, size_t cap) {
        return lzma::match_item(in, n, dict_size, table, stamp, seq, cap);
    }
};

// ---------------------------------------------------------------------------------------- pass 2
// The ring (seq_stage.hpp) holds 1 KiB; a byte beyond it is a long run of pending 0xFF bytes leaving at once.
using Sink = StageSink<kStageBytes>;

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
        Sink sink = {ring, origin, lead, lead, lead + cap, false};
        Coder<Sink> C;
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
                flush_ring<kStageBytes, false>(ring, origin, flushed, to, lane);
                flushed = over ? at : to;
            }
            if (lane == 0u) sink.flushed = flushed;
            __syncthreads();
        }
        if (lane == 0u) seq_item_end(out_len, status, c, flags, at - lead, NX_ERR_LZMA_ENCODE_FULL);
        __syncthreads();
    }
}

}  // namespace lzma
}  // namespace nx

namespace {
// Stamps are 32 bits; at most 16 384 table slots (8 GiB) for a standalone call, a larger batch runs in sub-batches.
constexpr nx::WsPairSpec kPair = {nx::WsKind::LzmaEnc, 0xFFFFFFF0u, 16384};
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
    nx::WsAreaCut cut = {in_len, [](uint32_t len) { return area_bytes(seq_cap(len <= kMaxItem ? len : 0u)); }};
    const Params P = {(uint32_t)lc, (uint32_t)lp, (uint32_t)pb, (uint32_t)dict_size, end_marker ? 1u : 0u};
    const uint32_t lds = code_lds_bytes(P.lc, P.lp);
    // as many waves per CU as models fit the 160 KiB of LDS, at most 8 (two per SIMD)
    const unsigned per_cu = std::min<unsigned>(8u, (160u << 10) / lds);
    return nx::ws_pair_launch(
        kPair, n, st, per_cu, &cut, true,
        [&](uint32_t base, uint32_t m, const nx::LaneGrid& g, nx::SharedWs& W, uint32_t stamp) {
            auto* k = g.spread ? nx::k_seq_match<Match, true> : nx::k_seq_match<Match, false>;
            hipLaunchKernelGGL(k, dim3(g.grid), dim3(g.block), 0, st, in, in_off + base, in_len + base, m, static_cast<uint8_t*>(W.p), stamp,
                               static_cast<uint8_t*>(W.side), cut.d_aoff(W) + base, P.dict_size);
        },
        [&](uint32_t base, uint32_t m, unsigned waves, nx::SharedWs& W) {
            hipLaunchKernelGGL(k_lzma_code, dim3(waves), dim3(64), lds, st, in, in_off + base, in_len + base, out, out_off + base,
                               out_len + base, status + base, m, static_cast<const uint8_t*>(W.side), cut.d_aoff(W) + base, P);
        });
}
