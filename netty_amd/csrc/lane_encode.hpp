// lane_encode.hpp — the kernel shell and the host launcher of the lane-per-chunk encoders (LZ4,
// LZ4 HC, LZF; nx_common.hpp chunk_slot / LaneGrid, workspace.hpp ws_lane_launch).
//
// A codec is a traits struct next to its format code.  It names what differs:
//   Entry, kEntries      a lane's table: kEntries entries of type Entry
//   kKind, kMaxStamp     the workspace of those tables and the stamp bound ws_lane_launch keeps
//   valid(len)           whether an item of len bytes may be encoded (else NX_ERR_INVALID_ARG, out_len 0)
//   stamp(base, iter)    the stamp of a lane's iter-th item in a launch with stamp base `base`
//   unstaged(len)        whether the item writes plain global bytes even in the dense form
//   encode(in, len, o, table, stamp)   the item's bytes through the sink o; returns their count
#pragma once
#include "nx_common.hpp"
#include "workspace.hpp"

namespace nx {

// The dense form gives every lane an item and stages its output in the lane's LDS slot; the spread
// form gives every wave one on lane 0, writing global bytes.
template <class Codec, bool SPREAD>
__global__ void __launch_bounds__(256) k_lane_encode(const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off,
                                                     const uint32_t* __restrict__ in_len, uint8_t* __restrict__ out,
                                                     const uint64_t* __restrict__ out_off, uint32_t* __restrict__ out_len,
                                                     int32_t* __restrict__ status, uint32_t n,
                                                     typename Codec::Entry* __restrict__ ws, uint32_t stamp_base) {
    uint32_t tid, nthreads;
    if (!chunk_slot<SPREAD>(tid, nthreads)) return;
    typename Codec::Entry* table = ws + (size_t)tid * Codec::kEntries;
    uint8_t* slot = nullptr;
    if constexpr (!SPREAD) {
        __shared__ __attribute__((aligned(16))) uint8_t stages[256 * kStageStride];
        slot = &stages[threadIdx.x * kStageStride];
    }
    uint32_t iter = 0;
    for (uint32_t c = tid; c < n; c += nthreads, ++iter) {
        const uint32_t len = in_len[c];
        if (!Codec::valid(len)) {
            out_len[c] = 0;
            status[c] = NX_ERR_INVALID_ARG;
            continue;
        }
        const uint32_t stamp = Codec::stamp(stamp_base, iter);
        if (SPREAD || Codec::unstaged(len)) {
            GOut o{out + out_off[c]};
            out_len[c] = Codec::encode(in + in_off[c], len, o, table, stamp);
        } else {
            ByteStage o(slot, out + out_off[c]);  // whole 128-byte units (nx_common.hpp)
            out_len[c] = Codec::encode(in + in_off[c], len, o, table, stamp);
        }
        status[c] = NX_OK;
    }
}

// The body of a codec's extern "C" batch call.
template <class Codec>
int32_t lane_encode_batch(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint8_t* out, const uint64_t* out_off,
                          uint32_t* out_len, int32_t* status, uint32_t n, void* stream) {
    using Entry = typename Codec::Entry;
    constexpr WsSpec spec = kWsSpec[(int)Codec::kKind];
    static_assert(((size_t)spec.entry_bytes << spec.lg) == sizeof(Entry) * Codec::kEntries, "table geometry");
    NX_CLEAR_STALE_ERROR();
    if (n == 0) return NX_OK;
    if (!in || !in_off || !in_len || !out || !out_off || !out_len || !status) return NX_ERR_INVALID_ARG;
    const hipStream_t st = (hipStream_t)stream;
    return ws_lane_launch(Codec::kKind, Codec::kMaxStamp, n, st,
                          [&](size_t base, uint32_t m, const LaneGrid& g, void* tables, uint32_t stamp) {
                              const auto kernel = g.spread ? k_lane_encode<Codec, true> : k_lane_encode<Codec, false>;
                              hipLaunchKernelGGL(kernel, dim3(g.grid), dim3(g.block), 0, st, in, in_off + base, in_len + base, out,
                                                 out_off + base, out_len + base, status + base, m, static_cast<Entry*>(tables), stamp);
                          });
}

}  // namespace nx
