// seq_stage.hpp — the device parts the two-pass sequence encoders share (lzma.hip, brotli.hip): the pass-1
// kernel, which runs a codec's matcher over one item a lane, and around the codec's own rounds of a pass-2
// kernel the LDS ring an item's bytes are staged in and the length and status the item leaves.  (How a pass-2
// item begins stands in each kernel: as a shared inlined function it moved k_brotli_emit's register allocation
// from 205 to 153 VGPRs and cost the kernel 1.2 % of its time.)
#pragma once
#include "nx_common.hpp"

namespace nx {

constexpr uint32_t kSeqLine = 128;  // the ring leaves in whole lines of the output

// Pass 1, one lane per item on the lane grid of the alt encoders.  Codec: kMaxItem, kSlotBytes, seq_cap(n) and
// match_item(in, len, param, table, stamp, seq, cap), which returns the sequences written or ~0.  The item's
// area of the arena takes the count (~0: none, pass 2 reports why) and, from its third word, the sequences.
template <class Codec, bool SPREAD>
__global__ void __launch_bounds__(256) k_seq_match(const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off,
                                                   const uint32_t* __restrict__ in_len, uint32_t n, uint8_t* __restrict__ tables,
                                                   uint32_t stamp, uint8_t* __restrict__ arena, const uint64_t* __restrict__ aoff,
                                                   uint32_t param) {
    uint32_t tid, nthreads;
    if (!chunk_slot<SPREAD>(tid, nthreads)) return;
    if (tid >= n) return;  // one item per slot: its sequences stay in the arena for pass 2
    const uint32_t len = in_len[tid];
    uint64_t* area = reinterpret_cast<uint64_t*>(arena + aoff[tid]);
    uint32_t ns = ~0u;
    if (len <= Codec::kMaxItem)
        ns = Codec::match_item(in + in_off[tid], len, param, reinterpret_cast<uint64_t*>(tables + (size_t)tid * Codec::kSlotBytes), stamp,
                               area + 2, Codec::seq_cap(len));
    area[0] = ns;
}

// The item's output bytes.  Positions count from `origin`, the 128-byte line holding the slot's first byte;
// bytes [flushed, at) that lie within kStageBytes of `flushed` are in the LDS ring, everything below `flushed`
// and any byte beyond the ring is in global memory.
template <uint32_t kStageBytes>
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

// All lanes: store the ring's bytes [from, to) (to - from <= kStageBytes), 16 bytes a lane where a piece is whole;
// CLEAR: and zero them in the ring, for a ring that bits are ORed into.
template <uint32_t kStageBytes, bool CLEAR>
__device__ __forceinline__ void flush_ring(uint8_t* ring, uint8_t* origin, uint32_t from, uint32_t to, uint32_t lane) {
    for (uint32_t c = (from & ~15u) + lane * 16u; c < to; c += 64u * 16u) {
        const uint32_t lo = c < from ? from : c, hi = c + 16u < to ? c + 16u : to;
        if (hi - lo == 16u) {
            uint4* piece = reinterpret_cast<uint4*>(ring + (c & (kStageBytes - 1u)));
            *reinterpret_cast<uint4*>(origin + c) = *piece;
            if (CLEAR) *piece = make_uint4(0, 0, 0, 0);
        } else {
            for (uint32_t b = lo; b < hi; ++b) {
                origin[b] = ring[b & (kStageBytes - 1u)];
                if (CLEAR) ring[b & (kStageBytes - 1u)] = 0;
            }
        }
    }
}

// Lane 0, after the rounds.  flags: 1 the coder is done, 2 the slot was full (status `full`), anything else a bug.
__device__ __forceinline__ void seq_item_end(uint32_t* out_len, int32_t* status, uint32_t c, uint32_t flags,
                                             uint32_t bytes, int32_t full) {
    const bool ok = flags == 1u;
    out_len[c] = ok ? bytes : 0u;
    status[c] = ok ? NX_OK : (flags & 2u) ? full : NX_ERR_INTERNAL;
}

}  // namespace nx
