// bzip2_decode.hip — bzip2 decoder over a batch of complete streams (nx_bzip2_decode_batch; what
// Bzip2Decoder.java does with a whole stream, one stream per item).
//
// One wave per stream (a block is one wave), as k_inflate and k_zstd_decode: the lanes of a wave share
// every branch and the tables fit its LDS.  A stream's blocks are done one after another by that wave.
// The format logic is bzip2_decode_core.hpp, the same functions the host decoder runs; the wave-wide parts of a
// block (decode_block and what it calls) are bzip2_decode_wave.hpp, shared with bzip2_decode_split.hip.  Per block:
//   1. lane 0 reads the headers, selectors and code lengths and builds the tables in LDS;
//   2. lane 0 decodes symbols and runs the move-to-front list (both serial by nature) into an LDS tile
//      that the wave flushes to the stream's workspace slot; a run longer than the tile's room is a wave
//      fill; the byte histogram stays in LDS;
//   3. after an exclusive scan of the 256 counts the wave builds the merged pointers, 64 positions a step
//      in order: a lane's rank among the step's lanes with the same byte comes from ballots over the
//      byte's eight bits and the group's leader advances the base in LDS, which keeps the sort stable;
//   4. the inverse BWT walk, a chain of n dependent loads, is split into kChains sublists: kChains
//      distinct entries, the start pointer's among them, are replaced by a flag and their chain's number
//      (the entries themselves wait in LDS); pass A walks every chain to the next flagged entry and
//      records its length and successor, lane 0 orders the chains from the start pointer's and
//      prefix-sums the lengths, pass B walks them again and writes their bytes at their offsets.  A lane
//      keeps its kChainsPerLane chains' loads in flight together.  j -> entry[j] >> 8 is a permutation,
//      so every chain ends within n steps and every index stays below n.  When the ordered chains close
//      on the first one after L < n bytes (the block of a periodic text, or a corrupt one), the serial
//      walk of the reference goes round the same cycle again: byte i is byte i mod L, a wave copy;
//   5. the final run-length stage goes from the slot through LDS tiles on lane 0 into an output tile
//      (runs of kRleInline bytes or more are wave fills) that the wave stores once lane 0 has checked it
//      against out_cap; the block CRC folds each output tile in wave-wide: sixteen bytes a lane, combined
//      by a six-level shift tree (crc32c.hip's method with bzip2's polynomial and bit order).
// The wave reads back its own stores from the slot under inflate.hip's discipline: wait for the wave's
// own stores (s_waitcnt vmcnt(0)), then load with agent scope, past the vector L1.
//
// Nothing is assumed about the input: the core bounds every read to [in_off, in_off + in_len) and every
// block to the declared size, at most 900 000 bytes, which is what a slot holds; lane 0 checks an output
// tile against out_cap before the wave stores it, so no store leaves [out_off, out_off + out_cap).
#include <hip/hip_runtime.h>
#include <algorithm>
#include "../../include/netty_amd.h"
#include "nx_common.hpp"
#include "workspace.hpp"
#include "bzip2_decode_core.hpp"
#include "bzip2_decode_wave.hpp"

namespace nx {
namespace bz2d {

__device__ void decode_stream(WaveLds& L, const uint8_t* in, uint32_t n, uint8_t* out, uint32_t cap, uint8_t* slot, uint32_t* out_len,
                              uint32_t* consumed, int32_t* status, int lane) {
    uint32_t level = 0;
    int32_t st = (int32_t)uni((uint32_t)stream_header(in, n, &level));  // the same on every lane
    uint32_t pos = 0, q = 0, stream_crc = 0;
    if (st == NX_OK) {
        level = uni(level);
        wave_sync();
        if (lane == 0) br_init(L.B.br, in, n, 4);
        for (;;) {  // every pass consumes a block of the input
            wave_sync();
            if (lane == 0) {
                uint32_t end = 0, crc = 0;
                L.mail[0] = (uint32_t)block_magic(L.B.br, &end, &crc);
                L.mail[1] = end;
                L.mail[2] = crc;
                L.mail[3] = L.B.br.at;
                L.B.crc = crc;
                L.B.block_size = level * kBaseBlock;
            }
            wave_sync();
            st = (int32_t)uni(L.mail[0]);
            if (st != NX_OK) break;
            const uint32_t crc = uni(L.mail[2]);
            if (uni(L.mail[1])) {
                if (crc != stream_crc) st = NX_ERR_BZIP2_STREAM_CRC;
                else q = uni(L.mail[3]);  // the combined CRC's last byte holds the padding
                break;
            }
            uint32_t produced = 0;
            st = decode_block(L, slot, out + pos, cap - pos, &produced, lane);
            if (st != NX_OK) break;
            stream_crc = crc_combine_stream(stream_crc, crc);
            pos += produced;
        }
    }
    if (lane == 0) {
        *consumed = st == NX_OK ? q : 0u;
        *out_len = pos;
        *status = st;
    }
}

__global__ void __launch_bounds__(64) k_bzip2_decode(const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off,
                                                     const uint32_t* __restrict__ in_len, uint8_t* out,
                                                     const uint64_t* __restrict__ out_off, const uint32_t* __restrict__ out_cap,
                                                     uint8_t* ws, uint32_t* out_len, uint32_t* consumed, int32_t* status, uint32_t n) {
    __shared__ WaveLds L;
    const int lane = (int)threadIdx.x;
    uint8_t* slot = ws + (size_t)blockIdx.x * kBzip2DecSlotBytes;
    for (uint32_t i = (uint32_t)lane; i < 256u; i += 64u) L.crc_table[i] = crc_table_entry(i);
    if (lane == 0) crc_shift_init(L.shift);
    wave_sync();
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        decode_stream(L, in + in_off[i], uni(in_len[i]), out + out_off[i], uni(out_cap[i]), slot, out_len + i, consumed + i, status + i,
                      lane);
        wave_sync();
    }
}

}  // namespace bz2d
}  // namespace nx

extern "C" int32_t nx_bzip2_decode_batch(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint8_t* out,
                                         const uint64_t* out_off, const uint32_t* out_cap, uint32_t* out_len, uint32_t* consumed,
                                         int32_t* status, uint32_t n, void* stream) {
    if (n == 0) return NX_OK;
    if (!in || !in_off || !in_len || !out || !out_off || !out_cap || !out_len || !consumed || !status) return NX_ERR_INVALID_ARG;
    NX_CLEAR_STALE_ERROR();
    int dev = 0, cus = 256;
    NX_HIP_CHECK(hipGetDevice(&dev));
    NX_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    hipStream_t st = (hipStream_t)stream;
    nx::WsLease lease(nx::WsKind::Bzip2Dec, dev, st);
    size_t first = 0, count = 0;  // one slot per wave of the launch; a wave takes streams blockIdx.x, + gridDim.x, ...
    NX_HIP_CHECK(lease.acquire_part(nx::ws_want(nx::WsKind::Bzip2Dec, n, cus), &first, &count));
    uint8_t* ws = static_cast<uint8_t*>(lease.ws().p) + first * nx::kBzip2DecSlotBytes;
    hipLaunchKernelGGL(nx::bz2d::k_bzip2_decode, dim3((unsigned)count), dim3(64), 0, st, in, in_off, in_len, out, out_off, out_cap, ws,
                       out_len, consumed, status, n);
    NX_HIP_CHECK(hipGetLastError());
    return NX_OK;
}

// Size the block workspace now: slots for max_streams streams in flight (at most kBzip2DecWavesPerCu waves
// per CU), and never more until nx_workspaces_trim; a batch of more streams runs on those slots, a wave
// taking several streams in turn.  A server calls it at start-up; a batch call without it sizes the
// workspace itself.
extern "C" int32_t nx_bzip2_decoder_reserve(uint32_t max_streams, void* stream) {
    if (max_streams == 0) return NX_ERR_INVALID_ARG;
    int dev = 0;
    NX_HIP_CHECK(hipGetDevice(&dev));
    nx::SharedWs& W = nx::shared_ws(nx::WsKind::Bzip2Dec, dev);
    {
        std::lock_guard<std::mutex> lk(W.mu);
        if (W.p && W.slots > max_streams) return NX_ERR_INVALID_ARG;  // already larger than the cap: trim first
        W.cap = max_streams;
    }
    const int32_t r = nx::ws_hold(nx::WsKind::Bzip2Dec, dev, max_streams, (hipStream_t)stream);
    if (r != NX_OK) return r;
    {
        std::lock_guard<std::mutex> lk(W.mu);
        W.kept = true;
    }
    nx::ws_unhold(nx::WsKind::Bzip2Dec, dev);
    return NX_OK;
}

// chains the inverse BWT walk of a block is split into (the tests size their edge cases by it)
extern "C" uint32_t nx_bzip2_decode_chains(void) { return nx::bz2d::kChains; }
