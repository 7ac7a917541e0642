// zlib_jobs.hpp — the device side of JdkZlibDecoder jobs on the batcher (zlib_jobs.hip; DESIGN.md §4
// "zlib jobs on the batcher").  A flush runs every decoder job's body step as one stream of one
// nx_inflate_batch call; these two launches move what a stream carries between flushes (its inflate state
// and the last 32 KiB it produced, both in the handle's device memory) into and out of the batch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nx {
namespace zj {

constexpr uint32_t kHist = 32768;

struct DecStream {            // one stream of the flush, written by the host and uploaded with the launch lists
    uint8_t* state;           // the handle's inflate state, NX_INFLATE_STATE_BYTES
    const uint8_t* carry_in;  // the handle's current carry: `hist` bytes ending at carry_in + kHist
    uint8_t* carry_out;       // its other carry buffer (kHist bytes used), never the same as carry_in
    uint64_t win;             // the stream's window in the batch's window region: [kHist history | out_cap], 128-byte aligned
    uint64_t out_off;         // the job's reservation (out_cap bytes, 16-byte aligned) in the result arena
    uint32_t hist;            // <= kHist
    uint32_t out_cap;
    uint32_t fresh;           // the stream starts from the all-zero state (a new member)
    uint32_t pad;
};
struct DecRes {  // per stream, for apply()
    uint32_t consumed, out_len;
    int32_t status;
    uint32_t sum;  // CRC32 / Adler32 of the out_len bytes (whichever the stream's list computed)
};

// history and state of every stream into the batch: win + zs[i].win, state + i * NX_INFLATE_STATE_BYTES
int32_t dec_begin(const DecStream* zs, uint32_t n, uint8_t* win, uint8_t* state, hipStream_t s);
// after the inflate and checksum launches: state and carry back to the handles, the output bytes to
// out + zs[i].out_off, the records to res
int32_t dec_finish(const DecStream* zs, uint32_t n, const uint8_t* win, const uint8_t* state, const uint32_t* consumed,
                   const uint32_t* out_len, const int32_t* status, const uint32_t* sum, uint8_t* out, DecRes* res, hipStream_t s);

}  // namespace zj
}  // namespace nx
