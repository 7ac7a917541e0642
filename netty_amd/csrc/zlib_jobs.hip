// zlib_jobs.hip — gather / scatter kernels around the batcher's one nx_inflate_batch call per flush
// (zlib_jobs.hpp).  The work is mapped over (stream, chunk) pairs: blockIdx.y walks the streams,
// the waves of blockIdx.x share a stream's bytes in 4 KiB chunks, so a 1 MiB output beside a 30-byte one
// is copied by many waves.  Every length is clamped to what the host wrote (hist <= 32768, out_len <=
// out_cap): no store leaves the stream's window, its reservation or the handle's carry.
#include "zlib_jobs.hpp"
#include "../../include/netty_amd.h"
#include "nx_common.hpp"
#include "wave_copy.hpp"

namespace nx {
namespace zj {

typedef uint32_t v4 __attribute__((ext_vector_type(4)));
static_assert(NX_INFLATE_STATE_BYTES == 32 * sizeof(v4), "one 16-byte access per lane of half a wave");

__global__ void __launch_bounds__(256) k_zlib_dec_begin(const DecStream* __restrict__ zs, uint32_t n, uint8_t* __restrict__ win,
                                                        uint8_t* __restrict__ state) {
    const int lane = threadIdx.x & 63;
    const uint32_t wave = blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = gridDim.x * 4;
    for (uint32_t j = blockIdx.y; j < n; j += gridDim.y) {
        const DecStream Z = zs[j];
        const uint32_t hist = Z.hist < kHist ? Z.hist : kHist;
        nx::bt::tiled_copy(win + Z.win + kHist - hist, Z.carry_in + kHist - hist, hist, wave, nwaves, lane);
        if (blockIdx.x == 0 && threadIdx.x < 32) {
            const v4 zero = {0, 0, 0, 0};
            reinterpret_cast<v4*>(state + (size_t)j * NX_INFLATE_STATE_BYTES)[threadIdx.x] =
                Z.fresh ? zero : reinterpret_cast<const v4*>(Z.state)[threadIdx.x];
        }
    }
}

__global__ void __launch_bounds__(256) k_zlib_dec_finish(const DecStream* __restrict__ zs, uint32_t n, const uint8_t* __restrict__ win,
                                                         const uint8_t* __restrict__ state, const uint32_t* __restrict__ consumed,
                                                         const uint32_t* __restrict__ out_len, const int32_t* __restrict__ status,
                                                         const uint32_t* __restrict__ sum, uint8_t* __restrict__ out,
                                                         DecRes* __restrict__ res) {
    const int lane = threadIdx.x & 63;
    const uint32_t wave = blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = gridDim.x * 4;
    for (uint32_t j = blockIdx.y; j < n; j += gridDim.y) {
        const DecStream Z = zs[j];
        const uint32_t m = out_len[j] < Z.out_cap ? out_len[j] : Z.out_cap;
        const uint32_t hist = Z.hist < kHist ? Z.hist : kHist;
        const uint8_t* W = win + Z.win;
        if (m) {
            // the last h bytes of [history | output] are the stream's next history
            const uint32_t h = hist + m < kHist ? hist + m : kHist;
            nx::bt::tiled_copy(Z.carry_out + kHist - h, W + kHist + m - h, h, wave, nwaves, lane);
            nx::bt::tiled_copy(out + Z.out_off, W + kHist, m, wave, nwaves, lane);
        }
        if (blockIdx.x == 0) {
            if (threadIdx.x < 32)
                reinterpret_cast<v4*>(Z.state)[threadIdx.x] = reinterpret_cast<const v4*>(state + (size_t)j * NX_INFLATE_STATE_BYTES)[threadIdx.x];
            if (threadIdx.x == 32) res[j] = DecRes{consumed[j], m, status[j], sum[j]};
        }
    }
}

// Device-only copies: up to 1024 blocks.  The finish kernel's output stores cross PCIe when the result
// arena is mapped host memory, so its grid is capped like the other finish kernels' (64 blocks: the
// link's speed, not the CUs', bounds it, and a wider grid holds the CUs the next flush needs).
static dim3 grid_for(uint32_t n, uint32_t max_blocks) {
    const uint32_t gy = n < max_blocks ? n : max_blocks;
    const uint32_t gx = max_blocks / gy < 8u ? max_blocks / gy : 8u;
    return dim3(gx ? gx : 1u, gy);
}

int32_t dec_begin(const DecStream* zs, uint32_t n, uint8_t* win, uint8_t* state, hipStream_t s) {
    if (!n) return NX_OK;
    hipLaunchKernelGGL(k_zlib_dec_begin, grid_for(n, 1024), dim3(256), 0, s, zs, n, win, state);
    NX_HIP_CHECK(hipGetLastError());
    return NX_OK;
}

int32_t dec_finish(const DecStream* zs, uint32_t n, const uint8_t* win, const uint8_t* state, const uint32_t* consumed,
                   const uint32_t* out_len, const int32_t* status, const uint32_t* sum, uint8_t* out, DecRes* res, hipStream_t s) {
    if (!n) return NX_OK;
    hipLaunchKernelGGL(k_zlib_dec_finish, grid_for(n, 64), dim3(256), 0, s, zs, n, win, state, consumed, out_len, status, sum, out, res);
    NX_HIP_CHECK(hipGetLastError());
    return NX_OK;
}

}  // namespace zj
}  // namespace nx
