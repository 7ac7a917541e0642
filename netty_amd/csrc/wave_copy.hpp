// wave_copy.hpp — the byte copies of the batcher's finish kernels (batcher.cpp, zlib_jobs.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nx {
namespace bt {

// Copy n bytes with the whole wave: 16-byte stores at 16-byte-aligned destinations (one PCIe write per
// lane when the destination is mapped host memory), bytes at the ragged ends.  The source may have any
// alignment.
__device__ inline void wave_copy(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, uint32_t n, int lane) {
    typedef uint32_t v4 __attribute__((ext_vector_type(4)));
    typedef v4 __attribute__((aligned(1))) v4u;
    const uint32_t head = (uint32_t)((16u - ((uintptr_t)dst & 15u)) & 15u) < n ? (uint32_t)((16u - ((uintptr_t)dst & 15u)) & 15u) : n;
    if ((uint32_t)lane < head) dst[lane] = src[lane];
    const uint32_t nv = (n - head) >> 4;
    uint32_t i = lane;
    for (; i + 192u < nv; i += 256u) {  // 4 KiB per wave per step: four loads in flight, then four stores
        v4 x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) x[u] = *reinterpret_cast<const v4u*>(src + head + 16u * (i + 64u * u));
#pragma unroll
        for (int u = 0; u < 4; ++u) *reinterpret_cast<v4*>(dst + head + 16u * (i + 64u * u)) = x[u];
    }
    for (; i < nv; i += 64u) *reinterpret_cast<v4*>(dst + head + 16u * i) = *reinterpret_cast<const v4u*>(src + head + 16u * i);
    const uint32_t t = head + (nv << 4);
    if (t + (uint32_t)lane < n) dst[t + lane] = src[t + lane];
}

// A copy of n bytes shared by `nwaves` waves: 4 KiB chunks cut at 16-byte-aligned destinations, chunk c to
// wave c mod nwaves, so every chunk but the first starts on an aligned store.
constexpr uint32_t kCopyChunk = 4096;
__device__ inline void tiled_copy(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, uint32_t n, uint32_t wave,
                                  uint32_t nwaves, int lane) {
    const uint32_t a = (uint32_t)((uintptr_t)dst & 15u);  // chunks are counted from dst rounded down to 16
    for (uint64_t v0 = (uint64_t)wave * kCopyChunk; v0 < (uint64_t)a + n; v0 += (uint64_t)nwaves * kCopyChunk) {
        const uint32_t lo = v0 < a ? 0u : (uint32_t)(v0 - a);
        const uint64_t end = v0 + kCopyChunk - a;
        const uint32_t hi = end < n ? (uint32_t)end : n;
        wave_copy(dst + lo, src + lo, hi - lo, lane);
    }
}

}  // namespace bt
}  // namespace nx
