// brotli_decode.hip — Brotli stream decoder over a batch of complete streams (nx_brotli_decode_batch; what
// BrotliDecoder.java gets from brotli4j's DecoderJNI, one stream per item).
//
// One wave per stream (a block is one wave), as k_zstd_decode and k_inflate: the lanes of a wave share every
// branch.  The format logic is brotli_decode_core.hpp, the same functions the host decoder runs: lane 0 parses
// the headers, builds the trees and decodes the commands and their literals; its results reach the other lanes
// through a mailbox and an Op in LDS.  The wave-level parts are here:
//   - an uncompressed meta-block is a wave copy from the input;
//   - a step's literals are flushed from an LDS stage (1 KiB), 64 bytes per pass;
//   - a copy runs 64 bytes per pass, an overlapping copy reading source byte k mod distance, so every source
//     byte lies before the copy; the lanes that hold its last two bytes hand them to the core (State::p1, p2),
//     which needs them for the next literal's context;
//   - a dictionary word is transformed into LDS by lane 0 and stored by the wave.
// The wave reads back its own output (copies) under inflate.hip's discipline: wait for the wave's own stores
// (s_waitcnt vmcnt(0)), then load with agent scope, past the vector L1.
//
// A meta-block's trees can reach 256 literal trees of 256 symbols, 256 command trees of 704 and 256 distance
// trees of 520 (16 + 120 + (48 << 3)); they do not fit LDS, so they live in the stream's slot of the BrotliDec
// workspace as compact canonical tables (per tree 16 counts and the symbols sorted by code, two bytes each):
//   256 x (32 + 512) + 256 x (32 + 1408) + 256 x (32 + 1040)  literal, command and distance trees   782 336
//   3 x (32 + 516) + 3 x (32 + 52)                             block-type and block-count trees       1 896
//   32 + 544                                                   the context maps' own code (272)         576
//   256 x 64 + 256 x 4                                         the two context maps                  17 408
// 802 216 bytes, rounded up to 802 304 (a multiple of 256).  Only lane 0 reads and writes the slot, with plain
// loads and stores: a lane sees its own stores in program order.
//
// Nothing is assumed about the input: the core checks a step against MLEN and out_cap before it hands it over,
// and a copy's distance against the bytes produced, so the copies need no checks of their own and no store
// leaves [out_off, out_off + out_cap); no load leaves [in_off, in_off + in_len).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <mutex>
#include "../../include/netty_amd.h"
#include "nx_common.hpp"
#include "workspace.hpp"
#include "brotli_decode_core.hpp"

namespace nx {
namespace brd {

static_assert(sizeof(Slot) <= kBrotliDecSlotBytes, "the slot holds a meta-block's trees and maps at their maxima");
static_assert(sizeof(Slot) + 256u > kBrotliDecSlotBytes, "the slot size is the derived bound, rounded up to 256");

constexpr uint32_t kStage = 1024;
struct WaveLds {
    State S;
    Op op;
    uint8_t stage[kStage];
    uint32_t mail[8];
};

__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// the wave's own earlier stores have landed: what it wrote may now be loaded with agent scope
__device__ __forceinline__ void own_stores_done() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
__device__ __forceinline__ uint32_t load_own(const uint8_t* p) {
    return (uint32_t)__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ void decode_stream(WaveLds& L, const uint8_t* in, uint32_t n, uint8_t* out, uint32_t cap, Slot* W, const uint8_t* dict,
                              uint32_t* out_len, uint32_t* consumed, int32_t* status, int lane) {
    wave_sync();
    if (lane == 0) L.mail[0] = (uint32_t)begin(L.S, in, n, cap);
    wave_sync();
    int32_t st = (int32_t)uni(L.mail[0]);
    uint32_t used = 0;
    while (st == NX_OK) {  // every pass consumes a meta-block header of the input
        wave_sync();
        if (lane == 0) {
            MbHead H;
            L.mail[0] = (uint32_t)metablock_header(L.S, W, nullptr, &H);
            L.mail[1] = H.kind;
            L.mail[2] = H.src;
            L.mail[3] = H.len;
            L.mail[4] = H.pos;
            L.mail[5] = L.S.is_last;
        }
        wave_sync();
        st = (int32_t)uni(L.mail[0]);
        if (st != NX_OK) break;
        const uint32_t kind = uni(L.mail[1]), last = uni(L.mail[5]);
        if (kind == kMbUncompressed) {
            const uint32_t src = uni(L.mail[2]), len = uni(L.mail[3]), at = uni(L.mail[4]);
            for (uint32_t k = (uint32_t)lane; k < len; k += 64u) out[at + k] = in[src + k];  // len = MLEN, checked against out_cap and in_len
        } else if (kind == kMbCompressed) {
            for (;;) {  // every step produces a byte at least, of MLEN
                wave_sync();
                if (lane == 0) L.mail[0] = (uint32_t)step(L.S, W, dict, nullptr, L.stage, kStage, &L.op);
                wave_sync();
                st = (int32_t)uni(L.mail[0]);
                if (st != NX_OK) break;
                const uint32_t nl = uni(L.op.n_lit), cl = uni(L.op.copy_len), dist = uni(L.op.dist), wl = uni(L.op.word_len);
                uint8_t* o = out + uni(L.op.pos);
                for (uint32_t k = (uint32_t)lane; k < nl; k += 64u) o[k] = L.stage[k];  // nl <= kStage
                o += nl;
                if (cl) {
                    own_stores_done();
                    const uint8_t* s0 = o - dist;
                    for (uint32_t k = (uint32_t)lane; k < cl; k += 64u) {  // cl <= MLEN's rest and out_cap's
                        const uint32_t v = load_own(s0 + (dist < cl ? k % dist : k));  // an overlapping copy repeats its first `dist` bytes
                        o[k] = (uint8_t)v;
                        if (k + 1u == cl) L.S.p1 = v;
                        if (k + 2u == cl) L.S.p2 = v;
                    }
                }
                for (uint32_t k = (uint32_t)lane; k < wl; k += 64u) o[k] = L.op.word[k];  // wl <= 37
                if (uni(L.op.done)) break;
            }
            if (st != NX_OK) break;
        }
        if (last) {
            wave_sync();
            if (lane == 0) {
                uint32_t c = 0;
                L.mail[0] = (uint32_t)finish(L.S, &c);
                L.mail[1] = c;
            }
            wave_sync();
            st = (int32_t)uni(L.mail[0]);
            used = uni(L.mail[1]);
            break;
        }
    }
    wave_sync();
    if (lane == 0) {
        st = settle(L.S, st);
        *consumed = st == NX_OK ? used : 0u;
        *out_len = L.S.pos;
        *status = st;
    }
}

__global__ void __launch_bounds__(64) k_brotli_decode(const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off,
                                                      const uint32_t* __restrict__ in_len, uint8_t* out,
                                                      const uint64_t* __restrict__ out_off, const uint32_t* __restrict__ out_cap,
                                                      uint8_t* ws, const uint8_t* __restrict__ dict, uint32_t* out_len,
                                                      uint32_t* consumed, int32_t* status, uint32_t n) {
    __shared__ WaveLds L;
    const int lane = (int)threadIdx.x;
    Slot* W = reinterpret_cast<Slot*>(ws + (size_t)blockIdx.x * kBrotliDecSlotBytes);
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {  // the wave's share of the n items
        decode_stream(L, in + in_off[i], uni(in_len[i]), out + out_off[i], uni(out_cap[i]), W, dict, out_len + i, consumed + i,
                      status + i, lane);
        wave_sync();
    }
}

// The static dictionary on device `dev`: uploaded at the first call, kept for the life of the process.
constexpr int kMaxDictDevices = 64;
static std::mutex g_dict_mu;
static uint8_t* g_dict[kMaxDictDevices];
static int32_t device_dictionary(int dev, const uint8_t** d) {
    if (dev < 0 || dev >= kMaxDictDevices) return NX_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(g_dict_mu);
    if (!g_dict[dev]) {
        size_t size = 0;
        const uint8_t* host = nx_brotli_dictionary(&size);
        if (size != kDictBytes) return NX_ERR_INTERNAL;
        uint8_t* p = nullptr;
        NX_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&p), kDictBytes));
        const hipError_t e = hipMemcpy(p, host, kDictBytes, hipMemcpyHostToDevice);  // blocking: complete before any launch reads it
        if (e != hipSuccess) {
            (void)hipFree(p);
            NX_HIP_CHECK(e);
        }
        g_dict[dev] = p;
    }
    *d = g_dict[dev];
    return NX_OK;
}

}  // namespace brd
}  // namespace nx

extern "C" int32_t nx_brotli_decode_batch(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint8_t* out,
                                          const uint64_t* out_off, const uint32_t* out_cap, uint32_t* out_len, uint32_t* consumed,
                                          int32_t* status, uint32_t n, void* stream) {
    if (n == 0) return NX_OK;
    if (!in || !in_off || !in_len || !out || !out_off || !out_cap || !out_len || !consumed || !status) return NX_ERR_INVALID_ARG;
    NX_CLEAR_STALE_ERROR();
    int dev = 0, cus = 256;
    NX_HIP_CHECK(hipGetDevice(&dev));
    NX_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    const uint8_t* dict = nullptr;
    const int32_t r = nx::brd::device_dictionary(dev, &dict);
    if (r != NX_OK) return r;
    hipStream_t st = (hipStream_t)stream;
    nx::WsLease lease(nx::WsKind::BrotliDec, dev, st);
    size_t first = 0, count = 0;  // one slot per wave of the launch; a wave takes streams blockIdx.x, + gridDim.x, ...
    NX_HIP_CHECK(lease.acquire_part(nx::ws_want(nx::WsKind::BrotliDec, n, cus), &first, &count));
    uint8_t* ws = static_cast<uint8_t*>(lease.ws().p) + first * nx::kBrotliDecSlotBytes;
    hipLaunchKernelGGL(nx::brd::k_brotli_decode, dim3((unsigned)count), dim3(64), 0, st, in, in_off, in_len, out, out_off, out_cap, ws,
                       dict, out_len, consumed, status, n);
    NX_HIP_CHECK(hipGetLastError());
    return NX_OK;
}

// Size the tree workspace now: slots for max_streams streams in flight (at most 4 waves per CU), and never more
// until nx_workspaces_trim; a batch of more streams runs on those slots, a wave taking several streams in turn.
// It also uploads the static dictionary, so that no later batch call does.
extern "C" int32_t nx_brotli_decoder_reserve(uint32_t max_streams, void* stream) {
    if (max_streams == 0) return NX_ERR_INVALID_ARG;
    int dev = 0;
    NX_HIP_CHECK(hipGetDevice(&dev));
    const uint8_t* dict = nullptr;  // the dictionary's blocking upload is paid here too, not at the first batch
    const int32_t up = nx::brd::device_dictionary(dev, &dict);
    if (up != NX_OK) return up;
    nx::SharedWs& W = nx::shared_ws(nx::WsKind::BrotliDec, dev);
    {
        std::lock_guard<std::mutex> lk(W.mu);
        if (W.p && W.slots > max_streams) return NX_ERR_INVALID_ARG;  // already larger than the cap: trim first
        W.cap = max_streams;
    }
    const int32_t r = nx::ws_hold(nx::WsKind::BrotliDec, dev, max_streams, (hipStream_t)stream);
    if (r != NX_OK) return r;
    {
        std::lock_guard<std::mutex> lk(W.mu);
        W.kept = true;
    }
    nx::ws_unhold(nx::WsKind::BrotliDec, dev);
    return NX_OK;
}
