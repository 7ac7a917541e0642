// zstd_decode.hip — Zstandard frame decoder over a batch of complete frames (nx_zstd_decode_batch and
// nx_zstd_decode_batch_ex, which also verifies a frame's content checksum; what Zstd.decompress does for
// ZstdDecoder.java, one frame per item).
//
// One wave per frame (a block is one wave), as k_inflate: the lanes of a wave share every branch and
// the tables fit its LDS.  The format logic is zstd_decode_core.hpp, the same functions the host decoder
// runs: lane 0 parses the headers, reads the distributions and the tree description and builds the
// tables in LDS (they persist across a frame's blocks for Repeat_Mode and Treeless literals); its
// results reach the other lanes through a mailbox in LDS.  The wave-level parts are here:
//   - Raw / RLE blocks and Raw / RLE literals are wave copies and fills;
//   - Huffman streams decode one lane per stream (1 or 4) through the table in LDS into the frame's
//     slot of the ZstdDec workspace (128 KiB, the most literals a block regenerates);
//   - sequences decode in tiles of 64 on lane 0 (the core's step: three interleaved FSE states, the
//     repeat offsets, every bound checked) into LDS as (literal length, match length, resolved offset);
//     the whole wave then runs the tile: literal runs and matches 64 bytes per step, an overlapping
//     match reading source byte k mod offset, so every source byte lies before the match;
//   - the content checksum (content_checksum): XXH64 of the frame's output, read back once.
// The wave reads back its own output (matches) and its own literals from HBM under inflate.hip's
// discipline: wait for the wave's own stores (s_waitcnt vmcnt(0)), then load with agent scope, past
// the vector L1.
//
// Nothing is assumed about the input: lane 0 validates a sequence against the literals left, the bytes
// produced and out_cap before it enters a tile, so the copies need no checks of their own and no store
// leaves [out_off, out_off + out_cap); no load leaves [in_off, in_off + in_len).
#include <hip/hip_runtime.h>
#include <algorithm>
#include "../../include/netty_amd.h"
#include "nx_common.hpp"
#include "workspace.hpp"
#include "zstd_decode_core.hpp"

namespace nx {
namespace zstdd {

struct WaveLds {
    Tables T;
    Entropy E;
    SeqCursor C;
    union {
        Seq tile[kTile];
        uint64_t stage[64];  // the checksum's staging, after the last block: 16 stripes, 8 bytes a lane
    };
    HufStreams S;
    uint32_t mail[8];
};
constexpr uint32_t kVerifyMail = 7;  // mail[7]: NX_ZSTD_DECODE_VERIFY_CHECKSUM of the launch (the blocks use mail[0..5])

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

// where a block's literals are
struct Lits {
    uint32_t kind;  // 0 the input (Raw), 1 one byte (RLE), 2 the workspace slot (Huffman)
    const uint8_t* p;
    uint32_t byte;
    __device__ __forceinline__ uint32_t at(uint32_t i) const { return kind == 0u ? (uint32_t)p[i] : kind == 1u ? byte : load_own(p + i); }
};

// One Compressed block: in[0, n) is its content; *pos advances by what it regenerates.
__device__ int32_t decode_block(WaveLds& L, const uint8_t* in, uint32_t n, uint32_t block_max, uint8_t* out, uint32_t cap,
                                uint8_t* ws, uint32_t* pos_io, int lane) {
    uint32_t pos = *pos_io;
    // literals: header, tree and stream geometry on lane 0
    wave_sync();
    if (lane == 0) {
        LitHeader LH;
        int32_t st = parse_literals_header(in, n, block_max, &LH);
        uint32_t tree = 0;
        if (st == NX_OK && LH.type >= 2u) {
            const uint8_t* body = in + LH.header_bytes;
            if (LH.type == 2u)
                st = huf_read_tree(L.T, L.E, body, LH.comp, &tree);
            else if (!L.E.huf_valid)
                st = NX_ERR_ZSTD_CORRUPT;  // Treeless with no earlier tree
            if (st == NX_OK) st = huf_streams(body + tree, LH.comp - tree, LH.streams, LH.regen, &L.S);
        }
        L.mail[0] = (uint32_t)st;
        L.mail[1] = LH.type;
        L.mail[2] = LH.header_bytes;
        L.mail[3] = LH.regen;
        L.mail[4] = LH.comp;
        L.mail[5] = tree;
    }
    wave_sync();
    int32_t st = (int32_t)uni(L.mail[0]);
    if (st != NX_OK) return st;
    const uint32_t ltype = uni(L.mail[1]), lhdr = uni(L.mail[2]), regen = uni(L.mail[3]), comp = uni(L.mail[4]), tree = uni(L.mail[5]);
    const uint8_t* body = in + lhdr;
    Lits lit{ltype < 2u ? ltype : 2u, ltype == 0u ? body : ws, ltype == 1u ? (uint32_t)body[0] : 0u};
    if (ltype >= 2u) {  // one lane per stream
        int32_t hs = NX_OK;
        if ((uint32_t)lane < L.S.count)
            hs = huf_decode_stream(L.T.huf, L.E.huf_log, body + tree + L.S.off[lane], L.S.len[lane], ws + L.S.out[lane], L.S.regen[lane]);
        if (__ballot(hs != NX_OK) != 0ull) return NX_ERR_ZSTD_CORRUPT;
        own_stores_done();
    }
    // sequences: header, tables and the initial states on lane 0
    const uint8_t* sq = body + comp;
    const uint32_t sn = n - lhdr - comp;
    wave_sync();
    if (lane == 0) {
        SeqHeader SH;
        int32_t s2 = parse_sequences_header(sq, sn, &SH);
        uint32_t at = SH.header_bytes;
        if (s2 == NX_OK && SH.nseq) {
            for (uint32_t w = 0; w < 3u && s2 == NX_OK; ++w) {
                uint32_t used = 0;
                s2 = seq_table(L.T, L.E, w, SH.modes[w], sq + at, sn - at, &used);
                at += used;
            }
            if (s2 == NX_OK) {
                L.E.seq_valid = 1;
                s2 = seq_begin(L.E, L.C, sq + at, sn - at, SH.nseq, pos, regen, cap);
            }
        }
        L.mail[0] = (uint32_t)s2;
        L.mail[1] = SH.nseq;
    }
    wave_sync();
    st = (int32_t)uni(L.mail[0]);
    if (st != NX_OK) return st;
    uint32_t left = uni(L.mail[1]), lit_at = 0;
    while (left != 0u) {  // every tile decodes at least one sequence or ends the block
        wave_sync();
        if (lane == 0) {
            uint32_t cnt = 0;
            L.mail[0] = (uint32_t)seq_decode_tile(L.T, L.E, L.C, L.tile, &cnt);
            L.mail[1] = cnt;
            L.mail[2] = L.C.left;
        }
        wave_sync();
        st = (int32_t)uni(L.mail[0]);
        const uint32_t cnt = uni(L.mail[1]);
        left = uni(L.mail[2]);
        for (uint32_t j = 0; j < cnt; ++j) {
            const uint32_t ll = uni(L.tile[j].ll), ml = uni(L.tile[j].ml), off = uni(L.tile[j].off);
            for (uint32_t k = (uint32_t)lane; k < ll; k += 64u) out[pos + k] = (uint8_t)lit.at(lit_at + k);
            lit_at += ll;
            pos += ll;
            own_stores_done();
            const uint32_t s0 = pos - off;
            for (uint32_t k = (uint32_t)lane; k < ml; k += 64u)
                out[pos + k] = (uint8_t)load_own(out + s0 + (off < ml ? k % off : k));  // an overlapping match repeats its first `off` bytes
            pos += ml;
        }
        if (st != NX_OK) {
            *pos_io = pos;
            return st;
        }
    }
    const uint32_t rest = regen - lit_at;  // the literals after the last sequence
    *pos_io = pos;
    if (rest > cap - pos) return NX_ERR_ZSTD_OUTPUT_FULL;
    for (uint32_t k = (uint32_t)lane; k < rest; k += 64u) out[pos + k] = (uint8_t)lit.at(lit_at + k);
    *pos_io = pos + rest;
    return NX_OK;
}

// The low 32 bits of XXH64 (seed 0) of out[0, len), a frame's whole regenerated content, which the wave
// reads back as its own stores.  A pass stages 16 stripes (512 bytes) in LDS, every lane fetching 8 of
// their bytes one by one (out has any alignment); XXH64's four accumulators are serial chains over the
// stripes, so lanes 0..3 then carry one each through the 16 in order.  Lane 0 merges the four and runs
// the tail and the avalanche.  The same value on every lane.
__device__ uint32_t content_checksum(WaveLds& L, const uint8_t* out, uint32_t len, int lane) {
    own_stores_done();
    const uint32_t stripes = len >> 5;
    uint64_t acc = xxh64_acc_init((uint32_t)lane & 3u, 0);
    for (uint32_t s0 = 0; s0 < stripes; s0 += 16u) {
        const uint32_t m = stripes - s0 < 16u ? stripes - s0 : 16u;
        wave_sync();  // the stage (and before the first pass the tile it shares memory with) has been read
        if ((uint32_t)lane < 4u * m) {
            const uint8_t* p = out + ((size_t)s0 << 5) + 8u * (uint32_t)lane;
            uint64_t v = 0;
            for (uint32_t b = 0; b < 8u; ++b) v |= (uint64_t)load_own(p + b) << (8u * b);
            L.stage[lane] = v;
        }
        wave_sync();
        if (lane < 4)
            for (uint32_t s = 0; s < m; ++s) acc = xxh64_round(acc, L.stage[4u * s + (uint32_t)lane]);
    }
    wave_sync();
    if (lane < 4) L.stage[lane] = acc;
    wave_sync();
    if (lane == 0) {
        const uint8_t* t = out + ((size_t)stripes << 5);
        L.mail[0] = (uint32_t)xxh64_finish(L.stage, len, 0, [t](uint32_t i) -> uint32_t { return load_own(t + i); });
    }
    wave_sync();
    return uni(L.mail[0]);
}

__device__ void decode_frame(WaveLds& L, const uint8_t* in, uint32_t n, uint8_t* out, uint32_t cap, uint8_t* ws, uint32_t* consumed,
                             uint32_t* out_len, int32_t* status, int lane) {
    FrameHeader H;
    int32_t st = (int32_t)uni((uint32_t)parse_frame_header(in, n, &H));  // the same on every lane
    // the launch's flags wait in the mailbox (kVerifyMail), read here only: nothing of them stays live in the blocks
    if (st == NX_OK && H.checksum && !uni(L.mail[kVerifyMail])) st = NX_ERR_ZSTD_CHECKSUM_UNSUPPORTED;
    uint32_t pos = 0, q = 0;
    if (st == NX_OK) {
        const uint32_t block_max = uni(H.block_max);
        q = uni(H.header_bytes);
        wave_sync();
        if (lane == 0) entropy_reset(L.E);
        for (;;) {  // every pass consumes a block header of the input
            BlockHeader B;
            st = (int32_t)uni((uint32_t)parse_block_header(in + q, n - q, block_max, &B));
            if (st != NX_OK) break;
            const uint32_t type = uni(B.type), size = uni(B.size);
            q += 3u;
            if (type == 2u) {
                st = decode_block(L, in + q, size, block_max, out, cap, ws, &pos, lane);
            } else if (size > cap - pos) {
                st = NX_ERR_ZSTD_OUTPUT_FULL;
            } else {
                const uint32_t fill = type == 1u ? (uint32_t)in[q] : 0u;  // (an empty Raw block may end the input)
                for (uint32_t k = (uint32_t)lane; k < size; k += 64u) out[pos + k] = (uint8_t)(type == 0u ? (uint32_t)in[q + k] : fill);
                pos += size;
            }
            if (st != NX_OK) break;
            q += uni(B.content);
            if (uni(B.last)) break;
        }
        const uint64_t fcs = H.content_size;
        if (st == NX_OK && fcs != UINT64_MAX && fcs != (uint64_t)pos) st = NX_ERR_ZSTD_CORRUPT;
        if (st == NX_OK && (uni(in[4]) & 4u)) {  // Content_Checksum, and the frame passed every other check: its four bytes
            if (n - q < 4u) {
                st = NX_ERR_ZSTD_TRUNCATED;
            } else if (content_checksum(L, out, pos, lane) != uni(le_bytes(in + q, 4))) {
                st = NX_ERR_ZSTD_CHECKSUM;
            } else {
                q += 4u;
            }
        }
    }
    if (lane == 0) {
        *consumed = st == NX_OK ? q : 0u;
        *out_len = pos;
        *status = st;
    }
}

__global__ void __launch_bounds__(64) k_zstd_decode(const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off,
                                                    const uint32_t* __restrict__ in_len, uint8_t* out,
                                                    const uint64_t* __restrict__ out_off, const uint32_t* __restrict__ out_cap,
                                                    uint8_t* ws, uint32_t verify, uint32_t* consumed, uint32_t* out_len,
                                                    int32_t* status, uint32_t n) {
    __shared__ WaveLds L;
    const int lane = (int)threadIdx.x;
    uint8_t* slot = ws + (size_t)blockIdx.x * kZstdDecSlotBytes;
    if (lane == 0) L.mail[kVerifyMail] = verify;
    wave_sync();
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        decode_frame(L, in + in_off[i], uni(in_len[i]), out + out_off[i], uni(out_cap[i]), slot, consumed + i, out_len + i, status + i,
                     lane);
        wave_sync();
    }
}

}  // namespace zstdd
}  // namespace nx

extern "C" int32_t nx_zstd_decode_batch_ex(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint8_t* out,
                                           const uint64_t* out_off, const uint32_t* out_cap, uint32_t* consumed, uint32_t* out_len,
                                           int32_t* status, uint32_t n, uint32_t flags, void* stream) {
    if (flags & ~NX_ZSTD_DECODE_VERIFY_CHECKSUM) return NX_ERR_INVALID_ARG;
    if (n == 0) return NX_OK;
    if (!in || !in_off || !in_len || !out || !out_off || !out_cap || !consumed || !out_len || !status) return NX_ERR_INVALID_ARG;
    NX_CLEAR_STALE_ERROR();
    int dev = 0, cus = 256;
    NX_HIP_CHECK(hipGetDevice(&dev));
    NX_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    hipStream_t st = (hipStream_t)stream;
    nx::WsLease lease(nx::WsKind::ZstdDec, dev, st);
    size_t first = 0, count = 0;  // one slot per wave of the launch; a wave takes frames blockIdx.x, + gridDim.x, ...
    NX_HIP_CHECK(lease.acquire_part(nx::ws_want(nx::WsKind::ZstdDec, n, cus), &first, &count));
    uint8_t* ws = static_cast<uint8_t*>(lease.ws().p) + first * nx::kZstdDecSlotBytes;
    hipLaunchKernelGGL(nx::zstdd::k_zstd_decode, dim3((unsigned)count), dim3(64), 0, st, in, in_off, in_len, out, out_off, out_cap, ws,
                       flags & NX_ZSTD_DECODE_VERIFY_CHECKSUM, consumed, out_len, status, n);
    NX_HIP_CHECK(hipGetLastError());
    return NX_OK;
}

extern "C" int32_t nx_zstd_decode_batch(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint8_t* out,
                                        const uint64_t* out_off, const uint32_t* out_cap, uint32_t* consumed, uint32_t* out_len,
                                        int32_t* status, uint32_t n, void* stream) {
    return nx_zstd_decode_batch_ex(in, in_off, in_len, out, out_off, out_cap, consumed, out_len, status, n, 0, stream);
}

// Size the literals workspace now: slots for max_frames frames in flight (at most 8 waves per CU), and
// never more until nx_workspaces_trim; a batch of more frames runs on those slots, a wave taking several
// frames in turn.  A server calls it at start-up; a batch call without it sizes the workspace itself.
extern "C" int32_t nx_zstd_decoder_reserve(uint32_t max_frames, void* stream) {
    if (max_frames == 0) return NX_ERR_INVALID_ARG;
    int dev = 0;
    NX_HIP_CHECK(hipGetDevice(&dev));
    nx::SharedWs& W = nx::shared_ws(nx::WsKind::ZstdDec, dev);
    {
        std::lock_guard<std::mutex> lk(W.mu);
        if (W.p && W.slots > max_frames) return NX_ERR_INVALID_ARG;  // already larger than the cap: trim first
        W.cap = max_frames;
    }
    const int32_t r = nx::ws_hold(nx::WsKind::ZstdDec, dev, max_frames, (hipStream_t)stream);
    if (r != NX_OK) return r;
    {
        std::lock_guard<std::mutex> lk(W.mu);
        W.kept = true;
    }
    nx::ws_unhold(nx::WsKind::ZstdDec, dev);
    return NX_OK;
}
