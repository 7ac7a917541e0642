// batcher.cpp — asynchronous, cross-channel batching executor for the Snappy frame handlers.
//
// Netty runs one SnappyFrameEncoder / SnappyFrameDecoder per channel on that channel's event loop
// (ByteToMessageDecoder.java:194-196) and the event loop must not block (BlockHound,
// common/.../internal/Hidden.java:38).  One encode()/decode() call carries ~1-33 chunks, far too few
// to fill an MI355X, so the batcher turns those calls into jobs of one shared GPU launch:
//
//   submit  (event loop, non-blocking)  the handler's framing runs on the host at once — the stream
//           identifier and slice split of SnappyFrameEncoder.encode (SnappyFrameEncoder.java:79-117),
//           the chunk-header walk of SnappyFrameDecoder.decode (:85-231) — so the handle's state
//           advances in call order; the chunk payloads are copied into a pinned staging arena
//           (MessageToByteEncoder releases `in` when encode() returns, :109), or, for an encoder input
//           the caller registered with nx_host_register and keeps alive, DMA'd straight from it.
//   flush   the staging arena and registered inputs to the device (one gather launch reading the
//           mapped pages; a large staging arena by one DMA copy), then ONE launch per kernel for every
//           job of every channel: CRC32C + Snappy.encode of all encoder slices, Snappy.decode (+ CRC
//           verify) of all compressed chunks, CRC32C of uncompressed chunks, and a finish kernel that
//           writes each job's result — framed encoder output, or the decoder's messages — straight
//           into mapped pinned host memory, or into a device mirror moved by one DMA copy when the
//           decoded messages fill most of a large result arena (only result bytes cross PCIe).
//   poll    hipEventQuery: 1 when the job's batch is done (never blocks); wait() blocks (tests).
//   streams flushes go round-robin to kStreams HIP streams, so one batch's host gather / result
//           writes (PCIe) overlap the next batch's kernels; results are still APPLIED in flush order
//           (a later batch waits for the earlier ones), which keeps each decoder's corrupted state
//           exactly as a serial execution would leave it.  An optional auto-flush threshold
//           (nx_batcher_set_flush_bytes) launches the collecting batch once its input reaches it.
//   result  zero-copy views of the job's output in the pinned arena, valid until release().
//
// Results are applied in submission order per decoder: a failing chunk marks the decoder corrupted
// (:227-230) and the jobs submitted after it on that decoder deliver nothing (Java skips all later
// input, :86-89).  A validating decoder's compressed chunk that decodes fewer bytes than its length
// leaves the rest to be parsed again as a chunk header (:206-212); that is known only at apply().  So a
// validating decoder keeps the bytes its unapplied jobs walked (and any partial chunk after them, which
// it carries into the next submit instead of leaving it in the caller's cumulation), and apply() walks
// them again from the leftover: the job continues in the collecting batch (launched by the next
// poll/wait) with the messages it has so far, and the decoder's jobs walked before that deliver
// nothing (their bytes are in the continuation).  Messages and errors equal the synchronous
// nx_snappy_frame_decoder_decode's, in the same order; they may arrive on an earlier ticket.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>
#include "../../include/netty_amd.h"
#include "frame_parse.hpp"
#include "handles.hpp"
#include "alt_frames.hpp"
#include "nx_common.hpp"
#include "wave_copy.hpp"
#include "workspace.hpp"
#include "zlib_jobs.hpp"

namespace nx {
namespace bt {

struct EncSlice {  // one SnappyFrameEncoder slice (:99-112) or the small-message unencoded chunk (:114-124)
    uint64_t in_off;
    uint64_t slot_off;
    uint32_t len;
    uint32_t comp;
};
struct EncJob {
    uint64_t out_off;  // in the mapped output arena
    uint32_t s0, ns;   // slices
    uint32_t stream_start;
    uint32_t pad;
};
struct DecAct {  // one UNCOMPRESSED_DATA (kind 1) or COMPRESSED_DATA (kind 2) chunk, in stream order
    uint64_t in_off;  // payload in the device input arena
    uint32_t len;     // payload bytes
    uint32_t kind;
    uint32_t chunk;   // kind 2: index into the decode batch; kind 1: index into the uncompressed-CRC batch
    uint32_t crc;     // stored masked CRC32C
    uint32_t cap;     // bytes reserved for its message: kind 2 the preamble's length (capped by the bound)
    uint32_t pad;
};
constexpr uint64_t kSpilled = ~0ull;  // DecRes::off of a message longer than its chunk's preamble said that
                                      // did not fit the flush's spill area (apply copies it from the slot)
constexpr uint64_t kSpillBytes = 1ull << 20;  // a flush's spill area (bytes; at most 64 KiB per compressed chunk)
struct DecJob {
    uint64_t out_off;
    uint32_t a0, na;
    uint32_t validate;
    uint32_t pad;
};
struct DecRes {  // per action, written by k_dec_finish
    uint64_t off;    // message bytes in the output arena
    uint32_t len;
    int32_t status;  // NX_OK or the chunk's error
    uint32_t crc;    // computed masked CRC32C (uncompressed chunks; compressed: see decode crc_out)
    uint32_t cons;   // compressed: input bytes consumed
};

// The kernels that move bytes across PCIe (k_gather_host reads mapped host pages, the finish kernels
// write the results into them) run on a capped grid, kPcieBlocks workgroups looping over the jobs:
// their speed is the link's, not the CUs', and a grid of one wave per job held every CU for the
// whole transfer, so the next batch's parse / expand / encode on another stream could not start
// (round 4 e2e trace: k_parse 5.9 ms alone, 17-23 ms beside a full-grid k_dec_finish).
#ifndef NX_PCIE_BLOCKS
#define NX_PCIE_BLOCKS 64
#endif
constexpr uint32_t kPcieBlocks = NX_PCIE_BLOCKS;
constexpr uint64_t kDmaOutMin = 64ull << 20;  // place(): result arenas at least this large may go by DMA
constexpr uint64_t kGatherStageMax = 8ull << 20;  // transfer_in(): staging arenas up to this size move by k_gather_host
constexpr uint64_t kGatherPiece = 64ull << 10;    // ... in ops of this many bytes
inline dim3 pcie_grid(uint32_t jobs) { return dim3(std::min((jobs + 3u) / 4u, kPcieBlocks)); }
// Registered host inputs -> the device input arena: one wave per input range, 16-byte loads from the
// mapped host pages (one launch instead of one DMA command per pooled-buffer message).
struct GatherOp {
    const uint8_t* src;  // device address of registered host memory
    uint64_t dst;        // offset in the device input arena
    uint64_t len;
};
__global__ void __launch_bounds__(256) k_gather_host(const GatherOp* __restrict__ ops, uint32_t n, uint8_t* __restrict__ din) {
    typedef uint32_t v4 __attribute__((ext_vector_type(4)));
    typedef v4 __attribute__((aligned(1))) v4u;
    const int lane = threadIdx.x & 63;
    for (uint32_t k = blockIdx.x * 4 + (threadIdx.x >> 6); k < n; k += gridDim.x * 4) {
        const GatherOp g = ops[k];
        uint8_t* d = din + g.dst;  // 16-byte aligned
        const uint64_t nv = g.len >> 4;
        uint64_t i = lane;
        for (; i + 192u < nv; i += 256u) {  // four PCIe reads per lane in flight
            v4 x[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) x[u] = *reinterpret_cast<const v4u*>(g.src + 16 * (i + 64u * u));
#pragma unroll
            for (int u = 0; u < 4; ++u) *reinterpret_cast<v4*>(d + 16 * (i + 64u * u)) = x[u];
        }
        for (; i < nv; i += 64) *reinterpret_cast<v4*>(d + 16 * i) = *reinterpret_cast<const v4u*>(g.src + 16 * i);
        for (uint64_t q = (nv << 4) + lane; q < g.len; q += 64) d[q] = g.src[q];
    }
}

// one wave per encoder job: [stream identifier] then [type][len+4: u24 LE][masked crc LE][payload] per slice
// res_len[j]: the job's framed bytes, or (negative) the Snappy.encode status of its first failing slice
__global__ void __launch_bounds__(256) k_enc_finish(const uint8_t* __restrict__ din, const uint8_t* __restrict__ slots,
                                                    const EncSlice* __restrict__ sl, const uint32_t* __restrict__ clen,
                                                    const int32_t* __restrict__ est, const uint32_t* __restrict__ crc,
                                                    const EncJob* __restrict__ jobs, uint32_t njobs, uint8_t* __restrict__ out,
                                                    int64_t* __restrict__ res_len) {
    const int lane = threadIdx.x & 63;
    for (uint32_t j = blockIdx.x * 4 + (threadIdx.x >> 6); j < njobs; j += gridDim.x * 4) [&] {
        const EncJob J = jobs[j];
        for (uint32_t s = J.s0; s < J.s0 + J.ns; ++s) {
            if (sl[s].comp && est[s] != NX_OK) {
                if (lane == 0) res_len[j] = est[s];
                return;
            }
        }
        uint8_t* o = out + J.out_off;
        uint64_t pos = 0;
        if (J.stream_start) {  // ff 06 00 00 "sNaPpY" (SnappyFrameEncoder.java:52-54)
            const uint64_t v = lane < 8 ? (0x50614e73000006ffull >> (8 * lane)) : (0x5970ull >> (8 * (lane - 8)));  // LE bytes
            if (lane < 10) o[lane] = (uint8_t)v;
            pos = 10;
        }
        for (uint32_t s = J.s0; s < J.s0 + J.ns; ++s) {
            const EncSlice S = sl[s];
            const uint32_t L = S.comp ? clen[s] : S.len;
            const uint32_t cl = L + 4;  // setChunkLength (:126-132) / writeUnencodedChunk (:119-124)
            const uint32_t c = crc[s];
            if (lane < 8) {
                const uint32_t b = lane == 0 ? (S.comp ? 0u : 1u) : lane < 4 ? (cl >> (8 * (lane - 1))) & 0xFF : (c >> (8 * (lane - 4))) & 0xFF;
                o[pos + lane] = (uint8_t)b;
            }
            wave_copy(o + pos + 8, S.comp ? slots + S.slot_off : din + S.in_off, L, lane);
            pos += 8 + L;
        }
        if (lane == 0) res_len[j] = (int64_t)pos;
    }();
}

// Bytes a Snappy block of clen bytes can decode to: at most 64 per 3 input bytes (a copy-2 tag; a
// copy-1 gives 11 per 2, a copy-4 64 per 5, a literal its own length), and never more than the frame
// decoder's 65536-byte buffer (SnappyFrameDecoder.java:203).  Sizes the decode slots and the job's
// output reservation, so a flush of many small chunks does not take 64 KiB for each.
__host__ __device__ inline uint32_t snappy_decoded_bound(uint32_t clen) {
    const uint64_t b = 64ull * ((clen + 2ull) / 3ull);
    return b < 65536u ? (uint32_t)b : 65536u;
}
inline uint64_t dec_slot_bytes(uint32_t clen) { return ((uint64_t)snappy_decoded_bound(clen) + 64u + 15u) & ~15ull; }

// one wave per decoder job: the decoded messages back to back, stopping at the first failing chunk
__global__ void __launch_bounds__(256) k_dec_finish(const uint8_t* __restrict__ din, const uint8_t* __restrict__ slots,
                                                    const uint64_t* __restrict__ dslot,
                                                    const DecAct* __restrict__ acts, const DecJob* __restrict__ jobs, uint32_t njobs,
                                                    const uint32_t* __restrict__ dlen, const uint32_t* __restrict__ dcons,
                                                    const int32_t* __restrict__ dstat, const uint32_t* __restrict__ dcrc,
                                                    const uint32_t* __restrict__ ucrc, uint8_t* __restrict__ out,
                                                    DecRes* __restrict__ res, uint64_t spill_off, uint32_t spill_cap,
                                                    uint32_t* __restrict__ spill_cur) {
    const int lane = threadIdx.x & 63;
    for (uint32_t j = blockIdx.x * 4 + (threadIdx.x >> 6); j < njobs; j += gridDim.x * 4) [&] {
        const DecJob J = jobs[j];
        uint64_t pos = J.out_off;
        for (uint32_t a = J.a0; a < J.a0 + J.na; ++a) {
            const DecAct A = acts[a];
            DecRes R{pos, 0, NX_OK, 0, 0};
            if (A.kind == 1) {
                R.crc = ucrc[A.chunk];
                R.len = A.len;
                if (J.validate && R.crc != A.crc) R.status = NX_ERR_SNAPPY_CRC_MISMATCH;  // (:171-175)
                else wave_copy(out + pos, din + A.in_off, A.len, lane);
            } else {
                R.status = dstat[A.chunk];
                // the decode launch verifies CRCs when any decoder of the batch validates; a decoder
                // built without validateChecksums ignores them (:205-216)
                if (R.status == NX_ERR_SNAPPY_CRC_MISMATCH && !J.validate) R.status = NX_OK;
                R.len = dlen[A.chunk];
                R.crc = dcrc[A.chunk];
                R.cons = dcons[A.chunk];
                if (R.status == NX_ERR_SNAPPY_LITERAL_LEN_INVALID && R.cons >= 4u) {  // the literal's length field, for the message
                    const uint8_t* f = din + A.in_off + R.cons - 4u;
                    R.crc = f[0] | (f[1] << 8) | (f[2] << 16) | ((uint32_t)f[3] << 24);
                }
                // a chunk that decodes past its preamble's length (Java allows it up to 65 536 bytes,
                // SnappyFrameDecoder.java:203) has no room here: it goes to the flush's spill area, or,
                // when that is full, apply() copies it from the slot
                if (R.status == NX_OK && R.len > A.cap) {
                    uint32_t at = 0;
                    if (lane == 0) at = atomicAdd(spill_cur, R.len);
                    at = (uint32_t)__shfl((int)at, 0);
                    if ((uint64_t)at + R.len <= spill_cap) {
                        R.off = spill_off + at;
                        wave_copy(out + R.off, slots + dslot[A.chunk], R.len, lane);
                    } else {
                        R.off = kSpilled;
                    }
                    if (lane == 0) res[a] = R;
                    continue;  // the message reservation holds nothing of it: pos stays
                } else if (R.status == NX_OK) {
                    wave_copy(out + pos, slots + dslot[A.chunk], R.len, lane);
                }
            }
            if (lane == 0) res[a] = R;
            if (R.status != NX_OK) break;
            pos += R.len;
        }
    }();
}

// ---------------------------------------------------------------- FastLZ / LZF / LZ4 jobs
// An alt-codec job's output is a list of PIECES in stream order: for an encoder one framed block each
// (written back to back into the job's output), for a decoder one block's message each.  The codec
// kernels of the flush leave their results in the alt slots and result arrays; k_alt_finish (one wave
// per job) writes each piece into mapped host memory and records where it went.
enum : uint32_t {
    AK_FLZ_ENC = 1,  // FastLzFrameEncoder block (:115-168): header, then compressed (slot) or raw (input) bytes
    AK_LZF_ENC,      // a complete "ZV" block from the LZF encoder (slot)
    AK_LZF_RAW,      // a non-compressed "ZV" block (encodeNonCompress, LzfEncoder.java:223-246)
    AK_LZ4_ENC,      // a framed block from the LZ4 frame encoder (slot; header included)
    AK_LZ4_END,      // Lz4FrameEncoder's end block (:326-335)
    AK_RAW,          // input bytes as they are (Lz4FrameEncoder after close(), :233-239)
    AK_DEC_FLZ,      // a FastLZ block decoded into its slot
    AK_DEC_LZF,      // an LZF block decoded into its slot
    AK_DEC_LZ4,      // an LZ4 block decoded into its slot
    AK_DEC_RAW,      // a non-compressed block: its payload (input)
    AK_DFL_ENC,      // a JdkZlibEncoder slice deflated into its slot (aux: its checksum, as for decoder pieces)
    AK_CONST,        // len <= 16 literal bytes held in src (the first 8, little-endian) and slot: JdkZlibEncoder's
                     // header, and its final block with the trailer's place (the host writes the trailer at apply)
};
struct AltPiece {
    uint64_t src;   // input arena offset of the raw bytes / payload
    uint64_t slot;  // alt slot offset of the codec's output
    uint32_t len;   // input bytes
    uint32_t olen;  // decoder: decoded bytes
    uint32_t kind;
    uint32_t res;   // index into the codec's result arrays
    uint32_t aux;   // AK_FLZ_ENC: bit 0 = with Adler32; AK_LZ4_END: compression level; decoder pieces with a
                    // checksum: 1 + its index in AltArrays::dcks (assigned at flush)
    uint32_t cks;   // decoder and deflate pieces, host only: the checksum to compute (CK_*)
};
enum : uint32_t { CK_NONE = 0, CK_ADLER32 = 1, CK_XXH32 = 2, CK_CRC32 = 3 };
struct AltJobD {
    uint64_t out_off;  // in the mapped output arena
    uint32_t p0, np;   // pieces
};
struct AltRes {  // per piece
    uint64_t off;    // bytes in the output arena
    uint32_t len;    // AK_DEC_FLZ failing: decompress()'s return value
    int32_t status;  // NX_OK, or the codec status
    uint32_t cks;    // decoder pieces with a checksum: Adler32 / XXH32 of the block's bytes
    uint32_t pad;
};
struct AltArrays {  // the flush's codec result arrays (device)
    const uint32_t* flz_clen;
    const int32_t* flz_st;
    const uint32_t* flz_adler;
    const uint32_t* lzf_olen;
    const int32_t* lzf_st;
    const uint32_t* lz4_olen;
    const int32_t* lz4_st;
    const int32_t* dflz_r;
    const int32_t* dlzf_st;
    const int32_t* dlz4_st;
    const uint32_t* dcks;  // decoder and deflate piece checksums, indexed by AltPiece::aux - 1
    const uint32_t* dfl_olen;  // deflate slices: the stored-only launch's, then the matcher launch's
    const int32_t* dfl_st;
};

__global__ void __launch_bounds__(256) k_alt_finish(const uint8_t* __restrict__ din, const uint8_t* __restrict__ aslots,
                                                    const AltPiece* __restrict__ pcs, const AltJobD* __restrict__ jobs, uint32_t njobs,
                                                    AltArrays R, uint8_t* __restrict__ out, AltRes* __restrict__ res) {
    const int lane = threadIdx.x & 63;
    for (uint32_t j = blockIdx.x * 4 + (threadIdx.x >> 6); j < njobs; j += gridDim.x * 4) [&] {
        const AltJobD J = jobs[j];
        uint64_t pos = J.out_off;
        for (uint32_t k = J.p0; k < J.p0 + J.np; ++k) {
            const AltPiece P = pcs[k];
            AltRes r{pos, 0, NX_OK, 0, 0};
            if (P.kind >= AK_DEC_FLZ && P.aux) r.cks = R.dcks[P.aux - 1];
            uint8_t* o = out + pos;
            switch (P.kind) {
                case AK_FLZ_ENC: {  // FastLzFrameEncoder.java:115-168
                    const bool cks = (P.aux & 1u) != 0;
                    const int32_t st = R.flz_st[P.res];
                    if (st != NX_OK) {
                        r.status = st;
                        break;
                    }
                    const uint32_t clen = R.flz_clen[P.res];
                    const bool comp = P.len >= 32u && clen < P.len;  // MIN_LENGTH_TO_COMPRESSION, :150-158
                    const uint32_t hdr = 4u + (cks ? 4u : 0u) + (comp ? 4u : 2u);
                    if (lane == 0) {
                        o[0] = 'F';
                        o[1] = 'L';
                        o[2] = 'Z';
                        o[3] = (uint8_t)((comp ? 1u : 0u) | (cks ? 0x10u : 0u));
                        uint32_t q = 4;
                        if (cks) {
                            const uint32_t a = R.flz_adler[P.res];
                            o[4] = (uint8_t)(a >> 24);
                            o[5] = (uint8_t)(a >> 16);
                            o[6] = (uint8_t)(a >> 8);
                            o[7] = (uint8_t)a;
                            q = 8;
                        }
                        if (comp) {
                            o[q] = (uint8_t)(clen >> 8);
                            o[q + 1] = (uint8_t)clen;
                            q += 2;
                        }
                        o[q] = (uint8_t)(P.len >> 8);
                        o[q + 1] = (uint8_t)P.len;
                    }
                    if (comp) wave_copy(o + hdr, aslots + P.slot, clen, lane);
                    else wave_copy(o + hdr, din + P.src, P.len, lane);
                    r.len = hdr + (comp ? clen : P.len);
                    break;
                }
                case AK_LZF_ENC:
                case AK_LZ4_ENC: {
                    const int32_t st = P.kind == AK_LZF_ENC ? R.lzf_st[P.res] : R.lz4_st[P.res];
                    if (st != NX_OK) {
                        r.status = st;
                        break;
                    }
                    r.len = P.kind == AK_LZF_ENC ? R.lzf_olen[P.res] : R.lz4_olen[P.res];
                    wave_copy(o, aslots + P.slot, r.len, lane);
                    break;
                }
                case AK_LZF_RAW:  // LZFChunk.appendNonCompressed: 'Z' 'V' 0 len(BE16) bytes
                    if (lane == 0) {
                        o[0] = 'Z';
                        o[1] = 'V';
                        o[2] = 0;
                        o[3] = (uint8_t)(P.len >> 8);
                        o[4] = (uint8_t)P.len;
                    }
                    wave_copy(o + 5, din + P.src, P.len, lane);
                    r.len = 5u + P.len;
                    break;
                case AK_LZ4_END:  // magic, token = BLOCK_TYPE_NON_COMPRESSED | level, then 12 zero bytes
                    if (lane < 21) o[lane] = lane < 8 ? (uint8_t)"LZ4Block"[lane] : (lane == 8 ? (uint8_t)(0x10u | P.aux) : 0);
                    r.len = 21;
                    break;
                case AK_RAW:
                case AK_DEC_RAW:
                    wave_copy(o, din + P.src, P.len, lane);
                    r.len = P.len;
                    break;
                case AK_DEC_FLZ: {  // FastLzFrameDecoder.java:154-165: decompress() must return originalLength
                    const int32_t v = R.dflz_r[P.res];
                    if (v < 0 || (uint32_t)v != P.olen) {
                        r.status = v < 0 ? v : NX_ERR_FASTLZ_LENGTH_MISMATCH;
                        r.len = (uint32_t)v;  // the value, for the message
                        break;
                    }
                    wave_copy(o, aslots + P.slot, P.olen, lane);
                    r.len = P.olen;
                    break;
                }
                case AK_DEC_LZF:
                case AK_DEC_LZ4: {
                    const int32_t st = P.kind == AK_DEC_LZF ? R.dlzf_st[P.res] : R.dlz4_st[P.res];
                    if (st != NX_OK) {
                        r.status = st;
                        break;
                    }
                    wave_copy(o, aslots + P.slot, P.olen, lane);
                    r.len = P.olen;
                    break;
                }
                case AK_DFL_ENC: {
                    const int32_t st = R.dfl_st[P.res];
                    if (st != NX_OK) {
                        r.status = st;
                        break;
                    }
                    r.len = R.dfl_olen[P.res];
                    wave_copy(o, aslots + P.slot, r.len, lane);
                    break;
                }
                case AK_CONST:
                    if ((uint32_t)lane < P.len && lane < 16) o[lane] = (uint8_t)((lane < 8 ? P.src : P.slot) >> (8 * (lane & 7)));
                    r.len = P.len < 16u ? P.len : 16u;
                    break;
                default:
                    r.status = NX_ERR_INTERNAL;
            }
            if (lane == 0) res[k] = r;
            if (r.status != NX_OK) break;
            pos += r.len;
        }
    }();
}

}  // namespace bt
}  // namespace nx

using nx::bt::DecAct;
using nx::bt::DecJob;
using nx::bt::DecRes;
using nx::bt::EncJob;
using nx::bt::EncSlice;
using nx::fr::SAct;
using nx::fr::SnappyAction;

namespace {

struct ArenaCount {  // the batcher's pinned arenas: allocations made (growth included) and bytes held
    uint64_t allocs = 0, bytes = 0;
};

struct Pinned {  // hipHostMalloc'd, mapped into the device address space; grows keeping its bytes
    uint8_t* h = nullptr;
    uint8_t* d = nullptr;
    size_t cap = 0;
    ArenaCount* cnt = nullptr;
    bool ensure(size_t n, size_t keep) {
        if (n <= cap) return true;
        size_t c = cap ? cap : (1u << 20);
        while (c < n) c *= 2;
        uint8_t *nh = nullptr, *nd = nullptr;
        // coarse-grained (host-cached) pinned memory: the GPU's writes are visible once the batch's
        // event completes, and host reads of the results run at cache speed
        if (hipHostMalloc((void**)&nh, c, hipHostMallocMapped | hipHostMallocNonCoherent) != hipSuccess) return false;
        if (hipHostGetDevicePointer((void**)&nd, nh, 0) != hipSuccess) {
            (void)hipHostFree(nh);
            return false;
        }
        if (h && keep) memcpy(nh, h, keep < cap ? keep : cap);
        if (h) (void)hipHostFree(h);
        if (cnt) {
            cnt->allocs += 1;
            cnt->bytes += c - cap;
        }
        h = nh;
        d = nd;
        cap = c;
        return true;
    }
    ~Pinned() {
        if (h) (void)hipHostFree(h);
        if (cnt) cnt->bytes -= cap;
    }
};

inline uint64_t align16(uint64_t x) { return (x + 15) & ~15ull; }

enum class JobKind { SnappyEnc, SnappyDec, AltEnc, AltDec, ZlibEnc, ZlibDec };
enum class Codec { FastLz, Lzf, Lz4 };  // of an alt-codec job

struct Batch;
struct Job {
    uint64_t ticket = 0;
    JobKind kind = JobKind::SnappyEnc;
    nx_snappy_frame_decoder* dec = nullptr;  // Snappy decoder jobs hold a reference (handles.hpp)
    uint32_t index = 0;  // EncJob / DecJob index in its batch
    std::vector<SnappyAction> acts;  // decode: the parsed actions (host copy, stream order)
    std::string parse_err;           // decode: the header-level error after them, if any
    bool has_parse_err = false;
    bool applied = false;
    int32_t status = NX_OK;
    std::vector<nx_msg> msgs;
    std::string err;
    // decode, validating decoders: the walked bytes start at stream position s_base (acts[].data is
    // relative to it), under the decoder's re-walk epoch; `walked` = s_base is in dec->outstanding
    uint64_t s_base = 0, epoch = 0;
    bool walked = false;
    std::vector<std::vector<uint8_t>> owned;  // messages delivered before a re-walk moved the job (a moved
                                              // vector keeps its buffer; a deque would allocate per Job)
    // alt-codec jobs (FastLZ / LZF / LZ4)
    Codec codec = Codec::FastLz;
    nx_alt_decoder_base* adec = nullptr;  // decoder jobs hold a reference (alt_frames.hpp)
    bool validate = false;
    std::vector<nx::af::Blk> ablk;      // decoder: the walked blocks, in order
    nx::af::WalkErr awerr;              // decoder: the walk's header failure after them
    uint64_t astage = 0;                // decoder: staging offset of the walked bytes (block data are relative)
    // JdkZlibEncoder jobs (pieces like an alt encoder's): the handle, and for a close the trailer's
    // length and the total-in it states
    nx_zlib_encoder* zenc = nullptr;
    uint32_t ztrailer = 0;
    uint64_t ztotal_in = 0;
    // JdkZlibDecoder jobs: the handle; the ticket's call state (its cumulation is the handle's pending
    // buffer); a held job's own bytes until it starts; the batch that owns the job
    nx_zlib_decoder* zdec = nullptr;
    nx::zl::Call zcall;
    std::vector<uint8_t> zin;
    bool zheld = false;
    Batch* zq = nullptr;    // the batch its current body step is queued in
    Batch* home = nullptr;
    Job() = default;
    Job(const Job&) = delete;
    Job& operator=(const Job&) = delete;
    // A decoder job takes its reference as it learns its handle (the submitting caller's own reference
    // keeps the handle alive meanwhile) and drops it with the job, queued or not.
    void bind(nx_snappy_frame_decoder* d) {
        dec = d;
        d->refs.fetch_add(1);
    }
    void bind(nx_alt_decoder_base* d) {
        adec = d;
        d->refs.fetch_add(1);
    }
    void bind(nx_zlib_encoder* e) {
        zenc = e;
        e->refs.fetch_add(1);
    }
    void bind(nx_zlib_decoder* d) {
        zdec = d;
        d->refs.fetch_add(1);
    }
    ~Job() {
        nx_decoder_unref(dec);
        nx_alt_decoder_unref(adec);
        nx_zlib_encoder_unref(zenc);
        nx_zlib_decoder_unref(zdec);
    }
};
using JobPtr = std::unique_ptr<Job>;  // a job not yet handed to its batch (register_job)

struct AltEntry {  // one block for a codec kernel; the flush lays each list out as the kernel's arrays
    uint64_t off, slot;
    uint32_t len, aux;  // aux: FastLZ encode level / decode in_avail; LZ4 encode level | highCompressor << 8; decode olen
    int32_t lim;        // FastLZ encode: readU16 limit; decode: originalLength
};
enum AltIx { FLZ_E, LZF_E, LZ4_E, FLZ_D, LZF_D, LZ4_D, DFL_S, DFL_M, kAltLists };  // encode / decode x codec, in Codec's order;
                                                                                   // deflate slices: stored-only (level 0), matcher

struct Batch {
    Pinned staging;  // chunk payloads, then the device arrays (one H2D copy at flush)
    size_t st_used = 0;
    struct Direct {
        const uint8_t* src;  // host address (adjacency test)
        const uint8_t* dsrc; // its device address (mapped registration)
        size_t len;
        uint64_t din_off;
    };
    std::vector<Direct> direct;  // registered inputs / cumulations, gathered at flush (din_off in the direct region)
    uint64_t direct_used = 0;
    std::vector<EncSlice> esl;
    std::vector<uint8_t> esl_direct;  // slice input lies in the direct region
    std::vector<EncJob> ejob;
    uint64_t eslots = 0;
    std::vector<DecAct> dact;
    std::vector<uint8_t> dact_direct;  // payload lies in the direct region (registered cumulation)
    std::vector<DecJob> djob;
    uint32_t ndc = 0, ndu = 0;  // compressed / uncompressed chunks among dact (DecAct::chunk counts them);
                                // their launch lists are derived from dact at flush
    bool dc_validate = false;   // some compressed chunk's decoder validates: the decode launch verifies CRCs
    // alt-codec jobs: their pieces and the launch lists of the codec kernels (inputs all staged)
    std::vector<nx::bt::AltPiece> apc;
    std::vector<nx::bt::AltJobD> ajob;
    uint64_t aslots = 0;  // alt slot bytes
    std::vector<AltEntry> alt[kAltLists];
    // JdkZlibDecoder jobs: one stream per job (its body step), the window region's bytes, the streams'
    // places in the launch order (set at flush: by checksum), the held jobs it owns
    struct ZStream {
        nx::zj::DecStream d;
        uint64_t in_off;
        uint32_t in_len;
        uint32_t ck;  // CK_CRC32 / CK_ADLER32 / CK_NONE
    };
    std::vector<ZStream> zst;
    std::vector<uint32_t> zpos;
    uint64_t zwin = 0, res_z = 0;
    uint32_t zheld_n = 0;
    Pinned out;  // mapped result arena: job outputs, then the result records
    uint64_t out_used = 0, res_enc = 0, res_dec = 0, res_alt = 0;
    // Bytes the finish kernels are known to write into `out`: decoded messages (lengths from the
    // chunks' preambles).  Encoder outputs are not counted (they fill ~half of their bound-sized
    // reservation).  When the known bytes fill most of a large arena the finish kernels write a device
    // mirror instead and one DMA copy moves it (place()).
    uint64_t est_out = 0;
    uint64_t res_spill = 0;  // the flush's spill area (decoded messages longer than their preamble said)
    std::vector<uint64_t> dslot_off;  // decode slot of each compressed chunk (device, from slots + eslots): set at
                                      // flush, kept for apply()'s spills beyond the spill area
    std::vector<Job*> jobs;
    nx::h::DevBuf din, slots;
    Pinned gops;  // k_gather_host's op list, read by the kernel from pinned memory
    hipEvent_t ev = nullptr;
    uint64_t seq = 0;  // flush order
    bool inflight = false, done = false;
    size_t live = 0;  // jobs not yet released
    void reset() {
        st_used = 0;
        direct.clear();
        direct_used = 0;
        esl.clear();
        esl_direct.clear();
        ejob.clear();
        eslots = 0;
        dact.clear();
        dact_direct.clear();
        djob.clear();
        ndc = ndu = 0;
        dc_validate = false;
        out_used = res_enc = res_dec = res_alt = res_spill = 0;
        est_out = 0;
        dslot_off.clear();
        apc.clear();
        ajob.clear();
        aslots = 0;
        for (std::vector<AltEntry>& L : alt) L.clear();
        zst.clear();
        zpos.clear();
        zwin = res_z = 0;
        for (Job* j : jobs) delete j;
        jobs.clear();
        inflight = done = false;
        live = 0;
    }
    uint8_t* stage(size_t n, uint64_t* din_off) {  // reserve n staging bytes (16-aligned)
        const size_t at = (st_used + 15) & ~(size_t)15;
        if (!staging.ensure(at + n + 16, st_used)) return nullptr;
        st_used = at + n;
        *din_off = at;
        return staging.h + at;
    }
    bool reserve_out(size_t n, uint64_t* off) {
        const uint64_t at = (out_used + 15) & ~15ull;
        if (!out.ensure(at + n + 16, out_used)) return false;
        out_used = at + n;
        *off = at;
        return true;
    }
    ~Batch() {
        for (Job* j : jobs) delete j;
        if (ev) (void)hipEventDestroy(ev);
    }
};

}  // namespace

namespace {
// nx_host_register'd ranges: host base -> (length, device address of the mapping)
std::mutex g_reg_mu;
std::map<uintptr_t, std::pair<size_t, uint8_t*>> g_reg;
const uint8_t* registered_device_ptr(const uint8_t* p, size_t n) {
    std::lock_guard<std::mutex> lk(g_reg_mu);
    auto it = g_reg.upper_bound((uintptr_t)p);
    if (it == g_reg.begin()) return nullptr;
    --it;
    const uintptr_t off = (uintptr_t)p - it->first;
    if (off + n > it->second.first) return nullptr;
    return it->second.second + off;
}
}  // namespace

#ifndef NX_BATCHER_STREAMS
#define NX_BATCHER_STREAMS 4
#endif
constexpr int kStreams = NX_BATCHER_STREAMS;
struct nx_batcher {
    std::mutex mu;
    hipStream_t s[kStreams] = {};
    // DMA result path: one device mirror per stream (flushes on one stream are ordered, so the next
    // flush on it reuses the mirror after the previous result copy), not one per batch object
    nx::h::DevBuf dmirror[kStreams];
    int dev = 0;
    uint32_t held = 0;  // bit per nx::WsKind whose shared workspace the batcher holds (workspace.hpp)
    std::deque<Batch*> all;  // every batch object (collecting, in flight, or done)
    Batch* cur = nullptr;    // the collecting batch
    std::unordered_map<uint64_t, std::pair<Batch*, Job*>> tickets;
    uint64_t next_ticket = 1;
    uint64_t launches = 0, chunks = 0, flushes = 0;
    uint64_t dma_flushes = 0, dma_bytes = 0;
    uint64_t applied = 0;     // batches applied, in flush order (Batch::seq < applied)
    size_t flush_bytes = 0;   // auto-flush threshold on a batch's input bytes (0 = only explicit flushes)
    ArenaCount arena;         // pinned staging / result arenas of all batches
    std::vector<std::pair<Job*, Batch*>> cont;  // re-walked jobs / zlib decoder jobs with a further body step to queue
                                                // again (found by apply())
    // JdkZlibDecoder handles with unapplied jobs: the one whose steps run (active), and the jobs submitted
    // behind it (held, in submit order; each stays in the batch that collected it until it starts)
    struct ZChan {
        Job* active = nullptr;
        std::deque<Job*> held;
    };
    std::unordered_map<nx_zlib_decoder*, ZChan> zchan;
    bool kick = false;        // the collecting batch holds a re-walked job: launch it at the next poll/wait
};

namespace {

bool advance(nx_batcher* b, uint64_t upto, bool block);

Batch* new_batch(nx_batcher* b) {  // a batch object with its event, its pinned arenas counted in b->arena
    Batch* x = new Batch();
    if (hipEventCreateWithFlags(&x->ev, hipEventDisableTiming) != hipSuccess) {
        delete x;
        return nullptr;
    }
    x->staging.cnt = x->out.cnt = x->gops.cnt = &b->arena;
    b->all.push_back(x);
    return x;
}

Batch* reuse_or_new_batch(nx_batcher* b) {
    for (Batch* x : b->all) {
        if (!x->inflight && x->live == 0 && x->zheld_n == 0 && x != b->cur) {
            x->reset();
            return x;
        }
    }
    return new_batch(b);
}

Batch* collecting(nx_batcher* b) {
    if (!b->cur) {
        advance(b, ~0ull, false);  // apply every completed batch (in flush order), even if its jobs were released unpolled
        Batch* x = reuse_or_new_batch(b);
        if (!b->cur) b->cur = x;  // advance() may have opened one for re-walked jobs
    }
    return b->cur;
}

// Drop the stream segments no unapplied job of a validating decoder can re-walk any more.
void trim_hist(nx_snappy_frame_decoder* d) {
    if (d->corrupted) {  // (:86-89): nothing is parsed again
        d->hist.clear(d->parse_pos);
        return;
    }
    d->hist.drop_before(d->outstanding.empty() ? d->parse_pos : *d->outstanding.begin());
}

void unwalk(Job* j) {  // the job no longer needs its walked bytes kept
    if (!j->walked) return;
    nx_snappy_frame_decoder* d = j->dec;
    auto it = d->outstanding.find(j->s_base);
    if (it != d->outstanding.end()) d->outstanding.erase(it);
    j->walked = false;
}

// Queue decoder job j's walked actions into batch bt.  Payloads are copied from S (host bytes the
// walk ran over), or, with dS (the device address of S in registered memory), gathered from there at
// flush.  The caller adds j to the batch's jobs.  On failure the batch's arrays go back to their sizes at
// entry (its other jobs stay valid).
// Snappy.decode's preamble (readPreamble, Snappy.java:404-420): the declared length, for sizing
// estimates only (65 536, the frame decoder's cap, when it is malformed or absent)
inline uint32_t snappy_declared_len(const uint8_t* p, size_t n) {
    uint32_t v = 0;
    for (size_t i = 0; i < n && i < 4; ++i) {
        v |= (uint32_t)(p[i] & 0x7f) << (7 * i);
        if ((p[i] & 0x80) == 0) return v < 65536u ? v : 65536u;
    }
    return 65536u;
}

int32_t enqueue_dec(Batch* bt, Job* j, const uint8_t* S, size_t walked, const uint8_t* dS, int64_t staged = -1) {
    const size_t n_act = bt->dact.size(), n_dir = bt->direct.size();
    const uint32_t n_dc = bt->ndc, n_du = bt->ndu;
    const uint64_t dir_used = bt->direct_used, est0 = bt->est_out;
    auto fail = [&](int32_t code) -> int32_t {
        bt->est_out = est0;
        bt->dact.resize(n_act);
        bt->dact_direct.resize(n_act);
        bt->ndc = n_dc;
        bt->ndu = n_du;
        bt->direct.resize(n_dir);
        bt->direct_used = dir_used;
        return code;
    };
    uint64_t rbase = 0;
    if (dS && walked) {
        rbase = (bt->direct_used + 15) & ~15ull;
        bt->direct.push_back({S, dS, walked, rbase});
        bt->direct_used = rbase + walked;
    }
    DecJob J{};
    J.a0 = (uint32_t)bt->dact.size();
    J.validate = j->dec->validate ? 1u : 0u;
    size_t out_need = 0;
    for (const SnappyAction& a : j->acts) {
        if (a.kind != SAct::Uncomp && a.kind != SAct::Comp) continue;
        uint64_t off = 0;
        if (dS) {
            off = rbase + a.data;
        } else if (staged >= 0) {  // the walked bytes are already in the staging arena at `staged`
            off = (uint64_t)staged + a.data;
        } else {
            uint8_t* st = bt->stage(a.dlen, &off);
            if (!st) return fail(NX_ERR_HIP);
            nx::copy_bytes(st, S + a.data, a.dlen);
        }
        bt->dact_direct.push_back(dS ? 1 : 0);
        DecAct A{off, a.dlen, 0, 0, a.crc, a.dlen, 0};
        if (a.kind == SAct::Comp) {
            A.kind = 2;
            A.chunk = bt->ndc++;
            if (j->dec->validate) bt->dc_validate = true;
            // the message's room: the preamble's length (never more than the bound); a chunk that
            // decodes longer (malformed, yet Java keeps it) spills (k_dec_finish, apply)
            A.cap = std::min<uint32_t>(snappy_declared_len(S + a.data, a.dlen), nx::bt::snappy_decoded_bound(a.dlen));
            out_need += A.cap;
            bt->est_out += A.cap;
        } else {
            A.kind = 1;
            A.chunk = bt->ndu++;
            out_need += a.dlen;
            bt->est_out += a.dlen;
        }
        bt->dact.push_back(A);
    }
    J.na = (uint32_t)bt->dact.size() - J.a0;
    if (!bt->reserve_out(out_need + 16, &J.out_off)) return fail(NX_ERR_HIP);
    j->index = (uint32_t)bt->djob.size();
    bt->djob.push_back(J);
    return NX_OK;
}

// The header walk of SnappyFrameDecoder.decode over S[0..n) from the decoder's state (:85-231); a
// header-level error ends it and is kept on the job, applied in order (the decoder turns corrupted then).
size_t walk(nx_snappy_frame_decoder* d, Job* j, const uint8_t* S, size_t n, bool& started, uint64_t& skip) {
    size_t p = 0;
    j->acts.clear();
    j->has_parse_err = false;
    j->parse_err.clear();
    while (p < n && nx::fr::snappy_parse_one(S, n, p, started, skip, d->validate, j->acts)) {
    }
    if (!j->acts.empty() && j->acts.back().kind == SAct::Error) {
        j->has_parse_err = true;
        j->parse_err = j->acts.back().err;
        p = j->acts.back().end;
        j->acts.pop_back();
    }
    return p;
}

bool has_gpu_work(const Job* j) {
    for (const SnappyAction& a : j->acts)
        if (a.kind == SAct::Uncomp || a.kind == SAct::Comp) return true;
    return false;
}

// Job j's compressed chunk decoded fewer bytes than its length, in validating mode: Java leaves the
// rest in the cumulation and parses it as the next chunk header (SnappyFrameDecoder.java:206-212).
// Walk the decoder's stream again from q (the first unread byte): every byte handed over so far, so
// the walks of the decoder's later, not yet applied jobs are void (new epoch; they deliver nothing and
// their bytes are covered here).  Returns true when j has GPU work again: it is queued into the
// collecting batch by queue_continuations() and completes there.
bool rewalk(nx_batcher* b, Batch* bt, Job* j, uint64_t q) {
    nx_snappy_frame_decoder* d = j->dec;
    d->epoch += 1;
    d->parse_failed = false;
    bool started = true;  // a compressed chunk was accepted (:180-183)
    uint64_t skip = 0;
    const uint8_t* S = d->hist.own_from(q);
    const size_t n = (size_t)(d->hist.end - q);
    const size_t p = walk(d, j, S, n, started, skip);
    d->started = started;
    d->skip = skip;
    d->parse_pos = q + p;
    if (j->has_parse_err) d->parse_failed = true;
    j->s_base = q;
    j->epoch = d->epoch;
    if (!has_gpu_work(j)) {
        if (j->has_parse_err) {
            j->status = NX_ERR_FRAME_CORRUPT;
            j->err = j->parse_err;
            d->corrupted = true;  // (:227-230)
        }
        return false;
    }
    // the messages so far live in bt's arena, which may be reused before j completes elsewhere
    for (nx_msg& m : j->msgs) {
        j->owned.emplace_back(m.data, m.data + m.len);
        m.data = j->owned.back().data();
    }
    d->outstanding.insert(q);
    j->walked = true;
    j->applied = false;
    b->cont.push_back({j, bt});
    return true;
}

// ---------------------------------------------------------------- one flush
// The arrays of a flush.  Each is reserved once, by element type and count, 16-byte aligned (struct
// Flush).  Its handle is an offset: the staging arena may move when the arrays' room is staged, and the
// kernels' arrays sit behind the slots.  Flush::operator() makes it a pointer once the bases are known.
template <class T>
struct In {  // filled by the host inside the staging arena, uploaded with it
    uint64_t off;
};
template <class T>
struct Dev {  // filled by the kernels: device only, after the alt slots in `slots`
    uint64_t off;
};

// Piece checksums run as up to six launches: Adler32 over decoded slots / over raw blocks' input bytes, XXH32
// over the same two, and for JdkZlibEncoder slices Adler32 / CRC32 over their input bytes.  The list of a
// piece that wants one, or -1:
constexpr int kCkLists = 6;
inline int ck_list(const nx::bt::AltPiece& q) {
    if (q.kind < nx::bt::AK_DEC_FLZ || !q.cks) return -1;
    if (q.kind == nx::bt::AK_DFL_ENC) return q.cks == nx::bt::CK_CRC32 ? 5 : 4;
    return (q.cks == nx::bt::CK_XXH32 ? 2 : 0) + (q.kind == nx::bt::AK_DEC_RAW ? 1 : 0);
}
inline bool ck_of_input(int c) { return c == 1 || c == 3 || c >= 4; }  // the list's bytes lie in the input arena
struct CkCount {
    uint32_t n[kCkLists] = {}, first[kCkLists] = {}, total = 0;  // first: the list's first result in AltArrays::dcks
    explicit CkCount(const std::vector<nx::bt::AltPiece>& apc) {
        for (const nx::bt::AltPiece& q : apc)
            if (const int c = ck_list(q); c >= 0) n[c] += 1;
        for (int c = 0; c < kCkLists; ++c) {
            first[c] = total;
            total += n[c];
        }
    }
};

// LZ4 frame encode takes one (level, compressor) per launch: the list is uploaded ordered by AltEntry::aux,
// submit order kept within each value.  Returns every entry's position in that order.
std::vector<uint32_t> order_by_aux(const std::vector<AltEntry>& L) {
    std::vector<uint32_t> perm(L.size()), pos(L.size());
    for (uint32_t i = 0; i < perm.size(); ++i) perm[i] = i;
    std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t c) { return L[a].aux < L[c].aux; });
    for (uint32_t k = 0; k < perm.size(); ++k) pos[perm[k]] = k;
    return pos;
}

// What the stages of one flush share.  Constructing it lays the flush out: every array is declared with
// its reservation, in the order of the declarations.
struct Flush {
    nx_batcher* const b;
    Batch* const bt;
    const hipStream_t s;
    uint8_t* H = nullptr;        // the uploaded arrays in the staging arena ...
    const uint8_t* A = nullptr;  // ... and in the device input arena
    uint8_t* din = nullptr;      // device input arena: [staging bytes][direct region, from d0]
    uint64_t d0 = 0;
    uint8_t *eslots = nullptr, *dslots = nullptr, *aslots = nullptr;  // Snappy encode / decode slots, alt slots
    uint8_t* D = nullptr;        // the kernels' arrays, after them
    uint8_t* ob = nullptr;       // where the finish kernels write: the mapped result arena, or its device mirror
    bool dma_out = false;        // ... the mirror, moved by one DMA copy
    template <class T>
    const T* operator()(In<T> a) const { return reinterpret_cast<const T*>(A + a.off); }
    template <class T>
    T* operator()(Dev<T> a) const { return reinterpret_cast<T*>(D + a.off); }
    template <class T>
    T* host(In<T> a) const { return reinterpret_cast<T*>(H + a.off); }

    uint64_t up_used = 0, up_off = 0, kern_used = 0;  // the host-filled arrays' room (uploaded from up_off in
                                                      // the staging arena), the kernel-filled arrays' room
    static uint64_t take(uint64_t& used, uint64_t bytes) {
        const uint64_t at = align16(used);
        used = at + bytes;
        return at;
    }
    struct Copy {
        uint64_t off;
        const void* src;
        size_t bytes;
    };
    std::vector<Copy> copies;  // carried out by fill_upload(), once the room is staged
    template <class T>
    In<T> room(size_t n) { return {take(up_used, sizeof(T) * n)}; }  // filled in place by fill_upload()
    template <class T>
    In<T> put(const std::vector<T>& v) {  // sent as it stands
        const In<T> a = room<T>(v.size());
        if (!v.empty()) copies.push_back({a.off, v.data(), sizeof(T) * v.size()});
        return a;
    }
    template <class T>
    Dev<T> out(size_t n) { return {take(kern_used, sizeof(T) * n)}; }

    // Snappy encoder: slices and jobs as submitted, the encode launch's lists (from the slices), the results
    const uint32_t nes = (uint32_t)bt->esl.size(), nej = (uint32_t)bt->ejob.size();
    const In<EncSlice> esl = put(bt->esl);
    const In<EncJob> ejob = put(bt->ejob);
    const In<uint64_t> ein = room<uint64_t>(nes), eslot = room<uint64_t>(nes);
    const In<uint32_t> elen = room<uint32_t>(nes);
    const Dev<uint32_t> eclen = out<uint32_t>(nes), ecrc = out<uint32_t>(nes);
    const Dev<int32_t> est = out<int32_t>(nes);
    // Snappy decoder: chunks and jobs as submitted, the compressed (dc) and uncompressed (du) chunks'
    // launch lists (from the chunks), the results, the spill area's cursor
    const uint32_t nda = (uint32_t)bt->dact.size(), ndj = (uint32_t)bt->djob.size(), ndc = bt->ndc, ndu = bt->ndu;
    const In<DecAct> dact = put(bt->dact);
    const In<DecJob> djob = put(bt->djob);
    const In<uint64_t> dcoff = room<uint64_t>(ndc), dslot = room<uint64_t>(ndc), duoff = room<uint64_t>(ndu);
    const In<uint32_t> dclen = room<uint32_t>(ndc), dccrc = room<uint32_t>(ndc), dulen = room<uint32_t>(ndu);
    const Dev<uint32_t> dlen = out<uint32_t>(ndc), dcons = out<uint32_t>(ndc), dcrc = out<uint32_t>(ndc), ducrc = out<uint32_t>(ndu);
    const Dev<int32_t> dst = out<int32_t>(ndc);
    const Dev<uint32_t> spill_cur = out<uint32_t>(1);
    uint64_t dslot_bytes = 0;  // the decode slots (fill_upload)
    uint32_t spill_cap = 0;
    // FastLZ / LZF / LZ4: the codec lists, the decoder checksum lists, pieces and jobs, the codecs' results
    const uint32_t nap = (uint32_t)bt->apc.size(), naj = (uint32_t)bt->ajob.size();
    struct AltIn {
        In<uint64_t> off, slot;
        In<uint32_t> len, aux;
        In<int32_t> lim;
        uint32_t n;
    };
    AltIn alt_room(AltIx c) {
        const uint32_t n = (uint32_t)bt->alt[c].size();
        return {room<uint64_t>(n), room<uint64_t>(n), room<uint32_t>(n), room<uint32_t>(n), room<int32_t>(n), n};
    }
    const AltIn al[kAltLists] = {alt_room(FLZ_E), alt_room(LZF_E), alt_room(LZ4_E), alt_room(FLZ_D),
                                 alt_room(LZF_D), alt_room(LZ4_D), alt_room(DFL_S), alt_room(DFL_M)};
    const CkCount cks{bt->apc};
    const In<uint64_t> ck_off[kCkLists] = {room<uint64_t>(cks.n[0]), room<uint64_t>(cks.n[1]), room<uint64_t>(cks.n[2]),
                                           room<uint64_t>(cks.n[3]), room<uint64_t>(cks.n[4]), room<uint64_t>(cks.n[5])};
    const In<uint32_t> ck_len[kCkLists] = {room<uint32_t>(cks.n[0]), room<uint32_t>(cks.n[1]), room<uint32_t>(cks.n[2]),
                                           room<uint32_t>(cks.n[3]), room<uint32_t>(cks.n[4]), room<uint32_t>(cks.n[5])};
    const In<nx::bt::AltPiece> apc = put(bt->apc);
    const In<nx::bt::AltJobD> ajob = put(bt->ajob);
    const Dev<uint32_t> fclen = out<uint32_t>(al[FLZ_E].n), fadl = out<uint32_t>(al[FLZ_E].n);
    const Dev<int32_t> fst = out<int32_t>(al[FLZ_E].n);
    const Dev<uint32_t> lolen = out<uint32_t>(al[LZF_E].n), zolen = out<uint32_t>(al[LZ4_E].n);
    const Dev<int32_t> lst = out<int32_t>(al[LZF_E].n), zst = out<int32_t>(al[LZ4_E].n);
    const Dev<int32_t> dfr = out<int32_t>(al[FLZ_D].n), dlst = out<int32_t>(al[LZF_D].n), dzst = out<int32_t>(al[LZ4_D].n);
    const Dev<uint32_t> dcks = out<uint32_t>(cks.total);
    const Dev<uint32_t> dfolen = out<uint32_t>(al[DFL_S].n + al[DFL_M].n);  // the stored-only launch's results, then the matcher's
    const Dev<int32_t> dfst = out<int32_t>(al[DFL_S].n + al[DFL_M].n);
    // JdkZlibDecoder: the streams of the one inflate call, ordered by checksum (CRC32, Adler32, none); the
    // windows lie after the kernels' arrays (zwin)
    const uint32_t nz = (uint32_t)bt->zst.size();
    uint32_t nz_crc = 0, nz_adler = 0;
    const In<nx::zj::DecStream> zrec = room<nx::zj::DecStream>(nz);
    const In<uint64_t> zin = room<uint64_t>(nz), zout = room<uint64_t>(nz), zsumoff = room<uint64_t>(nz);
    const In<uint32_t> zilen = room<uint32_t>(nz), zhist = room<uint32_t>(nz), zcap = room<uint32_t>(nz);
    const Dev<uint8_t> zstate = out<uint8_t>((size_t)NX_INFLATE_STATE_BYTES * nz);
    const Dev<uint32_t> zdcons = out<uint32_t>(nz), zdolen = out<uint32_t>(nz), zdsum = out<uint32_t>(nz);
    const Dev<int32_t> zdstat = out<int32_t>(nz);
    uint8_t* zwin = nullptr;

    Flush(nx_batcher* b_, Batch* bt_) : b(b_), bt(bt_), s(b_->s[b_->flushes % kStreams]) {}
};

// Stage the arrays' room and fill it: the copies, then one pass over each record array that moves the
// records of registered inputs into the direct region (d0 is known only now) and derives the kernels'
// launch lists, written where they are uploaded from.
int32_t fill_upload(Flush& F) {
    Batch* bt = F.bt;
    F.H = bt->stage(F.up_used + 16, &F.up_off);
    if (!F.H) return NX_ERR_HIP;
    for (const Flush::Copy& c : F.copies) memcpy(F.H + c.off, c.src, c.bytes);
    F.d0 = align16(bt->st_used);
    EncSlice* esl = F.host(F.esl);
    for (uint32_t i = 0; i < F.nes; ++i) {
        if (bt->esl_direct[i]) esl[i].in_off += F.d0;
        F.host(F.ein)[i] = esl[i].in_off;
        F.host(F.eslot)[i] = esl[i].slot_off;
        F.host(F.elen)[i] = esl[i].len;
    }
    DecAct* dact = F.host(F.dact);
    bt->dslot_off.resize(F.ndc);
    for (uint32_t i = 0; i < F.nda; ++i) {
        DecAct& a = dact[i];
        if (bt->dact_direct[i]) a.in_off += F.d0;
        if (a.kind == 2) {
            F.host(F.dcoff)[a.chunk] = a.in_off;
            F.host(F.dclen)[a.chunk] = a.len;
            F.host(F.dccrc)[a.chunk] = a.crc;
            F.host(F.dslot)[a.chunk] = bt->dslot_off[a.chunk] = F.dslot_bytes;
            F.dslot_bytes += nx::bt::dec_slot_bytes(a.len);
        } else {
            F.host(F.duoff)[a.chunk] = a.in_off;
            F.host(F.dulen)[a.chunk] = a.len;
        }
    }
    const std::vector<uint32_t> lz4_pos = order_by_aux(bt->alt[LZ4_E]);
    for (int c = 0; c < kAltLists; ++c) {
        const Flush::AltIn& L = F.al[c];
        for (uint32_t i = 0; i < L.n; ++i) {
            const AltEntry& e = bt->alt[c][i];
            const uint32_t k = c == LZ4_E ? lz4_pos[i] : i;
            F.host(L.off)[k] = e.off;
            F.host(L.slot)[k] = e.slot;
            F.host(L.len)[k] = e.len;
            F.host(L.aux)[k] = e.aux;
            F.host(L.lim)[k] = e.lim;
        }
    }
    // the uploaded pieces: an LZ4 block's results are at its place in the launch order; a decoder piece with
    // a checksum joins its list and learns its result's index (aux, 1-based)
    nx::bt::AltPiece* apc = F.host(F.apc);
    uint32_t nck[kCkLists] = {};
    for (uint32_t p = 0; p < F.nap; ++p) {
        nx::bt::AltPiece& q = apc[p];
        if (q.kind == nx::bt::AK_LZ4_ENC) q.res = lz4_pos[q.res];
        if (q.kind == nx::bt::AK_DFL_ENC && q.olen) q.res += F.al[DFL_S].n;  // olen: the slice is on the matcher list
        const int c = ck_list(q);
        if (c < 0) continue;
        const bool raw = ck_of_input(c);
        const uint32_t i = nck[c]++;
        F.host(F.ck_off[c])[i] = raw ? q.src : q.slot;
        F.host(F.ck_len[c])[i] = raw ? q.len : q.olen;
        q.aux = F.cks.first[c] + i + 1;
    }
    // the inflate call's streams: CRC32 streams first, then Adler32, then those without a checksum
    bt->zpos.resize(F.nz);
    for (const Batch::ZStream& z : bt->zst) {
        F.nz_crc += z.ck == nx::bt::CK_CRC32;
        F.nz_adler += z.ck == nx::bt::CK_ADLER32;
    }
    uint32_t at[3] = {0, F.nz_crc, F.nz_crc + F.nz_adler};
    for (uint32_t i = 0; i < F.nz; ++i) {
        const Batch::ZStream& z = bt->zst[i];
        const uint32_t k = at[z.ck == nx::bt::CK_CRC32 ? 0 : z.ck == nx::bt::CK_ADLER32 ? 1 : 2]++;
        bt->zpos[i] = k;
        F.host(F.zrec)[k] = z.d;
        F.host(F.zin)[k] = z.in_off;
        F.host(F.zilen)[k] = z.in_len;
        F.host(F.zout)[k] = z.d.win + nx::zj::kHist - z.d.hist;  // the window's history starts here
        F.host(F.zsumoff)[k] = z.d.win + nx::zj::kHist;
        F.host(F.zhist)[k] = z.d.hist;
        F.host(F.zcap)[k] = z.d.out_cap;
    }
    return NX_OK;
}

// Result records and spill area (in the mapped arena, after the job outputs), the result path, the device
// arenas and their bases.
int32_t place(Flush& F) {
    nx_batcher* b = F.b;
    Batch* bt = F.bt;
    if (F.naj && !bt->reserve_out(sizeof(nx::bt::AltRes) * F.nap + 8, &bt->res_alt)) return NX_ERR_HIP;
    if (F.nz && !bt->reserve_out(sizeof(nx::zj::DecRes) * F.nz + 8, &bt->res_z)) return NX_ERR_HIP;
    if (!bt->reserve_out(8ull * F.nej + 8, &bt->res_enc) || !bt->reserve_out(sizeof(DecRes) * F.nda + 8, &bt->res_dec)) return NX_ERR_HIP;
    // spill area: a chunk that decodes longer than its preamble said (Java grows its buffer up to
    // 65 536, SnappyFrameDecoder.java:203) has no room in its message reservation; k_dec_finish moves
    // it here, so apply() need not copy it from the device (only spills beyond this area do)
    F.spill_cap = (uint32_t)std::min<uint64_t>(nx::bt::kSpillBytes, 65536ull * F.ndc);
    if (F.ndc && !bt->reserve_out(F.spill_cap, &bt->res_spill)) return NX_ERR_HIP;
    // Where the finish kernels write: straight into the mapped arena (their stores cross PCIe), or,
    // when the expected bytes fill most of a large arena (decoded messages: lengths known from the
    // preambles), into a device mirror that one DMA copy then moves.  The copy engine does not hold
    // CUs or flood the memory system with partial writes while the next batch parses (round 4 e2e:
    // the finish kernel's host writes ran at 53 GB/s and slowed a concurrent k_parse 2-3x).
    // The spill area is reserved for rare malformed chunks: it counts neither as expected bytes nor
    // against them (counted in out_used it leaned mid-sized flushes away from the DMA path).
    const uint64_t est = bt->est_out + 8ull * F.nej + sizeof(DecRes) * F.nda + sizeof(nx::bt::AltRes) * (F.naj ? F.nap : 0);
    const uint64_t used_wo_spill = bt->out_used > F.spill_cap ? bt->out_used - F.spill_cap : 0;
    F.dma_out = bt->out_used >= nx::bt::kDmaOutMin && est * 5 >= used_wo_spill * 4;
    nx::h::DevBuf& mirror = b->dmirror[b->flushes % kStreams];
    if (F.dma_out && !mirror.ensure(bt->out_used)) return NX_ERR_HIP;
    F.ob = F.dma_out ? mirror.as<uint8_t>() : bt->out.d;
    if (!bt->din.ensure(F.d0 + bt->direct_used + 16) || !bt->slots.ensure(bt->eslots + F.dslot_bytes + bt->aslots + F.kern_used + bt->zwin + 256))
        return NX_ERR_HIP;
    F.din = bt->din.as<uint8_t>();
    F.A = F.din + F.up_off;
    F.eslots = bt->slots.as<uint8_t>();
    F.dslots = F.eslots + bt->eslots;
    F.aslots = reinterpret_cast<uint8_t*>(align16((uintptr_t)(F.dslots + F.dslot_bytes)));
    F.D = reinterpret_cast<uint8_t*>(align16((uintptr_t)(F.aslots + bt->aslots)));
    F.zwin = reinterpret_cast<uint8_t*>(((uintptr_t)(F.D + F.kern_used) + 127) & ~(uintptr_t)127);
    return NX_OK;
}

// Host -> device.  Registered inputs (and a small staging arena) move in one gather launch that
// reads the mapped pages, its op list itself read from pinned memory: no copy-engine work.  The
// copy engines run the batches' result copies in order, and a descriptor copy queued behind the
// previous batch's 500 MB result copy held this batch's gather (and, for an op list in pageable
// memory, the submitting thread) until that copy ended (round 4 e2e trace).  A large staging
// arena (payloads copied at submit) still goes by one DMA copy.
// (round 5 measured the whole staging arena through the gather as well, profiles/r05/s10: no better)
int32_t transfer_in(const Flush& F) {
    Batch* bt = F.bt;
    const bool dma_in = bt->direct.empty() && bt->st_used > nx::bt::kGatherStageMax;
    if (dma_in) {
        NX_HIP_CHECK(hipMemcpyAsync(F.din, bt->staging.h, bt->st_used, hipMemcpyHostToDevice, F.s));
    } else if (bt->st_used || !bt->direct.empty()) {
        const uint64_t piece = nx::bt::kGatherPiece;
        const uint32_t nst = (uint32_t)((bt->st_used + piece - 1) / piece);
        const uint32_t ng = nst + (uint32_t)bt->direct.size();
        if (!bt->gops.ensure(sizeof(nx::bt::GatherOp) * ng, 0)) return NX_ERR_HIP;
        nx::bt::GatherOp* ops = reinterpret_cast<nx::bt::GatherOp*>(bt->gops.h);
        for (uint32_t k = 0; k < nst; ++k) {
            const uint64_t o = (uint64_t)k * piece;
            ops[k] = {bt->staging.d + o, o, std::min<uint64_t>(piece, bt->st_used - o)};
        }
        for (uint32_t k = 0; k < (uint32_t)bt->direct.size(); ++k)
            ops[nst + k] = {bt->direct[k].dsrc, F.d0 + bt->direct[k].din_off, bt->direct[k].len};
        hipLaunchKernelGGL(nx::bt::k_gather_host, nx::bt::pcie_grid(ng), dim3(256), 0, F.s,
                           reinterpret_cast<const nx::bt::GatherOp*>(bt->gops.d), ng, F.din);
        NX_HIP_CHECK(hipGetLastError());
        F.b->launches += 1;
    }
    return NX_OK;
}

// CRC32C + Snappy.encode of every encoder slice of every channel, then the framed outputs
int32_t run_snappy_encode(const Flush& F) {
    if (!F.nes) return NX_OK;
    int32_t r = nx_crc32c_masked_batch(F.din, F(F.ein), F(F.elen), F(F.ecrc), F.nes, F.s);
    if (r != NX_OK) return r;
    r = nx_snappy_encode_batch(F.din, F(F.ein), F(F.elen), F.eslots, F(F.eslot), F(F.eclen), F(F.est), F.nes, F.s);
    if (r != NX_OK) return r;
    hipLaunchKernelGGL(nx::bt::k_enc_finish, nx::bt::pcie_grid(F.nej), dim3(256), 0, F.s, F.din, F.eslots, F(F.esl), F(F.eclen),
                       F(F.est), F(F.ecrc), F(F.ejob), F.nej, F.ob, reinterpret_cast<int64_t*>(F.ob + F.bt->res_enc));
    NX_HIP_CHECK(hipGetLastError());
    F.b->launches += 3;
    F.b->chunks += F.nes;
    return NX_OK;
}

// Snappy.decode (+ fused CRC verify) of every compressed chunk, CRC32C of the uncompressed ones, then
// the jobs' messages
int32_t run_snappy_decode(const Flush& F) {
    if (!F.ndj) return NX_OK;
    int32_t r;
    if (F.ndc) {
        r = nx_snappy_decode_batch(F.din, F(F.dcoff), F(F.dclen), F.dslots, F(F.dslot), nullptr, F(F.dlen), F(F.dcons), F(F.dst),
                                   F.bt->dc_validate ? F(F.dccrc) : nullptr, F(F.dcrc), F.ndc, F.s);
        if (r != NX_OK) return r;
        F.b->launches += 1;
    }
    if (F.ndu) {
        r = nx_crc32c_masked_batch(F.din, F(F.duoff), F(F.dulen), F(F.ducrc), F.ndu, F.s);
        if (r != NX_OK) return r;
        F.b->launches += 1;
    }
    if (F.ndc) NX_HIP_CHECK(hipMemsetAsync(F(F.spill_cur), 0, 4, F.s));
    hipLaunchKernelGGL(nx::bt::k_dec_finish, nx::bt::pcie_grid(F.ndj), dim3(256), 0, F.s, F.din, F.dslots, F(F.dslot), F(F.dact),
                       F(F.djob), F.ndj, F(F.dlen), F(F.dcons), F(F.dst), F(F.dcrc), F(F.ducrc), F.ob,
                       reinterpret_cast<DecRes*>(F.ob + F.bt->res_dec), F.bt->res_spill, F.spill_cap, F(F.spill_cur));
    NX_HIP_CHECK(hipGetLastError());
    F.b->launches += 1;
    F.b->chunks += F.ndc + F.ndu;
    return NX_OK;
}

// FastLZ / LZF / LZ4: one launch per codec kernel for every job of every channel, the decoders'
// checksums, then the jobs' outputs
int32_t run_alt(const Flush& F) {
    if (!F.naj) return NX_OK;
    nx_batcher* b = F.b;
    const hipStream_t s = F.s;
    int32_t r;
    if (const auto& L = F.al[FLZ_E]; L.n) {  // FastLz.compress + the frame's Adler32 of every block (FastLzFrameEncoder.java:136-158)
        r = nx_fastlz_compress_batch(F.din, F(L.off), F(L.len), F.aslots, F(L.slot), F(F.fclen), reinterpret_cast<const int32_t*>(F(L.aux)),
                                     F(L.lim), F(F.fst), L.n, s);
        if (r != NX_OK) return r;
        r = nx_adler32_batch(F.din, F(L.off), F(L.len), F(F.fadl), L.n, s);
        if (r != NX_OK) return r;
        b->launches += 2;
    }
    if (const auto& L = F.al[LZF_E]; L.n) {
        r = nx_lzf_encode_batch(F.din, F(L.off), F(L.len), F.aslots, F(L.slot), F(F.lolen), F(F.lst), L.n, s);
        if (r != NX_OK) return r;
        b->launches += 1;
    }
    const auto& Z = F.al[LZ4_E];
    const uint32_t* zaux = F.host(Z.aux);  // in launch order (fill_upload)
    for (uint32_t a0 = 0; a0 < Z.n;) {  // aux = compressionLevel | highCompressor << 8: one launch per value (usually one)
        uint32_t a1 = a0;
        while (a1 < Z.n && zaux[a1] == zaux[a0]) ++a1;
        r = nx_lz4_frame_encode_batch_ex(F.din, F(Z.off) + a0, F(Z.len) + a0, F.aslots, F(Z.slot) + a0, F(F.zolen) + a0,
                                         (int32_t)(zaux[a0] & 0xFFu), (int32_t)(zaux[a0] >> 8), F(F.zst) + a0, a1 - a0, s);
        if (r != NX_OK) return r;
        b->launches += 1;
        a0 = a1;
    }
    if (const auto& L = F.al[FLZ_D]; L.n) {  // FastLz.decompress (aux = in_avail: the cumulation's readable bytes from the block on)
        r = nx_fastlz_decompress_batch(F.din, F(L.off), F(L.len), F(L.aux), F.aslots, F(L.slot), reinterpret_cast<const uint32_t*>(F(L.lim)),
                                       F(F.dfr), L.n, s);
        if (r != NX_OK) return r;
        b->launches += 1;
    }
    if (const auto& L = F.al[LZF_D]; L.n) {
        r = nx_lzf_decode_batch(F.din, F(L.off), F(L.len), F.aslots, F(L.slot), F(L.aux), F(F.dlst), L.n, s);
        if (r != NX_OK) return r;
        b->launches += 1;
    }
    if (const auto& L = F.al[LZ4_D]; L.n) {
        r = nx_lz4_decode_batch(F.din, F(L.off), F(L.len), F.aslots, F(L.slot), F(L.aux), F(F.dzst), L.n, s);
        if (r != NX_OK) return r;
        b->launches += 1;
    }
    // JdkZlibEncoder slices: nx_deflate_encode_batch takes one level per launch, so one launch for the
    // stored-only slices (level 0) and one for the matcher's (1..9 and -1 run the same matcher)
    for (int c = DFL_S; c <= DFL_M; ++c) {
        const auto& L = F.al[c];
        if (!L.n) continue;
        const uint32_t r0 = c == DFL_M ? F.al[DFL_S].n : 0u;
        // the matcher list carries each slice's prefix_len (aux: a dictionary handle's first slice); a list
        // without one launches the plain entry point's kernels
        bool prefixed = false;
        for (uint32_t i = 0; c == DFL_M && i < L.n && !prefixed; ++i) prefixed = F.host(L.aux)[i] != 0u;
        r = nx_deflate_encode_batch_ex(F.din, F(L.off), F(L.len), prefixed ? F(L.aux) : nullptr, F.aslots, F(L.slot),
                                       F(F.dfolen) + r0, F(F.dfst) + r0, L.n, c == DFL_S ? 0 : 6, s);
        if (r != NX_OK) return r;
        b->launches += 1;
    }
    uint32_t* dcks = F(F.dcks);
    for (int c = 0; c < kCkLists; ++c) {  // piece checksums (after the decodes: stream order)
        const uint32_t n = F.cks.n[c];
        if (!n) continue;
        const uint8_t* base = ck_of_input(c) ? F.din : F.aslots;
        r = c == 5 ? nx_crc32_batch(base, F(F.ck_off[c]), F(F.ck_len[c]), dcks + F.cks.first[c], n, s)
            : c < 2 || c == 4 ? nx_adler32_batch(base, F(F.ck_off[c]), F(F.ck_len[c]), dcks + F.cks.first[c], n, s)
                  : nx_xxhash32_batch(base, F(F.ck_off[c]), F(F.ck_len[c]), nx::af::kLz4Seed, dcks + F.cks.first[c], n, s);
        if (r != NX_OK) return r;
        b->launches += 1;
    }
    const nx::bt::AltArrays R{F(F.fclen), F(F.fst), F(F.fadl), F(F.lolen), F(F.lst), F(F.zolen), F(F.zst), F(F.dfr), F(F.dlst), F(F.dzst), dcks, F(F.dfolen), F(F.dfst)};
    hipLaunchKernelGGL(nx::bt::k_alt_finish, nx::bt::pcie_grid(F.naj), dim3(256), 0, s, F.din, F.aslots, F(F.apc), F(F.ajob), F.naj, R,
                       F.ob, reinterpret_cast<nx::bt::AltRes*>(F.ob + F.bt->res_alt));
    NX_HIP_CHECK(hipGetLastError());
    b->launches += 1;
    for (int c = 0; c < kAltLists; ++c) b->chunks += F.al[c].n;
    return NX_OK;
}

// JdkZlibDecoder jobs: every stream's history and state into the batch, ONE inflate call, the outputs'
// checksums (their lengths are the inflate's out_len array, on the device), then state, carry, output and
// result record of every stream back out.  Five launches at most, however many jobs.
int32_t run_zlib_decode(const Flush& F) {
    if (!F.nz) return NX_OK;
    const hipStream_t s = F.s;
    int32_t r = nx::zj::dec_begin(F(F.zrec), F.nz, F.zwin, F(F.zstate), s);
    if (r != NX_OK) return r;
    r = nx_inflate_batch(F.din, F(F.zin), F(F.zilen), F.zwin, F(F.zout), F(F.zhist), F(F.zcap), F(F.zstate), F(F.zdcons), F(F.zdolen),
                         F(F.zdstat), F.nz, s);
    if (r != NX_OK) return r;
    F.b->launches += 2;
    if (F.nz_crc) {
        r = nx_crc32_batch(F.zwin, F(F.zsumoff), F(F.zdolen), F(F.zdsum), F.nz_crc, s);
        if (r != NX_OK) return r;
        F.b->launches += 1;
    }
    if (F.nz_adler) {
        const uint32_t a = F.nz_crc;
        r = nx_adler32_batch(F.zwin, F(F.zsumoff) + a, F(F.zdolen) + a, F(F.zdsum) + a, F.nz_adler, s);
        if (r != NX_OK) return r;
        F.b->launches += 1;
    }
    r = nx::zj::dec_finish(F(F.zrec), F.nz, F.zwin, F(F.zstate), F(F.zdcons), F(F.zdolen), F(F.zdstat), F(F.zdsum), F.ob,
                           reinterpret_cast<nx::zj::DecRes*>(F.ob + F.bt->res_z), s);
    if (r != NX_OK) return r;
    F.b->launches += 1;
    F.b->chunks += F.nz;
    return NX_OK;
}

// Device -> host for a mirrored result arena, then the batch's event: it is in flight, next in flush order.
int32_t transfer_out(const Flush& F) {
    nx_batcher* b = F.b;
    Batch* bt = F.bt;
    if (F.dma_out) {
        NX_HIP_CHECK(hipMemcpyAsync(bt->out.h, F.ob, bt->out_used, hipMemcpyDeviceToHost, F.s));
        b->dma_flushes += 1;
        b->dma_bytes += bt->out_used;
    }
    NX_HIP_CHECK(hipEventRecord(bt->ev, F.s));
    bt->inflight = true;
    bt->seq = b->flushes;
    b->flushes += 1;
    return NX_OK;
}

// Launch everything `bt` collected (batcher lock held).
int32_t launch_inner(nx_batcher* b, Batch* bt) {
    NX_CLEAR_STALE_ERROR();
    const nx::NoGrowScope no_grow;  // the workspaces reserved at nx_batcher_new: a flush never allocates them
    Flush F(b, bt);
    int32_t r = fill_upload(F);
    if (r == NX_OK) r = place(F);
    if (r == NX_OK) r = transfer_in(F);
    if (r == NX_OK) r = run_snappy_encode(F);
    if (r == NX_OK) r = run_snappy_decode(F);
    if (r == NX_OK) r = run_alt(F);
    if (r == NX_OK) r = run_zlib_decode(F);
    if (r == NX_OK) r = transfer_out(F);
    return r;
}

void zdec_fail(nx_batcher* b, Job* j, int32_t code);

// Job j could not run on the GPU: it completes with the error, and its decoder turns corrupted.
void complete_launch_failed(Job* j, int32_t code) {
    j->applied = true;
    j->status = code;
    j->err = "GPU batch launch failed";
    if (j->kind == JobKind::SnappyDec && j->dec) {
        unwalk(j);
        j->dec->corrupted = true;
        trim_hist(j->dec);
    }
    if (j->kind == JobKind::AltDec && j->adec) j->adec->corrupted = true;
}

// A launch that failed part-way: wait for whatever of it reached the stream, then complete every job
// of the batch with the error (each decoder it touched turns corrupted, as after the reference's
// exception), so poll() reports them done and result() returns the error.  The batch is not in the
// flush order (it never got a sequence number) and is reused once its jobs are released.
int32_t fail_batch(nx_batcher* b, Batch* bt, int32_t code) {
    (void)hipStreamSynchronize(b->s[b->flushes % kStreams]);
    for (size_t k = 0; k < bt->jobs.size(); ++k) {
        Job* j = bt->jobs[k];
        if (j->kind == JobKind::ZlibDec) {  // only a job whose body step this launch held fails with it
            if (!j->applied && !j->zheld && j->zq == bt) zdec_fail(b, j, code);
            continue;
        }
        if (j->kind == JobKind::ZlibEnc && !j->applied) j->zenc->pending.fetch_sub(1);  // (its checksum is lost: the stream is broken)
        complete_launch_failed(j, code);
        j->msgs.clear();
    }
    bt->inflight = false;
    bt->done = true;
    return code;
}

int32_t launch(nx_batcher* b, Batch* bt) {
    const int32_t r = launch_inner(b, bt);
    return r == NX_OK ? NX_OK : fail_batch(b, bt, r);
}

// ---------------------------------------------------------------- JdkZlibEncoder / JdkZlibDecoder jobs
// A JdkZlibEncoder job's pieces are an alt encoder's (apply_alt's sum); here the handle's running
// checksum takes the slices' in flush order, and a close's trailer is written into the place its
// AK_CONST piece reserved (JdkZlibEncoder.java:326-337).
void apply_zlib_enc(Batch* bt, Job* j, const nx::bt::AltRes* ares) {
    using namespace nx::bt;
    j->applied = true;
    nx_zlib_encoder* e = j->zenc;
    e->pending.fetch_sub(1);
    const AltJobD& J = bt->ajob[j->index];
    uint64_t total = 0;
    for (uint32_t k = J.p0; k < J.p0 + J.np; ++k) {
        if (ares[k].status != NX_OK) {
            j->status = ares[k].status;
            j->err = nx_status_string(ares[k].status);
            return;
        }
        total += ares[k].len;
    }
    for (uint32_t k = J.p0; k < J.p0 + J.np; ++k) {
        const AltPiece& P = bt->apc[k];
        if (P.kind != AK_DFL_ENC) continue;
        if (e->wrapper == 1) e->crc = nx_crc32_combine(e->crc, ares[k].cks, P.len);
        else if (e->wrapper == 0) e->adler = nx_adler32_combine(e->adler, ares[k].cks, P.len);
    }
    if (j->ztrailer) {
        uint8_t* t = bt->out.h + J.out_off + total - j->ztrailer;
        if (e->wrapper == 0) {  // Adler32, most significant byte first
            for (int k = 0; k < 4; ++k) t[k] = (uint8_t)(e->adler >> (8 * (3 - k)));
        } else {  // writeIntLE(crc), writeIntLE(totalIn) (:331-335)
            for (int k = 0; k < 4; ++k) t[k] = (uint8_t)(e->crc >> (8 * k));
            for (int k = 0; k < 4; ++k) t[4 + k] = (uint8_t)((uint32_t)j->ztotal_in >> (8 * k));
        }
    }
    j->msgs.push_back({bt->out.h + J.out_off, (size_t)total});
}

// Output room of one body step, from the staged input: four times the input bytes (text deflates to about
// a third to a quarter), within [64 KiB, 1 MiB] (the synchronous handle's chunk).  A step that fills it
// stops with NX_INFLATE_OUTPUT_FULL and the job continues in the next flush.
uint32_t zlib_out_cap(size_t in_len) {
    const uint64_t want = 4ull * in_len;
    const uint64_t c = want < (64u << 10) ? (64u << 10) : want > (1u << 20) ? (1u << 20) : want;
    return (uint32_t)((c + 127) & ~127ull);
}

// Queue the body step job j needs as one stream of batch `to`: the unused bytes of the ticket's cumulation
// are staged, the window and the output reservation are laid out.
int32_t zdec_enqueue(Batch* to, Job* j) {
    nx_zlib_decoder* d = j->zdec;
    const nx::zl::Call& c = j->zcall;
    const size_t left = c.n - c.rd;
    const uint32_t in_len = (uint32_t)(left < 0x7FFFFFFFu ? left : 0x7FFFFFFFu);
    Batch::ZStream z{};
    z.d.out_cap = zlib_out_cap(in_len);
    uint8_t* st = to->stage(in_len, &z.in_off);
    if (!st || !to->reserve_out(z.d.out_cap, &z.d.out_off)) return NX_ERR_HIP;
    nx::copy_bytes(st, c.in + c.rd, in_len);
    z.in_len = in_len;
    z.d.state = d->st.as<uint8_t>();
    z.d.carry_in = d->win[d->cur].as<uint8_t>();
    z.d.carry_out = d->win[d->cur ^ 1].as<uint8_t>();
    z.d.win = to->zwin;
    to->zwin += nx::zj::kHist + z.d.out_cap;  // (a multiple of 128)
    z.d.hist = d->hist;
    z.d.fresh = d->st_fresh ? 1u : 0u;
    z.ck = d->gzip ? nx::bt::CK_CRC32 : d->zlib ? nx::bt::CK_ADLER32 : nx::bt::CK_NONE;
    j->index = (uint32_t)to->zst.size();
    j->zq = to;
    to->zst.push_back(z);
    return NX_OK;
}

// The ticket is complete: its used bytes leave the handle's pending buffer.
void zdec_complete(Job* j, int32_t status) {
    nx_zlib_decoder* d = j->zdec;
    nx::zl::Call& c = j->zcall;
    d->pend.erase(d->pend.begin(), d->pend.begin() + (ptrdiff_t)(c.rd < d->pend.size() ? c.rd : d->pend.size()));
    if (!c.acc.empty()) {  // maxAllocation > 0: the ticket's one message
        j->owned.push_back(std::move(c.acc));
        j->msgs.push_back({j->owned.back().data(), j->owned.back().size()});
    }
    j->status = status;
    j->err = c.err;
    j->applied = true;
    j->zq = nullptr;
}

// Job j starts (it is its decoder's only running job): its cumulation is the handle's pending buffer, with
// the bytes a held job kept.  Runs the wrapper states; true = it needs a body step, false = complete.
bool zdec_start(Job* j) {
    nx_zlib_decoder* d = j->zdec;
    d->pend.insert(d->pend.end(), j->zin.begin(), j->zin.end());
    std::vector<uint8_t>().swap(j->zin);
    nx::zl::Call& c = j->zcall;
    c.in = d->pend.data();
    c.n = d->pend.size();
    c.rd = 0;
    const int step = nx::zl::wrapper_step(d, c);
    if (step == nx::zl::kBody) return true;
    zdec_complete(j, step < 0 ? step : NX_OK);
    return false;
}

// Decoder d's running job is complete: the next held one starts.  One that needs the device becomes the
// running job and joins the collecting batch (queue_continuations); the others complete at once.
void zdec_next(nx_batcher* b, nx_zlib_decoder* d) {
    auto it = b->zchan.find(d);
    if (it == b->zchan.end()) return;
    nx_batcher::ZChan& ch = it->second;
    ch.active = nullptr;
    while (!ch.held.empty()) {
        Job* h = ch.held.front();
        ch.held.pop_front();
        h->zheld = false;
        h->home->zheld_n -= 1;
        if (zdec_start(h)) {
            ch.active = h;
            b->cont.push_back({h, h->home});
            return;
        }
    }
    b->zchan.erase(it);
}

// A body step could not run (a failed launch, no room to queue it): the ticket fails with the code, the
// decoder skips what follows (its held jobs deliver nothing).
void zdec_fail(nx_batcher* b, Job* j, int32_t code) {
    nx_zlib_decoder* d = j->zdec;
    d->failed = true;
    j->msgs.clear();
    j->zcall.acc.clear();
    j->zcall.rd = j->zcall.n;
    j->zcall.err = "GPU batch launch failed";
    zdec_complete(j, code);
    auto it = b->zchan.find(d);
    if (it == b->zchan.end()) return;
    for (Job* h : it->second.held) {
        h->zheld = false;
        h->home->zheld_n -= 1;
        (void)zdec_start(h);  // skips: the decoder has failed
    }
    b->zchan.erase(it);
}

// A decoder job's body step ran in batch bt: account for it (nx::zl::body_result), go on with the wrapper
// states, and either complete the ticket or ask for the next step (b->cont).
void apply_zlib_dec(nx_batcher* b, Batch* bt, Job* j, const nx::zj::DecRes* zres) {
    namespace zl = nx::zl;
    nx_zlib_decoder* d = j->zdec;
    zl::Call& c = j->zcall;
    const nx::zj::DecRes& R = zres[bt->zpos[j->index]];
    const Batch::ZStream& Z = bt->zst[j->index];
    struct JobIo : zl::BodyIo {  // the bytes are in the result arena; the carry was written by k_zlib_dec_finish
        Job* j;
        const uint8_t* src;
        bool take(uint8_t* dst, uint32_t m) override {
            if (dst) memcpy(dst, src, m);
            else j->msgs.push_back({src, (size_t)m});
            return true;
        }
        void drop() override {
            j->msgs.clear();
            j->owned.clear();
        }
        bool carry(uint32_t, uint32_t) override { return true; }
    } io;
    io.j = j;
    io.src = bt->out.h + Z.d.out_off;
    d->st_fresh = false;
    const uint32_t m = R.out_len < Z.d.out_cap ? R.out_len : Z.d.out_cap;
    int step = zl::body_result(d, c, R.consumed <= Z.in_len ? R.consumed : Z.in_len, m, R.status, R.sum, io);
    if (step == zl::kWrapper) step = zl::wrapper_step(d, c);
    if (step == zl::kBody) {  // NX_INFLATE_OUTPUT_FULL, or a further member: the same ticket, the next flush
        for (nx_msg& q : j->msgs) {  // bt's arena may be reused before the ticket completes
            if (q.data < bt->out.h || q.data >= bt->out.h + bt->out.cap) continue;
            j->owned.emplace_back(q.data, q.data + q.len);
            q.data = j->owned.back().data();
        }
        j->zq = nullptr;
        b->cont.push_back({j, bt});
        return;
    }
    zdec_complete(j, step <= zl::kHalt ? step - zl::kHalt : step < 0 ? step : NX_OK);
    zdec_next(b, d);
}

// An alt-codec job's result (its batch complete): an encoder's framed bytes as one message, or the
// decoder's messages in block order up to its first failure, with the reference's message
// (FastLzFrameDecoder.java:154-180, LzfDecoder.java:205, Lz4FrameDecoder.java:215-241); then the
// walk's header failure, if any.  A failure marks the decoder corrupted; jobs applied after that on
// the same decoder deliver nothing (Java skips all later input).
void apply_alt(Batch* bt, Job* j, const nx::bt::AltRes* ares) {
    using namespace nx::bt;
    j->applied = true;
    const AltJobD& J = bt->ajob[j->index];
    if (j->kind == JobKind::AltEnc) {
        uint64_t total = 0;
        for (uint32_t k = J.p0; k < J.p0 + J.np; ++k) {
            if (ares[k].status != NX_OK) {
                j->status = ares[k].status;
                j->err = nx_status_string(ares[k].status);
                return;
            }
            total += ares[k].len;
        }
        j->msgs.push_back({bt->out.h + J.out_off, (size_t)total});
        return;
    }
    nx_alt_decoder_base* d = j->adec;
    if (d->corrupted) return;
    auto fail = [&](int32_t code, const std::string& msg) {
        j->status = code;
        j->err = msg;
        d->corrupted = true;
    };
    for (uint32_t i = 0; i < J.np; ++i) {
        const AltRes& R = ares[J.p0 + i];
        const AltPiece& P = bt->apc[J.p0 + i];
        const nx::af::Blk& B = j->ablk[i];
        bool emit = true;
        switch (j->codec) {
            case Codec::FastLz:
                if (R.status != NX_OK) {
                    int32_t code;
                    std::string msg;
                    const int32_t v = R.status == NX_ERR_FASTLZ_LENGTH_MISMATCH ? (int32_t)R.len : R.status;
                    const uint8_t first = B.clen ? bt->staging.h[P.src] : 0;
                    (void)nx::af::flz_block_error(v, B.olen, first, &code, &msg);
                    return fail(code, msg);
                }
                if (B.has_cks && j->validate && R.cks != B.cks)
                    return fail(NX_ERR_FASTLZ_CRC_MISMATCH, nx::af::flz_checksum_error(R.cks, B.cks));
                emit = B.olen > 0;
                break;
            case Codec::Lzf:
                if (R.status != NX_OK) return fail(R.status, nx::af::lzf_block_error());
                emit = B.comp || B.clen > 0;
                break;
            case Codec::Lz4:
                if (R.status != NX_OK) return fail(R.status, nx::af::lz4_block_error());
                if (j->validate && (R.cks & 0x0FFFFFFFu) != B.cks)
                    return fail(NX_ERR_LZ4_CHECKSUM_MISMATCH, nx::af::lz4_checksum_error(R.cks & 0x0FFFFFFFu, B.cks));
                break;
        }
        if (emit) j->msgs.push_back({bt->out.h + R.off, (size_t)R.len});
    }
    if (j->awerr.set) fail(j->awerr.code, j->awerr.msg);
}

// The batch is complete: turn the result records into each job's messages, in submission order.
void apply(nx_batcher* b, Batch* bt) {
    const int64_t* res_len = reinterpret_cast<const int64_t*>(bt->out.h + bt->res_enc);
    const DecRes* dres = reinterpret_cast<const DecRes*>(bt->out.h + bt->res_dec);
    char buf[160];
    const nx::bt::AltRes* ares = reinterpret_cast<const nx::bt::AltRes*>(bt->out.h + bt->res_alt);
    const nx::zj::DecRes* zres = reinterpret_cast<const nx::zj::DecRes*>(bt->out.h + bt->res_z);
    for (size_t k = 0; k < bt->jobs.size(); ++k) {
        Job* j = bt->jobs[k];
        if (j->kind == JobKind::ZlibEnc) {
            apply_zlib_enc(bt, j, ares);
            continue;
        }
        if (j->kind == JobKind::ZlibDec) {  // (complete since its submit, held, or running elsewhere: not this batch's)
            if (!j->applied && !j->zheld && j->zq == bt) apply_zlib_dec(b, bt, j, zres);
            continue;
        }
        if (j->kind == JobKind::AltEnc || j->kind == JobKind::AltDec) {
            apply_alt(bt, j, ares);
            continue;
        }
        if (j->kind == JobKind::SnappyEnc) {
            const EncJob& E = bt->ejob[j->index];
            const int64_t r = res_len[j->index];
            if (r < 0) {  // a slice the encoder failed: the job fails (no framed bytes)
                j->status = (int32_t)r;
                j->err = nx_status_string((int32_t)r);
            } else {
                j->msgs.push_back({bt->out.h + E.out_off, (size_t)r});
            }
            j->applied = true;
            continue;
        }
        nx_snappy_frame_decoder* d = j->dec;
        j->applied = true;
        unwalk(j);
        // an earlier job of this decoder failed: Java skips later input (:86-89); or a re-walk after an
        // earlier job's leftover covered this job's bytes
        if (d->corrupted || (d->validate && j->epoch != d->epoch)) {
            trim_hist(d);
            continue;
        }
        const DecJob& J = bt->djob[j->index];
        uint32_t a = J.a0;
        bool failed = false, moved = false;
        for (const SnappyAction& act : j->acts) {
            if (act.kind != SAct::Uncomp && act.kind != SAct::Comp) {
                if (act.kind == SAct::Stream) d->started = true;
                continue;
            }
            const DecRes& R = dres[a];
            const DecAct& A = bt->dact[a];
            ++a;
            if (R.status != NX_OK) {
                j->status = R.status;
                if (R.status == NX_ERR_SNAPPY_CRC_MISMATCH) {
                    snprintf(buf, sizeof buf, "mismatching checksum: %x (expected: %x)", R.crc, A.crc);
                    j->err = buf;
                } else {
                    j->err = nx::fr::snappy_block_error(R.status, R.crc, nx_status_string);
                }
                failed = true;
                break;
            }
            if (R.off == nx::bt::kSpilled) {  // longer than its preamble said, beyond the spill area: from the decode slot (blocking)
                j->owned.emplace_back(R.len);
                const uint8_t* src = bt->slots.as<uint8_t>() + bt->eslots + bt->dslot_off[A.chunk];
                if (hipMemcpy(j->owned.back().data(), src, R.len, hipMemcpyDeviceToHost) != hipSuccess) {
                    j->status = NX_ERR_HIP;
                    j->err = nx_status_string(NX_ERR_HIP);
                    failed = true;
                    break;
                }
                j->msgs.push_back({j->owned.back().data(), (size_t)R.len});
            } else {
                j->msgs.push_back({bt->out.h + R.off, (size_t)R.len});
            }
            if (A.kind == 2 && J.validate && R.cons < A.len) {  // validating-mode leftover (:206-212)
                moved = rewalk(b, bt, j, j->s_base + act.data + R.cons);
                break;
            }
        }
        if (!failed && !moved && j->has_parse_err) {
            j->status = NX_ERR_FRAME_CORRUPT;
            j->err = j->parse_err;
            failed = true;
        }
        if (failed) d->corrupted = true;  // (:227-230)
        trim_hist(d);
    }
    bt->done = true;
}

// Queue the jobs apply() re-walked into the collecting batch (after every job already in it: those of
// the same decoder were walked before the re-walk and deliver nothing).  The next poll()/wait() launches it.
void queue_continuations(nx_batcher* b) {
    // take every moved job out of its batch first, and pin those batches (live) so that none is reset
    // for reuse below while a job listed here may still go back to it
    for (auto& [j, from] : b->cont) {
        for (size_t k = 0; k < from->jobs.size(); ++k)
            if (from->jobs[k] == j) {
                from->jobs.erase(from->jobs.begin() + (ptrdiff_t)k);
                break;
            }
        from->live += 1;
    }
    for (auto& [j, from] : b->cont) {
        Batch* to = b->cur ? b->cur : reuse_or_new_batch(b);
        auto it = b->tickets.find(j->ticket);
        const bool live = it != b->tickets.end();
        if (j->kind == JobKind::ZlibDec) {
            if (!to || zdec_enqueue(to, j) != NX_OK) {
                zdec_fail(b, j, NX_ERR_HIP);
                from->jobs.push_back(j);
                continue;
            }
        } else {
            nx_snappy_frame_decoder* d = j->dec;
            const uint8_t* S = d->hist.at(j->s_base);  // the owned segment rewalk() made, from s_base on
            if (!to || !S || enqueue_dec(to, j, S, 0, nullptr) != NX_OK) {
                // cannot queue it: the job fails as a launch failure would (result() reports it)
                complete_launch_failed(j, NX_ERR_HIP);
                from->jobs.push_back(j);  // stays owned by its batch
                continue;
            }
        }
        to->jobs.push_back(j);
        j->home = to;
        b->cur = to;
        if (live) {
            if (from->live) from->live -= 1;
            to->live += 1;
            it->second.first = to;
        }
        b->kick = true;
    }
    for (auto& [j, from] : b->cont) from->live -= 1;
    b->cont.clear();
}

// Launch a collecting batch that holds re-walked jobs (their tickets are already out).
void kick(nx_batcher* b) {
    if (!b->kick) return;
    b->kick = false;
    Batch* bt = b->cur;
    if (!bt || bt->jobs.empty()) return;
    b->cur = nullptr;
    (void)launch(b, bt);  // a failed launch completes the batch's jobs with the error
}

// Apply completed batches in flush order up to (and including) sequence number `upto`; false if one
// of them is not complete (non-blocking) or failed.
bool advance(nx_batcher* b, uint64_t upto, bool block) {
    while (b->applied <= upto && b->applied < b->flushes) {
        Batch* bt = nullptr;
        for (Batch* x : b->all)
            if (x->inflight && x->seq == b->applied) bt = x;
        if (!bt) return false;  // unreachable: every launched batch stays in flight until applied
        const hipError_t e = block ? hipEventSynchronize(bt->ev) : hipEventQuery(bt->ev);
        if (e == hipErrorNotReady) (void)hipGetLastError();  // not an error: keep it from the next launch check
        if (e != hipSuccess) return false;
        apply(b, bt);
        bt->inflight = false;
        b->applied += 1;
        if (!b->cont.empty()) queue_continuations(b);
    }
    return true;
}

bool poll_batch(nx_batcher* b, Batch* bt, bool block) {
    if (bt->done) return true;
    if (!bt->inflight) return false;
    return advance(b, bt->seq, block) && bt->done;
}

// The batch whose completion moves job j forward: its own, or, for a held JdkZlibDecoder job, the batch of
// its decoder's running job.
Batch* progress_batch(nx_batcher* b, const Job* j, Batch* own) {
    if (j->kind != JobKind::ZlibDec || !j->zheld) return own;
    auto it = b->zchan.find(j->zdec);
    return it != b->zchan.end() && it->second.active ? it->second.active->home : own;
}

// Hold the shared workspace of kind k for the batcher's flushes (they run in a NoGrowScope): the full
// reservation, or a smaller one when the device cannot spare it (a flush caps its grid to what is
// held).  Done by the first submit that needs the kind, or up front by nx_batcher_reserve.
bool ensure_held(nx_batcher* b, nx::WsKind k) {
    const uint32_t bit = 1u << (int)k;
    if (b->held & bit) return true;
    const uint32_t first = k == nx::WsKind::SnappyEnc ? nx::kBatcherEncHoldUnits
                         : k == nx::WsKind::DecRecords ? nx::kBatcherDecHoldUnits : nx::kBatcherHoldUnits;
    for (uint32_t u = first; u >= nx::kHandleHoldUnits; u /= 4) {
        if (nx::ws_hold(k, b->dev, u, b->s[0]) == NX_OK) {
            b->held |= bit;
            return true;
        }
    }
    return false;
}

// Auto-flush: launch the collecting batch once its input reaches the threshold (batcher lock held).
int32_t maybe_autoflush(nx_batcher* b, Batch* bt) {
    if (!b->flush_bytes || bt != b->cur || bt->st_used + bt->direct_used < b->flush_bytes) return NX_OK;
    b->cur = nullptr;
    return launch(b, bt);
}

// Every submit starts here (batcher lock held): the workspace its kernels need is held (ws; Count for a
// job without GPU work), the collecting batch is open (bt) and the job has the next ticket.  The job is
// the caller's until register_job(): a submit that fails on the way drops it, its ticket number spent.
// nullptr: NX_ERR_HIP.
JobPtr open_job(nx_batcher* b, Batch*& bt, nx::WsKind ws, JobKind kind, Codec codec = Codec::FastLz) {
    if (ws != nx::WsKind::Count && !ensure_held(b, ws)) return nullptr;
    if (!(bt = collecting(b))) return nullptr;
    JobPtr j(new Job());
    j->ticket = b->next_ticket++;
    j->kind = kind;
    j->codec = codec;
    return j;
}

// ... and ends here: the batch owns the job and its ticket is out.
int64_t register_job(nx_batcher* b, Batch* bt, JobPtr job) {
    Job* j = job.release();
    bt->jobs.push_back(j);
    j->home = bt;
    bt->live += 1;
    b->tickets[j->ticket] = {bt, j};
    const int64_t t = (int64_t)j->ticket;
    (void)maybe_autoflush(b, bt);  // a failed launch completes the job with the error (result())
    return t;
}

}  // namespace

// ======================================================================= C-ABI
extern "C" nx_batcher* nx_batcher_new(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return nullptr;
    if (nx::crc_tables_init() != NX_OK) return nullptr;
    auto* b = new nx_batcher();
    for (int i = 0; i < kStreams; ++i) {
        if (hipStreamCreateWithFlags(&b->s[i], hipStreamNonBlocking) != hipSuccess) {
            for (int k = 0; k < i; ++k) (void)hipStreamDestroy(b->s[k]);
            delete b;
            return nullptr;
        }
    }
    // The workspaces (one per kind for the whole batcher, whichever of its streams a flush lands on)
    // are held by the first submit that needs them, or by nx_batcher_reserve.
    if (hipGetDevice(&b->dev) != hipSuccess) {
        nx_batcher_free(b);
        return nullptr;
    }
    return b;
}

extern "C" int32_t nx_batcher_reserve(nx_batcher* b, uint32_t kinds) {
    if (!b) return NX_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(b->mu);
    for (int k = 0; k < (int)nx::WsKind::Count; ++k)
        if ((kinds >> k) & 1u)
            if (!ensure_held(b, (nx::WsKind)k)) return NX_ERR_HIP;
    return NX_OK;
}

extern "C" void nx_batcher_free(nx_batcher* b) {
    if (!b) return;
    for (int i = 0; i < kStreams; ++i) (void)hipStreamSynchronize(b->s[i]);
    for (Batch* x : b->all) delete x;
    for (int i = 0; i < kStreams; ++i) {
        nx::ws_forget_stream(b->s[i]);  // no workspace event may outlive its stream
        (void)hipStreamDestroy(b->s[i]);
    }
    for (int k = 0; k < (int)nx::WsKind::Count; ++k)
        if ((b->held >> k) & 1u) nx::ws_unhold((nx::WsKind)k, b->dev);
    delete b;
}

extern "C" int32_t nx_host_register(void* p, size_t n) {
    if (!p || !n) return NX_ERR_INVALID_ARG;
    if (hipHostRegister(p, n, hipHostRegisterPortable | hipHostRegisterMapped) != hipSuccess) return NX_ERR_HIP;
    void* d = nullptr;
    if (hipHostGetDevicePointer(&d, p, 0) != hipSuccess) {
        (void)hipHostUnregister(p);
        return NX_ERR_HIP;
    }
    std::lock_guard<std::mutex> lk(g_reg_mu);
    g_reg[(uintptr_t)p] = {n, (uint8_t*)d};
    return NX_OK;
}

extern "C" int32_t nx_host_unregister(void* p) {
    if (!p) return NX_ERR_INVALID_ARG;
    {
        std::lock_guard<std::mutex> lk(g_reg_mu);
        g_reg.erase((uintptr_t)p);
    }
    return hipHostUnregister(p) == hipSuccess ? NX_OK : NX_ERR_HIP;
}

extern "C" int64_t nx_snappy_frame_encoder_submit(nx_snappy_frame_encoder* e, nx_batcher* b, const uint8_t* in, size_t n,
                                                  int32_t in_registered) {
    if (!e || !b || (!in && n)) return NX_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(b->mu);
    Batch* bt = nullptr;
    JobPtr j = open_job(b, bt, nx::WsKind::SnappyEnc, JobKind::SnappyEnc);
    if (!j) return NX_ERR_HIP;
    EncJob E{};
    E.s0 = (uint32_t)bt->esl.size();
    if (!bt->reserve_out(nx_snappy_frame_max_encoded_length(n), &E.out_off)) return NX_ERR_HIP;
    if (n) {  // SnappyFrameEncoder.encode (:79-117): !in.isReadable() writes nothing
        E.stream_start = e->started ? 0u : 1u;  // e->started is set below, once the submit cannot fail
        uint64_t base = 0;
        const uint8_t* dsrc = in_registered ? registered_device_ptr(in, n) : nullptr;
        if (in_registered && !dsrc) return NX_ERR_INVALID_ARG;  // not inside an nx_host_register'd range
        const bool direct = dsrc != nullptr;
        if (direct) {  // DMA'd into the device arena's direct region at flush; adjacent inputs share one copy
            Batch::Direct* last = bt->direct.empty() ? nullptr : &bt->direct.back();
            if (last && last->src + last->len == in && last->din_off + last->len == bt->direct_used) {
                base = bt->direct_used;
                last->len += n;
            } else {
                base = (bt->direct_used + 15) & ~15ull;
                bt->direct.push_back({in, dsrc, n, base});
            }
            bt->direct_used = base + n;
        } else {
            uint8_t* st = bt->stage(n, &base);
            if (!st) return NX_ERR_HIP;
            nx::copy_bytes(st, in, n);
        }
        auto add = [&](uint64_t off, uint32_t len, bool comp) {
            EncSlice S{base + off, bt->eslots, len, comp ? 1u : 0u};
            bt->eslots += (nx_snappy_max_compressed_length(len) + 15) & ~(size_t)15;
            bt->esl.push_back(S);
            bt->esl_direct.push_back(direct ? 1 : 0);
        };
        int64_t dl = (int64_t)n;
        if (dl > 18) {  // MIN_COMPRESSIBLE_LENGTH (:46,90-113)
            uint64_t pos = 0;
            for (;;) {
                if (dl < 18) {
                    add(pos, (uint32_t)dl, false);
                    break;
                }
                const uint32_t len = dl > e->slice ? (uint32_t)e->slice : (uint32_t)dl;
                add(pos, len, true);
                pos += len;
                if (dl > e->slice) dl -= e->slice;
                else break;
            }
        } else {
            add(0, (uint32_t)n, false);
        }
        e->started = true;
    }
    E.ns = (uint32_t)bt->esl.size() - E.s0;
    j->index = (uint32_t)bt->ejob.size();
    bt->ejob.push_back(E);
    return register_job(b, bt, std::move(j));
}

namespace {
int64_t decoder_submit(nx_snappy_frame_decoder* d, nx_batcher* b, const uint8_t* in, size_t n, size_t* consumed, bool registered) {
    if (!d || !b || (!in && n) || !consumed) return NX_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(b->mu);
    Batch* bt = nullptr;
    JobPtr job = open_job(b, bt, nx::WsKind::DecRecords, JobKind::SnappyDec);
    if (!job) return NX_ERR_HIP;
    Job* j = job.get();
    j->bind(d);
    size_t p = 0;  // bytes of `in` consumed
    // the chunk-header walk runs now, so the decoder's started/skip state advances in call order; it
    // is committed below, once the job is queued
    bool started = d->started;
    uint64_t skip = d->skip;
    const uint8_t* S = in;  // the walked bytes: a validating decoder's carried bytes, then `in`
    size_t carried = 0, walked = 0;
    std::vector<uint8_t> joined;
    const bool skipping = d->corrupted || d->parse_failed;  // (:86-89): an earlier input failed
    if (skipping) {
        p = n;
    } else {
        if (d->validate) {
            carried = (size_t)(d->hist.end - d->parse_pos);
            if (carried) {
                joined.reserve(carried + n);
                d->hist.copy_from(d->parse_pos, joined);
                joined.insert(joined.end(), in, in + n);
                S = joined.data();
            }
        }
        walked = walk(d, j, S, carried + n, started, skip);
        p = walked > carried ? walked - carried : 0;
    }
    // registered cumulation: the consumed bytes are gathered from the mapped pages at flush (the
    // caller keeps them valid until the job completes); else every payload is copied now
    const uint8_t* dS = nullptr;
    if (registered && walked && !carried) {
        dS = registered_device_ptr(in, walked);
        if (!dS) return NX_ERR_INVALID_ARG;  // not inside an nx_host_register'd range
    }
    // a validating decoder stages the walked bytes whole (headers too): the payloads are slices of
    // that copy, and its history references it instead of copying the bytes a second time
    int64_t staged = -1;
    if (d->validate && !dS && walked) {
        uint64_t off = 0;
        uint8_t* st = bt->stage(walked, &off);
        if (!st) return NX_ERR_HIP;
        nx::copy_bytes(st, S, walked);
        staged = (int64_t)off;
    }
    if (enqueue_dec(bt, j, S, walked, dS, staged) != NX_OK) return NX_ERR_HIP;
    *consumed = p;
    if (!skipping) {
        d->started = started;
        d->skip = skip;
        // later submits skip their input (:227-230); the decoder turns corrupted when this job is
        // applied, after the jobs submitted before it have delivered their messages
        if (j->has_parse_err) d->parse_failed = true;
    }
    if (d->validate && !d->corrupted) {
        // every consumed byte is kept until no unapplied job can re-walk it (a leftover, :206-212);
        // skipped input too, since a re-walk may find that the failure was not reached after all
        // a registered cumulation stays valid until this job completes, and so does the job's copy in
        // the staging arena: referenced, not copied
        if (staged >= 0)
            d->hist.append_staged(&bt->staging.h, (uint64_t)staged + carried, p);
        else
            d->hist.append(in, p, !registered);
        if (!skipping) {
            j->s_base = d->parse_pos;
            j->epoch = d->epoch;
            j->walked = true;
            d->outstanding.insert(j->s_base);
            d->parse_pos += walked;
        }
    }
    return register_job(b, bt, std::move(job));
}
}  // namespace

extern "C" int64_t nx_snappy_frame_decoder_submit(nx_snappy_frame_decoder* d, nx_batcher* b, const uint8_t* in, size_t n,
                                                  size_t* consumed) {
    return decoder_submit(d, b, in, n, consumed, false);
}

extern "C" int64_t nx_snappy_frame_decoder_submit_registered(nx_snappy_frame_decoder* d, nx_batcher* b, const uint8_t* in, size_t n,
                                                             size_t* consumed) {
    return decoder_submit(d, b, in, n, consumed, true);
}

// ---------------------------------------------------------------- FastLZ / LZF / LZ4 submits
namespace {
using nx::bt::AltPiece;

// Where an alt-codec submit found the batch: its pieces and list entries come after.  undo() takes them
// out again (the batch's other jobs stay valid).
struct AltMark {
    size_t apc, n[kAltLists];
    uint64_t aslots;
    explicit AltMark(const Batch* bt) : apc(bt->apc.size()), aslots(bt->aslots) {
        for (int c = 0; c < kAltLists; ++c) n[c] = bt->alt[c].size();
    }
    void undo(Batch* bt) const {
        bt->apc.resize(apc);
        for (int c = 0; c < kAltLists; ++c) bt->alt[c].resize(n[c]);
        bt->aslots = aslots;
    }
};

// Register job j, whose pieces are those added since `mark` (nothing else of the submit can fail once
// they are), with an output reservation of `out_need`.  On failure the batch is as it was at the mark.
// A decoder job learns its handle `dec` once registered: a failing launch of its own auto-flush fails the
// job and leaves the decoder as it is.
int64_t queue_alt(nx_batcher* b, Batch* bt, JobPtr j, const AltMark& mark, size_t out_need, nx_alt_decoder_base* dec = nullptr) {
    nx::bt::AltJobD J{};
    J.p0 = (uint32_t)mark.apc;
    J.np = (uint32_t)(bt->apc.size() - mark.apc);
    if (!bt->reserve_out(out_need + 16, &J.out_off)) {
        mark.undo(bt);
        return NX_ERR_HIP;
    }
    j->index = (uint32_t)bt->ajob.size();
    bt->ajob.push_back(J);
    Job* const queued = j.get();
    const int64_t t = register_job(b, bt, std::move(j));
    if (dec) queued->bind(dec);
    return t;
}

uint32_t push_list(std::vector<AltEntry>& L, uint64_t off, uint32_t len, uint64_t slot, uint32_t aux, int32_t lim = 0) {
    L.push_back({off, slot, len, aux, lim});
    return (uint32_t)L.size() - 1;
}

// Decoder submit, shared by the three codecs: the header walk runs now (the decoder's state advances
// in call order, as ByteToMessageDecoder would call decode()); the walked bytes are staged; the blocks
// decode at flush; apply() delivers messages / the first failure in order.
template <class D, class St, class Walk>
int64_t alt_decoder_submit(D* d, St& st, nx_batcher* b, const uint8_t* in, size_t n, size_t* consumed, Codec codec, bool validate,
                           Walk walk) {
    if (!d || !b || (!in && n) || !consumed) return NX_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(b->mu);
    Batch* bt = nullptr;
    JobPtr j = open_job(b, bt, nx::WsKind::DecRecords, JobKind::AltDec, codec);
    if (!j) return NX_ERR_HIP;
    j->validate = validate;
    const bool flz = codec == Codec::FastLz;
    const AltMark mark(bt);
    size_t p = n;
    size_t out_need = 0;
    St ns = st;
    const bool skipping = d->corrupted || d->parse_failed;  // an earlier input failed: Java skips everything
    if (!skipping) {
        p = walk(in, n, ns, j->ablk, j->awerr);
        if (j->awerr.set) p = n;  // the rest is skipped once the decoder is corrupted
    }
    if (!j->ablk.empty()) {
        // stage from the first block on; FastLZ's decompress() may read on to the end of the cumulation
        const size_t lo = j->ablk.front().data, hi = flz ? n : j->ablk.back().end;
        uint64_t off = 0;
        uint8_t* stg = bt->stage(hi - lo, &off);
        if (!stg) return NX_ERR_HIP;
        nx::copy_bytes(stg, in + lo, hi - lo);
        j->astage = off - lo;  // block b's payload is at staging offset astage + b.data
        for (const nx::af::Blk& k : j->ablk) {
            AltPiece P{};
            P.src = j->astage + k.data;
            P.len = k.clen;
            P.olen = k.olen;
            if (validate && k.has_cks) P.cks = flz ? nx::bt::CK_ADLER32 : nx::bt::CK_XXH32;  // its place in the lists: at flush
            if (!k.comp) {
                P.kind = nx::bt::AK_DEC_RAW;
            } else {
                P.slot = bt->aslots;
                bt->aslots += align16(k.olen) + 16;
                // FastLZ: aux = in_avail (readable bytes from the block on), lim = originalLength;
                // LZF / LZ4: aux = the decoded length
                P.res = push_list(bt->alt[FLZ_D + (int)codec], P.src, k.clen, P.slot, flz ? (uint32_t)(n - k.data) : k.olen, (int32_t)k.olen);
                P.kind = flz ? nx::bt::AK_DEC_FLZ : (codec == Codec::Lzf ? nx::bt::AK_DEC_LZF : nx::bt::AK_DEC_LZ4);
            }
            bt->apc.push_back(P);
            out_need += align16(k.olen);
        }
    }
    const bool walk_failed = j->awerr.set;
    const int64_t t = queue_alt(b, bt, std::move(j), mark, out_need, d);
    if (t < 0) return t;
    *consumed = p;
    if (!skipping) {
        st = ns;
        if (walk_failed) d->parse_failed = true;  // later submits skip; corrupted once applied
    }
    return t;
}
}  // namespace

extern "C" int64_t nx_fastlz_frame_decoder_submit(nx_fastlz_frame_decoder* d, nx_batcher* b, const uint8_t* in, size_t n,
                                                  size_t* consumed) {
    if (!d) return NX_ERR_INVALID_ARG;
    return alt_decoder_submit(d, d->st, b, in, n, consumed, Codec::FastLz, d->validate, nx::af::flz_walk);
}

extern "C" int64_t nx_lzf_decoder_submit(nx_lzf_decoder* d, nx_batcher* b, const uint8_t* in, size_t n, size_t* consumed) {
    if (!d) return NX_ERR_INVALID_ARG;
    return alt_decoder_submit(d, d->st, b, in, n, consumed, Codec::Lzf, false, nx::af::lzf_walk);
}

extern "C" int64_t nx_lz4_frame_decoder_submit(nx_lz4_frame_decoder* d, nx_batcher* b, const uint8_t* in, size_t n,
                                               size_t* consumed) {
    if (!d || !b || (!in && n) || !consumed) return NX_ERR_INVALID_ARG;
    if (d->st.state == 2 && !d->corrupted && !d->parse_failed) {  // FINISHED: everything is skipped (:250-254)
        std::lock_guard<std::mutex> lk(b->mu);
        Batch* bt = nullptr;
        JobPtr j = open_job(b, bt, nx::WsKind::Count, JobKind::AltDec, Codec::Lz4);
        if (!j) return NX_ERR_HIP;
        const int64_t t = queue_alt(b, bt, std::move(j), AltMark(bt), 0, d);
        if (t >= 0) *consumed = n;
        return t;
    }
    return alt_decoder_submit(d, d->st, b, in, n, consumed, Codec::Lz4, d->validate, nx::af::lz4_walk);
}

// FastLzFrameEncoder.encode(ctx, in, out) over buf[r0 .. r0 + n) as a job (the reader index enters the
// readU16 quirk, FastLz.java:552-557).  The message is copied now.
extern "C" int64_t nx_fastlz_frame_encoder_submit(nx_fastlz_frame_encoder* e, nx_batcher* b, const uint8_t* buf, size_t r0, size_t n) {
    if (!e || !b || (!buf && n)) return NX_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(b->mu);
    Batch* bt = nullptr;
    JobPtr j = open_job(b, bt, nx::WsKind::FastLzEnc, JobKind::AltEnc, Codec::FastLz);
    if (!j) return NX_ERR_HIP;
    const AltMark mark(bt);
    if (n) {
        uint64_t off = 0;
        uint8_t* stg = bt->stage(n, &off);
        if (!stg) return NX_ERR_HIP;
        nx::copy_bytes(stg, buf + r0, n);
        std::vector<nx::af::FlzPlan> plan;
        nx::af::flz_plan(r0, n, plan);
        for (const nx::af::FlzPlan& q : plan) {
            AltPiece P{};
            P.kind = nx::bt::AK_FLZ_ENC;
            P.src = off + q.ioff;
            P.len = q.ilen;
            P.slot = bt->aslots;
            bt->aslots += align16(nx_fastlz_max_compressed_length(q.ilen) + 16);
            P.res = push_list(bt->alt[FLZ_E], P.src, q.ilen, P.slot, (uint32_t)e->level, q.lim);
            P.aux = e->checksum ? 1u : 0u;
            bt->apc.push_back(P);
        }
    }
    return queue_alt(b, bt, std::move(j), mark, nx_fastlz_frame_max_encoded_length(n));
}

// LzfEncoder.encode(ctx, in, out) as a job (LzfEncoder.java:169-246): below the compress threshold the
// message leaves as non-compressed blocks, else every 65535-byte chunk goes to the GPU encoder.
extern "C" int64_t nx_lzf_encoder_submit(nx_lzf_encoder* e, nx_batcher* b, const uint8_t* in, size_t n) {
    if (!e || !b || (!in && n)) return NX_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(b->mu);
    Batch* bt = nullptr;
    JobPtr j = open_job(b, bt, nx::WsKind::LzfEnc, JobKind::AltEnc, Codec::Lzf);
    if (!j) return NX_ERR_HIP;
    const AltMark mark(bt);
    uint64_t off = 0;
    if (n) {
        uint8_t* stg = bt->stage(n, &off);
        if (!stg) return NX_ERR_HIP;
        nx::copy_bytes(stg, in, n);
    }
    const bool comp = (int64_t)n >= e->threshold;
    size_t ip = 0;
    do {  // encodeNonCompress writes one (possibly empty) block even for n == 0 (:223-246)
        const uint32_t len = (uint32_t)((n - ip) < 65535 ? (n - ip) : 65535);
        AltPiece P{};
        P.src = off + ip;
        P.len = len;
        if (comp) {
            P.kind = nx::bt::AK_LZF_ENC;
            P.slot = bt->aslots;
            bt->aslots += align16(nx_lzf_max_compressed_length(len) + 16);
            P.res = push_list(bt->alt[LZF_E], P.src, len, P.slot, 0);
        } else {
            P.kind = nx::bt::AK_LZF_RAW;
        }
        bt->apc.push_back(P);
        ip += len;
    } while (ip < n);
    return queue_alt(b, bt, std::move(j), mark, nx_lzf_frame_max_encoded_length(n));
}

// Lz4FrameEncoder as jobs: op 0 = encode(in) (full blocks of the block buffer leave, :231-248), 1 =
// flush() (the partial block too, :291-300), 2 = close() (flush + the end block, :317-336; afterwards
// encode passes bytes through, :233-239).  The handle's block buffer advances at submit.
extern "C" int64_t nx_lz4_frame_encoder_submit(nx_lz4_frame_encoder* e, nx_batcher* b, const uint8_t* in, size_t n, int32_t op) {
    if (!e || !b || (!in && n) || op < 0 || op > 2) return NX_ERR_INVALID_ARG;
    // allocateBuffer's maxEncodeSize check (Lz4FrameEncoder.java:190-214): write() sizes the message
    // plus the buffered bytes; a bare flush (op 1, no bytes) sizes the buffer (:296-304); finishEncode
    // checks nothing (:306-315).  Nothing is queued or buffered when it fails.
    if (n > 0 || op == 0 || (op == 1 && !e->buf.empty())) {
        int32_t target = 0;
        int32_t r = nx_lz4_frame_encoder_check_size(e, (uint64_t)n + e->buf.size(), &target);
        if (r == NX_OK) r = nx_lz4_frame_encoder_check_finished(e, n, target);  // IllegalStateException after close
        if (r != NX_OK) return r;
    }
    std::lock_guard<std::mutex> lk(b->mu);
    Batch* bt = nullptr;
    JobPtr j = open_job(b, bt, e->high ? nx::WsKind::Lz4HcEnc : nx::WsKind::Lz4Enc, JobKind::AltEnc, Codec::Lz4);
    if (!j) return NX_ERR_HIP;
    const AltMark mark(bt);
    std::vector<uint8_t> nbuf;  // the block buffer after this job
    size_t out_need = 0;
    if (e->finished) {  // pass-through (:233-239); flush / close after close write nothing
        if (n) {
            uint64_t off = 0;
            uint8_t* stg = bt->stage(n, &off);
            if (!stg) return NX_ERR_HIP;
            nx::copy_bytes(stg, in, n);
            AltPiece P{};
            P.kind = nx::bt::AK_RAW;
            P.src = off;
            P.len = (uint32_t)n;
            bt->apc.push_back(P);
            out_need = n;
        }
        nbuf = e->buf;
    } else {
        const size_t have = e->buf.size(), total = have + n, bs = e->block_size;
        const size_t full = op == 0 ? total / bs * bs : total;  // flush / close take the partial block too
        if (full) {
            uint64_t off = 0;
            uint8_t* stg = bt->stage(full, &off);
            if (!stg) return NX_ERR_HIP;
            const size_t from_buf = have < full ? have : full;
            nx::copy_bytes(stg, e->buf.data(), from_buf);
            if (full > from_buf) nx::copy_bytes(stg + from_buf, in, full - from_buf);
            for (size_t q = 0; q < full; q += bs) {
                const uint32_t len = (uint32_t)((full - q) < bs ? (full - q) : bs);
                AltPiece P{};
                P.kind = nx::bt::AK_LZ4_ENC;
                P.src = off + q;
                P.len = len;
                P.slot = bt->aslots;
                const uint64_t cap = nx::af::kLz4Header + nx_lz4_max_compressed_length(len);
                bt->aslots += align16(cap) + 16;
                P.res = push_list(bt->alt[LZ4_E], P.src, len, P.slot, (uint32_t)e->level | (e->high ? 0x100u : 0u));
                bt->apc.push_back(P);
                out_need += cap;
            }
        }
        if (full < have) nbuf.assign(e->buf.begin() + (ptrdiff_t)full, e->buf.end());  // (op 0 with a short input)
        if (full >= have) nbuf.assign(in + (full - have), in + n);
        else nbuf.insert(nbuf.end(), in, in + n);
        if (op == 2) {
            AltPiece P{};
            P.kind = nx::bt::AK_LZ4_END;
            P.aux = (uint32_t)e->level;
            bt->apc.push_back(P);
            out_need += nx::af::kLz4Header;
        }
    }
    const int64_t t = queue_alt(b, bt, std::move(j), mark, out_need);
    if (t < 0) return t;
    if (!e->finished) e->buf.swap(nbuf);
    if (op == 2) e->finished = true;
    return t;
}

// ---------------------------------------------------------------- JdkZlibEncoder / JdkZlibDecoder submits
// JdkZlibEncoder.encode / finishEncode as a job (JdkZlibEncoder.java:214-276, 308-340): the header on the
// first non-empty job or the close, one deflate slice per 64 KiB on the list of its level class, the final
// block and the trailer's place on a close.  write_header, finished and total_in advance now; the running
// checksum at apply().
extern "C" int64_t nx_zlib_encoder_submit(nx_zlib_encoder* e, nx_batcher* b, const uint8_t* in, size_t n, int32_t op) {
    if (!e || !b || (!in && n) || (op != 0 && op != 2)) return NX_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(b->mu);
    Batch* bt = nullptr;
    JobPtr j = open_job(b, bt, nx::WsKind::DeflateEnc, JobKind::ZlibEnc);
    if (!j) return NX_ERR_HIP;
    const AltMark mark(bt);
    size_t out_need = 0;
    auto constant = [&](const uint8_t* p, size_t len) {
        AltPiece P{};
        P.kind = nx::bt::AK_CONST;
        P.len = (uint32_t)len;
        for (size_t k = 0; k < len; ++k) (k < 8 ? P.src : P.slot) |= (uint64_t)p[k] << (8 * (k & 7));
        bt->apc.push_back(P);
        out_need += len;
    };
    // a dictionary handle's first non-empty message is staged behind the dictionary's tail, the history
    // prefix of its first slice
    const uint32_t tail = n && !e->finished && e->dict_armed ? (uint32_t)e->dict.size() : 0u;
    uint64_t off = 0;
    if (n) {
        uint8_t* stg = bt->stage(tail + n, &off);
        if (!stg) return NX_ERR_HIP;
        nx::copy_bytes(stg, e->dict.data(), tail);
        nx::copy_bytes(stg + tail, in, n);
        off += tail;
    }
    const bool close = op == 2 && !e->finished;
    if (e->finished) {  // out.writeBytes(uncompressed) (:215-218); a second close writes nothing (:309-312)
        if (n) {
            AltPiece P{};
            P.kind = nx::bt::AK_RAW;
            P.src = off;
            P.len = (uint32_t)n;  // (a message is a ByteBuf: below 2 GiB)
            bt->apc.push_back(P);
            out_need = n;
        }
    } else {
        uint8_t hdr[16];
        if (e->write_header && (n || close)) constant(hdr, nx::zl::write_header(e, hdr));
        nx::zl::for_slices(n, tail, [&](size_t q, uint32_t len, uint32_t pre) {
            const bool stored = e->level == 0;
            AltPiece P{};
            P.kind = nx::bt::AK_DFL_ENC;
            P.src = off + q;
            P.len = len;
            P.olen = stored ? 0u : 1u;  // which launch (fill_upload)
            P.cks = e->wrapper == 1 ? nx::bt::CK_CRC32 : e->wrapper == 0 ? nx::bt::CK_ADLER32 : nx::bt::CK_NONE;
            P.slot = bt->aslots;
            const size_t cap = nx_deflate_max_compressed_length(len);
            bt->aslots += (cap + 127) & ~(size_t)127;
            P.res = push_list(bt->alt[stored ? DFL_S : DFL_M], P.src, len, P.slot, pre);  // aux: the slice's prefix_len
            bt->apc.push_back(P);
            out_need += cap;
        });
        if (close) {  // the final block (an empty fixed-Huffman block), then the trailer's place
            const uint8_t fin[10] = {0x03, 0x00};
            j->ztrailer = e->wrapper == 0 ? 4u : e->wrapper == 1 ? 8u : 0u;
            constant(fin, 2 + j->ztrailer);
        }
    }
    j->ztotal_in = e->total_in + n;
    const bool had_header = e->write_header && !e->finished && (n || close);
    Job* const queued = j.get();
    queued->bind(e);
    e->pending.fetch_add(1);
    const int64_t t = queue_alt(b, bt, std::move(j), mark, out_need);
    if (t < 0) {  // (the job, dropped, gave its reference back)
        e->pending.fetch_sub(1);
        return t;
    }
    if (!e->finished) {
        if (had_header) e->write_header = false;
        e->total_in += n;
        if (n) e->dict_armed = false;
        if (close) e->finished = true;
    }
    return t;
}

// JdkZlibDecoder.decode over the bytes handed over so far, as a job.  One job of a decoder runs at a time:
// it starts here when none is unapplied (wrapper bytes are parsed now; a body step joins the collecting
// batch), else it is held with its bytes until the earlier ones are applied.
extern "C" int64_t nx_zlib_decoder_submit(nx_zlib_decoder* d, nx_batcher* b, const uint8_t* in, size_t n, size_t* consumed) {
    if (!d || !b || (!in && n) || !consumed) return NX_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(b->mu);
    nx_batcher* none = nullptr;
    if (!d->owner.compare_exchange_strong(none, b) && none != b) return NX_ERR_INVALID_ARG;  // its jobs run on another batcher
    Batch* bt = nullptr;
    JobPtr job = open_job(b, bt, nx::WsKind::Count, JobKind::ZlibDec);
    if (!job) return NX_ERR_HIP;
    Job* j = job.get();
    j->bind(d);
    j->zin.assign(in, in + n);
    auto ch = b->zchan.find(d);
    if (ch != b->zchan.end()) {  // an earlier job is unapplied: held
        j->zheld = true;
        bt->zheld_n += 1;
        ch->second.held.push_back(j);
    } else if (zdec_start(j)) {
        if (zdec_enqueue(bt, j) != NX_OK) {
            zdec_fail(b, j, NX_ERR_HIP);
        } else {
            b->zchan[d].active = j;
        }
    }
    *consumed = n;
    return register_job(b, bt, std::move(job));
}

extern "C" int32_t nx_batcher_flush(nx_batcher* b) {
    if (!b) return NX_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(b->mu);
    b->kick = false;
    Batch* bt = b->cur;
    if (!bt || bt->jobs.empty()) return NX_OK;
    b->cur = nullptr;
    return launch(b, bt);
}

extern "C" int32_t nx_batcher_poll(nx_batcher* b, int64_t ticket) {
    if (!b) return NX_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(b->mu);
    auto it = b->tickets.find((uint64_t)ticket);
    if (it == b->tickets.end()) return NX_ERR_INVALID_ARG;
    Job* j = it->second.second;
    (void)poll_batch(b, progress_batch(b, j, it->second.first), false);
    kick(b);
    return j->applied ? 1 : 0;  // a re-walked job continues in a later batch
}

extern "C" int32_t nx_batcher_wait(nx_batcher* b, int64_t ticket) {
    if (!b) return NX_ERR_INVALID_ARG;
    for (;;) {  // more than one pass only when a re-walk moved the job to a later batch
        Batch* bt;
        Job* j;
        {
            std::lock_guard<std::mutex> lk(b->mu);
            auto it = b->tickets.find((uint64_t)ticket);
            if (it == b->tickets.end()) return NX_ERR_INVALID_ARG;
            j = it->second.second;
            if (j->applied) return NX_OK;  // (a zlib decoder job that needed no body step: complete since its submit)
            bt = progress_batch(b, j, it->second.first);
            if (bt == b->cur) {  // not flushed yet: flush now
                b->cur = nullptr;
                (void)launch(b, bt);  // a failed launch completes the batch's jobs with the error
            }
            if (j->applied) return NX_OK;
        }
        if (hipEventSynchronize(bt->ev) != hipSuccess) return NX_ERR_HIP;
        std::lock_guard<std::mutex> lk(b->mu);
        // Unlocked, another thread's apply() may have moved the job into a continuation batch (a
        // re-walk), after which bt can be reset and reused: look the ticket up again, and wait on
        // its new batch if it moved.
        auto it = b->tickets.find((uint64_t)ticket);
        if (it == b->tickets.end()) return NX_ERR_INVALID_ARG;
        if (progress_batch(b, j, it->second.first) != bt) continue;
        if (!poll_batch(b, bt, true)) return NX_ERR_HIP;
        kick(b);
        if (j->applied) return NX_OK;
    }
}

extern "C" int32_t nx_batcher_result(nx_batcher* b, int64_t ticket, const nx_msg** msgs, size_t* n_msgs, const char** err_msg) {
    if (!b || !msgs || !n_msgs) return NX_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(b->mu);
    auto it = b->tickets.find((uint64_t)ticket);
    if (it == b->tickets.end()) return NX_ERR_INVALID_ARG;
    Job* j = it->second.second;
    if (!j->applied) return NX_ERR_INVALID_ARG;  // poll() / wait() first
    *msgs = j->msgs.data();
    *n_msgs = j->msgs.size();
    if (err_msg) *err_msg = j->err.empty() ? nullptr : j->err.c_str();
    return j->status;
}

extern "C" int32_t nx_batcher_release(nx_batcher* b, int64_t ticket) {
    if (!b) return NX_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(b->mu);
    auto it = b->tickets.find((uint64_t)ticket);
    if (it == b->tickets.end()) return NX_ERR_INVALID_ARG;
    Batch* bt = it->second.first;
    b->tickets.erase(it);
    if (bt->live) bt->live -= 1;
    return NX_OK;
}

extern "C" int32_t nx_batcher_set_flush_bytes(nx_batcher* b, size_t bytes) {
    if (!b) return NX_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(b->mu);
    b->flush_bytes = bytes;
    return NX_OK;
}

// Size the pinned arenas now: at least `nbatches` batch objects, each with a staging arena of
// staging_bytes and a result arena of out_bytes, so that submits (on the event loops) never call
// hipHostMalloc / hipHostFree once batches stay within those sizes (set the auto-flush threshold
// below staging_bytes).
extern "C" int32_t nx_batcher_reserve_arenas(nx_batcher* b, uint32_t nbatches, size_t staging_bytes, size_t out_bytes) {
    if (!b) return NX_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(b->mu);
    while (b->all.size() < nbatches)
        if (!new_batch(b)) return NX_ERR_HIP;
    // A batch that holds jobs is left alone: an in-flight batch's arenas are being written, and the
    // results of an applied batch whose tickets are not all released (nx_batcher_result's messages),
    // or the staged bytes a collecting batch's jobs point into, live in its arenas; growing one
    // frees the old buffer under them.  Such a batch is sized when it is reused (reset, then staged).
    for (Batch* x : b->all)
        if (!x->inflight && x->live == 0 && x->jobs.empty() &&
            (!x->staging.ensure(staging_bytes, x->st_used) || !x->out.ensure(out_bytes, x->out_used) || !x->gops.ensure(1u << 20, 0)))
            return NX_ERR_HIP;
    return NX_OK;
}

extern "C" int32_t nx_batcher_arena_stats(nx_batcher* b, uint64_t* allocs, uint64_t* bytes, uint32_t* batches) {
    if (!b) return NX_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(b->mu);
    if (allocs) *allocs = b->arena.allocs;
    if (bytes) *bytes = b->arena.bytes;
    if (batches) *batches = (uint32_t)b->all.size();
    return NX_OK;
}

extern "C" int32_t nx_batcher_dma_stats(nx_batcher* b, uint64_t* dma_flushes, uint64_t* dma_bytes) {
    if (!b) return NX_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(b->mu);
    if (dma_flushes) *dma_flushes = b->dma_flushes;
    if (dma_bytes) *dma_bytes = b->dma_bytes;
    return NX_OK;
}

extern "C" int32_t nx_batcher_stats(nx_batcher* b, uint64_t* flushes, uint64_t* launches, uint64_t* chunks) {
    if (!b) return NX_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(b->mu);
    if (flushes) *flushes = b->flushes;
    if (launches) *launches = b->launches;
    if (chunks) *chunks = b->chunks;
    return NX_OK;
}
