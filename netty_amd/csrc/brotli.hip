// brotli.hip — Brotli (RFC 7932) stream encoder for BrotliEncoder (BrotliEncoder.java:47-230), two passes over
// independent items of any length up to kMaxItem.
//
// Every item becomes one complete stream: the WBITS header, meta-blocks of at most 65 536 input bytes, the
// empty last meta-block.  (A write of the BrotliEncoder handle is the same with the header left out after the
// first write and the flush marker in place of the last block: `flags`.)  The format subset, the matcher's
// rule, the walker and the meta-block encoder are in brotli_encode_core.hpp, which nx_brotli_encode_host runs
// on the CPU; the kernels must write the host's bytes, and the GPU tests compare them.
//
//   pass 1, k_seq_match<Match> (seq_stage.hpp), one lane per item on the lane grid of the other alt encoders: match_item over a
//     stamped hash table of 65 536 entries (stamp << 32 | position) in the item's workspace slot.  It writes
//     one 64-bit word per sequence (literal run, copy length, distance) to the item's area of the sequence
//     arena.  Literal bytes stay in the input, where pass 2 reads them.
//   pass 2, k_brotli_emit, one wave per item, meta-block after meta-block, the bit position and the distance
//     ring carried from one to the next.  The wave's LDS holds the core's Work area (histograms, tree nodes,
//     lengths, codes, the run-length form of a code description: 17 220 bytes, 17 232 allocated), a chunk of 64
//     command records laid over the tree nodes, and a 2 KiB bit ring of output: 19 312 bytes, 8 waves per CU.  Per meta-block: lane 0 walks the sequences with the core's walker and cuts them
//     into chunks of up to 64 records (next_chunk); the wave takes the three histograms from the records with
//     LDS atomics, a record and its literals a lane; per alphabet the wave sorts the used symbols by (count, symbol),
//     a rank sort as in zstd.hip, and lane 0 runs the core's two-queue tree and length limiting (block_lengths);
//     lane 0 runs the core's finish_block (codes, the exact bit count, the choice of form, header and code
//     descriptions); then chunk by chunk again every lane counts
//     its record's bits, a prefix sum over the wave places them, and the lanes OR the command, literal and
//     distance bits into the ring.  An uncompressed block's bytes go into the ring 1 KiB a round, all lanes.
//     All lanes store the ring as 16-byte pieces of whole 128-byte lines; only an item's last line goes out in
//     smaller pieces.  No byte at or beyond the slot's capacity is stored.
//     What is shared with the host encoder is the walker (next_cmd), the symbols of a command (make_syms), the
//     tree (tree_depths) and finish_block.  The histograms, the sort and the command stream's bits are written
//     here by kernel-only code (next_chunk and the scan, sort and emit rounds) and checked byte for byte against
//     the host's scan_block, sort_symbols and step_command by tests/test_gpu_brotli_encode.py.
//
// The sequence arena is the side allocation of the NX_WS_BROTLI_ENC workspace, freed whenever its tables are: an
// item of n bytes takes 16 + 8 * seq_cap(n) bytes of it.  The host reads in_len back, lays the areas out and cuts
// the batch into launch pairs whose items fit the table slots and kWsAreaMax bytes of arena (WsAreaCut,
// workspace.hpp); a call therefore synchronises its stream once, before its first launch.
#include <algorithm>
#include "alt_frames.hpp"
#include "brotli_encode_core.hpp"
#include "nx_common.hpp"
#include "seq_stage.hpp"
#include "workspace.hpp"

namespace nx {
namespace brotli {

constexpr uint32_t kMaxItem = 256u << 20;
constexpr uint32_t kSlotBytes = 8u << kHashLog;
constexpr uint32_t kStageBytes = 2048, kLine = kSeqLine, kCtrlBytes = 32;
constexpr uint32_t kWorkBytes = (uint32_t)((sizeof(Work) + 15u) & ~(size_t)15);
constexpr uint32_t kLdsBytes = kStageBytes + kCtrlBytes + kWorkBytes;
static_assert(kLdsBytes <= 20480u, "eight waves of a CU share 160 KiB");

// pass 1: k_seq_match's codec; its parameter is lgwin
struct Match {
    static constexpr uint32_t kMaxItem = brotli::kMaxItem, kSlotBytes = brotli::kSlotBytes;
    static __device__ __forceinline__ size_t seq_cap(size_t n) { return brotli::seq_cap(n); }
    static __device__ __forceinline__ uint32_t match_item(const uint8_t* in, uint32_t n, uint32_t lgwin, uint64_t* table, uint32_t stamp,
                                                          uint64_t* seq, size_t cap) {
        return brotli::match_item(in, n, lgwin, table, stamp, seq, cap);
    }
};

// ---------------------------------------------------------------------------------------- pass 2
// The item's output.  The LDS ring (seq_stage.hpp) is a bit ring here: byte `p` of the output lives at
// ring[p & (kStageBytes - 1)] from the moment any of its bits is known until its line is stored, and every ring
// byte at or beyond `at` that no bit has reached is zero (the ring is cleared per item and again behind every
// stored piece), so lanes may OR bits in.  Lane 0's own bytes (the core's header and code descriptions) are
// stored whole at `at`.  A round adds at most kChunkBytes to under a line left from the round before, so the
// ring (2 KiB) is never passed; the sink's direct store is the guard for that, not a path.
using Sink = StageSink<kStageBytes>;

// A chunk of a meta-block's commands, cut by lane 0 for the wave: up to 64 records with at most kChunkLits
// literals between them.  A record is the bits before its literals (the command symbol and the insert and copy
// extra bits: up to 63), a run of literals in the input, and the bits after them (the distance symbol and its
// extra bits: up to 37).  A command with more literals than a chunk takes continues in records of literals alone.
constexpr uint32_t kChunkLits = 448, kNoCmd = 0xFFFFu, kNoDist = 0xFFu;
constexpr uint32_t kChunkBytes = (64u * (63u + 37u) + kChunkLits * 15u + 7u) / 8u + 1u;  // 1 641
constexpr uint32_t kRawRound = 1024;  // raw bytes of an uncompressed meta-block a round stages
// finish_block writes 33 header bits and three code descriptions of at most 2 + 18 * 4 bits and 8 bits a symbol
constexpr uint32_t kCloseBytes = (33u + 3u * 74u + 8u * kSyms + 7u) / 8u + 1u;  // 1 057
static_assert(kLine + kChunkBytes <= kStageBytes && kLine + kCloseBytes <= kStageBytes && kLine + kRawRound <= kStageBytes,
              "a round fits the ring");
struct Recs {
    uint64_t pre[64], post[64];
    uint32_t lit_start[64], lit_n[64];
    uint16_t cmd[64];
    uint8_t dsym[64], pre_nb[64], post_nb[64];
};

// The records lie over Work::node_w: the tree nodes are live only between a block's scan and its emit rounds.
static_assert(sizeof(Recs) <= sizeof(Work::node_w) && offsetof(Work, node_w) % 16u == 0u, "record area");

// Lane 0: the next chunk of the meta-block from walker w and ring r (the scan's or the emitter's) into R; emit:
// with the bits, which need the block's codes; else the scan, which adds up the extra bits.  Returns the records.
__device__ __forceinline__ uint32_t next_chunk(Encoder<Sink>& E, Walk& w, Ring& r, bool emit, Recs* R) {
    const Work* W = E.W;
    uint32_t cnt = 0, lits = 0;
    while (cnt < 64u) {
        uint32_t from, k;
        if (E.in_cmd) {  // the rest of a command's literals
            const uint32_t room = kChunkLits - lits, left = E.lit_end - E.lit_at;
            k = left < room ? left : room;
            if (k == 0u) break;
            from = E.lit_at;
            R->cmd[cnt] = (uint16_t)kNoCmd;
            R->pre[cnt] = 0;
            R->pre_nb[cnt] = 0;
        } else {
            if (w.ip >= E.mb_end) break;
            Walk t = w;
            from = t.ip;
            const Cmd c = next_cmd(t, E.seq, E.ns, E.n, E.mb_end);
            if (cnt != 0u && c.ins > kChunkLits - lits) break;  // it opens the next chunk
            w = t;
            E.sy = make_syms(c, r);
            k = c.ins < kChunkLits - lits ? c.ins : kChunkLits - lits;
            E.lit_end = from + c.ins;
            E.in_cmd = true;
            R->cmd[cnt] = (uint16_t)E.sy.cmd;
            if (emit) {
                const uint32_t d = W->depth[kCmd + E.sy.cmd];
                R->pre[cnt] = (uint64_t)W->code[kCmd + E.sy.cmd] | ((uint64_t)E.sy.ins_val << d) | ((uint64_t)E.sy.cp_val << (d + E.sy.ins_nb));
                R->pre_nb[cnt] = (uint8_t)(d + E.sy.ins_nb + E.sy.cp_nb);
            } else {
                E.scan_bits += E.sy.ins_nb + E.sy.cp_nb + E.sy.d_nb;
            }
        }
        R->lit_start[cnt] = from;
        R->lit_n[cnt] = k;
        R->dsym[cnt] = (uint8_t)kNoDist;
        R->post[cnt] = 0;
        R->post_nb[cnt] = 0;
        E.lit_at = from + k;
        lits += k;
        if (E.lit_at == E.lit_end) {  // the command is whole: its distance goes behind the literals
            E.in_cmd = false;
            if (E.sy.has_dist) {
                R->dsym[cnt] = (uint8_t)E.sy.dsym;
                if (emit) {
                    const uint32_t d = W->depth[kDist + E.sy.dsym];
                    R->post[cnt] = (uint64_t)W->code[kDist + E.sy.dsym] | ((uint64_t)E.sy.d_val << d);
                    R->post_nb[cnt] = (uint8_t)(d + E.sy.d_nb);
                }
            }
        }
        ++cnt;
    }
    return cnt;
}

// nb (<= 32) bits of v at bit position `bit` of the ring.
__device__ __forceinline__ void or_bits(uint32_t* ringw, uint32_t bit, uint32_t v, uint32_t nb) {
    if (nb == 0u) return;
    const uint32_t i = (bit >> 5) & (kStageBytes / 4u - 1u), sh = bit & 31u;
    atomicOr(&ringw[i], v << sh);
    if (sh + nb > 32u) atomicOr(&ringw[(i + 1u) & (kStageBytes / 4u - 1u)], v >> (32u - sh));
}
__device__ __forceinline__ void or_bits64(uint32_t* ringw, uint32_t bit, uint64_t v, uint32_t nb) {
    const uint32_t lo = nb < 32u ? nb : 32u;
    or_bits(ringw, bit, (uint32_t)v, lo);
    or_bits(ringw, bit + lo, (uint32_t)(v >> 32), nb - lo);
}

enum : uint32_t { kModeNone = 0, kModeClear, kModeScan, kModeSort, kModeEmit, kModeRaw };

__global__ void __launch_bounds__(64) k_brotli_emit(const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off,
                                                    const uint32_t* __restrict__ in_len, uint8_t* __restrict__ out,
                                                    const uint64_t* __restrict__ out_off, uint32_t* __restrict__ out_len,
                                                    int32_t* __restrict__ status, uint32_t n, const uint8_t* __restrict__ arena,
                                                    const uint64_t* __restrict__ aoff, uint32_t lgwin, uint32_t flags) {
    extern __shared__ __align__(16) uint8_t smem[];
    uint8_t* ring = smem;
    uint32_t* ringw = reinterpret_cast<uint32_t*>(smem);
    volatile uint32_t* ctrl = reinterpret_cast<volatile uint32_t*>(smem + kStageBytes);
    Work* work = reinterpret_cast<Work*>(smem + kStageBytes + kCtrlBytes);
    Recs* R = reinterpret_cast<Recs*>(work->node_w);
    const uint32_t lane = threadIdx.x;
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
        const uint8_t* src = in + in_off[c];
        uint8_t* dst = out + out_off[c];
        const uint32_t lead = (uint32_t)((uintptr_t)dst & (kLine - 1u));
        uint8_t* origin = dst - lead;
        const Sink sink = {ring, origin, lead, lead, lead + cap, false};
        Encoder<Sink> E;
        for (uint32_t i = lane; i < kStageBytes / 4u; i += 64u) ringw[i] = 0;
        if (lane == 0u) E.init(work, sink, nullptr, src, len, area + 2, ns, lgwin, flags);
        __syncthreads();
        // every round moves the item on: a step of the core, a chunk of records, or kRawRound raw bytes
        const uint64_t most = 2u * max_steps(len, ns) + 8u;
        uint32_t flushed = lead, fl = 0, at = lead, scanning = 0, sorted = 0;  // scanning 2 + a: alphabet a is sorted
        for (uint64_t round = 0; round <= most && !fl; ++round) {
            // lane 0: what this round is
            if (lane == 0u) {
                uint32_t mode = kModeNone, cnt = 0;
                if (E.state == Encoder<Sink>::kBlock) {
                    if (!scanning) {
                        E.open_block();
                        scanning = 1;
                        mode = kModeClear;
                    } else if (scanning == 1u) {
                        cnt = next_chunk(E, E.ws, E.rs, false, R);
                        if (cnt != 0u) {
                            mode = kModeScan;
                        } else {  // the histograms are whole: the wave sorts the literals' symbols
                            scanning = 2;
                            mode = kModeSort;
                        }
                    } else {  // alphabet scanning - 2 is sorted: its tree, then the next alphabet or the block's header
                        E.block_lengths(scanning - 2u, sorted);
                        if (++scanning < 5u) {
                            mode = kModeSort;
                        } else {
                            E.finish_block();
                            scanning = 0;
                        }
                    }
                    cnt = mode == kModeSort ? scanning - 2u : cnt;
                } else if (E.state == Encoder<Sink>::kCommands) {
                    cnt = next_chunk(E, E.w, E.r, true, R);
                    mode = kModeEmit;
                    or_bits(ringw, E.out.at * 8u, (uint32_t)E.acc, E.nacc);  // the bits of the byte that is not whole yet
                } else if (E.state == Encoder<Sink>::kRaw) {
                    const uint32_t left = E.mb_end - E.raw_at, room = E.out.end - E.out.at;
                    cnt = left < kRawRound ? left : kRawRound;
                    if (cnt > room) {
                        cnt = room;
                        E.out.full = true;
                    }
                    mode = kModeRaw;
                } else {
                    E.step();
                }
                ctrl[2] = mode;
                ctrl[3] = cnt;
                ctrl[4] = E.out.at * 8u + E.nacc;
                ctrl[5] = E.raw_at;
            }
            __syncthreads();
            const uint32_t mode = ctrl[2], cnt = ctrl[3];
            uint32_t total = 0;
            if (mode == kModeClear) {
                for (uint32_t s = lane; s < kSyms; s += 64u) work->hist[s] = 0;
            } else if (mode == kModeScan) {
                if (lane < cnt) {
                    if (R->cmd[lane] != kNoCmd) atomicAdd(&work->hist[kCmd + R->cmd[lane]], 1u);
                    if (R->dsym[lane] != kNoDist) atomicAdd(&work->hist[kDist + R->dsym[lane]], 1u);
                    const uint8_t* p = src + R->lit_start[lane];
                    for (uint32_t i = 0, k = R->lit_n[lane]; i < k; ++i) atomicAdd(&work->hist[kLit + p[i]], 1u);
                }
            } else if (mode == kModeSort) {
                // build_depths' sort across the wave: the used symbols gathered in symbol order, then each one's
                // rank by (count, symbol), which is the order the core's stable insertion sort gives
                const uint32_t base = cnt == 0u ? kLit : cnt == 1u ? kCmd : kDist, na = cnt == 0u ? 256u : cnt == 1u ? kNumCmd : kNumDist;
                uint16_t* used = work->node_parent;  // no tree is live
                uint32_t m = 0;
                for (uint32_t b = 0; b < na; b += 64u) {
                    const uint32_t s = b + lane;
                    const bool in_use = s < na && work->hist[base + s] != 0u;
                    if (s < na) work->depth[base + s] = 0;
                    const unsigned long long mask = __ballot(in_use);
                    if (in_use) used[m + __popcll(mask & ((1ull << lane) - 1ull))] = (uint16_t)s;
                    m += (uint32_t)__popcll(mask);
                }
                __syncthreads();
                for (uint32_t i = lane; i < m; i += 64u) {
                    const uint32_t s = used[i], h = work->hist[base + s];
                    uint32_t rank = 0;
                    for (uint32_t j = 0; j < m; ++j) {
                        const uint32_t hj = work->hist[base + used[j]];
                        rank += (hj < h || (hj == h && j < i)) ? 1u : 0u;
                    }
                    work->order[rank] = (uint16_t)s;
                }
                sorted = m;
            } else if (mode == kModeEmit) {
                // the record's bits, their place by a prefix sum over the wave, then the bits themselves
                uint32_t bits = 0;
                const uint8_t* p = src;
                uint32_t k = 0;
                if (lane < cnt) {
                    p = src + R->lit_start[lane];
                    k = R->lit_n[lane];
                    bits = (uint32_t)R->pre_nb[lane] + R->post_nb[lane];
                    for (uint32_t i = 0; i < k; ++i) bits += work->depth[kLit + p[i]];
                }
                uint32_t incl = bits;
                for (uint32_t d = 1; d < 64u; d <<= 1) {
                    const uint32_t o = __shfl_up(incl, d, 64);
                    if (lane >= d) incl += o;
                }
                total = __shfl(incl, 63, 64);
                if (lane < cnt) {
                    uint32_t bit = ctrl[4] + incl - bits;
                    or_bits64(ringw, bit, R->pre[lane], R->pre_nb[lane]);
                    bit += R->pre_nb[lane];
                    for (uint32_t i = 0; i < k; ++i) {
                        const uint32_t d = work->depth[kLit + p[i]];
                        or_bits(ringw, bit, work->code[kLit + p[i]], d);
                        bit += d;
                    }
                    or_bits64(ringw, bit, R->post[lane], R->post_nb[lane]);
                }
            } else if (mode == kModeRaw) {
                const uint32_t a0 = ctrl[4] >> 3, r0 = ctrl[5];  // a raw block starts on a byte
                for (uint32_t i = lane; i < cnt; i += 64u) ring[(a0 + i) & (kStageBytes - 1u)] = src[r0 + i];
            }
            __syncthreads();
            // lane 0: where the round left the output
            if (lane == 0u) {
                if (mode == kModeEmit) {
                    const uint32_t end_bit = ctrl[4] + total, nat = end_bit >> 3;
                    if (nat > E.out.end || (nat == E.out.end && (end_bit & 7u))) {
                        E.out.full = true;  // the ring took the bits; nothing at or beyond `end` is ever stored
                    } else {
                        E.out.at = nat;
                        E.nacc = end_bit & 7u;
                        E.acc = E.nacc ? (ring[nat & (kStageBytes - 1u)] & ((1u << E.nacc) - 1u)) : 0u;
                        if (!E.in_cmd && E.w.ip == E.mb_end) E.state = E.w.ip < E.n ? Encoder<Sink>::kBlock : Encoder<Sink>::kFinish;
                    }
                } else if (mode == kModeRaw) {
                    E.out.at += cnt;
                    E.raw_at += cnt;
                    if (E.raw_at == E.mb_end) {
                        E.w = E.w_end;  // the ring of distances keeps what it held
                        E.state = E.w.ip < E.n ? Encoder<Sink>::kBlock : Encoder<Sink>::kFinish;
                    }
                }
                ctrl[0] = E.out.at;
                ctrl[1] = (E.done ? 1u : 0u) | (E.out.full ? 2u : 0u);
            }
            __syncthreads();
            at = ctrl[0];
            fl = ctrl[1];
            // whole lines leave, and the rest with the last round; a byte that is not whole stays behind `at`
            const bool over = at - flushed >= kStageBytes;  // never: see Sink
            const uint32_t staged_end = over ? flushed + kStageBytes : at;
            const uint32_t to = fl || over ? staged_end : (staged_end & ~(kLine - 1u));
            if (to > flushed) {
                flush_ring<kStageBytes, true>(ring, origin, flushed, to, lane);
                flushed = over ? at : to;
            }
            if (lane == 0u) E.out.flushed = flushed;
            __syncthreads();
        }
        if (lane == 0u) seq_item_end(out_len, status, c, fl, at - lead, NX_ERR_BROTLI_ENCODE_FULL);
        __syncthreads();
    }
}

}  // namespace brotli

namespace {
// Stamps are 32 bits; at most 16 384 table slots (8 GiB) for a standalone call, a larger batch runs in sub-batches.
constexpr WsPairSpec kPair = {WsKind::BrotliEnc, 0xFFFFFFF0u, 16384};
constexpr WsSpec kSpec = kWsSpec[(int)WsKind::BrotliEnc];
static_assert(((size_t)kSpec.entry_bytes << kSpec.lg) == brotli::kSlotBytes, "brotli slot geometry");
}  // namespace

// nx_brotli_encode_batch with the handle's flags (alt_frames.hpp).
int32_t brotli_encode_items(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint8_t* out, const uint64_t* out_off,
                            uint32_t* out_len, int32_t* status, uint32_t n, int32_t lgwin, uint32_t flags, void* stream) {
    using namespace nx::brotli;
    NX_CLEAR_STALE_ERROR();
    if (lgwin == -1) lgwin = 22;
    if (lgwin < 10 || lgwin > 24) return NX_ERR_BROTLI_LGWIN;
    if (n == 0) return NX_OK;
    if (!in_off || !in_len || !out || !out_off || !out_len || !status) return NX_ERR_INVALID_ARG;
    const hipStream_t st = (hipStream_t)stream;
    WsAreaCut cut = {in_len, [](uint32_t len) { return area_bytes(seq_cap(len <= kMaxItem ? len : 0u)); }};
    // as many waves per CU as Work areas fit the 160 KiB of LDS, at most 8 (two per SIMD)
    const unsigned per_cu = std::min<unsigned>(8u, (160u << 10) / kLdsBytes);
    return ws_pair_launch(
        kPair, n, st, per_cu, &cut, true,
        [&](uint32_t base, uint32_t m, const LaneGrid& g, SharedWs& W, uint32_t stamp) {
            auto* k = g.spread ? k_seq_match<Match, true> : k_seq_match<Match, false>;
            hipLaunchKernelGGL(k, dim3(g.grid), dim3(g.block), 0, st, in, in_off + base, in_len + base, m, static_cast<uint8_t*>(W.p), stamp,
                               static_cast<uint8_t*>(W.side), cut.d_aoff(W) + base, (uint32_t)lgwin);
        },
        [&](uint32_t base, uint32_t m, unsigned waves, SharedWs& W) {
            hipLaunchKernelGGL(k_brotli_emit, dim3(waves), dim3(64), kLdsBytes, st, in, in_off + base, in_len + base, out, out_off + base,
                               out_len + base, status + base, m, static_cast<const uint8_t*>(W.side), cut.d_aoff(W) + base, (uint32_t)lgwin,
                               flags);
        });
}
}  // namespace nx

// One Brotli stream per item (netty_amd.h).
extern "C" int32_t nx_brotli_encode_batch(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint8_t* out,
                                          const uint64_t* out_off, uint32_t* out_len, int32_t* status, uint32_t n, int32_t lgwin,
                                          void* stream) {
    return nx::brotli_encode_items(in, in_off, in_len, out, out_off, out_len, status, n, lgwin, nx::brotli::kFlagHeader, stream);
}
