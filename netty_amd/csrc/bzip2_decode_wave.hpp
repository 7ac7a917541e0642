// bzip2_decode_wave.hpp — the wave-wide parts of the bzip2 decoder, shared by the kernel that decodes a stream
// on one wave (bzip2_decode.hip) and the kernels that decode a stream's blocks on a wave each
// (bzip2_decode_split.hip): the wave's LDS, the inverse BWT walk, the output tile flush with the CRC fold, and a
// block's two halves: block_front (stages 1-4 of bzip2_decode.hip's list, into the slot) and block_back
// (stage 5, from the slot to the output).  decode_block is the two in a row.
#pragma once
#include <hip/hip_runtime.h>
#include "workspace.hpp"
#include "bzip2_decode_core.hpp"

#ifndef NX_BZIP2_CHAINS_PER_LANE  // build option for A/B runs (scripts/build_lib_variant.sh)
#define NX_BZIP2_CHAINS_PER_LANE 8
#endif

namespace nx {
namespace bz2d {

#ifdef NX_BZIP2_SINGLE_CHAIN  // build option: the walk on one chain, lane 0 alone (the A/B baseline of the split)
constexpr uint32_t kChainsPerLane = 1;
constexpr uint32_t kChains = 1;
#else
constexpr uint32_t kChainsPerLane = NX_BZIP2_CHAINS_PER_LANE;
constexpr uint32_t kChains = 64u * kChainsPerLane;
#endif
static_assert(kChainsPerLane >= 1 && kChainsPerLane <= 16, "chain numbers fit the 16 bits under the flag, the arrays the LDS union");
constexpr uint32_t kTile = 1024;            // bytes per LDS tile (symbol decode, final stage)
constexpr uint32_t kFlag = 0x80000000u;     // above an entry's 28 bits: a chain starts here, its number below
constexpr uint32_t kNoOffset = 0xffffffffu;
// a slot: BWT bytes, merged pointers, the pre-RLE bytes of one block of up to 900 000
constexpr size_t kOffPtr = 900096, kOffPre = kOffPtr + 4u * (size_t)kMaxBlock;
static_assert(kOffPre + kMaxBlock <= kBzip2DecSlotBytes && kOffPtr % 64 == 0 && kOffPre % 64 == 0 && kMaxBlock % 4 == 0, "slot layout");

struct DecLds {
    uint8_t sel[kMaxSelectors + 2];
    uint8_t tile[kTile];  // the code lengths of the table being read, then the BWT tile
};
struct ChainLds {
    uint32_t orig[kChains];  // the entry a chain starts at
    uint32_t len[kChains];
    uint32_t off[kChains];
    uint16_t succ[kChains];
};
struct RleLds {
    uint32_t src[kTile / 4];
    uint8_t dst[kTile];
};
struct WaveLds {
    Block B;
    uint32_t crc_table[256];
    CrcShift shift;
    uint32_t base[256];
    Rle R;
    uint32_t mail[8];
    union {  // one per stage of a block
        DecLds dec;
        ChainLds ch;
        RleLds rle;
    };
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
__device__ __forceinline__ uint32_t load_own32(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Stage 4: pre[0, n) from the merged pointers tt[0, n) and the start pointer.
static __device__ void inverse_bwt(WaveLds& L, uint32_t* tt, uint32_t n, uint32_t start, uint8_t* pre, int lane) {
    const uint32_t C = n < kChains ? n : kChains;
    wave_sync();  // the decode stage's LDS has been read
    // chain c starts at floor(c n / C), the one whose range holds the start pointer at the start pointer
#pragma unroll
    for (uint32_t k = 0; k < kChainsPerLane; ++k) {
        const uint32_t c = (uint32_t)lane + 64u * k;
        if (c < C) {
            uint32_t s = (uint32_t)((uint64_t)c * n / C);
            const uint32_t s1 = c + 1u == C ? n : (uint32_t)((uint64_t)(c + 1u) * n / C);
            if (s <= start && start < s1) {
                s = start;
                L.mail[1] = c;
            }
            L.ch.orig[c] = load_own32(tt + s);
            L.ch.len[c] = s;  // until pass A: where the chain starts
            L.ch.off[c] = kNoOffset;
        }
    }
    wave_sync();
#pragma unroll
    for (uint32_t k = 0; k < kChainsPerLane; ++k) {
        const uint32_t c = (uint32_t)lane + 64u * k;
        if (c < C) tt[L.ch.len[c]] = kFlag | c;
    }
    own_stores_done();
    wave_sync();
    // pass A: every chain to the next flagged entry
    {
        uint32_t e[kChainsPerLane], ln[kChainsPerLane], live = 0;
#pragma unroll
        for (uint32_t k = 0; k < kChainsPerLane; ++k) {
            const uint32_t c = (uint32_t)lane + 64u * k;
            e[k] = c < C ? L.ch.orig[c] : 0u;
            ln[k] = 0;
            live |= c < C ? 1u << k : 0u;
        }
        for (uint32_t t = 0; live != 0u && t < n; ++t) {  // a chain is at most n long
            uint32_t v[kChainsPerLane];
#pragma unroll
            for (uint32_t k = 0; k < kChainsPerLane; ++k) v[k] = load_own32(tt + ((live >> k) & 1u ? (e[k] & kEntryMask) >> 8 : 0u));
#pragma unroll
            for (uint32_t k = 0; k < kChainsPerLane; ++k) {
                if (!((live >> k) & 1u)) continue;
                ln[k] += 1u;
                e[k] = v[k];
                if (v[k] & kFlag) {
                    const uint32_t c = (uint32_t)lane + 64u * k;
                    L.ch.len[c] = ln[k];
                    L.ch.succ[c] = (uint16_t)(v[k] & 0xffffu);
                    live &= ~(1u << k);
                }
            }
        }
    }
    wave_sync();
    // order: from the start pointer's chain along the successors until the cycle closes
    if (lane == 0) {
        const uint32_t first = L.mail[1];
        uint32_t cur = first, off = 0;
        for (uint32_t t = 0; t < C; ++t) {
            L.ch.off[cur] = off;
            off += L.ch.len[cur];
            cur = L.ch.succ[cur];
            if (cur == first) break;
        }
        L.mail[2] = off < n ? off : n;  // the cycle's length
    }
    wave_sync();
    const uint32_t period = uni(L.mail[2]);
    // pass B: the ordered chains' bytes at their offsets
    {
        uint32_t e[kChainsPerLane], o[kChainsPerLane], rem[kChainsPerLane], live = 0;
#pragma unroll
        for (uint32_t k = 0; k < kChainsPerLane; ++k) {
            const uint32_t c = (uint32_t)lane + 64u * k;
            const bool on = c < C && L.ch.off[c] != kNoOffset;
            e[k] = on ? L.ch.orig[c] : 0u;
            o[k] = on ? L.ch.off[c] : 0u;
            rem[k] = on ? L.ch.len[c] : 0u;
            if (on && rem[k] > period - o[k]) rem[k] = period - o[k];  // (offsets and lengths sum to the period: never taken)
            live |= rem[k] != 0u ? 1u << k : 0u;
        }
        while (live != 0u) {
            uint32_t v[kChainsPerLane];
#pragma unroll
            for (uint32_t k = 0; k < kChainsPerLane; ++k) {
                if ((live >> k) & 1u) pre[o[k]] = (uint8_t)e[k];
                v[k] = load_own32(tt + ((live >> k) & 1u ? (e[k] & kEntryMask) >> 8 : 0u));
            }
#pragma unroll
            for (uint32_t k = 0; k < kChainsPerLane; ++k) {
                if (!((live >> k) & 1u)) continue;
                e[k] = v[k];
                o[k] += 1u;
                if (--rem[k] == 0u) live &= ~(1u << k);
            }
        }
    }
    own_stores_done();
    if (period < n) {  // round the cycle again: byte i is byte i mod period
        for (uint32_t i = period + (uint32_t)lane; i < n; i += 64u) pre[i] = (uint8_t)load_own(pre + i % period);
        own_stores_done();
    }
}

// The output tile dst[0, cnt): checked against the room left, stored, folded into the block CRC.
static __device__ int32_t flush_out(WaveLds& L, uint8_t* out, uint32_t room, uint32_t cnt, uint32_t* crc, int lane) {
    if (cnt > room) return NX_ERR_BZIP2_OUTPUT_FULL;
    for (uint32_t k = (uint32_t)lane; k < cnt; k += 64u) out[k] = L.rle.dst[k];
    // the tile behind kTile - cnt zero bytes, sixteen bytes a lane: leading zeros leave a zero state alone
    const uint32_t pad = kTile - cnt;
    uint32_t c = 0;
#pragma unroll
    for (uint32_t t = 0; t < 16u; ++t) {
        const uint32_t v = 16u * (uint32_t)lane + t;
        if (v >= pad) c = crc_byte(L.crc_table, c, L.rle.dst[v - pad]);
    }
#pragma unroll
    for (uint32_t j = 0; j < 6u; ++j) {  // the lower half of a pair, shifted over the upper half's 16 * 2^j bytes
        const uint32_t other = (uint32_t)__shfl_xor((int)c, 1 << j);
        const bool is_lo = (((uint32_t)lane >> j) & 1u) == 0u;
        c = crc_mulmod(is_lo ? c : other, L.shift.x8[4u + j]) ^ (is_lo ? other : c);
    }
    *crc = crc_shift(L.shift, *crc, cnt) ^ uni(c);
    return NX_OK;
}

// Stages 1-4 of one block after its magic and CRC (L.B.crc, L.B.block_size set): *n_out pre-RLE bytes at
// slot + kOffPre.
__device__ __forceinline__ int32_t block_front(WaveLds& L, uint8_t* slot, uint32_t* n_out, int lane) {
    uint8_t* bwt = slot;
    uint32_t* tt = reinterpret_cast<uint32_t*>(slot + kOffPtr);
    uint8_t* pre = slot + kOffPre;
    // 1: headers and tables
    wave_sync();
    if (lane == 0) L.mail[0] = (uint32_t)block_tables(L.B, L.dec.sel, L.dec.tile);
    wave_sync();
    int32_t st = (int32_t)uni(L.mail[0]);
    if (st != NX_OK) return st;
    // 2: symbols into the slot's BWT bytes
    uint32_t n = 0;
    for (;;) {  // every tile takes a symbol of the input or ends the block
        wave_sync();
        if (lane == 0) {
            uint32_t cnt = 0, run_len = 0, run_byte = 0, done = 0;
            L.mail[0] = (uint32_t)sym_tile(L.B, L.dec.sel, L.dec.tile, kTile, &cnt, &run_len, &run_byte, &done);
            L.mail[1] = cnt;
            L.mail[2] = run_len;
            L.mail[3] = run_byte;
            L.mail[4] = done;
        }
        wave_sync();
        st = (int32_t)uni(L.mail[0]);
        if (st != NX_OK) return st;
        const uint32_t cnt = uni(L.mail[1]), run_len = uni(L.mail[2]), run_byte = uni(L.mail[3]);
        for (uint32_t k = (uint32_t)lane; k < cnt; k += 64u) bwt[n + k] = L.dec.tile[k];
        n += cnt;
        for (uint32_t k = (uint32_t)lane; k < run_len; k += 64u) bwt[n + k] = (uint8_t)run_byte;
        n += run_len;  // n = B.len, which the core keeps at or below the declared size
        if (uni(L.mail[4])) break;
    }
    const uint32_t start = uni(L.B.start);
    if (start >= n) return NX_ERR_BZIP2_START_POINTER;
    // 3: merged pointers
    if (lane == 0) {
        uint32_t sum = 0;
        for (uint32_t v = 0; v < 256u; ++v) {
            L.base[v] = sum;
            sum += L.B.counts[v];
        }
    }
    own_stores_done();
    wave_sync();
    {
        uint32_t next = (uint32_t)lane < n ? load_own(bwt + lane) : 0u;
        for (uint32_t i0 = 0; i0 < n; i0 += 64u) {
            const uint32_t i = i0 + (uint32_t)lane;
            const bool on = i < n;
            const uint32_t b = next;
            next = i + 64u < n ? load_own(bwt + i + 64u) : 0u;
            uint64_t same = __ballot(on);
#pragma unroll
            for (uint32_t bit = 0; bit < 8u; ++bit) {
                const bool one = (b >> bit) & 1u;
                const uint64_t ones = __ballot(on && one);
                same &= one ? ones : ~ones;
            }
            const uint32_t rank = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
            const uint32_t at = on ? L.base[b] : 0u;
            wave_sync();
            if (on && rank == 0u) L.base[b] = at + (uint32_t)__popcll(same);
            wave_sync();
            if (on) tt[at + rank] = (i << 8) | b;  // the counts are of these bytes: at + rank < n
        }
    }
    own_stores_done();
    // 4: the walk
    inverse_bwt(L, tt, n, start, pre, lane);
    *n_out = n;
    return NX_OK;
}

// Stage 5: the slot's n pre-RLE bytes through the final run-length stage: *produced bytes at out, room for
// `room`, their CRC held against `stored`.
__device__ __forceinline__ int32_t block_back(WaveLds& L, const uint8_t* pre, uint32_t n, uint32_t stored, uint8_t* out, uint32_t room,
                                              uint32_t* produced, int lane) {
    int32_t st = NX_OK;
    // 5: final run-length stage and CRC
    wave_sync();
    if (lane == 0) rle_init(L.R);
    uint32_t crc = 0xffffffffu, opos = 0, dcnt = 0;
    const uint32_t* pre32 = reinterpret_cast<const uint32_t*>(pre);
    for (uint32_t i0 = 0; i0 < n; i0 += kTile) {
        const uint32_t m = n - i0 < kTile ? n - i0 : kTile;
        wave_sync();
        for (uint32_t w = (uint32_t)lane; w < (m + 3u) / 4u; w += 64u) L.rle.src[w] = load_own32(pre32 + i0 / 4u + w);
        for (uint32_t used_all = 0; used_all < m;) {  // every step takes a byte of the tile or empties the output tile
            wave_sync();
            if (lane == 0) {
                uint32_t used = 0, cnt = 0, run_len = 0, run_byte = 0;
                rle_step(L.R, reinterpret_cast<const uint8_t*>(L.rle.src) + used_all, m - used_all, &used, L.rle.dst + dcnt, kTile - dcnt, &cnt,
                         &run_len, &run_byte);
                L.mail[0] = used;
                L.mail[1] = cnt;
                L.mail[2] = run_len;
                L.mail[3] = run_byte;
            }
            wave_sync();
            used_all += uni(L.mail[0]);
            dcnt += uni(L.mail[1]);
            const uint32_t run_len = uni(L.mail[2]), run_byte = uni(L.mail[3]);
            if (dcnt + run_len > kTile) {
                st = flush_out(L, out + opos, room - opos, dcnt, &crc, lane);
                if (st != NX_OK) return st;
                opos += dcnt;
                dcnt = 0;
                wave_sync();
            }
            for (uint32_t k = (uint32_t)lane; k < run_len; k += 64u) L.rle.dst[dcnt + k] = (uint8_t)run_byte;
            dcnt += run_len;
            if (dcnt == kTile) {
                wave_sync();
                st = flush_out(L, out + opos, room - opos, dcnt, &crc, lane);
                if (st != NX_OK) return st;
                opos += dcnt;
                dcnt = 0;
            }
        }
    }
    wave_sync();
    st = flush_out(L, out + opos, room - opos, dcnt, &crc, lane);
    if (st != NX_OK) return st;
    opos += dcnt;
    st = (int32_t)uni((uint32_t)rle_end(L.R));  // (lane 0's last rle_step lies before the wave_sync above)
    if (st != NX_OK) return st;
    if (~crc != stored) return NX_ERR_BZIP2_BLOCK_CRC;
    *produced = opos;
    return NX_OK;
}

// One block after its magic and CRC (L.B.crc, L.B.block_size set): *produced bytes at out, room for `room`.
__device__ __forceinline__ int32_t decode_block(WaveLds& L, uint8_t* slot, uint8_t* out, uint32_t room, uint32_t* produced, int lane) {
    uint32_t n = 0;
    const int32_t st = block_front(L, slot, &n, lane);
    if (st != NX_OK) return st;
    return block_back(L, slot + kOffPre, n, uni(L.B.crc), out, room, produced, lane);
}

}  // namespace bz2d
}  // namespace nx
