// brotli_decode_core.hpp — the format logic of the Brotli decoder (RFC 7932), written once for the host and
// the device: the stream header, meta-block headers, block types and counts, context modes and maps, simple
// and complex prefix codes, the insert-and-copy commands, the distance ring, static dictionary references and
// their 121 transforms.  Plain serial functions: no wave intrinsics, no LDS keywords.  The state of a stream
// (State) is small and comes in by reference (the kernel hands in LDS, the host a stack object); a meta-block's
// trees and context maps (Slot) come in as a pointer (the kernel hands in the stream's slot of the BrotliDec
// workspace, the host a heap block).  brotli_decode.hip runs these functions on lane 0 of a stream's wave and
// adds the wave-wide copies; brotli_decode_host.cpp runs them on the CPU, where the tests hold them against
// libbrotli.
//
// A stream is decoded by: begin (the stream header), then per meta-block metablock_header and, for a
// compressed one, step until Op::done, then finish after the ISLAST meta-block.  Everything between two
// meta-blocks lives in State (the ring, the last two bytes, the position, the bit reader), so a later handle
// can stop after a meta-block and go on from there.
//
// Trees are compact canonical tables: per tree the number of codes of each length 1..15 (cnt[1..15]; cnt[0] = 1
// marks the code of one symbol, which takes no bits) and the symbols sorted by code (by length, then value).
// A symbol is decoded bit by bit from a 15-bit peek, at most 15 steps.
//
// Nothing is assumed about the input.  The bit reader yields zeros past in_len and remembers it (br_over); it
// never loads outside [p, p + n).  Every error return is taken after the bits it depends on were consumed, and
// the callers turn any error into NX_ERR_BROTLI_TRUNCATED when the reader is past the end by then: libbrotli
// would have asked for more input before it reached that decision.  Every loop is bounded by a format constant,
// by MLEN or by the output capacity; the bound stands in a comment at the loop.  The checks and their order
// follow libbrotli 1.0.9 (decode.c), one status code per error of its decoder.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "../../include/netty_amd.h"

#ifndef NX_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define NX_HD __host__ __device__ inline
#else
#define NX_HD inline
#endif
#endif

namespace nx {
namespace brd {

constexpr uint32_t kMaxTrees = 256;      // NBLTYPES, NTREESL and NTREESD are at most 256
constexpr uint32_t kLitAlpha = 256;
constexpr uint32_t kCmdAlpha = 704;
constexpr uint32_t kDistAlphaMax = 16u + 120u + (48u << 3);  // 16 + NDIRECT + (48 << NPOSTFIX) at NPOSTFIX 3, NDIRECT 15 << 3
constexpr uint32_t kTypeAlphaMax = kMaxTrees + 2u;
constexpr uint32_t kCountAlpha = 26;
constexpr uint32_t kCmapAlphaMax = kMaxTrees + 16u;  // NTREES + RLEMAX
constexpr uint32_t kDictBytes = 122784;
constexpr uint32_t kTransforms = 121;
constexpr uint32_t kWordMax = 37;  // prefix (5) + word (24) + suffix (8)
constexpr uint32_t kWordBuf = 40;
constexpr uint32_t kMaxDistance = 0x7FFFFFFCu;  // libbrotli's BROTLI_MAX_ALLOWED_DISTANCE

template <uint32_t N>
struct Tree {
    uint16_t cnt[16];
    uint16_t sym[N];
};
// A meta-block's trees and maps: 256 x (544 + 1440 + 1072) + 3 x (548 + 84) + 576 + 16384 + 1024 = 802 216 bytes.
struct Slot {
    Tree<kLitAlpha> lit[kMaxTrees];
    Tree<kCmdAlpha> cmd[kMaxTrees];
    Tree<kDistAlphaMax> dist[kMaxTrees];
    Tree<kTypeAlphaMax> btype[3];
    Tree<kCountAlpha> bcount[3];
    Tree<kCmapAlphaMax> cmap_code;  // the code of the context map being read
    uint8_t cmap_l[kMaxTrees * 64];
    uint8_t cmap_d[kMaxTrees * 4];
};

struct BitReader {
    const uint8_t* p;
    uint32_t n;
    uint32_t cnt;  // bits in acc
    uint64_t at;   // bytes taken, the zero bytes past n included
    uint64_t acc;
};
NX_HD void br_init(BitReader& r, const uint8_t* p, uint32_t n) {
    r.p = p;
    r.n = n;
    r.cnt = 0;
    r.at = 0;
    r.acc = 0;
}
NX_HD void br_fill(BitReader& r) {
    while (r.cnt <= 56u) {  // at most 8 passes
        const uint64_t b = r.at < r.n ? r.p[r.at] : 0u;
        r.acc |= b << r.cnt;
        r.cnt += 8u;
        r.at += 1u;
    }
}
NX_HD uint32_t br_peek(BitReader& r, uint32_t k) {  // k <= 32
    br_fill(r);
    return (uint32_t)(r.acc & ((1ull << k) - 1ull));
}
NX_HD void br_drop(BitReader& r, uint32_t k) {
    r.acc >>= k;
    r.cnt -= k;
}
NX_HD uint32_t br_read(BitReader& r, uint32_t k) {
    const uint32_t v = br_peek(r, k);
    br_drop(r, k);
    return v;
}
NX_HD uint64_t br_bitpos(const BitReader& r) { return 8ull * r.at - r.cnt; }
NX_HD bool br_over(const BitReader& r) { return br_bitpos(r) > 8ull * r.n; }  // bits past the input were consumed

// What is being decoded.  Everything a later meta-block needs is here.
struct State {
    BitReader br;
    uint32_t wbits, max_backward;
    uint32_t ring_size;  // libbrotli's ring buffer for this meta-block (ring_update); it decides BLOCK_LENGTH_1 against _2
    uint32_t pos, cap;  // bytes produced, capacity
    uint32_t p1, p2;    // the last two bytes produced (0 before there are any)
    int32_t ring[4];
    uint32_t ring_idx;
    // the meta-block
    uint32_t is_last, mlen;  // mlen: bytes the meta-block has yet to produce
    uint32_t nbl[3], bl_len[3], bl_type[3], bl_rb[3][2];
    uint32_t npostfix, ndirect, dist_alpha, ntrees_l, ntrees_d;
    // the command
    uint32_t in_cmd, insert_left, copy_len, implicit;
    // scratch of the tree builds
    uint16_t off[16];
    uint16_t cl_cnt[16], cl_sym[18];
    uint32_t s4[4];
    uint8_t cl[18];
    uint8_t ctx_mode[kMaxTrees];
    uint8_t mtf[256];
    uint8_t lens[kCmdAlpha];
};

enum : uint32_t { kMbCompressed = 0, kMbUncompressed = 1, kMbNothing = 2 };
struct MbHead {
    uint32_t kind;
    uint32_t src;  // uncompressed: the bytes are in[src, src + len), and go to out[pos, pos + len)
    uint32_t len;
    uint32_t pos;
};
// One step's work for the copier, in this order: stage[0, n_lit) to out[pos ..), then copy_len bytes from
// `dist` back (an overlapping copy repeats its first dist bytes), then word[0, word_len).  After a copy the
// copier stores its last two bytes in State::p1 (the last) and p2.
struct Op {
    uint32_t pos, n_lit, copy_len, dist, word_len, done;
    uint8_t word[kWordBuf];
};

// libbrotli keeps its output in a ring buffer that it sizes at every meta-block with data
// (BrotliCalculateRingBufferSize): the window once reached, else the window halved while the half still holds
// what is there plus MLEN, and 1024 bytes or its earlier size at least.  The decoder here has no such buffer, but
// which of libbrotli's two codes an over-run gets depends on it (overrun_code).  At most 14 halvings.
NX_HD uint32_t ring_position(const State& S, uint32_t pos) { return S.ring_size == (1u << S.wbits) ? (pos & (S.ring_size - 1u)) : pos; }
NX_HD void ring_update(State& S, uint32_t mlen) {
    const uint32_t window = 1u << S.wbits;
    if (S.ring_size == window) return;
    const uint64_t need = (uint64_t)S.pos + mlen;  // (below the window the ring position is the position)
    const uint64_t floor = S.ring_size ? S.ring_size : 1024u;
    const uint64_t min_size = need > floor ? need : floor;
    uint32_t size = window;
    while ((size >> 1) >= min_size) size >>= 1;  // min_size >= 1024: at most 14 passes from a window of 2^24
    S.ring_size = size;
}
// A command's n bytes at position pos pass the end of the meta-block.  libbrotli writes them all the same and finds
// the over-run either when they reach the end of its ring buffer, which it then writes out (BLOCK_LENGTH_1), or
// when the meta-block is done (BLOCK_LENGTH_2).
NX_HD int32_t overrun_code(const State& S, uint32_t pos, uint32_t n) {
    return (uint64_t)ring_position(S, pos) + n >= S.ring_size ? NX_ERR_BROTLI_BLOCK_LENGTH_1 : NX_ERR_BROTLI_BLOCK_LENGTH_2;
}

NX_HD uint32_t bit_width(uint32_t v) { return v ? 32u - (uint32_t)__builtin_clz(v) : 0u; }

// lens[0, n) -> the canonical table.  Two passes of n.
NX_HD void build_tree(State& S, uint16_t* cnt, uint16_t* sym, const uint8_t* lens, uint32_t n) {
    for (uint32_t l = 0; l < 16u; ++l) cnt[l] = 0;          // 16: the code lengths 0..15
    for (uint32_t i = 0; i < n; ++i) cnt[lens[i]] += 1u;    // n: the alphabet, at most 704
    const uint32_t nz = n - cnt[0];
    uint32_t o = 0;
    for (uint32_t l = 1; l < 16u; ++l) {  // 15 lengths
        S.off[l] = (uint16_t)o;
        o += cnt[l];
    }
    for (uint32_t i = 0; i < n; ++i)  // n: the alphabet again
        if (lens[i]) sym[S.off[lens[i]]++] = (uint16_t)i;
    cnt[0] = nz == 1u ? 1u : 0u;
}

// One symbol: at most 15 steps.  A complete code always resolves; an incomplete one cannot be built.
NX_HD uint32_t read_symbol(BitReader& r, const uint16_t* cnt, const uint16_t* sym) {
    if (cnt[0]) return sym[0];
    uint32_t bits = br_peek(r, 15);
    uint32_t code = 0, first = 0, index = 0;
    for (uint32_t len = 1; len < 16u; ++len) {  // 15: the longest code
        code |= bits & 1u;
        bits >>= 1;
        const uint32_t c = cnt[len];
        if (code < first + c) {
            br_drop(r, len);
            return sym[index + (code - first)];
        }
        index += c;
        first = (first + c) << 1;
        code <<= 1;
    }
    br_drop(r, 15);
    return sym[0];
}

NX_HD uint32_t read_varlen8(BitReader& r) {  // 0..255
    if (!br_read(r, 1)) return 0;
    const uint32_t n = br_read(r, 3);
    return n ? (1u << n) + br_read(r, n) : 1u;
}

// A prefix code over `alpha` symbols (RFC 7932 section 3.4 and 3.5) into (cnt, sym).
NX_HD int32_t read_prefix_code(State& S, nx_brotli_decode_stats* st, uint32_t alpha, uint16_t* cnt, uint16_t* sym) {
    BitReader& r = S.br;
    uint8_t* lens = S.lens;
    for (uint32_t i = 0; i < alpha; ++i) lens[i] = 0;  // alpha <= 704
    const uint32_t h = br_read(r, 2);
    if (h == 1u) {  // simple
        const uint32_t max_bits = bit_width(alpha - 1u);
        const uint32_t nsym = br_read(r, 2) + 1u;
        for (uint32_t i = 0; i < nsym; ++i) {  // NSYM <= 4
            S.s4[i] = br_read(r, max_bits);
            if (S.s4[i] >= alpha) return NX_ERR_BROTLI_SIMPLE_HUFFMAN_ALPHABET;
        }
        for (uint32_t i = 0; i + 1u < nsym; ++i)  // at most six pairs of four symbols
            for (uint32_t k = i + 1u; k < nsym; ++k)
                if (S.s4[i] == S.s4[k]) return NX_ERR_BROTLI_SIMPLE_HUFFMAN_SAME;
        const uint32_t shape = nsym == 4u ? br_read(r, 1) : 0u;
        if (nsym == 1u) {
            lens[S.s4[0]] = 1;  // the only symbol: no bits (build_tree marks it)
        } else if (nsym == 2u) {
            lens[S.s4[0]] = lens[S.s4[1]] = 1;
        } else if (nsym == 3u) {
            lens[S.s4[0]] = 1;
            lens[S.s4[1]] = lens[S.s4[2]] = 2;
        } else if (!shape) {
            lens[S.s4[0]] = lens[S.s4[1]] = lens[S.s4[2]] = lens[S.s4[3]] = 2;
        } else {
            lens[S.s4[0]] = 1;
            lens[S.s4[1]] = 2;
            lens[S.s4[2]] = lens[S.s4[3]] = 3;
        }
        if (st) st->simple_codes[nsym - 1u] += 1u;
        if (st && nsym == 4u) st->simple_four_shapes |= 1u << shape;
    } else {  // complex: h is HSKIP
        static constexpr uint8_t kOrder[18] = {1, 2, 3, 4, 0, 5, 17, 6, 16, 7, 8, 9, 10, 11, 12, 13, 14, 15};
        static constexpr uint8_t kLen[16] = {2, 2, 2, 3, 2, 2, 2, 4, 2, 2, 2, 3, 2, 2, 2, 4};
        static constexpr uint8_t kVal[16] = {0, 4, 3, 2, 0, 4, 3, 1, 0, 4, 3, 2, 0, 4, 3, 5};
        for (uint32_t i = 0; i < 18u; ++i) S.cl[i] = 0;  // 18: the code-length alphabet
        uint32_t space = 32, num = 0;
        for (uint32_t i = h; i < 18u; ++i) {  // at most 18 code-length code lengths
            const uint32_t ix = br_peek(r, 4);
            const uint32_t v = kVal[ix];
            br_drop(r, kLen[ix]);
            S.cl[kOrder[i]] = (uint8_t)v;
            if (v) {
                space -= 32u >> v;
                num += 1u;
                if (space - 1u >= 32u) break;  // used up, or wrapped: over-subscribed
            }
        }
        if (!(num == 1u || space == 0u)) return NX_ERR_BROTLI_CL_SPACE;
        build_tree(S, S.cl_cnt, S.cl_sym, S.cl, 18);
        uint32_t symbol = 0, repeat = 0, prev = 8, rep_len = 0;
        space = 32768;
        while (symbol < alpha && space > 0u) {  // every pass advances symbol by one at least
            const uint32_t c = read_symbol(r, S.cl_cnt, S.cl_sym);
            if (c < 16u) {
                repeat = 0;
                if (c) {
                    lens[symbol] = (uint8_t)c;
                    prev = c;
                    space -= 32768u >> c;
                }
                symbol += 1u;
            } else {
                const uint32_t eb = c == 16u ? 2u : 3u;
                const uint32_t new_len = c == 16u ? prev : 0u;
                const uint32_t delta = br_read(r, eb);
                if (rep_len != new_len) {
                    repeat = 0;
                    rep_len = new_len;
                }
                const uint32_t old = repeat;
                if (repeat > 0u) repeat = (repeat - 2u) << eb;
                repeat += delta + 3u;
                const uint32_t d = repeat - old;
                if (st) (c == 16u ? st->repeat_16 : st->repeat_17) += 1u;
                if (symbol + d > alpha) {
                    space = 0xFFFFFu;
                    break;
                }
                if (rep_len) {
                    for (uint32_t k = 0; k < d; ++k) lens[symbol + k] = (uint8_t)rep_len;  // d <= alpha - symbol
                    space -= d << (15u - rep_len);
                }
                symbol += d;
            }
        }
        if (space != 0u) return NX_ERR_BROTLI_HUFFMAN_SPACE;
        if (st) st->complex_codes += 1u;
    }
    build_tree(S, cnt, sym, lens, alpha);
    return NX_OK;
}

NX_HD uint32_t read_block_length(BitReader& r, const Tree<kCountAlpha>& T) {
    static constexpr uint16_t kBase[26] = {1,  5,  9,  13,  17,  25,  33,  41,  49,   65,   81,   97,   113,
                                           145, 177, 209, 241, 305, 369, 497, 753, 1265, 2289, 4337, 8433, 16625};
    static constexpr uint8_t kBits[26] = {2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 6, 6, 7, 8, 9, 10, 11, 12, 13, 24};
    const uint32_t c = read_symbol(r, T.cnt, T.sym);
    return kBase[c] + br_read(r, kBits[c]);
}

// The block of category k is used up: the next type and its count.
NX_HD void block_switch(State& S, Slot* W, uint32_t k) {
    if (S.nbl[k] < 2u) {  // one type: its count is never read
        S.bl_len[k] = 1u << 24;
        return;
    }
    uint32_t t = read_symbol(S.br, W->btype[k].cnt, W->btype[k].sym);
    S.bl_len[k] = read_block_length(S.br, W->bcount[k]);
    if (t == 1u) t = S.bl_rb[k][1] + 1u;
    else if (t == 0u) t = S.bl_rb[k][0];
    else t -= 2u;
    if (t >= S.nbl[k]) t -= S.nbl[k];
    S.bl_rb[k][0] = S.bl_rb[k][1];
    S.bl_rb[k][1] = t;
    S.bl_type[k] = t;
}

// A context map of `size` entries (RFC 7932 section 7.3).
NX_HD int32_t read_context_map(State& S, Slot* W, nx_brotli_decode_stats* st, uint8_t* map, uint32_t size, uint32_t* ntrees) {
    BitReader& r = S.br;
    const uint32_t nt = read_varlen8(r) + 1u;
    *ntrees = nt;
    if (nt < 2u) {
        for (uint32_t i = 0; i < size; ++i) map[i] = 0;  // size <= 16384
        return NX_OK;
    }
    const uint32_t rlemax = br_read(r, 1) ? br_read(r, 4) + 1u : 0u;
    const int32_t e = read_prefix_code(S, st, nt + rlemax, W->cmap_code.cnt, W->cmap_code.sym);
    if (e != NX_OK) return e;
    for (uint32_t i = 0; i < size;) {  // every pass fills one entry at least
        const uint32_t c = read_symbol(r, W->cmap_code.cnt, W->cmap_code.sym);
        if (c == 0u) {
            map[i++] = 0;
        } else if (c > rlemax) {
            map[i++] = (uint8_t)(c - rlemax);
        } else {
            const uint32_t reps = (1u << c) + br_read(r, c);
            if (i + reps > size) return NX_ERR_BROTLI_CONTEXT_MAP_REPEAT;
            for (uint32_t k = 0; k < reps; ++k) map[i + k] = 0;  // reps <= size - i
            i += reps;
            if (st) st->cmap_rle_runs += 1u;
        }
    }
    if (br_read(r, 1)) {  // inverse move-to-front: size passes of at most 255 moves
        for (uint32_t i = 0; i < 256u; ++i) S.mtf[i] = (uint8_t)i;  // 256 tree indices
        for (uint32_t i = 0; i < size; ++i) {
            const uint32_t ix = map[i];
            const uint8_t v = S.mtf[ix];
            map[i] = v;
            for (uint32_t k = ix; k > 0u; --k) S.mtf[k] = S.mtf[k - 1u];
            S.mtf[0] = v;
        }
        if (st) st->cmap_imtf += 1u;
    }
    return NX_OK;
}

// The stream header: WBITS.
NX_HD int32_t begin(State& S, const uint8_t* in, uint32_t n, uint32_t cap) {
    br_init(S.br, in, n);
    S.pos = 0;
    S.cap = cap;
    S.p1 = S.p2 = 0;
    S.ring[0] = 16;
    S.ring[1] = 15;
    S.ring[2] = 11;
    S.ring[3] = 4;
    S.ring_idx = 0;
    S.ring_size = 0;
    S.is_last = 0;
    S.mlen = 0;
    S.in_cmd = 0;
    S.insert_left = 0;
    BitReader& r = S.br;
    uint32_t w = 16;
    if (br_read(r, 1)) {
        uint32_t v = br_read(r, 3);
        if (v) {
            w = 17u + v;
        } else {
            v = br_read(r, 3);
            if (v == 1u) return NX_ERR_BROTLI_WINDOW_BITS;  // 0010001: the large-window escape
            w = v ? 8u + v : 17u;
        }
    }
    S.wbits = w;
    S.max_backward = (1u << w) - 16u;
    return NX_OK;
}

// The next meta-block's header; for a compressed one all of its trees and maps, into *W.
NX_HD int32_t metablock_header(State& S, Slot* W, nx_brotli_decode_stats* st, MbHead* H) {
    BitReader& r = S.br;
    H->kind = kMbNothing;
    H->src = H->len = 0;
    H->pos = S.pos;
    S.is_last = br_read(r, 1);
    if (S.is_last && br_read(r, 1)) {  // ISLASTEMPTY
        if (st) st->mb_empty_last += 1u;
        return NX_OK;
    }
    const uint32_t mn = br_read(r, 2);
    if (mn == 3u) {  // metadata
        if (br_read(r, 1)) return NX_ERR_BROTLI_RESERVED;
        const uint32_t nb = br_read(r, 2);
        uint32_t skip = 0;
        for (uint32_t i = 0; i < nb; ++i) {  // MSKIPBYTES <= 3
            const uint32_t b = br_read(r, 8);
            if (i + 1u == nb && nb > 1u && b == 0u) return NX_ERR_BROTLI_EXUBERANT_META_NIBBLE;
            skip |= b << (8u * i);
        }
        if (nb) skip += 1u;
        if (br_read(r, (uint32_t)((8u - (br_bitpos(r) & 7u)) & 7u))) return NX_ERR_BROTLI_PADDING_1;
        if (br_over(r)) return NX_ERR_BROTLI_TRUNCATED;
        const uint64_t at = br_bitpos(r) >> 3;
        if (skip > r.n - at) return NX_ERR_BROTLI_TRUNCATED;
        br_init(r, r.p, r.n);  // go on behind the skipped bytes
        r.at = at + skip;
        if (st) st->mb_metadata += 1u;
        if (st && skip) st->metadata_skipped += skip;
        return NX_OK;
    }
    const uint32_t nn = mn + 4u;
    uint32_t mlen = 0;
    for (uint32_t i = 0; i < nn; ++i) {  // MNIBBLES: 4, 5 or 6
        const uint32_t b = br_read(r, 4);
        if (i + 1u == nn && nn > 4u && b == 0u) return NX_ERR_BROTLI_EXUBERANT_NIBBLE;
        mlen |= b << (4u * i);
    }
    mlen += 1u;
    ring_update(S, mlen);
    if (!S.is_last && br_read(r, 1)) {  // ISUNCOMPRESSED
        if (br_read(r, (uint32_t)((8u - (br_bitpos(r) & 7u)) & 7u))) return NX_ERR_BROTLI_PADDING_1;
        if (br_over(r)) return NX_ERR_BROTLI_TRUNCATED;
        const uint64_t at = br_bitpos(r) >> 3;
        if (mlen > S.cap - S.pos) return NX_ERR_BROTLI_OUTPUT_FULL;
        if (mlen > r.n - at) return NX_ERR_BROTLI_TRUNCATED;
        H->kind = kMbUncompressed;
        H->src = (uint32_t)at;
        H->len = mlen;
        S.p2 = mlen > 1u ? r.p[at + mlen - 2u] : S.p1;
        S.p1 = r.p[at + mlen - 1u];
        S.pos += mlen;
        br_init(r, r.p, r.n);
        r.at = at + mlen;
        if (st) st->mb_uncompressed += 1u;
        return NX_OK;
    }
    H->kind = kMbCompressed;
    H->len = mlen;
    S.mlen = mlen;
    S.in_cmd = 0;
    S.insert_left = 0;
    for (uint32_t k = 0; k < 3u; ++k) {  // the three categories
        S.nbl[k] = read_varlen8(r) + 1u;
        S.bl_type[k] = 0;
        S.bl_rb[k][0] = 1;
        S.bl_rb[k][1] = 0;
        S.bl_len[k] = 1u << 24;
        if (S.nbl[k] >= 2u) {
            int32_t e = read_prefix_code(S, st, S.nbl[k] + 2u, W->btype[k].cnt, W->btype[k].sym);
            if (e != NX_OK) return e;
            e = read_prefix_code(S, st, kCountAlpha, W->bcount[k].cnt, W->bcount[k].sym);
            if (e != NX_OK) return e;
            S.bl_len[k] = read_block_length(r, W->bcount[k]);
        }
        if (st && S.nbl[k] > st->max_nbltypes[k]) st->max_nbltypes[k] = S.nbl[k];
    }
    S.npostfix = br_read(r, 2);
    S.ndirect = br_read(r, 4) << S.npostfix;
    S.dist_alpha = 16u + S.ndirect + (48u << S.npostfix);
    for (uint32_t i = 0; i < S.nbl[0]; ++i) {  // at most 256
        S.ctx_mode[i] = (uint8_t)br_read(r, 2);
        if (st) st->context_modes |= 1u << S.ctx_mode[i];
    }
    int32_t e = read_context_map(S, W, st, W->cmap_l, S.nbl[0] * 64u, &S.ntrees_l);
    if (e != NX_OK) return e;
    e = read_context_map(S, W, st, W->cmap_d, S.nbl[2] * 4u, &S.ntrees_d);
    if (e != NX_OK) return e;
    for (uint32_t i = 0; i < S.ntrees_l; ++i) {  // at most 256
        e = read_prefix_code(S, st, kLitAlpha, W->lit[i].cnt, W->lit[i].sym);
        if (e != NX_OK) return e;
    }
    for (uint32_t i = 0; i < S.nbl[1]; ++i) {  // at most 256
        e = read_prefix_code(S, st, kCmdAlpha, W->cmd[i].cnt, W->cmd[i].sym);
        if (e != NX_OK) return e;
    }
    for (uint32_t i = 0; i < S.ntrees_d; ++i) {  // at most 256
        e = read_prefix_code(S, st, S.dist_alpha, W->dist[i].cnt, W->dist[i].sym);
        if (e != NX_OK) return e;
    }
    if (br_over(r)) return NX_ERR_BROTLI_TRUNCATED;
    if (st) {
        st->mb_compressed += 1u;
        if (S.ntrees_l > st->max_ntrees_l) st->max_ntrees_l = S.ntrees_l;
        if (S.ntrees_d > st->max_ntrees_d) st->max_ntrees_d = S.ntrees_d;
        if (S.npostfix > st->max_npostfix) st->max_npostfix = S.npostfix;
        if (S.ndirect > st->max_ndirect) st->max_ndirect = S.ndirect;
    }
    return NX_OK;
}

// The literal context of RFC 7932 section 7.1 from the last byte p1 and the one before it.
NX_HD uint32_t signed_lut(uint32_t b) { return b == 0u ? 0u : b < 16u ? 1u : b < 64u ? 2u : b < 128u ? 3u : b < 192u ? 4u : b < 240u ? 5u : b < 255u ? 6u : 7u; }
NX_HD uint32_t utf8_lut0(uint32_t b) {
    static constexpr uint8_t k[128] = {
        0,  0,  0,  0,  0,  0,  0,  0,  0,  4,  4,  0,  0,  4,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,
        8,  12, 16, 12, 12, 20, 12, 16, 24, 28, 12, 12, 32, 12, 36, 12, 44, 44, 44, 44, 44, 44, 44, 44, 44, 44, 32, 32, 24, 40, 28, 12,
        12, 48, 52, 52, 52, 48, 52, 52, 52, 48, 52, 52, 52, 52, 52, 48, 52, 52, 52, 52, 52, 48, 52, 52, 52, 52, 52, 24, 12, 28, 12, 12,
        12, 56, 60, 60, 60, 56, 60, 60, 60, 56, 60, 60, 60, 60, 60, 56, 60, 60, 60, 60, 60, 56, 60, 60, 60, 60, 60, 24, 12, 28, 12, 0};
    return b < 128u ? k[b] : b < 192u ? (b & 1u) : 2u + (b & 1u);
}
NX_HD uint32_t utf8_lut1(uint32_t b) {
    if (b < 128u) {
        if (b < 32u || b == 127u || b == 32u) return 0;
        if (b >= 48u && b < 58u) return 2;
        if (b >= 65u && b < 91u) return 2;
        if (b >= 97u && b < 123u) return 3;
        return 1;
    }
    return b < 224u ? 0u : 2u;
}
NX_HD uint32_t literal_context(uint32_t mode, uint32_t p1, uint32_t p2) {
    return mode == 0u ? (p1 & 63u) : mode == 1u ? (p1 >> 2) : mode == 2u ? (utf8_lut0(p1) | utf8_lut1(p2)) : ((signed_lut(p1) << 3) | signed_lut(p2));
}

// The static dictionary's geometry (RFC 7932 section 8): NDBITS and the offsets of the words of each length.
NX_HD uint32_t dict_bits(uint32_t len) {
    static constexpr uint8_t k[25] = {0, 0, 0, 0, 10, 10, 11, 11, 10, 10, 10, 10, 10, 9, 9, 8, 7, 7, 8, 7, 7, 6, 6, 5, 5};
    return k[len];
}
NX_HD uint32_t dict_offset(uint32_t len) {
    static constexpr uint32_t k[25] = {0,     0,     0,     0,     0,     4096,   9216,   21504,  35840,  44032,  53248,  63488, 74752,
                                       87040, 93696, 100864, 104704, 106752, 108928, 113536, 115968, 118528, 119872, 121280, 122016};
    return k[len];
}

// RFC 7932 Appendix B.  type: 0 identity, 1..9 omit the last 1..9, 10 uppercase the first, 11 uppercase all,
// 12..20 omit the first 1..9.
struct Transform {
    char pre[6];
    uint8_t type;
    char suf[9];
};
NX_HD uint32_t to_upper(uint8_t* p) {
    if (p[0] < 0xC0u) {
        if (p[0] >= 'a' && p[0] <= 'z') p[0] ^= 32u;
        return 1;
    }
    if (p[0] < 0xE0u) {
        p[1] ^= 32u;
        return 2;
    }
    p[2] ^= 5u;
    return 3;
}
// word[0, len) under transform t (below 121) into out (kWordBuf bytes); the result's length, at most kWordMax.
NX_HD uint32_t transform_word(uint32_t t, const uint8_t* word, uint32_t len, uint8_t* out) {
    static constexpr Transform kT[kTransforms] = {
        {"", 0, ""}, {"", 0, " "}, {" ", 0, " "}, {"", 12, ""}, {"", 10, " "}, {"", 0, " the "}, {" ", 0, ""}, {"s ", 0, " "},
        {"", 0, " of "}, {"", 10, ""}, {"", 0, " and "}, {"", 13, ""}, {"", 1, ""}, {", ", 0, " "}, {"", 0, ", "}, {" ", 10, " "},
        {"", 0, " in "}, {"", 0, " to "}, {"e ", 0, " "}, {"", 0, "\""}, {"", 0, "."}, {"", 0, "\">"}, {"", 0, "\n"}, {"", 3, ""},
        {"", 0, "]"}, {"", 0, " for "}, {"", 14, ""}, {"", 2, ""}, {"", 0, " a "}, {"", 0, " that "}, {" ", 10, ""}, {"", 0, ". "},
        {".", 0, ""}, {" ", 0, ", "}, {"", 15, ""}, {"", 0, " with "}, {"", 0, "'"}, {"", 0, " from "}, {"", 0, " by "}, {"", 16, ""},
        {"", 17, ""}, {" the ", 0, ""}, {"", 4, ""}, {"", 0, ". The "}, {"", 11, ""}, {"", 0, " on "}, {"", 0, " as "}, {"", 0, " is "},
        {"", 7, ""}, {"", 1, "ing "}, {"", 0, "\n\t"}, {"", 0, ":"}, {" ", 0, ". "}, {"", 0, "ed "}, {"", 20, ""}, {"", 18, ""},
        {"", 6, ""}, {"", 0, "("}, {"", 10, ", "}, {"", 8, ""}, {"", 0, " at "}, {"", 0, "ly "}, {" the ", 0, " of "}, {"", 5, ""},
        {"", 9, ""}, {" ", 10, ", "}, {"", 10, "\""}, {".", 0, "("}, {"", 11, " "}, {"", 10, "\">"}, {"", 0, "=\""}, {" ", 0, "."},
        {".com/", 0, ""}, {" the ", 0, " of the "}, {"", 10, "'"}, {"", 0, ". This "}, {"", 0, ","}, {".", 0, " "}, {"", 10, "("},
        {"", 10, "."}, {"", 0, " not "}, {" ", 0, "=\""}, {"", 0, "er "}, {" ", 11, " "}, {"", 0, "al "}, {" ", 11, ""}, {"", 0, "='"},
        {"", 11, "\""}, {"", 10, ". "}, {" ", 0, "("}, {"", 0, "ful "}, {" ", 10, ". "}, {"", 0, "ive "}, {"", 0, "less "},
        {"", 11, "'"}, {"", 0, "est "}, {" ", 10, "."}, {"", 11, "\">"}, {" ", 0, "='"}, {"", 10, ","}, {"", 0, "ize "}, {"", 11, "."},
        {"\302\240", 0, ""}, {" ", 0, ","}, {"", 10, "=\""}, {"", 11, "=\""}, {"", 0, "ous "}, {"", 11, ", "}, {"", 10, "='"},
        {" ", 10, ","}, {" ", 11, "=\""}, {" ", 11, ", "}, {"", 11, ","}, {"", 11, "("}, {"", 11, ". "}, {" ", 11, "."}, {"", 11, "='"},
        {" ", 11, ". "}, {" ", 10, "=\""}, {" ", 11, "='"}, {" ", 10, "='"}};
    const Transform& T = kT[t];
    uint32_t idx = 0;
    // prefix: at most 5 bytes; suffix below: at most 8
    for (uint32_t i = 0; i < 5u && T.pre[i]; ++i) out[idx++] = (uint8_t)T.pre[i];
    const uint32_t type = T.type;
    uint32_t from = 0, n = len;
    if (type >= 1u && type <= 9u) {
        n = len > type ? len - type : 0u;
    } else if (type >= 12u) {
        from = type - 11u;
        if (from > len) from = len;
        n = len - from;
    }
    for (uint32_t i = 0; i < n; ++i) out[idx++] = word[from + i];  // n <= 24
    if (type == 10u) {
        to_upper(out + idx - n);  // (a type 10 or 11 keeps the whole word: n = len >= 4)
    } else if (type == 11u) {
        uint32_t at = idx - n, left = n;
        while (left > 0u) {  // every pass takes 1..3 bytes of the word
            const uint32_t step = to_upper(out + at);
            at += step;
            left = left > step ? left - step : 0u;
        }
    }
    for (uint32_t i = 0; i < 8u && T.suf[i]; ++i) out[idx++] = (uint8_t)T.suf[i];
    return idx;
}

// One step of a compressed meta-block: the next command's insert-and-copy lengths if none is open, up to
// stage_cap of its literals into stage, and, once its literals are through, its distance.  *op says what to copy
// (on an error nothing).  Bounded: at most stage_cap literals, each a symbol of at most 15 steps.
NX_HD int32_t step(State& S, Slot* W, const uint8_t* dict, nx_brotli_decode_stats* st, uint8_t* stage, uint32_t stage_cap, Op* op) {
    BitReader& r = S.br;
    op->pos = S.pos;
    op->n_lit = op->copy_len = op->dist = op->word_len = op->done = 0;
    const uint64_t b0 = br_bitpos(r);
    if (!S.in_cmd) {
        static constexpr uint8_t kInsCell[11] = {0, 0, 0, 0, 8, 8, 0, 16, 8, 16, 16};
        static constexpr uint8_t kCopyCell[11] = {0, 8, 0, 8, 0, 8, 16, 0, 16, 8, 16};
        static constexpr uint16_t kInsBase[24] = {0, 1, 2, 3, 4, 5, 6, 8, 10, 14, 18, 26, 34, 50, 66, 98, 130, 194, 322, 578, 1090, 2114, 6210, 22594};
        static constexpr uint8_t kInsBits[24] = {0, 0, 0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 7, 8, 9, 10, 12, 14, 24};
        static constexpr uint16_t kCopyBase[24] = {2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 14, 18, 22, 30, 38, 54, 70, 102, 134, 198, 326, 582, 1094, 2118};
        static constexpr uint8_t kCopyBits[24] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 7, 8, 9, 10, 24};
        if (S.bl_len[1] == 0u) block_switch(S, W, 1);
        S.bl_len[1] -= 1u;
        const Tree<kCmdAlpha>& T = W->cmd[S.bl_type[1]];
        const uint32_t c = read_symbol(r, T.cnt, T.sym);
        const uint32_t cell = c >> 6;
        const uint32_t ic = kInsCell[cell] + ((c >> 3) & 7u), cc = kCopyCell[cell] + (c & 7u);
        const uint32_t ins = kInsBase[ic] + br_read(r, kInsBits[ic]);
        const uint32_t cpy = kCopyBase[cc] + br_read(r, kCopyBits[cc]);
        if (br_over(r)) return NX_ERR_BROTLI_TRUNCATED;
        if (ins > S.mlen) return overrun_code(S, S.pos, ins);
        S.in_cmd = 1;
        S.insert_left = ins;
        S.copy_len = cpy;
        S.implicit = c < 128u ? 1u : 0u;
    }
    uint32_t n = S.insert_left < stage_cap ? S.insert_left : stage_cap;
    if (n > S.cap - S.pos) return NX_ERR_BROTLI_OUTPUT_FULL;
    uint32_t p1 = S.p1, p2 = S.p2;
    for (uint32_t i = 0; i < n; ++i) {  // n <= stage_cap, and n <= MLEN's rest
        if (S.bl_len[0] == 0u) block_switch(S, W, 0);
        S.bl_len[0] -= 1u;
        const uint32_t bt = S.bl_type[0];
        const Tree<kLitAlpha>& T = W->lit[W->cmap_l[bt * 64u + literal_context(S.ctx_mode[bt], p1, p2)]];
        p2 = p1;
        p1 = read_symbol(r, T.cnt, T.sym);
        stage[i] = (uint8_t)p1;
    }
    if (br_over(r)) return NX_ERR_BROTLI_TRUNCATED;
    if (n < S.insert_left) {  // the rest of the literals in the next step
        S.insert_left -= n;
        S.mlen -= n;
        S.pos += n;
        S.p1 = p1;
        S.p2 = p2;
        op->n_lit = n;
        return NX_OK;
    }
    const uint32_t pos = S.pos + n, mlen = S.mlen - n;
    uint32_t out_n = 0;
    if (mlen != 0u) {  // the copy (a meta-block may end after a command's literals)
        int64_t d;
        bool push = true;
        if (S.implicit) {
            d = S.ring[(S.ring_idx - 1u) & 3u];
            push = false;
        } else {
            if (S.bl_len[2] == 0u) block_switch(S, W, 2);
            S.bl_len[2] -= 1u;
            const uint32_t dctx = S.copy_len > 4u ? 3u : S.copy_len - 2u;
            const Tree<kDistAlphaMax>& T = W->dist[W->cmap_d[S.bl_type[2] * 4u + dctx]];
            const uint32_t dc = read_symbol(r, T.cnt, T.sym);
            if (dc < 16u) {
                if (st) st->ring_codes |= 1u << dc;
                if (dc == 0u) {
                    d = S.ring[(S.ring_idx - 1u) & 3u];
                    push = false;
                } else if (dc < 4u) {
                    d = S.ring[(S.ring_idx - 1u - dc) & 3u];
                } else {
                    const uint32_t k = (dc - 4u) % 6u;
                    const int32_t delta = (k & 1u) ? (int32_t)(k >> 1) + 1 : -((int32_t)(k >> 1) + 1);
                    d = (int64_t)S.ring[(S.ring_idx - (dc < 10u ? 1u : 2u)) & 3u] + delta;
                    if (d <= 0) d = 0x7FFFFFFF;  // refused below, as libbrotli does
                }
            } else if (dc < 16u + S.ndirect) {
                d = (int64_t)dc - 15;
            } else {
                const uint32_t v = dc - S.ndirect - 16u;
                const uint32_t hcode = v >> S.npostfix, lcode = v & ((1u << S.npostfix) - 1u);
                const uint32_t nbits = 1u + (hcode >> 1);
                const uint64_t offset = ((uint64_t)(2u + (hcode & 1u)) << nbits) - 4u;
                d = (int64_t)(((offset + br_read(r, nbits)) << S.npostfix) + lcode + S.ndirect + 1u);
            }
        }
        if (br_over(r)) return NX_ERR_BROTLI_TRUNCATED;
        const uint32_t maxd = pos < S.max_backward ? pos : S.max_backward;
        const uint32_t cl = S.copy_len;
        if (d > (int64_t)maxd) {  // a static dictionary reference
            if (d > (int64_t)kMaxDistance) return NX_ERR_BROTLI_DISTANCE;
            if (cl < 4u || cl > 24u) return NX_ERR_BROTLI_DICTIONARY;
            const uint64_t addr = (uint64_t)d - maxd - 1u;
            const uint32_t shift = dict_bits(cl);
            const uint32_t widx = (uint32_t)(addr & ((1u << shift) - 1u));
            const uint64_t tidx = addr >> shift;
            if (tidx >= kTransforms) return NX_ERR_BROTLI_TRANSFORM;
            const uint32_t wl = transform_word((uint32_t)tidx, dict + dict_offset(cl) + widx * cl, cl, op->word);
            if (wl > mlen) return overrun_code(S, pos, wl);
            if (wl > S.cap - pos) return NX_ERR_BROTLI_OUTPUT_FULL;
            op->word_len = wl;
            out_n = wl;
            if (wl == 1u) {
                p2 = p1;
                p1 = op->word[0];
            } else if (wl > 1u) {
                p2 = op->word[wl - 2u];
                p1 = op->word[wl - 1u];
            }
            if (st) {
                st->dict_refs += 1u;
                st->transforms[tidx >> 5] |= 1u << (tidx & 31u);
            }
        } else {
            if (cl > mlen) return overrun_code(S, pos, cl);
            if (cl > S.cap - pos) return NX_ERR_BROTLI_OUTPUT_FULL;
            op->copy_len = cl;
            op->dist = (uint32_t)d;
            out_n = cl;
            if (push) {
                S.ring[S.ring_idx & 3u] = (int32_t)d;
                S.ring_idx += 1u;
            }
        }
    }
    // A command of no literals whose dictionary word transforms to nothing produces no byte; from codes of one
    // symbol it consumes no bit either, and such commands would never end (libbrotli spins on them).  Refused.
    if (n + out_n == 0u && br_bitpos(r) == b0) return NX_ERR_BROTLI_DICTIONARY;
    S.in_cmd = 0;
    S.insert_left = 0;
    S.p1 = p1;
    S.p2 = p2;
    S.pos = pos + out_n;
    S.mlen = mlen - out_n;
    op->n_lit = n;
    op->done = S.mlen == 0u ? 1u : 0u;
    return NX_OK;
}

// After the ISLAST meta-block: the rest of its last byte is zero, and the stream ends with that byte.
NX_HD int32_t finish(State& S, uint32_t* consumed) {
    BitReader& r = S.br;
    const uint32_t pad = br_read(r, (uint32_t)((8u - (br_bitpos(r) & 7u)) & 7u));
    if (br_over(r)) return NX_ERR_BROTLI_TRUNCATED;
    if (pad) return NX_ERR_BROTLI_PADDING_2;
    *consumed = (uint32_t)(br_bitpos(r) >> 3);
    return NX_OK;
}

// An error decided on bits past the input's end is the input's end.
NX_HD int32_t settle(const State& S, int32_t e) { return e != NX_OK && e != NX_ERR_BROTLI_OUTPUT_FULL && br_over(S.br) ? NX_ERR_BROTLI_TRUNCATED : e; }

}  // namespace brd
}  // namespace nx
