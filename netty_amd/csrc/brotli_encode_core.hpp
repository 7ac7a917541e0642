// brotli_encode_core.hpp — the Brotli (RFC 7932) format core of BrotliEncoder, shared by the host encoder
// (brotli_encode_host.cpp) and the kernels (brotli.hip): the matcher, the command walker, the prefix-code
// builder and writer, and the meta-block encoder.  Everything here is __host__ __device__ and deterministic,
// and every array it indexes lives in a Work area the caller owns (LDS on the GPU), so the kernels need no
// scratch memory.  The kernels share the walker, the command symbols, the tree and finish_block with the host
// encoder; the histograms, the symbol sort and the command stream's bits they write with code of their own
// across the wave (brotli.hip), which the GPU tests hold to the host's bytes.
//
// The stream: the WBITS header for lgwin 10-24, then meta-blocks of at most 65 536 input bytes (MNIBBLES = 4),
// then the empty last meta-block (ISLAST = 1, ISLASTEMPTY = 1), or, for a write of the BrotliEncoder handle,
// the empty metadata meta-block libbrotli writes on a flush (ISLAST 0, MNIBBLES 3, reserved 0, MSKIPBYTES 0),
// either padded with zero bits to a byte.  An empty item is the header and that block.
//
// A compressed meta-block: ISLAST 0, MNIBBLES 0, MLEN - 1 in 16 bits, ISUNCOMPRESSED 0, then 13 zero bits
// (NBLTYPESL = NBLTYPESI = NBLTYPESD = 1, NPOSTFIX = 0, NDIRECT = 0, context mode 0, NTREESL = NTREESD = 1: one
// literal tree, one distance tree of 64 symbols, no context maps), then the literal, the insert-and-copy and the
// distance prefix code, then the commands: the insert-and-copy symbol, the insert and copy extra bits, the
// literals, then the distance symbol and its extra bits.  A prefix code with 1-4 used symbols (an alphabet
// nobody used counts as symbol 0) is a simple code, its symbols listed by (length, value); every other is a
// complex code: HSKIP 0, the code-length code lengths in the RFC's order with trailing zeros left out, then the
// lengths up to the last non-zero one, runs of three or more zeros as symbol 17 and of three or more repeats of
// a length as symbol 16, longer runs as the RFC's chained 16s and 17s.  Lengths are Huffman lengths limited to
// 15 (5 for the code-length code): the tree is built with every count raised to a floor of 1, 2, 4, ... until
// it is flat enough, ties going to the lower symbol and to leaves before inner nodes.
//
// Distances: codes 0-3 (the last four distances, exactly) and 16-63 are written; the commands below 128, whose
// distance is the last one with no distance symbol, are used wherever the insert code is below 8 and the copy
// code below 16.  The ring starts empty (four zeros, which no distance equals) and not at the RFC's 16, 15, 11,
// 4, so that a write of the handle, which does not know the distances of earlier writes, runs the same code.
// The emitter walks the meta-blocks in order and keeps the ring exactly: a copy pushes its distance unless it
// was coded as the last distance, and a meta-block that goes out uncompressed pushes nothing.
//
// Uncompressed fallback.  With p the bit position (mod 8) at which a meta-block of L bytes starts and C the
// exact bit count of its compressed form, the compressed form is written iff p + C < ceil8(p + 20) + 8 L,
// the bit position at which the uncompressed form (20 header bits, padding, L bytes) would end.  Every
// meta-block therefore ends at most 27 + 8 L bits after it started, the stream header is at most 7 bits and the
// last block 2 (a flush marker 6), so a stream of n bytes in m = ceil(n / 65536) meta-blocks has at most
// 7 + 27 m + 8 n + 6 bits, and ceil((27 m + 13) / 8) <= 4 m + 3 for every m >= 0:
//   max_stream_bytes(n) = n + 4 * ceil(n / 65536) + 3
// is a bound and not an allowance, for a stream and for a handle's write alike.
//
// The matcher (match_item) is greedy over a single-probe hash of four bytes.  Its rule, at position ip:
//   1. where ip + 4 <= n, the table entry of hash(in[ip..ip+4)) is read and replaced by ip; a candidate with
//      this call's stamp, below ip, at a distance <= min(ip, (1 << lgwin) - 16), whose four bytes are equal,
//      gives a match of length common_len up to min(n - ip, 65 536); otherwise the byte is a literal;
//   2. after a match of length L the positions ip + 1 .. ip + L - 1 that have four bytes left enter the table.
// A distance never passes min(position, (1 << lgwin) - 16): beyond it the decoder would read a reference to the
// static dictionary, which this encoder never writes.  A sequence is one 64-bit word: literal run (23 bits) |
// length << 23 (17 bits; 0: a run with no match after it, written when a run reaches 2^23 - 1 literals) |
// distance << 40.  The walker (next_cmd) turns sequences into commands that stay inside a meta-block: a literal
// run or a copy that crosses the boundary is cut there (a copy may not run past MLEN), a piece of a cut copy
// shorter than 2 bytes becomes a literal, and a meta-block that ends in literals ends with a command whose
// copy part (code 0) the decoder ignores.
#pragma once
#include "lz_seq_core.hpp"

namespace nx {
namespace brotli {
using namespace lzseq;

constexpr uint32_t kMbMax = 65536, kMinMatch = kHashBytes, kMaxCopy = 65536;
constexpr uint32_t kLenBits = 17;
constexpr uint32_t kLit = 0, kCmd = 256, kDist = 960, kSyms = 1024;  // the three alphabets side by side
constexpr uint32_t kNumCmd = 704, kNumDist = 64;
constexpr uint32_t kFlagHeader = 1u, kFlagFlush = 2u;  // write the WBITS header; end in the flush marker, not the last block
constexpr uint32_t kLitChunk = 32, kRawChunk = 64;    // most literals / raw bytes one step() writes

// a sequence with a match covers at least kMinMatch bytes, one without a match kRunMax literals
NX_HD size_t seq_cap(size_t n) { return n / kMinMatch + (n >> kRunBits) + 2u; }
NX_HD size_t max_stream_bytes(size_t n) { return n + 4u * ((n + kMbMax - 1u) / kMbMax) + 3u; }
NX_HD uint32_t max_distance(uint32_t lgwin) { return (1u << lgwin) - 16u; }

struct Stats {  // nx_brotli_encode_stats
    uint64_t compressed_blocks, uncompressed_blocks, commands, literals, ring_copies, implicit_copies, split_copies, simple_codes[4],
        complex_codes, limited_codes, max_depth_unlimited;
};

// Every array of the encoder, in LDS on the GPU (sizeof(Work), 17 220 bytes).
struct Work {
    uint32_t hist[kSyms];
    uint32_t node_w[2u * kNumCmd];    // tree weights, then node depths
    uint16_t node_parent[2u * kNumCmd];
    // the run-length form of a code description lives in the upper part of node_parent: it is built after the
    // alphabet's own tree, and the code-length code's tree (18 symbols) takes the first 35 nodes only
    NX_HD uint8_t* rle_sym() { return reinterpret_cast<uint8_t*>(node_parent + 64); }
    NX_HD uint8_t* rle_extra() { return reinterpret_cast<uint8_t*>(node_parent + 64) + kNumCmd; }
    uint16_t code[kSyms];
    uint16_t order[kNumCmd];          // used symbols by (count, symbol)
    uint8_t depth[kSyms];
    uint32_t cl_hist[18];
    uint16_t cl_code[18];
    uint16_t blc[16], next[16];
    uint8_t cl_depth[18];
    uint32_t unlimited;               // the deepest length of the last build before limiting
};

NX_HD uint32_t log2_floor(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); }

// The item's sequences into seq[0, cap) by the rule in the header comment; table: 2^kHashLog entries
// (stamp << 32 | position), an entry counts only with this call's stamp.  Returns the sequences written,
// or ~0 if cap would be passed (seq_cap(n) never is).
NX_HD uint32_t match_item(const uint8_t* in, uint32_t n, uint32_t lgwin, uint64_t* table, uint32_t stamp, uint64_t* seq, size_t cap) {
    SeqWriter out = {seq, cap, 0, 0};
    uint32_t ip = 0;
    const uint64_t stag = (uint64_t)stamp << 32;
    const uint32_t far = max_distance(lgwin);
    while (ip < n) {
        const uint32_t left = n - ip, maxlen = left < kMaxCopy ? left : kMaxCopy;
        uint32_t len = 0, dist = 0;
        if (left >= kMinMatch) {
            const uint32_t w = rd32(in + ip);
            const uint32_t cand = probe(table, stag, stamp, w, ip);
            if (cand != kNone && ip - cand <= far && rd32(in + cand) == w) {
                len = common_len(in + ip, in + cand, maxlen);
                dist = ip - cand;
            }
        }
        if (len == 0u) {
            ++ip;
            if (!out.literal()) return ~0u;
            continue;
        }
        if (!out.match(((uint64_t)len << kRunBits) | ((uint64_t)dist << (kRunBits + kLenBits)))) return ~0u;
        insert_span(table, stag, in, ip + 1u, ip + len, n);
        ip += len;
    }
    return out.ns;  // the literals after the last sequence are implied by n
}

// ------------------------------------------------------------------------------------------ commands
struct Walk {  // where the walker stands: the next input byte, the next sequence, what is left of the current one
    uint32_t ip, si, lit_left, cp_left, cp_dist;
};
struct Ring {  // the last four distances, d0 the latest; 0: none yet
    uint32_t d0, d1, d2, d3;
};
struct Cmd {
    uint32_t ins, copy, dist, split;  // copy 0: the meta-block ends in these literals
};

// The next command of the meta-block that ends at mb_end (w.ip < mb_end <= n).
__attribute__((always_inline)) NX_HD Cmd next_cmd(Walk& w, const uint64_t* seq, uint32_t ns, uint32_t n, uint32_t mb_end) {
    Cmd c = {0, 0, 0, 0};
    uint32_t pos = w.ip;
    for (;;) {
        if (w.lit_left == 0u && w.cp_left == 0u) {
            if (w.si < ns) {
                const uint64_t s = seq[w.si++];
                w.lit_left = (uint32_t)s & kRunMax;
                w.cp_left = (uint32_t)(s >> kRunBits) & ((1u << kLenBits) - 1u);
                w.cp_dist = (uint32_t)(s >> (kRunBits + kLenBits));
            } else {
                w.lit_left = n - pos;
            }
        }
        const uint32_t room = mb_end - pos, take = w.lit_left < room ? w.lit_left : room;
        c.ins += take;
        pos += take;
        w.lit_left -= take;
        if (pos == mb_end) break;
        if (w.cp_left != 0u) {
            const uint32_t left = mb_end - pos, k = w.cp_left < left ? w.cp_left : left;
            if (k < 2u) {  // a piece of a cut copy too short for a copy: one literal
                ++c.ins;
                ++pos;
                --w.cp_left;
                if (pos == mb_end) break;
                continue;
            }
            c.copy = k;
            c.dist = w.cp_dist;
            c.split = k < w.cp_left ? 1u : 0u;
            w.cp_left -= k;
            pos += k;
            break;
        }
    }
    w.ip = pos;
    return c;
}

NX_HD uint32_t insert_code(uint32_t l) {
    if (l < 6u) return l;
    if (l < 130u) {
        const uint32_t nb = log2_floor(l - 2u) - 1u;
        return (nb << 1) + ((l - 2u) >> nb) + 2u;
    }
    if (l < 2114u) return log2_floor(l - 66u) + 10u;
    return l < 6210u ? 21u : l < 22594u ? 22u : 23u;
}
NX_HD uint32_t insert_extra(uint32_t c) { return c < 6u ? 0u : c < 16u ? (c - 4u) >> 1 : c < 21u ? c - 10u : c == 21u ? 12u : c == 22u ? 14u : 24u; }
NX_HD uint32_t insert_base(uint32_t c) {
    if (c < 6u) return c;
    if (c < 16u) return ((2u + ((c - 4u) & 1u)) << ((c - 4u) >> 1)) + 2u;
    if (c < 21u) return 66u + (1u << (c - 10u));
    return c == 21u ? 2114u : c == 22u ? 6210u : 22594u;
}
NX_HD uint32_t copy_code(uint32_t l) {
    if (l < 10u) return l - 2u;
    if (l < 134u) {
        const uint32_t nb = log2_floor(l - 6u) - 1u;
        return (nb << 1) + ((l - 6u) >> nb) + 4u;
    }
    if (l < 2118u) return log2_floor(l - 70u) + 12u;
    return 23u;
}
NX_HD uint32_t copy_extra(uint32_t c) { return c < 8u ? 0u : c < 18u ? (c - 6u) >> 1 : c < 23u ? c - 12u : 24u; }
NX_HD uint32_t copy_base(uint32_t c) {
    if (c < 8u) return c + 2u;
    if (c < 18u) return ((2u + ((c - 6u) & 1u)) << ((c - 6u) >> 1)) + 6u;
    if (c < 23u) return 70u + (1u << (c - 12u));
    return 2118u;
}
// The insert-and-copy symbol of the RFC's cell table; implicit: the cells below 128 (insert code < 8, copy code < 16).
NX_HD uint32_t command_symbol(uint32_t ic, uint32_t cc, bool implicit) {
    const uint32_t low = ((ic & 7u) << 3) | (cc & 7u);
    if (implicit) return (cc < 8u ? 0u : 64u) | low;
    const uint32_t cell = (cc >> 3) + 3u * (ic >> 3);  // 128, 192, 384, 256, 320, 512, 448, 576, 640
    return ((uint32_t)(0xA97854632ull >> (4u * cell)) & 15u) * 64u + low;
}

struct Syms {  // what a command writes
    uint32_t cmd, ins_nb, ins_val, cp_nb, cp_val, has_dist, dsym, d_nb, d_val, kind;  // kind 0: explicit, 1: ring, 2: implicit
};
__attribute__((always_inline)) NX_HD Syms make_syms(const Cmd& c, Ring& r) {
    Syms s = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const uint32_t ic = insert_code(c.ins);
    s.ins_nb = insert_extra(ic);
    s.ins_val = c.ins - insert_base(ic);
    if (c.copy == 0u) {
        s.cmd = command_symbol(ic, 0u, false);
        return s;
    }
    const uint32_t cc = copy_code(c.copy);
    s.cp_nb = copy_extra(cc);
    s.cp_val = c.copy - copy_base(cc);
    uint32_t dcode;
    if (c.dist == r.d0) dcode = 0u;
    else if (c.dist == r.d1) dcode = 1u;
    else if (c.dist == r.d2) dcode = 2u;
    else if (c.dist == r.d3) dcode = 3u;
    else {
        const uint32_t d = c.dist + 3u, bucket = log2_floor(d) - 1u, prefix = (d >> bucket) & 1u;
        dcode = 16u + 2u * (bucket - 1u) + prefix;
        s.d_nb = bucket;
        s.d_val = d - ((2u + prefix) << bucket);
    }
    const bool implicit = dcode == 0u && ic < 8u && cc < 16u;
    s.cmd = command_symbol(ic, cc, implicit);
    s.has_dist = implicit ? 0u : 1u;
    s.dsym = dcode;
    s.kind = implicit ? 2u : dcode < 16u ? 1u : 0u;
    if (dcode != 0u) {
        r.d3 = r.d2;
        r.d2 = r.d1;
        r.d1 = r.d0;
        r.d0 = c.dist;
    }
    return s;
}

// ------------------------------------------------------------------------------------------ prefix codes
// The used symbols of hist[0, n) into W->order by (count, symbol), and depth[0, n) cleared; returns their number.
// (The kernel does this step across the wave as a rank sort, which gives the same order: brotli.hip.)
NX_HD uint32_t sort_symbols(Work* W, const uint32_t* hist, uint8_t* depth, uint32_t n) {
    uint32_t m = 0;
    for (uint32_t s = 0; s < n; ++s) {
        depth[s] = 0;
        if (hist[s] == 0u) continue;
        uint32_t j = m++;
        for (; j > 0u && hist[W->order[j - 1u]] > hist[s]; --j) W->order[j] = W->order[j - 1u];
        W->order[j] = (uint16_t)s;
    }
    return m;
}

// Huffman lengths of the m symbols in W->order, limited to `limit`, into depth (cleared before); returns m.  One
// used symbol gets length 0.  W->unlimited: the deepest length before limiting.
NX_HD uint32_t tree_depths(Work* W, const uint32_t* hist, uint8_t* depth, uint32_t m, uint32_t limit) {
    W->unlimited = 0;
    if (m < 2u) return m;
    for (uint32_t floor = 1u;; floor *= 2u) {
        for (uint32_t i = 0; i < m; ++i) {
            const uint32_t h = hist[W->order[i]];
            W->node_w[i] = h > floor ? h : floor;
        }
        uint32_t i = 0, j = m, k = m;
        while (k < 2u * m - 1u) {
            const uint32_t a = (i < m && (j >= k || W->node_w[i] <= W->node_w[j])) ? i++ : j++;
            const uint32_t b = (i < m && (j >= k || W->node_w[i] <= W->node_w[j])) ? i++ : j++;
            W->node_w[k] = W->node_w[a] + W->node_w[b];
            W->node_parent[a] = (uint16_t)k;
            W->node_parent[b] = (uint16_t)k;
            ++k;
        }
        W->node_w[2u * m - 2u] = 0;  // from here on node_w holds depths: a parent comes after its children
        for (uint32_t t = 2u * m - 2u; t-- > 0u;) W->node_w[t] = W->node_w[W->node_parent[t]] + 1u;
        uint32_t deepest = 0;
        for (uint32_t t = 0; t < m; ++t) deepest = W->node_w[t] > deepest ? W->node_w[t] : deepest;
        if (floor == 1u) W->unlimited = deepest;
        if (deepest <= limit) {
            for (uint32_t t = 0; t < m; ++t) depth[W->order[t]] = (uint8_t)W->node_w[t];
            return m;
        }
    }
}

NX_HD uint32_t build_depths(Work* W, const uint32_t* hist, uint8_t* depth, uint32_t n, uint32_t limit) {
    return tree_depths(W, hist, depth, sort_symbols(W, hist, depth, n), limit);
}

// Canonical codes of depth[0, n), bit-reversed, as the stream takes them least significant bit first.
NX_HD void assign_codes(Work* W, const uint8_t* depth, uint16_t* code, uint32_t n) {
    for (uint32_t l = 0; l < 16u; ++l) W->blc[l] = 0;
    for (uint32_t s = 0; s < n; ++s) ++W->blc[depth[s]];
    W->blc[0] = 0;
    uint32_t c = 0;
    for (uint32_t l = 1; l < 16u; ++l) {
        c = (c + W->blc[l - 1u]) << 1;
        W->next[l] = (uint16_t)c;
    }
    for (uint32_t s = 0; s < n; ++s) {
        const uint32_t l = depth[s];
        uint32_t v = l ? W->next[l]++ : 0u, rev = 0;
        for (uint32_t b = 0; b < l; ++b, v >>= 1) rev = (rev << 1) | (v & 1u);
        code[s] = (uint16_t)rev;
    }
}

struct BitCount {  // a writer that only counts
    uint64_t bits;
    NX_HD void put(uint32_t, uint32_t nb) { bits += nb; }
};

NX_HD uint32_t cl_order(uint32_t i) { return i < 4u ? i + 1u : i == 4u ? 0u : i == 5u ? 5u : i == 6u ? 17u : i == 7u ? 6u : i == 8u ? 16u : i - 2u; }

// A run of `reps` (>= 3) as chained repeat symbols `sym` with `bits` extra bits each (RFC 7932 section 3.5).
NX_HD uint32_t rle_chain(Work* W, uint32_t nr, uint32_t sym, uint32_t bits, uint32_t reps) {
    const uint32_t start = nr;
    for (uint32_t r = reps - 3u;;) {
        W->rle_sym()[nr] = (uint8_t)sym;
        W->rle_extra()[nr] = (uint8_t)(r & ((1u << bits) - 1u));
        ++nr;
        r >>= bits;
        if (r == 0u) break;
        --r;
    }
    for (uint32_t a = start, b = nr - 1u; a < b; ++a, --b) {  // the most significant digit goes first
        const uint8_t t = W->rle_extra()[a];
        W->rle_extra()[a] = W->rle_extra()[b];
        W->rle_extra()[b] = t;
    }
    return nr;
}

// The description of the prefix code of alphabet [base, base + n) (used: its used symbols; abits: the bits of a
// symbol in a simple code) to b.  The complex form overwrites the rle and code-length areas of W.
template <class B>
NX_HD void store_code(B& b, Work* W, uint32_t base, uint32_t n, uint32_t abits, uint32_t used) {
    const uint8_t* depth = W->depth + base;
    if (used <= 4u) {
        b.put(1u, 2u);
        b.put(used ? used - 1u : 0u, 2u);
        if (used == 0u) b.put(0u, abits);
        uint32_t deepest = 0;
        for (uint32_t d = 0; d < 4u; ++d)
            for (uint32_t s = 0; s < n; ++s)
                if (W->hist[base + s] != 0u && depth[s] == d) {
                    b.put(s, abits);
                    deepest = d;
                }
        if (used == 4u) b.put(deepest == 3u ? 1u : 0u, 1u);
        return;
    }
    uint32_t len_n = n;
    while (depth[len_n - 1u] == 0u) --len_n;
    uint32_t nr = 0, prev = 8u;
    for (uint32_t i = 0; i < len_n;) {
        const uint32_t v = depth[i];
        uint32_t reps = 1;
        while (i + reps < len_n && depth[i + reps] == v) ++reps;
        i += reps;
        if (v != 0u && prev != v) {
            W->rle_sym()[nr] = (uint8_t)v;
            W->rle_extra()[nr++] = 0;
            --reps;
            prev = v;
        }
        if (reps < 3u) {
            for (; reps; --reps) {
                W->rle_sym()[nr] = (uint8_t)v;
                W->rle_extra()[nr++] = 0;
            }
        } else {
            nr = v == 0u ? rle_chain(W, nr, 17u, 3u, reps) : rle_chain(W, nr, 16u, 2u, reps);
        }
    }
    for (uint32_t s = 0; s < 18u; ++s) W->cl_hist[s] = 0;
    for (uint32_t i = 0; i < nr; ++i) ++W->cl_hist[W->rle_sym()[i]];
    const uint32_t unlimited = W->unlimited;
    const uint32_t nc = build_depths(W, W->cl_hist, W->cl_depth, 18u, 5u);
    W->unlimited = unlimited;
    assign_codes(W, W->cl_depth, W->cl_code, 18u);
    b.put(0u, 2u);  // HSKIP
    uint32_t nstore = 18u;
    if (nc > 1u)  // a single code-length symbol is written as length 1 among all 18, and then takes no bits
        while (W->cl_depth[cl_order(nstore - 1u)] == 0u) --nstore;
    for (uint32_t i = 0; i < nstore; ++i) {
        const uint32_t s = cl_order(i), v = (nc == 1u && W->cl_hist[s] != 0u) ? 1u : W->cl_depth[s];
        b.put((0xF12370u >> (4u * v)) & 15u, (0x422342u >> (4u * v)) & 15u);  // the RFC's fixed code of 0..5
    }
    for (uint32_t i = 0; i < nr; ++i) {
        const uint32_t s = W->rle_sym()[i];
        b.put(W->cl_code[s], W->cl_depth[s]);
        if (s == 16u) b.put(W->rle_extra()[i], 2u);
        if (s == 17u) b.put(W->rle_extra()[i], 3u);
    }
}

// ------------------------------------------------------------------------------------------ the encoder
// One item or one write, in steps that each write a bounded number of bytes (about 1.3 KiB at the start of a
// meta-block, under 80 otherwise).  Sink: void put(uint8_t).  st: Stats* or nullptr.
template <class Sink>
struct Encoder {
    Work* W;
    Sink out;  // by value: a sink behind a pointer would live in scratch memory on the GPU
    Stats* st;
    const uint8_t* in;
    const uint64_t* seq;
    uint32_t n, ns, lgwin, flags;
    uint64_t acc;
    uint32_t nacc;
    Walk w, w_end, ws;  // ws, rs: the scan's walker and ring
    Ring r, rs;
    uint64_t scan_bits;
    uint32_t used0, used1, used2, deepest, limited;  // of the block being closed
    uint32_t mb_end, state, raw_at, lit_at, lit_end;
    Syms sy;
    bool in_cmd, done;

    enum : uint32_t { kStart = 0, kBlock, kCommands, kRaw, kFinish };

    NX_HD void init(Work* W_, const Sink& out_, Stats* st_, const uint8_t* in_, uint32_t n_, const uint64_t* seq_, uint32_t ns_, uint32_t lgwin_,
                    uint32_t flags_) {
        W = W_, out = out_, st = st_, in = in_, seq = seq_, n = n_, ns = ns_, lgwin = lgwin_, flags = flags_;
        acc = 0, nacc = 0;
        w = {0, 0, 0, 0, 0};
        w_end = w;
        ws = w;
        r = {0, 0, 0, 0};
        rs = r;
        scan_bits = 0;
        used0 = used1 = used2 = deepest = limited = 0;
        mb_end = 0, state = kStart, raw_at = 0, lit_at = 0, lit_end = 0;
        in_cmd = false, done = false;
    }

    NX_HD void put(uint32_t v, uint32_t nb) {  // nb <= 32
        acc |= (uint64_t)v << nacc;
        nacc += nb;
        while (nacc >= 8u) {
            out.put((uint8_t)acc);
            acc >>= 8;
            nacc -= 8u;
        }
    }
    NX_HD void pad() { put(0u, (8u - nacc) & 7u); }

    NX_HD void count_code(uint32_t used) {
        if (used <= 4u) ++st->simple_codes[used ? used - 1u : 0u];
        else ++st->complex_codes;
    }

    // A meta-block begins in three parts, which the kernel runs apart (its wave takes the histograms):
    // open_block: where it ends, and the scan's own walker and ring; scan_block: the three histograms and the
    // extra bits of its commands; close_block: the lengths and codes, the exact bit count, the choice of form,
    // the header and the code descriptions.
    NX_HD void open_block() {
        mb_end = n - w.ip < kMbMax ? n : w.ip + kMbMax;
        ws = w;
        rs = r;
        scan_bits = 33u;  // the header of a compressed meta-block
    }
    NX_HD void scan_block() {
        for (uint32_t s = 0; s < kSyms; ++s) W->hist[s] = 0;
        while (ws.ip < mb_end) {
            const uint32_t from = ws.ip;
            const Cmd c = next_cmd(ws, seq, ns, n, mb_end);
            const Syms s = make_syms(c, rs);
            ++W->hist[kCmd + s.cmd];
            for (uint32_t p = from; p < from + c.ins; ++p) ++W->hist[kLit + in[p]];
            if (s.has_dist) ++W->hist[kDist + s.dsym];
            scan_bits += s.ins_nb + s.cp_nb + s.d_nb;
        }
    }
    NX_HD void begin_block() {
        open_block();
        scan_block();
        close_block();
    }
    // close_block is itself in parts, which the kernel runs apart (its wave sorts the symbols): per alphabet a
    // (0 literals, 1 commands, 2 distances) the used symbols sorted into W->order, then block_lengths(a, m); then
    // finish_block.
    NX_HD void block_lengths(uint32_t a, uint32_t m) {
        const uint32_t base = a == 0u ? kLit : a == 1u ? kCmd : kDist;
        tree_depths(W, W->hist + base, W->depth + base, m, 15u);
        if (a == 0u) used0 = m, deepest = 0, limited = 0;
        if (a == 1u) used1 = m;
        if (a == 2u) used2 = m;
        deepest = W->unlimited > deepest ? W->unlimited : deepest, limited += W->unlimited > 15u;
    }
    NX_HD void close_block() {
        block_lengths(0u, sort_symbols(W, W->hist + kLit, W->depth + kLit, 256u));
        block_lengths(1u, sort_symbols(W, W->hist + kCmd, W->depth + kCmd, kNumCmd));
        block_lengths(2u, sort_symbols(W, W->hist + kDist, W->depth + kDist, kNumDist));
        finish_block();
    }
    NX_HD void finish_block() {
        const uint32_t mlen = mb_end - w.ip;
        uint64_t bits = scan_bits;
        w_end = ws;
        assign_codes(W, W->depth + kLit, W->code + kLit, 256u);
        assign_codes(W, W->depth + kCmd, W->code + kCmd, kNumCmd);
        assign_codes(W, W->depth + kDist, W->code + kDist, kNumDist);
        for (uint32_t s = 0; s < kSyms; ++s) bits += (uint64_t)W->hist[s] * W->depth[s];
        BitCount bc = {0};
        store_code(bc, W, kLit, 256u, 8u, used0);
        store_code(bc, W, kCmd, kNumCmd, 10u, used1);
        store_code(bc, W, kDist, kNumDist, 6u, used2);
        bits += bc.bits;
        const bool compressed = nacc + bits < ((nacc + 20u + 7u) & ~7u) + 8ull * mlen;
        put(0u, 3u);  // ISLAST 0, MNIBBLES 0: four nibbles
        put(mlen - 1u, 16u);
        if (compressed) {
            put(0u, 14u);  // ISUNCOMPRESSED 0 and the 13 bits of the header comment
            store_code(*this, W, kLit, 256u, 8u, used0);
            store_code(*this, W, kCmd, kNumCmd, 10u, used1);
            store_code(*this, W, kDist, kNumDist, 6u, used2);
            state = kCommands;
            if (st) {
                ++st->compressed_blocks;
                count_code(used0);
                count_code(used1);
                count_code(used2);
                st->limited_codes += limited;
                if (deepest > st->max_depth_unlimited) st->max_depth_unlimited = deepest;
            }
        } else {
            put(1u, 1u);  // ISUNCOMPRESSED
            pad();
            raw_at = w.ip;
            state = kRaw;
            if (st) ++st->uncompressed_blocks;
        }
    }

    NX_HD void step_command() {
        if (!in_cmd) {
            lit_at = w.ip;
            const Cmd c = next_cmd(w, seq, ns, n, mb_end);
            sy = make_syms(c, r);
            lit_end = lit_at + c.ins;
            put(W->code[kCmd + sy.cmd], W->depth[kCmd + sy.cmd]);
            put(sy.ins_val, sy.ins_nb);
            put(sy.cp_val, sy.cp_nb);
            in_cmd = true;
            if (st) {
                ++st->commands;
                st->literals += c.ins;
                st->ring_copies += sy.kind == 1u;
                st->implicit_copies += sy.kind == 2u;
                st->split_copies += c.split;
            }
        }
        const uint32_t e = lit_end - lit_at < kLitChunk ? lit_end : lit_at + kLitChunk;
        for (; lit_at < e; ++lit_at) put(W->code[kLit + in[lit_at]], W->depth[kLit + in[lit_at]]);
        if (lit_at != lit_end) return;
        if (sy.has_dist) {
            put(W->code[kDist + sy.dsym], W->depth[kDist + sy.dsym]);
            put(sy.d_val, sy.d_nb);
        }
        in_cmd = false;
        if (w.ip == mb_end) state = w.ip < n ? kBlock : kFinish;
    }

    NX_HD void step() {
        switch (state) {
            case kStart:
                if (flags & kFlagHeader) {
                    if (lgwin == 16u) put(0u, 1u);
                    else if (lgwin == 17u) put(1u, 7u);
                    else if (lgwin > 17u) put(((lgwin - 17u) << 1) | 1u, 4u);
                    else put(((lgwin - 8u) << 4) | 1u, 7u);
                }
                state = n ? kBlock : kFinish;
                break;
            case kBlock: begin_block(); break;
            case kCommands: step_command(); break;
            case kRaw: {
                const uint32_t e = mb_end - raw_at < kRawChunk ? mb_end : raw_at + kRawChunk;
                for (; raw_at < e; ++raw_at) out.put(in[raw_at]);
                if (raw_at == mb_end) {
                    w = w_end;  // the ring keeps what it held: the decoder saw no distance
                    state = w.ip < n ? kBlock : kFinish;
                }
                break;
            }
            default:
                if (flags & kFlagFlush) put(6u, 6u);  // ISLAST 0, MNIBBLES 3, reserved 0, MSKIPBYTES 0
                else put(3u, 2u);                      // ISLAST 1, ISLASTEMPTY 1
                pad();
                done = true;
                break;
        }
    }
};

// An upper bound of the steps an item takes.
NX_HD uint64_t max_steps(uint32_t n, uint32_t ns) {
    const uint64_t blocks = (uint64_t)n / kMbMax + 1u;
    return 4u + 2u * ns + 4u * blocks + (uint64_t)n / kLitChunk + (uint64_t)n / kRawChunk;
}

}  // namespace brotli
}  // namespace nx
