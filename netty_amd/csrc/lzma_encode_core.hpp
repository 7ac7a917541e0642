// lzma_encode_core.hpp — the LZMA format core of LzmaFrameEncoder, shared by the host encoder
// (lzma_encode_host.cpp) and the kernels (lzma.hip): the probability model's layout, the 12-state
// machine, the packet coders, the range coder and the matcher.  Everything here is __host__ __device__
// and deterministic, so that the host and the GPU write the same bytes.
//
// The stream (LzmaFrameEncoder.java:177-186): 13 header bytes (properties, dictionary size, the exact
// length) and the LZMA payload of the item, coded from a freshly initialised model, optionally closed by
// the end marker, then the range coder's five flush bytes.
//
// The model is one array of 11-bit probabilities (uint16_t, all 1024 at the start, moved by a shift of 5):
//   IsMatch[12][16], IsRep[12], IsRepG0[12], IsRepG1[12], IsRepG2[12], IsRep0Long[12][16],
//   PosSlot[4][64], SpecPos[115] (the reverse trees of slots 4..13), Align[16],
//   two length coders {choice, choice2, low[16][8], mid[16][8], high[256]}, and the literal coder's
//   0x300 << (lc + lp) entries at the end: 1848 + (0x300 << (lc + lp)) entries in all.
//
// The matcher (match_item) is greedy over a single-probe hash of four bytes.  Its rule, at position ip
// with limit = min(ip, dict_size) and maxlen = min(n - ip, 273):
//   1. each of the four rep distances d <= limit is compared at ip; the longest wins, the lower index on a
//      tie, and it counts from length 2;
//   2. where ip + 4 <= n, the table entry of hash(in[ip..ip+4)) is read and replaced by ip; a candidate
//      with this call's stamp, at a distance <= limit, whose four bytes are equal, gives the hash match,
//      of length >= 4;
//   3. a rep of length r >= 2 is taken if there is no hash match or r + 1 >= its length; else the hash match
//      is taken; else the byte is a literal;
//   4. after a match of length L the positions ip + 1 .. ip + L - 1 that have four bytes left enter the table.
// A match stops at maxlen; a longer repetition continues as rep0 packets by rule 1.  No short rep is written.
// A distance equal to a rep distance is coded as that rep (the lowest such index) by the packet coder.
// A sequence is one 64-bit word: literal run (23 bits) | length << 23 (9 bits; 0: a run with no match after
// it, written when a run reaches 2^23 - 1 literals) | distance << 32.
#pragma once
#include "lz_seq_core.hpp"

namespace nx {
namespace lzma {
using namespace lzseq;

constexpr uint32_t kHeaderBytes = 13;
constexpr uint32_t kStates = 12, kMatchMin = 2, kMatchMax = 273, kHashMin = kHashBytes;
constexpr uint32_t kProbInit = 1024, kMoveBits = 5, kBitModelBits = 11;
constexpr uint32_t kTopValue = 1u << 24;
// model layout
constexpr uint32_t kIsMatch = 0, kIsRep = kIsMatch + kStates * 16u, kIsRepG0 = kIsRep + kStates, kIsRepG1 = kIsRepG0 + kStates,
                   kIsRepG2 = kIsRepG1 + kStates, kIsRep0Long = kIsRepG2 + kStates, kPosSlot = kIsRep0Long + kStates * 16u,
                   kSpecPos = kPosSlot + 4u * 64u, kAlign = kSpecPos + 116u, kLenCoder = kAlign + 16u, kLenProbs = 2u + 128u + 128u + 256u,
                   kRepLenCoder = kLenCoder + kLenProbs, kLiteral = kRepLenCoder + kLenProbs;
static_assert(kLiteral == 1848u, "model layout");
NX_HD uint32_t model_probs(uint32_t lc, uint32_t lp) { return kLiteral + (0x300u << (lc + lp)); }

// matcher: the most sequences an n-byte item gives: a sequence with a match covers at least two bytes, one without a
// match kRunMax literals
NX_HD size_t seq_cap(size_t n) { return n / 2u + (n >> kRunBits) + 2u; }
NX_HD size_t max_stream_bytes(size_t n) { return kHeaderBytes + n + n / 3u + 128u; }

struct Params {
    uint32_t lc, lp, pb, dict_size, end_marker;
};

struct Stats {  // nx_lzma_encode_stats
    uint64_t literals, matched_literals, matches, short_reps, reps[4], carries, max_pending_ff, max_carry_ff;
};

NX_HD void reps_use(uint32_t* rep, uint32_t i) {  // rep[i] moves to the front
    const uint32_t d = rep[i];
    for (; i > 0u; --i) rep[i] = rep[i - 1u];
    rep[0] = d;
}
NX_HD void reps_push(uint32_t* rep, uint32_t d) {
    rep[3] = rep[2];
    rep[2] = rep[1];
    rep[1] = rep[0];
    rep[0] = d;
}

// The item's sequences into seq[0, cap) by the rule in the header comment; table: 2^kHashLog entries
// (stamp << 32 | position), an entry counts only with this call's stamp.  Returns the sequences written,
// or ~0 if cap would be passed (seq_cap(n) never is).
NX_HD uint32_t match_item(const uint8_t* in, uint32_t n, uint32_t dict_size, uint64_t* table, uint32_t stamp, uint64_t* seq,
                          size_t cap) {
    uint32_t rep[4] = {0, 0, 0, 0};  // distances - 1, as the coder keeps them
    SeqWriter out = {seq, cap, 0, 0};
    uint32_t ip = 0;
    const uint64_t stag = (uint64_t)stamp << 32;
    while (ip < n) {
        const uint32_t limit = ip < dict_size ? ip : dict_size;
        const uint32_t left = n - ip, maxlen = left < kMatchMax ? left : kMatchMax;
        uint32_t rlen = 0, ri = 0, mlen = 0, mdist = 0;
        if (maxlen >= kMatchMin) {
            for (uint32_t i = 0; i < 4u; ++i) {
                const uint32_t d = rep[i] + 1u;
                if (d > limit || d == 0u) continue;
                if (in[ip] != in[ip - d] || in[ip + 1u] != in[ip + 1u - d]) continue;
                const uint32_t l = common_len(in + ip, in + ip - d, maxlen);
                if (l > rlen) rlen = l, ri = i;
            }
        }
        if (left >= kHashMin) {
            const uint32_t w = rd32(in + ip);
            const uint32_t cand = probe(table, stag, stamp, w, ip);
            if (cand != kNone && ip - cand <= limit && rd32(in + cand) == w) {
                mlen = common_len(in + ip, in + cand, maxlen);
                mdist = ip - cand;
            }
        }
        uint32_t len = 0, dist = 0;
        if (rlen >= kMatchMin && (mlen == 0u || rlen + 1u >= mlen)) {
            len = rlen;
            dist = rep[ri] + 1u;
            reps_use(rep, ri);
        } else if (mlen >= kHashMin) {
            len = mlen;
            dist = mdist;
            uint32_t i = 0;
            while (i < 4u && rep[i] != dist - 1u) ++i;
            if (i < 4u) reps_use(rep, i);
            else reps_push(rep, dist - 1u);
        }
        if (len == 0u) {
            ++ip;
            if (!out.literal()) return ~0u;
            continue;
        }
        if (!out.match(((uint64_t)len << kRunBits) | ((uint64_t)dist << 32))) return ~0u;
        insert_span(table, stag, in, ip + 1u, ip + len, n);
        ip += len;
    }
    return out.ns;  // the literals after the last sequence are implied by n
}

// The 13 header bytes.
NX_HD void write_header(uint8_t* out, const Params& P, uint64_t n) {
    out[0] = (uint8_t)((P.pb * 5u + P.lp) * 9u + P.lc);
    for (uint32_t i = 0; i < 4u; ++i) out[1u + i] = (uint8_t)(P.dict_size >> (8u * i));
    for (uint32_t i = 0; i < 8u; ++i) out[5u + i] = (uint8_t)(n >> (8u * i));
}

// The range coder and the packet coders over model p.  Sink: void put(uint8_t).  S: Stats* or nullptr.
template <class Sink>
struct Coder {
    uint16_t* p;
    Sink* out;
    Stats* st;
    const uint8_t* in;
    const uint64_t* seq;
    uint32_t n, ns;
    Params P;
    // range coder
    uint64_t low;
    uint32_t range;
    uint32_t cache;
    uint64_t cache_size;
    // LZ state
    uint32_t state, rep[4], pos, si, run_left, cur_len, cur_dist;
    bool loaded, marker_done, done;

    NX_HD void init(uint16_t* probs, Sink* sink, Stats* stats, const uint8_t* src, uint32_t len, const uint64_t* s, uint32_t nseq,
                    const Params& params) {
        p = probs;
        out = sink;
        st = stats;
        in = src;
        seq = s;
        n = len;
        ns = nseq;
        P = params;
        low = 0;
        range = 0xFFFFFFFFu;
        cache = 0;
        cache_size = 1;
        state = 0;
        rep[0] = rep[1] = rep[2] = rep[3] = 0;
        pos = si = run_left = cur_len = cur_dist = 0;
        loaded = marker_done = done = false;
    }

    NX_HD void shift_low() {
        if ((uint32_t)low < 0xFF000000u || (uint32_t)(low >> 32) != 0u) {
            const uint32_t carry = (uint32_t)(low >> 32);
            if (st) {
                const uint64_t pending = cache_size - 1u;
                if (pending > st->max_pending_ff) st->max_pending_ff = pending;
                if (carry) {
                    st->carries += 1u;
                    if (pending > st->max_carry_ff) st->max_carry_ff = pending;
                }
            }
            uint32_t temp = cache;
            do {
                out->put((uint8_t)(temp + carry));
                temp = 0xFFu;
            } while (--cache_size != 0u);
            cache = (uint32_t)(low >> 24) & 0xFFu;
        }
        ++cache_size;
        low = (low & 0x00FFFFFFu) << 8;
    }
    NX_HD void bit(uint32_t idx, uint32_t b) {
        const uint32_t v = p[idx], bound = (range >> kBitModelBits) * v;
        if (b == 0u) {
            range = bound;
            p[idx] = (uint16_t)(v + (((1u << kBitModelBits) - v) >> kMoveBits));
        } else {
            low += bound;
            range -= bound;
            p[idx] = (uint16_t)(v - (v >> kMoveBits));
        }
        while (range < kTopValue) {
            range <<= 8;
            shift_low();
        }
    }
    NX_HD void direct(uint32_t v, uint32_t nbits) {
        for (uint32_t i = nbits; i-- > 0u;) {
            range >>= 1;
            if ((v >> i) & 1u) low += range;
            while (range < kTopValue) {
                range <<= 8;
                shift_low();
            }
        }
    }
    NX_HD void tree(uint32_t base, uint32_t nbits, uint32_t v) {
        uint32_t m = 1;
        for (uint32_t i = nbits; i-- > 0u;) {
            const uint32_t b = (v >> i) & 1u;
            bit(base + m, b);
            m = (m << 1) | b;
        }
    }
    NX_HD void rtree(uint32_t base, uint32_t nbits, uint32_t v) {
        uint32_t m = 1;
        for (uint32_t i = 0; i < nbits; ++i) {
            const uint32_t b = v & 1u;
            v >>= 1;
            bit(base + m, b);
            m = (m << 1) | b;
        }
    }
    NX_HD void length(uint32_t coder, uint32_t len, uint32_t ps) {
        const uint32_t l = len - kMatchMin;
        if (l < 8u) {
            bit(coder, 0);
            tree(coder + 2u + ps * 8u, 3, l);
        } else if (l < 16u) {
            bit(coder, 1);
            bit(coder + 1u, 0);
            tree(coder + 2u + 128u + ps * 8u, 3, l - 8u);
        } else {
            bit(coder, 1);
            bit(coder + 1u, 1);
            tree(coder + 2u + 256u, 8, l - 16u);
        }
    }
    NX_HD void literal() {
        const uint32_t ps = pos & ((1u << P.pb) - 1u);
        bit(kIsMatch + (state << 4) + ps, 0);
        const uint32_t prev = pos ? in[pos - 1u] : 0u, byte = in[pos];
        const uint32_t base = kLiteral + 0x300u * (((pos & ((1u << P.lp) - 1u)) << P.lc) + (prev >> (8u - P.lc)));
        if (state < 7u) {
            tree(base, 8, byte);
            if (st) st->literals += 1u;
        } else {
            uint32_t mb = in[pos - rep[0] - 1u], offs = 0x100u, sym = byte | 0x100u;
            do {
                mb <<= 1;
                bit(base + offs + (mb & offs) + (sym >> 8), (sym >> 7) & 1u);
                sym <<= 1;
                offs &= ~(mb ^ sym);
            } while (sym < 0x10000u);
            if (st) st->matched_literals += 1u;
        }
        state = state < 4u ? 0u : state < 10u ? state - 3u : state - 6u;
        ++pos;
    }
    // a match of `len` at distance - 1 = d0 (0xFFFFFFFF: the end marker)
    NX_HD void match(uint32_t len, uint32_t d0) {
        const uint32_t ps = pos & ((1u << P.pb) - 1u);
        bit(kIsMatch + (state << 4) + ps, 1);
        bit(kIsRep + state, 0);
        state = state < 7u ? 7u : 10u;
        length(kLenCoder, len, ps);
        const uint32_t ls = len - kMatchMin < 3u ? len - kMatchMin : 3u;
        uint32_t slot = d0;
        if (d0 >= 4u) {
            const uint32_t hb = 31u - (uint32_t)__builtin_clz(d0);
            slot = 2u * hb + ((d0 >> (hb - 1u)) & 1u);
        }
        tree(kPosSlot + ls * 64u, 6, slot);
        if (slot >= 4u) {
            const uint32_t fb = (slot >> 1) - 1u, base = (2u | (slot & 1u)) << fb, red = d0 - base;
            if (slot < 14u) {
                rtree(kSpecPos + base - slot - 1u, fb, red);
            } else {
                direct(red >> 4, fb - 4u);
                rtree(kAlign, 4, red & 15u);
            }
        }
        reps_push(rep, d0);
        pos += len;
        if (st && d0 != 0xFFFFFFFFu) st->matches += 1u;
    }
    NX_HD void rep_match(uint32_t i, uint32_t len) {
        const uint32_t ps = pos & ((1u << P.pb) - 1u);
        bit(kIsMatch + (state << 4) + ps, 1);
        bit(kIsRep + state, 1);
        if (i == 0u) {
            bit(kIsRepG0 + state, 0);
            bit(kIsRep0Long + (state << 4) + ps, 1);
        } else {
            bit(kIsRepG0 + state, 1);
            if (i == 1u) {
                bit(kIsRepG1 + state, 0);
            } else {
                bit(kIsRepG1 + state, 1);
                bit(kIsRepG2 + state, i - 2u);
            }
        }
        reps_use(rep, i);
        length(kRepLenCoder, len, ps);
        state = state < 7u ? 8u : 11u;
        pos += len;
        if (st) st->reps[i] += 1u;
    }
    // One packet (or the end marker, or the five flush bytes).  Sets done after the flush.
    NX_HD void step() {
        if (si < ns) {
            if (!loaded) {
                const uint64_t w = seq[si];
                run_left = (uint32_t)w & kRunMax;
                cur_len = ((uint32_t)w >> kRunBits) & 0x1FFu;
                cur_dist = (uint32_t)(w >> 32);
                loaded = true;
            }
            if (run_left) {
                literal();
                --run_left;
                return;
            }
            if (cur_len) {
                uint32_t i = 0;
                while (i < 4u && rep[i] != cur_dist - 1u) ++i;
                if (i < 4u) rep_match(i, cur_len);
                else match(cur_len, cur_dist - 1u);
            }
            ++si;
            loaded = false;
            return;
        }
        if (pos < n) {
            literal();
            return;
        }
        if (P.end_marker && !marker_done) {
            match(kMatchMin, 0xFFFFFFFFu);
            marker_done = true;
            return;
        }
        for (uint32_t i = 0; i < 5u; ++i) shift_low();
        done = true;
    }
};

// The most steps an item takes: a packet per byte at most, a sequence word without a match, the marker, the flush.
NX_HD uint64_t max_steps(uint32_t n, uint32_t ns) { return (uint64_t)n + ns + 4u; }

}  // namespace lzma
}  // namespace nx
