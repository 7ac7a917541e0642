// bzip2_encode_host.cpp — the host entries of the bzip2 encoder: nx_bzip2_max_compressed_length and
// nx_bzip2_encode_host, a single-threaded encode of one item (one encode(in) followed by close() of
// Bzip2Encoder.java) from the functions of bzip2_encode_core.hpp plus a serial rotation sort.  The host encoder
// is the CPU check of the format core and the GPU tests' second opinion; it is not a product path.  Beside it
// the host forms of the split path (nx_bzip2_encode_batch_split): nx_bzip2_blocks_bound, the planner
// (nx_bzip2_plan_host, nx_bzip2_plan_resume_host) and nx_bzip2_encode_segment_host, which encodes a segment's
// blocks one after another behind the carried bits, the way the one-shot encoder does behind the header.
//
// The sort is the one the kernel runs, one element at a time: prefix doubling over the cyclic rotations, each
// round a stable least-significant-digit radix sort by the rank of the first half over a list that is already
// in the order of the second half, then, where rotations are equal (ranks still tied once the compared length
// reaches the block length), a last sort of the indices 0..n-1 by rank, which leaves equal rotations in index order.
#include <string.h>
#include <memory>
#include <vector>
#include "../../include/netty_amd.h"
#include "bzip2_encode_core.hpp"

namespace {
using namespace nx::bz2e;

struct CrcTable {
    uint32_t t[256];
    CrcTable() {
        for (uint32_t i = 0; i < 256u; ++i) t[i] = nx::bz2d::crc_table_entry(i);
    }
};

struct Work {
    Rle1 R;
    Mtf2 M;
    uint8_t lens[kMaxTables][kMaxAlpha];
    uint32_t codes[kMaxTables][kMaxAlpha];
    uint32_t tfreq[kMaxTables][kMaxAlpha];
    int32_t merged[kMaxAlpha], sorted[kMaxAlpha];
    std::vector<uint8_t> block, bwt, sel;
    std::vector<uint32_t> la, lb, ra, rb, stg;
    std::vector<uint16_t> mtf;
};

// dst = src in the order of (key[src[j]] >> shift) & 255, stable
void radix_pass(const uint32_t* src, uint32_t* dst, const uint32_t* key, uint32_t shift, uint32_t n) {
    uint32_t base[257] = {0};
    for (uint32_t j = 0; j < n; ++j) base[((key[src[j]] >> shift) & 255u) + 1u] += 1u;
    for (uint32_t d = 0; d < 256u; ++d) base[d + 1] += base[d];
    for (uint32_t j = 0; j < n; ++j) dst[base[(key[src[j]] >> shift) & 255u]++] = src[j];
}
// the list in *src sorted by key (below 2^(8 * passes)); the result is in *src again
void sort_by_key(uint32_t** src, uint32_t** dst, const uint32_t* key, uint32_t passes, uint32_t n) {
    for (uint32_t p = 0; p < passes; ++p) {
        radix_pass(*src, *dst, key, 8u * p, n);
        std::swap(*src, *dst);
    }
}
// nr[sa[j]] = the first place of sa[j]'s group (equal key, and with h equal key at distance h): the groups counted
uint32_t rerank(const uint32_t* sa, const uint32_t* key, uint32_t* nr, uint32_t h, uint32_t n) {
    uint32_t groups = 0, head = 0;
    for (uint32_t j = 0; j < n; ++j) {
        const uint32_t a = sa[j], b = j ? sa[j - 1] : 0u;
        if (j == 0u || key[a] != key[b] || (h && key[(a + h) % n] != key[(b + h) % n])) {
            head = j;
            groups += 1u;
        }
        nr[a] = head;
    }
    return groups;
}
// W.bwt = the last column of the block's sorted rotations; returns the row of rotation 0
uint32_t host_bwt(Work& W, uint32_t n) {
    const uint8_t* b = W.block.data();
    uint32_t *src = W.la.data(), *dst = W.lb.data(), *rk = W.ra.data(), *nr = W.rb.data();
    const uint32_t passes = n <= 256u ? 1u : n <= 65536u ? 2u : 3u;
    for (uint32_t i = 0; i < n; ++i) {
        src[i] = i;
        rk[i] = ((uint32_t)b[i] << 8) | b[(i + 1u) % n];
    }
    sort_by_key(&src, &dst, rk, 2, n);
    uint32_t groups = rerank(src, rk, nr, 0, n);
    std::swap(rk, nr);
    for (uint32_t h = 2; groups < n && h < n; h *= 2u) {  // at most ceil(log2 n) rounds
        for (uint32_t j = 0; j < n; ++j) dst[j] = (src[j] + n - h) % n;
        std::swap(src, dst);
        sort_by_key(&src, &dst, rk, passes, n);
        groups = rerank(src, rk, nr, h, n);
        std::swap(rk, nr);
    }
    if (groups < n) {  // equal rotations: by index
        for (uint32_t i = 0; i < n; ++i) src[i] = i;
        sort_by_key(&src, &dst, rk, passes, n);
    }
    uint32_t start = 0;
    for (uint32_t j = 0; j < n; ++j) {
        W.bwt[j] = b[(src[j] + n - 1u) % n];
        if (src[j] == 0u) start = j;
    }
    return start;
}

// The Huffman stage of Bzip2HuffmanStageEncoder.encode up to the codes; returns the table count.
uint32_t host_tables(Work& W, uint32_t mtf_len, uint32_t alpha) {
    const uint32_t tables = select_table_count(mtf_len), groups = (mtf_len + kGroup - 1u) / kGroup;
    huffman_seeds(W.lens, W.M.freq, alpha, mtf_len, tables);
    for (uint32_t pass = 0; pass < kPasses; ++pass) {
        memset(W.tfreq, 0, sizeof(W.tfreq));
        for (uint32_t g = 0; g < groups; ++g) {
            const uint32_t s = g * kGroup, cnt = mtf_len - s < kGroup ? mtf_len - s : kGroup;
            const uint32_t best = group_best_table(W.lens, W.mtf.data() + s, cnt, tables);
            for (uint32_t i = 0; i < cnt; ++i) W.tfreq[best][W.mtf[s + i]] += 1u;
            W.sel[g] = (uint8_t)best;  // the last pass's stay
        }
        for (uint32_t t = 0; t < tables; ++t) {
            for (uint32_t k = 0; k < alpha; ++k) lengths_sort_one(W.tfreq[t], alpha, k, W.merged, W.sorted);
            ha_allocate(W.sorted, (int32_t)alpha, (int32_t)kEncMaxCodeLen);
            for (uint32_t i = 0; i < alpha; ++i) lengths_unsort_one(W.merged, W.sorted, i, W.lens[t]);
        }
    }
    for (uint32_t t = 0; t < tables; ++t) assign_codes(W.lens[t], alpha, W.codes[t]);
    return tables;
}

struct Out {
    uint8_t* p;
    size_t cap, pos;
    uint32_t carry, carry_n;  // the bits of the last, incomplete byte
    bool head;                // the stream header is still to be written
};
// the writer of the next piece of the stream over the zeroed staging words: the header or the carried bits first
void begin_piece(Work& W, Out& O, BitWriter& b, size_t words, uint32_t level) {
    memset(W.stg.data(), 0, words * 4u);
    bw_init(b, W.stg.data(), 0);
    if (O.head) {
        bw_put(b, 24, 0x425a68u);  // "BZh" (Bzip2Encoder.java:115-117)
        bw_put(b, 8, '0' + level);
        O.head = false;
    }
    bw_put(b, O.carry_n, O.carry);
}
// the whole bytes of `bits` staged bits to the output (all of them, zero-padded, when last); the rest is carried
int32_t end_piece(Work& W, Out& O, uint64_t bits, bool last) {
    const uint8_t* s = reinterpret_cast<const uint8_t*>(W.stg.data());
    const size_t bytes = last ? (size_t)((bits + 7u) / 8u) : (size_t)(bits / 8u);
    if (bytes > O.cap - O.pos) return NX_ERR_BZIP2_ENCODE_FULL;
    memcpy(O.p + O.pos, s, bytes);
    O.pos += bytes;
    O.carry_n = last ? 0u : (uint32_t)(bits & 7u);
    O.carry = O.carry_n ? (uint32_t)s[bytes] >> (8u - O.carry_n) : 0u;
    return NX_OK;
}

// Bzip2BlockCompressor.close for the filled block
int32_t host_block(Work& W, Out& O, const uint32_t* T, uint32_t level, uint32_t* crc_out) {
    rle1_close(W.R, W.block.data(), T);
    const uint32_t n = W.R.len, crc = ~W.R.crc;
    const uint32_t start = host_bwt(W, n);
    mtf2_init(W.M, W.R.present);
    mtf2_step(W.M, W.bwt.data(), n, W.mtf.data());
    const uint32_t mtf_len = mtf2_finish(W.M, W.mtf.data()), alpha = W.M.eob + 1u;
    const uint32_t tables = host_tables(W, mtf_len, alpha), groups = (mtf_len + kGroup - 1u) / kGroup;
    BitWriter b;
    begin_piece(W, O, b, (size_t)((block_bits_bound(n) + 40u) / 32u + 2u), level);
    write_block_head(b, crc, start, W.R.present, tables, W.sel.data(), groups, W.lens, alpha);
    emit_groups(&b, W.mtf.data(), mtf_len, W.sel.data(), W.codes, 0, groups);
    bw_flush(b);
    *crc_out = crc;
    return end_piece(W, O, bw_bits(b), false);
}
}  // namespace

extern "C" size_t nx_bzip2_max_compressed_length(size_t n, int32_t level) {
    if (level < 1 || level > 9) return 0;
    return (size_t)stream_bytes_bound(n, (uint32_t)level);
}

namespace {
// The blocks of in[0, n) behind what O carries (the stream header, or the bits of an earlier segment), then with
// `last` the footer and the padding; *stream_crc is folded in block order.
int32_t host_stream(const uint8_t* in, size_t n, uint32_t level, Out& O, uint32_t* stream_crc, bool last) {
    static const CrcTable table;
    const uint32_t S = level * kBaseBlock;
    std::unique_ptr<Work> W(new Work);
    const size_t room = n < S ? n + n / 4u + 8u : S + 8u;  // a block holds at most S bytes, and at most 5/4 of the item
    W->block.resize(room);
    W->bwt.resize(room);
    W->mtf.resize(room + 1u);
    W->sel.resize(room / kGroup + 2u);
    W->la.resize(room);
    W->lb.resize(room);
    W->ra.resize(room);
    W->rb.resize(room);
    W->stg.resize((size_t)((block_bits_bound(room) + 40u) / 32u + 2u));
    rle1_init(W->R, S);
    for (size_t i = 0; i <= n;) {  // Bzip2Encoder.java:112-148, then finishEncode's closeBlock at i == n
        if (i < n && rle1_write(W->R, W->block.data(), table.t, in[i])) {
            i += 1u;
            continue;
        }
        if (!rle1_empty(W->R)) {  // Bzip2Encoder.java:154-161 closeBlock
            uint32_t crc = 0;
            const int32_t st = host_block(*W, O, table.t, level, &crc);
            if (st != NX_OK) return st;
            *stream_crc = nx::bz2d::crc_combine_stream(*stream_crc, crc);
            rle1_init(W->R, S);
        }
        if (i == n) break;
    }
    if (!last) return NX_OK;
    BitWriter b;  // Bzip2Encoder.java:220-223
    begin_piece(*W, O, b, 8, level);
    bw_put(b, 24, nx::bz2d::kEndMagicHi);
    bw_put(b, 24, nx::bz2d::kEndMagicLo);
    bw_put(b, 32, *stream_crc);
    bw_flush(b);
    return end_piece(*W, O, bw_bits(b), true);
}
}  // namespace

extern "C" int32_t nx_bzip2_encode_host(const uint8_t* in, size_t n, int32_t level, uint8_t* out, size_t out_cap, size_t* out_len) {
    if ((!in && n) || (!out && out_cap) || !out_len) return NX_ERR_INVALID_ARG;
    *out_len = 0;
    if (level < 1 || level > 9) return NX_ERR_BZIP2_LEVEL;  // Bzip2Encoder.java:98-101
    Out O = {out, out_cap, 0, 0, 0, true};
    uint32_t stream_crc = 0;
    const int32_t st = host_stream(in, n, (uint32_t)level, O, &stream_crc, true);
    if (st != NX_OK) return st;
    *out_len = O.pos;
    return NX_OK;
}

extern "C" size_t nx_bzip2_blocks_bound(size_t n, int32_t level) {
    if (level < 1 || level > 9) return 0;
    return (size_t)blocks_bound(n, (uint32_t)level);
}

extern "C" int32_t nx_bzip2_plan_resume_host(const uint8_t* in, size_t n, int32_t level, uint32_t state[3], int32_t close, uint64_t* cuts,
                                             size_t cap, size_t* count) {
    if ((!in && n) || (!cuts && cap) || !count || !state) return NX_ERR_INVALID_ARG;
    *count = 0;
    if (level < 1 || level > 9) return NX_ERR_BZIP2_LEVEL;
    Plan P = {state[0], state[1], state[2]};
    uint64_t c = 0;
    plan_range(P, (uint32_t)level * kBaseBlock - 6u, in, n, close != 0, 0, cuts, cap, &c);
    state[0] = P.len;
    state[1] = P.run;
    state[2] = P.cur;
    *count = (size_t)c;
    return NX_OK;
}

extern "C" int32_t nx_bzip2_plan_host(const uint8_t* in, size_t n, int32_t level, uint64_t* cuts, size_t cap, size_t* count) {
    uint32_t state[3] = {0, 0, 0};
    return nx_bzip2_plan_resume_host(in, n, level, state, 1, cuts, cap, count);
}

extern "C" int32_t nx_bzip2_encode_segment_host(const uint8_t* in, size_t n, int32_t level, nx_bzip2_seg* seg, uint8_t* out, size_t out_cap,
                                                size_t* out_len) {
    if ((!in && n) || (!out && out_cap) || !out_len || !seg) return NX_ERR_INVALID_ARG;
    *out_len = 0;
    if (level < 1 || level > 9) return NX_ERR_BZIP2_LEVEL;
    const bool first = seg->flags & NX_BZIP2_SEG_FIRST, last = seg->flags & NX_BZIP2_SEG_LAST;
    if (!first && seg->carry_count >= 32u) return NX_ERR_INVALID_ARG;
    // the segment goes to a buffer of its own: without LAST up to three whole bytes are held back as carry
    std::vector<uint8_t> buf(stream_bytes_bound(n, (uint32_t)level) + 8u);
    Out O = {buf.data(), buf.size(), 0, first ? 0u : seg->carry_bits, first ? 0u : seg->carry_count, first};
    uint32_t crc = first ? 0u : seg->crc;
    const int32_t st = host_stream(in, n, (uint32_t)level, O, &crc, last);
    if (st != NX_OK) return st;
    if (!last && O.head) {  // no block: the header is still to be written
        buf[0] = 'B', buf[1] = 'Z', buf[2] = 'h', buf[3] = (uint8_t)('0' + level);
        O.pos = 4;
    }
    const size_t emit = last ? O.pos : O.pos / 4u * 4u;  // Bzip2BitWriter.java:41-56 hands over whole 32-bit words
    if (emit > out_cap) return NX_ERR_BZIP2_ENCODE_FULL;
    if (emit) memcpy(out, buf.data(), emit);
    uint32_t carry = 0;
    for (size_t k = emit; k < O.pos; ++k) carry = (carry << 8) | buf[k];
    seg->carry_bits = last ? 0u : (carry << O.carry_n) | O.carry;
    seg->carry_count = last ? 0u : (uint32_t)(O.pos - emit) * 8u + O.carry_n;
    seg->crc = crc;
    *out_len = emit;
    return NX_OK;
}
