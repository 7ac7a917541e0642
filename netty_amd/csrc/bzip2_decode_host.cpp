// bzip2_decode_host.cpp — the host entries of the bzip2 decoder: nx_bzip2_stream_info (what the first 14
// bytes of a stream say) and nx_bzip2_decode_host, a single-threaded decode of the first stream of the
// input from the functions of bzip2_decode_core.hpp plus plain copy loops.  The host decoder is the CPU
// check of the format core and the GPU tests' second opinion; it is not a product path.
#include <string.h>
#include <memory>
#include <vector>
#include "../../include/netty_amd.h"
#include "bzip2_decode_core.hpp"

namespace {
using namespace nx::bz2d;
constexpr uint32_t kTile = 1024;

struct CrcTable {
    uint32_t t[256];
    CrcTable() {
        for (uint32_t i = 0; i < 256u; ++i) t[i] = crc_table_entry(i);
    }
};

struct Work {
    Block B;
    uint8_t sel[kMaxSelectors];
    uint8_t lens[kMaxAlpha];
    uint32_t base[256];
    std::vector<uint8_t> bwt, pre;
    std::vector<uint32_t> tt;
};

// Stages 1-4 of a block after its magic and CRC: the pre-RLE bytes in W.pre[0, *n).
int32_t host_front(Work& W, uint32_t* n_out) {
    Block& B = W.B;
    int32_t st = block_tables(B, W.sel, W.lens);
    if (st != NX_OK) return st;
    uint8_t tile[kTile];
    for (uint32_t done = 0; !done;) {  // every tile takes a symbol of the input or ends the block
        const uint32_t at = B.len;
        uint32_t cnt = 0, run_len = 0, run_byte = 0;
        st = sym_tile(B, W.sel, tile, kTile, &cnt, &run_len, &run_byte, &done);
        if (st != NX_OK) return st;
        memcpy(W.bwt.data() + at, tile, cnt);
        memset(W.bwt.data() + at + cnt, (int)run_byte, run_len);
    }
    const uint32_t n = B.len;
    if (B.start >= n) return NX_ERR_BZIP2_START_POINTER;
    merged_pointers(B.counts, W.base, W.bwt.data(), n, W.tt.data());
    inverse_bwt_walk(W.tt.data(), n, B.start, W.pre.data());
    *n_out = n;
    return NX_OK;
}
// Stage 5: pre[0, n) through the final run-length stage to out (room: cap), *crc_out the CRC of the bytes.
int32_t host_back(const uint8_t* pre, uint32_t n, const uint32_t* T, uint8_t* out, size_t cap, size_t* produced, uint32_t* crc_out) {
    uint8_t tile[kTile];
    Rle R;
    rle_init(R);
    uint32_t crc = 0xffffffffu;
    size_t pos = 0;
    for (uint32_t i = 0; i < n;) {
        uint32_t used = 0, cnt = 0, run_len = 0, run_byte = 0;
        rle_step(R, pre + i, n - i, &used, tile, kTile, &cnt, &run_len, &run_byte);
        i += used;
        if ((size_t)cnt + run_len > cap - pos) return NX_ERR_BZIP2_OUTPUT_FULL;
        memcpy(out + pos, tile, cnt);
        memset(out + pos + cnt, (int)run_byte, run_len);
        for (uint32_t k = 0; k < cnt; ++k) crc = crc_byte(T, crc, tile[k]);
        for (uint32_t k = 0; k < run_len; ++k) crc = crc_byte(T, crc, run_byte);
        pos += (size_t)cnt + run_len;
    }
    const int32_t st = rle_end(R);
    if (st != NX_OK) return st;
    *produced = pos;
    *crc_out = ~crc;
    return NX_OK;
}
// One block after its magic and CRC: *produced bytes at out (room: cap), *crc_out their CRC.
int32_t host_block(Work& W, const uint32_t* T, uint8_t* out, size_t cap, size_t* produced, uint32_t* crc_out) {
    uint32_t n = 0;
    const int32_t st = host_front(W, &n);
    if (st != NX_OK) return st;
    return host_back(W.pre.data(), n, T, out, cap, produced, crc_out);
}

const uint32_t* crc_table() {
    static const CrcTable table;
    return table.t;
}
void work_size(Work& W, uint32_t block_size) {
    W.bwt.resize(block_size);
    W.pre.resize(block_size);
    W.tt.resize(block_size);
}
// The front of the candidate at bit `pos` of in[0, n): the magic must be the block magic.
void host_candidate(Work& W, const uint8_t* in, uint32_t n, uint64_t pos, uint32_t level, CandResult* c) {
    *c = CandResult{};
    br_init_bitpos(W.B.br, in, n, pos);
    uint32_t end = 0;
    int32_t st = block_magic(W.B.br, &end, &c->crc);
    if (st == NX_OK && end) st = NX_ERR_BZIP2_BLOCK_HEADER;
    if (st == NX_OK) {
        W.B.crc = c->crc;
        W.B.block_size = level * kBaseBlock;
        st = host_front(W, &c->pre_len);
    }
    c->status = st;
    if (st != NX_OK) return;
    c->end_bit = br_bitpos(W.B.br);
    Rle R;
    rle_init(R);
    c->final_len = rle_length(R, W.pre.data(), c->pre_len);
}
// Every magic of in[0, n) in position order, the kind flag in bit 63.
void host_scan(const uint8_t* in, uint32_t n, std::vector<uint64_t>& pos) {
    for (uint64_t b0 = 0; b0 < n; b0 += kScanWindow) {
        uint64_t blk = 0, end = 0;
        scan_window(in, n, b0, &blk, &end);
        for (uint64_t m = blk | end; m != 0u; m &= m - 1u) {
            const uint32_t k = (uint32_t)__builtin_ctzll(m);
            pos.push_back((8u * b0 + k) | ((end >> k) & 1u ? kCandEnd : 0u));
        }
    }
}
}  // namespace

extern "C" int32_t nx_bzip2_stream_info(const uint8_t* in, size_t n, uint32_t* level, uint32_t* first_block_crc, uint32_t* is_empty) {
    if ((!in && n) || !level || !first_block_crc || !is_empty) return NX_ERR_INVALID_ARG;
    if (n < 14) return NX_ERR_BZIP2_TRUNCATED;
    uint32_t lv = 0;
    int32_t st = stream_header(in, 14, &lv);
    if (st != NX_OK) return st;
    BitReader r;
    br_init(r, in, 14, 4);
    uint32_t end = 0, crc = 0;
    st = block_magic(r, &end, &crc);
    if (st != NX_OK) return st;
    *level = lv;
    *first_block_crc = end ? 0u : crc;
    *is_empty = end;
    return NX_OK;
}

extern "C" int32_t nx_bzip2_decode_host(const uint8_t* in, size_t n, uint8_t* out, size_t out_cap, size_t* out_len, size_t* consumed) {
    if ((!in && n) || (!out && out_cap) || !out_len || !consumed) return NX_ERR_INVALID_ARG;
    *out_len = 0;
    *consumed = 0;
    const uint32_t* table = crc_table();
    const uint32_t n32 = n > 0xffffffffu ? 0xffffffffu : (uint32_t)n;
    const size_t cap = out_cap > 0xffffffffu ? 0xffffffffu : out_cap;
    uint32_t level = 0;
    int32_t st = stream_header(in, n32, &level);
    if (st != NX_OK) return st;
    std::unique_ptr<Work> W(new Work);
    const uint32_t block_size = level * kBaseBlock;
    work_size(*W, block_size);
    br_init(W->B.br, in, n32, 4);
    uint32_t stream_crc = 0;
    size_t pos = 0;
    for (;;) {  // every pass consumes a block of the input
        uint32_t end = 0, crc = 0;
        st = block_magic(W->B.br, &end, &crc);
        if (st != NX_OK) return st;
        if (end) {
            if (crc != stream_crc) return NX_ERR_BZIP2_STREAM_CRC;
            *consumed = W->B.br.at;  // the combined CRC's last byte holds the padding
            return NX_OK;
        }
        W->B.crc = crc;
        W->B.block_size = block_size;
        size_t produced = 0;
        uint32_t got = 0;
        st = host_block(*W, table, out + pos, cap - pos, &produced, &got);
        if (st != NX_OK) return st;
        if (got != crc) return NX_ERR_BZIP2_BLOCK_CRC;
        stream_crc = crc_combine_stream(stream_crc, got);
        pos += produced;
        *out_len = pos;
    }
}

extern "C" int32_t nx_bzip2_scan_host(const uint8_t* in, size_t n, uint64_t* positions, size_t cap, size_t* count) {
    if ((!in && n) || (!positions && cap) || !count) return NX_ERR_INVALID_ARG;
    std::vector<uint64_t> pos;
    host_scan(in, n > 0xffffffffu ? 0xffffffffu : (uint32_t)n, pos);
    for (size_t k = 0; k < pos.size() && k < cap; ++k) positions[k] = pos[k];
    *count = pos.size();
    return NX_OK;
}

extern "C" int32_t nx_bzip2_decode_block_host(const uint8_t* in, size_t n, uint64_t bit_pos, int32_t level, uint8_t* out, size_t out_cap,
                                              nx_bzip2_block_info* info) {
    if ((!in && n) || (!out && out_cap) || !info || level < 1 || level > 9) return NX_ERR_INVALID_ARG;
    *info = nx_bzip2_block_info{};
    const uint32_t n32 = n > 0xffffffffu ? 0xffffffffu : (uint32_t)n;
    std::unique_ptr<Work> W(new Work);
    work_size(*W, (uint32_t)level * kBaseBlock);
    CandResult c;
    host_candidate(*W, in, n32, bit_pos, (uint32_t)level, &c);
    info->stored_crc = c.crc;
    if (c.status != NX_OK) return info->status = c.status;
    info->end_bit = c.end_bit;
    info->pre_len = c.pre_len;
    info->final_len = c.final_len;
    size_t produced = 0;
    info->status = host_back(W->pre.data(), c.pre_len, crc_table(), out, out_cap, &produced, &info->computed_crc);
    if (info->status == NX_OK && info->computed_crc != c.crc) info->status = NX_ERR_BZIP2_BLOCK_CRC;
    return info->status;
}

extern "C" int32_t nx_bzip2_decode_split_host(const uint8_t* in, size_t n, uint8_t* out, size_t out_cap, size_t* out_len, size_t* consumed,
                                              size_t max_blocks, size_t* blocks) {
    if ((!in && n) || (!out && out_cap) || !out_len || !consumed) return NX_ERR_INVALID_ARG;
    *out_len = 0;
    *consumed = 0;
    if (blocks) *blocks = 0;
    const uint32_t n32 = n > 0xffffffffu ? 0xffffffffu : (uint32_t)n;
    const uint32_t cap = out_cap > 0xffffffffu ? 0xffffffffu : (uint32_t)out_cap;
    std::vector<uint64_t> pos;
    host_scan(in, n32, pos);
    if (pos.size() > max_blocks) return NX_ERR_BZIP2_DECODE_BLOCKS;
    const uint32_t count = (uint32_t)pos.size();
    SplitItem I;
    split_begin(I, in, n32);
    std::vector<CandResult> res(count);
    std::vector<std::vector<uint8_t>> pre(count);  // a slot each: the candidates' pre-RLE bytes
    if (I.status == kChainOpen) {
        std::unique_ptr<Work> W(new Work);
        work_size(*W, I.level * kBaseBlock);
        for (uint32_t k = 0; k < count; ++k) {  // front
            if (pos[k] & kCandEnd) continue;
            host_candidate(*W, in, n32, pos[k] & kCandPos, I.level, &res[k]);
            if (res[k].status == NX_OK) pre[k].assign(W->pre.begin(), W->pre.begin() + res[k].pre_len);
        }
        split_stitch(I, in, n32, cap, pos.data(), res.data(), count, count);
        for (uint32_t k = 0; k < count; ++k) {  // back
            if (!res[k].member) continue;
            size_t produced = 0;
            res[k].back_status = host_back(pre[k].data(), res[k].pre_len, crc_table(), out + res[k].off, cap - res[k].off, &produced, &res[k].crc_got);
            if (res[k].back_status == NX_OK && res[k].crc_got != res[k].crc) res[k].back_status = NX_ERR_BZIP2_BLOCK_CRC;
        }
    }
    int32_t st = NX_OK;
    uint32_t ol = 0, cs = 0, nb = 0;
    split_finish(I, res.data(), count, &st, &ol, &cs, &nb);
    *out_len = ol;
    *consumed = cs;
    if (blocks) *blocks = nb;
    return st;
}
