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

// One block after its magic and CRC: *produced bytes at out (room: cap), *crc_out their CRC.
int32_t host_block(Work& W, const uint32_t* T, uint8_t* out, size_t cap, size_t* produced, uint32_t* crc_out) {
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
    Rle R;
    rle_init(R);
    uint32_t crc = 0xffffffffu;
    size_t pos = 0;
    for (uint32_t i = 0; i < n;) {
        uint32_t used = 0, cnt = 0, run_len = 0, run_byte = 0;
        rle_step(R, W.pre.data() + i, n - i, &used, tile, kTile, &cnt, &run_len, &run_byte);
        i += used;
        if ((size_t)cnt + run_len > cap - pos) return NX_ERR_BZIP2_OUTPUT_FULL;
        memcpy(out + pos, tile, cnt);
        memset(out + pos + cnt, (int)run_byte, run_len);
        for (uint32_t k = 0; k < cnt; ++k) crc = crc_byte(T, crc, tile[k]);
        for (uint32_t k = 0; k < run_len; ++k) crc = crc_byte(T, crc, run_byte);
        pos += (size_t)cnt + run_len;
    }
    st = rle_end(R);
    if (st != NX_OK) return st;
    *produced = pos;
    *crc_out = ~crc;
    return NX_OK;
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
    static const CrcTable table;
    const uint32_t n32 = n > 0xffffffffu ? 0xffffffffu : (uint32_t)n;
    const size_t cap = out_cap > 0xffffffffu ? 0xffffffffu : out_cap;
    uint32_t level = 0;
    int32_t st = stream_header(in, n32, &level);
    if (st != NX_OK) return st;
    std::unique_ptr<Work> W(new Work);
    const uint32_t block_size = level * kBaseBlock;
    W->bwt.resize(block_size);
    W->pre.resize(block_size);
    W->tt.resize(block_size);
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
        st = host_block(*W, table.t, out + pos, cap - pos, &produced, &got);
        if (st != NX_OK) return st;
        if (got != crc) return NX_ERR_BZIP2_BLOCK_CRC;
        stream_crc = crc_combine_stream(stream_crc, got);
        pos += produced;
        *out_len = pos;
    }
}
