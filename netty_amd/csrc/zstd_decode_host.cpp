// zstd_decode_host.cpp — the host entries of the Zstandard decoder: nx_zstd_frame_info and
// nx_zstd_next_frame, the frame walkers (the second is what the nx_zstd_decoder handle runs on its
// cumulation: skippable frames and an output bound too), and nx_zstd_decode_host[_ex], a single-threaded
// decode of one frame from the functions of zstd_decode_core.hpp plus plain copy loops.  The host decoder is the CPU
// check of the format core and the GPU tests' second opinion; it is not a product path.
#include <string.h>
#include <memory>
#include <vector>
#include "../../include/netty_amd.h"
#include "zstd_decode_core.hpp"

namespace {
using namespace nx::zstdd;

struct Out {
    uint8_t* p;
    uint32_t cap, pos;
};

int32_t host_block(Tables& T, Entropy& E, std::vector<uint8_t>& lits, const uint8_t* in, uint32_t n, uint32_t block_max, Out& O) {
    LitHeader LH;
    int32_t st = parse_literals_header(in, n, block_max, &LH);
    if (st != NX_OK) return st;
    const uint8_t* body = in + LH.header_bytes;
    const uint8_t* lit = nullptr;  // Raw: the input itself
    if (LH.type == 0u) {
        lit = body;
    } else if (LH.type == 1u) {
        memset(lits.data(), body[0], LH.regen);
        lit = lits.data();
    } else {
        uint32_t tree = 0;
        if (LH.type == 2u) {
            st = huf_read_tree(T, E, body, LH.comp, &tree);
            if (st != NX_OK) return st;
        } else if (!E.huf_valid) {
            return NX_ERR_ZSTD_CORRUPT;  // Treeless with no earlier tree
        }
        HufStreams S;
        st = huf_streams(body + tree, LH.comp - tree, LH.streams, LH.regen, &S);
        if (st != NX_OK) return st;
        for (uint32_t k = 0; k < S.count; ++k) {
            st = huf_decode_stream(T.huf, E.huf_log, body + tree + S.off[k], S.len[k], lits.data() + S.out[k], S.regen[k]);
            if (st != NX_OK) return st;
        }
        lit = lits.data();
    }
    const uint8_t* sq = body + LH.comp;
    uint32_t sn = n - LH.header_bytes - LH.comp;
    SeqHeader SH;
    st = parse_sequences_header(sq, sn, &SH);
    if (st != NX_OK) return st;
    sq += SH.header_bytes;
    sn -= SH.header_bytes;
    uint32_t lit_at = 0;
    if (SH.nseq) {
        for (uint32_t w = 0; w < 3u; ++w) {
            uint32_t used = 0;
            st = seq_table(T, E, w, SH.modes[w], sq, sn, &used);
            if (st != NX_OK) return st;
            sq += used;
            sn -= used;
        }
        E.seq_valid = 1;
        SeqCursor C;
        st = seq_begin(E, C, sq, sn, SH.nseq, O.pos, LH.regen, O.cap);
        if (st != NX_OK) return st;
        Seq tile[kTile];
        while (C.left) {
            uint32_t cnt = 0;
            st = seq_decode_tile(T, E, C, tile, &cnt);
            for (uint32_t j = 0; j < cnt; ++j) {
                memcpy(O.p + O.pos, lit + lit_at, tile[j].ll);
                lit_at += tile[j].ll;
                O.pos += tile[j].ll;
                for (uint32_t k = 0; k < tile[j].ml; ++k) O.p[O.pos + k] = O.p[O.pos + k - tile[j].off];
                O.pos += tile[j].ml;
            }
            if (st != NX_OK) return st;
        }
    }
    const uint32_t rest = LH.regen - lit_at;  // the literals after the last sequence
    if (rest > O.cap - O.pos) return NX_ERR_ZSTD_OUTPUT_FULL;
    memcpy(O.p + O.pos, lit + lit_at, rest);
    O.pos += rest;
    return NX_OK;
}
}  // namespace

extern "C" int32_t nx_zstd_frame_info(const uint8_t* in, size_t n, uint64_t* frame_bytes, uint64_t* content_size, uint32_t* flags) {
    if ((!in && n) || !frame_bytes || !content_size || !flags) return NX_ERR_INVALID_ARG;
    FrameHeader H;
    int32_t st = parse_frame_header(in, n, &H);
    if (st != NX_OK) return st;
    size_t q = H.header_bytes;
    for (;;) {  // every pass consumes a block header
        BlockHeader B;
        st = parse_block_header(in + q, n - q, H.block_max, &B);
        if (st != NX_OK) return st;
        q += 3u + B.content;
        if (B.last) break;
    }
    if (H.checksum) {
        if (n - q < 4) return NX_ERR_ZSTD_TRUNCATED;
        q += 4;
    }
    *frame_bytes = q;
    *content_size = H.content_size;
    *flags = (H.single_segment ? NX_ZSTD_FRAME_SINGLE_SEGMENT : 0u) | (H.checksum ? NX_ZSTD_FRAME_CHECKSUM : 0u) |
             (H.window_descriptor << 8);
    return NX_OK;
}

extern "C" int32_t nx_zstd_next_frame(const uint8_t* in, size_t n, uint32_t* kind, uint64_t* frame_bytes, uint64_t* out_bound,
                                      uint32_t* flags) {
    if ((!in && n) || !kind || !frame_bytes || !out_bound || !flags) return NX_ERR_INVALID_ARG;
    if (n == 0) return NX_ERR_ZSTD_TRUNCATED;
    static constexpr uint8_t kSkip[4] = {0x50, 0x2A, 0x4D, 0x18};  // 0x184D2A50..5F: the low nibble is free
    bool skippable = (in[0] & 0xF0u) == kSkip[0];
    for (size_t i = 1; i < 4 && i < n && skippable; ++i) skippable = in[i] == kSkip[i];
    if (skippable) {
        if (n < 8) return NX_ERR_ZSTD_TRUNCATED;
        const uint64_t len = le_bytes(in + 4, 4);
        if (n - 8 < len) return NX_ERR_ZSTD_TRUNCATED;
        *kind = NX_ZSTD_KIND_SKIPPABLE;
        *frame_bytes = 8 + len;
        *out_bound = 0;
        *flags = 0;
        return NX_OK;
    }
    uint64_t fb = 0, cs = 0;
    uint32_t fl = 0;
    const int32_t st = nx_zstd_frame_info(in, n, &fb, &cs, &fl);
    if (st != NX_OK) return st;
    if (cs == UINT64_MAX) {  // no Frame_Content_Size: what the blocks can regenerate at most
        FrameHeader H;
        (void)parse_frame_header(in, n, &H);  // walked by nx_zstd_frame_info just now, blocks included
        cs = 0;
        for (size_t q = H.header_bytes;;) {
            BlockHeader B;
            (void)parse_block_header(in + q, n - q, H.block_max, &B);
            cs += B.type == 2u ? H.block_max : B.size;
            q += 3u + B.content;
            if (B.last) break;
        }
    }
    *kind = NX_ZSTD_KIND_FRAME;
    *frame_bytes = fb;
    *out_bound = cs;
    *flags = fl;
    return NX_OK;
}

extern "C" int32_t nx_zstd_decode_host(const uint8_t* in, size_t n, uint8_t* out, size_t out_cap, size_t* out_len, size_t* consumed) {
    return nx_zstd_decode_host_ex(in, n, out, out_cap, out_len, consumed, 0);
}

extern "C" int32_t nx_zstd_decode_host_ex(const uint8_t* in, size_t n, uint8_t* out, size_t out_cap, size_t* out_len, size_t* consumed,
                                          uint32_t flags) {
    if ((!in && n) || (!out && out_cap) || !out_len || !consumed) return NX_ERR_INVALID_ARG;
    if (flags & ~NX_ZSTD_DECODE_VERIFY_CHECKSUM) return NX_ERR_INVALID_ARG;
    *out_len = 0;
    *consumed = 0;
    FrameHeader H;
    int32_t st = parse_frame_header(in, n, &H);
    if (st != NX_OK) return st;
    if (H.checksum && !(flags & NX_ZSTD_DECODE_VERIFY_CHECKSUM)) return NX_ERR_ZSTD_CHECKSUM_UNSUPPORTED;
    std::unique_ptr<Tables> T(new Tables);
    std::vector<uint8_t> lits(kBlockMax);
    Entropy E;
    entropy_reset(E);
    Out O{out, out_cap > 0xffffffffu ? 0xffffffffu : (uint32_t)out_cap, 0};
    size_t q = H.header_bytes;
    for (;;) {
        BlockHeader B;
        st = parse_block_header(in + q, n - q, H.block_max, &B);
        if (st != NX_OK) break;
        q += 3;
        if (B.type == 2u) {
            st = host_block(*T, E, lits, in + q, B.size, H.block_max, O);
        } else if (B.size > O.cap - O.pos) {
            st = NX_ERR_ZSTD_OUTPUT_FULL;
        } else {
            if (B.type == 0u) memcpy(O.p + O.pos, in + q, B.size);
            else memset(O.p + O.pos, in[q], B.size);
            O.pos += B.size;
        }
        if (st != NX_OK) break;
        q += B.content;
        if (B.last) break;
    }
    *out_len = O.pos;
    if (st != NX_OK) return st;
    if (H.content_size != UINT64_MAX && H.content_size != O.pos) return NX_ERR_ZSTD_CORRUPT;
    if (H.checksum) {  // the low 32 bits of XXH64 of the whole content, little-endian after the last block
        if (n - q < 4) return NX_ERR_ZSTD_TRUNCATED;
        if ((uint32_t)xxh64(O.p, O.pos, 0) != le_bytes(in + q, 4)) return NX_ERR_ZSTD_CHECKSUM;
        q += 4;
    }
    *consumed = q;
    return NX_OK;
}
