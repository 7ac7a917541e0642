// zstd_decode_core.hpp — the format logic of the Zstandard decoder (RFC 8878), written once for the
// host and the device: frame, block and literals headers, the FSE distribution reader and table
// build, the Huffman tree description, the backward bit reader, the sequence step and XXH64 (the
// content checksum).  Plain serial functions (XXH64 in pieces, for the kernel to spread over lanes):
// no wave intrinsics, no LDS keywords; tables come in as pointers (the kernel hands in LDS,
// the host decoder a heap block).  zstd_decode.hip runs them on one lane of a frame's wave and adds the
// wave-wide copies; zstd_decode_host.cpp runs them on the CPU, where the tests hold them against libzstd.
//
// Nothing is assumed about the input: every loop is bounded by an input length, an output capacity or
// a format constant, and every read is bounded by the section it belongs to.  Errors are the
// NX_ERR_ZSTD_* codes of netty_amd_status.h; the checks follow libzstd's (zstd_decompress.c,
// zstd_decompress_block.c, huf_decompress.c, entropy_common.c of zstd 1.5).
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "../../include/netty_amd_status.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NX_HD __host__ __device__ inline
#else
#define NX_HD inline
#endif

namespace nx {
namespace zstdd {

constexpr uint32_t kMagic = 0xFD2FB528u;
constexpr uint64_t kMaxWindow = 128ull << 20;  // window and content size cap: positions stay in 32 bits
constexpr uint32_t kBlockMax = 128u << 10;
constexpr uint32_t kLlMaxLog = 9, kOfMaxLog = 8, kMlMaxLog = 9, kHwMaxLog = 6, kHufMaxLog = 11;
constexpr uint32_t kLlSyms = 36, kOfSyms = 32, kMlSyms = 53;
constexpr uint32_t kTile = 64;  // sequences decoded per tile

struct FseEntry {
    uint16_t base;  // baseline of the next state
    uint8_t sym;
    uint8_t nbits;
};
struct HufEntry {
    uint8_t sym;
    uint8_t nbits;
};
// Everything a frame's decode keeps in fast memory: the three sequence tables and the Huffman table
// (persist across blocks), and the scratch of the table builds.
struct Tables {
    FseEntry ll[1u << kLlMaxLog];
    FseEntry of[1u << kOfMaxLog];
    FseEntry ml[1u << kMlMaxLog];
    FseEntry hw[1u << kHwMaxLog];  // the FSE code of a tree description's weights
    HufEntry huf[1u << kHufMaxLog];
    int16_t norm[256];
    uint16_t next[256];
    uint8_t weights[256];
    uint32_t rank[16];
};
// what persists across a frame's blocks beside the tables
struct Entropy {
    uint32_t ll_log, of_log, ml_log, huf_log;
    uint32_t seq_valid, huf_valid;  // a Repeat_Mode / Treeless block has a predecessor
    uint32_t rep[3];
};
NX_HD void entropy_reset(Entropy& E) {
    E.ll_log = E.of_log = E.ml_log = E.huf_log = 0;
    E.seq_valid = E.huf_valid = 0;
    E.rep[0] = 1;
    E.rep[1] = 4;
    E.rep[2] = 8;
}

NX_HD uint32_t highbit(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); }  // v != 0
NX_HD uint32_t le_bytes(const uint8_t* p, uint32_t n) {
    uint32_t v = 0;
    for (uint32_t i = 0; i < n; ++i) v |= (uint32_t)p[i] << (8u * i);
    return v;
}

// ---- XXH64 (the content checksum: its low 32 bits, seed 0, little-endian after the last block) ----
// Four accumulators run over the 32-byte stripes, accumulator k over bytes [8k, 8k + 8) of each; they are
// merged, the length is added, the last len % 32 bytes go in by 8-, 4- and 1-byte steps, then the
// avalanche.  In pieces, so that the kernel can keep one accumulator per lane and read its own output
// through its own loads; xxh64() below is the whole of it over plain memory.
constexpr uint64_t kXxP1 = 0x9E3779B185EBCA87ull, kXxP2 = 0xC2B2AE3D27D4EB4Full, kXxP3 = 0x165667B19E3779F9ull,
                   kXxP4 = 0x85EBCA77C2B2AE63ull, kXxP5 = 0x27D4EB2F165667C5ull;
NX_HD uint64_t xx_rotl(uint64_t v, uint32_t r) { return (v << r) | (v >> (64u - r)); }
NX_HD uint64_t xxh64_acc_init(uint32_t k, uint64_t seed) {  // accumulator k of 4
    return k == 0u ? seed + kXxP1 + kXxP2 : k == 1u ? seed + kXxP2 : k == 2u ? seed : seed - kXxP1;
}
NX_HD uint64_t xxh64_round(uint64_t acc, uint64_t v) { return xx_rotl(acc + v * kXxP2, 31) * kXxP1; }
// acc[4] after the len / 32 stripes (unused when len < 32); tail(i) = byte i of the last len % 32 bytes
template <class Tail>
NX_HD uint64_t xxh64_finish(const uint64_t* acc, uint64_t len, uint64_t seed, Tail tail) {
    uint64_t h;
    if (len >= 32u) {
        h = xx_rotl(acc[0], 1) + xx_rotl(acc[1], 7) + xx_rotl(acc[2], 12) + xx_rotl(acc[3], 18);
        for (uint32_t k = 0; k < 4u; ++k) h = (h ^ xxh64_round(0, acc[k])) * kXxP1 + kXxP4;
    } else {
        h = seed + kXxP5;
    }
    h += len;
    const uint32_t rest = (uint32_t)(len & 31u);
    uint32_t i = 0;
    for (; i + 8u <= rest; i += 8u) {
        uint64_t v = 0;
        for (uint32_t b = 0; b < 8u; ++b) v |= (uint64_t)tail(i + b) << (8u * b);
        h = xx_rotl(h ^ xxh64_round(0, v), 27) * kXxP1 + kXxP4;
    }
    if (i + 4u <= rest) {
        uint64_t v = 0;
        for (uint32_t b = 0; b < 4u; ++b) v |= (uint64_t)tail(i + b) << (8u * b);
        h = xx_rotl(h ^ v * kXxP1, 23) * kXxP2 + kXxP3;
        i += 4u;
    }
    for (; i < rest; ++i) h = xx_rotl(h ^ (uint64_t)tail(i) * kXxP5, 11) * kXxP1;
    h = (h ^ (h >> 33)) * kXxP2;
    h = (h ^ (h >> 29)) * kXxP3;
    return h ^ (h >> 32);
}
NX_HD uint64_t xxh64(const uint8_t* p, size_t n, uint64_t seed) {
    uint64_t acc[4];
    for (uint32_t k = 0; k < 4u; ++k) acc[k] = xxh64_acc_init(k, seed);
    const size_t stripes = n >> 5;
    for (size_t s = 0; s < stripes; ++s)
        for (uint32_t k = 0; k < 4u; ++k) {
            uint64_t v = 0;
            for (uint32_t b = 0; b < 8u; ++b) v |= (uint64_t)p[32u * s + 8u * k + b] << (8u * b);
            acc[k] = xxh64_round(acc[k], v);
        }
    const uint8_t* t = p + 32u * stripes;
    return xxh64_finish(acc, n, seed, [t](uint32_t i) -> uint32_t { return t[i]; });
}

// ---- frame header ----
struct FrameHeader {
    uint32_t header_bytes;
    uint32_t single_segment, checksum, window_descriptor;
    uint32_t dict_id;
    uint64_t content_size;  // UINT64_MAX when absent
    uint64_t window_size;
    uint32_t block_max;
};
// NX_OK, NX_ERR_ZSTD_TRUNCATED when [in, in + n) ends inside the header, or the header's error.  The
// Content_Checksum flag is reported, not refused: the walkers count its four bytes, the decoders verify
// it or, through the entry points without NX_ZSTD_DECODE_VERIFY_CHECKSUM, refuse the frame.
NX_HD int32_t parse_frame_header(const uint8_t* in, size_t n, FrameHeader* H) {
    for (uint32_t i = 0; i < 4u && i < n; ++i)
        if (in[i] != (uint8_t)(kMagic >> (8u * i))) return NX_ERR_ZSTD_MAGIC;
    if (n < 5) return NX_ERR_ZSTD_TRUNCATED;
    const uint32_t d = in[4];
    const uint32_t single = (d >> 5) & 1u, dn = (d & 3u) == 3u ? 4u : (d & 3u);
    const uint32_t fcs_code = d >> 6;
    const uint32_t fn = fcs_code == 0u ? single : fcs_code == 1u ? 2u : fcs_code == 2u ? 4u : 8u;
    if (d & 0x08u) return NX_ERR_ZSTD_CORRUPT;  // the reserved bit
    const uint32_t hb = 5u + (single ? 0u : 1u) + dn + fn;
    if (n < hb) return NX_ERR_ZSTD_TRUNCATED;
    uint32_t q = 5;
    H->window_descriptor = 0;
    H->window_size = 0;
    if (!single) {
        const uint32_t wd = in[q++];
        const uint64_t base = 1ull << (10u + (wd >> 3));
        H->window_descriptor = wd;
        H->window_size = base + (base >> 3) * (wd & 7u);
    }
    H->dict_id = le_bytes(in + q, dn);
    q += dn;
    H->content_size = UINT64_MAX;
    if (fn) {
        uint64_t v = 0;
        for (uint32_t i = 0; i < fn; ++i) v |= (uint64_t)in[q + i] << (8u * i);
        H->content_size = v + (fn == 2u ? 256u : 0u);
        q += fn;
    }
    if (single) H->window_size = H->content_size;
    H->header_bytes = hb;
    H->single_segment = single;
    H->checksum = (d >> 2) & 1u;
    if (H->dict_id != 0u) return NX_ERR_ZSTD_DICTIONARY;
    if (H->window_size > kMaxWindow || (fn && H->content_size > kMaxWindow)) return NX_ERR_ZSTD_WINDOW;
    H->block_max = H->window_size < kBlockMax ? (uint32_t)H->window_size : kBlockMax;
    return NX_OK;
}

// ---- block header ----
struct BlockHeader {
    uint32_t last, type, size;
    uint32_t content;  // bytes after the header: size, or 1 for an RLE block
};
NX_HD int32_t parse_block_header(const uint8_t* in, size_t n, uint32_t block_max, BlockHeader* B) {
    if (n < 3) return NX_ERR_ZSTD_TRUNCATED;
    const uint32_t h = le_bytes(in, 3);
    B->last = h & 1u;
    B->type = (h >> 1) & 3u;
    B->size = h >> 3;
    if (B->type == 3u) return NX_ERR_ZSTD_CORRUPT;
    if (B->size > block_max) return NX_ERR_ZSTD_CORRUPT;
    B->content = B->type == 1u ? 1u : B->size;
    if (n - 3 < B->content) return NX_ERR_ZSTD_TRUNCATED;
    return NX_OK;
}

// ---- literals section header ----
struct LitHeader {
    uint32_t type;  // 0 Raw, 1 RLE, 2 Compressed, 3 Treeless
    uint32_t header_bytes, regen, comp, streams;
};
// in[0, n): the block's content.  comp = bytes after the header (Raw: regen, RLE: 1).
NX_HD int32_t parse_literals_header(const uint8_t* in, uint32_t n, uint32_t block_max, LitHeader* L) {
    if (n < 1u) return NX_ERR_ZSTD_CORRUPT;
    const uint32_t b0 = in[0], type = b0 & 3u, fmt = (b0 >> 2) & 3u;
    L->type = type;
    if (type < 2u) {
        const uint32_t h = fmt == 1u ? 2u : fmt == 3u ? 3u : 1u;
        if (n < h) return NX_ERR_ZSTD_CORRUPT;
        const uint32_t v = le_bytes(in, h);
        L->regen = h == 1u ? v >> 3 : v >> 4;
        L->comp = type == 0u ? L->regen : 1u;
        L->streams = 0;
        L->header_bytes = h;
    } else {
        const uint32_t h = fmt < 2u ? 3u : fmt == 2u ? 4u : 5u, bits = fmt < 2u ? 10u : fmt == 2u ? 14u : 18u;
        if (n < h) return NX_ERR_ZSTD_CORRUPT;
        uint64_t v = 0;
        for (uint32_t i = 0; i < h; ++i) v |= (uint64_t)in[i] << (8u * i);
        v >>= 4;
        L->regen = (uint32_t)(v & ((1u << bits) - 1u));
        L->comp = (uint32_t)((v >> bits) & ((1u << bits) - 1u));
        L->streams = fmt == 0u ? 1u : 4u;
        L->header_bytes = h;
        if (L->regen == 0u || L->comp == 0u) return NX_ERR_ZSTD_CORRUPT;
        if (L->streams == 4u && L->regen < 6u) return NX_ERR_ZSTD_CORRUPT;
    }
    if (L->regen > block_max) return NX_ERR_ZSTD_CORRUPT;
    if (L->comp > n - L->header_bytes) return NX_ERR_ZSTD_CORRUPT;
    return NX_OK;
}

// ---- backward bit reader ----
// The stream is in[0, len), read from its end: the last byte's highest set bit is the padding marker.
// pos = bits still unread; a read past the start yields zeros and leaves pos negative (overflow).
struct BackBits {
    const uint8_t* p;
    uint32_t len;
    int32_t pos;
    int32_t lo;    // bit index of win's bit 0 (a multiple of 8)
    uint64_t win;  // stream bits [lo, lo + 64)
};
NX_HD int32_t bb_init(BackBits& b, const uint8_t* in, uint32_t len) {
    if (len == 0u || len > kBlockMax) return NX_ERR_ZSTD_CORRUPT;
    const uint32_t last = in[len - 1u];
    if (last == 0u) return NX_ERR_ZSTD_CORRUPT;
    b.p = in;
    b.len = len;
    b.pos = (int32_t)(8u * (len - 1u) + highbit(last));
    b.lo = 0x7fffff00;
    b.win = 0;
    return NX_OK;
}
// stream bits [at, at + n), n <= 32; bits below 0 are zero
NX_HD uint32_t bb_bits_at(BackBits& b, int32_t at, uint32_t n) {
    if (n == 0u) return 0u;
    uint32_t below = 0;  // bits of the request that lie before the stream's start
    if (at < 0) {
        if (at + (int32_t)n <= 0) return 0u;
        below = (uint32_t)(-at);
        n -= below;
        at = 0;
    }
    if (at < b.lo || at + (int32_t)n > b.lo + 64) {
        int32_t lo = ((at + (int32_t)n + 7) & ~7) - 64;
        if (lo < 0) lo = 0;
        const uint32_t byte = (uint32_t)lo >> 3;
        uint64_t w = 0;
        if (byte + 8u <= b.len) {
            __builtin_memcpy(&w, b.p + byte, 8);
        } else {
            for (uint32_t i = 0; i < 8u; ++i)
                if (byte + i < b.len) w |= (uint64_t)b.p[byte + i] << (8u * i);
        }
        b.lo = lo;
        b.win = w;
    }
    const uint64_t v = b.win >> (uint32_t)(at - b.lo);
    return ((uint32_t)v & (n >= 32u ? 0xffffffffu : (1u << n) - 1u)) << below;
}
NX_HD uint32_t bb_read(BackBits& b, uint32_t n) {
    b.pos -= (int32_t)n;
    return bb_bits_at(b, b.pos, n);
}
// the next n bits without consuming them (Huffman: n = the table's log)
NX_HD uint32_t bb_peek(BackBits& b, uint32_t n) { return bb_bits_at(b, b.pos - (int32_t)n, n); }

// ---- FSE ----
// Read a distribution from in[0, n) into norm[0, max_syms) (-1 = "less than 1"); *log = its accuracy
// log, *used = the bytes it occupies.
NX_HD int32_t fse_read_distribution(const uint8_t* in, uint32_t n, uint32_t max_log, uint32_t max_syms, int16_t* norm,
                                    uint32_t* log, uint32_t* used) {
    uint32_t bit = 0;
    const uint32_t nbits = n * 8u;
    bool bad = false;
    auto rd = [&](uint32_t k) -> uint32_t {  // k <= 16
        if (bit + k > nbits) {
            bad = true;
            return 0u;
        }
        uint32_t v = 0;
        const uint32_t byte = bit >> 3;
        for (uint32_t i = 0; i < 3u; ++i)
            if (byte + i < n) v |= (uint32_t)in[byte + i] << (8u * i);
        v = (v >> (bit & 7u)) & ((1u << k) - 1u);
        bit += k;
        return v;
    };
    const uint32_t al = 5u + rd(4);
    if (bad || al > max_log) return NX_ERR_ZSTD_CORRUPT;
    int32_t remaining = 1 << al;
    uint32_t sym = 0;
    while (remaining > 0 && sym < max_syms) {  // every pass adds a symbol
        const uint32_t bits = highbit((uint32_t)remaining + 1u) + 1u;
        uint32_t val = rd(bits);
        if (bad) return NX_ERR_ZSTD_CORRUPT;
        const uint32_t lower = (1u << (bits - 1u)) - 1u;
        const uint32_t threshold = (1u << bits) - 1u - ((uint32_t)remaining + 1u);
        if ((val & lower) < threshold) {
            bit -= 1u;
            val &= lower;
        } else if (val > lower) {
            val -= threshold;
        }
        const int32_t proba = (int32_t)val - 1;
        remaining -= proba < 0 ? -proba : proba;
        norm[sym++] = (int16_t)proba;
        if (proba == 0) {
            for (uint32_t guard = 0; guard < 256u; ++guard) {  // each repeat flag adds up to 3 symbols
                const uint32_t rep = rd(2);
                if (bad) return NX_ERR_ZSTD_CORRUPT;
                for (uint32_t i = 0; i < rep; ++i) {
                    if (sym >= max_syms) return NX_ERR_ZSTD_CORRUPT;
                    norm[sym++] = 0;
                }
                if (rep != 3u) break;
            }
        }
    }
    if (remaining != 0) return NX_ERR_ZSTD_CORRUPT;  // the sum lands exactly on the table size
    for (uint32_t s = sym; s < max_syms; ++s) norm[s] = 0;
    *log = al;
    *used = (bit + 7u) >> 3;
    return NX_OK;
}

// Build the decoding table of norm[0, nsyms) with accuracy log `log`; next[] is scratch of nsyms entries.
NX_HD int32_t fse_build_table(const int16_t* norm, uint32_t nsyms, uint32_t log, FseEntry* t, uint16_t* next) {
    const uint32_t size = 1u << log, mask = size - 1u;
    uint32_t high = size;
    for (uint32_t s = 0; s < nsyms; ++s)
        if (norm[s] == -1) {  // the "less than 1" symbols take the cells from the top
            if (high == 0u) return NX_ERR_ZSTD_CORRUPT;
            t[--high].sym = (uint8_t)s;
            next[s] = 1;
        }
    const uint32_t step = (size >> 1) + (size >> 3) + 3u;
    uint32_t pos = 0, placed = size - high;
    for (uint32_t s = 0; s < nsyms; ++s) {
        if (norm[s] <= 0) continue;
        next[s] = (uint16_t)norm[s];
        placed += (uint32_t)norm[s];
        if (placed > size) return NX_ERR_ZSTD_CORRUPT;
        for (int32_t i = 0; i < norm[s]; ++i) {
            t[pos].sym = (uint8_t)s;
            uint32_t guard = size;
            do {
                pos = (pos + step) & mask;
            } while (pos >= high && guard-- != 0u);
        }
    }
    if (pos != 0u || placed != size) return NX_ERR_ZSTD_CORRUPT;
    for (uint32_t i = 0; i < size; ++i) {
        const uint32_t nx = next[t[i].sym]++;
        const uint32_t nb = log - highbit(nx);
        t[i].nbits = (uint8_t)nb;
        t[i].base = (uint16_t)((nx << nb) - size);
    }
    return NX_OK;
}
NX_HD void fse_rle_table(FseEntry* t, uint32_t sym) {
    t[0].sym = (uint8_t)sym;
    t[0].nbits = 0;
    t[0].base = 0;
}

// the predefined distributions (RFC 8878 3.1.1.3.2.2), accuracy logs 6, 5, 6
NX_HD int32_t predefined_norm(uint32_t which, uint32_t s) {
    static constexpr int8_t kLl[36] = {4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2,
                                       2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1};
    static constexpr int8_t kOf[29] = {1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1};
    static constexpr int8_t kMl[53] = {1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                                       1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1};
    return which == 0u ? kLl[s] : which == 1u ? kOf[s] : kMl[s];
}
NX_HD uint32_t ll_base(uint32_t c, uint32_t* bits) {
    static constexpr uint32_t kBase[36] = {0,  1,  2,  3,  4,  5,  6,  7,  8,  9,   10,  11,  12,   13,   14,   15,   16,    18,
                                           20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536};
    static constexpr uint8_t kBits[36] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
    *bits = kBits[c];
    return kBase[c];
}
NX_HD uint32_t ml_base(uint32_t c, uint32_t* bits) {
    static constexpr uint32_t kBase[53] = {3,  4,  5,  6,  7,  8,  9,  10, 11, 12, 13, 14, 15, 16, 17,  18,  19,  20,
                                           21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35,  37,  39,  41,
                                           43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539};
    static constexpr uint8_t kBits[53] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                                          0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
    *bits = kBits[c];
    return kBase[c];
}

// One of the three sequence tables, by its mode (0 Predefined, 1 RLE, 2 FSE, 3 Repeat); which = 0 literal
// lengths, 1 offsets, 2 match lengths.  in[0, n) follows the modes byte; *used = bytes this table took.
NX_HD int32_t seq_table(Tables& T, Entropy& E, uint32_t which, uint32_t mode, const uint8_t* in, uint32_t n, uint32_t* used) {
    FseEntry* t = which == 0u ? T.ll : which == 1u ? T.of : T.ml;
    uint32_t* log = which == 0u ? &E.ll_log : which == 1u ? &E.of_log : &E.ml_log;
    const uint32_t nsyms = which == 0u ? kLlSyms : which == 1u ? kOfSyms : kMlSyms;
    *used = 0;
    if (mode == 0u) {
        const uint32_t dn = which == 1u ? 29u : nsyms;
        for (uint32_t s = 0; s < dn; ++s) T.norm[s] = (int16_t)predefined_norm(which, s);
        *log = which == 1u ? 5u : 6u;
        return fse_build_table(T.norm, dn, *log, t, T.next);
    }
    if (mode == 1u) {
        if (n < 1u || in[0] >= nsyms) return NX_ERR_ZSTD_CORRUPT;
        fse_rle_table(t, in[0]);
        *log = 0;
        *used = 1;
        return NX_OK;
    }
    if (mode == 2u) {
        const uint32_t max_log = which == 0u ? kLlMaxLog : which == 1u ? kOfMaxLog : kMlMaxLog;
        const int32_t st = fse_read_distribution(in, n, max_log, nsyms, T.norm, log, used);
        if (st != NX_OK) return st;
        return fse_build_table(T.norm, nsyms, *log, t, T.next);
    }
    return E.seq_valid ? NX_OK : NX_ERR_ZSTD_CORRUPT;  // Repeat_Mode needs a predecessor
}

// ---- Huffman tree description ----
// in[0, n): the literals section after its header.  Builds T.huf (2^huf_log entries); *used = the
// description's bytes.
NX_HD int32_t huf_read_tree(Tables& T, Entropy& E, const uint8_t* in, uint32_t n, uint32_t* used) {
    if (n < 1u) return NX_ERR_ZSTD_CORRUPT;
    const uint32_t hb = in[0];
    uint32_t nw = 0;  // weights present (the last symbol's is implied)
    if (hb >= 128u) {
        nw = hb - 127u;
        const uint32_t bytes = (nw + 1u) >> 1;
        if (1u + bytes > n) return NX_ERR_ZSTD_CORRUPT;
        for (uint32_t i = 0; i < nw; ++i) T.weights[i] = (uint8_t)((i & 1u) ? in[1u + (i >> 1)] & 15u : in[1u + (i >> 1)] >> 4);
        *used = 1u + bytes;
    } else {
        if (hb == 0u || 1u + hb > n) return NX_ERR_ZSTD_CORRUPT;
        uint32_t log = 0, dn = 0;
        int32_t st = fse_read_distribution(in + 1, hb, kHwMaxLog, 256u, T.norm, &log, &dn);
        if (st != NX_OK) return st;
        st = fse_build_table(T.norm, 256u, log, T.hw, T.next);
        if (st != NX_OK) return st;
        if (dn >= hb) return NX_ERR_ZSTD_CORRUPT;
        BackBits b;
        st = bb_init(b, in + 1u + dn, hb - dn);
        if (st != NX_OK) return st;
        uint32_t s1 = bb_read(b, log), s2 = bb_read(b, log);
        if (b.pos < 0) return NX_ERR_ZSTD_CORRUPT;
        for (;;) {  // two interleaved states; ends on the read that runs past the stream's start
            if (nw > 253u) return NX_ERR_ZSTD_CORRUPT;
            T.weights[nw++] = T.hw[s1].sym;
            s1 = T.hw[s1].base + bb_read(b, T.hw[s1].nbits);
            if (b.pos < 0) {
                T.weights[nw++] = T.hw[s2].sym;
                break;
            }
            if (nw > 253u) return NX_ERR_ZSTD_CORRUPT;
            T.weights[nw++] = T.hw[s2].sym;
            s2 = T.hw[s2].base + bb_read(b, T.hw[s2].nbits);
            if (b.pos < 0) {
                T.weights[nw++] = T.hw[s1].sym;
                break;
            }
        }
        *used = 1u + hb;
    }
    uint32_t sum = 0;
    for (uint32_t w = 0; w < 16u; ++w) T.rank[w] = 0;
    for (uint32_t i = 0; i < nw; ++i) {
        const uint32_t w = T.weights[i];
        if (w > kHufMaxLog) return NX_ERR_ZSTD_CORRUPT;
        T.rank[w] += 1u;
        sum += w ? 1u << (w - 1u) : 0u;
    }
    if (sum == 0u) return NX_ERR_ZSTD_CORRUPT;
    const uint32_t log = highbit(sum) + 1u;
    if (log > kHufMaxLog) return NX_ERR_ZSTD_CORRUPT;
    const uint32_t left = (1u << log) - sum;
    if (left & (left - 1u)) return NX_ERR_ZSTD_CORRUPT;  // the implied weight completes a power of two
    const uint32_t lastw = highbit(left) + 1u;
    T.weights[nw++] = (uint8_t)lastw;
    T.rank[lastw] += 1u;
    if (T.rank[1] < 2u || (T.rank[1] & 1u)) return NX_ERR_ZSTD_CORRUPT;
    uint32_t start = 0;  // rank[w] becomes the first cell of weight w: the longest codes take the lowest cells
    for (uint32_t w = 1; w <= log; ++w) {
        const uint32_t cur = start;
        start += T.rank[w] << (w - 1u);
        T.rank[w] = cur;
    }
    for (uint32_t s = 0; s < nw; ++s) {
        const uint32_t w = T.weights[s];
        if (w == 0u) continue;
        const uint32_t len = 1u << (w - 1u), at = T.rank[w];
        if (at + len > (1u << log)) return NX_ERR_ZSTD_CORRUPT;
        for (uint32_t i = 0; i < len; ++i) {
            T.huf[at + i].sym = (uint8_t)s;
            T.huf[at + i].nbits = (uint8_t)(log + 1u - w);
        }
        T.rank[w] = at + len;
    }
    E.huf_log = log;
    E.huf_valid = 1;
    return NX_OK;
}

// The geometry of a Compressed / Treeless literals section's streams: in[0, n) follows the tree
// description.  Stream k is in[off[k], off[k] + len[k]) and regenerates regen_k[k] bytes at out_k[k].
struct HufStreams {
    uint32_t count;
    uint32_t off[4], len[4], out[4], regen[4];
};
NX_HD int32_t huf_streams(const uint8_t* in, uint32_t n, uint32_t streams, uint32_t regen, HufStreams* S) {
    S->count = streams;
    if (streams == 1u) {
        if (n < 1u) return NX_ERR_ZSTD_CORRUPT;
        S->off[0] = 0;
        S->len[0] = n;
        S->out[0] = 0;
        S->regen[0] = regen;
        return NX_OK;
    }
    if (n < 10u) return NX_ERR_ZSTD_CORRUPT;  // the jump table and a byte per stream
    const uint32_t l1 = le_bytes(in, 2), l2 = le_bytes(in + 2, 2), l3 = le_bytes(in + 4, 2);
    if (6u + l1 + l2 + l3 >= n || l1 == 0u || l2 == 0u || l3 == 0u) return NX_ERR_ZSTD_CORRUPT;
    const uint32_t seg = (regen + 3u) >> 2;
    if (3u * seg > regen) return NX_ERR_ZSTD_CORRUPT;
    S->off[0] = 6u;
    S->len[0] = l1;
    S->off[1] = 6u + l1;
    S->len[1] = l2;
    S->off[2] = 6u + l1 + l2;
    S->len[2] = l3;
    S->off[3] = 6u + l1 + l2 + l3;
    S->len[3] = n - S->off[3];
    for (uint32_t k = 0; k < 4u; ++k) {
        S->out[k] = k * seg;
        S->regen[k] = k < 3u ? seg : regen - 3u * seg;
    }
    return NX_OK;
}
// one stream: `regen` symbols into out, the stream consumed exactly
NX_HD int32_t huf_decode_stream(const HufEntry* huf, uint32_t log, const uint8_t* in, uint32_t len, uint8_t* out, uint32_t regen) {
    BackBits b;
    const int32_t st = bb_init(b, in, len);
    if (st != NX_OK) return st;
    for (uint32_t i = 0; i < regen; ++i) {
        const HufEntry e = huf[bb_peek(b, log)];
        b.pos -= (int32_t)e.nbits;
        out[i] = e.sym;
        if (b.pos < 0) return NX_ERR_ZSTD_CORRUPT;
    }
    return b.pos == 0 ? NX_OK : NX_ERR_ZSTD_CORRUPT;
}

// ---- sequences ----
struct SeqHeader {
    uint32_t nseq, header_bytes;  // header_bytes includes the modes byte when nseq > 0
    uint32_t modes[3];            // literal lengths, offsets, match lengths
};
NX_HD int32_t parse_sequences_header(const uint8_t* in, uint32_t n, SeqHeader* S) {
    if (n < 1u) return NX_ERR_ZSTD_CORRUPT;
    const uint32_t b0 = in[0];
    uint32_t h = 1;
    if (b0 < 128u) {
        S->nseq = b0;
    } else if (b0 < 255u) {
        if (n < 2u) return NX_ERR_ZSTD_CORRUPT;
        S->nseq = ((b0 - 128u) << 8) + in[1];
        h = 2;
    } else {
        if (n < 3u) return NX_ERR_ZSTD_CORRUPT;
        S->nseq = le_bytes(in + 1, 2) + 0x7F00u;
        h = 3;
    }
    S->modes[0] = S->modes[1] = S->modes[2] = 0;
    if (S->nseq == 0u) {
        S->header_bytes = h;
        return n == h ? NX_OK : NX_ERR_ZSTD_CORRUPT;  // nothing follows an empty sequences section
    }
    if (n < h + 1u) return NX_ERR_ZSTD_CORRUPT;
    const uint32_t m = in[h];
    if (m & 3u) return NX_ERR_ZSTD_CORRUPT;
    S->modes[0] = m >> 6;
    S->modes[1] = (m >> 4) & 3u;
    S->modes[2] = (m >> 2) & 3u;
    S->header_bytes = h + 1u;
    return NX_OK;
}

struct Seq {
    uint32_t ll, ml, off;  // literal length, match length, resolved offset
};
// the decode position inside a block's sequences
struct SeqCursor {
    BackBits bits;
    uint32_t s_ll, s_of, s_ml;
    uint32_t left;      // sequences still to decode
    uint32_t pos;       // bytes the frame has regenerated once the decoded sequences have run
    uint32_t lit_left;  // literals of the block not yet claimed
    uint32_t cap;       // the frame's output capacity
};
NX_HD int32_t seq_begin(const Entropy& E, SeqCursor& C, const uint8_t* in, uint32_t n, uint32_t nseq, uint32_t pos, uint32_t lits,
                        uint32_t cap) {
    const int32_t st = bb_init(C.bits, in, n);
    if (st != NX_OK) return st;
    C.s_ll = bb_read(C.bits, E.ll_log);
    C.s_of = bb_read(C.bits, E.of_log);
    C.s_ml = bb_read(C.bits, E.ml_log);
    if (C.bits.pos < 0) return NX_ERR_ZSTD_CORRUPT;
    C.left = nseq;
    C.pos = pos;
    C.lit_left = lits;
    C.cap = cap;
    return NX_OK;
}
// One sequence: the three codes of the current states, their extra bits (offset, match length, literal
// length), the repeat-offset rules, then the state updates (literal lengths, match lengths, offsets)
// unless it is the block's last.  Checks it against the literals left, the bytes produced and the capacity.
NX_HD int32_t seq_step(const Tables& T, Entropy& E, SeqCursor& C, Seq* out) {
    const FseEntry el = T.ll[C.s_ll], eo = T.of[C.s_of], em = T.ml[C.s_ml];
    if (eo.sym > 31u || el.sym >= kLlSyms || em.sym >= kMlSyms) return NX_ERR_ZSTD_CORRUPT;
    uint32_t lbits, mbits;
    const uint32_t lbase = ll_base(el.sym, &lbits), mbase = ml_base(em.sym, &mbits);
    const uint32_t ov = (eo.sym == 31u ? 0x80000000u : 1u << eo.sym) + bb_read(C.bits, eo.sym);
    const uint32_t ml = mbase + bb_read(C.bits, mbits);
    const uint32_t ll = lbase + bb_read(C.bits, lbits);
    uint32_t off;
    if (ov > 3u) {
        off = ov - 3u;
        E.rep[2] = E.rep[1];
        E.rep[1] = E.rep[0];
        E.rep[0] = off;
    } else {
        const uint32_t idx = ov + (ll == 0u ? 1u : 0u);  // 1..4
        if (idx == 1u) {
            off = E.rep[0];
        } else {
            off = idx == 4u ? E.rep[0] - 1u : E.rep[idx - 1u];
            if (off == 0u) return NX_ERR_ZSTD_CORRUPT;
            if (idx != 2u) E.rep[2] = E.rep[1];
            E.rep[1] = E.rep[0];
            E.rep[0] = off;
        }
    }
    if (C.left > 1u) {
        C.s_ll = el.base + bb_read(C.bits, el.nbits);
        C.s_ml = em.base + bb_read(C.bits, em.nbits);
        C.s_of = eo.base + bb_read(C.bits, eo.nbits);
    }
    if (C.bits.pos < 0) return NX_ERR_ZSTD_CORRUPT;
    if (C.left == 1u && C.bits.pos != 0) return NX_ERR_ZSTD_CORRUPT;  // the bitstream is consumed exactly
    if (ll > C.lit_left) return NX_ERR_ZSTD_CORRUPT;
    if (ll > C.cap - C.pos || ml > C.cap - C.pos - ll) return NX_ERR_ZSTD_OUTPUT_FULL;
    if (off > C.pos + ll) return NX_ERR_ZSTD_CORRUPT;  // beyond the bytes produced so far
    C.lit_left -= ll;
    C.pos += ll + ml;
    C.left -= 1u;
    out->ll = ll;
    out->ml = ml;
    out->off = off;
    return NX_OK;
}
// Up to kTile sequences into out[]; *count = those decoded and valid (they are to be executed even when
// the status is an error: the bytes before an error stand).
NX_HD int32_t seq_decode_tile(const Tables& T, Entropy& E, SeqCursor& C, Seq* out, uint32_t* count) {
    uint32_t k = 0;
    int32_t st = NX_OK;
    while (k < kTile && C.left != 0u) {
        Seq s;
        st = seq_step(T, E, C, &s);
        if (st != NX_OK) break;
        out[k++] = s;
    }
    *count = k;
    return st;
}

}  // namespace zstdd
}  // namespace nx
