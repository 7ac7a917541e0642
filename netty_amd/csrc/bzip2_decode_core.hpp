// bzip2_decode_core.hpp — the format logic of the bzip2 decoder, written once for the host and the
// device: the stream and block headers, the symbol-use bitmaps, selectors and delta-coded code lengths,
// the Huffman table build and the bit-at-a-time symbol decode, run symbols and the move-to-front list,
// the final run-length stage and bzip2's CRC-32.  Plain serial functions: no wave intrinsics, no LDS
// keywords; tables come in as pointers (the kernel hands in LDS, the host decoder a heap block).
// bzip2_decode.hip runs them on lane 0 of a stream's wave and adds the wave-wide parts (tile flushes,
// the merged-pointer build, the split inverse-BWT walk, the CRC fold); bzip2_decode_host.cpp runs them
// on the CPU, where the tests hold them against libbz2.
//
// Semantics follow Bzip2Decoder.java, Bzip2BlockDecompressor.java, Bzip2HuffmanStageDecoder.java,
// Bzip2MoveToFrontTable.java, Bzip2BitReader.java and Crc32.java, one status per throw site
// (netty_amd_status.h).  Where the Java would throw an unchecked array-index exception, libbz2 decides:
//   - a selector's unary index at or above the table count (Bzip2Decoder.java:227 indexes the
//     move-to-front list with it, and the table arrays later) is NX_ERR_BZIP2_DECODING_BLOCK;
//   - a code length that leaves 1..23 (Bzip2Decoder.java:273 stores it unchecked and
//     createHuffmanDecodingTables indexes with it) is NX_ERR_BZIP2_CODE, checked on every value the
//     length takes, as libbz2 checks it (libbz2's own range is 1..20);
//   - a code whose index falls outside the symbol table (Bzip2HuffmanStageDecoder.java:196) is
//     NX_ERR_BZIP2_CODE.
// Incomplete and over-subscribed length sets build the same limit, base and symbol tables as the Java
// (32-bit wrapping arithmetic included) and decode from the table's minimum length one bit at a time,
// so they decode as they do there.  "block length exceeds max block length"
// (Bzip2BlockDecompressor.java:234) cannot be reached under the declared-size checks and has no code.
// A block with the randomised bit set is refused (NX_ERR_BZIP2_RANDOMISED): this library does not carry
// the format's 512-entry table.  A block that ends right after four equal bytes, with no count byte, is
// NX_ERR_BZIP2_DECODING_BLOCK (rle_end): the Java reads the count past the block's end
// (Bzip2BlockDecompressor.java:297) and never meets the end again, libbz2 calls the block corrupt.
//
// Nothing is assumed about the input: no read leaves [in, in + n) (the bit reader hands out zeros past the
// end and raises `over`, which every caller turns into NX_ERR_BZIP2_TRUNCATED before it trusts a value),
// and every loop is bounded by the input's bits or a format constant.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "../../include/netty_amd_status.h"

#ifndef NX_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define NX_HD __host__ __device__ inline
#else
#define NX_HD inline
#endif
#endif

namespace nx {
namespace bz2d {

constexpr uint32_t kBaseBlock = 100000;    // declared block size = level x this
constexpr uint32_t kMaxBlock = 900000;
constexpr uint32_t kMaxSelectors = 18002;  // Bzip2Constants.MAX_SELECTORS
constexpr uint32_t kMaxTables = 6, kMinTables = 2;
constexpr uint32_t kMaxAlpha = 258;
constexpr uint32_t kMaxCodeLen = 23;       // HUFFMAN_DECODE_MAX_CODE_LENGTH
constexpr uint32_t kGroup = 50;            // symbols per selector
constexpr uint32_t kRunA = 0, kRunB = 1;
constexpr uint32_t kNoSym = 0xffffffffu;
constexpr uint32_t kBlockMagicHi = 0x314159u, kBlockMagicLo = 0x265359u;
constexpr uint32_t kEndMagicHi = 0x177245u, kEndMagicLo = 0x385090u;
constexpr uint32_t kCrcPoly = 0x04C11DB7u;  // most significant bit first, not reflected
constexpr uint32_t kRleInline = 16;         // final-stage runs below this are written in place by rle_step

// ------------------------------------------------------------------ bit reader (Bzip2BitReader.java)
struct BitReader {
    const uint8_t* p;
    uint32_t n;    // bytes of input
    uint32_t at;   // next byte to load
    uint32_t cnt;  // unread bits in buf
    uint32_t over; // a load went past the end (zeros were handed out)
    uint64_t buf;
};
NX_HD void br_init(BitReader& r, const uint8_t* p, uint32_t n, uint32_t at) {
    r.p = p;
    r.n = n;
    r.at = at;
    r.cnt = 0;
    r.over = 0;
    r.buf = 0;
}
NX_HD uint32_t br_bits(BitReader& r, uint32_t k) {  // k <= 32
    while (r.cnt < k) {
        uint32_t b = 0;
        if (r.at < r.n) {
            b = r.p[r.at];
            r.at += 1;
        } else {
            r.over = 1;
        }
        r.buf = (r.buf << 8) | b;
        r.cnt += 8;
    }
    r.cnt -= k;
    return (uint32_t)((r.buf >> r.cnt) & ((1ull << k) - 1ull));
}
NX_HD uint32_t br_bit(BitReader& r) { return br_bits(r, 1); }

// ------------------------------------------------------------------ CRC-32, bzip2's bit order (Crc32.java)
NX_HD uint32_t crc_table_entry(uint32_t i) {
    uint32_t c = i << 24;
    for (int k = 0; k < 8; ++k) c = (c & 0x80000000u) ? (c << 1) ^ kCrcPoly : (c << 1);
    return c;
}
NX_HD uint32_t crc_byte(const uint32_t* T, uint32_t c, uint32_t b) { return (c << 8) ^ T[(c >> 24) ^ b]; }
// a * b modulo the polynomial; bit k of a word is the coefficient of x^k
NX_HD uint32_t crc_mulmod(uint32_t a, uint32_t b) {
    uint32_t r = 0;
    for (int i = 31; i >= 0; --i) {
        r = (r << 1) ^ ((r & 0x80000000u) ? kCrcPoly : 0u);
        if ((b >> i) & 1u) r ^= a;
    }
    return r;
}
// x^(8 * 2^j) modulo the polynomial, j = 0..20: the shift of a CRC state over 2^j bytes
struct CrcShift {
    uint32_t x8[21];
};
NX_HD void crc_shift_init(CrcShift& S) {
    S.x8[0] = 1u << 8;
    for (int j = 1; j < 21; ++j) S.x8[j] = crc_mulmod(S.x8[j - 1], S.x8[j - 1]);
}
// the state c after m more zero bytes (m < 2^21)
NX_HD uint32_t crc_shift(const CrcShift& S, uint32_t c, uint32_t m) {
    for (uint32_t j = 0; m != 0u; ++j, m >>= 1)
        if (m & 1u) c = crc_mulmod(c, S.x8[j]);
    return c;
}
NX_HD uint32_t crc_combine_stream(uint32_t stream_crc, uint32_t block_crc) { return ((stream_crc << 1) | (stream_crc >> 31)) ^ block_crc; }

// ------------------------------------------------------------------ headers
// "BZh" and the level: *level = 1..9.  in has at least 4 bytes.
NX_HD int32_t stream_header(const uint8_t* in, uint32_t n, uint32_t* level) {
    if (n < 4u) return NX_ERR_BZIP2_TRUNCATED;
    if (in[0] != 'B' || in[1] != 'Z' || in[2] != 'h') return NX_ERR_BZIP2_STREAM_ID;
    const int32_t lv = (int32_t)(int8_t)in[3] - '0';
    if (lv < 1 || lv > 9) return NX_ERR_BZIP2_BLOCK_SIZE;
    *level = (uint32_t)lv;
    return NX_OK;
}
// The 48-bit magic and the CRC after it: *end = 1 for the end-of-stream magic (*crc the combined CRC).
NX_HD int32_t block_magic(BitReader& r, uint32_t* end, uint32_t* crc) {
    const uint32_t hi = br_bits(r, 24), lo = br_bits(r, 24);
    const uint32_t c = br_bits(r, 32);
    if (r.over) return NX_ERR_BZIP2_TRUNCATED;  // (the reference waits for all ten bytes before it looks)
    *crc = c;
    if (hi == kEndMagicHi && lo == kEndMagicLo) {
        *end = 1;
        return NX_OK;
    }
    *end = 0;
    return hi == kBlockMagicHi && lo == kBlockMagicLo ? NX_OK : NX_ERR_BZIP2_BLOCK_HEADER;
}

struct HufTable {
    int32_t limit[kMaxCodeLen + 1];  // last code of each length
    int32_t base[kMaxCodeLen + 2];   // first code of each length minus the index of its first symbol
    uint16_t sym[kMaxAlpha];
    uint16_t minlen;
};
// A block's decode state: what the headers said, the tables, and the cursor of the symbol loop.
struct Block {
    BitReader br;
    uint32_t block_size;  // declared: 100 000 x level
    uint32_t crc;         // the block's stored CRC
    uint32_t start;       // BWT start pointer
    uint32_t eob;         // end-of-block symbol = symbols in use + 1
    uint32_t ntables, nsel;
    uint32_t gidx, gleft, cur;  // selector index, symbols left in its group, its table
    uint32_t rc, ri;            // RUNA/RUNB: repeat count and increment (Java ints: wrapping)
    uint32_t mtf_value;         // the front of the move-to-front list
    uint32_t pending;           // a decoded symbol the tile had no room for (kNoSym: none)
    uint32_t len;               // BWT bytes so far
    uint8_t symmap[256];
    uint8_t mtf[256];
    uint32_t counts[256];
    HufTable tab[kMaxTables];
};

NX_HD uint32_t mtf_to_front(uint8_t* mtf, uint32_t index) {  // Bzip2MoveToFrontTable.indexToFront
    const uint8_t v = mtf[index];
    for (uint32_t i = index; i > 0u; --i) mtf[i] = mtf[i - 1];
    mtf[0] = v;
    return v;
}

// createHuffmanDecodingTables for one table; every length is in 1..23
NX_HD void build_table(HufTable& H, const uint8_t* lens, uint32_t alpha) {
    uint32_t mn = kMaxCodeLen, mx = 0;
    for (uint32_t i = 0; i < alpha; ++i) {
        mx = lens[i] > mx ? lens[i] : mx;
        mn = lens[i] < mn ? lens[i] : mn;
    }
    H.minlen = (uint16_t)mn;
    for (uint32_t i = 0; i < kMaxCodeLen + 2; ++i) H.base[i] = 0;
    for (uint32_t i = 0; i < kMaxCodeLen + 1; ++i) H.limit[i] = 0;
    for (uint32_t i = 0; i < alpha; ++i) H.base[lens[i] + 1u] += 1;
    for (uint32_t i = 1; i < kMaxCodeLen + 2; ++i) H.base[i] += H.base[i - 1];
    uint32_t code = 0;
    for (uint32_t i = mn; i <= mx; ++i) {
        const uint32_t first = code;
        code += (uint32_t)(H.base[i + 1] - H.base[i]);
        H.base[i] = (int32_t)(first - (uint32_t)H.base[i]);
        H.limit[i] = (int32_t)(code - 1u);
        code <<= 1;
    }
    for (uint32_t i = 0; i < kMaxAlpha; ++i) H.sym[i] = 0;
    uint32_t idx = 0;
    for (uint32_t bl = mn; bl <= mx; ++bl)
        for (uint32_t s = 0; s < alpha; ++s)
            if (lens[s] == bl) H.sym[idx++] = (uint16_t)s;
}

// Everything of a block between its CRC and its first symbol (Bzip2Decoder.java:143-290): the randomised
// bit, the start pointer, the symbol-use bitmaps, the table and selector counts, the selectors and the
// code lengths; builds the tables and resets the symbol cursor.  sel: kMaxSelectors bytes; lens: kMaxAlpha.
NX_HD int32_t block_tables(Block& B, uint8_t* sel, uint8_t* lens) {
    BitReader r = B.br;
    const uint32_t randomised = br_bit(r);
    B.start = br_bits(r, 24);
    const uint32_t in_use16 = br_bits(r, 16);
    if (r.over) return NX_ERR_BZIP2_TRUNCATED;
    if (randomised) return NX_ERR_BZIP2_RANDOMISED;
    for (uint32_t i = 0; i < 256u; ++i) B.symmap[i] = 0;
    uint32_t nsym = 0;
    for (uint32_t i = 0; i < 16u; ++i) {
        if (!(in_use16 & (0x8000u >> i))) continue;
        const uint32_t m = br_bits(r, 16);
        for (uint32_t j = 0; j < 16u; ++j)
            if (m & (0x8000u >> j)) B.symmap[nsym++] = (uint8_t)(i * 16u + j);
    }
    B.eob = nsym + 1u;
    const uint32_t alpha = nsym + 2u;
    B.ntables = br_bits(r, 3);
    if (r.over) return NX_ERR_BZIP2_TRUNCATED;
    if (B.ntables < kMinTables || B.ntables > kMaxTables) return NX_ERR_BZIP2_HUFFMAN_GROUPS;
    if (alpha > kMaxAlpha) return NX_ERR_BZIP2_ALPHABET;  // (256 symbols at most: never taken, kept for the site)
    B.nsel = br_bits(r, 15);
    if (r.over) return NX_ERR_BZIP2_TRUNCATED;
    if (B.nsel < 1u || B.nsel > kMaxSelectors) return NX_ERR_BZIP2_SELECTORS;
    uint8_t tmtf[kMaxTables];
    for (uint32_t i = 0; i < kMaxTables; ++i) tmtf[i] = (uint8_t)i;
    for (uint32_t s = 0; s < B.nsel; ++s) {
        uint32_t index = 0;
        while (index < B.ntables && br_bit(r)) ++index;
        if (r.over) return NX_ERR_BZIP2_TRUNCATED;
        if (index >= B.ntables) return NX_ERR_BZIP2_DECODING_BLOCK;
        sel[s] = (uint8_t)mtf_to_front(tmtf, index);
    }
    for (uint32_t t = 0; t < B.ntables; ++t) {
        uint32_t len = br_bits(r, 5);
        for (uint32_t a = 0; a < alpha; ++a) {
            for (;;) {  // every pass but the last consumes two bits of the input
                if (r.over) return NX_ERR_BZIP2_TRUNCATED;
                if (len < 1u || len > kMaxCodeLen) return NX_ERR_BZIP2_CODE;
                if (!br_bit(r)) break;
                len += br_bit(r) ? 0xffffffffu : 1u;
            }
            lens[a] = (uint8_t)len;
        }
        if (r.over) return NX_ERR_BZIP2_TRUNCATED;
        build_table(B.tab[t], lens, alpha);
    }
    for (uint32_t i = 0; i < 256u; ++i) {
        B.mtf[i] = (uint8_t)i;
        B.counts[i] = 0;
    }
    B.gidx = 0xffffffffu;
    B.gleft = 0;
    B.cur = 0;
    B.rc = 0;
    B.ri = 1;
    B.mtf_value = 0;
    B.pending = kNoSym;
    B.len = 0;
    B.br = r;
    return NX_OK;
}

// Bzip2HuffmanStageDecoder.nextSymbol
NX_HD int32_t next_symbol(BitReader& r, Block& B, const uint8_t* sel, uint32_t* sym) {
    if (B.gleft == 0u) {
        B.gidx += 1u;
        if (B.gidx == B.nsel) return NX_ERR_BZIP2_DECODING_BLOCK;
        B.cur = sel[B.gidx];  // below ntables (block_tables)
        B.gleft = kGroup;
    }
    B.gleft -= 1u;
    const HufTable& H = B.tab[B.cur];
    uint32_t len = H.minlen;
    uint32_t code = br_bits(r, len);
    for (; len <= kMaxCodeLen; ++len) {
        if ((int32_t)code <= H.limit[len]) {
            if (r.over) return NX_ERR_BZIP2_TRUNCATED;
            const uint32_t idx = code - (uint32_t)H.base[len];
            if (idx >= kMaxAlpha) return NX_ERR_BZIP2_CODE;
            *sym = H.sym[idx];
            return NX_OK;
        }
        code = (code << 1) | br_bit(r);
    }
    return r.over ? NX_ERR_BZIP2_TRUNCATED : NX_ERR_BZIP2_CODE;
}

// decodeHuffmanData in tiles: decodes symbols into tile[0, cap) until the tile is full, the block ends
// (*done) or a run does not fit what is left of the tile: then *run_len > 0 and the caller writes
// run_len bytes run_byte after the tile's *cnt bytes.  B.len counts all of them.
NX_HD int32_t sym_tile(Block& B, const uint8_t* sel, uint8_t* tile, uint32_t cap, uint32_t* cnt_out, uint32_t* run_len,
                       uint32_t* run_byte, uint32_t* done) {
    BitReader r = B.br;
    uint32_t cnt = 0;
    int32_t st = NX_OK;
    *run_len = 0;
    *run_byte = 0;
    *done = 0;
    for (;;) {  // every pass consumes a symbol of the input or ends the tile
        uint32_t sym = B.pending;
        if (sym != kNoSym) {
            B.pending = kNoSym;  // its run, if any, went out with the last tile
        } else {
            st = next_symbol(r, B, sel, &sym);
            if (st != NX_OK) break;
            if (sym == kRunA) {
                B.rc += B.ri;
                B.ri <<= 1;
                continue;
            }
            if (sym == kRunB) {
                B.rc += B.ri << 1;
                B.ri <<= 1;
                continue;
            }
            if ((int32_t)B.rc > 0) {
                const uint32_t rc = B.rc;
                if ((uint64_t)B.len + rc > B.block_size) {
                    st = NX_ERR_BZIP2_BLOCK_EXCEEDS;
                    break;
                }
                const uint8_t b = B.symmap[B.mtf_value];
                B.counts[b] += rc;
                B.rc = 0;
                B.ri = 1;
                B.len += rc;
                if (rc <= cap - cnt) {
                    for (uint32_t k = 0; k < rc; ++k) tile[cnt + k] = b;
                    cnt += rc;
                } else {
                    *run_len = rc;
                    *run_byte = b;
                    B.pending = sym;
                    break;
                }
            }
        }
        if (sym == B.eob) {
            *done = 1;
            break;
        }
        if (cnt == cap) {
            B.pending = sym;
            break;
        }
        if (B.len >= B.block_size) {
            st = NX_ERR_BZIP2_BLOCK_EXCEEDS;
            break;
        }
        B.mtf_value = mtf_to_front(B.mtf, sym - 1u);
        const uint8_t b = B.symmap[B.mtf_value];
        B.counts[b] += 1u;
        tile[cnt++] = b;
        B.len += 1u;
    }
    B.br = r;
    *cnt_out = cnt;
    return st;
}

// ------------------------------------------------------------------ inverse BWT, serial (initialiseInverseBWT, decodeNextBWTByte)
// A position fits in 20 bits and a byte in 8, so an entry uses 28 bits; the kernel keeps a flag above them.
constexpr uint32_t kEntryBits = 28;
constexpr uint32_t kEntryMask = (1u << kEntryBits) - 1u;
// The merged pointers of bwt[0, n) by a stable counting sort: tt[k] = (position << 8) | byte.  base: 256 words.
NX_HD void merged_pointers(const uint32_t* counts, uint32_t* base, const uint8_t* bwt, uint32_t n, uint32_t* tt) {
    uint32_t sum = 0;
    for (uint32_t v = 0; v < 256u; ++v) {
        base[v] = sum;
        sum += counts[v];
    }
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t v = bwt[i];
        tt[base[v]++] = (i << 8) | v;
    }
}
// The walk from tt[start], n bytes into pre.  j -> tt[j] >> 8 is a permutation, so the walk follows one
// cycle, round and round when the cycle is shorter than n: the block of a periodic text (w repeated k
// times, 518 equal bytes after the first run-length stage for one) has k cycles of n / k, and n steps
// round one of them spell the text.  The kernel's split walk relies on the same fact.
NX_HD void inverse_bwt_walk(const uint32_t* tt, uint32_t n, uint32_t start, uint8_t* pre) {
    uint32_t e = tt[start];
    for (uint32_t i = 0; i < n; ++i) {
        pre[i] = (uint8_t)e;
        e = tt[e >> 8];
    }
}

// ------------------------------------------------------------------ final run-length stage (Bzip2BlockDecompressor.read)
struct Rle {
    int32_t last;         // the last byte, -1 at the start of a block
    uint32_t acc;         // equal bytes seen in a row
    uint32_t want_count;  // four equal bytes have gone out: the next byte is a repeat count
};
NX_HD void rle_init(Rle& R) {
    R.last = -1;
    R.acc = 0;
    R.want_count = 0;
}
// Takes src[0, n) into dst[0, cap) until src is used up, dst is full, or a repeat count asks for a run of
// kRleInline bytes or more (or more than dst has room for): then *run_len bytes *run_byte follow dst's *cnt.
NX_HD void rle_step(Rle& R, const uint8_t* src, uint32_t n, uint32_t* used, uint8_t* dst, uint32_t cap, uint32_t* cnt, uint32_t* run_len,
                    uint32_t* run_byte) {
    uint32_t i = 0, c = 0;
    *run_len = 0;
    *run_byte = 0;
    while (i < n) {
        if (R.want_count) {
            const uint32_t rep = src[i++];
            R.want_count = 0;
            R.acc = 0;
            if (rep >= kRleInline || rep > cap - c) {
                *run_len = rep;
                *run_byte = (uint32_t)R.last;
                break;
            }
            for (uint32_t k = 0; k < rep; ++k) dst[c + k] = (uint8_t)R.last;
            c += rep;
            continue;
        }
        if (c == cap) break;
        const uint8_t b = src[i++];
        if ((int32_t)b != R.last) {
            R.last = b;
            R.acc = 1;
        } else if (++R.acc == 4u) {
            R.want_count = 1;
        }
        dst[c++] = b;
    }
    *used = i;
    *cnt = c;
}
// After the block's last byte: four equal bytes whose count byte is missing are refused.
NX_HD int32_t rle_end(const Rle& R) { return R.want_count ? NX_ERR_BZIP2_DECODING_BLOCK : NX_OK; }

}  // namespace bz2d
}  // namespace nx
