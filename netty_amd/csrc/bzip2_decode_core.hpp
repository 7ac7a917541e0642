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
// A reader that starts at a bit position: byte `at` with its first `used` bits (0..7) already taken.
NX_HD void br_init_bit(BitReader& r, const uint8_t* p, uint32_t n, uint32_t at, uint32_t used) {
    br_init(r, p, n, at);
    if (used != 0u && at < n) {
        r.buf = p[at];
        r.at = at + 1u;
        r.cnt = 8u - used;
    } else if (used != 0u) {
        r.over = 1;  // the byte that holds the position is not there
    }
}
NX_HD void br_init_bitpos(BitReader& r, const uint8_t* p, uint32_t n, uint64_t bitpos) {
    const uint64_t at = bitpos >> 3;
    br_init_bit(r, p, n, at < n ? (uint32_t)at : n, at < n ? (uint32_t)(bitpos & 7u) : 0u);
}
// The position of the next unread bit (br_bits loads a byte only when it needs one, so fewer than eight bits
// wait in buf).  Meaningful while `over` is clear.
NX_HD uint64_t br_bitpos(const BitReader& r) { return 8ull * r.at - r.cnt; }

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
// The bytes src[0, n) become in the final stage, without writing them: what rle_step's outputs add up to.
NX_HD uint32_t rle_length(Rle& R, const uint8_t* src, uint32_t n) {
    uint32_t total = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint8_t b = src[i];
        if (R.want_count) {
            R.want_count = 0;
            R.acc = 0;
            total += b;
            continue;
        }
        if ((int32_t)b != R.last) {
            R.last = b;
            R.acc = 1;
        } else if (++R.acc == 4u) {
            R.want_count = 1;
        }
        total += 1u;
    }
    return total;
}

// ------------------------------------------------------------------ the split decode: magic scan and chain stitch
// A stream's blocks are independent once their first bit is known, and each starts with the 48-bit block
// magic.  The split decode (bzip2_decode_split.hip, nx_bzip2_decode_split_host) scans an item for both magics
// at every bit position, decodes every candidate block on its own (the front: everything up to the pre-RLE
// bytes, and the length the final stage will give), then walks the chain from the stream's first block: a
// block's end bit names the candidate that follows it.  A candidate the chain never reaches is a decoy (the
// magic's 48 bits spelt by data, or standing in bytes after the stream) and its result is dropped.
constexpr uint64_t kCandEnd = 1ull << 63;  // a candidate's kind flag: the end-of-stream magic
constexpr uint64_t kCandPos = kCandEnd - 1ull;
constexpr uint64_t kMagicBlock = ((uint64_t)kBlockMagicHi << 24) | kBlockMagicLo;
constexpr uint64_t kMagicEnd = ((uint64_t)kEndMagicHi << 24) | kEndMagicLo;
constexpr uint32_t kScanWindow = 8;        // bytes whose bit positions one window tests (it reads 6 more)
constexpr uint32_t kScanSegments = 64;     // an item is scanned in this many segments
constexpr int32_t kChainOpen = 1;          // SplitItem::status while the chain is being walked
// bytes per segment of an item of n bytes: a multiple of a wave's 64 windows
NX_HD uint64_t scan_segment_bytes(uint32_t n) {
    const uint64_t per = ((uint64_t)n + kScanSegments - 1u) / kScanSegments, step = 64u * kScanWindow;
    return (per + step - 1u) / step * step;
}
// The magics that start in the eight bytes from b0: bit k of *blk (*end) is set when the block (end) magic
// stands at bit 8 b0 + k and lies inside the item's n bytes.
NX_HD void scan_window(const uint8_t* p, uint32_t n, uint64_t b0, uint64_t* blk, uint64_t* end) {
    uint64_t mb = 0, me = 0;
    if (b0 < n) {
        uint8_t w[kScanWindow + 6];
        for (uint32_t j = 0; j < kScanWindow + 6u; ++j) w[j] = b0 + j < n ? p[b0 + j] : (uint8_t)0;
        uint64_t v = 0;  // the 56 bits from byte j
        for (uint32_t j = 0; j < 6u; ++j) v = (v << 8) | w[j];
        for (uint32_t j = 0; j < kScanWindow; ++j) {
            v = ((v << 8) | w[j + 6u]) & ((1ull << 56) - 1ull);
            for (uint32_t s = 0; s < 8u; ++s) {
                const uint64_t m = (v >> (8u - s)) & ((1ull << 48) - 1ull);
                const uint32_t k = 8u * j + s;
                if ((m == kMagicBlock || m == kMagicEnd) && 8ull * b0 + k + 48u <= 8ull * n) {
                    if (m == kMagicBlock) mb |= 1ull << k;
                    else me |= 1ull << k;
                }
            }
        }
    }
    *blk = mb;
    *end = me;
}

// What the front of a candidate block leaves, and what the stitch and the back add.
struct CandResult {
    uint64_t end_bit;    // the bit after the block's end-of-block symbol
    int32_t status;      // of stages 1-4
    uint32_t pre_len;    // bytes before the final run-length stage
    uint32_t final_len;  // bytes after it
    uint32_t crc;        // the block's stored CRC
    uint32_t member;     // stitch: the chain reaches this block
    uint32_t off;        // stitch: where its bytes go in the item's output
    int32_t back_status; // back: OUTPUT_FULL, the missing count byte, BLOCK_CRC or NX_OK
    uint32_t crc_got;    // back: the CRC of its bytes
};
// Where an item's chain starts when the item is not a whole stream (the Bzip2Decoder handle): the stream's
// header has been read before, the first block's magic stands at bit `expect` of the item, `crc` is the stream
// CRC folded so far.  Such an item is a stream still arriving, so a block is attempted only when a later
// candidate has arrived behind it, and the block at `expect` only when more than seen_after candidates have:
// the number that stood behind it when it last answered TRUNCATED.
struct SplitStart {
    uint64_t expect;
    uint32_t crc, level, seen_after, pad;
};
constexpr int32_t kNotAttempted = 2;  // CandResult::status of a block the rule above holds back
// An item's chain, carried from round to round.
struct SplitItem {
    uint64_t expect;   // where the chain's next member must stand
    uint64_t head;     // where the chain began
    uint32_t cursor;   // the first of the item's candidates the chain has not passed
    uint32_t off;      // output bytes given to members so far
    uint32_t crc;      // the stream CRC folded over them
    uint32_t blocks;   // members so far
    uint32_t level;
    uint32_t consumed;
    int32_t status;    // kChainOpen, or how the stream ended
    uint32_t arriving;        // a SplitStart was given
    uint32_t seen_after;
    uint32_t tail_attempted;  // status is TRUNCATED and it is the answer of a block's front
};
NX_HD void split_begin(SplitItem& I, const uint8_t* in, uint32_t n, const SplitStart* start = nullptr) {
    I.expect = 32;
    I.cursor = I.off = I.crc = I.blocks = I.level = I.consumed = 0;
    I.arriving = I.seen_after = I.tail_attempted = 0;
    if (start) {
        I.expect = start->expect;
        I.crc = start->crc;
        I.level = start->level;
        I.seen_after = start->seen_after;
        I.arriving = 1;
        I.status = kChainOpen;
    } else {
        const int32_t st = stream_header(in, n, &I.level);
        I.status = st == NX_OK ? kChainOpen : st;
    }
    I.head = I.expect;
}
// Whether the block at bit `pos` is decoded now: always in a whole stream; in one still arriving, when enough
// candidates stand behind it (`later` of them).
NX_HD bool split_attempt(const SplitItem& I, uint64_t pos, uint32_t later) {
    return !I.arriving || later > (pos == I.head ? I.seen_after : 0u);
}
// Extends the chain over the item's candidates pos[0, count), of which the first `ready` have a front result.
// The order of the checks is decode_stream's: ten bytes of magic and CRC or TRUNCATED, the end magic and the
// stream CRC, the block magic or BLOCK_HEADER, then the block.  Returns with I.status == kChainOpen when the
// next member waits for a later round.
NX_HD void split_stitch(SplitItem& I, const uint8_t* in, uint32_t n, uint32_t cap, const uint64_t* pos, CandResult* res, uint32_t count,
                        uint32_t ready) {
    while (I.status == kChainOpen) {  // every pass takes a candidate or ends the chain
        if (I.expect + 80u > 8ull * n) {
            I.status = NX_ERR_BZIP2_TRUNCATED;
            break;
        }
        while (I.cursor < count && (pos[I.cursor] & kCandPos) < I.expect) I.cursor += 1u;
        if (I.cursor == count || (pos[I.cursor] & kCandPos) != I.expect) {
            I.status = NX_ERR_BZIP2_BLOCK_HEADER;  // neither magic stands there
            break;
        }
        if (pos[I.cursor] & kCandEnd) {
            BitReader r;
            br_init_bitpos(r, in, n, I.expect + 48u);
            const uint32_t crc = br_bits(r, 32);
            if (crc != I.crc) {
                I.status = NX_ERR_BZIP2_STREAM_CRC;
            } else {
                I.status = NX_OK;
                I.consumed = r.at;  // the combined CRC's last byte holds the padding
            }
            break;
        }
        if (I.cursor >= ready) return;
        CandResult& c = res[I.cursor];
        if (c.status == kNotAttempted) {
            I.status = NX_ERR_BZIP2_TRUNCATED;  // still arriving
            break;
        }
        if (c.status != NX_OK) {
            I.status = c.status;
            I.tail_attempted = c.status == NX_ERR_BZIP2_TRUNCATED;
            break;
        }
        if (c.final_len > cap - I.off) {
            I.status = NX_ERR_BZIP2_OUTPUT_FULL;
            break;
        }
        c.member = 1;
        c.off = I.off;
        I.off += c.final_len;
        I.crc = crc_combine_stream(I.crc, c.crc);
        I.blocks += 1u;
        I.expect = c.end_bit;
        I.cursor += 1u;
    }
}
// After the last back: the first member whose final stage failed ends the stream there.
NX_HD void split_finish(const SplitItem& I, const CandResult* res, uint32_t count, int32_t* status, uint32_t* out_len, uint32_t* consumed,
                        uint32_t* blocks) {
    uint32_t members = 0;
    for (uint32_t k = 0; k < count && k < I.cursor; ++k) {
        if (!res[k].member) continue;
        if (res[k].back_status != NX_OK) {
            *status = res[k].back_status;
            *out_len = res[k].off;
            *consumed = 0;
            *blocks = members;
            return;
        }
        members += 1u;
    }
    *status = I.status == kChainOpen ? NX_ERR_INTERNAL : I.status;
    *out_len = I.off;
    *consumed = I.status == NX_OK ? I.consumed : 0u;
    *blocks = I.blocks;
}

}  // namespace bz2d
}  // namespace nx
