// bzip2_encode_core.hpp — the format logic of the bzip2 encoder, written once for the host and the device:
// the first run-length stage and block filling, the move-to-front / RUNA-RUNB stage, the Huffman stage
// (table count, seeds, selector search, length-limited code lengths, canonical codes) and the bit writer.
// Plain functions: no wave intrinsics, no LDS keywords; state and tables come in as references and pointers
// (the kernel hands in LDS and its workspace slot, the host encoder heap blocks).  bzip2_encode.hip runs the
// serial ones on one lane and the per-group ones across the workgroup; bzip2_encode_host.cpp runs all of
// them on the CPU, where the tests hold the streams against libbz2.
//
// Semantics follow Bzip2Encoder.java, Bzip2BlockCompressor.java, Bzip2MTFAndRLE2StageEncoder.java,
// Bzip2HuffmanStageEncoder.java, Bzip2HuffmanAllocator.java, Bzip2BitWriter.java and
// Bzip2MoveToFrontTable.java.  The Burrows-Wheeler transform is not Bzip2DivSufSort.java: it is the sort of
// the block's cyclic rotations, equal rotations in the order of their index (DESIGN.md "Bzip2 encode"); the
// host's sort is in bzip2_encode_host.cpp, the kernel's in bzip2_encode.hip, and both give that one order.
#pragma once
#include "bzip2_decode_core.hpp"

namespace nx {
namespace bz2e {

using bz2d::kBaseBlock;
using bz2d::kGroup;
using bz2d::kMaxAlpha;
using bz2d::kMaxSelectors;
using bz2d::kMaxTables;
constexpr uint32_t kEncMaxCodeLen = 20;  // Bzip2Constants.HUFFMAN_ENCODE_MAX_CODE_LENGTH
constexpr uint32_t kSeedCost = 15;       // Bzip2HuffmanStageEncoder.java:32 HUFFMAN_HIGH_SYMBOL_COST
constexpr uint32_t kPasses = 4;          // Bzip2HuffmanStageEncoder.java:365

// ------------------------------------------------------------------ sizes
// Bits of one block whose first-stage length is m, at most:
//   48 magic + 32 CRC + 1 randomised + 24 start pointer                         = 105
//   16 + 256 symbol map                                                         = 272
//   3 table count + 15 selector count                                           = 18
//   selectors: ceil((m + 1) / 50) <= m / 50 + 1 of them, at most 6 bits each (unary 0..5 and the stop bit)
//   six tables of 5 + 258 x (1 + 2 x 19) bits (lengths stay in 1..20: a delta is at most 19 two-bit steps)
//   20 bits for each of at most m + 1 symbols (a BWT byte gives at most one symbol; the end-of-block symbol)
constexpr uint64_t kBlockFixedBits = 105u + 272u + 18u + 6u * (5u + 258u * 39u) + 6u + 20u;
constexpr uint64_t block_bits_bound(uint64_t m) { return kBlockFixedBits + 6u * (m / 50u) + 20u * m; }
// A stream of n input bytes at `level`: the first stage grows n to at most r = n + n / 4 (four bytes become
// five); a block that is closed with input left holds more than S - 6 bytes (S = level x 100 000), so there
// are at most r / (S - 5) + 1 blocks; block_bits_bound is linear in m apart from its constant, and the
// m / 50 terms of the blocks sum to at most r / 50; 32 bits of stream header, 80 of footer, 7 of padding.
constexpr uint64_t stream_bytes_bound(uint64_t n, uint32_t level) {
    const uint64_t S = (uint64_t)level * kBaseBlock, r = n + n / 4u;
    const uint64_t blocks = n ? r / (S - 5u) + 1u : 0u;
    return (32u + 80u + 7u + blocks * kBlockFixedBits + 6u * (r / 50u) + 20u * r + 7u) / 8u;
}

// ------------------------------------------------------------------ bit writer (Bzip2BitWriter.java)
// Bits go most significant first into a zeroed array of 32-bit words that hold the stream's bytes in order.
// Every word is OR-ed in, so writers that start at different bit positions may share a word (the kernel's
// lanes emit their groups side by side); on the device the OR is an atomic.
NX_HD void or_word(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    (void)__hip_atomic_fetch_or(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    *p |= v;
#endif
}
struct BitWriter {
    uint32_t* w;
    uint64_t acc;  // the n pending bits, in its low bits
    uint32_t n;    // below 32
    uint32_t idx;  // next word
};
NX_HD void bw_init(BitWriter& b, uint32_t* w, uint64_t bitpos) {
    b.w = w;
    b.acc = 0;  // the bits before bitpos in its word are another writer's: zeros leave them alone
    b.n = (uint32_t)(bitpos & 31u);
    b.idx = (uint32_t)(bitpos >> 5);
}
NX_HD void bw_put(BitWriter& b, uint32_t cnt, uint32_t val) {  // Bzip2BitWriter.java:41-56; cnt <= 32
    if (cnt == 0u) return;
    b.acc = (b.acc << cnt) | (cnt == 32u ? (uint64_t)val : (uint64_t)(val & ((1u << cnt) - 1u)));
    b.n += cnt;
    if (b.n >= 32u) {
        b.n -= 32u;
        or_word(b.w + b.idx, __builtin_bswap32((uint32_t)(b.acc >> b.n)));
        b.idx += 1u;
        b.acc &= (1ull << b.n) - 1ull;
    }
}
NX_HD void bw_unary(BitWriter& b, uint32_t v) {  // Bzip2BitWriter.java:80-88; v <= 5 here
    bw_put(b, v + 1u, ((1u << v) - 1u) << 1);
}
NX_HD uint64_t bw_bits(const BitWriter& b) { return (uint64_t)b.idx * 32u + b.n; }
// the pending bits into their word, zero bits behind them (Bzip2BitWriter.java:102-119 pads the same way)
NX_HD void bw_flush(BitWriter& b) {
    if (b.n) or_word(b.w + b.idx, __builtin_bswap32((uint32_t)(b.acc << (32u - b.n))));
}

// ------------------------------------------------------------------ first run-length stage (Bzip2BlockCompressor.java)
struct Rle1 {
    uint32_t len;    // blockLength
    uint32_t limit;  // blockLengthLimit = blockSize - 6 (Bzip2BlockCompressor.java:102)
    uint32_t run;    // rleLength
    uint32_t cur;    // rleCurrentValue
    uint32_t crc;    // running, not yet inverted
    uint8_t present[256];
};
NX_HD void rle1_init(Rle1& R, uint32_t block_size) {
    R.len = 0;
    R.limit = block_size - 6u;
    R.run = 0;
    R.cur = 0;
    R.crc = 0xffffffffu;
    for (uint32_t i = 0; i < 256u; ++i) R.present[i] = 0;
}
// Bzip2BlockCompressor.java:141-176 writeRun
NX_HD void rle1_write_run(Rle1& R, uint8_t* block, const uint32_t* T, uint32_t value, uint32_t run) {
    R.present[value] = 1;
    for (uint32_t k = 0; k < run; ++k) R.crc = bz2d::crc_byte(T, R.crc, value);
    uint8_t* p = block + R.len;
    if (run < 4u) {
        for (uint32_t k = 0; k < run; ++k) p[k] = (uint8_t)value;
        R.len += run;
    } else {
        run -= 4u;
        R.present[run] = 1;  // the count byte is a value of the block like any other
        p[0] = p[1] = p[2] = p[3] = (uint8_t)value;
        p[4] = (uint8_t)run;
        R.len += 5u;
    }
}
// Bzip2BlockCompressor.java:183-207 write: false when the block takes no more
NX_HD bool rle1_write(Rle1& R, uint8_t* block, const uint32_t* T, uint32_t value) {
    if (R.len > R.limit) return false;
    if (R.run == 0u) {
        R.cur = value;
        R.run = 1;
    } else if (R.cur != value) {
        rle1_write_run(R, block, T, R.cur, R.run);
        R.cur = value;
        R.run = 1;
    } else if (R.run == 254u) {
        rle1_write_run(R, block, T, R.cur, 255);
        R.run = 0;
    } else {
        R.run += 1u;
    }
    return true;
}
// Bzip2BlockCompressor.java:225-229 close: the pending run; the block then holds at most blockSize bytes
NX_HD void rle1_close(Rle1& R, uint8_t* block, const uint32_t* T) {
    if (R.run > 0u) rle1_write_run(R, block, T, R.cur, R.run);
    R.run = 0;
}
NX_HD bool rle1_empty(const Rle1& R) { return R.len == 0u && R.run == 0u; }  // Bzip2BlockCompressor.java:287-289

// ------------------------------------------------------------------ the planner: where a stream's blocks are cut
// The block-filling rule above without the block's bytes (Bzip2BlockCompressor.java:141-207): the state is the
// block length, the run value and the run count, so it can be saved after any byte and resumed.  A block is
// closed as soon as it is full (blockLength > blockLengthLimit, Bzip2Encoder.java:132-143), which is where the
// next byte would be refused; closing flushes the pending run, and the next block starts with none.
struct Plan {
    uint32_t len, run, cur;
};
NX_HD void plan_init(Plan& P) { P.len = P.run = P.cur = 0; }
NX_HD uint32_t plan_run_bytes(uint32_t run) { return run < 4u ? run : 5u; }  // writeRun: a run of four or more is five bytes
NX_HD void plan_byte(Plan& P, uint32_t value) {                              // write(), for a block that is not full
    if (P.run == 0u) {
        P.cur = value;
        P.run = 1;
    } else if (P.cur != value) {
        P.len += plan_run_bytes(P.run);
        P.cur = value;
        P.run = 1;
    } else if (P.run == 254u) {
        P.len += 5u;
        P.run = 0;
    } else {
        P.run += 1u;
    }
}
NX_HD bool plan_full(const Plan& P, uint32_t limit) { return P.len > limit; }
NX_HD bool plan_empty(const Plan& P) { return P.len == 0u && P.run == 0u; }
// in[0, n) offered to P: the input end (base + index) of every block that closes goes to cuts[*count++] while
// *count < cap and is counted beyond; with `close` the open block, if it holds anything, is closed at base + n.
NX_HD void plan_range(Plan& P, uint32_t limit, const uint8_t* in, uint64_t n, bool close, uint64_t base, uint64_t* cuts, uint64_t cap,
                      uint64_t* count) {
    for (uint64_t i = 0; i < n; ++i) {
        plan_byte(P, in[i]);
        if (plan_full(P, limit)) {
            if (*count < cap) cuts[*count] = base + i + 1u;
            *count += 1u;
            plan_init(P);
        }
    }
    if (close && !plan_empty(P)) {
        if (*count < cap) cuts[*count] = base + n;
        *count += 1u;
        plan_init(P);
    }
}
// The blocks of n input bytes at `level`, at most: the derivation of stream_bytes_bound.
constexpr uint64_t blocks_bound(uint64_t n, uint32_t level) {
    return n ? (n + n / 4u) / ((uint64_t)level * kBaseBlock - 5u) + 1u : 0u;
}

// ------------------------------------------------------------------ the splice, as a gather
// Consecutive parts of a stream, each a run of bits from bit 0 of its own zero-padded bytes (the carried bits,
// blocks encoded from bit 0, the footer), land one behind another.  start[k] is the destination bit of part k,
// start[parts] the total.  A destination byte takes its first bits from the part that holds its first bit and
// the rest from the next part: a block is at least 105 bits and the footer 80, and only the carry (below 32
// bits, always first) can be shorter than a byte, so a byte never spans three.
struct SpliceSrc {
    uint32_t part;  // the part of the byte's first bit; `parts` when the byte lies past the total
    uint64_t off;   // that bit's offset in the part
    uint32_t have;  // the bits the part still holds from there, 8 at most: the other 8 - have come from bit 0 of part + 1
};
NX_HD SpliceSrc splice_source(const uint64_t* start, uint32_t parts, uint64_t byte) {
    const uint64_t bit = byte * 8u;
    if (bit >= start[parts]) return {parts, 0, 8};
    uint32_t lo = 0, hi = parts - 1u;  // the last part whose start is at or before `bit`; empty parts are passed over
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1u) >> 1;
        if (start[mid] <= bit) lo = mid;
        else hi = mid - 1u;
    }
    const uint64_t left = start[lo + 1u] - bit;
    return {lo, bit - start[lo], left < 8u ? (uint32_t)left : 8u};
}
// eight bits from bit `off` of bytes b (zeros behind the part's last bit), given a way to read byte i
template <class ByteAt>
NX_HD uint32_t splice_read8(ByteAt&& at, uint64_t off) {
    const uint64_t i = off >> 3;
    const uint32_t sh = (uint32_t)(off & 7u);
    const uint32_t v = (at(i) << 8) | (sh ? at(i + 1u) : 0u);
    return (v >> (8u - sh)) & 0xffu;
}

// ------------------------------------------------------------------ second stage (Bzip2MTFAndRLE2StageEncoder.java)
struct Mtf2 {
    uint8_t list[256];  // Bzip2MoveToFrontTable
    uint8_t map[256];   // huffmanSymbolMap
    uint32_t freq[kMaxAlpha];
    uint32_t repeat, idx, eob;
};
NX_HD void mtf2_init(Mtf2& M, const uint8_t* present) {  // Bzip2MTFAndRLE2StageEncoder.java:86-95
    uint32_t unique = 0;
    for (uint32_t i = 0; i < 256u; ++i) {
        M.list[i] = (uint8_t)i;
        M.map[i] = 0;
        if (present[i]) M.map[i] = (uint8_t)unique++;
    }
    for (uint32_t i = 0; i < kMaxAlpha; ++i) M.freq[i] = 0;
    M.repeat = 0;
    M.idx = 0;
    M.eob = unique + 1u;
}
NX_HD uint32_t mtf_value_to_front(uint8_t* list, uint8_t value) {  // Bzip2MoveToFrontTable.java:57-70
    uint32_t index = 0;
    uint8_t temp = list[0];
    if (value != temp) {
        list[0] = value;
        while (value != temp) {
            index += 1u;
            const uint8_t temp2 = temp;
            temp = list[index];
            list[index] = temp2;
        }
    }
    return index;
}
NX_HD void mtf2_flush_run(Mtf2& M, uint16_t* out) {  // Bzip2MTFAndRLE2StageEncoder.java:108-125
    if (M.repeat == 0u) return;
    uint32_t r = M.repeat - 1u;
    for (;;) {  // at most 20 symbols: the count halves
        const uint32_t s = r & 1u;  // RUNA = 0, RUNB = 1
        out[M.idx++] = (uint16_t)s;
        M.freq[s] += 1u;
        if (r <= 1u) break;
        r = (r - 2u) >> 1;
    }
    M.repeat = 0;
}
// cnt more bytes of the transformed block (Bzip2MTFAndRLE2StageEncoder.java:101-129)
NX_HD void mtf2_step(Mtf2& M, const uint8_t* bwt, uint32_t cnt, uint16_t* out) {
    for (uint32_t i = 0; i < cnt; ++i) {
        const uint32_t pos = mtf_value_to_front(M.list, M.map[bwt[i]]);
        if (pos == 0u) {
            M.repeat += 1u;
        } else {
            mtf2_flush_run(M, out);
            out[M.idx++] = (uint16_t)(pos + 1u);
            M.freq[pos + 1u] += 1u;
        }
    }
}
// Bzip2MTFAndRLE2StageEncoder.java:131-155: returns mtfLength; the alphabet size is M.eob + 1
NX_HD uint32_t mtf2_finish(Mtf2& M, uint16_t* out) {
    mtf2_flush_run(M, out);
    out[M.idx] = (uint16_t)M.eob;
    M.freq[M.eob] += 1u;
    return M.idx + 1u;
}

// ------------------------------------------------------------------ Huffman stage (Bzip2HuffmanStageEncoder.java)
NX_HD uint32_t select_table_count(uint32_t mtf_len) {  // Bzip2HuffmanStageEncoder.java:101-115
    return mtf_len >= 2400u ? 6u : mtf_len >= 1200u ? 5u : mtf_len >= 600u ? 4u : mtf_len >= 200u ? 3u : 2u;
}
// Bzip2HuffmanStageEncoder.java:162-195 generateHuffmanOptimisationSeeds: 0 inside a table's section, 15 outside
NX_HD void huffman_seeds(uint8_t (*lens)[kMaxAlpha], const uint32_t* freq, uint32_t alpha, uint32_t mtf_len, uint32_t tables) {
    int32_t remaining = (int32_t)mtf_len, low_end = -1;
    for (uint32_t i = 0; i < tables; ++i) {
        const int32_t target = remaining / (int32_t)(tables - i);
        const int32_t low_start = low_end + 1;
        int32_t actual = 0;
        while (actual < target && low_end < (int32_t)alpha - 1) actual += (int32_t)freq[++low_end];
        if (low_end > low_start && i != 0u && i != tables - 1u && ((tables - i) & 1u) == 0u) actual -= (int32_t)freq[low_end--];
        for (int32_t j = 0; j < (int32_t)alpha; ++j) lens[i][j] = (j < low_start || j > low_end) ? (uint8_t)kSeedCost : (uint8_t)0;
        remaining -= actual;
    }
}
// Bzip2HuffmanStageEncoder.java:222-240: the table that codes sym[0, cnt) in the fewest bits, the first on a tie
NX_HD uint32_t group_best_table(const uint8_t (*lens)[kMaxAlpha], const uint16_t* sym, uint32_t cnt, uint32_t tables) {
    uint32_t cost[kMaxTables] = {0, 0, 0, 0, 0, 0};
    for (uint32_t i = 0; i < cnt; ++i) {
        const uint32_t v = sym[i];
#pragma unroll
        for (uint32_t j = 0; j < kMaxTables; ++j) cost[j] += j < tables ? lens[j][v] : 0u;
    }
    uint32_t best = 0, best_cost = cost[0];
#pragma unroll
    for (uint32_t j = 1; j < kMaxTables; ++j)
        if (j < tables && cost[j] < best_cost) {
            best_cost = cost[j];
            best = j;
        }
    return best;
}

// ---- Bzip2HuffmanAllocator.java, on int32_t a[0, length)
NX_HD int32_t ha_first(const int32_t* a, int32_t length, int32_t i, int32_t nodes_to_move) {  // :33-53
    const int32_t limit = i;
    int32_t k = length - 2;
    while (i >= nodes_to_move && a[i] % length > limit) {
        k = i;
        i -= limit - i + 1;
    }
    i = nodes_to_move - 1 > i ? nodes_to_move - 1 : i;
    while (k > i + 1) {
        const int32_t temp = (int32_t)((uint32_t)(i + k) >> 1);
        if (a[temp] % length > limit) k = temp;
        else i = temp;
    }
    return k;
}
NX_HD void ha_parent_pointers(int32_t* a, int32_t length) {  // :59-80
    a[0] += a[1];
    for (int32_t head = 0, tail = 1, top = 2; tail < length - 1; ++tail) {
        int32_t temp;
        if (top >= length || a[head] < a[top]) {
            temp = a[head];
            a[head++] = tail;
        } else {
            temp = a[top++];
        }
        if (top >= length || (head < tail && a[head] < a[top])) {
            temp += a[head];
            a[head++] = tail + length;
        } else {
            temp += a[top++];
        }
        a[tail] = temp;
    }
}
NX_HD int32_t ha_nodes_to_relocate(const int32_t* a, int32_t length, int32_t max_len) {  // :88-94
    int32_t node = length - 2;
    for (int32_t depth = 1; depth < max_len - 1 && node > 1; ++depth) node = ha_first(a, length, node - 1, 0);
    return node;
}
NX_HD void ha_node_lengths(int32_t* a, int32_t length) {  // :100-114
    int32_t first_node = length - 2, next = length - 1;
    for (int32_t depth = 1, avail = 2; avail > 0; ++depth) {
        const int32_t last = first_node;
        first_node = ha_first(a, length, last - 1, 0);
        for (int32_t i = avail - (last - first_node); i > 0; --i) a[next--] = depth;
        avail = (last - first_node) << 1;
    }
}
NX_HD void ha_node_lengths_relocated(int32_t* a, int32_t length, int32_t nodes_to_move, int32_t insert_depth) {  // :122-150
    int32_t first_node = length - 2, next = length - 1;
    int32_t depth = insert_depth == 1 ? 2 : 1;
    int32_t left = insert_depth == 1 ? nodes_to_move - 2 : nodes_to_move;
    for (int32_t avail = depth << 1; avail > 0; ++depth) {
        const int32_t last = first_node;
        first_node = first_node <= nodes_to_move ? first_node : ha_first(a, length, last - 1, nodes_to_move);
        int32_t offset = 0;
        if (depth >= insert_depth) {
            const int32_t room = 1 << (depth - insert_depth);
            offset = left < room ? left : room;
        } else if (depth == insert_depth - 1) {
            offset = 1;
            if (a[first_node] == last) first_node += 1;
        }
        for (int32_t i = avail - (last - first_node + offset); i > 0; --i) a[next--] = depth;
        left -= offset;
        avail = (last - first_node + offset) << 1;
    }
}
// :158-181 allocateHuffmanCodeLengths: a = sorted frequencies in, code lengths out
NX_HD void ha_allocate(int32_t* a, int32_t length, int32_t max_len) {
    if (length == 2) a[1] = 1;
    if (length <= 2) {
        a[0] = 1;
        return;
    }
    ha_parent_pointers(a, length);
    const int32_t relocate = ha_nodes_to_relocate(a, length, max_len);
    if (a[0] % length >= relocate) {
        ha_node_lengths(a, length);
    } else {
        int32_t bits = 0;  // 32 - numberOfLeadingZeros(relocate - 1)
        for (uint32_t v = (uint32_t)(relocate - 1); v != 0u; v >>= 1) bits += 1;
        ha_node_lengths_relocated(a, length, relocate, max_len - bits);
    }
}
// Bzip2HuffmanStageEncoder.java:123-154 generateHuffmanCodeLengths, in three steps so that the kernel can
// spread the first and the last over its lanes.  The keys (freq << 9) | index are distinct, so a key's place in
// the sorted order is the number of smaller keys (what Arrays.sort arrives at).
NX_HD void lengths_sort_one(const uint32_t* freq, uint32_t alpha, uint32_t k, int32_t* merged, int32_t* sorted) {
    const int32_t key = (int32_t)((freq[k] << 9) | k);
    uint32_t rank = 0;
    for (uint32_t i = 0; i < alpha; ++i) rank += (int32_t)((freq[i] << 9) | i) < key ? 1u : 0u;
    merged[rank] = key;
    sorted[rank] = (int32_t)((uint32_t)key >> 9);
}
NX_HD void lengths_unsort_one(const int32_t* merged, const int32_t* sorted, uint32_t i, uint8_t* lens) {
    lens[merged[i] & 0x1ff] = (uint8_t)sorted[i];
}
// Bzip2HuffmanStageEncoder.java:264-297 assignHuffmanCodeSymbols for one table: codes[k] = (length << 24) | code
NX_HD void assign_codes(const uint8_t* lens, uint32_t alpha, uint32_t* codes) {
    uint32_t lo = 32, hi = 0;
    for (uint32_t j = 0; j < alpha; ++j) {
        const uint32_t l = lens[j];
        hi = l > hi ? l : hi;
        lo = l < lo ? l : lo;
    }
    uint32_t code = 0;
    for (uint32_t j = lo; j <= hi; ++j) {
        for (uint32_t k = 0; k < alpha; ++k)
            if (lens[k] == j) codes[k] = (j << 24) | code++;
        code <<= 1;
    }
}

// Everything of a block before its symbols (Bzip2BlockCompressor.java:241-248 and 108-134,
// Bzip2HuffmanStageEncoder.java:302-336): magic, CRC, the randomised bit (always 0), the start pointer, the
// symbol map, the table and selector counts, the selectors through a move-to-front list in unary, and the
// delta-coded lengths.
NX_HD void write_block_head(BitWriter& b, uint32_t crc, uint32_t start, const uint8_t* present, uint32_t tables, const uint8_t* sel,
                            uint32_t selectors, const uint8_t (*lens)[kMaxAlpha], uint32_t alpha) {
    bw_put(b, 24, bz2d::kBlockMagicHi);
    bw_put(b, 24, bz2d::kBlockMagicLo);
    bw_put(b, 32, crc);
    bw_put(b, 1, 0);
    bw_put(b, 24, start);
    uint32_t used16 = 0;
    for (uint32_t i = 0; i < 16u; ++i) {
        uint32_t any = 0;
        for (uint32_t j = 0; j < 16u; ++j) any |= present[16u * i + j];
        used16 = (used16 << 1) | (any ? 1u : 0u);
    }
    bw_put(b, 16, used16);
    for (uint32_t i = 0; i < 16u; ++i) {
        if (!((used16 >> (15u - i)) & 1u)) continue;
        uint32_t bits = 0;
        for (uint32_t j = 0; j < 16u; ++j) bits = (bits << 1) | (present[16u * i + j] ? 1u : 0u);
        bw_put(b, 16, bits);
    }
    bw_put(b, 3, tables);
    bw_put(b, 15, selectors);
    uint8_t list[kMaxTables] = {0, 1, 2, 3, 4, 5};
    for (uint32_t s = 0; s < selectors; ++s) {
        const uint8_t v = sel[s];
        uint32_t idx = 0;
        uint8_t carry = list[0];
        while (carry != v && idx < kMaxTables - 1u) {  // v is one of the six
            idx += 1u;
            const uint8_t t = list[idx];
            list[idx] = carry;
            carry = t;
        }
        list[0] = v;
        bw_unary(b, idx);
    }
    for (uint32_t t = 0; t < tables; ++t) {
        uint32_t cur = lens[t][0];
        bw_put(b, 5, cur);
        for (uint32_t j = 0; j < alpha; ++j) {
            const uint32_t l = lens[t][j];
            const uint32_t step = cur < l ? 2u : 3u;
            for (uint32_t d = cur < l ? l - cur : cur - l; d > 0u; --d) bw_put(b, 2, step);
            bw_put(b, 1, 0);
            cur = l;
        }
    }
}
// Bzip2HuffmanStageEncoder.java:341-357 writeBlockData for groups [g0, g1): their bits, or (b == nullptr) only the count
NX_HD uint64_t emit_groups(BitWriter* b, const uint16_t* mtf, uint32_t mtf_len, const uint8_t* sel, const uint32_t (*codes)[kMaxAlpha],
                           uint32_t g0, uint32_t g1) {
    uint64_t bits = 0;
    for (uint32_t g = g0; g < g1; ++g) {
        const uint32_t* C = codes[sel[g]];
        const uint32_t e = (g + 1u) * kGroup < mtf_len ? (g + 1u) * kGroup : mtf_len;
        for (uint32_t i = g * kGroup; i < e; ++i) {
            const uint32_t c = C[mtf[i]];
            bits += c >> 24;
            if (b) bw_put(*b, c >> 24, c & 0xffffffu);
        }
    }
    return bits;
}

}  // namespace bz2e
}  // namespace nx
