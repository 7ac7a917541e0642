// lz_seq_core.hpp — what the sequence matchers of the LZMA and Brotli encoders stand on (lzma_encode_core.hpp,
// brotli_encode_core.hpp), host and device: unaligned reads, the common length of two strings, the stamped
// single-probe hash table of four bytes and the writer of sequence words.  Each core keeps its own rule
// (match_item) and the layout of its word above the literal run.
//
// The table has 2^kHashLog entries of stamp << 32 | position; an entry counts only with this call's stamp, so a
// table is zeroed once and used by many calls.  A sequence is one 64-bit word whose low kRunBits bits count the
// literals before its match; a run that reaches kRunMax literals is written as a word with nothing above them.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string.h>

#ifndef NX_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define NX_HD __host__ __device__ inline
#else
#define NX_HD inline
#endif
#endif

namespace nx {
namespace lzseq {

constexpr uint32_t kHashLog = 16, kHashBytes = 4;
constexpr uint32_t kRunBits = 23, kRunMax = (1u << kRunBits) - 1u;
constexpr uint32_t kNone = ~0u;

// The bytes an item's sequences take in the arena: a count word, a spare one, `cap` sequence words, to 16 bytes.
NX_HD size_t area_bytes(size_t cap) { return (16u + 8u * cap + 15u) & ~(size_t)15; }

NX_HD uint32_t rd32(const uint8_t* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef uint32_t __attribute__((aligned(1))) u32u;
    return *reinterpret_cast<const u32u*>(p);
#else
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
#endif
}

NX_HD uint32_t common_len(const uint8_t* a, const uint8_t* b, uint32_t maxlen) {
    uint32_t l = 0;
    while (l + 4u <= maxlen) {
        const uint32_t x = rd32(a + l) ^ rd32(b + l);
        if (x) {
            // the first differing byte (little endian)
            return l + ((x & 0xFFu) ? 0u : (x & 0xFF00u) ? 1u : (x & 0xFF0000u) ? 2u : 3u);
        }
        l += 4u;
    }
    while (l < maxlen && a[l] == b[l]) ++l;
    return l;
}

NX_HD uint32_t hash4(uint32_t w) { return (w * 2654435761u) >> (32u - kHashLog); }

// The entry of the four bytes w at ip is read and replaced by ip.  Returns the position it held if this call
// wrote it and it lies below ip, else kNone; whether its bytes are w's is the caller's to check.
NX_HD uint32_t probe(uint64_t* table, uint64_t stag, uint32_t stamp, uint32_t w, uint32_t ip) {
    const uint32_t h = hash4(w);
    const uint64_t e = table[h];
    table[h] = stag | ip;
    const uint32_t cand = (uint32_t)e;
    return (e >> 32) == stamp && cand < ip ? cand : kNone;
}

// The positions [from, end) of in[0, n) that have four bytes left enter the table.
NX_HD void insert_span(uint64_t* table, uint64_t stag, const uint8_t* in, uint32_t from, uint32_t end, uint32_t n) {
    for (uint32_t q = from; q < end && q + kHashBytes <= n; ++q) table[hash4(rd32(in + q))] = stag | q;
}

// The sequence words of an item into seq[0, cap).  Both calls return false where cap would be passed.
struct SeqWriter {
    uint64_t* seq;
    size_t cap;
    uint32_t ns, run;
    // a word: `above` is what the codec keeps over the literal run
    NX_HD bool match(uint64_t above) {
        if (ns >= cap) return false;
        seq[ns++] = (uint64_t)run | above;
        run = 0;
        return true;
    }
    NX_HD bool literal() { return ++run != kRunMax || match(0); }
};

}  // namespace lzseq
}  // namespace nx
