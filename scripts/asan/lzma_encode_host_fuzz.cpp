// lzma_encode_host_fuzz.cpp — a host-only sanitizer run of the LZMA encoder's format core and host encoder:
// seeded random inputs of 0..6 000 bytes over alphabets of 1, 2, 4 and 256 values, with copied pieces, at random
// lc, lp, pb (lc + lp > 4 included), dictionary sizes 0..70 000 and both end-marker modes go through
// nx_lzma_encode_host into a heap block of exactly nx_lzma_max_compressed_length bytes; then into blocks of exactly
// the stream's size (must succeed with the same bytes), one byte less, half, 13, 12 and 0 bytes (must report
// NX_ERR_LZMA_ENCODE_FULL).  The heap blocks end at their capacity, so a byte written past it is ASan's to report.
// A few 300 000-byte inputs cross the 65 536-entry table and the 273 cap many times.  No GPU, no HIP:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       scripts/asan/lzma_encode_host_fuzz.cpp netty_amd/csrc/lzma_encode_host.cpp -o lzma_encode_host_fuzz \
//       && ./lzma_encode_host_fuzz
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../include/netty_amd.h"

static unsigned long g_items = 0, g_full = 0, g_carry_ff = 0;
static uint64_t g_seed = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    g_seed ^= g_seed << 13;
    g_seed ^= g_seed >> 7;
    g_seed ^= g_seed << 17;
    return (uint32_t)(g_seed >> 16);
}

static int64_t enc(const uint8_t* in, size_t n, const int* s, size_t cap, std::vector<uint8_t>* keep, nx_lzma_encode_stats* st) {
    uint8_t* out = (uint8_t*)malloc(cap ? cap : 1);  // exactly cap bytes where cap > 0
    const int64_t r = nx_lzma_encode_host(in, n, s[0], s[1], s[2], s[3], s[4], cap ? out : nullptr, cap, st);
    if (keep && r >= 0) keep->assign(out, out + r);
    free(out);
    return r;
}

static void one(const std::vector<uint8_t>& data, const int* s) {
    const size_t n = data.size();
    uint8_t* in = (uint8_t*)malloc(n ? n : 1);  // exactly n bytes: a read past the item is ASan's to report
    if (n) memcpy(in, data.data(), n);
    std::vector<uint8_t> a, b;
    nx_lzma_encode_stats st;
    const int64_t r = enc(in, n, s, nx_lzma_max_compressed_length(n), &a, &st);
    if (r < 18 || (size_t)r != a.size()) {
        fprintf(stderr, "encode of %zu bytes returned %lld\n", n, (long long)r);
        exit(1);
    }
    if (st.max_carry_ff) ++g_carry_ff;
    if (enc(in, n, s, (size_t)r, &b, nullptr) != r || a != b) {
        fprintf(stderr, "an exact-fit encode of %zu bytes differs\n", n);
        exit(1);
    }
    const size_t small[] = {(size_t)r - 1, (size_t)r / 2, 13, 12, 0};
    for (size_t cap : small) {
        if (enc(in, n, s, cap, nullptr, nullptr) != NX_ERR_LZMA_ENCODE_FULL) {
            fprintf(stderr, "capacity %zu of a %lld-byte stream was not refused\n", cap, (long long)r);
            exit(1);
        }
        ++g_full;
    }
    free(in);
    ++g_items;
}

static std::vector<uint8_t> make(size_t n, uint32_t alphabet) {
    std::vector<uint8_t> d;
    while (d.size() < n) {
        if (!d.empty() && rnd() % 4 == 0) {  // a copy from earlier, 2..600 bytes
            const size_t dist = 1 + rnd() % d.size(), len = 2 + rnd() % 600;
            for (size_t i = 0; i < len && d.size() < n; ++i) d.push_back(d[d.size() - dist]);
        } else {
            for (uint32_t i = 0, k = 1 + rnd() % 40; i < k && d.size() < n; ++i) d.push_back((uint8_t)(rnd() % alphabet));
        }
    }
    return d;
}

int main() {
    const uint32_t alphabets[] = {1, 2, 4, 256};
    for (int it = 0; it < 3000; ++it) {
        const int s[5] = {(int)(rnd() % 9), (int)(rnd() % 5), (int)(rnd() % 5),
                          (int)(rnd() % 3 == 0 ? rnd() % 40 : rnd() % 70001), (int)(rnd() & 1)};
        one(make(rnd() % 6001, alphabets[rnd() % 4]), s);
    }
    for (int it = 0; it < 4; ++it) {
        const int s[5] = {3, 0, 2, it < 2 ? 65536 : 1 << 20, it & 1};
        one(make(300000, alphabets[it]), s);
    }
    const int bad[][5] = {{9, 0, 0, 0, 0}, {0, 5, 0, 0, 0}, {0, 0, 5, 0, 0}, {-1, 0, 0, 0, 0}, {3, 0, 2, -1, 0}};
    for (const int* s : bad) {
        uint8_t x = 0, out[64];
        const int64_t r = nx_lzma_encode_host(&x, 1, s[0], s[1], s[2], s[3], s[4], out, sizeof out, nullptr);
        if (r != (s[3] < 0 ? NX_ERR_LZMA_DICT_SIZE : NX_ERR_LZMA_PROPS)) {
            fprintf(stderr, "bad settings returned %lld\n", (long long)r);
            return 1;
        }
    }
    printf("lzma_encode_host_fuzz: %lu items, %lu refused capacities, %lu items with a carry through a pending 0xFF: clean\n", g_items,
           g_full, g_carry_ff);
    return 0;
}
