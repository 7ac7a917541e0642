// brotli_encode_host_fuzz.cpp — a host-only sanitizer run of the Brotli encoder's format core and host encoder:
// seeded random inputs of 0..6 000 bytes over alphabets of 1, 2, 3, 4, 5 and 256 values, with copied pieces, at
// random lgwin 10-24 go through nx_brotli_encode_host into a heap block of exactly nx_brotli_max_compressed_length
// bytes (the bound must hold); then into blocks of exactly the stream's size (must succeed with the same bytes),
// one byte less, half and 0 bytes (must report NX_ERR_BROTLI_ENCODE_FULL).  The heap blocks end at their capacity,
// so a byte written past it is ASan's to report.  A few 300 000-byte inputs cross the 65 536-entry table and
// the meta-block boundary many times.  No GPU, no HIP:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       scripts/asan/brotli_encode_host_fuzz.cpp netty_amd/csrc/brotli_encode_host.cpp -o brotli_encode_host_fuzz \
//       && ./brotli_encode_host_fuzz
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../include/netty_amd.h"

static unsigned long g_items = 0, g_full = 0, g_raw = 0, g_split = 0, g_limited = 0;
static uint64_t g_seed = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    g_seed ^= g_seed << 13;
    g_seed ^= g_seed >> 7;
    g_seed ^= g_seed << 17;
    return (uint32_t)(g_seed >> 16);
}

static int64_t enc(const uint8_t* in, size_t n, int lgwin, size_t cap, std::vector<uint8_t>* keep, nx_brotli_encode_stats* st) {
    uint8_t* out = (uint8_t*)malloc(cap ? cap : 1);  // exactly cap bytes where cap > 0
    const int64_t r = nx_brotli_encode_host(in, n, lgwin, cap ? out : nullptr, cap, st);
    if (keep && r >= 0) keep->assign(out, out + r);
    free(out);
    return r;
}

static void one(const std::vector<uint8_t>& data, int lgwin) {
    const size_t n = data.size();
    uint8_t* in = (uint8_t*)malloc(n ? n : 1);  // exactly n bytes: a read past the item is ASan's to report
    if (n) memcpy(in, data.data(), n);
    std::vector<uint8_t> a, b;
    nx_brotli_encode_stats st;
    const int64_t r = enc(in, n, lgwin, nx_brotli_max_compressed_length(n), &a, &st);
    if (r < 1 || (size_t)r != a.size()) {
        fprintf(stderr, "encode of %zu bytes at lgwin %d returned %lld\n", n, lgwin, (long long)r);
        exit(1);
    }
    g_raw += st.uncompressed_blocks, g_split += st.split_copies, g_limited += st.limited_codes;
    if (enc(in, n, lgwin, (size_t)r, &b, nullptr) != r || a != b) {
        fprintf(stderr, "an exact-fit encode of %zu bytes differs\n", n);
        exit(1);
    }
    const size_t small[] = {(size_t)r - 1, (size_t)r / 2, 0};
    for (size_t cap : small) {
        if (enc(in, n, lgwin, cap, nullptr, nullptr) != NX_ERR_BROTLI_ENCODE_FULL) {
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
    const uint32_t alphabets[] = {1, 2, 3, 4, 5, 256};
    for (int it = 0; it < 3000; ++it) one(make(rnd() % 6001, alphabets[rnd() % 6]), 10 + (int)(rnd() % 15));
    for (int it = 0; it < 6; ++it) one(make(300000, alphabets[it]), it & 1 ? 24 : 16);
    for (int lgwin : {-2, 0, 9, 25}) {
        uint8_t x = 0, out[64];
        if (nx_brotli_encode_host(&x, 1, lgwin, out, sizeof out, nullptr) != NX_ERR_BROTLI_LGWIN) {
            fprintf(stderr, "lgwin %d was not refused\n", lgwin);
            return 1;
        }
    }
    printf("brotli_encode_host_fuzz: %lu items, %lu refused capacities, %lu uncompressed meta-blocks, %lu cut copies, %lu limited codes: clean\n",
           g_items, g_full, g_raw, g_split, g_limited);
    return 0;
}
