// bzip2_encode_host_fuzz.cpp — a host-only sanitizer run of the bzip2 encoder's format core and host encoder:
// the shapes of tests/bzip2_encode_inputs.py (short inputs, runs around 255, count bytes, periodic blocks, the
// blocks that are hard for sorters, the table counts, every level, the lengths around a level-1 block's limit)
// and a few thousand seeded random inputs of 0..3 000 bytes over alphabets of 1, 2, 4 and 256 values at levels
// 1 and 9 go through nx_bzip2_encode_host into a heap block of exactly nx_bzip2_max_compressed_length bytes,
// then through nx_bzip2_decode_host, and the round trip is compared.  One more encode into a block one byte
// short of the stream must report NX_ERR_BZIP2_ENCODE_FULL.  No GPU, no HIP:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       scripts/asan/bzip2_encode_host_fuzz.cpp netty_amd/csrc/bzip2_encode_host.cpp \
//       netty_amd/csrc/bzip2_decode_host.cpp -o bzip2_encode_host_fuzz && ./bzip2_encode_host_fuzz
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../include/netty_amd.h"

static unsigned long g_items = 0, g_blocks_gt1 = 0;
static uint64_t g_seed = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    g_seed ^= g_seed << 13;
    g_seed ^= g_seed >> 7;
    g_seed ^= g_seed << 17;
    return (uint32_t)(g_seed >> 16);
}

static void one(const std::vector<uint8_t>& data, int level) {
    const size_t n = data.size(), cap = nx_bzip2_max_compressed_length(n, level);
    uint8_t* in = (uint8_t*)malloc(n ? n : 1);
    if (n) memcpy(in, data.data(), n);
    uint8_t* out = (uint8_t*)malloc(cap);
    size_t len = 0;
    if (nx_bzip2_encode_host(n ? in : nullptr, n, level, out, cap, &len) != NX_OK || len < 14 || len > cap) abort();
    uint8_t* back = (uint8_t*)malloc(n ? n : 1);
    size_t bl = 0, co = 0;
    if (nx_bzip2_decode_host(out, len, back, n, &bl, &co) != NX_OK || bl != n || co != len || (n && memcmp(back, in, n))) abort();
    uint8_t* tight = (uint8_t*)malloc(len - 1);
    size_t tl = 0;
    if (nx_bzip2_encode_host(n ? in : nullptr, n, level, tight, len - 1, &tl) != NX_ERR_BZIP2_ENCODE_FULL || tl != 0) abort();
    g_items += 1;
    g_blocks_gt1 += n + n / 4 > (size_t)level * 100000u - 6u;
    free(tight);
    free(back);
    free(out);
    free(in);
}

static std::vector<uint8_t> random_bytes(size_t n, uint32_t alphabet) {
    std::vector<uint8_t> v(n);
    for (size_t i = 0; i < n; ++i) v[i] = (uint8_t)(alphabet == 256 ? rnd() & 255u : 'a' + rnd() % alphabet);
    return v;
}
static std::vector<uint8_t> repeat(const std::string& unit, size_t k, const std::string& tail = "") {
    std::string s;
    for (size_t i = 0; i < k; ++i) s += unit;
    s += tail;
    return std::vector<uint8_t>(s.begin(), s.end());
}
static std::vector<uint8_t> text(size_t n) {
    static const char* words[] = {"the", "stream", "of", "blocks", "is", "sorted", "by", "rotation", "and", "coded", "with", "six", "tables"};
    std::string s;
    while (s.size() < n) {
        s += words[rnd() % 13];
        s += rnd() % 11 ? " " : ".\n";
    }
    s.resize(n);
    return std::vector<uint8_t>(s.begin(), s.end());
}

int main() {
    one({}, 9);
    for (size_t n : {1, 2, 3, 4, 5, 63, 64, 65}) one(random_bytes(n, 256), 9);
    {
        std::vector<uint8_t> all(256);
        for (int i = 0; i < 256; ++i) all[i] = (uint8_t)i;
        one(all, 9);
    }
    for (size_t n : {3, 4, 5, 254, 255, 256, 259, 260, 510, 1000}) one(std::vector<uint8_t>(n, 'x'), 9);
    one(std::vector<uint8_t>(4, 0), 9);
    one(std::vector<uint8_t>(5, 1), 9);
    one({0, 0, 0, 0, 1}, 9);
    one(repeat("hello world", 10), 9);
    one(repeat("ab", 500), 9);
    one(std::vector<uint8_t>(5000, 'a'), 9);
    one(repeat("abc", 333, "ab"), 9);
    {
        std::string a = "a", b = "ab";  // a Fibonacci word
        while (b.size() < 90000) {
            std::string c = b + a;
            a = b;
            b = c;
        }
        b.resize(90000);
        one(std::vector<uint8_t>(b.begin(), b.end()), 1);
    }
    one(repeat("ab", 49000), 1);
    one(random_bytes(95000, 2), 1);
    for (size_t n : {100, 400, 1000, 2000, 5000}) one(random_bytes(n, 256), 1);
    for (int level = 1; level <= 9; ++level) one(text(30000), level);
    for (size_t n = 99993; n <= 100002; ++n) one(random_bytes(n, 256), 1);
    {
        std::vector<uint8_t> v = random_bytes(99990, 256);
        v.insert(v.end(), 300, 'z');
        one(v, 1);
    }
    one(text(250000), 1);
    const unsigned long shaped = g_items;
    for (int k = 0; k < 4000; ++k) {
        static const uint32_t alphabets[] = {1, 2, 4, 256};
        one(random_bytes(rnd() % 3001u, alphabets[k & 3]), k & 4 ? 9 : 1);
    }
    printf("%lu shaped inputs, %lu random inputs, %lu of more than one block: every round trip equal, no report\n", shaped,
           g_items - shaped, g_blocks_gt1);
    return 0;
}
