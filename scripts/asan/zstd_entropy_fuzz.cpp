// zstd_entropy_fuzz.cpp — a host-only sanitizer run of nx_zstd_decode_host on the generated frames of
// tests/zstd_entropy.py (real FSE and Huffman coding at the format's edges).  The input file holds records of
// a 4-byte little-endian length, a flag byte and the frame; python tests/zstd_entropy.py FILE writes it.
// Every frame is decoded whole; of those flagged 1 (the two small frames of the corruption tests) also every
// truncation and every single-bit flip of every byte.  Inputs are heap copies of their exact length and
// outputs heap blocks of their exact capacity, so a read or write one byte outside either is a report.
// No GPU, no HIP:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       scripts/asan/zstd_entropy_fuzz.cpp netty_amd/csrc/zstd_decode_host.cpp -o zstd_entropy_fuzz
//   python tests/zstd_entropy.py frames.bin && ./zstd_entropy_fuzz frames.bin
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../include/netty_amd.h"

static unsigned long g_calls = 0, g_ok = 0;

static int32_t one(const uint8_t* src, size_t n, size_t cap) {
    uint8_t* in = (uint8_t*)malloc(n ? n : 1);
    if (n) memcpy(in, src, n);
    uint8_t* out = (uint8_t*)malloc(cap ? cap : 1);
    size_t ol = 0, co = 0;
    const int32_t st = nx_zstd_decode_host(n ? in : nullptr, n, cap ? out : nullptr, cap, &ol, &co);
    if (ol > cap || co > n || (st != NX_OK && co != 0) || (st == NX_OK && co != n)) abort();
    g_calls += 1;
    g_ok += st == NX_OK;
    free(out);
    free(in);
    return st;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* fp = fopen(argv[1], "rb");
    if (!fp) return 2;
    unsigned long frames = 0;
    uint8_t head[5];
    while (fread(head, 1, 5, fp) == 5) {
        const size_t n = (size_t)head[0] | (size_t)head[1] << 8 | (size_t)head[2] << 16 | (size_t)head[3] << 24;
        std::vector<uint8_t> f(n);
        if (fread(f.data(), 1, n, fp) != n) return 2;
        frames += 1;
        uint32_t kind = 0, flags = 0;
        uint64_t fb = 0, bound = 0;
        if (nx_zstd_next_frame(f.data(), n, &kind, &fb, &bound, &flags) != NX_OK || fb != n) abort();  // the generator's frames are whole
        if (one(f.data(), n, (size_t)bound) != NX_OK) abort();
        if (head[4] != 1) continue;
        for (size_t k = 0; k < n; ++k)
            if (one(f.data(), k, (size_t)bound) == NX_OK) abort();  // every truncation fails
        for (size_t k = 0; k < n; ++k)
            for (int bit = 0; bit < 8; ++bit) {
                f[k] ^= (uint8_t)(1u << bit);
                one(f.data(), n, 4096);
                f[k] ^= (uint8_t)(1u << bit);
            }
    }
    fclose(fp);
    printf("%lu frames, %lu decodes, %lu accepted, no report\n", frames, g_calls, g_ok);
    return 0;
}
