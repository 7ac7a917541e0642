// zstd_walk_fuzz.cpp — a host-only sanitizer run of the Zstandard walker and host decoder: every truncation
// and every single-byte mutation (three values a byte) of the frames named on the command line goes through
// nx_zstd_next_frame and nx_zstd_decode_host_ex (flags 0 and NX_ZSTD_DECODE_VERIFY_CHECKSUM).  Inputs are
// heap copies of their exact length and outputs heap blocks of their exact capacity, so a read or write one
// byte outside either is a report.  No GPU, no HIP:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       scripts/asan/zstd_walk_fuzz.cpp netty_amd/csrc/zstd_decode_host.cpp -o zstd_walk_fuzz
//   ./zstd_walk_fuzz frame1.zst frame2.zst ...
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../include/netty_amd.h"

static unsigned long g_calls = 0, g_ok = 0;

static void one(const uint8_t* src, size_t n) {
    uint8_t* in = (uint8_t*)malloc(n ? n : 1);
    if (n) memcpy(in, src, n);
    uint32_t kind = 0, flags = 0;
    uint64_t fb = 0, bound = 0;
    const int32_t ws = nx_zstd_next_frame(n ? in : nullptr, n, &kind, &fb, &bound, &flags);
    if (ws == NX_OK && fb > n) abort();  // a frame is never longer than the bytes it was found in
    size_t cap = ws == NX_OK && bound < (1u << 20) ? (size_t)bound : 4096;
    for (uint32_t f = 0; f < 2; ++f) {
        uint8_t* out = (uint8_t*)malloc(cap ? cap : 1);
        size_t ol = 0, co = 0;
        const int32_t st = nx_zstd_decode_host_ex(n ? in : nullptr, n, cap ? out : nullptr, cap, &ol, &co, f);
        if (ol > cap || co > n || (st != NX_OK && co != 0)) abort();
        if (st == NX_OK && ws == NX_OK && kind == NX_ZSTD_KIND_FRAME && (co != fb || ol > bound)) abort();  // the walker's promises
        g_calls += 1;
        g_ok += st == NX_OK;
        free(out);
    }
    free(in);
}

int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        FILE* fp = fopen(argv[a], "rb");
        if (!fp) return 2;
        std::vector<uint8_t> f;
        uint8_t buf[4096];
        for (size_t r; (r = fread(buf, 1, sizeof buf, fp)) > 0;) f.insert(f.end(), buf, buf + r);
        fclose(fp);
        one(f.data(), f.size());
        for (size_t k = 0; k < f.size(); ++k) one(f.data(), k);
        for (size_t k = 0; k < f.size(); ++k)
            for (uint8_t x : {(uint8_t)0x01, (uint8_t)0x80, (uint8_t)0xFF}) {
                f[k] ^= x;
                one(f.data(), f.size());
                f[k] ^= x;
            }
    }
    printf("%lu decodes, %lu accepted, no report\n", g_calls, g_ok);
    return 0;
}
