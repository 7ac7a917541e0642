// bzip2_host_fuzz.cpp — a host-only sanitizer run of the bzip2 format core and host decoder: every record of
// the files named on the command line goes through nx_bzip2_stream_info and nx_bzip2_decode_host.  A file is
// a sequence of records, each a little-endian u32 stream length, a u32 output capacity and the stream's
// bytes; scripts/asan/bzip2_host_fuzz_inputs.py writes one with the tests' valid streams, every prefix of
// the small ones, the mutated streams and the mutation fuzz.  Inputs are heap copies of their exact length
// and outputs heap blocks of their exact capacity, so a read or write one byte outside either is a report.
// No GPU, no HIP:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       scripts/asan/bzip2_host_fuzz.cpp netty_amd/csrc/bzip2_decode_host.cpp -o bzip2_host_fuzz
//   python scripts/asan/bzip2_host_fuzz_inputs.py streams.bin && ./bzip2_host_fuzz streams.bin
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../include/netty_amd.h"

static unsigned long g_calls = 0, g_ok = 0;

static void one(const uint8_t* src, size_t n, size_t cap) {
    uint8_t* in = (uint8_t*)malloc(n ? n : 1);
    if (n) memcpy(in, src, n);
    uint32_t level = 0, crc = 0, empty = 0;
    const int32_t is = nx_bzip2_stream_info(n ? in : nullptr, n, &level, &crc, &empty);
    if (is == NX_OK && (level < 1 || level > 9)) abort();
    uint8_t* out = (uint8_t*)malloc(cap ? cap : 1);
    size_t ol = 0, co = 0;
    const int32_t st = nx_bzip2_decode_host(n ? in : nullptr, n, out, cap, &ol, &co);
    if (ol > cap || co > n || (st != NX_OK && co != 0)) abort();
    if (st == NX_OK && (is != NX_OK || co < 14)) abort();  // a stream that decodes has a header the walker accepts
    if (st != NX_OK && (st > NX_ERR_BZIP2_STREAM_ID || st < NX_ERR_BZIP2_RANDOMISED)) abort();
    g_calls += 1;
    g_ok += st == NX_OK;
    free(out);
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
        for (size_t q = 0; q + 8 <= f.size();) {
            uint32_t n = 0, cap = 0;
            memcpy(&n, f.data() + q, 4);
            memcpy(&cap, f.data() + q + 4, 4);
            q += 8;
            if (n > f.size() - q) return 3;
            one(f.data() + q, n, cap);
            q += n;
        }
    }
    printf("%lu decodes, %lu accepted, no report\n", g_calls, g_ok);
    return 0;
}
