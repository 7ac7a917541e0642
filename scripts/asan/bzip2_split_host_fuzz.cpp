// bzip2_split_host_fuzz.cpp — a host-only sanitizer run of the split bzip2 decode's host forms: every record of
// the files named on the command line goes through nx_bzip2_scan_host, nx_bzip2_decode_block_host at every
// candidate the scan lists and one bit to either side of it, and nx_bzip2_decode_split_host, whose answer must
// be nx_bzip2_decode_host's.  The record format is bzip2_host_fuzz.cpp's (u32 stream length, u32 output
// capacity, the bytes); scripts/asan/bzip2_split_host_fuzz_inputs.py writes one with the 40-block stream, the
// decoy streams and 200 mutants of them.  Inputs are heap copies of their exact length and outputs heap blocks
// of their exact capacity, so a read or write one byte outside either is a report.  No GPU, no HIP:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       scripts/asan/bzip2_split_host_fuzz.cpp netty_amd/csrc/bzip2_decode_host.cpp -o bzip2_split_host_fuzz
//   python scripts/asan/bzip2_split_host_fuzz_inputs.py streams.bin && ./bzip2_split_host_fuzz streams.bin
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../include/netty_amd.h"

static unsigned long g_streams = 0, g_ok = 0, g_cands = 0, g_blocks = 0;

static void one(const uint8_t* src, size_t n, size_t cap) {
    uint8_t* in = (uint8_t*)malloc(n ? n : 1);
    if (n) memcpy(in, src, n);
    const uint8_t* p = n ? in : nullptr;
    size_t count = 0;
    if (nx_bzip2_scan_host(p, n, nullptr, 0, &count) != NX_OK) abort();
    std::vector<uint64_t> pos(count + 1);
    size_t again = 0;
    if (nx_bzip2_scan_host(p, n, pos.data(), count, &again) != NX_OK || again != count) abort();
    uint8_t* out = (uint8_t*)malloc(cap ? cap : 1);
    const int32_t level = n >= 4 && in[3] >= '1' && in[3] <= '9' ? in[3] - '0' : 1;
    for (size_t k = 0; k < count; ++k) {
        const uint64_t at = pos[k] & ~NX_BZIP2_CAND_END;
        if (k && at <= (pos[k - 1] & ~NX_BZIP2_CAND_END)) abort();  // ascending
        if (at + 48 > 8 * (uint64_t)n) abort();
        for (int d = -1; d <= 1; ++d) {
            nx_bzip2_block_info info;
            const int32_t st = nx_bzip2_decode_block_host(p, n, at + (uint64_t)d, level, out, cap, &info);
            if (st != info.status) abort();
            if (st == NX_OK && (info.final_len > cap || info.end_bit > 8 * (uint64_t)n || info.stored_crc != info.computed_crc)) abort();
            if ((pos[k] & NX_BZIP2_CAND_END) && d == 0 && st != NX_ERR_BZIP2_BLOCK_HEADER && st != NX_ERR_BZIP2_TRUNCATED) abort();
            g_blocks += st == NX_OK;
        }
    }
    g_cands += count;
    uint8_t* ref = (uint8_t*)malloc(cap ? cap : 1);
    size_t ol = 0, co = 0, rl = 0, rc = 0, nb = 0;
    const int32_t st = nx_bzip2_decode_split_host(p, n, out, cap, &ol, &co, (size_t)-1, &nb);
    const int32_t rs = nx_bzip2_decode_host(p, n, ref, cap, &rl, &rc);
    if (st != rs || ol != rl || co != rc || ol > cap || memcmp(out, ref, ol) != 0 || nb > count) abort();
    if (count && nx_bzip2_decode_split_host(p, n, out, cap, &ol, &co, count - 1, &nb) != NX_ERR_BZIP2_DECODE_BLOCKS) abort();
    g_streams += 1;
    g_ok += st == NX_OK;
    free(ref);
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
    printf("%lu streams (%lu accepted), %lu candidates, %lu blocks decoded alone, split == serial, no report\n", g_streams, g_ok, g_cands,
           g_blocks);
    return 0;
}
