// brotli_decode_host.cpp — the host entries of the Brotli decoder: nx_brotli_decode_host, a single-threaded
// decode of one stream from the functions of brotli_decode_core.hpp plus plain copy loops (the CPU check of the
// format core and the GPU tests' second opinion; not a product path), nx_brotli_transform_word, and
// nx_brotli_dictionary: the static dictionary of RFC 7932 Appendix A, embedded from csrc/brotli_dictionary.bin
// (the Makefile compiles in netty_amd/, and a stand-alone build names the file with NX_BROTLI_DICT_PATH).
#include <string.h>
#include <memory>
#include "../../include/netty_amd.h"
#include "brotli_decode_core.hpp"

#ifndef NX_BROTLI_DICT_PATH
#define NX_BROTLI_DICT_PATH "csrc/brotli_dictionary.bin"
#endif
#if !defined(__HIP_DEVICE_COMPILE__)
__asm__(".section .rodata\n"
        ".balign 16\n"
        ".global nx_brotli_dictionary_data\n"
        ".hidden nx_brotli_dictionary_data\n"
        "nx_brotli_dictionary_data:\n"
        ".incbin \"" NX_BROTLI_DICT_PATH "\"\n"
        ".global nx_brotli_dictionary_end\n"
        ".hidden nx_brotli_dictionary_end\n"
        "nx_brotli_dictionary_end:\n"
        ".byte 0\n"
        ".previous\n");
#endif
extern "C" const uint8_t nx_brotli_dictionary_data[];
extern "C" const uint8_t nx_brotli_dictionary_end[];

extern "C" const uint8_t* nx_brotli_dictionary(size_t* size) {
    if (size) *size = (size_t)(nx_brotli_dictionary_end - nx_brotli_dictionary_data);
    return nx_brotli_dictionary_data;
}

extern "C" int32_t nx_brotli_transform_word(uint32_t transform, const uint8_t* word, uint32_t len, uint8_t* out) {
    if (transform >= nx::brd::kTransforms || !word || !out || len < 4u || len > 24u) return NX_ERR_INVALID_ARG;
    uint8_t buf[nx::brd::kWordBuf];
    const uint32_t n = nx::brd::transform_word(transform, word, len, buf);
    memcpy(out, buf, n);
    return (int32_t)n;
}

extern "C" int32_t nx_brotli_decode_host(const uint8_t* in, size_t n, uint8_t* out, size_t out_cap, size_t* out_len, size_t* consumed,
                                         nx_brotli_decode_stats* stats) {
    using namespace nx::brd;
    if ((!in && n) || (!out && out_cap) || !out_len || !consumed) return NX_ERR_INVALID_ARG;
    *out_len = 0;
    *consumed = 0;
    if (stats) memset(stats, 0, sizeof(*stats));
    size_t dict_size = 0;
    const uint8_t* dict = nx_brotli_dictionary(&dict_size);
    if (dict_size != kDictBytes) return NX_ERR_INTERNAL;
    std::unique_ptr<Slot> W(new Slot);
    std::unique_ptr<State> Sp(new State);
    State& S = *Sp;
    uint8_t stage[1024];
    Op op;
    int32_t st = begin(S, in, n > 0xffffffffu ? 0xffffffffu : (uint32_t)n, out_cap > 0xffffffffu ? 0xffffffffu : (uint32_t)out_cap);
    uint32_t used = 0;
    while (st == NX_OK) {  // every pass consumes a meta-block header of the input
        MbHead H;
        st = metablock_header(S, W.get(), stats, &H);
        if (st != NX_OK) break;
        if (H.kind == kMbUncompressed) {
            memcpy(out + H.pos, in + H.src, H.len);
        } else if (H.kind == kMbCompressed) {
            do {  // every step produces a byte at least, of MLEN
                st = step(S, W.get(), dict, stats, stage, sizeof(stage), &op);
                if (st != NX_OK) break;
                uint8_t* o = out + op.pos;
                memcpy(o, stage, op.n_lit);
                o += op.n_lit;
                if (op.copy_len) {
                    for (uint32_t k = 0; k < op.copy_len; ++k) o[k] = *(o + k - op.dist);
                    S.p1 = o[op.copy_len - 1u];
                    S.p2 = o[op.copy_len - 2u];
                }
                memcpy(o, op.word, op.word_len);
            } while (!op.done);
            if (st != NX_OK) break;
        }
        if (S.is_last) {
            st = finish(S, &used);
            break;
        }
    }
    st = settle(S, st);
    *out_len = S.pos;
    if (st == NX_OK) *consumed = used;
    return st;
}
