// lzma_encode_host.cpp — the host entries of the LZMA encoder: nx_lzma_max_compressed_length and
// nx_lzma_encode_host, a single-threaded encode of one item from the functions of lzma_encode_core.hpp:
// the matcher and the packet coders the kernels run, so the bytes are the GPU's.  It is the CPU check of the
// format core, the GPU tests' second opinion, and the path of a handle whose lc + lp > 4.
#include <string.h>
#include <vector>
#include "../../include/netty_amd.h"
#include "encode_host.hpp"
#include "lzma_encode_core.hpp"

using namespace nx::lzma;
using nx::HostSink;

extern "C" size_t nx_lzma_max_compressed_length(size_t n) { return max_stream_bytes(n); }

extern "C" int32_t nx_lzma_check_props(int32_t lc, int32_t lp, int32_t pb, int32_t dict_size) {
    if (lc < 0 || lc > 8 || lp < 0 || lp > 4 || pb < 0 || pb > 4) return NX_ERR_LZMA_PROPS;
    if (dict_size < 0) return NX_ERR_LZMA_DICT_SIZE;
    return NX_OK;
}

extern "C" int64_t nx_lzma_encode_host(const uint8_t* in, size_t n, int32_t lc, int32_t lp, int32_t pb, int32_t dict_size,
                                       int32_t end_marker, uint8_t* out, size_t out_cap, nx_lzma_encode_stats* stats) {
    const int32_t bad = nx_lzma_check_props(lc, lp, pb, dict_size);
    if (bad != NX_OK) return bad;
    if ((!in && n) || (!out && out_cap) || n > 0xFFFFFFFFu) return NX_ERR_INVALID_ARG;
    static_assert(sizeof(nx_lzma_encode_stats) == sizeof(Stats), "stats layout");
    Stats st;
    memset(&st, 0, sizeof(st));
    if (out_cap < kHeaderBytes) return NX_ERR_LZMA_ENCODE_FULL;
    const Params P = {(uint32_t)lc, (uint32_t)lp, (uint32_t)pb, (uint32_t)dict_size, end_marker ? 1u : 0u};
    write_header(out, P, n);
    std::vector<uint64_t> seq(seq_cap(n));
    std::vector<uint16_t> probs(model_probs(P.lc, P.lp), (uint16_t)kProbInit);
    uint32_t ns = 0;
    if (!nx::host_match(seq, &ns, [&](uint64_t* table, uint32_t stamp, uint64_t* s, size_t cap) {
            return match_item(in, (uint32_t)n, P.dict_size, table, stamp, s, cap);
        }))
        return NX_ERR_INTERNAL;
    HostSink sink = {out, out_cap, kHeaderBytes, false};
    Coder<HostSink> C;
    C.init(probs.data(), &sink, &st, in, (uint32_t)n, seq.data(), ns, P);
    if (!nx::host_steps(C, sink, max_steps((uint32_t)n, ns))) return NX_ERR_INTERNAL;
    if (stats) memcpy(stats, &st, sizeof(st));
    return sink.full ? (int64_t)NX_ERR_LZMA_ENCODE_FULL : (int64_t)sink.at;
}
