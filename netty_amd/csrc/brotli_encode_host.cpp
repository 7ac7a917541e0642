// brotli_encode_host.cpp — the host entries of the Brotli encoder: nx_brotli_max_compressed_length and
// nx_brotli_encode_host, a single-threaded encode of one item from the functions of brotli_encode_core.hpp:
// the matcher, the walker and the meta-block encoder the kernels run, so the bytes are the GPU's.  It is the
// CPU check of the format core and the GPU tests' second opinion.
#include <string.h>
#include <memory>
#include <vector>
#include "../../include/netty_amd.h"
#include "brotli_encode_core.hpp"
#include "encode_host.hpp"

using namespace nx::brotli;
using nx::HostSink;

extern "C" size_t nx_brotli_max_compressed_length(size_t n) { return max_stream_bytes(n); }

extern "C" int64_t nx_brotli_encode_host(const uint8_t* in, size_t n, int32_t lgwin, uint8_t* out, size_t out_cap,
                                         nx_brotli_encode_stats* stats) {
    if (lgwin == -1) lgwin = 22;
    if (lgwin < 10 || lgwin > 24) return NX_ERR_BROTLI_LGWIN;
    if ((!in && n) || (!out && out_cap) || n > (256u << 20)) return NX_ERR_INVALID_ARG;
    static_assert(sizeof(nx_brotli_encode_stats) == sizeof(Stats), "stats layout");
    Stats st;
    memset(&st, 0, sizeof(st));
    std::unique_ptr<Work> work(new Work());
    std::vector<uint64_t> seq(seq_cap(n));
    uint32_t ns = 0;
    if (!nx::host_match(seq, &ns, [&](uint64_t* table, uint32_t stamp, uint64_t* s, size_t cap) {
            return match_item(in, (uint32_t)n, (uint32_t)lgwin, table, stamp, s, cap);
        }))
        return NX_ERR_INTERNAL;
    const HostSink sink = {out, out_cap, 0, false};
    Encoder<HostSink> E;
    E.init(work.get(), sink, &st, in, (uint32_t)n, seq.data(), ns, (uint32_t)lgwin, kFlagHeader);
    if (!nx::host_steps(E, E.out, max_steps((uint32_t)n, ns))) return NX_ERR_INTERNAL;
    if (stats) memcpy(stats, &st, sizeof(st));
    return E.out.full ? (int64_t)NX_ERR_BROTLI_ENCODE_FULL : (int64_t)E.out.at;
}
