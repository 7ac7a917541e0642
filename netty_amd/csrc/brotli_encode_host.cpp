// brotli_encode_host.cpp — the host entries of the Brotli encoder: nx_brotli_max_compressed_length and
// nx_brotli_encode_host, a single-threaded encode of one item from the functions of brotli_encode_core.hpp:
// the matcher, the walker and the meta-block encoder the kernels run, so the bytes are the GPU's.  It is the
// CPU check of the format core and the GPU tests' second opinion.
#include <stdlib.h>
#include <string.h>
#include <memory>
#include <vector>
#include "../../include/netty_amd.h"
#include "brotli_encode_core.hpp"

namespace {
using namespace nx::brotli;

struct HostSink {
    uint8_t* out;
    size_t cap, at;
    bool full;
    void put(uint8_t b) {
        if (at < cap) out[at] = b;
        else full = true;
        ++at;
    }
};
}  // namespace

extern "C" size_t nx_brotli_max_compressed_length(size_t n) { return max_stream_bytes(n); }

extern "C" int64_t nx_brotli_encode_host(const uint8_t* in, size_t n, int32_t lgwin, uint8_t* out, size_t out_cap,
                                         nx_brotli_encode_stats* stats) {
    if (lgwin == -1) lgwin = 22;
    if (lgwin < 10 || lgwin > 24) return NX_ERR_BROTLI_LGWIN;
    if ((!in && n) || (!out && out_cap) || n > (256u << 20)) return NX_ERR_INVALID_ARG;
    static_assert(sizeof(nx_brotli_encode_stats) == sizeof(Stats), "stats layout");
    Stats st;
    memset(&st, 0, sizeof(st));
    std::unique_ptr<uint64_t, decltype(&free)> table(static_cast<uint64_t*>(calloc((size_t)1 << kHashLog, 8)), &free);
    std::unique_ptr<Work> work(new Work());
    std::vector<uint64_t> seq(seq_cap(n));
    if (!table) return NX_ERR_INTERNAL;
    const uint32_t ns = match_item(in, (uint32_t)n, (uint32_t)lgwin, table.get(), 1u, seq.data(), seq.size());
    if (ns == ~0u) return NX_ERR_INTERNAL;
    const HostSink sink = {out, out_cap, 0, false};
    Encoder<HostSink> E;
    E.init(work.get(), sink, &st, in, (uint32_t)n, seq.data(), ns, (uint32_t)lgwin, kFlagHeader);
    for (uint64_t left = max_steps((uint32_t)n, ns); !E.done && !E.out.full; --left) {
        if (left == 0u) return NX_ERR_INTERNAL;
        E.step();
    }
    if (stats) memcpy(stats, &st, sizeof(st));
    return E.out.full ? (int64_t)NX_ERR_BROTLI_ENCODE_FULL : (int64_t)E.out.at;
}
