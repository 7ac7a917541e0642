// encode_host.hpp — what the single-threaded host encoders of the sequence codecs share (lzma_encode_host.cpp,
// brotli_encode_host.cpp): the bounded byte sink, the matcher's run over a fresh table and the bounded step loop.
// No HIP here: scripts/asan/*_encode_host_fuzz.cpp build the host encoders with a plain compiler.
#pragma once
#include <stdlib.h>
#include <memory>
#include <vector>
#include "lz_seq_core.hpp"

namespace nx {

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

// The sequences of an item into seq (sized by the core's seq_cap) over a zeroed table at stamp 1:
// match(table, stamp, seq, cap) is the core's match_item on the item.  False: no table, or seq would be passed.
template <class Match>
inline bool host_match(std::vector<uint64_t>& seq, uint32_t* ns, Match&& match) {
    std::unique_ptr<uint64_t, decltype(&free)> table(static_cast<uint64_t*>(calloc((size_t)1 << lzseq::kHashLog, 8)), &free);
    if (!table) return false;
    *ns = match(table.get(), 1u, seq.data(), seq.size());
    return *ns != ~0u;
}

// c.step() until c is done or the sink is full.  False: `most` steps did not get there.
template <class Coder>
inline bool host_steps(Coder& c, const HostSink& sink, uint64_t most) {
    for (; !c.done && !sink.full; --most) {
        if (most == 0u) return false;
        c.step();
    }
    return true;
}

}  // namespace nx
