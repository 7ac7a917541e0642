// encode_items.hpp — the host-only part of the synchronous encoders' launch staging (handlers.cpp): the
// table of a launch's items with its output slot cursor, the cutter of fixed-stride pieces, and the block
// buffer of Lz4FrameEncoder and ZstdEncoder.  No HIP here: scripts/asan/encode_items_check.cpp drives it
// on the CPU.  The device side is nx::h::EncodeItems (handles.hpp).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

#pragma GCC visibility push(hidden)
namespace nx {
namespace h {

// [0, n) in pieces of `stride` bytes, the last one shorter: fn(offset, length)
template <class F>
inline void for_each_piece(size_t n, size_t stride, F&& fn) {
    for (size_t q = 0; q < n; q += stride) fn(q, n - q < stride ? n - q : stride);
}

// The items of one encode launch: where each one's input lies and how long it is, and its output slot.
// Slots follow one another from 0; how large an item's slot is (bound, rounding) is its codec's rule.
struct ItemTable {
    std::vector<uint64_t> in_off, out_off;
    std::vector<uint32_t> in_len;
    uint64_t out_bytes = 0;  // the slot cursor: the bytes of all slots so far
    void add(uint64_t off, uint32_t len, uint64_t slot_bytes) {
        in_off.push_back(off);
        in_len.push_back(len);
        out_off.push_back(out_bytes);
        out_bytes += slot_bytes;
    }
    uint32_t size() const { return (uint32_t)in_len.size(); }
};

// encode() of a handler with a block buffer (Lz4FrameEncoder.java:241-248, ZstdEncoder.java:136-143): the
// whole blocks of buf + in[0, n) go to flush(src, bytes) in one call, what is left stays in buf.  Returns
// what flush returned; a failed flush (< 0) leaves buf as it was.
template <class Flush>
inline int64_t write_blocks(std::vector<uint8_t>& buf, size_t block_size, const uint8_t* in, size_t n, Flush&& flush) {
    const size_t have = buf.size();
    const size_t full = (have + n) / block_size * block_size;
    if (full == 0) {
        buf.insert(buf.end(), in, in + n);
        return 0;
    }
    std::vector<uint8_t> joined;
    const uint8_t* src = in;
    if (have) {
        joined.reserve(full);
        joined.insert(joined.end(), buf.begin(), buf.end());
        joined.insert(joined.end(), in, in + (full - have));
        src = joined.data();
    }
    const int64_t w = flush(src, full);
    if (w < 0) return w;
    buf.assign(in + (full - have), in + n);
    return w;
}

}  // namespace h
}  // namespace nx
#pragma GCC visibility pop
