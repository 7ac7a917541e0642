// bzip2_decode_split.hpp — what the Bzip2Decoder handle (handlers.cpp) takes from bzip2_decode_split.hip beyond
// the C ABI: the split decode with a chain that starts at a given bit position (an item that is a stream still
// arriving, bzip2_decode_core.hpp SplitStart) and with the call's lists in memory the caller owns, so that it can
// copy them back: every candidate's position and CandResult and the item's SplitItem.  Private to the library.
#pragma once
#include <hip/hip_runtime.h>
#include "bzip2_decode_core.hpp"

namespace nx {
namespace bz2d {

struct SplitLists {
    uint32_t *seg_count = nullptr, *seg_place = nullptr, *first = nullptr, *count = nullptr, *total = nullptr, *cand_item = nullptr;
    int32_t* scan_status = nullptr;
    uint64_t* positions = nullptr;
    SplitItem* items = nullptr;
    CandResult* res = nullptr;
    void* mem = nullptr;
    size_t res_bytes = 0;
};
// The lists laid out from `mem` (nullptr: only the size is wanted); returns their bytes.  With decode the chain
// lists are one piece from S.first to the end of S.res.
size_t split_lists_layout(SplitLists& S, void* mem, uint32_t n, uint32_t max_blocks, bool decode);
// nx_bzip2_decode_batch_split with `start` (a device array of n entries, or nullptr: whole streams) and
// lists_mem (device memory of split_lists_layout(.., true) bytes, or nullptr: a stream-ordered allocation).
int32_t decode_split_launch(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint8_t* out, const uint64_t* out_off,
                            const uint32_t* out_cap, uint32_t* out_len, uint32_t* consumed, int32_t* status, uint32_t n,
                            uint32_t max_blocks, uint32_t* blocks, const SplitStart* start, void* lists_mem, hipStream_t st);

}  // namespace bz2d
}  // namespace nx
