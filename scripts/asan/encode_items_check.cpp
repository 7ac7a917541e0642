// encode_items_check.cpp — the host-only launch staging (netty_amd/csrc/encode_items.hpp) on the CPU, under
// the sanitizers.  No GPU, no library:
//   clang++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       scripts/asan/encode_items_check.cpp -o /tmp/encode_items_check && /tmp/encode_items_check
// Checks that the cutter's pieces tile [0, n) exactly (one level, and ZstdEncoder's block-then-slice cut),
// that the slot cursor is monotone, and that the block buffer hands every byte written either to the flush
// or to the buffer, in order, and is unchanged after a failed flush.
#include <assert.h>
#include <stdio.h>
#include <numeric>
#include "../../netty_amd/csrc/encode_items.hpp"

using nx::h::ItemTable;
using nx::h::for_each_piece;
using nx::h::write_blocks;

static void check_tiling(const ItemTable& t, size_t n, size_t max_len) {
    uint64_t at = 0, slot = 0;
    for (uint32_t i = 0; i < t.size(); ++i) {
        assert(t.in_off[i] == at && t.in_len[i] > 0 && t.in_len[i] <= max_len);
        at += t.in_len[i];
        assert(t.out_off[i] == slot && (i == 0 || t.out_off[i] > t.out_off[i - 1]));  // monotone, no slot shared
        slot += t.in_len[i] + 16;
    }
    assert(at == n && t.out_bytes == slot);
}

static void cutter() {
    for (size_t stride : {1u, 7u, 64u, 65535u, 65536u}) {
        for (size_t n : {(size_t)0, (size_t)1, stride - 1, stride, stride + 1, 3 * stride, 3 * stride + 5}) {
            ItemTable t;
            for_each_piece(n, stride, [&](size_t off, size_t len) { t.add(off, (uint32_t)len, len + 16); });
            assert(t.size() == (n + stride - 1) / stride);
            check_tiling(t, n, stride);
        }
    }
    // ZstdEncoder: blocks of bs bytes, each cut into slices of 65536
    const size_t slice = 65536;
    for (size_t bs : {(size_t)64, slice - 1, slice, slice + 1, (size_t)100000, 3 * slice + 9}) {
        for (size_t n : {(size_t)0, (size_t)1, bs - 1, bs, bs + 1, 2 * bs + 7}) {
            ItemTable t;
            size_t pieces = 0;
            for_each_piece(n, bs, [&](size_t b, size_t blen) {
                pieces += (blen + slice - 1) / slice;
                for_each_piece(blen, slice, [&](size_t q, size_t len) { t.add(b + q, (uint32_t)len, len + 16); });
            });
            assert(t.size() == pieces);
            check_tiling(t, n, slice < bs ? slice : bs);
            for (uint32_t i = 0; i < t.size(); ++i)  // no item reaches over a block's end
                assert(t.in_off[i] / bs == (t.in_off[i] + t.in_len[i] - 1) / bs);
        }
    }
}

static void block_buffer() {
    const size_t bs = 64;
    std::vector<uint8_t> in(3 * bs);
    std::iota(in.begin(), in.end(), (uint8_t)100);
    for (size_t have = 0; have < bs; ++have) {
        for (size_t n = 0; n <= 3 * bs; ++n) {
            const std::vector<uint8_t> before(have, (uint8_t)7);
            const std::vector<uint8_t> data(in.begin(), in.begin() + n);  // exactly n bytes: a read past them is caught
            std::vector<uint8_t> all(before);
            all.insert(all.end(), data.begin(), data.end());
            // a recording flush: called at most once, with whole blocks; flushed + buffer == everything written
            std::vector<uint8_t> buf(before), flushed;
            int calls = 0;
            const int64_t w = write_blocks(buf, bs, data.data(), n, [&](const uint8_t* src, size_t bytes) {
                ++calls;
                assert(bytes > 0 && bytes % bs == 0);
                flushed.assign(src, src + bytes);
                return (int64_t)bytes;
            });
            assert(w == (int64_t)flushed.size() && calls == ((have + n) / bs ? 1 : 0));
            assert(buf.size() == (have + n) % bs);
            flushed.insert(flushed.end(), buf.begin(), buf.end());
            assert(flushed == all);
            // a failing flush: its status comes back and the buffer is as it was
            std::vector<uint8_t> buf2(before);
            const int64_t f = write_blocks(buf2, bs, data.data(), n, [&](const uint8_t*, size_t) { return (int64_t)-100; });
            if ((have + n) / bs) assert(f == -100 && buf2 == before);
            else assert(f == 0 && buf2 == all);
        }
    }
}

int main() {
    cutter();
    block_buffer();
    printf("encode_items_check: clean\n");
    return 0;
}
