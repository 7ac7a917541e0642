// decode_call_check.cpp — the host-only part of the synchronous decoders' calls
// (netty_amd/csrc/decode_call.hpp) on the CPU, under the sanitizers.  No GPU, no library:
//   clang++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       scripts/asan/decode_call_check.cpp -o /tmp/decode_call_check && /tmp/decode_call_check
// Checks the call frame (every null argument refused with nothing touched, null err_msg accepted, the list
// emptied and the outputs zeroed, finish / fail / skip_all and a publish after a fail), the layout of a
// decode launch's two lists for empty and non-empty lists in both placements (no two arrays overlap, all lie
// inside their buffer), and that field_offset agrees with offsetof for every member of the parameter structs.
#include <assert.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>
#include "../../netty_amd/csrc/decode_call.hpp"

using namespace nx::h;

struct Handle {
    MsgList ml;
};

static void call_frame() {
    const uint8_t in[4] = {1, 2, 3, 4};
    Handle h;
    h.ml.msgs.push_back({in, 4});
    h.ml.err = "stale";
    size_t consumed = 77, n_msgs = 77;
    const nx_msg* msgs = h.ml.msgs.data();
    const char* err = "stale";
    // every null argument: refused, and neither the list nor an output is touched
    assert(DecodeCall((Handle*)nullptr, in, 4, &consumed, &msgs, &n_msgs, &err).refused());
    assert(DecodeCall(&h, nullptr, 4, &consumed, &msgs, &n_msgs, &err).refused());
    assert(DecodeCall(&h, in, 4, nullptr, &msgs, &n_msgs, &err).refused());
    assert(DecodeCall(&h, in, 4, &consumed, nullptr, &n_msgs, &err).refused());
    assert(DecodeCall(&h, in, 4, &consumed, &msgs, nullptr, &err).refused());
    assert(consumed == 77 && n_msgs == 77 && msgs == h.ml.msgs.data() && !strcmp(err, "stale"));
    assert(h.ml.msgs.size() == 1 && h.ml.err == "stale");
    assert(!DecodeCall(&h, nullptr, 0, &consumed, &msgs, &n_msgs, &err).refused());  // no bytes: `in` may be null
    {   // construction empties the list and zeroes the outputs
        h.ml.msgs.push_back({in, 4});
        DecodeCall c(&h, in, 4, &consumed, &msgs, &n_msgs, &err);
        assert(!c.refused() && &c.ml() == &h.ml && c.n == 4 && c.rd == 0);
        assert(h.ml.msgs.empty() && h.ml.owned.empty() && h.ml.err.empty());
        assert(consumed == 0 && n_msgs == 0 && msgs == nullptr && err == nullptr);
        // finish: the read position, the messages, no text
        c.ml().owned.emplace_back(3, (uint8_t)9);
        c.ml().msgs.push_back({c.ml().owned.back().data(), 3});
        c.rd = 2;
        assert(c.finish(NX_OK) == NX_OK);
        assert(consumed == 2 && n_msgs == 1 && msgs == h.ml.msgs.data() && msgs[0].len == 3 && err == nullptr);
        // fail: the text, where the reader stops, the messages before the failure still there
        assert(c.fail(-40, "bad chunk", 3) == -40);
        assert(consumed == 3 && n_msgs == 1 && err && !strcmp(err, "bad chunk") && err == h.ml.err.c_str());
        // a publish after the fail says the same
        assert(c.finish(-40) == -40);
        assert(consumed == 3 && n_msgs == 1 && !strcmp(err, "bad chunk"));
    }
    {   // skip_all: everything consumed, nothing delivered; err_msg may be null throughout
        DecodeCall c(&h, in, 4, &consumed, &msgs, &n_msgs, nullptr);
        assert(!c.refused());
        assert(c.skip_all() == NX_OK && consumed == 4 && n_msgs == 0);
        assert(c.fail(-7, "text kept in the list", 1) == -7 && consumed == 1 && h.ml.err == "text kept in the list");
    }
}

// [at, at + count) elements of `width` bytes, inside a buffer of `bytes`, not overlapping the one before
static size_t span(size_t at, size_t count, size_t width, size_t bytes, size_t prev_end) {
    assert(at * width >= prev_end && (at + count) * width <= bytes);
    return (at + count) * width;
}

static void layout() {
    for (uint32_t k : {0u, 1u, 3u, 512u}) {
        for (uint32_t m : {0u, 1u, 2u, 511u}) {
            const DecodeLayout behind{true, k, m};
            assert(behind.listed() == k + m);
            // in_off / in_len: the items, then the jobs
            span(behind.job_off_at(), m, 8, 8ull * behind.listed() + 8, 8ull * k);
            span(behind.job_len_at(), m, 4, 4ull * behind.listed() + 4, 4ull * k);
            // aux1: the items' statuses, then the jobs' values
            span(behind.job_val_at(), m, 4, behind.aux1_bytes(), 4ull * k);
            const DecodeLayout apart{false, k, m};
            assert(apart.listed() == k);
            size_t end = span(apart.job_off_at(), m, 8, apart.aux1_bytes(), 0);
            end = span(apart.job_len_at(), m, 4, apart.aux1_bytes(), end);
            end = span(apart.job_val_at(), m, 4, apart.aux1_bytes(), end);
            assert(end == apart.aux1_bytes() && (m != 0 || end == 0));  // no jobs: nothing is allocated for them
        }
    }
    // Zstd's packed views: the arrays follow one another, 64-bit ones first, inside bytes(nb)
    for (uint32_t nb : {1u, 2u, 5u, 64u}) {
        std::vector<uint64_t> mem(ZstdGeometry::bytes(nb) / 8);
        const ZstdGeometry g(mem.data(), nb);
        uint8_t* base = reinterpret_cast<uint8_t*>(mem.data());
        assert((uint8_t*)g.in_off == base && (uint8_t*)g.out_off == base + 8ull * nb && (uint8_t*)g.in_len == base + 16ull * nb &&
               (uint8_t*)g.out_cap == base + 20ull * nb && (uint8_t*)(g.out_cap + nb) == base + ZstdGeometry::bytes(nb));
        for (uint32_t i = 0; i < nb; ++i) g.in_off[i] = g.out_off[i] = i, g.in_len[i] = g.out_cap[i] = i;  // every element writable
        std::vector<uint32_t> res(ZstdResults::bytes(nb) / 4);
        const ZstdResults r(res.data(), nb);
        assert(ZstdResults::bytes(nb) % 16 == 0 && ZstdResults::bytes(nb) >= 12ull * nb);
        assert(r.consumed == res.data() && r.out_len == res.data() + nb && (void*)r.status == (void*)(res.data() + 2ull * nb));
        for (uint32_t i = 0; i < nb; ++i) r.consumed[i] = r.out_len[i] = i, r.status[i] = -1;
    }
}

#define SAME(T, member) assert(field_offset(&T::member) == offsetof(T, member))

static void fields() {
    SAME(ZlibLaunch, in_off); SAME(ZlibLaunch, out_off); SAME(ZlibLaunch, sum_off); SAME(ZlibLaunch, in_len);
    SAME(ZlibLaunch, hist_len); SAME(ZlibLaunch, out_cap); SAME(ZlibLaunch, consumed); SAME(ZlibLaunch, out_len);
    SAME(ZlibLaunch, status); SAME(ZlibLaunch, sum);
    // what the kernels write is one piece at the block's end, behind everything that is uploaded
    static_assert(offsetof(ZlibLaunch, consumed) == 36 && sizeof(ZlibLaunch) == 56, "ZlibLaunch layout");
    SAME(Bzip2Geom, in_off); SAME(Bzip2Geom, out_off); SAME(Bzip2Geom, in_len); SAME(Bzip2Geom, out_cap); SAME(Bzip2Geom, start);
    static_assert(offsetof(Bzip2Geom, start) == 24 && sizeof(Bzip2Geom) == 48, "Bzip2Geom layout");
    SAME(Bzip2Scan, first); SAME(Bzip2Scan, count); SAME(Bzip2Scan, status);
    SAME(Bzip2Result, out_len); SAME(Bzip2Result, consumed); SAME(Bzip2Result, status); SAME(Bzip2Result, blocks);
    static_assert(sizeof(Bzip2Scan) == 12 && sizeof(Bzip2Result) == 16, "Bzip2 words");
}

int main() {
    call_frame();
    layout();
    fields();
    printf("decode_call_check: clean\n");
    return 0;
}
