// decode_call.hpp — the host-only part of the synchronous decoders' calls (handlers.cpp): the call frame
// every decode() body starts with (DecodeCall), the layout arithmetic of a decode launch's two lists
// (DecodeLayout) and of a parameter block's fields (field_offset), and the parameter structs of the
// single-item decoders.  No HIP here: scripts/asan/decode_call_check.cpp drives it on the CPU.  The device
// side is nx::h::DecodeItems and nx::h::ParamBlock (handles.hpp).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string>
#include <vector>
#include "../../include/netty_amd.h"
#include "bzip2_decode_core.hpp"

namespace nx {
namespace h {

struct MsgList {
    std::vector<nx_msg> msgs;
    std::vector<std::vector<uint8_t>> owned;  // decoded payloads (stable storage)
    std::string err;
    void clear() {
        msgs.clear();
        owned.clear();
        err.clear();
    }
};

#pragma GCC visibility push(hidden)
// One decode() call of a handle: the argument check, the handle's message list emptied and the outputs
// zeroed, and the one place that writes the outputs.  A body constructs it first and leaves through
// finish, fail or skip_all; marking the decoder corrupted stays a line of the codec's own.
class DecodeCall {
public:
    const size_t n;  // the cumulation's length
    size_t rd = 0;   // the read position finish() publishes
    template <class D>
    DecodeCall(D* d, const uint8_t* in, size_t len, size_t* consumed, const nx_msg** msgs, size_t* n_msgs, const char** err_msg)
        : n(len), ml_(d ? &d->ml : nullptr), consumed_(consumed), msgs_(msgs), n_msgs_(n_msgs), err_msg_(err_msg) {
        if (!d || (!in && len) || !consumed || !msgs || !n_msgs) {  // err_msg may be null
            ml_ = nullptr;
            return;
        }
        ml_->clear();
        *consumed = 0;
        *msgs = nullptr;
        *n_msgs = 0;
        if (err_msg) *err_msg = nullptr;
    }
    bool refused() const { return !ml_; }  // the call returns NX_ERR_INVALID_ARG, nothing was touched
    MsgList& ml() const { return *ml_; }
    // publish the read position, the message list and the error text
    int32_t finish(int32_t r) {
        *consumed_ = rd;
        *msgs_ = ml_->msgs.data();
        *n_msgs_ = ml_->msgs.size();
        if (err_msg_) *err_msg_ = ml_->err.empty() ? nullptr : ml_->err.c_str();
        return r;
    }
    // the call fails with `text`, its reader left at consumed_at
    int32_t fail(int32_t code, const std::string& text, size_t consumed_at) {
        ml_->err = text;
        rd = consumed_at;
        return finish(code);
    }
    // a decoder that swallows its input (finished, or corrupted by an earlier call)
    int32_t skip_all() {
        rd = n;
        return finish(NX_OK);
    }

private:
    MsgList* ml_;
    size_t* consumed_;
    const nx_msg** msgs_;
    size_t* n_msgs_;
    const char** err_msg_;
};

// Where the arrays of a decode launch lie (DecodeItems): k items and a second list of m jobs.  The jobs'
// offsets and lengths either ride behind the items' in in_off / in_len, with aux1 holding the items'
// statuses and then the jobs' values (the Snappy kernel's layout), or stand apart in aux1 as
// [offsets | lengths | values] (the LZ decoders').  Counts are elements, sizes bytes.
struct DecodeLayout {
    bool jobs_behind_items;
    uint32_t k, m;
    uint32_t listed() const { return jobs_behind_items ? k + m : k; }  // entries of in_off and of in_len
    size_t job_off_at() const { return jobs_behind_items ? k : 0; }    // in in_off (behind) / aux1's 64-bit words (apart)
    size_t job_len_at() const { return jobs_behind_items ? k : 2ull * m; }       // in in_len / aux1's 32-bit words
    size_t job_val_at() const { return jobs_behind_items ? k : 3ull * m; }       // in aux1's 32-bit words
    size_t aux1_bytes() const { return jobs_behind_items ? 4ull * (k + m) + 4 : 16ull * m; }
};

// the offset of a member in a plain struct, from its member pointer
template <class T, class M>
inline size_t field_offset(M T::*member) {
    static const T probe{};
    return (size_t)(reinterpret_cast<const char*>(&(probe.*member)) - reinterpret_cast<const char*>(&probe));
}

// ---- the parameter blocks of the single-item launches: what goes up, then what the kernels write
struct ZlibLaunch {  // JdkZlibDecoder: one inflate launch and its checksum
    uint64_t in_off, out_off, sum_off;
    uint32_t in_len, hist_len, out_cap;
    uint32_t consumed, out_len;  // results from here on
    int32_t status;
    uint32_t sum;
};
struct Bzip2Geom {  // Bzip2Decoder: the one item of the scan and of the split decode
    uint64_t in_off, out_off;
    uint32_t in_len, out_cap;
    bz2d::SplitStart start;
};
struct Bzip2Scan {  // nx_bzip2_scan_batch's words of the item
    uint32_t first, count;
    int32_t status;
};
struct Bzip2Result {  // decode_split_launch's words of the item
    uint32_t out_len, consumed;
    int32_t status;
    uint32_t blocks;
};

// ZstdDecoder's geometry, packed: four arrays of nb, the 64-bit ones first; `base` is the host image or its
// device copy.  Its results lead the output buffer: three arrays of nb, padded to 16 bytes, then the slots.
struct ZstdGeometry {
    uint64_t *in_off, *out_off;
    uint32_t *in_len, *out_cap;
    static size_t bytes(uint32_t nb) { return 24ull * nb; }
    ZstdGeometry(void* base, uint32_t nb) {
        in_off = static_cast<uint64_t*>(base);
        out_off = in_off + nb;
        in_len = static_cast<uint32_t*>(static_cast<void*>(out_off + nb));
        out_cap = in_len + nb;
    }
};
struct ZstdResults {
    uint32_t *consumed, *out_len;
    int32_t* status;
    static size_t bytes(uint32_t nb) { return ((size_t)12 * nb + 15) / 16 * 16; }
    ZstdResults(void* base, uint32_t nb) {
        consumed = static_cast<uint32_t*>(base);
        out_len = consumed + nb;
        status = static_cast<int32_t*>(static_cast<void*>(out_len + nb));
    }
};
#pragma GCC visibility pop

}  // namespace h
}  // namespace nx
