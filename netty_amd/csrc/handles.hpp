// handles.hpp — device context, the synchronous handles' launch staging (EncodeItems, DecodeItems, ParamBlock)
// and the Snappy handler handles shared by the synchronous handler layer (handlers.cpp) and the asynchronous cross-channel batcher
// (batcher.cpp).  Private to the library.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <atomic>
#include <deque>
#include <set>
#include <string>
#include <vector>
#include "../../include/netty_amd.h"
#include "decode_call.hpp"
#include "encode_items.hpp"
#include "nx_common.hpp"
#include "workspace.hpp"

namespace nx {

// memcpy of n bytes that may be zero with a null source (an empty message or cumulation: memcpy's
// arguments must be valid pointers even for n = 0; found by the UBSan run, profiles/r05/s35)
inline void copy_bytes(void* dst, const void* src, size_t n) {
    if (n) memcpy(dst, src, n);
}

namespace h {

// ------------------------------------------------------------------ device context
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    bool ensure(size_t n) {
        if (n <= cap) return true;
        size_t c = cap ? cap : 4096;
        while (c < n) c += c / 2 + 4096;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        if (hipMalloc(&p, c) != hipSuccess) return false;
        cap = c;
        return true;
    }
    template <class T>
    T* as() const { return static_cast<T*>(p); }
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
};

struct Gpu {
    hipStream_t s = nullptr;
    int dev = 0;
    bool ok = false;
    uint32_t held = 0;  // bit per WsKind whose shared workspace this handle holds (workspace.hpp)
    // a launch's bytes and its per-item arrays, named for what the kernels take them as; aux0 and aux1 are
    // the codec's own (a checksum per item, FastLZ's limits and levels, the decoders' checksum lists)
    DevBuf din, dout, in_off, out_off, in_len, out_len, status, aux0, aux1;
    Gpu() {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return;
        if (hipGetDevice(&dev) != hipSuccess) return;
        if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return;
        ok = nx::crc_tables_init() == NX_OK;
    }
    // Reserve the device workspace of kind k for this handle's launches, at construction (its
    // encode/decode calls then never allocate: they run in a NoGrowScope).
    bool hold(WsKind k) {
        if (!ok || ws_hold(k, dev, kHandleHoldUnits, s) != NX_OK) return false;
        held |= 1u << (int)k;
        return true;
    }
    ~Gpu() {
        if (s) (void)hipStreamSynchronize(s);
        for (int k = 0; k < (int)WsKind::Count; ++k)
            if (held & (1u << k)) ws_unhold((WsKind)k, dev);
        if (s) {
            ws_forget_stream(s);
            (void)hipStreamDestroy(s);
        }
    }
    bool h2d(void* d, const void* h, size_t n) { return n == 0 || hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, s) == hipSuccess; }
    bool d2h(void* h, const void* d, size_t n) { return n == 0 || hipMemcpyAsync(h, d, n, hipMemcpyDeviceToHost, s) == hipSuccess; }
    bool sync() { return hipStreamSynchronize(s) == hipSuccess; }
};

#pragma GCC visibility push(hidden)  // the library exports its C ABI, not its staging
// One encode launch of a synchronous handle: the item table, staged into the handle's named arrays, and
// what comes back.  The order of its copies and syncs is the encoders' own: every array is sized before
// the first upload; the input bytes go up, then in_off, out_off and in_len; the lengths (and what else
// the codec reads) come back with one sync, the items' bytes with a second.
struct EncodeItems : ItemTable {
    Gpu& g;
    std::vector<uint32_t> len;  // fetch(): the bytes each item produced
    std::vector<int32_t> st;    // fetch(true, ..): each item's status
    explicit EncodeItems(Gpu& gpu) : g(gpu) {}
    // Size the arrays (aux0 / aux1 too, for the codec's own uploads) and upload src[0, n) to din + din_prefix
    // and the three item arrays.
    int32_t stage(const uint8_t* src, size_t n, size_t din_prefix = 0, size_t aux0_bytes = 0, size_t aux1_bytes = 0) {
        const size_t k = size();
        if (!g.din.ensure(din_prefix + n) || !g.dout.ensure(out_bytes) || !g.in_off.ensure(8 * k) || !g.out_off.ensure(8 * k) ||
            !g.in_len.ensure(4 * k) || !g.out_len.ensure(4 * k) || !g.status.ensure(4 * k) || !g.aux0.ensure(aux0_bytes) ||
            !g.aux1.ensure(aux1_bytes))
            return NX_ERR_HIP;
        const bool ok = g.h2d(g.din.as<uint8_t>() + din_prefix, src, n) && g.h2d(g.in_off.p, in_off.data(), 8 * k) &&
                        g.h2d(g.out_off.p, out_off.data(), 8 * k) && g.h2d(g.in_len.p, in_len.data(), 4 * k);
        return ok ? NX_OK : NX_ERR_HIP;
    }
    // a kernel's parameters, in the types it takes them
    const uint8_t* d_in() const { return g.din.as<uint8_t>(); }
    const uint64_t* d_in_off() const { return g.in_off.as<uint64_t>(); }
    const uint32_t* d_in_len() const { return g.in_len.as<uint32_t>(); }
    uint8_t* d_out() const { return g.dout.as<uint8_t>(); }
    const uint64_t* d_out_off() const { return g.out_off.as<uint64_t>(); }
    uint32_t* d_out_len() const { return g.out_len.as<uint32_t>(); }
    int32_t* d_status() const { return g.status.as<int32_t>(); }
    // The lengths, the statuses if asked for, and one more 32-bit value per item (a checksum) from d_extra if
    // given; then the sync.
    bool fetch(bool with_status, const void* d_extra = nullptr, uint32_t* extra = nullptr) {
        const size_t k = size();
        len = std::vector<uint32_t>(k);
        st = std::vector<int32_t>(with_status ? k : 0);
        return g.d2h(len.data(), g.out_len.p, 4 * k) && (!with_status || g.d2h(st.data(), g.status.p, 4 * k)) &&
               (!d_extra || g.d2h(extra, d_extra, 4 * k)) && g.sync();
    }
    int32_t first_status() const {  // in item order
        for (int32_t s : st)
            if (s != NX_OK) return s;
        return NX_OK;
    }
    // first_status, and NX_ERR_INVALID_ARG where the items' bytes, packed, would pass out_cap: whichever
    // an item reaches first
    int32_t check_packed(size_t out_cap) const {
        size_t op = 0;
        for (uint32_t i = 0; i < size(); ++i) {
            if (st[i] != NX_OK) return st[i];
            if (op + len[i] > out_cap) return NX_ERR_INVALID_ARG;
            op += len[i];
        }
        return NX_OK;
    }
    // Gather 1: an item's bytes (and nothing else of its slot) straight to their place in the caller's
    // buffer.  The caller syncs once after its last item.
    bool copy_item(uint32_t i, uint8_t* dst) { return g.d2h(dst, d_out() + out_off[i], len[i]); }
    // A whole call of one item whose batch call takes capacities in out_len (LZMA, Brotli): in[0, n) into a slot
    // of `bound` bytes, of which the kernel may write min(out_cap, bound); call(*this) is the batch call; the
    // item's bytes to out, synced.  Returns their number, or the call's or the item's status.
    template <class Call>
    int64_t encode_one(const uint8_t* in, size_t n, size_t bound, uint8_t* out, size_t out_cap, Call&& call) {
        const uint32_t cap = (uint32_t)(out_cap < bound ? out_cap : bound);
        add(0, (uint32_t)n, (bound + 15) / 16 * 16);
        int32_t r = stage(in, n);
        if (r != NX_OK) return r;
        if (!g.h2d(g.out_len.p, &cap, 4)) return NX_ERR_HIP;
        r = call(*this);
        if (r != NX_OK) return r;
        if (!fetch(true)) return NX_ERR_HIP;
        if (st[0] != NX_OK) return st[0];
        if (!copy_item(0, out) || !g.sync()) return NX_ERR_HIP;
        return (int64_t)len[0];
    }
    // ... every item, one behind the other from out + *op (advanced); synced
    bool copy_packed(uint8_t* out, size_t* op) {
        bool ok = true;
        for (uint32_t i = 0; i < size() && ok; ++i) {
            ok = copy_item(i, out + *op);
            *op += len[i];
        }
        return g.sync() && ok;
    }
    // Gather 2 (Zstd): one copy of the slots up to the last frame's end, then the frames are packed on the
    // host (a small block_size makes thousands of frames a call: a copy each would cost more than the bytes
    // between them).
    bool copy_span_packed(uint8_t* out, size_t* op) {
        std::vector<uint8_t> slots((size_t)out_off.back() + len.back());
        if (!g.d2h(slots.data(), g.dout.p, slots.size()) || !g.sync()) return false;
        for (uint32_t i = 0; i < size(); ++i) {
            copy_bytes(out + *op, slots.data() + out_off[i], len[i]);
            *op += len[i];
        }
        return true;
    }
};

// One decode launch of a synchronous handle with item lists (SnappyFrameDecoder; the FastLZ, LZF and LZ4
// decoders): the items to decode, each with its slot of dout, and a second list of jobs (Snappy's raw chunks
// to CRC, the LZ decoders' blocks to checksum), as DecodeLayout lays them out.  stage() sizes every array,
// then uploads: the input bytes, in_off, out_off, in_len, the codec's per-item words (the lengths the LZ
// blocks must decode to, into out_len; Snappy's expected CRCs or FastLZ's readable bytes, into aux0), then
// the jobs where they stand apart.  fetch() brings back what the kernels report per item and per job, and
// syncs.  How the decoded bytes come back is the codec's: Snappy copies each chunk's own bytes (copy_item),
// the LZ decoders their slots in one piece (fetch's `slots`).
struct DecodeItems : ItemTable {
    Gpu& g;
    const bool jobs_behind_items;
    std::vector<uint64_t> job_off;
    std::vector<uint32_t> job_len;
    std::vector<uint32_t> len, used, job_val;  // fetch(): bytes produced and input used per item (Snappy); a value per job
    std::vector<int32_t> st;                   // fetch(): each item's status
    DecodeItems(Gpu& gpu, bool behind) : g(gpu), jobs_behind_items(behind) {}
    void add_job(uint64_t off, uint32_t n) {
        job_off.push_back(off);
        job_len.push_back(n);
    }
    uint32_t jobs() const { return (uint32_t)job_len.size(); }
    DecodeLayout layout() const { return {jobs_behind_items, size(), jobs()}; }
    // expected_len and item_word: a value per item or nullptr (that array is then neither sized nor uploaded)
    int32_t stage(const uint8_t* src, size_t n, const std::vector<uint32_t>* expected_len, const std::vector<uint32_t>* item_word) {
        const DecodeLayout L = layout();
        const size_t k = L.k, m = L.m, listed = L.listed();
        if (!g.din.ensure(n + 1) || !g.dout.ensure(out_bytes + 16) || !g.in_off.ensure(8 * listed + 8) || !g.out_off.ensure(8 * k + 8) ||
            !g.in_len.ensure(4 * listed + 4) || !g.out_len.ensure(4 * k + 4) || !g.status.ensure(4 * k + 4) ||
            !g.aux0.ensure(item_word ? 4 * k + (jobs_behind_items ? 4 : 0) : 0) || !g.aux1.ensure(L.aux1_bytes()))
            return NX_ERR_HIP;
        std::vector<uint64_t> off_all;  // jobs behind the items: one upload of each array holds both lists
        std::vector<uint32_t> len_all;
        if (jobs_behind_items && m) {
            off_all = in_off;
            off_all.insert(off_all.end(), job_off.begin(), job_off.end());
            len_all = in_len;
            len_all.insert(len_all.end(), job_len.begin(), job_len.end());
        }
        const uint64_t* h_off = off_all.empty() ? in_off.data() : off_all.data();
        const uint32_t* h_len = len_all.empty() ? in_len.data() : len_all.data();
        bool ok = g.h2d(g.din.p, src, n) && g.h2d(g.in_off.p, h_off, 8 * listed) && g.h2d(g.out_off.p, out_off.data(), 8 * k) &&
                  g.h2d(g.in_len.p, h_len, 4 * listed) && (!expected_len || g.h2d(g.out_len.p, expected_len->data(), 4 * k)) &&
                  (!item_word || g.h2d(g.aux0.p, item_word->data(), 4 * k));
        if (!jobs_behind_items) ok = ok && g.h2d(d_job_off(), job_off.data(), 8 * m) && g.h2d(d_job_len(), job_len.data(), 4 * m);
        return ok ? NX_OK : NX_ERR_HIP;
    }
    // a kernel's parameters, in the types it takes them
    const uint8_t* d_in() const { return g.din.as<uint8_t>(); }
    const uint64_t* d_in_off() const { return g.in_off.as<uint64_t>(); }
    const uint32_t* d_in_len() const { return g.in_len.as<uint32_t>(); }
    uint8_t* d_out() const { return g.dout.as<uint8_t>(); }
    const uint64_t* d_out_off() const { return g.out_off.as<uint64_t>(); }
    uint32_t* d_out_len() const { return g.out_len.as<uint32_t>(); }
    uint32_t* d_item_word() const { return g.aux0.as<uint32_t>(); }
    uint32_t* d_used() const { return g.status.as<uint32_t>(); }  // Snappy: the input each item used
    int32_t* d_status() const { return jobs_behind_items ? g.aux1.as<int32_t>() : g.status.as<int32_t>(); }
    // the second list from job `from` on
    uint64_t* d_job_off(uint32_t from = 0) const {
        return (jobs_behind_items ? g.in_off.as<uint64_t>() : g.aux1.as<uint64_t>()) + layout().job_off_at() + from;
    }
    uint32_t* d_job_len(uint32_t from = 0) const {
        return (jobs_behind_items ? g.in_len.as<uint32_t>() : g.aux1.as<uint32_t>()) + layout().job_len_at() + from;
    }
    uint32_t* d_job_val(uint32_t from = 0) const { return g.aux1.as<uint32_t>() + layout().job_val_at() + from; }
    // Snappy: each item's length, used input and status; the LZ decoders: each item's status, then the slots
    // in one piece into `slots`.  Then the jobs' values, and the sync.
    bool fetch(uint8_t* slots = nullptr) {
        const size_t k = size(), m = jobs();
        st = std::vector<int32_t>(k);
        job_val = std::vector<uint32_t>(m);
        bool ok = true;
        if (jobs_behind_items) {
            len = std::vector<uint32_t>(k);
            used = std::vector<uint32_t>(k);
            ok = g.d2h(len.data(), g.out_len.p, 4 * k) && g.d2h(used.data(), d_used(), 4 * k);
        }
        return ok && g.d2h(st.data(), d_status(), 4 * k) && (!slots || g.d2h(slots, g.dout.p, out_bytes)) &&
               g.d2h(job_val.data(), d_job_val(), 4 * m) && g.sync();
    }
    // an item's own bytes (not its slot) to dst; the caller syncs once after its last item
    bool copy_item(uint32_t i, uint8_t* dst) { return g.d2h(dst, d_out() + out_off[i], len[i]); }
};

// A device copy of one plain struct T inside a DevBuf of the handle: a single item's launch arguments and
// results.  field() hands a kernel the device address of a member, in the member's type.
template <class T>
struct ParamBlock {
    Gpu& g;
    DevBuf& buf;
    ParamBlock(Gpu& gpu, DevBuf& b) : g(gpu), buf(b) {}
    bool ensure() const { return buf.ensure(sizeof(T)); }
    bool upload(const T& v, size_t bytes_in = sizeof(T)) const { return g.h2d(buf.p, &v, bytes_in); }
    template <class M>
    bool download(T& v, M T::*from_field) const {  // the block from that member to its end
        const size_t at = field_offset(from_field);
        return g.d2h(reinterpret_cast<uint8_t*>(&v) + at, buf.as<uint8_t>() + at, sizeof(T) - at);
    }
    template <class M>
    M* field(M T::*member) const {
        return static_cast<M*>(static_cast<void*>(buf.as<uint8_t>() + field_offset(member)));
    }
};

// new H holding the device workspace of kind k, or nullptr
template <class H>
H* make_handle(WsKind k) {
    auto* h = new H();
    if (h->g.hold(k)) return h;
    delete h;
    return nullptr;
}
#pragma GCC visibility pop

inline constexpr uint8_t kStreamStart[10] = {0xff, 0x06, 0x00, 0x00, 0x73, 0x4e, 0x61, 0x50, 0x70, 0x59};

// A validating batcher decoder's handed-over stream bytes, as segments in stream order: a reference to
// a registered cumulation or to the job's copy in its batch's staging arena (both valid while the job
// that consumed them is unapplied, which is as long as a re-walk can need them; a staging arena may
// be reallocated while its batch collects, so that reference is the arena's pointer + offset), or an
// owned copy.
struct StreamHist {
    struct Seg {
        uint64_t pos;
        const uint8_t* p;
        size_t n;
        std::vector<uint8_t> own;
        uint8_t* const* base = nullptr;  // staging reference: bytes at *base + off
        uint64_t off = 0;
        const uint8_t* data() const { return base ? *base + off : p; }
    };
    std::deque<Seg> segs;
    uint64_t end = 0;  // stream position after the last byte handed over
    void append(const uint8_t* p, size_t n, bool copy) {
        if (!n) return;
        Seg s{end, p, n, {}};
        if (copy) {
            s.own.assign(p, p + n);
            s.p = s.own.data();
        }
        segs.push_back(std::move(s));
        end += n;
    }
    void append_staged(uint8_t* const* base, uint64_t off, size_t n) {
        if (!n) return;
        Seg s{end, nullptr, n, {}, base, off};
        segs.push_back(std::move(s));
        end += n;
    }
    // [a, end) into `out` (appended)
    void copy_from(uint64_t a, std::vector<uint8_t>& out) const {
        for (const Seg& s : segs) {
            if (s.pos + s.n <= a) continue;
            const size_t o = a > s.pos ? (size_t)(a - s.pos) : 0;
            out.insert(out.end(), s.data() + o, s.data() + s.n);
        }
    }
    // Make [a, end) one owned, contiguous segment and return its bytes (a re-walk: what it leaves
    // carried outlives the jobs whose registered memory it was in).
    const uint8_t* own_from(uint64_t a) {
        std::vector<uint8_t> v;
        copy_from(a, v);
        while (!segs.empty() && segs.back().pos >= a) segs.pop_back();
        if (!segs.empty() && segs.back().pos + segs.back().n > a) {  // split the segment holding a
            Seg& s = segs.back();
            s.n = (size_t)(a - s.pos);
            if (!s.own.empty()) s.own.resize(s.n);  // (p stays valid: shrinking keeps the buffer)
        }
        Seg t{a, nullptr, v.size(), std::move(v)};
        t.p = t.own.data();
        segs.push_back(std::move(t));
        return segs.back().p;
    }
    // bytes at stream position a, contiguous to the end of its segment
    const uint8_t* at(uint64_t a) const {
        for (const Seg& s : segs)
            if (a >= s.pos && a < s.pos + s.n) return s.data() + (a - s.pos);
        return nullptr;
    }
    void drop_before(uint64_t a) {  // whole segments that end at or below a
        while (!segs.empty() && segs.front().pos + segs.front().n <= a) segs.pop_front();
    }
    void clear(uint64_t at_pos) {
        segs.clear();
        end = at_pos;
    }
};

}  // namespace h
}  // namespace nx

struct nx_snappy_frame_encoder {
    nx::h::Gpu g;
    bool started = false;
    int32_t slice;
};

struct nx_snappy_frame_decoder {
    nx::h::Gpu g;
    bool validate;
    bool started = false;
    bool corrupted = false;
    bool parse_failed = false;  // batcher: a submitted input failed its header walk (applied later, in order)
    uint64_t skip = 0;  // numBytesToSkip
    nx::h::MsgList ml;
    // Batcher, validating decoders only.  A compressed chunk that decodes fewer bytes than its length
    // leaves the rest to be parsed again as the next chunk header (SnappyFrameDecoder.java:206-212),
    // which is only known once the chunk is decoded.  So the handed-over byte stream is kept from the
    // first byte a not-yet-applied job walked (absolute positions in the decoder's stream): a leftover
    // found at apply() re-walks it from there.
    nx::h::StreamHist hist;            // stream bytes from the first an unapplied job walked to hist.end
    uint64_t parse_pos = 0;            // the header walk has reached here; [parse_pos, end) is carried into the next submit
    uint64_t epoch = 0;                // bumped by each re-walk: jobs walked under an older epoch deliver nothing
    std::multiset<uint64_t> outstanding;  // walk starts of jobs submitted and not yet applied
    // the owner's reference plus one per batcher job: nx_snappy_frame_decoder_free drops the owner's,
    // and the handle is deleted when the last job referring to it is deleted (a handler removed while
    // its jobs are in flight)
    std::atomic<int> refs{1};
};

inline void nx_decoder_unref(nx_snappy_frame_decoder* d) {
    if (d && d->refs.fetch_sub(1) == 1) delete d;
}

// ZstdDecoder (handlers.cpp): stateless between frames, so the handle is its options, the CORRUPTED
// state and the messages of the last call.
struct nx_zstd_decoder {
    nx::h::Gpu g;
    nx::h::MsgList ml;
    int32_t max_alloc = 0;       // maximumAllocationSize (ZstdDecoder.java:44), 0: no limit
    bool corrupted = false;      // State.CORRUPTED (:54-57)
    std::vector<uint8_t> back;   // the last launch's results and output slots, as copied back
    uint64_t launches = 0, frames = 0;  // nx_zstd_decoder_stats
};

// Bzip2Decoder (handlers.cpp): the stream header's level, the running stream CRC and the bits already used of the
// cumulation's first byte are carried between calls; a call's blocks come from one scan-and-decode sequence.
struct nx_bzip2_decoder {
    nx::h::Gpu g;
    nx::h::MsgList ml;
    bool have_header = false, closed = false, corrupted = false;
    uint32_t level = 0, crc = 0, bit_used = 0;
    uint32_t seen_after = 0;     // candidates behind the waiting block when its front last answered TRUNCATED
    std::vector<uint8_t> back;   // the last call's decoded bytes
    std::vector<uint8_t> lists;  // the last call's chain lists, as copied back
    uint64_t launches = 0, attempted = 0, emitted = 0;  // nx_bzip2_decoder_stats
};
