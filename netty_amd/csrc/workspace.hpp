// workspace.hpp — the device workspaces of the batch kernels (the encoders' per-lane hash tables,
// the decoder's per-frame record slots): one per device and kind, shared by every stream.
//
// Launches that use a workspace are ordered on the device: a batch waits (hipStreamWaitEvent) for
// the event the previous batch recorded after its launches, so the host never blocks and any number
// of streams (the batcher's four, every handle's own) share one allocation.  The decoder's record
// slots are leased by PART (WsLease::acquire_part): a batch of m frames takes the next m slots of a
// ring over the workspace and waits only for the earlier batches whose slots it reuses, so the
// parse / expand of batches on different streams overlap (round 4: with one lease for the whole
// workspace, a batcher's auto-flushed batches ran their decodes strictly one after another).  A workspace grows only
// where growth is allowed: in the standalone batch entry points (nx_*_batch called directly) and at
// set-up (nx_snappy_encoder_reserve, nx_batcher_new and the handle constructors, which hold it).
// Batches submitted by a batcher or a handle run inside a NoGrowScope: they use the slots the owner
// reserved and cap their grid to them, so a flush never allocates, frees or probes.  The last owner
// to let go frees it unless the standalone API grew it (then nx_workspaces_trim does).
#pragma once
#include <mutex>
#include <vector>
#include "nx_common.hpp"

namespace nx {

enum class WsKind : int { SnappyEnc = 0, Lz4Enc, FastLzEnc, LzfEnc, DecRecords, Lz4HcEnc, DeflateEnc, ZstdEnc, ZstdDec, Bzip2Dec, Bzip2Enc, LzmaEnc, BrotliEnc, BrotliDec, Count };

// Table geometry per encoder kind (entry bytes, log2 entries per table, waves per CU of its launch);
// each codec static_asserts its own constants against this.
struct WsSpec {
    uint32_t entry_bytes;
    uint32_t lg;
    unsigned waves_per_cu;
};
// SnappyEnc: 20 waves per CU (5 blocks of 256, 327 680 lanes on 256 CUs: 40 GiB of tables; round 6).
// Lz4HcEnc: 2^15 x 8 bytes = liblz4's HC tables per lane (u32 hashTable[2^15] + u16 chainTable[2^16]),
// 2 waves per CU, always one block per wave (kHcMaxSlots: at most cus * 2 tables, 128 MiB on 256 CUs).
// DeflateEnc: 128 KiB per chunk (4096 hash entries, then 96 KiB of tokens; deflate.hip), one chunk per
// slot and launch pair, 16 waves per CU of lanes in the dense form.
// ZstdEnc: 512 KiB per chunk (32 768 hash entries, then the chunk's literals and sequences; zstd.hip), one
// chunk per slot and launch pair as DeflateEnc, a workspace of its own.
// ZstdDec: no tables: 128 KiB per frame in flight (the literals of the block being decoded; zstd_decode.hip),
// leased by part as DecRecords is, one slot per wave of the launch on at most kZstdDecWavesPerCu waves per CU.
// Bzip2Dec: no tables: one slot per stream in flight holds a block's BWT bytes, merged pointers and pre-RLE
// bytes (6 x 900 000 bytes and padding; bzip2_decode.hip), leased by part, one slot per wave of the launch on
// at most kBzip2DecWavesPerCu waves per CU.
// Bzip2Enc: no tables: counted in units of one level's worth (a 100 000-byte block's bytes, transformed bytes, two
// index and two rank arrays of the rotation sort, MTF symbols and staged output; bzip2_encode.hip); a stream at
// level L takes L consecutive units, leased by part, one stream per workgroup of the launch on at most
// kBzip2EncGroupsPerCu workgroups per CU.
// LzmaEnc: 512 KiB per item in flight (65 536 stamped hash entries of the matcher; lzma.hip), one item per slot and
// launch pair as ZstdEnc; the items' sequence words live in the workspace's side allocation (SharedWs::side), sized
// per call from the lengths (WsAreaCut).
// BrotliEnc: the same geometry for the Brotli matcher (brotli.hip), with the same use of its own side allocation.
// BrotliDec: no tables: one slot per stream in flight holds a meta-block's trees and context maps at the format's
// maxima (802 304 bytes; brotli_decode.hip derives it), leased by part, one slot per wave of the launch on at most
// kBrotliDecWavesPerCu waves per CU.
#ifndef NX_LZ4_WPCU  // build options for A/B runs of the alt encoders' occupancy (scripts/build_lib_variant.sh; LZ4 at 20: level)
#define NX_LZ4_WPCU 16
#endif
#ifndef NX_FLZ_WPCU  // FastLZ: 16 waves per CU since round 6 (profiles/r06/s4: 310 vs 351-360 ms per 262 144 chunks)
#define NX_FLZ_WPCU 16
#endif
#ifndef NX_LZF_WPCU  // LZF: 16 waves per CU measured level with 8 (profiles/r06/s4), so the smaller workspace stays
#define NX_LZF_WPCU 8
#endif
constexpr WsSpec kWsSpec[] = {{8, 14, 20}, {8, 13, NX_LZ4_WPCU}, {8, 13, NX_FLZ_WPCU}, {8, 14, NX_LZF_WPCU}, {0, 0, 0}, {8, 15, 2}, {8, 14, 16}, {8, 16, 16}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {8, 16, 16}, {8, 16, 16}, {0, 0, 0}};
static_assert(sizeof(kWsSpec) / sizeof(kWsSpec[0]) == (size_t)WsKind::Count, "one spec per kind");
constexpr size_t kDecSlotBytes = 16384u * 4u + 8u;  // records of one frame + its count and length
#ifndef NX_DEC_MAX_FRAMES  // build option for A/B runs (scripts/build_lib_variant.sh)
#define NX_DEC_MAX_FRAMES 262144
#endif
constexpr uint32_t kDecMaxFrames = NX_DEC_MAX_FRAMES;  // frames per parse/expand launch pair
constexpr size_t kZstdDecSlotBytes = 128u << 10;  // Block_Maximum_Size: the most literals one block regenerates
constexpr unsigned kZstdDecWavesPerCu = 8;        // 2 048 frames in flight, 256 MiB, on 256 CUs
constexpr size_t kBzip2DecSlotBytes = 6u * 900000u + 256u;  // a 900 000-byte block: bytes, 4-byte pointers, pre-RLE bytes
// k_bzip2_decode keeps about 27 KiB of LDS per wave (tables, selectors, tiles): five waves fit a CU's 160 KiB;
// four leave one wave per SIMD and 5.2 GiB of slots on 256 CUs
constexpr unsigned kBzip2DecWavesPerCu = 4;
// 24 bytes per block byte and padding: a slot is 2 404 096 bytes at level 1 and 21 636 864 at level 9
constexpr size_t kBzip2EncUnitBytes = 24u * 100000u + 4096u;
// k_bzip2_encode is one workgroup of 1 024 lanes with about 69 KiB of LDS: one per CU, 256 slots, 5.5 GB at level 9
// (615 MB at level 1) on 256 CUs
constexpr unsigned kBzip2EncGroupsPerCu = 1;
// 256 literal, command and distance trees at 544, 1 440 and 1 072 bytes, the block trees, the context maps and their
// code: 802 216 bytes (brotli_decode.hip's header has the sum), rounded up to a multiple of 256
constexpr size_t kBrotliDecSlotBytes = 802304;
// k_brotli_decode keeps about 3 KiB of LDS per wave; four waves per CU leave one per SIMD and 822 MB of slots on 256 CUs
constexpr unsigned kBrotliDecWavesPerCu = 4;
// bytes per slot of a kind without tables (0 for the table kinds)
constexpr size_t ws_plain_slot_bytes(WsKind k) {
    return k == WsKind::DecRecords ? kDecSlotBytes : k == WsKind::ZstdDec ? kZstdDecSlotBytes : k == WsKind::Bzip2Dec ? kBzip2DecSlotBytes : k == WsKind::Bzip2Enc ? kBzip2EncUnitBytes : k == WsKind::BrotliDec ? kBrotliDecSlotBytes : 0;
}

struct WsUse {  // an in-flight part lease: slots [a, b), done when ev completes
    size_t a, b;
    hipEvent_t ev;
    hipStream_t st;  // the stream ev was recorded on (ws_forget_stream)
};
struct SharedWs {
    std::mutex mu;
    std::vector<WsUse> uses;        // part leases not yet known to be complete
    std::vector<hipEvent_t> spare;  // their recycled events
    size_t cursor = 0;              // next part lease starts here (wraps to 0)
    void* p = nullptr;
    size_t slots = 0;    // tables (lanes or waves) or frames
    void* side = nullptr;   // a second allocation some kinds keep beside the slots (ws_side_reserve): it is used under
    size_t side_bytes = 0;  // the lease as the slots are, and freed whenever they are
    uint32_t stamp = 0;  // encoders: last stamp used
    hipEvent_t ev = nullptr;
    hipStream_t ev_st = nullptr;  // the stream ev was last recorded on
    bool used = false;   // ev has been recorded
    int owners = 0;      // batchers and handles holding it
    bool kept = false;   // grown by the standalone API or a reserve: kept until nx_workspaces_trim
    size_t cap = 0;      // most slots it may ever grow to (nx_snappy_encoder_reserve_ex; 0: no cap)
    PlacementReport place;
};
// the slots a grow to `want` may take under W's cap
inline size_t ws_capped(const SharedWs& W, size_t want) { return W.cap && want > W.cap ? W.cap : want; }

SharedWs& shared_ws(WsKind k, int dev);
// slots a batch of n units asks for: the encoders' lane_grid slots, the decoder's frames per launch
size_t ws_want(WsKind k, uint32_t n, int cus);
// The lane-per-chunk grid for n chunks over at most `have` table slots: the dense form while it has
// at least kSpreadMaxChunks lanes (a dense wave does the work of ~16 spread waves), else one chunk
// per wave on up to cus * waves_per_cu waves.
LaneGrid ws_grid(WsKind k, uint32_t n, int cus, size_t have);

// At least `bytes` of side allocation (the caller holds W's lease, and nothing enqueued reads the side any more):
// kept when it is large enough, else freed and allocated anew; what it held is lost either way.
hipError_t ws_side_reserve(SharedWs& W, size_t bytes);

struct NoGrowScope {
    NoGrowScope();
    ~NoGrowScope();
    bool prev;
};
bool ws_no_grow();

// One batch's use of a workspace: holds its lock from acquire() to destruction.
class WsLease {
  public:
    WsLease(WsKind k, int dev, hipStream_t st);
    ~WsLease();
    // Grow to `want` slots when growth is allowed (blocking, set-up only), allocate if there is no
    // workspace yet, then order the stream after the previous user's launches.
    hipError_t acquire(size_t want);
    // The same for min(want, slots) slots [*first, *first + *count) of the ring: the stream waits for
    // the last whole-workspace user and for the part leases that overlap them.
    hipError_t acquire_part(size_t want, size_t* first, size_t* count);
    SharedWs& ws() { return W_; }

  private:
    WsKind k_;
    SharedWs& W_;
    std::unique_lock<std::mutex> lk_;
    hipStream_t st_;
    bool acquired_ = false;
    bool part_ = false;
    size_t a_ = 0, b_ = 0;
};

// One batch of a lane-per-chunk encoder over kind k's tables.  A lane stamps its table entries with
// stamp_base + its iteration, and stamps stay below max_stamp between two zeroings of the tables:
// the batch runs in launches of at most slots * (max_stamp - 1) chunks, and the tables are zeroed
// before a launch whose stamps would reach max_stamp.  launch(base, m, grid, tables, stamp_base)
// enqueues the kernel for chunks [base, base + m).
template <class Launch>
int32_t ws_lane_launch(WsKind k, uint32_t max_stamp, uint32_t n, hipStream_t st, Launch&& launch) {
    int dev = 0, cus = 256;
    NX_HIP_CHECK(hipGetDevice(&dev));
    NX_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    WsLease lease(k, dev, st);
    NX_HIP_CHECK(lease.acquire(ws_want(k, n, cus)));
    SharedWs& W = lease.ws();
    const LaneGrid g = ws_grid(k, n, cus, W.slots);
    const size_t table_bytes = (size_t)kWsSpec[(int)k].entry_bytes << kWsSpec[(int)k].lg;
    const size_t per_launch = g.slots * (max_stamp - 1);
    for (size_t base = 0; base < n; base += per_launch) {
        const uint32_t m = (uint32_t)(n - base < per_launch ? n - base : per_launch);
        const uint32_t iters = (uint32_t)((m + g.slots - 1) / g.slots);
        if (W.stamp + iters >= max_stamp) {
            NX_HIP_CHECK(hipMemsetAsync(W.p, 0, W.slots * table_bytes, st));
            W.stamp = 0;
        }
        launch(base, m, g, W.p, W.stamp);
        NX_HIP_CHECK(hipGetLastError());
        W.stamp += iters;
    }
    return NX_OK;
}

// How an arena encoder's batch is cut (ws_pair_launch): an item's sequence area is area(its length) bytes of the
// side allocation, whose first words are the items' offsets into it (d_aoff), and a launch pair takes items
// while their areas stay within kWsAreaMax, one item at least.  The first take reads in_len back, which
// synchronises the stream once: the stream has waited for the workspace's earlier users by then, so nothing
// reads the side any more.  The take that reaches item n reserves the side for the largest pair and copies
// the offsets there.
constexpr size_t kWsAreaMax = (size_t)4 << 30;
struct WsAreaCut {
    const uint32_t* in_len;         // of the batch, on the device
    size_t (*area)(uint32_t len);
    std::vector<uint32_t> len;
    std::vector<uint64_t> aoff;
    size_t need = 0;
    // how many of the items [base, base + most) the next pair takes
    int32_t take(SharedWs& W, uint32_t n, hipStream_t st, uint32_t base, uint32_t most, uint32_t* m);
    static const uint64_t* d_aoff(const SharedWs& W) { return static_cast<const uint64_t*>(W.side); }
};

// One batch of a two-pass encoder over kind k's slots, an item per slot from its pass 1 to its pass 2: the batch
// runs in launch pairs of at most the grid's slots (at most max_slots of them, to which a standalone call grows
// the workspace; 0: no such cap) and of what `cut` takes, if there is one.  A pair's matcher stamps its table
// entries with the next stamp, and stamps stay below max_stamp between two zeroings of the slots.
// match(base, m, grid, W, stamp) enqueues pass 1 for items [base, base + m), emit(base, m, waves, W) pass 2 on
// min(m, CUs * emit_waves_per_cu) waves.  stamped = false: no pass 1, and the stamp stays (deflate's level 0).
struct WsPairSpec {
    WsKind kind;
    uint32_t max_stamp;
    size_t max_slots;
};
template <class Match, class Emit>
int32_t ws_pair_launch(const WsPairSpec& S, uint32_t n, hipStream_t st, unsigned emit_waves_per_cu, WsAreaCut* cut, bool stamped,
                       Match&& match, Emit&& emit) {
    int dev = 0, cus = 256;
    NX_HIP_CHECK(hipGetDevice(&dev));
    NX_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    WsLease lease(S.kind, dev, st);
    const size_t want = ws_want(S.kind, n, cus);
    NX_HIP_CHECK(lease.acquire(S.max_slots && want > S.max_slots ? S.max_slots : want));
    SharedWs& W = lease.ws();
    const size_t have = S.max_slots && W.slots > S.max_slots ? S.max_slots : W.slots;
    const size_t slot_bytes = (size_t)kWsSpec[(int)S.kind].entry_bytes << kWsSpec[(int)S.kind].lg;
    // the pairs first: the last cut sizes the side allocation, before anything that uses it is enqueued
    struct Pair {
        uint32_t base, m;
        LaneGrid g;
    };
    std::vector<Pair> pairs;
    for (uint32_t base = 0; base < n;) {
        const uint32_t left = n - base;
        const LaneGrid g = ws_grid(S.kind, left, cus, have);
        uint32_t m = (uint32_t)(left < g.slots ? left : g.slots);
        if (cut) {
            const int32_t r = cut->take(W, n, st, base, m, &m);
            if (r != NX_OK) return r;
        }
        pairs.push_back({base, m, g});
        base += m;
    }
    const unsigned waves = (unsigned)cus * emit_waves_per_cu;
    for (const Pair& pr : pairs) {
        if (stamped) {
            if (W.stamp + 1u >= S.max_stamp) {
                NX_HIP_CHECK(hipMemsetAsync(W.p, 0, W.slots * slot_bytes, st));
                W.stamp = 0;
            }
            W.stamp += 1u;
            match(pr.base, pr.m, pr.g, W, W.stamp);
            NX_HIP_CHECK(hipGetLastError());
        }
        emit(pr.base, pr.m, pr.m < waves ? pr.m : waves, W);
        NX_HIP_CHECK(hipGetLastError());
    }
    return NX_OK;
}

// Owners: hold at creation (grows to `units` now), unhold at destruction (the last one frees).
int32_t ws_hold(WsKind k, int dev, uint32_t units, hipStream_t st);
void ws_unhold(WsKind k, int dev);
// A stream the library created is about to be destroyed, and its work is complete (the caller has
// synchronized it): forget the workspace events recorded on it, so that no later wait or drop
// touches an event whose stream no longer exists (the HIP runtime looks at that stream's capture
// state in hipEventSynchronize / hipStreamWaitEvent).
void ws_forget_stream(hipStream_t st);

// Owner sizes: a handle encodes a message of up to 1024 slices without waiting on another slot; a
// batcher flush of up to 16384 slices / frames runs at full grid.
constexpr uint32_t kHandleHoldUnits = 1024;
constexpr uint32_t kBatcherHoldUnits = 16384;
// A batcher's reservations.  Snappy tables in the DENSE form for 65 536 lanes (8 GiB): a flush of more
// than kSpreadMaxChunks slices runs lane-per-chunk on 256 blocks, one per CU (the table request rate
// saturates from ~32 K lanes; 16 640 lanes were only 65 blocks, and a reservation below
// kSpreadMaxChunks lanes runs one chunk per wave on 4 096 waves).  Records for 65 536 frames (4 GiB), so
// k_parse's lane-per-frame launch of a sub-batch fills every CU as well.
constexpr uint32_t kBatcherEncHoldUnits = 65536;
constexpr uint32_t kBatcherDecHoldUnits = 65536;

}  // namespace nx
