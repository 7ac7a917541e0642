// handlers.cpp — host handler layer: Netty's framing state machines over host memory, with every
// chunk of one encode()/decode() call batched into a single GPU launch.
//
//   SnappyFrameEncoder   SnappyFrameEncoder.java:79-152
//   SnappyFrameDecoder   SnappyFrameDecoder.java:85-258 (+ ByteToMessageDecoder.callDecode :464-517)
//   FastLzFrameEncoder   FastLzFrameEncoder.java:111-172
//   FastLzFrameDecoder   FastLzFrameDecoder.java:113-207
//   LzfEncoder           LzfEncoder.java:169-246
//   LzfDecoder           LzfDecoder.java:112-241
//   Lz4FrameEncoder      Lz4FrameEncoder.java:231-336
//   Lz4FrameDecoder      Lz4FrameDecoder.java:121-261
//   ZstdEncoder          ZstdEncoder.java:105-178
//   ZstdDecoder          ZstdDecoder.java:59-122
//   Bzip2Encoder         Bzip2Encoder.java:105-228
//   Bzip2Decoder         Bzip2Decoder.java:93-343
//   JdkZlibEncoder       JdkZlibEncoder.java:123-137, :214-276, :308-340
//   JdkZlibDecoder       JdkZlibDecoder.java:117-160, :198-520 (+ ZlibDecoder.java:49,62-84)
//
// Headers are parsed on the host exactly as the Java decode() does (they are a few bytes per
// chunk); the per-chunk arithmetic (the codecs and their checksums) runs on the GPU.  Results
// are applied in stream order, so the first failing chunk truncates the message list and marks the
// decoder corrupted just like the reference's exception path.
//
// The seven encoders stage a launch through nx::h::EncodeItems (handles.hpp): the codec cuts its message
// into items and says each one's slot size, calls its kernel with the typed device arrays, and says what
// it reads back and where each item's bytes go.
//
// The seven decoders start a call with nx::h::DecodeCall (decode_call.hpp): it checks the arguments, empties
// the handle's message list, and is the one place that writes consumed, msgs, n_msgs and err_msg (finish,
// fail, skip_all); marking the decoder corrupted stays the codec's line.  The decoders with item lists (Snappy;
// FastLZ, LZF and LZ4 in alt_decode) stage their launch through nx::h::DecodeItems (handles.hpp): the items and a
// second list of checksum jobs, typed device accessors on the launch lines, one fetch.  The single-item decoders
// (zlib, Bzip2; Bzip2Encoder's segment too) hand their kernels the fields of one small struct through
// nx::h::ParamBlock; Zstd's packed geometry and results are typed views (ZstdGeometry, ZstdResults).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../include/netty_amd.h"
#include "nx_common.hpp"
#include "frame_parse.hpp"
#include "handles.hpp"
#include "alt_frames.hpp"
#include "brotli_encode_core.hpp"
#include "bzip2_decode_split.hpp"

extern "C" int32_t nx_snappy_decode_batch(const uint8_t*, const uint64_t*, const uint32_t*, uint8_t*, const uint64_t*,
                                          const uint32_t*, uint32_t*, uint32_t*, int32_t*, const uint32_t*, uint32_t*, uint32_t,
                                          void*);

namespace {
using nx::h::DecodeCall;
using nx::h::DecodeItems;
using nx::h::DevBuf;
using nx::h::EncodeItems;
using nx::h::ParamBlock;
using nx::h::Gpu;
using nx::h::MsgList;
using nx::h::for_each_piece;
using nx::h::kStreamStart;
using nx::h::make_handle;

inline uint32_t le32(const uint8_t* p) { return p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24); }
inline uint32_t be16(const uint8_t* p) { return ((uint32_t)p[0] << 8) | p[1]; }
inline uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

// a decode() call's first failure in stream order: the status, the exception's text, where the reader stops
struct Failure {
    int32_t code = NX_OK;
    std::string text;
    size_t at = 0;
};

// the last failure's message of an encoder handle that keeps one (nullptr: none)
template <class E>
const char* last_error(const E* e) {
    return e && !e->err.empty() ? e->err.c_str() : nullptr;
}

}  // namespace

// ======================================================================= Snappy frame encoder

extern "C" nx_snappy_frame_encoder* nx_snappy_frame_encoder_new(int32_t jumbo) {
    auto* e = make_handle<nx_snappy_frame_encoder>(nx::WsKind::SnappyEnc);
    if (e) e->slice = jumbo ? 65535 : 32767;  // SnappyFrameEncoder.java:31,39
    return e;
}
extern "C" void nx_snappy_frame_encoder_free(nx_snappy_frame_encoder* e) { delete e; }
extern "C" size_t nx_snappy_frame_max_encoded_length(size_t n) { return 10 + (n / 32767 + 2) * 8 + 32 + n + n / 6; }

extern "C" int64_t nx_snappy_frame_encoder_encode(nx_snappy_frame_encoder* e, const uint8_t* in, size_t n, uint8_t* out,
                                                  size_t out_cap) {
    const nx::NoGrowScope no_grow;
    if (!e) return NX_ERR_INVALID_ARG;
    if (n == 0) return 0;  // !in.isReadable()
    if (out_cap < nx_snappy_frame_max_encoded_length(n)) return NX_ERR_INVALID_ARG;
    size_t op = 0;
    if (!e->started) {
        e->started = true;
        memcpy(out, kStreamStart, 10);
        op = 10;
    }
    EncodeItems it(e->g);
    bool last_raw = false;  // the last slice goes out uncompressed (every other one is a compressed chunk)
    auto add = [&](uint64_t off, uint32_t len, bool raw) {
        it.add(off, len, (nx_snappy_max_compressed_length(len) + 15) & ~15ull);
        last_raw = raw;
    };
    int64_t dl = (int64_t)n;
    if (dl > 18) {  // MIN_COMPRESSIBLE_LENGTH (:46,90-113)
        uint64_t pos = 0;
        for (;;) {
            if (dl < 18) {
                add(pos, (uint32_t)dl, true);
                break;
            }
            uint32_t len = dl > e->slice ? (uint32_t)e->slice : (uint32_t)dl;
            add(pos, len, false);
            pos += len;
            if (dl > e->slice) dl -= e->slice; else break;
        }
    } else {
        add(0, (uint32_t)n, true);
    }
    const uint32_t ns = it.size();
    auto comp = [&](uint32_t i) { return !(last_raw && i == ns - 1); };
    Gpu& g = e->g;
    int32_t r = it.stage(in, n, 0, 4ull * ns);
    if (r != NX_OK) return r;
    uint32_t* d_crc = g.aux0.as<uint32_t>();
    // masked CRC32C of every slice (calculateAndWriteChecksum :150-152, writeUnencodedChunk :119-124)
    r = nx_crc32c_masked_batch(it.d_in(), it.d_in_off(), it.d_in_len(), d_crc, ns, g.s);
    if (r != NX_OK) return r;
    // Snappy.encode of every slice (uncompressed slices are encoded too but ignored: keeps one launch)
    r = nx_snappy_encode_batch(it.d_in(), it.d_in_off(), it.d_in_len(), it.d_out(), it.d_out_off(), it.d_out_len(), it.d_status(), ns,
                               g.s);
    if (r != NX_OK) return r;
    std::vector<uint32_t> crc(ns);
    if (!it.fetch(false, d_crc, crc.data())) return NX_ERR_HIP;  // the lengths and the CRCs; the status is not read
    const std::vector<uint32_t>& clen = it.len;
    // the framed layout is known once the lengths are: each compressed chunk's bytes (and nothing
    // else of its slot) go straight to their place in `out`
    auto body = [&](uint32_t i) { return comp(i) ? clen[i] : it.in_len[i]; };  // a chunk's bytes behind its CRC
    for (uint32_t i = 0; i < ns; ++i)
        if (comp(i) && ((clen[i] + 4) >> 24)) return NX_ERR_INVALID_ARG;  // setChunkLength (:126-132)
    bool ok = true;
    size_t q = op;
    for (uint32_t i = 0; i < ns && ok; ++i) {
        if (comp(i)) ok = it.copy_item(i, out + q + 8);
        q += 8 + body(i);
    }
    if (!g.sync() || !ok) return NX_ERR_HIP;
    for (uint32_t i = 0; i < ns; ++i) {
        const uint32_t chunkLength = body(i) + 4;
        out[op++] = comp(i) ? 0 : 1;
        out[op++] = (uint8_t)chunkLength;
        out[op++] = (uint8_t)(chunkLength >> 8);
        out[op++] = (uint8_t)(chunkLength >> 16);
        memcpy(out + op, &crc[i], 4);
        op += 4;
        if (!comp(i)) nx::copy_bytes(out + op, in + it.in_off[i], it.in_len[i]);  // (a compressed chunk's came from the device)
        op += body(i);
    }
    return (int64_t)op;
}

// ======================================================================= Snappy frame decoder

extern "C" nx_snappy_frame_decoder* nx_snappy_frame_decoder_new(int32_t validate) {
    auto* d = make_handle<nx_snappy_frame_decoder>(nx::WsKind::DecRecords);
    if (d) d->validate = validate != 0;
    return d;
}
extern "C" void nx_snappy_frame_decoder_free(nx_snappy_frame_decoder* d) { nx_decoder_unref(d); }

using nx::fr::SAct;
using nx::fr::SnappyAction;
using nx::fr::snappy_parse_one;

extern "C" int32_t nx_snappy_frame_decoder_decode(nx_snappy_frame_decoder* d, const uint8_t* in, size_t n, size_t* consumed,
                                                  const nx_msg** msgs, size_t* n_msgs, const char** err_msg) {
    const nx::NoGrowScope no_grow;
    DecodeCall call(d, in, n, consumed, msgs, n_msgs, err_msg);
    if (call.refused()) return NX_ERR_INVALID_ARG;
    if (d->corrupted) return call.skip_all();  // :86-89
    MsgList& ml = call.ml();
    size_t& rd = call.rd;
    Failure bad;  // the first failing chunk ends the call, as the Java exception does
    for (;;) {  // loops again only for the validating-mode leftover case below
        std::vector<SnappyAction> acts;
        size_t p = rd;
        bool started = d->started;
        uint64_t skip = d->skip;
        while (p < n && snappy_parse_one(in, n, p, started, skip, d->validate, acts)) {
        }
        // ---- one GPU batch: decode every compressed chunk; CRC every uncompressed one if validating
        std::vector<int> comp_idx, unc_idx;
        size_t lo = (size_t)-1, hi = 0;
        for (size_t i = 0; i < acts.size(); ++i) {
            SnappyAction& a = acts[i];
            if (a.kind == SAct::Comp) {
                a.job = (int)comp_idx.size();
                comp_idx.push_back((int)i);
            } else if (a.kind == SAct::Uncomp && d->validate) {
                a.job = (int)unc_idx.size();
                unc_idx.push_back((int)i);
            } else {
                continue;
            }
            lo = a.data < lo ? a.data : lo;
            hi = a.data + a.dlen > hi ? a.data + a.dlen : hi;
        }
        // the items are the compressed chunks, a 64 KiB slot each; the raw chunks to CRC ride behind them
        DecodeItems it(d->g, true);
        std::vector<uint32_t> expect;
        for (int i : comp_idx) {
            it.add(acts[i].data - lo, acts[i].dlen, 65536);
            expect.push_back(acts[i].crc);
        }
        for (int i : unc_idx) it.add_job(acts[i].data - lo, acts[i].dlen);
        const uint32_t ncomp = it.size(), nunc = it.jobs();
        std::vector<std::vector<uint8_t>> outs(ncomp);  // each decoded chunk, exactly olen bytes
        if (ncomp + nunc) {
            int32_t r = it.stage(in + lo, hi - lo, nullptr, &expect);
            if (r == NX_OK && ncomp)
                r = nx_snappy_decode_batch(it.d_in(), it.d_in_off(), it.d_in_len(), it.d_out(), it.d_out_off(), nullptr, it.d_out_len(),
                                           it.d_used(), it.d_status(), d->validate ? it.d_item_word() : nullptr, nullptr, ncomp, d->g.s);
            if (r == NX_OK && nunc) r = nx_crc32c_masked_batch(it.d_in(), it.d_job_off(), it.d_job_len(), it.d_job_val(), nunc, d->g.s);
            if (r != NX_OK) return call.finish(r);
            if (!it.fetch()) return call.finish(NX_ERR_HIP);
            // only the bytes each chunk produced cross PCIe (a message's olen, not its 64 KiB slot)
            bool ok = true;
            for (uint32_t j = 0; j < ncomp && ok; ++j) {
                if (it.st[j] != NX_OK && it.st[j] != NX_ERR_SNAPPY_CRC_MISMATCH) continue;
                outs[j].resize(it.len[j]);
                ok = it.copy_item(j, outs[j].data());
            }
            if (!d->g.sync() || !ok) return call.finish(NX_ERR_HIP);
        }
        const std::vector<uint32_t>&olen = it.len, &cons = it.used, &ucrc = it.job_val;
        const std::vector<int32_t>& st = it.st;
        // ---- apply in stream order (the first failing chunk ends the call, as the Java exception does)
        bool reparse = false;
        char buf[128];
        for (const SnappyAction& a : acts) {
            if (a.kind == SAct::Error) {
                bad = {NX_ERR_FRAME_CORRUPT, a.err, a.end};
            } else if (a.kind == SAct::Stream) {
                d->started = true;
            } else if (a.kind == SAct::Uncomp) {
                if (d->validate && ucrc[a.job] != a.crc) {  // :171-175
                    snprintf(buf, sizeof buf, "mismatching checksum: %x (expected: %x)", ucrc[a.job], a.crc);
                    bad = {NX_ERR_SNAPPY_CRC_MISMATCH, buf, a.end};
                } else {
                    ml.msgs.push_back({in + a.data, a.dlen});  // readRetainedSlice: a view of the cumulation
                }
            } else if (a.kind == SAct::Comp) {
                const int j = a.job;
                if (st[j] == NX_ERR_SNAPPY_CRC_MISMATCH) {
                    snprintf(buf, sizeof buf, "mismatching checksum: %x (expected: %x)",
                             nx::host_mask(nx::host_crc32c(outs[j].data(), olen[j])), a.crc);
                    bad = {st[j], buf, a.end};
                } else if (st[j] != NX_OK) {
                    bad = {st[j], nx::fr::snappy_block_error(st[j], cons[j] >= 4 ? le32(in + a.data + cons[j] - 4) : 0u, nx_status_string),
                           a.end};
                } else {
                    ml.owned.push_back(std::move(outs[j]));
                    ml.msgs.push_back({ml.owned.back().data(), olen[j]});
                    if (d->validate && cons[j] < a.dlen) {
                        // validating mode restores the writer index and leaves the unread chunk bytes in
                        // the cumulation (:206-212); they are parsed again as the next chunk header.
                        rd = a.data + cons[j];
                        d->skip = 0;
                        reparse = true;
                        break;
                    }
                }
            }
            if (bad.code != NX_OK) break;
            rd = a.end;
            d->skip = a.skip;
        }
        if (!reparse) break;
    }
    if (bad.code == NX_OK) return call.finish(NX_OK);
    d->corrupted = true;  // :227-230
    return call.fail(bad.code, bad.text, bad.at);
}

// ======================================================================= FastLZ frame encoder

extern "C" nx_fastlz_frame_encoder* nx_fastlz_frame_encoder_new(int32_t level, int32_t checksum) {
    if (level != 0 && level != 1 && level != 2) return nullptr;  // FastLzFrameEncoder.java:101-105
    auto* e = make_handle<nx_fastlz_frame_encoder>(nx::WsKind::FastLzEnc);
    if (!e) return nullptr;
    e->level = level;
    e->checksum = checksum != 0;
    return e;
}
extern "C" void nx_fastlz_frame_encoder_free(nx_fastlz_frame_encoder* e) { delete e; }
extern "C" size_t nx_fastlz_frame_max_encoded_length(size_t n) { return (n / 65535 + 1) * (12 + 82) + n + n / 16; }

extern "C" int64_t nx_fastlz_frame_encoder_encode(nx_fastlz_frame_encoder* e, const uint8_t* buf, size_t r0, size_t n,
                                                  uint8_t* out, size_t out_cap) {
    const nx::NoGrowScope no_grow;
    if (!e) return NX_ERR_INVALID_ARG;
    if (n == 0) return 0;
    if (out_cap < nx_fastlz_frame_max_encoded_length(n)) return NX_ERR_INVALID_ARG;
    const uint8_t* in = buf + r0;
    const size_t w = r0 + n;
    EncodeItems it(e->g);
    std::vector<int32_t> lim;
    for_each_piece(n, 65535, [&](size_t off, size_t len) {
        const size_t r = r0 + off;
        const int64_t l64 = (int64_t)(w - r) - (int64_t)r;  // readableBytes() - inOffset (FastLz.java:552-557)
        lim.push_back(l64 < -0x40000000 ? -0x40000000 : (int32_t)l64);
        it.add(off, (uint32_t)len, nx_fastlz_max_compressed_length(len) + 16);
    });
    const uint32_t nc = it.size();
    const std::vector<int32_t> lvl(nc, e->level);
    Gpu& g = e->g;
    int32_t r = it.stage(in, n, 0, 4ull * nc, 8ull * nc);
    if (r != NX_OK) return r;
    int32_t* d_lim = g.aux0.as<int32_t>();
    int32_t* d_lvl = g.aux1.as<int32_t>();
    if (!g.h2d(d_lim, lim.data(), 4ull * nc) || !g.h2d(d_lvl, lvl.data(), 4ull * nc)) return NX_ERR_HIP;
    r = nx_fastlz_compress_batch(it.d_in(), it.d_in_off(), it.d_in_len(), it.d_out(), it.d_out_off(), it.d_out_len(), d_lvl, d_lim,
                                 it.d_status(), nc, g.s);
    if (r != NX_OK) return r;
    // The Adler32 values take the status array's place: this encoder never reads the statuses, and the
    // checksum kernel runs after the compress kernel on the same stream.
    uint32_t* d_adler = e->checksum ? reinterpret_cast<uint32_t*>(it.d_status()) : nullptr;
    if (d_adler) {
        r = nx_adler32_batch(it.d_in(), it.d_in_off(), it.d_in_len(), d_adler, nc, g.s);
        if (r != NX_OK) return r;
    }
    std::vector<uint32_t> ad(nc);
    if (!it.fetch(false, d_adler, ad.data())) return NX_ERR_HIP;
    const std::vector<uint32_t>&clen = it.len, &ilen = it.in_len;
    bool ok = true;
    size_t op = 0;
    for (uint32_t i = 0; i < nc; ++i) {
        const uint32_t length = ilen[i];
        const size_t outputIdx = op;
        out[op] = 'F';
        out[op + 1] = 'L';
        out[op + 2] = 'Z';
        size_t outputOffset = outputIdx + 4 + (e->checksum ? 4 : 0);
        if (e->checksum) {
            const uint32_t c = ad[i];
            out[outputIdx + 4] = (uint8_t)(c >> 24);
            out[outputIdx + 5] = (uint8_t)(c >> 16);
            out[outputIdx + 6] = (uint8_t)(c >> 8);
            out[outputIdx + 7] = (uint8_t)c;
        }
        uint8_t blockType;
        uint32_t chunkLength;
        if (length >= 32 && clen[i] < length) {  // MIN_LENGTH_TO_COMPRESSION (FastLz.java:59), :153-158
            blockType = 1;
            chunkLength = clen[i];
            out[outputOffset] = (uint8_t)(chunkLength >> 8);
            out[outputOffset + 1] = (uint8_t)chunkLength;
            outputOffset += 2;
            // only the compressed bytes cross PCIe, straight into their framed position
            ok = ok && it.copy_item(i, out + outputOffset + 2);
        } else {
            blockType = 0;
            chunkLength = length;
            nx::copy_bytes(out + outputOffset + 2, in + it.in_off[i], length);
        }
        out[outputOffset] = (uint8_t)(length >> 8);
        out[outputOffset + 1] = (uint8_t)length;
        out[outputIdx + 3] = (uint8_t)(blockType | (e->checksum ? 0x10 : 0));
        op = outputOffset + 2 + chunkLength;
    }
    if (!g.sync() || !ok) return NX_ERR_HIP;  // every queued copy has landed (or failed) before returning
    return (int64_t)op;
}

// ======================================================================= FastLZ / LZF / LZ4 decode()
// One body for the three decoders: the header walk on the host (alt_frames.hpp), every block's
// arithmetic in one GPU batch, the blocks applied in stream order.  A codec's traits say what differs.
namespace {
using nx::af::Blk;

struct FlzSync {
    static bool skips(const nx_fastlz_frame_decoder& d) { return d.corrupted || d.st.state == 3; }  // CORRUPTED (:197-199)
    static constexpr auto walk = nx::af::flz_walk;
    static constexpr bool kReadsOn = true;  // decompress may read past its chunk (in_avail = readable bytes)
    static size_t stage_end(size_t n, size_t, size_t) { return n; }
    static int32_t decode(const DecodeItems& it, uint32_t nz) {  // the item word: the bytes readable from the block on
        return nx_fastlz_decompress_batch(it.d_in(), it.d_in_off(), it.d_in_len(), it.d_item_word(), it.d_out(), it.d_out_off(),
                                          it.d_out_len(), it.d_status(), nz, it.g.s);
    }
    static bool block_error(int32_t r, const Blk& b, uint8_t first, int32_t* code, std::string* msg) {
        return nx::af::flz_block_error(r, b.olen, first, code, msg);
    }
    static bool checked(const nx_fastlz_frame_decoder& d, const Blk& b) { return b.has_cks && d.validate; }
    static int32_t checksum(const uint8_t* base, const uint64_t* off, const uint32_t* len, uint32_t* out, uint32_t n, hipStream_t s) {
        return nx_adler32_batch(base, off, len, out, n, s);
    }
    static bool checksum_error(uint32_t got, const Blk& b, int32_t* code, std::string* msg, size_t* at) {  // :171-180
        if (got == b.cks) return false;
        *code = NX_ERR_FASTLZ_CRC_MISMATCH;
        *msg = nx::af::flz_checksum_error(got, b.cks);
        *at = b.data;
        return true;
    }
    static bool emits(const Blk& b) { return b.olen > 0; }
};

struct LzfSync {
    static bool skips(const nx_lzf_decoder& d) { return d.corrupted || d.st.state == 3; }  // CORRUPTED (:229-231)
    static constexpr auto walk = nx::af::lzf_walk;
    static constexpr bool kReadsOn = false;
    static size_t stage_end(size_t, size_t p, size_t) { return p; }
    static int32_t decode(const DecodeItems& it, uint32_t nz) {
        return nx_lzf_decode_batch(it.d_in(), it.d_in_off(), it.d_in_len(), it.d_out(), it.d_out_off(), it.d_out_len(), it.d_status(), nz,
                                   it.g.s);
    }
    static bool block_error(int32_t st, const Blk&, uint8_t, int32_t* code, std::string* msg) {
        if (st == NX_OK) return false;
        *code = st;
        *msg = nx::af::lzf_block_error();
        return true;
    }
    static bool checked(const nx_lzf_decoder&, const Blk&) { return false; }  // LZF blocks carry no checksum
    static int32_t checksum(const uint8_t*, const uint64_t*, const uint32_t*, uint32_t*, uint32_t, hipStream_t) { return NX_OK; }
    static bool checksum_error(uint32_t, const Blk&, int32_t*, std::string*, size_t*) { return false; }
    static bool emits(const Blk& b) { return b.comp || b.clen > 0; }
};

struct Lz4Sync {
    static bool skips(const nx_lz4_frame_decoder& d) { return d.corrupted || d.st.state >= 2; }  // FINISHED / CORRUPTED :250-254
    static constexpr auto walk = nx::af::lz4_walk;
    static constexpr bool kReadsOn = false;
    static size_t stage_end(size_t, size_t, size_t last_end) { return last_end; }
    static int32_t decode(const DecodeItems& it, uint32_t nz) {
        return nx_lz4_decode_batch(it.d_in(), it.d_in_off(), it.d_in_len(), it.d_out(), it.d_out_off(), it.d_out_len(), it.d_status(), nz,
                                   it.g.s);
    }
    static bool block_error(int32_t st, const Blk&, uint8_t, int32_t* code, std::string* msg) {
        if (st == NX_OK) return false;  // LZ4Exception → DecompressionException (:240-241)
        *code = st;
        *msg = nx::af::lz4_block_error();
        return true;
    }
    static bool checked(const nx_lz4_frame_decoder& d, const Blk&) { return d.validate; }
    static int32_t checksum(const uint8_t* base, const uint64_t* off, const uint32_t* len, uint32_t* out, uint32_t n, hipStream_t s) {
        return nx_xxhash32_batch(base, off, len, nx::af::kLz4Seed, out, n, s);
    }
    // CompressionUtil.checkChecksum after the payload was skipped (:222-228; Lz4XXHash32.getValue masks, :101)
    static bool checksum_error(uint32_t h, const Blk& b, int32_t* code, std::string* msg, size_t* at) {
        const uint32_t got = h & 0x0FFFFFFFu;
        if (got == b.cks) return false;
        *code = NX_ERR_LZ4_CHECKSUM_MISMATCH;
        *msg = nx::af::lz4_checksum_error(got, b.cks);
        *at = b.end;
        return true;
    }
    static bool emits(const Blk&) { return true; }
};

template <class C, class D>
int32_t alt_decode(D* d, const uint8_t* in, size_t n, size_t* consumed, const nx_msg** msgs, size_t* n_msgs, const char** err_msg) {
    const nx::NoGrowScope no_grow;
    DecodeCall call(d, in, n, consumed, msgs, n_msgs, err_msg);
    if (call.refused()) return NX_ERR_INVALID_ARG;
    if (C::skips(*d)) return call.skip_all();
    MsgList& ml = call.ml();
    // host parse (decode() as callDecode drives it) on a copy of the header state, committed at the end
    auto ns = d->st;
    std::vector<Blk> blks;
    nx::af::WalkErr werr;
    const size_t p = C::walk(in, n, ns, blks, werr);
    const uint32_t nb = (uint32_t)blks.size();
    const size_t lo = nb ? blks.front().data : 0;
    // the items: every compressed block, into its 16-byte aligned slot of dout
    DecodeItems it(d->g, false);
    std::vector<uint32_t> job(nb), cjob(nb), olen, iav;
    for (uint32_t i = 0; i < nb; ++i) {
        const Blk& b = blks[i];
        if (!b.comp) continue;
        job[i] = it.size();
        it.add(b.data - lo, b.clen, ((uint64_t)b.olen + 15) & ~15ull);
        olen.push_back(b.olen);
        if (C::kReadsOn) iav.push_back((uint32_t)(n - b.data));
    }
    // the checksum jobs: the decoded blocks first (their bytes in dout), then the raw ones (where they lie
    // in the staged input, din)
    uint32_t ncz = 0;
    for (int raw = 0; raw < 2; ++raw) {
        for (uint32_t i = 0; i < nb; ++i) {
            const Blk& b = blks[i];
            if (b.comp == (raw != 0) || !C::checked(*d, b)) continue;
            cjob[i] = it.jobs();
            it.add_job(b.comp ? it.out_off[job[i]] : b.data - lo, b.comp ? b.olen : b.clen);
        }
        if (!raw) ncz = it.jobs();
    }
    const uint32_t nz = it.size(), ncr = it.jobs() - ncz;
    std::vector<uint8_t> hout(it.out_bytes);
    if (nz || it.jobs()) {  // everything is uploaded before the first launch; one sync at the end
        int32_t r = it.stage(in + lo, C::stage_end(n, p, blks.back().end) - lo, &olen, C::kReadsOn ? &iav : nullptr);
        if (r == NX_OK && nz) r = C::decode(it, nz);
        if (r == NX_OK && ncz) r = C::checksum(it.d_out(), it.d_job_off(), it.d_job_len(), it.d_job_val(), ncz, d->g.s);
        if (r == NX_OK && ncr) r = C::checksum(it.d_in(), it.d_job_off(ncz), it.d_job_len(ncz), it.d_job_val(ncz), ncr, d->g.s);
        if (r != NX_OK) return call.finish(r);
        if (!it.fetch(hout.data())) return call.finish(NX_ERR_HIP);
    }
    // apply in stream order: a block's failure, then its checksum, then its message
    Failure bad;
    for (uint32_t i = 0; i < nb; ++i) {
        const Blk& b = blks[i];
        if (b.comp && C::block_error(it.st[job[i]], b, b.data < n ? in[b.data] : 0, &bad.code, &bad.text)) bad.at = b.data;
        if (bad.code != NX_OK || (C::checked(*d, b) && C::checksum_error(it.job_val[cjob[i]], b, &bad.code, &bad.text, &bad.at))) break;
        if (!C::emits(b)) continue;
        if (b.comp) {  // decoded bytes are owned by the message list; a raw block is a view of `in`
            const uint8_t* data = hout.data() + it.out_off[job[i]];
            ml.owned.emplace_back(data, data + b.olen);
            ml.msgs.push_back({ml.owned.back().data(), b.olen});
        } else {
            ml.msgs.push_back({in + b.data, b.clen});
        }
    }
    if (bad.code == NX_OK && werr.set) bad = {werr.code, werr.msg, werr.at};
    if (bad.code != NX_OK) {  // the decoder turns CORRUPTED
        d->st.state = 3;
        d->corrupted = true;
        return call.fail(bad.code, bad.text, bad.at);
    }
    d->st = ns;
    call.rd = p;
    return call.finish(NX_OK);
}
}  // namespace

// ======================================================================= FastLZ frame decoder
extern "C" nx_fastlz_frame_decoder* nx_fastlz_frame_decoder_new(int32_t validate) {
    auto* d = make_handle<nx_fastlz_frame_decoder>(nx::WsKind::DecRecords);  // FastLZ blocks decode through the record expander
    if (d) d->validate = validate != 0;
    return d;
}
extern "C" void nx_fastlz_frame_decoder_free(nx_fastlz_frame_decoder* d) { nx_alt_decoder_unref(d); }

extern "C" int32_t nx_fastlz_frame_decoder_decode(nx_fastlz_frame_decoder* d, const uint8_t* in, size_t n, size_t* consumed,
                                                  const nx_msg** msgs, size_t* n_msgs, const char** err_msg) {
    return alt_decode<FlzSync>(d, in, n, consumed, msgs, n_msgs, err_msg);
}

// ======================================================================= LZF encoder / decoder
// LzfEncoder(totalLength, compressThreshold) (LzfEncoder.java:127-166).  totalLength is validated as
// :147-150 does (MIN_BLOCK_TO_COMPRESS 16 .. MAX_CHUNK_LEN 65535) and does not change the bytes: it
// only sizes the ChunkEncoder's hash table, and the non-allocating encoders LzfEncoder takes
// (ChunkEncoderFactory.optimalNonAllocatingInstance / safeNonAllocatingInstance, :161-163) size it from
// max(totalLength, MAX_CHUNK_LEN), i.e. the 16384-entry table for every totalLength (compress-lzf
// 1.0.3 ChunkEncoder(int, BufferRecycler, boolean); DESIGN.md §2: restated, not pinned).
extern "C" nx_lzf_encoder* nx_lzf_encoder_new_ex(int32_t total_length, int32_t compress_threshold) {
    if (total_length < 16 || total_length > 65535) return nullptr;  // :147-150
    return nx_lzf_encoder_new(compress_threshold);
}

extern "C" nx_lzf_encoder* nx_lzf_encoder_new(int32_t compress_threshold) {
    if (compress_threshold < 16) return nullptr;  // LzfEncoder.java:152-156
    auto* e = make_handle<nx_lzf_encoder>(nx::WsKind::LzfEnc);
    if (e) e->threshold = compress_threshold;
    return e;
}
extern "C" void nx_lzf_encoder_free(nx_lzf_encoder* e) { delete e; }
extern "C" size_t nx_lzf_frame_max_encoded_length(size_t n) { return (n / 65535 + 1) * 7 + n + n / 32 + 64; }

extern "C" int64_t nx_lzf_encoder_encode(nx_lzf_encoder* e, const uint8_t* in, size_t n, uint8_t* out, size_t out_cap) {
    const nx::NoGrowScope no_grow;
    if (!e) return NX_ERR_INVALID_ARG;
    if (out_cap < nx_lzf_frame_max_encoded_length(n)) return NX_ERR_INVALID_ARG;
    if ((int64_t)n < e->threshold) {  // encodeNonCompress (LzfEncoder.java:197-203,223-246)
        size_t op = 0, ip = 0;
        do {
            const uint32_t len = (uint32_t)((n - ip) < 65535 ? (n - ip) : 65535);
            out[op] = 'Z';
            out[op + 1] = 'V';
            out[op + 2] = 0;
            out[op + 3] = (uint8_t)(len >> 8);
            out[op + 4] = (uint8_t)len;
            nx::copy_bytes(out + op + 5, in + ip, len);
            op += 5 + len;
            ip += len;
        } while (ip < n);
        return (int64_t)op;
    }
    EncodeItems it(e->g);
    for_each_piece(n, 65535, [&](size_t off, size_t len) { it.add(off, (uint32_t)len, nx_lzf_max_compressed_length(len) + 16); });
    int32_t r = it.stage(in, n);
    if (r != NX_OK) return r;
    r = nx_lzf_encode_batch(it.d_in(), it.d_in_off(), it.d_in_len(), it.d_out(), it.d_out_off(), it.d_out_len(), it.d_status(),
                            it.size(), e->g.s);
    if (r != NX_OK) return r;
    // the lengths only: this encoder has never read its items' statuses, and still does not
    if (!it.fetch(false)) return NX_ERR_HIP;
    size_t op = 0;
    if (!it.copy_packed(out, &op)) return NX_ERR_HIP;  // each block's bytes only, concatenated in place
    return (int64_t)op;
}

extern "C" nx_lzf_decoder* nx_lzf_decoder_new(void) {
    return make_handle<nx_lzf_decoder>(nx::WsKind::DecRecords);  // LZF blocks decode through the record expander
}
extern "C" void nx_lzf_decoder_free(nx_lzf_decoder* d) { nx_alt_decoder_unref(d); }

extern "C" int32_t nx_lzf_decoder_decode(nx_lzf_decoder* d, const uint8_t* in, size_t n, size_t* consumed, const nx_msg** msgs,
                                         size_t* n_msgs, const char** err_msg) {
    return alt_decode<LzfSync>(d, in, n, consumed, msgs, n_msgs, err_msg);
}

// ======================================================================= LZ4 frame encoder / decoder
//   Lz4FrameEncoder   Lz4FrameEncoder.java:231-336 (encode, flushBufferedData, finishEncode)
//   Lz4FrameDecoder   Lz4FrameDecoder.java:121-261
// Every full block of one encode() call (and every block of one decode() call) goes to the GPU in
// one batch: nx_lz4_frame_encode_batch / nx_lz4_decode_batch + nx_xxhash32_batch.
using nx::af::kLz4Header;
using nx::af::kLz4Magic;

extern "C" nx_lz4_frame_encoder* nx_lz4_frame_encoder_new_ex(int32_t block_size, int32_t high_compressor, int32_t max_encode_size) {
    // compressionLevel(blockSize) :158-166; the device block encoder takes blocks below 32 MiB
    if (block_size < 64 || block_size > (1 << 25) || max_encode_size <= 0) return nullptr;
    auto* e = make_handle<nx_lz4_frame_encoder>(high_compressor ? nx::WsKind::Lz4HcEnc : nx::WsKind::Lz4Enc);
    if (!e) return nullptr;
    e->high = high_compressor != 0;
    e->max_encode_size = max_encode_size;
    e->block_size = (uint32_t)block_size;
    const int32_t ceil_log2 = 32 - __builtin_clz((uint32_t)block_size - 1u);
    e->level = ceil_log2 - 10 > 0 ? ceil_log2 - 10 : 0;
    e->buf.reserve(block_size);
    return e;
}
extern "C" nx_lz4_frame_encoder* nx_lz4_frame_encoder_new(int32_t block_size) {
    return nx_lz4_frame_encoder_new_ex(block_size, 0, 0x7FFFFFFF);
}
extern "C" void nx_lz4_frame_encoder_free(nx_lz4_frame_encoder* e) { delete e; }
extern "C" const char* nx_lz4_frame_encoder_error(nx_lz4_frame_encoder* e) { return last_error(e); }
extern "C" size_t nx_lz4_frame_max_encoded_length(size_t n, int32_t block_size) {
    const size_t bs = block_size > 0 ? (size_t)block_size : 65536;
    return (n / bs + 2) * (kLz4Header + 16 + bs / 255) + n + kLz4Header;
}

namespace {
// flushBufferedData (:248-284) for nb consecutive blocks of `src` (the last may be short).
int64_t lz4_flush_blocks(nx_lz4_frame_encoder* e, const uint8_t* src, size_t n, uint8_t* out, size_t out_cap) {
    if (n == 0) return 0;
    EncodeItems it(e->g);
    for_each_piece(n, e->block_size,
                   [&](size_t off, size_t len) { it.add(off, (uint32_t)len, kLz4Header + nx_lz4_max_compressed_length(len)); });
    int32_t r = it.stage(src, n);
    if (r != NX_OK) return r;
    r = nx_lz4_frame_encode_batch_ex(it.d_in(), it.d_in_off(), it.d_in_len(), it.d_out(), it.d_out_off(), it.d_out_len(), e->level,
                                     e->high ? 1 : 0, it.d_status(), it.size(), e->g.s);
    if (r != NX_OK) return r;
    if (!it.fetch(true)) return NX_ERR_HIP;
    r = it.check_packed(out_cap);
    if (r != NX_OK) return r;
    size_t op = 0;
    if (!it.copy_packed(out, &op)) return NX_ERR_HIP;  // each framed block's bytes only, concatenated in place
    return (int64_t)op;
}
}  // namespace

// allocateBuffer's size check (:190-214): the blocks of `remaining` pending bytes, each
// maxCompressedLength(curSize) + HEADER_LENGTH, against maxEncodeSize (Java int arithmetic: a sum
// that overflows is negative and fails too).  Returns NX_OK or NX_ERR_LZ4_ENCODE_SIZE with the message.
int32_t nx_lz4_frame_encoder_check_size(nx_lz4_frame_encoder* e, uint64_t remaining, int32_t* target_out) {
    if (target_out) *target_out = 0;
    if (remaining > 0x7FFFFFFFull) {  // int remaining < 0 (:195-197)
        e->err = "too much data to allocate a buffer for compression";
        return NX_ERR_LZ4_ENCODE_SIZE;
    }
    int64_t target = 0;
    while (remaining > 0) {
        const uint64_t cur = remaining < e->block_size ? remaining : e->block_size;
        remaining -= cur;
        target += (int64_t)nx_lz4_max_compressed_length(cur) + (int64_t)kLz4Header;
    }
    const int32_t t32 = (int32_t)(uint32_t)(uint64_t)target;  // the Java int sum
    if (t32 > e->max_encode_size || t32 < 0) {
        char buf[160];
        snprintf(buf, sizeof buf, "requested encode buffer size (%d bytes) exceeds the maximum allowable size (%d bytes)", t32,
                 e->max_encode_size);
        e->err = buf;
        return NX_ERR_LZ4_ENCODE_SIZE;
    }
    if (target_out) *target_out = t32;
    return NX_OK;
}

// encode() after close() (:233-239): write()'s allocateBuffer(allowEmptyReturn = true) hands encode an
// EMPTY_BUFFER when the message's blocks need fewer than blockSize bytes (:216-218), and encode then
// throws; a larger message gets a buffer of its size and passes through.
int32_t nx_lz4_frame_encoder_check_finished(nx_lz4_frame_encoder* e, size_t n, int32_t target) {
    if (!e->finished || n == 0 || target >= (int32_t)e->block_size) return NX_OK;
    e->err = "encode finished and not enough space to write remaining data";
    return NX_ERR_LZ4_ENCODE_FINISHED;
}

extern "C" int64_t nx_lz4_frame_encoder_encode(nx_lz4_frame_encoder* e, const uint8_t* in, size_t n, uint8_t* out,
                                               size_t out_cap) {
    const nx::NoGrowScope no_grow;
    if (!e || (!in && n)) return NX_ERR_INVALID_ARG;
    {   // MessageToByteEncoder.write: allocateBuffer before encode (:190-214), also after close()
        int32_t target = 0;
        int32_t r = nx_lz4_frame_encoder_check_size(e, (uint64_t)n + e->buf.size(), &target);
        if (r == NX_OK) r = nx_lz4_frame_encoder_check_finished(e, n, target);
        if (r != NX_OK) return r;
    }
    if (e->finished) {  // :233-239 — after close() a message of at least a block's buffer passes through
        if (out_cap < n) return NX_ERR_INVALID_ARG;
        if (n) memcpy(out, in, n);
        return (int64_t)n;
    }
    // :241-248 — fill the block buffer; every full buffer is flushed
    return nx::h::write_blocks(e->buf, e->block_size, in, n,
                               [&](const uint8_t* src, size_t full) { return lz4_flush_blocks(e, src, full, out, out_cap); });
}

static int64_t lz4_flush_buffer(nx_lz4_frame_encoder* e, uint8_t* out, size_t out_cap) {
    const int64_t w = lz4_flush_blocks(e, e->buf.data(), e->buf.size(), out, out_cap);
    if (w >= 0) e->buf.clear();
    return w;
}

extern "C" int64_t nx_lz4_frame_encoder_flush(nx_lz4_frame_encoder* e, uint8_t* out, size_t out_cap) {
    const nx::NoGrowScope no_grow;
    if (!e) return NX_ERR_INVALID_ARG;  // flush() :296-304: allocateBuffer(ctx, EMPTY_BUFFER, .., false) first
    if (!e->buf.empty()) {
        const int32_t r = nx_lz4_frame_encoder_check_size(e, e->buf.size());
        if (r != NX_OK) return r;
    }
    return lz4_flush_buffer(e, out, out_cap);
}

extern "C" int64_t nx_lz4_frame_encoder_close(nx_lz4_frame_encoder* e, uint8_t* out, size_t out_cap) {
    const nx::NoGrowScope no_grow;
    if (!e) return NX_ERR_INVALID_ARG;
    if (e->finished) return 0;  // finishEncode :306-310
    const int64_t w = lz4_flush_buffer(e, out, out_cap);  // the footer buffer: no maxEncodeSize check (:313-315)
    if (w < 0) return w;
    if ((size_t)w + kLz4Header > out_cap) return NX_ERR_INVALID_ARG;
    uint8_t* f = out + w;  // the end block :326-335
    memcpy(f, kLz4Magic, 8);
    f[8] = (uint8_t)(0x10 | e->level);
    memset(f + 9, 0, 12);
    e->finished = true;
    return w + kLz4Header;
}

// ------------------------------------------------------------------ ZstdEncoder
namespace {
constexpr size_t kZstdSlice = 65536;  // a frame of the batch encoder holds at most this much

// flushBufferedData (ZstdEncoder.java:146-168) for the consecutive blocks of `src` (the last may be
// short): one launch for all of them.  A block over 64 KiB is cut into 64 KiB slices, each its own frame.
int64_t zstd_flush_blocks(nx_zstd_encoder* e, const uint8_t* src, size_t n, uint8_t* out, size_t out_cap) {
    if (n == 0) return 0;
    EncodeItems it(e->g);
    for_each_piece(n, e->block_size, [&](size_t b, size_t blen) {
        for_each_piece(blen, kZstdSlice, [&](size_t q, size_t len) {
            it.add(b + q, (uint32_t)len, (nx_zstd_max_compressed_length(len) + 15) / 16 * 16);
        });
    });
    int32_t r = it.stage(src, n);
    if (r != NX_OK) return r;
    r = nx_zstd_encode_batch(it.d_in(), it.d_in_off(), it.d_in_len(), it.d_out(), it.d_out_off(), it.d_out_len(), it.d_status(),
                             it.size(), e->level, e->g.s);
    if (r != NX_OK) return r;
    if (!it.fetch(true)) return NX_ERR_HIP;
    r = it.check_packed(out_cap);
    if (r != NX_OK) return r;
    size_t op = 0;
    if (!it.copy_span_packed(out, &op)) return NX_ERR_HIP;
    return (int64_t)op;
}

// allocateBuffer's size check (:105-122): remaining as a Java int, the sum as a Java long.
int32_t zstd_check_size(nx_zstd_encoder* e, uint64_t remaining) {
    if (remaining > 0x7FFFFFFFull) {  // int remaining < 0 (:108-110)
        e->err = "too much data to allocate a buffer for compression";
        return NX_ERR_ZSTD_ENCODE_SIZE;
    }
    int64_t target = 0;
    if (remaining >= e->block_size) {  // the full blocks all have one bound
        const uint64_t full = remaining / e->block_size;
        target += (int64_t)(full * nx_zstd_max_compressed_length(e->block_size));
        remaining -= full * e->block_size;
    }
    if (remaining) target += (int64_t)nx_zstd_max_compressed_length(remaining);
    if (target > e->max_encode_size || target < 0) {
        char buf[160];
        snprintf(buf, sizeof buf, "requested encode buffer size (%lld bytes) exceeds the maximum allowable size (%d bytes)",
                 (long long)target, e->max_encode_size);
        e->err = buf;
        return NX_ERR_ZSTD_ENCODE_SIZE;
    }
    return NX_OK;
}
}  // namespace

extern "C" nx_zstd_encoder* nx_zstd_encoder_new(int32_t level, int32_t block_size, int32_t max_encode_size) {
    // checkInRange(compressionLevel, MIN, MAX), checkPositive(blockSize), checkPositive(maxEncodeSize) :92-95
    if (level < -131072 || level > 22 || block_size <= 0 || max_encode_size <= 0) return nullptr;
    auto* e = make_handle<nx_zstd_encoder>(nx::WsKind::ZstdEnc);
    if (!e) return nullptr;
    e->level = level;
    e->block_size = (uint32_t)block_size;
    e->max_encode_size = max_encode_size;
    return e;
}
extern "C" void nx_zstd_encoder_free(nx_zstd_encoder* e) { delete e; }
extern "C" const char* nx_zstd_encoder_error(nx_zstd_encoder* e) { return last_error(e); }
extern "C" size_t nx_zstd_max_encoded_length(size_t pending, int32_t block_size) {
    const size_t bs = block_size > 0 ? (size_t)block_size : 65536;
    return pending / bs * nx_zstd_max_compressed_length(bs) + nx_zstd_max_compressed_length(pending % bs);
}

extern "C" int64_t nx_zstd_encoder_encode(nx_zstd_encoder* e, const uint8_t* in, size_t n, uint8_t* out, size_t out_cap) {
    const nx::NoGrowScope no_grow;
    if (!e || (!in && n)) return NX_ERR_INVALID_ARG;
    {   // MessageToByteEncoder.write: allocateBuffer before encode (:105-122)
        const int32_t r = zstd_check_size(e, (uint64_t)n + e->buf.size());
        if (r != NX_OK) return r;
    }
    // :136-143 — fill the block buffer; every full buffer is flushed
    return nx::h::write_blocks(e->buf, e->block_size, in, n,
                               [&](const uint8_t* src, size_t full) { return zstd_flush_blocks(e, src, full, out, out_cap); });
}

extern "C" int64_t nx_zstd_encoder_flush(nx_zstd_encoder* e, uint8_t* out, size_t out_cap) {
    const nx::NoGrowScope no_grow;
    if (!e) return NX_ERR_INVALID_ARG;
    if (e->buf.empty()) return 0;  // flush() :171-178: nothing readable, nothing allocated
    const int32_t r = zstd_check_size(e, e->buf.size());
    if (r != NX_OK) return r;
    const int64_t w = zstd_flush_blocks(e, e->buf.data(), e->buf.size(), out, out_cap);
    if (w >= 0) e->buf.clear();
    return w;
}

// ------------------------------------------------------------------ LzmaFrameEncoder
// LzmaFrameEncoder.java:177-186: every encode() is one complete stream (header, payload from a fresh model).
extern "C" int32_t nx_lzma_frame_encoder_check(int32_t lc, int32_t lp, int32_t pb, int32_t dict_size, int32_t num_fast_bytes) {
    if (lc < 0 || lc > 8 || lp < 0 || lp > 4 || pb < 0 || pb > 4) return NX_ERR_LZMA_PROPS;  // :139-147
    if (dict_size < 0) return NX_ERR_LZMA_DICT_SIZE;                                        // :157-159
    if (num_fast_bytes < 5 || num_fast_bytes > 273) return NX_ERR_LZMA_FAST_BYTES;          // :160-164
    return NX_OK;
}

extern "C" nx_lzma_frame_encoder* nx_lzma_frame_encoder_new(int32_t lc, int32_t lp, int32_t pb, int32_t dict_size, int32_t end_marker,
                                                            int32_t num_fast_bytes) {
    if (nx_lzma_frame_encoder_check(lc, lp, pb, dict_size, num_fast_bytes) != NX_OK) return nullptr;
    auto* e = new nx_lzma_frame_encoder();
    // a write is one item: one table slot.  (lc + lp > 4 encodes on the host, and holds nothing.)
    if (lc + lp <= 4) {
        if (!e->g.ok || nx::ws_hold(nx::WsKind::LzmaEnc, e->g.dev, 1u, e->g.s) != NX_OK) {
            delete e;
            return nullptr;
        }
        e->g.held |= 1u << (int)nx::WsKind::LzmaEnc;
    }
    e->lc = lc;
    e->lp = lp;
    e->pb = pb;
    e->dict_size = dict_size;
    e->end_marker = end_marker != 0;
    e->num_fast_bytes = num_fast_bytes;
    return e;
}
extern "C" void nx_lzma_frame_encoder_free(nx_lzma_frame_encoder* e) { delete e; }
extern "C" const char* nx_lzma_frame_encoder_error(nx_lzma_frame_encoder* e) { return last_error(e); }
extern "C" size_t nx_lzma_frame_max_encoded_length(size_t n) { return nx_lzma_max_compressed_length(n); }

extern "C" int64_t nx_lzma_frame_encoder_encode(nx_lzma_frame_encoder* e, const uint8_t* in, size_t n, uint8_t* out, size_t out_cap) {
    const nx::NoGrowScope no_grow;
    if (!e || (!in && n) || (!out && out_cap) || n > 0x7FFFFFFFull) return NX_ERR_INVALID_ARG;
    auto fail = [&](int64_t r) {
        if (r < 0) e->err = r == NX_ERR_LZMA_ENCODE_FULL ? "the LZMA stream does not fit the output buffer" : nx_status_string((int32_t)r);
        return r;
    };
    if (e->lc + e->lp > 4)
        return fail(nx_lzma_encode_host(in, n, e->lc, e->lp, e->pb, e->dict_size, e->end_marker, out, out_cap, nullptr));
    return fail(EncodeItems(e->g).encode_one(in, n, nx_lzma_max_compressed_length(n), out, out_cap, [&](EncodeItems& it) {
        return nx_lzma_encode_batch(it.d_in(), it.d_in_off(), it.d_in_len(), it.d_out(), it.d_out_off(), it.d_out_len(), it.d_status(), 1u,
                                    e->lc, e->lp, e->pb, e->dict_size, e->end_marker, e->g.s);
    }));
}

// ------------------------------------------------------------------ BrotliEncoder
// BrotliEncoder.java:47-230: one stream per channel, every write compressed and flushed (Writer.write, :205-216).
extern "C" int32_t nx_brotli_encoder_check(int32_t quality, int32_t lgwin, int32_t mode) {
    if (quality < -1 || quality > 11) return NX_ERR_BROTLI_QUALITY;
    if (lgwin != -1 && (lgwin < 10 || lgwin > 24)) return NX_ERR_BROTLI_LGWIN;
    if (mode < 0 || mode > 2) return NX_ERR_BROTLI_MODE;
    return NX_OK;
}

extern "C" nx_brotli_encoder* nx_brotli_encoder_new(int32_t quality, int32_t lgwin, int32_t mode) {
    if (nx_brotli_encoder_check(quality, lgwin, mode) != NX_OK) return nullptr;
    auto* e = new nx_brotli_encoder();
    // a write is one item: one table slot
    if (!e->g.ok || nx::ws_hold(nx::WsKind::BrotliEnc, e->g.dev, 1u, e->g.s) != NX_OK) {
        delete e;
        return nullptr;
    }
    e->g.held |= 1u << (int)nx::WsKind::BrotliEnc;
    e->quality = quality;
    e->lgwin = lgwin == -1 ? 22 : lgwin;
    e->mode = mode;
    return e;
}
extern "C" void nx_brotli_encoder_free(nx_brotli_encoder* e) { delete e; }
extern "C" const char* nx_brotli_encoder_error(nx_brotli_encoder* e) { return last_error(e); }
extern "C" int32_t nx_brotli_encoder_is_closed(nx_brotli_encoder* e) { return e && e->closed ? 1 : 0; }
// a write: the header (under a byte), the bound, which has room for the flush marker's bits, and one byte to spare
extern "C" size_t nx_brotli_encoder_max_encoded_length(size_t n) { return 1u + nx_brotli_max_compressed_length(n) + 1u; }

extern "C" int64_t nx_brotli_encoder_encode(nx_brotli_encoder* e, const uint8_t* in, size_t n, uint8_t* out, size_t out_cap) {
    const nx::NoGrowScope no_grow;
    if (!e || (!in && n) || (!out && out_cap) || n > (256u << 20)) return NX_ERR_INVALID_ARG;
    if (n == 0 || e->closed) return 0;  // :125-127 an unreadable message; :136-139 no writer any more
    auto fail = [&](int64_t r) {
        if (r < 0) e->err = r == NX_ERR_BROTLI_ENCODE_FULL ? "the Brotli write does not fit the output buffer" : nx_status_string((int32_t)r);
        return r;
    };
    const int64_t w = EncodeItems(e->g).encode_one(in, n, nx_brotli_encoder_max_encoded_length(n), out, out_cap, [&](EncodeItems& it) {
        return nx::brotli_encode_items(it.d_in(), it.d_in_off(), it.d_in_len(), it.d_out(), it.d_out_off(), it.d_out_len(), it.d_status(), 1u,
                                       e->lgwin, (e->started ? 0u : nx::brotli::kFlagHeader) | nx::brotli::kFlagFlush, e->g.s);
    });
    if (w >= 0) e->started = true;
    return fail(w);
}

extern "C" int64_t nx_brotli_encoder_close(nx_brotli_encoder* e, uint8_t* out, size_t out_cap) {
    if (!e || (!out && out_cap)) return NX_ERR_INVALID_ARG;
    if (e->closed) return 0;
    int64_t r = 1;
    if (e->started) {
        if (out_cap < 1u) r = NX_ERR_BROTLI_ENCODE_FULL;
        else out[0] = 0x03;  // ISLAST 1, ISLASTEMPTY 1 on a byte boundary, which every write ends on
    } else {
        r = nx_brotli_encode_host(nullptr, 0, e->lgwin, out, out_cap, nullptr);  // the header and the last block
    }
    if (r < 0) {
        e->err = nx_status_string((int32_t)r);
        return r;
    }
    e->closed = true;
    return r;
}

// ------------------------------------------------------------------ Bzip2Encoder
// Bzip2Encoder.java:105-228 over nx_bzip2_encode_batch_split.  The planner runs on the host over every write
// (nx_bzip2_plan_resume_host), the open block's input stays in host memory, and a write that closes k blocks
// uploads their bytes and makes one call with a segment that is not the stream's last: the k blocks run on k
// workgroups, the call hands back whole 32-bit words as Bzip2BitWriter.writeBits does, and the other bits and the
// stream CRC wait in the handle.  close() sends the open block as the last segment.
namespace {
constexpr uint32_t kBzip2HandleBlocks = 4;  // blocks in flight the handle holds slots for; more run in rounds

// data[0, len) = `blocks` whole blocks behind the handle's carry, as one item of one launch
int64_t bzip2_segment(nx_bzip2_encoder* e, const uint8_t* data, size_t len, uint32_t blocks, bool last, uint8_t* out, size_t out_cap) {
    if (len > 0xffffffffull) return NX_ERR_INVALID_ARG;
    Gpu& g = e->g;
    const size_t cap = nx_bzip2_max_compressed_length(len, e->level) + 8u;
    struct Par {
        uint64_t in_off, out_off;
        uint32_t in_len, out_cap, out_len;
        int32_t status;
        nx_bzip2_seg seg;
    } p = {0, 0, (uint32_t)len, (uint32_t)cap, 0, 0, e->seg};
    p.seg.flags = last ? NX_BZIP2_SEG_LAST : 0u;
    const ParamBlock<Par> P(g, g.aux0);  // the one item's arrays, uploaded and read back whole
    if (!g.din.ensure(len ? len : 1u) || !g.dout.ensure(cap) || !P.ensure()) return NX_ERR_HIP;
    if (!g.h2d(g.din.p, data, len) || !P.upload(p)) return NX_ERR_HIP;
    const int32_t r = nx_bzip2_encode_batch_split(g.din.as<uint8_t>(), P.field(&Par::in_off), P.field(&Par::in_len), g.dout.as<uint8_t>(),
                                                  P.field(&Par::out_off), P.field(&Par::out_cap), P.field(&Par::out_len),
                                                  P.field(&Par::status), 1, e->level, blocks, P.field(&Par::seg), g.s);
    if (r != NX_OK) return r;
    e->launches += 1;
    if (!P.download(p, &Par::in_off) || !g.sync()) return NX_ERR_HIP;
    if (p.status != NX_OK) return p.status;
    if (p.out_len > out_cap) return NX_ERR_INVALID_ARG;
    if (!g.d2h(out, g.dout.p, p.out_len) || !g.sync()) return NX_ERR_HIP;
    e->seg = p.seg;
    return (int64_t)p.out_len;
}

// "BZh" and the level digit (Bzip2Encoder.java:114-119): 32 bits, so nothing is carried behind them
int64_t bzip2_start(nx_bzip2_encoder* e, uint8_t* out, size_t out_cap) {
    if (e->started) return 0;
    if (out_cap < 4u) return NX_ERR_INVALID_ARG;
    out[0] = 'B', out[1] = 'Z', out[2] = 'h', out[3] = (uint8_t)('0' + e->level);
    e->started = true;
    return 4;
}
}  // namespace

extern "C" nx_bzip2_encoder* nx_bzip2_encoder_new(int32_t level) {
    if (level < 1 || level > 9) return nullptr;  // Bzip2Encoder.java:98-101
    auto* e = new nx_bzip2_encoder();
    // the plan arrays' unit and slots for kBzip2HandleBlocks blocks at this level (Gpu::hold's size is the other handles')
    if (!e->g.ok || nx::ws_hold(nx::WsKind::Bzip2Enc, e->g.dev, 1u + kBzip2HandleBlocks * (uint32_t)level, e->g.s) != NX_OK) {
        delete e;
        return nullptr;
    }
    e->g.held |= 1u << (int)nx::WsKind::Bzip2Enc;
    e->level = level;
    return e;
}
extern "C" void nx_bzip2_encoder_free(nx_bzip2_encoder* e) { delete e; }
extern "C" const char* nx_bzip2_encoder_error(nx_bzip2_encoder* e) { return last_error(e); }
extern "C" int32_t nx_bzip2_encoder_is_closed(const nx_bzip2_encoder* e) { return e && e->finished ? 1 : 0; }
extern "C" uint64_t nx_bzip2_encoder_launches(const nx_bzip2_encoder* e) { return e ? e->launches : 0; }
extern "C" size_t nx_bzip2_encoder_max_encoded_length(const nx_bzip2_encoder* e, size_t n) {
    if (!e) return 0;
    if (e->finished) return n;
    return 4u + nx_bzip2_max_compressed_length(e->open.size() + n, e->level) + 8u;
}

extern "C" int64_t nx_bzip2_encoder_encode(nx_bzip2_encoder* e, const uint8_t* in, size_t n, uint8_t* out, size_t out_cap) {
    const nx::NoGrowScope no_grow;
    if (!e || (!in && n) || (!out && out_cap)) return NX_ERR_INVALID_ARG;
    if (e->finished) {  // :107-110 out.writeBytes(in)
        if (n > out_cap) return NX_ERR_INVALID_ARG;
        nx::copy_bytes(out, in, n);
        return (int64_t)n;
    }
    const int64_t w = bzip2_start(e, out, out_cap);  // State.INIT writes before it looks at `in`
    if (w < 0) return w;
    if (n == 0) return w;
    std::vector<uint64_t> cuts(nx_bzip2_blocks_bound(n, e->level) + 2u);
    size_t count = 0;
    const int32_t r = nx_bzip2_plan_resume_host(in, n, e->level, e->plan, 0, cuts.data(), cuts.size(), &count);
    if (r != NX_OK) return r;
    if (count == 0) {  // :132-138 the block is not full
        e->open.insert(e->open.end(), in, in + n);
        return w;
    }
    const size_t closed = (size_t)cuts[count - 1];  // the bytes of `in` in the blocks this write closes
    const uint8_t* src = in;
    size_t len = closed;
    if (!e->open.empty()) {
        e->open.insert(e->open.end(), in, in + closed);
        src = e->open.data();
        len = e->open.size();
    }
    const int64_t b = bzip2_segment(e, src, len, (uint32_t)count, false, out + w, out_cap - (size_t)w);
    if (b < 0) {
        e->err = nx_status_string((int32_t)b);
        return b;
    }
    e->open.assign(in + closed, in + n);
    return w + b;
}

extern "C" int64_t nx_bzip2_encoder_close(nx_bzip2_encoder* e, uint8_t* out, size_t out_cap) {
    const nx::NoGrowScope no_grow;
    if (!e || (!out && out_cap)) return NX_ERR_INVALID_ARG;
    if (e->finished) return 0;  // finishEncode :208-211
    const int64_t w = bzip2_start(e, out, out_cap);  // (a stream that was never written to still gets its header)
    if (w < 0) return w;
    const int64_t b = bzip2_segment(e, e->open.data(), e->open.size(), e->open.empty() ? 0u : 1u, true, out + w, out_cap - (size_t)w);
    if (b < 0) {
        e->err = nx_status_string((int32_t)b);
        return b;
    }
    e->finished = true;
    e->open.clear();
    e->open.shrink_to_fit();
    return w + b;
}

// ------------------------------------------------------------------ ZstdDecoder
// ZstdDecoder.java:59-122 over nx_zstd_decode_batch_ex: the cumulation is walked on the host
// (nx_zstd_next_frame), every complete frame of the call is an item of one launch.  Where the handle
// departs from the reference (whole frames only) is said at its declaration in netty_amd.h.
extern "C" nx_zstd_decoder* nx_zstd_decoder_new(int32_t maximum_allocation_size) {
    if (maximum_allocation_size < 0) return nullptr;  // checkPositiveOrZero (:64)
    auto* d = make_handle<nx_zstd_decoder>(nx::WsKind::ZstdDec);
    if (d) d->max_alloc = maximum_allocation_size;
    return d;
}
extern "C" void nx_zstd_decoder_free(nx_zstd_decoder* d) { delete d; }
extern "C" int32_t nx_zstd_decoder_stats(const nx_zstd_decoder* d, uint64_t* launches, uint64_t* frames) {
    if (!d || !launches || !frames) return NX_ERR_INVALID_ARG;
    *launches = d->launches;
    *frames = d->frames;
    return NX_OK;
}

extern "C" int32_t nx_zstd_decoder_decode(nx_zstd_decoder* d, const uint8_t* in, size_t n, size_t* consumed, const nx_msg** msgs,
                                          size_t* n_msgs, const char** err_msg) {
    const nx::NoGrowScope no_grow;
    DecodeCall call(d, in, n, consumed, msgs, n_msgs, err_msg);
    if (call.refused()) return NX_ERR_INVALID_ARG;
    if (d->corrupted) return call.skip_all();  // :71-75: in.skipBytes(in.readableBytes())
    MsgList& ml = call.ml();
    // the walk: skippable frames are stepped over, complete frames become items, a frame the input ends
    // inside stops it; `fail` is the status of the first frame the walker refuses
    constexpr uint64_t kMaxBound = 128ull << 20, kMaxFrameBytes = 0x7FFFFFFFull;  // the kernel's positions and lengths
    struct Item {
        uint64_t in_off, out_off;
        uint32_t in_len, out_cap;
    };
    std::vector<Item> items;
    size_t pos = 0;
    uint64_t oc = 0;
    int32_t fail = NX_OK;
    while (pos < n) {
        uint32_t kind = 0, flags = 0;
        uint64_t fb = 0, bound = 0;
        const int32_t st = nx_zstd_next_frame(in + pos, n - pos, &kind, &fb, &bound, &flags);
        if (st == NX_ERR_ZSTD_TRUNCATED) break;
        if (st == NX_OK && kind == NX_ZSTD_KIND_FRAME && (bound > kMaxBound || fb > kMaxFrameBytes)) fail = NX_ERR_ZSTD_WINDOW;
        if (st != NX_OK) fail = st;
        if (fail != NX_OK) break;
        if (kind == NX_ZSTD_KIND_FRAME) {
            items.push_back({pos, oc, (uint32_t)fb, (uint32_t)bound});
            oc += (bound + 15) / 16 * 16;
        }
        pos += (size_t)fb;
    }
    if (!items.empty()) {
        // one copy of the bytes and one of the items' geometry in, one launch, one copy back: the device
        // output starts with the three result arrays, the slots follow
        using nx::h::ZstdGeometry;
        using nx::h::ZstdResults;
        Gpu& g = d->g;
        const uint32_t nb = (uint32_t)items.size();
        const size_t res = ZstdResults::bytes(nb);
        const size_t bytes = (size_t)items.back().in_off + items.back().in_len;
        std::vector<uint64_t> par(ZstdGeometry::bytes(nb) / 8);
        const ZstdGeometry hg(par.data(), nb);
        for (uint32_t i = 0; i < nb; ++i) {
            hg.in_off[i] = items[i].in_off;
            hg.out_off[i] = res + items[i].out_off;
            hg.in_len[i] = items[i].in_len;
            hg.out_cap[i] = items[i].out_cap;
        }
        DevBuf& geom = g.aux0;
        if (!g.din.ensure(bytes) || !geom.ensure(ZstdGeometry::bytes(nb)) || !g.dout.ensure(res + oc)) return call.finish(NX_ERR_HIP);
        if (!g.h2d(g.din.p, in, bytes) || !g.h2d(geom.p, par.data(), ZstdGeometry::bytes(nb))) return call.finish(NX_ERR_HIP);
        const ZstdGeometry dg(geom.p, nb);
        const ZstdResults dr(g.dout.p, nb);
        const int32_t r = nx_zstd_decode_batch_ex(g.din.as<uint8_t>(), dg.in_off, dg.in_len, g.dout.as<uint8_t>(), dg.out_off, dg.out_cap,
                                                  dr.consumed, dr.out_len, dr.status, nb, NX_ZSTD_DECODE_VERIFY_CHECKSUM, g.s);
        if (r != NX_OK) return call.finish(r);
        d->back.resize(res + oc);
        if (!g.d2h(d->back.data(), g.dout.p, res + oc) || !g.sync()) return call.finish(NX_ERR_HIP);
        d->launches += 1;
        d->frames += nb;
        const ZstdResults hr(d->back.data(), nb);
        for (uint32_t i = 0; i < nb; ++i) {
            if (hr.status[i] != NX_OK) {  // the first failing frame: what the walker found later comes after it
                fail = hr.status[i];
                break;
            }
            // :99-110: buffers of min(maximumAllocationSize, uncompressedLength), fired while readable
            const uint8_t* o = d->back.data() + res + items[i].out_off;
            const size_t len = hr.out_len[i] <= items[i].out_cap ? hr.out_len[i] : items[i].out_cap;
            const size_t piece = d->max_alloc > 0 ? (size_t)d->max_alloc : len;
            for (size_t at = 0; at < len; at += piece) ml.msgs.push_back({o + at, len - at < piece ? len - at : piece});
        }
    }
    if (fail != NX_OK) {  // :116-118: CORRUPTED, the exception's text is libzstd's for the error
        d->corrupted = true;
        return call.fail(fail, nx_status_string(fail), n);
    }
    call.rd = pos;
    return call.finish(NX_OK);
}

extern "C" nx_lz4_frame_decoder* nx_lz4_frame_decoder_new(int32_t validate_checksums) {
    auto* d = make_handle<nx_lz4_frame_decoder>(nx::WsKind::DecRecords);
    if (d) d->validate = validate_checksums != 0;
    return d;
}
extern "C" void nx_lz4_frame_decoder_free(nx_lz4_frame_decoder* d) { nx_alt_decoder_unref(d); }

extern "C" int32_t nx_lz4_frame_decoder_decode(nx_lz4_frame_decoder* d, const uint8_t* in, size_t n, size_t* consumed,
                                               const nx_msg** msgs, size_t* n_msgs, const char** err_msg) {
    return alt_decode<Lz4Sync>(d, in, n, consumed, msgs, n_msgs, err_msg);
}

// ======================================================================= JdkZlibEncoder
// JdkZlibEncoder.java:123-137 (constructor), :214-276 (encode), :308-340 (finishEncode).  Every
// encode() ends in a sync flush, so a message is cut into 64 KiB slices that are deflated as
// independent chunks of one launch pair (deflate.hip) and concatenated; the slices' checksums come
// from the same launch sequence and are folded into the running value on the host.

namespace {
constexpr size_t kZlibSlice = 65536;
constexpr uint8_t kGzipHeader[10] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 0};  // gzipHeader (:59)

// the two bytes java.util.zip.Deflater (zlib's deflateInit) writes for a level: CMF 0x78, FLG with
// the level class in its top two bits and the check bits that make the pair a multiple of 31
}  // namespace
size_t nx::zl::write_header(const nx_zlib_encoder* e, uint8_t* out) {
    if (e->wrapper == 1) {
        memcpy(out, kGzipHeader, 10);
        return 10;
    }
    if (e->wrapper == 0) {
        const int32_t l = e->level;
        out[0] = 0x78;
        out[1] = l == 0 || l == 1 ? 0x01 : l >= 2 && l <= 5 ? 0x5E : l == 6 || l == -1 ? 0x9C : 0xDA;
        if (!e->has_dict || e->dict.empty()) return 2;
        // after deflateSetDictionary with a non-empty dictionary (zlib deflate.c, INIT_STATE): PRESET_DICT,
        // the check bits again, then DICTID most significant byte first
        const uint32_t flg = (out[1] & 0xC0u) | 0x20u;
        out[1] = (uint8_t)(flg + 31u - ((0x7800u | flg) % 31u));
        for (int k = 0; k < 4; ++k) out[2 + k] = (uint8_t)(e->dictid >> (8 * (3 - k)));
        return 6;
    }
    return 0;
}

namespace {
// java.util.zip.Adler32 over a dictionary on the host (once per handle)
uint32_t adler32_host(const uint8_t* p, size_t n) {
    uint32_t a = 1, b = 0;
    while (n) {
        const size_t k = n < 5552 ? n : 5552;  // zlib's NMAX: the sums stay below 2^32
        for (size_t i = 0; i < k; ++i) {
            a += p[i];
            b += a;
        }
        a %= 65521u;
        b %= 65521u;
        p += k;
        n -= k;
    }
    return (b << 16) | a;
}
constexpr size_t kZlibDictMax = 32768;  // what of a dictionary the window can hold
}  // namespace

extern "C" nx_zlib_encoder* nx_zlib_encoder_new(int32_t wrapper, int32_t level) {
    if (level < -1 || level > 9) return nullptr;     // checkInRange (:124-125)
    if (wrapper < 0 || wrapper > 2) return nullptr;  // ZLIB_OR_NONE is not allowed for compression (:128-132)
    auto* e = make_handle<nx_zlib_encoder>(nx::WsKind::DeflateEnc);
    if (!e) return nullptr;
    e->wrapper = wrapper;
    e->level = level;
    return e;
}
// JdkZlibEncoder(compressionLevel, dictionary) (:149-177): always ZlibWrapper.ZLIB (:173)
extern "C" nx_zlib_encoder* nx_zlib_encoder_new_dict(int32_t level, const uint8_t* dict, size_t dict_len) {
    if (!dict) return nullptr;  // checkNotNull(dictionary, "dictionary") (:172)
    nx_zlib_encoder* e = nx_zlib_encoder_new(0, level);
    if (!e) return nullptr;
    const size_t tail = dict_len < kZlibDictMax ? dict_len : kZlibDictMax;
    e->has_dict = true;
    e->dict_armed = tail != 0;
    e->dictid = adler32_host(dict, dict_len);
    e->dict.assign(dict + (dict_len - tail), dict + dict_len);
    if (tail && (!e->ddict.ensure(tail) || !e->g.h2d(e->ddict.p, e->dict.data(), tail) || !e->g.sync())) {
        delete e;
        return nullptr;
    }
    return e;
}
extern "C" void nx_zlib_encoder_free(nx_zlib_encoder* e) { nx_zlib_encoder_unref(e); }
extern "C" size_t nx_zlib_max_encoded_length(size_t n) { return 20 + n + (n / kZlibSlice + 1) * 15; }

extern "C" int64_t nx_zlib_encoder_encode(nx_zlib_encoder* e, const uint8_t* in, size_t n, uint8_t* out, size_t out_cap) {
    const nx::NoGrowScope no_grow;
    if (!e || (n && (!in || !out))) return NX_ERR_INVALID_ARG;
    if (e->pending.load()) return NX_ERR_INVALID_ARG;  // unapplied batcher jobs hold the running checksum
    if (e->finished) {  // out.writeBytes(uncompressed) (:215-218)
        if (out_cap < n) return NX_ERR_INVALID_ARG;
        nx::copy_bytes(out, in, n);
        return (int64_t)n;
    }
    if (n == 0) return 0;  // :220-223
    if (out_cap < nx_zlib_max_encoded_length(n)) return NX_ERR_INVALID_ARG;
    // the stream's first slice lies behind the dictionary's tail (its history prefix) in din
    const uint32_t tail = e->dict_armed ? (uint32_t)e->dict.size() : 0u;
    EncodeItems it(e->g);
    std::vector<uint32_t> plen;
    nx::zl::for_slices(n, tail, [&](size_t q, uint32_t len, uint32_t pre) {
        it.add(tail + q, len, (nx_deflate_max_compressed_length(len) + 127) & ~(size_t)127);
        plen.push_back(pre);
    });
    const uint32_t ns = it.size();
    Gpu& g = e->g;
    int32_t r = it.stage(in, n, tail, 4ull * ns, tail ? 4ull * ns : 0);
    if (r != NX_OK) return r;
    uint32_t* d_sum = g.aux0.as<uint32_t>();   // each slice's CRC32 / Adler32
    uint32_t* d_plen = g.aux1.as<uint32_t>();  // each slice's history prefix (the first write of a dictionary stream)
    if (tail && (!g.h2d(d_plen, plen.data(), 4ull * ns) ||
                 hipMemcpyAsync(g.din.p, e->ddict.p, tail, hipMemcpyDeviceToDevice, g.s) != hipSuccess))
        return NX_ERR_HIP;
    if (e->wrapper == 1)
        r = nx_crc32_batch(it.d_in(), it.d_in_off(), it.d_in_len(), d_sum, ns, g.s);
    else if (e->wrapper == 0)
        r = nx_adler32_batch(it.d_in(), it.d_in_off(), it.d_in_len(), d_sum, ns, g.s);
    if (r != NX_OK) return r;
    if (tail)
        r = nx_deflate_encode_batch_ex(it.d_in(), it.d_in_off(), it.d_in_len(), d_plen, it.d_out(), it.d_out_off(), it.d_out_len(),
                                       it.d_status(), ns, e->level, g.s);
    else
        r = nx_deflate_encode_batch(it.d_in(), it.d_in_off(), it.d_in_len(), it.d_out(), it.d_out_off(), it.d_out_len(), it.d_status(),
                                    ns, e->level, g.s);
    if (r != NX_OK) return r;
    std::vector<uint32_t> sum(ns, 0u);
    if (!it.fetch(true, e->wrapper == 2 ? nullptr : d_sum, sum.data())) return NX_ERR_HIP;
    r = it.first_status();
    if (r != NX_OK) return r;
    size_t op = 0;
    if (e->write_header) {
        e->write_header = false;
        op = nx::zl::write_header(e, out);
    }
    if (!it.copy_packed(out, &op)) return NX_ERR_HIP;  // each slice's bytes only, concatenated in place
    const std::vector<uint32_t>& ilen = it.in_len;
    for (uint32_t i = 0; i < ns; ++i) {
        if (e->wrapper == 1) e->crc = nx_crc32_combine(e->crc, sum[i], ilen[i]);
        else if (e->wrapper == 0) e->adler = nx_adler32_combine(e->adler, sum[i], ilen[i]);
    }
    e->total_in += n;
    e->dict_armed = false;
    return (int64_t)op;
}

// finishEncode (:308-340): the header if nothing was written, the final block (an empty fixed-Huffman
// block, what deflater.finish() adds after a sync flush), then the wrapper's trailer.
extern "C" int64_t nx_zlib_encoder_close(nx_zlib_encoder* e, uint8_t* out, size_t out_cap) {
    if (!e || e->pending.load()) return NX_ERR_INVALID_ARG;
    if (e->finished) return 0;  // :309-312
    if (!out || out_cap < 20) return NX_ERR_INVALID_ARG;
    e->finished = true;
    size_t op = 0;
    if (e->write_header) {
        e->write_header = false;
        op = nx::zl::write_header(e, out);
    }
    out[op++] = 0x03;
    out[op++] = 0x00;
    if (e->wrapper == 0) {  // the zlib trailer: Adler32, most significant byte first
        for (int k = 3; k >= 0; --k) out[op++] = (uint8_t)(e->adler >> (8 * k));
    } else if (e->wrapper == 1) {  // writeIntLE(crc), writeIntLE(totalIn) (:331-335)
        const uint32_t isize = (uint32_t)e->total_in;
        for (int k = 0; k < 4; ++k) out[op++] = (uint8_t)(e->crc >> (8 * k));
        for (int k = 0; k < 4; ++k) out[op++] = (uint8_t)(isize >> (8 * k));
    }
    return (int64_t)op;
}

// ======================================================================= JdkZlibDecoder
// JdkZlibDecoder.java:117-160 (constructors), :198-314 (decode), :316-520 (the GZIP header and footer),
// ZlibDecoder.java:49,62-84 (maxAllocation).  The wrappers are a few bytes per stream and are parsed
// here; the deflate body runs through nx_inflate_batch with n = 1 over a device window (32 KiB of
// history, then an output chunk), and the output's CRC32 / Adler32 comes from the batch checksum
// kernels over that window in the same launch sequence.  One call handles what ByteToMessageDecoder.
// callDecode's loop would hand to decode() in turn.

namespace {
constexpr uint32_t kZlibHist = 32768;
constexpr uint32_t kZlibChunk = 1u << 20;  // output bytes per inflate launch (one message each when maxAllocation == 0)
constexpr int32_t FHCRC = 0x02, FEXTRA = 0x04, FNAME = 0x08, FCOMMENT = 0x10, FRESERVED = 0xE0;  // :48-52

// java.util.zip.CRC32.update over the header bytes (a few bytes per stream)
uint32_t crc32_host(uint32_t crc, const uint8_t* p, size_t n) {
    crc = ~crc;
    for (size_t i = 0; i < n; ++i) {
        crc ^= p[i];
        for (int k = 0; k < 8; ++k) crc = (crc >> 1) ^ (nx::kCrc32Poly & (0u - (crc & 1u)));
    }
    return ~crc;
}

enum { kZNeed = 0, kZOk = 1 };  // (< 0: failed, ml.err holds the message)

// readGZIPHeader (:343-433), state for state.  xlen starts at -1 and the two length bytes are OR-ed
// into it (:393), so it stays -1 and the extra field is never skipped (:398): a header with a
// non-empty FEXTRA field leaves that field in front of the deflate data, as the reference does.
int gzip_header(nx_zlib_decoder* d, std::string& err, const uint8_t* in, size_t n, size_t& rd) {
    using Z = nx_zlib_decoder;
    auto skip_if_needed = [&](int32_t mask) {  // skipIfNeeded (:442-458)
        if (d->flags & mask) {
            for (;;) {
                if (rd == n) return false;
                const uint8_t b = in[rd++];
                d->hcrc = crc32_host(d->hcrc, &b, 1);
                if (b == 0) break;
            }
        }
        return true;
    };
    switch (d->gz) {
        case Z::HEADER_START: {
            if (n - rd < 10) return kZNeed;
            const uint8_t* h = in + rd;
            if (h[0] != 31) {
                err = "Input is not in the GZIP format";
                return NX_ERR_FRAME_CORRUPT;
            }
            if (h[2] != 8) {  // Deflater.DEFLATED
                err = "Unsupported compression method " + std::to_string((int)h[2]) + " in the GZIP header";
                return NX_ERR_FRAME_CORRUPT;
            }
            d->flags = h[3];
            if (d->flags & FRESERVED) {
                err = "Reserved flags are set in the GZIP header";
                return NX_ERR_FRAME_CORRUPT;
            }
            d->hcrc = crc32_host(d->hcrc, h, 10);  // magic, method, flags, mtime, extra flags, operating system
            rd += 10;
            d->gz = Z::FLG_READ;
        }  // fall through
        case Z::FLG_READ:
            if (d->flags & FEXTRA) {
                if (n - rd < 2) return kZNeed;
                const int32_t xlen1 = in[rd], xlen2 = in[rd + 1];
                d->hcrc = crc32_host(d->hcrc, in + rd, 2);
                rd += 2;
                d->xlen |= xlen1 << 8 | xlen2;
            }
            d->gz = Z::XLEN_READ;
            // fall through
        case Z::XLEN_READ:
            if (d->xlen != -1) {  // (never: see above)
                if (n - rd < (size_t)d->xlen) return kZNeed;
                d->hcrc = crc32_host(d->hcrc, in + rd, (size_t)d->xlen);
                rd += (size_t)d->xlen;
            }
            d->gz = Z::SKIP_FNAME;
            // fall through
        case Z::SKIP_FNAME:
            if (!skip_if_needed(FNAME)) return kZNeed;
            d->gz = Z::SKIP_COMMENT;
            // fall through
        case Z::SKIP_COMMENT:
            if (!skip_if_needed(FCOMMENT)) return kZNeed;
            d->gz = Z::PROCESS_FHCRC;
            // fall through
        case Z::PROCESS_FHCRC:
            if (d->flags & FHCRC) {  // verifyCrc16 (:506-520)
                if (n - rd < 2) return kZNeed;
                const int32_t want = in[rd] | (in[rd + 1] << 8), got = (int32_t)(d->hcrc & 0xFFFFu);
                rd += 2;
                if (want != got) {
                    err = "CRC16 value mismatch. Expected: " + std::to_string(want) + ", Got: " + std::to_string(got);
                    return NX_ERR_FRAME_CORRUPT;
                }
            }
            d->hcrc = 0;  // crc.reset()
            d->crc = 0;
            d->gz = Z::HEADER_END;
            // fall through
        default:
            return kZOk;
    }
}

// readGZIPFooter (:467-483) with verifyCrc (:492-504): all 8 bytes first, then the two checks with
// Java's formatting (the CRC as unsigned longs, the lengths as ints).
int gzip_footer(nx_zlib_decoder* d, std::string& err, const uint8_t* in, size_t n, size_t& rd) {
    if (n - rd < 8) return kZNeed;
    const uint32_t want_crc = le32(in + rd);
    const int32_t want_len = (int32_t)le32(in + rd + 4), got_len = (int32_t)(uint32_t)d->total_out;
    if (want_crc != d->crc) {
        rd += 4;
        err = "CRC value mismatch. Expected: " + std::to_string((unsigned long long)want_crc) +
                    ", Got: " + std::to_string((unsigned long long)d->crc);
        return NX_ERR_FRAME_CORRUPT;
    }
    rd += 8;
    if (want_len != got_len) {
        err = "Number of bytes mismatch. Expected: " + std::to_string(want_len) + ", Got: " + std::to_string(got_len);
        return NX_ERR_FRAME_CORRUPT;
    }
    return kZOk;
}

// inflater.reset() (:321) and crc.reset(): a new member starts with an empty window and, at its first
// body step, from the all-zero inflate state (st_fresh: whoever runs that step clears the state)
void zlib_reset_member(nx_zlib_decoder* d) {
    d->hist = 0;
    d->crc = 0;
    d->adler = 1;
    d->total_out = 0;
    d->st_fresh = true;
}
}  // namespace

extern "C" nx_zlib_decoder* nx_zlib_decoder_new(int32_t wrapper, int32_t decompress_concatenated, int32_t max_allocation) {
    if (wrapper < 0 || wrapper > 3 || max_allocation < 0) return nullptr;  // checkPositiveOrZero (ZlibDecoder.java:49)
    auto* d = new nx_zlib_decoder();
    if (!d->g.ok || !d->win[0].ensure(kZlibHist + kZlibChunk) || !d->win[1].ensure(kZlibHist + kZlibChunk) ||
        !d->st.ensure(NX_INFLATE_STATE_BYTES) || !d->par.ensure(sizeof(nx::h::ZlibLaunch)) ||
        hipMemsetAsync(d->st.p, 0, NX_INFLATE_STATE_BYTES, d->g.s) != hipSuccess || !d->g.sync()) {
        delete d;
        return nullptr;
    }
    d->max_allocation = max_allocation;
    d->concatenated = decompress_concatenated != 0;
    d->gzip = wrapper == 1;    // :141-159
    d->zlib = wrapper == 0;
    d->decide = wrapper == 3;
    return d;
}
// JdkZlibDecoder(dictionary, maxAllocation) (:96-111): ZlibWrapper.ZLIB, decompressConcatenated false
extern "C" nx_zlib_decoder* nx_zlib_decoder_new_dict(const uint8_t* dict, size_t dict_len, int32_t max_allocation) {
    if (!dict) return nullptr;
    nx_zlib_decoder* d = nx_zlib_decoder_new(0, 0, max_allocation);
    if (!d) return nullptr;
    const size_t tail = dict_len < kZlibDictMax ? dict_len : kZlibDictMax;
    d->has_dict = true;
    d->dictid = adler32_host(dict, dict_len);
    d->dict_n = (uint32_t)tail;
    if (tail && (!d->ddict.ensure(tail) || !d->g.h2d(d->ddict.p, dict + (dict_len - tail), tail) || !d->g.sync())) {
        delete d;
        return nullptr;
    }
    return d;
}
extern "C" void nx_zlib_decoder_free(nx_zlib_decoder* d) { nx_zlib_decoder_unref(d); }
extern "C" int32_t nx_zlib_decoder_is_closed(const nx_zlib_decoder* d) { return d && d->finished ? 1 : 0; }

// ---------------------------------------------------------------- the decoder's state machine
// JdkZlibDecoder.decode (:198-314) as two steps that nx_zlib_decoder_decode below and the batcher's
// decoder jobs (batcher.cpp) both drive: wrapper_step parses wrapper bytes until the deflate body needs
// the device; body_result accounts for one inflate launch of one stream.  What differs between the two
// drivers (where the launch runs, how its bytes reach the host, who copies the carry) is nx::zl::BodyIo.
namespace nx {
namespace zl {

int fail(nx_zlib_decoder* d, Call& c, int32_t code) {  // the exception leaves decode(): what was decoded is forwarded (:304-312)
    d->failed = true;
    c.rd = c.n;
    return code;
}

int wrapper_step(nx_zlib_decoder* d, Call& c) {
    using Z = nx_zlib_decoder;
    const uint8_t* in = c.in;
    const size_t n = c.n;
    size_t& rd = c.rd;
    if (d->finished || d->failed) {  // in.skipBytes(in.readableBytes()) (:200-204)
        rd = n;
        return kStop;
    }
    for (;;) {
        if (rd == n) return kStop;  // :206-209
        if (d->decide) {  // :211-220
            if (n - rd < 2) return kStop;
            const int32_t cmf_flg = (int16_t)be16(in + rd);  // looksLikeZlib on a Java short (:529-532)
            d->zlib = (cmf_flg & 0x7800) == 0x7800 && cmf_flg % 31 == 0;
            d->decide = false;
        }
        if (d->gzip && d->gz != Z::HEADER_END) {  // :222-242
            if (d->gz == Z::FOOTER_START) {
                const int r = gzip_footer(d, c.err, in, n, rd);
                if (r == kZNeed) return kStop;
                if (r < 0) return fail(d, c, r);
                if (!d->concatenated) {  // handleGzipFooter (:316-328); the next decode() skips the rest
                    d->finished = true;
                    rd = n;
                    return kStop;
                }
                zlib_reset_member(d);
                d->gz = Z::HEADER_START;
            }
            const int r = gzip_header(d, c.err, in, n, rd);
            if (r == kZNeed) return kStop;
            if (r < 0) return fail(d, c, r);
            continue;
        }
        if (d->zlib && d->zs != Z::Z_BODY) {  // inflate()'s HEAD / DICTID / CHECK states (zlib inflate.c)
            if (d->zs == Z::Z_HEAD) {
                if (n - rd < 2) return kStop;
                const uint32_t cmf = in[rd], flg = in[rd + 1];
                int32_t code = NX_OK;
                if (((cmf << 8) + flg) % 31) code = NX_ERR_ZLIB_HEADER_CHECK;
                else if ((cmf & 15u) != 8u) code = NX_ERR_ZLIB_METHOD;
                else if ((cmf >> 4) + 8u > 15u) code = NX_ERR_ZLIB_WINDOW;
                if (code == NX_OK && (flg & 0x20u)) {  // FDICT: zlib reads the dictionary id, then asks for it (:276-280)
                    if (n - rd < 6) return kStop;
                    if (!d->has_dict) {
                        c.err = "decompression failure, unable to set dictionary as non was specified";
                        return fail(d, c, NX_ERR_ZLIB_NEED_DICT);
                    }
                    // inflater.setDictionary (:281): zlib's inflateSetDictionary refuses a dictionary whose
                    // Adler32 is not DICTID, and Inflater throws IllegalArgumentException (zlib sets no text;
                    // the message is not pinned by a JVM run)
                    if (be32(in + rd + 2) != d->dictid) {
                        c.err = "java.lang.IllegalArgumentException";
                        return fail(d, c, NX_ERR_ZLIB_DICT_MISMATCH);
                    }
                    // the dictionary's tail is the window's content before the first output byte; the running
                    // Adler32 starts at 1 after it (inflate.c, DICT -> TYPE)
                    if (d->dict_n && (hipMemcpyAsync(d->win[d->cur].as<uint8_t>() + kZlibHist - d->dict_n, d->ddict.p, d->dict_n,
                                                     hipMemcpyDeviceToDevice, d->g.s) != hipSuccess ||
                                      !d->g.sync())) {
                        c.err = "GPU copy failed";
                        return fail(d, c, NX_ERR_HIP);
                    }
                    d->hist = d->dict_n;
                    rd += 6;
                    d->zs = Z::Z_BODY;
                    continue;
                }
                if (code != NX_OK) {
                    c.err = "decompression failure";
                    return fail(d, c, code);
                }
                rd += 2;
                d->zs = Z::Z_BODY;
                continue;
            }
            if (n - rd < 4) return kStop;  // the Adler32 trailer, most significant byte first
            if (be32(in + rd) != d->adler) {
                c.err = "decompression failure";
                return fail(d, c, NX_ERR_ZLIB_DATA_CHECK);
            }
            rd += 4;
            d->finished = true;  // inflater.finished() (:284-286)
            rd = n;
            return kStop;
        }
        return kBody;  // the deflate body: inflate until the input runs out, the stream ends or an error (:257-294)
    }
}

int body_result(nx_zlib_decoder* d, Call& c, uint32_t consumed, uint32_t m, int32_t status, uint32_t sum, BodyIo& io) {
    using Z = nx_zlib_decoder;
    if (status == NX_ERR_INVALID_ARG || status == NX_ERR_INTERNAL) return kHalt + status;
    c.rd += consumed;
    if (m) {
        if (d->max_allocation > 0) {
            if (c.acc.size() + m > (size_t)d->max_allocation) {  // prepareDecompressBuffer (ZlibDecoder.java:74-81)
                c.acc.clear();
                io.drop();
                d->finished = true;  // decompressionBufferExhausted (:331-333)
                c.err = "Decompression buffer has reached maximum size: " + std::to_string(d->max_allocation);
                c.rd = c.n;
                return NX_ERR_ZLIB_MAX_ALLOCATION;
            }
            const size_t at = c.acc.size();
            c.acc.resize(at + m);
            if (!io.take(c.acc.data() + at, m)) return kHalt + NX_ERR_HIP;
        } else if (!io.take(nullptr, m)) {
            return kHalt + NX_ERR_HIP;
        }
        if (d->gzip) d->crc = nx_crc32_combine(d->crc, sum, m);
        else if (d->zlib) d->adler = nx_adler32_combine(d->adler, sum, m);
        d->total_out += m;
        // the last 32 KiB of the stream's output become the other window's history
        const uint32_t h = d->hist + m < kZlibHist ? d->hist + m : kZlibHist;
        if (!io.carry(h, m)) return kHalt + NX_ERR_HIP;
        d->hist = h;
        d->cur ^= 1;
    }
    if (status < 0) {  // DataFormatException -> DecompressionException("decompression failure") (:302-303)
        c.err = "decompression failure";
        return fail(d, c, status);
    }
    if (status == NX_INFLATE_OUTPUT_FULL) return kBody;
    if (status != NX_OK) return kStop;  // the inflater needs input
    if (d->gzip) {
        d->gz = Z::FOOTER_START;  // :298-301
    } else if (d->zlib) {
        d->zs = Z::Z_TRAILER;
    } else {
        d->finished = true;  // :284-286
        c.rd = c.n;
        return kStop;
    }
    return kWrapper;
}

}  // namespace zl
}  // namespace nx

namespace {
// The synchronous driver of those steps: the status of the call, with c.rd, c.err and c.acc left for the frame.
int32_t zlib_sync_steps(nx_zlib_decoder* d, nx::zl::Call& c) {
    namespace zl = nx::zl;
    using nx::h::ZlibLaunch;
    Gpu& g = d->g;
    struct SyncIo : zl::BodyIo {  // the launch's bytes come by a copy of their own; the carry is a device copy
        nx_zlib_decoder* d;
        bool take(uint8_t* dst, uint32_t m) override {
            const uint8_t* W = d->win[d->cur].as<uint8_t>();
            if (!dst) {
                d->ml.owned.emplace_back(m);
                dst = d->ml.owned.back().data();
            }
            return d->g.d2h(dst, W + kZlibHist, m);
        }
        void drop() override { d->ml.owned.clear(); }
        bool carry(uint32_t h, uint32_t m) override {
            const uint8_t* W = d->win[d->cur].as<uint8_t>();
            return hipMemcpyAsync(d->win[d->cur ^ 1].as<uint8_t>() + kZlibHist - h, W + kZlibHist + m - h, h, hipMemcpyDeviceToDevice,
                                  d->g.s) == hipSuccess &&
                   d->g.sync();
        }
    } io;
    io.d = d;
    const ParamBlock<ZlibLaunch> P(g, d->par);
    bool uploaded = false;  // the cumulation is copied to the device once, when a body needs it
    int step = zl::kWrapper;
    for (;;) {
        if (step == zl::kWrapper) step = zl::wrapper_step(d, c);
        if (step != zl::kBody) break;
        if (!uploaded) {
            if (!g.din.ensure(c.n) || !g.h2d(g.din.p, c.in, c.n)) return NX_ERR_HIP;
            uploaded = true;
        }
        if (d->st_fresh) {  // inflater.reset() (:321): a new member starts from the all-zero state
            if (hipMemsetAsync(d->st.p, 0, NX_INFLATE_STATE_BYTES, g.s) != hipSuccess) return NX_ERR_HIP;
            d->st_fresh = false;
        }
        uint8_t* W = d->win[d->cur].as<uint8_t>();
        ZlibLaunch p{};
        p.in_off = c.rd;
        p.in_len = (uint32_t)(c.n - c.rd < 0x7FFFFFFFu ? c.n - c.rd : 0x7FFFFFFFu);
        p.out_off = kZlibHist - d->hist;
        p.hist_len = d->hist;
        p.out_cap = kZlibChunk;
        p.sum_off = kZlibHist;
        if (!P.upload(p, nx::h::field_offset(&ZlibLaunch::consumed))) return NX_ERR_HIP;  // the arguments: up to the first result
        int32_t r = nx_inflate_batch(g.din.as<uint8_t>(), P.field(&ZlibLaunch::in_off), P.field(&ZlibLaunch::in_len), W,
                                     P.field(&ZlibLaunch::out_off), P.field(&ZlibLaunch::hist_len), P.field(&ZlibLaunch::out_cap),
                                     d->st.as<uint8_t>(), P.field(&ZlibLaunch::consumed), P.field(&ZlibLaunch::out_len),
                                     P.field(&ZlibLaunch::status), 1, g.s);
        if (r != NX_OK) return r;
        if (d->gzip || d->zlib) {  // the checksum of what this launch produced (crc.update, :265-267)
            auto sum = d->gzip ? nx_crc32_batch : nx_adler32_batch;
            r = sum(W, P.field(&ZlibLaunch::sum_off), P.field(&ZlibLaunch::out_len), P.field(&ZlibLaunch::sum), 1, g.s);
            if (r != NX_OK) return r;
        }
        if (!P.download(p, &ZlibLaunch::consumed) || !g.sync()) return NX_ERR_HIP;
        step = zl::body_result(d, c, p.consumed, p.out_len, p.status, p.sum, io);
        if (step <= zl::kHalt) return step - zl::kHalt;  // the launch itself failed: the decoder is as it was
    }
    return step < 0 ? step : NX_OK;
}
}  // namespace

extern "C" int32_t nx_zlib_decoder_decode(nx_zlib_decoder* d, const uint8_t* in, size_t n, size_t* consumed, const nx_msg** msgs,
                                          size_t* n_msgs, const char** err_msg) {
    const nx::NoGrowScope no_grow;
    if (d && d->owner.load()) return NX_ERR_INVALID_ARG;  // a batcher decoder stays a batcher decoder
    DecodeCall call(d, in, n, consumed, msgs, n_msgs, err_msg);
    if (call.refused()) return NX_ERR_INVALID_ARG;
    nx::zl::Call c;
    c.in = in;
    c.n = n;
    const int32_t r = zlib_sync_steps(d, c);
    // the call's messages: each launch's bytes, or with maxAllocation the one accumulated buffer
    MsgList& ml = call.ml();
    ml.err = c.err;
    if (!c.acc.empty()) ml.owned.push_back(std::move(c.acc));
    for (auto& o : ml.owned) ml.msgs.push_back({o.data(), o.size()});
    call.rd = c.rd;
    return call.finish(r);
}

// ------------------------------------------------------------------ Bzip2Decoder
// Bzip2Decoder.java:93-343 over the split decode (bzip2_decode_split.hip).  The four header bytes are parsed
// here; everything behind them is one item of decode_split_launch whose chain starts at the carried bit
// position with the carried stream CRC.  Where the handle departs from the reference is said at its
// declaration in netty_amd.h.
extern "C" nx_bzip2_decoder* nx_bzip2_decoder_new(void) { return make_handle<nx_bzip2_decoder>(nx::WsKind::Bzip2Dec); }
extern "C" void nx_bzip2_decoder_free(nx_bzip2_decoder* d) { delete d; }
extern "C" int32_t nx_bzip2_decoder_is_closed(const nx_bzip2_decoder* d) { return d && d->closed ? 1 : 0; }
extern "C" int32_t nx_bzip2_decoder_stats(const nx_bzip2_decoder* d, uint64_t* launches, uint64_t* blocks_attempted,
                                          uint64_t* blocks_emitted) {
    if (!d || !launches || !blocks_attempted || !blocks_emitted) return NX_ERR_INVALID_ARG;
    *launches = d->launches;
    *blocks_attempted = d->attempted;
    *blocks_emitted = d->emitted;
    return NX_OK;
}

namespace {
// the first failing block: the decoder swallows what follows, the exception's text is the status's
int32_t bzip2_corrupt(nx_bzip2_decoder* d, DecodeCall& call, int32_t st) {
    d->corrupted = true;
    return call.fail(st, nx_status_string(st), call.n);
}
// where, in the lists' memory, the part that is copied back begins
size_t split_lists_back_offset(const nx::bz2d::SplitLists& S) {
    return (size_t)(reinterpret_cast<const uint8_t*>(S.first) - static_cast<const uint8_t*>(S.mem));
}
}  // namespace

extern "C" int32_t nx_bzip2_decoder_decode(nx_bzip2_decoder* d, const uint8_t* in, size_t n, size_t* consumed, const nx_msg** msgs,
                                           size_t* n_msgs, const char** err_msg) {
    using namespace nx::bz2d;
    using nx::h::Bzip2Geom;
    using nx::h::Bzip2Result;
    using nx::h::Bzip2Scan;
    const nx::NoGrowScope no_grow;
    DecodeCall call(d, in, n, consumed, msgs, n_msgs, err_msg);
    if (call.refused()) return NX_ERR_INVALID_ARG;
    // :328-330 in.skipBytes(in.readableBytes()); after an error: this handle's own state
    if (d->closed || d->corrupted) return call.skip_all();
    MsgList& ml = call.ml();
    size_t& pos = call.rd;
    if (!d->have_header) {  // :101-119
        if (n < 4) return call.finish(NX_OK);
        uint32_t level = 0;
        const int32_t st = stream_header(in, 4, &level);
        if (st != NX_OK) return bzip2_corrupt(d, call, st);
        d->have_header = true;
        d->level = level;
        d->crc = 0;
        d->bit_used = 0;
        d->seen_after = 0;
        pos = 4;
    }
    constexpr size_t kMaxCumulation = 0x7fffffffu;
    const size_t rem = n - pos < kMaxCumulation ? n - pos : kMaxCumulation;
    if (8ull * rem < d->bit_used + 80ull) return call.finish(NX_OK);  // not even a magic and a CRC
    Gpu& g = d->g;
    // the scan, and its list back: what stands in the received bytes decides whether anything is attempted
    const uint32_t scan_cap = (uint32_t)(rem / 6 + 2);
    const ParamBlock<Bzip2Geom> G(g, g.in_off);
    const ParamBlock<Bzip2Scan> S0(g, g.status);
    if (!g.din.ensure(rem + 16) || !g.aux1.ensure(8ull * scan_cap + 64) || !G.ensure() || !S0.ensure()) return call.finish(NX_ERR_HIP);
    Bzip2Geom geom = {0, 0, (uint32_t)rem, 0, {d->bit_used, d->crc, d->level, d->seen_after, 0}};
    if (!g.h2d(g.din.p, in + pos, rem) || !G.upload(geom)) return call.finish(NX_ERR_HIP);
    int32_t r = nx_bzip2_scan_batch(g.din.as<uint8_t>(), G.field(&Bzip2Geom::in_off), G.field(&Bzip2Geom::in_len), 1, scan_cap,
                                    g.aux1.as<uint64_t>(), S0.field(&Bzip2Scan::first), S0.field(&Bzip2Scan::count),
                                    S0.field(&Bzip2Scan::status), g.s);
    if (r != NX_OK) return call.finish(r);
    Bzip2Scan scan = {0, 0, 0};
    if (!S0.download(scan, &Bzip2Scan::first) || !g.sync()) return call.finish(NX_ERR_HIP);
    if (scan.status != NX_OK) return call.finish(NX_ERR_INTERNAL);  // (six bytes a magic: scan_cap always suffices for distinct magics)
    const uint32_t count = scan.count;
    std::vector<uint64_t> cand(count);
    if (count && (!g.d2h(cand.data(), g.aux1.p, 8ull * count) || !g.sync())) return call.finish(NX_ERR_HIP);
    uint32_t head = 0;
    while (head < count && (cand[head] & kCandPos) < d->bit_used) head += 1;
    const bool at_head = head < count && (cand[head] & kCandPos) == d->bit_used;
    if (!at_head) {
        // neither magic where the next block must stand: "bad block header" once its 48 bits are all there
        // (the reference looks after ten bytes, :122-140)
        return bzip2_corrupt(d, call, NX_ERR_BZIP2_BLOCK_HEADER);
    }
    if (!(cand[head] & kCandEnd) && count - 1u - head <= d->seen_after) return call.finish(NX_OK);  // the block is still arriving
    // one decode sequence over the chain head and every candidate; the output slot grows if the blocks need it
    uint64_t cap = (uint64_t)count * d->level * kBaseBlock + 65536;
    SplitLists S;
    const size_t lists_bytes = split_lists_layout(S, nullptr, 1, count, true);
    const ParamBlock<Bzip2Result> R(g, g.out_len);
    if (!g.aux0.ensure(lists_bytes) || !R.ensure()) return call.finish(NX_ERR_HIP);
    split_lists_layout(S, g.aux0.p, 1, count, true);
    const size_t back_off = split_lists_back_offset(S);  // what comes back starts at the items' `first` words
    const size_t back_bytes = lists_bytes - back_off;
    SplitLists H;  // the same layout over the host copy
    const SplitItem* I = nullptr;
    for (int attempt = 0;; ++attempt) {
        if (cap > 0xffffffffull) cap = 0xffffffffull;
        geom.out_cap = (uint32_t)cap;
        if (!g.dout.ensure(cap) || !G.upload(geom)) return call.finish(NX_ERR_HIP);
        r = decode_split_launch(g.din.as<uint8_t>(), G.field(&Bzip2Geom::in_off), G.field(&Bzip2Geom::in_len), g.dout.as<uint8_t>(),
                                G.field(&Bzip2Geom::out_off), G.field(&Bzip2Geom::out_cap), R.field(&Bzip2Result::out_len),
                                R.field(&Bzip2Result::consumed), R.field(&Bzip2Result::status), 1, count, R.field(&Bzip2Result::blocks),
                                G.field(&Bzip2Geom::start), g.aux0.p, g.s);
        if (r != NX_OK) return call.finish(r);
        d->lists.resize(lists_bytes);
        if (!g.d2h(d->lists.data() + back_off, g.aux0.as<uint8_t>() + back_off, back_bytes) || !g.sync()) return call.finish(NX_ERR_HIP);
        d->launches += 1;
        split_lists_layout(H, d->lists.data(), 1, count, true);
        I = H.items;
        if (I->status != NX_ERR_BZIP2_OUTPUT_FULL || cap == 0xffffffffull || attempt == 8) break;
        // the block at the cursor did not fit: room for it and a declared size for each behind it, at least twice the slot
        const uint64_t need = (uint64_t)I->off + H.res[I->cursor].final_len + (uint64_t)(count - I->cursor) * d->level * kBaseBlock;
        cap = need > 2 * cap ? need : 2 * cap;
    }
    // the members in chain order: a message each (:306-318) up to the first whose final stage failed
    int32_t bad = NX_OK;
    uint32_t members = 0, crc = d->crc;
    uint64_t total = 0, next_bit = d->bit_used;
    struct Piece {
        uint32_t off, len;
    };
    std::vector<Piece> pieces;
    for (uint32_t k = 0; k < I->cursor && k < count; ++k) {
        const CandResult& c = H.res[k];
        if (!c.member) continue;
        members += 1;
        if (c.back_status != NX_OK) {
            bad = c.back_status;
            break;
        }
        pieces.push_back({c.off, c.final_len});
        total = (uint64_t)c.off + c.final_len;
        crc = crc_combine_stream(crc, c.crc);
        next_bit = c.end_bit;
    }
    const bool front_answer = bad == NX_OK && I->status != NX_OK && I->status != NX_ERR_BZIP2_STREAM_CRC && I->status != NX_ERR_BZIP2_OUTPUT_FULL &&
                              I->status != NX_ERR_BZIP2_BLOCK_HEADER && (I->status != NX_ERR_BZIP2_TRUNCATED || I->tail_attempted);
    d->attempted += members + (front_answer ? 1u : 0u);
    d->emitted += pieces.size();
    d->back.resize(total);
    if (total && (!g.d2h(d->back.data(), g.dout.p, total) || !g.sync())) return call.finish(NX_ERR_HIP);
    for (const Piece& p : pieces) ml.msgs.push_back({d->back.data() + p.off, p.len});
    if (bad != NX_OK) return bzip2_corrupt(d, call, bad);
    if (I->status == NX_OK) {  // the end marker, stream CRC checked: EOF (:126-135); what follows is skipped
        d->closed = true;
        return call.skip_all();
    }
    if (I->status != NX_ERR_BZIP2_TRUNCATED) return bzip2_corrupt(d, call, I->status);
    // wait, as the reference waits: stop at the byte that holds the waiting block's first bit
    if (I->tail_attempted) d->seen_after = count - 1u - I->cursor;
    else if (!pieces.empty()) d->seen_after = 0;
    d->crc = crc;
    d->bit_used = (uint32_t)(next_bit & 7u);
    pos += (size_t)(next_bit >> 3);
    return call.finish(NX_OK);
}
