// kcemu — the LDS-table kernels of compress_amd/csrc compiled for the hipemu CPU emulator, behind a small C API for the
// tests (tests/test_emu_lds.py).  TEST INFRASTRUCTURE: the product (libkcgpu.so) never contains or loads this.
#include <hip/hip_runtime.h>
#include "../../compress_amd/csrc/kc_s2_lds.hip"
#include "../../compress_amd/csrc/kc_s2.hip"
#include "../../compress_amd/csrc/kc_zstd_match_lds.hip"
#include "../../compress_amd/csrc/kc_zstd_match.hip"
#include "../../compress_amd/csrc/kc_misc.hip"
#include "../../compress_amd/csrc/kc_zstd_entropy.hip"
#include "../../compress_amd/csrc/kc_zstd_prescan.hip"
#include "../../compress_amd/csrc/kc_zstd_first.hip"
#include "../../compress_amd/csrc/kc_zstd_prime.hip"
#include "../../compress_amd/csrc/kc_zstd_match_dfast.hip"
#include "../../compress_amd/csrc/kc_zstd_match_better.hip"
#include <vector>
#include "../../compress_amd/csrc/kc_s2_best.hip"
#include "../../compress_amd/csrc/kc_zstd_match_best.hip"
#include "../../compress_amd/csrc/kc_zstd_decode.hip"
#include "../../compress_amd/csrc/kc_zstd_plan.hip"
#include "../../compress_amd/csrc/kc_zstd_decode_all.hip"
#include "../../compress_amd/csrc/kc_dict.cpp"       // (host code: the dictionary loader the decoder options use)
#include "../../compress_amd/csrc/kc_zstd_dstream.hip"
#include "../../compress_amd/csrc/kc_zdstream_host.h"
#include "../../compress_amd/csrc/kc_s2_plan.hip"
#include "../../compress_amd/csrc/kc_s2_decode_all.hip"
#include "../../compress_amd/csrc/kc_s2_ranges.hip"
#include "../../compress_amd/csrc/kc_s2_index.cpp"   // (host code: s2.Index, exported from this library as from the product)
#include "../../compress_amd/csrc/kc_s2_rstream.hip"
#include "../../compress_amd/csrc/kc_s2rstream_host.h"
#include "../../compress_amd/csrc/kc_flate_inflate.hip"
#include "../../compress_amd/csrc/kc_flate_deflate.hip"
#include "../../compress_amd/csrc/kc_flate_stateless.hip"
#include "../../compress_amd/csrc/kc_zip.hip"
#include "../../compress_amd/csrc/kc_zip_dir.cpp"    // (host code: zip.NewReader's directory pass, exported from this library as from the product)

#include "../../compress_amd/csrc/kc_s2dec_host.h"
#include "../../compress_amd/csrc/kc_s2ranges_host.h"
#include "../../compress_amd/csrc/kc_flate_host.h"
#include "../../compress_amd/csrc/kc_deflate_host.h"
#include "../../compress_amd/csrc/kc_stateless_host.h"
#include "../../compress_amd/csrc/kc_zip_host.h"
#include "../../compress_amd/csrc/kc_zstd_opts.cpp"  // (host code: the encoder's option functions)
#include "../../compress_amd/csrc/kc_zenc_host.h"    // (host code: the rules of the zstd encode batch)

// The decoders' device (kc_decdev_host.h) over plain memory: every buffer a heap block of exactly the size asked for (a write outside
// it is one outside a heap block), filled with 0xA7 when it is made; copies are memcpy; the kernels run on the emulator.
static uint64_t g_budget = 0;   // kcemu_set_scratch_budget: what the batch decoders may ask for (0: anything)
static KcDecTimes g_last;       // what the last batch decoder's sequence reported
static int g_first_opt = 1;     // kcemu_set_first_filter: KC_OPT_ZFAST_FIRST_FILTER as kcemu_zstd_batch sees it (the library's default: on)
static int g_first_used = 0;    // the last kcemu_zstd_batch gave its match finder first-occurrence bits
struct KcemuDevice : KcDecDevice {
    std::vector<void*> buf;
    std::vector<size_t> cap;
    int reserve(int which, size_t bytes, void** p) override {
        if ((size_t)which >= buf.size()) { buf.resize(which + 1, nullptr); cap.resize(which + 1, 0); }
        if (cap[which] < bytes || !buf[which]) {
            free(buf[which]);
            buf[which] = malloc(bytes ? bytes : 1);
            cap[which] = bytes;
            if (buf[which]) memset(buf[which], 0xA7, bytes);
        }
        *p = buf[which];
        return buf[which] ? 0 : -6;
    }
    int h2d(void* d, const void* h, size_t n) override { if (n) memcpy(d, h, n); return 0; }
    int d2h(void* h, const void* d, size_t n) override { if (n) memcpy(h, d, n); return 0; }
    int d2d(void* d, const void* s, size_t n) override { if (n) memcpy(d, s, n); return 0; }
    int zero(void* d, size_t n) override { if (n) memset(d, 0, n); return 0; }
    int sync() override { return 0; }
    uint64_t budget() override { return g_budget ? g_budget : UINT64_MAX; }
    void lane_group(int lanes) override { hipemu::set_group(lanes); }
    ~KcemuDevice() override { for (void* b : buf) free(b); }
};
struct KcemuZsStream {
    KcemuDevice dev;
    KcZsStream s;
};
struct KcemuS2rStream {
    KcemuDevice dev;
    KcS2rStream s;
};

// n_dicts dictionaries back to back (dict_off: n_dicts + 1 offsets) into the decoder's options: full-format ones, or raw ones
// (WithDecoderDictRaw) as "KCRD", id, content.  False on a dictionary the loader refuses.
static bool kcemu_load_dicts(KcZdOpts& o, const uint8_t* dict_blobs, const uint64_t* dict_off, uint32_t n_dicts) {
    for (uint32_t k = 0; k < n_dicts; k++) {
        const uint8_t* blob = dict_blobs + dict_off[k];
        const uint64_t blen = dict_off[k + 1] - dict_off[k];
        if (blen >= 8 && memcmp(blob, "KCRD", 4) == 0) {
            uint32_t id;
            memcpy(&id, blob + 4, 4);
            if (kc_zd_add_dict_raw(o, id, blob + 8, blen - 8) != 0) return false;
            continue;
        }
        KcZdDict D;
        const uint8_t* content = nullptr;
        uint64_t clen = 0;
        if (kc_dict_load_decoder(blob, blen, &D, &content, &clen) != 0 || kc_zd_add_dict(o, D, content, clen) != 0) return false;
    }
    return true;
}

// s2.Reader / s2.Decode over n inputs: kc_s2dec_host.h's sequence over plain memory.  bound: the planned layout's sizes.
static int kcemu_s2_decode(const KcS2dMode& m, const uint8_t* src, const uint64_t* in_off, uint32_t n, uint8_t* dst, uint64_t dst_cap, uint64_t* out_off,
                           uint64_t* bound, uint32_t* status) {
    KcemuDevice dev;
    g_last = KcDecTimes();
    const int rc = kc_s2d_decode(&dev, m, src, in_off, n, dst, dst_cap, out_off, status, g_last);
    if (rc == 0 || rc == KC_ERR_DST_TOO_SMALL)
        for (uint32_t i = 0; i < n; i++) bound[i] = out_off[i + 1] - out_off[i];
    return rc;
}

// flate.NewReader / gzip.NewReader over n inputs: kc_flate_host.h's sequence over plain memory.  dst null: the sizing pass alone.
static int kcemu_flate(const KcFlOpts& o, const uint8_t* src, const uint64_t* in_off, uint32_t n, uint8_t* dst, uint64_t dst_cap, uint64_t* out_off,
                       uint64_t* bound, uint32_t* status, uint64_t* consumed) {
    KcemuDevice dev;
    g_last = KcDecTimes();
    if (!dst) return kc_fl_inflate(&dev, o, src, in_off, n, nullptr, 0, nullptr, status, consumed, bound, g_last);
    const int rc = kc_fl_inflate(&dev, o, src, in_off, n, dst, dst_cap, out_off, status, consumed, nullptr, g_last);
    if (rc == 0 || rc == KC_ERR_DST_TOO_SMALL)
        for (uint32_t i = 0; i < n; i++) bound[i] = out_off[i + 1] - out_off[i];
    return rc;
}

extern "C" {

// The scratch budget of the batch decoders' sequences in bytes (KC_OPT_MAX_SCRATCH_MIB's part on the device); 0: unlimited.
void kcemu_set_scratch_budget(uint64_t bytes) { g_budget = bytes; }
// What the last batch decoder call reported: the device batches it was cut into, and the largest single input's scratch with its
// 1/8 allowance (the least budget under which no input is refused for size).
int kcemu_last_batches() { return g_last.batches; }
uint64_t kcemu_last_max_need() { return g_last.max_need; }

// zstd.Decoder.DecodeAll over n inputs: kc_zdec_host.h's sequence over plain memory.  dict_blobs: as kcemu_load_dicts takes them, all
// registered at once.  Returns 0, -2 when dst_cap is too small, -1 on a dictionary the loader refuses.
int kcemu_zstd_decode_all(const uint8_t* src, const uint64_t* in_off, uint32_t n, uint64_t max_memory, uint64_t max_window, int ignore_checksum,
                          const uint8_t* dict_blobs, const uint64_t* dict_off, uint32_t n_dicts, uint8_t* dst, uint64_t dst_cap, uint64_t* out_off,
                          uint32_t* status) {
    KcZdOpts o;
    o.max_memory = max_memory; o.max_window = max_window; o.ignore_checksum = ignore_checksum;
    if (!kcemu_load_dicts(o, dict_blobs, dict_off, n_dicts)) return -1;
    KcemuDevice dev;
    g_last = KcDecTimes();
    return kc_zd_decode_all(&dev, o, src, in_off, n, dst, dst_cap, out_off, status, g_last);
}

// The verifier over n units on the emulator, one frame each and every frame's decoded length given (dst_off): the decode kernel, XXH64 of
// the decoded ranges and the checksum verdict — kc_zstd_decode_units_dict_dev's sequence (kc_s2_api.cpp) in plain memory.  dict: a raw
// dictionary's content in front of every frame, or null.  The literal scratch is a heap block of exactly the size the library gives it.
int kcemu_zstd_decode_units(const uint8_t* enc, const uint64_t* enc_off, uint32_t n, uint8_t* dst, const uint64_t* dst_off, const uint8_t* dict,
                            uint64_t dict_len, uint32_t* status) {
    if (n == 0) return 0;
    std::vector<uint8_t> lits((size_t)n * KC_ZD_LIT_STRIDE, 0xA7);
    std::vector<uint32_t> stored(n, 0), has(n, 0);
    std::vector<uint64_t> hash(n, 0);
    KcZstdDecParams P;
    memset(&P, 0, sizeof(P));
    P.enc = enc; P.enc_off = enc_off; P.dst = dst; P.dst_off = dst_off; P.lits = lits.data(); P.lit_stride = KC_ZD_LIT_STRIDE;
    P.status = status; P.crc_stored = stored.data(); P.has_crc = has.data(); P.n_units = n;
    P.dict = dict_len ? dict : nullptr; P.dict_len = (uint32_t)dict_len;
    kc_launch_zstd_decode(P, nullptr);
    hipemu::set_group(4);
    kc_launch_xxh64(dst, dst_off, n, hash.data(), nullptr);
    hipemu::set_group(64);
    for (uint32_t i = 0; i < n; i++)
        if (status[i] == 0 && has[i] && (uint32_t)hash[i] != stored[i]) status[i] = 30;  // checksum mismatch
    return 0;
}

// zstd.NewReader(r) on the emulator: kc_zstd_dstream_new / _feed / _free of include/kcgpu.h without the context — the state machine of
// kc_zdstream_host.h over KcemuDevice.  blocks: blocks per launch (KC_OPT_DSTREAM_BLOCKS); the dictionaries as kcemu_zstd_decode_all
// takes them.  Returns null on a dictionary the loader refuses.
void* kcemu_zstd_dstream_new(uint64_t max_memory, uint64_t max_window, int ignore_checksum, uint32_t blocks, const uint8_t* dict_blobs,
                             const uint64_t* dict_off, uint32_t n_dicts) {
    KcemuZsStream* z = new KcemuZsStream();
    z->s.dev = &z->dev;
    z->s.o.max_memory = max_memory; z->s.o.max_window = max_window; z->s.o.ignore_checksum = ignore_checksum; z->s.o.blocks = blocks;
    if (!kcemu_load_dicts(z->s.o, dict_blobs, dict_off, n_dicts)) { delete z; return nullptr; }
    return z;
}
int kcemu_zstd_dstream_feed(void* h, const uint8_t* src, uint64_t n, int eof, uint8_t* dst, uint64_t dst_cap, uint64_t* consumed, uint64_t* produced,
                            uint32_t* status) {
    return ((KcemuZsStream*)h)->s.feed(src, n, eof, dst, dst_cap, consumed, produced, status);
}
int kcemu_zstd_dstream_reset(void* h) { ((KcemuZsStream*)h)->s.reset(); return 0; }
void kcemu_zstd_dstream_free(void* h) { delete (KcemuZsStream*)h; }

// s2.NewReader(r).Read / Skip on the emulator: kc_s2_rstream_new / _feed / _skip / _skip_left / _on_skippable / _reset / _free of
// include/kcgpu.h without the context — the state machine of kc_s2rstream_host.h over KcemuDevice.  chunks: data chunks per launch
// (KC_OPT_S2_RSTREAM_CHUNKS); max_buf: MaxEncodedLen(max_block) + 4.
void* kcemu_s2_rstream_new(uint32_t max_block, uint32_t max_buf, int ignore_crc, int ignore_id, uint32_t chunks) {
    if (chunks < 1 || chunks > 4096) return nullptr;
    KcemuS2rStream* z = new KcemuS2rStream();
    z->s.dev = &z->dev;
    z->s.o.max_block = max_block; z->s.o.max_buf = max_buf; z->s.o.ignore_crc = ignore_crc; z->s.o.ignore_id = ignore_id; z->s.o.chunks = chunks;
    z->s.start();
    return z;
}
int kcemu_s2_rstream_feed(void* h, const uint8_t* src, uint64_t n, int eof, uint8_t* dst, uint64_t dst_cap, uint64_t* consumed, uint64_t* produced,
                          uint32_t* status) {
    return ((KcemuS2rStream*)h)->s.feed(src, n, eof, dst, dst_cap, consumed, produced, status);
}
int kcemu_s2_rstream_skip(void* h, uint64_t n) { ((KcemuS2rStream*)h)->s.skip_left += n; return 0; }
uint64_t kcemu_s2_rstream_skip_left(void* h) { return ((KcemuS2rStream*)h)->s.skip_left; }
int kcemu_s2_rstream_on_skippable(void* h, uint8_t id, kc_s2_skippable_fn fn, void* user) { return ((KcemuS2rStream*)h)->s.on_skippable(id, fn, user); }
int kcemu_s2_rstream_reset(void* h) { ((KcemuS2rStream*)h)->s.reset(); return 0; }
void kcemu_s2_rstream_free(void* h) { delete (KcemuS2rStream*)h; }

int kcemu_s2_decode_streams(const uint8_t* src, const uint64_t* in_off, uint32_t n, uint32_t max_block, uint32_t max_buf, int ignore_crc, int ignore_id,
                            uint8_t* dst, uint64_t dst_cap, uint64_t* out_off, uint64_t* bound, uint32_t* status) {
    KcS2dMode m;
    m.max_block = max_block; m.max_buf = max_buf; m.ignore_crc = ignore_crc; m.ignore_id = ignore_id;
    return kcemu_s2_decode(m, src, in_off, n, dst, dst_cap, out_off, bound, status);
}

// N x io.ReadAll(flate.NewReaderDict(input, dict)); dst null: the sizing pass alone
int kcemu_flate_inflate(const uint8_t* src, const uint64_t* in_off, uint32_t n, const uint8_t* dict, uint32_t dict_len, uint8_t* dst, uint64_t dst_cap,
                        uint64_t* out_off, uint64_t* bound, uint32_t* status, uint64_t* consumed) {
    KcFlOpts o;
    if (dict_len > 32768) { dict += dict_len - 32768; dict_len = 32768; }
    o.dict = dict; o.dict_len = dict_len;
    return kcemu_flate(o, src, in_off, n, dst, dst_cap, out_off, bound, status, consumed);
}
// N x io.ReadAll(gzip.NewReader(input)) under Multistream(multistream)
int kcemu_gzip_inflate(const uint8_t* src, const uint64_t* in_off, uint32_t n, int multistream, uint8_t* dst, uint64_t dst_cap, uint64_t* out_off,
                       uint64_t* bound, uint32_t* status, uint64_t* consumed) {
    KcFlOpts o;
    o.format = KCFL_FMT_GZIP; o.multistream = multistream;
    return kcemu_flate(o, src, in_off, n, dst, dst_cap, out_off, bound, status, consumed);
}
// N x io.ReadAll(zlib.NewReaderDict(input, dict)): the id from the whole dictionary, the window's tail to the device
int kcemu_zlib_inflate(const uint8_t* src, const uint64_t* in_off, uint32_t n, const uint8_t* dict, uint32_t dict_len, uint8_t* dst, uint64_t dst_cap,
                       uint64_t* out_off, uint64_t* bound, uint32_t* status, uint64_t* consumed) {
    KcFlOpts o;
    o.format = KCFL_FMT_ZLIB;
    o.dict_id = kc_fl_adler32(dict, dict_len);
    if (dict_len > 32768) { dict += dict_len - 32768; dict_len = 32768; }
    o.dict = dict; o.dict_len = dict_len;
    return kcemu_flate(o, src, in_off, n, dst, dst_cap, out_off, bound, status, consumed);
}

// n x (f.Open(); io.ReadAll; Close) over the members of one source buffer: kc_zip_host.h's sequence over plain memory.  dst null:
// the layout and the verdicts that need no decoding.  Returns 0, -2 when dst_cap is too small (out_off holds the layout, nothing is written).
int kcemu_zip_read(const uint8_t* src, uint64_t src_len, const kc_zip_member* members, uint32_t n, uint8_t* dst, uint64_t dst_cap, uint64_t* out_off,
                   uint32_t* status) {
    KcemuDevice dev;
    g_last = KcDecTimes();
    return kc_zp_read(&dev, src, src_len, members, n, dst, dst_cap, out_off, status, dst == nullptr, g_last);
}

// N x (flate.NewWriter(w, HuffmanOnly); Write(input); Close() -- or Flush() with end = 1): kc_deflate_host.h's sequence over plain
// memory, at the block size and penalty given (compressor.init's 32768 and 10).  Returns 0, -2 when dst_cap is below the exact total
// (out_off holds the layout, nothing is written), -4 for an input whose records exceed the scratch budget.
static int kcemu_deflate(uint32_t gzip, const uint8_t* src, const uint64_t* in_off, uint32_t n, int end, uint32_t block, uint32_t penalty, uint8_t* dst,
                         uint64_t dst_cap, uint64_t* out_off) {
    KcDfOpts o;
    o.gzip = gzip; o.end = end ? KCDF_END_FLUSH : KCDF_END_CLOSE; o.block = block; o.penalty = penalty;
    KcemuDevice dev;
    g_last = KcDecTimes();
    return kc_df_deflate(&dev, o, src, in_off, n, dst, dst_cap, out_off, g_last);
}
int kcemu_flate_deflate(const uint8_t* src, const uint64_t* in_off, uint32_t n, int end, uint32_t block, uint32_t penalty, uint8_t* dst, uint64_t dst_cap,
                        uint64_t* out_off) {
    return kcemu_deflate(0, src, in_off, n, end, block, penalty, dst, dst_cap, out_off);
}
// N x (gzip.NewWriterLevel(w, HuffmanOnly); Write(input); Close() -- or Flush())
int kcemu_gzip_deflate(const uint8_t* src, const uint64_t* in_off, uint32_t n, int end, uint32_t block, uint32_t penalty, uint8_t* dst, uint64_t dst_cap,
                       uint64_t* out_off) {
    return kcemu_deflate(1, src, in_off, n, end, block, penalty, dst, dst_cap, out_off);
}
uint64_t kcemu_flate_deflate_bound(uint64_t len, uint32_t block) { return kc_df_bound(len, block); }

// N x flate.StatelessDeflate(out, input, eof, dict) -- or, with gzip, N x (gzip.NewWriterLevel(w, StatelessCompression); Write(input);
// Close()): kc_stateless_host.h's sequence over plain memory.  counts: KCSL_N_COUNTS decision counters of the call.  Returns 0, -2
// when dst_cap is below the exact total (out_off holds the layout, nothing is written), -4 for an input beyond the scratch budget.
int kcemu_flate_stateless(uint32_t gzip, const uint8_t* src, const uint64_t* in_off, uint32_t n, int eof, const uint8_t* dict, uint64_t dict_len,
                          uint8_t* dst, uint64_t dst_cap, uint64_t* out_off, uint32_t* counts) {
    KcSlOpts o;
    o.gzip = gzip; o.eof = eof ? 1u : 0u;
    if (dict_len > KCSL_MAX_DICT) { dict += dict_len - KCSL_MAX_DICT; dict_len = KCSL_MAX_DICT; }
    if (dict_len && !gzip) o.dict.assign(dict, dict + dict_len);
    KcemuDevice dev;
    g_last = KcDecTimes();
    return kc_sl_deflate(&dev, o, src, in_off, n, dst, dst_cap, out_off, g_last, counts);
}
uint64_t kcemu_flate_stateless_bound(uint64_t len, uint64_t dict_len) { return kc_sl_bound(len, dict_len); }

// s2.ReadSeeker.ReadAt over m requests: kc_s2ranges_host.h's layout, Index.Find and sequence over plain memory.  Returns 0, -2 when
// dst_cap is too small (nothing written), -1 for a request that names no input or wraps.
int kcemu_s2_read_ranges(const uint8_t* src, const uint64_t* in_off, uint32_t n_streams, const kc_s2_index* const* index, const uint32_t* req_stream,
                         const uint64_t* req_off, const uint64_t* req_len, uint32_t m, uint32_t max_block, uint32_t max_buf, int ignore_crc, int ignore_id,
                         uint8_t* dst, uint64_t dst_cap, uint64_t* out_off, uint64_t* got, uint32_t* status) {
    std::vector<KcS2Req> R;
    std::vector<uint32_t> pre;
    const char* why = "";
    const int rc = kc_s2r_resolve(in_off, n_streams, index, req_stream, req_off, req_len, m, dst_cap, out_off, R, pre, &why);
    g_last = KcDecTimes();
    if (rc != 0 || m == 0) return rc;
    KcS2dMode o;
    o.max_block = max_block; o.max_buf = max_buf; o.ignore_crc = ignore_crc; o.ignore_id = ignore_id;
    KcemuDevice dev;
    return kc_s2r_read(&dev, o, src, R, pre, dst, out_off, got, status, g_last);
}

int kcemu_s2_decode_blocks_all(const uint8_t* src, const uint64_t* in_off, uint32_t n, uint8_t* dst, uint64_t dst_cap, uint64_t* out_off, uint64_t* bound,
                               uint32_t* status) {
    KcS2dMode m;
    m.blocks = 1;
    return kcemu_s2_decode(m, src, in_off, n, dst, dst_cap, out_off, bound, status);
}

// kc_zstd_prime_kernel: n table slots (zeroed by the caller) primed from the first unit_hist[u] bytes of their units; reverse = the
// emulator keeps the LOWEST lane's value where lanes of one store instruction share an address (the hardware may keep any)
int kcemu_zstd_prime(int level, int pos_bits, int reverse, const uint8_t* src, const uint64_t* unit_off, const uint32_t* unit_hist,
                     const uint32_t* unit_list, uint32_t n_launch, uint8_t* tables, uint64_t table_bytes) {
    KcPrimeParams P;
    memset(&P, 0, sizeof(P));
    P.src = src; P.unit_off = unit_off; P.unit_hist = unit_hist; P.unit_list = unit_list; P.unit_base = 0; P.n_launch = n_launch;
    P.level = level; P.pos_bits = pos_bits; P.tables = tables; P.table_bytes = (size_t)table_bytes;
    hipemu::set_reverse(reverse != 0);
    kc_launch_zstd_prime(P, nullptr);
    hipemu::set_reverse(false);
    return 0;
}

// N blocks through kc_s2_encode_lds_kernel; stage slots as the host library lays them out (stage_off, 64-byte aligned)
int kcemu_s2_encode(int level, int framed, int spec_w0, const uint8_t* src, const uint64_t* blk_off, uint32_t n, uint8_t* stage,
                    const uint64_t* stage_off, uint32_t* out_size) {
    KcS2Params P;
    memset(&P, 0, sizeof(P));
    P.src = src;
    P.blk_off = blk_off;
    P.stage_off = stage_off;
    P.stage = stage;
    P.out_size = out_size;
    P.n_blocks = n;
    P.level = level & 0xFF;
    P.variant = (level >> 8) & 0xFF;  // (bits 8..15: KC_S2_VARIANT_*)
    P.stored_only = (level >> 16) & 1; // (bit 16: s2.WriterUncompressed)
    P.spec_w0 = spec_w0;
    P.framed = framed;
    bool small = false, big = false;
    for (uint32_t i = 0; i < n; i++) ((blk_off[i + 1] - blk_off[i]) <= 65536 ? small : big) = true;
    kc_launch_s2_encode_lds(P, small, big, nullptr);
    return 0;
}

// N blocks through kc_s2_encode_kernel<LEVEL> (the HBM-table throughput kernel, 8 lanes per block: s2.Encode / EncodeBetter / EncodeSnappy /
// EncodeSnappyBetter; level bits 8+: KC_S2_VARIANT_*), tables as the host sizes and zeroes them
int kcemu_s2_hbm(int level, int framed, int w0, int w0b, int grow, const uint8_t* src, const uint64_t* blk_off, uint32_t n, uint8_t* stage,
                 const uint64_t* stage_off, uint32_t* out_size) {
    KcS2Params P;
    memset(&P, 0, sizeof(P));
    P.src = src; P.blk_off = blk_off; P.stage_off = stage_off; P.stage = stage; P.out_size = out_size; P.n_blocks = n;
    P.level = level & 0xFF; P.variant = level >> 8; P.spec_w0 = w0; P.spec_w0b = w0b; P.spec_grow = grow; P.framed = framed;
    uint64_t mx = 0;
    for (uint32_t i = 0; i < n; i++) mx = std::max<uint64_t>(mx, blk_off[i + 1] - blk_off[i]);
    const size_t tb = kc_s2_table_bytes(P.level, mx, P.variant);
    std::vector<uint32_t> tab((size_t)((n + 7) / 8 * 8) * (tb / 4), 0);
    P.tables = tab.data(); P.table_stride = (uint32_t)(tb / 4);
    hipemu::set_group(8);  // 8 blocks per wave, the groups diverge freely
    kc_launch_s2_encode(P, nullptr);
    hipemu::set_group(64);
    return 0;
}

// the SpeedFastest match finder (kc_zfast_match_lds_kernel) over n units: packed sequences + KcBlkMeta per block
int kcemu_zfast_parse(const uint8_t* src, const uint64_t* unit_off, uint32_t n, int block_size, int window, int hist0, int rep1, int rep2,
                      int stream_mode, const uint32_t* proto, uint64_t* seqs, KcBlkMeta* meta, uint32_t seq_stride, const uint32_t* unit_blk0,
                      int spec_w0, int pos_bits) {
    KcMatchParams P;
    memset(&P, 0, sizeof(P));
    P.src = src;
    P.src_end = src + unit_off[n];
    P.unit_off = unit_off;
    P.unit_blk0 = unit_blk0;
    P.seqs = seqs;
    P.meta = meta;
    P.seq_stride = seq_stride;
    P.block_size = block_size;
    P.max_match_off = window;
    P.spec_w0 = spec_w0;
    P.hist0 = hist0;
    P.pos_bits = pos_bits;
    P.rep1 = rep1;
    P.rep2 = rep2;
    P.stream_mode = stream_mode;
    for (uint32_t i = 0; i < n; i++) if (unit_off[i + 1] - unit_off[i] > 131072) P.lds_any_big = 1;
    kc_launch_zfast_match_lds(P, proto, 0u, n, nullptr);
    return 0;
}

// the SpeedFastest HBM-table group kernel (kc_zfast_match_grp_kernel<8>) over n units; tables: n x 2^15 u32 kept by the caller between
// calls (epoch 0: zeroed by the caller; else the launch's stamp)
static int kcemu_zfast_grp(const uint8_t* src, const uint64_t* unit_off, uint32_t n, int block_size, int window, int stream_mode, uint64_t* seqs,
                           KcBlkMeta* meta, uint32_t seq_stride, const uint32_t* unit_blk0, int spec_w0, int spec_grow, int pos_bits, uint32_t* tables,
                           uint32_t epoch, int xseg_k, const uint64_t* first_bits) {
    KcMatchParams P;
    memset(&P, 0, sizeof(P));
    P.src = src;
    P.src_end = src + unit_off[n];
    P.unit_off = unit_off;
    P.unit_blk0 = unit_blk0;
    P.seqs = seqs;
    P.meta = meta;
    P.seq_stride = seq_stride;
    P.block_size = block_size;
    P.max_match_off = window;
    P.spec_w0 = spec_w0;
    P.spec_grow = spec_grow;
    P.pos_bits = pos_bits;
    P.rep1 = 1;
    P.rep2 = 4;
    P.stream_mode = stream_mode;
    P.epoch = epoch;
    P.xseg_k = xseg_k & 0xFFFFFF;
    P.tuned = P.xseg_k < (1 << 20) ? 1 : 0;  // (2^20: the plain form, rounds inside one skip segment, no filter)
    P.empty_filter = (xseg_k >> 24) & 1 ? 0 : 1;  // (bit 24 of the argument switches the filter off)
    P.first_bits = first_bits;
    hipemu::set_group(8);  // 8 units per wave, the groups diverge freely
    kc_launch_zfast_match_grp(P, tables, n, nullptr);
    hipemu::set_group(64);
    return 0;
}
int kcemu_zfast_parse_grp(const uint8_t* src, const uint64_t* unit_off, uint32_t n, int block_size, int window, int stream_mode, uint64_t* seqs,
                          KcBlkMeta* meta, uint32_t seq_stride, const uint32_t* unit_blk0, int spec_w0, int spec_grow, int pos_bits, uint32_t* tables,
                          uint32_t epoch, int xseg_k) {
    return kcemu_zfast_grp(src, unit_off, n, block_size, window, stream_mode, seqs, meta, seq_stride, unit_blk0, spec_w0, spec_grow, pos_bits, tables, epoch,
                           xseg_k, nullptr);
}
// the same with the first-occurrence bits of kcemu_zfast_first over the same src / unit_off (the tables must start empty for this launch)
int kcemu_zfast_parse_grp_first(const uint8_t* src, const uint64_t* unit_off, uint32_t n, int block_size, int window, int stream_mode, uint64_t* seqs,
                                KcBlkMeta* meta, uint32_t seq_stride, const uint32_t* unit_blk0, int spec_w0, int spec_grow, int pos_bits, uint32_t* tables,
                                uint32_t epoch, int xseg_k, const uint64_t* first_bits) {
    return kcemu_zfast_grp(src, unit_off, n, block_size, window, stream_mode, seqs, meta, seq_stride, unit_blk0, spec_w0, spec_grow, pos_bits, tables, epoch,
                           xseg_k, first_bits);
}

// kc_zfast_first_kernel over n units: bits = kcemu_zfast_first_words(src, unit_off[n] - unit_off[0], n) words (KcFirstParams has the layout)
uint64_t kcemu_zfast_first_words(const uint8_t* src, uint64_t total_bytes, uint32_t n) { return kc_zfast_first_words(src, total_bytes, n); }
int kcemu_zfast_first(const uint8_t* src, const uint64_t* unit_off, uint32_t n, uint64_t* bits) {
    KcFirstParams P;
    P.src = src;
    P.unit_off = unit_off;
    P.n_units = n;
    P.bits = bits;
    kc_launch_zfast_first(P, nullptr);
    return 0;
}
// KC_OPT_ZFAST_FIRST_FILTER for kcemu_zstd_batch (default 1), and whether its last call handed the match finder the bits
void kcemu_set_first_filter(int on) { g_first_opt = on; }
int kcemu_last_first_filter() { return g_first_used; }
// kc_zenc_host.h's rule for a batch of n units at `level` with hist0 bytes of dictionary content, as the jobs of a stream, chunk-fed
int kcemu_zenc_first_filter(int level, int hist0, int jobs, int fed, uint32_t n, int first_opt) {
    kc_zstd_opts o;
    kc_zstd_opts_default(&o);
    kc_zstd_opts_level(&o, level);
    kci::KcZencPlan pl;
    pl.hist0 = hist0;
    pl.n_units = n;
    return kci::zenc_first_filter(&o, pl, first_opt != 0, jobs != 0, fed != 0) ? 1 : 0;
}

// kc_xxh64_fin_kernel: the checksum field of every frame, and the payload of the frames flagged in unit_raw copied from the source
int kcemu_xxh_fin(const uint8_t* src, const uint64_t* unit_off, uint32_t n, uint8_t* stage, const uint64_t* stage_off, const uint32_t* out_size,
                  const uint64_t* out_off, uint8_t* dst, const uint32_t* unit_raw, const KcRawDef* rawdef, const uint32_t* unit_blk0, uint64_t* xxh_out,
                  int mode) {
    KcXxhFinParams P;
    memset(&P, 0, sizeof(P));
    P.src = src; P.unit_off = unit_off; P.n_units = n; P.stage = stage; P.stage_off = stage_off; P.out_size = out_size; P.out_off = out_off;
    P.dst = dst; P.unit_raw = unit_raw; P.rawdef = rawdef; P.unit_blk0 = unit_blk0; P.xxh_out = xxh_out; P.mode = mode;
    hipemu::set_group(4);  // one unit per quad; the quads' trip counts differ
    kc_launch_xxh64_fin(P, nullptr);
    hipemu::set_group(64);
    return 0;
}

// the encode batch's stride and position width (kc_zenc_host.h) for the tests that call single kernels with buffers of their own
uint32_t kcemu_zenc_seq_stride(int block_size) { return kci::zenc_seq_stride(block_size); }
int kcemu_zenc_pos_bits(uint64_t hist0, uint64_t max_unit) { return kci::zenc_pos_bits(hist0, std::max<uint64_t>(max_unit, 16)); }

// The options of a kcemu_zstd_batch call, resolved by the library's own option functions (block_size / window 0: the level's)
static void kcemu_zstd_opts(kc_zstd_opts& o, int level, int block_size, int window, int crc, int single, int full_zero, int entropy_opts) {
    kc_zstd_opts_default(&o);
    kc_zstd_opts_level(&o, level);
    if (window > 0) kc_zstd_opts_window(&o, window);
    if (block_size > 0 && block_size != o.block_size) { o.block_size = block_size; o.custom_block = 1; }  // (tests: block sizes no option function gives)
    kc_zstd_opts_crc(&o, crc);
    kc_zstd_opts_zero_frames(&o, full_zero);
    kc_zstd_opts_no_entropy(&o, entropy_opts & 1);
    if (entropy_opts & 2) kc_zstd_opts_all_lit_entropy(&o, 1);
    if (single >= 0) kc_zstd_opts_single_segment(&o, single);
}

// The device's zstd encode batch on the emulator: the plan, the parameter fill, the path predicates and the speculation re-run are
// the library's (kc_zenc_host.h, the rules kc_batch.cpp runs); the buffers are plain vectors and the kernels run on the emulator.
// This function's own: the forced kernel forms — level 1: the LDS-table kernel (spec_w0 16), or with use_grp the HBM-table group
// kernel in the form `tuned` (bit 8: the pre-scan asked for, as KC_OPT_ZFAST_PRESCAN 1 asks); levels 2 / 3 / 4: the level's match
// finder, tables cleared per launch — the KC_EMU_SPEC_* overrides, and the view of the frames: with fused_dst null as they sit in
// their staging slots (raw blocks' payloads included: no rawdef), else the contiguous output behind batch_end's finishing pass.
// cut_off / cuts: null, or the streams' Flush points as kc_zstd_encode_streams_cuts takes them.  stage null: the plan alone
// (stage_off: n + 1 slot offsets).  err_out: [0] device error flag, [1] units the re-run took, [2] raw-only frames, [3] units the
// pre-scan settled.  Returns 0, -2 when stage_cap is below the plan's need, -3 when the re-run does not converge.
int kcemu_zstd_batch(const uint8_t* src, const uint64_t* unit_off, uint32_t n, int level, int block_size, int window, int crc, int single, int full_zero,
                     int stream_mode, int use_grp, int tuned, int entropy_opts /* bit 0: no_entropy, bit 1: all_lit_entropy */, const uint64_t* cut_off,
                     const uint64_t* cuts, uint8_t* stage, uint64_t stage_cap, uint64_t* stage_off, uint32_t* out_size, uint32_t* err_out,
                     uint8_t* fused_dst /* or null */, uint64_t* fused_off, int fused_mode) {
    using namespace kci;
    kc_zstd_opts o;
    kcemu_zstd_opts(o, level, block_size, window, crc, single, full_zero, entropy_opts);
    static const uint64_t none = 0;
    KcZencCuts fl;
    if (cut_off) { fl.cut_off = cut_off; fl.cuts = cuts ? cuts : &none; }
    KcZencPlan pl;
    zenc_plan(&o, unit_off, n, nullptr, fl, pl);
    memcpy(stage_off, pl.stage_off.data(), (size_t)(n + 1) * 8);
    if (!stage) return 0;
    if (pl.need > stage_cap || !zenc_offsets_fit(&o, pl)) return -2;
    const uint32_t nb = pl.n_blocks;
    const KcZencReserve r = zenc_reserve(&o, pl);
    std::vector<uint64_t> seqs(r.seqs / 8 + pl.seq_stride, 0), aux(r.aux / 8 + pl.seq_stride, 0), xxh(n + 1, 0);
    std::vector<uint8_t> lits(r.lits + pl.lit_stride, 0), redo_blk(nb + 1, 0), pop_blk, predef(kc_fse_predef_bytes() + 64, 0);
    std::vector<KcBlkMeta> meta(nb + 1);
    std::vector<KcRawDef> rawdef(nb + 1, KcRawDef{0, 0, 0, 0});
    std::vector<uint32_t> redo(n + 1, 0), unit_raw(n + 1, 0), unit_done, probe_rel, list, tables;
    std::vector<uint32_t> blk_start(pl.blk_start), unit_flags(pl.unit_flags);
    blk_start.push_back(0);
    unit_flags.push_back(0);
    uint32_t err[16] = {0};
    const bool fuse_xxh = zenc_fuse_xxh(&o, pl, fused_dst != nullptr, false, false);
    KcZencBufs b;
    b.src = src + unit_off[0]; b.unit_off = pl.rel_off.data(); b.unit_blk0 = pl.blk0.data(); b.blk_start = blk_start.data(); b.unit_flags = unit_flags.data();
    b.seqs = seqs.data(); b.aux = aux.data(); b.meta = meta.data(); b.lits = lits.data(); b.stage = stage; b.redo_blk = redo_blk.data();
    b.stage_off = pl.stage_off.data(); b.xxh = xxh.data(); b.out_size = out_size; b.redo = redo.data(); b.errflag = err; b.unit_raw = unit_raw.data();
    b.predef = predef.data(); b.rawdef = rawdef.data();
    KcZencSteer cx;
    cx.stream_mode = stream_mode;
    cx.fuse_xxh = fuse_xxh;
    if (level == KC_SPEED_DEFAULT) {  // (tests: other speculation policies = other round shapes)
        if (const char* e = getenv("KC_EMU_SPEC_W0")) cx.spec_w0 = atoi(e);
        if (const char* e = getenv("KC_EMU_SPEC_GROW")) cx.spec_grow = atoi(e);
    }
    KcMatchParams M;
    KcEntropyParams E;
    zenc_fill_params(&o, pl, b, cx, M, E);
    if (fused_dst == nullptr) E.rawdef = nullptr;  // the frames are read in their slots
    kc_launch_fse_predef_init(predef.data(), nullptr);
    const bool prescan = zenc_run_prescan(&o, pl, (tuned & 0x100) ? 1 : 0, false, fuse_xxh, stream_mode);
    tuned &= 0xFF;
    if (prescan) {
        probe_rel.resize(8192);
        const uint32_t np = kc_zfast_probe_positions(o.block_size, probe_rel.data(), (uint32_t)probe_rel.size());
        unit_done.assign(n + 1, 0xFFFFFFFFu);
        const KcPrescanParams Q = zenc_prescan_params(&o, pl, M, E, probe_rel.data(), np, unit_done.data());
        kc_launch_zfast_prescan(Q, nullptr);
        M.unit_done = E.unit_done = unit_done.data();
        uint32_t nd = 0;
        for (uint32_t i = 0; i < n; i++) nd += unit_done[i] == 1u;
        err_out[3] = nd;
    }
    if (o.crc && !fuse_xxh) {
        hipemu::set_group(4);
        kc_launch_xxh64(b.src, pl.rel_off.data(), n, xxh.data(), nullptr);
        hipemu::set_group(64);
    }
    // the match finder over n_launch units (all, or the re-run's list), in the forced form
    // the first-occurrence bits under the library's rule (the speculation re-run below reads the same ones)
    std::vector<uint64_t> first_bits;
    g_first_used = 0;
    if (use_grp && zenc_first_filter(&o, pl, g_first_opt != 0, false, false)) {
        first_bits.assign(kc_zfast_first_words(M.src, pl.rel_off[n], n), 0xA7A7A7A7A7A7A7A7ull);
        KcFirstParams F;
        F.src = M.src; F.unit_off = M.unit_off; F.n_units = n; F.bits = first_bits.data();
        kc_launch_zfast_first(F, nullptr);
        M.first_bits = first_bits.data();
        g_first_used = 1;
    }
    std::vector<uint64_t> btab;
    uint32_t bcur[2] = {0, 0};
    int32_t bcost[96];
    if (level == KC_SPEED_BEST) {  // two persistent table slots, the bit costs from the device's own kernel
        btab.assign((size_t)2 * (kc_zbest_table_bytes() / 8), 0);
        memset(bcost, 0, sizeof(bcost));
        kc_launch_zbest_cost(predef.data(), bcost, nullptr);
    }
    auto run_match = [&](uint32_t n_launch) {
        const int lanes = level == KC_SPEED_BETTER ? 16 : 8;  // lanes per unit of the group kernels
        if (level == KC_SPEED_BEST) {
            kc_launch_zbest_match(M, btab.data(), bcur, bcost, n_launch, 2, nullptr);
        } else if (level == KC_SPEED_FASTEST && !use_grp) {
            KcMatchParams ml = M;
            ml.spec_w0 = 16;
            kc_launch_zfast_match_lds(ml, nullptr, 0u, n_launch, nullptr);
        } else {
            const uint32_t per_wave = 64 / lanes;
            tables.assign((size_t)((n_launch + per_wave - 1) / per_wave * per_wave) * (zenc_table_bytes(level) / 4), 0);
            hipemu::set_group(lanes);
            if (level == KC_SPEED_DEFAULT) kc_launch_zdfast_match_grp(M, tables.data(), n_launch, nullptr);
            else if (level == KC_SPEED_BETTER) kc_launch_zbetter_match_grp(M, (uint8_t*)tables.data(), n_launch, false, nullptr);
            else {
                KcMatchParams mf = M;
                mf.tuned = tuned;
                mf.empty_filter = 1;
                kc_launch_zfast_match_grp(mf, tables.data(), n_launch, nullptr);
            }
            hipemu::set_group(64);
        }
    };
    // batch_end's finishing pass: sizes -> offsets, checksum (+ payload of the raw-only frames), compaction
    auto finish_pass = [&]() {
        kc_launch_scan_sizes(out_size, n, fused_off, nullptr);
        if (E.unit_raw != nullptr) {
            const KcXxhFinParams X = zenc_xxh_fin_params(E, n, fused_off, fused_dst, xxh.data(), fused_mode);
            hipemu::set_group(4);
            kc_launch_xxh64_fin(X, nullptr);
            hipemu::set_group(64);
        }
        kc_launch_compact(stage, E.stage_off, out_size, fused_off, fused_dst, n, nullptr, E.src, E.unit_off, E.unit_blk0, E.rawdef, E.unit_raw);
    };
    run_match(n);
    kc_launch_zstd_entropy(E, n, nullptr);
    if (fused_dst != nullptr) finish_pass();
    uint32_t redo_units = 0;
    const uint32_t max_passes = zenc_redo_max_passes(pl);
    for (uint32_t iter = 0;; iter++) {
        zenc_redo_units(redo.data(), n, list);
        if (err[0] != 0 || list.empty()) break;
        if (iter > max_passes) return -3;
        zenc_redo_mark(pl, list, redo_blk.data(), pop_blk);
        redo_units += (uint32_t)list.size();
        std::fill(redo.begin(), redo.end(), 0u);
        std::fill(redo_blk.begin(), redo_blk.end(), (uint8_t)0);
        M.pop_blk = pop_blk.data();
        M.unit_list = E.unit_list = list.data();
        run_match((uint32_t)list.size());
        kc_launch_zstd_entropy(E, (uint32_t)list.size(), nullptr);
    }
    if (redo_units != 0 && fused_dst != nullptr) finish_pass();
    if (fuse_xxh) {
        uint32_t nraw = 0;
        for (uint32_t i = 0; i < n; i++) nraw += unit_raw[i];
        err_out[2] = nraw;
    }
    err_out[0] = err[0];
    err_out[1] = redo_units;
    return 0;
}

// kcemu_zstd_batch under this export's earlier signature, which the test helpers of earlier revisions call: the level rides in use_grp (2 / 3 / 4),
// block_size and window are given, and the frames go to the caller's own slots (stage_off), as far as a slot holds them.
int kcemu_zstd_frames(const uint8_t* src, const uint64_t* unit_off, uint32_t n, int block_size, int window, int crc, int single, int full_zero,
                      int stream_mode, int use_grp, int tuned, int entropy_opts, uint8_t* stage, const uint64_t* stage_off, uint32_t* out_size,
                      uint32_t* err_out, uint8_t* fused_dst /* or null */, uint64_t* fused_off, int fused_mode) {
    const int level = use_grp >= 2 ? use_grp : KC_SPEED_FASTEST;
    std::vector<uint64_t> own_off(n + 1, 0);
    auto call = [&](uint8_t* st, uint64_t cap) {
        return kcemu_zstd_batch(src, unit_off, n, level, block_size, window, crc, single, full_zero, stream_mode, use_grp == 1, tuned, entropy_opts, nullptr,
                                nullptr, st, cap, own_off.data(), out_size, err_out, fused_dst, fused_off, fused_mode);
    };
    if (int r = call(nullptr, 0)) return r;
    std::vector<uint8_t> own((size_t)own_off[n] + 64, 0);
    if (int r = call(own.data(), own_off[n])) return r;
    for (uint32_t i = 0; i < n; i++)
        memcpy(stage + stage_off[i], own.data() + own_off[i], (size_t)std::min<uint64_t>(out_size[i], stage_off[i + 1] - stage_off[i]));
    return 0;
}

// N blocks through kc_s2_best_kernel (level 4: s2.EncodeBest, 5: s2.EncodeSnappyBest); tables: n x (4.5 MiB / 4) u32, zeroed by the caller
int kcemu_s2_best(int level, const uint8_t* src, const uint64_t* blk_off, uint32_t n, uint8_t* stage, const uint64_t* stage_off, uint32_t* out_size,
                  uint32_t* tables) {
    KcS2Params P;
    memset(&P, 0, sizeof(P));
    P.src = src;
    P.blk_off = blk_off;
    P.stage_off = stage_off;
    P.stage = stage;
    P.out_size = out_size;
    P.tables = tables;
    P.table_stride = (uint32_t)(kc_s2_table_bytes(level, 0) / 4);
    P.n_blocks = n;
    P.level = level;
    hipemu::set_group(SBG);  // 16 lanes per block, the groups of a wave diverge freely
    kc_launch_s2_best(P, nullptr);
    hipemu::set_group(64);
    return 0;
}

// n units through kc_zbest_match_kernel (SpeedBestCompression) on n_slots persistent table slots; tables: n_slots x 34 MiB / 8 u64,
// slot_cur: n_slots u32 (0 = fresh); cost: 96 int32 (the predefined-table bit costs)
int kcemu_zbest_parse(const uint8_t* src, const uint64_t* unit_off, uint32_t n, int block_size, int window, int hist0, int rep1, int rep2, int rep3,
                      int stream_mode, uint64_t* seqs, KcBlkMeta* meta, uint32_t seq_stride, const uint32_t* unit_blk0, const uint32_t* unit_hist,
                      const uint32_t* job_flags, uint64_t* tables, uint32_t* slot_cur, const int32_t* cost, uint32_t n_slots) {
    KcMatchParams P;
    memset(&P, 0, sizeof(P));
    P.src = src;
    P.src_end = src + unit_off[n];
    P.unit_off = unit_off;
    P.unit_blk0 = unit_blk0;
    P.seqs = seqs;
    P.meta = meta;
    P.seq_stride = seq_stride;
    P.block_size = block_size;
    P.max_match_off = window;
    P.hist0 = hist0;
    P.rep1 = rep1;
    P.rep2 = rep2;
    P.rep3 = rep3;
    P.stream_mode = stream_mode;
    P.unit_hist = unit_hist;
    P.job_flags = job_flags;
    kc_launch_zbest_match(P, tables, slot_cur, cost, n, n_slots, nullptr);
    return 0;
}

uint64_t kcemu_collectives() { return hipemu::collectives(); }

}  // extern "C"
