// kc_ctx.cpp — the context: device self-check, creation, options, scratch, timings.  (The zstd option functions: kc_zstd_opts.cpp.)
#include "kc_host.h"

extern "C" {

// ---------------------------------------------------------------------------------------
// device self-check (round 6).  Three GPU sessions of round 5 died in their first process on boxes whose GPU did
// not answer (memory-access faults in the first hipMalloc, a 20-minute hang before the first test line).  The first kc_ctx_create
// on a device therefore runs one known-answer launch on a thread of its own — a 256-byte buffer through the XXH64 kernel, digest
// compared with the published value (xxhash.go:27-230; XXH64(seed 0) of the bytes 0..255 = 0x1FACBE8406CD904B) — and waits for it
// with a deadline: a device that faults, hangs or computes something else makes kc_ctx_create return an error with a text
// (kc_create_error) instead of taking the host process with it.  The verdict is kept per device for the life of the process.
// ---------------------------------------------------------------------------------------
namespace {
struct SelfCheck {
    std::mutex m;
    std::condition_variable cv;
    bool done = false;
    kc_status st = KC_OK;
    std::string text;
};
std::mutex g_sc_m;
int g_sc_state[64] = {0};  // 0 not run, 1 passed, -1 failed
kc_status g_sc_status[64];
std::string g_sc_text[64];
thread_local std::string t_create_err;

void selfcheck_body(int device, const std::shared_ptr<SelfCheck>& sc) {
    kc_status st = KC_OK;
    std::string text;
    uint8_t h_in[256];
    for (int i = 0; i < 256; i++) h_in[i] = (uint8_t)i;
    const uint64_t h_off[2] = {0, 256};
    uint64_t h_out = 0;
    uint8_t* d_in = nullptr;
    uint64_t *d_off = nullptr, *d_out = nullptr;
    hipStream_t s = nullptr;
    auto fail = [&](const char* what, hipError_t e) { st = KC_ERR_HIP; text = std::string("device self-check: ") + what + ": " + hipGetErrorString(e); };
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) fail("hipSetDevice", e);
    if (st == KC_OK && (e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking)) != hipSuccess) fail("hipStreamCreate", e);
    if (st == KC_OK && (e = hipMalloc((void**)&d_in, 256 + 64)) != hipSuccess) fail("hipMalloc", e);
    if (st == KC_OK && (e = hipMalloc((void**)&d_off, 16)) != hipSuccess) fail("hipMalloc", e);
    if (st == KC_OK && (e = hipMalloc((void**)&d_out, 8)) != hipSuccess) fail("hipMalloc", e);
    if (st == KC_OK && (e = hipMemcpyAsync(d_in, h_in, 256, hipMemcpyHostToDevice, s)) != hipSuccess) fail("hipMemcpyAsync (H2D)", e);
    if (st == KC_OK && (e = hipMemcpyAsync(d_off, h_off, 16, hipMemcpyHostToDevice, s)) != hipSuccess) fail("hipMemcpyAsync (H2D)", e);
    if (st == KC_OK) {
        kc_launch_xxh64(d_in, d_off, 1, d_out, s);
        if ((e = hipGetLastError()) != hipSuccess) fail("kernel launch", e);
    }
    if (st == KC_OK && (e = hipMemcpyAsync(&h_out, d_out, 8, hipMemcpyDeviceToHost, s)) != hipSuccess) fail("hipMemcpyAsync (D2H)", e);
    if (st == KC_OK && (e = hipStreamSynchronize(s)) != hipSuccess) fail("hipStreamSynchronize", e);
    if (st == KC_OK && h_out != 0x1FACBE8406CD904BULL) {
        char b[160];
        snprintf(b, sizeof(b), "device self-check: XXH64 known answer differs (got %016llx, want 1facbe8406cd904b): the device computes wrong results", (unsigned long long)h_out);
        st = KC_ERR_INTERNAL;
        text = b;
    }
    if (d_in) (void)hipFree(d_in);
    if (d_off) (void)hipFree(d_off);
    if (d_out) (void)hipFree(d_out);
    if (s) (void)hipStreamDestroy(s);
    std::lock_guard<std::mutex> lk(sc->m);
    sc->st = st;
    sc->text = text;
    sc->done = true;
    sc->cv.notify_all();
}

kc_status device_selfcheck(int device, std::string* text) {
    if (device < 0 || device >= 64) return KC_OK;
    std::lock_guard<std::mutex> g(g_sc_m);  // (a second creator waits for the first one's verdict)
    if (g_sc_state[device] == 0) {
        auto sc = std::make_shared<SelfCheck>();
        std::thread([device, sc] { selfcheck_body(device, sc); }).detach();  // detached: a device that never answers keeps this thread, not the caller
        std::unique_lock<std::mutex> lk(sc->m);
        const int deadline_s = 90;  // (the first launch of a process loads the code object and may page the runtime in: seconds on a healthy box)
        if (!sc->cv.wait_for(lk, std::chrono::seconds(deadline_s), [&] { return sc->done; })) {
            g_sc_state[device] = -1;
            g_sc_status[device] = KC_ERR_HIP;
            g_sc_text[device] = "device self-check: the device did not answer a 256-byte known-answer launch within " + std::to_string(deadline_s) + " s (hung queue or faulted context): no kc_* call was attempted";
        } else {
            g_sc_state[device] = sc->st == KC_OK ? 1 : -1;
            g_sc_status[device] = sc->st;
            g_sc_text[device] = sc->text;
        }
    }
    if (g_sc_state[device] < 0) { *text = g_sc_text[device]; return g_sc_status[device]; }
    return KC_OK;
}
}  // namespace

const char* kc_create_error(void) { return t_create_err.c_str(); }

// ---------------------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------------------
kc_status kc_ctx_create(kc_ctx** out, int device, void* stream) {
    if (!out) return KC_ERR_BAD_ARG;
    *out = nullptr;
    t_create_err.clear();
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) { t_create_err = "no such HIP device"; return KC_ERR_NO_DEVICE; }
    {
        const kc_status sc = device_selfcheck(device, &t_create_err);
        if (sc != KC_OK) return sc;
    }
    kc_ctx* c = new kc_ctx();
    c->device = device;
    if (hipSetDevice(device) != hipSuccess || hipGetDeviceProperties(&c->prop, device) != hipSuccess) {
        delete c;
        return KC_ERR_NO_DEVICE;
    }
    if (stream) {
        c->stream = (hipStream_t)stream;
    } else {
        if (hipStreamCreate(&c->stream) != hipSuccess) { delete c; return KC_ERR_HIP; }
        c->own_stream = true;
    }
    for (auto& e : c->ev)
        if (hipEventCreate(&e) != hipSuccess) { delete c; return KC_ERR_HIP; }
    // every tunable is a field of the context with its default in KcCfg; kc_ctx_set_option is the only way to change one (the library
    // reads no environment variable: measurement harnesses map their KC_* variables to options above the C ABI, compress_amd/_lib.py)
    *out = c;
    return KC_OK;
}

kc_status kc_ctx_set_option(kc_ctx* c, int key, int64_t v) {
    if (!c) return KC_ERR_BAD_ARG;
    KcCfg& g = c->cfg;
    switch (key) {
        case KC_OPT_MATCH_PATH: if (v < KC_PATH_AUTO || v > KC_PATH_LDS) return KC_ERR_BAD_ARG; g.match_path = v; break;
        case KC_OPT_ZFAST_LDS_MAX_UNITS: g.zfast_lds_max_units = v; break;
        case KC_OPT_S2_LDS_MAX_BLOCKS: g.s2_lds_max_blocks = v; break;
        case KC_OPT_SPEC_W0: g.spec_w0 = v; break;
        case KC_OPT_SPEC_GROW: g.spec_grow = v; break;
        case KC_OPT_LDS_SPEC_W0: g.lds_spec_w0 = v; break;
        case KC_OPT_S2_LDS_SPEC_W0: g.s2_lds_spec_w0 = v; break;
        case KC_OPT_HOST_SERIAL: g.host_serial = v; break;
        case KC_OPT_HOST_PIPE_MIB: g.host_pipe_mib = v; break;
        case KC_OPT_HOST_OVERLAP_MIN_MIB: g.host_overlap_min_mib = v; break;
        case KC_OPT_HOST_COPY_THREADS: g.host_copy_threads = v; break;
        case KC_OPT_HOST_TRACE: g.host_trace = v; break;
        case KC_OPT_HOST_ROLL: g.host_roll = v != 0; break;
        case KC_OPT_HOST_ROLL_MIB: if (v < 0) return KC_ERR_BAD_ARG; g.host_roll_mib = v; break;
        case KC_OPT_HOST_CHUNK_MIB: g.host_chunks.clear(); if (v > 0) g.host_chunks.push_back((uint64_t)v << 20); break;
        case KC_OPT_HOST_CHUNK_MIB_APPEND: if (v < 1) return KC_ERR_BAD_ARG; g.host_chunks.push_back((uint64_t)v << 20); break;
        case KC_OPT_K2_PROF: g.k2_prof = v; break;
        case KC_OPT_S2_HOOK_WAIT_US: g.hook_wait_us = v; break;
        case KC_OPT_S2_HOOK_BATCH: g.hook_batch = v < 1 ? 1 : v; break;
        case KC_OPT_S2_HOOK_LANES: g.hook_lanes = v < 1 ? 1 : (v > 8 ? 8 : v); break;
        case KC_OPT_S2_HOOK_HOST_FIRST: g.hook_host_first = v < -1 ? -1 : v; break;
        case KC_OPT_TEST_FEED_REDO: g.test_feed_redo = v; break;
        case KC_OPT_MAX_SCRATCH_MIB: if (v < 1) return KC_ERR_BAD_ARG; c->max_scratch_bytes = (uint64_t)v << 20; break;
        case KC_OPT_BEST_SLOTS: if (v < 1 || v > 8192) return KC_ERR_BAD_ARG; g.best_slots = v; break;
        case KC_OPT_S2_VARIANT: if (v != KC_S2_VARIANT_GO && v != KC_S2_VARIANT_AMD64) return KC_ERR_BAD_ARG; g.s2_variant = v; break;
        case KC_OPT_BETTER_DICT_EPOCH: g.better_dict_epoch = v != 0; break;
        case KC_OPT_ZFAST_EPOCH: g.zfast_epoch = v != 0; break;
        case KC_OPT_ZFAST_XSEG_K: if (v < 0) return KC_ERR_BAD_ARG; g.zfast_xseg_k = v > (1 << 30) ? (1 << 30) : v; break;
        case KC_OPT_FUSE_RAW_XXH: g.fuse_raw_xxh = v != 0; break;
        case KC_OPT_ZFAST_FILTER: g.zfast_filter = v != 0; break;
        case KC_OPT_ZFAST_VARIANT: if (v < -1 || v > 1) return KC_ERR_BAD_ARG; g.zfast_variant = v; break;
        case KC_OPT_ZFAST_PRESCAN: if (v < -1 || v > 1) return KC_ERR_BAD_ARG; g.zfast_prescan = v; break;
        case KC_OPT_ZFAST_FIRST_FILTER: g.zfast_first_filter = v != 0; break;
        case KC_OPT_XXH_FIN_MODE: if (v < 0 || v > 3) return KC_ERR_BAD_ARG; g.xxh_fin_mode = v; break;
        case KC_OPT_JOB_PRIME: g.job_prime = v != 0; break;
        case KC_OPT_DSTREAM_BLOCKS: if (v < 1 || v > 4096) return KC_ERR_BAD_ARG; g.dstream_blocks = v; break;
        case KC_OPT_S2_RSTREAM_CHUNKS: if (v < 1 || v > 4096) return KC_ERR_BAD_ARG; g.s2_rstream_chunks = v; break;
        case KC_OPT_STAGE2_STREAM: if (c->pend) return KC_ERR_BAD_ARG; c->stream2 = (hipStream_t)(intptr_t)v; break;
        default: return KC_ERR_BAD_ARG;
    }
    return KC_OK;
}

int64_t kc_ctx_get_option(const kc_ctx* c, int key) {
    if (!c) return -1;
    const KcCfg& g = c->cfg;
    switch (key) {
        case KC_OPT_MATCH_PATH: return g.match_path;
        case KC_OPT_ZFAST_LDS_MAX_UNITS: return g.zfast_lds_max_units;
        case KC_OPT_S2_LDS_MAX_BLOCKS: return g.s2_lds_max_blocks;
        case KC_OPT_SPEC_W0: return g.spec_w0;
        case KC_OPT_SPEC_GROW: return g.spec_grow;
        case KC_OPT_LDS_SPEC_W0: return g.lds_spec_w0;
        case KC_OPT_S2_LDS_SPEC_W0: return g.s2_lds_spec_w0;
        case KC_OPT_HOST_SERIAL: return g.host_serial;
        case KC_OPT_HOST_PIPE_MIB: return g.host_pipe_mib;
        case KC_OPT_HOST_OVERLAP_MIN_MIB: return g.host_overlap_min_mib;
        case KC_OPT_HOST_COPY_THREADS: return g.host_copy_threads;
        case KC_OPT_HOST_TRACE: return g.host_trace;
        case KC_OPT_HOST_ROLL: return g.host_roll;
        case KC_OPT_HOST_ROLL_MIB: return g.host_roll_mib;
        case KC_OPT_HOST_CHUNK_MIB: return g.host_chunks.empty() ? 0 : (int64_t)(g.host_chunks[0] >> 20);
        case KC_OPT_K2_PROF: return g.k2_prof;
        case KC_OPT_S2_HOOK_WAIT_US: return g.hook_wait_us;
        case KC_OPT_S2_HOOK_BATCH: return g.hook_batch;
        case KC_OPT_S2_HOOK_LANES: return g.hook_lanes;
        case KC_OPT_S2_HOOK_HOST_FIRST: return g.hook_host_first;
        case KC_OPT_TEST_FEED_REDO: return g.test_feed_redo;
        case KC_OPT_MAX_SCRATCH_MIB: return (int64_t)(c->max_scratch_bytes >> 20);
        case KC_OPT_BEST_SLOTS: return g.best_slots;
        case KC_OPT_S2_VARIANT: return g.s2_variant;
        case KC_OPT_BETTER_DICT_EPOCH: return g.better_dict_epoch;
        case KC_OPT_ZFAST_EPOCH: return g.zfast_epoch;
        case KC_OPT_ZFAST_XSEG_K: return g.zfast_xseg_k;
        case KC_OPT_FUSE_RAW_XXH: return g.fuse_raw_xxh;
        case KC_OPT_ZFAST_FILTER: return g.zfast_filter;
        case KC_OPT_ZFAST_VARIANT: return g.zfast_variant;
        case KC_OPT_ZFAST_PRESCAN: return g.zfast_prescan;
        case KC_OPT_ZFAST_FIRST_FILTER: return g.zfast_first_filter;
        case KC_OPT_XXH_FIN_MODE: return g.xxh_fin_mode;
        case KC_OPT_JOB_PRIME: return g.job_prime;
        case KC_OPT_DSTREAM_BLOCKS: return g.dstream_blocks;
        case KC_OPT_S2_RSTREAM_CHUNKS: return g.s2_rstream_chunks;
        case KC_OPT_STAGE2_STREAM: return (int64_t)(intptr_t)c->stream2;
        case KC_OPT_LAST_PATH: return c->last_path;
        case KC_OPT_LAST_PRESCAN_UNITS: return c->last_prescan_units;
        case KC_OPT_LAST_FIRST_BITS: return c->last_first_bits;
        case KC_OPT_LAST_BATCHES: return c->last_batches;
        default: return -1;
    }
}

static void ctx_free_scratch(kc_ctx* c) {
    DevBuf* bufs[] = {&c->unit_off, &c->unit_blk0, &c->stage_off, &c->seqs, &c->aux, &c->lits, &c->meta, &c->stage, &c->out_size, &c->xxh,
                      &c->redo, &c->popmask, &c->unit_list, &c->out_off, &c->blk_start, &c->unit_flags, &c->redo_blk, &c->pop_blk, &c->predef, &c->errflag, &c->tmp_src, &c->tmp_dst, &c->tables, &c->prof, &c->work, &c->work_off, &c->dictbuf, &c->proto, &c->dicthuf,
                      &c->d_job_hist, &c->d_job_flags, &c->rawdef, &c->unit_raw, &c->unit_done, &c->probe_rel, &c->first_bits, &c->best_tables, &c->best_cur, &c->best_cost};
    for (DevBuf* b : bufs) {
        if (b->p) (void)hipFree(b->p);
        b->p = nullptr;
        b->cap = 0;
    }
    auto free_all = [](DevBuf* b, size_t n) {
        for (; n; b++, n--) {
            if (b->p) (void)hipFree(b->p);
            b->p = nullptr;
            b->cap = 0;
        }
    };
    free_all(c->zd, sizeof(c->zd) / sizeof(DevBuf));    // DecodeAll (kc_zstd_dec_api.cpp)
    free_all(c->s2d, sizeof(c->s2d) / sizeof(DevBuf));  // s2.Reader (kc_s2_dec_api.cpp)
    free_all(c->s2r, sizeof(c->s2r) / sizeof(DevBuf));  // ranged reads (kc_s2_ranges_api.cpp)
    free_all(c->fl, sizeof(c->fl) / sizeof(DevBuf));    // flate / gzip readers (kc_flate_api.cpp)
    free_all(c->df, sizeof(c->df) / sizeof(DevBuf));    // flate / gzip writers (kc_deflate_api.cpp)
    free_all(c->sl, sizeof(c->sl) / sizeof(DevBuf));    // flate / gzip stateless writers (kc_stateless_api.cpp)
    free_all(c->zp, sizeof(c->zp) / sizeof(DevBuf));    // zip members (kc_zip_api.cpp)
    // what the context remembered about the freed buffers' contents
    c->predef_ready = false;
    c->tab_owner = 0;
    c->tab_ptr = nullptr;
    c->tab_units = c->tab_ep = 0;
    c->proto_key = 0;
    c->proto_ptr = c->dictbuf_ptr = nullptr;
    c->best_n = 0;
    c->probe_bs = 0;
    c->probe_n = 0;
    c->preclear_bytes = 0;
    c->preclear_ptr = nullptr;
    c->up_ptr[0] = c->up_ptr[1] = c->up_ptr[2] = nullptr;
}

kc_status kc_ctx_trim(kc_ctx* c) {
    if (!c) return KC_ERR_BAD_ARG;
    if (c->pend || c->job_active) { c->err = "kc_ctx_trim: a batch or a submitted job is in flight on this context"; return KC_ERR_BAD_ARG; }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    ctx_free_scratch(c);
    if (c->hpipe) { host_pipe_free(c->hpipe); c->hpipe = nullptr; }
    return KC_OK;
}

kc_status kc_device_trim(int device) { return kci::host_roll_trim(device); }

kc_status kc_host_alloc(void** out, uint64_t bytes) {
    if (!out || bytes == 0) return KC_ERR_BAD_ARG;
    *out = nullptr;
    const hipError_t e = hipHostMalloc(out, (size_t)bytes, hipHostMallocDefault);
    if (e != hipSuccess) { (void)hipGetLastError(); *out = nullptr; return e == hipErrorOutOfMemory ? KC_ERR_UNSUPPORTED : KC_ERR_HIP; }
    return KC_OK;
}
void kc_host_free(void* p) {
    if (p) (void)hipHostFree(p);
}

void kc_ctx_destroy(kc_ctx* c) {
    if (!c) return;
    if (c->job_active && c->job.joinable()) c->job.join();
    (void)hipSetDevice(c->device);
    ctx_free_scratch(c);
    for (auto& e : c->ev)
        if (e) (void)hipEventDestroy(e);
    if (c->ev_preclear) (void)hipEventDestroy(c->ev_preclear);
    if (c->pend) { delete (Pending*)c->pend; c->pend = nullptr; }
    if (c->hook) { s2_hook_free(c->hook); c->hook = nullptr; }
    if (c->hpipe) { host_pipe_free(c->hpipe); c->hpipe = nullptr; }
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

const char* kc_last_error(const kc_ctx* c) { return c ? c->err.c_str() : "null context"; }

kc_status kc_device_info(const kc_ctx* c, int32_t* n_cu, int32_t* lds_per_cu, int32_t* clock_khz, char* name, size_t name_cap) {
    if (!c) return KC_ERR_BAD_ARG;
    if (n_cu) *n_cu = c->prop.multiProcessorCount;
    if (lds_per_cu) *lds_per_cu = (int32_t)c->prop.maxSharedMemoryPerMultiProcessor;
    if (clock_khz) *clock_khz = c->prop.clockRate;
    if (name && name_cap) { strncpy(name, c->prop.gcnArchName, name_cap - 1); name[name_cap - 1] = 0; }
    return KC_OK;
}

kc_status kc_last_timings(const kc_ctx* c, kc_timings* t) {
    if (!c || !t) return KC_ERR_BAD_ARG;
    *t = c->last;
    return KC_OK;
}

}  // extern "C"

