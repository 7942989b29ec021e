// kc_batch.cpp — the zstd device pipeline: table preparation, batch_begin / batch_end (match finder, entropy stage, speculation
// re-run, size scan, checksum, compaction), scratch budgeting, and the device-resident entry points.
#include "kc_host.h"

// ---------------------------------------------------------------------------------------
// zstd device pipeline
// ---------------------------------------------------------------------------------------
namespace kci {


// Host-side construction of the dictionary-primed tables of betterFastEncoderDict.Reset
// (zstd/enc_better.go:1114-1183) in the device entry format (position+1 | tag << pos_bits).
void build_better_dict_tables(const uint8_t* dict, size_t len, int pos_bits, uint8_t* out, int reserved_bits = 0) {
    const int TB = (32 - pos_bits - reserved_bits) > 16 ? 16 : (32 - pos_bits - reserved_bits);  // reserved: the epoch stamp's bits (kc_zstd_match_better.hip)
    auto tagOf = [&](uint32_t v) -> uint32_t { return TB > 0 ? ((v * 2654435761u) >> (32 - TB)) : 0u; };
    auto mk = [&](uint64_t pos, uint32_t val) -> uint32_t { return ((uint32_t)pos + 1u) | (tagOf(val) << pos_bits); };
    auto ld64h = [&](size_t i) -> uint64_t { uint64_t v; memcpy(&v, dict + i, 8); return v; };
    uint32_t* ltab = (uint32_t*)out;  // pairs {offset, prev}
    uint32_t* stab = (uint32_t*)(out + ((size_t)8 << 19));
    if (len < 8) return;
    // short table: every position i, i+1, i+2, i+3 for i stepping by 4 while i < len-8 (:1126-1152)
    for (size_t i = 0; i + 8 < len; i += 4) {
        const uint64_t cv = ld64h(i);
        for (int k = 0; k < 4; k++) {
            const uint64_t v = cv >> (8 * k);
            const uint32_t h = (uint32_t)(((v << 24) * 889523592379ULL) >> (64 - 13));
            stab[h] = mk(i + k, (uint32_t)v);
        }
    }
    // long table: every position 0 .. len-9, chained (:1161-1183)
    for (size_t i = 0; i + 8 < len || i == 0; i++) {
        const uint64_t cv = ld64h(i);
        const uint32_t h = (uint32_t)((cv * 0xcf1bbcdcb7a56463ULL) >> (64 - 19));
        const uint32_t old = ltab[2 * h];
        ltab[2 * h] = mk(i, (uint32_t)cv);
        ltab[2 * h + 1] = old;
        if (i + 8 >= len) break;
    }
}

// fastEncoderDict.Reset (zstd/enc_fast.go:813-845): 2^15 table, 6-byte hash, positions i and i+1 for i stepping by 2.
// Also the SHORT table of doubleFastEncoderDict, which embeds fastEncoderDict and keeps this priming although its
// lookups use the 5-byte hash (enc_dfast.go:1053-1056).
void build_fast_dict_table(const uint8_t* dict, size_t len, int pos_bits, uint32_t* tab) {
    const int TB = (32 - pos_bits) > 16 ? 16 : (32 - pos_bits);
    auto tagOf = [&](uint32_t v) -> uint32_t { return TB > 0 ? ((v * 2654435761u) >> (32 - TB)) : 0u; };
    auto mk = [&](uint64_t pos, uint32_t val) -> uint32_t { return ((uint32_t)pos + 1u) | (tagOf(val) << pos_bits); };
    if (len < 8) return;
    for (size_t i = 0; i + 8 < len; i += 2) {
        uint64_t cv;
        memcpy(&cv, dict + i, 8);
        const uint32_t h0 = (uint32_t)(((cv << 16) * 227718039650203ULL) >> (64 - 15));
        const uint32_t h1 = (uint32_t)((((cv >> 8) << 16) * 227718039650203ULL) >> (64 - 15));
        tab[h0] = mk(i, (uint32_t)cv);
        tab[h1] = mk(i + 1, (uint32_t)(cv >> 8));
    }
}
// doubleFastEncoderDict.Reset long table (zstd/enc_dfast.go:1060-1083): every position 0 .. len-9, 8-byte hash, 2^17.
void build_dfast_dict_long(const uint8_t* dict, size_t len, int pos_bits, uint32_t* ltab) {
    const int TB = (32 - pos_bits) > 16 ? 16 : (32 - pos_bits);
    auto tagOf = [&](uint32_t v) -> uint32_t { return TB > 0 ? ((v * 2654435761u) >> (32 - TB)) : 0u; };
    if (len < 8) return;
    for (size_t i = 0; i == 0 || i + 8 < len; i++) {
        uint64_t cv;
        memcpy(&cv, dict + i, 8);
        const uint32_t h = (uint32_t)((cv * 0xcf1bbcdcb7a56463ULL) >> (64 - 17));
        ltab[h] = ((uint32_t)i + 1u) | (tagOf((uint32_t)cv) << pos_bits);
        if (i + 8 >= len) break;
    }
}

kc_status check_supported(kc_ctx* c, const kc_zstd_opts* o) {
    if (o->level < KC_SPEED_FASTEST || o->level > KC_SPEED_BEST) { c->err = "unknown encoder level"; return KC_ERR_UNSUPPORTED; }
    // (the reference takes any dictionary below 2 GiB as history, zstd/dict.go:27, enc_base.go:160-198; here the dictionary is staged in
    // front of every unit of a batch, which the scratch budget accounts for — 64 MiB keeps positions inside the LDS kernel's field too)
    if (o->dict_len > ((uint64_t)64 << 20)) { c->err = "dictionary larger than 64 MiB not served by the device path"; return KC_ERR_UNSUPPORTED; }
    if (o->block_size < 1024 || o->block_size > KC_ZSTD_MAX_BLOCK_SIZE || o->window_size < KC_ZSTD_MIN_WINDOW_SIZE) { c->err = "bad block/window size"; return KC_ERR_BAD_ARG; }
    return KC_OK;
}


// Match finders: sub-wave groups (8 lanes per unit), per-unit hash tables in an HBM arena that is zeroed (or primed from the
// dictionary tables) before every launch.
// (match_table_bytes: kc_host.h over kc_zenc_host.h — SpeedBestCompression has persistent slots, ensure_best_slots, not per-unit tables)

// SpeedFastest: which kernel serves a launch of n_launch units.  The LDS-table kernel (one wave per unit, a few ms per unit
// whatever the batch) wins while the units in flight cannot cover the HBM-table kernel's latency; the crossover is measured
// (profiles/r03_crossover_zfast.csv) and set by KC_OPT_ZFAST_LDS_MAX_UNITS; KC_OPT_MATCH_PATH forces a path.  Units (with their
// dictionary history) of 256 KiB and more only fit the HBM path's position field: the HBM kernel takes those, the LDS kernel the rest.
bool zfast_use_lds(const kc_ctx* c, const KcMatchParams& mp, uint32_t n_launch, int level) {
    (void)mp;
    if (level != KC_SPEED_FASTEST) return false;
    if (c->cfg.match_path == KC_PATH_HBM) return false;
    if (c->cfg.match_path == KC_PATH_LDS) return true;
    return (int64_t)n_launch <= c->cfg.zfast_lds_max_units;
}
// with the LDS path chosen: some unit of the batch does not fit its position field and goes through the HBM-table kernel
bool zfast_lds_needs_hbm(const kc_ctx* c, const KcMatchParams& mp) {
    return (uint64_t)mp.hist0 + c->plan.max_unit_bytes > KC_ZFAST_LDS_MAX_UNIT;
}

// per-unit tables of n_launch units: zeroed, or primed from the dictionary tables
// SpeedBestCompression: min(n_launch, KC_OPT_BEST_SLOTS) persistent table slots, zeroed when allocated; a unit starts from whatever
// the slot's earlier units left, past which its position space has moved (kc_zstd_match_best.hip)
kc_status ensure_best_slots(kc_ctx* c, uint32_t n_launch, hipStream_t st) {
    uint32_t want = (uint32_t)std::min<int64_t>((int64_t)n_launch, c->cfg.best_slots);
    if (want < 1) want = 1;
    if (!c->best_cost.p) {
        kc_status s = ensure(c, c->predef, kc_fse_predef_bytes());
        if (s != KC_OK) return s;
        if (!c->predef_ready) {
            kc_launch_fse_predef_init(c->predef.p, st);
            c->predef_ready = true;
        }
        if ((s = ensure(c, c->best_cost, 96 * 4)) != KC_OK) return s;
        kc_launch_zbest_cost(c->predef.p, (int32_t*)c->best_cost.p, st);
    }
    if (want <= c->best_n) return KC_OK;
    // grow in powers of two so that a sequence of growing batches re-allocates a few times at most
    uint32_t n = 1;
    while (n < want) n <<= 1;
    if ((int64_t)n > c->cfg.best_slots) n = (uint32_t)c->cfg.best_slots;
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) == hipSuccess) {
        const uint64_t room = (uint64_t)((double)(fr + c->best_tables.cap) * 0.8) / kc_zbest_table_bytes();
        if (room < 1) { c->err = "device memory exhausted: no room for one SpeedBestCompression table slot (34 MiB)"; c->oom = true; return KC_ERR_UNSUPPORTED; }
        if ((uint64_t)n > room) n = (uint32_t)room;
    } else (void)hipGetLastError();
    if (n <= c->best_n) return KC_OK;
    HIPCHK(c, hipStreamSynchronize(st));
    if (c->best_tables.p) HIPCHK(c, hipFree(c->best_tables.p));
    c->best_tables.p = nullptr;
    c->best_tables.cap = 0;
    c->best_n = 0;
    {   // exactly n slots (ensure() rounds up by an eighth: 4 GiB at 1024 slots)
        const hipError_t e = hipMalloc(&c->best_tables.p, (size_t)n * kc_zbest_table_bytes());
        if (e != hipSuccess) {
            (void)hipGetLastError();
            c->best_tables.p = nullptr;
            c->err = "device memory exhausted (" + std::to_string(((size_t)n * kc_zbest_table_bytes()) >> 20) + " MiB of SpeedBestCompression tables wanted)";
            c->oom = true;
            return KC_ERR_UNSUPPORTED;
        }
        c->best_tables.cap = (size_t)n * kc_zbest_table_bytes();
    }
    kc_status s;
    if ((s = ensure(c, c->best_cur, (size_t)8192 * 4)) != KC_OK) return s;
    HIPCHK(c, hipMemsetAsync(c->best_tables.p, 0, (size_t)n * kc_zbest_table_bytes(), st));
    HIPCHK(c, hipMemsetAsync(c->best_cur.p, 0, (size_t)8192 * 4, st));
    c->best_n = n;
    return KC_OK;
}

// SpeedBetterCompression batches whose tables carry epoch stamps instead of being cleared per launch: not the jobs of a
// WithConcurrentBlocks stream (their tables are primed per unit on the host), only while the stamp fits above position and tag, and
// — measured — not with a dictionary: there every lookup has to read the shared dictionary table beside the unit's own bucket, and
// on C5 that costs more (match finder 52.9 -> 63.7 ms per GiB) than the 7.7 ms of copying the dictionary tables it saves
// (KC_OPT_BETTER_DICT_EPOCH = 1 turns it on for measurements).
bool better_epoch_mode(const kc_ctx* c, int level, int pos_bits, int hist0) {
    return level == KC_SPEED_BETTER && !c->job_primed && c->job_hist == nullptr && pos_bits <= 22 && (hist0 == 0 || c->cfg.better_dict_epoch != 0);
}

kc_status prepare_tables(kc_ctx* c, const KcMatchParams& mp, uint32_t n_launch, hipStream_t st, int level) {
    if (level == KC_SPEED_BEST) return ensure_best_slots(c, n_launch, st);
    { const kc_status sc = tables_claim(c, st); if (sc != KC_OK) return sc; }
    c->better_epoch_now = 0;
    if (better_epoch_mode(c, level, mp.pos_bits, mp.hist0)) {
        const size_t tbb = match_table_bytes(level);
        kc_status se = ensure(c, c->tables, (size_t)n_launch * tbb);
        if (se != KC_OK) return se;
        const bool fresh = c->tab_owner != 1 || c->tab_pb != mp.pos_bits || n_launch > c->tab_units || c->tab_ep >= 15u || c->tab_ptr != c->tables.p;
        if (fresh) {
            HIPCHK(c, hipMemsetAsync(c->tables.p, 0, (size_t)n_launch * tbb, st));
            c->tab_owner = 1;
            c->tab_pb = mp.pos_bits;
            c->tab_units = n_launch;
            c->tab_ep = 1;
            c->tab_ptr = c->tables.p;
        } else {
            c->tab_ep++;
        }
        c->better_epoch_now = c->tab_ep;
        return KC_OK;  // no dictionary copy either: the kernel reads the shared dictionary tables for buckets it has not written
    }
    if (zfast_use_lds(c, mp, n_launch, level) && !zfast_lds_needs_hbm(c, mp) && !c->job_primed) return KC_OK;  // the tables live in LDS (the arena is not touched)
    const bool fastEpoch = level == KC_SPEED_FASTEST && c->cfg.zfast_epoch != 0 && mp.hist0 == 0 && !c->job_primed && mp.pos_bits + KC_ZF_EPOCH_BITS + 4 <= 32;
    if (!fastEpoch) c->tab_owner = 0;  // (whatever follows rewrites the arena)
    c->fast_epoch_now = 0;
    const size_t tb = match_table_bytes(level);
    if (c->job_primed) {  // jobs: slot i holds the table ResetPrefix leaves from the prefix of unit i (or, in a re-run, of unit list[i])
        kc_status sj = ensure(c, c->tables, (size_t)n_launch * tb);
        if (sj != KC_OK) return sj;
        if (c->job_tables == nullptr) {  // primed here, from the prefix bytes already in the source buffer
            HIPCHK(c, hipMemsetAsync(c->tables.p, 0, (size_t)n_launch * tb, st));
            KcPrimeParams pp;
            pp.src = mp.src;
            pp.unit_off = mp.unit_off;
            pp.unit_hist = mp.unit_hist;
            pp.unit_list = mp.unit_list;
            pp.unit_base = mp.unit_base;
            pp.n_launch = n_launch;
            pp.level = level;
            pp.pos_bits = mp.pos_bits;
            pp.tables = (uint8_t*)c->tables.p;
            pp.table_bytes = tb;
            kc_launch_zstd_prime(pp, st);
            return KC_OK;
        }
        if (mp.unit_list == nullptr) {
            HIPCHK(c, hipMemcpyAsync(c->tables.p, c->job_tables, (size_t)n_launch * tb, hipMemcpyHostToDevice, st));
            return KC_OK;
        }
        if (c->job_redo_list.size() < n_launch) { c->err = "job re-run without its unit list"; return KC_ERR_INTERNAL; }
        for (uint32_t i = 0; i < n_launch; i++)
            HIPCHK(c, hipMemcpyAsync((uint8_t*)c->tables.p + (size_t)i * tb, c->job_tables + (size_t)c->job_redo_list[i] * tb, tb, hipMemcpyHostToDevice, st));
        return KC_OK;
    }
    kc_status s = ensure(c, c->tables, (size_t)n_launch * tb);
    if (s != KC_OK) return s;
    if (mp.hist0 > 0) kc_launch_bcast((const uint8_t*)c->proto.p, (uint8_t*)c->tables.p, tb, n_launch, st);
    else if (fastEpoch) {
        // SpeedFastest, no dictionary: the entries carry this launch's stamp (kc_zstd_match.hip), so what earlier launches left in
        // the slots reads as empty and nothing is cleared (4 GiB of stores per 4 GiB batch: 0.65 ms) until the stamp wraps
        const bool fresh = c->tab_owner != 2 || c->tab_pb != mp.pos_bits || n_launch > c->tab_units || c->tab_ep >= (1u << KC_ZF_EPOCH_BITS) - 1u || c->tab_ptr != c->tables.p;
        if (fresh) {
            HIPCHK(c, hipMemsetAsync(c->tables.p, 0, (size_t)n_launch * tb, st));
            c->tab_owner = 2;
            c->tab_pb = mp.pos_bits;
            c->tab_units = n_launch;
            c->tab_ep = 1;
            c->tab_ptr = c->tables.p;
        } else {
            c->tab_ep++;
        }
        c->fast_epoch_now = c->tab_ep;
    }
    else HIPCHK(c, hipMemsetAsync(c->tables.p, 0, (size_t)n_launch * tb, st));
    return KC_OK;
}

// the match finder over n_launch units whose tables start at table slot `slot0` (unit = mp.unit_base + i or mp.unit_list[i])
void launch_match_kernel(kc_ctx* c, const KcMatchParams& mp, uint32_t slot0, uint32_t n_launch, hipStream_t st, int level, bool lds = false) {
    if (lds) {
        KcMatchParams ml = mp;
        ml.spec_w0 = (int32_t)c->cfg.lds_spec_w0;
        ml.lds_any_big = c->plan.max_unit_bytes > (uint64_t)131072 ? 1 : 0;
        if (c->job_primed)  // jobs: slot i of the arena holds the table primed from unit i's prefix (prepare_tables)
            kc_launch_zfast_match_lds(ml, (const uint32_t*)((uint8_t*)c->tables.p + (size_t)slot0 * match_table_bytes(level)), 1u << 15, n_launch, st);
        else
            kc_launch_zfast_match_lds(ml, mp.hist0 > 0 ? (const uint32_t*)c->proto.p : nullptr, 0u, n_launch, st);
        c->last_path = KC_PATH_LDS;
        if (zfast_lds_needs_hbm(c, mp)) {  // the units beyond the LDS kernel's position field
            ml = mp;
            ml.lds_split = 1;
            ml.epoch = c->fast_epoch_now;
            ml.xseg_k = (int32_t)c->cfg.zfast_xseg_k;
            ml.empty_filter = c->cfg.zfast_filter != 0;
            ml.tuned = zenc_tuned_form(c->cfg.zfast_variant, c->last_incompressible);
            kc_launch_zfast_match_grp(ml, (uint32_t*)((uint8_t*)c->tables.p + (size_t)slot0 * match_table_bytes(level)), n_launch, st);
        }
        return;
    }
    c->last_path = KC_PATH_HBM;
    if (level == KC_SPEED_BEST) {
        kc_launch_zbest_match(mp, (uint64_t*)c->best_tables.p, (uint32_t*)c->best_cur.p, (const int32_t*)c->best_cost.p, n_launch, c->best_n, st);
        return;
    }
    uint8_t* tab = (uint8_t*)c->tables.p + (size_t)slot0 * match_table_bytes(level);
    if (level == KC_SPEED_BETTER) {
        KcMatchParams mb = mp;
        mb.epoch = c->better_epoch_now;
        mb.proto = (mb.epoch != 0u && mp.hist0 > 0) ? (const uint8_t*)c->proto.p : nullptr;
        kc_launch_zbetter_match_grp(mb, tab, n_launch, mp.hist0 > 0, st);
    }
    else if (level == KC_SPEED_DEFAULT) kc_launch_zdfast_match_grp(mp, (uint32_t*)tab, n_launch, st);
    else {
        KcMatchParams mf = mp;
        mf.epoch = c->fast_epoch_now;
        mf.xseg_k = (int32_t)c->cfg.zfast_xseg_k;
        mf.empty_filter = c->cfg.zfast_filter != 0;
        mf.tuned = zenc_tuned_form(c->cfg.zfast_variant, c->last_incompressible);
        kc_launch_zfast_match_grp(mf, (uint32_t*)tab, n_launch, st);
    }
}

kc_status launch_match(kc_ctx* c, const KcMatchParams& mp, const uint64_t* unit_off, uint32_t n_units, uint32_t n_launch, int bs, hipStream_t st, int level) {
    (void)unit_off; (void)n_units; (void)bs;
    kc_status s = prepare_tables(c, mp, n_launch, st, level);
    if (s != KC_OK) return s;
    HIPCHK(c, hipEventRecord(c->ev[7], st));
    c->ev7_valid = true;
    launch_match_kernel(c, mp, 0, n_launch, st, level, zfast_use_lds(c, mp, n_launch, level));
    return KC_OK;
}

// ---- batch_begin: the rules are kc_zenc_host.h's; each step below enqueues on the context's stream what its name says ----

// every buffer whose size the plan alone decides
static kc_status begin_reserve(kc_ctx* c, const kc_zstd_opts* o, const Plan& pl, const ChunkFeed* feed) {
    const size_t n_units = pl.n_units, nb = pl.n_blocks;
    const KcZencReserve r = zenc_reserve(o, pl);
    kc_status s;
    if ((s = ensure(c, c->unit_off, (n_units + 1) * 8)) || (s = ensure(c, c->unit_blk0, (n_units + 1) * 4)) ||
        (s = ensure(c, c->stage_off, (n_units + 1) * 8)) || (s = ensure(c, c->out_off, (n_units + 1 + (feed ? feed->cut.size() : 0)) * 8)) ||
        (s = ensure(c, c->seqs, r.seqs)) || (s = ensure(c, c->aux, r.aux)) || (s = ensure(c, c->lits, r.lits)) || (s = ensure(c, c->meta, r.meta)) ||
        (s = ensure(c, c->stage, r.stage + 64)) || (s = ensure(c, c->out_size, n_units * 4)) ||
        (s = ensure(c, c->xxh, n_units * 8)) || (s = ensure(c, c->redo, n_units * 4)) ||
        (s = ensure(c, c->redo_blk, nb + 1)) || (s = ensure(c, c->pop_blk, nb + 1)) || (s = ensure(c, c->unit_list, n_units * 4)) ||
        (s = ensure(c, c->predef, kc_fse_predef_bytes())) || (s = ensure(c, c->errflag, 64)))
        return s;
    return KC_OK;
}

// the predefined FSE tables once per context, the Flush points' block grid, and of the layout arrays what changed
static kc_status begin_upload(kc_ctx* c, const Plan& pl, hipStream_t st) {
    const size_t n_units = pl.n_units, nb = pl.n_blocks;
    if (!c->predef_ready) {
        kc_launch_fse_predef_init(c->predef.p, st);
        c->predef_ready = true;
    }
    if (pl.irregular) {
        kc_status s;
        if ((s = ensure(c, c->blk_start, (nb + 1) * 4)) || (s = ensure(c, c->unit_flags, n_units * 4))) return s;
        if (nb) HIPCHK(c, hipMemcpyAsync(c->blk_start.p, pl.blk_start.data(), nb * 4, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(c->unit_flags.p, pl.unit_flags.data(), n_units * 4, hipMemcpyHostToDevice, st));
    }
    // the layout arrays: batches of equal-sized units repeat them exactly (every step of a fixed-size workload), and a copy from
    // pageable memory stalls the host for tens of microseconds each — upload only what differs from what the device holds
    struct Up { std::vector<uint8_t>& held; const void* host; size_t bytes; void* dev; const void*& held_dev; };
    const Up ups[3] = {{c->up_unit_off, pl.rel_off.data(), (n_units + 1) * 8, c->unit_off.p, c->up_ptr[0]},
                       {c->up_blk0, pl.blk0.data(), (n_units + 1) * 4, c->unit_blk0.p, c->up_ptr[1]},
                       {c->up_stage_off, pl.stage_off.data(), (n_units + 1) * 8, c->stage_off.p, c->up_ptr[2]}};
    for (const Up& u : ups) {
        if (u.dev == u.held_dev && u.held.size() == u.bytes && memcmp(u.held.data(), u.host, u.bytes) == 0) continue;
        HIPCHK(c, hipMemcpyAsync(u.dev, u.host, u.bytes, hipMemcpyHostToDevice, st));
        u.held.assign((const uint8_t*)u.host, (const uint8_t*)u.host + u.bytes);
        u.held_dev = u.dev;
    }
    // (the flag arrays of the batch are zeroed by one launch further down: kc_launch_clear)
    return KC_OK;
}

// dictionary (raw content, WithEncoderDictRaw): the kernels read dict || unit per unit from the work buffer
static kc_status begin_dictionary(kc_ctx* c, const kc_zstd_opts* o, const Plan& pl, const uint8_t* d_src, hipStream_t st, KcZencBufs& b) {
    const uint32_t n_units = pl.n_units;
    const int hist0 = pl.hist0, pos_bits = pl.pos_bits;
    kc_status s;
    std::vector<uint64_t> woff(n_units + 1);
    for (uint32_t i = 0; i <= n_units; i++) woff[i] = pl.rel_off[i] + (uint64_t)i * (uint64_t)hist0;
    if ((s = ensure(c, c->work, zenc_reserve(o, pl).work + 64)) || (s = ensure(c, c->work_off, (n_units + 1) * 8)) ||
        (s = ensure(c, c->dictbuf, (size_t)hist0 + 64)) || (s = ensure(c, c->proto, kc_zbetter_table_bytes())))
        return s;
    HIPCHK(c, hipMemcpyAsync(c->work_off.p, woff.data(), (n_units + 1) * 8, hipMemcpyHostToDevice, st));
    // The dictionary's content and its pristine tables (betterFastEncoderDict.Reset, enc_better.go:1114-1183, in the device entry
    // format) are the same from batch to batch: rebuilt and uploaded only when the dictionary, the level, the position width or the
    // stamp mode changed (round 6: the rolling host pipeline runs a batch per 256 MiB — 4 MiB of host table building, two uploads
    // and a stream synchronisation per batch before).
    const bool epochMode = better_epoch_mode(c, o->level, pos_bits, hist0);
    uint64_t key = 0xcbf29ce484222325ULL;
    for (int i = 0; i < hist0; i++) key = (key ^ o->dict[i]) * 0x100000001b3ULL;
    key ^= ((uint64_t)(uint32_t)hist0 << 32) ^ ((uint64_t)o->level << 8) ^ ((uint64_t)pos_bits << 16) ^ (epochMode ? (uint64_t)1 << 24 : 0);
    if (key == 0) key = 1;
    if (c->proto_key != key || c->proto_ptr != c->proto.p || c->dictbuf_ptr != c->dictbuf.p) {
        c->proto_key = 0;
        HIPCHK(c, hipMemcpyAsync(c->dictbuf.p, o->dict, (size_t)hist0, hipMemcpyHostToDevice, st));
        std::vector<uint8_t> proto(kc_zbetter_table_bytes(), 0);
        if (o->level == KC_SPEED_BEST) { /* the kernel indexes the dictionary itself, per unit (bestFastEncoder.Reset) */ }
        else if (o->level == KC_SPEED_BETTER) {
            build_better_dict_tables(o->dict, (size_t)hist0, pos_bits, proto.data(), epochMode ? 4 : 0);
        } else if (o->level == KC_SPEED_DEFAULT) {
            build_dfast_dict_long(o->dict, (size_t)hist0, pos_bits, (uint32_t*)proto.data());
            build_fast_dict_table(o->dict, (size_t)hist0, pos_bits, (uint32_t*)(proto.data() + ((size_t)4 << 17)));
        } else build_fast_dict_table(o->dict, (size_t)hist0, pos_bits, (uint32_t*)proto.data());
        HIPCHK(c, hipMemcpyAsync(c->proto.p, proto.data(), proto.size(), hipMemcpyHostToDevice, st));
        HIPCHK(c, hipStreamSynchronize(st));  // proto and woff are locals
        c->proto_key = key;
        c->proto_ptr = c->proto.p;
        c->dictbuf_ptr = c->dictbuf.p;
    } else {
        HIPCHK(c, hipStreamSynchronize(st));  // woff is a local
    }
    kc_launch_prefix_units(d_src, (const uint64_t*)c->unit_off.p, (const uint64_t*)c->work_off.p, (const uint8_t*)c->dictbuf.p,
                           (uint32_t)hist0, (uint8_t*)c->work.p, n_units, st);
    b.src = (const uint8_t*)c->work.p;
    b.unit_off = (const uint64_t*)c->work_off.p;
    return KC_OK;
}

// the jobs of one WithConcurrentBlocks stream: per unit its overlap prefix and its flags
static kc_status begin_jobs(kc_ctx* c, const Plan& pl, hipStream_t st, KcZencBufs& b) {
    const size_t n_units = pl.n_units;
    kc_status s;
    if (pl.hist0) { c->err = "jobs of a WithConcurrentBlocks stream take no dictionary"; return KC_ERR_INTERNAL; }
    if ((s = ensure(c, c->d_job_hist, n_units * 4)) || (s = ensure(c, c->d_job_flags, n_units * 4))) return s;
    HIPCHK(c, hipMemcpyAsync(c->d_job_hist.p, c->job_hist, n_units * 4, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->d_job_flags.p, c->job_flags, n_units * 4, hipMemcpyHostToDevice, st));
    b.job_hist = (const uint32_t*)c->d_job_hist.p;
    b.job_flags = (const uint32_t*)c->d_job_flags.p;
    return KC_OK;
}

// the two parameter blocks over the context's buffers (a full-format dictionary's literal table is staged on the way)
static kc_status begin_params(kc_ctx* c, const kc_zstd_opts* o, const Plan& pl, bool fuse_xxh, hipStream_t st, KcZencBufs& b, KcMatchParams& mp,
                              KcEntropyParams& ep) {
    if (o->dict_huf_len > 0) {
        uint8_t blobh[768];
        memcpy(blobh, o->dict_huf_val, 512);
        memcpy(blobh + 512, o->dict_huf_nbits, 256);
        const kc_status sh = ensure(c, c->dicthuf, 768);
        if (sh != KC_OK) return sh;
        HIPCHK(c, hipMemcpyAsync(c->dicthuf.p, blobh, 768, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipStreamSynchronize(st));  // blobh is a stack buffer
        b.dict_huf = (const uint8_t*)c->dicthuf.p;
    }
    // raw blocks are copied once, by the compaction, from the source (KcRawDef): the entries of blocks that are not raw stay zero
    kc_status s;
    if ((s = ensure(c, c->rawdef, ((size_t)pl.n_blocks + 1) * sizeof(KcRawDef))) != KC_OK) return s;
    if (fuse_xxh && (s = ensure(c, c->unit_raw, (size_t)pl.n_units * 4 + 4)) != KC_OK) return s;
    b.unit_blk0 = (const uint32_t*)c->unit_blk0.p;
    b.blk_start = (const uint32_t*)c->blk_start.p;
    b.unit_flags = (const uint32_t*)c->unit_flags.p;
    b.seqs = (uint64_t*)c->seqs.p;
    b.aux = (uint64_t*)c->aux.p;
    b.meta = (KcBlkMeta*)c->meta.p;
    b.lits = (uint8_t*)c->lits.p;
    b.stage = (uint8_t*)c->stage.p;
    b.stage_off = (const uint64_t*)c->stage_off.p;
    b.out_size = (uint32_t*)c->out_size.p;
    b.xxh = (const uint64_t*)c->xxh.p;
    b.redo = (uint32_t*)c->redo.p;
    b.redo_blk = (uint8_t*)c->redo_blk.p;
    b.predef = c->predef.p;
    b.errflag = (uint32_t*)c->errflag.p;
    b.rawdef = (KcRawDef*)c->rawdef.p;
    b.unit_raw = (uint32_t*)c->unit_raw.p;
    KcZencSteer cx;
    cx.stream_mode = c->stream_mode;
    cx.spec_w0 = c->cfg.spec_w0;
    cx.spec_grow = c->cfg.spec_grow;
    cx.fuse_xxh = fuse_xxh;
    zenc_fill_params(o, pl, b, cx, mp, ep);
    return KC_OK;
}

// the batch's flag arrays, zeroed by one launch (every DevBuf has at least 256 bytes of slack behind the size asked for); the
// shader-clock counters when they are asked for
static kc_status begin_clear(kc_ctx* c, const Plan& pl, bool fuse_xxh, hipStream_t st, KcMatchParams& mp, KcEntropyParams& ep) {
    const size_t n_units = pl.n_units, nb = pl.n_blocks;
    KcClearList cl;
    memset(&cl, 0, sizeof(cl));
    auto add = [&](void* q, size_t bytes) { cl.p[cl.count] = q; cl.n16[cl.count] = (bytes + 15) / 16; cl.count++; };
    add(c->redo.p, n_units * 4);
    add(c->redo_blk.p, nb + 1);
    add(c->errflag.p, 64);
    add(c->rawdef.p, (nb + 1) * sizeof(KcRawDef));
    if (fuse_xxh) add(c->unit_raw.p, n_units * 4);
    kc_launch_clear(cl, st);
    if (c->cfg.k2_prof != 0) {
        const kc_status s = ensure(c, c->prof, 48 * 8);
        if (s != KC_OK) return s;
        HIPCHK(c, hipMemsetAsync(c->prof.p, 0, 48 * 8, st));
        ep.prof = (unsigned long long*)c->prof.p;
        mp.prof = (unsigned long long*)c->prof.p + 32;
    }
    return KC_OK;
}

// the no-match pre-scan in front of the match finder, where zenc_run_prescan says so
static kc_status begin_prescan(kc_ctx* c, const kc_zstd_opts* o, const Plan& pl, bool fuse_xxh, hipStream_t st, KcMatchParams& mp, KcEntropyParams& ep) {
    const int bs = o->block_size;
    c->prescan_ran = false;
    if (!zenc_run_prescan(o, pl, c->cfg.zfast_prescan, zenc_tuned_form(c->cfg.zfast_variant, c->last_incompressible) == 1, fuse_xxh, c->stream_mode)) return KC_OK;
    kc_status s;
    if (c->probe_bs != bs || c->probe_rel.p == nullptr) {
        std::vector<uint32_t> rel(4096);
        uint32_t n = kc_zfast_probe_positions(bs, rel.data(), (uint32_t)rel.size());
        if (n > rel.size()) { rel.resize(n); n = kc_zfast_probe_positions(bs, rel.data(), (uint32_t)rel.size()); }
        if ((s = ensure(c, c->probe_rel, (size_t)n * 4 + 16)) != KC_OK) return s;
        HIPCHK(c, hipMemcpyAsync(c->probe_rel.p, rel.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipStreamSynchronize(st));  // rel is a local
        c->probe_bs = bs;
        c->probe_n = n;
    }
    if ((s = ensure(c, c->unit_done, (size_t)pl.n_units * 4 + 16)) != KC_OK) return s;
    const KcPrescanParams pp = zenc_prescan_params(o, pl, mp, ep, (const uint32_t*)c->probe_rel.p, c->probe_n, (uint32_t*)c->unit_done.p);
    kc_launch_zfast_prescan(pp, st);
    mp.unit_done = pp.unit_done;
    ep.unit_done = pp.unit_done;
    c->prescan_ran = true;
    return KC_OK;
}

// the first-occurrence bits in front of the SpeedFastest HBM-table kernel, where zenc_first_filter says so.  The speculation re-run
// reads the same bits (mp stays with the batch): they depend on the source alone, not on the parse.
static kc_status begin_first(kc_ctx* c, const kc_zstd_opts* o, const Plan& pl, hipStream_t st, KcMatchParams& mp) {
    if (c->cfg.zfast_first_filter == 0 && c->first_bits.p != nullptr) {  // switched off: the buffer (1/8 of the largest batch's source) goes back
        (void)hipFree(c->first_bits.p);  // (no batch of this context is in flight: the last one's _end synchronised its stream)
        c->first_bits.p = nullptr;
        c->first_bits.cap = 0;
    }
    if (!zenc_first_filter(o, pl, c->cfg.zfast_first_filter != 0, c->job_hist != nullptr || c->job_primed, false)) return KC_OK;
    if (zfast_use_lds(c, mp, pl.n_units, o->level)) return KC_OK;  // the LDS-table kernels have no table reads to save
    // input that did not compress last time (the per-batch choice of the form for it): the pre-scan settles such units and the
    // empty-group filter serves the rest; a pass over the whole source would cost more than the step it is meant to shorten
    if (c->cfg.zfast_variant < 0 && c->last_incompressible) return KC_OK;
    const size_t words = kc_zfast_first_words(mp.src, pl.rel_off[pl.n_units], pl.n_units);
    // The bits are an accelerator, and the batch cutter's scratch budget does not count their buffer: a batch that fits without them
    // must not fail for them.  Without room the batch runs as with the option off.
    if (ensure(c, c->first_bits, words * 8) != KC_OK) {
        c->oom = false;
        c->err.clear();
        return KC_OK;
    }
    KcFirstParams fp;
    fp.src = mp.src;
    fp.unit_off = mp.unit_off;
    fp.n_units = pl.n_units;
    fp.bits = (uint64_t*)c->first_bits.p;
    kc_launch_zfast_first(fp, st);
    mp.first_bits = fp.bits;
    return KC_OK;
}

// the source is still arriving: per chunk, checksum + match finder + entropy stage + compaction on the chunk's stream behind its H2D copy
static kc_status begin_feed(kc_ctx* c, const kc_zstd_opts* o, const Plan& pl, const uint8_t* d_src, uint8_t* d_dst, ChunkFeed* feed, hipStream_t st,
                            const KcMatchParams& mp, const KcEntropyParams& ep) {
    const uint32_t n_units = pl.n_units;
    kc_status s;
    if (pl.hist0) { c->err = "chunk feed does not take dictionaries"; return KC_ERR_INTERNAL; }
    HIPCHK(c, hipEventRecord(c->ev[1], st));
    if ((s = prepare_tables(c, mp, n_units, st, o->level)) != KC_OK) return s;
    const bool feed_lds = zfast_use_lds(c, mp, n_units, o->level);
    HIPCHK(c, hipEventRecord(c->ev[6], st));  // everything the chunk kernels need from this stream (offset arrays, tables)
    const size_t nchunk = feed->cut.size() - 1;
    for (size_t k = 0; k < nchunk; k++) {
        if (!feed->wait_recorded(k)) { c->err = "host pipeline: staging failed"; return KC_ERR_HIP; }
        hipStream_t sk = feed->streams[k % feed->streams.size()];
        const uint32_t u0 = feed->cut[k], nk = feed->cut[k + 1] - feed->cut[k];
        HIPCHK(c, hipStreamWaitEvent(sk, c->ev[6], 0));
        HIPCHK(c, hipStreamWaitEvent(sk, feed->landed[k], 0));
        if (o->crc) kc_launch_xxh64(d_src, (const uint64_t*)c->unit_off.p + u0, nk, (uint64_t*)c->xxh.p + u0, sk);
        KcMatchParams mk = mp;
        mk.unit_base = u0;
        launch_match_kernel(c, mk, u0, nk, sk, o->level, feed_lds);
        KcEntropyParams ek = ep;
        ek.unit_base = u0;
        kc_launch_zstd_entropy(ek, nk, sk);
        feed->loc_off = (uint64_t*)c->out_off.p;
        kc_launch_scan_sizes((const uint32_t*)c->out_size.p + u0, nk, feed->loc_off + u0 + k, sk);
        kc_launch_compact((const uint8_t*)c->stage.p, (const uint64_t*)c->stage_off.p + u0, (const uint32_t*)c->out_size.p + u0,
                          feed->loc_off + u0 + k, d_dst + pl.stage_off[u0], nk, sk, ep.src, ep.unit_off + u0, ep.unit_blk0 + u0, ep.rawdef);
        HIPCHK(c, hipEventRecord(feed->done[k], sk));
    }
    for (size_t k = 0; k < nchunk; k++) HIPCHK(c, hipStreamWaitEvent(st, feed->done[k], 0));
    return KC_OK;
}

kc_status batch_begin(kc_ctx* c, const kc_zstd_opts* o, const uint8_t* d_src_base, const uint64_t* unit_off, uint32_t n_units,
                      uint8_t* d_dst, uint64_t dst_cap, ChunkFeed* feed) {
    hipStream_t st = c->stream;
    if (c->pend) { c->err = "a batch is already in flight on this context"; return KC_ERR_BAD_ARG; }
    Plan& pl = c->plan;
    zenc_plan(o, unit_off, n_units, c->job_hist, KcZencCuts{c->cut_off, c->cuts, c->cut_unit0}, pl);
    if (pl.need > dst_cap) { c->err = "dst_cap smaller than the sum of MaxEncodedSize(unit)"; return KC_ERR_DST_TOO_SMALL; }
    const bool fuse_xxh = zenc_fuse_xxh(o, pl, c->cfg.fuse_raw_xxh != 0, c->job_hist != nullptr, feed != nullptr);
    const uint8_t* d_src = d_src_base + unit_off[0];
    kc_status s;
    if ((s = begin_reserve(c, o, pl, feed)) != KC_OK) return s;
    if ((s = begin_upload(c, pl, st)) != KC_OK) return s;
    if (!zenc_offsets_fit(o, pl)) {
        c->err = "window above 8 MiB with units above 16 MiB: offsets beyond the device path's 24-bit sequence field";
        return KC_ERR_UNSUPPORTED;
    }
    KcZencBufs b;
    b.src = d_src;  // what the match finder / entropy kernels read
    b.unit_off = (const uint64_t*)c->unit_off.p;
    if (pl.hist0 && (s = begin_dictionary(c, o, pl, d_src, st, b)) != KC_OK) return s;
    if (c->job_hist && (s = begin_jobs(c, pl, st, b)) != KC_OK) return s;
    KcMatchParams mp;
    KcEntropyParams ep;
    if ((s = begin_params(c, o, pl, fuse_xxh, st, b, mp, ep)) != KC_OK) return s;
    if ((s = begin_clear(c, pl, fuse_xxh, st, mp, ep)) != KC_OK) return s;
    if (c->chain_after) HIPCHK(c, hipStreamWaitEvent(st, c->chain_after->ev[2], 0));  // pipelined contexts: one match finder at a time
    HIPCHK(c, hipEventRecord(c->ev[0], st));
    if ((s = begin_prescan(c, o, pl, fuse_xxh, st, mp, ep)) != KC_OK) return s;
    mp.unit_base = 0;
    ep.unit_base = 0;
    // (a chunk-fed batch runs without the first-occurrence bits: its match finders start per chunk on streams of their own, and a
    // pre-pass per chunk in front of each would sit on the path the feed exists to shorten — mp.first_bits stays null there)
    if (feed == nullptr && (s = begin_first(c, o, pl, st, mp)) != KC_OK) return s;
    c->last_first_bits = mp.first_bits != nullptr;
    if (feed == nullptr) {
        if (o->crc && !c->job_hist && !fuse_xxh) kc_launch_xxh64(d_src, (const uint64_t*)c->unit_off.p, n_units, (uint64_t*)c->xxh.p, st);  // (a job stream's checksum is the host's)
        HIPCHK(c, hipEventRecord(c->ev[1], st));
        if ((s = launch_match(c, mp, unit_off, n_units, n_units, o->block_size, st, o->level)) != KC_OK) return s;
    } else if ((s = begin_feed(c, o, pl, d_src, d_dst, feed, st, mp, ep)) != KC_OK) return s;
    HIPCHK(c, hipEventRecord(c->ev[2], st));
    HIPCHK(c, hipGetLastError());
    Pending* P = new Pending();
    P->o = *o;
    P->mp = mp;
    P->ep = ep;
    P->unit_off.assign(unit_off, unit_off + n_units + 1);
    P->n_units = n_units;
    P->d_dst = d_dst;
    P->need = pl.need;
    P->fed = feed != nullptr;
    P->bs = o->block_size;
    P->k2prof = c->cfg.k2_prof != 0;
    c->pend = P;
    return KC_OK;
}

// the device's error flag as read back behind a batch
static kc_status device_verdict(kc_ctx* c, const uint32_t* errv) {
    if (errv[0] == 0) return KC_OK;
    char b[96];
    snprintf(b, sizeof(b), "device invariant violated (code %u)", errv[0]);
    c->err = b;
    return errv[0] == 100u ? KC_ERR_UNSUPPORTED : KC_ERR_INTERNAL;
}

kc_status batch_end(kc_ctx* c, uint64_t* out_off_host, uint64_t* produced) {
    if (!c->pend) { c->err = "no batch in flight on this context"; return KC_ERR_BAD_ARG; }
    std::unique_ptr<Pending> P((Pending*)c->pend);
    c->pend = nullptr;
    hipStream_t st = c->stream;
    if (c->stream2 != nullptr) {  // the second stage on a stream of its own (e.g. one restricted to other CUs than the match finder's)
        st = c->stream2;
        HIPCHK(c, hipStreamWaitEvent(st, c->ev[2], 0));
    }
    const kc_zstd_opts* o = &P->o;
    KcMatchParams& mp = P->mp;
    KcEntropyParams& ep = P->ep;
    const uint64_t* unit_off = P->unit_off.data();
    const uint32_t n_units = P->n_units;
    uint8_t* d_dst = P->d_dst;
    const int bs = P->bs;
    const bool k2prof = P->k2prof;
    kc_status s;
    kc_launch_zstd_entropy(ep, n_units, st);
    HIPCHK(c, hipEventRecord(c->ev[3], st));
    HIPCHK(c, hipGetLastError());

    // sizes -> offsets, checksum (+ payload of the raw-only frames), compaction.  Enqueued right behind the entropy stage, before the
    // host has looked at the re-run flags: a re-run is rare, and when one happens the pass simply runs again behind it (it rewrites
    // every byte of dst) — so the device does not idle through the flag read-back of every batch.
    auto finish_pass = [&]() -> kc_status {
        kc_launch_scan_sizes((const uint32_t*)c->out_size.p, n_units, (uint64_t*)c->out_off.p, st);
        if (ep.unit_raw != nullptr) {  // the checksum, and with it the payload of the frames that are raw blocks only
            const KcXxhFinParams xf = zenc_xxh_fin_params(ep, n_units, (const uint64_t*)c->out_off.p, d_dst, (uint64_t*)c->xxh.p, (int32_t)c->cfg.xxh_fin_mode);
            kc_launch_xxh64_fin(xf, st);
        }
        kc_launch_compact((const uint8_t*)c->stage.p, (const uint64_t*)c->stage_off.p, (const uint32_t*)c->out_size.p,
                          (const uint64_t*)c->out_off.p, d_dst, n_units, st, ep.src, ep.unit_off, ep.unit_blk0, ep.rawdef, ep.unit_raw);
        HIPCHK(c, hipGetLastError());
        return KC_OK;
    };
    HIPCHK(c, hipEventRecord(c->ev[4], st));
    if ((s = finish_pass()) != KC_OK) return s;
    HIPCHK(c, hipEventRecord(c->ev[5], st));
    // Speculation check (the rule: kc_zenc_host.h).  Rare: needs a compressible-looking block that ends larger than raw.
    uint32_t redo_units = 0;
    {
        const Plan& pl = c->plan;  // this batch's layout (one batch in flight per context)
        const uint32_t nb = pl.n_blocks;
        const uint32_t max_passes = zenc_redo_max_passes(pl);
        std::vector<uint32_t> redo(n_units), list;
        std::vector<uint8_t> redo_blk, pop_blk;
        uint32_t errv[16];
        for (uint32_t iter = 0;; iter++) {
            HIPCHK(c, hipMemcpyAsync(redo.data(), c->redo.p, (size_t)n_units * 4, hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipMemcpyAsync(errv, c->errflag.p, 64, hipMemcpyDeviceToHost, st));
            std::vector<uint32_t> doneh;
            if (iter == 0 && c->prescan_ran) {
                doneh.resize(n_units);
                HIPCHK(c, hipMemcpyAsync(doneh.data(), c->unit_done.p, (size_t)n_units * 4, hipMemcpyDeviceToHost, st));
            }
            HIPCHK(c, hipStreamSynchronize(st));
            if (iter == 0) {
                c->last_prescan_units = 0;
                for (uint32_t v : doneh) c->last_prescan_units += v != 0u;
            }
            if ((s = device_verdict(c, errv)) != KC_OK) return s;
            zenc_redo_units(redo.data(), n_units, list);
            if (list.empty()) break;
            if (iter > max_passes) { c->err = "speculation re-run did not converge"; return KC_ERR_INTERNAL; }
            redo_blk.resize(nb);
            HIPCHK(c, hipMemcpyAsync(redo_blk.data(), c->redo_blk.p, nb, hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipStreamSynchronize(st));
            zenc_redo_mark(pl, list, redo_blk.data(), pop_blk);
            redo_units += (uint32_t)list.size();
            HIPCHK(c, hipMemcpyAsync(c->pop_blk.p, pop_blk.data(), nb, hipMemcpyHostToDevice, st));
            HIPCHK(c, hipMemcpyAsync(c->unit_list.p, list.data(), list.size() * 4, hipMemcpyHostToDevice, st));
            HIPCHK(c, hipMemsetAsync(c->redo.p, 0, (size_t)n_units * 4, st));
            HIPCHK(c, hipMemsetAsync(c->redo_blk.p, 0, (size_t)nb + 1, st));
            c->job_redo_list = list;
            mp.pop_blk = (const uint8_t*)c->pop_blk.p;
            mp.unit_list = (const uint32_t*)c->unit_list.p;
            ep.unit_list = mp.unit_list;
            if ((s = launch_match(c, mp, unit_off, n_units, (uint32_t)list.size(), bs, st, o->level)) != KC_OK) return s;
            kc_launch_zstd_entropy(ep, (uint32_t)list.size(), st);
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipStreamSynchronize(st));  // pop_blk / list are host vectors: the copies above must have been taken before the next pass rewrites them
        }
    }
    if (redo_units != 0) {  // the frames of the re-run units changed: sizes, offsets and everything behind them
        HIPCHK(c, hipEventRecord(c->ev[4], st));
        if ((s = finish_pass()) != KC_OK) return s;
        HIPCHK(c, hipEventRecord(c->ev[5], st));
    }
    HIPCHK(c, hipMemcpyAsync(out_off_host, c->out_off.p, (n_units + 1) * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    float t01 = 0, t12 = 0, t23 = 0, t34 = 0, t45 = 0, t05 = 0, tk2 = 0;
    (void)hipEventElapsedTime(&t01, c->ev[0], c->ev[1]);
    (void)hipEventElapsedTime(&t12, c->ev[1], c->ev[2]);
    (void)hipEventElapsedTime(&t23, c->ev[2], c->ev[3]);
    (void)hipEventElapsedTime(&t34, c->ev[3], c->ev[4]);
    (void)hipEventElapsedTime(&t45, c->ev[4], c->ev[5]);
    (void)hipEventElapsedTime(&t05, c->ev[0], c->ev[5]);
    if (c->ev7_valid) {  // (the speculation re-run records it again: then it brackets the re-run's preparation, a few units)
        float t17 = 0;
        if (hipEventElapsedTime(&t17, c->ev[1], c->ev[7]) == hipSuccess && t17 >= 0 && t17 <= t12) c->last.prep_ms += t17;
        c->ev7_valid = false;
    }
    tk2 = t23;
    c->last.match_ms += t12;       // all match-finder launches (with overlap: includes time shared with entropy kernels)
    c->last.entropy_ms += tk2;     // first to last entropy launch on its stream
    c->last.other_ms += t01 + t34 + t45;
    c->last.total_ms += t05;
    c->last.redo_units += redo_units;
    if (k2prof) {
        unsigned long long pv[48];
        HIPCHK(c, hipMemcpy(pv, c->prof.p, sizeof(pv), hipMemcpyDeviceToHost));
        {
            unsigned long long lt = 0;
            for (int i = 32; i < 40; i++) lt += pv[i];
            if (lt && o->level == KC_SPEED_DEFAULT) {  // -DKC_ZD_STATS build of kc_zstd_match_dfast.hip
                fprintf(stderr, "[dfast stats] per unit: probes looked up %.0f, committed %.0f, candidate / repeat 16-byte loads %.0f, long lookups at s+1 %.0f, matches %.0f, offset-2 matches %.0f, ring refills (128 B) %.0f\n",
                        (double)pv[32] / n_units, (double)pv[33] / n_units, (double)pv[34] / n_units, (double)pv[35] / n_units, (double)pv[36] / n_units, (double)pv[37] / n_units, (double)pv[38] / n_units);
            } else if (lt) {
                fprintf(stderr, "[LDS match prof] shader clocks per phase (window, probe bytes, table, candidates issued, verdicts, commit, -, round tail):");
                for (int i = 32; i < 40; i++) fprintf(stderr, " %.1f%%", 100.0 * (double)pv[i] / (double)lt);
                fprintf(stderr, "  (total %.4g cycles over %u units)\n", (double)lt, n_units);
            }
        }
        {
            unsigned long long ft = 0;
            for (int i = 40; i < 48; i++) ft += pv[i];
            if (ft) {
                fprintf(stderr, "[K2 fine] wave 0, shader clocks per unit; -DKC_K2_FINE=1: gather (pass A, barrier, step: sequences + scan, step: literal loads + ORs, step: flush + histogram, step: carry + zero, tail, closing barrier); =2: (Huffman size pass, payload zero fill + barrier, stream emit, barrier, payload copy + headers, code staging, chains, pack):");
                for (int i = 40; i < 48; i++) fprintf(stderr, " %.0f", (double)pv[i] / (double)(n_units ? n_units : 1));
                fprintf(stderr, "\n");
            }
        }
        unsigned long long tot = 0;
        for (int i = 0; i < 16; i++) tot += pv[i];
        fprintf(stderr, "[K2 prof] shader-clock share per phase:");
        for (int i = 0; i < 14; i++) fprintf(stderr, " p%d=%.1f%%", i, tot ? 100.0 * (double)pv[i] / (double)tot : 0.0);
        fprintf(stderr, "  (total %.3g cycles over %u units)\n", (double)tot, n_units);
        fprintf(stderr, "[K2 prof] tANS chains (counted with -DKC_CHAIN_STATS): %llu chunk-streams (%llu RLE, %llu predefined), %llu repair passes (LL %llu, OF %llu, ML %llu; %llu on RLE tables), %llu segments re-encoded\n",
                pv[16], pv[26], pv[27], pv[17], pv[18], pv[19], pv[20], pv[25], pv[24]);
    }
    *produced = out_off_host[n_units];
    {
        const uint64_t in_total = unit_off[n_units] - unit_off[0];
        c->last_incompressible = in_total >= (1u << 20) && (double)*produced >= 0.98 * (double)in_total;
    }
    return KC_OK;
}

// Scratch a batch may ask for: the configured ceiling, or 85 % of what is free plus what this context already owns (re-used).
uint64_t scratch_budget(kc_ctx* c) {
    uint64_t budget = c->max_scratch_bytes;
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) == hipSuccess) {
        uint64_t held = 0;
        const DevBuf* bufs[] = {&c->seqs, &c->aux, &c->lits, &c->meta, &c->stage, &c->tables, &c->work};
        for (const DevBuf* b : bufs) held += b->cap;
        const uint64_t avail = (uint64_t)((double)(fr + held) * 0.85);
        if (avail < budget) budget = avail;
    } else {
        (void)hipGetLastError();
    }
    return budget;
}

// End of a chunk-fed batch (batch_begin with a ChunkFeed): every chunk has already been entropy coded and compacted on its own
// stream.  *redo is set when a unit needs the speculation re-run (see batch_end): the caller encodes the batch again the plain way.
kc_status feed_finish(kc_ctx* c, bool* redo_needed) {
    if (!c->pend) { c->err = "no batch in flight on this context"; return KC_ERR_BAD_ARG; }
    std::unique_ptr<Pending> P((Pending*)c->pend);
    c->pend = nullptr;
    hipStream_t st = c->stream;
    const uint32_t n_units = P->n_units;
    std::vector<uint32_t> redo(n_units);
    uint32_t errv[16];
    HIPCHK(c, hipMemcpyAsync(redo.data(), c->redo.p, (size_t)n_units * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(errv, c->errflag.p, 64, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    const kc_status sv = device_verdict(c, errv);
    if (sv != KC_OK) return sv;
    *redo_needed = false;
    for (uint32_t i = 0; i < n_units; i++) if (redo[i]) *redo_needed = true;
    return KC_OK;
}

kc_status run_batch(kc_ctx* c, const kc_zstd_opts* o, const uint8_t* d_src_base, const uint64_t* unit_off, uint32_t n_units,
                    uint8_t* d_dst, uint64_t dst_cap, uint64_t* out_off_host, uint64_t* produced) {
    kc_status s = batch_begin(c, o, d_src_base, unit_off, n_units, d_dst, dst_cap);
    if (s != KC_OK) return s;
    return batch_end(c, out_off_host, produced);
}

}  // namespace kci

extern "C" {

kc_status kc_zstd_encode_units_dev(kc_ctx* c, const kc_zstd_opts* o, const uint8_t* d_src, const uint64_t* unit_off, uint32_t n_units,
                                   uint8_t* d_dst, uint64_t dst_cap, uint64_t* out_off) {
    if (!c || !o || !unit_off || !out_off || (n_units && (!d_src || !d_dst))) return KC_ERR_BAD_ARG;
    c->err.clear();
    c->last = kc_timings{0, 0, 0, 0, 0, 0};
    kc_status s = check_supported(c, o);
    if (s != KC_OK) return s;
    HIPCHK(c, hipSetDevice(c->device));
    if ((s = validate_units(c, o, unit_off, n_units)) != KC_OK) return s;
    out_off[0] = 0;
    c->last_batches = 0;
    uint64_t pos = 0;
    uint32_t i0 = 0;
    std::vector<uint64_t> tmp;
    auto unit_len = [&](uint32_t i) { return unit_off[i + 1] - unit_off[i]; };
    auto unit_scratch = [&](uint32_t i) {
        const uint64_t nc = c->cuts ? c->cut_off[i + 1] - c->cut_off[i] : 0;
        return zstd_unit_scratch(o, unit_off[i + 1] - unit_off[i], nc);
    };
    uint64_t budget = scratch_budget(c);
    for (int attempt = 0;; attempt++) {
        bool oom = false;
        while (i0 < n_units) {
            const uint32_t i1 = zenc_cut_batch(i0, n_units, unit_len, unit_scratch, zenc_level_caps(o, c->max_batch_bytes), budget);
            const uint32_t nb = i1 - i0;
            tmp.resize(nb + 1);
            uint64_t produced = 0;
            c->cut_unit0 = i0;
            c->oom = false;
            s = run_batch(c, o, d_src, unit_off + i0, nb, d_dst + pos, dst_cap - pos, tmp.data(), &produced);
            if (s == KC_ERR_UNSUPPORTED && c->oom && nb > 1 && attempt < 6) { oom = true; break; }
            if (s != KC_OK) return s;
            c->last_batches++;
            for (uint32_t k = 0; k <= nb; k++) out_off[i0 + k] = pos + tmp[k];
            pos += produced;
            i0 = i1;
        }
        if (!oom) break;
        budget /= 2;  // another process took device memory since hipMemGetInfo: retry this batch at half the size
        c->err.clear();
    }
    if (n_units == 0) out_off[0] = 0;
    return KC_OK;
}

}  // extern "C"
namespace kci {
kc_status validate_units(kc_ctx* c, const kc_zstd_opts* o, const uint64_t* unit_off, uint32_t n_units) {
    for (uint32_t i = 0; i < n_units; i++) {
        if (unit_off[i + 1] < unit_off[i]) { c->err = "unit_off not ascending"; return KC_ERR_BAD_ARG; }
        if (unit_off[i + 1] - unit_off[i] > KC_MAX_UNIT_BYTES) {
            c->err = "unit larger than 1 GiB: not served by the device path";
            return KC_ERR_UNSUPPORTED;
        }
    }
    return KC_OK;
}
}  // namespace kci
extern "C" {

kc_status kc_zstd_encode_units_dev_begin(kc_ctx* c, const kc_zstd_opts* o, const uint8_t* d_src, const uint64_t* unit_off, uint32_t n_units,
                                         uint8_t* d_dst, uint64_t dst_cap) {
    if (!c || !o || !unit_off || n_units == 0 || !d_src || !d_dst) return KC_ERR_BAD_ARG;
    c->err.clear();
    c->last = kc_timings{0, 0, 0, 0, 0, 0};
    kc_status s = check_supported(c, o);
    if (s != KC_OK) return s;
    HIPCHK(c, hipSetDevice(c->device));
    if ((s = validate_units(c, o, unit_off, n_units)) != KC_OK) return s;
    const KcZencCaps caps = zenc_level_caps(o, c->max_batch_bytes);
    if (unit_off[n_units] - unit_off[0] > caps.bytes || n_units > caps.units) {
        c->err = "begin/end serves one device batch; use kc_zstd_encode_units_dev for larger inputs";
        return KC_ERR_UNSUPPORTED;
    }
    return batch_begin(c, o, d_src, unit_off, n_units, d_dst, dst_cap);
}

kc_status kc_zstd_encode_units_dev_end(kc_ctx* c, uint64_t* out_off) {
    if (!c || !out_off) return KC_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    uint64_t produced = 0;
    return batch_end(c, out_off, &produced);
}

kc_status kc_zstd_encode_units_dev_end_at(kc_ctx* c, uint8_t* d_dst, uint64_t dst_cap, uint64_t* out_off) {
    if (!c || !out_off || !d_dst) return KC_ERR_BAD_ARG;
    if (!c->pend) { c->err = "no batch in flight on this context"; return KC_ERR_BAD_ARG; }
    Pending* P = (Pending*)c->pend;
    // the frames leave the staging slots only in _end (sizes -> offsets -> compaction): until then their place can still be named
    if (P->fed) { c->err = "a chunk-fed batch has written its frames already"; return KC_ERR_UNSUPPORTED; }
    if (P->need > dst_cap) { c->err = "dst_cap smaller than the sum of MaxEncodedSize(unit)"; return KC_ERR_DST_TOO_SMALL; }
    P->d_dst = d_dst;
    return kc_zstd_encode_units_dev_end(c, out_off);
}

void kc_ctx_chain_after(kc_ctx* c, kc_ctx* prev) {
    if (c) c->chain_after = prev;
}

kc_status kc_zstd_encode_streams_dev(kc_ctx* c, const kc_zstd_opts* o, const uint8_t* d_src, const uint64_t* unit_off, uint32_t n_units,
                                     uint8_t* d_dst, uint64_t dst_cap, uint64_t* out_off) {
    if (!c || !o) return KC_ERR_BAD_ARG;
    c->stream_mode = 1;
    const kc_status s = kc_zstd_encode_units_dev(c, o, d_src, unit_off, n_units, d_dst, dst_cap, out_off);
    c->stream_mode = 0;
    return s;
}

}  // extern "C"

