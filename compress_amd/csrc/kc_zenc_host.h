#pragma once
// kc_zenc_host.h — the host rules of one zstd encode batch, free of HIP calls and of the context: how a batch is laid out (block
// grid, staging slots, strides, position width), what it reserves and what one unit is estimated to cost, how KcMatchParams /
// KcEntropyParams are filled, which path a batch takes (checksum behind the entropy stage, the no-match pre-scan), which units and
// blocks the speculation re-run takes, and where a call is cut into batches.  kc_batch.cpp runs these rules on the device (it owns
// the buffers, streams and events), tools/hipemu/kcemu.cpp runs the same rules on the wave emulator over plain memory, and
// tools/zenc_plan_check_main.cpp runs them alone.
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../../include/kcgpu.h"
#include "kc_kernels.h"

namespace kci {

// Blocks of one stream with Flush points (zstd/encoder.go): writeBlocks cuts a block every blockSize bytes after the last Flush
// (:226-253); a Flush that finds nothing buffered does nothing (:552).  Close: a single block still buffered with no header
// written yet is the EncodeAll frame (:272-288), otherwise the stream frame, with an empty last block when nothing is buffered
// (:315-329).  Appends the block starts to *starts; *flags: bit 0 stream frame, bit 1 empty last block.  Returns the block count.
inline uint32_t plan_stream_blocks(uint64_t bs, uint64_t len, const uint64_t* cuts, uint64_t n_cuts, std::vector<uint32_t>* starts, uint32_t* flags) {
    uint64_t pos = 0, ci = 0, lastStart = 0;
    uint32_t ub = 0;
    while (pos < len) {
        uint64_t e = pos + bs;
        while (ci < n_cuts && cuts[ci] <= pos) ci++;
        if (ci < n_cuts && cuts[ci] < e) e = cuts[ci];
        if (e > len) e = len;
        if (starts) starts->push_back((uint32_t)pos);
        lastStart = pos;
        pos = e;
        ub++;
    }
    const bool flushedAtEnd = n_cuts > 0 && cuts[n_cuts - 1] >= len;
    const bool tailBuffered = ub > 0 && !flushedAtEnd && (len - lastStart) < bs;
    const bool streamU = len > 0 && !(ub == 1 && tailBuffered);
    *flags = (streamU ? 1u : 0u) | ((streamU && !tailBuffered) ? 2u : 0u);
    return ub;
}

// ---- per-block and per-unit terms: the plan, the reservations and the estimate are all written from these ----
inline uint32_t zenc_seq_stride(int bs) { return (uint32_t)(bs / 4 + 8); }  // packed sequences (and aux words) per block
inline uint32_t zenc_lit_stride(int bs) { return (uint32_t)(bs + 64); }     // literal bytes per block
inline uint64_t zenc_block_scratch(int bs) { return 2ull * zenc_seq_stride(bs) * 8 + zenc_lit_stride(bs) + sizeof(KcBlkMeta); }  // seqs, aux, lits, meta
inline uint64_t zenc_table_bytes(int level) {  // per unit; SpeedBestCompression: persistent slots of the context, not per unit
    if (level == KC_SPEED_BEST) return 0;
    return level == KC_SPEED_BETTER ? kc_zbetter_table_bytes() : (level == KC_SPEED_DEFAULT ? kc_zdfast_table_bytes() : kc_zfast_table_bytes());
}
// The staging slot of one unit.  Every block costs a 3-byte header: Flush points add blocks that MaxEncodedSize(len) does not count.
inline uint64_t zenc_unit_slot(const kc_zstd_opts* o, uint64_t len, bool flush, uint64_t n_cuts) {
    return ((uint64_t)kc_zstd_max_encoded_size(o, (int64_t)len) + (flush ? 3 * n_cuts + 3 : 0) + 15) & ~(uint64_t)15;
}
// A unit is parsed with positions of pos_bits bits (position + 1 in a tagged table entry), wide enough for the longest unit of the
// batch behind its dictionary.
inline uint64_t zenc_max_unit(const uint64_t* unit_off, uint32_t n_units) {
    uint64_t m = 16;
    for (uint32_t i = 0; i < n_units; i++) m = std::max<uint64_t>(m, unit_off[i + 1] - unit_off[i]);
    return m;
}
inline int zenc_pos_bits(uint64_t hist0, uint64_t max_unit) {
    int pb = 1;
    while (((uint64_t)1 << pb) <= hist0 + max_unit + 2) pb++;
    return pb;
}
inline int zenc_hist0(const kc_zstd_opts* o) { return (o->dict != nullptr && o->dict_len > 0) ? (int)o->dict_len : 0; }  // raw content, WithEncoderDictRaw: history = dict || unit (enc_base.go:189-198)

// A batch is bounded by its input bytes AND by the device scratch it needs: tables are per unit, sequences / literals /
// staging are per block at a fixed stride whatever the block's actual length, so many small units need far more than the
// "~6x input" of full-size units (1M x 4 KiB units at SpeedDefault would ask for hundreds of GiB in one batch).
// The estimate of one unit: every Flush point can add a block, at the full per-block strides; the slot with the Flush headers.
inline uint64_t zstd_unit_scratch(const kc_zstd_opts* o, uint64_t len, uint64_t n_cuts = 0) {
    const uint64_t bsz = (uint64_t)o->block_size;
    const uint64_t hist0 = (o->dict != nullptr) ? o->dict_len : 0;
    const uint64_t blocks = (len + bsz - 1) / bsz + n_cuts;
    return zenc_table_bytes(o->level) + blocks * zenc_block_scratch(o->block_size) + zenc_unit_slot(o, len, true, n_cuts) + (hist0 ? hist0 + len : 0) + 64;
}

// ---- the plan ----
struct KcZencCuts {  // Flush points of a call's streams (cuts null: none); the batch's first unit is unit0 of the call
    const uint64_t* cut_off = nullptr;
    const uint64_t* cuts = nullptr;
    uint32_t unit0 = 0;
};
// Host-side layout of one device batch.
struct KcZencPlan {
    uint32_t n_units = 0, n_blocks = 0;
    std::vector<uint32_t> blk0;       // n+1
    std::vector<uint64_t> stage_off;  // n+1
    std::vector<uint32_t> blk_start, unit_flags;  // streams with Flush points: per block / per unit (see KcMatchParams)
    std::vector<uint64_t> rel_off;    // n+1 unit offsets relative to the batch base
    uint32_t seq_stride = 0, lit_stride = 0;
    uint64_t max_unit_bytes = 0;      // longest unit of the batch
    bool irregular = false;           // the batch's streams have Flush points: blocks start where blk_start says
    int hist0 = 0, pos_bits = 0;
    uint64_t need = 0;                // sum of the staging slots: what dst must hold
};
// job_hist: null, or per unit the bytes of overlap prefix in front of it (history, not blocks)
inline void zenc_plan(const kc_zstd_opts* o, const uint64_t* unit_off, uint32_t n_units, const uint32_t* job_hist, const KcZencCuts& fl, KcZencPlan& pl) {
    const int bs = o->block_size;
    pl.n_units = n_units;
    pl.blk0.resize(n_units + 1);
    pl.stage_off.resize(n_units + 1);
    pl.rel_off.resize(n_units + 1);
    pl.irregular = fl.cuts != nullptr;
    pl.blk_start.clear();
    pl.unit_flags.clear();
    uint64_t so = 0;
    uint32_t nb = 0;
    for (uint32_t i = 0; i < n_units; i++) {
        const uint64_t len = unit_off[i + 1] - unit_off[i];
        pl.blk0[i] = nb;
        pl.stage_off[i] = so;
        pl.rel_off[i] = unit_off[i] - unit_off[0];
        uint32_t ub = (uint32_t)((len - (job_hist ? job_hist[i] : 0) + bs - 1) / bs);
        uint64_t nc = 0;
        if (pl.irregular) {
            const uint64_t c0 = fl.cut_off[fl.unit0 + i];
            nc = fl.cut_off[fl.unit0 + i + 1] - c0;
            uint32_t f = 0;
            ub = plan_stream_blocks((uint64_t)bs, len, fl.cuts + c0, nc, &pl.blk_start, &f);
            pl.unit_flags.push_back(f);
        }
        nb += ub;
        so += zenc_unit_slot(o, len, pl.irregular, nc);
    }
    pl.blk0[n_units] = nb;
    pl.stage_off[n_units] = so;
    pl.rel_off[n_units] = unit_off[n_units] - unit_off[0];
    pl.n_blocks = nb;
    pl.need = so;
    pl.seq_stride = zenc_seq_stride(bs);
    pl.lit_stride = zenc_lit_stride(bs);
    pl.hist0 = zenc_hist0(o);
    pl.max_unit_bytes = zenc_max_unit(unit_off, n_units);
    pl.pos_bits = zenc_pos_bits((uint64_t)pl.hist0, pl.max_unit_bytes);
}
// the packed sequences keep offset + 3 in 24 bits: fine for the default windows (4 / 8 MiB) and for any unit below 16 MiB
inline bool zenc_offsets_fit(const kc_zstd_opts* o, const KcZencPlan& pl) {
    return std::min<uint64_t>((uint64_t)o->window_size, (uint64_t)pl.hist0 + pl.max_unit_bytes) + 3 <= 0xFFFFFFull;
}
// What the batch reserves of the buffers that grow with it (bytes, before the 64 bytes of slack the device buffers get): the terms
// of zstd_unit_scratch, summed over the plan.  The per-unit and per-block flag and offset arrays (under 70 bytes a unit, 18 a block)
// are not estimated: the scratch budget leaves 15 % of the device free.
struct KcZencReserve {
    uint64_t seqs, aux, lits, meta, stage, work, tables;
    uint64_t sum() const { return seqs + aux + lits + meta + stage + work + tables; }
};
inline KcZencReserve zenc_reserve(const kc_zstd_opts* o, const KcZencPlan& pl) {
    KcZencReserve r;
    r.seqs = r.aux = (uint64_t)pl.n_blocks * pl.seq_stride * 8;
    r.lits = (uint64_t)pl.n_blocks * pl.lit_stride;
    r.meta = (uint64_t)pl.n_blocks * sizeof(KcBlkMeta);
    r.stage = pl.need;
    r.work = pl.hist0 ? pl.rel_off[pl.n_units] + (uint64_t)pl.n_units * (uint64_t)pl.hist0 : 0;  // dictionary || unit, per unit
    r.tables = (uint64_t)pl.n_units * zenc_table_bytes(o->level);
    return r;
}

// ---- the two path predicates ----
// SpeedFastest HBM-table kernel: the form for input without matches — by option, or (-1) when the context's previous batch did not compress
inline int32_t zenc_tuned_form(int64_t zfast_variant, bool last_incompressible) { return zfast_variant < 0 ? (last_incompressible ? 1 : 0) : (int32_t)zfast_variant; }
// The checksum moves behind the entropy stage (kc_xxh64_fin_kernel) where the batch has a regular block grid and no history in
// front of its units: frames that turn out to be raw blocks only then get their payload copied by the pass that hashes it.
inline bool zenc_fuse_xxh(const kc_zstd_opts* o, const KcZencPlan& pl, bool fuse_opt, bool jobs, bool fed) {
    return fuse_opt && o->crc && !jobs && pl.hist0 == 0 && !pl.irregular && (o->block_size % 256) == 0 && !fed;
}
// The no-match pre-scan (kc_zstd_prescan.hip): SpeedFastest EncodeAll batches whose frames take the deferred-payload path
// (fuse_xxh: checksum on, regular block grid, no dictionary / job prefix / chunk feed), literal-only blocks going out raw
// (rawAllLits, the default below SpeedBetterCompression).  On by option (prescan_opt 1), or per batch (-1) when the context's
// previous batch did not compress (the same signal that picks the match finder's form for such input).
inline bool zenc_run_prescan(const kc_zstd_opts* o, const KcZencPlan& pl, int64_t prescan_opt, bool tuned_now, bool fuse_xxh, int stream_mode) {
    const bool want = prescan_opt > 0 || (prescan_opt < 0 && tuned_now);
    return want && o->level == KC_SPEED_FASTEST && fuse_xxh && !stream_mode && !o->all_lit_entropy && o->block_size >= 16 && pl.n_units > 0;
}

// The first-occurrence filter of the SpeedFastest HBM-table kernel (kc_zstd_first.hip): exactly where every unit's table starts
// empty and the unit has nothing in front of it — no dictionary, no job prefix, no primed tables — and the whole batch is on the
// device before the match finder starts (not chunk-fed).  The caller adds "the HBM-table kernel runs" (its own path choice).
inline bool zenc_first_filter(const kc_zstd_opts* o, const KcZencPlan& pl, bool first_opt, bool jobs, bool fed) {
    return first_opt && o->level == KC_SPEED_FASTEST && pl.hist0 == 0 && !jobs && !fed && pl.n_units > 0;
}

// ---- the parameter fill ----
struct KcZencBufs {  // device pointers of the buffers a batch reserves
    const uint8_t* src = nullptr;        // what the kernels read: the source at the batch's first unit, or the work buffer (dictionary || unit)
    const uint64_t* unit_off = nullptr;  // ... and its n+1 offsets
    const uint32_t *unit_blk0 = nullptr, *blk_start = nullptr, *unit_flags = nullptr, *job_hist = nullptr, *job_flags = nullptr;
    uint64_t *seqs = nullptr, *aux = nullptr;
    KcBlkMeta* meta = nullptr;
    uint8_t *lits = nullptr, *stage = nullptr, *redo_blk = nullptr;
    const uint64_t *stage_off = nullptr, *xxh = nullptr;
    uint32_t *out_size = nullptr, *redo = nullptr, *errflag = nullptr, *unit_raw = nullptr;
    const void* predef = nullptr;
    KcRawDef* rawdef = nullptr;
    const uint8_t* dict_huf = nullptr;   // null, or the dictionary's literal table (256 x u16 val, 256 x u8 nBits)
};
struct KcZencSteer {
    int stream_mode = 0;
    int64_t spec_w0 = -1, spec_grow = -1;  // -1: the per-level defaults
    bool fuse_xxh = false;
};
inline void zenc_fill_params(const kc_zstd_opts* o, const KcZencPlan& pl, const KcZencBufs& b, const KcZencSteer& cx, KcMatchParams& mp, KcEntropyParams& ep) {
    memset(&mp, 0, sizeof(mp));  // (pop_blk, unit_list: the re-run's; unit_base, unit_done, prof, epoch and the kernel forms: the launcher's)
    mp.src = b.src;
    mp.src_end = b.src + pl.rel_off[pl.n_units] + (uint64_t)pl.n_units * (uint64_t)pl.hist0;
    mp.unit_off = b.unit_off;
    mp.unit_hist = b.job_hist;
    mp.job_flags = b.job_flags;
    mp.hist0 = pl.hist0;
    mp.pos_bits = pl.pos_bits;
    mp.stream_mode = cx.stream_mode;
    mp.rep1 = (int32_t)o->dict_offsets[0];
    mp.rep2 = (int32_t)o->dict_offsets[1];
    mp.rep3 = (int32_t)o->dict_offsets[2];
    if (mp.rep1 <= 0 || mp.rep2 <= 0 || mp.rep3 <= 0) { mp.rep1 = 1; mp.rep2 = 4; mp.rep3 = 8; }  // opts not initialised through kc_zstd_opts_default
    mp.unit_blk0 = b.unit_blk0;
    mp.seqs = b.seqs;
    mp.meta = b.meta;
    mp.seq_stride = pl.seq_stride;
    mp.blk_start = pl.irregular ? b.blk_start : nullptr;
    mp.unit_flags = pl.irregular ? b.unit_flags : nullptr;
    mp.block_size = o->block_size;
    mp.max_match_off = o->window_size;
    // SpeedDefault, round 2 (ms per launch): at 4 GiB (32768 units: DRAM-transaction bound, wasted probes cost) width 2 / 3 / 4 then doubling
    // 265.9 / 266.7 / 274.0, 2 then +1 264.1; at 2 GiB (latency bound) 163.6 / - / 155.4, fixed 1: 285.5.  The BASELINE size is 4 GiB.
    // SpeedBetterCompression (1 GiB = 8192 units: latency-bound, wide speculation pays): width 1 / 2 / 4 then doubling 98.6 / 91.5 / 86.0,
    // fixed 4: 101.4, fixed 8: 80.4 ms with 8 lanes per unit; 16 lanes per unit, fixed 16: 61.1 ms (one probe per round, round 1: 181 ms)
    mp.spec_w0 = cx.spec_w0 >= 0 ? (int)cx.spec_w0 : (o->level == KC_SPEED_DEFAULT ? 2 : (o->level == KC_SPEED_BETTER ? 16 : 1));
    // measured on C2 (ms per 4 GiB): width 1 then +1 per miss 137, fixed 2 136.5, 1 then doubling 140, fixed 1 167, fixed 4 157
    mp.spec_grow = cx.spec_grow >= 0 ? (int)cx.spec_grow : (o->level == KC_SPEED_FASTEST ? 1 : (o->level == KC_SPEED_BETTER ? 0 : 2));
    mp.spec_w0 = std::min(std::max(mp.spec_w0, 1), 64);  // the kernels clamp to their group size

    memset(&ep, 0, sizeof(ep));
    ep.src = b.src;
    ep.unit_off = b.unit_off;
    ep.unit_hist = mp.unit_hist;
    ep.job_flags = mp.job_flags;
    ep.hist0 = pl.hist0;
    ep.stream_mode = cx.stream_mode;
    ep.stream_sync = o->concurrent == 1;
    if (b.dict_huf != nullptr) { ep.dict_huf = b.dict_huf; ep.dict_huf_len = o->dict_huf_len; ep.dict_huf_log = o->dict_huf_log; }  // -> prevTable of every unit's first block
    ep.unit_blk0 = mp.unit_blk0;
    ep.seqs = mp.seqs;
    ep.meta = mp.meta;
    ep.blk_start = mp.blk_start;
    ep.unit_flags = mp.unit_flags;
    ep.lits = b.lits;
    ep.aux = b.aux;
    ep.stage = b.stage;
    ep.stage_off = b.stage_off;
    ep.out_size = b.out_size;
    ep.xxh = b.xxh;
    ep.redo_mask = b.redo;
    ep.redo_blk = b.redo_blk;
    ep.predef = b.predef;
    ep.err_flag = b.errflag;
    ep.seq_stride = pl.seq_stride;
    ep.lit_stride = pl.lit_stride;
    ep.block_size = o->block_size;
    ep.window_size = o->window_size;
    ep.crc = o->crc;
    ep.single = o->single;
    ep.no_entropy = o->no_entropy;
    ep.all_lit_entropy = o->all_lit_entropy;
    ep.full_zero = o->full_zero;
    ep.dict_id = o->dict_id;
    ep.rawdef = b.rawdef;  // raw blocks are copied once, by the compaction, from the source (KcRawDef): the entries of blocks that are not raw stay zero
    if (cx.fuse_xxh) { ep.unit_raw = b.unit_raw; ep.xxh = nullptr; }  // the checksum field is left to kc_xxh64_fin_kernel
}
// the pre-scan's parameters from the batch's; the caller sets mp.unit_done / ep.unit_done to unit_done once it has launched
inline KcPrescanParams zenc_prescan_params(const kc_zstd_opts* o, const KcZencPlan& pl, const KcMatchParams& mp, const KcEntropyParams& ep,
                                           const uint32_t* probe_rel, uint32_t n_probe, uint32_t* unit_done) {
    KcPrescanParams pp;
    memset(&pp, 0, sizeof(pp));
    pp.src = ep.src;
    pp.unit_off = ep.unit_off;
    pp.unit_blk0 = mp.unit_blk0;
    pp.n_units = pl.n_units;
    pp.block_size = o->block_size;
    pp.probe_rel = probe_rel;
    pp.n_probe = n_probe;
    pp.rep1 = mp.rep1;
    pp.rep2 = mp.rep2;
    pp.meta = mp.meta;
    pp.unit_done = unit_done;
    pp.stage = ep.stage;
    pp.stage_off = ep.stage_off;
    pp.out_size = ep.out_size;
    pp.rawdef = ep.rawdef;
    pp.unit_raw = ep.unit_raw;
    pp.window_size = o->window_size;
    pp.crc = o->crc;
    pp.single = o->single;
    pp.dict_id = o->dict_id;
    return pp;
}
// the finishing pass's checksum kernel (with it the payload of the frames that are raw blocks only) from the batch's parameters
inline KcXxhFinParams zenc_xxh_fin_params(const KcEntropyParams& ep, uint32_t n_units, const uint64_t* out_off, uint8_t* dst, uint64_t* xxh_out, int32_t mode) {
    KcXxhFinParams xf;
    memset(&xf, 0, sizeof(xf));
    xf.src = ep.src;
    xf.unit_off = ep.unit_off;
    xf.n_units = n_units;
    xf.stage = ep.stage;
    xf.stage_off = ep.stage_off;
    xf.out_size = ep.out_size;
    xf.out_off = out_off;
    xf.dst = dst;
    xf.unit_raw = ep.unit_raw;
    xf.rawdef = ep.rawdef;
    xf.unit_blk0 = ep.unit_blk0;
    xf.xxh_out = xxh_out;
    xf.mode = mode;
    return xf;
}

// ---- the speculation re-run ----
// A block that fell back to raw only after entropy coding (blockenc.go:811-817) pops the repeat offsets; if the following block was
// parsed with the un-popped offsets the entropy stage flags the unit (redo) and the block (redo_blk), and the unit is parsed again
// with that verdict forced (pop_blk).  The blocks behind a flagged block were themselves parsed from offsets that may be wrong, so
// of a unit's flags only the lowest is trustworthy: every pass settles one more block per unit, and a batch whose longest unit has
// B blocks is settled after at most B + 1 passes.
inline void zenc_redo_units(const uint32_t* redo, uint32_t n_units, std::vector<uint32_t>& list) {
    list.clear();
    for (uint32_t i = 0; i < n_units; i++)
        if (redo[i]) list.push_back(i);
}
inline void zenc_redo_mark(const KcZencPlan& pl, const std::vector<uint32_t>& list, const uint8_t* redo_blk, std::vector<uint8_t>& pop_blk) {
    if (pop_blk.empty()) pop_blk.assign(pl.n_blocks, 0);  // (the marks of earlier passes stay)
    for (uint32_t i : list)
        for (uint32_t b = pl.blk0[i]; b < pl.blk0[i + 1]; b++)
            if (redo_blk[b]) { pop_blk[b] = 1; break; }
}
inline uint32_t zenc_redo_max_passes(const KcZencPlan& pl) {
    uint32_t maxBlocks = 1;
    for (uint32_t i = 0; i < pl.n_units; i++) maxBlocks = std::max(maxBlocks, pl.blk0[i + 1] - pl.blk0[i]);
    return maxBlocks + 1;
}

// ---- the batch cutter ----
struct KcZencCaps {
    uint64_t bytes;   // input bytes per batch
    uint32_t units;   // units per batch
};
// SpeedBetterCompression: 4 MiB of tables per unit
inline KcZencCaps zenc_level_caps(const kc_zstd_opts* o, uint64_t max_batch_bytes) {
    if (o->level == KC_SPEED_BETTER) return KcZencCaps{(uint64_t)1 << 30, 16384u};
    return KcZencCaps{max_batch_bytes, 0xFFFFFFFFu};
}
// The end of the batch that starts at unit i0 (never i0 itself while i0 < n): units are taken while the batch stays inside the caps
// and its scratch, with the 1/8 the device buffers over-allocate, inside the budget.  len(i) / scratch(i): unit i's bytes / estimate.
template <class LenFn, class ScratchFn>
inline uint32_t zenc_cut_batch(uint32_t i0, uint32_t n, LenFn len, ScratchFn scratch, const KcZencCaps& caps, uint64_t budget) {
    uint32_t i1 = i0;
    uint64_t bytes = 0, sc = 0;
    while (i1 < n) {
        const uint64_t us = scratch(i1), ul = len(i1);
        if (i1 > i0 && (bytes + ul > caps.bytes || i1 - i0 >= caps.units || (sc + us) + ((sc + us) >> 3) > budget)) break;
        sc += us;
        bytes += ul;
        i1++;
    }
    return i1;
}

}  // namespace kci
