// zenc_plan_check — the host rules of the zstd encode batch (compress_amd/csrc/kc_zenc_host.h) alone in ONE ordinary executable that is
// built with -fsanitize=address,undefined and run on the host.  TEST INFRASTRUCTURE; nothing of it is loaded into another process and
// nothing of it runs on a device (the header calls no kernel; tools/hipemu only supplies the types kc_kernels.h names).
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -I tools/hipemu tools/zenc_plan_check_main.cpp
//       compress_amd/csrc/kc_zstd_opts.cpp -o tools/_build/zenc_plan_check
//   tools/_build/zenc_plan_check
//
// For every level, with the level's window and with a 16 KiB one: units of 0, 1, bs - 1, bs, bs + 1 and 5 bs + 7 bytes go through the
// plan without Flush points, with them, with job prefixes and with a dictionary.  Checked: `need` is the sum of the units' slots; the
// sum of the units' scratch estimates covers the plan's reservations; the block grid is the one the lengths, prefixes and cuts give;
// the position width holds the longest unit.  The cutter never returns an empty batch, covers every unit once and keeps every batch of
// more than one unit inside the caps and the budget.  The re-run rule lists the flagged units and marks only the lowest flagged block
// of each listed unit, keeping the marks of earlier passes.  Every array handed in is a vector of exactly its size, so a read past its
// end is a sanitizer report.  Exit status 0: clean.
#include <stdio.h>
#include <stdlib.h>
#include "../compress_amd/csrc/kc_zenc_host.h"

using namespace kci;

static int g_failed = 0, g_checks = 0;
#define CHECK(cond, ...)                                                       \
    do {                                                                       \
        g_checks++;                                                            \
        if (!(cond)) {                                                         \
            g_failed++;                                                        \
            fprintf(stderr, "FAILED %s:%d: %s  ", __FILE__, __LINE__, #cond);  \
            fprintf(stderr, __VA_ARGS__);                                      \
            fprintf(stderr, "\n");                                             \
        }                                                                      \
    } while (0)

static std::vector<uint64_t> offsets(const std::vector<uint64_t>& lens, uint64_t base) {
    std::vector<uint64_t> off(lens.size() + 1, base);
    for (size_t i = 0; i < lens.size(); i++) off[i + 1] = off[i] + lens[i];
    return off;
}

// one plan against what its inputs say; cuts: empty, or per unit its Flush points; hist: empty, or per unit its job prefix
static void check_plan(const kc_zstd_opts& o, const std::vector<uint64_t>& lens, const std::vector<std::vector<uint64_t>>& cuts, const std::vector<uint32_t>& hist,
                       const char* what) {
    const uint32_t n = (uint32_t)lens.size();
    const uint64_t bs = (uint64_t)o.block_size;
    const std::vector<uint64_t> off = offsets(lens, 4096);  // (a batch in the middle of a call: offsets from a base)
    std::vector<uint64_t> cut_off, flat;
    KcZencCuts fl;
    if (!cuts.empty()) {
        cut_off.assign(3, 0);  // (and in the middle of the call's streams: unit0 = 2)
        for (const auto& c : cuts) { flat.insert(flat.end(), c.begin(), c.end()); cut_off.push_back(flat.size()); }
        flat.push_back(0);
        fl.cut_off = cut_off.data(); fl.cuts = flat.data(); fl.unit0 = 2;
    }
    KcZencPlan pl;
    pl.blk_start.assign(7, 99);  // (a plan is re-used from batch to batch: what the last one left must not show)
    pl.unit_flags.assign(3, 99);
    zenc_plan(&o, off.data(), n, hist.empty() ? nullptr : hist.data(), fl, pl);
    uint64_t slots = 0, est = 0, blocks = 0, longest = 16;
    for (uint32_t i = 0; i < n; i++) {
        const uint64_t nc = cuts.empty() ? 0 : cuts[i].size();
        CHECK(pl.stage_off[i] == slots && (slots & 15) == 0, "%s unit %u", what, i);
        CHECK(pl.blk0[i] == blocks, "%s unit %u", what, i);
        CHECK(pl.rel_off[i] == off[i] - off[0], "%s unit %u", what, i);
        const uint64_t slot = zenc_unit_slot(&o, lens[i], !cuts.empty(), nc);
        CHECK(slot >= (uint64_t)kc_zstd_max_encoded_size(&o, (int64_t)lens[i]) + (cuts.empty() ? 0 : 3 * nc + 3), "%s unit %u", what, i);
        slots += slot;
        est += zstd_unit_scratch(&o, lens[i], nc);
        const uint64_t ub = pl.blk0[i + 1] - pl.blk0[i];
        if (cuts.empty()) CHECK(ub == (lens[i] - (hist.empty() ? 0 : hist[i]) + bs - 1) / bs, "%s unit %u: %llu blocks", what, i, (unsigned long long)ub);
        else {
            CHECK(ub <= (lens[i] + bs - 1) / bs + nc, "%s unit %u: %llu blocks", what, i, (unsigned long long)ub);
            for (uint64_t k = 0; k < ub; k++) {  // the blocks start in order, none longer than a block, the first at 0
                const uint32_t s0 = pl.blk_start[blocks + k], s1 = k + 1 < ub ? pl.blk_start[blocks + k + 1] : (uint32_t)lens[i];
                CHECK((k > 0 || s0 == 0) && s0 < s1 && s1 - s0 <= bs, "%s unit %u block %llu", what, i, (unsigned long long)k);
            }
            CHECK((lens[i] == 0) == ((pl.unit_flags[i] & 1u) == 0u) || ub == 1, "%s unit %u flags %u", what, i, pl.unit_flags[i]);
        }
        blocks += ub;
        longest = std::max(longest, lens[i]);
    }
    CHECK(pl.need == slots && pl.stage_off[n] == slots, "%s: need %llu, slots %llu", what, (unsigned long long)pl.need, (unsigned long long)slots);
    CHECK(pl.n_blocks == blocks && pl.blk0[n] == blocks, "%s", what);
    CHECK(pl.blk_start.size() == (cuts.empty() ? 0 : blocks) && pl.unit_flags.size() == (cuts.empty() ? 0u : n), "%s", what);
    CHECK(pl.seq_stride == zenc_seq_stride(o.block_size) && pl.lit_stride == zenc_lit_stride(o.block_size), "%s", what);
    CHECK(pl.max_unit_bytes == longest && pl.hist0 == zenc_hist0(&o), "%s", what);
    const uint64_t top = (uint64_t)pl.hist0 + longest + 2;
    CHECK(((uint64_t)1 << pl.pos_bits) > top && ((uint64_t)1 << (pl.pos_bits - 1)) <= top, "%s: pos_bits %d", what, pl.pos_bits);
    const KcZencReserve r = zenc_reserve(&o, pl);
    CHECK(est >= r.sum(), "%s: estimate %llu below the reservations %llu", what, (unsigned long long)est, (unsigned long long)r.sum());
    CHECK(r.stage == pl.need && r.seqs == blocks * zenc_seq_stride(o.block_size) * 8, "%s", what);
}

static void check_cutter(const kc_zstd_opts& o, const std::vector<uint64_t>& lens) {
    const uint32_t n = (uint32_t)lens.size();
    auto len = [&](uint32_t i) { return lens[i]; };
    auto sc = [&](uint32_t i) { return zstd_unit_scratch(&o, lens[i]); };
    uint64_t all = 0;
    for (uint32_t i = 0; i < n; i++) all += sc(i);
    const KcZencCaps level = zenc_level_caps(&o, (uint64_t)8 << 30);
    CHECK(o.level == KC_SPEED_BETTER ? (level.bytes == ((uint64_t)1 << 30) && level.units == 16384u) : (level.bytes == ((uint64_t)8 << 30) && level.units == 0xFFFFFFFFu), "caps");
    const KcZencCaps capv[] = {level, {1, 0xFFFFFFFFu}, {(uint64_t)3 * o.block_size, 0xFFFFFFFFu}, {level.bytes, 1}, {level.bytes, 2}};
    const uint64_t budgets[] = {0, 1, sc(0), all / 3, all, all + (all >> 3), UINT64_MAX};
    for (const KcZencCaps& caps : capv)
        for (uint64_t budget : budgets) {
            uint32_t i0 = 0, batches = 0;
            while (i0 < n) {
                const uint32_t i1 = zenc_cut_batch(i0, n, len, sc, caps, budget);
                CHECK(i1 > i0 && i1 <= n, "cutter: empty batch at %u (budget %llu)", i0, (unsigned long long)budget);
                if (i1 <= i0) return;
                uint64_t bytes = 0, s = 0;
                for (uint32_t i = i0; i < i1; i++) { bytes += lens[i]; s += sc(i); }
                if (i1 - i0 > 1) CHECK(bytes <= caps.bytes && i1 - i0 <= caps.units && s + (s >> 3) <= budget, "cutter: batch %u..%u outside its bounds", i0, i1);
                if (i1 < n) {  // ... and it stopped for a reason: the next unit would not have fitted
                    const uint64_t s2 = s + sc(i1);
                    CHECK(bytes + lens[i1] > caps.bytes || i1 - i0 >= caps.units || s2 + (s2 >> 3) > budget, "cutter: batch %u..%u ends early", i0, i1);
                }
                i0 = i1;
                batches++;
            }
            CHECK(batches >= 1 && batches <= n, "cutter");
        }
}

static void check_redo(const kc_zstd_opts& o) {
    const uint64_t bs = (uint64_t)o.block_size;
    const std::vector<uint64_t> lens = {5 * bs + 7, 0, bs, 3 * bs, 5 * bs + 7, 1, 2 * bs + 1};  // 6, 0, 1, 3, 6, 1, 3 blocks
    const std::vector<uint64_t> off = offsets(lens, 0);
    KcZencPlan pl;
    zenc_plan(&o, off.data(), (uint32_t)lens.size(), nullptr, KcZencCuts(), pl);
    CHECK(pl.n_blocks == 20 && zenc_redo_max_passes(pl) == 7, "re-run: %u blocks, %u passes", pl.n_blocks, zenc_redo_max_passes(pl));
    std::vector<uint32_t> redo = {1, 0, 0, 7, 1, 0, 0}, list;
    std::vector<uint8_t> redo_blk(pl.n_blocks, 0), pop_blk;
    // unit 0: blocks 2, 3 and 5 flagged; unit 3 (blocks 7..9): 8 and 9; unit 4 (10..15): its last; unit 6 (17..19) flagged but not listed
    for (uint32_t b : {2u, 3u, 5u, 8u, 9u, 15u, 17u, 18u}) redo_blk[b] = 1;
    zenc_redo_units(redo.data(), (uint32_t)redo.size(), list);
    CHECK(list == (std::vector<uint32_t>{0, 3, 4}), "re-run: the unit list");
    zenc_redo_mark(pl, list, redo_blk.data(), pop_blk);
    std::vector<uint8_t> want(pl.n_blocks, 0);
    want[2] = want[8] = want[15] = 1;
    CHECK(pop_blk == want, "re-run: only the lowest flagged block of a listed unit is marked");
    // the next pass: unit 0 alone, its block 4 now; the marks of the first pass stay
    redo = {1, 0, 0, 0, 0, 0, 0};
    std::fill(redo_blk.begin(), redo_blk.end(), 0);
    redo_blk[4] = redo_blk[5] = 1;
    zenc_redo_units(redo.data(), (uint32_t)redo.size(), list);
    zenc_redo_mark(pl, list, redo_blk.data(), pop_blk);
    want[4] = 1;
    CHECK(list == (std::vector<uint32_t>{0}) && pop_blk == want, "re-run: second pass");
    std::fill(redo.begin(), redo.end(), 0);
    zenc_redo_units(redo.data(), (uint32_t)redo.size(), list);
    CHECK(list.empty(), "re-run: settled");
}

int main() {
    static const uint8_t dict[5000] = {1, 2, 3};
    for (int level = KC_SPEED_FASTEST; level <= KC_SPEED_BEST; level++)
        for (int window : {0, 16 << 10}) {
            kc_zstd_opts o;
            kc_zstd_opts_default(&o);
            kc_zstd_opts_level(&o, level);
            if (window) kc_zstd_opts_window(&o, window);
            const uint64_t bs = (uint64_t)o.block_size;
            char what[64];
            const std::vector<uint64_t> lens = {0, 1, bs - 1, bs, bs + 1, 5 * bs + 7};
            snprintf(what, sizeof(what), "level %d bs %d plain", level, o.block_size);
            check_plan(o, lens, {}, {}, what);
            check_plan(o, {}, {}, {}, what);
            snprintf(what, sizeof(what), "level %d bs %d flush", level, o.block_size);
            check_plan(o, lens, {{}, {0, 1}, {10, bs - 1}, {bs}, {bs - 1, bs, bs + 1}, {7, 7, 7, 2 * bs + 7, 5 * bs + 7, 5 * bs + 9}}, {}, what);
            check_plan(o, lens, {{0}, {}, {}, {}, {}, {}}, {}, what);
            snprintf(what, sizeof(what), "level %d bs %d jobs", level, o.block_size);
            check_plan(o, lens, {}, {0, 1, 1000, (uint32_t)bs / 2, (uint32_t)bs, (uint32_t)bs + 7}, what);
            check_cutter(o, lens);
            check_cutter(o, std::vector<uint64_t>(40, bs + 1));
            check_redo(o);
            kc_zstd_opts od = o;
            kc_zstd_opts_dict_raw(&od, 7, dict, sizeof(dict));
            snprintf(what, sizeof(what), "level %d bs %d dictionary", level, o.block_size);
            check_plan(od, lens, {}, {}, what);
        }
    {   // the 24-bit offset field: windows up to 8 MiB always fit, a larger window only while the units stay below 16 MiB
        kc_zstd_opts o;
        kc_zstd_opts_default(&o);
        KcZencPlan pl;
        const uint64_t big[2] = {0, (uint64_t)17 << 20};
        zenc_plan(&o, big, 1, nullptr, KcZencCuts(), pl);
        CHECK(zenc_offsets_fit(&o, pl), "8 MiB window");
        kc_zstd_opts_window(&o, 32 << 20);
        CHECK(!zenc_offsets_fit(&o, pl), "32 MiB window, 17 MiB unit");
        const uint64_t small[2] = {0, (uint64_t)15 << 20};
        zenc_plan(&o, small, 1, nullptr, KcZencCuts(), pl);
        CHECK(zenc_offsets_fit(&o, pl), "32 MiB window, 15 MiB unit");
    }
    printf("zenc_plan_check: %d checks, %d failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
