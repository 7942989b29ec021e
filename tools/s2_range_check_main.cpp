// s2_range_check — a stand-alone memory-error hunt for the host side of the ranged reads: the index code (compress_amd/csrc/
// kc_s2_index.cpp: kc_s2_index_load, _load_stream, _find, kc_s2_index_stream) linked into ONE ordinary executable that is built with
// -fsanitize=address,undefined and run on the host.  TEST INFRASTRUCTURE; nothing of it is loaded into another process and nothing of
// it runs on a device.
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer tools/s2_range_check_main.cpp \
//       compress_amd/csrc/kc_s2_index.cpp -o tools/_build/s2_range_check
//   tools/_build/s2_range_check [-n mutations-per-index] [-s seed] file...
//
// Every file named is framed into S2 streams of uncompressed chunks (blocks of 1 KiB and 4 KiB; repeated to 3 MiB in blocks of 64 KiB,
// where the 1 MiB spacing of Index.add leaves three entries).  For every stream: kc_s2_index_stream builds its index; the index is
// loaded, every entry must point at a data chunk header with the decoded offset the chunk table gives, Find must return the entry at
// or before seeded offsets, and the index must be found behind the stream by kc_s2_index_load_stream.  Then seeded mutations of the
// index (bit flip, truncation, insertion, deletion) go through load / find, and mutations of the stream through kc_s2_index_stream and
// kc_s2_index_load_stream.  Every buffer handed in is a heap block of exactly its size, so a read past its end is a sanitizer report.
// Exit status 0: clean.
#include <algorithm>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../include/kcgpu.h"

namespace {

struct Rng {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
    uint32_t below(uint32_t n) { return n ? next() % n : 0; }
};

uint64_t g_inputs = 0, g_loaded = 0, g_refused = 0;

struct Exact {  // a heap block of exactly n bytes
    uint8_t* p;
    uint64_t n;
    explicit Exact(const std::vector<uint8_t>& v) : p((uint8_t*)malloc(v.size() ? v.size() : 1)), n(v.size()) { if (n) memcpy(p, v.data(), n); }
    ~Exact() { free(p); }
};

std::vector<uint8_t> frame(const std::vector<uint8_t>& data, size_t block) {
    std::vector<uint8_t> s = {0xff, 6, 0, 0, 'S', '2', 's', 'T', 'w', 'O'};
    for (size_t at = 0; at < data.size(); at += block) {
        const size_t n = std::min(block, data.size() - at), cl = n + 4;
        const uint8_t h[8] = {1, (uint8_t)cl, (uint8_t)(cl >> 8), (uint8_t)(cl >> 16), 0, 0, 0, 0};  // (the CRC is not read by the index code)
        s.insert(s.end(), h, h + 8);
        s.insert(s.end(), data.begin() + at, data.begin() + at + n);
    }
    return s;
}

std::vector<uint8_t> mutate(const std::vector<uint8_t>& base, Rng& r) {
    std::vector<uint8_t> b = base;
    if (b.empty()) return b;
    switch (r.below(4)) {
        case 0: b[r.below((uint32_t)b.size())] ^= (uint8_t)(1u << r.below(8)); break;
        case 1: b.resize(r.below((uint32_t)b.size())); break;
        case 2: b.insert(b.begin() + r.below((uint32_t)b.size() + 1), (uint8_t)r.next()); break;
        default: b.erase(b.begin() + r.below((uint32_t)b.size())); break;
    }
    return b;
}

bool fail(const char* what) {
    fprintf(stderr, "s2_range_check: %s\n", what);
    return false;
}

// load + find over one (possibly hostile) index; returns the load's status
int load_and_find(const std::vector<uint8_t>& index, Rng& r) {
    Exact e(index);
    kc_s2_index* ix = kc_s2_index_new();
    uint64_t used = 0;
    const int rc = kc_s2_index_load(ix, e.p, e.n, &used);
    g_inputs++;
    if (rc) g_refused++; else g_loaded++;
    const int64_t total = kc_s2_index_total_uncompressed(ix);
    for (int k = 0; k < 8; k++) {  // (after a failed load too: the index is partly overwritten, as the reference's is)
        int64_t c = 0, u = 0;
        const int64_t off = k == 0 ? 0 : k == 1 ? total : k == 2 ? -1 : (int64_t)r.next() * (int64_t)(r.below(3) ? 1 : -1);
        (void)kc_s2_index_find(ix, off, &c, &u);
    }
    std::vector<int64_t> cc(kc_s2_index_entries(ix, nullptr, nullptr, 0) + 1), uu(cc.size());
    (void)kc_s2_index_entries(ix, cc.data(), uu.data(), (uint32_t)cc.size());
    kc_s2_index_free(ix);
    return rc;
}

bool run_stream(const std::vector<uint8_t>& stream, size_t block, uint32_t per_index, Rng& r) {
    bool good = true;
    Exact s(stream);
    std::vector<uint8_t> index(1 << 16);
    uint64_t n = 0;
    uint32_t st = 0;
    if (kc_s2_index_stream(s.p, s.n, index.data(), index.size(), &n, &st) != KC_OK || st) return fail("kc_s2_index_stream refused a well-formed stream");
    index.resize(n);
    g_inputs++;
    {  // the pristine index: loads, points at chunk headers, answers Find like a scan of its entries
        Exact e(index);
        kc_s2_index* ix = kc_s2_index_new();
        uint64_t used = 0;
        if (kc_s2_index_load(ix, e.p, e.n, &used) != KC_S2I_OK || used != e.n) good = fail("the index of kc_s2_index_stream does not load");
        const uint64_t total = stream.size() > 10 ? (uint64_t)(stream.size() - 10) - 8 * ((stream.size() - 10 + block + 7) / (block + 8)) : 0;
        if ((uint64_t)kc_s2_index_total_uncompressed(ix) != total) good = fail("total uncompressed differs from the chunk table's");
        const uint32_t ne = kc_s2_index_entries(ix, nullptr, nullptr, 0);
        std::vector<int64_t> cc(ne + 1), uu(ne + 1);
        kc_s2_index_entries(ix, cc.data(), uu.data(), ne);
        for (uint32_t k = 0; k < ne && good; k++) {
            if (cc[k] < 10 || (uint64_t)cc[k] >= stream.size() || stream[(size_t)cc[k]] != 1) good = fail("an entry does not point at a data chunk header");
            else if ((uint64_t)(cc[k] - 10) / (block + 8) * block != (uint64_t)uu[k] || (uint64_t)(cc[k] - 10) % (block + 8)) good = fail("an entry's offsets disagree");
        }
        for (int k = 0; k < 64 && good; k++) {
            const int64_t off = k == 0 ? 0 : k == 1 ? (int64_t)total : (int64_t)r.below((uint32_t)total + 1);
            int64_t c = -1, u = -1, wc = 0, wu = 0;
            for (uint32_t i = 0; i < ne && uu[i] <= off; i++) { wc = cc[i]; wu = uu[i]; }
            if (kc_s2_index_find(ix, off, &c, &u) != KC_S2I_OK || c != wc || u != wu) good = fail("Find differs from a scan of the entries");
            if (kc_s2_index_find(ix, off - (int64_t)total - 1, &c, &u) != (off ? KC_S2I_OK : KC_S2I_UNEXPECTED_EOF) && total) good = fail("Find from the end");
        }
        int64_t c, u;
        if (kc_s2_index_find(ix, (int64_t)total + 1, &c, &u) != KC_S2I_UNEXPECTED_EOF) good = fail("Find past the end");
        kc_s2_index_free(ix);
        std::vector<uint8_t> both = stream;
        both.insert(both.end(), index.begin(), index.end());
        Exact b(both);
        ix = kc_s2_index_new();
        if (kc_s2_index_load_stream(ix, b.p, b.n) != KC_S2I_OK) good = fail("the index is not found behind its stream");
        if (kc_s2_index_load_stream(ix, s.p, s.n) == KC_S2I_OK) good = fail("an index was found in a stream without one");
        kc_s2_index_free(ix);
        g_inputs += 2;
    }
    for (uint32_t k = 0; k < per_index; k++) {
        std::vector<uint8_t> m = mutate(index, r);
        if (r.below(4) == 0) m = mutate(m, r);
        load_and_find(m, r);
        std::vector<uint8_t> both = stream.size() > 4096 ? std::vector<uint8_t>(stream.end() - 4096, stream.end()) : stream;  // LoadStream reads the tail
        both.insert(both.end(), m.begin(), m.end());
        Exact b(both);
        kc_s2_index* ix = kc_s2_index_new();
        (void)kc_s2_index_load_stream(ix, b.p, b.n);
        kc_s2_index_free(ix);
        g_inputs++;
    }
    for (uint32_t k = 0; k < per_index / 4 + 1; k++) {  // hostile streams through IndexStream, into a buffer that may be too small
        const std::vector<uint8_t> m = mutate(stream, r);
        Exact b(m);
        const uint64_t cap = r.below(2) ? 1 << 16 : r.below(40);
        std::vector<uint8_t> out(cap ? cap : 1);
        uint64_t need = 0;
        uint32_t st2 = 0;
        const kc_status rc = kc_s2_index_stream(b.p, b.n, cap ? out.data() : nullptr, cap, &need, &st2);
        if (rc != KC_OK && rc != KC_ERR_DST_TOO_SMALL) good = fail("kc_s2_index_stream: unexpected return");
        if (rc == KC_OK && !st2) { out.resize(need); load_and_find(out, r); }
        g_inputs++;
    }
    return good;
}

}  // namespace

int main(int argc, char** argv) {
    uint32_t per_index = 400;
    uint64_t seed = 0x52D0002;
    std::vector<std::string> files;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "-n") && i + 1 < argc) per_index = (uint32_t)strtoul(argv[++i], nullptr, 0);
        else if (!strcmp(argv[i], "-s") && i + 1 < argc) seed = strtoull(argv[++i], nullptr, 0);
        else files.push_back(argv[i]);
    }
    if (files.empty()) { fprintf(stderr, "usage: s2_range_check [-n mutations-per-index] [-s seed] file...\n"); return 2; }
    bool good = true;
    for (const std::string& f : files) {
        FILE* fp = fopen(f.c_str(), "rb");
        if (!fp) { fprintf(stderr, "s2_range_check: cannot read %s\n", f.c_str()); return 2; }
        std::vector<uint8_t> base;
        uint8_t tmp[65536];
        size_t got;
        while ((got = fread(tmp, 1, sizeof(tmp), fp)) > 0) base.insert(base.end(), tmp, tmp + got);
        fclose(fp);
        if (base.empty()) continue;
        Rng r{seed ^ (uint64_t)base.size() * 0x9E3779B97F4A7C15ull};
        good = run_stream(frame(base, 1 << 10), 1 << 10, per_index, r) && good;
        good = run_stream(frame(base, 4 << 10), 4 << 10, per_index, r) && good;
        std::vector<uint8_t> big;
        while (big.size() < (3u << 20)) big.insert(big.end(), base.begin(), base.end());
        big.resize(3u << 20);
        good = run_stream(frame(big, 64 << 10), 64 << 10, per_index, r) && good;
    }
    printf("s2_range_check: %llu inputs over %zu files (%llu indexes loaded, %llu refused): %s\n", (unsigned long long)g_inputs, files.size(),
           (unsigned long long)g_loaded, (unsigned long long)g_refused, good ? "clean" : "FAILED");
    return good ? 0 : 1;
}
