// zlib_check — a stand-alone memory-error hunt for the zlib inflate kernels: kc_zlib_size_kernel, kc_zlib_write_kernel and what they
// run (fl_zlib_input, fl_inflate, fl_adler32_wave of compress_amd/csrc/kc_flate_dev.h) compiled for the CPU wave emulator and linked
// into ONE ordinary executable that is built with -fsanitize=address,undefined and run on the host.  TEST INFRASTRUCTURE; nothing of it
// is loaded into another process and nothing of it runs on a device.
//
//   python tools/zlib_dump_inputs.py tools/_build/zlib_inputs
//   g++ -O1 -g -std=c++17 -x c++ -fsanitize=address,undefined -fno-omit-frame-pointer -I tools/hipemu \
//       tools/zlib_check_main.cpp tools/hipemu/hipemu.cpp -o tools/_build/zlib_check -ldl -lpthread
//   ASAN_OPTIONS=detect_leaks=0 tools/_build/zlib_check [-n mutations-per-file] [-s seed] tools/_build/zlib_inputs/*
// (the emulator keeps its lanes' fiber stacks until the process ends: the leak check at exit is off, every other check is on)
//
// A file is a stream, or — where its name ends in ".dict" — the preset dictionary of the stream file of the same name without that
// ending.  Every stream is inflated as it is (with its dictionary, with none, and with a dictionary of one byte), followed by seeded
// mutations of it (bit flips, truncations, insertions, deletions, overwritten runs) in batches of 8.  The inputs, the dictionary's
// tail and the output live in heap blocks of exactly their sizes, the output at every offset 0..3 from its block's start, so a read
// past an input's end, in front of or behind the range the Adler-32 sums, or a write outside the planned range is a sanitizer
// report.  The program itself checks what needs no judge: both passes agree on sizes and verdicts short of the checksum, a failed
// input leaves zeroes or nothing, and the Adler-32 the write pass accepted is the host's plain one.  Exit status 0: clean.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../compress_amd/csrc/kc_flate_inflate.hip"
#include "../compress_amd/csrc/kc_flate_host.h"

namespace {

struct Rng {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
    uint32_t below(uint32_t n) { return n ? next() % n : 0; }
};

uint64_t g_cases = 0, g_ok = 0, g_refused = 0;

bool fail(const char* what, uint32_t i) {
    fprintf(stderr, "zlib_check: %s (input %u of its batch)\n", what, i);
    return false;
}

// one batch through the sizing pass, the layout and the write pass, as kc_flate_host.h runs them; dst begins `shift` bytes into its block
bool run_batch(const std::vector<std::vector<uint8_t>>& inputs, const std::vector<uint8_t>& dict, uint32_t shift) {
    const uint32_t n = (uint32_t)inputs.size();
    std::vector<uint64_t> in_off(n + 1, 0);
    for (uint32_t i = 0; i < n; i++) in_off[i + 1] = in_off[i] + inputs[i].size();
    uint8_t* src = (uint8_t*)malloc(in_off[n] ? in_off[n] : 1);  // exactly the inputs: a read behind the last one is a report
    for (uint32_t i = 0; i < n; i++) if (!inputs[i].empty()) memcpy(src + in_off[i], inputs[i].data(), inputs[i].size());
    const uint64_t keep = dict.size() > 32768 ? 32768 : dict.size();
    uint8_t* tail = (uint8_t*)malloc(keep ? keep : 1);             // exactly the window's worth
    if (keep) memcpy(tail, dict.data() + (dict.size() - keep), keep);
    std::vector<uint64_t> size(n), used(n), out0(n + 1, 0);
    std::vector<uint32_t> st(n), members(n), wst(n, 0xA7A7A7A7u);
    KcFlateParams P;
    memset(&P, 0, sizeof(P));
    P.src = src; P.in_off = in_off.data(); P.n = n; P.gzip = KCFL_FMT_ZLIB; P.dict = keep ? tail : nullptr; P.dict_len = (uint32_t)keep;
    P.dict_id = kc_fl_adler32(dict.data(), dict.size());
    P.size = size.data(); P.status = st.data(); P.consumed = used.data(); P.members = members.data();
    kc_launch_zlib_size(P, nullptr);
    bool good = true;
    for (uint32_t i = 0; i < n; i++) {
        if (st[i] > KCFL_DICTIONARY) good = fail("a verdict is no status class", i);
        if ((st[i] != 0) != (members[i] == 0) || (st[i] && (size[i] || used[i])) || used[i] > inputs[i].size()) good = fail("the sizing pass contradicts itself", i);
        out0[i + 1] = out0[i] + size[i];
    }
    const uint64_t cap = out0[n];
    uint8_t* block = (uint8_t*)malloc(cap + shift ? cap + shift : 1);  // exactly the planned layout, `shift` bytes in
    memset(block, 0xA5, cap + shift ? cap + shift : 1);
    uint8_t* dst = block + shift;
    P.out0 = out0.data(); P.dst = dst; P.wstatus = wst.data();
    if (good) kc_launch_zlib_write(P, nullptr);
    for (uint32_t i = 0; i < n && good; i++) {
        const uint32_t v = members[i] ? wst[i] : st[i];
        if (members[i] && v != KCFL_OK && v != KCFL_CHECKSUM) good = fail("the write pass found what the sizing pass did not", i);
        if (v == KCFL_OK) {
            const uint32_t want = (uint32_t)inputs[i][used[i] - 4] << 24 | (uint32_t)inputs[i][used[i] - 3] << 16 | (uint32_t)inputs[i][used[i] - 2] << 8 | inputs[i][used[i] - 1];
            if (kc_fl_adler32(dst + out0[i], size[i]) != want) good = fail("an accepted Adler-32 is not the host's", i);
        } else {
            for (uint64_t k = 0; k < size[i]; k++) if (dst[out0[i] + k]) { good = fail("a failed input left decoded bytes", i); break; }
        }
        g_cases++;
        if (v) g_refused++; else g_ok++;
    }
    for (uint32_t k = 0; k < shift; k++) if (block[k] != 0xA5) good = fail("a write in front of dst", k);
    free(block);
    free(tail);
    free(src);
    return good;
}

std::vector<uint8_t> mutate(const std::vector<uint8_t>& base, Rng& r) {
    std::vector<uint8_t> b = base;
    const uint32_t rounds = 1 + r.below(3);
    for (uint32_t k = 0; k < rounds && !b.empty(); k++) {
        switch (r.below(6)) {
            case 0: b[r.below((uint32_t)b.size())] ^= (uint8_t)(1u << r.below(8)); break;
            case 1: b.resize(r.below((uint32_t)b.size())); break;
            case 2: b.insert(b.begin() + r.below((uint32_t)b.size() + 1), (uint8_t)r.next()); break;
            case 3: b.erase(b.begin() + r.below((uint32_t)b.size())); break;
            case 4: { const uint32_t at = r.below((uint32_t)b.size()), len = 1 + r.below(8); for (uint32_t i = at; i < at + len && i < b.size(); i++) b[i] = (uint8_t)r.next(); break; }
            default: b[r.below(b.size() < 16 ? (uint32_t)b.size() : 16u)] = (uint8_t)r.next(); break;  // near the front: header, DICTID, first block header
        }
    }
    return b;
}

bool read_file(const std::string& f, std::vector<uint8_t>& out) {
    FILE* fp = fopen(f.c_str(), "rb");
    if (!fp) return false;
    uint8_t tmp[65536];
    size_t got;
    while ((got = fread(tmp, 1, sizeof(tmp), fp)) > 0) out.insert(out.end(), tmp, tmp + got);
    fclose(fp);
    return true;
}

bool ends_with(const std::string& s, const char* e) { return s.size() >= strlen(e) && s.compare(s.size() - strlen(e), strlen(e), e) == 0; }

}  // namespace

int main(int argc, char** argv) {
    uint32_t per_file = 200;
    uint64_t seed = 0x21B0001;
    std::vector<std::string> files;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "-n") && i + 1 < argc) per_file = (uint32_t)strtoul(argv[++i], nullptr, 0);
        else if (!strcmp(argv[i], "-s") && i + 1 < argc) seed = strtoull(argv[++i], nullptr, 0);
        else if (!ends_with(argv[i], ".dict")) files.push_back(argv[i]);
    }
    if (files.empty()) { fprintf(stderr, "usage: zlib_check [-n mutations-per-file] [-s seed] file...\n"); return 2; }
    bool good = true;
    uint32_t shift = 0;
    for (const std::string& f : files) {
        std::vector<uint8_t> base, dict;
        if (!read_file(f, base)) { fprintf(stderr, "zlib_check: cannot read %s\n", f.c_str()); return 2; }
        (void)read_file(f + ".dict", dict);  // (absent: no dictionary)
        Rng r{seed ^ (uint64_t)base.size() * 0x9E3779B97F4A7C15ull};
        for (uint32_t s = 0; s < 4; s++) good = run_batch({base}, dict, s) && good;
        good = run_batch({base}, {}, 1) && good;
        good = run_batch({base}, {0x5A}, 2) && good;
        for (uint32_t k = 0; k < per_file; k += 8) {  // batches of 8: neighbours in one src and one dst
            std::vector<std::vector<uint8_t>> batch;
            for (uint32_t j = 0; j < 8 && k + j < per_file; j++) batch.push_back(mutate(base, r));
            good = run_batch(batch, dict, shift++ & 3) && good;
        }
    }
    printf("zlib_check: %llu inputs over %zu files (%llu decoded, %llu refused): %s\n", (unsigned long long)g_cases, files.size(),
           (unsigned long long)g_ok, (unsigned long long)g_refused, good ? "clean" : "FAILED");
    return good ? 0 : 1;
}
