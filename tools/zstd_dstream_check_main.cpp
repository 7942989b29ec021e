// zstd_dstream_check — a stand-alone memory-error hunt for the zstd stream reader: its three kernels (compress_amd/csrc/
// kc_zstd_dstream.hip) and the state machine that drives them (kc_zdstream_host.h) compiled for the CPU wave emulator and linked into
// ONE ordinary executable that is built with -fsanitize=address,undefined and run on the host.  TEST INFRASTRUCTURE; nothing of it is
// loaded into another process and nothing of it runs on a device.
//
//   g++ -O1 -g -std=c++17 -x c++ -fsanitize=address,undefined -fno-omit-frame-pointer -I tools/hipemu \
//       tools/zstd_dstream_check_main.cpp tools/hipemu/hipemu.cpp -o tools/_build/zstd_dstream_check -ldl -lpthread
//   ASAN_OPTIONS=detect_leaks=0 tools/_build/zstd_dstream_check [-n mutations-per-file] [-s seed] file.zst...
// (the emulator keeps its lanes' fiber stacks until the process ends: the leak check at exit would name only them)
//
// Every file named is read as a stream — whole, and in pieces of a seeded size — at 512 blocks and at one block per launch, followed by
// seeded mutations of it (bit flips, truncations, overwritten bytes).  What is presented to a call, the caller's dst and every device
// buffer live in heap blocks of exactly their sizes, so a read past the input or a write outside a slice, the history buffer or dst is a
// sanitizer report.  The program checks what needs no judge: consumed and produced stay inside what was given, a failed stream stays
// failed, and the unmutated file decodes to the same bytes whichever way it is cut.  Exit status 0: clean.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../compress_amd/csrc/kc_zstd_dstream.hip"
#include "../compress_amd/csrc/kc_zdstream_host.h"

namespace {

struct Rng {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
    uint32_t below(uint32_t n) { return n ? next() % n : 0; }
};

struct HeapDevice : KcDecDevice {
    void* buf[ZS_N] = {nullptr};
    size_t cap[ZS_N] = {0};
    int reserve(int which, size_t bytes, void** p) override {
        if (cap[which] < bytes || !buf[which]) {
            free(buf[which]);
            buf[which] = malloc(bytes ? bytes : 1);
            cap[which] = bytes;
        }
        *p = buf[which];
        return 0;
    }
    int h2d(void* d, const void* h, size_t n) override { if (n) memcpy(d, h, n); return 0; }
    int d2h(void* h, const void* d, size_t n) override { if (n) memcpy(h, d, n); return 0; }
    int d2d(void* d, const void* s, size_t n) override { if (n) memcpy(d, s, n); return 0; }
    int zero(void* d, size_t n) override { if (n) memset(d, 0, n); return 0; }
    int sync() override { return 0; }
    ~HeapDevice() override { for (void* b : buf) free(b); }
};

uint64_t g_streams = 0, g_ok = 0, g_refused = 0;

// one stream; piece 0: whole.  Returns false on a broken promise of the interface.
bool run(const std::vector<uint8_t>& data, uint32_t blocks, uint32_t piece, std::vector<uint8_t>* out, uint32_t* status) {
    HeapDevice dev;
    KcZsStream s;
    s.dev = &dev;
    s.o.blocks = blocks;
    const uint64_t dst_cap = 128u << 10;
    std::vector<uint8_t> pend;
    size_t pos = 0;
    out->clear();
    *status = 0;
    g_streams++;
    for (;;) {
        const size_t take = piece ? (piece < data.size() - pos ? piece : data.size() - pos) : data.size() - pos;
        pend.insert(pend.end(), data.begin() + pos, data.begin() + pos + take);
        pos += take;
        const int eof = pos == data.size();
        for (;;) {
            uint8_t* src = (uint8_t*)malloc(pend.size() ? pend.size() : 1);  // exactly what is presented
            if (!pend.empty()) memcpy(src, pend.data(), pend.size());
            uint8_t* dst = (uint8_t*)malloc(dst_cap);
            uint64_t consumed = 0, produced = 0;
            uint32_t st = 0;
            const int rc = s.feed(src, pend.size(), eof, dst, dst_cap, &consumed, &produced, &st);
            bool good = rc == 0 && consumed <= pend.size() && produced <= dst_cap;
            if (good) out->insert(out->end(), dst, dst + produced);
            free(src);
            free(dst);
            if (!good) { fprintf(stderr, "feed: rc %d, consumed %llu of %zu, produced %llu\n", rc, (unsigned long long)consumed, pend.size(), (unsigned long long)produced); return false; }
            pend.erase(pend.begin(), pend.begin() + consumed);
            if (st) {
                uint64_t c2 = 0, p2 = 0;
                uint32_t st2 = 0;
                uint8_t one = 0;
                if (s.feed(&one, 0, 1, &one, 0, &c2, &p2, &st2) != 0 || st2 != st || c2 || p2) { fprintf(stderr, "a failed stream does not stay failed\n"); return false; }
                *status = st;
                g_refused++;
                return true;
            }
            if (!consumed && !produced) break;
        }
        if (eof) break;
    }
    g_ok++;
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    int nmut = 40;
    Rng rng{0x5EED0D57ull};
    std::vector<std::string> files;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "-n") && i + 1 < argc) nmut = atoi(argv[++i]);
        else if (!strcmp(argv[i], "-s") && i + 1 < argc) rng.s = strtoull(argv[++i], nullptr, 0);
        else files.push_back(argv[i]);
    }
    if (files.empty()) { fprintf(stderr, "usage: zstd_dstream_check [-n mutations] [-s seed] file.zst...\n"); return 2; }
    for (const std::string& f : files) {
        FILE* fp = fopen(f.c_str(), "rb");
        if (!fp) { fprintf(stderr, "%s: cannot open\n", f.c_str()); return 2; }
        std::vector<uint8_t> data;
        uint8_t tmp[65536];
        size_t n;
        while ((n = fread(tmp, 1, sizeof(tmp), fp)) > 0) data.insert(data.end(), tmp, tmp + n);
        fclose(fp);
        std::vector<uint8_t> whole, cut;
        uint32_t st = 0, st2 = 0;
        if (!run(data, 512, 0, &whole, &st)) return 1;
        for (uint32_t blocks : {512u, 1u, 3u}) {
            if (!run(data, blocks, 1 + rng.below(70000), &cut, &st2)) return 1;
            if (st2 != st || cut != whole) { fprintf(stderr, "%s: %u blocks per launch, cut: status %u with %zu bytes, whole: status %u with %zu bytes\n", f.c_str(), blocks, st2, cut.size(), st, whole.size()); return 1; }
        }
        for (int m = 0; m < nmut; m++) {
            std::vector<uint8_t> mu = data;
            const uint32_t kind = rng.below(3);
            if (mu.empty()) break;
            if (kind == 0) { const uint32_t p = rng.below((uint32_t)mu.size() * 8); mu[p >> 3] ^= (uint8_t)(1u << (p & 7)); }
            else if (kind == 1) mu.resize(rng.below((uint32_t)mu.size()));
            else mu[rng.below((uint32_t)mu.size())] = (uint8_t)rng.below(256);
            if (!run(mu, m & 1 ? 1u : 512u, m & 2 ? 1 + rng.below(5000) : 0, &cut, &st2)) return 1;
        }
    }
    printf("zstd_dstream_check: %llu streams, %llu read to a clean end, %llu refused, no broken promise\n", (unsigned long long)g_streams,
           (unsigned long long)g_ok, (unsigned long long)g_refused);
    return 0;
}
