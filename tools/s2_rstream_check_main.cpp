// s2_rstream_check — a stand-alone memory-error hunt for the S2 stream reader: its kernel (compress_amd/csrc/kc_s2_rstream.hip) and the
// state machine that drives it (kc_s2rstream_host.h, with the partial chunk walk of kc_s2_plan_dev.h) compiled for the CPU wave
// emulator and linked into ONE ordinary executable that is built with -fsanitize=address,undefined and run on the host.  TEST
// INFRASTRUCTURE; nothing of it is loaded into another process and nothing of it runs on a device.
//
//   g++ -O1 -g -std=c++17 -x c++ -fsanitize=address,undefined -fno-omit-frame-pointer -I tools/hipemu \
//       tools/s2_rstream_check_main.cpp tools/hipemu/hipemu.cpp -o tools/_build/s2_rstream_check -ldl -lpthread
//   python tools/s2_rstream_dump_inputs.py DIR      (the item-1 streams and the 480 mutations of tests/s2_decode_cases.py as files)
//   ASAN_OPTIONS=detect_leaks=0 tools/_build/s2_rstream_check [-n mutations-per-file] [-s seed] DIR/item*.s2
//   ASAN_OPTIONS=detect_leaks=0 tools/_build/s2_rstream_check -n 0 DIR/mut*.s2
// (the emulator keeps its lanes' fiber stacks until the process ends: the leak check at exit would name only them)
//
// Every file named is read as a stream — whole, in pieces of 7 and of 1000 bytes — at 4096, 3 and 1 chunks per launch, with and
// without a pending skip, followed by seeded mutations of it in the six kinds of tests/s2_decode_cases.py (a bit flip anywhere, a
// truncation, a bit flip in a chunk header, a bit flip in the 16 bytes behind a header, an inserted byte, a deleted byte).  What is
// presented to a call, the caller's dst and every device buffer live in heap blocks of exactly their sizes, so a read past the input or
// a write outside the staged bytes, the window or dst is a sanitizer report.  The program checks what needs no judge: consumed and
// produced stay inside what was given, a failed stream stays failed, and a file decodes to the same bytes and status whichever way it
// is cut; with a skip of n, to the bytes behind the first n.  Exit status 0: clean.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../compress_amd/csrc/kc_s2_rstream.hip"
#include "../compress_amd/csrc/kc_s2rstream_host.h"

namespace {

struct Rng {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
    uint32_t below(uint32_t n) { return n ? next() % n : 0; }
};

struct HeapDevice : KcDecDevice {
    void* buf[RS_N] = {nullptr};
    size_t cap[RS_N] = {0};
    int reserve(int which, size_t bytes, void** p) override {  // exactly what is asked for, every time
        free(buf[which]);
        buf[which] = malloc(bytes ? bytes : 1);
        cap[which] = bytes;
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

uint32_t max_buf_of(uint32_t n) {  // MaxEncodedLen(n) + 4 (s2/encode.go:389-418)
    uint64_t v = n;
    for (uint32_t x = n; x > 0; x >>= 7) v++;
    v += n == 0 ? 0 : n < 60 ? 1 : n < (1u << 8) ? 2 : n < (1u << 16) ? 3 : n < (1u << 24) ? 4 : 5;
    return (uint32_t)v + 4;
}

uint64_t g_streams = 0, g_ok = 0, g_refused = 0;

// one stream; piece 0: whole.  Returns false on a broken promise of the interface.
bool run(const std::vector<uint8_t>& data, uint32_t chunks, uint32_t piece, uint64_t skip, std::vector<uint8_t>* out, uint32_t* status) {
    HeapDevice dev;
    KcS2rStream s;
    s.dev = &dev;
    s.o.max_buf = max_buf_of(s.o.max_block);
    s.o.chunks = chunks;
    s.start();
    s.skip_left = skip;
    const uint64_t dst_cap = 64u << 10;
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
            const bool small = rc == KC_ERR_DST_TOO_SMALL && consumed == 0 && produced == 0;  // (a mutated header may state a chunk above dst)
            bool good = (rc == 0 || small) && consumed <= pend.size() && produced <= dst_cap;
            if (good) out->insert(out->end(), dst, dst + produced);
            free(src);
            free(dst);
            if (!good) { fprintf(stderr, "feed: rc %d, consumed %llu of %zu, produced %llu\n", rc, (unsigned long long)consumed, pend.size(), (unsigned long long)produced); return false; }
            if (small) { *status = 0xFFFFu; g_refused++; return true; }
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
    if (!pend.empty()) { fprintf(stderr, "a clean end left %zu bytes unconsumed\n", pend.size()); return false; }
    g_ok++;
    return true;
}

std::vector<size_t> headers(const std::vector<uint8_t>& b) {
    std::vector<size_t> h;
    size_t pos = 0;
    while (pos + 4 <= b.size()) {
        h.push_back(pos);
        pos += 4 + ((size_t)b[pos + 1] | (size_t)b[pos + 2] << 8 | (size_t)b[pos + 3] << 16);
    }
    return h;
}

// every way of cutting one input gives the same bytes and status
bool all_ways(const std::vector<uint8_t>& data, const char* what, int k) {
    std::vector<uint8_t> whole, cut;
    uint32_t st = 0, st2 = 0;
    if (!run(data, 4096, 0, 0, &whole, &st)) return false;
    for (uint32_t chunks : {4096u, 3u, 1u})
        for (uint32_t piece : {7u, 1000u}) {
            if (!run(data, chunks, piece, 0, &cut, &st2)) return false;
            if (st2 != st || cut != whole) {
                fprintf(stderr, "%s [%d]: %u chunks per launch, pieces of %u: status %u with %zu bytes, whole: status %u with %zu bytes\n", what, k, chunks, piece, st2,
                        cut.size(), st, whole.size());
                return false;
            }
        }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    int nmut = 36;
    Rng rng{0x52D0001ull};
    std::vector<std::string> files;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "-n") && i + 1 < argc) nmut = atoi(argv[++i]);
        else if (!strcmp(argv[i], "-s") && i + 1 < argc) rng.s = strtoull(argv[++i], nullptr, 0);
        else files.push_back(argv[i]);
    }
    if (files.empty()) { fprintf(stderr, "usage: s2_rstream_check [-n mutations] [-s seed] file.s2...\n"); return 2; }
    for (const std::string& f : files) {
        FILE* fp = fopen(f.c_str(), "rb");
        if (!fp) { fprintf(stderr, "%s: cannot open\n", f.c_str()); return 2; }
        std::vector<uint8_t> data;
        uint8_t tmp[65536];
        size_t n;
        while ((n = fread(tmp, 1, sizeof(tmp), fp)) > 0) data.insert(data.end(), tmp, tmp + n);
        fclose(fp);
        if (!all_ways(data, f.c_str(), -1)) return 1;
        // a pending skip: the bytes behind it, whichever way the input is cut
        std::vector<uint8_t> whole, part;
        uint32_t st = 0, st2 = 0;
        if (!run(data, 4096, 0, 0, &whole, &st)) return 1;
        if (st == 0 && !whole.empty()) {
            for (int k = 0; k < 4; k++) {
                const uint64_t skip = rng.below((uint32_t)whole.size() + 1);
                if (!run(data, k & 1 ? 1u : 4096u, k & 2 ? 7u : 0u, skip, &part, &st2)) return 1;
                if (st2 != 0 || part.size() != whole.size() - skip || memcmp(part.data(), whole.data() + skip, part.size()) != 0) {
                    fprintf(stderr, "%s: skip %llu: status %u with %zu bytes\n", f.c_str(), (unsigned long long)skip, st2, part.size());
                    return 1;
                }
            }
        }
        for (int m = 0; m < nmut && !data.empty(); m++) {
            std::vector<uint8_t> mu = data;
            const std::vector<size_t> hs = headers(mu);
            switch (m % 6) {
                case 0: mu[rng.below((uint32_t)mu.size())] ^= (uint8_t)(1u << rng.below(8)); break;
                case 1: mu.resize(rng.below((uint32_t)mu.size())); break;
                case 2: if (!hs.empty()) mu[hs[rng.below((uint32_t)hs.size())] + rng.below(4)] ^= (uint8_t)(1u << rng.below(8)); break;
                case 3: if (!hs.empty()) { size_t p = hs[rng.below((uint32_t)hs.size())] + 4 + rng.below(16); if (p >= mu.size()) p = mu.size() - 1; mu[p] ^= (uint8_t)(1u << rng.below(8)); } break;
                case 4: mu.insert(mu.begin() + rng.below((uint32_t)mu.size() + 1), (uint8_t)rng.below(256)); break;
                default: mu.erase(mu.begin() + rng.below((uint32_t)mu.size())); break;
            }
            if (!all_ways(mu, f.c_str(), m)) return 1;
            if (!run(mu, m & 1 ? 1u : 4096u, m & 2 ? 1000u : 7u, 1 + rng.below(20000), &part, &st2)) return 1;
        }
    }
    printf("s2_rstream_check: %llu streams, %llu read to a clean end, %llu refused, no broken promise\n", (unsigned long long)g_streams,
           (unsigned long long)g_ok, (unsigned long long)g_refused);
    return 0;
}
