// stateless_check — a stand-alone memory-error hunt for the stateless writers: the gather, match, plan, chain, emit and edge kernels
// of compress_amd/csrc/kc_flate_stateless.hip compiled for the CPU wave emulator, under the host sequence that ships
// (compress_amd/csrc/kc_stateless_host.h), linked into ONE ordinary executable that is built with -fsanitize=address,undefined and
// run on the host.  TEST INFRASTRUCTURE; nothing of it is loaded into another process and nothing of it runs on a device.
//
//   python tools/stateless_dump_inputs.py tools/_build/stateless_inputs
//   g++ -O1 -g -std=c++17 -x c++ -fsanitize=address,undefined -fno-omit-frame-pointer -I tools/hipemu \
//       tools/stateless_check_main.cpp tools/hipemu/hipemu.cpp -o tools/_build/stateless_check -ldl -lpthread
//   ASAN_OPTIONS=detect_leaks=0 tools/_build/stateless_check tools/_build/stateless_inputs/*
// (the emulator keeps its lanes' fiber stacks until the process ends: the leak check at exit is off, every other check is on)
//
// Every file is one input.  All files go through the sequence as ONE batch and in batches of 5, as flate with and without eof and as
// gzip, without a dictionary and behind dictionaries of 1, 100 and 8192 bytes (the head of the largest input), with dst at every
// offset 0..3 from the start of its heap block.  The inputs, every device buffer — the token scratch among them — and the output live
// in heap blocks of exactly their sizes, so a read past an input's end, a token beyond a block's share, a word access over the end of
// dst or a write outside the planned layout is a sanitizer report.  The program itself checks what needs no judge: the sizes respect
// kc_flate_stateless_bound, a capacity one byte short is refused with nothing written, and a scratch budget that cuts the batch into
// groups gives the same bytes.  Exit status 0: clean.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../compress_amd/csrc/kc_flate_stateless.hip"
#include "../compress_amd/csrc/kc_stateless_host.h"

namespace {

// the sequence's device over plain memory: every buffer a heap block of exactly the size asked for
struct HeapDevice : KcDecDevice {
    std::vector<void*> buf;
    std::vector<size_t> cap;
    uint64_t limit = UINT64_MAX;
    int reserve(int which, size_t bytes, void** p) override {
        if ((size_t)which >= buf.size()) { buf.resize(which + 1, nullptr); cap.resize(which + 1, 0); }
        if (cap[which] != bytes || !buf[which]) {
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
    uint64_t budget() override { return limit; }
    ~HeapDevice() override { for (void* b : buf) free(b); }
};

uint64_t g_calls = 0, g_inputs = 0;

bool fail(const char* what) {
    fprintf(stderr, "stateless_check: %s\n", what);
    return false;
}

// one batch; *out: the bytes written (the whole dst range)
bool run(const std::vector<std::vector<uint8_t>>& inputs, const KcSlOpts& o, uint32_t shift, uint64_t budget, std::vector<uint8_t>* out, int* batches) {
    const uint32_t n = (uint32_t)inputs.size();
    std::vector<uint64_t> in_off(n + 1, 0), out_off(n + 1, 0);
    uint64_t bound = 0;
    for (uint32_t i = 0; i < n; i++) {
        in_off[i + 1] = in_off[i] + inputs[i].size();
        bound += kc_sl_bound(inputs[i].size(), o.gzip ? 0 : o.dict.size()) + (o.gzip ? KCSL_GZIP_EXTRA : 0);
    }
    uint8_t* src = (uint8_t*)malloc(in_off[n] ? in_off[n] : 1);  // exactly the inputs
    for (uint32_t i = 0; i < n; i++) if (!inputs[i].empty()) memcpy(src + in_off[i], inputs[i].data(), inputs[i].size());
    bool good = true;
    // the sizes first (a capacity of 0 is refused with the layout), then a block of exactly the total
    {
        HeapDevice dev;
        dev.limit = budget;
        KcDecTimes T;
        uint8_t none = 0xA5;
        const int rc = kc_sl_deflate(&dev, o, src, in_off.data(), n, &none, 0, out_off.data(), T);
        if (rc != KC_ERR_DST_TOO_SMALL || none != 0xA5) good = fail("a capacity of 0 was not refused clean");
    }
    const uint64_t total = out_off[n];
    if (total > bound) good = fail("the exact total is above the bound");
    for (uint32_t i = 0; i < n; i++)
        if (out_off[i + 1] - out_off[i] > kc_sl_bound(inputs[i].size(), o.gzip ? 0 : o.dict.size()) + (o.gzip ? KCSL_GZIP_EXTRA : 0)) good = fail("an input's size is above its bound");
    uint8_t* block = (uint8_t*)malloc(total + shift);
    memset(block, 0xA5, total + shift);
    if (good && total > 1) {  // one byte short: refused, nothing written
        HeapDevice dev;
        dev.limit = budget;
        KcDecTimes T;
        std::vector<uint64_t> oo(n + 1, 0);
        const int rc = kc_sl_deflate(&dev, o, src, in_off.data(), n, block + shift, total - 1, oo.data(), T);
        if (rc != KC_ERR_DST_TOO_SMALL || oo[n] != total) good = fail("a capacity one byte short was not refused with the layout");
        for (uint64_t k = 0; k < total + shift; k++) if (block[k] != 0xA5) { good = fail("a refused call wrote"); break; }
    }
    if (good) {
        HeapDevice dev;
        dev.limit = budget;
        KcDecTimes T;
        std::vector<uint64_t> oo(n + 1, 0);
        const int rc = kc_sl_deflate(&dev, o, src, in_off.data(), n, block + shift, total, oo.data(), T);
        if (rc != KC_OK || oo != out_off) good = fail("the exact capacity was refused, or the layout changed");
        for (uint32_t k = 0; k < shift; k++) if (block[k] != 0xA5) good = fail("a write in front of dst");
        if (batches) *batches = T.batches;
        if (out) out->assign(block + shift, block + shift + total);
    }
    g_calls++;
    g_inputs += n;
    free(block);
    free(src);
    return good;
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

}  // namespace

int main(int argc, char** argv) {
    std::vector<std::vector<uint8_t>> all;
    for (int i = 1; i < argc; i++) {
        std::vector<uint8_t> b;
        if (!read_file(argv[i], b)) { fprintf(stderr, "stateless_check: cannot read %s\n", argv[i]); return 2; }
        all.push_back(b);
    }
    if (all.empty()) { fprintf(stderr, "usage: stateless_check file...\n"); return 2; }
    all.push_back({});  // an empty input, last in its batch
    size_t largest = 0;
    for (size_t k = 0; k < all.size(); k++)
        if (all[k].size() > all[largest].size()) largest = k;
    // room for the largest input and a quarter more: its tokens, its records, its dictionary slot
    const uint64_t need = all[largest].size() * 4 + (kc_sl_records(all[largest].size(), 0) + 1) * (sizeof(KcSlBlock) + 16) + KCSL_COMB + KCSL_MAX_DICT + 4096;
    const size_t dict_lens[4] = {0, 1, 100, 8192};
    bool good = true;
    uint32_t shift = 0;
    for (int d = 0; d < 4; d++)
        for (uint32_t mode = 0; mode < 3; mode++) {  // eof, non-eof, gzip
            if (mode == 2 && d != 0) continue;
            KcSlOpts o;
            o.gzip = mode == 2; o.eof = mode == 0;
            if (dict_lens[d] && all[largest].size() >= dict_lens[d]) o.dict.assign(all[largest].begin(), all[largest].begin() + dict_lens[d]);
            std::vector<uint8_t> whole, cut;
            int batches = 0;
            good = run(all, o, shift++ & 3, UINT64_MAX, &whole, nullptr) && good;
            good = run(all, o, shift++ & 3, need + (need >> 2), &cut, &batches) && good;
            if (whole != cut) good = fail("a batch cut to the scratch budget wrote other bytes");
            if (batches < 2) good = fail("the scratch budget did not cut the batch");
            for (size_t k = 0; k < all.size(); k += 5) {
                std::vector<std::vector<uint8_t>> part(all.begin() + k, all.begin() + (k + 5 < all.size() ? k + 5 : all.size()));
                good = run(part, o, shift++ & 3, UINT64_MAX, nullptr, nullptr) && good;
            }
        }
    printf("stateless_check: %llu inputs in %llu batches over %zu files: %s\n", (unsigned long long)g_inputs, (unsigned long long)g_calls, all.size() - 1,
           good ? "clean" : "FAILED");
    return good ? 0 : 1;
}
