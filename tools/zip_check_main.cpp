// zip_check — a stand-alone memory-error hunt for the zip reader: the host parser (compress_amd/csrc/kc_zip_dir.cpp) and, behind it,
// the member kernels of kc_zip.hip under the host sequence of kc_zip_host.h, compiled for the CPU wave emulator and linked into ONE
// ordinary executable that is built with -fsanitize=address,undefined and run on the host.  TEST INFRASTRUCTURE; nothing of it is
// loaded into another process and nothing of it runs on a device.
//
//   python tools/zip_dump_inputs.py tools/_build/zip_inputs
//   g++ -O1 -g -std=c++17 -x c++ -fsanitize=address,undefined -fno-omit-frame-pointer -I tools/hipemu \
//       tools/zip_check_main.cpp tools/hipemu/hipemu.cpp -o tools/_build/zip_check -ldl -lpthread
//   ASAN_OPTIONS=detect_leaks=0 tools/_build/zip_check [-n mutations-per-file] [-s seed] [-k] tools/_build/zip_inputs/*
// (the emulator keeps its lanes' fiber stacks until the process ends: the leak check at exit is off, every other check is on;
//  -k: the host parser alone, without the kernels)
//
// A file is an archive, or any bytes.  Every file is parsed as it is, followed by seeded mutations of it (bit flips, overwritten
// bytes, truncations, insertions).  The buffer is a heap block of exactly the file's size, so a read of the parser past the
// buffer's end, or in front of it, is a sanitizer report; every name, comment and extra the parser hands out is read through.
// Where the directory stands, its members are read on the emulator into a heap block of exactly the planned size, and the program
// checks what needs no judge: a member that stands has the CRC-32 the table states (or the table states none), a failed one
// leaves zeroes, and the layout-only call plans the same layout.  Exit status 0: clean.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../compress_amd/csrc/kc_zip.hip"
#include "../compress_amd/csrc/kc_zip_dir.cpp"
#include "../compress_amd/csrc/kc_zip_host.h"

namespace {

struct Rng {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
    uint32_t below(uint32_t n) { return n ? next() % n : 0; }
};

// the decoders' device over heap blocks of exactly the size asked for
struct HeapDevice : KcDecDevice {
    std::vector<void*> buf;
    std::vector<size_t> cap;
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
    ~HeapDevice() override { for (void* b : buf) free(b); }
};

uint64_t g_files = 0, g_dirs = 0, g_members = 0, g_stand = 0;
bool g_kernels = true;

uint32_t crc32_plain(const uint8_t* p, uint64_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (uint64_t i = 0; i < n; i++) {
        c ^= p[i];
        for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
    }
    return ~c;
}

bool fail(const char* what, uint64_t i) {
    fprintf(stderr, "zip_check: %s (member %llu)\n", what, (unsigned long long)i);
    return false;
}

bool run_one(const std::vector<uint8_t>& data) {
    uint8_t* buf = (uint8_t*)malloc(data.size() ? data.size() : 1);  // exactly the archive: a read behind it is a report
    if (!data.empty()) memcpy(buf, data.data(), data.size());
    bool ok = true;
    kc_zip_dir* d = nullptr;
    const int st = kc_zip_dir_load(buf, data.size(), &d);
    g_files++;
    if (st != KC_ZIP_OK) {
        if (d) ok = fail("a directory handed out with an error", 0);
    } else {
        g_dirs++;
        uint64_t sum = 0;
        uint32_t cl = 0;
        const uint8_t* c = kc_zip_dir_comment(d, &cl);
        for (uint32_t k = 0; k < cl; k++) sum += c[k];
        const uint64_t n = kc_zip_dir_count(d);
        for (uint64_t i = 0; i < n; i++) {
            kc_zip_entry e;
            if (kc_zip_dir_entry(d, i, &e) != 0) { ok = fail("entry not handed out", i); break; }
            for (uint32_t k = 0; k < e.name_len; k++) sum += e.name[k];
            for (uint32_t k = 0; k < e.comment_len; k++) sum += e.comment[k];
            for (uint32_t k = 0; k < e.extra_len; k++) sum += e.extra[k];
        }
        if (sum == 0xFFFFFFFFFFFFFFFFull) puts("");  // (the sums are read)
        std::vector<kc_zip_member> mem((size_t)n + 1);
        if (kc_zip_dir_members(d, 0, n, mem.data()) != 0) ok = fail("member table not filled", 0);
        if (ok && g_kernels && n && n < 100000) {
            const uint32_t nm = (uint32_t)n;
            std::vector<uint64_t> oo0(n + 1), oo(n + 1);
            std::vector<uint32_t> s0(n, 0xEE), s1(n, 0xEE);
            KcDecTimes T;
            HeapDevice dev;
            if (kc_zp_read(&dev, buf, data.size(), mem.data(), nm, nullptr, 0, oo0.data(), s0.data(), true, T) != 0) ok = fail("layout call failed", 0);
            uint8_t* dst = (uint8_t*)malloc(oo0[n] ? oo0[n] : 1);  // exactly the layout: a write outside it is a report
            memset(dst, 0xA5, oo0[n] ? oo0[n] : 1);
            if (ok && kc_zp_read(&dev, buf, data.size(), mem.data(), nm, dst, oo0[n], oo.data(), s1.data(), false, T) != 0) ok = fail("read call failed", 0);
            for (uint32_t i = 0; ok && i < nm; i++) {
                g_members++;
                if (oo[i] != oo0[i] || oo[i + 1] != oo0[i + 1]) ok = fail("the two calls plan different layouts", i);
                const uint64_t len = oo[i + 1] - oo[i];
                if (s1[i] == 0) {
                    g_stand++;
                    if (len != (mem[i].is_dir ? 0 : mem[i].uncompressed_size)) ok = fail("a member that stands without its stated size", i);
                    const uint32_t crc = crc32_plain(dst + oo[i], len);
                    if (!mem[i].is_dir && crc != mem[i].crc32 && (mem[i].crc32 != 0 || (mem[i].flags & 8))) ok = fail("a member that stands with a wrong CRC-32", i);
                } else {
                    for (uint64_t k = 0; ok && k < len; k++)
                        if (dst[oo[i] + k] != 0) ok = fail("bytes of a failed member left in its range", i);
                }
            }
            free(dst);
        }
    }
    kc_zip_dir_free(d);
    free(buf);
    return ok;
}

std::vector<uint8_t> mutate(const std::vector<uint8_t>& base, Rng& r) {
    std::vector<uint8_t> v = base;
    const uint32_t ops = 1 + r.below(3);
    for (uint32_t k = 0; k < ops && !v.empty(); k++) {
        // the end record and the directory sit at the tail: half of the mutations land in the last 200 bytes
        const uint32_t span = r.below(2) ? (uint32_t)v.size() : (v.size() < 200 ? (uint32_t)v.size() : 200u);
        const size_t p = v.size() - 1 - r.below(span);
        switch (r.below(5)) {
        case 0: v[p] ^= (uint8_t)(1u << r.below(8)); break;
        case 1: v[p] = (uint8_t)r.next(); break;
        case 2: v.resize(p); break;
        case 3: v.insert(v.begin() + p, (uint8_t)r.next()); break;
        default: v[p] = r.below(2) ? 0xFF : 0x00; break;
        }
    }
    return v;
}

}  // namespace

int main(int argc, char** argv) {
    uint32_t n_mut = 8;
    Rng rng{0x5EED};
    std::vector<std::string> files;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "-n") && i + 1 < argc) n_mut = (uint32_t)atoi(argv[++i]);
        else if (!strcmp(argv[i], "-s") && i + 1 < argc) rng.s = strtoull(argv[++i], nullptr, 0);
        else if (!strcmp(argv[i], "-k")) g_kernels = false;
        else files.push_back(argv[i]);
    }
    if (files.empty()) { fprintf(stderr, "usage: zip_check [-n mutations-per-file] [-s seed] [-k] files...\n"); return 2; }
    bool ok = true;
    for (const std::string& f : files) {
        FILE* fp = fopen(f.c_str(), "rb");
        if (!fp) { fprintf(stderr, "zip_check: cannot open %s\n", f.c_str()); return 2; }
        std::vector<uint8_t> data;
        uint8_t tmp[65536];
        size_t k;
        while ((k = fread(tmp, 1, sizeof(tmp), fp)) > 0) data.insert(data.end(), tmp, tmp + k);
        fclose(fp);
        if (!run_one(data)) { fprintf(stderr, "zip_check: in %s\n", f.c_str()); ok = false; }
        for (uint32_t m = 0; m < n_mut; m++)
            if (!run_one(mutate(data, rng))) { fprintf(stderr, "zip_check: in mutation %u of %s\n", m, f.c_str()); ok = false; }
    }
    printf("zip_check: %llu buffers, %llu directories read, %llu members read on the emulator, %llu stand: %s\n", (unsigned long long)g_files,
           (unsigned long long)g_dirs, (unsigned long long)g_members, (unsigned long long)g_stand, ok ? "clean" : "FAILED");
    return ok ? 0 : 1;
}
