// s2_decode_check — a stand-alone memory-error hunt for the s2.Reader / s2.Decode kernels: the plan kernel, the decode kernel and the
// chunk walk (compress_amd/csrc/kc_s2_plan_dev.h, kc_s2_plan.hip, kc_s2_decode_all.hip) compiled for the CPU wave emulator and linked
// into ONE ordinary executable that is built with -fsanitize=address,undefined and run on the host.  TEST INFRASTRUCTURE; nothing of it
// is loaded into another process and nothing of it runs on a device.
//
//   g++ -O1 -g -std=c++17 -x c++ -fsanitize=address,undefined -fno-omit-frame-pointer -I tools/hipemu \
//       tools/s2_decode_check_main.cpp tools/hipemu/hipemu.cpp -o tools/_build/s2_decode_check -ldl -lpthread
//   tools/_build/s2_decode_check [-n mutations-per-file] [-s seed] file...
//
// Every file named is decoded as a framed stream (default options, then ignore_crc + ignore_stream_identifier + a 64 KiB block limit)
// and as a bare block, followed by seeded mutations of it (bit flips, truncations, insertions, deletions, overwritten runs).  Input
// and output live in heap blocks of exactly their sizes, so a read past an input's end or a write outside the planned range is a
// sanitizer report.  The program itself checks what needs no judge: the host walk and the plan kernel agree, out_off is the prefix sum
// of bound and every chunk record stays inside its input and its planned range.  Exit status 0: clean.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../compress_amd/csrc/kc_s2_plan.hip"
#include "../compress_amd/csrc/kc_s2_decode_all.hip"

namespace {

struct Rng {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
    uint32_t below(uint32_t n) { return n ? next() % n : 0; }
};

uint32_t max_encoded_len(uint32_t n) {  // s2.MaxEncodedLen (s2/encode.go:389-418)
    const uint32_t lb = n == 0 ? 0 : 32 - (uint32_t)__builtin_clz(n);
    return n + (lb + 7) / 7 + (n == 0 ? 0 : n < 60 ? 1 : n < (1u << 8) ? 2 : n < (1u << 16) ? 3 : n < (1u << 24) ? 4 : 5);
}

struct Opts { uint32_t max_block; int ignore_crc, ignore_id, blocks; };

uint64_t g_cases = 0, g_ok = 0, g_refused = 0;

bool fail(const char* what, const Opts& o) {
    fprintf(stderr, "s2_decode_check: %s (max_block %u ignore_crc %d ignore_id %d blocks %d)\n", what, o.max_block, o.ignore_crc, o.ignore_id, o.blocks);
    return false;
}

// one batch of inputs through plan, decode, verdict and zero-fill, as kc_s2_dec_api.cpp runs them
bool run_batch(const std::vector<std::vector<uint8_t>>& inputs, const Opts& o) {
    const uint32_t n = (uint32_t)inputs.size();
    std::vector<uint64_t> in_off(n + 1, 0);
    for (uint32_t i = 0; i < n; i++) in_off[i + 1] = in_off[i] + inputs[i].size();
    uint8_t* src = (uint8_t*)malloc(in_off[n] ? in_off[n] : 1);  // exactly the inputs: a read behind the last one is a report
    for (uint32_t i = 0; i < n; i++) if (!inputs[i].empty()) memcpy(src + in_off[i], inputs[i].data(), inputs[i].size());
    KcS2PlanParams P;
    memset(&P, 0, sizeof(P));
    std::vector<uint32_t> nc(n), st(n), chunk0(n);
    std::vector<uint64_t> bound(n), out_off(n + 1, 0);
    P.src = src; P.in_off = in_off.data(); P.n = n; P.max_block = o.max_block; P.max_buf = max_encoded_len(o.max_block) + 4; P.ignore_id = o.ignore_id;
    P.blocks = o.blocks; P.n_chunks = nc.data(); P.bound = bound.data(); P.status = st.data();
    kc_launch_s2_plan(P, nullptr);
    bool good = true;
    uint32_t total = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (!o.blocks) {  // the walk on the host, the function the host-buffer entry points call
            auto none = [](uint32_t, uint64_t, uint32_t, uint32_t, uint64_t, uint32_t, uint32_t) {};
            const KcS2Walk W = kc_s2_walk(src, in_off[i], in_off[i + 1], P.max_block, P.max_buf, o.ignore_id != 0, none);
            if (W.status != st[i] || W.n_chunks != nc[i] || W.total != bound[i]) good = fail("host walk and plan kernel disagree", o);
        }
        chunk0[i] = total;
        total += nc[i];
        out_off[i + 1] = out_off[i] + bound[i];
    }
    const uint64_t cap = out_off[n];
    uint8_t* dst = (uint8_t*)malloc(cap ? cap : 1);  // exactly the planned layout
    memset(dst, 0xA5, cap ? cap : 1);
    std::vector<KcS2Chunk> ch(total ? total : 1);
    std::vector<uint32_t> cs(total ? total : 1, 0xA7A7A7A7u);
    if (total) {
        P.chunk0 = chunk0.data(); P.out0 = out_off.data(); P.chunks = ch.data();
        kc_launch_s2_plan(P, nullptr);
        for (uint32_t k = 0; k < total; k++)
            if (ch[k].out_off + ch[k].dlen > cap || ch[k].body_off + ch[k].body_len > in_off[n]) good = fail("a chunk record leaves its buffers", o);
        KcS2DecodeAllParams D;
        memset(&D, 0, sizeof(D));
        D.src = src; D.chunks = ch.data(); D.n_chunks = total; D.dst = dst; D.ignore_crc = o.ignore_crc; D.status = cs.data();
        if (good) kc_launch_s2_decode_all(D, nullptr);
    }
    for (uint32_t i = 0; i < n && good; i++) {
        uint32_t v = 0;
        for (uint32_t k = 0; k < nc[i] && !v; k++) v = cs[chunk0[i] + k];
        if (v > KCS2D_CRC) good = fail("a chunk verdict is no status class", o);
        if (!v) v = st[i];
        if (v && bound[i]) memset(dst + out_off[i], 0, bound[i]);
        g_cases++;
        if (v) g_refused++; else g_ok++;
    }
    free(dst);
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
            default: b[r.below(b.size() < 64 ? (uint32_t)b.size() : 64u)] = (uint8_t)r.next(); break;  // near the front: identifiers, first headers
        }
    }
    return b;
}

}  // namespace

int main(int argc, char** argv) {
    uint32_t per_file = 400;
    uint64_t seed = 0x52D0001;
    std::vector<std::string> files;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "-n") && i + 1 < argc) per_file = (uint32_t)strtoul(argv[++i], nullptr, 0);
        else if (!strcmp(argv[i], "-s") && i + 1 < argc) seed = strtoull(argv[++i], nullptr, 0);
        else files.push_back(argv[i]);
    }
    if (files.empty()) { fprintf(stderr, "usage: s2_decode_check [-n mutations-per-file] [-s seed] file...\n"); return 2; }
    const Opts modes[3] = {{4u << 20, 0, 0, 0}, {64u << 10, 1, 1, 0}, {4u << 20, 0, 0, 1}};
    bool good = true;
    for (const std::string& f : files) {
        FILE* fp = fopen(f.c_str(), "rb");
        if (!fp) { fprintf(stderr, "s2_decode_check: cannot read %s\n", f.c_str()); return 2; }
        std::vector<uint8_t> base;
        uint8_t tmp[65536];
        size_t got;
        while ((got = fread(tmp, 1, sizeof(tmp), fp)) > 0) base.insert(base.end(), tmp, tmp + got);
        fclose(fp);
        Rng r{seed ^ (uint64_t)base.size() * 0x9E3779B97F4A7C15ull};
        for (const Opts& o : modes) {
            good = run_batch({base}, o) && good;
            for (uint32_t k = 0; k < per_file; k += 8) {  // batches of 8: neighbours in one src and one dst
                std::vector<std::vector<uint8_t>> batch;
                for (uint32_t j = 0; j < 8 && k + j < per_file; j++) batch.push_back(mutate(base, r));
                good = run_batch(batch, o) && good;
            }
        }
    }
    printf("s2_decode_check: %llu inputs over %zu files (%llu decoded, %llu refused): %s\n", (unsigned long long)g_cases, files.size(),
           (unsigned long long)g_ok, (unsigned long long)g_refused, good ? "clean" : "FAILED");
    return good ? 0 : 1;
}
