// kc_s2_index.h — what s2.Index holds (s2/index.go:25-33), shared by the index code (kc_s2_index.cpp) and the ranged reads that
// ask it where to start (kc_s2_ranges_api.cpp).  Plain C++: no device code, no HIP.
#pragma once
#include <stdint.h>
#include <vector>

struct kc_s2_index {
    int64_t total_uncompressed = -1;  // Index.TotalUncompressed, -1: unknown
    int64_t total_compressed = -1;
    int64_t est_block_uncomp = 0;
    std::vector<int64_t> c_off, u_off;  // Index.info
};
