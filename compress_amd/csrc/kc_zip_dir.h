// kc_zip_dir.h — what zip.Reader holds after init (zip/reader.go:37-47, 63-69): the archive comment, baseOffset and the entries of
// the central directory, shared by the parser (kc_zip_dir.cpp) and whoever fills a member table from it.  Plain C++: no device code,
// no HIP.  Names, comments and extras point into the caller's buffer.
#pragma once
#include <stdint.h>
#include <vector>
#include "../../include/kcgpu.h"

struct kc_zip_dir {
    const uint8_t* comment = nullptr;  // Reader.Comment
    uint32_t comment_len = 0;
    int64_t base_offset = 0;           // Reader.baseOffset
    std::vector<kc_zip_entry> files;   // Reader.File, header offsets with baseOffset applied
};
