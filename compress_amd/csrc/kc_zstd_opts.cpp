// kc_zstd_opts.cpp — option resolution of the zstd encoder (mirrors zstd/encoder_options.go) and MaxEncodedSize.  Plain host code over
// include/kcgpu.h alone: the library, the wave emulator (tools/hipemu/kcemu.cpp) and tools/zenc_plan_check_main.cpp compile this file.
#include <string.h>
#include "../../include/kcgpu.h"

extern "C" {

// ---------------------------------------------------------------------------------------
// options (zstd/encoder_options.go)
// ---------------------------------------------------------------------------------------
void kc_zstd_opts_default(kc_zstd_opts* o) {  // setDefault :36-48
    memset(o, 0, sizeof(*o));
    o->level = KC_SPEED_DEFAULT;
    o->window_size = 8 << 20;
    o->block_size = KC_ZSTD_MAX_BLOCK_SIZE;
    o->crc = 1;
    o->single = -1;
    o->full_zero = 1;
    o->no_entropy = 0;
    o->all_lit_entropy = 0;
    o->low_mem = 0;
    o->dict_offsets[0] = 1; o->dict_offsets[1] = 4; o->dict_offsets[2] = 8;
    o->concurrent = 0;
}

int kc_zstd_opts_concurrency(kc_zstd_opts* o, int n) {  // WithEncoderConcurrency :76-87
    if (n < 1) return KC_ERR_BAD_ARG;
    o->concurrent = n;
    return KC_OK;
}

int kc_zstd_opts_level(kc_zstd_opts* o, int l) {  // WithEncoderLevel :236-266
    if (l < KC_SPEED_FASTEST || l > 4) return KC_ERR_BAD_ARG;  // speedNotSet < l < speedLast
    o->level = l;
    if (!o->custom_window) {
        switch (l) {
        case KC_SPEED_FASTEST:
            o->window_size = 4 << 20;
            if (!o->custom_block) o->block_size = 1 << 16;
            break;
        default:
            o->window_size = 8 << 20;
            break;
        }
    }
    if (!o->custom_alent) o->all_lit_entropy = l > KC_SPEED_DEFAULT;
    return KC_OK;
}

int kc_zstd_opts_window(kc_zstd_opts* o, int n) {  // WithWindowSize :110-133
    if (n < KC_ZSTD_MIN_WINDOW_SIZE || n > KC_ZSTD_MAX_WINDOW_SIZE || (n & (n - 1)) != 0) return KC_ERR_BAD_ARG;
    o->window_size = n;
    o->custom_window = 1;
    if (o->block_size > o->window_size) {
        o->block_size = o->window_size;
        o->custom_block = 1;
    }
    return KC_OK;
}
int kc_zstd_opts_crc(kc_zstd_opts* o, int b) { o->crc = b != 0; return KC_OK; }
int kc_zstd_opts_zero_frames(kc_zstd_opts* o, int b) { o->full_zero = b != 0; return KC_OK; }
int kc_zstd_opts_no_entropy(kc_zstd_opts* o, int b) { o->no_entropy = b != 0; return KC_OK; }
int kc_zstd_opts_all_lit_entropy(kc_zstd_opts* o, int b) { o->custom_alent = 1; o->all_lit_entropy = b != 0; return KC_OK; }
int kc_zstd_opts_single_segment(kc_zstd_opts* o, int b) { o->single = b != 0; return KC_OK; }
int kc_zstd_opts_dict_raw(kc_zstd_opts* o, uint32_t id, const uint8_t* content, uint64_t len) {  // :398-406
    if (len > ((uint64_t)1 << 31)) return KC_ERR_BAD_ARG;
    o->dict_id = id;
    o->dict = content;
    o->dict_len = len;
    o->dict_offsets[0] = 1; o->dict_offsets[1] = 4; o->dict_offsets[2] = 8;  // offsets: [3]int{1, 4, 8}, no litEnc
    o->dict_huf_len = 0;
    o->dict_huf_log = 0;
    return KC_OK;
}

int64_t kc_zstd_max_encoded_size(const kc_zstd_opts* o, int64_t size) {  // encoder.go:843-873
    int64_t frameHeader = 4 + 2;
    if (o->dict != nullptr || o->dict_id != 0) frameHeader += 4;
    if (size < 256) frameHeader++;
    else if (size < 65536 + 256) frameHeader += 2;
    else if (size < 0x7fffffff) frameHeader += 4;
    else frameHeader += 8;
    if (o->crc) frameHeader += 4;
    const int64_t blocks = (size + o->block_size) / o->block_size;
    return frameHeader + 3 * blocks + size;
}

}  // extern "C"
