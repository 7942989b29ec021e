/* kcgpu.h — C ABI of the MI355X-native block-parallel zstd / S2 encode engine.
 *
 * This is the drop-in boundary for the encode hot path of klauspost/compress: every entry
 * point below is what a cgo binding in the reference would call instead of its pure-Go
 * encoder.  Plain pointers and sizes only; no exceptions cross this boundary; every call
 * returns a kc_status (0 == KC_OK, negative == error) and never aborts the host process
 * (the reference turns encoder panics into errors at its goroutine boundaries,
 * zstd/encoder.go:397-403,421-427).
 *
 * Reference seams replaced (file:line under the reference tree):
 *   kc_zstd_encode_units[_dev]  == N x (*Encoder).EncodeAll(unit, nil)   zstd/encoder.go:722-839
 *   kc_zstd_max_encoded_size    == (*Encoder).MaxEncodedSize             zstd/encoder.go:843-873
 *   kc_s2_encode_blocks[_dev]   == N x s2.Encode(nil, block)             s2/encode.go:29-56
 *   kc_zstd_encode_streams[_dev]      == N x NewWriter(w); Write(unit); Close()                zstd/encoder.go:154-428, 589-649
 *   kc_zstd_encode_streams_cuts[_dev] == the same with Flush() at given byte counts             zstd/encoder.go:547-570
 *   kc_s2_encode_blocks_lvl[_dev]     == N x s2.EncodeBetter / EncodeSnappy / EncodeSnappyBetter(nil, block)   s2/encode.go:117-276
 *   kc_s2_encode_block          == the s2.WriterCustomEncoder callback   s2/writer.go:1053-1064
 *   kc_s2_max_encoded_len       == s2.MaxEncodedLen                      s2/encode.go:389-418
 *   kc_s2_encode_stream_dev     == s2.Writer.EncodeBuffer framing        s2/writer.go:357-451
 *   kc_zstd_decode_units_dev    == N x Decoder.DecodeAll (verifier)       zstd/framedec.go, blockdec.go, seqdec_generic.go
 *   kc_zstd_decode_all[_dev]    == N x (*Decoder).DecodeAll(input, nil)   zstd/decoder.go:319-410 (the decoder as a product)
 *   kc_zstd_dstream_new / _feed == NewReader(r) + (*Decoder).Read / WriteTo zstd/decoder.go:88-312 (one stream, bounded memory)
 *   kc_s2_decode_blocks_dev     == N x s2.Decode (verifier)              s2/decode.go:58, decode_other.go:22
 *   kc_xxh64_units_dev          == xxhash.Digest over each unit          zstd/internal/xxhash/xxhash.go:27-230
 */
#ifndef KCGPU_H
#define KCGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct kc_ctx kc_ctx; /* opaque: device buffers, stream, scratch */

typedef enum {
    KC_OK = 0,
    KC_ERR_BAD_ARG = -1,       /* null pointer, unsorted offsets, zero units ... */
    KC_ERR_DST_TOO_SMALL = -2, /* dst_cap < sum of MaxEncodedSize(unit) */
    KC_ERR_HIP = -3,           /* a HIP runtime call failed; kc_last_error() has the text */
    KC_ERR_UNSUPPORTED = -4,   /* options outside what the device path implements; caller falls back to the CPU encoder */
    KC_ERR_NO_DEVICE = -5,     /* no gfx950 device visible */
    KC_ERR_INTERNAL = -6       /* device-side invariant violated (reported, never silently ignored) */
} kc_status;

/* Which build of the reference the S2 default / Snappy-compatible levels are byte-identical to.  The reference has two block
 * encoders for them: portable Go (s2/encode_all.go: arm64, noasm and every non-amd64 build) and generated amd64 assembly
 * (s2/encode_amd64.go + encodeblock_amd64.s: other table sizes, hash lengths and skip rates per input size class, matches extended
 * to the very end of the block).  Both write valid, different streams.  KC_OPT_S2_VARIANT picks the one to match. */
#define KC_S2_VARIANT_GO 0
#define KC_S2_VARIANT_AMD64 1

/* zstd.EncoderLevel (zstd/encoder_options.go:163-179) */
typedef enum { KC_SPEED_FASTEST = 1, KC_SPEED_DEFAULT = 2, KC_SPEED_BETTER = 3, KC_SPEED_BEST = 4 } kc_level;

/* Resolved zstd encoder options == the fields of encoderOptions (zstd/encoder_options.go:18-34)
 * that change output bytes.  Use kc_zstd_opts_default() + kc_zstd_opts_* helpers, which apply the
 * reference's EOption functions with the same order-dependent side effects. */
typedef struct {
    int32_t level;           /* o.level */
    int32_t window_size;     /* o.windowSize */
    int32_t block_size;      /* o.blockSize */
    int32_t crc;             /* o.crc            (WithEncoderCRC) */
    int32_t single;          /* o.single: -1 nil, 0 false, 1 true (WithSingleSegment) */
    int32_t full_zero;       /* o.fullZero       (WithZeroFrames) */
    int32_t no_entropy;      /* o.noEntropy      (WithNoEntropyCompression) */
    int32_t all_lit_entropy; /* o.allLitEntropy  (WithAllLitEntropyCompression) */
    int32_t low_mem;         /* o.lowMem         (WithLowerEncoderMem; no effect on bytes) */
    int32_t custom_window, custom_block, custom_alent; /* o.customWindow / customBlockSize / customALEntropy */
    uint32_t dict_id;        /* WithEncoderDictRaw id (0 = no dictionary) */
    const uint8_t* dict;     /* dictionary content (host pointer), used as initial history */
    uint64_t dict_len;
    /* full-format dictionaries only (kc_zstd_opts_dict); raw dictionaries keep {1,4,8} and no literal table */
    uint32_t dict_offsets[3];     /* dict.offsets -> blk.recentOffsets (zstd/enc_base.go:189-195) */
    int32_t dict_huf_len;         /* len(dict.litEnc.prevTable); 0 = no literal table */
    int32_t dict_huf_log;         /* dict.litEnc.prevTableLog */
    uint16_t dict_huf_val[256];   /* cTableEntry.val  (huff0/decompress.go:142-165) */
    uint8_t dict_huf_nbits[256];  /* cTableEntry.nBits */
    int32_t concurrent;           /* o.concurrent (WithEncoderConcurrency); 0 = the default (> 1).  Only "1 or not" changes bytes, and
                                   * only of dictionary streams: with 1 the reference takes nextBlock's synchronous form
                                   * (zstd/encoder.go:364-391), whose blk.reset(nil) drops the dictionary's literal table before the
                                   * first block; otherwise the first block starts from it (kc_zstd_encode_streams*) */
} kc_zstd_opts;

/* the limits the option functions and the device path check */
#define KC_ZSTD_MIN_WINDOW_SIZE (1 << 10)      /* zstd/decoder_options.go MinWindowSize */
#define KC_ZSTD_MAX_WINDOW_SIZE (1 << 29)      /* zstd MaxWindowSize */
#define KC_ZSTD_MAX_BLOCK_SIZE (128 << 10)     /* maxCompressedBlockSize, zstd/blockdec.go:40 */

/* encoderOptions.setDefault, zstd/encoder_options.go:36-48 */
void kc_zstd_opts_default(kc_zstd_opts* o);
/* WithEncoderLevel, zstd/encoder_options.go:236-266 */
int kc_zstd_opts_level(kc_zstd_opts* o, int level);
/* WithWindowSize, zstd/encoder_options.go:110-133 */
int kc_zstd_opts_window(kc_zstd_opts* o, int n);
/* WithEncoderCRC / WithZeroFrames / WithNoEntropyCompression / WithAllLitEntropyCompression / WithSingleSegment */
int kc_zstd_opts_crc(kc_zstd_opts* o, int b);
int kc_zstd_opts_zero_frames(kc_zstd_opts* o, int b);
int kc_zstd_opts_no_entropy(kc_zstd_opts* o, int b);
int kc_zstd_opts_all_lit_entropy(kc_zstd_opts* o, int b);
int kc_zstd_opts_single_segment(kc_zstd_opts* o, int b);
/* WithEncoderConcurrency, zstd/encoder_options.go:76-87 (n < 1: error) */
int kc_zstd_opts_concurrency(kc_zstd_opts* o, int n);
/* WithEncoderDictRaw, zstd/encoder_options.go:398-406 */
int kc_zstd_opts_dict_raw(kc_zstd_opts* o, uint32_t id, const uint8_t* content, uint64_t len);
/* WithEncoderDict, zstd/encoder_options.go:382-391: a dictionary in the "zstd --train" format.  Parses it like loadDict
 * (zstd/dict.go:71-150): ID, literal Huffman table (becomes huff0 prevTable of each unit's first block,
 * zstd/blockenc.go:518-522), repeat offsets, content.  `blob` must outlive every encode call using `o`
 * (o->dict points into it).  Returns 0, or -1 when the reference's loadDict would return an error. */
int kc_zstd_opts_dict(kc_zstd_opts* o, const uint8_t* blob, uint64_t len);

/* (*Encoder).MaxEncodedSize, zstd/encoder.go:843-873 (padding off) */
int64_t kc_zstd_max_encoded_size(const kc_zstd_opts* o, int64_t size);

/* ---- context ---- */
/* device: HIP device ordinal.  stream: a hipStream_t to launch on (NULL = the context's own stream).
 * The context owns all device scratch: one call at a time per context (kc_s2_encode_block excepted, see there); any number of
 * contexts may work on one device at the same time from different host threads — how the drop-ins make EncodeAll safe for concurrent
 * callers on ONE encoder like the reference's (zstd/encoder.go:90-99, 722-729: a channel of encoder states; here a pool of contexts:
 * shim/go/zstdgpu, compress_amd/zstd.py; tests/test_zz_gpu_threads.py runs 8 threads on one encoder on the device). */
kc_status kc_ctx_create(kc_ctx** out, int device, void* stream);
void kc_ctx_destroy(kc_ctx* ctx);
/* Why the last kc_ctx_create of the calling thread failed ("" after a success).  The first kc_ctx_create on a device runs a
 * known-answer launch (256 bytes through the XXH64 kernel) on a thread of its own and waits for it with a 90 s deadline: a device
 * that faults, hangs or miscomputes makes kc_ctx_create return KC_ERR_HIP / KC_ERR_INTERNAL with the reason here instead of hanging
 * or aborting the host (the promise at the top of this file); the verdict is remembered per device for the life of the process. */
const char* kc_create_error(void);
/* Give device memory back without giving the handles up (long-lived hosts, several processes on one device).  kc_ctx_trim frees
 * the context's device scratch (it grows back with the next call; KC_ERR_BAD_ARG while a begin / submit is in flight on it).
 * kc_device_trim frees what the device's rolling host pipeline holds (kc_zstd_encode_units / kc_s2_encode_blocks_lvl on large inputs:
 * ten device slots of a sub-batch each and the scratch of its eight encoder lanes, ~100 GiB after 1 GiB SpeedFastest sub-batches);
 * KC_ERR_BAD_ARG while host-buffer calls are in flight on that device, KC_OK when the pipeline never started. */
kc_status kc_ctx_trim(kc_ctx* ctx);
kc_status kc_device_trim(int device);
/* Page-locked host memory for callers that own their buffers (a Go caller: C memory wrapped in a slice with unsafe.Slice).  The
 * host-buffer entry points recognise page-locked source / destination buffers — these, hipHostMalloc'ed or hipHostRegister'ed ones —
 * and DMA straight from / into them: the rolling pipeline's staging copies (16 host threads at ~100 GB/s while a call runs) are not
 * made at all.  Pageable buffers work as before.  kc_host_alloc: KC_ERR_UNSUPPORTED when the host cannot lock that much memory. */
kc_status kc_host_alloc(void** out, uint64_t bytes);
void kc_host_free(void* p);
const char* kc_last_error(const kc_ctx* ctx);
/* ONE stream with WithConcurrentBlocks(true) (zstd/encoder_options.go:340-353; zstd/enc_jobs.go): the bytes equal
 *   enc, _ := zstd.NewWriter(w, opts..., zstd.WithConcurrentBlocks(true))   (with WithEncoderConcurrency > 1)
 *   enc.Write(src[...]) with enc.Flush() after cuts[0], cuts[1], ... bytes (ascending; a Write followed by ReadFrom is such a point, encoder.go:500-507); enc.Close()
 * The reference cuts the stream into jobs of kc_zstd_job_size() input bytes (a Flush ends a job early), encodes each on a freshly
 * reset encoder whose history is the last kc_zstd_overlap_size() bytes of the previous job's input (ResetPrefix,
 * zstd/enc_fast.go:800-811, enc_dfast.go:1040-1050, enc_better.go:1099-1112) and concatenates the outputs behind one frame header:
 * the jobs are independent units, which is what this engine wants: this is the reference's own way of turning ONE stream into
 * device work.  src / dst are HOST buffers; dst_cap >= sum over jobs of kc_zstd_max_encoded_size(job + overlap) + 16.  A stream of
 * at most one block is the EncodeAll frame (enc_jobs.go:263-279).  With a dictionary the reference switches the option off
 * (zstd/encoder.go:81,174): KC_ERR_UNSUPPORTED.  The frame is assembled in dst batch by batch: on any error *out_len is 0 and the
 * bytes already written to dst (the frame header, earlier batches) are unspecified — dst is clobbered, not rolled back. */
kc_status kc_zstd_encode_jobs(kc_ctx* ctx, const kc_zstd_opts* o, const uint8_t* src, uint64_t len, const uint64_t* cuts, uint64_t n_cuts,
                              uint8_t* dst, uint64_t dst_cap, uint64_t* out_len);
int64_t kc_zstd_job_size(const kc_zstd_opts* o);     /* encoderOptions.jobSize, zstd/encoder_options.go:356-359 */
int64_t kc_zstd_overlap_size(const kc_zstd_opts* o); /* encoderOptions.overlapSize, zstd/encoder_options.go:362-371 */

/* ---- context options ----
 * Every tunable of the library is a field of the context with a built-in default; kc_ctx_set_option is the only way to change one.
 * The library reads NO environment variable (round 5).  The name beside each key is the variable the measurement harness above the
 * C ABI maps to it (compress_amd/_lib.py: Context applies KC_* variables as options after kc_ctx_create) — a convenience of the
 * Python tooling, not of the shipped library.
 *
 * Two kernel families serve SpeedFastest and s2.Encode / s2.EncodeSnappy (KC_OPT_MATCH_PATH):
 *   KC_PATH_HBM  per-unit hash tables in an HBM arena, 8 units per wave: the throughput path, needs ~10^4 units in flight;
 *   KC_PATH_LDS  the unit's hash table (and, for S2 blocks up to 64 KiB, the block) in the CU's LDS, one wave per unit: the
 *                latency path — one unit in a few ms instead of ~30 ms; also the faster one for sparse scans (high-entropy input);
 *   KC_PATH_AUTO by units in flight, against the measured crossovers (profiles/r03_crossover_*.csv).
 * Both produce the same bytes (the GPU parity tests run on both). */
enum { KC_PATH_AUTO = 0, KC_PATH_HBM = 1, KC_PATH_LDS = 2 };
typedef enum {
    KC_OPT_MATCH_PATH = 1,           /* KC_MATCH_PATH             KC_PATH_* */
    KC_OPT_ZFAST_LDS_MAX_UNITS = 2,  /* KC_ZFAST_LDS_MAX_UNITS    auto: SpeedFastest batches of at most this many units take KC_PATH_LDS */
    KC_OPT_S2_LDS_MAX_BLOCKS = 3,    /* KC_S2_LDS_MAX_BLOCKS      auto: s2 block batches of at most this many blocks take KC_PATH_LDS */
    KC_OPT_SPEC_W0 = 4,              /* KC_SPEC_W0                HBM kernels: probe steps per round after a match (-1: per-level default) */
    KC_OPT_SPEC_GROW = 5,            /* KC_SPEC_GROW              HBM kernels: width after a miss: 0 keep, 1 +1, 2 double (-1: default) */
    KC_OPT_LDS_SPEC_W0 = 6,          /* KC_LDS_SPEC_W0            SpeedFastest LDS kernel: probe steps per round after a match (doubles on a miss, max 64; default 16); 0 = units up to 128 KiB without history through the source-ring instantiation at 16 */
    KC_OPT_S2_LDS_SPEC_W0 = 17,      /* KC_S2_LDS_SPEC_W0         S2 LDS kernel: the same; blocks up to 64 KiB: 0 (default) the fused wave-uniform step, 1 its first form */
    KC_OPT_HOST_SERIAL = 7,          /* KC_HOST_SERIAL            host-buffer entry points: no pipelining (copy, encode, copy) */
    KC_OPT_HOST_PIPE_MIB = 8,        /* KC_HOST_PIPE_MIB          host-buffer entry points: sub-batch size of the three-stage pipeline */
    KC_OPT_HOST_OVERLAP_MIN_MIB = 9, /* KC_HOST_OVERLAP_MIN_MIB   smallest input that takes the chunk-fed path (-1: default) */
    KC_OPT_HOST_COPY_THREADS = 10,   /* KC_HOST_COPY_THREADS      threads of the pageable <-> pinned copies (0: the cgroup's CPUs, max 16) */
    KC_OPT_HOST_TRACE = 11,          /* KC_HOST_TRACE             timeline of the chunk-fed path on stderr */
    KC_OPT_HOST_CHUNK_MIB = 12,      /* KC_HOST_CHUNKS_MIB (list) chunk size of the chunk-fed path (0: a quarter of the batch) */
    KC_OPT_K2_PROF = 13,             /* KC_K2_PROF                per-phase shader clocks of the entropy kernel on stderr */
    KC_OPT_S2_HOOK_WAIT_US = 14,     /* KC_S2_HOOK_WAIT_US        kc_s2_encode_block: time a batch leader waits for more callers */
    KC_OPT_S2_HOOK_BATCH = 15,       /* KC_S2_HOOK_BATCH          kc_s2_encode_block: most blocks per device batch */
    KC_OPT_TEST_FEED_REDO = 16,      /* (no variable)             diagnostics: force the chunk-fed path's re-encode fallback */
    KC_OPT_MAX_SCRATCH_MIB = 18,     /* (no variable)             ceiling of the device scratch one batch may take (default 160 GiB, and 85 % of the free memory): larger calls are cut into several batches */
    KC_OPT_BEST_SLOTS = 19,          /* (no variable)             SpeedBestCompression: table slots of 34 MiB = units encoded at a time (default 6144 = 204 GiB; allocated on demand for the units a batch has, never more than 80 % of the free device memory) */
    KC_OPT_S2_VARIANT = 20,          /* (no variable)             s2.Encode / s2.EncodeSnappy: KC_S2_VARIANT_GO (default) or KC_S2_VARIANT_AMD64 */
    KC_OPT_BETTER_DICT_EPOCH = 21,   /* (no variable)             SpeedBetterCompression with a dictionary: 1 = epoch-stamped tables + shared dictionary table (measurements; default 0: per-batch copy) */
    KC_OPT_ZFAST_EPOCH = 22,         /* KC_ZFAST_EPOCH            SpeedFastest HBM-table kernel, no dictionary: 1 (default) = epoch-stamped table entries, the arena is cleared every 15 batches instead of every batch */
    KC_OPT_ZFAST_XSEG_K = 23,        /* KC_ZFAST_XSEG_K           SpeedFastest HBM-table kernel: a probe round crosses skip-segment boundaries once (s - nextEmit) >> 5 has reached this value (default 0: always; large: never); acts in the kernel form KC_OPT_ZFAST_VARIANT selects */
    KC_OPT_FUSE_RAW_XXH = 24,        /* KC_FUSE_RAW_XXH           frames made of raw blocks only: 1 (default) = XXH64 and the payload copy in one pass over the source */
    KC_OPT_ZFAST_FILTER = 25,        /* KC_ZFAST_FILTER           SpeedFastest HBM-table kernel: 1 (default) = units that have emitted no sequence yet skip the table loads of bucket groups they have not written (a 512-bit map in their idle sequence buffer) */
    KC_OPT_XXH_FIN_MODE = 26,        /* KC_XXH_FIN_MODE           checksum-and-copy kernel, payload of raw-only frames: 0 stored from the registers, 1 the same software-pipelined, 2 through an LDS ring as aligned stores, 3 like 1 with eight 16-byte loads per lane in flight instead of four */
    KC_OPT_ZFAST_VARIANT = 27,       /* KC_ZFAST_VARIANT          SpeedFastest HBM-table kernel: 0 the plain form, 1 the form for input without matches (KC_OPT_ZFAST_XSEG_K, KC_OPT_ZFAST_FILTER), -1 (default) per batch: form 1 when the context's previous batch did not compress */
    KC_OPT_ZFAST_PRESCAN = 28,       /* KC_ZFAST_PRESCAN          SpeedFastest, EncodeAll batches without dictionary: 1 = a pre-scan proves units free of matches from their probe positions alone and writes their (raw-block) frames, the match finder and the entropy stage skip them; 0 off; -1 (default) per batch: on when the context's previous batch did not compress */
    KC_OPT_S2_HOOK_LANES = 29,       /* KC_S2_HOOK_LANES          kc_s2_encode_block: batches of concurrent callers on the device at once (own stream and scratch each; default 4, at most 8).  Footprint: on the first hook call the context creates `lanes` contexts and (lanes + 2) slots of 2 x 8 MiB pinned host memory (96 MiB at the default), each lane's device scratch grows to its largest batch (a few MiB per 256 blocks of 64 KiB); a lane takes the caller's variant / kernel-family options and scratch ceiling per batch */
    KC_OPT_JOB_PRIME = 30,           /* KC_JOB_PRIME              kc_zstd_encode_jobs: where a job's tables are primed from its overlap prefix (ResetPrefix): 1 (default) on the device (kc_zstd_prime.hip), 0 on the host, uploaded per batch */
    KC_OPT_HOST_CHUNK_MIB_APPEND = 32, /* KC_HOST_CHUNKS_MIB (list) one more chunk size behind KC_OPT_HOST_CHUNK_MIB's: an uneven chunk schedule (the last size repeats) */
    KC_OPT_STAGE2_STREAM = 31,       /* (no variable)             a hipStream_t handle (0: none): kc_zstd_encode_units_dev[_begin/_end] run the entropy stage and everything behind it on this stream, behind an event of the match finder's — for callers that give the two stages different CU masks (hipExtStreamCreateWithCUMask).  Scope: the device-resident zstd entry points only (the host-buffer entry points and S2 ignore it).  Lifetime: the handle must belong to the context's device and outlive the option — reset it to 0 before destroying the stream; the library never destroys it */
    KC_OPT_HOST_ROLL = 33,           /* KC_HOST_ROLL              host-buffer entry points, large inputs: 1 (default) = the device's rolling pipeline (sub-batches of all calls in flight staged, encoded on four lanes and drained in arrival order: consecutive calls overlap), 0 = one chunk-fed device batch per call (round 5) */
    KC_OPT_HOST_ROLL_MIB = 34,       /* KC_HOST_ROLL_MIB          rolling pipeline: sub-batch size (0: a quarter of the call's input — SpeedBetterCompression and S2: half —, 64 MiB .. 1 GiB) */
    KC_OPT_S2_HOOK_HOST_FIRST = 35,  /* KC_S2_HOOK_HOST_FIRST     kc_s2_encode_block: how many callers at a time are left to the host's built-in encoder (they get -1) before the overflow goes to the device: -1 (default) the host's hardware threads, 0 every caller to the device (see kc_s2_encode_block) */
    KC_OPT_DSTREAM_BLOCKS = 36,      /* (no variable)             zstd stream reader (kc_zstd_dstream_new): blocks per launch, 1 .. 4096 (default 512); at 1 every block is a launch of its own */
    KC_OPT_S2_RSTREAM_CHUNKS = 37,   /* (no variable)             S2 stream reader (kc_s2_rstream_new): data chunks per launch, 1 .. 4096 (default 4096: the smallest value within the spread of the best rate at 64 KiB blocks, profiles/s2_stream_reader.json); at 1 every chunk is a launch of its own */
    KC_OPT_ZFAST_FIRST_FILTER = 38,  /* KC_ZFAST_FIRST_FILTER     SpeedFastest HBM-table kernel, batches whose tables start empty (no dictionary, no job prefix, not chunk-fed): 1 (default) = a streaming pre-pass marks every position that is the first of its unit with its table hash, and the match finder takes "no candidate" there without reading the table; 0 = every lookup reads the table.  The frames are the same bytes either way (profiles/zfast_first_filter_ab.txt has the measurements) */
    KC_OPT_LAST_PRESCAN_UNITS = 102, /* read-only: units of the last batch the pre-scan settled */
    KC_OPT_LAST_FIRST_BITS = 103,    /* read-only: 1 = the last zstd batch's match finder was handed first-occurrence bits (KC_OPT_ZFAST_FIRST_FILTER), 0 = it read every bucket */
    KC_OPT_LAST_PATH = 100,          /* read-only: KC_PATH_HBM / KC_PATH_LDS the last batch ran on */
    KC_OPT_LAST_BATCHES = 101        /* read-only: device batches the last kc_zstd_encode_units_dev / kc_s2_encode_*_dev call was cut into */
} kc_option;
kc_status kc_ctx_set_option(kc_ctx* ctx, int key, int64_t value);
int64_t kc_ctx_get_option(const kc_ctx* ctx, int key);
/* Device properties as probed (CU count, LDS bytes per CU, clock, name) */
kc_status kc_device_info(const kc_ctx* ctx, int32_t* n_cu, int32_t* lds_per_cu, int32_t* clock_khz, char* name, size_t name_cap);

/* ---- zstd: N independent units, each == EncodeAll(unit, nil) ----
 * src:       all units, concatenated (host memory for the plain call, device memory for _dev)
 * unit_off:  n_units+1 ascending byte offsets into src (HOST memory in both variants)
 * dst:       output buffer; unit i's frame is written at dst + out_off[i]
 * dst_cap:   must be >= sum_i kc_zstd_max_encoded_size(unit_i)
 * out_off:   n_units+1 offsets of the compacted frames (HOST memory in both variants)
 * The _dev variant leaves the frames in device memory (dst is a device pointer) and only
 * copies the n_units+1 offsets back; it synchronises the stream before returning.
 * A unit may have any number of blocks up to 1 GiB (beyond: KC_ERR_UNSUPPORTED); its blocks are parsed one after the other by
 * one lane group, so the device pays with thousands of units in flight, not with a few long ones. */
kc_status kc_zstd_encode_units(kc_ctx* ctx, const kc_zstd_opts* o, const uint8_t* src, const uint64_t* unit_off,
                               uint32_t n_units, uint8_t* dst, uint64_t dst_cap, uint64_t* out_off);
kc_status kc_zstd_encode_units_dev(kc_ctx* ctx, const kc_zstd_opts* o, const uint8_t* d_src, const uint64_t* unit_off,
                                   uint32_t n_units, uint8_t* d_dst, uint64_t dst_cap, uint64_t* out_off);
/* N independent STREAMS: unit i's output equals NewWriter(w).Write(unit_i) ... Close() (zstd/encoder.go:154-428, 567-649;
 * no Flush in between — see kc_zstd_encode_streams_cuts): below one block that is the EncodeAll frame; from one block on, a frame without content size whose
 * blocks all see the history, with the `last` flag on a short final block or else a trailing empty raw block.  Same limits as
 * kc_zstd_encode_units_dev (a stream of more than 1 GiB is KC_ERR_UNSUPPORTED); dictionaries are KC_ERR_UNSUPPORTED. */
kc_status kc_zstd_encode_streams_dev(kc_ctx* ctx, const kc_zstd_opts* o, const uint8_t* d_src, const uint64_t* unit_off,
                                     uint32_t n_units, uint8_t* d_dst, uint64_t dst_cap, uint64_t* out_off);
/* host-buffer form (src / dst in host memory), like kc_zstd_encode_units */
kc_status kc_zstd_encode_streams(kc_ctx* ctx, const kc_zstd_opts* o, const uint8_t* src, const uint64_t* unit_off,
                                 uint32_t n_units, uint8_t* dst, uint64_t dst_cap, uint64_t* out_off);
/* The same with Flush points (zstd/encoder.go:547-570: Flush ends the block being filled; a Flush that finds nothing buffered does
 * nothing): cuts[cut_off[i] .. cut_off[i+1]) lists, ascending, how many bytes of stream i had been written at each Flush.  A Write
 * that precedes ReadFrom is such a point too (ReadFrom first ends the block being filled, :482-486).  The output is the
 * concatenation of what the reference's writer received, delivered when the call returns.
 * dst_cap: >= sum_i (kc_zstd_max_encoded_size(unit_i) + 3 * ncuts_i + 3, rounded up to 16). */
kc_status kc_zstd_encode_streams_cuts_dev(kc_ctx* ctx, const kc_zstd_opts* o, const uint8_t* d_src, const uint64_t* unit_off,
                                          uint32_t n_units, const uint64_t* cut_off, const uint64_t* cuts, uint8_t* d_dst,
                                          uint64_t dst_cap, uint64_t* out_off);
kc_status kc_zstd_encode_streams_cuts(kc_ctx* ctx, const kc_zstd_opts* o, const uint8_t* src, const uint64_t* unit_off,
                                      uint32_t n_units, const uint64_t* cut_off, const uint64_t* cuts, uint8_t* dst,
                                      uint64_t dst_cap, uint64_t* out_off);
/* Host logic only: the block plan of one stream with Flush points as kc_zstd_encode_streams_cuts lays it out — block starts
 * (starts may be NULL), *flags bit 0 = stream frame (a block was written before Close), bit 1 = Close found nothing buffered
 * (empty last block).  Returns the number of blocks, -1 bad argument, -2 starts_cap too small. */
int64_t kc_zstd_plan_stream_blocks(int32_t block_size, uint64_t len, const uint64_t* cuts, uint64_t n_cuts, uint32_t* starts,
                                   uint64_t starts_cap, uint32_t* flags);
/* Asynchronous form of the host-buffer entry points (SURVEY §8(b) "async submit/wait"): submit returns at once and the call runs
 * on a thread of its own; kc_wait blocks until it is done and returns ITS status (kc_last_error for the text).  One job per
 * context.  Inside one call the source staging, the kernels and the drain of the frames already overlap chunk by chunk; with
 * two contexts the caller also overlaps consecutive batches (submit(A, batch k+1); wait(B) ...).  src, unit_off / blk_off, dst,
 * out_off and a dictionary referenced by *o must stay valid until kc_wait returns; *o itself is copied. */
kc_status kc_zstd_encode_units_submit(kc_ctx* ctx, const kc_zstd_opts* o, const uint8_t* src, const uint64_t* unit_off,
                                      uint32_t n_units, uint8_t* dst, uint64_t dst_cap, uint64_t* out_off);
kc_status kc_s2_encode_blocks_lvl_submit(kc_ctx* ctx, int level, const uint8_t* src, const uint64_t* blk_off, uint32_t n_blocks,
                                         uint8_t* dst, uint64_t dst_cap, uint64_t* out_off);
kc_status kc_wait(kc_ctx* ctx);
/* Split form of kc_zstd_encode_units_dev for ONE device batch (<= 8 GiB): _begin enqueues everything up to and including
 * the match finder and returns without waiting; _end enqueues the entropy stage, waits, and returns the offsets.  With two
 * contexts (two streams, two sets of scratch) a caller pipelines consecutive batches:
 *     begin(A, batch0); begin(B, batch1); end(A); begin(A, batch2); end(B); ...
 * so that the match finder of batch i+1 runs under the entropy stage of batch i.  kc_ctx_chain_after(B, A) makes B's match
 * finder wait for A's (and vice versa), which keeps one match finder on the device at a time: right for SpeedFastest and
 * SpeedDefault, whose kernels are one residency of the chip per 4 GiB batch.  A SpeedBetterCompression batch of 1 GiB fills
 * 8 of 12 wave slots per CU and every unit is a chain of dependent table trips: with three contexts chained two apart
 * (chain_after(C, A), chain_after(A, B), chain_after(B, C)) — or not chained at all — consecutive batches' match finders share the
 * chip (measured +16-20 %: DESIGN.md 4.2).  d_src, d_dst and the options' dictionary must stay valid until _end returns; unit_off
 * is copied. */
kc_status kc_zstd_encode_units_dev_begin(kc_ctx* ctx, const kc_zstd_opts* o, const uint8_t* d_src, const uint64_t* unit_off,
                                         uint32_t n_units, uint8_t* d_dst, uint64_t dst_cap);
kc_status kc_zstd_encode_units_dev_end(kc_ctx* ctx, uint64_t* out_off);
/* _end with the place of the frames named only now (d_dst of _begin is then just the capacity check): the frames of a batch leave
 * their staging slots in _end, so a caller that runs ONE EncodeAll batch as several smaller launches — two halves of a 4 GiB batch
 * on three contexts, chained two apart, are 4-8 % faster than one launch (the second half's units fill the first half's tail:
 * DESIGN.md 4.1) — puts each part's frames right behind the previous part's and gets the same contiguous output, out_off relative
 * to the d_dst given here.  KC_ERR_DST_TOO_SMALL if dst_cap is below the sum of MaxEncodedSize(unit) of this batch. */
kc_status kc_zstd_encode_units_dev_end_at(kc_ctx* ctx, uint8_t* d_dst, uint64_t dst_cap, uint64_t* out_off);
void kc_ctx_chain_after(kc_ctx* ctx, kc_ctx* prev);

/* XXH64(seed 0) of every unit (the frame checksum primitive), device-resident input, host output. */
kc_status kc_xxh64_units_dev(kc_ctx* ctx, const uint8_t* d_src, const uint64_t* unit_off, uint32_t n_units, uint64_t* out_hash);

/* Debug/inspection (parity of intermediates): run only the match finder on device-resident units and
 * return, for every block, the sequence list as (litLen, matchLen, offset) u32 triples.
 * blk_first_seq has n_blocks+1 entries; blk_flags (may be NULL) receives KC_BF_* verdict bits in bits 0..7 and
 * the number of speculative probe rounds in bits 8..31.  Buffers are HOST memory. */
kc_status kc_zstd_debug_parse_dev(kc_ctx* ctx, const kc_zstd_opts* o, const uint8_t* d_src, const uint64_t* unit_off,
                                  uint32_t n_units, uint32_t* seqs, uint64_t seq_cap, uint64_t* blk_first_seq,
                                  uint32_t* blk_extra_lits, uint32_t* blk_flags, uint32_t blk_cap, uint32_t* n_blocks_out);

/* ---- S2: N independent blocks, each == s2.Encode(nil, block) (varint length + body) ---- */
int64_t kc_s2_max_encoded_len(int64_t src_len);
kc_status kc_s2_encode_blocks(kc_ctx* ctx, const uint8_t* src, const uint64_t* blk_off, uint32_t n_blocks,
                              uint8_t* dst, uint64_t dst_cap, uint64_t* out_off);
kc_status kc_s2_encode_blocks_dev(kc_ctx* ctx, const uint8_t* d_src, const uint64_t* blk_off, uint32_t n_blocks,
                                  uint8_t* d_dst, uint64_t dst_cap, uint64_t* out_off);
/* The same at a chosen level: KC_S2_LEVEL_DEFAULT == s2.Encode (encodeBlockGo / encodeBlockGo64K, s2/encode_all.go:72-500),
 * KC_S2_LEVEL_BETTER == s2.EncodeBetter (s2/encode.go:117-144: encodeBlockBetterGo / encodeBlockBetterGo64K,
 * s2/encode_better.go:50-307 / 485-730), KC_S2_LEVEL_SNAPPY == s2.EncodeSnappy (s2/encode.go:204-232: encodeBlockSnappyGo /
 * encodeBlockSnappyGo64K, s2/encode_all.go:502-690 / 692-880 — blocks a Snappy decoder reads: no repeat tags),
 * KC_S2_LEVEL_SNAPPY_BETTER == s2.EncodeSnappyBetter, KC_S2_LEVEL_BEST == s2.EncodeBest (s2/encode.go:146-202: encodeBlockBest,
 * s2/encode_best.go:22-455), KC_S2_LEVEL_SNAPPY_BEST == s2.EncodeSnappyBest (s2/encode.go:278-305: encodeBlockBestSnappy,
 * s2/encode_best.go:457-710).  The best levels take 4.5 MiB of tables per block: large calls are cut into batches. */
#define KC_S2_LEVEL_DEFAULT 0
#define KC_S2_LEVEL_BETTER 1
#define KC_S2_LEVEL_SNAPPY 2
#define KC_S2_LEVEL_BEST 4
#define KC_S2_LEVEL_SNAPPY_BEST 5
#define KC_S2_LEVEL_UNCOMPRESSED 6 /* kc_s2_encode_stream_lvl_dev only: s2.WriterUncompressed (s2/writer.go:951) — every block an uncompressed chunk */
#define KC_S2_LEVEL_SNAPPY_BETTER 3   /* s2.EncodeSnappyBetter (s2/encode.go:248-276: encodeBlockBetterSnappyGo / ...64K, s2/encode_better.go:310-483 / 733-900) */
kc_status kc_s2_encode_blocks_lvl(kc_ctx* ctx, int level, const uint8_t* src, const uint64_t* blk_off, uint32_t n_blocks,
                                  uint8_t* dst, uint64_t dst_cap, uint64_t* out_off);
kc_status kc_s2_encode_blocks_lvl_dev(kc_ctx* ctx, int level, const uint8_t* d_src, const uint64_t* blk_off, uint32_t n_blocks,
                                      uint8_t* d_dst, uint64_t dst_cap, uint64_t* out_off);
/* Split form of kc_s2_encode_blocks_lvl_dev for ONE device batch of bare blocks below the best levels (the S2 sibling of
 * kc_zstd_encode_units_dev_begin / _end_at): _begin enqueues everything up to and including the encoder kernel and returns without
 * waiting; _end_at compacts the blocks to the d_dst named there, copies the offsets (relative to it) and waits.  A 2 GiB batch of
 * 64 KiB blocks is exactly one residency of the chip; run as two launches on three contexts (three host threads, or begin / begin /
 * end_at / ...) the next launch's blocks take the wave slots as the previous launch's leave them: measured +5-6 %.
 * d_src must stay valid until _end_at returns; blk_off is copied.  KC_ERR_UNSUPPORTED: framed, best levels, more than one batch. */
kc_status kc_s2_encode_blocks_lvl_dev_begin(kc_ctx* ctx, int level, const uint8_t* d_src, const uint64_t* blk_off, uint32_t n_blocks);
kc_status kc_s2_encode_blocks_lvl_dev_end_at(kc_ctx* ctx, uint8_t* d_dst, uint64_t dst_cap, uint64_t* out_off);
/* kc_s2_encode_stream_dev at a chosen level (s2.WriterBetterCompression, s2/writer.go:931) */
kc_status kc_s2_encode_stream_lvl_dev(kc_ctx* ctx, int level, const uint8_t* d_src, const uint64_t* blk_off, uint32_t n_blocks,
                                      uint8_t* d_dst, uint64_t dst_cap, uint64_t* out_off, int with_stream_id);
/* s2.Writer framing on the device (s2/writer.go:394-451): every block becomes one chunk
 * `type(1) | len24 | masked CRC32C(4) | body` (compressed 0x00: uvarint(len) + block; incompressible 0x01: raw bytes),
 * optionally preceded by the stream identifier `ff 06 00 00 "S2sTwO"`.  The result is a complete, concatenable .s2
 * stream; out_off[i] is the start of chunk i (out_off[0] == 10 with the identifier).  dst_cap >= sum(MaxEncodedLen+8)+10.
 * A block of a framed stream is at most 4 MiB (s2.maxBlockSize: the chunk header holds a 24-bit length and the reference's
 * Reader refuses larger chunks): a larger block is KC_ERR_BAD_ARG (bare blocks: kc_s2_encode_blocks*, up to 1 GiB). */
kc_status kc_s2_encode_stream_dev(kc_ctx* ctx, const uint8_t* d_src, const uint64_t* blk_off, uint32_t n_blocks,
                                  uint8_t* d_dst, uint64_t dst_cap, uint64_t* out_off, int with_stream_id);
/* s2.Decode (s2/decode.go:58 -> s2Decode, s2/decode_other.go:22) over N encoded blocks (uvarint length + body), for
 * on-device round-trip verification: block i decodes to d_dst + dst_off[i] and must produce exactly dst_off[i+1]-dst_off[i]
 * bytes.  enc_off / dst_off / status are host arrays; status[i] = 0 or the first error met in block i (corrupt input is
 * reported, never written out of bounds). */
kc_status kc_s2_decode_blocks_dev(kc_ctx* ctx, const uint8_t* d_enc, const uint64_t* enc_off, uint32_t n_blocks, uint8_t* d_dst,
                                  const uint64_t* dst_off, uint32_t* status);
/* zstd frame decoder (zstd/framedec.go:65-330, blockdec.go:227-690, seqdec_generic.go) over N units, one frame each, for
 * on-device round-trip verification: unit i decodes to d_dst + dst_off[i] and must produce exactly dst_off[i+1]-dst_off[i]
 * bytes; the frame checksum, if present, is checked against XXH64 of the decoded bytes (status 30 on mismatch).  All block,
 * literal and sequence modes; dictionary frames need kc_zstd_decode_units_dict_dev (status 20 otherwise).  enc_off / dst_off / status are host arrays.
 * The block parser is the one DecodeAll and the stream reader use, so the verifier refuses what the reference refuses in the four-stream
 * jump table (ten bytes at least), the weight parity check, an FSE description with fewer than four bytes behind it, the literal size
 * limits (128 KiB and the window) and a window above 2^29 (status 1); a repeat offset that resolves to 0 stays refused. */
kc_status kc_zstd_decode_units_dev(kc_ctx* ctx, const uint8_t* d_enc, const uint64_t* enc_off, uint32_t n_units, uint8_t* d_dst,
                                   const uint64_t* dst_off, uint32_t* status);
/* the same with a dictionary's CONTENT (host pointer) as history in front of every frame: frames written with
 * WithEncoderDictRaw, or with WithEncoderDict as long as they do not reuse the dictionary's entropy tables */
kc_status kc_zstd_decode_units_dict_dev(kc_ctx* ctx, const uint8_t* d_enc, const uint64_t* enc_off, uint32_t n_units, uint8_t* d_dst,
                                        const uint64_t* dst_off, uint32_t* status, const uint8_t* dict, uint64_t dict_len);
/* ---- zstd.Decoder.DecodeAll over N independent inputs (zstd/decoder.go:319-410) ----
 * The decoder as a product: no decoded length is supplied; an input is any concatenation of frames and skippable frames, as DecodeAll
 * takes it; window, size and dictionary rules are the reference's; untrusted input is safe (every read is checked against the
 * input's end, every write against the input's own output range; a failing input never touches another input's bytes).
 *
 * Options == decoderOptions (zstd/decoder_options.go): kc_zstd_dopts_default returns a new object with the reference's defaults
 * (WithDecoderMaxMemory 64 GiB, WithDecoderMaxWindow 512 MiB); the setters return 0, or -1 where the reference's option returns an
 * error.  kc_zstd_dopts_dict == WithDecoderDicts (one full-format dictionary per call: ID, content, repeat offsets and the Huffman /
 * FSE tables a frame's first block may reuse; parsed once, here), kc_zstd_dopts_dict_raw == WithDecoderDictRaw; any number may be
 * registered, a frame's Dictionary_ID picks one, a later registration of an ID replaces an earlier one.  The bytes are copied.
 * One deviation: a single frame of more than 4 GiB - 256 decoded bytes is refused with KC_ZD_SIZE_EXCEEDED whatever the limit. */
typedef struct kc_zstd_dopts kc_zstd_dopts;
kc_zstd_dopts* kc_zstd_dopts_default(void);
void kc_zstd_dopts_free(kc_zstd_dopts* o);
int kc_zstd_dopts_max_memory(kc_zstd_dopts* o, uint64_t n);
int kc_zstd_dopts_max_window(kc_zstd_dopts* o, uint64_t n);
int kc_zstd_dopts_ignore_checksum(kc_zstd_dopts* o, int b);
int kc_zstd_dopts_dict(kc_zstd_dopts* o, const uint8_t* blob, uint64_t len);
int kc_zstd_dopts_dict_raw(kc_zstd_dopts* o, uint32_t id, const uint8_t* content, uint64_t len);
/* Per-input status: 0, or the class of the reference's error */
enum {
    KC_ZD_OK = 0,
    KC_ZD_MAGIC = 1,            /* ErrMagicMismatch */
    KC_ZD_EOF = 2,              /* the input ends inside a frame (io.ErrUnexpectedEOF) */
    KC_ZD_UNKNOWN_DICT = 3,     /* ErrUnknownDictionary */
    KC_ZD_WINDOW_EXCEEDED = 4,  /* ErrWindowSizeExceeded */
    KC_ZD_SIZE_EXCEEDED = 5,    /* ErrDecoderSizeExceeded */
    KC_ZD_CRC = 6,              /* ErrCRCMismatch */
    KC_ZD_CORRUPT = 7           /* every other error */
};
/* src: the inputs, concatenated; in_off: n + 1 ascending offsets into it.  Input i decodes to dst + out_off[i] .. out_off[i + 1]
 * (dense: out_off[0] == 0); an input that fails gets status[i] != 0 and an empty range, its neighbours are not affected.  in_off,
 * out_off, status (and bound) are HOST arrays in both forms; src / dst are device memory for _dev, host memory otherwise.
 * KC_ERR_DST_TOO_SMALL when the decoded inputs do not fit dst_cap: nothing is written past dst_cap, out_off and status are
 * unspecified.  The device memory a call takes stays inside the context's scratch ceiling (KC_OPT_MAX_SCRATCH_MIB, and what is free):
 * a batch whose staging does not fit is cut, an input that cannot fit alone gets KC_ZD_SIZE_EXCEEDED.
 * kc_zstd_decode_all_bound[_dev]: the plan alone — bound[i] = the decoded size of input i, exact when every frame carries its
 * content size, else an upper bound from the block headers (at most the size limit); status[i] = the first header-level error. */
kc_status kc_zstd_decode_all_dev(kc_ctx* ctx, const kc_zstd_dopts* o, const uint8_t* d_src, const uint64_t* in_off, uint32_t n,
                                 uint8_t* d_dst, uint64_t dst_cap, uint64_t* out_off, uint32_t* status);
kc_status kc_zstd_decode_all(kc_ctx* ctx, const kc_zstd_dopts* o, const uint8_t* src, const uint64_t* in_off, uint32_t n, uint8_t* dst,
                             uint64_t dst_cap, uint64_t* out_off, uint32_t* status);
kc_status kc_zstd_decode_all_bound_dev(kc_ctx* ctx, const kc_zstd_dopts* o, const uint8_t* d_src, const uint64_t* in_off, uint32_t n,
                                       uint64_t* bound, uint32_t* status);
kc_status kc_zstd_decode_all_bound(kc_ctx* ctx, const kc_zstd_dopts* o, const uint8_t* src, const uint64_t* in_off, uint32_t n,
                                   uint64_t* bound, uint32_t* status);
/* ---- zstd.NewReader(r): the Decoder as a stream reader (zstd/decoder.go:88-118 NewReader, :120-159 Read, :166-234 Reset,
 * :284-312 WriteTo, :486-567 nextBlockSync, :649-940 startStreamDecoder) ----
 * One stream at a time is fed piece by piece from host memory and decoded in bounded memory: the device keeps the frame's last
 * `window` bytes, the tables and repeat offsets a block may reuse, and the running XXH64.  A frame of many blocks is decoded on many
 * waves: every compressed block's literals and sequences on a wave of its own, then one wave executes the blocks in order.
 *
 * kc_zstd_dstream_new (NewReader / Reset): a fresh stream on `ctx` with a copy of the options; blocks per launch from
 * KC_OPT_DSTREAM_BLOCKS.  kc_zstd_dstream_reset (Decoder.Reset, decoder.go:166): the same object for a new stream.
 * kc_zstd_dstream_feed: src[0 .. n) is what the caller holds of the stream from the first byte not yet consumed; eof != 0 says nothing
 * follows it.  A frame header, a block and a checksum are consumed only when whole, a skippable frame's payload piece by piece
 * (never buffered): the caller presents src[*consumed .. n) again with more behind it; fewer than 128 KiB + 3 bytes are ever left.
 * Decoded bytes go to dst[0 .. *produced): as many whole blocks as fit dst_cap by their bound (a raw or RLE block: its size; a
 * compressed block: min(window, 128 KiB)), at most the launch limit at a time; KC_ERR_DST_TOO_SMALL when dst_cap is below one
 * block's bound.  *status: 0, or the KC_ZD_* class of the first error — the bytes of every block in front of it are produced first
 * (all of a frame's bytes in front of KC_ZD_CRC), and the stream stays failed: later calls return the class and nothing else.
 * eof inside a frame is KC_ZD_EOF; eof between frames, an empty stream included, ends the stream cleanly (decoder.go:493).
 * Verdicts follow the reference's stream form: a window above WithDecoderMaxWindow or WithDecoderMaxMemory is KC_ZD_SIZE_EXCEEDED
 * (decoder.go:500, :861-866), WithDecoderMaxMemory never bounds the stream's total, ErrFrameSizeExceeded / ErrFrameSizeMismatch
 * (decoder.go:529-545, :794-801) are KC_ZD_CORRUPT.  Deviations: a stream frame has no 4 GiB limit; the block that overruns
 * Frame_Content_Size is not handed out in front of its error; a dictionary's content is out of reach once the frame's history has
 * slid for the first time (more than window + one launch of output in front of it). */
typedef struct kc_zstd_dstream kc_zstd_dstream;
kc_zstd_dstream* kc_zstd_dstream_new(kc_ctx* ctx, const kc_zstd_dopts* o);
kc_status kc_zstd_dstream_feed(kc_zstd_dstream* s, const uint8_t* src, uint64_t n, int eof, uint8_t* dst, uint64_t dst_cap,
                               uint64_t* consumed, uint64_t* produced, uint32_t* status);
kc_status kc_zstd_dstream_reset(kc_zstd_dstream* s);
void kc_zstd_dstream_free(kc_zstd_dstream* s);
/* ---- s2.Reader / s2.Decode over N independent inputs (s2/reader.go:249-405, s2/decode.go:58-76) ----
 * The S2 decoder as a product: no decoded length is supplied, CRCs are checked, errors carry the reference's classes; untrusted input
 * is safe (every read is checked against the chunk's end, every write against the chunk's own output range).
 * kc_s2_decode_blocks_dev above stays what it is: a verifier that is told every size and has status numbers of its own.
 *
 * Options == the ReaderOptions: kc_s2_ropts_default returns a new object with the reference's defaults (blocks up to 4 MiB, CRCs
 * checked, a stream identifier required); kc_s2_ropts_max_block_size == ReaderMaxBlockSize (s2/reader.go:64: -1 for n <= 0 or
 * n > 4 MiB), kc_s2_ropts_ignore_crc == ReaderIgnoreCRC, kc_s2_ropts_ignore_stream_identifier == ReaderIgnoreStreamIdentifier. */
typedef struct kc_s2_ropts kc_s2_ropts;
kc_s2_ropts* kc_s2_ropts_default(void);
void kc_s2_ropts_free(kc_s2_ropts* o);
int kc_s2_ropts_max_block_size(kc_s2_ropts* o, int64_t n);
int kc_s2_ropts_ignore_crc(kc_s2_ropts* o, int b);
int kc_s2_ropts_ignore_stream_identifier(kc_s2_ropts* o, int b);
/* Per-input status: 0, or the class of the reference's error */
enum {
    KC_S2D_OK = 0,
    KC_S2D_CORRUPT = 1,        /* ErrCorrupt */
    KC_S2D_CRC = 2,            /* ErrCRC */
    KC_S2D_UNSUPPORTED = 3,    /* ErrUnsupported */
    KC_S2D_SIZE_EXCEEDED = 4,  /* a limit of this library: host-buffer calls, an input that does not fit the scratch ceiling alone */
    KC_S2D_EOF = 5,            /* ranged reads: io.EOF — the input ended inside the range, got < len */
    KC_S2D_UNEXPECTED_EOF = 6, /* ranged reads: io.ErrUnexpectedEOF — the input ended in front of the range (Reader.Skip, Index.Find) */
    KC_S2D_CALLBACK = 7        /* stream reader: a skippable-chunk callback returned non-zero (the reference returns the callback's error) */
};
/* kc_s2_decode_streams[_dev] == io.ReadAll(s2.NewReader(input, options)) for every input (s2/reader.go:249-405).  src: the inputs,
 * concatenated; in_off: n + 1 ascending offsets into it.  Input i is any concatenation of .s2 or Snappy-framed streams, as
 * s2.NewReader reads it: stream identifiers of both kinds, compressed and uncompressed chunks, padding, index and other skippable
 * chunks.  in_off, out_off, status (and bound) are HOST arrays in both forms; src / dst are device memory for _dev, host memory
 * otherwise.
 *
 * The output contract differs from kc_zstd_decode_all's ON PURPOSE.  An S2 chunk states its decoded length in its header, so the sizes
 * are exact before any byte is decoded: out_off (n + 1 entries, out_off[0] == 0, ascending) is the PLANNED layout — the prefix sum of
 * bound — and every chunk decodes straight into dst at its planned place; there is no staging copy and no compaction pass.  An input
 * that fails (status[i] != 0) KEEPS its planned range — the decoded bytes of the chunks in front of the first header-level error — and
 * the library ZERO-FILLS that range before it returns: no byte decoded from a corrupt stream is left in dst, and its neighbours are
 * untouched.  (The reference's sequential Reader hands out the chunks in front of an error; this API does not.)  The first failing
 * chunk in stream order decides the status, in the reference's order inside a chunk: DecodedLen, Snappy's 64 KiB limit, the block
 * size limit, the decode, the CRC.  KC_ERR_DST_TOO_SMALL when out_off[n] > dst_cap: nothing is written in that case.
 *
 * Host-buffer form: the inputs go to the device in groups cut between inputs, each group's bytes and decoded bytes within a quarter of
 * the context's scratch ceiling (KC_OPT_MAX_SCRATCH_MIB, and what is free); an input that does not fit alone gets
 * KC_S2D_SIZE_EXCEEDED and a zero-filled range.  It does not use the rolling host pipeline.
 * kc_s2_decode_streams_bound[_dev]: the plan alone (s2/reader.go:259-404, the chunk headers) — bound[i] = the bytes input i decodes to,
 * exact if the input stands; status[i] = the first header-level error.
 * kc_s2_decode_blocks_all[_dev]: N bare blocks (uvarint length + body, S2 or Snappy) == N x s2.Decode(nil, block) (s2/decode.go:58-76)
 * with the same output contract; every error is KC_S2D_CORRUPT.  _bound == N x s2.DecodedLen (s2/decode.go:29-47). */
kc_status kc_s2_decode_streams_dev(kc_ctx* ctx, const kc_s2_ropts* o, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, uint8_t* d_dst,
                                   uint64_t dst_cap, uint64_t* out_off, uint32_t* status);
kc_status kc_s2_decode_streams(kc_ctx* ctx, const kc_s2_ropts* o, const uint8_t* src, const uint64_t* in_off, uint32_t n, uint8_t* dst,
                               uint64_t dst_cap, uint64_t* out_off, uint32_t* status);
kc_status kc_s2_decode_streams_bound_dev(kc_ctx* ctx, const kc_s2_ropts* o, const uint8_t* d_src, const uint64_t* in_off, uint32_t n,
                                         uint64_t* bound, uint32_t* status);
kc_status kc_s2_decode_streams_bound(kc_ctx* ctx, const kc_s2_ropts* o, const uint8_t* src, const uint64_t* in_off, uint32_t n,
                                     uint64_t* bound, uint32_t* status);
kc_status kc_s2_decode_blocks_all_dev(kc_ctx* ctx, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, uint8_t* d_dst, uint64_t dst_cap,
                                      uint64_t* out_off, uint32_t* status);
kc_status kc_s2_decode_blocks_all(kc_ctx* ctx, const uint8_t* src, const uint64_t* in_off, uint32_t n, uint8_t* dst, uint64_t dst_cap,
                                  uint64_t* out_off, uint32_t* status);
kc_status kc_s2_decode_blocks_all_bound_dev(kc_ctx* ctx, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, uint64_t* bound,
                                            uint32_t* status);
kc_status kc_s2_decode_blocks_all_bound(kc_ctx* ctx, const uint8_t* src, const uint64_t* in_off, uint32_t n, uint64_t* bound,
                                        uint32_t* status);
/* ---- s2.Index and ranged reads: Index.Load / LoadStream / Find, IndexStream, ReadSeeker.ReadAt over a batch of requests ----
 * (s2/index.go, s2/reader.go:669-1041)
 *
 * The index on the host (plain C++, no device): a kc_s2_index holds what s2.Index holds — the totals, the block size estimate and the
 * (compressed offset, uncompressed offset) entries.  Every read of index bytes is bounds-checked; the results are the reference's:
 * KC_S2I_UNEXPECTED_EOF == io.ErrUnexpectedEOF, KC_S2I_CORRUPT == ErrCorrupt, KC_S2I_UNSUPPORTED == ErrUnsupported, returned at the
 * places where Index.Load (index.go:238-374), Index.LoadStream (:381-413, over a buffer: a missing trailer is KC_S2I_UNSUPPORTED,
 * fewer than 10 bytes: the reference's Seek fails; here KC_S2I_UNEXPECTED_EOF) and Index.Find (:97-127; negative offsets
 * count from the end, an offset behind the end is KC_S2I_UNEXPECTED_EOF) return them.  The numbers equal the KC_S2D_* classes.
 * kc_s2_index_load: *consumed (may be null) = the bytes of b in front of the rest Index.Load returns.  Like the reference, a failed
 * load leaves the index partly overwritten.  kc_s2_index_entries copies up to cap entries and returns the entry count.
 * kc_s2_index_stream == s2.IndexStream (:420-516): walks the chunk headers of src and writes the index chunk Index.appendTo builds
 * to out (cap bytes; KC_ERR_DST_TOO_SMALL with *out_len = the bytes needed).  *status = 0 or the class of the reference's error
 * (nothing is written then).  Its checks are IndexStream's own, not the Reader's: chunkLen < 4 is corrupt for every chunk type and
 * the block limit is maxBlockSize (4 MiB) whatever a reader would be told. */
enum { KC_S2I_OK = 0, KC_S2I_CORRUPT = 1, KC_S2I_UNSUPPORTED = 3, KC_S2I_UNEXPECTED_EOF = 6 };
typedef struct kc_s2_index kc_s2_index;
kc_s2_index* kc_s2_index_new(void);
void kc_s2_index_free(kc_s2_index* ix);
int kc_s2_index_load(kc_s2_index* ix, const uint8_t* b, uint64_t n, uint64_t* consumed);
int kc_s2_index_load_stream(kc_s2_index* ix, const uint8_t* stream, uint64_t n);
int kc_s2_index_find(const kc_s2_index* ix, int64_t offset, int64_t* c_off, int64_t* u_off);
int64_t kc_s2_index_total_uncompressed(const kc_s2_index* ix);
int64_t kc_s2_index_total_compressed(const kc_s2_index* ix);
int64_t kc_s2_index_est_block_uncompressed(const kc_s2_index* ix);
uint32_t kc_s2_index_entries(const kc_s2_index* ix, int64_t* c_off, int64_t* u_off, uint32_t cap);
kc_status kc_s2_index_stream(const uint8_t* src, uint64_t n, uint8_t* out, uint64_t cap, uint64_t* out_len, uint32_t* status);
/* kc_s2_read_ranges[_dev] == for every request j: s2.NewReader(input req_stream[j], options).ReadSeeker(true, index).ReadAt(p, req_off[j])
 * with len(p) == req_len[j], as one batch.  src / in_off / n_streams: the inputs as for kc_s2_decode_streams.  index: n_streams
 * pointers (the array itself may be null), a null entry = no index: the request is then served by walking the input from its start
 * (Reader.Skip), otherwise from the entry Index.Find gives for req_off[j].  All arrays are HOST arrays; src / dst are device memory
 * for _dev, host memory otherwise.
 *
 * Layout: request j owns dst[out_off[j], out_off[j + 1]) with out_off the prefix sum of req_len (m + 1 entries), whatever the data
 * holds.  KC_ERR_DST_TOO_SMALL when out_off[m] > dst_cap, before anything is written; KC_ERR_BAD_ARG for a request that names an input
 * >= n_streams or whose off + len wraps.  status[j] / got[j]:
 *   KC_S2D_OK               got == len.
 *   KC_S2D_EOF              the input ended inside the range: got < len bytes stand at the front of the request's range, the rest
 *                           is zero-filled (ReadAt: n < len(p), io.EOF).
 *   KC_S2D_UNEXPECTED_EOF   the input ended in front of off (Skip), or Index.Find refused off; got == 0.
 *   any other class         the first failing covered chunk in stream order, else the first header-level error of the walk; got == 0.
 * Whenever got == 0 by an error the request's whole range is zero-filled.  A request whose Find fails never reaches the device.
 *
 * What is read: the chunk headers from the walk's start up to the chunk whose decoded end reaches off + len, and the bodies of the
 * chunks from the one that holds off onwards (the covered chunks; their CRCs are checked over the whole chunk).  Chunks in front of
 * off are passed by their headers alone — chunk type, chunk length, DecodedLen and the block size limits are checked, bodies and
 * CRCs are not ("CRC is not checked on skipped blocks", reader.go:671) — and nothing behind the last covered chunk is read.  For
 * len == 0 the chunk that holds off is still decoded and checked, unless off is a chunk's end (or the walk's start).
 * A walk that starts at an index entry starts in the state the reader has behind the stream identifier at the input's front: an
 * input without one is KC_S2D_CORRUPT unless identifiers are ignored.
 * Differences from the reference, on purpose: (1) Reader.Skip CRC-checks an UNCOMPRESSED chunk it passes when the chunk is shorter
 * than what is left to skip (reader.go:799); here no skipped chunk's body is read.  (2) The reference's first Seek decodes the first
 * data chunk of the input before it seeks (reader.go:953-959); here the front is read for its identifier only.  (3) Skip does not
 * apply Snappy's 64 KiB limit to the chunks it passes; the walk here does, as for every chunk.
 *
 * Host-buffer form: per request only the compressed bytes from its index entry up to the first entry at or above off + len (the
 * input's end without an index, or behind the last entry) are staged, in groups whose staged bytes and lengths fit a quarter of
 * the scratch ceiling; a request that does not fit alone gets KC_S2D_SIZE_EXCEEDED and a zero-filled range.  An index that lies
 * about where chunks start can so turn into KC_S2D_CORRUPT / KC_S2D_EOF where the device-resident form would read on. */
kc_status kc_s2_read_ranges_dev(kc_ctx* ctx, const kc_s2_ropts* o, const uint8_t* d_src, const uint64_t* in_off, uint32_t n_streams,
                                const kc_s2_index* const* index, const uint32_t* req_stream, const uint64_t* req_off, const uint64_t* req_len,
                                uint32_t m, uint8_t* d_dst, uint64_t dst_cap, uint64_t* out_off, uint64_t* got, uint32_t* status);
kc_status kc_s2_read_ranges(kc_ctx* ctx, const kc_s2_ropts* o, const uint8_t* src, const uint64_t* in_off, uint32_t n_streams,
                            const kc_s2_index* const* index, const uint32_t* req_stream, const uint64_t* req_off, const uint64_t* req_len,
                            uint32_t m, uint8_t* dst, uint64_t dst_cap, uint64_t* out_off, uint64_t* got, uint32_t* status);
/* ---- s2.NewReader(r) as a stream reader: Read / Skip / ReadByte / skippable-chunk callbacks (s2/reader.go:249-405 Read, :190-198
 * readFull, :200-246 skippable, :109 ReaderSkippableCB, :674-842 Skip, :177 Reset) ----
 * One stream at a time is fed piece by piece from host memory and decoded in bounded memory: a .s2 file larger than memory can be read.
 * The device keeps one window — the staged compressed bytes of up to KC_OPT_S2_RSTREAM_CHUNKS data chunks and their decoded bytes —,
 * decodes it with one wave per chunk and copies the deliverable prefix straight to the caller's dst.  One window at a time, synchronous.
 *
 * kc_s2_rstream_new (NewReader): a fresh stream on `ctx` with a copy of the options.  kc_s2_rstream_reset (Reset, :177): the same
 * object and the same device buffers for a new stream; options and callbacks stay.  Both take KC_OPT_S2_RSTREAM_CHUNKS as the
 * context holds it at that moment.  A copy or launch that fails is no verdict on the input: feed returns that kc_status, and every
 * later feed returns it again until the stream is reset.  kc_s2_rstream_free releases the stream and its device buffers.
 * kc_s2_rstream_feed (Read, :249-405): src[0 .. n) is what the caller holds of the stream from the first byte not yet consumed;
 * eof != 0 says nothing follows it.  src and dst are host memory.  KC_ERR_BAD_ARG while the context has a pending batch or job.
 *   Consuming: a data chunk that is to be decoded is consumed only when whole (fewer than 4 + MaxEncodedLen(max block) + 4 bytes are
 *   ever left unconsumed), a stream identifier when whole.  The payload of a skippable, padding or index chunk and the body of a data
 *   chunk that lies wholly inside a pending skip are counted down piece by piece and never buffered; for such a data chunk only the
 *   header is needed, for type 0x00 also the uvarint.
 *   Producing: dst[0 .. *produced) receives as many whole chunks, in stream order, as fit dst_cap by their stated decoded length, at
 *   most the window limit per launch; nothing is written at or behind dst + *produced.  KC_ERR_DST_TOO_SMALL when the next chunk to
 *   hand out does not fit dst_cap and nothing else can be produced: nothing is consumed or written then and the stream stays usable.
 *   Errors: *status is 0 or the KC_S2D_* class of the first error in stream order — the reference's sequential behaviour, which
 *   kc_s2_decode_streams deliberately does not have: the bytes of every chunk in front of the error are produced first, in the same
 *   call or earlier ones, and the stream stays failed: later calls return the class and nothing else.  Inside a chunk the order is
 *   that of kc_s2_decode_streams: DecodedLen, Snappy's 64 KiB limit, the block size limit, the decode, the CRC.
 *   End of input: eof at a chunk boundary, an empty input included, is the clean end (consumed == n, produced == 0, status 0;
 *   :259-261); eof with 1-3 stray bytes or inside any chunk is KC_S2D_CORRUPT (readFull, :190-198); eof while a skip is pending is
 *   KC_S2D_UNEXPECTED_EOF (:700-705).  The same bytes without eof: the call waits — status 0, consumption stops at the boundary.
 * kc_s2_rstream_skip (Skip, :674-842) adds n to the pending skip, kc_s2_rstream_skip_left returns what is left of it; the following
 * feeds pass the chunks wholly inside the skip by their headers — their bodies are not staged, decoded or CRC-checked — and decode
 * the chunk that holds the skip's end whole, checked over the whole chunk; only its bytes behind the skip go to dst and must fit
 * dst_cap.  Verdicts and deviations are those of kc_s2_read_ranges: (1) no body of a skipped chunk is read (the reference CRC-checks
 * some skipped uncompressed chunks, :799); (2) Snappy's 64 KiB limit applies to passed chunks too; (3) a CRC mismatch in the partly
 * skipped chunk is KC_S2D_CRC and honours ReaderIgnoreCRC (the reference says ErrCorrupt there, :757-760).
 * kc_s2_rstream_on_skippable (ReaderSkippableCB, :109): id outside 0x80 .. 0xfd is KC_ERR_BAD_ARG, a null fn removes the callback.  A
 * chunk with a callback is handed over as pieces, in order: fn(user, id, piece, n, left) with `left` the bytes of the chunk still to
 * come; a chunk of length 0 gets one call with n == 0, left == 0.  The callback runs inside feed, and only after every decoded byte in
 * front of that chunk has been returned by an earlier feed (a window never reaches past such a chunk): a caller that asks for more
 * only when it has handed everything out sees the reference's lazy order.  A non-zero return fails the stream with KC_S2D_CALLBACK. */
typedef struct kc_s2_rstream kc_s2_rstream;
typedef int (*kc_s2_skippable_fn)(void* user, uint8_t id, const uint8_t* piece, uint64_t n, uint64_t left);
kc_s2_rstream* kc_s2_rstream_new(kc_ctx* ctx, const kc_s2_ropts* o);
kc_status kc_s2_rstream_feed(kc_s2_rstream* s, const uint8_t* src, uint64_t n, int eof, uint8_t* dst, uint64_t dst_cap,
                             uint64_t* consumed, uint64_t* produced, uint32_t* status);
kc_status kc_s2_rstream_skip(kc_s2_rstream* s, uint64_t n);
uint64_t kc_s2_rstream_skip_left(const kc_s2_rstream* s);
kc_status kc_s2_rstream_on_skippable(kc_s2_rstream* s, uint8_t id, kc_s2_skippable_fn fn, void* user);
kc_status kc_s2_rstream_reset(kc_s2_rstream* s);
void kc_s2_rstream_free(kc_s2_rstream* s);
/* ---- flate.NewReader / gzip.NewReader / zlib.NewReader over a batch of independent inputs (inflate) ----
 * Raw DEFLATE (RFC 1951), gzip (RFC 1952) and zlib (RFC 1950), whole inputs, ONE WAVE PER INPUT: zip members, gzip members, BGZF blocks, HTTP
 * bodies, PNG IDAT runs.  No sizes are supplied: a sizing pass walks every input and yields its exact decoded size before any byte
 * is written, the prefix sum of the sizes is the output layout, and a write pass decodes every input straight to its place.
 * Options: kc_flate_ropts_default returns a new object with the reference's defaults (no dictionary, multistream on);
 * kc_flate_ropts_dict == flate.NewReaderDict (flate/inflate.go:948-957): ONE preset dictionary per call, of which the last 32 KiB
 * count (the window) and all bytes make zlib's DICTID; it is read by the flate and zlib entry points.  kc_flate_ropts_multistream == gzip.Reader.Multistream
 * (gzip/gunzip.go:126-144), read by the gzip entry points only.  Both return 0, -1 on a null object. */
typedef struct kc_flate_ropts kc_flate_ropts;
kc_flate_ropts* kc_flate_ropts_default(void);
void kc_flate_ropts_free(kc_flate_ropts* o);
int kc_flate_ropts_dict(kc_flate_ropts* o, const uint8_t* bytes, uint64_t len);
int kc_flate_ropts_multistream(kc_flate_ropts* o, int b);
/* per-input status of the inflate entry points */
enum {
    KC_FL_OK = 0,
    KC_FL_CORRUPT = 1,        /* flate.CorruptInputError, whatever its offset */
    KC_FL_EOF = 2,            /* io.ErrUnexpectedEOF; also a gzip input of zero bytes, for which gzip.NewReader returns io.EOF */
    KC_FL_HEADER = 3,         /* gzip.ErrHeader */
    KC_FL_CHECKSUM = 4,       /* gzip.ErrChecksum: CRC-32 or ISIZE */
    KC_FL_SIZE_EXCEEDED = 5,  /* a limit of this library, the one deviation from the reference: an input that decodes to more than 1 GiB,
                                 or (host-buffer forms) one whose input bytes plus decoded bytes are above a quarter of the context's
                                 scratch budget (KC_OPT_MAX_SCRATCH_MIB, and 85 % of what is free) */
    KC_FL_DICTIONARY = 6      /* zlib.ErrDictionary: the stream names a preset dictionary other than the call's (zlib/reader.go:164-168) */
};
/* kc_flate_inflate[_dev] == io.ReadAll(flate.NewReaderDict(bytes.NewReader(input), dict)) for every input (flate/inflate.go:352-395
 * nextBlock, :464-597 readHuffman, :600-670 dataBlock / copyData, :116-176 huffmanDecoder.init, :740-783 huffSym;
 * flate/inflate_gen.go:45-270 the block body).  src: the inputs, concatenated; in_off: n + 1 ascending offsets; dst / dst_cap: the
 * output; out_off[n + 1], status[n], consumed[n] (may be NULL): host arrays in both forms.  The _dev form takes device pointers
 * for src and dst.
 * Output: out_off is dense — input i owns dst[out_off[i], out_off[i + 1]), its exact decoded size.  An input that fails gets an
 * empty range, or (gzip) the range of its members in front of the failure, zero-filled: in neither case is a byte decoded from a
 * failed input left in dst, and its neighbours are untouched.  KC_ERR_DST_TOO_SMALL when out_off[n] > dst_cap: nothing is written,
 * and out_off holds the planned layout — out_off[n] is the capacity to come back with.
 * consumed[i]: the input bytes up to and including the byte that holds the last bit of the final block — the reference never reads
 * past it from a ByteReader (inflate.go:582-594); bytes behind it are ignored.  0 for an input that failed.
 * The reference's own quirk is kept: an input that ends inside the extra bits of a length or distance, or inside a fixed block's
 * five distance bits, ends with the raw io.EOF (inflate_gen.go:114-122, 142-151, 210-219), so ReadAll returns what was decoded
 * WITHOUT an error: KC_FL_OK.  (gzip then misses its trailer: KC_FL_EOF.)
 * One divergence from the reference, observed against its own code (profiles/flate_reference_parity.md): a symbol read through an
 * EMPTY Huffman table — a match in a dynamic block without a distance code, a block without a literal/length code, a header without
 * a code-length code — is KC_FL_CORRUPT, as in RFC 1951 and zlib.  The reference's huffmanDecoder.init returns on an empty code before
 * it clears the table (inflate.go:154-156), so it decodes such a symbol through what that decoder held last — the previous dynamic
 * block's distance code, the same block's code-length code, the previous literal/length code — and accepts some of these inputs,
 * answers others with io.ErrUnexpectedEOF or a flate.InternalError.  No encoder writes such a block.
 * kc_flate_inflate_bound[_dev]: the sizing pass alone — bound[i] = the exact decoded size of every input that stands, status[i] its
 * verdict, consumed[i] as above.
 * The host-buffer forms stage the inputs in groups cut between inputs: a group's input bytes (first sweep, the sizes) and its input
 * bytes plus decoded bytes (second sweep, the write) stay within a QUARTER of the context's scratch budget — the smaller of
 * KC_OPT_MAX_SCRATCH_MIB and 85 % of the free device memory.  An input whose bytes, or whose bytes plus decoded bytes, are above
 * that quarter alone gets KC_FL_SIZE_EXCEEDED.  They do not use the rolling host pipeline. */
kc_status kc_flate_inflate_dev(kc_ctx* ctx, const kc_flate_ropts* o, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, uint8_t* d_dst,
                               uint64_t dst_cap, uint64_t* out_off, uint32_t* status, uint64_t* consumed);
kc_status kc_flate_inflate(kc_ctx* ctx, const kc_flate_ropts* o, const uint8_t* src, const uint64_t* in_off, uint32_t n, uint8_t* dst,
                           uint64_t dst_cap, uint64_t* out_off, uint32_t* status, uint64_t* consumed);
kc_status kc_flate_inflate_bound_dev(kc_ctx* ctx, const kc_flate_ropts* o, const uint8_t* d_src, const uint64_t* in_off, uint32_t n,
                                     uint64_t* bound, uint32_t* status, uint64_t* consumed);
kc_status kc_flate_inflate_bound(kc_ctx* ctx, const kc_flate_ropts* o, const uint8_t* src, const uint64_t* in_off, uint32_t n,
                                 uint64_t* bound, uint32_t* status, uint64_t* consumed);
/* kc_gzip_inflate[_dev] == io.ReadAll(gzip.NewReader(bytes.NewReader(input))) for every input, under Multistream (gzip/gunzip.go:94-124
 * NewReader / Reset, :183-253 readHeader, :255-295 Read: the trailer, the next member).  Arguments and output as above.
 * consumed[i] runs through the last trailer read; with Multistream off, what lies behind it is the next member's header.  One input
 * is read further and still stands: behind a complete member, a next header whose name or comment runs into the input's end is the
 * reference's raw io.EOF (gunzip.go:157-160) — the file ends there, and consumed[i] is the whole input, which the reader has read.
 * The sizing pass walks headers, streams, trailers and the ISIZE compare, member after member; the write pass computes the CRC-32 of
 * every member's bytes and compares it with the trailer (KC_FL_CHECKSUM: the planned range is zero-filled).  An input that fails
 * behind complete members keeps their range, zero-filled.  kc_gzip_inflate_bound[_dev]: the sizing pass alone — the first error short
 * of the CRC-32; bound[i] of a failed input is the size of the range it would keep.  The Header fields are parsed by the caller
 * (compress_amd/gzip.py).  ISIZE is compared modulo 2^32 as in the reference. */
kc_status kc_gzip_inflate_dev(kc_ctx* ctx, const kc_flate_ropts* o, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, uint8_t* d_dst,
                              uint64_t dst_cap, uint64_t* out_off, uint32_t* status, uint64_t* consumed);
kc_status kc_gzip_inflate(kc_ctx* ctx, const kc_flate_ropts* o, const uint8_t* src, const uint64_t* in_off, uint32_t n, uint8_t* dst,
                          uint64_t dst_cap, uint64_t* out_off, uint32_t* status, uint64_t* consumed);
kc_status kc_gzip_inflate_bound_dev(kc_ctx* ctx, const kc_flate_ropts* o, const uint8_t* d_src, const uint64_t* in_off, uint32_t n,
                                    uint64_t* bound, uint32_t* status, uint64_t* consumed);
kc_status kc_gzip_inflate_bound(kc_ctx* ctx, const kc_flate_ropts* o, const uint8_t* src, const uint64_t* in_off, uint32_t n,
                                uint64_t* bound, uint32_t* status, uint64_t* consumed);
/* kc_zlib_inflate[_dev] == io.ReadAll(zlib.NewReaderDict(bytes.NewReader(input), dict)) for every input, each from a FRESH reader
 * (zlib/reader.go:84-91 NewReaderDict, :134-187 Reset: the header, :93-121 Read: the trailer): zlib streams (RFC 1950) such as PNG
 * IDAT runs, git objects, PDF streams, HTTP `deflate` bodies.  Arguments and output as above; kc_flate_ropts_dict gives the preset
 * dictionary, multistream is not read.
 * Fewer than 2 bytes: KC_FL_EOF (:143-149).  CM other than 8, CINFO above 7 or a header not divisible by 31: KC_FL_HEADER (:150-154).
 * With FDICT four more bytes are needed (KC_FL_EOF) and are compared, big-endian, with the Adler-32 of the WHOLE dictionary given
 * to kc_flate_ropts_dict — not of the 32 KiB the window keeps —: KC_FL_DICTIONARY when they differ (:155-169).  Without a dictionary
 * the value compared with is adler32(nil) = 1, so a stream with FDICT and DICTID 1 is accepted and decoded without history, as in the
 * reference.  Without FDICT the dictionary is ignored (:171-176).  The reference hands the dictionary to a REUSED decompressor even
 * without FDICT (Reset, :177-179); that is not modelled: every input has a fresh reader, and so has compress_amd.zlib's Reader.Reset.
 * The DEFLATE stream is decoded as for kc_flate_inflate, divergence and raw io.EOF included (the trailer is then missing: KC_FL_EOF).
 * Four bytes follow the byte that holds the stream's last bit (fewer: KC_FL_EOF, :107-113): the big-endian Adler-32 of the decoded
 * bytes.  The write pass computes it wave-wide over what it wrote; a mismatch is KC_FL_CHECKSUM (:115-119) and leaves the planned
 * range zero-filled; every other failure leaves an empty range.  Bytes behind the trailer are ignored — there is no second member —
 * and consumed[i] runs through the trailer.  kc_zlib_inflate_bound[_dev]: the sizing pass alone, every verdict short of the Adler-32. */
kc_status kc_zlib_inflate_dev(kc_ctx* ctx, const kc_flate_ropts* o, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, uint8_t* d_dst,
                              uint64_t dst_cap, uint64_t* out_off, uint32_t* status, uint64_t* consumed);
kc_status kc_zlib_inflate(kc_ctx* ctx, const kc_flate_ropts* o, const uint8_t* src, const uint64_t* in_off, uint32_t n, uint8_t* dst,
                          uint64_t dst_cap, uint64_t* out_off, uint32_t* status, uint64_t* consumed);
kc_status kc_zlib_inflate_bound_dev(kc_ctx* ctx, const kc_flate_ropts* o, const uint8_t* d_src, const uint64_t* in_off, uint32_t n,
                                    uint64_t* bound, uint32_t* status, uint64_t* consumed);
kc_status kc_zlib_inflate_bound(kc_ctx* ctx, const kc_flate_ropts* o, const uint8_t* src, const uint64_t* in_off, uint32_t n,
                                uint64_t* bound, uint32_t* status, uint64_t* consumed);

/* ---- zip.NewReader / File.Open over a batch of archive members (zip/reader.go, zip/struct.go) ----
 * Two halves.  The DIRECTORY is read on the host, from an archive held in memory, without a device or a context: kc_zip_dir_load is
 * Reader.init (reader.go:146-207) with readDirectoryEnd (:605-682: the end record searched in the last 1 KiB, then the last 65 KiB;
 * the zip64 locator and end record followed; baseOffset, and a valid header at offset 0 winning over it, :668-679), and
 * readDirectoryHeader (:386-564) until a bad header, the count compared modulo 65536 only (:188).  The zip64 extra replaces only the
 * fields that are maxed out, a short one is KC_ZIP_FORMAT, an uncompressed size of 2^32 - 1 stands without one (:446-561); NonUTF8
 * follows the three-way rule of :428-444.  Returns KC_ZIP_OK and *dir, or the class of the reference's error and *dir = null:
 * KC_ZIP_FORMAT (zip.ErrFormat), KC_ZIP_EOF (io.ErrUnexpectedEOF; also the plain io.EOF that the ReaderAt returns for a zip64 end
 * record past the archive's end and that a directory running exactly to the archive's end yields), KC_ZIP_COMMENT ("zip: invalid
 * comment length").  The entries' name, comment and extra and the archive comment point into buf, which must outlive the object.
 * header_offset has baseOffset applied.  kc_zip_dir_members fills the member table below from the entries [first, first + n).
 *
 * The MEMBERS are read on the device, one call over one source buffer and a table of n members whose header offsets are absolute in
 * that buffer (the entries of several archives laid into one buffer are one batch).  Every member gets the verdict of f.Open(),
 * io.ReadAll, Close (reader.go:247-362, 368-381, 566-603), in this order:
 *   1. thirty bytes at header_offset: not all inside the buffer, or a negative offset: KC_ZIP_READAT (the ReaderAt's own error, io.EOF
 *      over a byte slice); a wrong signature: KC_ZIP_FORMAT.  The body starts 30 + name length + extra length of the LOCAL header on.
 *   2. is_dir (a name ending in "/"): a nonzero uncompressed size is KC_ZIP_FORMAT, else the member is empty and KC_ZIP_OK (:252-267).
 *   3. a method other than 0 (Store) and 8 (Deflate): KC_ZIP_ALGORITHM (:270-273).
 *   4. a compressed or uncompressed size above 1 GiB: KC_ZIP_SIZE, a limit of this library and its one deviation from the reference.
 *   5. the body is [body, body + compressed_size) clipped to the buffer (a SectionReader over a shorter file ends early).  With d the
 *      bytes the decompressor yields before it ends or fails (the bytes of a cut stored DEFLATE block included): d above the
 *      uncompressed size is KC_ZIP_FORMAT whatever follows (:331-333); else the decompressor's own KC_FL_CORRUPT / KC_FL_EOF stands;
 *      else d below the uncompressed size is KC_FL_EOF (:338-340).  The raw io.EOF of kc_flate_inflate counts as an end.
 *   6. flag bit 3: the data descriptor behind body + compressed_size, 16 bytes with the signature 0x08074b50 and 12 without (:566-603);
 *      absent or short: KC_FL_EOF; its CRC field, then the CRC-32 of the decoded bytes, against the table's: KC_ZIP_CHECKSUM.
 *   7. else the CRC-32 of the decoded bytes is compared where the table's is nonzero (:352-357): KC_ZIP_CHECKSUM.
 * The device decodes every member ONCE, straight to its place, bounded by the size the table states: there is no sizing pass.
 * out_off[n + 1] is the prefix sum of the stated uncompressed sizes over the members that get a range.  None get: the verdicts of
 * rules 1 to 4; a stored member whose clipped compressed size differs from its uncompressed size; a deflated member whose stated
 * size exceeds 1032 x its clipped compressed size + 1032 (DEFLATE cannot expand further: it is walked without writing to learn
 * whether it is KC_FL_CORRUPT or KC_FL_EOF).  KC_ERR_DST_TOO_SMALL when out_off[n] > dst_cap: the layout is filled, nothing is
 * written.  A member that fails with a range keeps it, zero-filled.  CRC-32s are computed on the device: wave-wide for a deflated
 * member, per 64 KiB chunk with the chunk values combined for a stored one.
 * kc_zip_read: host buffers, staged whole as kc_flate_inflate stages a group (KC_ERR_UNSUPPORTED when the archive and the layout
 * exceed the scratch budget); kc_zip_read_bound: the layout and the verdicts that need no decoding (rules 1 to 4 and the size
 * rules above; the others KC_ZIP_OK). */
enum {
    KC_ZIP_OK = 0,          /* per member: also KC_FL_CORRUPT (1) and KC_FL_EOF (2) */
    KC_ZIP_FORMAT = 16,     /* zip.ErrFormat "zip: not a valid zip file" */
    KC_ZIP_EOF = 17,        /* directory only: io.ErrUnexpectedEOF / io.EOF */
    KC_ZIP_COMMENT = 18,    /* directory only: "zip: invalid comment length" */
    KC_ZIP_ALGORITHM = 19,  /* zip.ErrAlgorithm "zip: unsupported compression algorithm" */
    KC_ZIP_CHECKSUM = 20,   /* zip.ErrChecksum "zip: checksum error" */
    KC_ZIP_READAT = 21,     /* the ReaderAt's error for the local header: io.EOF, or "negative offset" */
    KC_ZIP_SIZE = 22        /* a member above 1 GiB: this library's limit */
};
typedef struct kc_zip_entry {   /* zip.FileHeader, the fields read from the directory (struct.go:86-160) */
    const uint8_t* name;        /* Name, Comment, Extra: raw bytes inside the archive buffer */
    const uint8_t* comment;
    const uint8_t* extra;
    uint32_t name_len, comment_len, extra_len;
    uint32_t non_utf8;          /* NonUTF8 */
    uint16_t creator_version, reader_version, flags, method, modified_time, modified_date;
    uint32_t crc32;
    uint64_t compressed_size64, uncompressed_size64;
    int64_t header_offset;      /* File.headerOffset: baseOffset applied */
    uint32_t external_attrs;
    uint32_t reserved;
} kc_zip_entry;
typedef struct kc_zip_member {
    int64_t header_offset;      /* absolute in the source buffer */
    uint64_t compressed_size, uncompressed_size;
    uint32_t crc32;
    uint16_t method, flags;
    uint32_t is_dir;            /* the name ends in "/" */
    uint32_t reserved;
} kc_zip_member;
typedef struct kc_zip_dir kc_zip_dir;
int kc_zip_dir_load(const uint8_t* buf, uint64_t len, kc_zip_dir** dir);
void kc_zip_dir_free(kc_zip_dir* dir);
uint64_t kc_zip_dir_count(const kc_zip_dir* dir);
int64_t kc_zip_dir_base_offset(const kc_zip_dir* dir);
const uint8_t* kc_zip_dir_comment(const kc_zip_dir* dir, uint32_t* len);
int kc_zip_dir_entry(const kc_zip_dir* dir, uint64_t i, kc_zip_entry* out);
int kc_zip_dir_members(const kc_zip_dir* dir, uint64_t first, uint64_t n, kc_zip_member* out);
kc_status kc_zip_read_dev(kc_ctx* ctx, const uint8_t* d_src, uint64_t src_len, const kc_zip_member* members, uint32_t n, uint8_t* d_dst,
                          uint64_t dst_cap, uint64_t* out_off, uint32_t* status);
kc_status kc_zip_read(kc_ctx* ctx, const uint8_t* src, uint64_t src_len, const kc_zip_member* members, uint32_t n, uint8_t* dst,
                      uint64_t dst_cap, uint64_t* out_off, uint32_t* status);
kc_status kc_zip_read_bound(kc_ctx* ctx, const uint8_t* src, uint64_t src_len, const kc_zip_member* members, uint32_t n, uint64_t* out_off,
                            uint32_t* status);

/* ---- flate.NewWriter / gzip.NewWriterLevel at flate.HuffmanOnly over a batch of independent inputs (deflate) ----
 * The output of every input is, byte for byte, what flate.NewWriter(w, flate.HuffmanOnly); Write(input); Close() writes
 * (flate/deflate.go:755-770 write, :701-708 storeHuff, :865-880 close; flate/huffman_bit_writer.go:987-1174 writeBlockHuff,
 * :269-348 generateCodegen, :458-497 writeDynamicHeader, :502-529 writeStoredHeader; flate/huffman_code.go:339-371 generate,
 * :183-309 bitCounts).  The level has no match finder and no history: blocks depend on each other only through the table in force
 * and the bit position, so the device works BY BLOCK — a plan kernel (histogram, candidate table, header; one wave per block), a
 * chain kernel (the stored / reuse / new-table decisions in order; one wave per input) and an emit kernel (one wave per block).
 * Options: kc_flate_wopts_default returns a new object at HuffmanOnly with the reference's values.
 * kc_flate_wopts_level: -2 (flate.HuffmanOnly) is the one level served; any other is KC_ERR_UNSUPPORTED (levels 0, 1 - 9 and the
 * custom windows have no device writer).  kc_flate_wopts_end: KC_FL_END_CLOSE (the default; Close, :865-880) or KC_FL_END_FLUSH
 * (Flush in Close's place, syncFlush :772-785: the stream ends with an empty stored block and stays open; gzip then has no trailer).
 * kc_flate_wopts_block(bytes, penalty): the two values compressor.init fixes per level (:787-827) — the window that becomes one
 * block (32768 at HuffmanOnly; 1 .. 65535) and logNewTablePenalty (10 at HuffmanOnly; 0 .. 31).  (65535, 8) reproduces the
 * reference's own goldens of writeBlockHuff (flate/testdata/huffman-*.golden).  KC_ERR_BAD_ARG outside these ranges. */
typedef struct kc_flate_wopts kc_flate_wopts;
enum { KC_FL_END_CLOSE = 0, KC_FL_END_FLUSH = 1 };
kc_flate_wopts* kc_flate_wopts_default(void);
void kc_flate_wopts_free(kc_flate_wopts* o);
kc_status kc_flate_wopts_level(kc_flate_wopts* o, int level);
kc_status kc_flate_wopts_end(kc_flate_wopts* o, int end);
kc_status kc_flate_wopts_block(kc_flate_wopts* o, uint32_t bytes, uint32_t penalty);
/* The most bytes one input of len bytes becomes at the given block size, in closed form (0: block outside 1 .. 65535); gzip adds
 * 18.  Per block its bytes and 176, and 8 for the stream's end.  Stored framing (5 bytes a block) is NOT the worst case: a Huffman
 * block is chosen against the reference's 560-bit GUESS of its header (:1009, :1036-1046), while a real header may reach
 * 17 + 19*3 + 258*7 = 1880 bits, and an EOB owed to the table before and the block's own add 30. */
uint64_t kc_flate_deflate_bound(uint64_t len, uint32_t block);
/* src: the inputs, concatenated; in_off: n + 1 ascending offsets; dst / dst_cap: the output; out_off[n + 1]: host array in both
 * forms.  The _dev forms take device pointers for src and dst.  Output: out_off is dense — input i owns dst[out_off[i],
 * out_off[i + 1]), its exact size.  An empty input is the ten-bit fixed block alone (:513-518).  KC_ERR_DST_TOO_SMALL when the
 * exact total is above dst_cap: nothing is written beyond dst_cap (the _dev forms: nothing at all, and out_off holds the layout —
 * out_off[n] is the capacity to come back with).  KC_ERR_UNSUPPORTED: an input above 1 GiB, or one whose block records alone
 * exceed the context's scratch budget.  The _dev forms cut a batch into groups of inputs whose block records fit the scratch budget
 * (about 2 KiB per block; a call of several groups plans each group twice).  The host-buffer forms stage groups of inputs whose bytes
 * and bound together stay within half of the budget; they do not use the rolling host pipeline. */
kc_status kc_flate_deflate_dev(kc_ctx* ctx, const kc_flate_wopts* o, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, uint8_t* d_dst,
                               uint64_t dst_cap, uint64_t* out_off);
kc_status kc_flate_deflate(kc_ctx* ctx, const kc_flate_wopts* o, const uint8_t* src, const uint64_t* in_off, uint32_t n, uint8_t* dst,
                           uint64_t dst_cap, uint64_t* out_off);
/* gzip.NewWriterLevel(w, gzip.HuffmanOnly); Write(input); Close() for every input (gzip/gzip.go:171-243 Write: the header, :264-290
 * Close: the trailer): the default Header only — 1f 8b 08 00, MTIME 0, XFL 0 at this level, OS 255 —, the stream as above, CRC-32
 * and the size modulo 2^32, little-endian.  With KC_FL_END_FLUSH (gzip.Writer.Flush, :245-262) the trailer is missing. */
kc_status kc_gzip_deflate_dev(kc_ctx* ctx, const kc_flate_wopts* o, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, uint8_t* d_dst,
                              uint64_t dst_cap, uint64_t* out_off);
kc_status kc_gzip_deflate(kc_ctx* ctx, const kc_flate_wopts* o, const uint8_t* src, const uint64_t* in_off, uint32_t n, uint8_t* dst,
                          uint64_t dst_cap, uint64_t* out_off);

/* ---- flate.StatelessDeflate / gzip.NewWriterLevel(w, gzip.StatelessCompression) over a batch of independent inputs ----
 * The output of every input is, byte for byte, what flate.StatelessDeflate(out, input, eof, dict) writes (flate/stateless.go:76-162;
 * statelessEnc :176-325; flate/token.go:212-309; flate/huffman_bit_writer.go:620-765 writeBlockDynamic, :824-975 writeTokens,
 * :987-1174 writeBlockHuff): the one LZ77 writer of the reference whose blocks are found independently of each other.  The input is
 * cut at fixed places — the first block 32767 - len(dict) bytes, every later one 24575 behind 8192 bytes of history that are the
 * input's own — and every block has a fresh 8192-entry table, so the device works BY BLOCK: match (one wave per block, the table in
 * LDS, tokens to scratch), plan (one wave per block: the block's tables, header and sizes), chain (one wave per input: stored /
 * fixed / reuse / new table, the owed EOBs, in the reference's order) and emit (one wave per block).  The bit writer is the
 * reference's pooled one, so logNewTablePenalty is 0: the estimate of a new table is doubled (:665, :1042).  tokens.EstimatedBits is
 * float32 arithmetic; the value reproduced is that of the reference's default amd64 build (nothing fused).  This is not a level of
 * flate.NewWriter in the reference either: kc_flate_wopts_level keeps refusing everything but -2.
 * Options: kc_flate_swopts_default returns a new object with eof = 1 and no dictionary.  kc_flate_swopts_eof(0): the non-eof call —
 * the stream ends with an empty stored block and stays open (one Write of flate.NewStatelessWriter).  kc_flate_swopts_dict: one
 * dictionary for the whole call, copied; only its last 8192 bytes count, as in the reference (:93-95). */
typedef struct kc_flate_swopts kc_flate_swopts;
kc_flate_swopts* kc_flate_swopts_default(void);
void kc_flate_swopts_free(kc_flate_swopts* o);
kc_status kc_flate_swopts_eof(kc_flate_swopts* o, int eof);
kc_status kc_flate_swopts_dict(kc_flate_swopts* o, const uint8_t* dict, uint64_t len);
/* The most bytes one input of len bytes becomes behind a dictionary of dict_len bytes, in closed form; gzip adds 20 (header 10,
 * trailer 8, the two bytes of Close's eof call).  Per block its bytes and 176, and 8 for the stream's end.  A block without a match
 * is stored (5 bytes and an owed EOB).  A dynamic, reused-table or fixed block is never taken where stored is not larger:
 * writeBlockDynamic compares exact sizes with the stored size before it writes (:731, :745; under a table in force :684, :698, where
 * the size is the estimate newSize when a new table wins — then nothing is written there but a fixed block that is below it, and
 * the exact comparison at :745 follows).  kc_last_timings after a call: match_ms the match kernel, prep_ms plan, other_ms chain,
 * entropy_ms emit.  A Huffman-only block is writeBlockHuff's and inherits the 176
 * bytes of kc_flate_deflate_bound (its header is chosen against a 560-bit guess).  Blocks: 0 for an empty input, 1 up to
 * 32767 - min(dict_len, 8192) bytes, then one per 24575. */
uint64_t kc_flate_stateless_bound(uint64_t len, uint64_t dict_len);
/* Conventions as for kc_flate_deflate[_dev]: in_off[n + 1], a dense out_off, KC_ERR_DST_TOO_SMALL with the exact layout and (the
 * _dev forms) nothing written, KC_ERR_UNSUPPORTED for an input above 1 GiB or one whose scratch alone exceeds the budget.  The
 * scratch is about 2.5 KiB per block and FOUR bytes of tokens per input byte (with a dictionary 32 KiB per input more); the _dev
 * forms cut a batch into groups of inputs that fit the budget (a call of several groups runs match, plan and chain twice per
 * group).  An empty input with eof is the ten-bit fixed block alone (03 00); without eof the empty stored block (00 00 00 ff ff). */
kc_status kc_flate_stateless_deflate_dev(kc_ctx* ctx, const kc_flate_swopts* o, const uint8_t* d_src, const uint64_t* in_off, uint32_t n,
                                         uint8_t* d_dst, uint64_t dst_cap, uint64_t* out_off);
kc_status kc_flate_stateless_deflate(kc_ctx* ctx, const kc_flate_swopts* o, const uint8_t* src, const uint64_t* in_off, uint32_t n, uint8_t* dst,
                                     uint64_t dst_cap, uint64_t* out_off);
/* gzip.NewWriterLevel(w, gzip.StatelessCompression); Write(input); Close() for every input (gzip/gzip.go:171-235, :264-290): the
 * default header (1f 8b 08 00, MTIME 0, XFL 0, OS 255), one non-eof StatelessDeflate of the input — its blocks and 00 00 ff ff from the
 * next byte —, Close's eof call on nothing (the ten-bit fixed block, 03 00), CRC-32 and the size modulo 2^32.  eof and the dictionary
 * of the options do not apply: the reference's gzip writer passes false and nil. */
kc_status kc_gzip_stateless_deflate_dev(kc_ctx* ctx, const kc_flate_swopts* o, const uint8_t* d_src, const uint64_t* in_off, uint32_t n,
                                        uint8_t* d_dst, uint64_t dst_cap, uint64_t* out_off);
kc_status kc_gzip_stateless_deflate(kc_ctx* ctx, const kc_flate_swopts* o, const uint8_t* src, const uint64_t* in_off, uint32_t n, uint8_t* dst,
                                    uint64_t dst_cap, uint64_t* out_off);

/* Single-block form with the WriterCustomEncoder contract (s2/writer.go:1053-1064): no varint header;
 * returns bytes used, 0 = incompressible (store raw), <0 = fall back to the built-in encoder.
 * "The function should expect to be called concurrently" (writer.go:1058; s2.Writer calls it from one goroutine per block,
 * writer.go:455-460): this entry point — and only this one — is safe to call from any number of host threads on ONE
 * context.  Concurrent callers are micro-batched: the blocks that arrive while the previous batch is on the device share
 * one H2D copy, one kernel launch and one D2H copy (pinned staging; KC_S2_HOOK_WAIT_US adds an optional collection window,
 * KC_S2_HOOK_BATCH caps the blocks per launch, default 256).  A context serving this hook must not be used for other calls
 * at the same time.
 * Host first (round 6): one block through the device takes ~3 ms (copy in, one wave on one CU, copy out) where the reference's own
 * encoder takes ~0.1 ms on a host core, so a caller the host could serve is never faster here (measured: 23 MB/s per lone caller,
 * 669 MB/s at 64 callers against ~600 MB/s per core for the built-in encoder; profiles/r04_hook_bench_final.json).  The hook
 * therefore answers -1 ("use the built-in encoder", writer.go:455-460) while fewer callers than the host has hardware threads are
 * busy encoding on the host — it books every caller it sends back as busy until that thread calls again, or for the time a slow core
 * needs for the block (len / 500 MB/s) — and takes only the overflow: callers that arrive while every hardware thread is booked.
 * Wiring the hook is so never slower than not wiring it (tools/hook_bench.cpp, profiles/r06_hook_bench.json: within 4 % of the
 * built-in encoder at 1 / 4 / 16 / 64 callers; forced to the device 23 / 92 / 265 / 630 MB/s against 1 250 / 4 970 / 19 400 /
 * 60 000).  KC_OPT_S2_HOOK_HOST_FIRST: the number of callers left to the host (default: its hardware threads), 0 = every caller to
 * the device (what the parity tests and a host without spare CPUs want). */
int64_t kc_s2_encode_block(kc_ctx* ctx, uint8_t* dst, uint64_t dst_cap, const uint8_t* src, uint64_t src_len);
/* hook diagnostics: calls served and device batches run on this context so far */
void kc_s2_hook_stats(const kc_ctx* ctx, uint64_t* calls, uint64_t* batches);
/* calls the hook answered -1 by the host-first rule (left to the caller's built-in encoder) */
uint64_t kc_s2_hook_declined(const kc_ctx* ctx);

/* ---- timing of the last call (HIP events recorded on the launch stream) ---- */
typedef struct {
    float total_ms;   /* all kernels of the last encode call */
    float match_ms;   /* match-finder kernel(s) */
    float entropy_ms; /* histogram + table build + bitstream emit kernel(s) */
    float other_ms;   /* checksum, scan, compaction */
    uint32_t redo_units; /* units re-run because a speculated block verdict was wrong */
    float prep_ms;    /* part of match_ms: zeroing / dictionary-priming of the per-unit hash tables before the match finder */
} kc_timings;
kc_status kc_last_timings(const kc_ctx* ctx, kc_timings* t);

/* ---- probes (measurement only; nothing on the encode path calls them) ----
 * kc_probe_table_pattern: the match finders' hash-table traffic on THIS device — scattered 4-byte accesses into n_tables tables of
 * table_bytes each (8 lanes per table, 8 tables per wave, two independent accesses per lane per iteration: the two buckets a
 * fastEncoder step looks up and overwrites, zstd/enc_fast.go:147-207).  out3[0] = read + write-back pairs per second, out3[1] = plain
 * reads per second, out3[2] = plain stores per second (each counts one request per access).  bench.py prices the match finder's
 * measured transactions per unit at these rates (roofline.floor).  Allocates and frees n_tables * table_bytes of device memory.
 * kc_probe_pcie: one pinned copy of `bytes` each way.  out7[0] H2D GB/s, [1] D2H GB/s, [2] / [3] H2D / D2H GB/s with both in flight,
 * [4] pageable -> pinned host copy GB/s with the context's copy threads (KC_OPT_HOST_COPY_THREADS), [5] pinned -> pageable, [6] the
 * thread count: the ceilings of the host-buffer entry points (bench.py end_to_end.pcie_ceiling). */
kc_status kc_probe_table_pattern(kc_ctx* ctx, uint32_t n_tables, uint32_t table_bytes, uint32_t waves, uint32_t iters, double* out3);
kc_status kc_probe_pcie(kc_ctx* ctx, uint64_t bytes, double* out7);

/* ---- synthetic corpora: deterministic, per-unit seeded, host-side generator ----
 * kind: 'T' enwik-style text, 'H' high-entropy, 'J' JSON records, 'M' mixed.  Fills
 * n_units * unit_size bytes at dst (host memory) using `threads` host threads. */
kc_status kc_corpus_fill(int kind, uint64_t seed, uint64_t first_unit, uint32_t n_units, uint32_t unit_size, uint8_t* dst, int threads);

#ifdef __cplusplus
}
#endif
#endif /* KCGPU_H */
