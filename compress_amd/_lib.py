"""ctypes binding of include/kcgpu.h (libkcgpu.so).  Fails loudly when the library is missing."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# KC_LIB_TAG=<tag>: a measurement build of the same sources with other compile-time constants (compress_amd/build.py, KC_BUILD_TAG)
_SO = os.path.join(_HERE, "libkcgpu%s.so" % ("_" + os.environ["KC_LIB_TAG"] if os.environ.get("KC_LIB_TAG") else ""))

KC_OK = 0
# per-input status classes of zstd.Decoder.DecodeAll (include/kcgpu.h KC_ZD_*)
ZD_NAMES = {0: "KC_ZD_OK", 1: "KC_ZD_MAGIC", 2: "KC_ZD_EOF", 3: "KC_ZD_UNKNOWN_DICT", 4: "KC_ZD_WINDOW_EXCEEDED", 5: "KC_ZD_SIZE_EXCEEDED",
            6: "KC_ZD_CRC", 7: "KC_ZD_CORRUPT"}
# per-input status classes of s2.Reader / s2.Decode (include/kcgpu.h KC_S2D_*)
S2D_NAMES = {0: "KC_S2D_OK", 1: "KC_S2D_CORRUPT", 2: "KC_S2D_CRC", 3: "KC_S2D_UNSUPPORTED", 4: "KC_S2D_SIZE_EXCEEDED", 5: "KC_S2D_EOF",
             6: "KC_S2D_UNEXPECTED_EOF", 7: "KC_S2D_CALLBACK"}
KC_ERR_BAD_ARG, KC_ERR_DST_TOO_SMALL, KC_ERR_HIP, KC_ERR_UNSUPPORTED, KC_ERR_NO_DEVICE, KC_ERR_INTERNAL = -1, -2, -3, -4, -5, -6
_NAMES = {0: "KC_OK", -1: "KC_ERR_BAD_ARG", -2: "KC_ERR_DST_TOO_SMALL", -3: "KC_ERR_HIP", -4: "KC_ERR_UNSUPPORTED",
          -5: "KC_ERR_NO_DEVICE", -6: "KC_ERR_INTERNAL"}


class KcError(RuntimeError):
    def __init__(self, status, msg=""):
        self.status = status
        super().__init__("%s%s" % (_NAMES.get(status, str(status)), (": " + msg) if msg else ""))


class ZstdOpts(C.Structure):
    _fields_ = [
        ("level", C.c_int32), ("window_size", C.c_int32), ("block_size", C.c_int32), ("crc", C.c_int32),
        ("single", C.c_int32), ("full_zero", C.c_int32), ("no_entropy", C.c_int32), ("all_lit_entropy", C.c_int32),
        ("low_mem", C.c_int32), ("custom_window", C.c_int32), ("custom_block", C.c_int32), ("custom_alent", C.c_int32),
        ("dict_id", C.c_uint32), ("dict", C.c_void_p), ("dict_len", C.c_uint64),
        ("dict_offsets", C.c_uint32 * 3), ("dict_huf_len", C.c_int32), ("dict_huf_log", C.c_int32),
        ("dict_huf_val", C.c_uint16 * 256), ("dict_huf_nbits", C.c_uint8 * 256), ("concurrent", C.c_int32),
    ]


class Timings(C.Structure):
    _fields_ = [("total_ms", C.c_float), ("match_ms", C.c_float), ("entropy_ms", C.c_float), ("other_ms", C.c_float),
                ("redo_units", C.c_uint32), ("prep_ms", C.c_float)]


# every symbol include/kcgpu.h declares (checked by tests/test_abi.py)
SYMBOLS = [
    "kc_zstd_opts_default", "kc_zstd_opts_level", "kc_zstd_opts_window", "kc_zstd_opts_crc", "kc_zstd_opts_zero_frames",
    "kc_zstd_opts_no_entropy", "kc_zstd_opts_all_lit_entropy", "kc_zstd_opts_single_segment", "kc_zstd_opts_concurrency", "kc_zstd_opts_dict_raw", "kc_zstd_opts_dict",
    "kc_zstd_max_encoded_size", "kc_ctx_create", "kc_ctx_destroy", "kc_last_error", "kc_device_info",
    "kc_zstd_encode_units", "kc_zstd_encode_units_dev", "kc_zstd_encode_streams_dev", "kc_zstd_encode_streams", "kc_zstd_encode_streams_cuts_dev", "kc_zstd_encode_streams_cuts", "kc_zstd_encode_units_submit", "kc_s2_encode_blocks_lvl_submit", "kc_wait", "kc_zstd_plan_stream_blocks", "kc_zstd_encode_units_dev_begin", "kc_zstd_encode_units_dev_end", "kc_zstd_encode_units_dev_end_at", "kc_ctx_chain_after", "kc_xxh64_units_dev", "kc_zstd_debug_parse_dev",
    "kc_s2_max_encoded_len", "kc_s2_encode_blocks", "kc_s2_encode_blocks_dev", "kc_s2_encode_stream_dev", "kc_s2_decode_blocks_dev", "kc_zstd_decode_units_dev", "kc_zstd_decode_units_dict_dev", "kc_s2_encode_block", "kc_s2_hook_stats", "kc_s2_encode_blocks_lvl", "kc_s2_encode_blocks_lvl_dev", "kc_s2_encode_blocks_lvl_dev_begin", "kc_s2_encode_blocks_lvl_dev_end_at", "kc_s2_encode_stream_lvl_dev",
    "kc_last_timings", "kc_corpus_fill", "kc_ctx_set_option", "kc_ctx_get_option", "kc_zstd_encode_jobs", "kc_zstd_job_size", "kc_zstd_overlap_size",
    "kc_zstd_dopts_default", "kc_zstd_dopts_free", "kc_zstd_dopts_max_memory", "kc_zstd_dopts_max_window", "kc_zstd_dopts_ignore_checksum", "kc_zstd_dopts_dict", "kc_zstd_dopts_dict_raw",
    "kc_zstd_decode_all_dev", "kc_zstd_decode_all", "kc_zstd_decode_all_bound_dev", "kc_zstd_decode_all_bound",
    "kc_zstd_dstream_new", "kc_zstd_dstream_feed", "kc_zstd_dstream_reset", "kc_zstd_dstream_free",
    "kc_s2_ropts_default", "kc_s2_ropts_free", "kc_s2_ropts_max_block_size", "kc_s2_ropts_ignore_crc", "kc_s2_ropts_ignore_stream_identifier",
    "kc_s2_decode_streams_dev", "kc_s2_decode_streams", "kc_s2_decode_streams_bound_dev", "kc_s2_decode_streams_bound",
    "kc_s2_decode_blocks_all_dev", "kc_s2_decode_blocks_all", "kc_s2_decode_blocks_all_bound_dev", "kc_s2_decode_blocks_all_bound",
    "kc_s2_index_new", "kc_s2_index_free", "kc_s2_index_load", "kc_s2_index_load_stream", "kc_s2_index_find", "kc_s2_index_total_uncompressed",
    "kc_s2_index_total_compressed", "kc_s2_index_est_block_uncompressed", "kc_s2_index_entries", "kc_s2_index_stream",
    "kc_s2_read_ranges_dev", "kc_s2_read_ranges",
    "kc_s2_rstream_new", "kc_s2_rstream_feed", "kc_s2_rstream_skip", "kc_s2_rstream_skip_left", "kc_s2_rstream_on_skippable", "kc_s2_rstream_reset",
    "kc_s2_rstream_free",
    "kc_flate_ropts_default", "kc_flate_ropts_free", "kc_flate_ropts_dict", "kc_flate_ropts_multistream",
    "kc_flate_inflate_dev", "kc_flate_inflate", "kc_flate_inflate_bound_dev", "kc_flate_inflate_bound",
    "kc_gzip_inflate_dev", "kc_gzip_inflate", "kc_gzip_inflate_bound_dev", "kc_gzip_inflate_bound",
    "kc_zlib_inflate_dev", "kc_zlib_inflate", "kc_zlib_inflate_bound_dev", "kc_zlib_inflate_bound",
    "kc_zip_dir_load", "kc_zip_dir_free", "kc_zip_dir_count", "kc_zip_dir_base_offset", "kc_zip_dir_comment", "kc_zip_dir_entry", "kc_zip_dir_members",
    "kc_zip_read_dev", "kc_zip_read", "kc_zip_read_bound",
    "kc_flate_wopts_default", "kc_flate_wopts_free", "kc_flate_wopts_level", "kc_flate_wopts_end", "kc_flate_wopts_block",
    "kc_flate_deflate_bound", "kc_flate_deflate_dev", "kc_flate_deflate", "kc_gzip_deflate_dev", "kc_gzip_deflate",
    "kc_flate_swopts_default", "kc_flate_swopts_free", "kc_flate_swopts_eof", "kc_flate_swopts_dict", "kc_flate_stateless_bound",
    "kc_flate_stateless_deflate_dev", "kc_flate_stateless_deflate", "kc_gzip_stateless_deflate_dev", "kc_gzip_stateless_deflate",
    "kc_probe_table_pattern", "kc_probe_pcie", "kc_ctx_trim", "kc_device_trim", "kc_s2_hook_declined", "kc_create_error", "kc_host_alloc", "kc_host_free",
]

# kc_option / KC_PATH_* (include/kcgpu.h)
PATH_AUTO, PATH_HBM, PATH_LDS = 0, 1, 2
OPT_MATCH_PATH, OPT_ZFAST_LDS_MAX_UNITS, OPT_S2_LDS_MAX_BLOCKS, OPT_SPEC_W0, OPT_SPEC_GROW, OPT_LDS_SPEC_W0 = 1, 2, 3, 4, 5, 6
OPT_HOST_SERIAL, OPT_HOST_PIPE_MIB, OPT_HOST_OVERLAP_MIN_MIB, OPT_HOST_COPY_THREADS, OPT_HOST_TRACE, OPT_HOST_CHUNK_MIB = 7, 8, 9, 10, 11, 12
OPT_K2_PROF, OPT_S2_HOOK_WAIT_US, OPT_S2_HOOK_BATCH, OPT_TEST_FEED_REDO, OPT_S2_LDS_SPEC_W0, OPT_MAX_SCRATCH_MIB, OPT_LAST_PATH, OPT_LAST_BATCHES = 13, 14, 15, 16, 17, 18, 100, 101
OPT_JOB_PRIME = 30
OPT_STAGE2_STREAM = 31
OPT_HOST_CHUNK_MIB_APPEND = 32
OPT_HOST_ROLL, OPT_HOST_ROLL_MIB = 33, 34
OPT_S2_HOOK_HOST_FIRST = 35
OPT_DSTREAM_BLOCKS = 36
OPT_S2_RSTREAM_CHUNKS = 37
# kc_s2_skippable_fn: int fn(void* user, uint8_t id, const uint8_t* piece, uint64_t n, uint64_t left)
S2_SKIPPABLE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint8, C.POINTER(C.c_uint8), C.c_uint64, C.c_uint64)
_PATHS = {"auto": PATH_AUTO, "hbm": PATH_HBM, "lds": PATH_LDS, None: PATH_AUTO}

_lib = None


def declare_s2_index(L):
    """ctypes signatures of the kc_s2_index_* functions (plain host code: any library that exports them)."""
    vp, u64, i64 = C.c_void_p, C.c_uint64, C.c_int64
    L.kc_s2_index_new.argtypes = []
    L.kc_s2_index_new.restype = vp
    L.kc_s2_index_free.argtypes = [vp]
    L.kc_s2_index_free.restype = None
    L.kc_s2_index_load.argtypes = [vp, vp, u64, C.POINTER(u64)]
    L.kc_s2_index_load.restype = C.c_int
    L.kc_s2_index_load_stream.argtypes = [vp, vp, u64]
    L.kc_s2_index_load_stream.restype = C.c_int
    L.kc_s2_index_find.argtypes = [vp, i64, C.POINTER(i64), C.POINTER(i64)]
    L.kc_s2_index_find.restype = C.c_int
    for n in ("total_uncompressed", "total_compressed", "est_block_uncompressed"):
        f = getattr(L, "kc_s2_index_" + n)
        f.argtypes = [vp]
        f.restype = i64
    L.kc_s2_index_entries.argtypes = [vp, vp, vp, C.c_uint32]
    L.kc_s2_index_entries.restype = C.c_uint32
    L.kc_s2_index_stream.argtypes = [vp, u64, vp, u64, C.POINTER(u64), C.POINTER(C.c_uint32)]
    L.kc_s2_index_stream.restype = C.c_int


class ZipEntry(C.Structure):
    """kc_zip_entry (include/kcgpu.h): zip.FileHeader's directory fields; name, comment and extra point into the archive buffer."""
    _fields_ = [("name", C.c_void_p), ("comment", C.c_void_p), ("extra", C.c_void_p), ("name_len", C.c_uint32), ("comment_len", C.c_uint32),
                ("extra_len", C.c_uint32), ("non_utf8", C.c_uint32), ("creator_version", C.c_uint16), ("reader_version", C.c_uint16),
                ("flags", C.c_uint16), ("method", C.c_uint16), ("modified_time", C.c_uint16), ("modified_date", C.c_uint16), ("crc32", C.c_uint32),
                ("compressed_size64", C.c_uint64), ("uncompressed_size64", C.c_uint64), ("header_offset", C.c_int64),
                ("external_attrs", C.c_uint32), ("reserved", C.c_uint32)]


class ZipMember(C.Structure):
    """kc_zip_member (include/kcgpu.h): one row of the member table of kc_zip_read."""
    _fields_ = [("header_offset", C.c_int64), ("compressed_size", C.c_uint64), ("uncompressed_size", C.c_uint64), ("crc32", C.c_uint32),
                ("method", C.c_uint16), ("flags", C.c_uint16), ("is_dir", C.c_uint32), ("reserved", C.c_uint32)]


def declare_zip_dir(L):
    """ctypes signatures of the kc_zip_dir_* functions (plain host code: any library that exports them)."""
    vp, u64 = C.c_void_p, C.c_uint64
    L.kc_zip_dir_load.argtypes = [vp, u64, C.POINTER(vp)]
    L.kc_zip_dir_load.restype = C.c_int
    L.kc_zip_dir_free.argtypes = [vp]
    L.kc_zip_dir_free.restype = None
    L.kc_zip_dir_count.argtypes = [vp]
    L.kc_zip_dir_count.restype = u64
    L.kc_zip_dir_base_offset.argtypes = [vp]
    L.kc_zip_dir_base_offset.restype = C.c_int64
    L.kc_zip_dir_comment.argtypes = [vp, C.POINTER(C.c_uint32)]
    L.kc_zip_dir_comment.restype = vp
    L.kc_zip_dir_entry.argtypes = [vp, u64, C.POINTER(ZipEntry)]
    L.kc_zip_dir_entry.restype = C.c_int
    L.kc_zip_dir_members.argtypes = [vp, u64, u64, vp]
    L.kc_zip_dir_members.restype = C.c_int
    return L


def lib_path():
    return _SO


def load():
    """Load libkcgpu.so; raises if it has not been built (python -m compress_amd.build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_SO):
        raise KcError(KC_ERR_NO_DEVICE, "libkcgpu.so not built: run `python -m compress_amd.build` (no CPU fallback exists)")
    # One HIP runtime per process: when PyTorch is present it must be imported first so that
    # libkcgpu.so binds to the libamdhip64.so.7 PyTorch already mapped (device pointers and
    # streams are then shareable); without PyTorch the system ROCm runtime is used.
    if os.environ.get("KC_NO_TORCH_PRELOAD") != "1":
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    L = C.CDLL(_SO)
    vp, u64 = C.c_void_p, C.c_uint64
    po = C.POINTER(ZstdOpts)
    L.kc_zstd_opts_default.argtypes = [po]
    L.kc_zstd_opts_default.restype = None
    for n in ("level", "window", "crc", "zero_frames", "no_entropy", "all_lit_entropy", "single_segment", "concurrency"):
        f = getattr(L, "kc_zstd_opts_" + n)
        f.argtypes = [po, C.c_int]
        f.restype = C.c_int
    L.kc_zstd_opts_dict_raw.argtypes = [po, C.c_uint32, vp, u64]
    L.kc_zstd_opts_dict_raw.restype = C.c_int
    L.kc_zstd_opts_dict.argtypes = [po, vp, u64]
    L.kc_zstd_opts_dict.restype = C.c_int
    L.kc_zstd_max_encoded_size.argtypes = [po, C.c_int64]
    L.kc_zstd_max_encoded_size.restype = C.c_int64
    L.kc_ctx_create.argtypes = [C.POINTER(vp), C.c_int, vp]
    L.kc_ctx_create.restype = C.c_int
    L.kc_ctx_destroy.argtypes = [vp]
    L.kc_ctx_destroy.restype = None
    L.kc_last_error.argtypes = [vp]
    L.kc_last_error.restype = C.c_char_p
    L.kc_device_info.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_char_p, C.c_size_t]
    L.kc_device_info.restype = C.c_int
    for n in ("kc_zstd_encode_units", "kc_zstd_encode_units_dev", "kc_zstd_encode_streams_dev", "kc_zstd_encode_streams"):
        f = getattr(L, n)
        f.argtypes = [vp, po, vp, vp, C.c_uint32, vp, u64, vp]
        f.restype = C.c_int
    L.kc_zstd_encode_units_submit.argtypes = [vp, po, vp, vp, C.c_uint32, vp, u64, vp]
    L.kc_zstd_encode_units_submit.restype = C.c_int
    L.kc_s2_encode_blocks_lvl_submit.argtypes = [vp, C.c_int, vp, vp, C.c_uint32, vp, u64, vp]
    L.kc_s2_encode_blocks_lvl_submit.restype = C.c_int
    L.kc_zstd_plan_stream_blocks.argtypes = [C.c_int32, u64, vp, u64, vp, u64, vp]
    L.kc_zstd_plan_stream_blocks.restype = C.c_int64
    L.kc_wait.argtypes = [vp]
    L.kc_wait.restype = C.c_int
    for n in ("kc_zstd_encode_streams_cuts_dev", "kc_zstd_encode_streams_cuts"):
        f = getattr(L, n)
        f.argtypes = [vp, po, vp, vp, C.c_uint32, vp, vp, vp, u64, vp]
        f.restype = C.c_int
    L.kc_zstd_encode_units_dev_begin.argtypes = [vp, po, vp, vp, C.c_uint32, vp, u64]
    L.kc_zstd_encode_units_dev_begin.restype = C.c_int
    L.kc_zstd_encode_units_dev_end.argtypes = [vp, vp]
    L.kc_zstd_encode_units_dev_end.restype = C.c_int
    L.kc_zstd_encode_units_dev_end_at.argtypes = [vp, vp, C.c_uint64, vp]
    L.kc_s2_encode_blocks_lvl_dev_begin.argtypes = [vp, C.c_int, vp, vp, C.c_uint32]
    L.kc_s2_encode_blocks_lvl_dev_begin.restype = C.c_int
    L.kc_s2_encode_blocks_lvl_dev_end_at.argtypes = [vp, vp, C.c_uint64, vp]
    L.kc_s2_encode_blocks_lvl_dev_end_at.restype = C.c_int
    L.kc_zstd_encode_units_dev_end_at.restype = C.c_int
    L.kc_ctx_chain_after.argtypes = [vp, vp]
    L.kc_ctx_chain_after.restype = None
    L.kc_xxh64_units_dev.argtypes = [vp, vp, vp, C.c_uint32, vp]
    L.kc_xxh64_units_dev.restype = C.c_int
    L.kc_zstd_debug_parse_dev.argtypes = [vp, po, vp, vp, C.c_uint32, vp, u64, vp, vp, vp, C.c_uint32, C.POINTER(C.c_uint32)]
    L.kc_zstd_debug_parse_dev.restype = C.c_int
    L.kc_s2_max_encoded_len.argtypes = [C.c_int64]
    L.kc_s2_max_encoded_len.restype = C.c_int64
    for n in ("kc_s2_encode_blocks", "kc_s2_encode_blocks_dev"):
        f = getattr(L, n)
        f.argtypes = [vp, vp, vp, C.c_uint32, vp, u64, vp]
        f.restype = C.c_int
    for n in ("kc_s2_encode_blocks_lvl", "kc_s2_encode_blocks_lvl_dev"):
        f = getattr(L, n)
        f.argtypes = [vp, C.c_int, vp, vp, C.c_uint32, vp, u64, vp]
        f.restype = C.c_int
    L.kc_s2_encode_stream_lvl_dev.argtypes = [vp, C.c_int, vp, vp, C.c_uint32, vp, u64, vp, C.c_int]
    L.kc_s2_encode_stream_lvl_dev.restype = C.c_int
    L.kc_s2_encode_stream_dev.argtypes = [vp, vp, vp, C.c_uint32, vp, u64, vp, C.c_int]
    L.kc_s2_encode_stream_dev.restype = C.c_int
    L.kc_zstd_decode_units_dev.argtypes = [vp, vp, vp, C.c_uint32, vp, vp, vp]
    L.kc_zstd_decode_units_dev.restype = C.c_int
    L.kc_zstd_decode_units_dict_dev.argtypes = [vp, vp, vp, C.c_uint32, vp, vp, vp, vp, u64]
    L.kc_zstd_decode_units_dict_dev.restype = C.c_int
    L.kc_s2_decode_blocks_dev.argtypes = [vp, vp, vp, C.c_uint32, vp, vp, vp]
    L.kc_zstd_dopts_default.argtypes = []
    L.kc_zstd_dopts_default.restype = vp
    L.kc_zstd_dopts_free.argtypes = [vp]
    L.kc_zstd_dopts_free.restype = None
    for n in ("max_memory", "max_window"):
        f = getattr(L, "kc_zstd_dopts_" + n)
        f.argtypes = [vp, u64]
        f.restype = C.c_int
    L.kc_zstd_dopts_ignore_checksum.argtypes = [vp, C.c_int]
    L.kc_zstd_dopts_ignore_checksum.restype = C.c_int
    L.kc_zstd_dopts_dict.argtypes = [vp, vp, u64]
    L.kc_zstd_dopts_dict.restype = C.c_int
    L.kc_zstd_dopts_dict_raw.argtypes = [vp, C.c_uint32, vp, u64]
    L.kc_zstd_dopts_dict_raw.restype = C.c_int
    for n in ("kc_zstd_decode_all_dev", "kc_zstd_decode_all"):
        f = getattr(L, n)
        f.argtypes = [vp, vp, vp, vp, C.c_uint32, vp, u64, vp, vp]
        f.restype = C.c_int
    for n in ("kc_zstd_decode_all_bound_dev", "kc_zstd_decode_all_bound"):
        f = getattr(L, n)
        f.argtypes = [vp, vp, vp, vp, C.c_uint32, vp, vp]
        f.restype = C.c_int
    L.kc_s2_decode_blocks_dev.restype = C.c_int
    L.kc_zstd_dstream_new.argtypes = [vp, vp]
    L.kc_zstd_dstream_new.restype = vp
    L.kc_zstd_dstream_feed.argtypes = [vp, vp, u64, C.c_int, vp, u64, C.POINTER(u64), C.POINTER(u64), C.POINTER(C.c_uint32)]
    L.kc_zstd_dstream_feed.restype = C.c_int
    L.kc_zstd_dstream_reset.argtypes = [vp]
    L.kc_zstd_dstream_reset.restype = C.c_int
    L.kc_zstd_dstream_free.argtypes = [vp]
    L.kc_zstd_dstream_free.restype = None
    L.kc_s2_ropts_default.argtypes = []
    L.kc_s2_ropts_default.restype = vp
    L.kc_s2_ropts_free.argtypes = [vp]
    L.kc_s2_ropts_free.restype = None
    L.kc_s2_ropts_max_block_size.argtypes = [vp, C.c_int64]
    L.kc_s2_ropts_max_block_size.restype = C.c_int
    for n in ("ignore_crc", "ignore_stream_identifier"):
        f = getattr(L, "kc_s2_ropts_" + n)
        f.argtypes = [vp, C.c_int]
        f.restype = C.c_int
    for n in ("kc_s2_decode_streams_dev", "kc_s2_decode_streams"):
        f = getattr(L, n)
        f.argtypes = [vp, vp, vp, vp, C.c_uint32, vp, u64, vp, vp]
        f.restype = C.c_int
    for n in ("kc_s2_decode_streams_bound_dev", "kc_s2_decode_streams_bound"):
        f = getattr(L, n)
        f.argtypes = [vp, vp, vp, vp, C.c_uint32, vp, vp]
        f.restype = C.c_int
    for n in ("kc_s2_decode_blocks_all_dev", "kc_s2_decode_blocks_all"):
        f = getattr(L, n)
        f.argtypes = [vp, vp, vp, C.c_uint32, vp, u64, vp, vp]
        f.restype = C.c_int
    for n in ("kc_s2_decode_blocks_all_bound_dev", "kc_s2_decode_blocks_all_bound"):
        f = getattr(L, n)
        f.argtypes = [vp, vp, vp, C.c_uint32, vp, vp]
        f.restype = C.c_int
    declare_s2_index(L)
    for n in ("kc_s2_read_ranges_dev", "kc_s2_read_ranges"):
        f = getattr(L, n)
        f.argtypes = [vp, vp, vp, vp, C.c_uint32, vp, vp, vp, vp, C.c_uint32, vp, u64, vp, vp, vp]
        f.restype = C.c_int
    L.kc_s2_rstream_new.argtypes = [vp, vp]
    L.kc_s2_rstream_new.restype = vp
    L.kc_s2_rstream_feed.argtypes = [vp, vp, u64, C.c_int, vp, u64, C.POINTER(u64), C.POINTER(u64), C.POINTER(C.c_uint32)]
    L.kc_s2_rstream_feed.restype = C.c_int
    L.kc_s2_rstream_skip.argtypes = [vp, u64]
    L.kc_s2_rstream_skip.restype = C.c_int
    L.kc_s2_rstream_skip_left.argtypes = [vp]
    L.kc_s2_rstream_skip_left.restype = u64
    L.kc_s2_rstream_on_skippable.argtypes = [vp, C.c_uint8, S2_SKIPPABLE_FN, vp]
    L.kc_s2_rstream_on_skippable.restype = C.c_int
    L.kc_s2_rstream_reset.argtypes = [vp]
    L.kc_s2_rstream_reset.restype = C.c_int
    L.kc_s2_rstream_free.argtypes = [vp]
    L.kc_s2_rstream_free.restype = None
    L.kc_flate_ropts_default.argtypes = []
    L.kc_flate_ropts_default.restype = vp
    L.kc_flate_ropts_free.argtypes = [vp]
    L.kc_flate_ropts_free.restype = None
    L.kc_flate_ropts_dict.argtypes = [vp, vp, u64]
    L.kc_flate_ropts_dict.restype = C.c_int
    L.kc_flate_ropts_multistream.argtypes = [vp, C.c_int]
    L.kc_flate_ropts_multistream.restype = C.c_int
    for n in ("kc_flate_inflate_dev", "kc_flate_inflate", "kc_gzip_inflate_dev", "kc_gzip_inflate", "kc_zlib_inflate_dev", "kc_zlib_inflate"):
        f = getattr(L, n)
        f.argtypes = [vp, vp, vp, vp, C.c_uint32, vp, u64, vp, vp, vp]
        f.restype = C.c_int
    for n in ("kc_flate_inflate_bound_dev", "kc_flate_inflate_bound", "kc_gzip_inflate_bound_dev", "kc_gzip_inflate_bound",
              "kc_zlib_inflate_bound_dev", "kc_zlib_inflate_bound"):
        f = getattr(L, n)
        f.argtypes = [vp, vp, vp, vp, C.c_uint32, vp, vp, vp]
        f.restype = C.c_int
    declare_zip_dir(L)
    for n in ("kc_zip_read_dev", "kc_zip_read"):
        f = getattr(L, n)
        f.argtypes = [vp, vp, u64, vp, C.c_uint32, vp, u64, vp, vp]
        f.restype = C.c_int
    L.kc_zip_read_bound.argtypes = [vp, vp, u64, vp, C.c_uint32, vp, vp]
    L.kc_zip_read_bound.restype = C.c_int
    L.kc_flate_wopts_default.argtypes = []
    L.kc_flate_wopts_default.restype = vp
    L.kc_flate_wopts_free.argtypes = [vp]
    L.kc_flate_wopts_free.restype = None
    L.kc_flate_wopts_level.argtypes = [vp, C.c_int]
    L.kc_flate_wopts_level.restype = C.c_int
    L.kc_flate_wopts_end.argtypes = [vp, C.c_int]
    L.kc_flate_wopts_end.restype = C.c_int
    L.kc_flate_wopts_block.argtypes = [vp, C.c_uint32, C.c_uint32]
    L.kc_flate_wopts_block.restype = C.c_int
    L.kc_flate_deflate_bound.argtypes = [u64, C.c_uint32]
    L.kc_flate_deflate_bound.restype = u64
    for n in ("kc_flate_deflate_dev", "kc_flate_deflate", "kc_gzip_deflate_dev", "kc_gzip_deflate"):
        f = getattr(L, n)
        f.argtypes = [vp, vp, vp, vp, C.c_uint32, vp, u64, vp]
        f.restype = C.c_int
    L.kc_flate_swopts_default.argtypes = []
    L.kc_flate_swopts_default.restype = vp
    L.kc_flate_swopts_free.argtypes = [vp]
    L.kc_flate_swopts_free.restype = None
    L.kc_flate_swopts_eof.argtypes = [vp, C.c_int]
    L.kc_flate_swopts_eof.restype = C.c_int
    L.kc_flate_swopts_dict.argtypes = [vp, C.c_char_p, u64]
    L.kc_flate_swopts_dict.restype = C.c_int
    L.kc_flate_stateless_bound.argtypes = [u64, u64]
    L.kc_flate_stateless_bound.restype = u64
    for n in ("kc_flate_stateless_deflate_dev", "kc_flate_stateless_deflate", "kc_gzip_stateless_deflate_dev", "kc_gzip_stateless_deflate"):
        f = getattr(L, n)
        f.argtypes = [vp, vp, vp, vp, C.c_uint32, vp, u64, vp]
        f.restype = C.c_int
    L.kc_s2_encode_block.argtypes = [vp, vp, u64, vp, u64]
    L.kc_s2_encode_block.restype = C.c_int64
    L.kc_s2_hook_stats.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
    L.kc_s2_hook_stats.restype = None
    L.kc_last_timings.argtypes = [vp, C.POINTER(Timings)]
    L.kc_last_timings.restype = C.c_int
    L.kc_zstd_encode_jobs.argtypes = [vp, po, vp, u64, vp, u64, vp, u64, C.POINTER(u64)]
    L.kc_zstd_encode_jobs.restype = C.c_int
    L.kc_zstd_job_size.argtypes = [po]
    L.kc_zstd_job_size.restype = C.c_int64
    L.kc_zstd_overlap_size.argtypes = [po]
    L.kc_zstd_overlap_size.restype = C.c_int64
    L.kc_ctx_set_option.argtypes = [vp, C.c_int, C.c_int64]
    L.kc_ctx_set_option.restype = C.c_int
    L.kc_ctx_get_option.argtypes = [vp, C.c_int]
    L.kc_ctx_get_option.restype = C.c_int64
    L.kc_s2_hook_declined.argtypes = [vp]
    L.kc_s2_hook_declined.restype = C.c_uint64
    L.kc_host_alloc.argtypes = [C.POINTER(vp), u64]
    L.kc_host_alloc.restype = C.c_int
    L.kc_host_free.argtypes = [vp]
    L.kc_host_free.restype = None
    L.kc_create_error.argtypes = []
    L.kc_create_error.restype = C.c_char_p
    L.kc_ctx_trim.argtypes = [vp]
    L.kc_ctx_trim.restype = C.c_int
    L.kc_device_trim.argtypes = [C.c_int]
    L.kc_device_trim.restype = C.c_int
    L.kc_corpus_fill.argtypes = [C.c_int, u64, u64, C.c_uint32, C.c_uint32, vp, C.c_int]
    L.kc_corpus_fill.restype = C.c_int
    if hasattr(L, "kc_probe_pcie"):  # (the wave-emulator build of the library, tools/build_emu_lib.sh, leaves the device probes out)
        L.kc_probe_table_pattern.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_double)]
        L.kc_probe_table_pattern.restype = C.c_int
        L.kc_probe_pcie.argtypes = [vp, u64, C.POINTER(C.c_double)]
        L.kc_probe_pcie.restype = C.c_int
    _lib = L
    return L


class Context:
    """kc_ctx: device scratch + stream.  stream: an int hipStream_t handle (e.g. torch.cuda.current_stream().cuda_stream)."""

    def __init__(self, device=0, stream=None):
        self.L = load()
        h = C.c_void_p()
        st = self.L.kc_ctx_create(C.byref(h), device, C.c_void_p(stream) if stream else None)
        if st != KC_OK:
            why = self.L.kc_create_error().decode(errors="replace")
            raise KcError(st, "kc_ctx_create: %s (is a gfx950 GPU visible? there is no CPU fallback)" % (why or "no reason recorded"))
        self.h = h
        self._apply_env()

    # Measurement knobs: the library itself reads no environment variable (include/kcgpu.h); this harness maps the KC_* variables the
    # tools/ scripts set onto kc_ctx_set_option, once per context.
    _ENV_OPTS = (("KC_MATCH_PATH", 1), ("KC_ZFAST_LDS_MAX_UNITS", 2), ("KC_S2_LDS_MAX_BLOCKS", 3), ("KC_SPEC_W0", 4), ("KC_SPEC_GROW", 5),
                 ("KC_LDS_SPEC_W0", 6), ("KC_S2_LDS_SPEC_W0", 17), ("KC_HOST_PIPE_MIB", 8), ("KC_HOST_OVERLAP_MIN_MIB", 9),
                 ("KC_HOST_COPY_THREADS", 10), ("KC_S2_HOOK_WAIT_US", 14), ("KC_S2_HOOK_BATCH", 15), ("KC_S2_HOOK_LANES", 29),
                 ("KC_ZFAST_EPOCH", 22), ("KC_ZFAST_XSEG_K", 23), ("KC_FUSE_RAW_XXH", 24), ("KC_ZFAST_FILTER", 25), ("KC_XXH_FIN_MODE", 26),
                 ("KC_ZFAST_VARIANT", 27), ("KC_ZFAST_PRESCAN", 28), ("KC_ZFAST_FIRST_FILTER", 38), ("KC_JOB_PRIME", 30), ("KC_HOST_ROLL", 33), ("KC_HOST_ROLL_MIB", 34), ("KC_S2_HOOK_HOST_FIRST", 35), ("KC_BETTER_DICT_EPOCH", 21), ("KC_BEST_SLOTS", 19), ("KC_MAX_SCRATCH_MIB", 18))
    _ENV_FLAGS = (("KC_HOST_SERIAL", 7), ("KC_HOST_TRACE", 11), ("KC_K2_PROF", 13))  # set by their presence

    def _apply_env(self):
        for name, key in self._ENV_OPTS:
            v = os.environ.get(name)
            if v not in (None, ""):
                try:
                    self.set_option(key, int(v))
                except (ValueError, KcError) as e:  # say WHICH variable
                    raise ValueError("environment variable %s=%r is not a valid value of option %d: %s" % (name, v, key, e)) from None
        for name, key in self._ENV_FLAGS:
            if os.environ.get(name) not in (None, "", "0"):  # '0' and the empty string mean off
                self.set_option(key, 1)
        v = os.environ.get("KC_HOST_CHUNKS_MIB")
        if v:
            sizes = [int(x) for x in v.split(",") if x.strip()]
            self.set_option(OPT_HOST_CHUNK_MIB, sizes[0])
            for x in sizes[1:]:
                self.set_option(OPT_HOST_CHUNK_MIB_APPEND, x)

    def close(self):
        if getattr(self, "h", None):
            self.L.kc_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, st):
        if st != KC_OK:
            raise KcError(st, self.L.kc_last_error(self.h).decode(errors="replace"))

    def set_option(self, key, value):
        """kc_ctx_set_option (keys: OPT_* above)."""
        self.check(self.L.kc_ctx_set_option(self.h, int(key), int(value)))

    def get_option(self, key):
        return int(self.L.kc_ctx_get_option(self.h, int(key)))

    def set_path(self, path):
        """'auto' | 'hbm' | 'lds': which kernel family serves SpeedFastest / s2.Encode batches (KC_OPT_MATCH_PATH)."""
        self.set_option(OPT_MATCH_PATH, _PATHS[path] if not isinstance(path, int) else path)

    def last_path(self):
        return {PATH_HBM: "hbm", PATH_LDS: "lds"}.get(self.get_option(OPT_LAST_PATH), "none")

    def device_info(self):
        ncu, lds, clk = C.c_int32(), C.c_int32(), C.c_int32()
        name = C.create_string_buffer(128)
        self.check(self.L.kc_device_info(self.h, C.byref(ncu), C.byref(lds), C.byref(clk), name, 128))
        return {"n_cu": ncu.value, "lds_per_cu": lds.value, "clock_khz": clk.value, "arch": name.value.decode()}

    def probe_table_pattern(self, n_tables=32768, table_bytes=131072, waves=4096, iters=512):
        """kc_probe_table_pattern: requests per second of the match finders' table traffic on this device."""
        out = (C.c_double * 3)()
        self.check(self.L.kc_probe_table_pattern(self.h, n_tables, table_bytes, waves, iters, out))
        return {"pairs_per_s": out[0], "reads_per_s": out[1], "stores_per_s": out[2]}

    def probe_pcie(self, nbytes=1 << 30):
        """kc_probe_pcie: pinned H2D / D2H GB/s (alone, both at once) and the pageable <-> pinned host copy rates."""
        out = (C.c_double * 7)()
        self.check(self.L.kc_probe_pcie(self.h, nbytes, out))
        return {"h2d_GBps": out[0], "d2h_GBps": out[1], "h2d_bidir_GBps": out[2], "d2h_bidir_GBps": out[3],
                "host_copy_in_GBps": out[4], "host_copy_out_GBps": out[5], "copy_threads": int(out[6])}

    def trim(self):
        """kc_ctx_trim: free this context's device scratch (it grows back with the next call)."""
        self.check(self.L.kc_ctx_trim(self.h))

    def timings(self):
        t = Timings()
        self.check(self.L.kc_last_timings(self.h, C.byref(t)))
        return {"total_ms": t.total_ms, "match_ms": t.match_ms, "entropy_ms": t.entropy_ms, "other_ms": t.other_ms,
                "redo_units": t.redo_units, "prep_ms": t.prep_ms}


class PinnedBuffer:
    """kc_host_alloc: page-locked host memory as a numpy uint8 array (`.a`); the host-buffer entry points DMA straight from / into it."""

    def __init__(self, nbytes):
        import numpy as np
        self.L = load()
        p = C.c_void_p()
        st = self.L.kc_host_alloc(C.byref(p), int(nbytes))
        if st != KC_OK:
            raise KcError(st, "kc_host_alloc(%d)" % nbytes)
        self.p = p
        self.a = np.ctypeslib.as_array((C.c_uint8 * int(nbytes)).from_address(p.value))

    def free(self):
        if getattr(self, "p", None):
            self.a = None
            self.L.kc_host_free(self.p)
            self.p = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def device_trim(device=0):
    """kc_device_trim: free what the device's rolling host pipeline holds (slots + lane scratch); raises while calls are in flight."""
    st = load().kc_device_trim(int(device))
    if st != KC_OK:
        raise KcError(st, "kc_device_trim")


def corpus_fill(kind, seed, first_unit, n_units, unit_size, threads=None):
    """Deterministic synthetic corpus (kc_corpus_fill): returns a numpy uint8 array of n_units*unit_size bytes."""
    import numpy as np
    L = load()
    buf = np.empty(int(n_units) * int(unit_size), dtype=np.uint8)
    if threads is None:
        threads = os.cpu_count() or 1
    st = L.kc_corpus_fill(ord(kind), seed, first_unit, n_units, unit_size, buf.ctypes.data, threads)
    if st != KC_OK:
        raise KcError(st, "kc_corpus_fill")
    return buf
