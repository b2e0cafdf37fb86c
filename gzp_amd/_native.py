"""ctypes binding of the C ABI in include/gzpx.h (gzp_amd/lib/libgzpx.so, built by hipcc for gfx950).

There is no fallback: if the HIP library is missing or no GPU is present, loading / context
creation raises -- the product path never routes through a CPU implementation.
"""
import ctypes
import os
import struct

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libgzpx.so")

OK = 0
ERR_INVALID_ARG = 1
ERR_BUFFER_SIZE = 2
ERR_COMPRESSION_LEVEL = 3
ERR_INSUFFICIENT_SPACE = 4
ERR_BLOCK_SIZE_EXCEEDED = 5
ERR_DEVICE = 6
ERR_NO_DEVICE = 7
ERR_UNSUPPORTED = 8
ERR_NUM_THREADS = 9
ERR_IO = 10
ERR_CHANNEL = 11
ERR_INVALID_HEADER = 12
ERR_INVALID_CHECK = 13
ERR_BAD_DATA = 14
ERR_BUSY = 15

SLAB_FULL_BLOCKS = 0
SLAB_LAST = 1
SLAB_FLUSH = 2

FORMAT_BGZF = 0
FORMAT_MGZIP = 1
FORMAT_SNAP = 2  # compression only (gzp has no ParDecompress<Snap>)
COMPAT_1_24 = 0
COMPAT_1_10 = 1
STREAM_NONE = ctypes.c_void_p(-1).value  # GZPX_STREAM_NONE: the caller has synchronized, no stream dependency
N_STAGES = 9
INFLATE_SEG, INFLATE_WAVE = 0, 1
# GZPX_HANDBACK_*: why the decode / copy pair handed a member to k_inflate (DContext.debug_handback)
(HANDBACK_NONE, HANDBACK_HEADER, HANDBACK_STORED, HANDBACK_NO_EOB, HANDBACK_RESYNC, HANDBACK_SPAN_SYMBOL, HANDBACK_SPAN_OVERRUN,
 HANDBACK_DISTANCE, HANDBACK_OFFSET_SYMBOL, HANDBACK_CODEWORD, HANDBACK_COUNT_MISMATCH, HANDBACK_FINAL, HANDBACK_LZCOPY) = range(13)
RANGE_UNCOMPRESSED, RANGE_VIRTUAL = 0, 1
WRAP_RAW, WRAP_ZLIB, WRAP_GZIP = 0, 1, 2  # inflate_batch_device: RFC 1951 / 1950 / 1952
BATCH_SHORT_OK = 1
CHECK_CRC32, CHECK_ADLER32, CHECK_CRC32C = 0, 1, 2  # checksum_batch_device: zlib crc32 / zlib adler32 / Castagnoli
LINES_TILE = 16384  # GZPX_LINES_TILE: the tile of the line table, in bytes of the inflated stream
FIND_MAX_PATTERN = 256  # GZPX_FIND_MAX_PATTERN
FIND_NO_LINES = -1      # GZPX_FIND_NO_LINES
SELECT_INVERT = 1       # GZPX_SELECT_INVERT
FINDSET_MAX_PATTERNS = 256  # GZPX_FINDSET_MAX_PATTERNS
FINDSET_MAX_BYTES = 16384   # GZPX_FINDSET_MAX_BYTES: the sum of a set's pattern lengths
FIELDS_MAX_RANGES = 64           # GZPX_FIELDS_MAX_RANGES
FIELDS_COMPLEMENT = 1            # GZPX_FIELDS_COMPLEMENT
FIELDS_TO_END = (1 << 64) - 1    # GZPX_FIELDS_TO_END: as a field range's end, through the line's last field
COLUMNS_MAX = 16                 # GZPX_COLUMNS_MAX
CELL_MAX_BYTES = 64              # GZPX_CELL_MAX_BYTES
COL_INT64, COL_FLOAT64 = 0, 1    # GZPX_COL_*
CELL_OK, CELL_MISSING, CELL_EMPTY, CELL_INVALID, CELL_RANGE = range(5)  # GZPX_CELL_*
COLUMN_DTYPE = [("field", "<u8"), ("type", "<u4"), ("reserved", "<u4")]  # gzpx_column, as a numpy record
WHERE_MAX_TERMS = 32             # GZPX_WHERE_MAX_TERMS
WHERE_LT, WHERE_LE, WHERE_EQ, WHERE_NE, WHERE_GE, WHERE_GT, WHERE_IS_OK, WHERE_NOT_OK = range(8)  # GZPX_WHERE_*: a term's op
WHERE_ANY, WHERE_INVERT = 1, 2   # GZPX_WHERE_ANY, GZPX_WHERE_INVERT: flags
COL_TEXT = 2                     # GZPX_COL_TEXT: gzpx_where_text_device's terms only
WHERE_PREFIX, WHERE_NOT_PREFIX = 8, 9  # GZPX_WHERE_PREFIX, GZPX_WHERE_NOT_PREFIX: ops of TEXT terms
WHERE_TEXT_MAX = 64              # GZPX_WHERE_TEXT_MAX: the bytes of one constant
WHERE_TEXT_POOL_MAX = 2048       # GZPX_WHERE_TEXT_POOL_MAX
WHERE_TERM_DTYPE = [("field", "<u8"), ("type", "<u4"), ("op", "<u4"), ("value", "<u8")]  # gzpx_where_term, as a numpy record

EXPORTS = [
    "gzpx_config_default", "gzpx_ctx_create", "gzpx_ctx_destroy", "gzpx_slab_bound",
    "gzpx_compress_slab", "gzpx_compress_slab_device", "gzpx_encode_block",
    "gzpx_alloc_compressor", "gzpx_deflate_compress", "gzpx_deflate_compress_bound",
    "gzpx_free_compressor", "gzpx_compressor_set_compat", "gzpx_crc32",
    "gzpx_ctx_set_profiling", "gzpx_ctx_last_stage_ms", "gzpx_stage_name", "gzpx_ctx_stage_kernel", "gzpx_debug_tokens",
    "gzpx_debug_set_flags", "gzpx_debug_redo_count", "gzpx_strerror", "gzpx_device_name", "gzpx_version",
    "gzpx_compress_slab_submit", "gzpx_compress_slab_submit_device", "gzpx_compress_slab_wait",
    "gzpx_compress_slab_event", "gzpx_crc32_checked", "gzpx_last_status", "gzpx_crc32_combine", "gzpx_adler32",
    "gzpx_adler32_checked", "gzpx_adler32_combine",
    "gzpx_par_create", "gzpx_par_write", "gzpx_par_write_chunked", "gzpx_par_flush", "gzpx_par_finish", "gzpx_par_destroy",
    "gzpx_par_last_error", "gzpx_par_create_pinned", "gzpx_par_reserve", "gzpx_par_commit", "gzpx_par_index", "gzpx_gzi_size",
    "gzpx_gzi_write", "gzpx_dctx_create", "gzpx_dctx_destroy", "gzpx_scan_blocks",
    "gzpx_decompress_blocks", "gzpx_decompress_blocks_device", "gzpx_decompress_blocks_submit",
    "gzpx_decompress_blocks_wait", "gzpx_alloc_decompressor", "gzpx_deflate_decompress",
    "gzpx_free_decompressor", "gzpx_pard_create", "gzpx_pard_read", "gzpx_pard_fill_buf", "gzpx_pard_consume", "gzpx_pard_destroy",
    "gzpx_pard_last_error", "gzpx_host_alloc", "gzpx_host_free", "gzpx_dctx_last_inflate_ms",
    "gzpx_debug_inflate", "gzpx_debug_inflate_handback", "gzpx_dctx_last_inflate_stage_ms", "gzpx_dctx_set_route", "gzpx_dctx_last_redo_count", "gzpx_synth_fastq_device", "gzpx_synth_ascii_device",
    "gzpx_ctx_active_compat", "gzpx_build_id", "gzpx_multi_create", "gzpx_multi_destroy", "gzpx_multi_devices", "gzpx_multi_compress_slab",
    "gzpx_multi_shard", "gzpx_multi_compress_slab_device", "gzpx_debug_snap",
    "gzpx_scan_blocks_device", "gzpx_decompress_stream_device", "gzpx_index_device", "gzpx_dctx_last_scan_ms",
    "gzpx_dindex_build_device", "gzpx_dindex_entries", "gzpx_dindex_destroy", "gzpx_read_ranges_device",
    "gzpx_dctx_last_ranges_members", "gzpx_dctx_last_ranges_ms",
    "gzpx_inflate_batch_device", "gzpx_dctx_last_check_ms", "gzpx_inflate_batch_sizes_device",
    "gzpx_checksum_batch_device", "gzpx_dctx_set_checksum_width",
    "gzpx_dlines_build_device", "gzpx_dlines_prefix", "gzpx_dlines_destroy", "gzpx_line_offsets_device",
    "gzpx_read_lines_device", "gzpx_dctx_set_lines_batch", "gzpx_dctx_last_lines_members", "gzpx_dctx_last_lines_ms",
    "gzpx_dctx_last_lines_build_ms",
    "gzpx_find_device", "gzpx_dctx_last_find_ms",
    "gzpx_select_lines_device", "gzpx_dctx_last_select_ms", "gzpx_read_lines_table_device",
    "gzpx_find_set_device", "gzpx_dctx_last_find_set_ms", "gzpx_select_lines_set_device",
    "gzpx_read_fields_device", "gzpx_read_fields_table_device", "gzpx_dctx_last_fields_ms",
    "gzpx_read_columns_device", "gzpx_read_columns_table_device", "gzpx_dctx_last_columns_ms",
    "gzpx_where_lines_device", "gzpx_where_lines_table_device", "gzpx_dctx_last_where_ms",
    "gzpx_where_text_device", "gzpx_where_text_table_device",
]


class GzpxConfig(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int), ("format", ctypes.c_int), ("level", ctypes.c_int),
                ("compat", ctypes.c_int), ("buffer_size", ctypes.c_size_t),
                ("max_slab_bytes", ctypes.c_size_t)]


class GzpxParConfig(ctypes.Structure):
    _fields_ = [("format", ctypes.c_int), ("level", ctypes.c_int), ("compat", ctypes.c_int),
                ("device", ctypes.c_int), ("buffer_size", ctypes.c_size_t),
                ("num_threads", ctypes.c_size_t), ("batch_blocks", ctypes.c_size_t)]


class GzpxCheckInfo(ctypes.Structure):
    _fields_ = [("block", ctypes.c_size_t), ("found", ctypes.c_uint32), ("expected", ctypes.c_uint32)]


class GzpxMemberResult(ctypes.Structure):
    """gzpx_member_result: one row of inflate_batch_device's d_results."""
    _fields_ = [("status", ctypes.c_uint32), ("produced", ctypes.c_uint32), ("found", ctypes.c_uint32),
                ("expected", ctypes.c_uint32)]


READ_FN = ctypes.CFUNCTYPE(ctypes.c_long, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint8), ctypes.c_size_t)
WRITE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint8), ctypes.c_size_t)


class GzpxError(RuntimeError):
    def __init__(self, code, msg, block=None, range_index=None, needed=None):
        super().__init__("gzpx error %d: %s%s%s" % (code, msg, "" if block is None else " (block %d)" % block,
                                                   "" if range_index is None else " (range %d)" % range_index))
        self.code = code
        self.block = block
        self.range_index = range_index  # read_ranges_device: the first range that is invalid
        self.needed = needed            # read_ranges_device, ERR_INSUFFICIENT_SPACE in front of the inflate: bytes of output


class GzpxLib:
    """All entry points of include/gzpx.h with argtypes set."""

    def __init__(self, path=LIB_PATH):
        if not os.path.exists(path):
            raise ImportError(
                "gzp_amd: %s not found -- build it with `python -c 'import __graft_entry__ as g; "
                "g.build()'` (hipcc --offload-arch=gfx950); there is no CPU fallback" % path)
        self.path = path
        # PyTorch-ROCm bundles its own HIP runtime (same SONAME as /opt/rocm's).  Two copies in one
        # process fight over the device, so when torch is importable let it load first; libgzpx.so
        # then binds to the runtime that is already resident.
        try:
            import torch  # noqa: F401
        except Exception:  # pragma: no cover - torch-less hosts use the system ROCm runtime
            pass
        L = self.L = ctypes.CDLL(path)
        vp, sz, i32, u32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint32
        psz = ctypes.POINTER(ctypes.c_size_t)
        L.gzpx_config_default.restype = None
        L.gzpx_config_default.argtypes = [ctypes.POINTER(GzpxConfig), i32]
        L.gzpx_ctx_create.restype = i32
        L.gzpx_ctx_create.argtypes = [ctypes.POINTER(GzpxConfig), ctypes.POINTER(vp)]
        L.gzpx_ctx_destroy.restype = None
        L.gzpx_ctx_destroy.argtypes = [vp]
        L.gzpx_slab_bound.restype = sz
        L.gzpx_slab_bound.argtypes = [vp, sz]
        L.gzpx_build_id.restype = ctypes.c_char_p
        L.gzpx_build_id.argtypes = []
        L.gzpx_ctx_active_compat.restype = i32
        L.gzpx_ctx_active_compat.argtypes = [vp]
        L.gzpx_compress_slab.restype = i32
        L.gzpx_compress_slab.argtypes = [vp, vp, sz, i32, vp, sz, psz, vp, sz, psz]
        L.gzpx_compress_slab_device.restype = i32
        L.gzpx_compress_slab_device.argtypes = [vp, vp, sz, i32, vp, sz, psz, vp, sz, psz, vp]
        L.gzpx_encode_block.restype = i32
        L.gzpx_encode_block.argtypes = [vp, vp, sz, i32, vp, sz, psz]
        L.gzpx_alloc_compressor.restype = vp
        L.gzpx_alloc_compressor.argtypes = [i32]
        L.gzpx_deflate_compress.restype = sz
        L.gzpx_deflate_compress.argtypes = [vp, vp, sz, vp, sz]
        L.gzpx_deflate_compress_bound.restype = sz
        L.gzpx_deflate_compress_bound.argtypes = [vp, sz]
        L.gzpx_free_compressor.restype = None
        L.gzpx_free_compressor.argtypes = [vp]
        L.gzpx_compressor_set_compat.restype = i32
        L.gzpx_compressor_set_compat.argtypes = [vp, i32]
        L.gzpx_crc32.restype = u32
        L.gzpx_crc32.argtypes = [u32, vp, sz]
        L.gzpx_ctx_set_profiling.restype = i32
        L.gzpx_ctx_set_profiling.argtypes = [vp, i32]
        L.gzpx_ctx_last_stage_ms.restype = i32
        L.gzpx_ctx_last_stage_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
        L.gzpx_stage_name.restype = ctypes.c_char_p
        L.gzpx_stage_name.argtypes = [i32]
        L.gzpx_ctx_stage_kernel.restype = ctypes.c_char_p
        L.gzpx_ctx_stage_kernel.argtypes = [vp, i32]
        L.gzpx_debug_tokens.restype = i32
        L.gzpx_debug_tokens.argtypes = [vp, sz, vp, sz, psz, vp, psz]
        L.gzpx_debug_set_flags.restype = i32
        L.gzpx_debug_set_flags.argtypes = [vp, u32]
        L.gzpx_debug_redo_count.restype = i32
        L.gzpx_debug_redo_count.argtypes = [vp, ctypes.POINTER(ctypes.c_uint32)]
        pu64 = ctypes.POINTER(ctypes.c_uint64)
        L.gzpx_compress_slab_submit.restype = i32
        L.gzpx_compress_slab_submit.argtypes = [vp, vp, sz, i32, vp, sz, pu64]
        L.gzpx_compress_slab_submit_device.restype = i32
        L.gzpx_compress_slab_submit_device.argtypes = [vp, vp, sz, i32, vp, sz, vp, pu64]
        L.gzpx_compress_slab_wait.restype = i32
        L.gzpx_compress_slab_wait.argtypes = [vp, ctypes.c_uint64, psz, vp, sz, psz]
        L.gzpx_compress_slab_event.restype = i32
        L.gzpx_compress_slab_event.argtypes = [vp, ctypes.c_uint64, ctypes.POINTER(vp)]
        L.gzpx_crc32_checked.restype = i32
        L.gzpx_crc32_checked.argtypes = [u32, vp, sz, ctypes.POINTER(u32)]
        L.gzpx_last_status.restype = i32
        L.gzpx_last_status.argtypes = []
        L.gzpx_strerror.restype = ctypes.c_char_p
        L.gzpx_strerror.argtypes = [i32]
        L.gzpx_device_name.restype = ctypes.c_char_p
        L.gzpx_device_name.argtypes = [vp]
        L.gzpx_version.restype = ctypes.c_char_p
        L.gzpx_version.argtypes = []
        L.gzpx_par_create.restype = i32
        L.gzpx_par_create.argtypes = [ctypes.POINTER(GzpxParConfig), WRITE_FN, vp, ctypes.POINTER(vp)]
        L.gzpx_par_create_pinned.restype = i32
        L.gzpx_par_create_pinned.argtypes = [ctypes.POINTER(GzpxParConfig), sz, WRITE_FN, vp, ctypes.POINTER(vp)]
        L.gzpx_par_write.restype = i32
        L.gzpx_par_write.argtypes = [vp, vp, sz]
        L.gzpx_par_write_chunked.restype = i32
        L.gzpx_par_write_chunked.argtypes = [vp, vp, sz, sz]
        L.gzpx_par_reserve.restype = i32
        L.gzpx_par_reserve.argtypes = [vp, ctypes.POINTER(vp), psz]
        L.gzpx_par_commit.restype = i32
        L.gzpx_par_commit.argtypes = [vp, sz]
        L.gzpx_par_index.restype = i32
        L.gzpx_par_index.argtypes = [vp, vp, sz, psz]
        L.gzpx_gzi_size.restype = sz
        L.gzpx_gzi_size.argtypes = [sz]
        L.gzpx_gzi_write.restype = i32
        L.gzpx_gzi_write.argtypes = [vp, sz, vp, sz, psz]
        L.gzpx_par_flush.restype = i32
        L.gzpx_par_flush.argtypes = [vp]
        L.gzpx_par_finish.restype = i32
        L.gzpx_par_finish.argtypes = [vp]
        L.gzpx_par_destroy.restype = None
        L.gzpx_par_destroy.argtypes = [vp]
        L.gzpx_par_last_error.restype = ctypes.c_char_p
        L.gzpx_par_last_error.argtypes = [vp]
        pinfo = ctypes.POINTER(GzpxCheckInfo)
        L.gzpx_dctx_create.restype = i32
        L.gzpx_dctx_create.argtypes = [i32, i32, ctypes.POINTER(vp)]
        L.gzpx_dctx_destroy.restype = None
        L.gzpx_dctx_destroy.argtypes = [vp]
        L.gzpx_scan_blocks.restype = i32
        L.gzpx_scan_blocks.argtypes = [i32, vp, sz, vp, vp, sz, psz, psz]
        L.gzpx_decompress_blocks.restype = i32
        L.gzpx_decompress_blocks.argtypes = [vp, vp, sz, vp, vp, sz, vp, sz, psz, pinfo]
        L.gzpx_decompress_blocks_submit.restype = i32
        L.gzpx_decompress_blocks_submit.argtypes = [vp, vp, sz, vp, vp, sz, vp, sz, ctypes.POINTER(ctypes.c_uint64)]
        L.gzpx_decompress_blocks_wait.restype = i32
        L.gzpx_decompress_blocks_wait.argtypes = [vp, ctypes.c_uint64, psz, pinfo]
        L.gzpx_decompress_blocks_device.restype = i32
        L.gzpx_decompress_blocks_device.argtypes = [vp, vp, sz, vp, vp, sz, vp, sz, psz, pinfo, vp]
        L.gzpx_scan_blocks_device.restype = i32
        L.gzpx_scan_blocks_device.argtypes = [vp, vp, sz, vp, vp, sz, psz, psz, vp]
        L.gzpx_decompress_stream_device.restype = i32
        L.gzpx_decompress_stream_device.argtypes = [vp, vp, sz, vp, sz, psz, psz, psz, pinfo, vp]
        L.gzpx_index_device.restype = i32
        L.gzpx_index_device.argtypes = [vp, vp, sz, vp, sz, psz, psz, pu64, vp]
        L.gzpx_dctx_last_scan_ms.restype = i32
        L.gzpx_dctx_last_scan_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
        L.gzpx_dindex_build_device.restype = i32
        L.gzpx_dindex_build_device.argtypes = [vp, vp, sz, ctypes.POINTER(vp), psz, psz, pu64, vp]
        L.gzpx_dindex_entries.restype = i32
        L.gzpx_dindex_entries.argtypes = [vp, vp, sz, psz]
        L.gzpx_dindex_destroy.restype = None
        L.gzpx_dindex_destroy.argtypes = [vp]
        L.gzpx_read_ranges_device.restype = i32
        L.gzpx_read_ranges_device.argtypes = [vp, vp, vp, sz, vp, sz, i32, vp, sz, psz, vp, psz,
                                              ctypes.POINTER(GzpxCheckInfo), vp]
        L.gzpx_dctx_last_ranges_members.restype = i32
        L.gzpx_dctx_last_ranges_members.argtypes = [vp, psz]
        L.gzpx_dctx_last_ranges_ms.restype = i32
        L.gzpx_dctx_last_ranges_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
        L.gzpx_dlines_build_device.restype = i32
        L.gzpx_dlines_build_device.argtypes = [vp, vp, vp, sz, ctypes.c_uint, ctypes.POINTER(vp), pu64, pu64,
                                               ctypes.POINTER(GzpxCheckInfo), vp]
        L.gzpx_dlines_prefix.restype = i32
        L.gzpx_dlines_prefix.argtypes = [vp, vp, sz, psz]
        L.gzpx_dlines_destroy.restype = None
        L.gzpx_dlines_destroy.argtypes = [vp]
        L.gzpx_line_offsets_device.restype = i32
        L.gzpx_line_offsets_device.argtypes = [vp, vp, vp, vp, sz, vp, sz, vp, psz, ctypes.POINTER(GzpxCheckInfo), vp]
        L.gzpx_read_lines_device.restype = i32
        L.gzpx_read_lines_device.argtypes = [vp, vp, vp, vp, sz, vp, sz, vp, sz, psz, vp, vp, psz,
                                             ctypes.POINTER(GzpxCheckInfo), vp]
        L.gzpx_dctx_set_lines_batch.restype = i32
        L.gzpx_dctx_set_lines_batch.argtypes = [vp, sz]
        L.gzpx_dctx_last_lines_members.restype = i32
        L.gzpx_dctx_last_lines_members.argtypes = [vp, psz]
        L.gzpx_dctx_last_lines_ms.restype = i32
        L.gzpx_dctx_last_lines_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
        L.gzpx_dctx_last_lines_build_ms.restype = i32
        L.gzpx_dctx_last_lines_build_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
        L.gzpx_find_device.restype = i32
        L.gzpx_find_device.argtypes = [vp, vp, vp, sz, vp, sz, ctypes.c_int, vp, vp, sz, pu64, ctypes.POINTER(GzpxCheckInfo), vp]
        L.gzpx_dctx_last_find_ms.restype = i32
        L.gzpx_dctx_last_find_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
        L.gzpx_select_lines_device.restype = i32
        L.gzpx_select_lines_device.argtypes = [vp, vp, vp, vp, sz, vp, sz, ctypes.c_uint64, ctypes.c_uint, vp, sz, pu64, pu64, pu64,
                                               ctypes.POINTER(GzpxCheckInfo), vp]
        L.gzpx_dctx_last_select_ms.restype = i32
        L.gzpx_dctx_last_select_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
        L.gzpx_find_set_device.restype = i32
        L.gzpx_find_set_device.argtypes = [vp, vp, vp, sz, vp, vp, sz, ctypes.c_int, vp, vp, vp, sz, vp, pu64,
                                           ctypes.POINTER(GzpxCheckInfo), vp]
        L.gzpx_dctx_last_find_set_ms.restype = i32
        L.gzpx_dctx_last_find_set_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
        L.gzpx_select_lines_set_device.restype = i32
        L.gzpx_select_lines_set_device.argtypes = [vp, vp, vp, vp, sz, vp, vp, sz, ctypes.c_uint64, ctypes.c_uint, vp, sz, pu64, pu64,
                                                   pu64, ctypes.POINTER(GzpxCheckInfo), vp]
        L.gzpx_read_lines_table_device.restype = i32
        L.gzpx_read_lines_table_device.argtypes = [vp, vp, vp, vp, sz, vp, sz, vp, sz, psz, vp, vp, psz,
                                                   ctypes.POINTER(GzpxCheckInfo), vp]
        for fn in (L.gzpx_read_fields_device, L.gzpx_read_fields_table_device):
            fn.restype = i32
            fn.argtypes = [vp, vp, vp, vp, sz, vp, sz, ctypes.c_uint, vp, sz, ctypes.c_uint, vp, sz, psz, vp, psz,
                           ctypes.POINTER(GzpxCheckInfo), vp]
        L.gzpx_dctx_last_fields_ms.restype = i32
        L.gzpx_dctx_last_fields_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
        for fn in (L.gzpx_read_columns_device, L.gzpx_read_columns_table_device):
            fn.restype = i32
            fn.argtypes = [vp, vp, vp, vp, sz, vp, sz, ctypes.c_uint, vp, sz, vp, vp, sz, pu64, pu64, vp, vp, psz,
                           ctypes.POINTER(GzpxCheckInfo), vp]
        L.gzpx_dctx_last_columns_ms.restype = i32
        L.gzpx_dctx_last_columns_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
        for fn in (L.gzpx_where_lines_device, L.gzpx_where_lines_table_device):
            fn.restype = i32
            fn.argtypes = [vp, vp, vp, vp, sz, vp, sz, ctypes.c_uint, vp, sz, ctypes.c_uint, vp, sz, pu64, pu64, pu64, pu64, psz,
                           ctypes.POINTER(GzpxCheckInfo), vp]
        for fn in (L.gzpx_where_text_device, L.gzpx_where_text_table_device):
            fn.restype = i32
            fn.argtypes = [vp, vp, vp, vp, sz, vp, sz, ctypes.c_uint, vp, sz, vp, sz, ctypes.c_uint, vp, sz, pu64, pu64, pu64, pu64,
                           psz, ctypes.POINTER(GzpxCheckInfo), vp]
        L.gzpx_dctx_last_where_ms.restype = i32
        L.gzpx_dctx_last_where_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
        L.gzpx_inflate_batch_device.restype = i32
        L.gzpx_inflate_batch_device.argtypes = [vp, i32, ctypes.c_uint, vp, sz, vp, vp, vp, sz, vp, sz, vp, vp, psz, psz,
                                                ctypes.POINTER(GzpxCheckInfo), vp]
        L.gzpx_inflate_batch_sizes_device.restype = i32
        L.gzpx_inflate_batch_sizes_device.argtypes = [vp, i32, vp, sz, vp, vp, sz, ctypes.c_uint32, vp, vp, vp, pu64, psz,
                                                      ctypes.POINTER(GzpxCheckInfo), vp]
        L.gzpx_checksum_batch_device.restype = i32
        L.gzpx_checksum_batch_device.argtypes = [vp, i32, vp, sz, vp, vp, sz, vp, vp, vp, vp, psz,
                                                 ctypes.POINTER(GzpxCheckInfo), vp]
        L.gzpx_dctx_set_checksum_width.restype = i32
        L.gzpx_dctx_set_checksum_width.argtypes = [vp, ctypes.c_uint]
        L.gzpx_dctx_last_check_ms.restype = i32
        L.gzpx_dctx_last_check_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
        L.gzpx_alloc_decompressor.restype = vp
        L.gzpx_alloc_decompressor.argtypes = []
        L.gzpx_deflate_decompress.restype = i32
        L.gzpx_deflate_decompress.argtypes = [vp, vp, sz, vp, sz, psz]
        L.gzpx_free_decompressor.restype = None
        L.gzpx_free_decompressor.argtypes = [vp]
        L.gzpx_host_alloc.restype = vp
        L.gzpx_host_alloc.argtypes = [sz]
        L.gzpx_host_free.restype = None
        L.gzpx_host_free.argtypes = [vp]
        L.gzpx_dctx_last_inflate_ms.restype = i32
        L.gzpx_dctx_last_inflate_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
        L.gzpx_debug_inflate.restype = i32
        L.gzpx_debug_inflate.argtypes = [vp, i32, ctypes.POINTER(ctypes.c_uint64)]
        L.gzpx_debug_inflate_handback.restype = i32
        L.gzpx_debug_inflate_handback.argtypes = [vp, ctypes.POINTER(ctypes.c_uint32), ctypes.c_size_t]
        L.gzpx_debug_snap.restype = i32
        L.gzpx_debug_snap.argtypes = [vp, i32, ctypes.POINTER(ctypes.c_uint64)]
        L.gzpx_crc32_combine.restype = ctypes.c_uint32
        L.gzpx_crc32_combine.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64]
        L.gzpx_adler32_combine.restype = ctypes.c_uint32
        L.gzpx_adler32_combine.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64]
        L.gzpx_adler32.restype = ctypes.c_uint32
        L.gzpx_adler32.argtypes = [ctypes.c_uint32, vp, ctypes.c_size_t]
        L.gzpx_adler32_checked.restype = i32
        L.gzpx_adler32_checked.argtypes = [ctypes.c_uint32, vp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint32)]
        L.gzpx_dctx_last_inflate_stage_ms.restype = i32
        L.gzpx_dctx_last_inflate_stage_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
        L.gzpx_dctx_set_route.restype = i32
        L.gzpx_dctx_set_route.argtypes = [vp, i32]
        L.gzpx_dctx_last_redo_count.restype = i32
        L.gzpx_dctx_last_redo_count.argtypes = [vp, ctypes.POINTER(ctypes.c_uint32)]
        L.gzpx_synth_fastq_device.restype = i32
        L.gzpx_synth_fastq_device.argtypes = [vp, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, vp]
        L.gzpx_multi_create.restype = i32
        L.gzpx_multi_create.argtypes = [ctypes.POINTER(GzpxConfig), ctypes.POINTER(ctypes.c_int), sz, ctypes.POINTER(vp)]
        L.gzpx_multi_destroy.restype = None
        L.gzpx_multi_destroy.argtypes = [vp]
        L.gzpx_multi_devices.restype = sz
        L.gzpx_multi_devices.argtypes = [vp]
        L.gzpx_multi_compress_slab.restype = i32
        L.gzpx_multi_compress_slab.argtypes = [vp, vp, sz, i32, vp, sz, psz, vp, sz, psz]
        L.gzpx_multi_shard.restype = i32
        L.gzpx_multi_shard.argtypes = [vp, sz, sz, psz, psz]
        L.gzpx_multi_compress_slab_device.restype = i32
        L.gzpx_multi_compress_slab_device.argtypes = [vp, ctypes.POINTER(vp), sz, i32, sz, vp, sz, psz, vp, sz, psz]
        L.gzpx_synth_ascii_device.restype = i32
        L.gzpx_synth_ascii_device.argtypes = [vp, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, vp]
        L.gzpx_pard_create.restype = i32
        L.gzpx_pard_create.argtypes = [i32, i32, sz, READ_FN, vp, ctypes.POINTER(vp)]
        L.gzpx_pard_read.restype = i32
        L.gzpx_pard_read.argtypes = [vp, vp, sz, psz]
        L.gzpx_pard_fill_buf.restype = i32
        L.gzpx_pard_fill_buf.argtypes = [vp, ctypes.POINTER(vp), psz]
        L.gzpx_pard_consume.restype = i32
        L.gzpx_pard_consume.argtypes = [vp, sz]
        L.gzpx_pard_destroy.restype = None
        L.gzpx_pard_destroy.argtypes = [vp]
        L.gzpx_pard_last_error.restype = ctypes.c_char_p
        L.gzpx_pard_last_error.argtypes = [vp]

    def build_id(self):
        """gzpx_build_id(): which sources this library was built from (gzp_amd/build.py: source_id())."""
        return self.L.gzpx_build_id().decode()

    def strerror(self, code):
        return self.L.gzpx_strerror(code).decode()

    def check(self, code, block=None):
        if code != OK:
            raise GzpxError(code, self.strerror(code), block)


_default = None


def load():
    """The product library (HIP build).  Raises ImportError when it has not been built."""
    global _default
    if _default is None:
        _default = GzpxLib(LIB_PATH)
    return _default


def _u8(data):
    if isinstance(data, np.ndarray):
        return np.ascontiguousarray(data, dtype=np.uint8)
    return np.frombuffer(bytes(data), dtype=np.uint8)


class Context:
    """gzpx_ctx: one device, one format/level/buffer_size -- the GPU-side `create_compressor`."""

    def __init__(self, format=FORMAT_BGZF, level=1, buffer_size=None, compat=COMPAT_1_24, device=0,
                 max_slab_bytes=1 << 30, lib=None):
        self.lib = lib or load()
        cfg = GzpxConfig()
        self.lib.L.gzpx_config_default(ctypes.byref(cfg), format)
        cfg.device = device
        cfg.level = level
        cfg.compat = compat
        if buffer_size is not None:
            cfg.buffer_size = buffer_size
        cfg.max_slab_bytes = max_slab_bytes
        self.cfg = cfg
        self.buffer_size = cfg.buffer_size
        self.format = format
        h = ctypes.c_void_p()
        self.lib.check(self.lib.L.gzpx_ctx_create(ctypes.byref(cfg), ctypes.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.L.gzpx_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def device_name(self):
        return self.lib.L.gzpx_device_name(self.h).decode()

    def slab_bound(self, n):
        return int(self.lib.L.gzpx_slab_bound(self.h, n))

    def active_compat(self):
        """The GZPX_COMPAT_* rules the context really runs (levels 10-12: always the 1.10 ones)."""
        return int(self.lib.L.gzpx_ctx_active_compat(self.h))

    def n_blocks(self, n):
        return 1 if n == 0 else -(-n // self.buffer_size)

    @staticmethod
    def _mode(is_last):
        if is_last is True:
            return SLAB_LAST
        if is_last is False:
            return SLAB_FULL_BLOCKS
        return int(is_last)

    def compress_slab(self, data, is_last=True, return_block_sizes=False):
        """Host buffer in, framed bytes out (gzpx_compress_slab).  is_last: True = SLAB_LAST,
        False = SLAB_FULL_BLOCKS, or an explicit SLAB_* mode."""
        a = _u8(data)
        cap = self.slab_bound(a.size)
        out = np.empty(cap, dtype=np.uint8)
        nb_max = self.n_blocks(a.size)
        sizes = np.zeros(nb_max, dtype=np.uint32)
        out_len = ctypes.c_size_t(0)
        nb = ctypes.c_size_t(0)
        rc = self.lib.L.gzpx_compress_slab(self.h, a.ctypes.data, a.size, self._mode(is_last),
                                           out.ctypes.data, cap, ctypes.byref(out_len),
                                           sizes.ctypes.data, nb_max, ctypes.byref(nb))
        self.lib.check(rc, nb.value if rc == ERR_BLOCK_SIZE_EXCEEDED else None)
        res = out[:out_len.value].tobytes()
        if return_block_sizes:
            return res, sizes[:nb.value].copy()
        return res

    def compress_slab_device(self, d_in_ptr, in_len, d_out_ptr, out_cap, is_last=True, stream=None,
                             block_sizes=None):
        """Device pointers in/out (gzpx_compress_slab_device).  Returns (out_len, n_blocks)."""
        out_len = ctypes.c_size_t(0)
        nb = ctypes.c_size_t(0)
        bs_ptr, bs_n = (None, 0)
        if block_sizes is not None:
            bs_ptr, bs_n = block_sizes.ctypes.data, block_sizes.size
        rc = self.lib.L.gzpx_compress_slab_device(self.h, d_in_ptr, in_len, self._mode(is_last), d_out_ptr,
                                                  out_cap, ctypes.byref(out_len), bs_ptr, bs_n,
                                                  ctypes.byref(nb), stream)
        self.lib.check(rc, nb.value if rc == ERR_BLOCK_SIZE_EXCEEDED else None)
        return out_len.value, nb.value

    def encode_block(self, data, is_last=False):
        a = _u8(data)
        cap = self.slab_bound(a.size)
        out = np.empty(cap, dtype=np.uint8)
        out_len = ctypes.c_size_t(0)
        self.lib.check(self.lib.L.gzpx_encode_block(self.h, a.ctypes.data, a.size, int(is_last),
                                                    out.ctypes.data, cap, ctypes.byref(out_len)))
        return out[:out_len.value].tobytes()

    def set_profiling(self, on=True):
        self.lib.check(self.lib.L.gzpx_ctx_set_profiling(self.h, int(on)))

    def last_stage_ms(self):
        ms = (ctypes.c_float * N_STAGES)()
        self.lib.check(self.lib.L.gzpx_ctx_last_stage_ms(self.h, ms))
        out = {}
        for i in range(N_STAGES):
            name = self.lib.L.gzpx_ctx_stage_kernel(self.h, i).decode()
            if name != "-":
                out[name] = float(ms[i])
        return out

    def debug_set_flags(self, flags):
        self.lib.check(self.lib.L.gzpx_debug_set_flags(self.h, flags))

    def debug_redo_count(self):
        """Level 1: blocks of the last batch that k_mparse handed back to the dense kernels.  Levels 2-4 (round 5: the same
        scratch list serves them): blocks that k_parse_hc listed for k_match_hc_stale -- a sub-block with another min_len
        behind a start that k_match_hc_sparse compacted."""
        c = ctypes.c_uint32(0)
        self.lib.check(self.lib.L.gzpx_debug_redo_count(self.h, ctypes.byref(c)))
        return c.value

    def submit(self, in_ptr, in_len, out_ptr, out_cap, mode=SLAB_LAST):
        """gzpx_compress_slab_submit on raw host pointers (page-locked for DMA overlap); returns the
        ticket, or None when every slot is in flight."""
        t = ctypes.c_uint64(0)
        rc = self.lib.L.gzpx_compress_slab_submit(self.h, in_ptr, in_len, int(mode), out_ptr, out_cap,
                                                  ctypes.byref(t))
        if rc == ERR_BUSY:
            return None
        self.lib.check(rc)
        return t.value

    def submit_device(self, d_in_ptr, in_len, d_out_ptr, out_cap, mode=SLAB_LAST, after_stream=None):
        t = ctypes.c_uint64(0)
        rc = self.lib.L.gzpx_compress_slab_submit_device(self.h, d_in_ptr, in_len, int(mode), d_out_ptr,
                                                         out_cap, after_stream, ctypes.byref(t))
        if rc == ERR_BUSY:
            return None
        self.lib.check(rc)
        return t.value

    def wait(self, ticket, block_sizes=None):
        """gzpx_compress_slab_wait: (out_len, n_blocks)."""
        out_len = ctypes.c_size_t(0)
        nb = ctypes.c_size_t(0)
        bs_ptr, bs_n = (None, 0)
        if block_sizes is not None:
            bs_ptr, bs_n = block_sizes.ctypes.data, block_sizes.size
        rc = self.lib.L.gzpx_compress_slab_wait(self.h, ticket, ctypes.byref(out_len), bs_ptr, bs_n,
                                                ctypes.byref(nb))
        self.lib.check(rc, nb.value if rc == ERR_BLOCK_SIZE_EXCEEDED else None)
        return out_len.value, nb.value

    def debug_snap(self, enable):
        """Snap: k_snap_chunk's phase clocks of the last batch summed over its chunks (gzpx_debug_snap), then switch them
        on (enable) or off: [cycles, crc, scan, extend, emit, scan steps, copies, bytes]."""
        sums = (ctypes.c_uint64 * 8)()
        self.lib.check(self.lib.L.gzpx_debug_snap(self.h, int(enable), sums))
        return [int(v) for v in sums]

    def debug_tokens(self, block):
        toks = np.empty(max(65536, int(self.buffer_size)), dtype=np.uint32)
        first = np.zeros(int(self.buffer_size) // 5000 + 4, dtype=np.uint32)
        n = ctypes.c_size_t(0)
        ns = ctypes.c_size_t(0)
        self.lib.check(self.lib.L.gzpx_debug_tokens(self.h, block, toks.ctypes.data, toks.size,
                                                    ctypes.byref(n), first.ctypes.data,
                                                    ctypes.byref(ns)))
        return toks[:n.value].copy(), first[:ns.value].copy()


class MultiContext:
    """gzpx_multi: one slab sharded over several devices, written out in order."""

    def __init__(self, devices, format=FORMAT_BGZF, level=1, buffer_size=None, compat=COMPAT_1_24,
                 max_slab_bytes=1 << 30, lib=None):
        self.lib = lib or load()
        cfg = GzpxConfig()
        self.lib.L.gzpx_config_default(ctypes.byref(cfg), format)
        cfg.level = level
        cfg.compat = compat
        if buffer_size is not None:
            cfg.buffer_size = buffer_size
        cfg.max_slab_bytes = max_slab_bytes
        self.buffer_size = cfg.buffer_size
        devs = (ctypes.c_int * len(devices))(*devices)
        h = ctypes.c_void_p()
        self.lib.check(self.lib.L.gzpx_multi_create(ctypes.byref(cfg), devs, len(devices), ctypes.byref(h)))
        self.h = h
        self.devices = list(devices)

    def compress_slab(self, data, mode=SLAB_LAST, return_block_sizes=False):
        a = _u8(data)
        nb_max = 1 if a.size == 0 else -(-a.size // self.buffer_size)
        cap = nb_max * (self.buffer_size + max(128, self.buffer_size // 10) + 28) + 128
        out = np.empty(cap, dtype=np.uint8)
        sizes = np.zeros(nb_max, dtype=np.uint32)
        out_len = ctypes.c_size_t(0)
        nb = ctypes.c_size_t(0)
        rc = self.lib.L.gzpx_multi_compress_slab(self.h, a.ctypes.data, a.size, int(mode), out.ctypes.data, cap,
                                                 ctypes.byref(out_len), sizes.ctypes.data, nb_max, ctypes.byref(nb))
        self.lib.check(rc, nb.value if rc == ERR_BLOCK_SIZE_EXCEEDED else None)
        res = out[:out_len.value].tobytes()
        return (res, sizes[:nb.value].copy()) if return_block_sizes else res

    def shard(self, in_len, g):
        """(offset, length) of the block range device g takes of a slab of in_len bytes."""
        off, n = ctypes.c_size_t(0), ctypes.c_size_t(0)
        self.lib.check(self.lib.L.gzpx_multi_shard(self.h, in_len, g, ctypes.byref(off), ctypes.byref(n)))
        return off.value, n.value

    def compress_slab_device(self, d_in_ptrs, in_len, d_out_ptr, out_cap, mode=SLAB_LAST, root=0, sync=True, wait_events=None):
        """Every range already on its own device (d_in_ptrs[g]); the shards are gathered device to device
        into d_out_ptr on devices[root].  Returns (out_len, block_sizes).

        Caller contract of gzpx_multi_compress_slab_device (include/gzpx.h): the ranges are COMPLETE and d_out is IDLE
        on entry -- the call takes no stream of the caller's to wait behind (it submits with GZPX_STREAM_NONE; since
        round 4 nothing is ordered behind the legacy default stream either).  `sync=True` (the default) makes that true
        for PyTorch callers, whose producers run asynchronously on torch's current stream: every device of the context
        is synchronised first.  Pass sync=False only when the inputs were produced synchronously.

        `wait_events` (round 6): the producers' own events (objects with .synchronize(): torch.cuda.Event, or anything
        else a runtime hands out) -- waited for INSTEAD of whole devices, so that what the caller has queued for slab
        k + 1 keeps running while slab k is compressed.  The full-device wait assumes that this context's device numbers
        are torch's ordinals (true when both see the same HIP_VISIBLE_DEVICES) and does nothing for producers of a
        runtime that is not torch: those callers pass their events, or synchronise themselves and say sync=False."""
        if wait_events is not None:
            for ev in wait_events:
                ev.synchronize()
            sync = False
        if sync:
            import sys
            torch = sys.modules.get("torch")  # (only callers that use torch have asynchronous producers to wait for)
            if torch is not None and torch.cuda.is_available():
                for d in sorted(set(self.devices)):
                    torch.cuda.synchronize(d)
        ptrs = (ctypes.c_void_p * len(d_in_ptrs))(*[ctypes.c_void_p(int(p) if p else None) for p in d_in_ptrs])
        nb_max = 1 if in_len == 0 else -(-in_len // self.buffer_size)
        sizes = np.zeros(nb_max, dtype=np.uint32)
        out_len = ctypes.c_size_t(0)
        nb = ctypes.c_size_t(0)
        rc = self.lib.L.gzpx_multi_compress_slab_device(self.h, ptrs, in_len, int(mode), root, d_out_ptr, out_cap,
                                                        ctypes.byref(out_len), sizes.ctypes.data, nb_max, ctypes.byref(nb))
        self.lib.check(rc, nb.value if rc == ERR_BLOCK_SIZE_EXCEEDED else None)
        return out_len.value, sizes[:nb.value].copy()

    def slab_bound(self, n):
        nb_max = 1 if n == 0 else -(-n // self.buffer_size)
        return nb_max * (self.buffer_size + max(128, self.buffer_size // 10) + 28) + 128

    def close(self):
        if getattr(self, "h", None):
            self.lib.L.gzpx_multi_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Compressor:
    """libdeflater::Compressor shape: alloc / deflate_compress / bound / free."""

    def __init__(self, level=1, compat=COMPAT_1_24, lib=None):
        self.lib = lib or load()
        self.h = self.lib.L.gzpx_alloc_compressor(level)
        if not self.h:
            raise GzpxError(ERR_COMPRESSION_LEVEL, "gzpx_alloc_compressor failed")
        self.lib.check(self.lib.L.gzpx_compressor_set_compat(self.h, compat))

    def deflate_compress(self, data, cap=None):
        a = _u8(data)
        if cap is None:
            cap = int(self.lib.L.gzpx_deflate_compress_bound(self.h, a.size))
        out = np.empty(max(cap, 1), dtype=np.uint8)
        n = self.lib.L.gzpx_deflate_compress(self.h, a.ctypes.data, a.size, out.ctypes.data, cap)
        if n == 0:
            raise GzpxError(ERR_INSUFFICIENT_SPACE, "gzpx_deflate_compress returned 0")
        return out[:n].tobytes()

    def close(self):
        if getattr(self, "h", None):
            self.lib.L.gzpx_free_compressor(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def synth_fastq_device(d_out_ptr, stream_offset, n, seed=20250927, stream=None, lib=None):
    """Fill device memory with bytes [stream_offset, stream_offset + n) of the synthetic FASTQ stream
    (BASELINE configs[3]); asynchronous on `stream`."""
    lib = lib or load()
    lib.check(lib.L.gzpx_synth_fastq_device(d_out_ptr, stream_offset, n, seed, stream))


def synth_ascii_device(d_out_ptr, stream_offset, n, seed=8, stream=None, lib=None):
    """Fill device memory with bytes [stream_offset, +n) of synth.ascii_random's stream (BASELINE configs[2])."""
    lib = lib or load()
    lib.check(lib.L.gzpx_synth_ascii_device(d_out_ptr, stream_offset, n, seed, stream))


def crc32(data, crc=0, lib=None):
    lib = lib or load()
    a = _u8(data)
    out = ctypes.c_uint32(0)
    lib.check(lib.L.gzpx_crc32_checked(crc, a.ctypes.data, a.size, ctypes.byref(out)))
    return int(out.value)


def crc32_combine(crc1, crc2, len2, lib=None):
    """Crc32::combine (src/check.rs:160-163): the CRC-32 of A || B from crc(A), crc(B), len(B)."""
    lib = lib or load()
    return int(lib.L.gzpx_crc32_combine(crc1, crc2, len2))


def adler32(data, adler=1, lib=None):
    """Adler32::update (src/check.rs:112-119) on the device."""
    lib = lib or load()
    a = _u8(data)
    out = ctypes.c_uint32(0)
    lib.check(lib.L.gzpx_adler32_checked(adler, a.ctypes.data, a.size, ctypes.byref(out)))
    return int(out.value)


def adler32_combine(adler1, adler2, len2, lib=None):
    """Adler32::combine (src/check.rs:121-127)."""
    lib = lib or load()
    return int(lib.L.gzpx_adler32_combine(adler1, adler2, len2))


class DContext:
    """gzpx_dctx: the GPU side of ParDecompress<Bgzf/Mgzip> (create_decompressor + decode_block +
    the per-block CRC check, for every block of a slab at once)."""

    def __init__(self, format=FORMAT_BGZF, device=0, lib=None):
        self.lib = lib or load()
        self.format = format
        h = ctypes.c_void_p()
        self.lib.check(self.lib.L.gzpx_dctx_create(device, format, ctypes.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.L.gzpx_dctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def scan_blocks(self, data):
        """(offsets uint64[], sizes uint32[], consumed) of the complete blocks in `data`."""
        a = _u8(data)
        nb = ctypes.c_size_t(0)
        used = ctypes.c_size_t(0)
        self.lib.check(self.lib.L.gzpx_scan_blocks(self.format, a.ctypes.data, a.size, None, None, 0,
                                                   ctypes.byref(nb), ctypes.byref(used)))
        offs = np.zeros(max(nb.value, 1), dtype=np.uint64)
        sizes = np.zeros(max(nb.value, 1), dtype=np.uint32)
        self.lib.check(self.lib.L.gzpx_scan_blocks(self.format, a.ctypes.data, a.size, offs.ctypes.data,
                                                   sizes.ctypes.data, offs.size, ctypes.byref(nb),
                                                   ctypes.byref(used)))
        return offs[:nb.value], sizes[:nb.value], used.value

    def _raise(self, rc, info):
        if rc == ERR_INVALID_CHECK:
            raise GzpxError(rc, "InvalidCheck { found: %d, expected: %d }" % (info.found, info.expected), info.block)
        raise GzpxError(rc, self.lib.strerror(rc), info.block)

    def decompress(self, data):
        """Host bytes of whole blocks in, inflated bytes out."""
        a = _u8(data)
        offs, sizes, used = self.scan_blocks(a)
        if used != a.size:
            raise GzpxError(ERR_INVALID_ARG, "trailing partial block (%d bytes)" % (a.size - used))
        isz = 0
        if offs.size:  # ISIZE fields of all blocks (little-endian u32 at the end of every member)
            ends = offs.astype(np.int64) + sizes.astype(np.int64)
            fields = a[(ends[:, None] - 4) + np.arange(4)].astype(np.uint64)
            isz = int((fields[:, 0] | (fields[:, 1] << np.uint64(8)) | (fields[:, 2] << np.uint64(16)) |
                       (fields[:, 3] << np.uint64(24))).sum())
        out = np.empty(max(isz, 1), dtype=np.uint8)
        out_len = ctypes.c_size_t(0)
        info = GzpxCheckInfo()
        rc = self.lib.L.gzpx_decompress_blocks(self.h, a.ctypes.data, a.size, offs.ctypes.data,
                                               sizes.ctypes.data, offs.size, out.ctypes.data, isz,
                                               ctypes.byref(out_len), ctypes.byref(info))
        if rc != OK:
            self._raise(rc, info)
        return out[:out_len.value].tobytes()

    def last_inflate_ms(self):
        ms = ctypes.c_float(0)
        self.lib.check(self.lib.L.gzpx_dctx_last_inflate_ms(self.h, ctypes.byref(ms)))
        return ms.value

    def last_inflate_stage_ms(self):
        """(k_inflate_seg ms, k_lzcopy + hand-backs ms) of the last launch on the decode / copy route."""
        ms = (ctypes.c_float * 2)()
        self.lib.check(self.lib.L.gzpx_dctx_last_inflate_stage_ms(self.h, ms))
        return ms[0], ms[1]

    def set_route(self, route):
        """INFLATE_SEG (default): k_inflate_seg + k_lzcopy, hand-backs to k_inflate; INFLATE_WAVE: k_inflate for every member."""
        self.lib.check(self.lib.L.gzpx_dctx_set_route(self.h, int(route)))

    def last_redo_count(self):
        """Members of the last launch that the decode / copy pair handed to k_inflate."""
        n = ctypes.c_uint32(0)
        self.lib.check(self.lib.L.gzpx_dctx_last_redo_count(self.h, ctypes.byref(n)))
        return n.value

    def debug_inflate(self, enable):
        """Switch the instrumented inflate kernels on/off; returns the counters of the last launch."""
        c = (ctypes.c_uint64 * 8)()
        self.lib.check(self.lib.L.gzpx_debug_inflate(self.h, int(enable), c))
        return list(c)

    def debug_handback(self, n):
        """HANDBACK_* of members 0 .. n - 1 of the last launch, made under debug_inflate(1): why the decode / copy pair
        handed each to k_inflate, HANDBACK_NONE for a member it decoded."""
        r = (ctypes.c_uint32 * max(n, 1))()
        self.lib.check(self.lib.L.gzpx_debug_inflate_handback(self.h, r, n))
        return list(r)[:n]

    def decompress_device(self, d_in_ptr, in_len, offsets, sizes, d_out_ptr, out_cap, stream=None):
        out_len = ctypes.c_size_t(0)
        info = GzpxCheckInfo()
        rc = self.lib.L.gzpx_decompress_blocks_device(self.h, d_in_ptr, in_len, offsets.ctypes.data,
                                                      sizes.ctypes.data, offsets.size, d_out_ptr, out_cap,
                                                      ctypes.byref(out_len), ctypes.byref(info), stream)
        if rc != OK:
            self._raise(rc, info)
        return out_len.value

    # ---- streams that lie in device memory: the members are found on the device (gzpx_mscan.h)
    def scan_blocks_device(self, d_in_ptr, in_len, max_blocks=None, want_tables=True, stream=None):
        """gzpx_scan_blocks for d_in[0..in_len) in device memory: (offsets uint64[], sizes uint32[], consumed), or
        (n_blocks, consumed) with want_tables=False.  max_blocks=None: room for every member."""
        nb = ctypes.c_size_t(0)
        used = ctypes.c_size_t(0)
        if not want_tables or max_blocks is None:
            self.lib.check(self.lib.L.gzpx_scan_blocks_device(self.h, d_in_ptr, in_len, None, None, max_blocks or 0,
                                                              ctypes.byref(nb), ctypes.byref(used), stream))
            if not want_tables:
                return nb.value, used.value
            max_blocks = nb.value
        offs = np.zeros(max(max_blocks, 1), dtype=np.uint64)
        sizes = np.zeros(max(max_blocks, 1), dtype=np.uint32)
        self.lib.check(self.lib.L.gzpx_scan_blocks_device(self.h, d_in_ptr, in_len, offs.ctypes.data, sizes.ctypes.data,
                                                          max_blocks, ctypes.byref(nb), ctypes.byref(used), stream))
        return offs[:nb.value], sizes[:nb.value], used.value

    def decompress_stream_device(self, d_in_ptr, in_len, d_out_ptr, out_cap, stream=None):
        """Scan + inflate of every complete member of d_in[0..in_len): (out_len, n_blocks, consumed)."""
        out_len, nb, used = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
        info = GzpxCheckInfo()
        rc = self.lib.L.gzpx_decompress_stream_device(self.h, d_in_ptr, in_len, d_out_ptr, out_cap, ctypes.byref(out_len),
                                                      ctypes.byref(nb), ctypes.byref(used), ctypes.byref(info), stream)
        if rc != OK:
            self._raise(rc, info)
        return out_len.value, nb.value, used.value

    def index_device(self, d_in_ptr, in_len, stream=None):
        """The block index of a stream in device memory, one row per member as a reader sees them:
        (idx[n, 2] uint64 = (compressed offset, uncompressed offset), consumed, inflated_len)."""
        n, used, total = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_uint64(0)
        self.lib.check(self.lib.L.gzpx_index_device(self.h, d_in_ptr, in_len, None, 0, ctypes.byref(n), ctypes.byref(used),
                                                    ctypes.byref(total), stream))
        idx = np.zeros((max(n.value, 1), 2), dtype=np.uint64)
        self.lib.check(self.lib.L.gzpx_index_device(self.h, d_in_ptr, in_len, idx.ctypes.data, n.value, ctypes.byref(n),
                                                    ctypes.byref(used), ctypes.byref(total), stream))
        return idx[:n.value], used.value, total.value

    def last_scan_ms(self):
        """HIP-event duration of the member-discovery kernels of the last *_device call that scanned."""
        ms = ctypes.c_float(0)
        self.lib.check(self.lib.L.gzpx_dctx_last_scan_ms(self.h, ctypes.byref(ms)))
        return ms.value

    # ---- random access by range (gzpx_ranges.h)
    def build_index_device(self, d_in_ptr, in_len, stream=None):
        """The index of d_in[0..in_len), kept in device memory: a DIndex for read_ranges_device."""
        h = ctypes.c_void_p()
        n, used, total = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_uint64(0)
        self.lib.check(self.lib.L.gzpx_dindex_build_device(self.h, d_in_ptr, in_len, ctypes.byref(h), ctypes.byref(n),
                                                           ctypes.byref(used), ctypes.byref(total), stream))
        return DIndex(self.lib, h, n.value, used.value, total.value)

    def read_ranges_device(self, index, d_in_ptr, in_len, ranges, d_out_ptr, out_cap, coords="uncompressed", stream=None):
        """ranges[n, 2] (begin, end) of the inflated stream -- or BGZF virtual offsets with coords="virtual" -- into
        d_out back to back: (out_len, out_offsets uint64[n + 1]).  Only the members the ranges touch are inflated.  A
        bad range raises GzpxError with .range_index; too small an out_cap raises it with .needed."""
        r = np.ascontiguousarray(np.asarray(ranges, dtype=np.uint64).reshape(-1, 2))
        mode = {"uncompressed": RANGE_UNCOMPRESSED, "virtual": RANGE_VIRTUAL}[coords]
        offs = np.zeros(r.shape[0] + 1, dtype=np.uint64)
        out_len, bad = ctypes.c_size_t(0), ctypes.c_size_t(0)
        info = GzpxCheckInfo()
        rc = self.lib.L.gzpx_read_ranges_device(self.h, index.h, d_in_ptr, in_len, r.ctypes.data, r.shape[0], mode,
                                                d_out_ptr, out_cap, ctypes.byref(out_len), offs.ctypes.data,
                                                ctypes.byref(bad), ctypes.byref(info), stream)
        if rc == OK:
            return out_len.value, offs
        if bad.value != ctypes.c_size_t(-1).value:
            raise GzpxError(rc, "range %d does not lie in the stream" % bad.value, range_index=bad.value)
        if rc == ERR_INSUFFICIENT_SPACE and out_len.value:
            raise GzpxError(rc, "the ranges hold %d bytes" % out_len.value, needed=out_len.value)
        if rc in (ERR_INVALID_CHECK, ERR_BAD_DATA, ERR_INSUFFICIENT_SPACE):
            self._raise(rc, info)
        raise GzpxError(rc, self.lib.strerror(rc))

    def last_ranges_members(self):
        """Members the last read_ranges_device inflated: the union of the ranges' [first, last]."""
        n = ctypes.c_size_t(0)
        self.lib.check(self.lib.L.gzpx_dctx_last_ranges_members(self.h, ctypes.byref(n)))
        return n.value

    def last_ranges_ms(self):
        """HIP-event durations of the last read_ranges_device: (locate + select, inflate, gather)."""
        ms = (ctypes.c_float * 3)()
        self.lib.check(self.lib.L.gzpx_dctx_last_ranges_ms(self.h, ms))
        return ms[0], ms[1], ms[2]

    # ---- reads by line (gzpx_lines.h)
    def build_lines_device(self, index, d_in_ptr, in_len, delim=10, stream=None):
        """The line table of the stream `index` was built from, for the delimiter byte `delim`: a DLines for
        line_offsets_device / read_lines_device.  Every member is inflated and checked once."""
        h = ctypes.c_void_p()
        d, n = ctypes.c_uint64(0), ctypes.c_uint64(0)
        info = GzpxCheckInfo()
        rc = self.lib.L.gzpx_dlines_build_device(self.h, index.h, d_in_ptr, in_len, int(delim), ctypes.byref(h), ctypes.byref(d),
                                                 ctypes.byref(n), ctypes.byref(info), stream)
        if rc in (ERR_INVALID_CHECK, ERR_BAD_DATA, ERR_INSUFFICIENT_SPACE):
            self._raise(rc, info)
        self.lib.check(rc)
        return DLines(self.lib, h, d.value, n.value)

    def line_offsets_device(self, index, lines, d_in_ptr, in_len, line_numbers, stream=None):
        """start(k) for every k of line_numbers (0 <= k <= n_lines): uint64[n], byte offsets into the inflated stream.
        Only the members that hold the boundaries' tiles are inflated.  A bad k raises GzpxError with .range_index."""
        k = np.ascontiguousarray(np.asarray(line_numbers, dtype=np.uint64).reshape(-1))
        offs = np.zeros(k.size, dtype=np.uint64)
        bad = ctypes.c_size_t(0)
        info = GzpxCheckInfo()
        rc = self.lib.L.gzpx_line_offsets_device(self.h, index.h, lines.h, d_in_ptr, in_len, k.ctypes.data, k.size,
                                                 offs.ctypes.data, ctypes.byref(bad), ctypes.byref(info), stream)
        if rc == OK:
            return offs
        if bad.value != ctypes.c_size_t(-1).value:
            raise GzpxError(rc, "line %d does not lie in the stream" % bad.value, range_index=bad.value)
        if rc in (ERR_INVALID_CHECK, ERR_BAD_DATA, ERR_INSUFFICIENT_SPACE):
            self._raise(rc, info)
        raise GzpxError(rc, self.lib.strerror(rc))

    def read_lines_device(self, index, lines, d_in_ptr, in_len, line_ranges, d_out_ptr, out_cap, stream=None):
        """line_ranges[n, 2] = [a, b) in line numbers, into d_out back to back: (out_len, out_offsets uint64[n + 1],
        byte_ranges uint64[n, 2] = what each range was in bytes of the inflated stream; an empty range is (0, 0)).  A
        bad range raises GzpxError with .range_index; too small an out_cap raises it with .needed."""
        r = np.ascontiguousarray(np.asarray(line_ranges, dtype=np.uint64).reshape(-1, 2))
        offs = np.zeros(r.shape[0] + 1, dtype=np.uint64)
        br = np.zeros((r.shape[0], 2), dtype=np.uint64)
        out_len, bad = ctypes.c_size_t(0), ctypes.c_size_t(0)
        info = GzpxCheckInfo()
        rc = self.lib.L.gzpx_read_lines_device(self.h, index.h, lines.h, d_in_ptr, in_len, r.ctypes.data, r.shape[0], d_out_ptr,
                                               out_cap, ctypes.byref(out_len), offs.ctypes.data, br.ctypes.data,
                                               ctypes.byref(bad), ctypes.byref(info), stream)
        if rc == OK:
            return out_len.value, offs, br
        if bad.value != ctypes.c_size_t(-1).value:
            raise GzpxError(rc, "line range %d does not lie in the stream" % bad.value, range_index=bad.value)
        if rc == ERR_INSUFFICIENT_SPACE and out_len.value:
            raise GzpxError(rc, "the line ranges hold %d bytes" % out_len.value, needed=out_len.value)
        if rc in (ERR_INVALID_CHECK, ERR_BAD_DATA, ERR_INSUFFICIENT_SPACE):
            self._raise(rc, info)
        raise GzpxError(rc, self.lib.strerror(rc))

    def set_lines_batch(self, inflated_bytes):
        """Inflated bytes a batch of build_lines_device and of find_device holds at most (0: the default, 256 MiB)."""
        self.lib.check(self.lib.L.gzpx_dctx_set_lines_batch(self.h, int(inflated_bytes)))

    def last_lines_members(self):
        """Members the last line_offsets_device / read_lines_device inflated: the union over the covers."""
        n = ctypes.c_size_t(0)
        self.lib.check(self.lib.L.gzpx_dctx_last_lines_members(self.h, ctypes.byref(n)))
        return n.value

    def last_lines_ms(self):
        """HIP-event durations of the last line search: (boundary tiles + locate + select, inflate, boundary search, gather)."""
        ms = (ctypes.c_float * 4)()
        self.lib.check(self.lib.L.gzpx_dctx_last_lines_ms(self.h, ms))
        return tuple(ms)

    def last_lines_build_ms(self):
        """HIP-event durations of the last build_lines_device, summed over its batches: (inflate, count)."""
        ms = (ctypes.c_float * 2)()
        self.lib.check(self.lib.L.gzpx_dctx_last_lines_build_ms(self.h, ms))
        return ms[0], ms[1]

    # ---- search (gzpx_find.h)
    def find_device(self, index, d_in_ptr, in_len, pattern, delim=None, d_positions_ptr=None, d_lines_ptr=None, hits_cap=0,
                    stream=None):
        """Every position of the inflated stream at which the bytes `pattern` start, ascending, into the device array
        d_positions_ptr (uint64[hits_cap]) and, for the delimiter byte `delim`, the line of each into d_lines_ptr; either
        may be None, both None counts only.  Returns n_hits.  More hits than hits_cap: the first hits_cap are written and
        GzpxError is raised with .needed = n_hits."""
        pat = bytes(pattern)
        n = ctypes.c_uint64(0)
        info = GzpxCheckInfo()
        rc = self.lib.L.gzpx_find_device(self.h, index.h, d_in_ptr, in_len, pat, len(pat), FIND_NO_LINES if delim is None else int(delim),
                                         d_positions_ptr, d_lines_ptr, hits_cap, ctypes.byref(n), ctypes.byref(info), stream)
        if rc == OK:
            return n.value
        if rc == ERR_INSUFFICIENT_SPACE and n.value:
            raise GzpxError(rc, "the stream holds %d hits" % n.value, needed=n.value)
        if rc in (ERR_INVALID_CHECK, ERR_BAD_DATA, ERR_INSUFFICIENT_SPACE):
            self._raise(rc, info)
        raise GzpxError(rc, self.lib.strerror(rc))

    def last_find_ms(self):
        """HIP-event durations of the last find_device, summed over its batches: (inflate, count, write)."""
        ms = (ctypes.c_float * 3)()
        self.lib.check(self.lib.L.gzpx_dctx_last_find_ms(self.h, ms))
        return ms[0], ms[1], ms[2]

    # ---- selection of lines by content (gzpx_select.h)
    def select_lines_device(self, index, lines, d_in_ptr, in_len, pattern, group=1, invert=False, d_runs_ptr=None, runs_cap=0,
                            stream=None):
        """The records of `group` lines in which a hit of `pattern` lies (invert: in which none does), as runs of
        consecutive records: line ranges (begin, end) uint64 pairs, ascending, into the device array d_runs_ptr
        (runs_cap entries; None counts only).  Returns (n_runs, n_records, n_hits).  More runs than runs_cap: the first
        runs_cap are written and GzpxError is raised with .needed = n_runs."""
        pat = bytes(pattern)
        runs, records, hits = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        info = GzpxCheckInfo()
        rc = self.lib.L.gzpx_select_lines_device(self.h, index.h, lines.h, d_in_ptr, in_len, pat, len(pat), int(group),
                                                 SELECT_INVERT if invert else 0, d_runs_ptr, runs_cap, ctypes.byref(runs),
                                                 ctypes.byref(records), ctypes.byref(hits), ctypes.byref(info), stream)
        if rc == OK:
            return runs.value, records.value, hits.value
        if rc == ERR_INSUFFICIENT_SPACE and runs.value:
            raise GzpxError(rc, "the selection has %d runs" % runs.value, needed=runs.value)
        if rc in (ERR_INVALID_CHECK, ERR_BAD_DATA, ERR_INSUFFICIENT_SPACE):
            self._raise(rc, info)
        raise GzpxError(rc, self.lib.strerror(rc))

    def last_select_ms(self):
        """HIP-event durations of the last select_lines_device: (inflate, count + scan + mark, runs); the first two summed
        over its batches."""
        ms = (ctypes.c_float * 3)()
        self.lib.check(self.lib.L.gzpx_dctx_last_select_ms(self.h, ms))
        return ms[0], ms[1], ms[2]

    # ---- search for a set of patterns (gzpx_findset.h)
    @staticmethod
    def _pattern_set(patterns):
        """A sequence of bytes-likes as the C ABI takes a set: (the bytes joined, uint32 offsets[K + 1], K)."""
        pats = [bytes(p) for p in patterns]
        offsets = (ctypes.c_uint32 * (len(pats) + 1))()
        for k, p in enumerate(pats):
            offsets[k + 1] = offsets[k] + len(p)
        return b"".join(pats), offsets, len(pats)

    def find_set_device(self, index, d_in_ptr, in_len, patterns, delim=None, d_positions_ptr=None, d_ids_ptr=None, d_lines_ptr=None,
                        hits_cap=0, d_counts_ptr=None, stream=None):
        """Every (position, k) at which pattern k of the sequence `patterns` starts, ascending by position and at one
        position by k: the positions into the device array d_positions_ptr (uint64[hits_cap]), the ids into d_ids_ptr
        (uint32[hits_cap]) and, for the delimiter byte `delim`, the lines into d_lines_ptr (uint64[hits_cap]); each may be
        None, all None counts only.  d_counts_ptr (uint64[len(patterns)], optional) receives the hits of every pattern.
        Returns n_hits.  More hits than hits_cap: the first hits_cap are written and GzpxError is raised with
        .needed = n_hits."""
        blob, offsets, k = self._pattern_set(patterns)
        n = ctypes.c_uint64(0)
        info = GzpxCheckInfo()
        rc = self.lib.L.gzpx_find_set_device(self.h, index.h, d_in_ptr, in_len, blob, offsets, k,
                                             FIND_NO_LINES if delim is None else int(delim), d_positions_ptr, d_ids_ptr, d_lines_ptr,
                                             hits_cap, d_counts_ptr, ctypes.byref(n), ctypes.byref(info), stream)
        if rc == OK:
            return n.value
        if rc == ERR_INSUFFICIENT_SPACE and n.value:
            raise GzpxError(rc, "the stream holds %d hits" % n.value, needed=n.value)
        if rc in (ERR_INVALID_CHECK, ERR_BAD_DATA, ERR_INSUFFICIENT_SPACE):
            self._raise(rc, info)
        raise GzpxError(rc, self.lib.strerror(rc))

    def last_find_set_ms(self):
        """HIP-event durations of the last find_set_device, summed over its batches: (inflate, count, write)."""
        ms = (ctypes.c_float * 3)()
        self.lib.check(self.lib.L.gzpx_dctx_last_find_set_ms(self.h, ms))
        return ms[0], ms[1], ms[2]

    def select_lines_set_device(self, index, lines, d_in_ptr, in_len, patterns, group=1, invert=False, d_runs_ptr=None,
                                runs_cap=0, stream=None):
        """select_lines_device with a hit of any pattern of the sequence `patterns` as "a hit".  Returns
        (n_runs, n_records, n_hits); timings through last_select_ms."""
        blob, offsets, k = self._pattern_set(patterns)
        runs, records, hits = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        info = GzpxCheckInfo()
        rc = self.lib.L.gzpx_select_lines_set_device(self.h, index.h, lines.h, d_in_ptr, in_len, blob, offsets, k, int(group),
                                                     SELECT_INVERT if invert else 0, d_runs_ptr, runs_cap, ctypes.byref(runs),
                                                     ctypes.byref(records), ctypes.byref(hits), ctypes.byref(info), stream)
        if rc == OK:
            return runs.value, records.value, hits.value
        if rc == ERR_INSUFFICIENT_SPACE and runs.value:
            raise GzpxError(rc, "the selection has %d runs" % runs.value, needed=runs.value)
        if rc in (ERR_INVALID_CHECK, ERR_BAD_DATA, ERR_INSUFFICIENT_SPACE):
            self._raise(rc, info)
        raise GzpxError(rc, self.lib.strerror(rc))

    def read_lines_table_device(self, index, lines, d_in_ptr, in_len, d_line_ranges_ptr, n_ranges, d_out_ptr, out_cap,
                                d_out_offsets_ptr=None, d_byte_ranges_ptr=None, stream=None):
        """read_lines_device with its tables in device memory: d_line_ranges_ptr is uint64[n_ranges, 2], and the optional
        d_out_offsets_ptr (uint64[n_ranges + 1]) and d_byte_ranges_ptr (uint64[n_ranges, 2]) are written there.  Returns
        out_len.  A bad range raises GzpxError with .range_index; too small an out_cap raises it with .needed."""
        out_len, bad = ctypes.c_size_t(0), ctypes.c_size_t(0)
        info = GzpxCheckInfo()
        rc = self.lib.L.gzpx_read_lines_table_device(self.h, index.h, lines.h, d_in_ptr, in_len, d_line_ranges_ptr, n_ranges,
                                                     d_out_ptr, out_cap, ctypes.byref(out_len), d_out_offsets_ptr,
                                                     d_byte_ranges_ptr, ctypes.byref(bad), ctypes.byref(info), stream)
        if rc == OK:
            return out_len.value
        if bad.value != ctypes.c_size_t(-1).value:
            raise GzpxError(rc, "line range %d does not lie in the stream" % bad.value, range_index=bad.value)
        if rc == ERR_INSUFFICIENT_SPACE and out_len.value:
            raise GzpxError(rc, "the line ranges hold %d bytes" % out_len.value, needed=out_len.value)
        if rc in (ERR_INVALID_CHECK, ERR_BAD_DATA, ERR_INSUFFICIENT_SPACE):
            self._raise(rc, info)
        raise GzpxError(rc, self.lib.strerror(rc))

    # ---- fields of lines (gzpx_fields.h)
    def _read_fields(self, fn, index, lines, d_in_ptr, in_len, ranges_ptr, n_ranges, field_delim, fields, complement, d_out_ptr,
                     out_cap, offsets_ptr, stream):
        f = np.ascontiguousarray(np.asarray(fields, dtype=np.uint64).reshape(-1, 2))
        out_len, bad = ctypes.c_size_t(0), ctypes.c_size_t(0)
        info = GzpxCheckInfo()
        rc = fn(self.h, index.h, lines.h, d_in_ptr, in_len, ranges_ptr, n_ranges, int(field_delim), f.ctypes.data, f.shape[0],
                FIELDS_COMPLEMENT if complement else 0, d_out_ptr, out_cap if d_out_ptr is not None else 0, ctypes.byref(out_len),
                offsets_ptr, ctypes.byref(bad), ctypes.byref(info), stream)
        if rc == OK:
            return out_len.value
        if bad.value != ctypes.c_size_t(-1).value:
            raise GzpxError(rc, "line range %d does not lie in the stream" % bad.value, range_index=bad.value)
        if rc == ERR_INSUFFICIENT_SPACE and out_len.value:
            raise GzpxError(rc, "the selected fields hold %d bytes" % out_len.value, needed=out_len.value)
        if rc in (ERR_INVALID_CHECK, ERR_BAD_DATA, ERR_INSUFFICIENT_SPACE):
            self._raise(rc, info)
        raise GzpxError(rc, self.lib.strerror(rc))

    def read_fields_device(self, index, lines, d_in_ptr, in_len, line_ranges, field_delim, fields, d_out_ptr, out_cap,
                           complement=False, stream=None):
        """cut -f on the lines of line_ranges[n, 2]: of every line the fields whose numbers (from 0) lie in `fields`, a
        sequence of [begin, end) pairs, ascending and disjoint, FIELDS_TO_END as the last end for "through the last field"
        (complement: every field that does not), joined by the byte field_delim, then the line's delimiter if it has one;
        into d_out back to back.  Returns (out_len, out_offsets uint64[n + 1]).  d_out_ptr None is the size query.  A bad
        line range raises GzpxError with .range_index; too small an out_cap raises it with .needed."""
        r = np.ascontiguousarray(np.asarray(line_ranges, dtype=np.uint64).reshape(-1, 2))
        offs = np.zeros(r.shape[0] + 1, dtype=np.uint64)
        out_len = self._read_fields(self.lib.L.gzpx_read_fields_device, index, lines, d_in_ptr, in_len, r.ctypes.data, r.shape[0],
                                    field_delim, fields, complement, d_out_ptr, out_cap, offs.ctypes.data, stream)
        return out_len, offs

    def read_fields_table_device(self, index, lines, d_in_ptr, in_len, d_line_ranges_ptr, n_ranges, field_delim, fields, d_out_ptr,
                                 out_cap, complement=False, d_out_offsets_ptr=None, stream=None):
        """read_fields_device with its tables in device memory: d_line_ranges_ptr is uint64[n_ranges, 2] (the table
        select_lines_device wrote, for one), the optional d_out_offsets_ptr uint64[n_ranges + 1].  Returns out_len."""
        return self._read_fields(self.lib.L.gzpx_read_fields_table_device, index, lines, d_in_ptr, in_len, d_line_ranges_ptr,
                                 n_ranges, field_delim, fields, complement, d_out_ptr, out_cap, d_out_offsets_ptr, stream)

    def last_fields_ms(self):
        """HIP-event durations of the last read_fields call's passes behind the search: (carry + scan, count + scan, write)."""
        ms = (ctypes.c_float * 3)()
        self.lib.check(self.lib.L.gzpx_dctx_last_fields_ms(self.h, ms))
        return ms[0], ms[1], ms[2]

    # ---- numeric columns of lines (gzpx_columns.h)
    def _read_columns(self, fn, index, lines, d_in_ptr, in_len, ranges_ptr, n_ranges, field_delim, cols, d_values_ptr, d_status_ptr,
                      rows_cap, d_col_not_ok_ptr, offsets_ptr, stream):
        cl = np.zeros(len(cols), dtype=COLUMN_DTYPE)
        for i, (field, kind) in enumerate(cols):
            cl[i] = (field, kind, 0)
        n_rows, n_not_ok, bad = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_size_t(0)
        info = GzpxCheckInfo()
        rc = fn(self.h, index.h, lines.h, d_in_ptr, in_len, ranges_ptr, n_ranges, int(field_delim), cl.ctypes.data, cl.shape[0],
                d_values_ptr, d_status_ptr, rows_cap, ctypes.byref(n_rows), ctypes.byref(n_not_ok), d_col_not_ok_ptr, offsets_ptr,
                ctypes.byref(bad), ctypes.byref(info), stream)
        if rc == OK:
            return n_rows.value, n_not_ok.value
        if bad.value != ctypes.c_size_t(-1).value:
            raise GzpxError(rc, "line range %d does not lie in the stream" % bad.value, range_index=bad.value)
        if rc == ERR_INSUFFICIENT_SPACE and n_rows.value:
            raise GzpxError(rc, "the line ranges hold %d rows" % n_rows.value, needed=n_rows.value)
        if rc in (ERR_INVALID_CHECK, ERR_BAD_DATA, ERR_INSUFFICIENT_SPACE):
            self._raise(rc, info)
        raise GzpxError(rc, self.lib.strerror(rc))

    def read_columns_device(self, index, lines, d_in_ptr, in_len, line_ranges, field_delim, cols, d_values_ptr, d_status_ptr,
                            rows_cap, d_col_not_ok_ptr=None, stream=None):
        """Numbers of the lines of line_ranges[n, 2]: `cols` is a sequence of (field number, COL_INT64 | COL_FLOAT64), the
        field numbers strictly ascending, COLUMNS_MAX at most.  Line i of range r is row row_offsets[r] + i; column c, row i is
        the 8-byte cell d_values[c * rows_cap + i] (int64 / float64) with its CELL_* byte at d_status[c * rows_cap + i].
        Either pointer may be None; with both None the call only counts.  d_col_not_ok_ptr: an optional device array
        uint64[len(cols)].  Returns (n_rows, n_not_ok, row_offsets uint64[n + 1]).  A bad line range raises GzpxError with
        .range_index; more rows than rows_cap raises it with .needed."""
        r = np.ascontiguousarray(np.asarray(line_ranges, dtype=np.uint64).reshape(-1, 2))
        offs = np.zeros(r.shape[0] + 1, dtype=np.uint64)
        n_rows, n_not_ok = self._read_columns(self.lib.L.gzpx_read_columns_device, index, lines, d_in_ptr, in_len, r.ctypes.data,
                                              r.shape[0], field_delim, cols, d_values_ptr, d_status_ptr, rows_cap, d_col_not_ok_ptr,
                                              offs.ctypes.data, stream)
        return n_rows, n_not_ok, offs

    def read_columns_table_device(self, index, lines, d_in_ptr, in_len, d_line_ranges_ptr, n_ranges, field_delim, cols, d_values_ptr,
                                  d_status_ptr, rows_cap, d_col_not_ok_ptr=None, d_row_offsets_ptr=None, stream=None):
        """read_columns_device with its tables in device memory: d_line_ranges_ptr is uint64[n_ranges, 2] (the table
        select_lines_device wrote, for one), the optional d_row_offsets_ptr uint64[n_ranges + 1].  Returns (n_rows, n_not_ok,
        d_row_offsets_ptr): the third is the device array that was given."""
        n_rows, n_not_ok = self._read_columns(self.lib.L.gzpx_read_columns_table_device, index, lines, d_in_ptr, in_len,
                                              d_line_ranges_ptr, n_ranges, field_delim, cols, d_values_ptr, d_status_ptr, rows_cap,
                                              d_col_not_ok_ptr, d_row_offsets_ptr, stream)
        return n_rows, n_not_ok, d_row_offsets_ptr

    def last_columns_ms(self):
        """HIP-event durations of the last read_columns call's stages behind the search: (carries + row scan, parse)."""
        ms = (ctypes.c_float * 2)()
        self.lib.check(self.lib.L.gzpx_dctx_last_columns_ms(self.h, ms))
        return ms[0], ms[1]

    # ---- selection of lines by their numbers (gzpx_where.h)
    @staticmethod
    def where_terms(terms):
        """`terms` as gzpx_where_term records: (field, COL_*, WHERE_*, value), the value a Python int or float packed by the type."""
        tm = np.zeros(len(terms), dtype=WHERE_TERM_DTYPE)
        for i, (field, kind, op, value) in enumerate(terms):
            bits = struct.unpack("<Q", struct.pack("<d", float(value)) if kind == COL_FLOAT64 else struct.pack("<q", int(value)))[0]
            tm[i] = (field, kind, op, bits)
        return tm

    @staticmethod
    def where_text_terms(terms):
        """`terms` as (gzpx_where_term records, the pool of constants): (field, COL_*, WHERE_*, value), the value of a COL_TEXT
        term a bytes object (None or b"" for IS_OK / NOT_OK), of the others as for where_terms.  A constant that the pool
        already holds is not added again."""
        tm = np.zeros(len(terms), dtype=WHERE_TERM_DTYPE)
        pool = bytearray()
        for i, (field, kind, op, value) in enumerate(terms):
            if kind != COL_TEXT:
                tm[i] = DContext.where_terms([(field, kind, op, value)])[0]
            elif op in (WHERE_IS_OK, WHERE_NOT_OK):
                if value:
                    raise ValueError("IS_OK and NOT_OK take no constant")
                tm[i] = (field, kind, op, 0)
            else:
                value = bytes(value)
                at = pool.find(value)
                if at < 0:
                    at = len(pool)
                    pool += value
                tm[i] = (field, kind, op, at | len(value) << 32)
        return tm, bytes(pool)

    def _where_lines(self, fn, index, lines, d_in_ptr, in_len, ranges_ptr, n_ranges, field_delim, terms, any, invert, d_runs_ptr,
                     runs_cap, stream, text=False):
        if text:
            tm, pool = self.where_text_terms(terms)
            extra = (pool if pool else None, len(pool))
        else:
            tm, extra = self.where_terms(terms), ()
        runs, selected, rows, not_ok, bad = (ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0),
                                             ctypes.c_size_t(0))
        info = GzpxCheckInfo()
        rc = fn(self.h, index.h, lines.h, d_in_ptr, in_len, ranges_ptr, n_ranges, int(field_delim), tm.ctypes.data, tm.shape[0], *extra,
                (WHERE_ANY if any else 0) | (WHERE_INVERT if invert else 0), d_runs_ptr, runs_cap, ctypes.byref(runs),
                ctypes.byref(selected), ctypes.byref(rows), ctypes.byref(not_ok), ctypes.byref(bad), ctypes.byref(info), stream)
        if rc == OK:
            return runs.value, selected.value, rows.value, not_ok.value
        if bad.value != ctypes.c_size_t(-1).value:
            raise GzpxError(rc, "line range %d does not lie in the stream" % bad.value, range_index=bad.value)
        if rc == ERR_INSUFFICIENT_SPACE and runs.value:
            raise GzpxError(rc, "the selection has %d runs" % runs.value, needed=runs.value)
        if rc in (ERR_INVALID_CHECK, ERR_BAD_DATA, ERR_INSUFFICIENT_SPACE):
            self._raise(rc, info)
        raise GzpxError(rc, self.lib.strerror(rc))

    def where_lines_device(self, index, lines, d_in_ptr, in_len, line_ranges, field_delim, terms, any=False, invert=False,
                           d_runs_ptr=None, runs_cap=0, stream=None):
        """The lines of line_ranges[n, 2] whose numbers pass a predicate: `terms` is a sequence of (field number, COL_INT64 |
        COL_FLOAT64, WHERE_*, value), the field numbers non-descending, WHERE_MAX_TERMS at most on COLUMNS_MAX distinct
        fields.  A row passes when all terms hold (any: when one does); invert selects the rows that do not pass.  The
        selected rows as runs of consecutive rows of one range: line ranges (begin, end) uint64 pairs, in row order, into
        the device array d_runs_ptr (runs_cap entries; None counts only).  Returns (n_runs, n_selected, n_rows, n_not_ok).
        A bad line range raises GzpxError with .range_index; more runs than runs_cap: the first runs_cap are written and
        GzpxError is raised with .needed = n_runs."""
        r = np.ascontiguousarray(np.asarray(line_ranges, dtype=np.uint64).reshape(-1, 2))
        return self._where_lines(self.lib.L.gzpx_where_lines_device, index, lines, d_in_ptr, in_len, r.ctypes.data, r.shape[0],
                                 field_delim, terms, any, invert, d_runs_ptr, runs_cap, stream)

    def where_lines_table_device(self, index, lines, d_in_ptr, in_len, d_line_ranges_ptr, n_ranges, field_delim, terms, any=False,
                                 invert=False, d_runs_ptr=None, runs_cap=0, stream=None):
        """where_lines_device with its line ranges in device memory: d_line_ranges_ptr is uint64[n_ranges, 2] (the table
        select_lines_device wrote, for one)."""
        return self._where_lines(self.lib.L.gzpx_where_lines_table_device, index, lines, d_in_ptr, in_len, d_line_ranges_ptr,
                                 n_ranges, field_delim, terms, any, invert, d_runs_ptr, runs_cap, stream)

    def where_text_device(self, index, lines, d_in_ptr, in_len, line_ranges, field_delim, terms, any=False, invert=False,
                          d_runs_ptr=None, runs_cap=0, stream=None):
        """where_lines_device with terms on the TEXT of fields as well: a term may be (field number, COL_TEXT, WHERE_* |
        WHERE_PREFIX | WHERE_NOT_PREFIX, bytes of at most WHERE_TEXT_MAX), compared with the field's bytes as Python
        compares bytes; a field that the line does not have fails every op but WHERE_NOT_OK.  awk '$1 == "chr7" && $7 ==
        "PASS" && $6 >= 30' is [(0, COL_TEXT, WHERE_EQ, b"chr7"), (5, COL_FLOAT64, WHERE_GE, 30.0), (6, COL_TEXT, WHERE_EQ,
        b"PASS")].  Everything else, the return value and the errors are where_lines_device's."""
        r = np.ascontiguousarray(np.asarray(line_ranges, dtype=np.uint64).reshape(-1, 2))
        return self._where_lines(self.lib.L.gzpx_where_text_device, index, lines, d_in_ptr, in_len, r.ctypes.data, r.shape[0],
                                 field_delim, terms, any, invert, d_runs_ptr, runs_cap, stream, text=True)

    def where_text_table_device(self, index, lines, d_in_ptr, in_len, d_line_ranges_ptr, n_ranges, field_delim, terms, any=False,
                                invert=False, d_runs_ptr=None, runs_cap=0, stream=None):
        """where_text_device with its line ranges in device memory, as where_lines_table_device: "CHROM in {a, b, c} and QUAL
        >= 30" is an `any` call on CHROM whose table this call takes with the term on QUAL."""
        return self._where_lines(self.lib.L.gzpx_where_text_table_device, index, lines, d_in_ptr, in_len, d_line_ranges_ptr,
                                 n_ranges, field_delim, terms, any, invert, d_runs_ptr, runs_cap, stream, text=True)

    def last_where_ms(self):
        """HIP-event durations of the last where_lines call's stages behind the search: (carries + row scan, parse with the
        predicate, runs)."""
        ms = (ctypes.c_float * 3)()
        self.lib.check(self.lib.L.gzpx_dctx_last_where_ms(self.h, ms))
        return ms[0], ms[1], ms[2]

    # ---- batches of raw / zlib / gzip members that lie in device memory (gzpx_wrap.h)
    def inflate_batch_device(self, wrap, d_in_ptr, in_len, d_in_offsets_ptr, d_in_sizes_ptr, d_out_sizes_ptr, n, d_out_ptr,
                             out_cap, d_out_offsets_ptr=None, d_results_ptr=None, short_ok=False, stream=None,
                             raise_on_member_error=True):
        """n independent members in the wrapper `wrap` (WRAP_RAW / WRAP_ZLIB / WRAP_GZIP), member i at
        d_in[offsets[i], offsets[i] + sizes[i]), inflated into slots of out_sizes[i] bytes back to back in d_out.  Every
        table is a DEVICE array (offsets uint64, sizes uint32; d_out_sizes_ptr may be None for WRAP_GZIP: the trailers'
        ISIZE); d_out_offsets_ptr (uint64[n + 1]) and d_results_ptr (GzpxMemberResult[n]) are optional and written.
        short_ok: out_sizes are capacities (RAW, ZLIB; the one-wave-per-member route).  Returns (out_len, n_failed);
        a failing member raises GzpxError with block= the first one's index, unless raise_on_member_error=False:
        then (out_len, n_failed, first_failed) with first_failed None when every member is good."""
        out_len, n_failed = ctypes.c_size_t(0), ctypes.c_size_t(0)
        info = GzpxCheckInfo()
        rc = self.lib.L.gzpx_inflate_batch_device(self.h, int(wrap), BATCH_SHORT_OK if short_ok else 0, d_in_ptr, in_len,
                                                  d_in_offsets_ptr, d_in_sizes_ptr, d_out_sizes_ptr, n, d_out_ptr, out_cap,
                                                  d_out_offsets_ptr, d_results_ptr, ctypes.byref(out_len),
                                                  ctypes.byref(n_failed), ctypes.byref(info), stream)
        if n_failed.value == 0:
            if rc != OK:  # the call itself was refused, or the device failed
                raise GzpxError(rc, self.lib.strerror(rc))
            return (out_len.value, 0) if raise_on_member_error else (out_len.value, 0, None)
        if raise_on_member_error:
            self._raise(rc, info)
        return out_len.value, n_failed.value, info.block

    def inflate_batch_sizes_device(self, wrap, d_in_ptr, in_len, d_in_offsets_ptr, d_in_sizes_ptr, n, d_out_sizes_ptr,
                                   d_in_used_ptr=None, d_results_ptr=None, max_out_size=0, stream=None,
                                   raise_on_member_error=True):
        """The size query in front of inflate_batch_device: what each of n members inflates to (d_out_sizes_ptr,
        uint32[n], written) and how long it is (d_in_used_ptr, uint32[n], optional), with d_in_sizes as UPPER BOUNDS;
        nothing is inflated and no check is verified.  max_out_size caps a member's output (0: 2^32 - 1).  Returns
        (total_out, n_failed); a failing member raises GzpxError with block= the first one's index, unless
        raise_on_member_error=False: then (total_out, n_failed, first_failed)."""
        total, n_failed = ctypes.c_uint64(0), ctypes.c_size_t(0)
        info = GzpxCheckInfo()
        rc = self.lib.L.gzpx_inflate_batch_sizes_device(self.h, int(wrap), d_in_ptr, in_len, d_in_offsets_ptr, d_in_sizes_ptr, n,
                                                        int(max_out_size), d_out_sizes_ptr, d_in_used_ptr, d_results_ptr,
                                                        ctypes.byref(total), ctypes.byref(n_failed), ctypes.byref(info), stream)
        if n_failed.value == 0:
            if rc != OK:  # the call itself was refused, or the device failed
                raise GzpxError(rc, self.lib.strerror(rc))
            return (total.value, 0) if raise_on_member_error else (total.value, 0, None)
        if raise_on_member_error:
            self._raise(rc, info)
        return total.value, n_failed.value, info.block

    # ---- checksums of a table of buffers that lie in device memory (gzpx_cksum.h)
    def checksum_batch_device(self, kind, d_in_ptr, in_len, d_offsets_ptr, d_sizes_ptr, n, d_sums_ptr=None, d_seeds_ptr=None,
                              d_expected_ptr=None, d_results_ptr=None, stream=None, raise_on_entry_error=True):
        """CRC-32 / Adler-32 / CRC-32C (kind: CHECK_CRC32 / CHECK_ADLER32 / CHECK_CRC32C) of n entries of d_in, entry i at
        d_in[offsets[i], offsets[i] + sizes[i]) -- or, with d_sizes_ptr None, d_in[offsets[i], offsets[i + 1]): the
        d_out_offsets array (n + 1 entries) of inflate_batch_device as it is.  Every table is a DEVICE array (offsets
        uint64, the others uint32); d_sums_ptr is written, d_seeds_ptr gives running values (zlib's second argument),
        d_expected_ptr makes the call verify (d_sums_ptr may then be None), d_results_ptr (GzpxMemberResult[n]) is
        written.  Returns (n_failed, info) with info None when every entry is good; a failing entry raises GzpxError
        with block= the first one's index, unless raise_on_entry_error=False: then info is its GzpxCheckInfo."""
        n_failed = ctypes.c_size_t(0)
        info = GzpxCheckInfo()
        rc = self.lib.L.gzpx_checksum_batch_device(self.h, int(kind), d_in_ptr, in_len, d_offsets_ptr, d_sizes_ptr, n,
                                                   d_seeds_ptr, d_expected_ptr, d_sums_ptr, d_results_ptr,
                                                   ctypes.byref(n_failed), ctypes.byref(info), stream)
        if n_failed.value == 0:
            if rc != OK:  # the call itself was refused, or the device failed
                raise GzpxError(rc, self.lib.strerror(rc))
            return 0, None
        if raise_on_entry_error:
            if rc == ERR_INVALID_CHECK:
                self._raise(rc, info)
            raise GzpxError(rc, self.lib.strerror(rc), block=info.block)
        return n_failed.value, info

    def set_checksum_width(self, workgroups):
        """Diagnostics: the persistent workgroups of checksum_batch_device's tile kernel (0: the default)."""
        self.lib.check(self.lib.L.gzpx_dctx_set_checksum_width(self.h, int(workgroups)))

    def last_check_ms(self):
        """HIP-event duration of the check kernel (Adler-32 / CRC-32) of the last inflate_batch_device."""
        ms = ctypes.c_float(0)
        self.lib.check(self.lib.L.gzpx_dctx_last_check_ms(self.h, ctypes.byref(ms)))
        return ms.value


class DIndex:
    """gzpx_dindex: the member index of a device-resident stream, in device memory (DContext.build_index_device)."""

    def __init__(self, lib, h, n_members, consumed, inflated_len):
        self.lib, self.h = lib, h
        self.n_members, self.consumed, self.inflated_len = n_members, consumed, inflated_len

    def entries(self):
        """idx[n, 2] uint64 = (compressed offset, uncompressed offset), as DContext.index_device returns."""
        n = ctypes.c_size_t(0)
        idx = np.zeros((max(self.n_members, 1), 2), dtype=np.uint64)
        self.lib.check(self.lib.L.gzpx_dindex_entries(self.h, idx.ctypes.data, self.n_members, ctypes.byref(n)))
        return idx[:n.value]

    def close(self):
        if getattr(self, "h", None):
            self.lib.L.gzpx_dindex_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class DLines:
    """gzpx_dlines: the line table of a device-resident stream, in device memory (DContext.build_lines_device)."""

    def __init__(self, lib, h, n_delims, n_lines):
        self.lib, self.h = lib, h
        self.n_delims, self.n_lines = n_delims, n_lines

    def prefix(self):
        """P: uint64[tiles + 1], the delimiters in front of every tile of LINES_TILE inflated bytes; P[-1] = n_delims."""
        n = ctypes.c_size_t(0)
        self.lib.check(self.lib.L.gzpx_dlines_prefix(self.h, None, 0, ctypes.byref(n)))
        p = np.zeros(n.value, dtype=np.uint64)
        self.lib.check(self.lib.L.gzpx_dlines_prefix(self.h, p.ctypes.data, p.size, ctypes.byref(n)))
        return p

    def close(self):
        if getattr(self, "h", None):
            self.lib.L.gzpx_dlines_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class Decompressor:
    """libdeflater::Decompressor shape: deflate_decompress(raw, out_size)."""

    def __init__(self, lib=None):
        self.lib = lib or load()
        self.h = self.lib.L.gzpx_alloc_decompressor()

    def deflate_decompress(self, data, out_size):
        a = _u8(data)
        out = np.empty(max(out_size, 1), dtype=np.uint8)
        actual = ctypes.c_size_t(0)
        rc = self.lib.L.gzpx_deflate_decompress(self.h, a.ctypes.data, a.size, out.ctypes.data, out_size,
                                                ctypes.byref(actual))
        self.lib.check(rc)
        return out[:actual.value].tobytes()

    def close(self):
        if getattr(self, "h", None):
            self.lib.L.gzpx_free_decompressor(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
