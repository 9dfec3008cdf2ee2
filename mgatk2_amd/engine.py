"""ctypes binding of libmgpileup.so (include/mgpileup.h).

This is the only way the package reaches the GPU: there is no CPU fallback.
If the library is missing or no HIP device is present, :class:`Engine` raises.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from pathlib import Path

import numpy as np

from .exceptions import BAMFormatError, BAMReadError, InvalidInputError, ProcessingError
from .synth import ReadSoA

import os

# MGP_LIB selects an alternative build of the same engine (A/B experiments only)
LIB_PATH = Path(os.environ.get("MGP_LIB") or Path(__file__).resolve().parent / "_lib" / "libmgpileup.so")

MGP_OK = 0
MGP_E_INVALID = -1
MGP_E_HIP = -2
MGP_E_OOM = -3
MGP_E_UNSORTED = -4
MGP_E_BADREAD = -5
MGP_E_SPAN = -6
MGP_E_STATE = -7
MGP_E_COMM = -8

DEDUP_MODES = {"none": 0, "alignment_start": 1, "alignment_and_fragment_length": 2}

# names of every entry point declared in include/mgpileup.h
ABI_SYMBOLS = (
    "mgp_abi_version", "mgp_last_error", "mgp_device_count", "mgp_open", "mgp_close", "mgp_host_alloc",
    "mgp_host_free", "mgp_push_batch", "mgp_reset", "mgp_resident", "mgp_run", "mgp_sync", "mgp_fetch",
    "mgp_finish", "mgp_kernel_times", "mgp_comm_unique_id", "mgp_comm_init", "mgp_synth_generate",
    "mgp_download_inputs", "mgp_set_stage_timing", "mgp_fetch_cells", "mgp_fetch_rows16", "mgp_windows",
    "mgp_stream_info", "mgp_set_streaming", "mgp_set_rows16_target", "mgp_copy_wait", "mgp_set_cell_range",
    "mgp_push_batch16", "mgp_txt_gz_run", "mgp_txt_gz_fetch", "mgp_txt_gz_rows", "mgp_set_rows_target",
    "mgp_h5_tiles_run", "mgp_h5_tiles_fetch", "mgp_h5_tiles_rows", "mgp_variant_moments_run", "mgp_variant_dev2_run",
    "mgp_allele_freq_run", "mgp_variant_moments_rows", "mgp_variant_dev2_rows", "mgp_allele_freq_rows",
    "mgp_cell_coverage_run", "mgp_position_coverage_run", "mgp_position_depth_hist_run",
    "mgp_position_depth_next_run", "mgp_cell_coverage_rows", "mgp_position_coverage_rows",
    "mgp_position_depth_hist_rows", "mgp_position_depth_next_rows", "mgp_pair_dist", "mgp_hclust_dist", "mgp_hclust",
    "mgp_knn", "mgp_snn", "mgp_louvain", "mgp_bgzf_inflate", "mgp_inflater_create", "mgp_inflater_destroy",
    "mgp_inflater_run", "mgp_inflater_host_alloc", "mgp_inflater_host_release", "mgp_inflater_times",
    "mgp_zlib_inflate", "mgp_open_table", "mgp_table_load", "mgp_table_load_planes", "mgp_table_check",
    "mgp_table_ready", "mgp_group_moments_run", "mgp_rows_group_moments", "mgp_rank_sums", "mgp_pca", "mgp_sym_eig",
)
ABI_VERSION = 7
CFG_KEEP_TN5 = 0x1
CFG_STREAM = 0x2


class mgp_config(C.Structure):
    _fields_ = [
        ("min_baseq", C.c_int32),
        ("min_mapq", C.c_int32),
        ("min_dist_from_end", C.c_int32),
        ("dedup_mode", C.c_int32),
        ("max_strand_bias", C.c_double),
        ("min_reads", C.c_int32),
        ("n_cells", C.c_int32),
        ("mito_len", C.c_int32),
        ("flags", C.c_int32),
        ("reserve_reads", C.c_int64),
        ("reserve_payload", C.c_int64),
    ]


class mgp_batch16(C.Structure):
    _fields_ = [
        ("n_reads", C.c_int64),
        ("bc", C.c_void_p),
        ("abs_tlen", C.c_void_p),
        ("flag", C.c_void_p),
        ("mapq", C.c_void_p),
        ("payload", C.c_void_p),
        ("payload_bytes", C.c_int64),
    ]


class mgp_batch(C.Structure):
    _fields_ = [
        ("n_reads", C.c_int64),
        ("start", C.c_void_p),
        ("bc", C.c_void_p),
        ("tlen", C.c_void_p),
        ("flag", C.c_void_p),
        ("mapq", C.c_void_p),
        ("span", C.c_void_p),
        ("rec_off", C.c_void_p),
        ("payload", C.c_void_p),
        ("payload_bytes", C.c_int64),
    ]


class mgp_stats(C.Structure):
    _fields_ = [
        ("total_reads", C.c_int64),
        ("filtered_reads", C.c_int64),
        ("n_barcodes", C.c_int64),
        ("duplicate_reads_with_length", C.c_int64),
        ("duplicate_reads_position_only", C.c_int64),
        ("cells_passed", C.c_int64),
        ("max_span", C.c_int32),
        ("error_bits", C.c_int32),
    ]

    def as_dict(self) -> dict:
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class mgp_result(C.Structure):
    _fields_ = [
        ("counts", C.c_void_p),
        ("tn5", C.c_void_p),
        ("depth", C.c_void_p),
        ("n_reads", C.c_void_p),
        ("any_paired", C.c_void_p),
        ("passed", C.c_void_p),
        ("covered", C.c_void_p),
        ("depth_sum", C.c_void_p),
        ("depth_max", C.c_void_p),
        ("median_lo", C.c_void_p),
        ("median_hi", C.c_void_p),
        ("first_read", C.c_void_p),
        ("ref_tally", C.c_void_p),
        ("stats", C.POINTER(mgp_stats)),
    ]


class mgp_synth_params(C.Structure):
    _fields_ = [
        ("seed", C.c_uint64),
        ("n_reads", C.c_int64),
        ("read_len", C.c_int32),
        ("n_cells", C.c_int32),
        ("cell_cdf", C.c_void_p),
        ("ref_codes", C.c_void_p),
        ("rec_align", C.c_int32),
        ("pack", C.c_int32),
        ("rec_off", C.c_void_p),
        ("payload_bytes", C.c_int64),
        ("cell_lo", C.c_int32),
        ("cell_hi", C.c_int32),
        ("shard_rank", C.c_int32),
        ("shard_world", C.c_int32),
        ("pack_min_baseq", C.c_int32),
        ("pack_min_dist", C.c_int32),
        ("n_rec_off", C.c_int64),
    ]


class mgp_txt_gz(C.Structure):
    _fields_ = [
        ("n_cells", C.c_int64),
        ("cells", C.c_void_p),
        ("names", C.c_void_p),
        ("name_off", C.c_void_p),
        ("member_bytes", C.c_void_p),
        ("text_bytes", C.c_void_p),
    ]


class mgp_h5_tiles(C.Structure):
    _fields_ = [
        ("n_cols", C.c_int64),
        ("cell_of_col", C.c_void_p),
        ("chunk_rows", C.c_int32),
        ("chunk_cols", C.c_int32),
        ("col_chunk_lo", C.c_int32),
        ("col_chunk_hi", C.c_int32),
        ("chunk_bytes", C.c_void_p),
        ("col_sums", C.c_void_p),
    ]


class mgp_variant_job(C.Structure):
    _fields_ = [
        ("n_cells", C.c_int64),
        ("cells", C.c_void_p),
        ("low_coverage_threshold", C.c_int32),
    ]


# the arrays of mgp_variant_moments, in its order: uint64 [L, 4] except s_cov and n_low
# (uint64 [L]) and s_af (float64 [L, 4])
MOMENT_FIELDS = ("n_det", "n_conf", "s_total", "s_cov", "m", "sf", "sr", "sff", "srr", "sfr", "n_low", "s_af")
MOMENT_PER_POS = ("s_cov", "n_low")


class mgp_variant_moments(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in MOMENT_FIELDS]


# the arrays of mgp_group_moments, in its order, with their dtypes: [n_groups, L, 4] except cov ([n_groups, L])
GROUP_FIELDS = (("fwd", np.uint64), ("rev", np.uint64), ("cov", np.uint64), ("n_det", np.uint32), ("n_conf", np.uint32))
GROUP_MAX_GROUPS = 256  # groups of one mgp_group_moments call (MGP_GROUP_MAX_GROUPS)


class mgp_group_moments(C.Structure):
    _fields_ = [(k, C.c_void_p) for k, _ in GROUP_FIELDS]


# the arrays of mgp_cell_coverage ([n_cells]) and mgp_position_coverage ([L]; tally [L, 4]),
# in their order, with their dtypes
CELL_COVERAGE_FIELDS = (("s_depth", np.uint64), ("s_depth2", np.uint64), ("max_depth", np.uint32),
                        ("n_covered", np.uint32), ("n_10x", np.uint32), ("n_50x", np.uint32), ("mid_lo", np.uint32),
                        ("mid_hi", np.uint32))
POSITION_COVERAGE_FIELDS = (("s_depth", np.uint64), ("s_depth2", np.uint64), ("s_fwd", np.uint64), ("s_rev", np.uint64),
                            ("s_tn5_fwd", np.uint64), ("s_tn5_rev", np.uint64), ("tally", np.uint64),
                            ("n_covered", np.uint32), ("n_10x", np.uint32), ("n_50x", np.uint32), ("n_tn5", np.uint32),
                            ("max_depth", np.uint32))


class mgp_cell_coverage(C.Structure):
    _fields_ = [(k, C.c_void_p) for k, _ in CELL_COVERAGE_FIELDS]


class mgp_position_coverage(C.Structure):
    _fields_ = [(k, C.c_void_p) for k, _ in POSITION_COVERAGE_FIELDS]


H5_PLANES = ("A_fwd", "A_rev", "C_fwd", "C_rev", "G_fwd", "G_rev", "T_fwd", "T_rev", "tn5_cuts_fwd", "tn5_cuts_rev",
             "coverage")  # the planes of mgp_h5_tiles, in its order


class mgp_table_chunks(C.Structure):
    _fields_ = [
        ("n_cols", C.c_int64),
        ("chunk_rows", C.c_int32),
        ("chunk_cols", C.c_int32),
        ("col_chunk_lo", C.c_int32),
        ("col_chunk_hi", C.c_int32),
        ("first_cell", C.c_int32),
        ("reserved", C.c_int32),
        ("src", C.c_void_p),
        ("src_bytes", C.c_int64),
        ("chunk_bytes", C.c_void_p),
        ("raw", C.c_void_p),
        ("n_saturated", C.c_int64),
        ("ms", C.c_double * 3),
    ]


CHUNK_ZLIB, CHUNK_RAW, CHUNK_ABSENT = 0, 1, 2  # mgp_table_chunks.raw


class mgp_rows16(C.Structure):
    _fields_ = [
        ("counts", C.c_void_p),
        ("tn5", C.c_void_p),
        ("depth", C.c_void_p),
        ("wide", C.c_void_p),
    ]


class mgp_rows8(C.Structure):
    _fields_ = [
        ("counts", C.c_void_p),
        ("tn5", C.c_void_p),
        ("depth", C.c_void_p),
        ("narrow", C.c_void_p),
    ]


_lib = None


def load_library(path: Path | None = None) -> C.CDLL:
    """Load libmgpileup.so; raises if it is absent (no fallback)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = Path(path) if path else LIB_PATH
    if not p.exists():
        raise ProcessingError(
            f"HIP engine library not found at {p}; build it with `python -m mgatk2_amd.build` "
            "(hipcc --offload-arch=gfx950)"
        )
    lib = C.CDLL(str(p))
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    sig = {
        "mgp_abi_version": ([], C.c_int),
        "mgp_last_error": ([], C.c_char_p),
        "mgp_device_count": ([C.POINTER(C.c_int)], C.c_int),
        "mgp_open": ([C.POINTER(mgp_config), C.c_int, C.POINTER(vp)], C.c_int),
        "mgp_close": ([vp], None),
        "mgp_host_alloc": ([i64, C.POINTER(vp)], C.c_int),
        "mgp_host_free": ([vp], C.c_int),
        "mgp_push_batch": ([vp, C.POINTER(mgp_batch)], C.c_int),
        "mgp_push_batch16": ([vp, C.POINTER(mgp_batch16)], C.c_int),
        "mgp_reset": ([vp], C.c_int),
        "mgp_resident": ([vp, C.POINTER(i64), C.POINTER(i64)], C.c_int),
        "mgp_run": ([vp], C.c_int),
        "mgp_sync": ([vp], C.c_int),
        "mgp_fetch": ([vp, C.POINTER(mgp_result)], C.c_int),
        "mgp_finish": ([vp, C.POINTER(mgp_result)], C.c_int),
        "mgp_kernel_times": (
            [vp, C.c_int, C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_int), C.c_char_p, C.c_int], C.c_int
        ),
        "mgp_set_stage_timing": ([vp, C.c_int], C.c_int),
        "mgp_comm_unique_id": ([C.c_char_p], C.c_int),
        "mgp_comm_init": ([vp, C.c_char_p, C.c_int, C.c_int], C.c_int),
        "mgp_synth_generate": ([vp, C.POINTER(mgp_synth_params)], C.c_int),
        "mgp_download_inputs": ([vp] + [vp] * 8, C.c_int),
        "mgp_fetch_cells": ([vp, i32, i32, C.POINTER(mgp_result)], C.c_int),
        "mgp_fetch_rows16": ([vp, i32, i32, C.POINTER(mgp_rows16)], C.c_int),
        "mgp_set_rows16_target": ([vp, C.POINTER(mgp_rows16)], C.c_int),
        "mgp_set_rows_target": ([vp, C.POINTER(mgp_rows16), C.POINTER(mgp_rows8)], C.c_int),
        "mgp_windows": ([vp, C.POINTER(i32), C.POINTER(i32)], C.c_int),
        "mgp_stream_info": ([vp, C.POINTER(i64), C.POINTER(i32)], C.c_int),
        "mgp_set_streaming": ([vp, C.c_int], C.c_int),
        "mgp_set_cell_range": ([vp, C.c_int32, C.c_int32], C.c_int),
        "mgp_copy_wait": ([vp], C.c_int),
        "mgp_txt_gz_run": ([vp, C.POINTER(mgp_txt_gz), C.POINTER(i64)], C.c_int),
        "mgp_h5_tiles_run": ([vp, C.POINTER(mgp_h5_tiles), C.POINTER(i64)], C.c_int),
        "mgp_h5_tiles_fetch": ([vp, vp, i64], C.c_int),
        "mgp_txt_gz_fetch": ([vp, vp, i64], C.c_int),
        "mgp_h5_tiles_rows": (
            [C.c_int, vp, vp, vp, i32, i32, C.POINTER(mgp_h5_tiles), vp, i64, C.POINTER(i64)], C.c_int
        ),
        "mgp_txt_gz_rows": ([C.c_int, vp, vp, i32, i32, C.POINTER(mgp_txt_gz), vp, i64, C.POINTER(i64)], C.c_int),
        "mgp_variant_moments_run": ([vp, C.POINTER(mgp_variant_job), C.POINTER(mgp_variant_moments)], C.c_int),
        "mgp_variant_dev2_run": ([vp, C.POINTER(mgp_variant_job), vp, vp], C.c_int),
        "mgp_allele_freq_run": ([vp, C.POINTER(mgp_variant_job), i64, vp, vp, i32, vp], C.c_int),
        "mgp_variant_moments_rows": (
            [C.c_int, vp, vp, i32, i32, C.POINTER(mgp_variant_job), C.POINTER(mgp_variant_moments)], C.c_int
        ),
        "mgp_variant_dev2_rows": ([C.c_int, vp, vp, i32, i32, C.POINTER(mgp_variant_job), vp, vp], C.c_int),
        "mgp_allele_freq_rows": (
            [C.c_int, vp, vp, i32, i32, C.POINTER(mgp_variant_job), i64, vp, vp, i32, vp], C.c_int
        ),
        "mgp_group_moments_run": (
            [vp, C.POINTER(mgp_variant_job), vp, i32, i32, C.POINTER(mgp_group_moments)], C.c_int
        ),
        "mgp_rows_group_moments": (
            [C.c_int, vp, vp, i32, i32, C.POINTER(mgp_variant_job), vp, i32, i32, C.POINTER(mgp_group_moments)], C.c_int
        ),
        "mgp_cell_coverage_run": ([vp, C.POINTER(mgp_variant_job), C.POINTER(mgp_cell_coverage)], C.c_int),
        "mgp_position_coverage_run": ([vp, C.POINTER(mgp_variant_job), C.POINTER(mgp_position_coverage)], C.c_int),
        "mgp_position_depth_hist_run": ([vp, C.POINTER(mgp_variant_job), i32, vp, vp], C.c_int),
        "mgp_position_depth_next_run": ([vp, C.POINTER(mgp_variant_job), vp, vp, vp], C.c_int),
        "mgp_cell_coverage_rows": (
            [C.c_int, vp, i32, i32, C.POINTER(mgp_variant_job), C.POINTER(mgp_cell_coverage)], C.c_int
        ),
        "mgp_position_coverage_rows": (
            [C.c_int, vp, vp, vp, i32, i32, C.POINTER(mgp_variant_job), C.POINTER(mgp_position_coverage)], C.c_int
        ),
        "mgp_position_depth_hist_rows": ([C.c_int, vp, i32, i32, C.POINTER(mgp_variant_job), i32, vp, vp], C.c_int),
        "mgp_position_depth_next_rows": ([C.c_int, vp, i32, i32, C.POINTER(mgp_variant_job), vp, vp, vp], C.c_int),
        "mgp_pair_dist": ([C.c_int, vp, i64, i64, vp], C.c_int),
        "mgp_hclust_dist": ([C.c_int, vp, i64, vp, vp, vp], C.c_int),
        "mgp_hclust": ([C.c_int, vp, i64, i64, vp, vp, vp, vp], C.c_int),
        "mgp_knn": ([C.c_int, vp, i64, i64, i32, vp, vp], C.c_int),
        "mgp_rank_sums": ([C.c_int, vp, i64, i64, vp, i32, vp, vp, vp], C.c_int),
        "mgp_snn": ([C.c_int, vp, i64, i32, i32, i64, C.POINTER(i64), vp, vp, vp], C.c_int),
        "mgp_pca": ([C.c_int, vp, i64, i64, i32, i32, vp, vp, vp, vp, vp, vp, C.POINTER(i32)], C.c_int),
        "mgp_sym_eig": ([C.c_int, vp, i64, vp, vp, C.POINTER(i32)], C.c_int),
        "mgp_louvain": (
            [C.c_int, i64, i64, vp, vp, vp, C.c_double, i32, i32, vp, C.POINTER(i64), C.POINTER(C.c_double), vp,
             C.POINTER(i32), vp], C.c_int
        ),
        "mgp_bgzf_inflate": ([C.c_int, vp, i64, i64, vp, vp, vp, vp, vp, i64, vp], C.c_int),
        "mgp_inflater_create": ([C.c_int, i64, i64, C.POINTER(vp)], C.c_int),
        "mgp_inflater_destroy": ([vp], None),
        "mgp_inflater_run": ([vp, vp, i64, i64, vp, vp, vp, vp, vp, i64, vp], C.c_int),
        "mgp_inflater_host_alloc": ([i64], vp),
        "mgp_inflater_host_release": ([vp], None),
        "mgp_inflater_times": ([vp, C.POINTER(C.c_double), C.POINTER(i64), C.POINTER(i64)], C.c_int),
        "mgp_zlib_inflate": ([C.c_int, vp, i64, i64, vp, vp, vp, vp, vp, i64, vp], C.c_int),
        "mgp_open_table": ([C.c_int, i32, i32, C.POINTER(vp)], C.c_int),
        "mgp_table_load": ([vp, C.POINTER(mgp_table_chunks)], C.c_int),
        "mgp_table_load_planes": ([vp, C.POINTER(mgp_table_chunks)], C.c_int),
        "mgp_table_check": ([i32, i32, C.POINTER(mgp_table_chunks), C.c_int], C.c_int),
        "mgp_table_ready": ([vp], C.c_int),
    }
    for name, (args, res) in sig.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = res
    if lib.mgp_abi_version() != ABI_VERSION:
        raise ProcessingError("libmgpileup ABI version mismatch")
    if path is None:
        _lib = lib
    return lib


def _raise(code: int, what: str):
    lib = load_library()
    msg = (lib.mgp_last_error() or b"").decode(errors="replace")
    text = f"{what}: {msg} (code {code})"
    if code == MGP_E_INVALID or code == MGP_E_SPAN:
        raise InvalidInputError(text)
    if code == MGP_E_UNSORTED:
        raise BAMFormatError("<resident reads>", text)
    if code == MGP_E_BADREAD:
        raise BAMReadError("<resident reads>", text)
    raise ProcessingError(text)


def _ck(code: int, what: str):
    if code != MGP_OK:
        _raise(code, what)


def _ptr(a: np.ndarray | None):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@dataclass
class EngineConfig:
    """POD restatement of the hot-path fields of PipelineConfig (config.py:77-114)."""

    n_cells: int
    min_baseq: int = 20
    min_mapq: int = 30
    min_distance_from_end: int = 5
    dedup_mode: str | int = "alignment_and_fragment_length"
    max_strand_bias: float = 1.0
    min_reads: int = 1
    mito_len: int = 16569
    reserve_reads: int = 0
    reserve_payload: int = 0
    keep_tn5: bool = False  # MGP_CFG_KEEP_TN5
    stream: bool = False  # MGP_CFG_STREAM: pushes run the windows they complete (overlapped H2D)

    def to_c(self) -> mgp_config:
        dm = DEDUP_MODES[self.dedup_mode] if isinstance(self.dedup_mode, str) else int(self.dedup_mode)
        flags = (CFG_KEEP_TN5 if self.keep_tn5 else 0) | (CFG_STREAM if self.stream else 0)
        return mgp_config(
            int(self.min_baseq), int(self.min_mapq), int(self.min_distance_from_end), dm,
            float(self.max_strand_bias), int(self.min_reads), int(self.n_cells), int(self.mito_len),
            flags, int(self.reserve_reads), int(self.reserve_payload),
        )


@dataclass
class EngineResult:
    """Host copy of mgp_result (cell-major arrays)."""

    counts: np.ndarray | None  # [n_cells, L, 8] u32
    tn5: np.ndarray | None  # [n_cells, L, 2] u32
    depth: np.ndarray | None  # [n_cells, L] u32
    n_reads: np.ndarray
    any_paired: np.ndarray
    passed: np.ndarray
    covered: np.ndarray
    depth_sum: np.ndarray
    depth_max: np.ndarray
    median_lo: np.ndarray
    median_hi: np.ndarray
    first_read: np.ndarray
    ref_tally: np.ndarray  # [L, 4] u64
    stats: dict
    # what a CellProcessor run adds (None: that step was not enabled, or has not run)
    txt_gz_cells: np.ndarray | None = None  # the device txt writer: the cells whose count lines it wrote [n written]
    h5_tiles: tuple | None = None  # the device HDF5 writer: (cell of column [n], chunks, {plane: tiles}, column sums)
    coverage: object | None = None  # enable_coverage: the CoverageResult over every cell of the run
    variants: object | None = None  # enable_variants: the VariantTable
    allele_freq: np.ndarray | None = None  # enable_variants: f64 [n variants, n population cells]
    variant_cells: np.ndarray | None = None  # enable_variants after enable_coverage: allele_freq's columns [n kept]
    variant_seconds: dict | None = None  # enable_variants: run_variants' seconds by pass
    clusters: object | None = None  # cluster_result: the ClusterResult
    neighbors: object | None = None  # neighbor_result: the NeighborGraph
    clonotypes: object | None = None  # clonotype_result: the Clonotypes
    groups: object | None = None  # enable_groups: the GroupResult (analysis/groups.py)
    pca: object | None = None  # enable_pca: the PcaResult (analysis/pca.py)

    @staticmethod
    def alloc(n_cells: int, L: int, dense: bool = True) -> EngineResult:
        return EngineResult(
            counts=np.zeros((n_cells, L, 8), np.uint32) if dense else None,
            tn5=np.zeros((n_cells, L, 2), np.uint32) if dense else None,
            depth=np.zeros((n_cells, L), np.uint32) if dense else None,
            n_reads=np.zeros(n_cells, np.uint32),
            any_paired=np.zeros(n_cells, np.uint8),
            passed=np.zeros(n_cells, np.uint8),
            covered=np.zeros(n_cells, np.uint32),
            depth_sum=np.zeros(n_cells, np.uint64),
            depth_max=np.zeros(n_cells, np.uint32),
            median_lo=np.zeros(n_cells, np.uint32),
            median_hi=np.zeros(n_cells, np.uint32),
            first_read=np.zeros(n_cells, np.uint32),
            ref_tally=np.zeros((L, 4), np.uint64),
            stats={},
        )

    def to_c(self, stats: mgp_stats) -> mgp_result:
        return mgp_result(
            _ptr(self.counts), _ptr(self.tn5), _ptr(self.depth), _ptr(self.n_reads), _ptr(self.any_paired),
            _ptr(self.passed), _ptr(self.covered), _ptr(self.depth_sum), _ptr(self.depth_max),
            _ptr(self.median_lo), _ptr(self.median_hi), _ptr(self.first_read), _ptr(self.ref_tally),
            C.pointer(stats),
        )

    def cell_order(self) -> np.ndarray:
        """Cells with >= 1 kept read in first-seen BAM order (dict order of reads_by_barcode)."""
        idx = np.flatnonzero(self.n_reads > 0)
        return idx[np.argsort(self.first_read[idx], kind="stable")]


@dataclass
class Rows16:
    """The pileup's 16-bit result rows of a cell range (mgp_rows16): exact except in
    `wide` (cell, window) pairs, where they saturate at 65535."""

    counts: np.ndarray  # [cells, L, 8] u16
    tn5: np.ndarray  # [cells, L, 2] u16
    depth: np.ndarray  # [cells, L] u16
    wide: np.ndarray  # [cells, n_windows] u8
    window_width: int

    def wide_cells(self) -> np.ndarray:
        """Cells (range-relative) with a window whose 16-bit rows are not exact."""
        return np.flatnonzero(self.wide.any(axis=1))


@dataclass
class Rows8:
    """The 8-bit rows target beside a Rows16 one (mgp_rows8, ABI 7): the rows of the
    (cell, window) pairs whose values all fit a byte (`narrow`); the others are in the
    16-bit target."""

    counts: np.ndarray  # [cells, L, 8] u8
    tn5: np.ndarray  # [cells, L, 2] u8
    depth: np.ndarray  # [cells, L] u8
    narrow: np.ndarray  # [cells, n_windows] u8


def merge_rows(r16: Rows16, r8: Rows8 | None, lo: int, hi: int) -> dict:
    """Cells [lo, hi) of a rows target as u32 arrays (counts, tn5, depth): each window
    from the 8-bit target where it is narrow, else from the 16-bit one (exact unless
    r16.wide)."""
    out = {"counts": r16.counts[lo:hi].astype(np.uint32), "tn5": r16.tn5[lo:hi].astype(np.uint32),
           "depth": r16.depth[lo:hi].astype(np.uint32)}
    if r8 is None:
        return out
    W = r16.window_width
    L = out["depth"].shape[1]
    nar = r8.narrow[lo:hi].astype(bool)
    for k in range(nar.shape[1]):
        m = np.flatnonzero(nar[:, k])
        if m.size == 0:
            continue
        a, b = k * W, min(L, (k + 1) * W)
        for key in ("counts", "tn5", "depth"):
            out[key][m, a:b] = getattr(r8, key)[lo + m, a:b]
    return out


def batch_struct(soa: ReadSoA) -> mgp_batch:
    """The C batch of a ReadSoA. ``span`` and ``rec_off`` may be None (ABI v3.1): the
    spans then come from the records' CIGARs on the device, and the records are dense
    in BAM order (record i at i x payload bytes / n); ``start`` may be None (ABI 4):
    taken from each record on the device."""
    for name in ("start", "bc", "tlen", "flag", "mapq", "span", "rec_off", "payload"):
        a = getattr(soa, name)
        if a is None and name in ("start", "span", "rec_off"):
            continue
        if not a.flags["C_CONTIGUOUS"]:
            raise InvalidInputError(f"batch array {name} must be C-contiguous")
    return mgp_batch(
        soa.n, _ptr(soa.start), _ptr(soa.bc), _ptr(soa.tlen), _ptr(soa.flag), _ptr(soa.mapq), _ptr(soa.span),
        _ptr(soa.rec_off), _ptr(soa.payload), int(soa.payload.shape[0]),
    )


TXT_FILES = ("coverage", "A", "C", "G", "T")  # the member order of mgp_txt_gz (file-major)


@dataclass
class TxtMembers:
    """The gzip members of mgp_txt_gz: `blob` holds them file-major (all coverage
    members in cell order, then A, C, G, T); member_bytes / text_bytes are [5, n]."""

    blob: np.ndarray
    member_bytes: np.ndarray
    text_bytes: np.ndarray

    def file_part(self, f: int) -> np.ndarray:
        """The bytes of file f (0 coverage, 1..4 A..T): its members back to back."""
        per = self.member_bytes.sum(axis=1)
        a = int(per[:f].sum())
        return self.blob[a:a + int(per[f])]


def _txt_job(cells, names: list):
    """(names: str, or bytes taken as they are)"""
    cells = np.ascontiguousarray(cells, dtype=np.int32)
    enc = [bytes(n) if isinstance(n, (bytes, bytearray)) else n.encode() for n in names]
    if len(enc) != cells.shape[0]:
        raise InvalidInputError("one barcode per written cell")
    off = np.zeros(len(enc) + 1, np.int64)
    off[1:] = np.cumsum([len(b) for b in enc])
    blob = np.frombuffer(b"".join(enc) or b"\0", np.uint8)
    n = cells.shape[0]
    mb = np.zeros((5, n), np.int64)
    tb = np.zeros((5, n), np.int64)
    job = mgp_txt_gz(n, _ptr(cells), _ptr(blob), _ptr(off), _ptr(mb), _ptr(tb))
    return job, (cells, blob, off), mb, tb


def txt_gz_rows(counts: np.ndarray, depth: np.ndarray, cells, names: list[str], device: int = 0) -> TxtMembers:
    """mgp_txt_gz_rows: the txt members of `cells` from caller-supplied u32 rows
    (counts [n, L, 8], depth [n, L]), no engine context."""
    lib = load_library()
    counts = np.ascontiguousarray(counts, np.uint32)
    depth = np.ascontiguousarray(depth, np.uint32)
    n_rows, L = depth.shape
    if counts.shape != (n_rows, L, 8):
        raise InvalidInputError("counts must be [n, L, 8]")
    job, keep, mb, tb = _txt_job(cells, names)
    # a bound: every member's text (<= bc + 29 bytes per covered position) plus stored-block overhead
    # (a cell out of range is the library's to refuse: it only has to get a bound here)
    rows = np.clip(np.asarray(keep[0], np.int64), 0, max(0, n_rows - 1))
    nnz = np.count_nonzero(depth, axis=1)[rows] if len(names) and n_rows else np.zeros(len(names), np.int64)
    text = nnz.astype(np.int64) * (np.diff(keep[2]) + 29)
    cap = int((5 * (text + 5 * (text // 65535 + 1) + 96)).sum()) + 64
    out = np.empty(cap, np.uint8)
    tot = C.c_int64()
    _ck(lib.mgp_txt_gz_rows(int(device), _ptr(counts), _ptr(depth), int(n_rows), int(L), C.byref(job), _ptr(out), cap,
                            C.byref(tot)), "mgp_txt_gz_rows")
    return TxtMembers(out[:int(tot.value)], mb, tb)


def _h5_grid(streams: np.ndarray, cb: np.ndarray, nrc: int, ncc: int) -> dict:
    """{plane: [chunk streams, row-major over an nrc x ncc grid]}: views of `streams`, which
    holds them plane-major with sizes cb."""
    offs = np.concatenate([[0], np.cumsum(cb)]).tolist()
    return {p: [streams[offs[k]:offs[k + 1]] for k in range(i * nrc * ncc, (i + 1) * nrc * ncc)]
            for i, p in enumerate(H5_PLANES)}


def h5_tiles_rows(counts: np.ndarray, tn5: np.ndarray, depth: np.ndarray, cell_of_col, chunks: tuple[int, int],
                  col_chunks: tuple[int, int] | None = None, sums: dict | None = None, device: int = 0) -> dict:
    """mgp_h5_tiles_rows: what Engine.h5_tiles returns, from caller-supplied u32 rows (counts
    [n, L, 8], tn5 [n, L, 2], depth [n, L]; stored as min(v, 65535)), no engine context;
    cell_of_col indexes the rows. One call covers all of col_chunks."""
    lib = load_library()
    counts = np.ascontiguousarray(counts, np.uint32)
    tn5 = np.ascontiguousarray(tn5, np.uint32)
    depth = np.ascontiguousarray(depth, np.uint32)
    n_rows, L = depth.shape
    if counts.shape != (n_rows, L, 8) or tn5.shape != (n_rows, L, 2):
        raise InvalidInputError("counts must be [n, L, 8] and tn5 [n, L, 2]")
    coc = np.ascontiguousarray(cell_of_col, np.int32)
    crow, ccol = int(chunks[0]), int(chunks[1])
    if crow <= 0 or ccol <= 0:
        raise InvalidInputError("chunk shape must be positive")
    nrc = -(-L // crow)
    c0, c1 = (0, -(-coc.size // ccol)) if col_chunks is None else (int(col_chunks[0]), int(col_chunks[1]))
    nch = len(H5_PLANES) * nrc * max(0, c1 - c0)
    cb = np.zeros(max(1, nch), np.int64)
    part = np.zeros((3, L), np.int64)
    job = mgp_h5_tiles(coc.size, _ptr(coc), crow, ccol, c0, c1, _ptr(cb), _ptr(part))
    # a bound: every chunk stored, with the frame (the device's own bound is no larger)
    raw = 2 * crow * ccol
    cap = nch * (raw + 5 * (raw // 65535 + 1) + 6) if crow * ccol <= 1 << 22 else 0
    out = np.empty(max(1, cap), np.uint8)
    tot = C.c_int64()
    _ck(lib.mgp_h5_tiles_rows(int(device), _ptr(counts), _ptr(tn5), _ptr(depth), int(n_rows), int(L), C.byref(job),
                              _ptr(out), cap, C.byref(tot)), "mgp_h5_tiles_rows")
    if sums is not None:
        sums.update(coverage=part[0].copy(), tn5_fwd=part[1].copy(), tn5_rev=part[2].copy())
    return _h5_grid(out[:int(tot.value)], cb[:nch], nrc, c1 - c0)


VARIANT_MAX_CELLS = 1 << 16  # cells of one mgp_variant_* call (the u64 moments' exactness bound)
ALLELE_FREQ_MAX_VALUES = 1 << 29  # values of one mgp_allele_freq_* call


def alloc_moments(L: int) -> dict:
    """Zeroed host arrays of mgp_variant_moments, by field name (MOMENT_FIELDS)."""
    return {k: np.zeros(L if k in MOMENT_PER_POS else (L, 4), np.float64 if k == "s_af" else np.uint64)
            for k in MOMENT_FIELDS}


def _variant_job(cells, low_coverage_threshold: int = 0):
    cells = None if cells is None else np.ascontiguousarray(cells, dtype=np.int32)
    job = mgp_variant_job(0 if cells is None else cells.shape[0], _ptr(cells), int(low_coverage_threshold))
    return job, cells


def _variant_list(variants):
    """(pos int32 [n_var], base int32 [n_var]) of an iterable of (0-based position, base 0..3)."""
    v = np.asarray(list(variants), dtype=np.int64).reshape(-1, 2)
    return np.ascontiguousarray(v[:, 0], np.int32), np.ascontiguousarray(v[:, 1], np.int32)


def _variant_calls(call, n_rows: int, L: int):
    """The three reductions over one row source: call(name, *args) runs mgp_<name>_run on a
    context or mgp_<name>_rows on caller rows."""

    def moments(cells=None, low_coverage_threshold: int = 0) -> dict:
        job, keep = _variant_job(cells, low_coverage_threshold)
        out = alloc_moments(L)
        call("mgp_variant_moments", C.byref(job), C.byref(mgp_variant_moments(*[_ptr(out[k]) for k in MOMENT_FIELDS])))
        return out

    def dev2(mean_af, cells=None, low_coverage_threshold: int = 0) -> np.ndarray:
        job, keep = _variant_job(cells, low_coverage_threshold)
        mu = np.ascontiguousarray(mean_af, np.float64)
        if mu.shape != (L, 4):
            raise InvalidInputError("mean_af must be [mito_len, 4]")
        out = np.zeros((L, 4), np.float64)
        call("mgp_variant_dev2", C.byref(job), _ptr(mu), _ptr(out))
        return out

    def allele_freq(variants, cells=None, min_coverage: int = 1) -> np.ndarray:
        job, keep = _variant_job(cells)
        pos, base = _variant_list(variants)
        n = n_rows if keep is None else keep.shape[0]
        out = np.zeros((pos.shape[0], n), np.float64)
        step = max(1, ALLELE_FREQ_MAX_VALUES // max(1, n))
        for a in range(0, pos.shape[0], step):
            b = min(pos.shape[0], a + step)
            call("mgp_allele_freq", C.byref(job), b - a, _ptr(pos[a:b]), _ptr(base[a:b]), int(min_coverage),
                 _ptr(out[a:b]))
        return out

    return moments, dev2, allele_freq


def _rows_calls(counts: np.ndarray, depth: np.ndarray, device: int):
    lib = load_library()
    counts = np.ascontiguousarray(counts, np.uint32)
    depth = np.ascontiguousarray(depth, np.uint32)
    n_rows, L = depth.shape
    if counts.shape != (n_rows, L, 8):
        raise InvalidInputError("counts must be [n, L, 8]")

    def call(name, *args):
        _ck(getattr(lib, name + "_rows")(int(device), _ptr(counts), _ptr(depth), int(n_rows), int(L), *args),
            name + "_rows")

    return _variant_calls(call, n_rows, L)


def variant_moments_rows(counts: np.ndarray, depth: np.ndarray, cells=None, low_coverage_threshold: int = 0,
                         device: int = 0) -> dict:
    """mgp_variant_moments_rows: Engine.variant_moments on caller-supplied u32 rows (counts
    [n, L, 8], depth [n, L]), no engine context."""
    return _rows_calls(counts, depth, device)[0](cells, low_coverage_threshold)


def variant_dev2_rows(counts: np.ndarray, depth: np.ndarray, mean_af, cells=None, low_coverage_threshold: int = 0,
                      device: int = 0) -> np.ndarray:
    """mgp_variant_dev2_rows: Engine.variant_dev2 on caller-supplied u32 rows."""
    return _rows_calls(counts, depth, device)[1](mean_af, cells, low_coverage_threshold)


def allele_freq_rows(counts: np.ndarray, depth: np.ndarray, variants, cells=None, min_coverage: int = 1,
                     device: int = 0) -> np.ndarray:
    """mgp_allele_freq_rows: Engine.allele_freq on caller-supplied u32 rows."""
    return _rows_calls(counts, depth, device)[2](variants, cells, min_coverage)


def alloc_group_moments(n_groups: int, L: int) -> dict:
    """Zeroed host arrays of mgp_group_moments for n_groups groups, by field name (GROUP_FIELDS)."""
    return {k: np.zeros((n_groups, L) if k == "cov" else (n_groups, L, 4), dt) for k, dt in GROUP_FIELDS}


def _group_calls(call, n_rows: int, L: int, group, n_groups: int, cells, max_item_cells: int) -> dict:
    """mgp_group_moments over one row source, call(job, group, n_groups, max_item_cells, out): any n_groups >= 1,
    in calls of at most GROUP_MAX_GROUPS groups, each with the other calls' labels set to -1 (it sweeps its own
    cells only), the results concatenated."""
    job, keep = _variant_job(cells)
    group = np.ascontiguousarray(group, np.int32)
    n = n_rows if keep is None else keep.shape[0]
    n_groups = int(n_groups)
    if group.shape != (n,):
        raise InvalidInputError(f"group_moments: {group.shape[0] if group.ndim == 1 else group.shape} labels for "
                                f"{n} cells")
    out = alloc_group_moments(max(n_groups, 0), L)
    if n_groups <= GROUP_MAX_GROUPS:  # one call, the library's own checks
        call(C.byref(job), _ptr(group), n_groups, int(max_item_cells),
             C.byref(mgp_group_moments(*[_ptr(out[k]) for k, _ in GROUP_FIELDS])))
        return out
    if group.size and (int(group.min()) < -1 or int(group.max()) >= n_groups):
        raise InvalidInputError("group_moments: group label out of range")
    for g0 in range(0, n_groups, GROUP_MAX_GROUPS):
        g1 = min(n_groups, g0 + GROUP_MAX_GROUPS)
        lab = np.where((group >= g0) & (group < g1), group - g0, -1).astype(np.int32)
        part = mgp_group_moments(*[_ptr(out[k][g0:g1]) for k, _ in GROUP_FIELDS])
        call(C.byref(job), _ptr(lab), g1 - g0, int(max_item_cells), C.byref(part))
    return out


def group_moments_rows(counts: np.ndarray, depth: np.ndarray, group, n_groups: int, cells=None,
                       max_item_cells: int = 0, device: int = 0) -> dict:
    """mgp_rows_group_moments: Engine.group_moments on caller-supplied u32 rows (counts [n, L, 8], depth
    [n, L]), no engine context."""
    lib = load_library()
    counts = np.ascontiguousarray(counts, np.uint32)
    depth = np.ascontiguousarray(depth, np.uint32)
    n_rows, L = depth.shape
    if counts.shape != (n_rows, L, 8):
        raise InvalidInputError("counts must be [n, L, 8]")

    def call(*args):
        _ck(lib.mgp_rows_group_moments(int(device), _ptr(counts), _ptr(depth), int(n_rows), int(L), *args),
            "mgp_rows_group_moments")

    return _group_calls(call, n_rows, L, group, n_groups, cells, max_item_cells)


def _coverage_calls(call, n_rows: int, L: int):
    """The four coverage QC passes over one row source: call(name, *args) runs mgp_<name>_run
    on a context or mgp_<name>_rows on caller rows. Each returns a dict of numpy arrays."""

    def cell_coverage(cells=None) -> dict:
        job, keep = _variant_job(cells)
        n = n_rows if keep is None else keep.shape[0]
        out = {k: np.zeros(n, dt) for k, dt in CELL_COVERAGE_FIELDS}
        call("mgp_cell_coverage", C.byref(job),
             C.byref(mgp_cell_coverage(*[_ptr(out[k]) for k, _ in CELL_COVERAGE_FIELDS])))
        return out

    def position_coverage(cells=None) -> dict:
        job, keep = _variant_job(cells)
        out = {k: np.zeros((L, 4) if k == "tally" else L, dt) for k, dt in POSITION_COVERAGE_FIELDS}
        call("mgp_position_coverage", C.byref(job),
             C.byref(mgp_position_coverage(*[_ptr(out[k]) for k, _ in POSITION_COVERAGE_FIELDS])))
        return out

    def position_depth_hist(shift: int, prefix=None, cells=None) -> dict:
        job, keep = _variant_job(cells)
        pre = np.zeros(L, np.uint32) if prefix is None else np.ascontiguousarray(prefix, np.uint32)
        if pre.shape != (L,):
            raise InvalidInputError("prefix must be [mito_len]")
        hist = np.zeros((L, 256), np.uint32)
        call("mgp_position_depth_hist", C.byref(job), int(shift), _ptr(pre), _ptr(hist))
        return {"hist": hist}

    def position_depth_next(v, cells=None) -> dict:
        job, keep = _variant_job(cells)
        at = np.ascontiguousarray(v, np.uint32)
        if at.shape != (L,):
            raise InvalidInputError("v must be [mito_len]")
        n_le, nxt = np.zeros(L, np.uint32), np.zeros(L, np.uint32)
        call("mgp_position_depth_next", C.byref(job), _ptr(at), _ptr(n_le), _ptr(nxt))
        return {"n_le": n_le, "next": nxt}

    return cell_coverage, position_coverage, position_depth_hist, position_depth_next


def _coverage_rows_calls(counts, tn5, depth: np.ndarray, device: int):
    lib = load_library()
    depth = np.ascontiguousarray(depth, np.uint32)
    n_rows, L = depth.shape
    if counts is not None:
        counts = np.ascontiguousarray(counts, np.uint32)
        tn5 = np.ascontiguousarray(tn5, np.uint32)
        if counts.shape != (n_rows, L, 8) or tn5.shape != (n_rows, L, 2):
            raise InvalidInputError("counts must be [n, L, 8] and tn5 [n, L, 2]")

    def call(name, *args):
        rows = (_ptr(counts), _ptr(tn5), _ptr(depth)) if name == "mgp_position_coverage" else (_ptr(depth),)
        _ck(getattr(lib, name + "_rows")(int(device), *rows, int(n_rows), int(L), *args), name + "_rows")

    return _coverage_calls(call, n_rows, L)


def cell_coverage_rows(depth: np.ndarray, cells=None, device: int = 0) -> dict:
    """mgp_cell_coverage_rows: Engine.cell_coverage on caller-supplied u32 depths [n, L]."""
    return _coverage_rows_calls(None, None, depth, device)[0](cells)


def position_coverage_rows(counts: np.ndarray, tn5: np.ndarray, depth: np.ndarray, cells=None, device: int = 0) -> dict:
    """mgp_position_coverage_rows: Engine.position_coverage on caller-supplied u32 rows (counts
    [n, L, 8], tn5 [n, L, 2], depth [n, L])."""
    return _coverage_rows_calls(counts, tn5, depth, device)[1](cells)


def position_depth_hist_rows(depth: np.ndarray, shift: int, prefix=None, cells=None, device: int = 0) -> dict:
    """mgp_position_depth_hist_rows: Engine.position_depth_hist on caller-supplied u32 depths."""
    return _coverage_rows_calls(None, None, depth, device)[2](shift, prefix, cells)


def position_depth_next_rows(depth: np.ndarray, v, cells=None, device: int = 0) -> dict:
    """mgp_position_depth_next_rows: Engine.position_depth_next on caller-supplied u32 depths."""
    return _coverage_rows_calls(None, None, depth, device)[3](v, cells)


CLUSTER_MAX_ITEMS = 1 << 16  # items of one mgp_pair_dist / mgp_hclust* call (8 n^2 bytes of distances)


def _cluster_x(x) -> np.ndarray:
    x = np.ascontiguousarray(x, np.float64)
    if x.ndim != 2:
        raise InvalidInputError("x is [n_feat, n_items]")
    return x


def _cluster_outputs(n: int):
    return np.zeros((max(n - 1, 0), 2), np.int32), np.zeros(max(n - 1, 0), np.float64), np.zeros(n, np.int32)


def cluster_pair_dist(x, device: int = 0) -> np.ndarray:
    """mgp_pair_dist: [n, n] Euclidean distances of the columns of x [n_feat, n_items] (fp64,
    every value finite; at most CLUSTER_MAX_ITEMS items)."""
    x = _cluster_x(x)
    nf, n = x.shape
    out = np.zeros((n, n), np.float64) if n <= CLUSTER_MAX_ITEMS else None  # (above: refused before any use)
    _ck(load_library().mgp_pair_dist(int(device), _ptr(x), n, nf, _ptr(out)), "mgp_pair_dist")
    return out


def cluster_hclust_dist(dist, device: int = 0):
    """mgp_hclust_dist: (merge [n - 1, 2], height [n - 1], order [n]) of complete linkage on
    the symmetric, finite, non-negative matrix dist [n, n], in R's hclust conventions."""
    dist = np.ascontiguousarray(dist, np.float64)
    if dist.ndim != 2 or dist.shape[0] != dist.shape[1]:
        raise InvalidInputError("dist is [n, n]")
    n = dist.shape[0]
    merge, height, order = _cluster_outputs(min(n, CLUSTER_MAX_ITEMS))
    _ck(load_library().mgp_hclust_dist(int(device), _ptr(dist), n, _ptr(merge), _ptr(height), _ptr(order)),
        "mgp_hclust_dist")
    return merge, height, order


def cluster_hclust(x, device: int = 0, want_dist: bool = False):
    """mgp_hclust: the distances and the linkage of the columns of x [n_feat, n_items] in one
    call; (merge, height, order, dist or None). The matrix stays on the device unless asked for."""
    x = _cluster_x(x)
    nf, n = x.shape
    merge, height, order = _cluster_outputs(min(n, CLUSTER_MAX_ITEMS))
    dist = np.zeros((n, n), np.float64) if want_dist and n <= CLUSTER_MAX_ITEMS else None
    _ck(load_library().mgp_hclust(int(device), _ptr(x), n, nf, _ptr(merge), _ptr(height), _ptr(order), _ptr(dist)),
        "mgp_hclust")
    return merge, height, order, dist


GRAPH_MAX_ITEMS = 1 << 20  # items of one mgp_knn / mgp_snn call
GRAPH_MAX_K = 64           # neighbours per item (Seurat's k.param - 1)


def graph_knn(x, k: int, device: int = 0):
    """mgp_knn: (idx [n, k] int32, dist [n, k]) of the columns of x [n_feat, n_items]: per item
    the k others smallest under (distance, index), in that order; the distances are
    mgp_pair_dist's. 1 <= k <= min(GRAPH_MAX_K, n - 1)."""
    x = _cluster_x(x)
    nf, n = x.shape
    ok = n <= GRAPH_MAX_ITEMS and 1 <= int(k) <= GRAPH_MAX_K  # (otherwise refused before any use)
    idx = np.zeros((n, int(k)), np.int32) if ok else None
    dist = np.zeros((n, int(k)), np.float64) if ok else None
    _ck(load_library().mgp_knn(int(device), _ptr(x), n, nf, int(k), _ptr(idx), _ptr(dist)), "mgp_knn")
    return idx, dist


def graph_snn(idx, min_shared: int, device: int = 0):
    """mgp_snn: (i, j, shared) int32 arrays of the pairs i < j whose sets S = {row} + idx[row]
    share at least min_shared members, from the kNN table idx [n, k]; sorted by (i, j) here (the
    device's order is free). Two calls: the count, then the triples."""
    idx = np.ascontiguousarray(idx, np.int32)
    if idx.ndim != 2:
        raise InvalidInputError("idx is [n_items, k]")
    n, k = idx.shape
    lib = load_library()
    count = C.c_int64(0)
    rc = lib.mgp_snn(int(device), _ptr(idx), n, k, int(min_shared), 0, C.byref(count), None, None, None)
    if rc != MGP_OK and not (rc == MGP_E_INVALID and 0 < count.value <= 1 << 30):
        _raise(rc, "mgp_snn")
    ne = int(count.value)
    out = [np.zeros(ne, np.int32) for _ in range(3)]
    if ne:
        _ck(lib.mgp_snn(int(device), _ptr(idx), n, k, int(min_shared), ne, C.byref(count), *map(_ptr, out)), "mgp_snn")
        order = np.lexsort((out[1], out[0]))
        out = [a[order] for a in out]
    return tuple(out)


RANK_MAX_ITEMS = 1 << 20   # items of one mgp_rank_sums call
RANK_MAX_GROUPS = 1 << 16  # groups of one call
RANK_LDS_GROUPS = 2048     # groups up to here: the rank kernel's table is in LDS (rank::kLdsGroups)


def rank_sums(x, group, n_groups: int, device: int = 0) -> dict:
    """mgp_rank_sums: per feature (row of x [n_feat, n_items], fp64, every value finite) the items ordered by
    value (-0.0 equals +0.0), a tie class at the 0-based sorted positions lo..hi having the midrank
    (lo + hi + 2) / 2. group[i] in 0 .. n_groups - 1 labels item i (checked on the device). A dict: `r2`
    [n_feat, n_groups] uint64, the sum over the group's items of lo + hi + 2; `pos` [n_feat, n_groups] uint32,
    the group's items with a value > 0; `ties` [n_feat] uint64, the sum over the tie classes of t^3 - t. Exact
    integers, a function of the input alone. At most RANK_MAX_ITEMS items and RANK_MAX_GROUPS groups."""
    x = _cluster_x(x)
    nf, n = x.shape
    group = np.ascontiguousarray(group, np.int32)
    if group.shape != (n,):
        raise InvalidInputError(f"rank_sums: {group.shape[0] if group.ndim == 1 else group.shape} labels for {n} items")
    n_groups = int(n_groups)
    ok = n <= RANK_MAX_ITEMS and 1 <= n_groups <= RANK_MAX_GROUPS  # (otherwise refused before any use)
    shape = (nf, n_groups) if ok else (0, 0)
    out = {"r2": np.zeros(shape, np.uint64), "pos": np.zeros(shape, np.uint32), "ties": np.zeros(shape[0], np.uint64)}
    _ck(load_library().mgp_rank_sums(int(device), _ptr(x), n, nf, _ptr(group), n_groups, _ptr(out["r2"]),
                                     _ptr(out["pos"]), _ptr(out["ties"])), "mgp_rank_sums")
    return out


PCA_MAX_ITEMS = 1 << 20  # items of one mgp_pca call
PCA_MAX_FEAT = 2048      # features of one mgp_pca call, rows of one mgp_sym_eig call
PCA_SLAB = 1024          # items of a slab of the sums (part of the definition, pca::kSlab)


def pca(x, n_comp: int, scale: bool = False, device: int = 0, want_cov: bool = False) -> dict:
    """mgp_pca: the principal components of the columns of x [n_feat, n_items] (fp64, every value finite), R's
    prcomp(t(x), center = TRUE, scale. = scale), every number a fixed chain of fp64 operations (include/mgpileup.h).
    A dict: `mean` [m], `sd` [m] (the divisor with scale, otherwise the square root of the covariance's diagonal),
    `eigenvalues` [m] descending, `loadings` [n_comp, m], `scores` [n_comp, n], `sweeps`, and `cov` [m, m] when
    asked for. 2 <= n_items <= PCA_MAX_ITEMS, n_feat <= PCA_MAX_FEAT, 1 <= n_comp <= min(n_feat, n_items - 1)."""
    x = _cluster_x(x)
    m, n = x.shape
    k = int(n_comp)
    ok = 2 <= n <= PCA_MAX_ITEMS and m <= PCA_MAX_FEAT and 1 <= k <= min(m, n - 1)  # (otherwise refused before any use)
    out = {"mean": np.zeros(m if ok else 0), "sd": np.zeros(m if ok else 0), "eigenvalues": np.zeros(m if ok else 0),
           "loadings": np.zeros((k, m) if ok else (0, 0)), "scores": np.zeros((k, n) if ok else (0, 0))}
    cov = np.zeros((m, m)) if ok and want_cov else None
    sweeps = C.c_int32(0)
    _ck(load_library().mgp_pca(int(device), _ptr(x), n, m, int(bool(scale)), k, _ptr(out["mean"]), _ptr(out["sd"]),
                               _ptr(out["eigenvalues"]), _ptr(out["loadings"]), _ptr(out["scores"]), _ptr(cov),
                               C.byref(sweeps)), "mgp_pca")
    out["sweeps"] = int(sweeps.value)
    if want_cov:
        out["cov"] = cov
    return out


def sym_eig(a, device: int = 0):
    """mgp_sym_eig: (eigenvalues [m] descending, vectors [m, m] with row c the eigenvector c, sweeps) of the
    symmetric finite matrix a [m, m] by the fixed-order Jacobi iteration on the device (include/mgpileup.h); the
    same bytes on every call. m <= PCA_MAX_FEAT."""
    a = np.ascontiguousarray(a, np.float64)
    if a.ndim != 2 or a.shape[0] != a.shape[1]:
        raise InvalidInputError("a is [m, m]")
    m = a.shape[0]
    ok = m <= PCA_MAX_FEAT  # (otherwise refused before any use)
    eig, vec = np.zeros(m if ok else 0), np.zeros((m, m) if ok else (0, 0))
    sweeps = C.c_int32(0)
    _ck(load_library().mgp_sym_eig(int(device), _ptr(a), m, _ptr(eig), _ptr(vec), C.byref(sweeps)), "mgp_sym_eig")
    return eig, vec, int(sweeps.value)


LOUVAIN_MAX_VERTICES = 1 << 20  # vertices of one mgp_louvain call
LOUVAIN_MAX_EDGES = 1 << 30     # undirected edges of one call
LOUVAIN_MAX_WEIGHT = 1 << 20    # an edge's integer weight, in units of 2^-20
LOUVAIN_MAX_LEVELS = 64         # the cap on max_levels
LOUVAIN_MAX_PASSES = 1 << 16    # the cap on max_passes
LOUVAIN_WAVE_ROW = 64           # rows up to here are a wave's (MGP_LOUVAIN_WAVE_ROW lowers it)
LOUVAIN_LDS_ROW = 2048          # rows up to here use the LDS table (MGP_LOUVAIN_LDS_ROW lowers it)


def graph_louvain(n: int, i, j, wq, resolution: float = 1.0, max_levels: int = 32, max_passes: int = 64,
                  device: int = 0) -> dict:
    """mgp_louvain: the communities of the graph of n vertices with the undirected edges (i, j),
    i < j, each pair once, and integer weights wq in 1..2^20 (units of 2^-20). A dict: labels
    [n] int32 (numbered by descending size, ties by smallest member), n_communities, modularity,
    m2, internal, b (Python integers) and levels, the (vertices, communities, passes, accepted)
    of each level. The edges are checked on the device (InvalidInputError)."""
    i, j, wq = (np.ascontiguousarray(a, np.int32).reshape(-1) for a in (i, j, wq))
    if not i.size == j.size == wq.size:
        raise InvalidInputError("i, j and wq have one entry per edge")
    n, ne = int(n), int(i.size)
    ok = 0 <= n <= LOUVAIN_MAX_VERTICES and 1 <= int(max_levels) <= LOUVAIN_MAX_LEVELS  # (otherwise refused first)
    labels = np.zeros(n if ok else 0, np.int32)
    levels = np.zeros((int(max_levels) if ok else 1, 4), np.int64)
    sums = np.zeros(4, np.uint64)
    nc, nl, q = C.c_int64(0), C.c_int32(0), C.c_double(0.0)
    _ck(load_library().mgp_louvain(int(device), n, ne, _ptr(i), _ptr(j), _ptr(wq), float(resolution), int(max_levels),
                                   int(max_passes), _ptr(labels), C.byref(nc), C.byref(q), _ptr(sums), C.byref(nl),
                                   _ptr(levels)), "mgp_louvain")
    return {"labels": labels, "n_communities": int(nc.value), "modularity": float(q.value), "m2": int(sums[0]),
            "internal": int(sums[1]), "b": (int(sums[2]) << 64) | int(sums[3]),
            "levels": [tuple(int(x) for x in row) for row in levels[: nl.value]]}


INFLATE_MAX_ISIZE = 65536  # inflated bytes of one BGZF block


def _inflate_args(src, coff, clen, isize, out_off, out):
    """The arrays of one inflate call in the C-ABI's types, and the statuses' array."""
    src = np.ascontiguousarray(np.frombuffer(src, np.uint8) if isinstance(src, (bytes, bytearray)) else src, np.uint8)
    coff = np.ascontiguousarray(coff, np.uint64)
    clen = np.ascontiguousarray(clen, np.uint32)
    isize = np.ascontiguousarray(isize, np.uint32)
    out_off = np.ascontiguousarray(out_off, np.uint64)
    n = int(coff.shape[0])
    if not (clen.shape[0] == isize.shape[0] == out_off.shape[0] == n):
        raise InvalidInputError("coff, clen, isize and out_off have one entry per block")
    if out.dtype != np.uint8 or not out.flags.c_contiguous or not out.flags.writeable:
        raise InvalidInputError("out is a writable contiguous uint8 array")
    status = np.full(n, -1, np.int32)
    return (_ptr(src), int(src.shape[0]), n, _ptr(coff), _ptr(clen), _ptr(isize), _ptr(out_off), _ptr(out),
            int(out.shape[0]), _ptr(status)), status, (src, coff, clen, isize, out_off)


def inflate_bgzf(src, coff, clen, isize, out_off, out: np.ndarray, device: int = 0) -> np.ndarray:
    """mgp_bgzf_inflate: block i is the raw deflate stream src[coff[i], coff[i] + clen[i]) and
    inflates to isize[i] bytes at out[out_off[i], ...) on the device; returns the blocks'
    statuses (0 ok, 1 invalid stream, 2 wrong size or input ended early). CRC32 is the
    caller's."""
    args, status, keep = _inflate_args(src, coff, clen, isize, out_off, out)
    _ck(load_library().mgp_bgzf_inflate(int(device), *args), "mgp_bgzf_inflate")
    del keep
    return status


def inflate_zlib(src, coff, clen, isize, out_off, out: np.ndarray, device: int = 0) -> np.ndarray:
    """mgp_zlib_inflate: stream i is the whole zlib stream src[coff[i], coff[i] + clen[i]) and
    inflates to isize[i] bytes (any size below 2^31) at out[out_off[i], ...) on the device;
    returns the streams' statuses (0 ok, 1 invalid stream, 2 wrong size or input ended early,
    3 Adler-32 differs or bytes follow the trailer). out receives the bytes of the streams with
    status 0 alone."""
    args, status, keep = _inflate_args(src, coff, clen, isize, out_off, out)
    _ck(load_library().mgp_zlib_inflate(int(device), *args), "mgp_zlib_inflate")
    del keep
    return status


class Inflater:
    """An mgp_inflater: device buffers for max_src_bytes / max_out_bytes per call, a stream
    and pinned staging kept across calls (the BAM ingest's form, BamFile.set_device_inflate)."""

    def __init__(self, device: int = 0, max_src_bytes: int = 20 << 20, max_out_bytes: int = 80 << 20):
        self.lib = load_library()
        self.device = int(device)
        self.max_src_bytes, self.max_out_bytes = int(max_src_bytes), int(max_out_bytes)
        h = C.c_void_p()
        _ck(self.lib.mgp_inflater_create(self.device, self.max_src_bytes, self.max_out_bytes, C.byref(h)),
            "mgp_inflater_create")
        self._h = h

    @property
    def handle(self) -> int:
        """The mgp_inflater's address (the ctx of mgp_inflater_run)."""
        if not self._h:
            raise ProcessingError("the inflater is closed")
        return int(self._h.value)

    def run(self, src, coff, clen, isize, out_off, out: np.ndarray) -> np.ndarray:
        """mgp_inflater_run: as :func:`inflate_bgzf`."""
        args, status, keep = _inflate_args(src, coff, clen, isize, out_off, out)
        _ck(self.lib.mgp_inflater_run(self.handle, *args), "mgp_inflater_run")
        del keep
        return status

    def times(self) -> dict:
        """mgp_inflater_times: the calls' device milliseconds so far (H2D, kernel, D2H), summed."""
        ms = (C.c_double * 3)()
        calls, blocks = C.c_int64(0), C.c_int64(0)
        _ck(self.lib.mgp_inflater_times(self.handle, ms, C.byref(calls), C.byref(blocks)), "mgp_inflater_times")
        return {"h2d_ms": ms[0], "kernel_ms": ms[1], "d2h_ms": ms[2], "calls": int(calls.value),
                "blocks": int(blocks.value)}

    def close(self):
        if getattr(self, "_h", None):
            self.lib.mgp_inflater_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Engine:
    """One device context (one GPU). Not thread-safe."""

    def __init__(self, cfg: EngineConfig, device: int = 0):
        self.lib = load_library()
        self.cfg = cfg
        self._c = cfg.to_c()
        h = C.c_void_p()
        _ck(self.lib.mgp_open(C.byref(self._c), int(device), C.byref(h)), "mgp_open")
        self._h = h
        self._keep: list = []  # keep host batches alive until the next sync

    # -- a loaded table (mgp_open_table) ------------------------------------
    @classmethod
    def open_table(cls, n_cells: int, mito_len: int, device: int = 0) -> Engine:
        """mgp_open_table: a context of n_cells x mito_len whose 16-bit rows are loaded from a
        finished run's count files (load / load_planes, then ready) and not made by a run.
        Every row job (h5_tiles, txt_gz, the coverage and variant passes) then works on it;
        push, run, sync and fetch are refused. cfg holds n_cells and mito_len alone."""
        self = cls.__new__(cls)
        self.lib = load_library()
        self.cfg = EngineConfig(n_cells=int(n_cells), mito_len=int(mito_len))
        self._c = None
        self._keep = []
        h = C.c_void_p()
        _ck(self.lib.mgp_open_table(int(device), int(n_cells), int(mito_len), C.byref(h)), "mgp_open_table")
        self._h = h
        return self

    def _table_job(self, n_cols, chunks, col_chunks, first_cell, src, chunk_bytes=None, raw=None):
        src = np.ascontiguousarray(np.frombuffer(src, np.uint8) if isinstance(src, (bytes, bytearray)) else src)
        src = src.view(np.uint8).reshape(-1)
        cb = None if chunk_bytes is None else np.ascontiguousarray(chunk_bytes, np.int64)
        rw = None if raw is None else np.ascontiguousarray(raw, np.uint8)
        job = mgp_table_chunks(int(n_cols), int(chunks[0]), int(chunks[1]), int(col_chunks[0]), int(col_chunks[1]),
                               int(first_cell), 0, _ptr(src), int(src.shape[0]), _ptr(cb), _ptr(rw), 0)
        return job, (src, cb, rw)

    @staticmethod
    def _table_out(job) -> dict:
        return {"n_saturated": int(job.n_saturated), "h2d_ms": job.ms[0], "inflate_ms": job.ms[1],
                "transpose_ms": job.ms[2]}

    def load(self, n_cols: int, chunks: tuple[int, int], col_chunks: tuple[int, int], first_cell: int, src,
             chunk_bytes, raw) -> dict:
        """mgp_table_load: the column chunks [col_chunks[0], col_chunks[1]) of the 11 datasets
        ([mito_len][n_cols], chunk shape `chunks`) into the table's cells from first_cell on.
        src: the chunks' stored bytes, plane-major (H5_PLANES), then row chunk, then column
        chunk; chunk_bytes their sizes; raw their kinds (CHUNK_ZLIB, CHUNK_RAW, CHUNK_ABSENT).
        Returns n_saturated and the device milliseconds of the H2D, the inflate and the
        transposition."""
        job, keep = self._table_job(n_cols, chunks, col_chunks, first_cell, src, chunk_bytes, raw)
        _ck(self.lib.mgp_table_load(self._h, C.byref(job)), "mgp_table_load")
        del keep
        return self._table_out(job)

    def load_planes(self, n_cols: int, chunks: tuple[int, int], col_chunks: tuple[int, int], first_cell: int,
                    tiles) -> dict:
        """mgp_table_load_planes: the same batch as inflated tiles (u16 [11][row chunks][column
        chunks][chunk rows][chunk columns], edges padded): the transposition alone."""
        job, keep = self._table_job(n_cols, chunks, col_chunks, first_cell, tiles)
        _ck(self.lib.mgp_table_load_planes(self._h, C.byref(job)), "mgp_table_load_planes")
        del keep
        return self._table_out(job)

    def ready(self):
        """mgp_table_ready: the load is complete; the row jobs serve the table from here."""
        _ck(self.lib.mgp_table_ready(self._h), "mgp_table_ready")

    # -- lifecycle ---------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self.lib.mgp_close(self._h)
            self._h = None
        self._keep = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- data --------------------------------------------------------------
    def push(self, soa: ReadSoA):
        """mgp_push_batch; a batch whose bc and tlen are uint16 arrays (16-bit barcode
        index, 0xFFFF = none, and |tlen|; dense records, no start / span / rec_off) goes
        through mgp_push_batch16."""
        if soa.bc is not None and soa.bc.dtype == np.uint16:
            for name in ("bc", "tlen", "flag", "mapq", "payload"):
                if not getattr(soa, name).flags["C_CONTIGUOUS"]:
                    raise InvalidInputError(f"batch array {name} must be C-contiguous")
            if soa.tlen.dtype != np.uint16 or soa.start is not None or soa.span is not None or soa.rec_off is not None:
                raise InvalidInputError("a 16-bit batch has uint16 bc and |tlen| and dense records only")
            b = mgp_batch16(soa.n, _ptr(soa.bc), _ptr(soa.tlen), _ptr(soa.flag), _ptr(soa.mapq), _ptr(soa.payload),
                            int(soa.payload.shape[0]))
            _ck(self.lib.mgp_push_batch16(self._h, C.byref(b)), "mgp_push_batch16")
        else:
            b = batch_struct(soa)
            _ck(self.lib.mgp_push_batch(self._h, C.byref(b)), "mgp_push_batch")
        self._keep.append(soa)

    def reset(self):
        _ck(self.lib.mgp_reset(self._h), "mgp_reset")
        self._keep = []

    def resident(self) -> tuple[int, int]:
        n, p = C.c_int64(), C.c_int64()
        _ck(self.lib.mgp_resident(self._h, C.byref(n), C.byref(p)), "mgp_resident")
        return int(n.value), int(p.value)

    def synth(self, seed: int, n_reads: int, cdf: np.ndarray, ref: np.ndarray, read_len: int = 50,
              rec_align: int = 64, pack: bool = True, rec_off: np.ndarray | None = None, payload_bytes: int = 0,
              cells: tuple[int, int] | None = None, shard: tuple[int, int] = (0, 0), pack32: int | None = None,
              pack32_dist: int = 5):
        """Device-side synthetic workload (replaces the resident set). rec_off: an
        explicit placement of the records (e.g. host placement of
        mgp_place_records, `synth.place_records`); None = dense in BAM order.
        cells=(lo, hi): only the reads of those cells of the n_reads-read global set
        (len(cdf) cells; this context's n_cells must be hi - lo), barcodes rebased to
        lo, plus the reads without a whitelisted barcode whose index % world == rank
        for shard=(rank, world) (world 0: none). pack32 (a min_baseq): 32-byte
        records made for that threshold and min_dist_from_end pack32_dist (MGP_FLAG_PACK32)
        instead of packed 64-byte ones."""
        cdf = np.ascontiguousarray(cdf, np.uint32)
        ref = np.ascontiguousarray(ref, np.uint8)
        ro = None if rec_off is None else np.ascontiguousarray(rec_off, np.uint64)
        lo, hi = cells if cells is not None else (0, 0)
        if ro is not None and cells is None and ro.shape[0] != n_reads:
            raise ValueError("rec_off must have n_reads entries")
        p = mgp_synth_params(int(seed), int(n_reads), int(read_len), int(cdf.shape[0]), _ptr(cdf), _ptr(ref),
                             int(rec_align), 2 if pack32 is not None else int(bool(pack)),
                             None if ro is None else _ptr(ro), int(payload_bytes) if ro is not None else 0, int(lo),
                             int(hi), int(shard[0]), int(shard[1]), int(pack32 or 0), int(pack32_dist),
                             0 if ro is None else int(ro.shape[0]))
        _ck(self.lib.mgp_synth_generate(self._h, C.byref(p)), "mgp_synth_generate")

    def download_inputs(self, columns: tuple[str, ...] | None = None, alloc=None) -> ReadSoA:
        """Resident inputs back on the host; `columns` limits the copy to those SoA
        fields (the others are empty arrays). alloc(n, dtype) -> array: where the
        columns go (e.g. views of a PinnedBuffer); np.zeros by default."""
        n, pay = self.resident()

        def col(name, dt, m):
            m = m if columns is None or name in columns else 0
            return alloc(m, dt) if alloc is not None and m else np.zeros(m, dt)

        soa = ReadSoA(
            col("start", np.int32, n), col("bc", np.int32, n), col("tlen", np.int32, n), col("flag", np.uint16, n),
            col("mapq", np.uint8, n), col("span", np.uint32, n), col("rec_off", np.uint64, n),
            col("payload", np.uint8, pay),
        )
        _ck(
            self.lib.mgp_download_inputs(
                self._h, *[_ptr(a) if a.shape[0] else None for a in (soa.start, soa.bc, soa.tlen, soa.flag,
                                                                        soa.mapq, soa.span, soa.rec_off,
                                                                        soa.payload)],
            ),
            "mgp_download_inputs",
        )
        return soa

    # -- compute -----------------------------------------------------------
    def run(self):
        _ck(self.lib.mgp_run(self._h), "mgp_run")

    def sync(self):
        code = self.lib.mgp_sync(self._h)
        self._keep = []
        _ck(code, "mgp_sync")

    def fetch(self, dense: bool = True) -> EngineResult:
        res = EngineResult.alloc(self.cfg.n_cells, self.cfg.mito_len, dense)
        st = mgp_stats()
        cres = res.to_c(st)
        _ck(self.lib.mgp_fetch(self._h, C.byref(cres)), "mgp_fetch")
        res.stats = st.as_dict()
        return res

    def fetch_cells(self, lo: int, hi: int, dense: bool = True) -> EngineResult:
        """mgp_fetch_cells: the results of cells [lo, hi) (cell lo at index 0)."""
        res = EngineResult.alloc(hi - lo, self.cfg.mito_len, dense)
        st = mgp_stats()
        cres = res.to_c(st)
        _ck(self.lib.mgp_fetch_cells(self._h, int(lo), int(hi), C.byref(cres)), "mgp_fetch_cells")
        res.stats = st.as_dict()
        return res

    def fetch_compact(self) -> EngineResult:
        """The run's results with the per-position arrays as the pileup's exact
        16-bit rows (u16 counts/tn5/depth: half the bytes of mgp_fetch's u32 arrays,
        no widening pass on the device). A run with a wide window (a cell window of
        more than 65535 reads) falls back to the exact u32 arrays."""
        res = self.fetch(dense=False)
        r16 = self.fetch_rows16()
        if r16.wide.any():
            return self.fetch(dense=True)
        res.counts, res.tn5, res.depth = r16.counts, r16.tn5, r16.depth
        return res

    def txt_gz(self, cells, names: list[str], out: np.ndarray | None = None) -> TxtMembers:
        """mgp_txt_gz_run + mgp_txt_gz_fetch: the txt count files' gzip members of the run's
        `cells` (context cell indices, in output order) named `names`, formatted and
        deflated on the device (writers.py:430-486). `out`: where the members go (e.g. a
        pinned buffer's view, large enough); a new array otherwise."""
        job, keep, mb, tb = _txt_job(cells, names)
        tot = C.c_int64()
        _ck(self.lib.mgp_txt_gz_run(self._h, C.byref(job), C.byref(tot)), "mgp_txt_gz_run")
        n = int(tot.value)
        if out is None or out.shape[0] < n:
            out = np.empty(max(1, n), np.uint8)
        _ck(self.lib.mgp_txt_gz_fetch(self._h, _ptr(out), int(out.shape[0])), "mgp_txt_gz_fetch")
        return TxtMembers(out[:n], mb, tb)

    def h5_tiles(self, cell_of_col, chunks: tuple[int, int] = (1000, 100), cols_per_call: int = 3200,
                 sums: dict | None = None, col_chunks: tuple[int, int] | None = None) -> dict:
        """mgp_h5_tiles_run / _fetch over every column chunk (cols_per_call columns at a
        time): the zlib streams of the HDF5 count datasets' chunks of the run
        (writers.py:60-131), {plane: [chunk (u8 array), row-major over the chunk grid]} for
        the planes of H5_PLANES; column j holds the run's cell cell_of_col[j] (-1: zeros).
        sums (a dict): filled with the per-position sums over the columns of the stored
        coverage / tn5 planes ("coverage", "tn5_fwd", "tn5_rev", int64 [L]). col_chunks
        (c0, c1): only those column chunks (the lists then row-major over that sub-grid)."""
        coc = np.ascontiguousarray(cell_of_col, np.int32)
        crow, ccol = int(chunks[0]), int(chunks[1])
        nrc = -(-self.cfg.mito_len // crow)
        c0, c1 = (0, -(-coc.size // ccol)) if col_chunks is None else (int(col_chunks[0]), int(col_chunks[1]))
        step = max(1, int(cols_per_call) // ccol)
        grid = {p: [[None] * (c1 - c0) for _ in range(nrc)] for p in H5_PLANES}
        L = self.cfg.mito_len
        acc = np.zeros((3, L), np.int64)
        part = np.zeros((3, L), np.int64)
        for lo in range(c0, c1, step):
            hi = min(c1, lo + step)
            cb = np.zeros(len(H5_PLANES) * nrc * (hi - lo), np.int64)
            job = mgp_h5_tiles(coc.size, _ptr(coc), crow, ccol, lo, hi, _ptr(cb), _ptr(part))
            tot = C.c_int64()
            _ck(self.lib.mgp_h5_tiles_run(self._h, C.byref(job), C.byref(tot)), "mgp_h5_tiles_run")
            buf = np.empty(max(1, int(tot.value)), np.uint8)
            _ck(self.lib.mgp_h5_tiles_fetch(self._h, _ptr(buf), int(buf.shape[0])), "mgp_h5_tiles_fetch")
            offs = np.concatenate([[0], np.cumsum(cb)]).tolist()
            k = 0
            for p in H5_PLANES:
                for rc in range(nrc):
                    row = grid[p][rc]
                    for cc in range(lo, hi):
                        row[cc - c0] = buf[offs[k]:offs[k + 1]]  # (views of the call's buffer)
                        k += 1
            acc += part
        if sums is not None:
            sums.update(coverage=acc[0], tn5_fwd=acc[1], tn5_rev=acc[2])
        return {p: [b for row in grid[p] for b in row] for p in H5_PLANES}

    def _variant_calls(self):
        def call(name, *args):
            _ck(getattr(self.lib, name + "_run")(self._h, *args), name + "_run")

        return _variant_calls(call, self.cfg.n_cells, self.cfg.mito_len)

    def _coverage_calls(self):
        def call(name, *args):
            _ck(getattr(self.lib, name + "_run")(self._h, *args), name + "_run")

        return _coverage_calls(call, self.cfg.n_cells, self.cfg.mito_len)

    def cell_coverage(self, cells=None) -> dict:
        """mgp_cell_coverage_run (after run()): per cell of the population `cells` (as for
        variant_moments), over all mito_len positions: CELL_COVERAGE_FIELDS arrays [n]: the
        depth's exact sum and sum of squares, max, the positions with depth > 0, >= 10,
        >= 50, and the two middle order statistics. Depths below 2^24, mito_len <= 2^16."""
        return self._coverage_calls()[0](cells)

    def position_coverage(self, cells=None) -> dict:
        """mgp_position_coverage_run: per position over the population, POSITION_COVERAGE_FIELDS
        arrays [L] (tally [L, 4]): the depth, strand and Tn5 sums, the cell counts and the max.
        At most VARIANT_MAX_CELLS cells per call, every depth and count below 2^24."""
        return self._coverage_calls()[1](cells)

    def position_depth_hist(self, shift: int, prefix=None, cells=None) -> dict:
        """mgp_position_depth_hist_run: {"hist": uint32 [L, 256]}, one round of the radix
        select over cells (analysis/coverage.py: position_medians drives it)."""
        return self._coverage_calls()[2](shift, prefix, cells)

    def position_depth_next(self, v, cells=None) -> dict:
        """mgp_position_depth_next_run: {"n_le": cells with depth <= v[p], "next": the smallest
        depth > v[p] (0xFFFFFFFF: none)}, uint32 [L] each."""
        return self._coverage_calls()[3](v, cells)

    def variant_moments(self, cells=None, low_coverage_threshold: int = 0) -> dict:
        """mgp_variant_moments_run (pass 1 of the variant statistics, after run()): the
        per-(position, base) moments over the population `cells` (context cell indices in
        order, -1 = an all-zero row; None = every cell) from the run's rows in HBM, as a
        dict of MOMENT_FIELDS arrays: exact uint64 sums, and s_af, the fp64 sum of the
        allele frequencies of the cells with depth >= low_coverage_threshold (0: all).
        At most VARIANT_MAX_CELLS cells per call, every count below 2^24."""
        return self._variant_calls()[0](cells, low_coverage_threshold)

    def group_moments(self, group, n_groups: int, cells=None, max_item_cells: int = 0) -> dict:
        """mgp_group_moments_run (after run(), or on a ready table): the pseudobulk of every group of the
        population `cells` (as for variant_moments) in one sweep. group[k] is entry k's label, 0 .. n_groups - 1
        or -1 (in no group). A dict of GROUP_FIELDS arrays: per group, position and base the exact sums of the
        fwd and of the rev counts ([n_groups, L, 4] uint64), the depth sum `cov` ([n_groups, L]), and the
        cells with fwd + rev > 0 (`n_det`) and with fwd >= 2 and rev >= 2 (`n_conf`, uint32). The same bytes
        for every max_item_cells (0: sized to fill the device). At most VARIANT_MAX_CELLS cells per call,
        every count below 2^24; more than GROUP_MAX_GROUPS groups go in several device calls."""
        def call(*args):
            _ck(self.lib.mgp_group_moments_run(self._h, *args), "mgp_group_moments_run")

        return _group_calls(call, self.cfg.n_cells, self.cfg.mito_len, group, n_groups, cells, max_item_cells)

    def variant_dev2(self, mean_af, cells=None, low_coverage_threshold: int = 0) -> np.ndarray:
        """mgp_variant_dev2_run (pass 2): [L, 4] sums of (af - mean_af)^2 over the cells of
        the population that are not low."""
        return self._variant_calls()[1](mean_af, cells, low_coverage_threshold)

    def allele_freq(self, variants, cells=None, min_coverage: int = 1) -> np.ndarray:
        """mgp_allele_freq_run: the heteroplasmy matrix [n_variants, n_cells] of `variants`
        ((0-based position, base 0..3) pairs) over the population: (fwd + rev) / depth
        where depth >= min_coverage, else 0."""
        return self._variant_calls()[2](variants, cells, min_coverage)

    def windows(self) -> tuple[int, int]:
        nw, w = C.c_int32(), C.c_int32()
        _ck(self.lib.mgp_windows(self._h, C.byref(nw), C.byref(w)), "mgp_windows")
        return int(nw.value), int(w.value)

    def fetch_rows16(self, lo: int = 0, hi: int | None = None, out: Rows16 | None = None) -> Rows16:
        """mgp_fetch_rows16: the 16-bit result rows of cells [lo, hi) (into `out`'s
        arrays when given, e.g. pinned host memory)."""
        hi = self.cfg.n_cells if hi is None else hi
        nw, w = self.windows()
        L, m = self.cfg.mito_len, hi - lo
        if out is None:
            out = Rows16(np.empty((m, L, 8), np.uint16), np.empty((m, L, 2), np.uint16), np.empty((m, L), np.uint16),
                         np.empty((m, nw), np.uint8), w)
        for a, shape in ((out.counts, (m, L, 8)), (out.tn5, (m, L, 2)), (out.depth, (m, L)), (out.wide, (m, nw))):
            if a.shape != shape or not a.flags["C_CONTIGUOUS"]:
                raise InvalidInputError(f"rows16 array of shape {a.shape}, expected {shape}")
        r = mgp_rows16(_ptr(out.counts), _ptr(out.tn5), _ptr(out.depth), _ptr(out.wide))
        _ck(self.lib.mgp_fetch_rows16(self._h, int(lo), int(hi), C.byref(r)), "mgp_fetch_rows16")
        return out

    def set_rows16_target(self, rows: Rows16 | None):
        """mgp_set_rows16_target: every run's 16-bit rows of all cells go to `rows`
        (pinned arrays, e.g. PinnedBuffer views) as its windows complete; sync() waits
        for them. None stops it."""
        if rows is None:
            _ck(self.lib.mgp_set_rows16_target(self._h, None), "mgp_set_rows16_target")
            self._rows_tgt = None
            return
        nw, _ = self.windows()
        L, m = self.cfg.mito_len, self.cfg.n_cells
        for a, shape in ((rows.counts, (m, L, 8)), (rows.tn5, (m, L, 2)), (rows.depth, (m, L)), (rows.wide, (m, nw))):
            if a.shape != shape or not a.flags["C_CONTIGUOUS"]:
                raise InvalidInputError(f"rows16 array of shape {a.shape}, expected {shape}")
        r = mgp_rows16(_ptr(rows.counts), _ptr(rows.tn5), _ptr(rows.depth), _ptr(rows.wide))
        _ck(self.lib.mgp_set_rows16_target(self._h, C.byref(r)), "mgp_set_rows16_target")
        self._rows_tgt = rows  # kept alive while the engine copies into it

    def set_rows_target(self, rows: Rows16 | None, rows8: Rows8 | None = None):
        """mgp_set_rows_target (ABI 7): set_rows16_target with the 8-bit target beside
        it (the windows whose values all fit a byte leave as half the bytes; merge_rows
        reads them back)."""
        if rows is None or rows8 is None:
            self.set_rows16_target(rows)
            return
        nw, _ = self.windows()
        L, m = self.cfg.mito_len, self.cfg.n_cells
        for a, shape in ((rows.counts, (m, L, 8)), (rows.tn5, (m, L, 2)), (rows.depth, (m, L)), (rows.wide, (m, nw)),
                         (rows8.counts, (m, L, 8)), (rows8.tn5, (m, L, 2)), (rows8.depth, (m, L)),
                         (rows8.narrow, (m, nw))):
            if a.shape != shape or not a.flags["C_CONTIGUOUS"]:
                raise InvalidInputError(f"rows array of shape {a.shape}, expected {shape}")
        r = mgp_rows16(_ptr(rows.counts), _ptr(rows.tn5), _ptr(rows.depth), _ptr(rows.wide))
        r8 = mgp_rows8(_ptr(rows8.counts), _ptr(rows8.tn5), _ptr(rows8.depth), _ptr(rows8.narrow))
        _ck(self.lib.mgp_set_rows_target(self._h, C.byref(r), C.byref(r8)), "mgp_set_rows_target")
        self._rows_tgt = (rows, rows8)

    def copy_wait(self):
        """mgp_copy_wait: every pushed batch's H2D copies are done (their host
        buffers may be reused). The batches stay referenced until the next sync."""
        _ck(self.lib.mgp_copy_wait(self._h), "mgp_copy_wait")

    def set_cell_range(self, lo: int, hi: int):
        """mgp_set_cell_range: this context's cells are whitelist indices [lo, hi) of the
        batches pushed from now on (hi - lo = its n_cells); the reads of other cells
        count only toward total_reads."""
        _ck(self.lib.mgp_set_cell_range(self._h, int(lo), int(hi)), "mgp_set_cell_range")

    def set_streaming(self, on: bool):
        """Streaming runs on or off for the next pushes (EngineConfig.stream initially)."""
        _ck(self.lib.mgp_set_streaming(self._h, int(bool(on))), "mgp_set_streaming")

    def stream_info(self) -> tuple[int, bool]:
        """(segments queued by pushes so far, whether the last run was streamed)."""
        n, last = C.c_int64(), C.c_int32()
        _ck(self.lib.mgp_stream_info(self._h, C.byref(n), C.byref(last)), "mgp_stream_info")
        return int(n.value), bool(last.value)

    def finish(self, dense: bool = True) -> EngineResult:
        self.run()
        return self.fetch(dense)

    def finish_raw(self) -> tuple[np.ndarray, np.ndarray]:
        """Unfiltered counts/Tn5 of a single-cell context (PileupGenerator.generate_pileup view)."""
        if self.cfg.n_cells != 1 or self.cfg.max_strand_bias < 1.0 or not self.cfg.keep_tn5:
            raise InvalidInputError("finish_raw needs n_cells=1, max_strand_bias>=1 and keep_tn5")
        self.run()
        r = self.fetch(dense=True)
        return r.counts[0], r.tn5[0]

    def kernel_times(self, last_runs: int = 1) -> dict[str, float]:
        """Per-stage device ms averaged over the last `last_runs` runs (HIP events)."""
        ms = (C.c_float * 32)()
        n = C.c_int()
        names = C.create_string_buffer(512)
        _ck(self.lib.mgp_kernel_times(self._h, int(last_runs), ms, 32, C.byref(n), names, 512), "mgp_kernel_times")
        keys = names.value.decode().split(",")
        return {k: float(ms[i]) for i, k in enumerate(keys[: n.value])}

    def set_stage_timing(self, all_stages: bool = True):
        """HIP events around every stage of the next runs (default), or around the
        pileup only: each event is a marker between two kernels of the stream."""
        _ck(self.lib.mgp_set_stage_timing(self._h, int(bool(all_stages))), "mgp_set_stage_timing")

    # -- multi-GPU ---------------------------------------------------------
    @staticmethod
    def comm_unique_id() -> bytes:
        lib = load_library()
        buf = C.create_string_buffer(128)
        _ck(lib.mgp_comm_unique_id(buf), "mgp_comm_unique_id")
        return buf.raw

    def comm_init(self, uid: bytes, nranks: int, rank: int):
        if len(uid) != 128:
            raise InvalidInputError("RCCL unique id must be 128 bytes")
        _ck(self.lib.mgp_comm_init(self._h, C.c_char_p(uid), int(nranks), int(rank)), "mgp_comm_init")


class _PinnedView:
    """numpy array-interface holder that keeps its PinnedBuffer alive."""

    def __init__(self, owner, addr: int, shape, dtype):
        self._owner = owner
        self.__array_interface__ = {"data": (addr, False), "shape": tuple(shape), "typestr": np.dtype(dtype).str,
                                    "version": 3}


class PinnedBuffer:
    """Page-locked host memory from mgp_host_alloc (hipHostMalloc): H2D/D2H copies
    from it run asynchronously at the link's rate. `array(shape, dtype, offset)`
    gives numpy views, which keep the buffer alive."""

    def __init__(self, nbytes: int):
        self.lib = load_library()
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        _ck(self.lib.mgp_host_alloc(max(self.nbytes, 1), C.byref(p)), "mgp_host_alloc")
        self._p = p

    def array(self, shape, dtype, offset: int = 0) -> np.ndarray:
        dt = np.dtype(dtype)
        shape = (int(shape),) if np.ndim(shape) == 0 else tuple(int(x) for x in shape)
        count = int(np.prod(shape))
        if offset % dt.itemsize or offset + count * dt.itemsize > self.nbytes:
            raise ValueError("pinned view outside the buffer or misaligned")
        return np.asarray(_PinnedView(self, self._p.value + offset, shape, dt))

    def __del__(self):
        try:
            if getattr(self, "_p", None) is not None and self._p.value:
                self.lib.mgp_host_free(self._p)
                self._p = None
        except Exception:
            pass


def device_count() -> int:
    lib = load_library()
    n = C.c_int()
    code = lib.mgp_device_count(C.byref(n))
    return int(n.value) if code == MGP_OK else 0
