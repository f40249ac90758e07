"""ctypes binding of libpgenhip.so -- one Python method per C entry point of
``include/pgenhip.h``.  Thin on purpose: argument marshalling and status ->
exception translation only (PGH_ERR_ARG -> ValueError ~ InvalidInputException,
everything else -> IOError ~ IOException, the reference's convention,
src/plink_freq.cpp:152,181,485)."""

from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# PGENHIP_LIB: another build of the library (tools/i8_experiment.sh's knock-out builds live under /tmp and never
# replace the in-tree file)
LIB_PATH = os.environ.get("PGENHIP_LIB") or os.path.join(_HERE, "libpgenhip.so")

ERRBUF_LEN = 256
PGH_OK, PGH_ERR_OPEN, PGH_ERR_FORMAT, PGH_ERR_ARG, PGH_ERR_DEVICE, PGH_ERR_NOMEM, PGH_ERR_UNSUPPORTED = range(7)
SCORE_MEAN_IMPUTE, SCORE_NO_MEAN_IMPUTATION, SCORE_CENTER = 0, 1, 2

# every symbol include/pgenhip.h declares (tests/test_abi.py checks the .so exports each)
EXPORTED_SYMBOLS = [
    "pgh_version", "pgh_device_count", "pgh_set_device", "pgh_open", "pgh_probe", "pgh_normalize_range_host",
    "pgh_from_host_rows", "pgh_open_sharded", "pgh_group_create", "pgh_group_uses_rccl", "pgh_shard_count", "pgh_shard",
    "pgh_synth_create", "pgh_synth_record_host", "pgh_synth_write_files", "pgh_copy_rows_to_host", "pgh_get_info", "pgh_device_rows",
    "pgh_close", "pgh_subset_create", "pgh_subset_size", "pgh_subset_destroy", "pgh_counts_range",
    "pgh_counts_range_dev", "pgh_freq_from_counts_dev", "pgh_fused_tally_dev", "pgh_missing_per_sample", "pgh_missing_per_sample_dev", "pgh_unpack_range",
    "pgh_unpack_range_dev", "pgh_probe_unpack_shape_dev", "pgh_score", "pgh_score_counts", "pgh_score_dev", "pgh_score_plan_create", "pgh_score_run_dev",
    "pgh_score_plan_destroy", "pgh_pca", "pgh_pca_sharded", "pgh_pca_streamed", "pgh_ld_pairs", "pgh_ld_pairs_dev", "pgh_ld_pairs_status", "pgh_sample_counts", "pgh_sample_counts_dev",
    "pgh_synth_add_dosage", "pgh_synth_write_dosage_files", "pgh_dosage_sums", "pgh_dosage_sums_dev", "pgh_dosage_unpack", "pgh_dosage_unpack_dev", "pgh_unpack_samples", "pgh_dosage_unpack_samples", "pgh_reader_create", "pgh_reader_destroy",
    "pgh_reader_unpack_start", "pgh_reader_unpack_wait", "pgh_get_2bit", "pgh_get_counts", "pgh_get_missingness", "pgh_get_int8", "pgh_get_dosage_f64", "pgh_get_phased",
    "pgh_tally_start", "pgh_tally_request", "pgh_tally_wait", "pgh_tally_counts", "pgh_tally_hwe_lnp",
    "pgh_tally_sample_missing", "pgh_tally_destroy", "pgh_tally_passes_started", "pgh_host_alloc", "pgh_host_free", "pgh_trim_device_cache",
    "pgh_reader_error", "pgh_open_sparse", "pgh_get_sparse_info", "pgh_sparse_opens_started", "pgh_glm", "pgh_glm_multi", "pgh_glm_sparse", "pgh_glm_score_sparse", "pgh_glm_score_multi", "pgh_glm_score_multi_dosage", "pgh_glm_score_multi_dosage_spa", "pgh_glm_score_sparse_spa", "pgh_glm_score_multi_spa", "pgh_glm_score_multi_firth", "pgh_glm_score_multi_dosage_firth", "pgh_glm_score_sparse_firth", "pgh_glm_score_sparse_multi", "pgh_glm_sparse_multi", "pgh_glm_score_sparse_multi_spa", "pgh_glm_score_sparse_multi_firth", "pgh_burden_sparse", "pgh_skat_sparse", "pgh_skat_p_from_lambda", "pgh_symmetric_eigenvalues", "pgh_score_sparse", "pgh_glm_p_from_t", "pgh_glm_p_from_z", "pgh_hwe_lnp", "pgh_hwe_xchr_lnp", "pgh_hwe_lnp_batch", "pgh_hwe_lnp_batch_dev", "pgh_hwe_xchr_lnp_batch",
    "pgh_king_counts", "pgh_king_table", "pgh_king_kinship",
    "pgh_ld_window_sums", "pgh_ld_prune", "pgh_ld_exceeds", "pgh_ld_scores", "pgh_ld_r2",
    "pgh_grm", "pgh_grm_standardize",
    "pgh_het", "pgh_het_expected", "pgh_het_scale",
]


class PghInfo(C.Structure):
    _fields_ = [
        ("raw_variant_ct", C.c_uint32), ("raw_sample_ct", C.c_uint32), ("variant_begin", C.c_uint32),
        ("variant_end", C.c_uint32), ("has_dosage", C.c_uint32), ("has_phase", C.c_uint32),
        ("max_record_bytes", C.c_uint32), ("record_bytes", C.c_uint32), ("pitch_bytes", C.c_uint64),
        ("vrtype_hist", C.c_uint32 * 8), ("device", C.c_int32),
        ("dosage_variant_ct", C.c_uint32), ("dosage_value_ct", C.c_uint64),
    ]


class PghSparseInfo(C.Structure):
    _fields_ = [
        ("sparse_variant_ct", C.c_uint32), ("dense_variant_ct", C.c_uint32), ("entry_ct", C.c_uint64),
        ("resident_bytes", C.c_uint64), ("dense_bytes", C.c_uint64), ("base_hist", C.c_uint32 * 4),
    ]


# pgh_allreduce_fn(ctx, d_buf, count, stream) -> 0 on success
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p)


GLM_LINEAR, GLM_LOGISTIC = 0, 1
# pgh_glm_row.errcode -> the reference's ERRCODE strings (None = NULL)
GLM_ERRCODES = [None, "TOO_FEW_SAMPLES", "CONST_ALLELE", "ZERO_VARIANCE", "SINGULAR_MATRIX", "NO_CONVERGENCE",
                "SEPARATION"]
GLM_MAX_COVAR = 20


class PghGlmRow(C.Structure):
    _fields_ = [
        ("beta", C.c_double), ("se", C.c_double), ("stat", C.c_double), ("p", C.c_double), ("a1_freq", C.c_double),
        ("obs_ct", C.c_uint32), ("errcode", C.c_uint8), ("firth", C.c_uint8), ("pad", C.c_uint8 * 2),
    ]


class PghBurdenRow(C.Structure):
    _fields_ = [
        ("beta", C.c_double), ("se", C.c_double), ("stat", C.c_double), ("p", C.c_double), ("mean", C.c_double),
        ("obs_ct", C.c_uint32), ("n_nonzero", C.c_uint32), ("errcode", C.c_uint8), ("pad", C.c_uint8 * 7),
    ]


class PghHetRow(C.Structure):
    _fields_ = [
        ("e_hom", C.c_double), ("f", C.c_double), ("e_sum", C.c_int64), ("hom_ct", C.c_uint32), ("obs_ct", C.c_uint32),
    ]


class PghSkatRow(C.Structure):
    _fields_ = [
        ("q", C.c_double), ("p_skat", C.c_double), ("beta", C.c_double), ("se", C.c_double), ("stat", C.c_double),
        ("p", C.c_double), ("lambda_sum", C.c_double), ("lambda_max", C.c_double), ("obs_ct", C.c_uint32),
        ("n_carriers", C.c_uint32), ("n_lambda", C.c_uint32), ("errcode", C.c_uint8), ("p_state", C.c_uint8),
        ("pad", C.c_uint8 * 2),
    ]


# pgh_king_counts' planes, pgh_king_pair, and the kernel's tile of sample pairs (a test of tile edges names it)
KING_NSNP, KING_HETHET, KING_IBS0, KING_HET1HOM2, KING_HET2HOM1, KING_PLANES = 0, 1, 2, 3, 4, 5
KING_TILE = 128
KING_PAIR_DTYPE = np.dtype([("i", "<u4"), ("j", "<u4"), ("nsnp", "<u4"), ("hethet", "<u4"), ("ibs0", "<u4"),
                            ("het1hom2", "<u4"), ("het2hom1", "<u4"), ("pad", "<u4"), ("kinship", "<f8")])
# pgh_ld_window_sums' planes (pgh_ld_pairs' order), the kernel's tile of variant pairs (anchors x partners; a test of
# tile edges names it) and the environment variable that sets pgh_ld_prune's launch size in tiles
LD_N, LD_SUM_A, LD_SUM_B, LD_SUM_AB, LD_SUM_A2, LD_SUM_B2, LD_PLANES = 0, 1, 2, 3, 4, 5, 6
LD_TILE_A, LD_TILE_B = 96, 128
LD_PRUNE_CHUNK_ENV = "PGH_LD_PRUNE_CHUNK_TILES"
# pgh_ld_scores' flag and the environment variable that sets its launch size in tiles (results do not depend on it)
LDSCORE_UNBIASED = 1
LD_SCORE_CHUNK_ENV = "PGH_LD_SCORE_CHUNK_TILES"
# pgh_grm's flag, the kernel's tile of sample pairs (a test of tile edges names it) and the environment variable that
# lowers the byte budget of a band of rows (results do not depend on it)
GRM_MEANIMPUTE = 1
GRM_TILE = 128
GRM_BAND_ENV = "PGH_GRM_BAND_BYTES"
# pgh_het's flag, the kernel's tile of samples (a test of tile edges names it), the environment variable that sets the
# variant slices of its grid (results do not depend on it) and pgh_het_row
HET_SMALL_SAMPLE = 1
HET_TILE = 4096
HET_SLICES_ENV = "PGH_HET_SLICES"
HET_ROW_DTYPE = np.dtype([("e_hom", "<f8"), ("f", "<f8"), ("e_sum", "<i8"), ("hom_ct", "<u4"), ("obs_ct", "<u4")])
GLM_ROW_DTYPE = np.dtype([("beta", "<f8"), ("se", "<f8"), ("stat", "<f8"), ("p", "<f8"), ("a1_freq", "<f8"),
                          ("obs_ct", "<u4"), ("errcode", "u1"), ("firth", "u1"), ("pad", "u1", (2,))])
# pgh_glm_firth_row
GLM_FIRTH_ROW_DTYPE = np.dtype([("beta", "<f8"), ("se", "<f8"), ("p", "<f8"), ("state", "u1"), ("pad", "u1", (7,))])
# pgh_burden_row, and the environment variable that bounds pgh_burden_sparse's device scratch (results do not depend
# on it)
BURDEN_ROW_DTYPE = np.dtype([("beta", "<f8"), ("se", "<f8"), ("stat", "<f8"), ("p", "<f8"), ("mean", "<f8"),
                             ("obs_ct", "<u4"), ("n_nonzero", "<u4"), ("errcode", "u1"), ("pad", "u1", (7,))])
BURDEN_SCRATCH_ENV = "PGH_BURDEN_SCRATCH_BYTES"
# pgh_skat_row, the largest set, pgh_skat_row.p_state's values and the environment variable that bounds
# pgh_skat_sparse's device scratch (results do not depend on it)
SKAT_ROW_DTYPE = np.dtype([("q", "<f8"), ("p_skat", "<f8"), ("beta", "<f8"), ("se", "<f8"), ("stat", "<f8"),
                           ("p", "<f8"), ("lambda_sum", "<f8"), ("lambda_max", "<f8"), ("obs_ct", "<u4"),
                           ("n_carriers", "<u4"), ("n_lambda", "<u4"), ("errcode", "u1"), ("p_state", "u1"),
                           ("pad", "u1", (2,))])
SKAT_MAX_SET = 256
SKAT_P_NONE, SKAT_P_EXACT, SKAT_P_SADDLEPOINT, SKAT_P_NEAR_MEAN, SKAT_P_FAILED = range(5)
SKAT_SCRATCH_ENV = "PGH_SKAT_SCRATCH_BYTES"
# pgh_score_sparse: weight columns per walk of the entries, the LDS bytes of a sample tile's accumulators (a tile holds
# SCORE_SPARSE_ACC_BYTES // (8 * accumulators + 4) samples, rounded down to a multiple of 64) and the environment
# variable that sets the row slices per tile (results do not depend on it)
SCORE_SPARSE_CHUNK = 8
SCORE_SPARSE_ACC_BYTES = 131072
SCORE_SPARSE_SLICES_ENV = "PGH_SCORE_SPARSE_SLICES"


class PghError(IOError):
    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


class PghArgError(ValueError):
    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with plinking_duck_amd/csrc/build.sh "
            "(python -c 'import __graft_entry__ as g; g.build()').  There is no CPU fallback.")
    # PyTorch-ROCm wheels bundle their own HIP runtime (torch/lib/libamdhip64.so).  A process that
    # ends up with two HIP runtimes -- this library bound to /opt/rocm first, torch's loaded later --
    # leaves the second one without a device ("No HIP GPUs are available").  Loading torch first makes
    # both bind the same runtime, so do that whenever torch is installed; the library itself needs
    # neither torch nor Python.
    if os.environ.get("PGH_NO_TORCH_PRELOAD", "") in ("", "0"):
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    lib = C.CDLL(LIB_PATH)
    vp, u32, u64, i32, cp = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int32, C.c_char_p
    sigs = {
        "pgh_version": (cp, []),
        "pgh_device_count": (C.c_int, []),
        "pgh_set_device": (C.c_int, [C.c_int, cp]),
        "pgh_open": (C.c_int, [cp, cp, u32, u32, C.POINTER(vp), cp]),
        "pgh_probe": (C.c_int, [cp, cp, C.POINTER(PghInfo), cp]),
        "pgh_normalize_range_host": (C.c_int, [cp, cp, u32, u32, vp, C.c_size_t, cp]),
        "pgh_from_host_rows": (C.c_int, [vp, C.c_size_t, u32, u32, C.POINTER(vp), cp]),
        "pgh_synth_create": (C.c_int, [u32, u32, u32, u64, C.c_double, C.POINTER(vp), cp]),
        "pgh_open_sharded": (C.c_int, [cp, cp, u32, u32, vp, u32, C.POINTER(vp), cp]),
        "pgh_group_create": (C.c_int, [vp, u32, C.POINTER(vp), cp]),
        "pgh_shard_count": (u32, [vp]),
        "pgh_group_uses_rccl": (C.c_int, [vp]),
        "pgh_shard": (vp, [vp, u32]),
        "pgh_synth_record_host": (C.c_int, [u32, u32, u64, C.c_double, vp]),
        "pgh_synth_write_files": (C.c_int, [cp, u32, u32, u64, C.c_double, cp]),
        "pgh_copy_rows_to_host": (C.c_int, [vp, u32, u32, vp, C.c_size_t, cp]),
        "pgh_freq_from_counts_dev": (C.c_int, [vp, u32, vp, vp, vp, cp]),
        "pgh_hwe_lnp_batch_dev": (C.c_int, [vp, u32, u32, vp, vp, cp]),
        "pgh_get_info": (C.c_int, [vp, C.POINTER(PghInfo)]),
        "pgh_device_rows": (vp, [vp]),
        "pgh_close": (None, [vp]),
        "pgh_subset_create": (C.c_int, [vp, vp, C.POINTER(vp), cp]),
        "pgh_subset_size": (u32, [vp]),
        "pgh_subset_destroy": (None, [vp]),
        "pgh_counts_range": (C.c_int, [vp, vp, u32, u32, vp, cp]),
        "pgh_counts_range_dev": (C.c_int, [vp, vp, u32, u32, vp, vp, cp]),
        "pgh_fused_tally_dev": (C.c_int, [vp, u32, u32, vp, vp, vp, cp]),
        "pgh_missing_per_sample": (C.c_int, [vp, vp, u32, u32, vp, cp]),
        "pgh_missing_per_sample_dev": (C.c_int, [vp, u32, u32, vp, vp, cp]),
        "pgh_unpack_range": (C.c_int, [vp, vp, u32, u32, vp, vp, C.c_int, cp]),
        "pgh_unpack_range_dev": (C.c_int, [vp, vp, u32, u32, vp, C.c_size_t, vp, C.c_int, vp, cp]),
        "pgh_probe_unpack_shape_dev": (C.c_int, [vp, C.c_size_t, vp, vp, vp, cp]),
        "pgh_score": (C.c_int, [vp, vp, u32, vp, vp, vp, u32, C.c_int, vp, vp, vp, cp]),
        "pgh_score_dev": (C.c_int, [vp, vp, u32, vp, vp, vp, u32, C.c_int, vp, vp, vp, vp, cp]),
        "pgh_score_counts": (C.c_int, [vp, vp, u32, vp, vp, vp, u32, C.c_int, vp, vp, vp, vp, cp]),
        "pgh_score_plan_create": (C.c_int, [vp, vp, u32, vp, vp, vp, u32, C.c_int, C.POINTER(vp), cp]),
        "pgh_score_run_dev": (C.c_int, [vp, vp, vp, vp, vp, cp]),
        "pgh_score_plan_destroy": (None, [vp]),
        "pgh_pca": (C.c_int, [vp, vp, u32, vp, vp, vp, u32, vp, vp, vp, cp]),
        "pgh_ld_pairs": (C.c_int, [vp, vp, u32, vp, vp, vp, cp]),
        "pgh_hwe_xchr_lnp_batch": (C.c_int, [vp, u32, u32, vp, cp]),
        "pgh_sample_counts": (C.c_int, [vp, vp, u32, u32, vp, vp, cp]),
        "pgh_sample_counts_dev": (C.c_int, [vp, u32, u32, vp, vp, cp]),
        "pgh_synth_add_dosage": (C.c_int, [vp, C.c_double, C.c_uint64, cp]),
        "pgh_synth_write_dosage_files": (C.c_int, [cp, u32, u32, C.c_uint64, C.c_double, C.c_double, cp]),
        "pgh_dosage_sums": (C.c_int, [vp, vp, u32, u32, vp, vp, cp]),
        "pgh_dosage_sums_dev": (C.c_int, [vp, vp, u32, u32, vp, vp, cp]),
        "pgh_dosage_unpack": (C.c_int, [vp, vp, u32, u32, vp, vp, cp]),
        "pgh_unpack_samples": (C.c_int, [vp, vp, u32, vp, vp, C.c_int, cp]),
        "pgh_dosage_unpack_samples": (C.c_int, [vp, vp, u32, vp, vp, cp]),
        "pgh_dosage_unpack_dev": (C.c_int, [vp, vp, u32, u32, vp, C.c_size_t, vp, cp]),
        "pgh_ld_pairs_dev": (C.c_int, [vp, vp, u32, vp, vp, vp, vp, cp]),
        "pgh_ld_pairs_status": (C.c_int, [cp]),
        "pgh_pca_sharded": (C.c_int, [vp, vp, u32, vp, vp, vp, C.c_uint64, u32, vp, ALLREDUCE_FN, vp, vp, vp, cp]),
        "pgh_pca_streamed": (C.c_int, [C.c_char_p, C.c_char_p, vp, u32, vp, vp, vp, u32, vp, C.c_uint64, vp, vp, cp]),
        "pgh_reader_create": (C.c_int, [vp, vp, C.POINTER(vp), cp]),
        "pgh_reader_destroy": (None, [vp]),
        "pgh_reader_unpack_start": (C.c_int, [vp, C.c_int, u32, u32, vp, vp, C.c_int]),
        "pgh_reader_unpack_wait": (C.c_int, [vp, C.c_int]),
        "pgh_get_2bit": (C.c_int, [vp, u32, vp]),
        "pgh_get_counts": (C.c_int, [vp, u32, vp]),
        "pgh_get_missingness": (C.c_int, [vp, u32, vp]),
        "pgh_get_int8": (C.c_int, [vp, u32, vp]),
        "pgh_get_dosage_f64": (C.c_int, [vp, u32, vp]),
        "pgh_get_phased": (C.c_int, [vp, u32, vp, vp, vp]),
        "pgh_reader_error": (cp, [vp]),
        "pgh_hwe_lnp": (C.c_double, [i32, i32, i32, u32]),
        "pgh_hwe_xchr_lnp": (C.c_double, [i32, i32, i32, i32, i32, u32]),
        "pgh_hwe_lnp_batch": (C.c_int, [vp, u32, u32, vp, cp]),
        "pgh_tally_start": (C.c_int, [vp, vp, u32, u32, u32, C.POINTER(vp), cp]),
        "pgh_tally_request": (C.c_int, [vp, u32, cp]),
        "pgh_tally_wait": (C.c_int, [vp, u32, u32, u32, cp]),
        "pgh_tally_counts": (vp, [vp]),
        "pgh_tally_hwe_lnp": (vp, [vp, u32]),
        "pgh_tally_sample_missing": (C.c_int, [vp, vp, cp]),
        "pgh_tally_destroy": (None, [vp]),
        "pgh_tally_passes_started": (u64, []),
        "pgh_open_sparse": (C.c_int, [cp, cp, u32, u32, u32, C.POINTER(vp), cp]),
        "pgh_get_sparse_info": (C.c_int, [vp, C.POINTER(PghSparseInfo)]),
        "pgh_sparse_opens_started": (u64, []),
        "pgh_host_alloc": (C.c_int, [C.c_size_t, C.POINTER(vp), cp]),
        "pgh_host_free": (None, [vp]),
        "pgh_trim_device_cache": (None, []),
        "pgh_glm": (C.c_int, [vp, vp, u32, u32, vp, u32, vp, C.c_int, C.c_int, vp, cp]),
        "pgh_glm_multi": (C.c_int, [vp, vp, u32, u32, u32, vp, u32, vp, C.c_int, C.c_int, vp, cp]),
        "pgh_glm_sparse": (C.c_int, [vp, vp, u32, u32, vp, u32, vp, vp, cp]),
        "pgh_glm_score_sparse": (C.c_int, [vp, vp, u32, u32, vp, u32, vp, vp, cp]),
        "pgh_glm_score_multi": (C.c_int, [vp, vp, u32, u32, u32, vp, u32, vp, vp, cp]),
        "pgh_glm_score_multi_dosage": (C.c_int, [vp, vp, u32, u32, u32, vp, u32, vp, vp, cp]),
        "pgh_glm_score_sparse_multi": (C.c_int, [vp, vp, u32, u32, u32, vp, u32, vp, vp, cp]),
        "pgh_glm_sparse_multi": (C.c_int, [vp, vp, u32, u32, u32, vp, u32, vp, vp, cp]),
        "pgh_glm_score_sparse_spa": (C.c_int, [vp, vp, u32, u32, vp, u32, vp, C.c_double, vp, vp, vp, cp]),
        "pgh_glm_score_multi_spa": (C.c_int, [vp, vp, u32, u32, u32, vp, u32, vp, C.c_double, vp, vp, vp, cp]),
        "pgh_glm_score_multi_dosage_spa": (C.c_int, [vp, vp, u32, u32, u32, vp, u32, vp, C.c_double, vp, vp, vp, cp]),
        "pgh_glm_score_sparse_multi_spa": (C.c_int, [vp, vp, u32, u32, u32, vp, u32, vp, C.c_double, vp, vp, vp, cp]),
        "pgh_glm_score_multi_firth": (C.c_int, [vp, vp, u32, u32, u32, vp, u32, vp, C.c_double, vp, vp, cp]),
        "pgh_glm_score_multi_dosage_firth": (C.c_int, [vp, vp, u32, u32, u32, vp, u32, vp, C.c_double, vp, vp, cp]),
        "pgh_glm_score_sparse_multi_firth": (C.c_int, [vp, vp, u32, u32, u32, vp, u32, vp, C.c_double, vp, vp, cp]),
        "pgh_glm_score_sparse_firth": (C.c_int, [vp, vp, u32, u32, vp, u32, vp, C.c_double, vp, vp, cp]),
        "pgh_burden_sparse": (C.c_int, [vp, vp, vp, u32, vp, u32, vp, vp, vp, vp, cp]),
        "pgh_skat_sparse": (C.c_int, [vp, vp, vp, u32, vp, u32, vp, vp, vp, vp, vp, cp]),
        "pgh_skat_p_from_lambda": (C.c_double, [C.c_double, vp, u32, vp]),
        "pgh_symmetric_eigenvalues": (C.c_int, [vp, u32, vp]),
        "pgh_score_sparse": (C.c_int, [vp, vp, u32, vp, vp, vp, u32, C.c_int, vp, vp, vp, cp]),
        "pgh_glm_p_from_t": (C.c_double, [C.c_double, C.c_double]),
        "pgh_glm_p_from_z": (C.c_double, [C.c_double]),
        "pgh_king_counts": (C.c_int, [vp, vp, u32, u32, vp, u32, u32, u32, u32, vp, cp]),
        "pgh_king_table": (C.c_int, [vp, vp, u32, u32, vp, C.c_double, vp, u64, C.POINTER(u64), cp]),
        "pgh_king_kinship": (C.c_double, [u32, u32, u32, u32]),
        "pgh_ld_window_sums": (C.c_int, [vp, vp, u32, u32, vp, u32, u32, u32, u32, vp, cp]),
        "pgh_ld_prune": (C.c_int, [vp, vp, u32, u32, vp, vp, C.c_double, vp, C.POINTER(u64), cp]),
        "pgh_ld_exceeds": (C.c_int, [vp, C.c_double]),
        "pgh_ld_scores": (C.c_int, [vp, vp, u32, u32, vp, vp, u32, vp, vp, cp]),
        "pgh_ld_r2": (C.c_int, [vp, u32, C.POINTER(C.c_double)]),
        "pgh_grm": (C.c_int, [vp, vp, u32, u32, vp, vp, u32, u32, u32, u32, u32, vp, vp, C.POINTER(u32), cp]),
        "pgh_grm_standardize": (C.c_double, [u32, u32, u32, vp]),
        "pgh_het": (C.c_int, [vp, vp, u32, u32, vp, vp, u32, vp, vp, C.POINTER(u32), cp]),
        "pgh_het_expected": (C.c_int, [u32, u32, u32, C.c_double, u32, C.POINTER(C.c_double)]),
        "pgh_het_scale": (u32, [u32]),
    }
    for name, (res, args) in sigs.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


_lib = _load()


def raw():
    """The ctypes CDLL (for tests that probe the ABI directly)."""
    return _lib


def _check(rc, errbuf):
    if rc == PGH_OK:
        return
    msg = errbuf.value.decode("utf-8", "replace") if errbuf is not None else f"pgenhip error {rc}"
    if rc == PGH_ERR_ARG:
        raise PghArgError(rc, msg)
    raise PghError(rc, msg)


def _errbuf():
    return C.create_string_buffer(ERRBUF_LEN)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def glm_p_from_t(t: float, df: float) -> float:
    """Two-sided p of Student's t with df degrees of freedom (the reference's TstatToPvalue)."""
    return _lib.pgh_glm_p_from_t(float(t), float(df))


def glm_p_from_z(z: float) -> float:
    """Two-sided p of a standard normal z (ZstatToPvalue)."""
    return _lib.pgh_glm_p_from_z(float(z))


def skat_p_from_lambda(q: float, lam, return_state: bool = False):
    """pgh_skat_p_from_lambda: the upper tail of sum_k lam[k] chi^2_1 at q (exact for one eigenvalue, Kuonen's
    saddlepoint approximation otherwise).  With return_state also the state, SKAT_P_*."""
    a = np.ascontiguousarray(lam, dtype=np.float64)
    if a.ndim != 1:
        raise ValueError("lam must be a one-dimensional array of eigenvalues")
    state = C.c_uint8(0)
    p = _lib.pgh_skat_p_from_lambda(float(q), _ptr(a) if a.size else None, a.size, C.byref(state))
    return (p, state.value) if return_state else p


def symmetric_eigenvalues(a) -> np.ndarray:
    """pgh_symmetric_eigenvalues: the eigenvalues of a symmetric matrix, descending."""
    m = np.ascontiguousarray(a, dtype=np.float64)
    if m.ndim != 2 or m.shape[0] != m.shape[1] or m.shape[0] == 0:
        raise ValueError(f"a must be a square matrix, got shape {m.shape}")
    out = np.zeros(m.shape[0], dtype=np.float64)
    rc = _lib.pgh_symmetric_eigenvalues(_ptr(m), m.shape[0], _ptr(out))
    if rc != PGH_OK:
        raise PghArgError(rc, "pgh_symmetric_eigenvalues refused its arguments")
    return out


def king_kinship(hethet: int, ibs0: int, het1hom2: int, het2hom1: int) -> float:
    """pgh_king_kinship: 0.5 - (4 IBS0 + HET1HOM2 + HET2HOM1) / (4 (HETHET + min(HET1HOM2, HET2HOM1))), NaN when the
    denominator is zero -- the function king_table's kinship column is of its own counts."""
    return _lib.pgh_king_kinship(int(hethet), int(ibs0), int(het1hom2), int(het2hom1))


def grm_standardize(het: int, alt: int, called: int):
    """pgh_grm_standardize: (p, z) with p = (het + 2 alt) / (2 called) and z[c] = (c - 2 p) / sqrt((2 p) (1 - p)) for
    the codes 0, 1, 2 -- the table pgh_grm builds per variant.  (NaN, None) when the variant is skipped: nothing
    called, p <= 0 or p >= 1."""
    z = np.zeros(3, dtype=np.float64)
    p = _lib.pgh_grm_standardize(int(het), int(alt), int(called), _ptr(z))
    return (p, None) if p != p else (p, z)


def het_expected(het: int, alt: int, called: int, freq: float | None = None, small_sample: bool = True):
    """pgh_het_expected: e = 1 - (2 p)(1 - p) [times 2 called / (2 called - 1) with small_sample] of one variant, with
    p = (het + 2 alt) / (2 called) or `freq` -- the expected homozygosity pgh_het sums per sample.  None when the
    variant is skipped: nothing called, p not finite, p <= 0 or p >= 1 (and for freq together with small_sample)."""
    e = C.c_double(0.0)
    used = _lib.pgh_het_expected(int(het), int(alt), int(called), float("nan") if freq is None else float(freq),
                                 HET_SMALL_SAMPLE if small_sample else 0, C.byref(e))
    return e.value if used else None


def het_scale(n_var: int) -> int:
    """pgh_het_scale: k = 62 - L with L the smallest integer with 2^L >= max(n_var, 1) -- pgh_het's fixed-point sums
    are multiples of 2^-k."""
    return int(_lib.pgh_het_scale(int(n_var)))


def ld_exceeds(sums, r2: float) -> bool:
    """pgh_ld_exceeds: whether sums = (n, sum_a, sum_b, sum_ab, sum_a2, sum_b2) has r2 > `r2` -- in int64
    num = n sum_ab - sum_a sum_b, va = n sum_a2 - sum_a^2, vb = n sum_b2 - sum_b^2; never when n < 2, va <= 0 or
    vb <= 0; else (float(num) * float(num)) / (float(va) * float(vb)) > r2.  The function ld_prune applies to every
    pair of its band."""
    s = np.ascontiguousarray(sums, dtype=np.uint32)
    if s.shape != (6,):
        raise ValueError(f"ld_exceeds: six sums expected, got shape {s.shape}")
    return bool(_lib.pgh_ld_exceeds(_ptr(s), float(r2)))


def ld_r2(sums, unbiased: bool = False):
    """pgh_ld_r2: the term a pair with sums = (n, sum_a, sum_b, sum_ab, sum_a2, sum_b2) adds to an LD score, or None
    when the pair has no r2 (n < 2, or n < 3 with unbiased; va <= 0 or vb <= 0).  r2 = (float(num) * float(num)) /
    (float(va) * float(vb)) as in ld_exceeds; unbiased: r2 - (1.0 - r2) / float(n - 2).  The function ld_scores
    applies to every pair of its band."""
    s = np.ascontiguousarray(sums, dtype=np.uint32)
    if s.shape != (6,):
        raise ValueError(f"ld_r2: six sums expected, got shape {s.shape}")
    term = C.c_double(0.0)
    ok = _lib.pgh_ld_r2(_ptr(s), LDSCORE_UNBIASED if unbiased else 0, C.byref(term))
    return term.value if ok else None


def ld_windows(chrom, pos, kb: float) -> np.ndarray:
    """win_end for ld_prune from a map: win_end[k] = one past the last u >= k with chrom[u] == chrom[k] and
    pos[u] - pos[k] <= 1000 kb.  Every chromosome must be one run of variants and pos must not decrease inside it
    (ValueError otherwise).  Host only."""
    chrom = np.asarray(chrom)
    pos = np.asarray(pos, dtype=np.int64)
    if chrom.ndim != 1 or chrom.shape != pos.shape:
        raise ValueError("ld_windows: chrom and pos must be one-dimensional and of one length")
    if not kb >= 0:
        raise ValueError("ld_windows: kb must be a number >= 0")
    n = len(pos)
    out = np.zeros(n, dtype=np.uint32)
    if n == 0:
        return out
    starts = np.concatenate([[0], np.flatnonzero(chrom[1:] != chrom[:-1]) + 1, [n]])
    names = [chrom[s].item() if hasattr(chrom[s], "item") else chrom[s] for s in starts[:-1]]
    if len(set(names)) != len(names):
        raise ValueError("ld_windows: the variants of a chromosome must be contiguous")
    span = int(1000 * kb)
    for s, e in zip(starts[:-1], starts[1:]):
        p = pos[s:e]
        if (np.diff(p) < 0).any():
            raise ValueError(f"ld_windows: positions decrease inside chromosome {chrom[s]}")
        out[s:e] = s + np.searchsorted(p, p + span, side="right")
    return out


def glm_model(phenotype, model: str = "auto"):
    """plink_glm's bind-time model rule (src/plink_glm.cpp:720-760): returns (model, phenotype) with model
    GLM_LINEAR or GLM_LOGISTIC.  'auto': all non-missing values 0/1 -> logistic; all 1/2 -> logistic, recoded to 0/1;
    anything else -> linear.  NaN (or None) marks a missing value and is kept."""
    y = np.array([np.nan if v is None else v for v in phenotype], dtype=np.float64)
    if model == "linear":
        return GLM_LINEAR, y
    if model == "logistic":
        return GLM_LOGISTIC, y
    if model != "auto":
        raise ValueError(f"plink_glm: model must be 'auto', 'linear', or 'logistic', got '{model}'")
    obs = y[~np.isnan(y)]
    if np.all((obs == 0.0) | (obs == 1.0)):
        return GLM_LOGISTIC, y
    if np.all((obs == 1.0) | (obs == 2.0)):
        return GLM_LOGISTIC, y - 1.0
    return GLM_LINEAR, y


def version() -> str:
    return _lib.pgh_version().decode()


def device_count() -> int:
    return _lib.pgh_device_count()


def set_device(dev: int):
    eb = _errbuf()
    _check(_lib.pgh_set_device(dev, eb), eb)


def probe(path: str, pgi_path: str | None = None) -> PghInfo:
    info = PghInfo()
    eb = _errbuf()
    _check(_lib.pgh_probe(path.encode(), pgi_path.encode() if pgi_path else None, C.byref(info), eb), eb)
    return info


def normalize_range_host(path: str, v_begin: int = 0, v_end: int | None = None, pgi_path: str | None = None):
    """Host normaliser only: plain 2-bit rows uint8[v_end-v_begin][ceil(N/4)]."""
    info = probe(path, pgi_path)
    v_end = info.raw_variant_ct if v_end is None else v_end
    rows = np.zeros((max(0, v_end - v_begin), info.record_bytes), dtype=np.uint8)
    eb = _errbuf()
    _check(_lib.pgh_normalize_range_host(path.encode(), pgi_path.encode() if pgi_path else None, v_begin, v_end,
                                         _ptr(rows), info.record_bytes, eb), eb)
    return rows


def hwe_lnp(hets: int, hom1: int, hom2: int, midp: bool = False) -> float:
    return _lib.pgh_hwe_lnp(hets, hom1, hom2, 1 if midp else 0)


def hwe_xchr_lnp_batch(strata, midp: bool = False) -> np.ndarray:
    """strata: int32[n][5] = {female_hets, female_hom1, female_hom2, male1, male2} -> ln p per variant (device)."""
    st = np.ascontiguousarray(strata, dtype=np.int32)
    assert st.ndim == 2 and st.shape[1] == 5
    out = np.zeros(len(st), dtype=np.float64)
    eb = _errbuf()
    _check(_lib.pgh_hwe_xchr_lnp_batch(_ptr(st), len(st), 1 if midp else 0, _ptr(out), eb), eb)
    return out


def hwe_xchr_lnp(fhets: int, fhom1: int, fhom2: int, male1: int, male2: int, midp: bool = False) -> float:
    return _lib.pgh_hwe_xchr_lnp(fhets, fhom1, fhom2, male1, male2, 1 if midp else 0)


def hwe_lnp_batch(counts: np.ndarray, midp: bool = False) -> np.ndarray:
    counts = np.ascontiguousarray(counts, dtype=np.uint32).reshape(-1, 4)
    out = np.empty(len(counts), dtype=np.float64)
    eb = _errbuf()
    _check(_lib.pgh_hwe_lnp_batch(_ptr(counts), len(counts), 1 if midp else 0, _ptr(out), eb), eb)
    return out


def freq_from_counts_dev(d_counts: int, n: int, d_alt_freq: int, d_obs_ct: int, stream: int = 0):
    eb = _errbuf()
    _check(_lib.pgh_freq_from_counts_dev(d_counts, n, d_alt_freq, d_obs_ct, stream, eb), eb)


def hwe_lnp_batch_dev(d_counts: int, n: int, d_ln_p: int, midp: bool = False, stream: int = 0):
    eb = _errbuf()
    _check(_lib.pgh_hwe_lnp_batch_dev(d_counts, n, 1 if midp else 0, d_ln_p, stream, eb), eb)


def ld_pairs_status():
    """pgh_ld_pairs_status: waits for the calling thread's last ld_pairs(_dev) launch; raises if it refused a task."""
    eb = _errbuf()
    _check(_lib.pgh_ld_pairs_status(eb), eb)


def probe_unpack_shape_dev(d_src: int, n_vec: int, d_dst: int, d_val: int, stream: int = 0):
    eb = _errbuf()
    _check(_lib.pgh_probe_unpack_shape_dev(d_src, n_vec, d_dst, d_val, stream, eb), eb)


def synth_record_host(v: int, n: int, seed: int, missing_rate: float) -> np.ndarray:
    out = np.zeros((n + 3) // 4, dtype=np.uint8)
    rc = _lib.pgh_synth_record_host(v, n, seed, missing_rate, _ptr(out))
    if rc != PGH_OK:
        raise PghArgError(rc, "pgh_synth_record_host: bad argument")
    return out


def synth_write_files(prefix: str, m: int, n: int, seed: int, missing_rate: float):
    eb = _errbuf()
    _check(_lib.pgh_synth_write_files(prefix.encode(), m, n, seed, missing_rate, eb), eb)


def synth_write_dosage_files(prefix: str, m: int, n: int, seed: int, missing_rate: float, dosage_rate: float):
    eb = _errbuf()
    _check(_lib.pgh_synth_write_dosage_files(prefix.encode(), m, n, seed, missing_rate, dosage_rate, eb), eb)


TALLY_COUNTS, TALLY_SAMPLE_MISSING, TALLY_HWE, TALLY_HWE_MIDP = 1, 2, 4, 8


def pca_streamed(path: str, vidx, center, inv_stdev, n_pcs: int, g1_init, window_variants: int, sample_include=None,
                 pgi_path: str | None = None):
    """pgh_pca over a .pgen that is not made resident: windows of at most `window_variants` variants, one at a time.
    sample_include: uint64 words of the subset's bit mask over the raw samples (None: everybody)."""
    vidx = np.ascontiguousarray(vidx, dtype=np.uint32)
    center = np.ascontiguousarray(center, dtype=np.float64)
    inv_stdev = np.ascontiguousarray(inv_stdev, dtype=np.float64)
    g1_init = np.ascontiguousarray(g1_init, dtype=np.float64)
    n_out = g1_init.shape[0]
    mask = None if sample_include is None else np.ascontiguousarray(sample_include, dtype=np.uint64)
    ev = np.zeros(n_pcs, dtype=np.float64)
    vec = np.zeros((n_out, n_pcs), dtype=np.float64)
    eb = _errbuf()
    rc = raw().pgh_pca_streamed(path.encode(), pgi_path.encode() if pgi_path else None, None if mask is None else _ptr(mask),
                                len(vidx), _ptr(vidx), _ptr(center), _ptr(inv_stdev), n_pcs, _ptr(g1_init),
                                int(window_variants), _ptr(ev), _ptr(vec), eb)
    _check(rc, eb)
    return ev, vec


def trim_device_cache():
    """Hand the call-scoped work blocks the library keeps between calls back to the driver."""
    raw().pgh_trim_device_cache()


def tally_passes_started() -> int:
    return int(_lib.pgh_tally_passes_started())


def sparse_opens_started() -> int:
    """pgh_open_sparse calls made by this process so far."""
    return int(_lib.pgh_sparse_opens_started())


class TallyPass:
    """pgh_tally: one asynchronous walk of [v_begin, v_end) whose products land in pinned host memory."""

    def __init__(self, ds: "Dataset", v_begin: int = 0, v_end: int | None = None, products: int = TALLY_COUNTS,
                 subset: "Subset | None" = None):
        self.ds, self.subset = ds, subset
        self.v_begin = v_begin
        self.v_end = ds.info.variant_end if v_end is None else v_end
        self.n_out = subset.size if subset is not None else ds.info.raw_sample_ct
        self._h = C.c_void_p()
        eb = _errbuf()
        _check(_lib.pgh_tally_start(ds._h, subset._h if subset is not None else None, self.v_begin, self.v_end,
                                    products, C.byref(self._h), eb), eb)

    def request(self, products: int):
        eb = _errbuf()
        _check(_lib.pgh_tally_request(self._h, products, eb), eb)

    def wait(self, products: int = TALLY_COUNTS, v_begin: int | None = None, v_end: int | None = None):
        eb = _errbuf()
        _check(_lib.pgh_tally_wait(self._h, products, self.v_begin if v_begin is None else v_begin,
                                   self.v_end if v_end is None else v_end, eb), eb)

    def _view(self, addr, dtype, shape):
        n = int(np.prod(shape))
        if n == 0:
            return np.zeros(shape, dtype=dtype)
        buf = (C.c_char * (n * np.dtype(dtype).itemsize)).from_address(addr)
        return np.frombuffer(buf, dtype=dtype).reshape(shape)

    def counts(self) -> np.ndarray:
        """uint32[v_end - v_begin][4], a copy of the pass's pinned array (everything waited for)."""
        self.wait(TALLY_COUNTS)
        return self._view(_lib.pgh_tally_counts(self._h), np.uint32, (self.v_end - self.v_begin, 4)).copy()

    def hwe_lnp(self, midp: bool = False) -> np.ndarray:
        bit = TALLY_HWE_MIDP if midp else TALLY_HWE
        self.request(bit)
        self.wait(bit)
        return self._view(_lib.pgh_tally_hwe_lnp(self._h, 1 if midp else 0), np.float64,
                          (self.v_end - self.v_begin,)).copy()

    def sample_missing(self) -> np.ndarray:
        out = np.zeros(self.n_out, dtype=np.uint32)
        eb = _errbuf()
        _check(_lib.pgh_tally_sample_missing(self._h, _ptr(out), eb), eb)
        return out

    def close(self):
        if self._h:
            _lib.pgh_tally_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        self.close()


class Subset:
    def __init__(self, ds: "Dataset", include_mask: np.ndarray):
        """include_mask: bool[N]."""
        include_mask = np.asarray(include_mask, dtype=bool)
        n = ds.info.raw_sample_ct
        assert include_mask.shape == (n,)
        words = np.zeros((n + 63) // 64, dtype=np.uint64)
        bits = np.packbits(include_mask, bitorder="little")
        words.view(np.uint8)[: len(bits)] = bits
        self._h = C.c_void_p()
        self.ds = ds
        eb = _errbuf()
        _check(_lib.pgh_subset_create(ds._h, _ptr(words), C.byref(self._h), eb), eb)
        self.size = _lib.pgh_subset_size(self._h)

    def close(self):
        if self._h:
            _lib.pgh_subset_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        self.close()


class Dataset:
    """A genotype matrix resident in HBM (pgh_dataset)."""

    def __init__(self, handle):
        self._h = handle
        self.info = PghInfo()
        _lib.pgh_get_info(self._h, C.byref(self.info))

    @classmethod
    def open(cls, path: str, pgi_path: str | None = None, variant_begin: int = 0, variant_end: int | None = None,
             sparse: bool = False, max_minor: int = 0):
        """sparse=True: the sparse-resident form (pgh_open_sparse; hardcall counts only).  max_minor > 0 makes a
        variant sparse iff at most that many samples differ from its majority call (0: whichever form is smaller)."""
        h = C.c_void_p()
        eb = _errbuf()
        pgi = pgi_path.encode() if pgi_path else None
        v_end = 0xFFFFFFFF if variant_end is None else variant_end
        if sparse:
            _check(_lib.pgh_open_sparse(path.encode(), pgi, variant_begin, v_end, max_minor, C.byref(h), eb), eb)
        else:
            _check(_lib.pgh_open(path.encode(), pgi, variant_begin, v_end, C.byref(h), eb), eb)
        return cls(h)

    def sparse_info(self) -> PghSparseInfo:
        """pgh_get_sparse_info (ValueError for a dataset that is not sparse-resident)."""
        out = PghSparseInfo()
        rc = _lib.pgh_get_sparse_info(self._h, C.byref(out))
        if rc != PGH_OK:
            raise PghArgError(rc, "not a sparse-resident dataset (Dataset.open(..., sparse=True))")
        return out

    @classmethod
    def open_sharded(cls, path: str, devices, pgi_path: str | None = None, variant_begin: int = 0,
                     variant_end: int | None = None):
        """One handle over len(devices) contiguous variant ranges of the file, shard k resident on devices[k]."""
        h, eb = C.c_void_p(), _errbuf()
        dev = np.ascontiguousarray(devices, dtype=np.int32)
        _check(_lib.pgh_open_sharded(path.encode(), pgi_path.encode() if pgi_path else None, variant_begin,
                                     0xFFFFFFFF if variant_end is None else variant_end, _ptr(dev), len(dev),
                                     C.byref(h), eb), eb)
        return cls(h)

    @classmethod
    def group(cls, shards):
        """A shard group over datasets that hold contiguous, ascending variant ranges; takes them over."""
        h, eb = C.c_void_p(), _errbuf()
        arr = (C.c_void_p * len(shards))(*[s._h for s in shards])
        _check(_lib.pgh_group_create(arr, len(shards), C.byref(h), eb), eb)
        for s in shards:
            s._h = None  # owned by the group now
        return cls(h)

    @property
    def uses_rccl(self) -> bool:
        """The group's per-sample merges are RCCL collectives (shards on distinct devices)."""
        return bool(_lib.pgh_group_uses_rccl(self._h))

    @property
    def shard_count(self) -> int:
        return int(_lib.pgh_shard_count(self._h))

    @classmethod
    def from_host_rows(cls, rows: np.ndarray, n_samples: int):
        rows = np.ascontiguousarray(rows, dtype=np.uint8)
        assert rows.ndim == 2
        h = C.c_void_p()
        eb = _errbuf()
        _check(_lib.pgh_from_host_rows(_ptr(rows), rows.shape[1], rows.shape[0], n_samples, C.byref(h), eb), eb)
        return cls(h)

    @classmethod
    def synth(cls, variant_begin: int, variant_end: int, n_samples: int, seed: int, missing_rate: float):
        h = C.c_void_p()
        eb = _errbuf()
        _check(_lib.pgh_synth_create(variant_begin, variant_end, n_samples, seed, missing_rate, C.byref(h), eb), eb)
        return cls(h)

    # -- properties -------------------------------------------------------
    @property
    def n_samples(self):
        return self.info.raw_sample_ct

    @property
    def v_begin(self):
        return self.info.variant_begin

    @property
    def v_end(self):
        return self.info.variant_end

    @property
    def device_rows(self) -> int:
        return _lib.pgh_device_rows(self._h)

    def copy_rows_to_host(self, v_begin: int, v_end: int) -> np.ndarray:
        rows = np.zeros((max(0, v_end - v_begin), self.info.record_bytes), dtype=np.uint8)
        eb = _errbuf()
        _check(_lib.pgh_copy_rows_to_host(self._h, v_begin, v_end, _ptr(rows), self.info.record_bytes, eb), eb)
        return rows

    def subset(self, include_mask) -> Subset:
        return Subset(self, include_mask)

    def close(self):
        if self._h:
            _lib.pgh_close(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        self.close()

    # -- batched calls ------------------------------------------------------
    def counts_range(self, v_begin=None, v_end=None, subset: Subset | None = None) -> np.ndarray:
        v_begin = self.v_begin if v_begin is None else v_begin
        v_end = self.v_end if v_end is None else v_end
        out = np.zeros((max(0, v_end - v_begin), 4), dtype=np.uint32)
        eb = _errbuf()
        _check(_lib.pgh_counts_range(self._h, subset._h if subset else None, v_begin, v_end, _ptr(out), eb), eb)
        return out

    def counts_range_dev(self, v_begin, v_end, d_out: int, stream: int = 0, subset: Subset | None = None):
        eb = _errbuf()
        _check(_lib.pgh_counts_range_dev(self._h, subset._h if subset else None, v_begin, v_end, d_out, stream, eb), eb)

    def missing_per_sample(self, v_begin=None, v_end=None, subset: Subset | None = None) -> np.ndarray:
        v_begin = self.v_begin if v_begin is None else v_begin
        v_end = self.v_end if v_end is None else v_end
        n_out = subset.size if subset else self.n_samples
        out = np.zeros(n_out, dtype=np.uint32)
        eb = _errbuf()
        _check(_lib.pgh_missing_per_sample(self._h, subset._h if subset else None, v_begin, v_end, _ptr(out), eb), eb)
        return out

    def fused_tally_dev(self, v_begin, v_end, d_counts: int, d_missing: int, stream: int = 0):
        eb = _errbuf()
        _check(_lib.pgh_fused_tally_dev(self._h, v_begin, v_end, d_counts, d_missing, stream, eb), eb)

    def missing_per_sample_dev(self, v_begin, v_end, d_out: int, stream: int = 0):
        eb = _errbuf()
        _check(_lib.pgh_missing_per_sample_dev(self._h, v_begin, v_end, d_out, stream, eb), eb)

    def unpack_range(self, v_begin=None, v_end=None, subset: Subset | None = None, missing_code: int = -9,
                     want_validity: bool = True):
        v_begin = self.v_begin if v_begin is None else v_begin
        v_end = self.v_end if v_end is None else v_end
        n_out = subset.size if subset else self.n_samples
        rows = max(0, v_end - v_begin)
        out = np.zeros((rows, n_out), dtype=np.int8)
        val = np.zeros((rows, (n_out + 63) // 64), dtype=np.uint64) if want_validity else None
        eb = _errbuf()
        _check(_lib.pgh_unpack_range(self._h, subset._h if subset else None, v_begin, v_end, _ptr(out), _ptr(val),
                                     missing_code, eb), eb)
        return out, val

    def unpack_range_dev(self, v_begin, v_end, d_out: int, out_pitch: int, d_validity: int, missing_code: int = 0,
                         stream: int = 0, subset: Subset | None = None):
        eb = _errbuf()
        _check(_lib.pgh_unpack_range_dev(self._h, subset._h if subset else None, v_begin, v_end, d_out, out_pitch,
                                         d_validity, missing_code, stream, eb), eb)

    def score(self, vidx, weights, flip=None, mode: int = SCORE_MEAN_IMPUTE, subset: Subset | None = None,
              want_dosage_sum: bool = True, counts=None):
        """counts (optional): uint32[n_scored][4], the scored variants' class tallies (pgh_score_counts)."""
        vidx = np.ascontiguousarray(vidx, dtype=np.uint32)
        weights = np.ascontiguousarray(weights, dtype=np.float64)
        if weights.ndim == 1:
            weights = weights.reshape(-1, 1)
        n_scored, n_cols = weights.shape
        assert len(vidx) == n_scored
        flip_a = None if flip is None else np.ascontiguousarray(flip, dtype=np.uint8)
        n_out = subset.size if subset else self.n_samples
        score = np.zeros((n_out, n_cols), dtype=np.float64)
        dos = np.zeros(n_out, dtype=np.float64) if want_dosage_sum else None
        ac = np.zeros(n_out, dtype=np.uint32)
        eb = _errbuf()
        if counts is not None:
            counts = np.ascontiguousarray(counts, dtype=np.uint32).reshape(n_scored, 4)
            _check(_lib.pgh_score_counts(self._h, subset._h if subset else None, n_scored, _ptr(vidx), _ptr(weights),
                                         _ptr(flip_a), n_cols, mode, _ptr(counts), _ptr(score), _ptr(dos), _ptr(ac), eb), eb)
            return score, dos, ac
        _check(_lib.pgh_score(self._h, subset._h if subset else None, n_scored, _ptr(vidx), _ptr(weights), _ptr(flip_a),
                              n_cols, mode, _ptr(score), _ptr(dos), _ptr(ac), eb), eb)
        return score, dos, ac

    def score_dev(self, vidx, weights, d_score: int, d_dosage: int, d_allele: int, flip=None,
                  mode: int = SCORE_MEAN_IMPUTE, stream: int = 0, subset: Subset | None = None):
        vidx = np.ascontiguousarray(vidx, dtype=np.uint32)
        weights = np.ascontiguousarray(weights, dtype=np.float64)
        if weights.ndim == 1:
            weights = weights.reshape(-1, 1)
        flip_a = None if flip is None else np.ascontiguousarray(flip, dtype=np.uint8)
        eb = _errbuf()
        _check(_lib.pgh_score_dev(self._h, subset._h if subset else None, weights.shape[0], _ptr(vidx), _ptr(weights),
                                  _ptr(flip_a), weights.shape[1], mode, d_score, d_dosage, d_allele, stream, eb), eb)

    def score_plan(self, vidx, weights, flip=None, mode: int = SCORE_MEAN_IMPUTE, subset: Subset | None = None):
        return ScorePlan(self, vidx, weights, flip, mode, subset)

    def pca(self, vidx, center, inv_stdev, n_pcs: int, g1_init, subset: Subset | None = None):
        vidx = np.ascontiguousarray(vidx, dtype=np.uint32)
        center = np.ascontiguousarray(center, dtype=np.float64)
        inv_stdev = np.ascontiguousarray(inv_stdev, dtype=np.float64)
        g1 = np.ascontiguousarray(g1_init, dtype=np.float64)
        n_out = subset.size if subset else self.n_samples
        assert g1.shape == (n_out, 2 * n_pcs)
        ev = np.zeros(n_pcs, dtype=np.float64)
        vecs = np.zeros((n_out, n_pcs), dtype=np.float64)
        eb = _errbuf()
        _check(_lib.pgh_pca(self._h, subset._h if subset else None, len(vidx), _ptr(vidx), _ptr(center),
                            _ptr(inv_stdev), n_pcs, _ptr(g1), _ptr(ev), _ptr(vecs), eb), eb)
        return ev, vecs

    def sample_counts(self, v_begin: int | None = None, v_end: int | None = None, vidx=None,
                      subset: Subset | None = None) -> np.ndarray:
        """uint32[n_out][4] = {hom_ref, het, hom_alt, missing} per sample over a variant range or list."""
        n_out = subset.size if subset else self.n_samples
        out = np.zeros((n_out, 4), dtype=np.uint32)
        eb = _errbuf()
        if vidx is not None:
            v = np.ascontiguousarray(vidx, dtype=np.uint32)
            _check(_lib.pgh_sample_counts(self._h, subset._h if subset else None, 0, len(v), _ptr(v), _ptr(out), eb), eb)
        else:
            v0 = self.v_begin if v_begin is None else v_begin
            v1 = self.v_end if v_end is None else v_end
            _check(_lib.pgh_sample_counts(self._h, subset._h if subset else None, v0, v1 - v0, None, _ptr(out), eb), eb)
        return out

    def synth_add_dosage(self, rate: float, seed: int):
        """Seeded synthetic dosage tracks on every resident variant (benchmark input)."""
        eb = _errbuf()
        _check(_lib.pgh_synth_add_dosage(self._h, rate, seed, eb), eb)
        _lib.pgh_get_info(self._h, C.byref(self.info))

    def _range_or_list(self, v_begin, v_end, vidx):
        if vidx is not None:
            v = np.ascontiguousarray(vidx, dtype=np.uint32)
            return 0, len(v), v
        v0 = self.v_begin if v_begin is None else v_begin
        v1 = self.v_end if v_end is None else v_end
        return v0, v1 - v0, None

    def dosage_sums(self, v_begin: int | None = None, v_end: int | None = None, vidx=None,
                    subset: Subset | None = None) -> np.ndarray:
        """uint64[n][3] = {sum, sum of squares, observed samples} of the dosages (16384 per ALT copy)."""
        v0, n, v = self._range_or_list(v_begin, v_end, vidx)
        out = np.zeros((n, 3), dtype=np.uint64)
        eb = _errbuf()
        _check(_lib.pgh_dosage_sums(self._h, subset._h if subset else None, v0, n, _ptr(v) if v is not None else None,
                                    _ptr(out), eb), eb)
        return out

    def dosage_unpack(self, v_begin: int | None = None, v_end: int | None = None, vidx=None,
                      subset: Subset | None = None) -> np.ndarray:
        """float64[n][n_out]: dosages, -9 where a sample has neither a dosage nor a call."""
        v0, n, v = self._range_or_list(v_begin, v_end, vidx)
        out = np.zeros((n, subset.size if subset else self.n_samples), dtype=np.float64)
        eb = _errbuf()
        _check(_lib.pgh_dosage_unpack(self._h, subset._h if subset else None, v0, n, _ptr(v) if v is not None else None,
                                      _ptr(out), eb), eb)
        return out

    def glm(self, phenotype, covariates=None, model="linear", firth: bool = True, v_begin: int | None = None,
            v_end: int | None = None, subset: Subset | None = None) -> dict:
        """pgh_glm over [v_begin, v_end): per-variant regression of phenotype (one value per output sample, NaN =
        missing) on the ALT dosage plus covariates (n_covar x n_out, or None).  model: "linear" / "logistic" (or
        GLM_LINEAR / GLM_LOGISTIC; apply glm_model() first for the reference's 'auto').  Returns numpy arrays beta, se,
        stat, p, a1_freq (NaN where the reference emits NULL), obs_ct, errcode (strings or None) and firth (bool)."""
        v0 = self.v_begin if v_begin is None else v_begin
        v1 = self.v_end if v_end is None else v_end
        n_out = subset.size if subset else self.n_samples
        y = np.ascontiguousarray(phenotype, dtype=np.float64)
        if y.shape != (n_out,):
            raise ValueError(f"phenotype must hold one value per output sample ({n_out}), got shape {y.shape}")
        if covariates is None:
            z = np.zeros((0, n_out), dtype=np.float64)
        else:
            z = np.ascontiguousarray(np.atleast_2d(np.asarray(covariates, dtype=np.float64)))
            if z.shape[1] != n_out:
                raise ValueError(f"covariates must be n_covar x {n_out}, got shape {z.shape}")
        m = {"linear": GLM_LINEAR, "logistic": GLM_LOGISTIC}.get(model, model)
        rows = np.zeros(max(0, v1 - v0), dtype=GLM_ROW_DTYPE)
        eb = _errbuf()
        _check(_lib.pgh_glm(self._h, subset._h if subset else None, v0, v1, _ptr(y), z.shape[0],
                            _ptr(z) if z.size else None, int(m), int(bool(firth)), _ptr(rows), eb), eb)
        return {
            "beta": rows["beta"].copy(), "se": rows["se"].copy(), "stat": rows["stat"].copy(), "p": rows["p"].copy(),
            "a1_freq": rows["a1_freq"].copy(), "obs_ct": rows["obs_ct"].astype(np.int64),
            "errcode": np.array([GLM_ERRCODES[c] for c in rows["errcode"]], dtype=object),
            "firth": rows["firth"].astype(bool),
        }

    def glm_multi(self, phenotypes, covariates=None, model="linear", firth: bool = True, v_begin: int | None = None,
                  v_end: int | None = None, subset: Subset | None = None) -> dict:
        """pgh_glm_multi: glm() for every row of phenotypes (P x n_out, NaN = missing) in one call.  Returns glm()'s
        keys, each a (V, P) array: [v, p] is phenotype p's row for variant v_begin + v.  glm_model() stays per
        phenotype and is the caller's."""
        v0 = self.v_begin if v_begin is None else v_begin
        v1 = self.v_end if v_end is None else v_end
        n_out = subset.size if subset else self.n_samples
        y = np.ascontiguousarray(phenotypes, dtype=np.float64)
        if y.ndim != 2 or y.shape[0] == 0 or y.shape[1] != n_out:
            raise ValueError(f"phenotypes must be n_pheno x {n_out} with n_pheno >= 1, got shape {y.shape}")
        if covariates is None:
            z = np.zeros((0, n_out), dtype=np.float64)
        else:
            z = np.ascontiguousarray(np.atleast_2d(np.asarray(covariates, dtype=np.float64)))
            if z.shape[1] != n_out:
                raise ValueError(f"covariates must be n_covar x {n_out}, got shape {z.shape}")
        m = {"linear": GLM_LINEAR, "logistic": GLM_LOGISTIC}.get(model, model)
        rows = np.zeros((max(0, v1 - v0), y.shape[0]), dtype=GLM_ROW_DTYPE)
        eb = _errbuf()
        _check(_lib.pgh_glm_multi(self._h, subset._h if subset else None, v0, v1, y.shape[0], _ptr(y), z.shape[0],
                                  _ptr(z) if z.size else None, int(m), int(bool(firth)), _ptr(rows), eb), eb)
        return {
            "beta": rows["beta"].copy(), "se": rows["se"].copy(), "stat": rows["stat"].copy(), "p": rows["p"].copy(),
            "a1_freq": rows["a1_freq"].copy(), "obs_ct": rows["obs_ct"].astype(np.int64),
            "errcode": np.array(GLM_ERRCODES, dtype=object)[rows["errcode"]],
            "firth": rows["firth"].astype(bool),
        }

    def glm_sparse(self, phenotype, covariates=None, v_begin: int | None = None, v_end: int | None = None,
                   subset: Subset | None = None) -> dict:
        """pgh_glm_sparse: glm()'s linear fit over a sparse-resident dataset (Dataset.open(..., sparse=True)), from each
        variant's entries.  Returns glm()'s dict (firth is False everywhere)."""
        v0 = self.v_begin if v_begin is None else v_begin
        v1 = self.v_end if v_end is None else v_end
        n_out = subset.size if subset else self.n_samples
        y = np.ascontiguousarray(phenotype, dtype=np.float64)
        if y.shape != (n_out,):
            raise ValueError(f"phenotype must hold one value per output sample ({n_out}), got shape {y.shape}")
        if covariates is None:
            z = np.zeros((0, n_out), dtype=np.float64)
        else:
            z = np.ascontiguousarray(np.atleast_2d(np.asarray(covariates, dtype=np.float64)))
            if z.shape[1] != n_out:
                raise ValueError(f"covariates must be n_covar x {n_out}, got shape {z.shape}")
        rows = np.zeros(max(0, v1 - v0), dtype=GLM_ROW_DTYPE)
        eb = _errbuf()
        _check(_lib.pgh_glm_sparse(self._h, subset._h if subset else None, v0, v1, _ptr(y), z.shape[0],
                                   _ptr(z) if z.size else None, _ptr(rows), eb), eb)
        return {
            "beta": rows["beta"].copy(), "se": rows["se"].copy(), "stat": rows["stat"].copy(), "p": rows["p"].copy(),
            "a1_freq": rows["a1_freq"].copy(), "obs_ct": rows["obs_ct"].astype(np.int64),
            "errcode": np.array([GLM_ERRCODES[c] for c in rows["errcode"]], dtype=object),
            "firth": rows["firth"].astype(bool),
        }

    def glm_sparse_multi(self, phenotypes, covariates=None, v_begin: int | None = None, v_end: int | None = None,
                         subset: Subset | None = None) -> dict:
        """pgh_glm_sparse_multi: glm_sparse() for every row of phenotypes (P x n_out, NaN = missing, each row with its
        own missing-value pattern) in one walk of the variants' entries per block of 64 phenotypes.  Returns
        glm_multi()'s dict of (V, P) arrays: [v, p] is glm_sparse()'s row of phenotype p alone for variant v_begin + v,
        to rounding."""
        v0, v1, y, z = Dataset._score_multi_args(self, phenotypes, covariates, v_begin, v_end, subset)
        rows = np.zeros((max(0, v1 - v0), y.shape[0]), dtype=GLM_ROW_DTYPE)
        eb = _errbuf()
        _check(_lib.pgh_glm_sparse_multi(self._h, subset._h if subset else None, v0, v1, y.shape[0], _ptr(y), z.shape[0],
                                         _ptr(z) if z.size else None, _ptr(rows), eb), eb)
        return Dataset._glm_multi_rows_dict(rows)

    def _score_sparse_args(self, phenotype, covariates, v_begin, v_end, subset):
        """(v0, v1, y, z) of the score-test calls, after their shape checks."""
        v0 = self.v_begin if v_begin is None else v_begin
        v1 = self.v_end if v_end is None else v_end
        n_out = subset.size if subset else self.n_samples
        y = np.ascontiguousarray(phenotype, dtype=np.float64)
        if y.shape != (n_out,):
            raise ValueError(f"phenotype must hold one value per output sample ({n_out}), got shape {y.shape}")
        if covariates is None:
            z = np.zeros((0, n_out), dtype=np.float64)
        else:
            z = np.ascontiguousarray(np.atleast_2d(np.asarray(covariates, dtype=np.float64)))
            if z.shape[1] != n_out:
                raise ValueError(f"covariates must be n_covar x {n_out}, got shape {z.shape}")
        return v0, v1, y, z

    @staticmethod
    def _glm_rows_dict(rows) -> dict:
        return {
            "beta": rows["beta"].copy(), "se": rows["se"].copy(), "stat": rows["stat"].copy(), "p": rows["p"].copy(),
            "a1_freq": rows["a1_freq"].copy(), "obs_ct": rows["obs_ct"].astype(np.int64),
            "errcode": np.array([GLM_ERRCODES[c] for c in rows["errcode"]], dtype=object),
            "firth": rows["firth"].astype(bool),
        }

    def glm_score_sparse(self, phenotype, covariates=None, v_begin: int | None = None, v_end: int | None = None,
                         subset: Subset | None = None) -> dict:
        """pgh_glm_score_sparse: the logistic score test of every variant of a sparse-resident dataset
        (Dataset.open(..., sparse=True)), from each variant's entries.  phenotype: 0.0 / 1.0 per output sample, NaN =
        missing (apply glm_model() first for 1/2 coding).  Returns glm()'s dict (firth is False everywhere)."""
        v0, v1, y, z = Dataset._score_sparse_args(self, phenotype, covariates, v_begin, v_end, subset)
        rows = np.zeros(max(0, v1 - v0), dtype=GLM_ROW_DTYPE)
        eb = _errbuf()
        _check(_lib.pgh_glm_score_sparse(self._h, subset._h if subset else None, v0, v1, _ptr(y), z.shape[0],
                                         _ptr(z) if z.size else None, _ptr(rows), eb), eb)
        return Dataset._glm_rows_dict(rows)

    def glm_score_multi(self, phenotypes, covariates=None, v_begin: int | None = None, v_end: int | None = None,
                        subset: Subset | None = None) -> dict:
        """pgh_glm_score_multi: the logistic score test of every variant of a dense-resident dataset for every row of
        phenotypes (P x n_out; 0.0 / 1.0, NaN = missing) in one call, on the FP64 matrix cores.  Returns glm_multi()'s
        dict of (V, P) arrays: [v, p] is glm_score_sparse()'s row of phenotype p alone for variant v_begin + v."""
        v0, v1, y, z = Dataset._score_multi_args(self, phenotypes, covariates, v_begin, v_end, subset)
        rows = np.zeros((max(0, v1 - v0), y.shape[0]), dtype=GLM_ROW_DTYPE)
        eb = _errbuf()
        _check(_lib.pgh_glm_score_multi(self._h, subset._h if subset else None, v0, v1, y.shape[0], _ptr(y), z.shape[0],
                                        _ptr(z) if z.size else None, _ptr(rows), eb), eb)
        return Dataset._glm_multi_rows_dict(rows)

    def glm_score_multi_dosage(self, phenotypes, covariates=None, v_begin: int | None = None, v_end: int | None = None,
                               subset: Subset | None = None) -> dict:
        """pgh_glm_score_multi_dosage: glm_score_multi() over a dataset that may hold dosage tracks, with a variant's
        genotype value the explicit dosage / 16384 where a sample has one and its call otherwise (glm()'s rule).
        Returns glm_score_multi()'s dict of (V, P) arrays."""
        v0, v1, y, z = Dataset._score_multi_args(self, phenotypes, covariates, v_begin, v_end, subset)
        rows = np.zeros((max(0, v1 - v0), y.shape[0]), dtype=GLM_ROW_DTYPE)
        eb = _errbuf()
        _check(_lib.pgh_glm_score_multi_dosage(self._h, subset._h if subset else None, v0, v1, y.shape[0], _ptr(y),
                                               z.shape[0], _ptr(z) if z.size else None, _ptr(rows), eb), eb)
        return Dataset._glm_multi_rows_dict(rows)

    def glm_score_sparse_multi(self, phenotypes, covariates=None, v_begin: int | None = None, v_end: int | None = None,
                               subset: Subset | None = None) -> dict:
        """pgh_glm_score_sparse_multi: the logistic score test of every variant of a sparse-resident dataset
        (Dataset.open(..., sparse=True)) for every row of phenotypes (P x n_out; 0.0 / 1.0, NaN = missing) in one walk
        of the variants' entries per block of 64 phenotypes.  Returns glm_score_multi()'s dict of (V, P) arrays: [v, p]
        is glm_score_sparse()'s row of phenotype p alone for variant v_begin + v, to rounding."""
        v0, v1, y, z = Dataset._score_multi_args(self, phenotypes, covariates, v_begin, v_end, subset)
        rows = np.zeros((max(0, v1 - v0), y.shape[0]), dtype=GLM_ROW_DTYPE)
        eb = _errbuf()
        _check(_lib.pgh_glm_score_sparse_multi(self._h, subset._h if subset else None, v0, v1, y.shape[0], _ptr(y),
                                               z.shape[0], _ptr(z) if z.size else None, _ptr(rows), eb), eb)
        return Dataset._glm_multi_rows_dict(rows)

    def _score_multi_args(self, phenotypes, covariates, v_begin, v_end, subset):
        """(v0, v1, y, z) of the many-phenotype score-test calls, after their shape checks."""
        v0 = self.v_begin if v_begin is None else v_begin
        v1 = self.v_end if v_end is None else v_end
        n_out = subset.size if subset else self.n_samples
        y = np.ascontiguousarray(phenotypes, dtype=np.float64)
        if y.ndim != 2 or y.shape[0] == 0 or y.shape[1] != n_out:
            raise ValueError(f"phenotypes must be n_pheno x {n_out} with n_pheno >= 1, got shape {y.shape}")
        if covariates is None:
            z = np.zeros((0, n_out), dtype=np.float64)
        else:
            z = np.ascontiguousarray(np.atleast_2d(np.asarray(covariates, dtype=np.float64)))
            if z.shape[1] != n_out:
                raise ValueError(f"covariates must be n_covar x {n_out}, got shape {z.shape}")
        return v0, v1, y, z

    @staticmethod
    def _glm_multi_rows_dict(rows) -> dict:
        return {
            "beta": rows["beta"].copy(), "se": rows["se"].copy(), "stat": rows["stat"].copy(), "p": rows["p"].copy(),
            "a1_freq": rows["a1_freq"].copy(), "obs_ct": rows["obs_ct"].astype(np.int64),
            "errcode": np.array(GLM_ERRCODES, dtype=object)[rows["errcode"]],
            "firth": rows["firth"].astype(bool),
        }

    def glm_score_multi_spa(self, phenotypes, covariates=None, spa_cutoff: float = 2.0, subset: Subset | None = None,
                            v_begin: int | None = None, v_end: int | None = None) -> dict:
        """pgh_glm_score_multi_spa: glm_score_multi() plus a saddlepoint p-value for the rows with |stat| > spa_cutoff
        (spa_cutoff >= 0.1; inf = never).  Returns glm_score_multi()'s dict (p stays the normal p-value) and, both of
        shape (V, P), p_spa (float64: NaN for a row that is not fitted, p where the saddlepoint was not applied or
        failed) and spa_state (uint8: 0 = not applied, 1 = applied, 2 = attempted and failed)."""
        v0, v1, y, z = Dataset._score_multi_args(self, phenotypes, covariates, v_begin, v_end, subset)
        shape = (max(0, v1 - v0), y.shape[0])
        rows = np.zeros(shape, dtype=GLM_ROW_DTYPE)
        p_spa = np.zeros(shape, dtype=np.float64)
        state = np.zeros(shape, dtype=np.uint8)
        eb = _errbuf()
        _check(_lib.pgh_glm_score_multi_spa(self._h, subset._h if subset else None, v0, v1, y.shape[0], _ptr(y),
                                            z.shape[0], _ptr(z) if z.size else None, float(spa_cutoff), _ptr(rows),
                                            _ptr(p_spa), _ptr(state), eb), eb)
        return dict(Dataset._glm_multi_rows_dict(rows), p_spa=p_spa, spa_state=state)

    def glm_score_multi_dosage_spa(self, phenotypes, covariates=None, spa_cutoff: float = 2.0,
                                   subset: Subset | None = None, v_begin: int | None = None,
                                   v_end: int | None = None) -> dict:
        """pgh_glm_score_multi_dosage_spa: glm_score_multi_spa() over a dataset that may hold dosage tracks, with
        glm_score_multi_dosage()'s genotype values.  Returns glm_score_multi_spa()'s dict: the rows are
        glm_score_multi_dosage()'s, and p_spa and spa_state are of shape (V, P)."""
        v0, v1, y, z = Dataset._score_multi_args(self, phenotypes, covariates, v_begin, v_end, subset)
        shape = (max(0, v1 - v0), y.shape[0])
        rows = np.zeros(shape, dtype=GLM_ROW_DTYPE)
        p_spa = np.zeros(shape, dtype=np.float64)
        state = np.zeros(shape, dtype=np.uint8)
        eb = _errbuf()
        _check(_lib.pgh_glm_score_multi_dosage_spa(self._h, subset._h if subset else None, v0, v1, y.shape[0], _ptr(y),
                                                   z.shape[0], _ptr(z) if z.size else None, float(spa_cutoff),
                                                   _ptr(rows), _ptr(p_spa), _ptr(state), eb), eb)
        return dict(Dataset._glm_multi_rows_dict(rows), p_spa=p_spa, spa_state=state)

    def glm_score_sparse_multi_spa(self, phenotypes, covariates=None, spa_cutoff: float = 2.0,
                                   subset: Subset | None = None, v_begin: int | None = None,
                                   v_end: int | None = None) -> dict:
        """pgh_glm_score_sparse_multi_spa: glm_score_sparse_multi() plus a saddlepoint p-value for the rows with
        |stat| > spa_cutoff (spa_cutoff >= 0.1; inf = never).  Returns glm_score_sparse_multi()'s dict (p stays the
        normal p-value) and, both of shape (V, P), p_spa and spa_state as glm_score_multi_spa() returns them."""
        v0, v1, y, z = Dataset._score_multi_args(self, phenotypes, covariates, v_begin, v_end, subset)
        shape = (max(0, v1 - v0), y.shape[0])
        rows = np.zeros(shape, dtype=GLM_ROW_DTYPE)
        p_spa = np.zeros(shape, dtype=np.float64)
        state = np.zeros(shape, dtype=np.uint8)
        eb = _errbuf()
        _check(_lib.pgh_glm_score_sparse_multi_spa(self._h, subset._h if subset else None, v0, v1, y.shape[0], _ptr(y),
                                                   z.shape[0], _ptr(z) if z.size else None, float(spa_cutoff),
                                                   _ptr(rows), _ptr(p_spa), _ptr(state), eb), eb)
        return dict(Dataset._glm_multi_rows_dict(rows), p_spa=p_spa, spa_state=state)

    def glm_score_multi_firth(self, phenotypes, covariates=None, firth_cutoff: float = 2.0, v_begin: int | None = None,
                              v_end: int | None = None, subset: Subset | None = None) -> dict:
        """pgh_glm_score_multi_firth: glm_score_multi() plus the approximate Firth estimate (the covariate effects
        fixed at the null fit) for the rows with |stat| > firth_cutoff (firth_cutoff >= 0.1; inf = never).  Returns
        glm_score_multi()'s dict unchanged and, all of shape (V, P), beta_firth, se_firth, p_firth (float64: NaN for a
        row that is not fitted, the score row's beta, se, p where Firth was not applied or failed) and firth_state
        (uint8: 0 = not applied, 1 = applied, 2 = attempted and failed)."""
        v0, v1, y, z = Dataset._score_multi_args(self, phenotypes, covariates, v_begin, v_end, subset)
        if not firth_cutoff >= 0.1:
            raise ValueError(f"firth_cutoff must be at least 0.1, got {firth_cutoff}")
        shape = (max(0, v1 - v0), y.shape[0])
        rows = np.zeros(shape, dtype=GLM_ROW_DTYPE)
        firth = np.zeros(shape, dtype=GLM_FIRTH_ROW_DTYPE)
        eb = _errbuf()
        _check(_lib.pgh_glm_score_multi_firth(self._h, subset._h if subset else None, v0, v1, y.shape[0], _ptr(y),
                                              z.shape[0], _ptr(z) if z.size else None, float(firth_cutoff), _ptr(rows),
                                              _ptr(firth), eb), eb)
        return dict(Dataset._glm_multi_rows_dict(rows), beta_firth=firth["beta"].copy(), se_firth=firth["se"].copy(),
                    p_firth=firth["p"].copy(), firth_state=firth["state"].copy())

    def glm_score_multi_dosage_firth(self, phenotypes, covariates=None, firth_cutoff: float = 2.0,
                                     v_begin: int | None = None, v_end: int | None = None,
                                     subset: Subset | None = None) -> dict:
        """pgh_glm_score_multi_dosage_firth: glm_score_multi_firth() over a dataset that may hold dosage tracks, with
        glm_score_multi_dosage()'s genotype values.  Returns glm_score_multi_firth()'s dict: the rows are
        glm_score_multi_dosage()'s, and beta_firth, se_firth, p_firth and firth_state are of shape (V, P)."""
        v0, v1, y, z = Dataset._score_multi_args(self, phenotypes, covariates, v_begin, v_end, subset)
        if not firth_cutoff >= 0.1:
            raise ValueError(f"firth_cutoff must be at least 0.1, got {firth_cutoff}")
        shape = (max(0, v1 - v0), y.shape[0])
        rows = np.zeros(shape, dtype=GLM_ROW_DTYPE)
        firth = np.zeros(shape, dtype=GLM_FIRTH_ROW_DTYPE)
        eb = _errbuf()
        _check(_lib.pgh_glm_score_multi_dosage_firth(self._h, subset._h if subset else None, v0, v1, y.shape[0], _ptr(y),
                                                     z.shape[0], _ptr(z) if z.size else None, float(firth_cutoff),
                                                     _ptr(rows), _ptr(firth), eb), eb)
        return dict(Dataset._glm_multi_rows_dict(rows), beta_firth=firth["beta"].copy(), se_firth=firth["se"].copy(),
                    p_firth=firth["p"].copy(), firth_state=firth["state"].copy())

    def glm_score_sparse_multi_firth(self, phenotypes, covariates=None, firth_cutoff: float = 2.0,
                                     subset: Subset | None = None, v_begin: int | None = None,
                                     v_end: int | None = None) -> dict:
        """pgh_glm_score_sparse_multi_firth: glm_score_sparse_multi() plus the approximate Firth estimate (the
        covariate effects fixed at the null fit, the genotype coded against the row's base code) for the rows with
        |stat| > firth_cutoff (firth_cutoff >= 0.1; inf = never).  Returns glm_score_sparse_multi()'s dict unchanged
        and, all of shape (V, P), beta_firth, se_firth, p_firth and firth_state as glm_score_multi_firth() returns
        them."""
        v0, v1, y, z = Dataset._score_multi_args(self, phenotypes, covariates, v_begin, v_end, subset)
        if not firth_cutoff >= 0.1:
            raise ValueError(f"firth_cutoff must be at least 0.1, got {firth_cutoff}")
        shape = (max(0, v1 - v0), y.shape[0])
        rows = np.zeros(shape, dtype=GLM_ROW_DTYPE)
        firth = np.zeros(shape, dtype=GLM_FIRTH_ROW_DTYPE)
        eb = _errbuf()
        _check(_lib.pgh_glm_score_sparse_multi_firth(self._h, subset._h if subset else None, v0, v1, y.shape[0],
                                                     _ptr(y), z.shape[0], _ptr(z) if z.size else None,
                                                     float(firth_cutoff), _ptr(rows), _ptr(firth), eb), eb)
        return dict(Dataset._glm_multi_rows_dict(rows), beta_firth=firth["beta"].copy(), se_firth=firth["se"].copy(),
                    p_firth=firth["p"].copy(), firth_state=firth["state"].copy())

    def glm_score_sparse_spa(self, phenotype, covariates=None, cutoff: float = 2.0, v_begin: int | None = None,
                             v_end: int | None = None, subset: Subset | None = None) -> dict:
        """pgh_glm_score_sparse_spa: glm_score_sparse() plus a saddlepoint p-value for the rows with |stat| > cutoff
        (cutoff >= 0.1; inf = never).  Returns glm_score_sparse()'s dict (p stays the normal p-value) and p_spa
        (float64: NaN for a row that is not fitted, p where the saddlepoint was not applied or failed) and spa_state
        (uint8: 0 = not applied, 1 = applied, 2 = attempted and failed)."""
        v0, v1, y, z = Dataset._score_sparse_args(self, phenotype, covariates, v_begin, v_end, subset)
        nv = max(0, v1 - v0)
        rows = np.zeros(nv, dtype=GLM_ROW_DTYPE)
        p_spa = np.zeros(nv, dtype=np.float64)
        state = np.zeros(nv, dtype=np.uint8)
        eb = _errbuf()
        _check(_lib.pgh_glm_score_sparse_spa(self._h, subset._h if subset else None, v0, v1, _ptr(y), z.shape[0],
                                             _ptr(z) if z.size else None, float(cutoff), _ptr(rows), _ptr(p_spa),
                                             _ptr(state), eb), eb)
        return dict(Dataset._glm_rows_dict(rows), p_spa=p_spa, spa_state=state)

    def glm_score_sparse_firth(self, phenotype, covariates=None, firth_cutoff: float = 2.0, v_begin: int | None = None,
                               v_end: int | None = None, subset: Subset | None = None) -> dict:
        """pgh_glm_score_sparse_firth: glm_score_sparse() plus the approximate Firth estimate (the covariate effects
        fixed at the null fit, the genotype coded against the row's base code) for the rows with |stat| > firth_cutoff
        (firth_cutoff >= 0.1; inf = never).  Returns glm_score_sparse()'s dict unchanged and, all of shape
        (n_variants,), beta_firth, se_firth, p_firth (float64: NaN for a row that is not fitted, the score row's beta,
        se, p where Firth was not applied or failed) and firth_state (uint8: 0 = not applied, 1 = applied,
        2 = attempted and failed)."""
        v0, v1, y, z = Dataset._score_sparse_args(self, phenotype, covariates, v_begin, v_end, subset)
        nv = max(0, v1 - v0)
        rows = np.zeros(nv, dtype=GLM_ROW_DTYPE)
        firth = np.zeros(nv, dtype=GLM_FIRTH_ROW_DTYPE)
        eb = _errbuf()
        _check(_lib.pgh_glm_score_sparse_firth(self._h, subset._h if subset else None, v0, v1, _ptr(y), z.shape[0],
                                               _ptr(z) if z.size else None, float(firth_cutoff), _ptr(rows),
                                               _ptr(firth), eb), eb)
        return dict(Dataset._glm_rows_dict(rows), beta_firth=firth["beta"].copy(), se_firth=firth["se"].copy(),
                    p_firth=firth["p"].copy(), firth_state=firth["state"].copy())

    @staticmethod
    def _set_args(set_off, set_vidx, weights):
        """(set_off as uint64, set_vidx as uint32, weights as float64 or None) of the set calls, after their shape
        checks."""
        off = np.asarray(set_off)
        vidx = np.asarray(set_vidx)
        for name, a in (("set_off", off), ("set_vidx", vidx)):
            if a.ndim != 1 or (a.size and (a.dtype.kind not in "iu" or int(a.min()) < 0)):
                raise ValueError(f"{name} must be a one-dimensional array of non-negative integers")
        if off.size == 0:
            raise ValueError("set_off must hold n_sets + 1 offsets")
        if vidx.size and int(vidx.max()) > 0xFFFFFFFF:
            raise ValueError("set_vidx holds an index that is not an unsigned 32-bit number")
        off = np.ascontiguousarray(off, dtype=np.uint64)
        vidx = np.ascontiguousarray(vidx, dtype=np.uint32)
        n_sets = off.size - 1
        # the library reads set_off[n_sets] memberships: the arrays must hold them (the rest is the library's to check)
        if n_sets and np.all(off[1:] >= off[:-1]) and int(off[-1]) != vidx.size:
            raise ValueError(f"set_vidx must hold set_off[-1] = {int(off[-1])} memberships, got {vidx.size}")
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.float64)
            if w.shape != vidx.shape:
                raise ValueError(f"weights must hold one value per membership ({vidx.size}), got shape {w.shape}")
        return off, vidx, w

    def burden_sparse(self, phenotype, set_off, set_vidx, weights=None, covariates=None,
                      subset: Subset | None = None) -> np.ndarray:
        """pgh_burden_sparse: per variant set, the linear fit of phenotype on the weighted burden of the set's variants
        plus covariates, over a sparse-resident dataset.  The sets are in CSR form: set s is
        set_vidx[set_off[s]:set_off[s + 1]], indices into the dataset's resident variants (0 = v_begin), any order,
        repeats counted; weights: None (1.0) or one per membership.  Returns one BURDEN_ROW_DTYPE row per set
        (errcode: an index into GLM_ERRCODES)."""
        n_out = subset.size if subset else self.n_samples
        y = np.ascontiguousarray(phenotype, dtype=np.float64)
        if y.shape != (n_out,):
            raise ValueError(f"phenotype must hold one value per output sample ({n_out}), got shape {y.shape}")
        if covariates is None:
            z = np.zeros((0, n_out), dtype=np.float64)
        else:
            z = np.ascontiguousarray(np.atleast_2d(np.asarray(covariates, dtype=np.float64)))
            if z.shape[1] != n_out:
                raise ValueError(f"covariates must be n_covar x {n_out}, got shape {z.shape}")
        off, vidx, w = Dataset._set_args(set_off, set_vidx, weights)
        n_sets = off.size - 1
        rows = np.zeros(n_sets, dtype=BURDEN_ROW_DTYPE)
        eb = _errbuf()
        _check(_lib.pgh_burden_sparse(self._h, subset._h if subset else None, _ptr(y), z.shape[0],
                                      _ptr(z) if z.size else None, n_sets, _ptr(off), _ptr(vidx) if vidx.size else None,
                                      _ptr(w) if w is not None and w.size else None, _ptr(rows), eb), eb)
        return rows

    def skat_sparse(self, phenotype, set_off, set_vidx, weights=None, covariates=None, subset: Subset | None = None,
                    return_lambda: bool = False):
        """pgh_skat_sparse: per variant set, the SKAT test and the burden score test of a 0 / 1 phenotype (NaN =
        missing) under glm_score_sparse()'s null model, over a sparse-resident dataset.  The sets and weights are
        burden_sparse()'s, at most SKAT_MAX_SET memberships a set.  Returns one SKAT_ROW_DTYPE row per set (errcode: an
        index into GLM_ERRCODES; p_state: SKAT_P_*), and with return_lambda also the eigenvalues of every set, all
        memberships of set s at set_off[s], descending (float64; NaN for a row that is not decided)."""
        _, _, y, z = Dataset._score_sparse_args(self, phenotype, covariates, None, None, subset)
        off, vidx, w = Dataset._set_args(set_off, set_vidx, weights)
        n_sets = off.size - 1
        rows = np.zeros(n_sets, dtype=SKAT_ROW_DTYPE)
        lam = np.zeros(vidx.size, dtype=np.float64) if return_lambda else None
        eb = _errbuf()
        _check(_lib.pgh_skat_sparse(self._h, subset._h if subset else None, _ptr(y), z.shape[0],
                                    _ptr(z) if z.size else None, n_sets, _ptr(off), _ptr(vidx) if vidx.size else None,
                                    _ptr(w) if w is not None and w.size else None, _ptr(rows),
                                    _ptr(lam) if lam is not None and lam.size else None, eb), eb)
        return (rows, lam) if return_lambda else rows

    def score_sparse(self, vidx, weights, flip=None, mode: int = SCORE_MEAN_IMPUTE, subset: Subset | None = None,
                     dosage_sum: bool = True):
        """pgh_score_sparse: score() over a sparse-resident dataset (Dataset.open(..., sparse=True)), from the listed
        variants' entries.  weights: n_scored finite values, or n_scored x n_cols.  Returns what score() returns:
        (score_sum [n_out][n_cols], dosage_sum [n_out] or None, allele_ct [n_out])."""
        v = np.asarray(vidx)
        if v.ndim != 1 or (v.size and (v.dtype.kind not in "iu" or int(v.min()) < 0 or int(v.max()) > 0xFFFFFFFF)):
            raise ValueError("vidx must be a one-dimensional array of unsigned 32-bit variant indices")
        v = np.ascontiguousarray(v, dtype=np.uint32)
        w = np.ascontiguousarray(weights, dtype=np.float64)
        if w.ndim == 1:
            w = w.reshape(-1, 1)
        if w.ndim != 2 or w.shape[0] != v.size:
            raise ValueError(f"weights must be n_scored ({v.size}) values or n_scored x n_cols, got shape {w.shape}")
        n_scored, n_cols = w.shape
        flip_a = None
        if flip is not None:
            flip_a = np.ascontiguousarray(flip, dtype=np.uint8)
            if flip_a.shape != (n_scored,):
                raise ValueError(f"flip must hold one value per scored variant ({n_scored}), got shape {flip_a.shape}")
        n_out = subset.size if subset else self.n_samples
        score = np.zeros((n_out, n_cols), dtype=np.float64)
        dos = np.zeros(n_out, dtype=np.float64) if dosage_sum else None
        ac = np.zeros(n_out, dtype=np.uint32)
        eb = _errbuf()
        _check(_lib.pgh_score_sparse(self._h, subset._h if subset else None, n_scored, _ptr(v) if n_scored else None,
                                     _ptr(w) if w.size else None, _ptr(flip_a) if n_scored and flip_a is not None else None,
                                     n_cols, int(mode), _ptr(score), _ptr(dos), _ptr(ac), eb), eb)
        return score, dos, ac

    def king_counts(self, v_begin: int | None = None, v_end: int | None = None, vidx=None,
                    subset: Subset | None = None, i_range=None, j_range=None) -> np.ndarray:
        """pgh_king_counts: uint32[KING_PLANES][ni][nj], the KING pair counts (NSNP, HETHET, IBS0, HET1HOM2, HET2HOM1;
        "1" is the row sample) of output samples i_range x j_range (default: all of them) over a variant range or
        list."""
        n_out = subset.size if subset else self.n_samples
        i0, i1 = (0, n_out) if i_range is None else (int(i_range[0]), int(i_range[1]))
        j0, j1 = (0, n_out) if j_range is None else (int(j_range[0]), int(j_range[1]))
        v0, n, v = self._range_or_list(v_begin, v_end, vidx)
        for x in (i0, i1, j0, j1, v0, n):
            if not 0 <= x <= 0xFFFFFFFF:
                raise ValueError(f"king_counts: {x} is not an unsigned 32-bit index")
        out = np.zeros((KING_PLANES, max(0, i1 - i0), max(0, j1 - j0)), dtype=np.uint32)
        eb = _errbuf()
        _check(_lib.pgh_king_counts(self._h, subset._h if subset else None, v0, n, _ptr(v) if v is not None else None,
                                    i0, i1, j0, j1, _ptr(out), eb), eb)
        return out

    def king_table_capped(self, min_kinship: float, capacity: int, v_begin: int | None = None,
                          v_end: int | None = None, vidx=None, subset: Subset | None = None):
        """pgh_king_table as it is: (rows, n_pairs) -- the first `capacity` rows at most of the table in (i, j) order
        (a KING_PAIR_DTYPE array) and the number of qualifying pairs.  capacity 0 is a counting call."""
        v0, n, v = self._range_or_list(v_begin, v_end, vidx)
        for x in (v0, n):
            if not 0 <= x <= 0xFFFFFFFF:
                raise ValueError(f"king_table: {x} is not an unsigned 32-bit index")
        capacity = int(capacity)
        rows = np.zeros(capacity, dtype=KING_PAIR_DTYPE)
        found = C.c_uint64(0)
        eb = _errbuf()
        _check(_lib.pgh_king_table(self._h, subset._h if subset else None, v0, n, _ptr(v) if v is not None else None,
                                   float(min_kinship), _ptr(rows) if capacity else None, capacity, C.byref(found), eb),
               eb)
        return rows[: min(found.value, capacity)], int(found.value)

    def king_table(self, min_kinship: float = float("-inf"), v_begin: int | None = None, v_end: int | None = None,
                   vidx=None, subset: Subset | None = None) -> np.ndarray:
        """The pairs i < j of the output samples with kinship >= min_kinship (-inf or NaN: every pair, NaN ones
        included), ascending by (i, j), as a KING_PAIR_DTYPE array (i, j, nsnp, hethet, ibs0, het1hom2, het2hom1,
        kinship).  A second call with a buffer of the reported size follows when the first was too small."""
        rows, found = self.king_table_capped(min_kinship, 65536, v_begin, v_end, vidx, subset)
        if found > len(rows):
            rows, found = self.king_table_capped(min_kinship, found, v_begin, v_end, vidx, subset)
        return rows

    def grm(self, v_begin: int | None = None, v_end: int | None = None, vidx=None, subset: Subset | None = None,
            freq=None, i_range=None, j_range=None, meanimpute: bool = False, want_nobs: bool = True):
        """pgh_grm: (rel float64[ni][nj], nobs uint32[ni][nj], n_used) -- the variance-standardised relationship
        matrix of output samples i_range x j_range (default: all of them) over a variant range or list.  rel is the
        sum over the used variants of z_i z_j divided by nobs (the variants at which both are called), or by n_used
        with meanimpute; freq: one allele frequency per variant of the call instead of the counted one.  want_nobs=False
        passes NULL for nobs (a smaller device block and a third less to copy back) and returns None in its place."""
        n_out = subset.size if subset else self.n_samples
        i0, i1 = (0, n_out) if i_range is None else (int(i_range[0]), int(i_range[1]))
        j0, j1 = (0, n_out) if j_range is None else (int(j_range[0]), int(j_range[1]))
        v0, n, v = self._range_or_list(v_begin, v_end, vidx)
        for x in (i0, i1, j0, j1, v0, n):
            if not 0 <= x <= 0xFFFFFFFF:
                raise ValueError(f"grm: {x} is not an unsigned 32-bit index")
        f = None
        if freq is not None:
            f = np.ascontiguousarray(freq, dtype=np.float64)
            if f.shape != (n,):
                raise ValueError(f"grm: freq must hold one frequency per variant of the call ({n})")
        rel = np.zeros((max(0, i1 - i0), max(0, j1 - j0)), dtype=np.float64)
        nobs = np.zeros(rel.shape, dtype=np.uint32) if want_nobs else None
        used = C.c_uint32(0)
        eb = _errbuf()
        _check(_lib.pgh_grm(self._h, subset._h if subset else None, v0, n, _ptr(v) if v is not None else None,
                            _ptr(f) if f is not None else None, i0, i1, j0, j1,
                            GRM_MEANIMPUTE if meanimpute else 0, _ptr(rel), _ptr(nobs) if want_nobs else None,
                            C.byref(used), eb), eb)
        return rel, nobs, int(used.value)

    def het(self, v_begin: int | None = None, v_end: int | None = None, vidx=None, subset: Subset | None = None,
            freq=None, small_sample: bool = True):
        """pgh_het: (rows, used, n_used) -- per output sample a HET_ROW_DTYPE row (e_hom, f, e_sum, hom_ct, obs_ct):
        the expected and observed homozygous calls over the used variants of a range or list and the inbreeding
        coefficient f = (hom_ct - e_hom) / (obs_ct - e_hom); used: uint8 per variant of the call, 1 where it was not
        skipped.  freq: one allele frequency per variant of the call instead of the counted one (then small_sample
        must be False).  The same variants give the same bytes from a dataset, a window or a shard group."""
        n_out = subset.size if subset else self.n_samples
        v0, n, v = self._range_or_list(v_begin, v_end, vidx)
        for x in (v0, n):
            if not 0 <= x <= 0xFFFFFFFF:
                raise ValueError(f"het: {x} is not an unsigned 32-bit index")
        f = None
        if freq is not None:
            f = np.ascontiguousarray(freq, dtype=np.float64)
            if f.shape != (n,):
                raise ValueError(f"het: freq must hold one frequency per variant of the call ({n})")
        rows = np.zeros(max(n_out, 1), dtype=HET_ROW_DTYPE)  # (never a null pointer, also under the empty subset)
        used = np.zeros(max(n, 1), dtype=np.uint8)
        n_used = C.c_uint32(0)
        eb = _errbuf()
        _check(_lib.pgh_het(self._h, subset._h if subset else None, v0, n, _ptr(v) if v is not None else None,
                            _ptr(f) if f is not None else None, HET_SMALL_SAMPLE if small_sample else 0, _ptr(rows),
                            _ptr(used), C.byref(n_used), eb), eb)
        return rows[:n_out], used[:n], int(n_used.value)

    def ld_window_sums(self, v_begin: int | None = None, v_end: int | None = None, vidx=None,
                       subset: Subset | None = None, a_range=None, b_range=None) -> np.ndarray:
        """pgh_ld_window_sums: uint32[LD_PLANES][na][nb], ld_pairs' six sums (n, sum_a, sum_b, sum_ab, sum_a2, sum_b2)
        of the variant pairs a_range x b_range (indices into the call's variants; default: all of them) over a
        variant range or list."""
        v0, n, v = self._range_or_list(v_begin, v_end, vidx)
        a0, a1 = (0, n) if a_range is None else (int(a_range[0]), int(a_range[1]))
        b0, b1 = (0, n) if b_range is None else (int(b_range[0]), int(b_range[1]))
        for x in (a0, a1, b0, b1, v0, n):
            if not 0 <= x <= 0xFFFFFFFF:
                raise ValueError(f"ld_window_sums: {x} is not an unsigned 32-bit index")
        out = np.zeros((LD_PLANES, max(0, a1 - a0), max(0, b1 - b0)), dtype=np.uint32)
        eb = _errbuf()
        _check(_lib.pgh_ld_window_sums(self._h, subset._h if subset else None, v0, n,
                                       _ptr(v) if v is not None else None, a0, a1, b0, b1, _ptr(out), eb), eb)
        return out

    def _ld_band_args(self, who, win_end, window, v_begin, v_end, vidx):
        """The argument checks ld_prune and ld_scores share: (variant_begin, n_var, vidx or None, win_end)."""
        if (win_end is None) == (window is None):
            raise ValueError(f"{who}: pass exactly one of win_end and window")
        v0, n, v = self._range_or_list(v_begin, v_end, vidx)
        for x in (v0, n):
            if not 0 <= x <= 0xFFFFFFFF:
                raise ValueError(f"{who}: {x} is not an unsigned 32-bit index")
        if window is not None:
            if not 1 <= int(window) <= 0xFFFFFFFF:
                raise ValueError(f"{who}: window must be at least 1")
            w = np.minimum(np.arange(n, dtype=np.int64) + int(window), n).astype(np.uint32)
        else:
            w = np.asarray(win_end)
            if w.shape != (n,) or (n and (w.min() < 0 or w.max() > 0xFFFFFFFF)):
                raise ValueError(f"{who}: win_end must hold one unsigned 32-bit value per variant ({n})")
            w = np.ascontiguousarray(w, dtype=np.uint32)
        return v0, n, v, w

    def ld_prune(self, r2: float, win_end=None, window: int | None = None, v_begin: int | None = None,
                 v_end: int | None = None, vidx=None, subset: Subset | None = None) -> np.ndarray:
        """pgh_ld_prune: the boolean keep array of greedy pruning at r2 over a variant range or (strictly increasing)
        list.  Exactly one of win_end (the exclusive end of each variant's window, see ld_windows) and window (W:
        win_end[k] = min(k + W, n_var)) must be given."""
        v0, n, v, w = self._ld_band_args("ld_prune", win_end, window, v_begin, v_end, vidx)
        keep = np.zeros(n, dtype=np.uint8)
        kept = C.c_uint64(0)
        eb = _errbuf()
        _check(_lib.pgh_ld_prune(self._h, subset._h if subset else None, v0, n, _ptr(v) if v is not None else None,
                                 _ptr(w), float(r2), _ptr(keep), C.byref(kept), eb), eb)
        assert int(keep.sum()) == kept.value
        return keep.astype(bool)

    def ld_scores(self, win_end=None, window: int | None = None, unbiased: bool = False, want_counts: bool = False,
                  v_begin: int | None = None, v_end: int | None = None, vidx=None, subset: Subset | None = None):
        """pgh_ld_scores: float64[n_var], the LD score of every variant of a range or (strictly increasing) list:
        its self term plus ld_r2 of every defined pair of the band k < u < win_end[k] it belongs to, as anchor or as
        partner.  win_end / window as in ld_prune.  want_counts: (scores, uint32[n_var] defined partners)."""
        v0, n, v, w = self._ld_band_args("ld_scores", win_end, window, v_begin, v_end, vidx)
        score = np.zeros(n, dtype=np.float64)
        partners = np.zeros(n, dtype=np.uint32) if want_counts else None
        eb = _errbuf()
        _check(_lib.pgh_ld_scores(self._h, subset._h if subset else None, v0, n, _ptr(v) if v is not None else None,
                                  _ptr(w), LDSCORE_UNBIASED if unbiased else 0, _ptr(score), _ptr(partners), eb), eb)
        return (score, partners) if want_counts else score

    def unpack_samples(self, vidx, subset: Subset | None = None, missing_code: int = -9) -> np.ndarray:
        """int8[n_out][len(vidx)]: the calls sample-major (read_pfile orient := 'sample')."""
        v = np.ascontiguousarray(vidx, dtype=np.uint32)
        out = np.zeros((subset.size if subset else self.n_samples, len(v)), dtype=np.int8)
        eb = _errbuf()
        _check(_lib.pgh_unpack_samples(self._h, subset._h if subset else None, len(v), _ptr(v), _ptr(out), missing_code, eb), eb)
        return out

    def dosage_unpack_samples(self, vidx, subset: Subset | None = None) -> np.ndarray:
        """float64[n_out][len(vidx)]: the dosages sample-major, -9 = missing."""
        v = np.ascontiguousarray(vidx, dtype=np.uint32)
        out = np.zeros((subset.size if subset else self.n_samples, len(v)), dtype=np.float64)
        eb = _errbuf()
        _check(_lib.pgh_dosage_unpack_samples(self._h, subset._h if subset else None, len(v), _ptr(v), _ptr(out), eb), eb)
        return out

    def dosage_sums_dev(self, v_begin, v_end, d_sums: int, stream: int = 0, subset: Subset | None = None):
        eb = _errbuf()
        _check(_lib.pgh_dosage_sums_dev(self._h, subset._h if subset else None, v_begin, v_end, d_sums, stream, eb), eb)

    def dosage_unpack_dev(self, v_begin, v_end, d_out: int, out_stride: int, stream: int = 0,
                          subset: Subset | None = None):
        eb = _errbuf()
        _check(_lib.pgh_dosage_unpack_dev(self._h, subset._h if subset else None, v_begin, v_end, d_out, out_stride,
                                          stream, eb), eb)

    def sample_counts_dev(self, v_begin, v_end, d_classes: int, stream: int = 0):
        eb = _errbuf()
        _check(_lib.pgh_sample_counts_dev(self._h, v_begin, v_end, d_classes, stream, eb), eb)

    def ld_pairs_dev(self, vidx_a: np.ndarray, vidx_b: np.ndarray, d_sums: int, stream: int = 0,
                     subset: Subset | None = None):
        """vidx_a / vidx_b: contiguous uint32 host arrays (kept by the caller); sums land in d_sums."""
        eb = _errbuf()
        _check(_lib.pgh_ld_pairs_dev(self._h, subset._h if subset else None, len(vidx_a), _ptr(vidx_a), _ptr(vidx_b),
                                     d_sums, stream, eb), eb)

    def ld_pairs(self, vidx_a, vidx_b, subset: Subset | None = None) -> np.ndarray:
        """uint32[n_pairs][6] = {n, sum_a, sum_b, sum_ab, sum_a2, sum_b2} per pair."""
        a = np.ascontiguousarray(vidx_a, dtype=np.uint32)
        b = np.ascontiguousarray(vidx_b, dtype=np.uint32)
        assert a.shape == b.shape and a.ndim == 1
        out = np.zeros((len(a), 6), dtype=np.uint32)
        eb = _errbuf()
        _check(_lib.pgh_ld_pairs(self._h, subset._h if subset else None, len(a), _ptr(a), _ptr(b), _ptr(out), eb), eb)
        return out

    def pca_sharded(self, vidx, center, inv_stdev, n_var_total: int, n_pcs: int, g1_init, allreduce,
                    subset: Subset | None = None):
        """pgh_pca_sharded: this rank's effective variants + `allreduce(d_ptr, count, stream)`, a
        callable that sums `count` doubles at device pointer `d_ptr` in place over all ranks
        (see sharding.device_allreduce for the torch.distributed one)."""
        vidx = np.ascontiguousarray(vidx, dtype=np.uint32)
        center = np.ascontiguousarray(center, dtype=np.float64)
        inv_stdev = np.ascontiguousarray(inv_stdev, dtype=np.float64)
        g1 = np.ascontiguousarray(g1_init, dtype=np.float64)
        n_out = subset.size if subset else self.n_samples
        assert g1.shape == (n_out, 2 * n_pcs)
        ev = np.zeros(n_pcs, dtype=np.float64)
        vecs = np.zeros((n_out, n_pcs), dtype=np.float64)
        failure = []

        def trampoline(_ctx, d_buf, count, stream):
            try:
                allreduce(int(d_buf), int(count), int(stream or 0))
                return 0
            except BaseException as exc:  # an exception must not unwind through the C frames
                failure.append(exc)
                return 1

        cb = ALLREDUCE_FN(trampoline)
        eb = _errbuf()
        rc = _lib.pgh_pca_sharded(self._h, subset._h if subset else None, len(vidx), _ptr(vidx), _ptr(center),
                                  _ptr(inv_stdev), n_var_total, n_pcs, _ptr(g1), cb, None, _ptr(ev), _ptr(vecs), eb)
        if failure:
            raise failure[0]
        _check(rc, eb)
        return ev, vecs

    def reader(self, subset: Subset | None = None) -> "Reader":
        return Reader(self, subset)


class ScorePlan:
    """Uploaded weights + per-variant tables of one plink_score call (pgh_score_plan)."""

    def __init__(self, ds: Dataset, vidx, weights, flip, mode, subset):
        vidx = np.ascontiguousarray(vidx, dtype=np.uint32)
        weights = np.ascontiguousarray(weights, dtype=np.float64)
        if weights.ndim == 1:
            weights = weights.reshape(-1, 1)
        flip_a = None if flip is None else np.ascontiguousarray(flip, dtype=np.uint8)
        self.ds = ds
        self.n_cols = weights.shape[1]
        self._h = C.c_void_p()
        eb = _errbuf()
        _check(_lib.pgh_score_plan_create(ds._h, subset._h if subset else None, weights.shape[0], _ptr(vidx),
                                          _ptr(weights), _ptr(flip_a), weights.shape[1], mode, C.byref(self._h), eb), eb)

    def run_dev(self, d_score: int, d_dosage: int, d_allele: int, stream: int = 0):
        eb = _errbuf()
        _check(_lib.pgh_score_run_dev(self._h, d_score, d_dosage, d_allele, stream, eb), eb)

    def close(self):
        if self._h:
            _lib.pgh_score_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        self.close()


class Reader:
    """Per-scan-thread view with pgenlib-shaped per-variant calls (pgh_reader)."""

    def __init__(self, ds: Dataset, subset: Subset | None = None):
        self.ds = ds
        self.subset = subset
        self.n_out = subset.size if subset else ds.n_samples
        self._h = C.c_void_p()
        eb = _errbuf()
        _check(_lib.pgh_reader_create(ds._h, subset._h if subset else None, C.byref(self._h), eb), eb)

    def _chk(self, rc):
        if rc != PGH_OK:
            msg = _lib.pgh_reader_error(self._h).decode("utf-8", "replace")
            raise (PghArgError if rc == PGH_ERR_ARG else PghError)(rc, msg)

    def get_counts(self, vidx: int) -> np.ndarray:
        out = np.zeros(4, dtype=np.uint32)
        self._chk(_lib.pgh_get_counts(self._h, vidx, _ptr(out)))
        return out

    def get_2bit(self, vidx: int) -> np.ndarray:
        out = np.zeros((self.n_out + 31) // 32, dtype=np.uint64)
        self._chk(_lib.pgh_get_2bit(self._h, vidx, _ptr(out)))
        return out

    def get_missingness(self, vidx: int) -> np.ndarray:
        out = np.zeros((self.n_out + 63) // 64, dtype=np.uint64)
        self._chk(_lib.pgh_get_missingness(self._h, vidx, _ptr(out)))
        return out

    def get_int8(self, vidx: int) -> np.ndarray:
        out = np.zeros(self.n_out, dtype=np.int8)
        self._chk(_lib.pgh_get_int8(self._h, vidx, _ptr(out)))
        return out

    def get_phased(self, vidx: int):
        g = np.zeros((self.n_out + 31) // 32, dtype=np.uint64)
        pp = np.zeros((self.n_out + 63) // 64, dtype=np.uint64)
        pi = np.zeros((self.n_out + 63) // 64, dtype=np.uint64)
        self._chk(_lib.pgh_get_phased(self._h, vidx, _ptr(g), _ptr(pp), _ptr(pi)))
        return g, pp, pi

    def get_dosage_f64(self, vidx: int) -> np.ndarray:
        out = np.zeros(self.n_out, dtype=np.float64)
        self._chk(_lib.pgh_get_dosage_f64(self._h, vidx, _ptr(out)))
        return out

    def close(self):
        if self._h:
            _lib.pgh_reader_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        self.close()
