"""ctypes binding of libpfmscan.so (include/pfmscan.h).

The product path has no CPU fallback: if the library is missing or no gfx950
device is visible, everything here raises.  Nothing under ``oracle/`` is ever
imported from this package.
"""
import ctypes
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PFMSCAN_LIB") or os.path.join(HERE, "libpfmscan.so")   # override: A/B of two builds

OK = 0
E_BADARG, E_BADSHAPE, E_OOM, E_HIP, E_CAPACITY = -1, -2, -3, -4, -5
PROFILE_NONE, PROFILE_F32, PROFILE_F64 = 0, 1, 2
SEP = 7
NCODE = 8
NSTRUCT = 7
MAX_M = 64            # widest PFM of the tuned kernels and of PFM libraries
MAX_WIDTH = 4096      # widest PFM accepted (wider than MAX_M: the plain rolled-loop kernel)
ABI_VERSION = 27          # the posterior site map (pfmscan_footprint_*) added entry points under the same number

# every symbol include/pfmscan.h declares (checked by tests/test_abi.py)
SYMBOLS = [
    "pfmscan_abi_version", "pfmscan_ctx_create", "pfmscan_ctx_destroy", "pfmscan_last_error",
    "pfmscan_device_info", "pfmscan_synchronize", "pfmscan_motif_create", "pfmscan_motif_destroy",
    "pfmscan_pwm_calculate", "pfmscan_scan_dev", "pfmscan_scan_letters_f64_dev", "pfmscan_hits_dev",
    "pfmscan_scan_host", "pfmscan_scan_letters_f64_host", "pfmscan_hits_host", "pfmscan_time_scan_dev",
    "pfmscan_stage", "pfmscan_scan_staged", "pfmscan_hits_staged", "pfmscan_hits_adaptive_dev",
    "pfmscan_library_create", "pfmscan_library_destroy", "pfmscan_library_info", "pfmscan_library_hits_dev",
    "pfmscan_library_hits_staged", "pfmscan_library_hits_host", "pfmscan_library_hits_pipeline_host", "pfmscan_debug_credit_table",
    "pfmscan_library_create_letters", "pfmscan_library_hits_letters_dev", "pfmscan_library_hits_letters_host", "pfmscan_debug_library8_credits",
    "pfmscan_debug_credit8_table",
    "pfmscan_hits_pipeline_host", "pfmscan_staged_positions",
    "pfmscan_hits_letters_f64_dev", "pfmscan_hits_letters_f64_staged", "pfmscan_hits_letters_f64_host",
    "pfmscan_hits_pair_dev", "pfmscan_stage_codes2", "pfmscan_hits_pair_staged", "pfmscan_hits_pair_host", "pfmscan_round_decimals",
    "pfmscan_set_upload_mode", "pfmscan_upload_source_file", "pfmscan_upload_source_file_checked", "pfmscan_fasta_lone_cr", "pfmscan_count_bytes", "pfmscan_fasta_index", "pfmscan_fasta_ids", "pfmscan_gather_spans", "pfmscan_fasta_encode", "pfmscan_tsv_format", "pfmscan_profile_parse", "pfmscan_tsv_number",
    "pfmscan_place_alloc", "pfmscan_place_free", "pfmscan_place_note", "pfmscan_place_trim",
    "pfmscan_dotbracket_annotate_dev", "pfmscan_dotbracket_stage", "pfmscan_dotbracket_annotate_host",
    "pfmscan_average_dev", "pfmscan_average_host", "pfmscan_average_stage", "pfmscan_fragment_ids",
    "pfmscan_profile_colsums_dev", "pfmscan_profile_colsums_host", "pfmscan_profile_colsums_staged",
    "pfmscan_hits_sum_dev", "pfmscan_hits_sum_staged", "pfmscan_hits_sum_host", "pfmscan_hits_sum_pipeline_host",
    "pfmscan_library_hits_sum_dev", "pfmscan_library_hits_sum_staged", "pfmscan_library_hits_sum_host",
    "pfmscan_profile_row_bound_dev", "pfmscan_profile_row_bound_staged", "pfmscan_library_sum_thresholds",
    "pfmscan_site_groups", "pfmscan_site_sums_dev", "pfmscan_site_sums_staged", "pfmscan_site_sums_host",
    "pfmscan_site_groups_lib", "pfmscan_site_order_lib", "pfmscan_site_acc_add", "pfmscan_site_acc_round",
    "pfmscan_site_acc_from_doubles", "pfmscan_site_sums_lib_dev", "pfmscan_site_sums_lib_staged",
    "pfmscan_hits_pair_sum_dev", "pfmscan_hits_pair_sum_staged", "pfmscan_hits_pair_sum_host", "pfmscan_pair_sum_route",
    "pfmscan_debug_round3d", "pfmscan_debug_pair_sum_test", "pfmscan_debug_pair_credits",
    "pfmscan_library_hits_letters_sum_dev", "pfmscan_library_hits_letters_sum_host", "pfmscan_library_letters_sum_thresholds",
    "pfmscan_library_last_launches",
    "pfmscan_site_joint_dev", "pfmscan_site_joint_staged",
    "pfmscan_mutmap_dev", "pfmscan_mutmap_staged", "pfmscan_mutmap_events_dev", "pfmscan_mutmap_events_staged",
    "pfmscan_variants_dev", "pfmscan_variants_staged",
    "pfmscan_occupancy_dev", "pfmscan_occupancy_staged",
    "pfmscan_occupancy_profile_dev", "pfmscan_occupancy_profile_staged",
    "pfmscan_expect_dev", "pfmscan_expect_staged",
    "pfmscan_expect_profile_dev", "pfmscan_expect_profile_staged",
    "pfmscan_occupancy_pair_dev", "pfmscan_occupancy_pair_staged", "pfmscan_expect_pair_dev", "pfmscan_expect_pair_staged",
    "pfmscan_expect_merge_dev", "pfmscan_expect_merged_staged", "pfmscan_expect_profile_merged_staged", "pfmscan_expect_pair_merged_staged",
    "pfmscan_expect_pair_joint_dev", "pfmscan_expect_pair_joint_staged", "pfmscan_expect_pair_joint_merged_staged",
    # added under ABI 27, as the footprint entry points were: the number stays, the suite pins it
    "pfmscan_expect_profile_joint_dev", "pfmscan_expect_profile_joint_staged", "pfmscan_expect_profile_joint_merged_staged",
    "pfmscan_footprint_dev", "pfmscan_footprint_staged", "pfmscan_footprint_events_dev", "pfmscan_footprint_events_staged",
    "pfmscan_footprint_profile_dev", "pfmscan_footprint_profile_staged", "pfmscan_footprint_profile_events_dev", "pfmscan_footprint_profile_events_staged",
    "pfmscan_mutocc_dev", "pfmscan_mutocc_staged", "pfmscan_mutocc_events_dev", "pfmscan_mutocc_events_staged",
    "pfmscan_multisite_dev", "pfmscan_multisite_staged", "pfmscan_multisite_events_dev", "pfmscan_multisite_events_staged",
    "pfmscan_multisite_profile_dev", "pfmscan_multisite_profile_staged", "pfmscan_multisite_profile_events_dev", "pfmscan_multisite_profile_events_staged",
]
PAIR_ROUTE_NONE, PAIR_ROUTE_FUSED, PAIR_ROUTE_TWO_PHASE, PAIR_ROUTE_DENSE, PAIR_ROUTE_CREDITS = range(5)   # Context.pair_sum_route()
SITE_GROUP = 4096     # most hits of one group of the site profiles
SITE_LIMBS = 66       # 64-bit limbs of one cell of a long accumulator (site profiles of a library)
SITE_JOINT_COLS = 64  # columns of one LDS tile of the letter-pair counts (PFMSCAN_SITE_JOINT_COLS)
EXPECT_RATIO, EXPECT_POSTERIOR = 0, 1   # weight of a window in the expected counts (PFMSCAN_EXPECT_*)
OCC_FANIN = 32        # fan-in of the occupancy's summation tree (PFMSCAN_OCC_FANIN)
FOOTPRINT_SLOTS = 512  # windows a workgroup of the posterior site map makes (PFMSCAN_FOOTPRINT_SLOTS): its tile is SLOTS - (m - 1) positions
FOOTPRINT_PROFILE_SLOTS = 256  # the same on averaged-structure profiles (PFMSCAN_FOOTPRINT_PROFILE_SLOTS)
MULTISITE_SLOTS = 512  # windows a workgroup of the multi-site model's tile-parallel kernels holds (PFMSCAN_MULTISITE_SLOTS): its tile is SLOTS - (m - 1) positions
MULTISITE_CHUNK = 28   # positions of a record a lane of its two serial kernels holds in LDS at a time (PFMSCAN_MULTISITE_CHUNK)
MUTOCC_TILE = 512     # positions of ONE record a workgroup of the threshold-free mutagenesis owns (PFMSCAN_MUTOCC_TILE)
MAX_COVER = 1024      # largest coverage of a row the averaging accepts
AVG_OK, AVG_DOTBRACKET, AVG_UNCOVERED, AVG_COVER, AVG_BAD_TABLE = range(5)   # what a rejected averaging names
TSV_CONST, TSV_I64, TSV_F32, TSV_F64, TSV_INDEXED, TSV_FIXED, TSV_WINDOW, TSV_SPAN = range(8)


class TsvColumn(ctypes.Structure):
    """pfmscan_tsv_column of include/pfmscan.h"""
    _fields_ = [("kind", ctypes.c_int32), ("reserved", ctypes.c_int32), ("data", ctypes.c_void_p),
                ("aux", ctypes.c_void_p), ("blob", ctypes.c_void_p), ("width", ctypes.c_int64)]



class CapacityError(RuntimeError):
    """Hit buffer too small; ``required`` holds the number of hits."""

    def __init__(self, msg, required):
        RuntimeError.__init__(self, msg)
        self.required = required


_lib = None


def _preload_hip_runtime():
    """A process must hold ONE HIP/HSA runtime.  PyTorch-ROCm wheels bundle their own
    libamdhip64.so / libhsa-runtime64.so; if libpfmscan (linked against /opt/rocm) came
    first, a later ``import torch`` would bring a second HSA runtime and see no GPU.  So
    when torch is installed its copy of the HIP runtime is loaded first -- by path, without
    importing torch -- and libpfmscan's NEEDED libamdhip64.so.7 binds to it."""
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)


def load():
    """Load the shared library (once).  Raises ImportError when it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "rnascan_amd: %s is missing -- build it with `python -m rnascan_amd.build` "
            "(hipcc --offload-arch=gfx950); there is no CPU fallback" % LIB_PATH)
    _preload_hip_runtime()
    L = ctypes.CDLL(LIB_PATH)
    vp, i32, i64, dbl = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
    L.pfmscan_abi_version.restype = i32
    L.pfmscan_ctx_create.argtypes = [i32, ctypes.POINTER(vp)]
    L.pfmscan_ctx_destroy.argtypes = [vp]
    L.pfmscan_ctx_destroy.restype = None
    L.pfmscan_last_error.argtypes = [vp]
    L.pfmscan_last_error.restype = ctypes.c_char_p
    L.pfmscan_device_info.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(i64), ctypes.c_char_p, i32]
    L.pfmscan_synchronize.argtypes = [vp]
    L.pfmscan_motif_create.argtypes = [vp, vp, vp, i32, ctypes.POINTER(vp)]
    L.pfmscan_motif_destroy.argtypes = [vp]
    L.pfmscan_motif_destroy.restype = None
    L.pfmscan_pwm_calculate.argtypes = [vp, ctypes.c_char_p, i64, vp, i64, vp]
    L.pfmscan_scan_dev.argtypes = [vp, vp, vp, vp, i32, i64, vp, vp, vp]
    L.pfmscan_scan_letters_f64_dev.argtypes = [vp, vp, vp, i64, vp, vp]
    L.pfmscan_hits_dev.argtypes = [vp, vp, vp, vp, i32, i64, dbl, dbl, i64, vp, vp, vp, vp, vp]
    L.pfmscan_hits_adaptive_dev.argtypes = [vp, vp, vp, vp, i32, i64, dbl, dbl, i64, vp, vp, vp, vp, vp]
    L.pfmscan_scan_host.argtypes = [vp, vp, vp, vp, i32, i64, vp, vp]
    L.pfmscan_scan_letters_f64_host.argtypes = [vp, vp, vp, i64, vp]
    L.pfmscan_hits_host.argtypes = [vp, vp, vp, vp, i32, i64, dbl, dbl, i64, vp, vp, vp, ctypes.POINTER(i64)]
    L.pfmscan_stage.argtypes = [vp, vp, vp, i32, i64]
    L.pfmscan_scan_staged.argtypes = [vp, vp, vp, vp]
    L.pfmscan_staged_positions.argtypes = [vp]
    L.pfmscan_hits_staged.argtypes = [vp, vp, dbl, dbl, i64, vp, vp, vp, ctypes.POINTER(i64)]
    L.pfmscan_hits_sum_dev.argtypes = [vp, vp, vp, vp, i32, i64, dbl, dbl, dbl, i64, vp, vp, vp, vp, vp]
    L.pfmscan_hits_sum_staged.argtypes = [vp, vp, dbl, dbl, dbl, i64, vp, vp, vp, ctypes.POINTER(i64)]
    L.pfmscan_hits_sum_host.argtypes = [vp, vp, vp, vp, i32, i64, dbl, dbl, dbl, i64, vp, vp, vp, ctypes.POINTER(i64)]
    L.pfmscan_hits_sum_pipeline_host.argtypes = [vp, vp, vp, vp, i32, i64, i64, dbl, dbl, dbl, i64, vp, vp, vp, ctypes.POINTER(i64)]
    L.pfmscan_time_scan_dev.argtypes = [vp, vp, vp, vp, i32, i64, vp, vp, vp, i32, i32, ctypes.POINTER(dbl)]
    L.pfmscan_library_create.argtypes = [vp, vp, vp, i32, i32, ctypes.POINTER(vp)]
    L.pfmscan_library_create_letters.argtypes = [vp, vp, vp, i32, i32, ctypes.POINTER(vp)]
    L.pfmscan_library_hits_letters_dev.argtypes = [vp, vp, vp, vp, i64, vp, vp, i64, vp, vp, vp, vp, vp, vp]
    L.pfmscan_library_hits_letters_host.argtypes = [vp, vp, vp, vp, i64, vp, vp, i64, vp, vp, vp, vp, ctypes.POINTER(i64)]
    L.pfmscan_library_destroy.argtypes = [vp]
    L.pfmscan_library_destroy.restype = None
    L.pfmscan_library_info.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(i32),
                                       ctypes.POINTER(dbl)]
    L.pfmscan_library_hits_dev.argtypes = [vp, vp, vp, vp, i32, i64, vp, vp, i64, vp, vp, vp, vp, vp, vp]
    L.pfmscan_library_hits_staged.argtypes = [vp, vp, vp, vp, i64, vp, vp, vp, vp, ctypes.POINTER(i64)]
    L.pfmscan_library_hits_host.argtypes = [vp, vp, vp, vp, i32, i64, vp, vp, i64, vp, vp, vp, vp, ctypes.POINTER(i64)]
    L.pfmscan_library_hits_sum_dev.argtypes = [vp, vp, vp, vp, i32, i64, vp, vp, vp, dbl, i64, vp, vp, vp, vp, vp, vp]
    L.pfmscan_library_hits_sum_staged.argtypes = [vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, ctypes.POINTER(i64)]
    L.pfmscan_library_hits_sum_host.argtypes = [vp, vp, vp, vp, i32, i64, vp, vp, vp, i64, vp, vp, vp, vp, ctypes.POINTER(i64)]
    L.pfmscan_profile_row_bound_dev.argtypes = [vp, vp, vp, i32, i64, vp, vp]
    L.pfmscan_profile_row_bound_staged.argtypes = [vp, ctypes.POINTER(dbl)]
    L.pfmscan_library_sum_thresholds.argtypes = [vp, vp, i32, i32, vp, vp, dbl, vp]
    L.pfmscan_hits_pipeline_host.argtypes = [vp, vp, vp, vp, i32, i64, i64, dbl, dbl, i64, vp, vp, vp, ctypes.POINTER(i64)]
    L.pfmscan_library_hits_pipeline_host.argtypes = [vp, vp, vp, vp, i32, i64, i64, vp, vp, i64, vp, vp, vp, vp, ctypes.POINTER(i64)]
    L.pfmscan_debug_credit_table.argtypes = [vp, i32, dbl, i32, vp, ctypes.POINTER(dbl)]
    L.pfmscan_debug_credit8_table.argtypes = [vp, i32, dbl, vp, ctypes.POINTER(i32)]
    L.pfmscan_set_upload_mode.argtypes = [vp, i32]
    L.pfmscan_upload_source_file.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_char_p, i64]
    L.pfmscan_upload_source_file_checked.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_char_p, i64, i64, i64, i64]
    L.pfmscan_fasta_lone_cr.argtypes = [vp, i64, ctypes.POINTER(i32), i32]
    L.pfmscan_dotbracket_annotate_dev.argtypes = [vp, vp, vp, i64, vp, vp, ctypes.POINTER(i64), vp]
    L.pfmscan_dotbracket_stage.argtypes = [vp, vp, i64, i32, vp, vp, ctypes.POINTER(i64)]
    L.pfmscan_dotbracket_annotate_host.argtypes = [vp, vp, vp, i64, vp, vp, ctypes.POINTER(i64)]
    L.pfmscan_average_dev.argtypes = [vp, vp, i64, vp, vp, vp, i64, i64, vp, vp, vp, i64, i64, vp, i32, vp, i32,
                                      ctypes.POINTER(i64), ctypes.POINTER(i32), vp]
    L.pfmscan_average_host.argtypes = [vp, vp, i64, vp, vp, vp, i64, vp, vp, vp, i64, vp, i32, vp, i32,
                                       ctypes.POINTER(i64), ctypes.POINTER(i32)]
    L.pfmscan_average_stage.argtypes = [vp, vp, i64, vp, vp, vp, i64, vp, vp, vp, i64, vp, i32, i32,
                                        ctypes.POINTER(i64), ctypes.POINTER(i64), ctypes.POINTER(i32)]
    L.pfmscan_fragment_ids.argtypes = [vp, vp, vp, i64, vp, vp, ctypes.POINTER(i64)]
    L.pfmscan_profile_colsums_dev.argtypes = [vp, vp, i32, i64, vp, vp, i64, vp, ctypes.POINTER(i64), vp]
    L.pfmscan_profile_colsums_host.argtypes = [vp, vp, i32, i64, vp, vp, i64, vp, ctypes.POINTER(i64)]
    L.pfmscan_profile_colsums_staged.argtypes = [vp, vp, vp, i64, vp, ctypes.POINTER(i64)]
    L.pfmscan_site_groups.argtypes = [vp, i64, vp, vp, i64, i32, i64, vp, vp, ctypes.POINTER(i64)]
    L.pfmscan_site_sums_dev.argtypes = [vp, vp, vp, i32, i64, vp, i64, vp, vp, i64, vp, vp, i64, i32, i32, vp, vp,
                                        ctypes.POINTER(i64), vp]
    L.pfmscan_site_sums_staged.argtypes = [vp, i32, i32, vp, i64, vp, vp, i64, i32, i32, i64, vp, vp, vp, ctypes.POINTER(i64),
                                           ctypes.POINTER(i64)]
    L.pfmscan_site_sums_host.argtypes = [vp, vp, vp, i32, i64, vp, i64, vp, vp, i64, i32, i32, i64, vp, vp, vp,
                                         ctypes.POINTER(i64), ctypes.POINTER(i64)]
    L.pfmscan_site_groups_lib.argtypes = [vp, vp, i64, i32, vp, vp, i64, i32, i64, vp, vp, vp, ctypes.POINTER(i64)]
    L.pfmscan_site_order_lib.argtypes = [vp, vp, i64, i32, vp]
    L.pfmscan_site_acc_add.argtypes = [vp, vp, i64, i64]
    L.pfmscan_site_acc_round.argtypes = [vp, i64, i64, vp]
    L.pfmscan_site_acc_from_doubles.argtypes = [vp, i64, vp]
    L.pfmscan_site_sums_lib_dev.argtypes = [vp, vp, vp, i32, i64, vp, i64, vp, vp, vp, i64, vp, vp, i64, i32, i32, i32, vp, vp,
                                            ctypes.POINTER(i64), vp]
    L.pfmscan_site_sums_lib_staged.argtypes = [vp, i32, i32, vp, vp, i64, vp, vp, i64, i32, i32, i32, vp, vp, ctypes.POINTER(i64)]
    L.pfmscan_site_joint_dev.argtypes = [vp, vp, vp, i64, vp, vp, i64, vp, vp, i64, i32, i32, i32, vp, vp]
    L.pfmscan_site_joint_staged.argtypes = [vp, i32, i32, vp, vp, i64, vp, vp, i64, i32, i32, i32, vp]
    L.pfmscan_count_bytes.argtypes = [vp, i64, vp, i32]
    L.pfmscan_place_alloc.argtypes = [vp, i32, vp, vp, i32]
    L.pfmscan_place_free.argtypes = [vp, vp]
    L.pfmscan_place_trim.argtypes = [vp]
    L.pfmscan_place_note.argtypes = [vp]
    L.pfmscan_place_note.restype = ctypes.c_char_p
    L.pfmscan_fasta_index.argtypes = [vp, i64, i64, vp, vp, vp, vp, vp, ctypes.POINTER(i64), i32]
    L.pfmscan_fasta_ids.argtypes = [vp, vp, vp, i64, vp, vp, ctypes.POINTER(i32)]
    L.pfmscan_gather_spans.argtypes = [vp, vp, i64, i32, vp, i64, ctypes.POINTER(i64)]
    L.pfmscan_fasta_encode.argtypes = [vp, vp, vp, vp, i64, i64, vp, i32, vp, vp, i32]
    L.pfmscan_profile_parse.argtypes = [ctypes.c_char_p, i64, i32, i64, vp, ctypes.POINTER(i64)]
    L.pfmscan_tsv_number.argtypes = [vp, i64, i64, vp, i64, ctypes.POINTER(i64), ctypes.POINTER(i64), ctypes.POINTER(i32)]
    L.pfmscan_hits_letters_f64_dev.argtypes = [vp, vp, vp, i64, dbl, i64, vp, vp, vp, vp]
    L.pfmscan_hits_letters_f64_staged.argtypes = [vp, vp, dbl, i64, vp, vp, ctypes.POINTER(i64)]
    L.pfmscan_hits_letters_f64_host.argtypes = [vp, vp, vp, i64, dbl, i64, vp, vp, ctypes.POINTER(i64)]
    L.pfmscan_hits_pair_dev.argtypes = [vp, vp, vp, vp, vp, i64, dbl, dbl, i64, vp, vp, vp, vp, vp]
    L.pfmscan_stage_codes2.argtypes = [vp, vp, i64]
    L.pfmscan_hits_pair_staged.argtypes = [vp, vp, vp, dbl, dbl, i64, vp, vp, vp, ctypes.POINTER(i64)]
    L.pfmscan_hits_pair_host.argtypes = [vp, vp, vp, vp, vp, i64, dbl, dbl, i64, vp, vp, vp, ctypes.POINTER(i64)]
    L.pfmscan_round_decimals.argtypes = [vp, i64, i32, vp, i32]
    L.pfmscan_hits_pair_sum_dev.argtypes = [vp, vp, vp, vp, vp, i64, dbl, dbl, dbl, i64, vp, vp, vp, vp, vp]
    L.pfmscan_hits_pair_sum_staged.argtypes = [vp, vp, vp, dbl, dbl, dbl, i64, vp, vp, vp, ctypes.POINTER(i64)]
    L.pfmscan_hits_pair_sum_host.argtypes = [vp, vp, vp, vp, vp, i64, dbl, dbl, dbl, i64, vp, vp, vp, ctypes.POINTER(i64)]
    L.pfmscan_pair_sum_route.argtypes = [vp]
    L.pfmscan_library_last_launches.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.pfmscan_debug_round3d.argtypes = [vp, i64, vp]
    L.pfmscan_library_hits_letters_sum_dev.argtypes = [vp, vp, vp, vp, i64, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp]
    L.pfmscan_library_hits_letters_sum_host.argtypes = [vp, vp, vp, vp, i64, vp, vp, vp, i64, vp, vp, vp, vp, ctypes.POINTER(i64)]
    L.pfmscan_library_letters_sum_thresholds.argtypes = [vp, vp, i32, i32, vp, vp, vp]
    L.pfmscan_debug_pair_credits.argtypes = [vp, vp, i32, dbl, vp, vp] + [ctypes.POINTER(dbl)] * 4 + [ctypes.POINTER(i32)]
    L.pfmscan_debug_pair_sum_test.argtypes = [vp, vp, i64, dbl, vp, vp, ctypes.POINTER(dbl)]
    L.pfmscan_mutmap_dev.argtypes = [vp, vp, vp, i64, vp, vp, vp]
    L.pfmscan_mutmap_staged.argtypes = [vp, vp, vp, vp]
    L.pfmscan_mutmap_events_dev.argtypes = [vp, vp, vp, i64, dbl, i64, vp, vp, vp, vp, vp]
    L.pfmscan_mutmap_events_staged.argtypes = [vp, vp, dbl, i64, vp, vp, vp, ctypes.POINTER(i64)]
    L.pfmscan_variants_dev.argtypes = [vp, vp, i32, i32, vp, i64, vp, vp, i64, vp, vp, vp, vp, vp]
    L.pfmscan_variants_staged.argtypes = [vp, vp, i32, i32, vp, vp, i64, vp, vp, vp, vp]
    L.pfmscan_occupancy_dev.argtypes = [vp, vp, i32, i32, i32, vp, i64, vp, vp, i64, vp, vp]
    L.pfmscan_occupancy_staged.argtypes = [vp, i32, vp, i32, i32, i32, vp, vp, i64, vp, vp]
    L.pfmscan_occupancy_profile_dev.argtypes = [vp, vp, vp, i32, i32, vp, vp, i32, i64, vp, vp, i64, vp, vp]
    L.pfmscan_occupancy_profile_staged.argtypes = [vp, vp, vp, i32, i32, vp, vp, i64, vp, vp]
    L.pfmscan_expect_dev.argtypes = [vp, vp, i32, i32, i32, i32, vp, i64, vp, vp, i64, vp, vp, vp]
    L.pfmscan_expect_staged.argtypes = [vp, i32, vp, i32, i32, i32, i32, vp, vp, i64, vp, vp, vp]
    L.pfmscan_expect_profile_dev.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, i32, i64, vp, vp, i64, vp, vp, vp, vp]
    L.pfmscan_expect_profile_staged.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, i64, vp, vp, vp, vp]
    L.pfmscan_occupancy_pair_dev.argtypes = [vp, vp, vp, i32, i32, vp, vp, i64, vp, vp, i64, vp, vp]
    L.pfmscan_occupancy_pair_staged.argtypes = [vp, vp, vp, i32, i32, vp, vp, i64, vp, vp]
    L.pfmscan_expect_pair_dev.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, i64, vp, vp, i64, vp, vp, vp, vp]
    L.pfmscan_expect_pair_staged.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, i64, vp, vp, vp, vp]
    L.pfmscan_expect_merge_dev.argtypes = [vp, vp, i64, i32, i32, i32, vp, vp]
    L.pfmscan_expect_merged_staged.argtypes = [vp, i32, vp, i32, i32, i32, i32, vp, vp, i64, vp, vp, vp, vp]
    L.pfmscan_expect_profile_merged_staged.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, i64, vp, vp, vp, vp, vp, vp]
    L.pfmscan_expect_pair_merged_staged.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, i64, vp, vp, vp, vp, vp, vp]
    L.pfmscan_expect_pair_joint_dev.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, i64, vp, vp, i64, vp, vp, vp, vp, vp]
    L.pfmscan_expect_pair_joint_staged.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, i64, vp, vp, vp, vp, vp]
    L.pfmscan_expect_pair_joint_merged_staged.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp]
    L.pfmscan_footprint_dev.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, i64, vp, vp, i64, vp, vp, vp, vp]
    L.pfmscan_footprint_staged.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, i64, vp, vp, vp, vp]
    L.pfmscan_footprint_events_dev.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, i64, vp, vp, i64, dbl, i64, vp, vp, vp, vp, vp, vp]
    L.pfmscan_footprint_events_staged.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, i64, dbl, i64, vp, vp, vp, ctypes.POINTER(i64), vp, vp]
    L.pfmscan_multisite_dev.argtypes = [vp, vp, vp, i32, i32, vp, vp, i64, vp, vp, i64, vp, vp, vp, vp, vp, vp]
    L.pfmscan_multisite_staged.argtypes = [vp, vp, vp, i32, i32, vp, vp, i64, vp, vp, vp, vp, vp, vp]
    L.pfmscan_multisite_events_dev.argtypes = [vp, vp, vp, i32, i32, vp, vp, i64, vp, vp, i64, vp, dbl, i64, vp, vp, vp, vp, vp, vp, vp]
    L.pfmscan_multisite_events_staged.argtypes = [vp, vp, vp, i32, i32, vp, vp, i64, vp, dbl, i64, vp, vp, vp, ctypes.POINTER(i64), vp, vp, vp]
    L.pfmscan_multisite_profile_dev.argtypes = [vp, vp, vp, i32, i32, vp, vp, i32, i64, vp, vp, i64, vp, vp, vp, vp, vp, vp]
    L.pfmscan_multisite_profile_staged.argtypes = [vp, vp, vp, i32, i32, vp, vp, i64, vp, vp, vp, vp, vp, vp]
    L.pfmscan_multisite_profile_events_dev.argtypes = [vp, vp, vp, i32, i32, vp, vp, i32, i64, vp, vp, i64, vp, dbl, i64, vp, vp, vp, vp, vp, vp, vp]
    L.pfmscan_multisite_profile_events_staged.argtypes = [vp, vp, vp, i32, i32, vp, vp, i64, vp, dbl, i64, vp, vp, vp, ctypes.POINTER(i64), vp, vp, vp]
    L.pfmscan_footprint_profile_dev.argtypes =[vp, vp, vp, i32, i32, i32, vp, vp, i32, i64, vp, vp, i64, vp, vp, vp, vp]
    L.pfmscan_footprint_profile_staged.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, i64, vp, vp, vp, vp]
    L.pfmscan_footprint_profile_events_dev.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, i32, i64, vp, vp, i64, dbl, i64, vp, vp, vp, vp, vp, vp]
    L.pfmscan_footprint_profile_events_staged.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, i64, dbl, i64, vp, vp, vp, ctypes.POINTER(i64), vp, vp]
    L.pfmscan_mutocc_dev.argtypes = [vp, vp, i32, i32, vp, i64, vp, vp, i64, vp, vp, vp]
    L.pfmscan_mutocc_staged.argtypes = [vp, vp, i32, i32, vp, vp, i64, vp, vp, vp]
    L.pfmscan_mutocc_events_dev.argtypes = [vp, vp, i32, i32, vp, i64, vp, vp, i64, dbl, i64, vp, vp, vp, vp, vp, vp]
    L.pfmscan_mutocc_events_staged.argtypes = [vp, vp, i32, i32, vp, vp, i64, dbl, i64, vp, vp, vp, ctypes.POINTER(i64), vp, vp]
    L.pfmscan_expect_profile_joint_dev.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, i32, i64, vp, vp, i64, vp, vp, vp, vp, vp]
    L.pfmscan_expect_profile_joint_staged.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, i64, vp, vp, vp, vp, vp]
    L.pfmscan_expect_profile_joint_merged_staged.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp]
    L.pfmscan_tsv_format.argtypes = [ctypes.POINTER(TsvColumn), i32, i64, i64, vp, i64, ctypes.POINTER(i64), vp, ctypes.POINTER(i32), i32]
    for name in SYMBOLS:          # every other entry point returns a status
        if name not in ("pfmscan_ctx_destroy", "pfmscan_motif_destroy", "pfmscan_last_error", "pfmscan_library_destroy",
                        "pfmscan_staged_positions", "pfmscan_place_note"):
            getattr(L, name).restype = i32
    L.pfmscan_staged_positions.restype = i64
    if L.pfmscan_abi_version() != ABI_VERSION:
        raise ImportError("libpfmscan ABI %d, bindings expect %d" % (L.pfmscan_abi_version(), ABI_VERSION))
    _lib = L
    return L


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data_as(ctypes.c_void_p)
    return ctypes.c_void_p(int(a))          # raw device address (e.g. torch.Tensor.data_ptr())


def is_file_mapping(a):
    """True for an array whose memory is a mapped file (numpy memmap or a view of one / of an mmap object)"""
    import mmap
    while a is not None:
        if isinstance(a, (np.memmap, mmap.mmap)):
            return True
        a = getattr(a, "base", None)
    return False


def root_memmap(a):
    """the numpy.memmap an array is (a view of) -- the one that owns the mapping and knows its file -- or None"""
    root = None
    while a is not None:
        if isinstance(a, np.memmap) and getattr(a, "filename", None) is not None:
            root = a
        a = getattr(a, "base", None)
    return root


def _raise(L, ctx, rc, n_hits=None):
    msg = L.pfmscan_last_error(ctx).decode("utf-8", "replace")
    if rc in (E_BADARG, E_BADSHAPE):
        raise ValueError(msg)               # _pwm.c:96-113 raise ValueError
    if rc == E_OOM:
        raise MemoryError(msg)              # _pwm.c:27-31
    if rc == E_CAPACITY:
        raise CapacityError(msg, n_hits)
    raise RuntimeError("libpfmscan: " + msg)


# ---------------------------------------------------------------------------
# host ingest / output (no device, no context)
# ---------------------------------------------------------------------------
def site_groups(pos, offsets, lengths, m):
    """the groups of a sorted hit list (pfmscan_site_groups, include/pfmscan.h) -> (grp_first int64 [n_grp + 1], grp_rec
    int64 [n_grp]).  ValueError when the hits do not ascend strictly, a window [pos, pos + m) does not lie inside one
    record, or the record table is broken."""
    L = load()
    pos = np.ascontiguousarray(pos, dtype=np.int64)
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    ln = np.ascontiguousarray(lengths, dtype=np.int64)
    if pos.ndim != 1 or off.ndim != 1 or off.shape != ln.shape:
        raise ValueError("positions, offsets and lengths must be one-dimensional, the last two of the same size")
    n = ctypes.c_int64(0)
    first = np.zeros(1, dtype=np.int64)
    rc = L.pfmscan_site_groups(_ptr(pos), pos.size, _ptr(off), _ptr(ln), off.size, int(m), 0, _ptr(first), None, ctypes.byref(n))
    if rc == E_CAPACITY:
        first = np.zeros(n.value + 1, dtype=np.int64)
        rec = np.zeros(n.value, dtype=np.int64)
        rc = L.pfmscan_site_groups(_ptr(pos), pos.size, _ptr(off), _ptr(ln), off.size, int(m), n.value, _ptr(first), _ptr(rec),
                                   ctypes.byref(n))
    else:
        rec = np.zeros(0, dtype=np.int64)
    if rc != 0:
        raise ValueError("site groups: the hits must ascend strictly and every window of width %d must lie inside one record "
                         "of a record table whose records ascend, each behind the separator of the one before" % int(m))
    return first, rec


def site_groups_lib(pos, motif, n_motifs, offsets, lengths, m):
    """the per-motif groups of a MOTIF-MAJOR hit list (pfmscan_site_groups_lib, include/pfmscan.h) -> (grp_first int64
    [n_grp + 1], grp_rec int64 [n_grp], grp_motif int64 [n_grp]).  ValueError for a list that is not motif-major, a motif
    index outside [0, n_motifs), a window outside its record or a broken record table."""
    L = load()
    pos = np.ascontiguousarray(pos, dtype=np.int64)
    motif = np.ascontiguousarray(motif, dtype=np.int32)
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    ln = np.ascontiguousarray(lengths, dtype=np.int64)
    if pos.ndim != 1 or pos.shape != motif.shape or off.ndim != 1 or off.shape != ln.shape:
        raise ValueError("positions and motifs, offsets and lengths must be one-dimensional and pairwise of the same size")
    n = ctypes.c_int64(0)
    first = np.zeros(1, dtype=np.int64)
    rec = mot = np.zeros(0, dtype=np.int64)
    args = (_ptr(pos), _ptr(motif), pos.size, int(n_motifs), _ptr(off), _ptr(ln), off.size, int(m))
    rc = L.pfmscan_site_groups_lib(*args, 0, _ptr(first), None, None, ctypes.byref(n))
    if rc == E_CAPACITY:
        first = np.zeros(n.value + 1, dtype=np.int64)
        rec = np.zeros(n.value, dtype=np.int64)
        mot = np.zeros(n.value, dtype=np.int64)
        rc = L.pfmscan_site_groups_lib(*args, n.value, _ptr(first), _ptr(rec), _ptr(mot), ctypes.byref(n))
    if rc != 0:
        raise ValueError("site groups: the hit list must be motif-major with motif indices in [0, %d), ascend strictly inside a "
                         "motif, and every window of width %d must lie inside one record of a valid record table" % (int(n_motifs), int(m)))
    return first, rec, mot


def site_order_lib(pos, motif, n_motifs):
    """the stable permutation that makes a (position, motif)-ordered hit list motif-major (pfmscan_site_order_lib) -> int64 [n]"""
    L = load()
    pos = np.ascontiguousarray(pos, dtype=np.int64)
    motif = np.ascontiguousarray(motif, dtype=np.int32)
    if pos.ndim != 1 or pos.shape != motif.shape:
        raise ValueError("positions and motifs must be one-dimensional and of the same size")
    order = np.zeros(pos.size, dtype=np.int64)
    if L.pfmscan_site_order_lib(_ptr(pos), _ptr(motif), pos.size, int(n_motifs), _ptr(order)) != 0:
        raise ValueError("site order: a motif index lies outside [0, %d)" % int(n_motifs))
    return order


def site_acc_from_doubles(values):
    """RAW long accumulator uint64 [SITE_LIMBS] of one cell: the exact sum of finite values >= 0 (pfmscan_site_acc_from_doubles)"""
    L = load()
    values = np.ascontiguousarray(values, dtype=np.float64).ravel()
    acc = np.zeros(SITE_LIMBS, dtype=np.uint64)
    if L.pfmscan_site_acc_from_doubles(_ptr(values), values.size, _ptr(acc)) != 0:
        raise ValueError("site accumulator: every value must be finite and at least 0")
    return acc


def site_acc_add(dst, src):
    """dst (normalised, uint64 [..][SITE_LIMBS][n], C-contiguous, changed in place) += src (raw or normalised, same shape);
    dst is normalised again (pfmscan_site_acc_add).  Returns dst."""
    L = load()
    src = np.ascontiguousarray(src, dtype=np.uint64)
    if not (isinstance(dst, np.ndarray) and dst.dtype == np.uint64 and dst.flags.c_contiguous and dst.flags.writeable):
        raise ValueError("dst must be a writable C-contiguous uint64 array")
    if dst.shape != src.shape or dst.ndim < 2 or dst.shape[-2] != SITE_LIMBS:
        raise ValueError("accumulators are uint64 [..][%d][n] of the same shape" % SITE_LIMBS)
    n_acc = int(np.prod(dst.shape[:-2], dtype=np.int64))
    rc = L.pfmscan_site_acc_add(_ptr(dst), _ptr(src), n_acc, dst.shape[-1])
    if rc != 0:
        raise OverflowError("site accumulator: the top limb overflows")
    return dst


def site_acc_round(acc):
    """uint64 [..][SITE_LIMBS][n] (raw or normalised) -> float64 [..][n]: A * 2^-1074 to the nearest double, ties to even,
    +inf beyond DBL_MAX (pfmscan_site_acc_round)"""
    L = load()
    acc = np.ascontiguousarray(acc, dtype=np.uint64)
    if acc.ndim < 2 or acc.shape[-2] != SITE_LIMBS:
        raise ValueError("accumulators are uint64 [..][%d][n]" % SITE_LIMBS)
    out = np.zeros(acc.shape[:-2] + acc.shape[-1:], dtype=np.float64)
    if L.pfmscan_site_acc_round(_ptr(acc), int(np.prod(acc.shape[:-2], dtype=np.int64)), acc.shape[-1], _ptr(out)) != 0:
        raise ValueError("site accumulator: bad shape")
    return out


def fasta_index(buf, threads=0):
    """uint8 array of FASTA bytes -> (hdr_off, hdr_len, seq_off, seq_end, n_letters), int64 [n_records] each."""
    L = load()
    buf = np.asarray(buf)
    n = ctypes.c_int64(0)
    cap = max(1024, buf.size // 64)            # untouched pages of an over-sized np.empty cost nothing
    while True:
        cols = [np.empty(cap, dtype=np.int64) for _ in range(5)]
        rc = L.pfmscan_fasta_index(_ptr(buf), buf.size, cap, *[_ptr(c) for c in cols], ctypes.byref(n), int(threads))
        if rc == E_CAPACITY and n.value > cap:
            cap = n.value                      # a file of very short records: once more with the exact count
            continue
        if rc != OK:
            _raise(L, None, rc)
        return tuple(c[:n.value] for c in cols)


def fasta_lone_cr(buf, threads=0):
    """True when the FASTA bytes hold a carriage return that is not part of \\r\\n (anywhere in the buffer)"""
    L = load()
    buf = np.asarray(buf)
    found = ctypes.c_int(0)
    rc = L.pfmscan_fasta_lone_cr(_ptr(buf), buf.size, ctypes.byref(found), int(threads))
    if rc != OK:
        _raise(L, None, rc)
    return bool(found.value)


def count_bytes(buf, threads=0):
    """int64 [256]: occurrences of every byte value in a uint8 array (numpy.bincount widens 3x10^8 bytes to int64 first: 10 s)"""
    L = load()
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    counts = np.zeros(256, dtype=np.int64)
    rc = L.pfmscan_count_bytes(_ptr(buf), buf.size, _ptr(counts), int(threads))
    if rc != OK:
        _raise(L, None, rc)
    return counts


def fasta_ids(buf, hdr_off, hdr_len):
    """(id spans int64 [n][2] = (offset, length) of every record's first header word, all headers ASCII?)"""
    L = load()
    n = int(hdr_off.size)
    off, ln = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int64)
    ascii_ = ctypes.c_int(1)
    rc = L.pfmscan_fasta_ids(_ptr(np.asarray(buf)), _ptr(hdr_off), _ptr(hdr_len), n, _ptr(off), _ptr(ln), ctypes.byref(ascii_))
    if rc != OK:
        _raise(L, None, rc)
    return np.stack([off, ln], axis=1), bool(ascii_.value)


def fragment_ids(buf, id_spans):
    """id spans (int64 [n][2], pfmscan_fasta_ids) of ids named <key>_frag_<start> -> (key lengths int64 [n], starts int64 [n]);
    ValueError with ``.index`` = the first id that does not parse"""
    L = load()
    spans = np.ascontiguousarray(id_spans, dtype=np.int64).reshape(-1, 2)
    n = int(spans.shape[0])
    off, ln = np.ascontiguousarray(spans[:, 0]), np.ascontiguousarray(spans[:, 1])
    key_len, start = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int64)
    bad = ctypes.c_int64(-1)
    rc = L.pfmscan_fragment_ids(_ptr(np.asarray(buf)), _ptr(off), _ptr(ln), n, _ptr(key_len), _ptr(start), ctypes.byref(bad))
    if rc != OK:
        err = ValueError(L.pfmscan_last_error(None).decode("utf-8", "replace"))
        err.index = int(bad.value)
        raise err
    return key_len, start


def gather_spans(buf, spans, separator=10):
    """bytes of the (offset, length) spans of buf, each followed by the separator byte, as one bytes object"""
    L = load()
    spans = np.ascontiguousarray(spans, dtype=np.int64)
    n = int(spans.shape[0])
    cap = int(spans[:, 1].sum()) + n if n else 0
    out = np.empty(max(cap, 1), dtype=np.uint8)
    got = ctypes.c_int64(0)
    rc = L.pfmscan_gather_spans(_ptr(np.asarray(buf)), _ptr(spans), n, int(separator), _ptr(out), cap, ctypes.byref(got))
    if rc != OK:
        _raise(L, None, rc)
    return out[:got.value].tobytes()


def fasta_encode(buf, seq_off, seq_end, n_letters, lo, hi, lut, separator=SEP, threads=0):
    """records [lo, hi) of an indexed FASTA buffer -> (codes uint8 [sum(L + 1)], offsets int64 [hi - lo])."""
    L = load()
    total = int(n_letters[lo:hi].sum()) + (hi - lo)
    codes = np.empty(total, dtype=np.uint8)
    offsets = np.empty(hi - lo, dtype=np.int64)
    lut = np.ascontiguousarray(lut, dtype=np.uint8)
    if lut.size != 256:
        raise ValueError("lut must have 256 entries")
    if hi > lo:
        rc = L.pfmscan_fasta_encode(_ptr(buf), _ptr(seq_off), _ptr(seq_end), _ptr(n_letters), lo, hi, _ptr(lut), int(separator),
                                    _ptr(codes), _ptr(offsets), int(threads))
        if rc != OK:
            _raise(L, None, rc)
    return codes, offsets


def profile_parse(data, n_cols):
    """bytes of an averaged-structure profile file -> float64 [n_rows][n_cols] (first column dropped, header skipped), the
    numbers converted exactly as pandas' read_table converts them; None when the file is one for pandas to judge"""
    L = load()
    cap = data.count(b"\n") + 1
    out = np.empty((cap, n_cols), dtype=np.float64)
    k = ctypes.c_int64(0)
    rc = L.pfmscan_profile_parse(data, len(data), int(n_cols), cap, _ptr(out), ctypes.byref(k))
    if rc == E_BADSHAPE:
        return None
    if rc != OK:
        _raise(L, None, rc)
    return out[:k.value]


def round_decimals(values, decimals=3, threads=0):
    """``[round(float(x), decimals) for x in values]`` as a float64 array: Python's float rounding (the nearest decimal
    of the EXACT binary value, ties to even -- rnascan.py:273 applies it to every reported score), natively and in
    parallel.  numpy.round is a different function (scale, rint, unscale) and differs from it near ties."""
    L = load()
    a = np.ascontiguousarray(values, dtype=np.float64)
    out = np.empty_like(a)
    rc = L.pfmscan_round_decimals(_ptr(a), a.size, int(decimals), _ptr(out), int(threads))
    if rc != OK:
        _raise(L, None, rc)
    return out


def debug_round3d(values):
    """Host-only diagnostic: ``round(float(x), 3)`` for every x as the joint-threshold kernels compute it (round3d of
    csrc/pfmscan_exact.hpp: no strings) -> float64 array"""
    L = load()
    a = np.ascontiguousarray(values, dtype=np.float64)
    out = np.empty_like(a)
    if L.pfmscan_debug_round3d(_ptr(a), a.size, _ptr(out)) != OK:
        raise ValueError("pfmscan_debug_round3d: bad argument")
    return out


def library_letters_sum_thresholds(seq_tables, struct_tables, thr_seq, thr_sum):
    """Host-only (no device needed): the letters thresholds the two-FASTA library kernel's prefilter is built for under joint
    thresholds ``thr_sum`` -> float64 [n]; -inf where the route is closed for that pair.  seq_tables / struct_tables [n][m][8],
    thr_seq / thr_sum scalars or [n]"""
    L = load()
    T = np.ascontiguousarray(seq_tables, dtype=np.float64)
    S = np.ascontiguousarray(struct_tables, dtype=np.float64)
    if T.ndim != 3 or T.shape[2] != NCODE or T.shape != S.shape:
        raise ValueError("both table arrays must be [n][m][8]")
    n = T.shape[0]
    ts = np.ascontiguousarray(np.broadcast_to(np.asarray(thr_seq, dtype=np.float64), (n,)))
    tj = np.ascontiguousarray(np.broadcast_to(np.asarray(thr_sum, dtype=np.float64), (n,)))
    out = np.empty(n, dtype=np.float64)
    if L.pfmscan_library_letters_sum_thresholds(_ptr(T), _ptr(S), n, T.shape[1], _ptr(ts), _ptr(tj), _ptr(out)) != OK:
        raise ValueError("pfmscan_library_letters_sum_thresholds: bad argument")
    return out


def debug_pair_credits(letters_seq, letters_struct, thr_sum):
    """Host-only diagnostic: the joint credit tables of k_pair_cred_sum for one pair ([m][8] tables, m <= 32) at thr_sum
    -> dict(seq uint16 [m][8], struct uint16 [m][8], quantum, slack, thr_joint, survive, mode)"""
    L = load()
    A = np.ascontiguousarray(letters_seq, dtype=np.float64)
    B = np.ascontiguousarray(letters_struct, dtype=np.float64)
    if A.ndim != 2 or A.shape[1] != NCODE or A.shape != B.shape:
        raise ValueError("both letter tables must be [m][8]")
    c1, c2 = np.zeros(A.shape, dtype=np.uint16), np.zeros(A.shape, dtype=np.uint16)
    q, sl, tj, sv = (ctypes.c_double(0.0) for _ in range(4))
    mode = ctypes.c_int32(0)
    rc = L.pfmscan_debug_pair_credits(_ptr(A), _ptr(B), A.shape[0], float(thr_sum), _ptr(c1), _ptr(c2), ctypes.byref(q), ctypes.byref(sl),
                                      ctypes.byref(tj), ctypes.byref(sv), ctypes.byref(mode))
    if rc != OK:
        raise ValueError("pfmscan_debug_pair_credits: bad argument")
    return {"seq": c1, "struct": c2, "quantum": q.value, "slack": sl.value, "thr_joint": tj.value, "survive": sv.value, "mode": mode.value}


def debug_pair_sum_test(seq, st, thr_sum):
    """Host-only diagnostic: the joint decision of pfmscan_hits_pair_sum_* for windows with float32 sequence scores ``seq``
    and fp64 structure scores ``st`` that passed both single thresholds -> (maybe bool[n]: the cheap superset test,
    passes bool[n]: the exact predicate behind it, margin0)"""
    L = load()
    f = np.ascontiguousarray(seq, dtype=np.float32)
    s = np.ascontiguousarray(st, dtype=np.float64)
    if f.shape != s.shape:
        raise ValueError("seq and st must have the same shape")
    maybe, passes = np.zeros(f.size, dtype=np.uint8), np.zeros(f.size, dtype=np.uint8)
    m0 = ctypes.c_double(0.0)
    if L.pfmscan_debug_pair_sum_test(_ptr(f), _ptr(s), f.size, float(thr_sum), _ptr(maybe), _ptr(passes), ctypes.byref(m0)) != OK:
        raise ValueError("pfmscan_debug_pair_sum_test: bad argument")
    return maybe.astype(bool).reshape(f.shape), passes.astype(bool).reshape(f.shape), m0.value


TSV_MAX_PIECES = 16


def tsv_number(block, first_id, in_quotes=0):
    """rows formatted WITHOUT their Match_ID column (bytes) -> (the rows with it, number of rows, quote state at the end of
    the block): "\\t<id>" in front of every line end outside a quoted field, ids counting up from ``first_id``"""
    L = load()
    src = np.frombuffer(block, dtype=np.uint8) if len(block) else np.zeros(1, dtype=np.uint8)
    n = len(block)
    cap = n + 21 * (block.count(b"\n") + 1) + 32
    out = np.empty(cap, dtype=np.uint8)
    n_out, n_rows, q = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int(int(in_quotes))
    rc = L.pfmscan_tsv_number(_ptr(src), n, int(first_id), _ptr(out), cap, ctypes.byref(n_out), ctypes.byref(n_rows), ctypes.byref(q))
    if rc != OK:
        _raise(L, None, rc)
    return out[:n_out.value].tobytes(), int(n_rows.value), int(q.value)


def tsv_format(columns, n_rows, first_match_id=-1, threads=0, estimate=None, scratch=None):
    """columns: list of (kind, data, aux, blob, width) with numpy arrays / bytes.  Returns the rows as a list of
    memoryviews (one per formatting thread) whose concatenation is the table.
    ``scratch``: a one-element list holding a reusable uint8 array (grown here when too small) -- a writer that formats
    chunk after chunk then touches fresh pages only once; the views point into it until the next call."""
    L = load()
    keep, desc = [], (TsvColumn * len(columns))()
    for i, (kind, data, aux, blob, width) in enumerate(columns):
        ptrs = []
        for obj in (data, aux, blob):
            if obj is None:
                ptrs.append(None)
            elif isinstance(obj, (bytes, bytearray)):
                arr = np.frombuffer(obj, dtype=np.uint8) if len(obj) else np.zeros(1, dtype=np.uint8)
                keep.append(arr)
                ptrs.append(arr.ctypes.data)
            else:
                arr = np.ascontiguousarray(obj)
                keep.append(arr)
                ptrs.append(arr.ctypes.data)
        desc[i] = TsvColumn(int(kind), 0, ptrs[0], ptrs[1], ptrs[2], int(width))
    cap = int(estimate) if estimate else max(1 << 16, n_rows * 128)
    need, n_pieces = ctypes.c_int64(0), ctypes.c_int(0)
    pieces = np.zeros(2 * TSV_MAX_PIECES, dtype=np.int64)
    while True:
        if scratch is not None and scratch[0] is not None and scratch[0].size >= cap:
            out = scratch[0]
            cap = out.size
        else:
            out = np.empty(cap, dtype=np.uint8)
            if scratch is not None:
                scratch[0] = out
        rc = L.pfmscan_tsv_format(desc, len(columns), int(n_rows), int(first_match_id), _ptr(out), cap, ctypes.byref(need),
                                  _ptr(pieces), ctypes.byref(n_pieces), int(threads))
        if rc == E_CAPACITY and need.value > cap:
            cap = need.value
            continue
        if rc != OK:
            _raise(L, None, rc)
        view = memoryview(out)
        return [view[int(pieces[2 * k]):int(pieces[2 * k] + pieces[2 * k + 1])] for k in range(n_pieces.value)]


PLACE_PLAIN = 1


class PlacedArray(object):
    """one array of a set of Context.place_alloc: a raw device range that outlives this object (the set is freed by
    Context.place_free(first array) or with the context)"""

    def __init__(self, ctx, ptr, nbytes, first):
        self.ctx, self.ptr, self.nbytes, self.first = ctx, ptr, nbytes, first

    @property
    def __cuda_array_interface__(self):
        return {"shape": (self.nbytes,), "typestr": "|u1", "data": (self.ptr, False), "version": 2}


class Context(object):
    """One device context (one per GPU / per host thread)."""

    def __init__(self, device=0):
        self._L = load()
        h = ctypes.c_void_p()
        rc = self._L.pfmscan_ctx_create(int(device), ctypes.byref(h))
        if rc != OK:
            _raise(self._L, None, rc)
        self._h = h
        self.device = int(device)
        self._staged_n = -1
        self.scratch_gen = 0        # bumped whenever the ctx's device scratch is (re)written

    def close(self):
        if getattr(self, "_h", None):
            self._L.pfmscan_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc, n_hits=None):
        if rc != OK:
            _raise(self._L, self._h, rc, n_hits)

    def device_info(self):
        n_cu, hbm = ctypes.c_int(), ctypes.c_int64()
        name = ctypes.create_string_buffer(128)
        self._check(self._L.pfmscan_device_info(self._h, ctypes.byref(n_cu), ctypes.byref(hbm), name, 128))
        return {"name": name.value.decode(), "n_cu": n_cu.value, "hbm_bytes": hbm.value}

    def synchronize(self):
        self._check(self._L.pfmscan_synchronize(self._h))

    # -- device arrays of one scan, placed together (pfmscan_place_alloc) ------------
    def place_alloc(self, sizes, plain=False):
        """device arrays of ``sizes`` bytes that one scan walks in lock-step, in parts of HBM that do not share DRAM banks
        (include/pfmscan.h: pfmscan_place_alloc); returns a list of PlacedArray (``.ptr``, ``.nbytes``, and
        ``__cuda_array_interface__``: ``torch.as_tensor(a, device=...)`` views it as uint8 without a copy)"""
        n = len(sizes)
        b = (ctypes.c_int64 * n)(*[int(x) for x in sizes])
        out = (ctypes.c_void_p * n)()
        self._check(self._L.pfmscan_place_alloc(self._h, n, b, out, PLACE_PLAIN if plain else 0))
        return [PlacedArray(self, int(out[r]), int(sizes[r]), r == 0) for r in range(n)]

    def place_free(self, first):
        self._check(self._L.pfmscan_place_free(self._h, ctypes.c_void_p(first.ptr if isinstance(first, PlacedArray) else int(first))))

    def place_note(self):
        return (self._L.pfmscan_place_note(self._h) or b"").decode()

    def place_trim(self):
        """give back the memory of the sets pfmscan_place_free keeps for reuse (include/pfmscan.h)"""
        self._check(self._L.pfmscan_place_trim(self._h))

    # -- PSSM operands ----------------------------------------------------------
    def motif(self, letter_table=None, struct_pssm=None):
        return Motif(self, letter_table, struct_pssm)

    # -- _pwm.calculate drop-in -------------------------------------------------
    def pwm_calculate(self, sequence, matrix):
        """``_pwm.calculate(sequence, matrix)`` (_pwm.c:79-121) on the GPU."""
        seq = sequence.encode("ascii") if isinstance(sequence, str) else bytes(sequence)
        M = np.asarray(matrix)
        if M.dtype != np.float64:
            raise ValueError("position-weight matrix should contain floating-point values")
        if M.ndim != 2:
            raise ValueError("position-weight matrix has incorrect rank (%d expected 2)" % M.ndim)
        if M.shape[1] != 4:
            raise ValueError("position-weight matrix should have four columns (%d columns found)" % M.shape[1])
        M = np.ascontiguousarray(M)
        n = len(seq) - M.shape[0] + 1
        if n < 0:
            raise MemoryError("failed to create output data")      # _pwm.c:26-31 on a negative shape
        out = np.empty(n, dtype=np.float32)
        self.scratch_gen += 1
        self._staged_n = -1                 # the C side restages: a following scan_staged must not trust the old length
        self._check(self._L.pfmscan_pwm_calculate(self._h, seq, len(seq), _ptr(M), M.shape[0], _ptr(out)))
        return out

    # -- host-buffer scans ------------------------------------------------------
    def scan_host(self, motif, codes, profile=None, want_seq=True, want_struct=True):
        """All window scores of a packed stream -> (seq float32[n] | None, struct float64[n] | None)."""
        n, codes, profile, dt = _stream_args(motif, codes, profile)
        out_seq = np.empty(n, dtype=np.float32) if (want_seq and motif.has_letters) else None
        out_struct = np.empty(n, dtype=np.float64) if (want_struct and motif.has_struct) else None
        self.scratch_gen += 1
        self._staged_n = -1
        self._upload_mode_for(codes, profile)
        self._check(self._L.pfmscan_scan_host(self._h, motif._h, _ptr(codes), _ptr(profile), dt, n,
                                              _ptr(out_seq), _ptr(out_struct)))
        self._staged_n = n                  # scan_host = stage + scan_staged: the stream stays staged
        return out_seq, out_struct

    def scan_letters_f64_host(self, motif, codes):
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        out = np.empty(codes.size, dtype=np.float64)
        self.scratch_gen += 1
        self._staged_n = -1
        self._check(self._L.pfmscan_scan_letters_f64_host(self._h, motif._h, _ptr(codes), codes.size, _ptr(out)))
        return out

    def hits_sum_host(self, motif, codes, profile, thr_seq, thr_struct, thr_sum, capacity=None):
        """hits_host with the joint threshold ``LogOdds.SeqStruct > thr_sum`` on the printed sum (pfmscan_hits_sum_host)"""
        return self.hits_host(motif, codes, profile, thr_seq, thr_struct, capacity, thr_sum=thr_sum)

    def hits_sum_pipeline_host(self, motif, codes, profile, thr_seq, thr_struct, thr_sum, chunk_positions=0, capacity=None):
        """hits_pipeline_host with the joint threshold on the printed sum (pfmscan_hits_sum_pipeline_host)"""
        return self.hits_pipeline_host(motif, codes, profile, thr_seq, thr_struct, chunk_positions, capacity, thr_sum=thr_sum)

    def hits_sum_staged(self, motif, thr_seq, thr_struct, thr_sum, capacity=None):
        """hits_staged with the joint threshold on the printed sum (pfmscan_hits_sum_staged)"""
        return self.hits_staged(motif, thr_seq, thr_struct, capacity, thr_sum=thr_sum)

    def hits_sum_dev(self, motif, d_codes, d_profile, profile_dtype, n_pos, thr_seq, thr_struct, thr_sum, capacity,
                     d_hit_pos, d_hit_seq, d_hit_struct, d_hit_count, stream=None):
        """hits_dev with the joint threshold on the printed sum: one fused pass, asynchronous on ``stream``"""
        self._check(self._L.pfmscan_hits_sum_dev(self._h, motif._h, _ptr(d_codes), _ptr(d_profile), int(profile_dtype),
                                                 int(n_pos), float(thr_seq), float(thr_struct), float(thr_sum), int(capacity),
                                                 _ptr(d_hit_pos), _ptr(d_hit_seq), _ptr(d_hit_struct), _ptr(d_hit_count),
                                                 _ptr(stream)))

    def hits_host(self, motif, codes, profile=None, thr_seq=-np.inf, thr_struct=-np.inf, capacity=None, thr_sum=None):
        """Thresholded hits sorted by position -> (pos int64[k], seq float32[k], struct float64[k]).
        Grows the buffer and retries when the first guess was too small.  ``thr_sum``: see hits_sum_host."""
        n, codes, profile, dt = _stream_args(motif, codes, profile)
        cap = int(capacity) if capacity is not None else max(1024, n // 64)
        self.scratch_gen += 1
        self._staged_n = -1
        self._upload_mode_for(codes, profile)
        while True:
            pos = np.empty(cap, dtype=np.int64)
            sq = np.empty(cap, dtype=np.float32)
            st = np.empty(cap, dtype=np.float64)
            k = ctypes.c_int64(0)
            if thr_sum is None:
                rc = self._L.pfmscan_hits_host(self._h, motif._h, _ptr(codes), _ptr(profile), dt, n,
                                               float(thr_seq), float(thr_struct), cap,
                                               _ptr(pos), _ptr(sq), _ptr(st), ctypes.byref(k))
            else:
                rc = self._L.pfmscan_hits_sum_host(self._h, motif._h, _ptr(codes), _ptr(profile), dt, n,
                                                   float(thr_seq), float(thr_struct), float(thr_sum), cap,
                                                   _ptr(pos), _ptr(sq), _ptr(st), ctypes.byref(k))
            if rc == E_CAPACITY and capacity is None:
                cap = int(k.value)
                continue
            self._check(rc, k.value)
            k = int(k.value)
            self._staged_n = n              # hits_host = stage + hits_staged: the stream stays staged
            return pos[:k].copy(), (sq[:k].copy() if motif.has_letters else None), (st[:k].copy() if motif.has_struct else None)

    def hits_pipeline_host(self, motif, codes, profile=None, thr_seq=-np.inf, thr_struct=-np.inf, chunk_positions=0,
                           capacity=None, thr_sum=None):
        """hits_host for streams of any length (numpy arrays or memory maps): chunked, the upload of the next chunk
        overlaps the scan of the current one, device scratch = two chunks.  Same return values as hits_host."""
        n, codes, profile, dt = _stream_args(motif, codes, profile)
        cap = int(capacity) if capacity is not None else max(1024, n // 64)
        self.scratch_gen += 1
        self._staged_n = -1
        self._upload_mode_for(codes, profile)
        while True:
            pos = np.empty(cap, dtype=np.int64)
            sq = np.empty(cap, dtype=np.float32)
            st = np.empty(cap, dtype=np.float64)
            k = ctypes.c_int64(0)
            if thr_sum is None:
                rc = self._L.pfmscan_hits_pipeline_host(self._h, motif._h, _ptr(codes), _ptr(profile), dt, n, int(chunk_positions),
                                                        float(thr_seq), float(thr_struct), cap, _ptr(pos), _ptr(sq), _ptr(st),
                                                        ctypes.byref(k))
            else:
                rc = self._L.pfmscan_hits_sum_pipeline_host(self._h, motif._h, _ptr(codes), _ptr(profile), dt, n, int(chunk_positions),
                                                            float(thr_seq), float(thr_struct), float(thr_sum), cap, _ptr(pos),
                                                            _ptr(sq), _ptr(st), ctypes.byref(k))
            if rc == E_CAPACITY and capacity is None:
                cap = int(k.value)
                continue
            self._check(rc, k.value)
            k = int(k.value)
            return pos[:k].copy(), (sq[:k].copy() if motif.has_letters else None), (st[:k].copy() if motif.has_struct else None)

    def _upload_mode_for(self, *arrays):
        """staged uploads (parallel copy into pinned buffers) for sources that are file mappings -- a packed profile
        store -- and the runtime's in-place pinning for ordinary memory (include/pfmscan.h, pfmscan_set_upload_mode)"""
        mode = 1 if any(is_file_mapping(a) for a in arrays) else 0
        if mode != getattr(self, "_upload_mode", 0):
            self._check(self._L.pfmscan_set_upload_mode(self._h, mode))
            self._upload_mode = mode
        if mode:
            for a in arrays:
                self._register_mapping(root_memmap(a))

    def _register_mapping(self, mm):
        """tell the uploader which file a read-only numpy.memmap maps (pfmscan_upload_source_file): staged transfers then
        pread the file and never touch the mapping (no page faults, nothing to unmap page by page at exit).  The range is
        forgotten again just before the memmap goes away."""
        import weakref
        if mm is None or getattr(mm, "mode", None) != "r" or mm.nbytes == 0:      # "c": private changes are not in the file
            return
        known = self.__dict__.setdefault("_mappings", {})
        base = mm.ctypes.data
        if base in known:
            return
        # which file was mapped: recorded by whoever opened the memmap (store.ProfileStore), else taken now -- the checked
        # form refuses a path that has come to name another file since (a re-packed store), uploads then read the mapping
        ident = getattr(mm, "_mapped_file_id", None)
        if ident is None:
            try:
                st = os.stat(mm.filename)
                ident = (st.st_dev, st.st_ino, st.st_size)
            except OSError:
                return
        rc = self._L.pfmscan_upload_source_file_checked(self._h, ctypes.c_void_p(base), mm.nbytes, os.fsencode(str(mm.filename)),
                                                        int(mm.offset), int(ident[0]), int(ident[1]), int(ident[2]))
        if rc:
            return                                      # not fatal: the mapping itself is still a valid source
        ctx_ref = weakref.ref(self)

        def forget(base=base):
            ctx = ctx_ref()
            if ctx is not None and getattr(ctx, "_h", None):
                ctx._L.pfmscan_upload_source_file(ctx._h, ctypes.c_void_p(base), 0, None, 0)
                ctx.__dict__.get("_mappings", {}).pop(base, None)
        known[base] = weakref.finalize(mm, forget)

    # -- staged stream: upload once, run many motifs ------------------------------------
    def stage(self, codes=None, profile=None):
        """copy a packed stream into the ctx's device scratch; returns n_pos"""
        n = None
        dt = PROFILE_NONE
        if codes is not None:
            codes = np.ascontiguousarray(codes, dtype=np.uint8)
            n = codes.size
        if profile is not None:
            if profile.dtype == np.float32:
                dt = PROFILE_F32
            elif profile.dtype == np.float64:
                dt = PROFILE_F64
            else:
                raise ValueError("profile must be float32 or float64")
            profile = np.ascontiguousarray(profile)
            if profile.ndim != 2 or profile.shape[1] != NSTRUCT:
                raise ValueError("profile must be [n_pos][7]")
            if n is not None and profile.shape[0] != n:
                raise ValueError("codes and profile disagree on n_pos")
            n = profile.shape[0]
        if n is None:
            raise ValueError("nothing to stage")
        self.scratch_gen += 1
        self._upload_mode_for(codes, profile)
        self._check(self._L.pfmscan_stage(self._h, _ptr(codes), _ptr(profile), dt, n))
        self._staged_n = n
        return self.scratch_gen

    def scan_staged(self, motif, want_seq=True, want_struct=True):
        n = int(self._L.pfmscan_staged_positions(self._h))      # the library's own count sizes the outputs, not a Python copy of it
        if n < 0:
            raise ValueError("no stream staged (call stage first)")
        out_seq = np.empty(n, dtype=np.float32) if (want_seq and motif.has_letters) else None
        out_struct = np.empty(n, dtype=np.float64) if (want_struct and motif.has_struct) else None
        self._check(self._L.pfmscan_scan_staged(self._h, motif._h, _ptr(out_seq), _ptr(out_struct)))
        return out_seq, out_struct

    def hits_staged(self, motif, thr_seq=-np.inf, thr_struct=-np.inf, capacity=None, thr_sum=None):
        n = int(self._L.pfmscan_staged_positions(self._h))
        if n < 0:
            raise ValueError("no stream staged (call stage first)")
        cap = int(capacity) if capacity is not None else max(1024, n // 64)
        while True:
            pos = np.empty(cap, dtype=np.int64)
            sq = np.empty(cap, dtype=np.float32)
            st = np.empty(cap, dtype=np.float64)
            k = ctypes.c_int64(0)
            if thr_sum is None:
                rc = self._L.pfmscan_hits_staged(self._h, motif._h, float(thr_seq), float(thr_struct), cap,
                                                 _ptr(pos), _ptr(sq), _ptr(st), ctypes.byref(k))
            else:
                rc = self._L.pfmscan_hits_sum_staged(self._h, motif._h, float(thr_seq), float(thr_struct), float(thr_sum), cap,
                                                     _ptr(pos), _ptr(sq), _ptr(st), ctypes.byref(k))
            if rc == E_CAPACITY and capacity is None:
                cap = int(k.value)
                continue
            self._check(rc, k.value)
            k = int(k.value)
            return pos[:k].copy(), (sq[:k].copy() if motif.has_letters else None), (st[:k].copy() if motif.has_struct else None)

    # -- dot-bracket structures -> structure-context letters ---------------------------------------------------
    def _dotbracket_check(self, rc, bad):
        """a rejected stream raises ValueError whose ``position`` attribute is the first bad stream position"""
        if rc in (E_BADARG, E_BADSHAPE) and bad.value >= 0:
            err = ValueError(self._L.pfmscan_last_error(self._h).decode("utf-8", "replace"))
            err.position = int(bad.value)
            raise err
        self._check(rc)

    @staticmethod
    def _dotbracket_map(letter_map):
        m = np.ascontiguousarray(np.arange(7) if letter_map is None else letter_map, dtype=np.uint8)
        if m.shape != (7,):
            raise ValueError("the letter map has 7 entries (the codes of E, H, T, B, L, R, M)")
        return m

    def dotbracket_annotate_host(self, codes, letter_map=None, want_counts=True):
        """dot-bracket codes (dotbracket.LUT) -> structure-letter codes of the same layout, and int64 [7] letter counts
        (or None).  ValueError naming the first invalid stream position (``.position``) on a rejected stream."""
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        out = np.empty_like(codes)
        counts = np.zeros(7, dtype=np.int64) if want_counts else None
        bad = ctypes.c_int64(-1)
        rc = self._L.pfmscan_dotbracket_annotate_host(self._h, _ptr(codes), _ptr(out), codes.size,
                                                      _ptr(self._dotbracket_map(letter_map)), _ptr(counts), ctypes.byref(bad))
        self._dotbracket_check(rc, bad)
        return out, counts

    def dotbracket_stage(self, codes, which=0, letter_map=None):
        """upload dot-bracket codes and leave the annotated stream staged (which = 0: the codes slot, 1: the second code
        stream); returns the int64 [7] letter counts"""
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        counts = np.zeros(7, dtype=np.int64)
        bad = ctypes.c_int64(-1)
        if which == 0:
            self.scratch_gen += 1
            self._staged_n = -1
        rc = self._L.pfmscan_dotbracket_stage(self._h, _ptr(codes), codes.size, int(which),
                                              _ptr(self._dotbracket_map(letter_map)), _ptr(counts), ctypes.byref(bad))
        self._dotbracket_check(rc, bad)
        if which == 0:
            self._staged_n = codes.size
        return counts

    def dotbracket_annotate_dev(self, d_in, d_out, n_pos, letter_map=None, d_counts=None, stream=None):
        """device buffers (raw addresses or objects with data_ptr()); asynchronous on `stream` except for the verdict"""
        bad = ctypes.c_int64(-1)
        addr = lambda a: None if a is None else (a.data_ptr() if hasattr(a, "data_ptr") else a)   # noqa: E731
        rc = self._L.pfmscan_dotbracket_annotate_dev(self._h, _ptr(addr(d_in)), _ptr(addr(d_out)), int(n_pos),
                                                     _ptr(self._dotbracket_map(letter_map)), _ptr(addr(d_counts)),
                                                     ctypes.byref(bad), _ptr(stream))
        self._dotbracket_check(rc, bad)

    # -- fragment structures -> averaged-structure profile rows ------------------------------------------------
    def _average_check(self, rc, bad, kind):
        """a rejected averaging raises ValueError with ``kind`` (AVG_*) and ``position`` (row, stream position or record)"""
        if rc in (E_BADARG, E_BADSHAPE) and kind.value != AVG_OK:
            err = ValueError(self._L.pfmscan_last_error(self._h).decode("utf-8", "replace"))
            err.kind, err.position = int(kind.value), int(bad.value)
            raise err
        self._check(rc)

    @staticmethod
    def _average_args(codes, frag_off, frag_len, frag_row, rec_row, rec_len, rec_frag, table, n_max):
        arrs = [np.ascontiguousarray(codes, dtype=np.uint8)] + \
               [np.ascontiguousarray(a, dtype=np.int64) for a in (frag_off, frag_len, frag_row, rec_row, rec_len, rec_frag)]
        table = np.ascontiguousarray(table, dtype=np.float64)
        if table.size < (n_max + 1) * (n_max + 2) // 2:
            raise ValueError("the table needs (n_max + 1)(n_max + 2) / 2 entries")
        if arrs[6].size != arrs[4].size + 1:
            raise ValueError("rec_frag needs n_rec + 1 entries")
        return arrs, table

    def average_host(self, codes, frag_off, frag_len, frag_row, rec_row, rec_len, rec_frag, table, n_max, dtype=np.float64):
        """dot-bracket codes of the fragments (dotbracket.LUT, stream layout) + the fragment and record tables ->
        profile rows [n_rows][7] (B E H L M R T, a zero row after each record) in ``dtype``; see include/pfmscan.h"""
        (c, fo, fl, fr, rr, rl, rf), table = self._average_args(codes, frag_off, frag_len, frag_row, rec_row, rec_len, rec_frag,
                                                                table, n_max)
        dtype = np.dtype(dtype)
        n_rows = int(rl.sum()) + rl.size
        out = np.empty((n_rows, NSTRUCT), dtype=dtype)
        bad, kind = ctypes.c_int64(-1), ctypes.c_int32(0)
        rc = self._L.pfmscan_average_host(self._h, _ptr(c), c.size, _ptr(fo), _ptr(fl), _ptr(fr), fo.size, _ptr(rr), _ptr(rl),
                                          _ptr(rf), rl.size, _ptr(table), int(n_max), _ptr(out),
                                          PROFILE_F32 if dtype == np.float32 else PROFILE_F64, ctypes.byref(bad), ctypes.byref(kind))
        self._average_check(rc, bad, kind)
        return out

    def average_stage(self, codes, frag_off, frag_len, frag_row, rec_row, rec_len, rec_frag, table, n_max, dtype=np.float64):
        """average_host's rows left staged in the profile slot (structure motifs then scan them with *_staged); returns n_rows"""
        (c, fo, fl, fr, rr, rl, rf), table = self._average_args(codes, frag_off, frag_len, frag_row, rec_row, rec_len, rec_frag,
                                                                table, n_max)
        n_rows, bad, kind = ctypes.c_int64(0), ctypes.c_int64(-1), ctypes.c_int32(0)
        self.scratch_gen += 1
        self._staged_n = -1
        rc = self._L.pfmscan_average_stage(self._h, _ptr(c), c.size, _ptr(fo), _ptr(fl), _ptr(fr), fo.size, _ptr(rr), _ptr(rl),
                                           _ptr(rf), rl.size, _ptr(table), int(n_max),
                                           PROFILE_F32 if np.dtype(dtype) == np.float32 else PROFILE_F64,
                                           ctypes.byref(n_rows), ctypes.byref(bad), ctypes.byref(kind))
        self._average_check(rc, bad, kind)
        self._staged_n = int(n_rows.value)
        return self._staged_n

    def average_dev(self, d_letters, n_letters, d_frag_off, d_frag_len, d_frag_row, n_frag, max_len, d_rec_row, d_rec_len,
                    d_rec_frag, n_rec, n_rows, d_table, n_max, d_out, dtype=np.float64, stream=None):
        """device buffers (raw addresses or objects with data_ptr()); asynchronous on `stream` except for the verdict"""
        addr = lambda a: None if a is None else (a.data_ptr() if hasattr(a, "data_ptr") else a)   # noqa: E731
        bad, kind = ctypes.c_int64(-1), ctypes.c_int32(0)
        rc = self._L.pfmscan_average_dev(self._h, _ptr(addr(d_letters)), int(n_letters), _ptr(addr(d_frag_off)),
                                         _ptr(addr(d_frag_len)), _ptr(addr(d_frag_row)), int(n_frag), int(max_len),
                                         _ptr(addr(d_rec_row)), _ptr(addr(d_rec_len)), _ptr(addr(d_rec_frag)), int(n_rec),
                                         int(n_rows), _ptr(addr(d_table)), int(n_max), _ptr(addr(d_out)),
                                         PROFILE_F32 if np.dtype(dtype) == np.float32 else PROFILE_F64,
                                         ctypes.byref(bad), ctypes.byref(kind), _ptr(stream))
        self._average_check(rc, bad, kind)

    # -- averaged-structure profiles -> per-record column sums -------------------------------------------------
    def _colsums_check(self, rc, bad):
        """a rejected cell raises ValueError whose ``element`` attribute is its flat index row * 7 + column"""
        if rc == E_BADARG and bad.value >= 0:
            err = ValueError(self._L.pfmscan_last_error(self._h).decode("utf-8", "replace"))
            err.element = int(bad.value)
            raise err
        self._check(rc)

    @staticmethod
    def _colsums_tables(offsets, lengths):
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        ln = np.ascontiguousarray(lengths, dtype=np.int64)
        if off.ndim != 1 or off.shape != ln.shape:
            raise ValueError("offsets and lengths must be one-dimensional and of the same size")
        return off, ln

    def profile_colsums_host(self, profile, offsets, lengths):
        """per-record column sums, float64 [n_rec][7], of a packed host profile (numpy array or memory map) of any
        length; see include/pfmscan.h.  ValueError (``.element``) when a record holds a NaN, infinite or negative cell"""
        off, ln = self._colsums_tables(offsets, lengths)
        if profile.dtype not in (np.float32, np.float64) or profile.ndim != 2 or profile.shape[1] != NSTRUCT:
            raise ValueError("profile must be float32 or float64 [n_pos][7]")
        profile = np.ascontiguousarray(profile)
        sums = np.zeros((off.size, NSTRUCT), dtype=np.float64)
        bad = ctypes.c_int64(-1)
        self._upload_mode_for(profile)
        rc = self._L.pfmscan_profile_colsums_host(self._h, _ptr(profile), PROFILE_F32 if profile.dtype == np.float32 else PROFILE_F64,
                                                  profile.shape[0], _ptr(off), _ptr(ln), off.size, _ptr(sums), ctypes.byref(bad))
        self._colsums_check(rc, bad)
        return sums

    def profile_colsums_staged(self, offsets, lengths):
        """the same for the profile that stage() / average_stage() left on the device"""
        off, ln = self._colsums_tables(offsets, lengths)
        sums = np.zeros((off.size, NSTRUCT), dtype=np.float64)
        bad = ctypes.c_int64(-1)
        rc = self._L.pfmscan_profile_colsums_staged(self._h, _ptr(off), _ptr(ln), off.size, _ptr(sums), ctypes.byref(bad))
        self._colsums_check(rc, bad)
        return sums

    def profile_colsums_dev(self, d_profile, dtype, n_pos, d_offsets, d_lengths, n_rec, d_sums, stream=None):
        """device buffers (raw addresses or objects with data_ptr()); asynchronous on `stream` except for the verdict"""
        addr = lambda a: None if a is None else (a.data_ptr() if hasattr(a, "data_ptr") else a)   # noqa: E731
        bad = ctypes.c_int64(-1)
        rc = self._L.pfmscan_profile_colsums_dev(self._h, _ptr(addr(d_profile)),
                                                 PROFILE_F32 if np.dtype(dtype) == np.float32 else PROFILE_F64, int(n_pos),
                                                 _ptr(addr(d_offsets)), _ptr(addr(d_lengths)), int(n_rec), _ptr(addr(d_sums)),
                                                 ctypes.byref(bad), _ptr(stream))
        self._colsums_check(rc, bad)

    # -- site profiles: rows and letters summed under hit windows (include/pfmscan.h) ---------------------------
    site_groups = staticmethod(site_groups)

    def _site_call(self, fn, pos, offsets, lengths, m, flank, want_counts, want_sums):
        """the capacity protocol of the _staged / _host forms: fn(pos, off, ln, capacity, grp_rec, sums, counts, n, bad) -> rc"""
        pos = np.ascontiguousarray(pos, dtype=np.int64)
        off, ln = self._colsums_tables(offsets, lengths)
        W = int(m) + 2 * int(flank)
        cap = max(1, min(pos.size, off.size + pos.size // SITE_GROUP))
        while True:
            grp_rec = np.zeros(cap, dtype=np.int64)
            sums = np.zeros((cap, W, NSTRUCT), dtype=np.float64) if want_sums else None
            counts = np.zeros((cap, W, NCODE), dtype=np.uint32) if want_counts else None
            n, bad = ctypes.c_int64(0), ctypes.c_int64(-1)
            rc = fn(pos, off, ln, cap, grp_rec, sums, counts, n, bad)
            if rc == E_CAPACITY and n.value > cap:
                cap = int(n.value)
                continue
            self._colsums_check(rc, bad)
            k = int(n.value)
            return grp_rec[:k], (None if sums is None else sums[:k]), (None if counts is None else counts[:k])

    def site_sums_staged(self, pos, offsets, lengths, m, flank=0, letters=True, profile=True):
        """group sums / counts under the hits ``pos`` of the staged stream -> (grp_rec, sums float64 [n_grp][W][7] | None,
        counts uint32 [n_grp][W][8] | None).  ValueError (``.element``) for a NaN, infinite or negative cell under a hit"""
        def fn(pos, off, ln, cap, grp_rec, sums, counts, n, bad):
            return self._L.pfmscan_site_sums_staged(self._h, int(bool(letters)), int(bool(profile)), _ptr(pos), pos.size, _ptr(off),
                                                    _ptr(ln), off.size, int(m), int(flank), cap, _ptr(grp_rec), _ptr(sums),
                                                    _ptr(counts), ctypes.byref(n), ctypes.byref(bad))
        return self._site_call(fn, pos, offsets, lengths, m, flank, letters, profile)

    def site_sums_host(self, codes, profile, pos, offsets, lengths, m, flank=0):
        """the same for a packed host stream of any length (numpy arrays or a mapped store); either part may be None"""
        n_pos = None
        dt = PROFILE_NONE
        if codes is not None:
            codes = np.ascontiguousarray(codes, dtype=np.uint8)
            n_pos = codes.size
        if profile is not None:
            if profile.dtype not in (np.float32, np.float64) or profile.ndim != 2 or profile.shape[1] != NSTRUCT:
                raise ValueError("profile must be float32 or float64 [n_pos][7]")
            profile = np.ascontiguousarray(profile)
            dt = PROFILE_F32 if profile.dtype == np.float32 else PROFILE_F64
            if n_pos is not None and n_pos != profile.shape[0]:
                raise ValueError("codes and profile differ in length")
            n_pos = profile.shape[0]
        if n_pos is None:
            raise ValueError("neither codes nor a profile")
        self._upload_mode_for(codes, profile)

        def fn(pos, off, ln, cap, grp_rec, sums, counts, n, bad):
            return self._L.pfmscan_site_sums_host(self._h, _ptr(codes), _ptr(profile), dt, n_pos, _ptr(pos), pos.size, _ptr(off),
                                                  _ptr(ln), off.size, int(m), int(flank), cap, _ptr(grp_rec), _ptr(sums),
                                                  _ptr(counts), ctypes.byref(n), ctypes.byref(bad))
        return self._site_call(fn, pos, offsets, lengths, m, flank, codes is not None, profile is not None)

    def site_sums_dev(self, d_codes, d_profile, dtype, n_pos, d_pos, n_hits, d_grp_first, d_grp_rec, n_grp, d_offsets, d_lengths,
                      n_rec, m, flank, d_sums, d_counts, stream=None):
        """device buffers (raw addresses or objects with data_ptr()); asynchronous on `stream` except for the verdict"""
        addr = lambda a: None if a is None else (a.data_ptr() if hasattr(a, "data_ptr") else a)   # noqa: E731
        bad = ctypes.c_int64(-1)
        rc = self._L.pfmscan_site_sums_dev(self._h, _ptr(addr(d_codes)), _ptr(addr(d_profile)),
                                           PROFILE_F32 if np.dtype(dtype) == np.float32 else PROFILE_F64, int(n_pos),
                                           _ptr(addr(d_pos)), int(n_hits), _ptr(addr(d_grp_first)), _ptr(addr(d_grp_rec)), int(n_grp),
                                           _ptr(addr(d_offsets)), _ptr(addr(d_lengths)), int(n_rec), int(m), int(flank),
                                           _ptr(addr(d_sums)), _ptr(addr(d_counts)), ctypes.byref(bad), _ptr(stream))
        self._colsums_check(rc, bad)

    # -- site profiles of a library: exact per-motif sums (include/pfmscan.h) --------------------------------------
    def site_sums_lib_staged(self, pos, motif, n_motifs, offsets, lengths, m, flank=0, letters=True, profile=True):
        """per-motif long accumulators under the hits (pos, motif) -- as the library scans return them -- of the staged
        stream -> (acc uint64 [n_motifs][SITE_LIMBS][W * 7] normalised | None, counts uint64 [n_motifs][W][8] | None).
        ValueError (``.element``) for a NaN, infinite or negative cell under a hit of any motif"""
        pos = np.ascontiguousarray(pos, dtype=np.int64)
        motif = np.ascontiguousarray(motif, dtype=np.int32)
        if pos.ndim != 1 or pos.shape != motif.shape:
            raise ValueError("positions and motifs must be one-dimensional and of the same size")
        off, ln = self._colsums_tables(offsets, lengths)
        W, n_motifs = int(m) + 2 * int(flank), int(n_motifs)
        if n_motifs < 0 or W < 1 or W > MAX_WIDTH:
            raise ValueError("site sums: a negative number of motifs, or width + 2 x flank outside [1, PFMSCAN_MAX_WIDTH]")
        acc = np.zeros((n_motifs, SITE_LIMBS, W * NSTRUCT), dtype=np.uint64) if profile else None
        counts = np.zeros((n_motifs, W, NCODE), dtype=np.uint64) if letters else None
        bad = ctypes.c_int64(-1)
        rc = self._L.pfmscan_site_sums_lib_staged(self._h, int(bool(letters)), int(bool(profile)), _ptr(pos), _ptr(motif), pos.size,
                                                  _ptr(off), _ptr(ln), off.size, n_motifs, int(m), int(flank), _ptr(acc),
                                                  _ptr(counts), ctypes.byref(bad))
        self._colsums_check(rc, bad)
        return acc, counts

    def site_sums_lib_dev(self, d_codes, d_profile, dtype, n_pos, d_pos, n_hits, d_grp_first, d_grp_rec, d_grp_motif, n_grp,
                          d_offsets, d_lengths, n_rec, n_motifs, m, flank, d_acc, d_counts, stream=None):
        """device buffers (raw addresses or objects with data_ptr()); zeroes d_acc / d_counts and leaves RAW sums there;
        asynchronous on `stream` except for the verdict"""
        addr = lambda a: None if a is None else (a.data_ptr() if hasattr(a, "data_ptr") else a)   # noqa: E731
        bad = ctypes.c_int64(-1)
        rc = self._L.pfmscan_site_sums_lib_dev(self._h, _ptr(addr(d_codes)), _ptr(addr(d_profile)),
                                               PROFILE_F32 if np.dtype(dtype) == np.float32 else PROFILE_F64, int(n_pos),
                                               _ptr(addr(d_pos)), int(n_hits), _ptr(addr(d_grp_first)), _ptr(addr(d_grp_rec)),
                                               _ptr(addr(d_grp_motif)), int(n_grp), _ptr(addr(d_offsets)), _ptr(addr(d_lengths)),
                                               int(n_rec), int(n_motifs), int(m), int(flank), _ptr(addr(d_acc)), _ptr(addr(d_counts)),
                                               ctypes.byref(bad), _ptr(stream))
        self._colsums_check(rc, bad)

    # -- site profiles on letter streams: letter-pair counts under hits (include/pfmscan.h) ---------------------------
    def site_joint_staged(self, pos, motif, n_motifs, offsets, lengths, m, flank=0, first=True, second=True):
        """letter-pair counts under the hits (pos, motif) -- as the library scans return them; motif None: one motif -- of
        the staged code streams -> uint64 [n_motifs][W][8][8]: cell [k][j][a][b] counts the hits of motif k whose column j
        lies inside the hit's record with code a in the staged codes (``first``) and code b in the staged codes2
        (``second``), both taken & 7; a stream that is not used has index 0.  ValueError for a hit outside the stream,
        a window that leaves its record or a motif index that is no motif"""
        pos = np.ascontiguousarray(pos, dtype=np.int64)
        if motif is not None:
            motif = np.ascontiguousarray(motif, dtype=np.int32)
        if pos.ndim != 1 or (motif is not None and pos.shape != motif.shape):
            raise ValueError("positions and motifs must be one-dimensional and of the same size")
        off, ln = self._colsums_tables(offsets, lengths)
        W, n_motifs = int(m) + 2 * int(flank), int(n_motifs)
        if n_motifs < 0 or W < 1 or W > MAX_WIDTH:
            raise ValueError("site joint: a negative number of motifs, or width + 2 x flank outside [1, PFMSCAN_MAX_WIDTH]")
        joint = np.zeros((n_motifs, W, NCODE, NCODE), dtype=np.uint64)
        self._check(self._L.pfmscan_site_joint_staged(self._h, int(bool(first)), int(bool(second)), _ptr(pos), _ptr(motif), pos.size,
                                                      _ptr(off), _ptr(ln), off.size, n_motifs, int(m), int(flank), _ptr(joint)))
        return joint

    def site_joint_dev(self, d_codes, d_codes2, n_pos, d_pos, d_motif, n_hits, d_offsets, d_lengths, n_rec, n_motifs, m, flank,
                       d_joint, stream=None):
        """device buffers (raw addresses or objects with data_ptr(); d_codes, d_codes2 or d_motif may be None): the hit list
        is motif-major; zeroes d_joint uint64 [n_motifs][W][8][8] itself; asynchronous on `stream` except for the verdict"""
        addr = lambda a: None if a is None else (a.data_ptr() if hasattr(a, "data_ptr") else a)   # noqa: E731
        self._check(self._L.pfmscan_site_joint_dev(self._h, _ptr(addr(d_codes)), _ptr(addr(d_codes2)), int(n_pos), _ptr(addr(d_pos)),
                                                   _ptr(addr(d_motif)), int(n_hits), _ptr(addr(d_offsets)), _ptr(addr(d_lengths)),
                                                   int(n_rec), int(n_motifs), int(m), int(flank), _ptr(addr(d_joint)), _ptr(stream)))

    # -- generic-alphabet letter hits in fp64; two code streams ---------------------------------
    def hits_letters_f64_staged(self, motif, thr, capacity=None):
        """hits of a letters-only motif over the staged codes, fp64 compare and score (matrix.py:25-43 + rnascan.py:263)
        -> (pos int64[k] sorted, score float64[k])"""
        n = int(self._L.pfmscan_staged_positions(self._h))
        if n < 0:
            raise ValueError("no stream staged (call stage first)")
        cap = int(capacity) if capacity is not None else max(1024, n // 64)
        while True:
            pos = np.empty(cap, dtype=np.int64)
            sc = np.empty(cap, dtype=np.float64)
            k = ctypes.c_int64(0)
            rc = self._L.pfmscan_hits_letters_f64_staged(self._h, motif._h, float(thr), cap, _ptr(pos), _ptr(sc), ctypes.byref(k))
            if rc == E_CAPACITY and capacity is None:
                cap = int(k.value)
                continue
            self._check(rc, k.value)
            k = int(k.value)
            return pos[:k].copy(), sc[:k].copy()

    def hits_letters_f64_host(self, motif, codes, thr, capacity=None):
        self.stage(codes, None)
        return self.hits_letters_f64_staged(motif, thr, capacity)

    def stage_codes2(self, codes2):
        """a second code stream (the structure letters of the staged records) beside the staged one"""
        codes2 = np.ascontiguousarray(codes2, dtype=np.uint8)
        self._check(self._L.pfmscan_stage_codes2(self._h, _ptr(codes2), codes2.size))

    def hits_pair_staged(self, motif_seq, motif_struct, thr_seq, thr_struct, capacity=None):
        """hits of (sequence letters AND structure letters) over the two staged code streams
        -> (pos int64[k] sorted, seq float32[k], struct float64[k])"""
        n = int(self._L.pfmscan_staged_positions(self._h))
        if n < 0:
            raise ValueError("no stream staged (call stage first)")
        cap = int(capacity) if capacity is not None else max(1024, n // 64)
        while True:
            pos = np.empty(cap, dtype=np.int64)
            sq = np.empty(cap, dtype=np.float32)
            st = np.empty(cap, dtype=np.float64)
            k = ctypes.c_int64(0)
            rc = self._L.pfmscan_hits_pair_staged(self._h, motif_seq._h, motif_struct._h, float(thr_seq), float(thr_struct), cap,
                                                  _ptr(pos), _ptr(sq), _ptr(st), ctypes.byref(k))
            if rc == E_CAPACITY and capacity is None:
                cap = int(k.value)
                continue
            self._check(rc, k.value)
            k = int(k.value)
            return pos[:k].copy(), sq[:k].copy(), st[:k].copy()

    def hits_pair_host(self, motif_seq, motif_struct, codes, codes2, thr_seq, thr_struct, capacity=None):
        self.stage(codes, None)
        self.stage_codes2(codes2)
        return self.hits_pair_staged(motif_seq, motif_struct, thr_seq, thr_struct, capacity)

    def hits_pair_sum_staged(self, motif_seq, motif_struct, thr_seq, thr_struct, thr_sum, capacity=None):
        """hits_pair_staged with the joint threshold on the printed sum: additionally
        float64(np.round(seq, 3)) + round(struct, 3) > thr_sum, decided on the device (rnascan.py:273, :416-434)
        -> (pos int64[k] sorted, seq float32[k], struct float64[k])"""
        n = int(self._L.pfmscan_staged_positions(self._h))
        if n < 0:
            raise ValueError("no stream staged (call stage first)")
        cap = int(capacity) if capacity is not None else max(1024, n // 64)
        while True:
            pos = np.empty(cap, dtype=np.int64)
            sq = np.empty(cap, dtype=np.float32)
            st = np.empty(cap, dtype=np.float64)
            k = ctypes.c_int64(0)
            rc = self._L.pfmscan_hits_pair_sum_staged(self._h, motif_seq._h, motif_struct._h, float(thr_seq), float(thr_struct),
                                                      float(thr_sum), cap, _ptr(pos), _ptr(sq), _ptr(st), ctypes.byref(k))
            if rc == E_CAPACITY and capacity is None:
                cap = int(k.value)
                continue
            self._check(rc, k.value)
            k = int(k.value)
            return pos[:k].copy(), sq[:k].copy(), st[:k].copy()

    def hits_pair_sum_host(self, motif_seq, motif_struct, codes, codes2, thr_seq, thr_struct, thr_sum, capacity=None):
        """one call of pfmscan_hits_pair_sum_host (stages both streams itself)"""
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        codes2 = np.ascontiguousarray(codes2, dtype=np.uint8)
        if codes.size != codes2.size:
            raise ValueError("the two code streams must have the same length")
        cap = int(capacity) if capacity is not None else max(1024, codes.size // 64)
        while True:
            pos = np.empty(cap, dtype=np.int64)
            sq = np.empty(cap, dtype=np.float32)
            st = np.empty(cap, dtype=np.float64)
            k = ctypes.c_int64(0)
            rc = self._L.pfmscan_hits_pair_sum_host(self._h, motif_seq._h, motif_struct._h, _ptr(codes), _ptr(codes2), codes.size,
                                                    float(thr_seq), float(thr_struct), float(thr_sum), cap, _ptr(pos), _ptr(sq),
                                                    _ptr(st), ctypes.byref(k))
            if rc == E_CAPACITY and capacity is None:
                cap = int(k.value)
                continue
            self._check(rc, k.value)
            k = int(k.value)
            return pos[:k].copy(), sq[:k].copy(), st[:k].copy()

    def hits_pair_sum_dev(self, motif_seq, motif_struct, d_codes, d_codes2, n_pos, thr_seq, thr_struct, thr_sum, capacity,
                          d_hit_pos, d_hit_seq, d_hit_struct, d_hit_count, stream=None):
        self._check(self._L.pfmscan_hits_pair_sum_dev(self._h, motif_seq._h, motif_struct._h, _ptr(d_codes), _ptr(d_codes2), int(n_pos),
                                                      float(thr_seq), float(thr_struct), float(thr_sum), int(capacity), _ptr(d_hit_pos),
                                                      _ptr(d_hit_seq), _ptr(d_hit_struct), _ptr(d_hit_count), _ptr(stream)))

    def pair_sum_route(self):
        """PAIR_ROUTE_* of the last hits_pair_sum_* call (NONE: thr_sum was -inf, or a plain hits_pair_* call came after)"""
        return int(self._L.pfmscan_pair_sum_route(self._h))

    def hits_letters_f64_dev(self, motif, d_codes, n_pos, thr, capacity, d_hit_pos, d_hit_score, d_hit_count, stream=None):
        self._check(self._L.pfmscan_hits_letters_f64_dev(self._h, motif._h, _ptr(d_codes), int(n_pos), float(thr), int(capacity),
                                                         _ptr(d_hit_pos), _ptr(d_hit_score), _ptr(d_hit_count), _ptr(stream)))

    def hits_pair_dev(self, motif_seq, motif_struct, d_codes, d_codes2, n_pos, thr_seq, thr_struct, capacity,
                      d_hit_pos, d_hit_seq, d_hit_struct, d_hit_count, stream=None):
        self._check(self._L.pfmscan_hits_pair_dev(self._h, motif_seq._h, motif_struct._h, _ptr(d_codes), _ptr(d_codes2), int(n_pos),
                                                  float(thr_seq), float(thr_struct), int(capacity), _ptr(d_hit_pos), _ptr(d_hit_seq),
                                                  _ptr(d_hit_struct), _ptr(d_hit_count), _ptr(stream)))

    # -- multi-PFM libraries (every motif in one pass) --------------------------------
    def library(self, letter_tables, struct_pssms=None, struct_letters=None):
        return Library(self, letter_tables, struct_pssms, struct_letters)

    def library_hits_letters_dev(self, lib, d_codes, d_codes2, n_pos, thr_seq, thr_struct, capacity,
                                 d_hit_pos, d_hit_motif, d_hit_seq, d_hit_struct, d_hit_count, stream=None):
        """LETTER library on device-resident code streams (d_codes2 None for a structure-letter library): asynchronous on
        ``stream``; hits unordered, *d_hit_count = total (above capacity = incomplete)"""
        ts, tt = lib.thresholds(thr_seq, thr_struct)
        self._check(self._L.pfmscan_library_hits_letters_dev(self._h, lib._h, _ptr(d_codes), _ptr(d_codes2), int(n_pos), _ptr(ts), _ptr(tt),
                                                             int(capacity), _ptr(d_hit_pos), _ptr(d_hit_motif), _ptr(d_hit_seq),
                                                             _ptr(d_hit_struct), _ptr(d_hit_count), _ptr(stream)))

    def library_hits_letters_host(self, lib, codes, codes2=None, thr_seq=None, thr_struct=None, capacity=None):
        """hits of a LETTER library (Library(struct_letters=...)): ``codes`` is the 8-code stream of a structure-letter library,
        or the sequence codes of a two-FASTA library whose structure strings are ``codes2`` -> as library_hits_staged"""
        if not lib.letter_kind:
            raise ValueError("not a letter library")
        self.stage(codes, None)
        if lib.has_letters:
            self.stage_codes2(codes2)
        return self.library_hits_staged(lib, thr_seq, thr_struct, capacity)

    def library_hits_letters_sum_dev(self, lib, d_codes, d_codes2, n_pos, thr_seq, thr_struct, thr_sum, capacity,
                                     d_hit_pos, d_hit_motif, d_hit_seq, d_hit_struct, d_hit_count, stream=None):
        """two-FASTA library with joint thresholds on device-resident code streams: asynchronous on ``stream``; hits unordered"""
        ts, tt = lib.thresholds(thr_seq, thr_struct)
        tj = np.ascontiguousarray(np.broadcast_to(np.asarray(thr_sum, dtype=np.float64), (lib.n,)))
        self._check(self._L.pfmscan_library_hits_letters_sum_dev(self._h, lib._h, _ptr(d_codes), _ptr(d_codes2), int(n_pos), _ptr(ts), _ptr(tt),
                                                                 _ptr(tj), int(capacity), _ptr(d_hit_pos), _ptr(d_hit_motif), _ptr(d_hit_seq),
                                                                 _ptr(d_hit_struct), _ptr(d_hit_count), _ptr(stream)))

    def library_hits_letters_sum_host(self, lib, codes, codes2, thr_seq, thr_struct, thr_sum, capacity=None):
        """hits of a two-FASTA library (Library(letter_tables, struct_letters=...)) with the joint threshold of hits_pair_sum per
        pair (scalar or [n]), decided in the one-pass library kernel -> (pos, motif, seq float32, struct float64) sorted by
        (position, motif index); stages both streams"""
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        codes2 = np.ascontiguousarray(codes2, dtype=np.uint8)
        if codes.size != codes2.size:
            raise ValueError("the two code streams must have the same length")
        ts, tt = lib.thresholds(thr_seq, thr_struct)
        tj = np.ascontiguousarray(np.broadcast_to(np.asarray(thr_sum, dtype=np.float64), (lib.n,)))
        self.scratch_gen += 1
        self._staged_n = -1
        cap = int(capacity) if capacity is not None else max(4096, codes.size // 16)
        while True:
            pos = np.empty(cap, dtype=np.int64)
            mo = np.empty(cap, dtype=np.int32)
            sq = np.empty(cap, dtype=np.float32)
            st = np.empty(cap, dtype=np.float64)
            k = ctypes.c_int64(0)
            rc = self._L.pfmscan_library_hits_letters_sum_host(self._h, lib._h, _ptr(codes), _ptr(codes2), codes.size, _ptr(ts), _ptr(tt), _ptr(tj),
                                                               cap, _ptr(pos), _ptr(mo), _ptr(sq), _ptr(st), ctypes.byref(k))
            if rc == E_CAPACITY and capacity is None:
                cap = int(k.value)
                continue
            self._check(rc, k.value)
            k = int(k.value)
            return pos[:k].copy(), mo[:k].copy(), sq[:k].copy(), st[:k].copy()

    def library_hits_staged(self, lib, thr_seq, thr_struct=None, capacity=None):
        """hits of every motif of ``lib`` over the staged stream, sorted by (position, motif index)
        -> (pos int64[k], motif int32[k], seq float32[k], struct float64[k] | None)"""
        n = int(self._L.pfmscan_staged_positions(self._h))
        if n < 0:
            raise ValueError("no stream staged (call stage first)")
        ts, tt = lib.thresholds(thr_seq, thr_struct)
        cap = int(capacity) if capacity is not None else max(4096, n // 16)
        while True:
            pos = np.empty(cap, dtype=np.int64)
            mo = np.empty(cap, dtype=np.int32)
            sq = np.empty(cap, dtype=np.float32)
            st = np.empty(cap, dtype=np.float64)
            k = ctypes.c_int64(0)
            rc = self._L.pfmscan_library_hits_staged(self._h, lib._h, _ptr(ts), _ptr(tt), cap, _ptr(pos), _ptr(mo),
                                                     _ptr(sq), _ptr(st), ctypes.byref(k))
            if rc == E_CAPACITY and capacity is None:
                cap = int(k.value)
                continue
            self._check(rc, k.value)
            k = int(k.value)
            return pos[:k].copy(), mo[:k].copy(), (sq[:k].copy() if lib.has_letters else None), (st[:k].copy() if lib.has_struct else None)

    def library_hits_host(self, lib, codes, profile=None, thr_seq=None, thr_struct=None, capacity=None):
        self.stage(codes if lib.has_letters else None, profile if lib.has_struct else None)
        return self.library_hits_staged(lib, thr_seq, thr_struct, capacity)

    def library_hits_sum_staged(self, lib, thr_seq, thr_struct, thr_sum, capacity=None):
        """library_hits_staged of a seq + struct library with the joint threshold ``LogOdds.SeqStruct > thr_sum[k]`` on the
        printed sum, decided in the library kernel (pfmscan_library_hits_sum_staged).  thr_seq may be -inf: ValueError when
        a motif's effective letters threshold (``library_sum_thresholds``) is -inf too."""
        n = int(self._L.pfmscan_staged_positions(self._h))
        if n < 0:
            raise ValueError("no stream staged (call stage first)")
        ts, tt = lib.thresholds(thr_seq, thr_struct)
        tj = np.ascontiguousarray(np.broadcast_to(np.asarray(thr_sum, dtype=np.float64), (lib.n,)))
        cap = int(capacity) if capacity is not None else max(4096, n // 16)
        while True:
            pos = np.empty(cap, dtype=np.int64)
            mo = np.empty(cap, dtype=np.int32)
            sq = np.empty(cap, dtype=np.float32)
            st = np.empty(cap, dtype=np.float64)
            k = ctypes.c_int64(0)
            rc = self._L.pfmscan_library_hits_sum_staged(self._h, lib._h, _ptr(ts), _ptr(tt), _ptr(tj), cap, _ptr(pos), _ptr(mo),
                                                         _ptr(sq), _ptr(st), ctypes.byref(k))
            if rc == E_CAPACITY and capacity is None:
                cap = int(k.value)
                continue
            self._check(rc, k.value)
            k = int(k.value)
            return pos[:k].copy(), mo[:k].copy(), sq[:k].copy(), st[:k].copy()

    def library_hits_sum_host(self, lib, codes, profile, thr_seq, thr_struct, thr_sum, capacity=None):
        self.stage(codes, profile)
        return self.library_hits_sum_staged(lib, thr_seq, thr_struct, thr_sum, capacity)

    def library_hits_sum_dev(self, lib, d_codes, d_profile, profile_dtype, n_pos, thr_seq, thr_struct, thr_sum, row_sum_max, capacity,
                             d_hit_pos, d_hit_motif, d_hit_seq, d_hit_struct, d_hit_count, stream=None):
        """asynchronous on ``stream``; ``row_sum_max``: the caller's promise about the profile rows (inf: none), see
        pfmscan_library_hits_sum_dev; hits unordered, *d_hit_count = total (above capacity = incomplete)"""
        ts, tt = lib.thresholds(thr_seq, thr_struct)
        tj = np.ascontiguousarray(np.broadcast_to(np.asarray(thr_sum, dtype=np.float64), (lib.n,)))
        self._check(self._L.pfmscan_library_hits_sum_dev(self._h, lib._h, _ptr(d_codes), _ptr(d_profile), int(profile_dtype),
                                                         int(n_pos), _ptr(ts), _ptr(tt), _ptr(tj), float(row_sum_max), int(capacity),
                                                         _ptr(d_hit_pos), _ptr(d_hit_motif), _ptr(d_hit_seq), _ptr(d_hit_struct),
                                                         _ptr(d_hit_count), _ptr(stream)))

    def profile_row_bound_staged(self):
        """the staged profile's row bound: the largest fp64 row sum over the rows not under code 7, inf when one of them holds
        a NaN, infinite or negative entry (pfmscan_profile_row_bound_staged; cached until the next stage)"""
        v = ctypes.c_double(0.0)
        self._check(self._L.pfmscan_profile_row_bound_staged(self._h, ctypes.byref(v)))
        return v.value

    def profile_row_bound_dev(self, d_codes, d_profile, profile_dtype, n_pos, d_out, stream=None):
        """the same for device arrays: one float64 to ``d_out``, asynchronous on ``stream``"""
        self._check(self._L.pfmscan_profile_row_bound_dev(self._h, _ptr(d_codes), _ptr(d_profile), int(profile_dtype), int(n_pos),
                                                          _ptr(d_out), _ptr(stream)))

    def library_hits_pipeline_host(self, lib, codes, profile=None, thr_seq=None, thr_struct=None, chunk_positions=0, capacity=None):
        """library_hits_host for host streams of any length (numpy arrays or memory maps): chunked, the upload of the next
        chunk overlaps the scan of the current one, device scratch = two chunks; nothing stays staged"""
        codes = None if (codes is None or not lib.has_letters) else np.ascontiguousarray(codes, dtype=np.uint8)
        dt = PROFILE_NONE
        if lib.has_struct:
            if profile is None:
                raise ValueError("library has structure PSSMs: profile required")
            if profile.dtype == np.float32:
                dt = PROFILE_F32
            elif profile.dtype == np.float64:
                dt = PROFILE_F64
            else:
                raise ValueError("profile must be float32 or float64")
            profile = np.ascontiguousarray(profile)
            if profile.ndim != 2 or profile.shape[1] != NSTRUCT:
                raise ValueError("profile must be [n_pos][7]")
        else:
            profile = None
        n = int(codes.size if codes is not None else profile.shape[0])
        if codes is not None and profile is not None and profile.shape[0] != n:
            raise ValueError("codes and profile disagree on n_pos")
        ts, tt = lib.thresholds(thr_seq, thr_struct)
        cap = int(capacity) if capacity is not None else max(4096, n // 16)
        self.scratch_gen += 1
        self._staged_n = -1
        self._upload_mode_for(codes, profile)
        while True:
            pos = np.empty(cap, dtype=np.int64)
            mo = np.empty(cap, dtype=np.int32)
            sq = np.empty(cap, dtype=np.float32)
            st = np.empty(cap, dtype=np.float64)
            k = ctypes.c_int64(0)
            rc = self._L.pfmscan_library_hits_pipeline_host(self._h, lib._h, _ptr(codes), _ptr(profile), dt, n, int(chunk_positions),
                                                            _ptr(ts), _ptr(tt), cap, _ptr(pos), _ptr(mo), _ptr(sq), _ptr(st),
                                                            ctypes.byref(k))
            if rc == E_CAPACITY and capacity is None:
                cap = int(k.value)
                continue
            self._check(rc, k.value)
            k = int(k.value)
            return pos[:k].copy(), mo[:k].copy(), (sq[:k].copy() if lib.has_letters else None), (st[:k].copy() if lib.has_struct else None)

    def library_hits_dev(self, lib, d_codes, d_profile, profile_dtype, n_pos, thr_seq, thr_struct, capacity,
                         d_hit_pos, d_hit_motif, d_hit_seq, d_hit_struct, d_hit_count, stream=None):
        """asynchronous on ``stream``; hits unordered, *d_hit_count = total (above capacity = incomplete)"""
        ts, tt = lib.thresholds(thr_seq, thr_struct)
        self._check(self._L.pfmscan_library_hits_dev(self._h, lib._h, _ptr(d_codes), _ptr(d_profile), int(profile_dtype),
                                                     int(n_pos), _ptr(ts), _ptr(tt), int(capacity), _ptr(d_hit_pos),
                                                     _ptr(d_hit_motif), _ptr(d_hit_seq), _ptr(d_hit_struct),
                                                     _ptr(d_hit_count), _ptr(stream)))

    # -- device-pointer scans (pointers are ints, e.g. torch data_ptr()) ----------
    def scan_dev(self, motif, d_codes, d_profile, profile_dtype, n_pos, d_out_seq, d_out_struct, stream=None):
        self._check(self._L.pfmscan_scan_dev(self._h, motif._h, _ptr(d_codes), _ptr(d_profile), int(profile_dtype),
                                             int(n_pos), _ptr(d_out_seq), _ptr(d_out_struct), _ptr(stream)))

    def scan_letters_f64_dev(self, motif, d_codes, n_pos, d_out, stream=None):
        self._check(self._L.pfmscan_scan_letters_f64_dev(self._h, motif._h, _ptr(d_codes), int(n_pos), _ptr(d_out), _ptr(stream)))

    def hits_dev(self, motif, d_codes, d_profile, profile_dtype, n_pos, thr_seq, thr_struct, capacity,
                 d_hit_pos, d_hit_seq, d_hit_struct, d_hit_count, stream=None):
        self._check(self._L.pfmscan_hits_dev(self._h, motif._h, _ptr(d_codes), _ptr(d_profile), int(profile_dtype),
                                             int(n_pos), float(thr_seq), float(thr_struct), int(capacity),
                                             _ptr(d_hit_pos), _ptr(d_hit_seq), _ptr(d_hit_struct), _ptr(d_hit_count),
                                             _ptr(stream)))

    def hits_adaptive_dev(self, motif, d_codes, d_profile, profile_dtype, n_pos, thr_seq, thr_struct, capacity,
                          d_hit_pos, d_hit_seq, d_hit_struct, d_hit_count, stream=None):
        """hits_dev that may run candidate-then-verify (synchronises the stream)"""
        self._check(self._L.pfmscan_hits_adaptive_dev(self._h, motif._h, _ptr(d_codes), _ptr(d_profile),
                                                      int(profile_dtype), int(n_pos), float(thr_seq), float(thr_struct),
                                                      int(capacity), _ptr(d_hit_pos), _ptr(d_hit_seq), _ptr(d_hit_struct),
                                                      _ptr(d_hit_count), _ptr(stream)))

    # -- in-silico mutagenesis (include/pfmscan.h: pfmscan_mutmap_*, pfmscan_variants_*) --------------------
    def mutmap_dev(self, motif, d_codes, n_pos, d_best, d_where=None, stream=None):
        self._check(self._L.pfmscan_mutmap_dev(self._h, motif._h, _ptr(d_codes), int(n_pos), _ptr(d_best), _ptr(d_where), _ptr(stream)))

    def mutmap_staged(self, motif, where=True):
        """best float32 [n_pos][4] (and where int8 [n_pos][4], or None) of the staged codes"""
        n = int(self._L.pfmscan_staged_positions(self._h))
        if n < 0:
            raise ValueError("no stream staged (call stage first)")
        best = np.empty((n, 4), dtype=np.float32)
        wh = np.empty((n, 4), dtype=np.int8) if where else None
        self._check(self._L.pfmscan_mutmap_staged(self._h, motif._h, _ptr(best), _ptr(wh)))
        return best, wh

    def mutmap_events_dev(self, motif, d_codes, n_pos, thr, capacity, d_ev_key, d_ev_ref, d_ev_alt, d_ev_count, stream=None):
        self._check(self._L.pfmscan_mutmap_events_dev(self._h, motif._h, _ptr(d_codes), int(n_pos), float(thr), int(capacity),
                                                      _ptr(d_ev_key), _ptr(d_ev_ref), _ptr(d_ev_alt), _ptr(d_ev_count), _ptr(stream)))

    def mutmap_events_staged(self, motif, thr, capacity=None):
        """gain / loss events of the staged codes at thr -> (key int64[k] = 4 p + a sorted, ref float32[k], alt float32[k])"""
        n = int(self._L.pfmscan_staged_positions(self._h))
        if n < 0:
            raise ValueError("no stream staged (call stage first)")
        cap = int(capacity) if capacity is not None else max(1024, n // 16)
        while True:
            key = np.empty(cap, dtype=np.int64)
            ref = np.empty(cap, dtype=np.float32)
            alt = np.empty(cap, dtype=np.float32)
            k = ctypes.c_int64(0)
            rc = self._L.pfmscan_mutmap_events_staged(self._h, motif._h, float(thr), cap, _ptr(key), _ptr(ref), _ptr(alt), ctypes.byref(k))
            if rc == E_CAPACITY and capacity is None:
                cap = int(k.value)
                continue
            self._check(rc, k.value)
            k = int(k.value)
            return key[:k].copy(), ref[:k].copy(), alt[:k].copy()

    @staticmethod
    def _variant_tables(letter_tables):
        lt = np.ascontiguousarray(letter_tables, dtype=np.float64)
        if lt.ndim == 2:
            lt = lt[None]
        if lt.ndim != 3 or lt.shape[2] != NCODE:
            raise ValueError("letter_tables must be [n_motifs][m][8]")
        return lt

    def variants_dev(self, letter_tables, d_codes, n_pos, d_var_pos, d_var_alt, n_var, d_ref, d_alt, d_ref_where=None,
                     d_alt_where=None, stream=None):
        lt = self._variant_tables(letter_tables)
        self._check(self._L.pfmscan_variants_dev(self._h, _ptr(lt), lt.shape[0], lt.shape[1], _ptr(d_codes), int(n_pos), _ptr(d_var_pos),
                                                 _ptr(d_var_alt), int(n_var), _ptr(d_ref), _ptr(d_alt), _ptr(d_ref_where),
                                                 _ptr(d_alt_where), _ptr(stream)))

    def variants_staged(self, letter_tables, pos, alt, where=True):
        """-> ref, alt float32 [n_var][n_motifs], ref_where, alt_where int8 (or None) over the staged codes"""
        lt = self._variant_tables(letter_tables)
        pos = np.ascontiguousarray(pos, dtype=np.int64)
        alt = np.ascontiguousarray(alt, dtype=np.uint8)
        if pos.ndim != 1 or pos.shape != alt.shape:
            raise ValueError("pos and alt must be lists of one length")
        shape = (pos.size, lt.shape[0])
        ref_s, alt_s = np.empty(shape, dtype=np.float32), np.empty(shape, dtype=np.float32)
        ref_w = np.empty(shape, dtype=np.int8) if where else None
        alt_w = np.empty(shape, dtype=np.int8) if where else None
        self._check(self._L.pfmscan_variants_staged(self._h, _ptr(lt), lt.shape[0], lt.shape[1], _ptr(pos), _ptr(alt), pos.size,
                                                    _ptr(ref_s), _ptr(alt_s), _ptr(ref_w), _ptr(alt_w)))
        return ref_s, alt_s, ref_w, alt_w

    # -- occupancy (include/pfmscan.h: pfmscan_occupancy_*) ------------------------------------------------
    @staticmethod
    def _ratio_tables(ratio_tables):
        rt = np.ascontiguousarray(ratio_tables, dtype=np.float64)
        if rt.ndim == 2:
            rt = rt[None]
        if rt.ndim != 3 or rt.shape[2] != NCODE:
            raise ValueError("ratio_tables must be [n_motifs][m][8]")
        return rt

    def occupancy_dev(self, ratio_tables, n_letters, d_codes, n_pos, d_rec_off, d_rec_len, n_rec, d_occ, d_windows=None):
        rt = self._ratio_tables(ratio_tables)
        self._check(self._L.pfmscan_occupancy_dev(self._h, _ptr(rt), rt.shape[0], rt.shape[1], int(n_letters), _ptr(d_codes), int(n_pos),
                                                  _ptr(d_rec_off), _ptr(d_rec_len), int(n_rec), _ptr(d_occ), _ptr(d_windows)))

    # -- what every *_staged call of the occupancy / expected-counts family starts with -------------------
    @staticmethod
    def _records(rec_off, rec_len):
        rec_off = np.ascontiguousarray(rec_off, dtype=np.int64)
        rec_len = np.ascontiguousarray(rec_len, dtype=np.int64)
        if rec_off.ndim != 1 or rec_off.shape != rec_len.shape:
            raise ValueError("rec_off and rec_len must be lists of one length")
        return rec_off, rec_len

    @staticmethod
    def _occ_windows(n_rec, n_motifs):
        return np.zeros((n_rec, n_motifs), dtype=np.float64), np.zeros(n_rec, dtype=np.int64)

    def occupancy_staged(self, ratio_tables, n_letters, rec_off, rec_len, which=0):
        """-> occ float64 [n_rec][n_motifs], windows int64 [n_rec] over the staged codes (which = 0) or codes2 (1)"""
        rt = self._ratio_tables(ratio_tables)
        rec_off, rec_len = self._records(rec_off, rec_len)
        occ, windows = self._occ_windows(rec_off.size, rt.shape[0])
        self._check(self._L.pfmscan_occupancy_staged(self._h, int(which), _ptr(rt), rt.shape[0], rt.shape[1], int(n_letters), _ptr(rec_off),
                                                     _ptr(rec_len), rec_off.size, _ptr(occ), _ptr(windows)))
        return occ, windows

    # -- occupancy on averaged-structure profiles (include/pfmscan.h: pfmscan_occupancy_profile_*) --------
    @staticmethod
    def _profile_tables(struct_tables, seq_tables):
        st = np.ascontiguousarray(struct_tables, dtype=np.float64)
        if st.ndim == 2:
            st = st[None]
        if st.ndim != 3 or st.shape[2] != NSTRUCT:
            raise ValueError("struct_tables must be [n_motifs][m][7]")
        sq = None
        if seq_tables is not None:
            sq = Context._ratio_tables(seq_tables)
            if sq.shape[:2] != st.shape[:2]:
                raise ValueError("seq_tables must hold as many motifs of the same width as struct_tables")
        return st, sq

    def occupancy_profile_dev(self, struct_tables, seq_tables, d_codes, d_profile, profile_dtype, n_pos, d_rec_off, d_rec_len, n_rec,
                              d_occ, d_windows=None):
        st, sq = self._profile_tables(struct_tables, seq_tables)
        self._check(self._L.pfmscan_occupancy_profile_dev(self._h, _ptr(st), _ptr(sq), st.shape[0], st.shape[1], _ptr(d_codes), _ptr(d_profile),
                                                          int(profile_dtype), int(n_pos), _ptr(d_rec_off), _ptr(d_rec_len), int(n_rec),
                                                          _ptr(d_occ), _ptr(d_windows)))

    def occupancy_profile_staged(self, struct_tables, seq_tables, rec_off, rec_len):
        """-> occ float64 [n_rec][n_motifs], windows int64 [n_rec] over the staged profile (structure only) or the staged
        codes and profile (joint: seq_tables [n_motifs][m][8])"""
        st, sq = self._profile_tables(struct_tables, seq_tables)
        rec_off, rec_len = self._records(rec_off, rec_len)
        occ, windows = self._occ_windows(rec_off.size, st.shape[0])
        self._check(self._L.pfmscan_occupancy_profile_staged(self._h, _ptr(st), _ptr(sq), st.shape[0], st.shape[1], _ptr(rec_off),
                                                             _ptr(rec_len), rec_off.size, _ptr(occ), _ptr(windows)))
        return occ, windows

    # -- expected counts (include/pfmscan.h: pfmscan_expect_*) ---------------------------------------------
    def expect_dev(self, ratio_tables, n_letters, mode, d_codes, n_pos, d_rec_off, d_rec_len, n_rec, d_exp, d_occ=None, d_windows=None):
        rt = self._ratio_tables(ratio_tables)
        self._check(self._L.pfmscan_expect_dev(self._h, _ptr(rt), rt.shape[0], rt.shape[1], int(n_letters), int(mode), _ptr(d_codes), int(n_pos),
                                               _ptr(d_rec_off), _ptr(d_rec_len), int(n_rec), _ptr(d_exp), _ptr(d_occ), _ptr(d_windows)))

    def expect_staged(self, ratio_tables, n_letters, mode, rec_off, rec_len, which=0):
        """-> exp float64 [n_rec][n_motifs][m][8], occ float64 [n_rec][n_motifs], windows int64 [n_rec] over the staged codes
        (which = 0) or codes2 (1); mode EXPECT_RATIO or EXPECT_POSTERIOR"""
        rt = self._ratio_tables(ratio_tables)
        rec_off, rec_len = self._records(rec_off, rec_len)
        exp = np.zeros((rec_off.size, rt.shape[0], rt.shape[1], NCODE), dtype=np.float64)
        occ, windows = self._occ_windows(rec_off.size, rt.shape[0])
        self._check(self._L.pfmscan_expect_staged(self._h, int(which), _ptr(rt), rt.shape[0], rt.shape[1], int(n_letters), int(mode),
                                                  _ptr(rec_off), _ptr(rec_len), rec_off.size, _ptr(exp), _ptr(occ), _ptr(windows)))
        return exp, occ, windows

    # -- expected counts on averaged-structure profiles (include/pfmscan.h: pfmscan_expect_profile_*) ------
    @staticmethod
    def _expect_profile_tables(struct_tables, seq_tables):
        if struct_tables is None and seq_tables is None:
            raise ValueError("struct_tables and seq_tables are both None")
        if struct_tables is None:
            return None, Context._ratio_tables(seq_tables)
        return Context._profile_tables(struct_tables, seq_tables)

    def expect_profile_dev(self, struct_tables, seq_tables, mode, d_codes, d_profile, profile_dtype, n_pos, d_rec_off, d_rec_len, n_rec,
                           d_exp_struct, d_exp_seq=None, d_occ=None, d_windows=None):
        st, sq = self._expect_profile_tables(struct_tables, seq_tables)
        n_motifs, m = (st if st is not None else sq).shape[:2]
        self._check(self._L.pfmscan_expect_profile_dev(self._h, _ptr(st), _ptr(sq), n_motifs, m, int(mode), _ptr(d_codes), _ptr(d_profile),
                                                       int(profile_dtype), int(n_pos), _ptr(d_rec_off), _ptr(d_rec_len), int(n_rec),
                                                       _ptr(d_exp_struct), _ptr(d_exp_seq), _ptr(d_occ), _ptr(d_windows)))

    def expect_profile_staged(self, struct_tables, seq_tables, mode, rec_off, rec_len):
        """-> exp_struct float64 [n_rec][n_motifs][m][8], exp_seq the same or None (no seq_tables), occ float64
        [n_rec][n_motifs], windows int64 [n_rec] over the staged profile (and codes where seq_tables is given); the weights
        come from struct_tables [n_motifs][m][7], seq_tables [n_motifs][m][8] or both; mode EXPECT_RATIO or EXPECT_POSTERIOR"""
        st, sq = self._expect_profile_tables(struct_tables, seq_tables)
        n_motifs, m = (st if st is not None else sq).shape[:2]
        rec_off, rec_len = self._records(rec_off, rec_len)
        exp_struct = np.zeros((rec_off.size, n_motifs, m, NCODE), dtype=np.float64)
        exp_seq = None if sq is None else np.zeros((rec_off.size, n_motifs, m, NCODE), dtype=np.float64)
        occ, windows = self._occ_windows(rec_off.size, n_motifs)
        self._check(self._L.pfmscan_expect_profile_staged(self._h, _ptr(st), _ptr(sq), n_motifs, m, int(mode), _ptr(rec_off), _ptr(rec_len),
                                                          rec_off.size, _ptr(exp_struct), _ptr(exp_seq), _ptr(occ), _ptr(windows)))
        return exp_struct, exp_seq, occ, windows

    def expect_profile_joint_dev(self, struct_tables, seq_tables, mode, d_codes, d_profile, profile_dtype, n_pos, d_rec_off, d_rec_len, n_rec,
                                 d_exp_struct, d_exp_seq, d_exp_joint, d_occ=None, d_windows=None):
        """``expect_profile_dev`` with the nucleotide x context table d_exp_joint float64 [n_rec][n_motifs][m][4][8]; any of the three
        may be None"""
        st, sq = self._expect_profile_tables(struct_tables, seq_tables)
        n_motifs, m = (st if st is not None else sq).shape[:2]
        self._check(self._L.pfmscan_expect_profile_joint_dev(self._h, _ptr(st), _ptr(sq), n_motifs, m, int(mode), _ptr(d_codes), _ptr(d_profile),
                                                             int(profile_dtype), int(n_pos), _ptr(d_rec_off), _ptr(d_rec_len), int(n_rec),
                                                             _ptr(d_exp_struct), _ptr(d_exp_seq), _ptr(d_exp_joint), _ptr(d_occ), _ptr(d_windows)))

    def expect_profile_joint_staged(self, struct_tables, seq_tables, mode, rec_off, rec_len, want_struct=True, want_seq=True, want_joint=True):
        """``expect_profile_staged`` with the nucleotide x context table -> exp_struct, exp_seq, exp_joint float64
        [n_rec][n_motifs][m][4][8] (cell [k][a][c]: the rows' cell c, in stored column order, under nucleotide a at column k; c = 7 is
        +0.0), occ, windows; None where not wanted"""
        st, sq = self._expect_profile_tables(struct_tables, seq_tables)
        n_motifs, m = (st if st is not None else sq).shape[:2]
        rec_off, rec_len = self._records(rec_off, rec_len)
        exp_struct = np.zeros((rec_off.size, n_motifs, m, NCODE), dtype=np.float64) if want_struct else None
        exp_seq = np.zeros((rec_off.size, n_motifs, m, NCODE), dtype=np.float64) if want_seq else None
        exp_joint = np.zeros((rec_off.size, n_motifs, m, 4, NCODE), dtype=np.float64) if want_joint else None
        occ, windows = self._occ_windows(rec_off.size, n_motifs)
        self._check(self._L.pfmscan_expect_profile_joint_staged(self._h, _ptr(st), _ptr(sq), n_motifs, m, int(mode), _ptr(rec_off), _ptr(rec_len),
                                                                rec_off.size, _ptr(exp_struct), _ptr(exp_seq), _ptr(exp_joint), _ptr(occ),
                                                                _ptr(windows)))
        return exp_struct, exp_seq, exp_joint, occ, windows

    # -- two code streams (include/pfmscan.h: pfmscan_occupancy_pair_*, pfmscan_expect_pair_*) ---------------
    @staticmethod
    def _pair_tables(seq_tables, struct_tables):
        sq, st = Context._ratio_tables(seq_tables), Context._ratio_tables(struct_tables)
        if sq.shape != st.shape:
            raise ValueError("seq_tables and struct_tables must hold as many motifs of the same width")
        return sq, st

    def occupancy_pair_dev(self, seq_tables, struct_tables, d_codes, d_codes2, n_pos, d_rec_off, d_rec_len, n_rec, d_occ, d_windows=None):
        sq, st = self._pair_tables(seq_tables, struct_tables)
        self._check(self._L.pfmscan_occupancy_pair_dev(self._h, _ptr(sq), _ptr(st), sq.shape[0], sq.shape[1], _ptr(d_codes), _ptr(d_codes2),
                                                       int(n_pos), _ptr(d_rec_off), _ptr(d_rec_len), int(n_rec), _ptr(d_occ), _ptr(d_windows)))

    def occupancy_pair_staged(self, seq_tables, struct_tables, rec_off, rec_len):
        """-> occ float64 [n_rec][n_motifs], windows int64 [n_rec] over the staged codes and codes2; pair q is
        (seq_tables[q], struct_tables[q]), [m][8] both"""
        sq, st = self._pair_tables(seq_tables, struct_tables)
        rec_off, rec_len = self._records(rec_off, rec_len)
        occ, windows = self._occ_windows(rec_off.size, sq.shape[0])
        self._check(self._L.pfmscan_occupancy_pair_staged(self._h, _ptr(sq), _ptr(st), sq.shape[0], sq.shape[1], _ptr(rec_off), _ptr(rec_len),
                                                          rec_off.size, _ptr(occ), _ptr(windows)))
        return occ, windows

    def expect_pair_dev(self, seq_tables, struct_tables, mode, d_codes, d_codes2, n_pos, d_rec_off, d_rec_len, n_rec, d_exp_seq, d_exp_struct,
                        d_occ=None, d_windows=None):
        sq, st = self._pair_tables(seq_tables, struct_tables)
        self._check(self._L.pfmscan_expect_pair_dev(self._h, _ptr(sq), _ptr(st), sq.shape[0], sq.shape[1], int(mode), _ptr(d_codes), _ptr(d_codes2),
                                                    int(n_pos), _ptr(d_rec_off), _ptr(d_rec_len), int(n_rec), _ptr(d_exp_seq), _ptr(d_exp_struct),
                                                    _ptr(d_occ), _ptr(d_windows)))

    def expect_pair_staged(self, seq_tables, struct_tables, mode, rec_off, rec_len, want_seq=True, want_struct=True):
        """-> exp_seq, exp_struct float64 [n_rec][n_motifs][m][8] (None where not wanted), occ float64 [n_rec][n_motifs], windows
        int64 [n_rec] over the staged codes and codes2; mode EXPECT_RATIO or EXPECT_POSTERIOR"""
        sq, st = self._pair_tables(seq_tables, struct_tables)
        n_motifs, m = sq.shape[:2]
        rec_off, rec_len = self._records(rec_off, rec_len)
        exp_seq = np.zeros((rec_off.size, n_motifs, m, NCODE), dtype=np.float64) if want_seq else None
        exp_struct = np.zeros((rec_off.size, n_motifs, m, NCODE), dtype=np.float64) if want_struct else None
        occ, windows = self._occ_windows(rec_off.size, n_motifs)
        self._check(self._L.pfmscan_expect_pair_staged(self._h, _ptr(sq), _ptr(st), n_motifs, m, int(mode), _ptr(rec_off), _ptr(rec_len),
                                                       rec_off.size, _ptr(exp_seq), _ptr(exp_struct), _ptr(occ), _ptr(windows)))
        return exp_seq, exp_struct, occ, windows

    def expect_pair_joint_dev(self, seq_tables, struct_tables, mode, d_codes, d_codes2, n_pos, d_rec_off, d_rec_len, n_rec, d_exp_seq, d_exp_struct,
                              d_exp_joint, d_occ=None, d_windows=None):
        """``expect_pair_dev`` with the letter-pair table d_exp_joint float64 [n_rec][n_motifs][m][4][8]; any of the three may be None"""
        sq, st = self._pair_tables(seq_tables, struct_tables)
        self._check(self._L.pfmscan_expect_pair_joint_dev(self._h, _ptr(sq), _ptr(st), sq.shape[0], sq.shape[1], int(mode), _ptr(d_codes),
                                                          _ptr(d_codes2), int(n_pos), _ptr(d_rec_off), _ptr(d_rec_len), int(n_rec), _ptr(d_exp_seq),
                                                          _ptr(d_exp_struct), _ptr(d_exp_joint), _ptr(d_occ), _ptr(d_windows)))

    def expect_pair_joint_staged(self, seq_tables, struct_tables, mode, rec_off, rec_len, want_seq=True, want_struct=True, want_joint=True):
        """``expect_pair_staged`` with the letter-pair table -> exp_seq, exp_struct, exp_joint float64 [n_rec][n_motifs][m][4][8]
        (cell [k][a][b]: nucleotide a over structure letter b under column k; b = 7 is +0.0), occ, windows; None where not wanted"""
        sq, st = self._pair_tables(seq_tables, struct_tables)
        n_motifs, m = sq.shape[:2]
        rec_off, rec_len = self._records(rec_off, rec_len)
        exp_seq = np.zeros((rec_off.size, n_motifs, m, NCODE), dtype=np.float64) if want_seq else None
        exp_struct = np.zeros((rec_off.size, n_motifs, m, NCODE), dtype=np.float64) if want_struct else None
        exp_joint = np.zeros((rec_off.size, n_motifs, m, 4, NCODE), dtype=np.float64) if want_joint else None
        occ, windows = self._occ_windows(rec_off.size, n_motifs)
        self._check(self._L.pfmscan_expect_pair_joint_staged(self._h, _ptr(sq), _ptr(st), n_motifs, m, int(mode), _ptr(rec_off), _ptr(rec_len),
                                                             rec_off.size, _ptr(exp_seq), _ptr(exp_struct), _ptr(exp_joint), _ptr(occ), _ptr(windows)))
        return exp_seq, exp_struct, exp_joint, occ, windows

    # -- expected counts, the records added up on the device (include/pfmscan.h: pfmscan_expect_merge_dev, *_merged_staged) --
    def expect_merge_dev(self, d_exp, n_rec, n_motifs, m, zero_first, d_acc, d_bad):
        """d_exp [n_rec][n_motifs][m][8] -> d_acc uint64 [n_motifs][SITE_LIMBS][m * 8] (RAW sums, added unless zero_first),
        d_bad int64 [n_motifs][2]; device buffers, asynchronous on the ctx's stream"""
        self._check(self._L.pfmscan_expect_merge_dev(self._h, _ptr(d_exp), int(n_rec), int(n_motifs), int(m), int(bool(zero_first)), _ptr(d_acc),
                                                     _ptr(d_bad)))

    @staticmethod
    def _merge_acc(acc, n_motifs, m, name):
        if not (isinstance(acc, np.ndarray) and acc.dtype == np.uint64 and acc.flags.c_contiguous and acc.flags.writeable) or \
                acc.shape != (n_motifs, SITE_LIMBS, m * NCODE):
            raise ValueError("%s must be a writable C-contiguous uint64 [%d][%d][%d]" % (name, n_motifs, SITE_LIMBS, m * NCODE))
        return acc

    def expect_merged_staged(self, ratio_tables, n_letters, mode, rec_off, rec_len, acc, which=0):
        """``expect_staged`` with the matrices added up over the records on the device: acc uint64 [n_motifs][SITE_LIMBS][m * 8]
        (normalised, changed in place: this call's sums are added) -> bad int64 [n_motifs][2] of this call (first record with a
        non-finite cell, first with a negative one; -1: none), occ float64 [n_rec][n_motifs], windows int64 [n_rec]"""
        rt = self._ratio_tables(ratio_tables)
        rec_off, rec_len = self._records(rec_off, rec_len)
        self._merge_acc(acc, rt.shape[0], rt.shape[1], "acc")
        bad = np.full((rt.shape[0], 2), -1, dtype=np.int64)
        occ, windows = self._occ_windows(rec_off.size, rt.shape[0])
        self._check(self._L.pfmscan_expect_merged_staged(self._h, int(which), _ptr(rt), rt.shape[0], rt.shape[1], int(n_letters), int(mode),
                                                         _ptr(rec_off), _ptr(rec_len), rec_off.size, _ptr(acc), _ptr(bad), _ptr(occ), _ptr(windows)))
        return bad, occ, windows

    def expect_profile_merged_staged(self, struct_tables, seq_tables, mode, rec_off, rec_len, acc_struct, acc_seq=None):
        """``expect_profile_staged`` with both matrices added up over the records on the device into acc_struct and (with
        seq_tables) acc_seq, uint64 [n_motifs][SITE_LIMBS][m * 8] normalised, changed in place ->
        bad_struct int64 [n_motifs][2], bad_seq the same | None, occ float64 [n_rec][n_motifs], windows int64 [n_rec]"""
        st, sq = self._expect_profile_tables(struct_tables, seq_tables)
        n_motifs, m = (st if st is not None else sq).shape[:2]
        rec_off, rec_len = self._records(rec_off, rec_len)
        self._merge_acc(acc_struct, n_motifs, m, "acc_struct")
        if acc_seq is not None:
            self._merge_acc(acc_seq, n_motifs, m, "acc_seq")
        bad_struct = np.full((n_motifs, 2), -1, dtype=np.int64)
        bad_seq = None if acc_seq is None else np.full((n_motifs, 2), -1, dtype=np.int64)
        occ, windows = self._occ_windows(rec_off.size, n_motifs)
        self._check(self._L.pfmscan_expect_profile_merged_staged(self._h, _ptr(st), _ptr(sq), n_motifs, m, int(mode), _ptr(rec_off), _ptr(rec_len),
                                                                 rec_off.size, _ptr(acc_struct), _ptr(acc_seq), _ptr(bad_struct), _ptr(bad_seq),
                                                                 _ptr(occ), _ptr(windows)))
        return bad_struct, bad_seq, occ, windows

    def expect_profile_joint_merged_staged(self, struct_tables, seq_tables, mode, rec_off, rec_len, acc_struct, acc_seq, acc_joint):
        """``expect_profile_merged_staged`` with the table's accumulator acc_joint uint64 [n_motifs][SITE_LIMBS][4 m * 8] (any of the
        three may be None) -> bad_struct, bad_seq, bad_joint (None where no accumulator), occ, windows"""
        st, sq = self._expect_profile_tables(struct_tables, seq_tables)
        n_motifs, m = (st if st is not None else sq).shape[:2]
        rec_off, rec_len = self._records(rec_off, rec_len)
        accs = ((acc_struct, "acc_struct", m), (acc_seq, "acc_seq", m), (acc_joint, "acc_joint", 4 * m))
        for acc, name, rows in accs:
            if acc is not None:
                self._merge_acc(acc, n_motifs, rows, name)
        bads = [None if acc is None else np.full((n_motifs, 2), -1, dtype=np.int64) for acc, _, _ in accs]
        occ, windows = self._occ_windows(rec_off.size, n_motifs)
        self._check(self._L.pfmscan_expect_profile_joint_merged_staged(self._h, _ptr(st), _ptr(sq), n_motifs, m, int(mode), _ptr(rec_off),
                                                                       _ptr(rec_len), rec_off.size, _ptr(acc_struct), _ptr(acc_seq), _ptr(acc_joint),
                                                                       _ptr(bads[0]), _ptr(bads[1]), _ptr(bads[2]), _ptr(occ), _ptr(windows)))
        return bads[0], bads[1], bads[2], occ, windows

    def expect_pair_merged_staged(self, seq_tables, struct_tables, mode, rec_off, rec_len, acc_seq, acc_struct):
        """``expect_pair_staged`` with the matrices added up over the records on the device into acc_seq and acc_struct (either
        may be None), uint64 [n_motifs][SITE_LIMBS][m * 8] normalised, changed in place ->
        bad_seq, bad_struct int64 [n_motifs][2] (None where no accumulator), occ float64 [n_rec][n_motifs], windows int64 [n_rec]"""
        sq, st = self._pair_tables(seq_tables, struct_tables)
        n_motifs, m = sq.shape[:2]
        rec_off, rec_len = self._records(rec_off, rec_len)
        for acc, name in ((acc_seq, "acc_seq"), (acc_struct, "acc_struct")):
            if acc is not None:
                self._merge_acc(acc, n_motifs, m, name)
        bad_seq = None if acc_seq is None else np.full((n_motifs, 2), -1, dtype=np.int64)
        bad_struct = None if acc_struct is None else np.full((n_motifs, 2), -1, dtype=np.int64)
        occ, windows = self._occ_windows(rec_off.size, n_motifs)
        self._check(self._L.pfmscan_expect_pair_merged_staged(self._h, _ptr(sq), _ptr(st), n_motifs, m, int(mode), _ptr(rec_off), _ptr(rec_len),
                                                              rec_off.size, _ptr(acc_seq), _ptr(acc_struct), _ptr(bad_seq), _ptr(bad_struct), _ptr(occ),
                                                              _ptr(windows)))
        return bad_seq, bad_struct, occ, windows

    def expect_pair_joint_merged_staged(self, seq_tables, struct_tables, mode, rec_off, rec_len, acc_seq, acc_struct, acc_joint):
        """``expect_pair_merged_staged`` with the letter-pair table's accumulator acc_joint uint64 [n_motifs][SITE_LIMBS][4 m * 8]
        (any of the three may be None) -> bad_seq, bad_struct, bad_joint (None where no accumulator), occ, windows"""
        sq, st = self._pair_tables(seq_tables, struct_tables)
        n_motifs, m = sq.shape[:2]
        rec_off, rec_len = self._records(rec_off, rec_len)
        accs = ((acc_seq, "acc_seq", m), (acc_struct, "acc_struct", m), (acc_joint, "acc_joint", 4 * m))
        for acc, name, rows in accs:
            if acc is not None:
                self._merge_acc(acc, n_motifs, rows, name)
        bads = [None if acc is None else np.full((n_motifs, 2), -1, dtype=np.int64) for acc, _, _ in accs]
        occ, windows = self._occ_windows(rec_off.size, n_motifs)
        self._check(self._L.pfmscan_expect_pair_joint_merged_staged(self._h, _ptr(sq), _ptr(st), n_motifs, m, int(mode), _ptr(rec_off), _ptr(rec_len),
                                                                    rec_off.size, _ptr(acc_seq), _ptr(acc_struct), _ptr(acc_joint), _ptr(bads[0]),
                                                                    _ptr(bads[1]), _ptr(bads[2]), _ptr(occ), _ptr(windows)))
        return bads[0], bads[1], bads[2], occ, windows

    # -- posterior site map (include/pfmscan.h: pfmscan_footprint_*) ------------------------------------------
    @staticmethod
    def _footprint_tables(seq_tables, struct_tables):
        """either table stack may be None (not both): seq alone reads codes, struct alone codes2, both are the pair"""
        if seq_tables is None and struct_tables is None:
            raise ValueError("seq_tables and struct_tables are both None")
        if seq_tables is not None and struct_tables is not None:
            return Context._pair_tables(seq_tables, struct_tables)
        return (None if seq_tables is None else Context._ratio_tables(seq_tables),
                None if struct_tables is None else Context._ratio_tables(struct_tables))

    def footprint_dev(self, seq_tables, struct_tables, mode, d_codes, d_codes2, n_pos, d_rec_off, d_rec_len, n_rec, d_start, d_cover,
                      d_occ=None, d_windows=None):
        sq, st = self._footprint_tables(seq_tables, struct_tables)
        n_motifs, m = (sq if sq is not None else st).shape[:2]
        self._check(self._L.pfmscan_footprint_dev(self._h, _ptr(sq), _ptr(st), n_motifs, m, int(mode), _ptr(d_codes), _ptr(d_codes2), int(n_pos),
                                                  _ptr(d_rec_off), _ptr(d_rec_len), int(n_rec), _ptr(d_start), _ptr(d_cover), _ptr(d_occ),
                                                  _ptr(d_windows)))

    def footprint_staged(self, seq_tables, struct_tables, mode, rec_off, rec_len, want_start=True, want_cover=True):
        """-> start, cover float64 [n_motifs][n_pos] aligned with the staged stream (None where not wanted; +0.0 outside the
        records of the table), occ float64 [n_rec][n_motifs], windows int64 [n_rec]; mode EXPECT_RATIO or EXPECT_POSTERIOR"""
        sq, st = self._footprint_tables(seq_tables, struct_tables)
        n_motifs, m = (sq if sq is not None else st).shape[:2]
        n = int(self._L.pfmscan_staged_positions(self._h))
        if n < 0:
            raise ValueError("no stream staged (call stage first)")
        rec_off, rec_len = self._records(rec_off, rec_len)
        start = np.zeros((n_motifs, n), dtype=np.float64) if want_start else None
        cover = np.zeros((n_motifs, n), dtype=np.float64) if want_cover else None
        occ, windows = self._occ_windows(rec_off.size, n_motifs)
        self._check(self._L.pfmscan_footprint_staged(self._h, _ptr(sq), _ptr(st), n_motifs, m, int(mode), _ptr(rec_off), _ptr(rec_len),
                                                     rec_off.size, _ptr(start), _ptr(cover), _ptr(occ), _ptr(windows)))
        return start, cover, occ, windows

    def footprint_events_dev(self, seq_tables, struct_tables, mode, d_codes, d_codes2, n_pos, d_rec_off, d_rec_len, n_rec, thr, capacity,
                             d_ev_key, d_ev_cover, d_ev_start, d_ev_count, d_occ=None, d_windows=None):
        sq, st = self._footprint_tables(seq_tables, struct_tables)
        n_motifs, m = (sq if sq is not None else st).shape[:2]
        self._check(self._L.pfmscan_footprint_events_dev(self._h, _ptr(sq), _ptr(st), n_motifs, m, int(mode), _ptr(d_codes), _ptr(d_codes2),
                                                         int(n_pos), _ptr(d_rec_off), _ptr(d_rec_len), int(n_rec), float(thr), int(capacity),
                                                         _ptr(d_ev_key), _ptr(d_ev_cover), _ptr(d_ev_start), _ptr(d_ev_count), _ptr(d_occ),
                                                         _ptr(d_windows)))

    def footprint_events_staged(self, seq_tables, struct_tables, mode, rec_off, rec_len, thr, capacity=None):
        """the positions of the staged stream whose cover > thr, decided on the device -> (key int64[k] = motif * n_pos + position
        sorted, cover float64[k], start float64[k], occ float64 [n_rec][n_motifs], windows int64 [n_rec]).  capacity None: a
        capacity verdict is answered by one retry with the capacity it names; else CapacityError carries it"""
        sq, st = self._footprint_tables(seq_tables, struct_tables)
        n_motifs, m = (sq if sq is not None else st).shape[:2]
        n = int(self._L.pfmscan_staged_positions(self._h))
        if n < 0:
            raise ValueError("no stream staged (call stage first)")
        rec_off, rec_len = self._records(rec_off, rec_len)
        cap = int(capacity) if capacity is not None else max(1024, n // 16)
        while True:
            key = np.empty(cap, dtype=np.int64)
            cover = np.empty(cap, dtype=np.float64)
            start = np.empty(cap, dtype=np.float64)
            occ, windows = self._occ_windows(rec_off.size, n_motifs)
            k = ctypes.c_int64(0)
            rc = self._L.pfmscan_footprint_events_staged(self._h, _ptr(sq), _ptr(st), n_motifs, m, int(mode), _ptr(rec_off), _ptr(rec_len),
                                                         rec_off.size, float(thr), cap, _ptr(key), _ptr(cover), _ptr(start), ctypes.byref(k),
                                                         _ptr(occ), _ptr(windows))
            if rc == E_CAPACITY and capacity is None:
                cap = int(k.value)
                continue
            self._check(rc, k.value)
            k = int(k.value)
            return key[:k].copy(), cover[:k].copy(), start[:k].copy(), occ, windows

    # -- multi-site model (include/pfmscan.h: pfmscan_multisite_*) ------------------------------------------------
    @staticmethod
    def _lam(lam, n_rec):
        lam = np.ascontiguousarray(lam, dtype=np.float64)
        if lam.shape != (n_rec,):
            raise ValueError("lam must hold one double per record")
        return lam

    def multisite_dev(self, seq_tables, struct_tables, d_codes, d_codes2, n_pos, d_rec_off, d_rec_len, n_rec, d_lam, d_start, d_cover,
                      d_z=None, d_nsites=None, d_windows=None):
        sq, st = self._footprint_tables(seq_tables, struct_tables)
        n_motifs, m = (sq if sq is not None else st).shape[:2]
        self._check(self._L.pfmscan_multisite_dev(self._h, _ptr(sq), _ptr(st), n_motifs, m, _ptr(d_codes), _ptr(d_codes2), int(n_pos),
                                                  _ptr(d_rec_off), _ptr(d_rec_len), int(n_rec), _ptr(d_lam), _ptr(d_start), _ptr(d_cover),
                                                  _ptr(d_z), _ptr(d_nsites), _ptr(d_windows)))

    def multisite_staged(self, seq_tables, struct_tables, rec_off, rec_len, lam, want_start=True, want_cover=True):
        """-> start, cover float64 [n_motifs][n_pos] aligned with the staged stream (None where not wanted; +0.0 outside the
        records of the table), z, nsites float64 [n_rec][n_motifs], windows int64 [n_rec]; lam float64 [n_rec]"""
        sq, st = self._footprint_tables(seq_tables, struct_tables)
        n_motifs, m = (sq if sq is not None else st).shape[:2]
        n = int(self._L.pfmscan_staged_positions(self._h))
        if n < 0:
            raise ValueError("no stream staged (call stage first)")
        rec_off, rec_len = self._records(rec_off, rec_len)
        lam = self._lam(lam, rec_off.size)
        start = np.zeros((n_motifs, n), dtype=np.float64) if want_start else None
        cover = np.zeros((n_motifs, n), dtype=np.float64) if want_cover else None
        z, windows = self._occ_windows(rec_off.size, n_motifs)
        nsites = np.zeros_like(z)
        self._check(self._L.pfmscan_multisite_staged(self._h, _ptr(sq), _ptr(st), n_motifs, m, _ptr(rec_off), _ptr(rec_len), rec_off.size,
                                                     _ptr(lam), _ptr(start), _ptr(cover), _ptr(z), _ptr(nsites), _ptr(windows)))
        return start, cover, z, nsites, windows

    def multisite_events_dev(self, seq_tables, struct_tables, d_codes, d_codes2, n_pos, d_rec_off, d_rec_len, n_rec, d_lam, thr, capacity,
                             d_ev_key, d_ev_cover, d_ev_start, d_ev_count, d_z=None, d_nsites=None, d_windows=None):
        sq, st = self._footprint_tables(seq_tables, struct_tables)
        n_motifs, m = (sq if sq is not None else st).shape[:2]
        self._check(self._L.pfmscan_multisite_events_dev(self._h, _ptr(sq), _ptr(st), n_motifs, m, _ptr(d_codes), _ptr(d_codes2), int(n_pos),
                                                         _ptr(d_rec_off), _ptr(d_rec_len), int(n_rec), _ptr(d_lam), float(thr), int(capacity),
                                                         _ptr(d_ev_key), _ptr(d_ev_cover), _ptr(d_ev_start), _ptr(d_ev_count), _ptr(d_z),
                                                         _ptr(d_nsites), _ptr(d_windows)))

    def multisite_events_staged(self, seq_tables, struct_tables, rec_off, rec_len, lam, thr, capacity=None):
        """the positions of the staged stream whose cover > thr, decided on the device -> (key int64[k] = motif * n_pos + position
        sorted, cover float64[k], start float64[k], z, nsites float64 [n_rec][n_motifs], windows int64 [n_rec]).  capacity None:
        a capacity verdict is answered by one retry with the capacity it names; else CapacityError carries it"""
        sq, st = self._footprint_tables(seq_tables, struct_tables)
        n_motifs, m = (sq if sq is not None else st).shape[:2]
        n = int(self._L.pfmscan_staged_positions(self._h))
        if n < 0:
            raise ValueError("no stream staged (call stage first)")
        rec_off, rec_len = self._records(rec_off, rec_len)
        lam = self._lam(lam, rec_off.size)
        cap = int(capacity) if capacity is not None else max(1024, n // 16)
        while True:
            key = np.empty(cap, dtype=np.int64)
            cover = np.empty(cap, dtype=np.float64)
            start = np.empty(cap, dtype=np.float64)
            z, windows = self._occ_windows(rec_off.size, n_motifs)
            nsites = np.zeros_like(z)
            k = ctypes.c_int64(0)
            rc = self._L.pfmscan_multisite_events_staged(self._h, _ptr(sq), _ptr(st), n_motifs, m, _ptr(rec_off), _ptr(rec_len), rec_off.size,
                                                         _ptr(lam), float(thr), cap, _ptr(key), _ptr(cover), _ptr(start), ctypes.byref(k),
                                                         _ptr(z), _ptr(nsites), _ptr(windows))
            if rc == E_CAPACITY and capacity is None:
                cap = int(k.value)
                continue
            self._check(rc, k.value)
            k = int(k.value)
            return key[:k].copy(), cover[:k].copy(), start[:k].copy(), z, nsites, windows

    # -- threshold-free mutagenesis (include/pfmscan.h: pfmscan_mutocc_*) -------------------------------------
    def mutocc_dev(self, ratio_tables, d_codes, n_pos, d_rec_off, d_rec_len, n_rec, d_local, d_occ=None, d_windows=None):
        T = self._ratio_tables(ratio_tables)
        self._check(self._L.pfmscan_mutocc_dev(self._h, _ptr(T), T.shape[0], T.shape[1], _ptr(d_codes), int(n_pos), _ptr(d_rec_off), _ptr(d_rec_len),
                                               int(n_rec), _ptr(d_local), _ptr(d_occ), _ptr(d_windows)))

    def mutocc_staged(self, ratio_tables, rec_off, rec_len):
        """-> local float64 [n_motifs][n_pos][4] aligned with the staged stream (NaN outside the records of the table and where
        a record holds no letter), occ float64 [n_rec][n_motifs], windows int64 [n_rec]"""
        T = self._ratio_tables(ratio_tables)
        n_motifs = T.shape[0]
        n = int(self._L.pfmscan_staged_positions(self._h))
        if n < 0:
            raise ValueError("no stream staged (call stage first)")
        rec_off, rec_len = self._records(rec_off, rec_len)
        local = np.full((n_motifs, n, 4), np.nan, dtype=np.float64)
        occ, windows = self._occ_windows(rec_off.size, n_motifs)
        self._check(self._L.pfmscan_mutocc_staged(self._h, _ptr(T), n_motifs, T.shape[1], _ptr(rec_off), _ptr(rec_len), rec_off.size, _ptr(local),
                                                  _ptr(occ), _ptr(windows)))
        return local, occ, windows

    def mutocc_events_dev(self, ratio_tables, d_codes, n_pos, d_rec_off, d_rec_len, n_rec, frac, capacity, d_ev_key, d_ev_alt, d_ev_ref,
                          d_ev_count, d_occ=None, d_windows=None):
        T = self._ratio_tables(ratio_tables)
        self._check(self._L.pfmscan_mutocc_events_dev(self._h, _ptr(T), T.shape[0], T.shape[1], _ptr(d_codes), int(n_pos), _ptr(d_rec_off),
                                                      _ptr(d_rec_len), int(n_rec), float(frac), int(capacity), _ptr(d_ev_key), _ptr(d_ev_alt),
                                                      _ptr(d_ev_ref), _ptr(d_ev_count), _ptr(d_occ), _ptr(d_windows)))

    def mutocc_events_staged(self, ratio_tables, rec_off, rec_len, frac, capacity=None):
        """the single-letter changes of the staged stream that add or remove more than frac of their record's occupancy, decided
        on the device -> (key int64[k] = (motif * n_pos + position) * 4 + alt letter sorted, alt float64[k], ref float64[k], occ
        float64 [n_rec][n_motifs], windows int64 [n_rec]).  capacity None: a capacity verdict is answered by one retry with the
        capacity it names; else CapacityError carries it"""
        T = self._ratio_tables(ratio_tables)
        n_motifs = T.shape[0]
        n = int(self._L.pfmscan_staged_positions(self._h))
        if n < 0:
            raise ValueError("no stream staged (call stage first)")
        rec_off, rec_len = self._records(rec_off, rec_len)
        cap = int(capacity) if capacity is not None else max(1024, n // 16)
        while True:
            key = np.empty(cap, dtype=np.int64)
            alt = np.empty(cap, dtype=np.float64)
            ref = np.empty(cap, dtype=np.float64)
            occ, windows = self._occ_windows(rec_off.size, n_motifs)
            k = ctypes.c_int64(0)
            rc = self._L.pfmscan_mutocc_events_staged(self._h, _ptr(T), n_motifs, T.shape[1], _ptr(rec_off), _ptr(rec_len), rec_off.size,
                                                      float(frac), cap, _ptr(key), _ptr(alt), _ptr(ref), ctypes.byref(k), _ptr(occ), _ptr(windows))
            if rc == E_CAPACITY and capacity is None:
                cap = int(k.value)
                continue
            self._check(rc, k.value)
            k = int(k.value)
            return key[:k].copy(), alt[:k].copy(), ref[:k].copy(), occ, windows

    # -- posterior site map on averaged-structure profiles (include/pfmscan.h: pfmscan_footprint_profile_*) ---
    def footprint_profile_dev(self, struct_tables, seq_tables, mode, d_codes, d_profile, profile_dtype, n_pos, d_rec_off, d_rec_len, n_rec,
                              d_start, d_cover, d_occ=None, d_windows=None):
        st, sq = self._profile_tables(struct_tables, seq_tables)
        self._check(self._L.pfmscan_footprint_profile_dev(self._h, _ptr(st), _ptr(sq), st.shape[0], st.shape[1], int(mode), _ptr(d_codes),
                                                          _ptr(d_profile), int(profile_dtype), int(n_pos), _ptr(d_rec_off), _ptr(d_rec_len),
                                                          int(n_rec), _ptr(d_start), _ptr(d_cover), _ptr(d_occ), _ptr(d_windows)))

    def footprint_profile_staged(self, struct_tables, seq_tables, mode, rec_off, rec_len, want_start=True, want_cover=True):
        """-> start, cover float64 [n_motifs][n_pos] aligned with the staged profile (None where not wanted; +0.0 outside the
        records of the table), occ float64 [n_rec][n_motifs], windows int64 [n_rec]; struct_tables [n_motifs][m][7] in the
        profile's stored column order, seq_tables [n_motifs][m][8] | None (joint: the staged codes too)"""
        st, sq = self._profile_tables(struct_tables, seq_tables)
        n_motifs, m = st.shape[:2]
        n = int(self._L.pfmscan_staged_positions(self._h))
        if n < 0:
            raise ValueError("no stream staged (call stage first)")
        rec_off, rec_len = self._records(rec_off, rec_len)
        start = np.zeros((n_motifs, n), dtype=np.float64) if want_start else None
        cover = np.zeros((n_motifs, n), dtype=np.float64) if want_cover else None
        occ, windows = self._occ_windows(rec_off.size, n_motifs)
        self._check(self._L.pfmscan_footprint_profile_staged(self._h, _ptr(st), _ptr(sq), n_motifs, m, int(mode), _ptr(rec_off), _ptr(rec_len),
                                                             rec_off.size, _ptr(start), _ptr(cover), _ptr(occ), _ptr(windows)))
        return start, cover, occ, windows

    def footprint_profile_events_dev(self, struct_tables, seq_tables, mode, d_codes, d_profile, profile_dtype, n_pos, d_rec_off, d_rec_len,
                                     n_rec, thr, capacity, d_ev_key, d_ev_cover, d_ev_start, d_ev_count, d_occ=None, d_windows=None):
        st, sq = self._profile_tables(struct_tables, seq_tables)
        self._check(self._L.pfmscan_footprint_profile_events_dev(self._h, _ptr(st), _ptr(sq), st.shape[0], st.shape[1], int(mode), _ptr(d_codes),
                                                                 _ptr(d_profile), int(profile_dtype), int(n_pos), _ptr(d_rec_off),
                                                                 _ptr(d_rec_len), int(n_rec), float(thr), int(capacity), _ptr(d_ev_key),
                                                                 _ptr(d_ev_cover), _ptr(d_ev_start), _ptr(d_ev_count), _ptr(d_occ), _ptr(d_windows)))

    def footprint_profile_events_staged(self, struct_tables, seq_tables, mode, rec_off, rec_len, thr, capacity=None):
        """the positions of the staged profile whose cover > thr, decided on the device -> (key int64[k] = motif * n_pos +
        position sorted, cover float64[k], start float64[k], occ float64 [n_rec][n_motifs], windows int64 [n_rec]).  capacity
        None: a capacity verdict is answered by one retry with the capacity it names; else CapacityError carries it"""
        st, sq = self._profile_tables(struct_tables, seq_tables)
        n_motifs, m = st.shape[:2]
        n = int(self._L.pfmscan_staged_positions(self._h))
        if n < 0:
            raise ValueError("no stream staged (call stage first)")
        rec_off, rec_len = self._records(rec_off, rec_len)
        cap = int(capacity) if capacity is not None else max(1024, n // 16)
        while True:
            key = np.empty(cap, dtype=np.int64)
            cover = np.empty(cap, dtype=np.float64)
            start = np.empty(cap, dtype=np.float64)
            occ, windows = self._occ_windows(rec_off.size, n_motifs)
            k = ctypes.c_int64(0)
            rc = self._L.pfmscan_footprint_profile_events_staged(self._h, _ptr(st), _ptr(sq), n_motifs, m, int(mode), _ptr(rec_off),
                                                                 _ptr(rec_len), rec_off.size, float(thr), cap, _ptr(key), _ptr(cover),
                                                                 _ptr(start), ctypes.byref(k), _ptr(occ), _ptr(windows))
            if rc == E_CAPACITY and capacity is None:
                cap = int(k.value)
                continue
            self._check(rc, k.value)
            k = int(k.value)
            return key[:k].copy(), cover[:k].copy(), start[:k].copy(), occ, windows

    # -- multi-site model on averaged-structure profiles (include/pfmscan.h: pfmscan_multisite_profile_*) ------
    def multisite_profile_dev(self, struct_tables, seq_tables, d_codes, d_profile, profile_dtype, n_pos, d_rec_off, d_rec_len, n_rec, d_lam,
                              d_start, d_cover, d_z=None, d_nsites=None, d_windows=None):
        st, sq = self._profile_tables(struct_tables, seq_tables)
        self._check(self._L.pfmscan_multisite_profile_dev(self._h, _ptr(st), _ptr(sq), st.shape[0], st.shape[1], _ptr(d_codes), _ptr(d_profile),
                                                          int(profile_dtype), int(n_pos), _ptr(d_rec_off), _ptr(d_rec_len), int(n_rec),
                                                          _ptr(d_lam), _ptr(d_start), _ptr(d_cover), _ptr(d_z), _ptr(d_nsites), _ptr(d_windows)))

    def multisite_profile_staged(self, struct_tables, seq_tables, rec_off, rec_len, lam, want_start=True, want_cover=True):
        """-> start, cover float64 [n_motifs][n_pos] aligned with the staged profile (None where not wanted; +0.0 outside the
        records of the table), z, nsites float64 [n_rec][n_motifs], windows int64 [n_rec]; struct_tables [n_motifs][m][7] in the
        profile's stored column order, seq_tables [n_motifs][m][8] | None (joint: the staged codes too), lam float64 [n_rec]"""
        st, sq = self._profile_tables(struct_tables, seq_tables)
        n_motifs, m = st.shape[:2]
        n = int(self._L.pfmscan_staged_positions(self._h))
        if n < 0:
            raise ValueError("no stream staged (call stage first)")
        rec_off, rec_len = self._records(rec_off, rec_len)
        lam = self._lam(lam, rec_off.size)
        start = np.zeros((n_motifs, n), dtype=np.float64) if want_start else None
        cover = np.zeros((n_motifs, n), dtype=np.float64) if want_cover else None
        z, windows = self._occ_windows(rec_off.size, n_motifs)
        nsites = np.zeros_like(z)
        self._check(self._L.pfmscan_multisite_profile_staged(self._h, _ptr(st), _ptr(sq), n_motifs, m, _ptr(rec_off), _ptr(rec_len), rec_off.size,
                                                             _ptr(lam), _ptr(start), _ptr(cover), _ptr(z), _ptr(nsites), _ptr(windows)))
        return start, cover, z, nsites, windows

    def multisite_profile_events_dev(self, struct_tables, seq_tables, d_codes, d_profile, profile_dtype, n_pos, d_rec_off, d_rec_len, n_rec,
                                     d_lam, thr, capacity, d_ev_key, d_ev_cover, d_ev_start, d_ev_count, d_z=None, d_nsites=None, d_windows=None):
        st, sq = self._profile_tables(struct_tables, seq_tables)
        self._check(self._L.pfmscan_multisite_profile_events_dev(self._h, _ptr(st), _ptr(sq), st.shape[0], st.shape[1], _ptr(d_codes),
                                                                 _ptr(d_profile), int(profile_dtype), int(n_pos), _ptr(d_rec_off),
                                                                 _ptr(d_rec_len), int(n_rec), _ptr(d_lam), float(thr), int(capacity),
                                                                 _ptr(d_ev_key), _ptr(d_ev_cover), _ptr(d_ev_start), _ptr(d_ev_count), _ptr(d_z),
                                                                 _ptr(d_nsites), _ptr(d_windows)))

    def multisite_profile_events_staged(self, struct_tables, seq_tables, rec_off, rec_len, lam, thr, capacity=None):
        """the positions of the staged profile whose cover > thr under the multi-site model, decided on the device -> (key int64[k]
        = motif * n_pos + position sorted, cover float64[k], start float64[k], z, nsites float64 [n_rec][n_motifs], windows int64
        [n_rec]).  capacity None: a capacity verdict is answered by one retry with the capacity it names; else CapacityError
        carries it"""
        st, sq = self._profile_tables(struct_tables, seq_tables)
        n_motifs, m = st.shape[:2]
        n = int(self._L.pfmscan_staged_positions(self._h))
        if n < 0:
            raise ValueError("no stream staged (call stage first)")
        rec_off, rec_len = self._records(rec_off, rec_len)
        lam = self._lam(lam, rec_off.size)
        cap = int(capacity) if capacity is not None else max(1024, n // 16)
        while True:
            key = np.empty(cap, dtype=np.int64)
            cover = np.empty(cap, dtype=np.float64)
            start = np.empty(cap, dtype=np.float64)
            z, windows = self._occ_windows(rec_off.size, n_motifs)
            nsites = np.zeros_like(z)
            k = ctypes.c_int64(0)
            rc = self._L.pfmscan_multisite_profile_events_staged(self._h, _ptr(st), _ptr(sq), n_motifs, m, _ptr(rec_off), _ptr(rec_len),
                                                                 rec_off.size, _ptr(lam), float(thr), cap, _ptr(key), _ptr(cover), _ptr(start),
                                                                 ctypes.byref(k), _ptr(z), _ptr(nsites), _ptr(windows))
            if rc == E_CAPACITY and capacity is None:
                cap = int(k.value)
                continue
            self._check(rc, k.value)
            k = int(k.value)
            return key[:k].copy(), cover[:k].copy(), start[:k].copy(), z, nsites, windows

    def time_scan_dev(self, motif, d_codes, d_profile, profile_dtype, n_pos, d_out_seq, d_out_struct,
                      stream=None, warmup=1, iters=5):
        ms = ctypes.c_double(0.0)
        self._check(self._L.pfmscan_time_scan_dev(self._h, motif._h, _ptr(d_codes), _ptr(d_profile), int(profile_dtype),
                                                  int(n_pos), _ptr(d_out_seq), _ptr(d_out_struct), _ptr(stream),
                                                  int(warmup), int(iters), ctypes.byref(ms)))
        return ms.value


class Motif(object):
    """Device-resident PSSM operands: letter table [m][8] and/or structure PSSM [m][7]."""

    def __init__(self, ctx, letter_table=None, struct_pssm=None):
        self._ctx = ctx
        self._L = ctx._L
        lt = None if letter_table is None else np.ascontiguousarray(letter_table, dtype=np.float64)
        sp = None if struct_pssm is None else np.ascontiguousarray(struct_pssm, dtype=np.float64)
        if lt is not None and (lt.ndim != 2 or lt.shape[1] != NCODE):
            raise ValueError("letter_table must be [m][8]")
        if sp is not None and (sp.ndim != 2 or sp.shape[1] != NSTRUCT):
            raise ValueError("struct_pssm must be [m][7]")
        if lt is None and sp is None:
            raise ValueError("motif needs a letter table and/or a structure PSSM")
        if lt is not None and sp is not None and lt.shape[0] != sp.shape[0]:
            raise ValueError("sequence and structure PFMs must have the same width for a combined scan")
        self.m = int((lt if lt is not None else sp).shape[0])
        self.has_letters = lt is not None
        self.has_struct = sp is not None
        h = ctypes.c_void_p()
        ctx._check(self._L.pfmscan_motif_create(ctx._h, _ptr(lt), _ptr(sp), self.m, ctypes.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None) and getattr(self._ctx, "_h", None):
            self._L.pfmscan_motif_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Library(object):
    """n motifs of one width resident on the device for one-pass scans:
    letter_tables [n][m][8] (4-letter alphabet), struct_pssms [n][m][7] or None.
    letter_tables None + struct_pssms: a STRUCTURE-ONLY library (k_profile_lib: every motif in one pass over the profile).
    ``struct_letters`` [n][m][8] (up to 7 letters, fp64 scores) instead of struct_pssms: a LETTER library --
    alone a structure-letter library over one 8-code stream (k_library8), with letter_tables a two-FASTA library over two
    code streams (the structure letters of k_library's survivors)."""

    def __init__(self, ctx, letter_tables, struct_pssms=None, struct_letters=None):
        self._ctx = ctx
        self._L = ctx._L
        lt = None if letter_tables is None else np.ascontiguousarray(letter_tables, dtype=np.float64)
        if lt is not None and (lt.ndim != 3 or lt.shape[2] != NCODE):
            raise ValueError("letter_tables must be [n][m][8]")
        sp = None
        self.letter_kind = struct_letters is not None
        if self.letter_kind:
            if struct_pssms is not None:
                raise ValueError("struct_pssms and struct_letters exclude each other")
            sp = np.ascontiguousarray(struct_letters, dtype=np.float64)
            if sp.ndim != 3 or sp.shape[2] != NCODE or (lt is not None and sp.shape[:2] != lt.shape[:2]):
                raise ValueError("struct_letters must be [n][m][8] with the letter tables' n and m")
        elif struct_pssms is not None:
            sp = np.ascontiguousarray(struct_pssms, dtype=np.float64)
            if sp.ndim != 3 or sp.shape[2] != NSTRUCT or (lt is not None and sp.shape[:2] != lt.shape[:2]):
                raise ValueError("struct_pssms must be [n][m][7] with the letter tables' n and m")
        if lt is None and sp is None:
            raise ValueError("library needs letter tables and/or structure PSSMs")
        shape = (lt if lt is not None else sp).shape
        self.n, self.m = int(shape[0]), int(shape[1])
        self.has_letters = lt is not None
        self.has_struct = sp is not None
        h = ctypes.c_void_p()
        if self.letter_kind:
            ctx._check(self._L.pfmscan_library_create_letters(ctx._h, _ptr(lt), _ptr(sp), self.n, self.m, ctypes.byref(h)))
        else:
            ctx._check(self._L.pfmscan_library_create(ctx._h, _ptr(lt), _ptr(sp), self.n, self.m, ctypes.byref(h)))
        self._h = h

    def thresholds(self, thr_seq, thr_struct=None):
        """scalars or per-motif arrays -> float64 [n] arrays (None for a side the library does not have)"""
        ts = None
        if self.has_letters:
            ts = np.ascontiguousarray(np.broadcast_to(np.asarray(thr_seq, dtype=np.float64), (self.n,)))
        tt = None
        if self.has_struct:
            tt = np.ascontiguousarray(np.broadcast_to(np.asarray(-np.inf if thr_struct is None else thr_struct,
                                                                 dtype=np.float64), (self.n,)))
        return ts, tt

    def info(self):
        n, m, npass, per, eps = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_double()
        self._ctx._check(self._L.pfmscan_library_info(self._h, ctypes.byref(n), ctypes.byref(m), ctypes.byref(npass),
                                                      ctypes.byref(per), ctypes.byref(eps)))
        return {"n_motifs": n.value, "m": m.value, "passes": npass.value, "motifs_per_pass": per.value,
                "max_prefilter_eps": eps.value}

    def last_launches(self):
        """how the last scan of this library ran (pfmscan_library_last_launches): its kernel launches, how many of them ran
        several passes side by side as teams, the most passes in one launch; all 0 before the first scan"""
        n, teams, most = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        self._ctx._check(self._L.pfmscan_library_last_launches(self._h, ctypes.byref(n), ctypes.byref(teams), ctypes.byref(most)))
        return {"n_launches": n.value, "n_team_launches": teams.value, "max_teams": most.value}

    def close(self):
        if getattr(self, "_h", None) and getattr(self._ctx, "_h", None):
            self._L.pfmscan_library_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def credit_table(letter_table, thr_seq, bits=16):
    """Host-only diagnostic (no device needed): the unsigned two-letter credit table the integer prefilters use for
    ONE motif at threshold ``thr_seq`` -> (credits uint16 [ceil(m/2)][16], slack in score units).  ``bits`` = 16, 10
    (the library kernel's twelve-motifs-per-entry form for widths up to 16) or 0 (what the library kernel uses at
    this width).  A window whose credits sum (mod 2**bits) has bit bits - 1 clear cannot be a hit; tests check that
    exhaustively."""
    L = load()
    T = np.ascontiguousarray(letter_table, dtype=np.float64)
    if T.ndim != 2 or T.shape[1] != NCODE:
        raise ValueError("letter_table must be [m][8]")
    m = T.shape[0]
    out = np.zeros(((m + 1) // 2, 16), dtype=np.uint16)
    slack = ctypes.c_double(0.0)
    rc = L.pfmscan_debug_credit_table(_ptr(T), m, float(thr_seq), int(bits), _ptr(out), ctypes.byref(slack))
    if rc != OK:
        raise ValueError("pfmscan_debug_credit_table: bad argument")
    return out, slack.value


def library_sum_thresholds(letter_tables, struct_pssms, thr_seq, thr_sum, row_sum_max):
    """Host-only diagnostic (no device needed): the letters thresholds the library kernel's prefilter is built for under
    joint thresholds ``thr_sum`` on the printed LogOdds.SeqStruct -> float64 [n].  letter_tables [n][m][8], struct_pssms
    [n][m][7], thr_seq / thr_sum scalars or [n], ``row_sum_max`` the profile's row bound (inf: nothing is known about the
    rows -> thr_seq comes back).  Every window that passes all three predicates has float64(seq) > thr_eff."""
    L = load()
    T = np.ascontiguousarray(letter_tables, dtype=np.float64)
    P = np.ascontiguousarray(struct_pssms, dtype=np.float64)
    if T.ndim != 3 or T.shape[2] != NCODE or P.ndim != 3 or P.shape[2] != NSTRUCT or P.shape[:2] != T.shape[:2]:
        raise ValueError("letter_tables must be [n][m][8] and struct_pssms [n][m][7]")
    n, m = T.shape[:2]
    ts = np.ascontiguousarray(np.broadcast_to(np.asarray(thr_seq, dtype=np.float64), (n,)))
    tj = np.ascontiguousarray(np.broadcast_to(np.asarray(thr_sum, dtype=np.float64), (n,)))
    out = np.empty(n, dtype=np.float64)
    rc = L.pfmscan_library_sum_thresholds(_ptr(T), _ptr(P), n, m, _ptr(ts), _ptr(tj), float(row_sum_max), _ptr(out))
    if rc != OK:
        raise ValueError("pfmscan_library_sum_thresholds: bad argument")
    return out


def library8_credits(letter_table, thr):
    """Host-only diagnostic: the single-letter credits k_library8 uses for ONE motif of a structure-letter library
    -> (credits uint16 [4 ceil(m/4)][8], slack in score units; inf: no prefilter for this motif)"""
    L = load()
    T = np.ascontiguousarray(letter_table, dtype=np.float64)
    if T.ndim != 2 or T.shape[1] != NCODE:
        raise ValueError("letter_table must be [m][8]")
    rows = (T.shape[0] + 3) // 4 * 4
    out = np.zeros((rows, 8), dtype=np.uint16)
    slack = ctypes.c_double(0.0)
    L.pfmscan_debug_library8_credits.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]
    rc = L.pfmscan_debug_library8_credits(_ptr(T), T.shape[0], float(thr), _ptr(out), ctypes.byref(slack))
    if rc != OK:
        raise ValueError("pfmscan_debug_library8_credits: bad argument")
    return out, slack.value


def credit8_table(letter_table, thr):
    """Host-only diagnostic: the single-letter credit table of k_letters_cred8 for ONE generic-alphabet motif (width <= 32)
    -> (credits uint16 [m][8], mode).  mode 1: used; 2: dense threshold (exact kernel instead); 3: no prefilter possible."""
    L = load()
    T = np.ascontiguousarray(letter_table, dtype=np.float64)
    if T.ndim != 2 or T.shape[1] != NCODE:
        raise ValueError("letter_table must be [m][8]")
    out = np.zeros((T.shape[0], 8), dtype=np.uint16)
    mode = ctypes.c_int(0)
    rc = L.pfmscan_debug_credit8_table(_ptr(T), T.shape[0], float(thr), _ptr(out), ctypes.byref(mode))
    if rc != OK:
        raise ValueError("pfmscan_debug_credit8_table: bad argument")
    return out, mode.value


def _stream_args(motif, codes, profile):
    if motif.has_letters:
        if codes is None:
            raise ValueError("motif has a letter table: codes required")
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        n = codes.size
    dt = PROFILE_NONE
    if motif.has_struct:
        if profile is None:
            raise ValueError("motif has a structure PSSM: profile required")
        if profile.dtype == np.float32:
            dt = PROFILE_F32
        elif profile.dtype == np.float64:
            dt = PROFILE_F64
        else:
            raise ValueError("profile must be float32 or float64")
        profile = np.ascontiguousarray(profile)
        if profile.ndim != 2 or profile.shape[1] != NSTRUCT:
            raise ValueError("profile must be [n_pos][7]")
        if motif.has_letters and profile.shape[0] != n:
            raise ValueError("codes and profile disagree on n_pos")
        n = profile.shape[0]
    else:
        profile = None
    return n, (codes if motif.has_letters else None), profile, dt
