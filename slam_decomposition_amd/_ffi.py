"""ctypes binding of ``libslamhip.so`` (C ABI: ``include/slam_hip.h``).

No torch, no NumPy-on-CPU fallback: if the shared library is missing or no GPU
is usable every entry point raises -- the product path never computes on the
host.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# SLAM_HIP_LIB selects another build of the same library (kernel A/B experiments); never a fallback
LIB_PATH = os.environ.get("SLAM_HIP_LIB") or os.path.join(_HERE, "lib", "libslamhip.so")

ABI_VERSION = 7  # include/slam_hip.h: SLAM_ABI_VERSION
MAX_SPAN_QUAD = 5  # SLAM_MAX_SPAN_QUAD: the register-resident kernels
MAX_SPAN_EVAL = 16
MAX_SPAN_MINIMIZE = 16

ST_CONVERGED, ST_MAXITER, ST_LINESEARCH, ST_NONFINITE, ST_STALLED, ST_PREEMPTED = range(6)
FLAG_EARLY_EXIT = 1
FLAG_ORDERED = 2  # with EARLY_EXIT: the lowest-index successful restart wins (reference semantics, reproducible)
FLAG_STAGED = 4  # span loops: never use the one-wavefront-per-target kernel (small batches)
FLAG_OVERLAP = 8  # SLAM_FLAG_OVERLAP: the spans of a loop side by side whatever the call's size
FLAG_NO_OVERLAP = 16  # SLAM_FLAG_NO_OVERLAP: not even for medium calls (several calls in flight on the device)
FLAG_NO_EXTERIOR = 32  # SLAM_FLAG_NO_EXTERIOR: CircuitTemplate(no_exterior_1q=True) -- layers 0 and k pinned at the identity
MAX_MAXITER = 4000
V2_MAX_SPAN = 5
SMUSH_MAX_SLICES = 58  # SLAM_SMUSH_MAX_SLICES
SMUSH_RAW = 2 + 2 * SMUSH_MAX_SLICES
SMUSH_MAX_SPAN = 6
SMUSH_MAX_N = 128
OP_SUM, OP_MAX, OP_MIN = 0, 2, 3
COMM_ID_BYTES = 128
COST_BASIC, COST_SQUARE, COST_MAKHLIN = 0, 1, 2
COST_MUTUAL_INFO, COST_MUTUAL_INFO_SQUARE = 3, 4  # the state objectives: slam_q3s_eval / slam_q3s_minimize only
PD_MAX_SPAN = 8  # SLAM_PD_MAX_SPAN
PD_MAX_SLICES = 16  # SLAM_PD_MAX_SLICES
PD_MAX_DIRS = 1024  # SLAM_PD_MAX_DIRS
REGION_MAX = 256  # SLAM_REGION_MAX
FAMILY_MAX_MEMBERS = 32  # SLAM_FAMILY_MAX_MEMBERS
FAMILY_MAX_BINS = 8192  # slam_family_lookup: E + E_0 + 4 histogram bins at most
CANDIDATE_MAX_K = 64  # SLAM_CANDIDATE_MAX_K
CANDIDATE_MAX_GATES = 65536  # SLAM_CANDIDATE_MAX_GATES
POLICY_REFERENCE, POLICY_BEST = 0, 1  # slam_family_lookup: the reference's walk / the cheapest member

# every symbol include/slam_hip.h declares (checked by tests/test_abi.py)
EXPORTED_SYMBOLS = (
    "slam_last_error",
    "slam_version",
    "slam_abi_version",
    "slam_hw_queues_requested",
    "slam_device_count",
    "slam_ctx_create",
    "slam_ctx_destroy",
    "slam_ctx_device_info",
    "slam_set_targets",
    "slam_set_gates",
    "slam_c1c2c3",
    "slam_targets_c1c2c3",
    "slam_kak",
    "slam_targets_kak",
    "slam_complete_locals",
    "slam_sqiswap_decompose",
    "slam_cx_decompose",
    "slam_b_decompose",
    "slam_approx_decompose",
    "slam_approx_counts",
    "slam_sc_decompose",
    "slam_sc_counts",
    "slam_sqiswap_approx_decompose",
    "slam_sqiswap_approx_counts",
    "slam_predict_spans",
    "slam_coverage_lookup",
    "slam_family_lookup",
    "slam_candidate_scores",
    "slam_eval_c1c2c3",
    "slam_sample_haar",
    "slam_sample_haar_indexed",
    "slam_haar_select_spans",
    "slam_get_targets",
    "slam_eval_loss_grad",
    "slam_eval_unitary",
    "slam_minimize_stage",
    "slam_decompose",
    "slam_decompose_resident",
    "slam_fetch_results",
    "slam_decompose_range",
    "slam_decompose_list",
    "slam_decompose_predicted",
    "slam_decompose_multi",
    "slam_decompose_range_fetch",
    "slam_fetch_results_range",
    "slam_fetch_span_losses",
    "slam_minimize_stage_trace",
    "slam_v2_set_gates",
    "slam_v2_set_constraint",
    "slam_v2_eval_loss_grad",
    "slam_v2_minimize_stage",
    "slam_v2_minimize_stage_trace",
    "slam_v2_decompose_range",
    "slam_smush_set_gates",
    "slam_smush_eval_loss_grad",
    "slam_smush_minimize_stage",
    "slam_smush_minimize_stage_trace",
    "slam_pd_sample",
    "slam_pd_extremes",
    "slam_pd_filter",
    "slam_region_lookup",
    "slam_q3_eval",
    "slam_q3_minimize",
    "slam_q3m_eval",
    "slam_q3m_minimize",
    "slam_q3s_eval",
    "slam_q3s_minimize",
    "slam_ham_eval",
    "slam_ham_minimize",
    "slam_hams_eval",
    "slam_hams_minimize",
    "slam_set_cost",
    "slam_synchronize",
    "slam_host_alloc",
    "slam_host_free",
    "slam_get_stats",
    "slam_reset_stats",
    "slam_best_loss_device_ptr",
    "slam_metric_update_check",
    "slam_ctx_device",
    "slam_comm_get_unique_id",
    "slam_comm_init",
    "slam_comm_destroy",
    "slam_comm_rank",
    "slam_comm_allreduce_f64",
    "slam_comm_barrier",
    "slam_comm_merge_begin",
    "slam_comm_merge_add",
    "slam_comm_merge_add_host",
    "slam_allreduce_min",
)


class SlamHipError(RuntimeError):
    """A libslamhip call returned a negative SLAM_ERR_* code."""

    def __init__(self, code: int, message: str):
        super().__init__(f"libslamhip error {code}: {message}")
        self.code = code


class OptParams(C.Structure):
    _fields_ = [
        ("restarts", C.c_int32),
        ("maxiter", C.c_int32),
        ("gtol", C.c_double),
        ("stop_loss", C.c_double),
        ("seed", C.c_uint64),
        ("flags", C.c_uint32),
        ("items_per_quad", C.c_uint32),
        ("gtol_far", C.c_double),
        ("far_loss", C.c_double),
        ("target_base", C.c_int64),
    ]

    def __init__(self, restarts=5, maxiter=2500, gtol=1e-9, stop_loss=1e-13, seed=0, flags=0, gtol_far=1e-5, far_loss=1e-6,
                 items_per_quad=0, target_base=0):
        super().__init__(int(restarts), int(maxiter), float(gtol), float(stop_loss), int(seed) & 0xFFFFFFFFFFFFFFFF,
                         int(flags), int(items_per_quad), float(gtol_far), float(far_loss), int(target_base))

    def replace(self, **changes) -> "OptParams":
        """A copy with every field carried over and the named ones changed."""
        return OptParams(**{**{name: getattr(self, name) for name, _ in self._fields_}, **changes})


class V2Gate(C.Structure):
    """``slam_v2_gate``: raw angles (a, phi_c, b, phi_g)[r] = scale[r] * q[sel[r]] + offset[r] of a conversion-gain gate."""

    _fields_ = [("n_params", C.c_int32), ("sel", C.c_int32 * 4), ("scale", C.c_double * 4), ("offset", C.c_double * 4)]

    def __init__(self, n_params, sel, scale, offset):
        super().__init__(int(n_params), (C.c_int32 * 4)(*[int(v) for v in sel]), (C.c_double * 4)(*[float(v) for v in scale]),
                         (C.c_double * 4)(*[float(v) for v in offset]))


class SmushGate(C.Structure):
    """``slam_smush_gate``: raw pulse values (gc, gg, gx[0..N), gy[0..N))[r] = scale[r] * q[sel[r]] + offset[r] of a smush gate
    with N slices of pulse time t (phases folded into the signs of gc / gg)."""

    _fields_ = [("n_params", C.c_int32), ("n_slices", C.c_int32), ("t", C.c_double), ("sel", C.c_int32 * SMUSH_RAW),
                ("scale", C.c_double * SMUSH_RAW), ("offset", C.c_double * SMUSH_RAW)]

    def __init__(self, n_params, n_slices, t, sel, scale, offset):
        nr = 2 + 2 * int(n_slices)
        if not (len(sel) == len(scale) == len(offset) == nr) or nr > SMUSH_RAW:
            raise ValueError(f"a smush gate of {n_slices} slices has {nr} raw values (at most {SMUSH_RAW})")
        pad = SMUSH_RAW - nr
        super().__init__(int(n_params), int(n_slices), float(t), (C.c_int32 * SMUSH_RAW)(*([int(v) for v in sel] + [-1] * pad)),
                         (C.c_double * SMUSH_RAW)(*([float(v) for v in scale] + [0.0] * pad)),
                         (C.c_double * SMUSH_RAW)(*([float(v) for v in offset] + [0.0] * pad)))


class Stats(C.Structure):
    _fields_ = [
        ("kernel_ms", C.c_double),
        ("kernel_launches", C.c_int64),
        ("evals", C.c_int64 * (MAX_SPAN_EVAL + 1)),
        ("items", C.c_int64 * (MAX_SPAN_EVAL + 1)),
        ("total_ms", C.c_double),
        ("kernel_ms_span", C.c_double * (MAX_SPAN_EVAL + 1)),
        ("wave_rounds", C.c_int64 * (MAX_SPAN_EVAL + 1)),
        ("evals_accepted", C.c_int64 * (MAX_SPAN_EVAL + 1)),
        ("evals_preempted", C.c_int64 * (MAX_SPAN_EVAL + 1)),
    ]


_lib = None


def load_library() -> C.CDLL:
    """Load libslamhip.so (built in-tree by ``__graft_entry__.build()`` / ``make``)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `make` (hipcc --offload-arch=gfx950); "
            "slam_decomposition_amd has no CPU fallback"
        )
    lib = C.CDLL(LIB_PATH)
    P = C.c_void_p
    dp = np.ctypeslib.ndpointer
    lib.slam_last_error.restype = C.c_char_p
    lib.slam_version.restype = C.c_char_p
    variant = "SLAM_HIP_LIB" in os.environ  # an A/B build selected by a dev tool: older entry points are tolerated
    if hasattr(lib, "slam_abi_version"):
        lib.slam_abi_version.restype = C.c_int
        abi = int(lib.slam_abi_version())
    else:
        abi = 0
    if abi != ABI_VERSION and not variant:
        raise ImportError(f"{LIB_PATH}: binary interface revision {abi}, this binding is written for {ABI_VERSION} (include/slam_hip.h: "
                          "SLAM_ABI_VERSION): rebuild the library with `make`")
    if hasattr(lib, "slam_hw_queues_requested"):
        lib.slam_hw_queues_requested.argtypes = []
    lib.slam_device_count.argtypes = [C.POINTER(C.c_int)]
    lib.slam_ctx_create.argtypes = [C.c_int, C.POINTER(P)]
    lib.slam_ctx_destroy.argtypes = [P]
    lib.slam_ctx_device_info.argtypes = [P, C.c_char_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.slam_set_targets.argtypes = [P, P, C.c_int64]
    lib.slam_set_gates.argtypes = [P, P, C.c_int32]
    lib.slam_c1c2c3.argtypes = [P, P, C.c_int64, C.c_int32, P]
    lib.slam_targets_c1c2c3.argtypes = [P, C.c_int64, C.c_int64, C.c_int32, P]
    if hasattr(lib, "slam_kak"):
        lib.slam_kak.argtypes = [P, P, C.c_int64] + [P] * 6
        lib.slam_targets_kak.argtypes = [P, C.c_int64, C.c_int64] + [P] * 6
        lib.slam_complete_locals.argtypes = [P, C.c_int, P, P, P, C.c_int64, P, P, P]
    if hasattr(lib, "slam_sqiswap_decompose"):
        lib.slam_sqiswap_decompose.argtypes = [P, C.c_int64, C.c_int64, P, P, P, P]
    if hasattr(lib, "slam_cx_decompose"):
        lib.slam_cx_decompose.argtypes = [P, C.c_int64, C.c_int64, C.c_int, P, P, P, P, P, P]
    if hasattr(lib, "slam_b_decompose"):
        lib.slam_b_decompose.argtypes = [P, C.c_int64, C.c_int64, P, P, P, P, P, P]
    if hasattr(lib, "slam_approx_decompose"):
        lib.slam_approx_decompose.argtypes = [P, C.c_int64, C.c_int64, C.c_int, P, P, C.c_double, C.c_int, P, P, P, P, P]
        lib.slam_approx_counts.argtypes = [P, C.c_int64, C.c_int64, C.c_int, C.c_int32, P, P, P]
    if hasattr(lib, "slam_sc_decompose"):
        lib.slam_sc_decompose.argtypes = [P, C.c_int64, C.c_int64, P, P, C.c_double, C.c_int, P, P, P, P, P]
        lib.slam_sc_counts.argtypes = [P, C.c_int64, C.c_int64, P, P, C.c_int32, P, P, P]
    if hasattr(lib, "slam_sqiswap_approx_decompose"):
        lib.slam_sqiswap_approx_decompose.argtypes = [P, C.c_int64, C.c_int64, C.c_double, C.c_int, P, P, P, P, P]
        lib.slam_sqiswap_approx_counts.argtypes = [P, C.c_int64, C.c_int64, C.c_int32, P, P, P]
    lib.slam_predict_spans.argtypes = [P, C.c_int64, C.c_int64, C.c_int32, P, P, C.c_double, P]
    if hasattr(lib, "slam_coverage_lookup"):
        lib.slam_coverage_lookup.argtypes = [P, C.c_int64, C.c_int64, C.c_int32, P, P, P, P, C.c_double, P, P]
    if hasattr(lib, "slam_family_lookup"):
        lib.slam_family_lookup.argtypes = [P, C.c_int64, C.c_int64, C.c_int32] + [P] * 7 + [C.c_double, C.c_double, C.c_int32] + [P] * 4
    if hasattr(lib, "slam_candidate_scores"):
        lib.slam_candidate_scores.argtypes = [P, C.c_int64, C.c_int64, C.c_int32, P, C.c_int32, C.c_double, P, C.c_int32, P, P, P]
    lib.slam_eval_c1c2c3.argtypes = [P, C.c_int32, P, P, C.c_int64, C.c_int32, P]
    lib.slam_sample_haar.argtypes = [P, C.c_uint64, C.c_int64, C.c_int64]
    if hasattr(lib, "slam_haar_select_spans"):
        lib.slam_sample_haar_indexed.argtypes = [P, C.c_uint64, P, C.c_int64]
        lib.slam_haar_select_spans.argtypes = [P, C.c_uint64, C.c_int64, C.c_int64, C.c_int32, P, P, C.c_double, C.c_double, C.c_int32,
                                               C.c_int32, C.c_int64, C.POINTER(C.c_int64), P, P]
    lib.slam_get_targets.argtypes = [P, C.c_int64, C.c_int64, P]
    lib.slam_eval_loss_grad.argtypes = [P, C.c_int, P, P, P, C.c_int64, P, P]
    lib.slam_eval_unitary.argtypes = [P, C.c_int, P, P, P, C.c_int64, P, P]
    lib.slam_minimize_stage.argtypes = [P, C.c_int, P, P, C.c_int64, P, C.POINTER(OptParams)] + [P] * 7
    lib.slam_decompose.argtypes = [P, C.c_int, C.c_int, P, C.POINTER(OptParams), C.c_double, P, P, P]
    lib.slam_decompose_resident.argtypes = [P, C.c_int, C.c_int, P, C.POINTER(OptParams), C.c_double]
    lib.slam_fetch_results.argtypes = [P, C.c_int, P, P, P]
    lib.slam_decompose_range.argtypes = [P, C.c_int64, C.c_int64, C.c_int, C.c_int, P, C.POINTER(OptParams), C.c_double]
    if hasattr(lib, "slam_decompose_range_fetch"):  # (absent from older A/B builds selected with SLAM_HIP_LIB)
        lib.slam_decompose_range_fetch.argtypes = [P, C.c_int64, C.c_int64, C.c_int, C.c_int, P, C.POINTER(OptParams), C.c_double, P, P, P]
    lib.slam_decompose_list.argtypes = [P, P, C.c_int64, C.c_int, C.c_int, C.c_int, P, C.POINTER(OptParams), C.c_double]
    lib.slam_decompose_predicted.argtypes = [P, C.c_int64, C.c_int64, C.c_int, P, P, C.c_double, C.c_int, P, C.POINTER(OptParams), C.c_double, P, P]
    if hasattr(lib, "slam_decompose_multi"):
        lib.slam_decompose_multi.argtypes = [C.POINTER(P), C.c_int32, C.c_int64, C.c_int64, C.c_int, C.c_int, P, C.POINTER(OptParams), C.c_double]
    lib.slam_fetch_results_range.argtypes = [P, C.c_int, C.c_int64, C.c_int64, P, P, P]
    if hasattr(lib, "slam_minimize_stage_trace"):
        lib.slam_fetch_span_losses.argtypes = [P, C.c_int64, C.c_int64, P]
        lib.slam_minimize_stage_trace.argtypes = [P, C.c_int, P, P, C.c_int64, P, C.POINTER(OptParams), C.c_double, C.c_int32] + [P] * 8
    if hasattr(lib, "slam_v2_set_gates"):
        lib.slam_v2_set_gates.argtypes = [P, C.POINTER(V2Gate), C.c_int32]
        if hasattr(lib, "slam_v2_set_constraint"):
            lib.slam_v2_set_constraint.argtypes = [P, C.c_int, P, C.c_int, C.c_double]
        lib.slam_v2_eval_loss_grad.argtypes = [P, C.c_int, P, P, P, C.c_int64, P, P, P]
        lib.slam_v2_minimize_stage.argtypes = [P, C.c_int, P, P, C.c_int64, P, P, P, P, P, C.POINTER(OptParams), C.c_double] + [P] * 7
        if hasattr(lib, "slam_v2_decompose_range"):
            lib.slam_v2_decompose_range.argtypes = [P, C.c_int64, C.c_int64, C.c_int, C.c_int, P, P, P, P, P, C.POINTER(OptParams), C.c_double, P, P, P]
        if hasattr(lib, "slam_v2_minimize_stage_trace"):
            lib.slam_v2_minimize_stage_trace.argtypes = [P, C.c_int, P, P, C.c_int64, P, P, P, P, P, C.POINTER(OptParams), C.c_double, C.c_int32] + [P] * 8
    if hasattr(lib, "slam_smush_set_gates"):
        lib.slam_smush_set_gates.argtypes = [P, C.POINTER(SmushGate), C.c_int32]
        lib.slam_smush_eval_loss_grad.argtypes = [P, C.c_int, P, P, P, C.c_int64, P, P, P]
        lib.slam_smush_minimize_stage.argtypes = [P, C.c_int, P, P, C.c_int64, P, P, P, P, P, C.POINTER(OptParams), C.c_double] + [P] * 7
        lib.slam_smush_minimize_stage_trace.argtypes = [P, C.c_int, P, P, C.c_int64, P, P, P, P, P, C.POINTER(OptParams), C.c_double, C.c_int32] + [P] * 8
    if hasattr(lib, "slam_pd_sample"):
        lib.slam_pd_sample.argtypes = [P, C.c_double, C.c_double, C.c_double, C.c_int32, C.c_int32, C.c_double, C.c_uint64, C.c_int64, C.c_int64,
                                       P, C.c_int, P, P, P]
        lib.slam_pd_extremes.argtypes = [P, P, C.c_int32, P, P]
        lib.slam_pd_filter.argtypes = [P, P, C.c_int32, C.c_double, C.c_int64, C.POINTER(C.c_int64), P, P]
        lib.slam_region_lookup.argtypes = [P, C.c_int64, C.c_int64, C.c_int32, P, P, P, P, P, C.c_double, P]
    if hasattr(lib, "slam_q3_eval"):
        lib.slam_q3_eval.argtypes = [P, P, C.c_int32, C.c_int32, P, P, P, C.c_int64, P, P, C.c_int64, C.c_int32, P, P, P]
        lib.slam_q3_minimize.argtypes = [P, P, C.c_int32, C.c_int32, P, P, P, C.c_int64, C.c_int32, C.POINTER(OptParams), C.c_double] + [P] * 10
    if hasattr(lib, "slam_q3m_eval"):
        lib.slam_q3m_eval.argtypes = [P, P, C.c_int32, P, C.c_int32, C.c_int32, P, P, P, P, C.c_int64, P, P, C.c_int64, C.c_int32, P, P, P]
        lib.slam_q3m_minimize.argtypes = ([P, P, C.c_int32, P, C.c_int32, C.c_int32, P, P, P, P, C.c_int64, C.c_int32, C.POINTER(OptParams),
                                           C.c_double] + [P] * 10)
    if hasattr(lib, "slam_q3s_eval"):
        lib.slam_q3s_eval.argtypes = lib.slam_q3m_eval.argtypes
        lib.slam_q3s_minimize.argtypes = lib.slam_q3m_minimize.argtypes
    if hasattr(lib, "slam_ham_eval"):
        ham = [P, C.c_int32, C.c_int32, C.c_int32, P, P, P, C.c_int32, P, C.c_int64]
        lib.slam_ham_eval.argtypes = ham + [P, P, C.c_int64, C.c_int32, P, P, P]
        lib.slam_ham_minimize.argtypes = ham + [C.c_int32, C.POINTER(OptParams), C.c_double] + [P] * 10
    if hasattr(lib, "slam_hams_eval"):
        hams = [P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, P, P, P, C.c_int32, P, C.c_int64]
        lib.slam_hams_eval.argtypes = hams + [P, P, C.c_int64, C.c_int32, P, P, P]
        lib.slam_hams_minimize.argtypes = hams + [C.c_int32, C.POINTER(OptParams), C.c_double] + [P] * 10
    lib.slam_set_cost.argtypes = [P, C.c_int]
    lib.slam_synchronize.argtypes = [P]
    if hasattr(lib, "slam_host_alloc"):
        lib.slam_host_alloc.argtypes = [C.c_size_t, C.POINTER(P)]
        lib.slam_host_free.argtypes = [P]
    lib.slam_get_stats.argtypes = [P, C.POINTER(Stats)]
    lib.slam_reset_stats.argtypes = [P]
    lib.slam_best_loss_device_ptr.argtypes = [P, C.POINTER(P), C.POINTER(C.c_int64)]
    lib.slam_metric_update_check.argtypes = [P, C.c_int, P, P, P, P, C.c_int64, P, P]
    if hasattr(lib, "slam_ctx_device"):
        lib.slam_ctx_device.argtypes = [P, C.POINTER(C.c_int)]
    if hasattr(lib, "slam_comm_init") and (abi >= 4 or not variant):  # (older variants: slam_allreduce_min had four arguments)
        lib.slam_comm_get_unique_id.argtypes = [P]
        lib.slam_comm_init.argtypes = [C.c_int, C.c_int, C.c_int, P, C.POINTER(P)]
        lib.slam_comm_destroy.argtypes = [P]
        lib.slam_comm_rank.argtypes = [P, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        lib.slam_comm_allreduce_f64.argtypes = [P, P, C.c_int64, C.c_int]
        lib.slam_comm_barrier.argtypes = [P]
        lib.slam_comm_merge_begin.argtypes = [P, C.c_int64]
        lib.slam_comm_merge_add.argtypes = [P, P, C.c_int64, C.c_int64, C.c_int64]
        lib.slam_comm_merge_add_host.argtypes = [P, P, C.c_int64, C.c_int64]
        lib.slam_allreduce_min.argtypes = [P, C.c_double, C.POINTER(C.c_int64), P, C.c_int64]
    for name in EXPORTED_SYMBOLS:
        if "SLAM_HIP_LIB" in os.environ and not hasattr(lib, name):
            continue  # an older A/B build: newer entry points are simply not used
        fn = getattr(lib, name)
        if name not in ("slam_last_error", "slam_version", "slam_abi_version"):
            fn.restype = C.c_int
    _lib = lib
    return lib


def hw_queues_requested() -> int:
    """``slam_hw_queues_requested``: the ``GPU_MAX_HW_QUEUES`` in force after the library's load-time initialiser ran (it raises
    the variable to 16 by itself; ``SLAM_HW_QUEUES=0`` switches that off -> 0).  The change is made in the C environment:
    ``os.environ`` is a snapshot taken at interpreter start and does not show it."""
    return int(load_library().slam_hw_queues_requested())


def _check(rc: int) -> None:
    if rc != 0:
        raise SlamHipError(rc, load_library().slam_last_error().decode("utf-8", "replace"))


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ------------------------------------------------------------------------------------------------
# Result arrays in page-locked memory, recycled (slam_host_alloc, include/slam_hip.h): a result array of a big window (12.6 MB for
# 65 536 x 24 parameters) is a view of a pinned block that goes back to the pool when the last view of it dies -- the device copies
# into it by DMA, and the call's results are never handed back to the C allocator (measured: freeing 12.6 MB arrays that the runtime
# had pinned around a copy stalled the next call's first launches for 13-18 ms).  For ONE blocking call alone on the device
# (``pinned=True``; TemplateOptimizer's single-call path): 18.2 -> 16.9 ms for 65 536 x 32 sqrt(iSWAP).  NOT for several calls in
# flight: the copy into pinned memory is a device-side copy that needs wave slots behind the other calls' persistent kernels, while
# the pageable path's staging runs on the calling host thread beside them (profiles/r5_pinned_results_ab.txt: the driver's command 14.4 -> 14.9 ms
# per step, 327 680 targets through the API 79 -> 82 ms with everything pinned).  Pageable result arrays are recycled the same way
# (``pageable_pool``): with glibc told never to return memory the 327 680-target call went 86-88 -> 79 ms on a box where the default
# allocator had it in its slow mode (tools/r5_malloc_ab.sh); the pool gets that without touching the process's allocator settings.
# ------------------------------------------------------------------------------------------------
class _PoolBlock:
    __slots__ = ("ptr", "cap", "buf", "_pool", "__weakref__")

    def __init__(self, pool, ptr, cap, buf):
        self.ptr, self.cap, self.buf, self._pool = ptr, cap, buf, pool

    @property
    def __array_interface__(self):
        return {"shape": (self.cap,), "typestr": "|u1", "data": (self.ptr, False), "version": 3}

    def __del__(self):
        try:
            self._pool._release(self.ptr, self.cap, self.buf)
        except Exception:  # (interpreter shutdown)
            pass


class ResultPool:
    """Big result arrays as views of recycled blocks: page-locked ones from ``slam_host_alloc`` (``pinned=True``) or ordinary NumPy
    buffers.  A block goes back to the pool when the last view of it dies."""

    MIN_BYTES = 1 << 18           # smaller arrays stay ordinary NumPy arrays (the library stages small fetches itself)
    GRANULE = 1 << 20
    MAX_IDLE_BYTES = 2 << 30      # idle blocks beyond this are given up

    def __init__(self, pinned: bool):
        import threading

        self.pinned = bool(pinned)
        self._lock = threading.RLock()  # (re-entrant: a block's __del__ may run -- garbage collection -- while this thread holds it)
        self._free = {}
        self._idle = 0
        self.allocated = 0        # blocks obtained so far (tests / diagnostics)

    def empty(self, shape, dtype) -> np.ndarray:
        dtype = np.dtype(dtype)
        nbytes = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
        if nbytes < self.MIN_BYTES:
            return np.empty(shape, dtype=dtype)
        cap = -(-nbytes // self.GRANULE) * self.GRANULE
        entry = None
        with self._lock:
            lst = self._free.get(cap)
            if lst:
                entry = lst.pop()
                self._idle -= cap
        if entry is None:
            if self.pinned:
                lib = load_library()
                out = C.c_void_p()
                if not hasattr(lib, "slam_host_alloc") or lib.slam_host_alloc(cap, C.byref(out)) != 0 or not out.value:
                    return np.empty(shape, dtype=dtype)  # (no page-locked memory: pageable results are slower, not wrong)
                entry = (int(out.value), None)
            else:
                buf = np.empty(cap, dtype=np.uint8)
                entry = (buf.ctypes.data, buf)
            self.allocated += 1
        block = _PoolBlock(self, entry[0], cap, entry[1])
        return np.asarray(block)[:nbytes].view(dtype).reshape(shape)

    def _release(self, ptr, cap, buf):
        with self._lock:
            if self._idle + cap <= self.MAX_IDLE_BYTES:
                self._free.setdefault(cap, []).append((ptr, buf))
                self._idle += cap
                return
        if buf is None:
            load_library().slam_host_free(C.c_void_p(ptr))


PinnedPool = ResultPool  # (name of the first version, tests)
result_pool = ResultPool(pinned=True)      # ONE blocking call alone on the device (``pinned=True`` below)
pageable_pool = ResultPool(pinned=False)   # everything else


def _result_triple(new, count: int, width: int):
    """``(best_loss [count], best_x [count, width], best_cycles [count])`` of a span loop from the allocator ``new``
    (``result_pool.empty`` / ``pageable_pool.empty``)."""
    return new(count, np.float64), new((count, width), np.float64), new(count, np.int32)


class KakResult(NamedTuple):
    """``U[i] = exp(1j * phase[i]) * kron(a1[i], a2[i]) @ CAN(c[i]) @ kron(b1[i], b2[i])``: phase float64[N], the SU(2) factors
    complex128[N, 2, 2], c float64[N, 3] in units of pi (the chamber point of ``c1c2c3(..., ndigits=-1)``)."""

    phase: np.ndarray
    a1: np.ndarray
    a2: np.ndarray
    c: np.ndarray
    b1: np.ndarray
    b2: np.ndarray


def _mat_to_ri(mats: np.ndarray) -> np.ndarray:
    """complex128[..., 4, 4] -> float64[..., 4, 4, 2] (row-major re, im), contiguous."""
    m = np.ascontiguousarray(np.asarray(mats, dtype=np.complex128))
    if m.shape[-2:] != (4, 4):
        raise ValueError(f"expected 4x4 matrices, got shape {m.shape}")
    return m.view(np.float64).reshape(m.shape + (2,))


def device_count() -> int:
    n = C.c_int(0)
    _check(load_library().slam_device_count(C.byref(n)))
    return n.value


def _span_half_spaces(gate_coords_seq, k_max: int):
    """What slam_predict_spans / slam_haar_select_spans take for a gate sequence: the first gate's alcove point [4] and the half-spaces
    of the prefixes g_1 .. g_k, k = 2 .. k_max, as rows k - 1 of [k_max, 14] (coverage.region)."""
    from . import coverage

    g = np.asarray(gate_coords_seq, dtype=np.float64).reshape(-1, 3)
    if not 1 <= k_max <= min(len(g), MAX_SPAN_EVAL):
        raise ValueError(f"k_max must be 1..{min(len(g), MAX_SPAN_EVAL)}")
    point = np.ascontiguousarray(coverage.alcove_coordinates(g[:1])[0])
    bounds = np.full((k_max, len(coverage._PATTERNS)), -np.inf)
    for k in range(2, k_max + 1):
        bounds[k - 1] = coverage.region(g[:k])
    return point, bounds


_POLICIES = {"reference": POLICY_REFERENCE, "best": POLICY_BEST, POLICY_REFERENCE: POLICY_REFERENCE, POLICY_BEST: POLICY_BEST}


def family_arguments(tables, child_even, child_odd, durations, cost_1q, policy):
    """What slam_family_lookup takes for a gate family, checked here as the library checks it (no device is needed to be told of a
    malformed family): ``(offsets, kinds, points, bounds, child_even, child_odd, durations, cost_1q, policy)``.  ``tables``: one object
    per member with ``kinds`` / ``points`` / ``bounds`` as ``Context.coverage_lookup`` reads them, row j = j + 1 applications."""
    tables = list(tables)
    n = len(tables)
    if not 1 <= n <= FAMILY_MAX_MEMBERS:
        raise ValueError(f"a family has 1..{FAMILY_MAX_MEMBERS} members (got {n})")
    if policy not in _POLICIES:
        raise ValueError(f"policy must be 'reference' or 'best' (got {policy!r})")
    sizes = [len(np.asarray(t.kinds).reshape(-1)) for t in tables]
    if min(sizes) < 1:
        raise ValueError("every member needs at least one row")
    offsets = np.zeros(n + 1, dtype=np.int32)
    offsets[1:] = np.cumsum(sizes)
    if int(offsets[-1]) + sizes[0] + 4 > FAMILY_MAX_BINS:
        raise ValueError(f"too many coverage rows ({int(offsets[-1])})")
    kinds = np.ascontiguousarray(np.concatenate([np.asarray(t.kinds, dtype=np.int32).reshape(-1) for t in tables]))
    points = [np.asarray(t.points, dtype=np.float64) for t in tables]
    bounds = [np.asarray(t.bounds, dtype=np.float64) for t in tables]
    for m, (s, p, b) in enumerate(zip(sizes, points, bounds)):
        if p.shape != (s, 4) or b.shape != (s, 14):
            raise ValueError(f"member {m}: points must have shape [{s}, 4] and bounds [{s}, 14] (got {p.shape}, {b.shape})")
    if np.any((kinds != 0) & (kinds != 1)):
        raise ValueError("kinds must be 0 (one gate) or 1 (half-spaces)")
    links = []
    for name, child in (("child_even", child_even), ("child_odd", child_odd)):
        c = np.ascontiguousarray(child, dtype=np.int32).reshape(-1)
        if c.shape != (n,):
            raise ValueError(f"{name} must have one entry per member ({n}), got {c.shape[0]}")
        bad = np.nonzero((c != -1) & ((c <= np.arange(n)) | (c >= n)))[0]
        if len(bad):
            raise ValueError(f"{name}[{int(bad[0])}] = {int(c[bad[0]])}: a child is -1 or a member behind its parent")
        links.append(c)
    d = np.ascontiguousarray(durations, dtype=np.float64).reshape(-1)
    if d.shape != (n,):
        raise ValueError(f"durations must have one entry per member ({n}), got {d.shape[0]}")
    if not np.all(np.isfinite(d)) or not np.isfinite(cost_1q):
        raise ValueError("durations and cost_1q must be finite")
    return (offsets, kinds, np.ascontiguousarray(np.concatenate(points)), np.ascontiguousarray(np.concatenate(bounds)), links[0], links[1],
            d, float(cost_1q), _POLICIES[policy])


CX_DRESS = 99  # SLAM_CX_DRESS
_CX12 = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1], [0, 0, 1, 0]], dtype=np.complex128)  # control on the high bit
_CX21 = np.array([[1, 0, 0, 0], [0, 0, 0, 1], [0, 0, 1, 0], [0, 1, 0, 0]], dtype=np.complex128)
_SWAP = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1]], dtype=np.complex128)
_CX_CLASSES = ((0.5, 0.0, 0.0), (0.5, 0.5, 0.0))


def _in_class(gate, point):
    """``(is the 4x4 gate of the class of CAN(point)?, its Weyl coordinates)``, judged on the 8-digit coordinates with
    ``span_rules._TOL``."""
    from . import span_rules, weyl

    c = weyl.c1c2c3(np.asarray(gate, dtype=np.complex128))
    f = np.abs(span_rules._fold(c)[0])
    return bool(np.max(np.abs(f - np.array(point))) < span_rules._TOL), c


def _dress_head(gate, check):
    """What ``cx_dress`` and ``b_dress`` start with: the gate as a 4x4 complex128 array, what ``check`` (``cx_family``, ``b_class``)
    says of it, and its ``weyl.kak``."""
    from . import weyl

    g = np.ascontiguousarray(gate, dtype=np.complex128)
    if g.shape != (4, 4):
        raise ValueError("the basis gate must be a 4x4 matrix")
    return g, check(g), weyl.kak(g)


def cx_family(gate) -> int:
    """0 for a 4x4 gate of the CNOT class, 1 for one of the iSWAP class, judged on the 8-digit Weyl coordinates with
    ``span_rules._TOL``; ``ValueError`` (naming the coordinates) for any other gate."""
    for family, ref in enumerate(_CX_CLASSES):
        inside, c = _in_class(gate, ref)
        if inside:
            return family
    raise ValueError(f"the gate is neither of the CNOT class nor of the iSWAP class (Weyl coordinates {tuple(float(v) for v in c)})")


def cx_dress(gate):
    """The host's reduction of a basis gate for slam_cx_decompose (include/slam_hip.h): ``(family, gate [4, 4] complex128,
    dress float64[CX_DRESS])`` from three ``weyl.kak`` calls -- G = e^{i .} (l1 (x) l0) CAN(c) (r1 (x) r0), and CX12, CX21 written
    through D = CAN(class point) (family 0) or SWAP CAN(class point) (family 1), a gate of the CNOT class in both."""
    from . import weyl
    from .gates import canonical_matrix

    g, family, (_, l1, l0, c, r1, r0) = _dress_head(gate, cx_family)
    D = canonical_matrix(*_CX_CLASSES[family])
    if family:
        D = _SWAP @ D
    _, u1, u0, _, v1, v0 = weyl.kak(D)  # D = e^{i .} (u1 (x) u0) CAN(1/2, 0, 0) (v1 (x) v0)
    factors = [l1, l0, r1, r0]
    for cx in (_CX12, _CX21):
        _, a1, a0, _, b1, b0 = weyl.kak(cx)
        factors += [a1 @ u1.conj().T, a0 @ u0.conj().T, v1.conj().T @ b1, v0.conj().T @ b0]
    dress = np.concatenate([np.ascontiguousarray(np.stack(factors), dtype=np.complex128).view(np.float64).ravel(), np.asarray(c, dtype=np.float64)])
    assert dress.shape == (CX_DRESS,)
    return family, g, dress


B_DRESS = 35  # SLAM_B_DRESS
_B_CLASS = (0.5, 0.25, 0.0)


def b_class(gate) -> None:
    """Passes for a 4x4 gate of the B class, judged on the 8-digit Weyl coordinates with ``span_rules._TOL``; ``ValueError`` (naming
    the coordinates) for any other gate."""
    inside, c = _in_class(gate, _B_CLASS)
    if not inside:
        raise ValueError(f"the gate is not of the B class (0.5, 0.25, 0) (Weyl coordinates {tuple(float(v) for v in c)})")


def b_dress(gate):
    """The host's reduction of a basis gate for slam_b_decompose (include/slam_hip.h): ``(gate [4, 4] complex128,
    dress float64[B_DRESS])`` from one ``weyl.kak`` call -- G = e^{i .} (l1 (x) l0) CAN(c) (r1 (x) r0)."""
    g, _, (_, l1, l0, c, r1, r0) = _dress_head(gate, b_class)
    dress = np.concatenate([np.ascontiguousarray(np.stack([l1, l0, r1, r0]), dtype=np.complex128).view(np.float64).ravel(),
                            np.asarray(c, dtype=np.float64)])
    assert dress.shape == (B_DRESS,)
    return g, dress


APPROX_MAX_FID = 64  # slam_approx_counts: fidelities per call
FAMILY_CNOT, FAMILY_ISWAP, FAMILY_B = 0, 1, 2  # slam_approx_decompose, slam_approx_counts


def approx_family(gate) -> int:
    """The family of a 4x4 basis gate for slam_approx_decompose: 0 (CNOT class), 1 (iSWAP class), 2 (B class), found with
    ``cx_family`` and ``b_class``; ``ValueError`` (naming the coordinates) for any other gate."""
    try:
        return cx_family(gate)
    except ValueError:
        pass
    try:
        b_class(gate)
    except ValueError:
        from . import weyl

        c = tuple(float(v) for v in weyl.c1c2c3(np.asarray(gate, dtype=np.complex128)))
        raise ValueError(f"the gate is of none of the CNOT, iSWAP and B classes (Weyl coordinates {c})") from None
    return FAMILY_B


def approx_dress(gate):
    """``(family, gate [4, 4] complex128, dress)`` for slam_approx_decompose: ``cx_dress`` for families 0 and 1, ``b_dress`` for 2."""
    family = approx_family(gate)
    if family == FAMILY_B:
        return (family,) + b_dress(gate)
    return cx_dress(gate)


SC_DRESS = 35  # SLAM_SC_DRESS


def sc_class(gate) -> float:
    """beta of a 4x4 supercontrolled gate, one of the class CAN(1/2, beta, 0) with 0 <= beta <= 1/2 (the CNOT, B and iSWAP classes are
    beta = 0, 1/4, 1/2), judged on the 8-digit Weyl coordinates with ``span_rules._TOL``; ``ValueError`` (naming the coordinates) for
    any other gate."""
    from . import span_rules, weyl

    c = weyl.c1c2c3(np.asarray(gate, dtype=np.complex128))
    f = span_rules._fold(c)[0]
    if not (abs(f[0] - 0.5) < span_rules._TOL and abs(f[2]) < span_rules._TOL):
        raise ValueError(f"the gate is not supercontrolled, of a class (0.5, beta, 0) (Weyl coordinates {tuple(float(v) for v in c)})")
    return float(min(max(f[1], 0.0), 0.5))


def sc_dress(gate):
    """The host's reduction of a basis gate for slam_sc_decompose and slam_sc_counts (include/slam_hip.h): ``(gate [4, 4] complex128,
    dress float64[SC_DRESS])`` from one ``weyl.kak`` call -- G = e^{i .} (l1 (x) l0) CAN(c) (r1 (x) r0)."""
    g, _, (_, l1, l0, c, r1, r0) = _dress_head(gate, sc_class)
    dress = np.concatenate([np.ascontiguousarray(np.stack([l1, l0, r1, r0]), dtype=np.complex128).view(np.float64).ravel(),
                            np.asarray(c, dtype=np.float64)])
    assert dress.shape == (SC_DRESS,)
    return g, dress


def check_basis_fidelity(f) -> float:
    """``f`` as a float in (0, 1]; ``ValueError`` otherwise."""
    f = float(f)
    if not (0.0 < f <= 1.0):  # a NaN fails both
        raise ValueError(f"basis_fidelity must be in (0, 1], got {f}")
    return f


class Context:
    """One GPU: resident targets + gate table + work buffers (``slam_ctx``)."""

    def __init__(self, device: int = 0):
        self._lib = load_library()
        self._h = C.c_void_p()
        _check(self._lib.slam_ctx_create(int(device), C.byref(self._h)))
        self.device = int(device)
        self.n_targets = 0
        self.n_gates = 0

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.slam_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- residency -------------------------------------------------------
    def device_info(self) -> Tuple[str, int, int]:
        buf = C.create_string_buffer(256)
        cu, khz = C.c_int(0), C.c_int(0)
        _check(self._lib.slam_ctx_device_info(self._h, buf, 256, C.byref(cu), C.byref(khz)))
        return buf.value.decode(), cu.value, khz.value

    def set_targets(self, targets: np.ndarray) -> None:
        t = _mat_to_ri(targets)
        if t.ndim != 4:
            raise ValueError("targets must have shape [N, 4, 4]")
        _check(self._lib.slam_set_targets(self._h, _ptr(t), t.shape[0]))
        self.n_targets = t.shape[0]

    def c1c2c3(self, unitaries: np.ndarray, ndigits: int = 8) -> np.ndarray:
        """Weyl coordinates of ``unitaries[N, 4, 4]`` (weylchamber.c1c2c3, basis_abc.py:80-84) -> float64[N, 3]."""
        u = np.ascontiguousarray(unitaries, dtype=np.complex128)
        if u.ndim != 3 or u.shape[1:] != (4, 4):
            raise ValueError("expected an array of shape [N, 4, 4]")
        out = np.zeros((u.shape[0], 3), dtype=np.float64)
        _check(self._lib.slam_c1c2c3(self._h, _ptr(u.view(np.float64)), u.shape[0], int(ndigits), _ptr(out)))
        return out

    def targets_c1c2c3(self, first: int = 0, count: Optional[int] = None, ndigits: int = 8) -> np.ndarray:
        """Weyl coordinates of the resident targets [first, first + count) -> float64[count, 3]."""
        count = self.n_targets - first if count is None else count
        out = np.zeros((count, 3), dtype=np.float64)
        _check(self._lib.slam_targets_c1c2c3(self._h, int(first), int(count), int(ndigits), _ptr(out)))
        return out

    def _kak_call(self, fn, head, count: int) -> KakResult:
        phase = np.zeros(count)
        f = [np.zeros((count, 2, 2), dtype=np.complex128) for _ in range(4)]
        c = np.zeros((count, 3))
        _check(fn(self._h, *head, count, _ptr(phase), _ptr(f[0]), _ptr(f[1]), _ptr(c), _ptr(f[2]), _ptr(f[3])))
        return KakResult(phase, f[0], f[1], c, f[2], f[3])

    def kak(self, unitaries: np.ndarray) -> KakResult:
        """KAK decomposition of ``unitaries[N, 4, 4]`` on the device (slam_kak): a :class:`KakResult`."""
        u = np.ascontiguousarray(unitaries, dtype=np.complex128)
        if u.ndim != 3 or u.shape[1:] != (4, 4):
            raise ValueError("expected an array of shape [N, 4, 4]")
        return self._kak_call(self._lib.slam_kak, (_ptr(u.view(np.float64)),), u.shape[0])

    def targets_kak(self, first: int = 0, count: Optional[int] = None) -> KakResult:
        """KAK decomposition of the resident targets [first, first + count) (slam_targets_kak): a :class:`KakResult`."""
        count = self.n_targets - first if count is None else int(count)
        if first < 0 or count < 0 or first + count > self.n_targets:
            raise ValueError(f"target window [{first}, {first + count}) outside the resident batch of {self.n_targets}")
        return self._kak_call(self._lib.slam_targets_kak, (int(first),), count)

    def complete_locals(self, gate_seq: Sequence[int], x: np.ndarray, target_of: np.ndarray):
        """Local-gate completion (slam_complete_locals): rows ``x[M, 6 (k + 1)]`` whose template unitaries equal the resident targets
        ``target_of[M]`` up to single-qubit gates -> ``(x_out [M, 6 (k + 1)], loss [M], gap [M])``: the rows with the missing local
        gates folded into layers 0 and k, their BasicCost loss against the targets, and the coordinate gap of the fit."""
        k = len(gate_seq)
        n = 6 * (k + 1)
        x = np.ascontiguousarray(x, dtype=np.float64)
        if k < 1 or x.ndim != 2 or x.shape[1] != n:
            raise ValueError(f"x must have shape [M, {n}] for a sequence of {k} gates")
        M = x.shape[0]
        tof = np.ascontiguousarray(target_of, dtype=np.int32)
        if tof.shape != (M,):
            raise ValueError("target_of must have shape [M]")
        gs = np.ascontiguousarray(gate_seq, dtype=np.int32)
        x_out = np.zeros((M, n))
        loss = np.zeros(M)
        gap = np.zeros(M)
        _check(self._lib.slam_complete_locals(self._h, k, _ptr(gs), _ptr(x), _ptr(tof), M, _ptr(x_out), _ptr(loss), _ptr(gap)))
        return x_out, loss, gap

    def _closed_form_call(self, fn, head_args, first: int, count: Optional[int]):
        """``fn(ctx, first, count, *head_args, x, cycles, loss, gap)`` of a closed-form entry point with its four outputs allocated."""
        count = self.n_targets - first if count is None else int(count)
        n = max(count, 0)
        x = np.zeros((n, 24))
        cycles = np.zeros(n, dtype=np.int32)
        loss = np.zeros(n)
        gap = np.zeros(n)
        _check(fn(self._h, int(first), count, *head_args, _ptr(x), _ptr(cycles), _ptr(loss), _ptr(gap)))
        return x, cycles, loss, gap

    def sqiswap_decompose(self, first: int = 0, count: Optional[int] = None):
        """Closed-form circuits of two or three sqrt(iSWAP) gates for the resident targets [first, first + count)
        (slam_sqiswap_decompose; nothing is uploaded, no gate table is needed) -> ``(x [count, 24], cycles [count], loss [count],
        gap [count])``: row i holds the 6 (cycles[i] + 1) template angles of a circuit that equals target first + i up to a phase,
        zeros behind; loss is its BasicCost loss, gap the coordinate gap left by the interior formula (units of pi)."""
        return self._closed_form_call(self._lib.slam_sqiswap_decompose, (), first, count)

    def cx_decompose(self, gate, first: int = 0, count: Optional[int] = None):
        """Closed-form circuits of one, two or three gates ``gate`` -- a 4x4 matrix of the CNOT class or of the iSWAP class -- for the
        resident targets [first, first + count) (slam_cx_decompose; nothing is uploaded, no gate table is needed) -> ``(x [count, 24],
        cycles [count], loss [count], gap [count])``: row i holds the 6 (cycles[i] + 1) template angles of a circuit of ``gate`` that
        equals target first + i up to a phase, zeros behind; loss is its BasicCost loss, gap the coordinate gap left by the alignment
        of the interior circuit (units of pi).  ``ValueError`` for a gate outside both classes (``span_rules._TOL``)."""
        family, g, dress = cx_dress(gate)
        return self._closed_form_call(self._lib.slam_cx_decompose, (family, _ptr(g), _ptr(dress)), first, count)

    def b_decompose(self, gate, first: int = 0, count: Optional[int] = None):
        """Closed-form circuits of one or two gates ``gate`` -- a 4x4 matrix of the B class -- for the resident targets
        [first, first + count) (slam_b_decompose; nothing is uploaded, no gate table is needed) -> ``(x [count, 24], cycles [count],
        loss [count], gap [count])`` as ``cx_decompose`` returns them.  ``ValueError`` for a gate outside the class
        (``span_rules._TOL``)."""
        g, dress = b_dress(gate)
        return self._closed_form_call(self._lib.slam_b_decompose, (_ptr(g), _ptr(dress)), first, count)

    def approx_decompose(self, gate, basis_fidelity: float = 1.0, cycles: Optional[int] = None, first: int = 0, count: Optional[int] = None):
        """Fidelity-aware approximate circuits of ``gate`` -- a 4x4 matrix of the CNOT, the iSWAP or the B class -- for the resident
        targets [first, first + count) (slam_approx_decompose) -> ``(x [count, 24], cycles [count], loss [count], predicted [count],
        gap [count])``: per target the size with the highest expected fidelity when one gate has ``basis_fidelity`` (``cycles=k``: that
        size for every target), the 6 (cycles[i] + 1) angles of the best circuit of that size (one layer for no gate), its BasicCost
        loss from a forward pass, the loss the closed form predicts, and the chamber distance to the nearest reachable point.
        ``ValueError`` for a gate outside the classes, a fidelity outside (0, 1] and a size the family does not have."""
        family, g, dress = approx_dress(gate)
        f = check_basis_fidelity(basis_fidelity)
        k_max = 2 if family == FAMILY_B else 3
        force = -1 if cycles is None else int(cycles)
        if cycles is not None and not 0 <= force <= k_max:
            raise ValueError(f"cycles must be None or 0..{k_max} for this basis gate, got {cycles}")
        count = self.n_targets - first if count is None else int(count)
        n = max(count, 0)
        x = np.zeros((n, 24))
        size = np.zeros(n, dtype=np.int32)
        loss, predicted, gap = np.zeros(n), np.zeros(n), np.zeros(n)
        _check(self._lib.slam_approx_decompose(self._h, int(first), count, family, _ptr(g), _ptr(dress), f, force, _ptr(x), _ptr(size),
                                               _ptr(loss), _ptr(predicted), _ptr(gap)))
        return x, size, loss, predicted, gap

    def approx_counts(self, gate, basis_fidelities, first: int = 0, count: Optional[int] = None):
        """The selection of ``approx_decompose`` for up to ``APPROX_MAX_FID`` basis fidelities in one launch over the resident targets
        [first, first + count) (slam_approx_counts) -> ``(counts int64[n, 4], fidsum int64[n])``: targets per chosen size, and the sum
        of the chosen expected fidelities in units of 2^-32."""
        family = approx_family(np.ascontiguousarray(gate, dtype=np.complex128))
        f = np.ascontiguousarray(basis_fidelities, dtype=np.float64).reshape(-1)
        if not 1 <= len(f) <= APPROX_MAX_FID:
            raise ValueError(f"between 1 and {APPROX_MAX_FID} basis fidelities per call, got {len(f)}")
        for v in f:
            check_basis_fidelity(v)
        count = self.n_targets - first if count is None else int(count)
        counts = np.zeros((len(f), 4), dtype=np.int64)
        fidsum = np.zeros(len(f), dtype=np.int64)
        _check(self._lib.slam_approx_counts(self._h, int(first), count, family, len(f), _ptr(f), _ptr(counts), _ptr(fidsum)))
        return counts, fidsum

    def sc_decompose(self, gate, basis_fidelity: float = 1.0, cycles: Optional[int] = None, first: int = 0, count: Optional[int] = None):
        """``approx_decompose`` for ``gate`` of any supercontrolled class CAN(1/2, beta, 0) (slam_sc_decompose): the same five arrays,
        sizes 0..3 for every beta.  ``ValueError`` for a gate off that line, a fidelity outside (0, 1] and a size outside 0..3."""
        g, dress = sc_dress(gate)
        f = check_basis_fidelity(basis_fidelity)
        force = -1 if cycles is None else int(cycles)
        if cycles is not None and not 0 <= force <= 3:
            raise ValueError(f"cycles must be None or 0..3, got {cycles}")
        predicted = np.zeros(max(self.n_targets - first if count is None else int(count), 0))

        def fn(h, first, count, x, size, loss, gap):  # the four outputs of _closed_form_call, `predicted` between loss and gap
            return self._lib.slam_sc_decompose(h, first, count, _ptr(g), _ptr(dress), f, force, x, size, loss, _ptr(predicted), gap)

        x, size, loss, gap = self._closed_form_call(fn, (), first, count)
        return x, size, loss, predicted, gap

    def sc_counts(self, gate, basis_fidelities, first: int = 0, count: Optional[int] = None):
        """``approx_counts`` for ``gate`` of any supercontrolled class (slam_sc_counts) -> ``(counts int64[n, 4], fidsum int64[n])``."""
        g, dress = sc_dress(gate)
        f = np.ascontiguousarray(basis_fidelities, dtype=np.float64).reshape(-1)
        if not 1 <= len(f) <= APPROX_MAX_FID:
            raise ValueError(f"between 1 and {APPROX_MAX_FID} basis fidelities per call, got {len(f)}")
        for v in f:
            check_basis_fidelity(v)
        count = self.n_targets - first if count is None else int(count)
        counts = np.zeros((len(f), 4), dtype=np.int64)
        fidsum = np.zeros(len(f), dtype=np.int64)
        _check(self._lib.slam_sc_counts(self._h, int(first), count, _ptr(g), _ptr(dress), len(f), _ptr(f), _ptr(counts), _ptr(fidsum)))
        return counts, fidsum

    def sqiswap_approx_decompose(self, basis_fidelity: float = 1.0, cycles: Optional[int] = None, first: int = 0, count: Optional[int] = None):
        """``approx_decompose`` for sqrt(iSWAP) = ``RiSwapGate(1/2)`` (slam_sqiswap_approx_decompose; no gate is uploaded): the same five
        arrays, sizes 0..3; with ``basis_fidelity=1`` no gate for a local target, one for a target of the gate's class and otherwise the
        sizes of ``sqiswap_decompose``.  ``ValueError`` for a fidelity outside (0, 1] and a size outside 0..3."""
        f = check_basis_fidelity(basis_fidelity)
        force = -1 if cycles is None else int(cycles)
        if cycles is not None and not 0 <= force <= 3:
            raise ValueError(f"cycles must be None or 0..3, got {cycles}")
        predicted = np.zeros(max(self.n_targets - first if count is None else int(count), 0))

        def fn(h, first, count, x, size, loss, gap):  # the four outputs of _closed_form_call, `predicted` between loss and gap
            return self._lib.slam_sqiswap_approx_decompose(h, first, count, f, force, x, size, loss, _ptr(predicted), gap)

        x, size, loss, gap = self._closed_form_call(fn, (), first, count)
        return x, size, loss, predicted, gap

    def sqiswap_approx_counts(self, basis_fidelities, first: int = 0, count: Optional[int] = None):
        """``approx_counts`` for sqrt(iSWAP) (slam_sqiswap_approx_counts) -> ``(counts int64[n, 4], fidsum int64[n])``."""
        f = np.ascontiguousarray(basis_fidelities, dtype=np.float64).reshape(-1)
        if not 1 <= len(f) <= APPROX_MAX_FID:
            raise ValueError(f"between 1 and {APPROX_MAX_FID} basis fidelities per call, got {len(f)}")
        for v in f:
            check_basis_fidelity(v)
        count = self.n_targets - first if count is None else int(count)
        counts = np.zeros((len(f), 4), dtype=np.int64)
        fidsum = np.zeros(len(f), dtype=np.int64)
        _check(self._lib.slam_sqiswap_approx_counts(self._h, int(first), count, len(f), _ptr(f), _ptr(counts), _ptr(fidsum)))
        return counts, fidsum

    def metric_update_check(self, h: np.ndarray, s: np.ndarray, w: np.ndarray, v: np.ndarray):
        """Device check of the metric's rank-2 update ``H += s w^T + v s^T`` (slam_metric_update_check): ``h[n, na (na + 1) / 2, 4, 4]``
        upper blocks (block (a, b) at b (b + 1) / 2 + a, element [q][e] = H[4a + q][4b + e]) and ``s, w, v [n, 4 na]``, float32, na in
        (3, 5, 6) -> ``(h_shipped, h_vector)``: the update through the form the optimizer kernels run and through the vector form."""
        s = np.ascontiguousarray(s, dtype=np.float32)
        if s.ndim != 2 or s.shape[1] % 4:
            raise ValueError("s must have shape [n, 4 na]")
        n, na = s.shape[0], s.shape[1] // 4
        w = np.ascontiguousarray(w, dtype=np.float32)
        v = np.ascontiguousarray(v, dtype=np.float32)
        h = np.ascontiguousarray(h, dtype=np.float32)
        if w.shape != s.shape or v.shape != s.shape or h.shape != (n, na * (na + 1) // 2, 4, 4):
            raise ValueError(f"w, v must have shape {s.shape} and h [{n}, {na * (na + 1) // 2}, 4, 4]")
        h_shipped = np.zeros_like(h)
        h_vector = np.zeros_like(h)
        _check(self._lib.slam_metric_update_check(self._h, na, _ptr(h), _ptr(s), _ptr(w), _ptr(v), n, _ptr(h_shipped), _ptr(h_vector)))
        return h_shipped, h_vector

    def predict_spans(self, gate_coords_seq, k_max: int, first: int = 0, count: Optional[int] = None, tol: float = 2e-8) -> np.ndarray:
        """Template size every resident target of [first, first + count) needs with the gate sequence whose Weyl coordinates are
        ``gate_coords_seq`` (0 local, 1..k_max, k_max + 1 out of reach): ``coverage.minimal_prefix`` evaluated on the device
        (slam_predict_spans) -- the half-spaces of the sequence's prefixes are computed here, the targets never leave the GPU."""
        point, bounds = _span_half_spaces(gate_coords_seq, k_max)
        count = self.n_targets - first if count is None else count
        out = np.zeros(count, dtype=np.int32)
        _check(self._lib.slam_predict_spans(self._h, int(first), int(count), int(k_max), _ptr(point), _ptr(bounds), float(tol), _ptr(out)))
        return out

    def coverage_lookup(self, tables, first: int = 0, count: Optional[int] = None, want_entries: bool = False, tol: float = 1e-7):
        """First entry of each cost-ordered coverage table that contains each resident target of [first, first + count)
        (slam_coverage_lookup; the targets and their Weyl coordinates stay on the device).  ``tables``: objects with ``kinds``
        (int32 [n]: 0 one gate, 1 half-spaces), ``points`` ([n, 4]) and ``bounds`` ([n, 14]) -- ``basis.CoverageTable``, as
        ``MixedOrderBasisCircuitTemplate.coverage_table`` builds them; ``tol`` is the widening ``CircuitCoverage.inside`` applies
        (``span_rules._TOL`` + its default slack).  Returns ``(counts, entries)``: per table int64 [n + 2] (hits per entry, then local
        targets, then targets no entry contains) and -- with ``want_entries`` -- int32 [n_tables, count] of those bin indices (else
        None), all tables in ONE launch."""
        tables = list(tables)
        if not tables:
            raise ValueError("coverage_lookup needs at least one table")
        count = self.n_targets - first if count is None else int(count)
        sizes = [len(np.asarray(t.kinds)) for t in tables]
        offsets = np.zeros(len(tables) + 1, dtype=np.int32)
        offsets[1:] = np.cumsum(sizes)
        kinds = np.ascontiguousarray(np.concatenate([np.asarray(t.kinds, dtype=np.int32).reshape(-1) for t in tables]))
        points = np.ascontiguousarray(np.concatenate([np.asarray(t.points, dtype=np.float64).reshape(-1, 4) for t in tables]))
        bounds = np.ascontiguousarray(np.concatenate([np.asarray(t.bounds, dtype=np.float64).reshape(-1, 14) for t in tables]))
        counts = np.zeros(int(offsets[-1]) + 2 * len(tables), dtype=np.int64)
        entries = np.zeros((len(tables), max(count, 0)), dtype=np.int32) if want_entries else None
        _check(self._lib.slam_coverage_lookup(self._h, int(first), int(count), len(tables), _ptr(offsets), _ptr(kinds), _ptr(points),
                                              _ptr(bounds), float(tol), _ptr(counts), _ptr(entries)))
        per_table = [counts[int(offsets[t]) + 2 * t : int(offsets[t + 1]) + 2 * (t + 1)] for t in range(len(tables))]
        return per_table, entries

    def family_lookup(self, tables, child_even, child_odd, durations, cost_1q: float = 0.1, policy="reference", first: int = 0,
                      count: Optional[int] = None, want_targets: bool = False, tol: float = 1e-7):
        """The cheapest family member and gate count for each resident target of [first, first + count) (slam_family_lookup; the
        targets stay on the device).  ``tables``: one per member, rows k = 1, 2, ... applications as ``coverage_lookup`` reads them;
        ``child_even`` / ``child_odd`` [n_members]: where the walk goes from a member at an even / odd k (-1: nowhere);
        ``durations`` [n_members]; ``policy``: "reference" (the walk of recursive_sibling_check) or "best" (the cheapest member).
        Returns ``(counts int64[E + 2], base_counts int64[E_0 + 2], members, gates)``: targets per (member, k) row, then local, then
        unreachable ones; the same for member 0 alone; and -- with ``want_targets`` -- int32[count] each (-1 / 0 local, -1 / -1
        unreachable), else None.  Malformed families raise ``ValueError`` before the library is called."""
        offsets, kinds, points, bounds, ce, co, d, c1q, pol = family_arguments(tables, child_even, child_odd, durations, cost_1q, policy)
        count = self.n_targets - first if count is None else int(count)
        counts = np.zeros(int(offsets[-1]) + 2, dtype=np.int64)
        base_counts = np.zeros(int(offsets[1]) + 2, dtype=np.int64)
        members = np.zeros(max(count, 0), dtype=np.int32) if want_targets else None
        gates = np.zeros(max(count, 0), dtype=np.int32) if want_targets else None
        _check(self._lib.slam_family_lookup(self._h, int(first), int(count), len(offsets) - 1, _ptr(offsets), _ptr(kinds), _ptr(points),
                                            _ptr(bounds), _ptr(ce), _ptr(co), _ptr(d), c1q, float(tol), pol, _ptr(counts), _ptr(base_counts),
                                            _ptr(members), _ptr(gates)))
        return counts, base_counts, members, gates

    def candidate_scores(self, coords, k_cap: int, groups=None, n_groups: int = 1, first: int = 0, count: Optional[int] = None,
                         want_first: bool = False, tol: float = 1e-7):
        """First number of applications of every candidate gate that reaches each resident target of [first, first + count)
        (slam_candidate_scores; the device derives the coverage rows from ``coords`` [G, 3], Weyl coordinates in units of pi).
        ``groups``: int32[count] group of every target of the window (None: one group).  Returns ``(counts, first_k)``:
        int64 [n_groups, G, k_cap + 2] -- bin k - 1 targets first reached at k, bin ``k_cap`` local targets, bin ``k_cap + 1`` targets
        not reached -- and, with ``want_first``, int32 [G, count] (k; 0 local; ``k_cap + 1`` not reached), else None.  The device time
        of the call's kernels is left in ``self.last_candidate_kernel_ms``."""
        c = np.ascontiguousarray(coords, dtype=np.float64)
        if c.ndim != 2 or c.shape[1] != 3 or c.shape[0] < 1:
            raise ValueError("coords must be [G, 3] with G >= 1")
        count = self.n_targets - first if count is None else int(count)
        g = None
        if groups is not None:
            g = np.ascontiguousarray(groups, dtype=np.int32).reshape(-1)
            if g.size != max(count, 0):
                raise ValueError(f"groups has {g.size} entries for a window of {count} targets")
        elif int(n_groups) != 1:
            raise ValueError("n_groups != 1 needs groups")
        if int(n_groups) < 1:
            raise ValueError("n_groups must be >= 1")
        counts = np.zeros((int(n_groups), c.shape[0], max(int(k_cap), 0) + 2), dtype=np.int64)
        first_k = np.zeros((c.shape[0], max(count, 0)), dtype=np.int32) if want_first else None
        ms = C.c_double(0.0)
        _check(self._lib.slam_candidate_scores(self._h, int(first), int(count), c.shape[0], _ptr(c), int(k_cap), float(tol), _ptr(g),
                                               int(n_groups), _ptr(counts), _ptr(first_k), C.byref(ms)))
        self.last_candidate_kernel_ms = float(ms.value)
        return counts, first_k

    # -- parallel-drive coverage (slam_pd_*, slam_region_lookup) --------------------------------------------------------------------------
    def pd_sample(self, gc: float, gg: float, t: float, n_slices: int, k: int, n_samples: int, seed: int = 0, bound: float = 4 * np.pi,
                  first_index: int = 0, indices=None, ndigits: int = 8, want_coords: bool = False, want_params: bool = False,
                  want_unitaries: bool = False):
        """``n_samples`` random parallel-drive templates of k gates on the device (slam_pd_sample); their folded Weyl coordinates stay
        resident for ``pd_extremes`` / ``pd_filter``.  ``indices`` (int64[n]) replays chosen samples instead of ``first_index + i``.
        Returns ``(coords [n, 3], params [n, P], unitaries [n, 4, 4])``, each None unless asked for."""
        idx = None
        if indices is not None:
            idx = np.ascontiguousarray(indices, dtype=np.int64).reshape(-1)
            n_samples = idx.size
        n = int(n_samples)
        P = 6 * (int(k) - 1) + int(k) * (2 + 2 * int(n_slices))
        coords = np.zeros((max(n, 0), 3)) if want_coords else None
        params = np.zeros((max(n, 0), max(P, 0))) if want_params else None
        uni = np.zeros((max(n, 0), 4, 4, 2)) if want_unitaries else None
        _check(self._lib.slam_pd_sample(self._h, float(gc), float(gg), float(t), int(n_slices), int(k), float(bound),
                                        int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_index), n, _ptr(idx), int(ndigits), _ptr(coords),
                                        _ptr(params), _ptr(uni)))
        if uni is not None:
            uni = uni[..., 0] + 1j * uni[..., 1]
        return coords, params, uni

    def pd_extremes(self, directions) -> Tuple[np.ndarray, np.ndarray]:
        """The resident sample that is extreme in each direction (slam_pd_extremes): ``(indices int64[D], coords [D, 3])``."""
        d = np.ascontiguousarray(directions, dtype=np.float64).reshape(-1, 3)
        idx = np.zeros(len(d), dtype=np.int64)
        out = np.zeros((len(d), 3))
        _check(self._lib.slam_pd_extremes(self._h, _ptr(d), len(d), _ptr(idx), _ptr(out)))
        return idx, out

    def pd_filter(self, facets, capacity: int, eps: float = 1e-12) -> Tuple[np.ndarray, np.ndarray]:
        """The resident samples not strictly inside every facet ``n . c <= b`` (rows (n, b)) -- slam_pd_filter; sorted by sample
        index: ``(indices int64[m], coords [m, 3])``."""
        f = np.ascontiguousarray(facets, dtype=np.float64).reshape(-1, 4)
        cap = int(capacity)
        idx = np.zeros(cap, dtype=np.int64)
        out = np.zeros((cap, 3))
        m = C.c_int64(0)
        _check(self._lib.slam_pd_filter(self._h, _ptr(f), len(f), float(eps), cap, C.byref(m), _ptr(idx), _ptr(out)))
        if m.value > cap:
            raise RuntimeError(f"pd_filter: {m.value} survivors, capacity {cap}")
        order = np.argsort(idx[: m.value], kind="stable")
        return idx[: m.value][order], out[: m.value][order]

    def region_lookup(self, region_offsets, kinds, facet_offsets, facets, aux=None, first: int = 0, count: Optional[int] = None,
                      tol: float = 1e-7) -> np.ndarray:
        """Resident targets [first, first + count) against unions of polytopes (slam_region_lookup): int64[2 R + 1] -- per region the
        targets inside, then the first-containing-region histogram (last bin: in none)."""
        ro = np.ascontiguousarray(region_offsets, dtype=np.int32).reshape(-1)
        ki = np.ascontiguousarray(kinds, dtype=np.int32).reshape(-1)
        fo = np.ascontiguousarray(facet_offsets, dtype=np.int32).reshape(-1)
        fa = np.ascontiguousarray(facets, dtype=np.float64).reshape(-1, 4)
        ax = None if aux is None else np.ascontiguousarray(aux, dtype=np.float64).reshape(-1, 14)
        count = self.n_targets - first if count is None else int(count)
        R = len(ro) - 1
        counts = np.zeros(2 * max(R, 0) + 1, dtype=np.int64)
        _check(self._lib.slam_region_lookup(self._h, int(first), int(count), R, _ptr(ro), _ptr(ki), _ptr(fo), _ptr(fa), _ptr(ax), float(tol),
                                            _ptr(counts)))
        return counts

    def eval_c1c2c3(self, gate_seq: Sequence[int], x: np.ndarray, ndigits: int = 8) -> np.ndarray:
        """Weyl coordinates of CircuitTemplate.eval(x[m]) for ``x[M, n]`` (optimizer.py:85,103) -> float64[M, 3];
        the unitaries never leave the device."""
        k = len(gate_seq)
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.ndim != 2 or x.shape[1] != 6 * (k + 1):
            raise ValueError(f"x must have shape [M, {6 * (k + 1)}]")
        gs = np.ascontiguousarray(gate_seq, dtype=np.int32)
        out = np.zeros((x.shape[0], 3), dtype=np.float64)
        _check(self._lib.slam_eval_c1c2c3(self._h, k, _ptr(gs), _ptr(x), x.shape[0], int(ndigits), _ptr(out)))
        return out

    def sample_haar(self, seed: int, n_targets: int, first_index: int = 0) -> None:
        """Generate the resident batch on the device: T_i = Haar(seed, first_index + i)."""
        _check(self._lib.slam_sample_haar(self._h, int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_index), int(n_targets)))
        self.n_targets = int(n_targets)

    def sample_haar_indexed(self, seed: int, indices) -> None:
        """Generate the resident batch on the device from chosen stream indices: T_i = Haar(seed, indices[i]) (any order, repeats
        allowed) -- slam_sample_haar_indexed."""
        idx = np.ascontiguousarray(indices, dtype=np.int64).reshape(-1)
        _check(self._lib.slam_sample_haar_indexed(self._h, int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(idx), idx.size))
        self.n_targets = int(idx.size)

    def haar_select_spans(self, seed: int, first_index: int, n_candidates: int, gate_coords_seq, k_max: int, span_lo: int, span_hi: int,
                          capacity: int, tol: float = 2e-8, margin: float = 0.0):
        """Among the Haar candidates ``first_index .. first_index + n_candidates`` of the stream ``seed``, those whose template size
        with the gate sequence ``gate_coords_seq`` (as ``predict_spans`` sees it: 0 local, 1..k_max, k_max + 1 out of reach) lies in
        ``[span_lo, span_hi]`` -- and, with ``margin > 0``, does not change at ``tol + margin`` and ``tol - margin``
        (slam_haar_select_spans: drawn, classified and ranked on the device; the resident targets are not touched).  Returns
        ``(indices, n_selected, span_counts)``: the stream indices of the first ``min(n_selected, capacity)`` selected candidates in
        increasing order (int64), the number selected in the whole range, and int64[k_max + 2] candidates per span at ``tol``."""
        point, bounds = _span_half_spaces(gate_coords_seq, k_max)
        cap = max(int(capacity), 0)
        idx = np.zeros(cap, dtype=np.int64)
        counts = np.zeros(int(k_max) + 2, dtype=np.int64)
        m = C.c_int64(0)
        _check(self._lib.slam_haar_select_spans(self._h, int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_index), int(n_candidates), int(k_max),
                                                _ptr(point), _ptr(bounds), float(tol), float(margin), int(span_lo), int(span_hi),
                                                int(capacity), C.byref(m), _ptr(idx) if cap else None, _ptr(counts)))
        return idx[: min(int(m.value), cap)], int(m.value), counts

    def get_targets(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """Resident targets [first, first + count) as complex128[count, 4, 4]."""
        count = self.n_targets - first if count is None else count
        out = np.empty((count, 4, 4, 2), dtype=np.float64)
        _check(self._lib.slam_get_targets(self._h, int(first), int(count), _ptr(out)))
        return out.view(np.complex128).reshape(count, 4, 4)

    def set_gates(self, gates: np.ndarray) -> None:
        g = _mat_to_ri(gates)
        if g.ndim != 4:
            raise ValueError("gates must have shape [G, 4, 4]")
        # the same table as the last upload (one basis, many calls): nothing to do -- the upload is a synchronous copy (~25 us)
        last = getattr(self, "_gates_uploaded", None)
        if last is not None and last.shape == g.shape and np.array_equal(last, g):
            return
        _check(self._lib.slam_set_gates(self._h, _ptr(g), g.shape[0]))
        self.n_gates = g.shape[0]
        self._gates_uploaded = g.copy()

    # -- fused loss + gradient -------------------------------------------
    def eval_loss_grad(self, gate_seq: Sequence[int], x: np.ndarray, target_of: np.ndarray, want_grad=True):
        k = len(gate_seq)
        n = 6 * (k + 1)
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.ndim != 2 or x.shape[1] != n:
            raise ValueError(f"x must have shape [M, {n}]")
        M = x.shape[0]
        tof = np.ascontiguousarray(target_of, dtype=np.int32)
        if tof.shape != (M,):
            raise ValueError("target_of must have shape [M]")
        gs = np.ascontiguousarray(gate_seq, dtype=np.int32)
        loss = np.empty(M, dtype=np.float64)
        grad = np.empty((M, n), dtype=np.float64) if want_grad else None
        _check(self._lib.slam_eval_loss_grad(self._h, k, _ptr(gs), _ptr(x), _ptr(tof), M, _ptr(loss), _ptr(grad)))
        return loss, grad

    def eval_unitary(self, gate_seq: Sequence[int], x: np.ndarray, target_of: Optional[np.ndarray] = None):
        """W(x) for each row of x: complex128[M, 4, 4] (and BasicCost vs target_of if given)."""
        k = len(gate_seq)
        n = 6 * (k + 1)
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.ndim != 2 or x.shape[1] != n:
            raise ValueError(f"x must have shape [M, {n}]")
        M = x.shape[0]
        tof = np.zeros(M, np.int32) if target_of is None else np.ascontiguousarray(target_of, dtype=np.int32)
        gs = np.ascontiguousarray(gate_seq, dtype=np.int32)
        w = np.empty((M, 4, 4, 2), dtype=np.float64)
        loss = np.empty(M, dtype=np.float64)
        _check(self._lib.slam_eval_unitary(self._h, k, _ptr(gs), _ptr(x), _ptr(tof), M, _ptr(w), _ptr(loss)))
        return w.view(np.complex128).reshape(M, 4, 4), loss

    # -- one span stage ----------------------------------------------------
    def _stage_call(self, fn, qn: int, gate_seq, params: OptParams, active, x0, vecs=(), exit_loss=None, trace_cap=None,
                    want_items: bool = True) -> dict:
        """The one marshalling routine of the six stage entry points: ``fn(ctx, k, gate_seq, active, na, x0, *vecs, params,
        [exit_loss], [trace_cap], outputs...)`` for a template of n = 6 (k + 1) + ``qn`` k parameters.  ``vecs``: the four per-parameter
        vectors of the V2 / smush forms (each may be None).  The outputs go to the library in the order of the returned dictionary:
        ``best_loss`` [na], ``best_x`` [na, n], ``best_restart`` [na], the per-item arrays [na, R] (None without ``want_items``;
        ``item_evals`` only without a trace), then -- with ``trace_cap`` -- ``trace_loss`` [na, R, cap] and ``trace_x`` [na, R, cap, n]."""
        k = len(gate_seq)
        n = 6 * (k + 1) + qn * k
        gs = np.ascontiguousarray(gate_seq, dtype=np.int32)
        if active is not None:
            active = np.ascontiguousarray(active, dtype=np.int32)
            na = active.shape[0]
        else:
            na = self.n_targets
        R = int(params.restarts)
        vecs = [None if v is None else np.ascontiguousarray(v, dtype=np.float64) for v in vecs]
        for v in vecs:
            if v is not None and v.shape != (n,):
                raise ValueError(f"per-parameter arrays must have shape [{n}]")
        if x0 is not None:
            x0 = np.ascontiguousarray(x0, dtype=np.float64)
            if x0.shape != (na, R, n):
                raise ValueError(f"x0 must have shape [{na}, {R}, {n}]")
        out = {"best_loss": np.empty(na, dtype=np.float64), "best_x": np.empty((na, n), dtype=np.float64),
               "best_restart": np.empty(na, dtype=np.int32)}
        per_item = {"item_loss": np.float64, "item_iters": np.int32, "item_status": np.int32}
        if trace_cap is None:
            per_item["item_evals"] = np.int32
        for key, dtype in per_item.items():
            out[key] = np.empty((na, R), dtype=dtype) if want_items else None
        scalars = [] if exit_loss is None else [float(exit_loss)]
        if trace_cap is not None:
            cap = int(trace_cap)
            scalars.append(cap)
            out["trace_loss"] = np.empty((na, R, cap), dtype=np.float64)
            out["trace_x"] = np.empty((na, R, cap, n), dtype=np.float64)
        _check(fn(self._h, k, _ptr(gs), _ptr(active), na, _ptr(x0), *[_ptr(v) for v in vecs], C.byref(params), *scalars,
                  *[_ptr(a) for a in out.values()]))
        return out

    def minimize_stage(
        self,
        gate_seq: Sequence[int],
        params: OptParams,
        active: Optional[np.ndarray] = None,
        x0: Optional[np.ndarray] = None,
        want_items: bool = True,
    ) -> dict:
        out = self._stage_call(self._lib.slam_minimize_stage, 0, gate_seq, params, active, x0, want_items=want_items)
        return {key: a for key, a in out.items() if a is not None}  # (without items: no item_* keys here, None in the V2 / smush form)

    # -- three-qubit templates (slam_q3_*): self-contained calls, nothing resident -------------------------------------------
    @staticmethod
    def _q3_template(gates, gate_index, edges, targets):
        g = _mat_to_ri(gates)
        if g.ndim != 4:
            raise ValueError("gates must have shape [G, 4, 4]")
        gi = np.ascontiguousarray(gate_index, dtype=np.int32).reshape(-1)
        ed = np.ascontiguousarray(edges, dtype=np.int32)
        if ed.shape != (len(gi), 2):
            raise ValueError(f"edges must have shape [{len(gi)}, 2]")
        t = np.ascontiguousarray(np.asarray(targets, dtype=np.complex128))
        if t.ndim != 3 or t.shape[1:] != (8, 8):
            raise ValueError(f"expected targets of shape [N, 8, 8], got {t.shape}")
        return g, gi, ed, t.view(np.float64).reshape(t.shape + (2,))

    def q3_eval(self, gates, gate_index, edges, targets, x, target_of=None, cost_kind: int = 0, want_grad=True, want_unitary=False):
        """``slam_q3_eval``: loss [M], gradient [M, n] (or None) and 8x8 unitary complex128 [M, 8, 8] (or None) of M parameter rows of
        the three-qubit template (gate table [G, 4, 4], per position its table index and its edge (a, b)); n = 9 + 6 k."""
        g, gi, ed, t = self._q3_template(gates, gate_index, edges, targets)
        k = len(gi)
        n = 9 + 6 * k
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.ndim != 2 or x.shape[1] != n:
            raise ValueError(f"x must have shape [M, {n}]")
        M = x.shape[0]
        tof = np.zeros(M, np.int32) if target_of is None else np.ascontiguousarray(target_of, dtype=np.int32)
        if tof.shape != (M,):
            raise ValueError("target_of must have shape [M]")
        loss = np.empty(M, dtype=np.float64)
        grad = np.empty((M, n), dtype=np.float64) if want_grad else None
        w = np.empty((M, 8, 8, 2), dtype=np.float64) if want_unitary else None
        _check(self._lib.slam_q3_eval(self._h, _ptr(g), g.shape[0], k, _ptr(gi), _ptr(ed), _ptr(t), t.shape[0], _ptr(x), _ptr(tof), M,
                                      int(cost_kind), _ptr(loss), _ptr(grad), _ptr(w)))
        return loss, grad, (None if w is None else w.view(np.complex128).reshape(M, 8, 8))

    def q3_minimize(self, gates, gate_index, edges, targets, params: OptParams, exit_loss: float, cost_kind: int = 0, x0=None) -> dict:
        """``slam_q3_minimize``: one stage over all targets x ``params.restarts``.  Returns ``best_loss`` [N], ``best_x`` [N, n],
        ``best_restart`` [N], the per-item arrays [N, R] ``item_loss`` / ``item_iters`` / ``item_status`` / ``item_evals``, ``item_x``
        [N, R, n] and ``kernel_ms``."""
        g, gi, ed, t = self._q3_template(gates, gate_index, edges, targets)
        k = len(gi)
        n = 9 + 6 * k
        N, R = t.shape[0], int(params.restarts)
        if x0 is not None:
            x0 = np.ascontiguousarray(x0, dtype=np.float64)
            if x0.shape != (N, R, n):
                raise ValueError(f"x0 must have shape [{N}, {R}, {n}]")
        out = {"best_loss": np.empty(N, dtype=np.float64), "best_x": np.empty((N, n), dtype=np.float64),
               "best_restart": np.empty(N, dtype=np.int32), "item_loss": np.empty((N, R), dtype=np.float64),
               "item_iters": np.empty((N, R), dtype=np.int32), "item_status": np.empty((N, R), dtype=np.int32),
               "item_evals": np.empty((N, R), dtype=np.int32), "item_x": np.empty((N, R, n), dtype=np.float64)}
        ms = np.zeros(1, dtype=np.float64)
        _check(self._lib.slam_q3_minimize(self._h, _ptr(g), g.shape[0], k, _ptr(gi), _ptr(ed), _ptr(t), N, int(cost_kind), C.byref(params),
                                          float(exit_loss), _ptr(x0), *[_ptr(a) for a in out.values()], _ptr(ms)))
        out["kernel_ms"] = float(ms[0])
        return out

    # -- Hamiltonian templates (slam_ham_*): self-contained calls, nothing resident ----------------------------------------------
    @staticmethod
    def _ham_description(terms, targets):
        d, n = int(terms["dim"]), int(terms["n_params"])
        m = np.ascontiguousarray(np.asarray(terms["matrices"], dtype=np.complex128))
        if m.ndim != 3 or m.shape[1:] != (d, d):
            raise ValueError(f"terms['matrices'] must have shape [K, {d}, {d}]")
        slices = terms.get("n_slices")  # None: one exponential (slam_ham_*); S: S time slices (slam_hams_*), index arrays [S, K]
        si = np.ascontiguousarray(terms["s_index"], dtype=np.int32)
        pi = np.ascontiguousarray(terms["phi_index"], dtype=np.int32)
        if slices is None:
            si, pi = si.reshape(-1), pi.reshape(-1)
        if si.shape != pi.shape or si.shape != ((len(m),) if slices is None else (int(slices), len(m))):
            raise ValueError("terms: one s_index and one phi_index per matrix" + ("" if slices is None else " and slice"))
        t = np.ascontiguousarray(np.asarray(targets, dtype=np.complex128))
        if t.ndim != 3 or t.shape[1:] != (d, d):
            raise ValueError(f"expected targets of shape [N, {d}, {d}], got {t.shape}")
        head = (d, n, len(m)) + (() if slices is None else (int(slices),)) + (_ptr(m.view(np.float64)), _ptr(si), _ptr(pi), int(terms["t_index"]))
        return head, (m, si, pi), t.view(np.float64).reshape(t.shape + (2,)), d, n

    def ham_eval(self, terms, targets, x, target_of=None, cost_kind: int = 0, want_grad=True, want_unitary=False):
        """``slam_ham_eval``: loss [M], gradient [M, n] (or None) and unitary complex128 [M, dim, dim] (or None) of M parameter rows of
        the Hamiltonian described by ``terms`` (``hamiltonian.Hamiltonian.device_terms()``), item m against ``targets[target_of[m]]``."""
        if "n_slices" in terms:
            raise ValueError("a time-sliced description goes to hams_eval")
        return self._ham_eval(self._lib.slam_ham_eval, terms, targets, x, target_of, cost_kind, want_grad, want_unitary)

    def hams_eval(self, terms, targets, x, target_of=None, cost_kind: int = 0, want_grad=True, want_unitary=False):
        """``slam_hams_eval``: ``ham_eval`` for a time-sliced description (``hamiltonian.TimeSliced.device_terms()``: ``"n_slices"`` and
        index arrays [S, K])."""
        if "n_slices" not in terms:
            raise ValueError("hams_eval takes a time-sliced description (terms['n_slices'])")
        return self._ham_eval(self._lib.slam_hams_eval, terms, targets, x, target_of, cost_kind, want_grad, want_unitary)

    def _ham_eval(self, call, terms, targets, x, target_of, cost_kind, want_grad, want_unitary):
        head, keep, t, d, n = self._ham_description(terms, targets)
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.ndim != 2 or x.shape[1] != n:
            raise ValueError(f"x must have shape [M, {n}]")
        M = x.shape[0]
        tof = np.zeros(M, np.int32) if target_of is None else np.ascontiguousarray(target_of, dtype=np.int32)
        if tof.shape != (M,):
            raise ValueError("target_of must have shape [M]")
        loss = np.empty(M, dtype=np.float64)
        grad = np.empty((M, n), dtype=np.float64) if want_grad else None
        w = np.empty((M, d, d, 2), dtype=np.float64) if want_unitary else None
        _check(call(self._h, *head, _ptr(t), t.shape[0], _ptr(x), _ptr(tof), M, int(cost_kind), _ptr(loss), _ptr(grad), _ptr(w)))
        return loss, grad, (None if w is None else w.view(np.complex128).reshape(M, d, d))

    def ham_minimize(self, terms, targets, params: OptParams, exit_loss: float, x0, cost_kind: int = 0) -> dict:
        """``slam_ham_minimize``: one stage over all targets x ``params.restarts`` from the start points ``x0`` [N, R, n]; the keys of
        ``q3_minimize``."""
        if "n_slices" in terms:
            raise ValueError("a time-sliced description goes to hams_minimize")
        return self._ham_minimize(self._lib.slam_ham_minimize, terms, targets, params, exit_loss, x0, cost_kind)

    def hams_minimize(self, terms, targets, params: OptParams, exit_loss: float, x0, cost_kind: int = 0) -> dict:
        """``slam_hams_minimize``: ``ham_minimize`` for a time-sliced description."""
        if "n_slices" not in terms:
            raise ValueError("hams_minimize takes a time-sliced description (terms['n_slices'])")
        return self._ham_minimize(self._lib.slam_hams_minimize, terms, targets, params, exit_loss, x0, cost_kind)

    def _ham_minimize(self, call, terms, targets, params, exit_loss, x0, cost_kind):
        head, keep, t, d, n = self._ham_description(terms, targets)
        N, R = t.shape[0], int(params.restarts)
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        if x0.shape != (N, R, n):
            raise ValueError(f"x0 must have shape [{N}, {R}, {n}]")
        out = {"best_loss": np.empty(N, dtype=np.float64), "best_x": np.empty((N, n), dtype=np.float64),
               "best_restart": np.empty(N, dtype=np.int32), "item_loss": np.empty((N, R), dtype=np.float64),
               "item_iters": np.empty((N, R), dtype=np.int32), "item_status": np.empty((N, R), dtype=np.int32),
               "item_evals": np.empty((N, R), dtype=np.int32), "item_x": np.empty((N, R, n), dtype=np.float64)}
        ms = np.zeros(1, dtype=np.float64)
        _check(call(self._h, *head, _ptr(t), N, int(cost_kind), C.byref(params), float(exit_loss), _ptr(x0), *[_ptr(a) for a in out.values()],
                    _ptr(ms)))
        out["kernel_ms"] = float(ms[0])
        return out

    # -- mixed three-qubit templates (slam_q3m_*): positions of arity 2 or 3 -----------------------------------------------------
    @staticmethod
    def _q3m_template(gates2, gates3, arity, gate_index, qubits, targets):
        g2 = np.ascontiguousarray(np.asarray(gates2, dtype=np.complex128))
        g3 = np.ascontiguousarray(np.asarray(gates3, dtype=np.complex128))
        if g2.ndim != 3 or g2.shape[1:] != (4, 4):
            raise ValueError("gates2 must have shape [G2, 4, 4]")
        if g3.ndim != 3 or g3.shape[1:] != (8, 8):
            raise ValueError("gates3 must have shape [G3, 8, 8]")
        ar = np.ascontiguousarray(arity, dtype=np.int32).reshape(-1)
        gi = np.ascontiguousarray(gate_index, dtype=np.int32).reshape(-1)
        qb = np.ascontiguousarray(qubits, dtype=np.int32)
        if gi.shape != ar.shape or qb.shape != (len(ar), 3):
            raise ValueError(f"gate_index must have shape [{len(ar)}], qubits [{len(ar)}, 3]")
        t = np.ascontiguousarray(np.asarray(targets, dtype=np.complex128))
        if t.ndim != 3 or t.shape[1:] != (8, 8):
            raise ValueError(f"expected targets of shape [N, 8, 8], got {t.shape}")
        n = 9 + 3 * int(ar.sum())
        return (g2.view(np.float64).reshape(g2.shape + (2,)), g3.view(np.float64).reshape(g3.shape + (2,)), ar, gi, qb,
                t.view(np.float64).reshape(t.shape + (2,)), n)

    def q3m_eval(self, gates2, gates3, arity, gate_index, qubits, targets, x, target_of=None, cost_kind: int = 0, want_grad=True,
                 want_unitary=False):
        """``slam_q3m_eval``: as ``q3_eval`` for a template whose position j has ``arity[j]`` qubits, the gate ``gate_index[j]`` of the
        table of that arity (gates2 [G2, 4, 4], gates3 [G3, 8, 8]) on ``qubits[j]`` = (a, b, c) (c ignored at arity 2);
        n = 9 + 3 sum(arity)."""
        g2, g3, ar, gi, qb, t, n = self._q3m_template(gates2, gates3, arity, gate_index, qubits, targets)
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.ndim != 2 or x.shape[1] != n:
            raise ValueError(f"x must have shape [M, {n}]")
        M = x.shape[0]
        tof = np.zeros(M, np.int32) if target_of is None else np.ascontiguousarray(target_of, dtype=np.int32)
        if tof.shape != (M,):
            raise ValueError("target_of must have shape [M]")
        loss = np.empty(M, dtype=np.float64)
        grad = np.empty((M, n), dtype=np.float64) if want_grad else None
        w = np.empty((M, 8, 8, 2), dtype=np.float64) if want_unitary else None
        _check(self._lib.slam_q3m_eval(self._h, _ptr(g2), g2.shape[0], _ptr(g3), g3.shape[0], len(ar), _ptr(ar), _ptr(gi), _ptr(qb), _ptr(t),
                                       t.shape[0], _ptr(x), _ptr(tof), M, int(cost_kind), _ptr(loss), _ptr(grad), _ptr(w)))
        return loss, grad, (None if w is None else w.view(np.complex128).reshape(M, 8, 8))

    def q3m_minimize(self, gates2, gates3, arity, gate_index, qubits, targets, params: OptParams, exit_loss: float, cost_kind: int = 0,
                     x0=None) -> dict:
        """``slam_q3m_minimize``: ``q3_minimize`` for the template description of ``q3m_eval``; the same keys."""
        g2, g3, ar, gi, qb, t, n = self._q3m_template(gates2, gates3, arity, gate_index, qubits, targets)
        N, R = t.shape[0], int(params.restarts)
        if x0 is not None:
            x0 = np.ascontiguousarray(x0, dtype=np.float64)
            if x0.shape != (N, R, n):
                raise ValueError(f"x0 must have shape [{N}, {R}, {n}]")
        out = {"best_loss": np.empty(N, dtype=np.float64), "best_x": np.empty((N, n), dtype=np.float64),
               "best_restart": np.empty(N, dtype=np.int32), "item_loss": np.empty((N, R), dtype=np.float64),
               "item_iters": np.empty((N, R), dtype=np.int32), "item_status": np.empty((N, R), dtype=np.int32),
               "item_evals": np.empty((N, R), dtype=np.int32), "item_x": np.empty((N, R, n), dtype=np.float64)}
        ms = np.zeros(1, dtype=np.float64)
        _check(self._lib.slam_q3m_minimize(self._h, _ptr(g2), g2.shape[0], _ptr(g3), g3.shape[0], len(ar), _ptr(ar), _ptr(gi), _ptr(qb),
                                           _ptr(t), N, int(cost_kind), C.byref(params), float(exit_loss), _ptr(x0),
                                           *[_ptr(a) for a in out.values()], _ptr(ms)))
        out["kernel_ms"] = float(ms[0])
        return out

    # -- state objectives of the three-qubit templates (slam_q3s_*): mutual information of a start state ------------------------
    @staticmethod
    def _q3s_states(states):
        st = np.ascontiguousarray(np.asarray(states, dtype=np.complex128))
        if st.ndim != 2 or st.shape[1] != 8:
            raise ValueError(f"expected states of shape [N, 8], got {st.shape}")
        return st.view(np.float64).reshape(st.shape + (2,))

    def q3s_eval(self, gates2, gates3, arity, gate_index, qubits, states, x, state_of=None, cost_kind: int = COST_MUTUAL_INFO, want_grad=True,
                 want_state=False):
        """``slam_q3s_eval``: loss [M], gradient [M, n] (or None) and final state complex128 [M, 8] (or None) of M parameter rows of
        the template of ``q3m_eval``, item m starting from ``states[state_of[m]]``; ``cost_kind``: ``COST_MUTUAL_INFO`` or
        ``COST_MUTUAL_INFO_SQUARE``."""
        st = self._q3s_states(states)
        g2, g3, ar, gi, qb, _, n = self._q3m_template(gates2, gates3, arity, gate_index, qubits, np.zeros((1, 8, 8)))
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.ndim != 2 or x.shape[1] != n:
            raise ValueError(f"x must have shape [M, {n}]")
        M = x.shape[0]
        sof = np.zeros(M, np.int32) if state_of is None else np.ascontiguousarray(state_of, dtype=np.int32)
        if sof.shape != (M,):
            raise ValueError("state_of must have shape [M]")
        loss = np.empty(M, dtype=np.float64)
        grad = np.empty((M, n), dtype=np.float64) if want_grad else None
        v = np.empty((M, 8, 2), dtype=np.float64) if want_state else None
        _check(self._lib.slam_q3s_eval(self._h, _ptr(g2), g2.shape[0], _ptr(g3), g3.shape[0], len(ar), _ptr(ar), _ptr(gi), _ptr(qb), _ptr(st),
                                       st.shape[0], _ptr(x), _ptr(sof), M, int(cost_kind), _ptr(loss), _ptr(grad), _ptr(v)))
        return loss, grad, (None if v is None else v.view(np.complex128).reshape(M, 8))

    def q3s_minimize(self, gates2, gates3, arity, gate_index, qubits, states, params: OptParams, exit_loss: float,
                     cost_kind: int = COST_MUTUAL_INFO, x0=None) -> dict:
        """``slam_q3s_minimize``: ``q3m_minimize`` with one start state [8] in each target's place; the same keys."""
        st = self._q3s_states(states)
        g2, g3, ar, gi, qb, _, n = self._q3m_template(gates2, gates3, arity, gate_index, qubits, np.zeros((1, 8, 8)))
        N, R = st.shape[0], int(params.restarts)
        if x0 is not None:
            x0 = np.ascontiguousarray(x0, dtype=np.float64)
            if x0.shape != (N, R, n):
                raise ValueError(f"x0 must have shape [{N}, {R}, {n}]")
        out = {"best_loss": np.empty(N, dtype=np.float64), "best_x": np.empty((N, n), dtype=np.float64),
               "best_restart": np.empty(N, dtype=np.int32), "item_loss": np.empty((N, R), dtype=np.float64),
               "item_iters": np.empty((N, R), dtype=np.int32), "item_status": np.empty((N, R), dtype=np.int32),
               "item_evals": np.empty((N, R), dtype=np.int32), "item_x": np.empty((N, R, n), dtype=np.float64)}
        ms = np.zeros(1, dtype=np.float64)
        _check(self._lib.slam_q3s_minimize(self._h, _ptr(g2), g2.shape[0], _ptr(g3), g3.shape[0], len(ar), _ptr(ar), _ptr(gi), _ptr(qb),
                                           _ptr(st), N, int(cost_kind), C.byref(params), float(exit_loss), _ptr(x0),
                                           *[_ptr(a) for a in out.values()], _ptr(ms)))
        out["kernel_ms"] = float(ms[0])
        return out

    # -- the whole span loop -------------------------------------------------
    @staticmethod
    def _flat_gate_seqs(gate_seqs: Sequence[Sequence[int]], k_min: int, k_max: int) -> np.ndarray:
        if len(gate_seqs) != k_max - k_min + 1:
            raise ValueError("need one gate sequence per span")
        flat = []
        for k, gs in zip(range(k_min, k_max + 1), gate_seqs):
            if len(gs) != k:
                raise ValueError(f"gate sequence for span {k} has length {len(gs)}")
            flat.extend(int(g) for g in gs)
        return np.asarray(flat, dtype=np.int32)

    def decompose(self, k_min, k_max, gate_seqs, params: OptParams, success_threshold: float, fetch=True):
        flat = self._flat_gate_seqs(gate_seqs, k_min, k_max)
        _check(self._lib.slam_decompose_resident(self._h, k_min, k_max, _ptr(flat), C.byref(params), float(success_threshold)))
        if fetch:
            return self.fetch_results(k_max)
        return None

    def fetch_results(self, k_max: int):
        nmax = 6 * (k_max + 1)
        N = self.n_targets
        best_loss = np.empty(N, dtype=np.float64)
        best_x = np.zeros((N, nmax), dtype=np.float64)
        best_cycles = np.empty(N, dtype=np.int32)
        _check(self._lib.slam_fetch_results(self._h, k_max, _ptr(best_loss), _ptr(best_x), _ptr(best_cycles)))
        return best_loss, best_x, best_cycles

    def decompose_range(self, first, count, k_min, k_max, gate_seqs, params: OptParams, success_threshold: float, fetch=True, pinned=False):
        flat = self._flat_gate_seqs(gate_seqs, k_min, k_max)
        if not fetch or not hasattr(self._lib, "slam_decompose_range_fetch"):
            _check(self._lib.slam_decompose_range(self._h, int(first), int(count), k_min, k_max, _ptr(flat), C.byref(params), float(success_threshold)))
            return self.fetch_results_range(k_max, first, count, pinned=pinned) if fetch else None
        # (every row of best_x is written: the resident rows are zero-padded)
        best_loss, best_x, best_cycles = _result_triple(result_pool.empty if pinned else pageable_pool.empty, count, 6 * (k_max + 1))
        _check(self._lib.slam_decompose_range_fetch(self._h, int(first), int(count), k_min, k_max, _ptr(flat), C.byref(params),
                                                     float(success_threshold), _ptr(best_loss), _ptr(best_x), _ptr(best_cycles)))
        return best_loss, best_x, best_cycles

    def decompose_list(self, targets, k_min, k_max, gate_seqs, params: OptParams, success_threshold: float, k_layout: int = 0):
        """Span loop for an explicit list of resident-target indices (slam_decompose_list); results stay in the
        per-target resident arrays (row width 6 (k_layout + 1)): fetch with ``fetch_results_range(k_layout, ...)``."""
        idx = np.ascontiguousarray(targets, dtype=np.int32)
        flat = self._flat_gate_seqs(gate_seqs, k_min, k_max)
        _check(self._lib.slam_decompose_list(self._h, _ptr(idx), idx.shape[0], k_min, k_max, int(k_layout), _ptr(flat),
                                              C.byref(params), float(success_threshold)))

    def decompose_predicted(self, gate_coords_seq, k_max: int, gate_seqs, params: OptParams, success_threshold: float, first: int = 0,
                            count: Optional[int] = None, carry: bool = False, tol: float = 2e-8):
        """``use_polytopes`` mode for the resident targets [first, first + count) in one chain of kernels (slam_decompose_predicted): the
        coverage lookup of ``predict_spans``, per-size target lists and the span loop, all on the device.  ``gate_seqs``: the sequences
        of spans 1..k_max.  Results stay resident (``fetch_results_range(k_max, ...)``).  Returns (n_local, n_unreachable)."""
        from . import coverage

        g = np.asarray(gate_coords_seq, dtype=np.float64).reshape(-1, 3)
        if not 1 <= k_max <= min(len(g), MAX_SPAN_MINIMIZE):
            raise ValueError(f"k_max must be 1..{min(len(g), MAX_SPAN_MINIMIZE)}")
        count = self.n_targets - first if count is None else count
        point = np.ascontiguousarray(coverage.alcove_coordinates(g[:1])[0])
        bounds = np.full((k_max, len(coverage._PATTERNS)), -np.inf)
        for k in range(2, k_max + 1):
            bounds[k - 1] = coverage.region(g[:k])
        flat = self._flat_gate_seqs(gate_seqs, 1, k_max)
        n_loc, n_unr = C.c_int64(0), C.c_int64(0)
        _check(self._lib.slam_decompose_predicted(self._h, int(first), int(count), int(k_max), _ptr(point), _ptr(bounds), float(tol), int(bool(carry)),
                                                  _ptr(flat), C.byref(params), float(success_threshold), C.byref(n_loc), C.byref(n_unr)))
        return int(n_loc.value), int(n_unr.value)

    def fetch_results_range(self, k_max: int, first: int, count: int, pinned: bool = False):
        best_loss, best_x, best_cycles = _result_triple(result_pool.empty if pinned else pageable_pool.empty, count, 6 * (k_max + 1))
        _check(self._lib.slam_fetch_results_range(self._h, k_max, int(first), int(count), _ptr(best_loss), _ptr(best_x), _ptr(best_cycles)))
        return best_loss, best_x, best_cycles

    def fetch_span_losses(self, first: int, count: int) -> np.ndarray:
        """Running best loss after every span the last span loop ran: float64[count, MAX_SPAN_EVAL] (NaN = span not run)."""
        out = np.empty((count, MAX_SPAN_EVAL), dtype=np.float64)
        _check(self._lib.slam_fetch_span_losses(self._h, int(first), int(count), _ptr(out)))
        return out

    def minimize_stage_trace(self, gate_seq: Sequence[int], params: OptParams, exit_loss: float, trace_cap: int,
                             active: Optional[np.ndarray] = None, x0: Optional[np.ndarray] = None) -> dict:
        """``minimize_stage`` plus the per-iteration trajectories of every restart (use_callback, optimizer.py:217-224):
        ``trace_loss[na, R, cap]`` and ``trace_x[na, R, cap, n]`` (NaN beyond ``item_iters``)."""
        return self._stage_call(self._lib.slam_minimize_stage_trace, 0, gate_seq, params, active, x0, exit_loss=exit_loss, trace_cap=trace_cap)

    # -- templates with parametrised 2Q gates (CircuitTemplateV2) ------------------------
    def v2_set_gates(self, gates: Sequence["V2Gate"]) -> None:
        arr = (V2Gate * len(gates))(*gates)
        _check(self._lib.slam_v2_set_gates(self._h, arr, len(gates)))
        self.v2_qn = int(gates[0].n_params)

    def v2_set_constraint(self, k: int, weights: Optional[np.ndarray], cost_max: float = 0.0) -> None:
        """sum_i weights[i] x_i <= cost_max for every later stage of span k (device parameter order); None removes it.
        ``v2_set_gates`` removes the constraints of every span."""
        if weights is None:
            _check(self._lib.slam_v2_set_constraint(self._h, int(k), None, 0, 0.0))
            return
        w = np.ascontiguousarray(weights, dtype=np.float64)
        _check(self._lib.slam_v2_set_constraint(self._h, int(k), w.ctypes.data, int(w.size), float(cost_max)))

    def v2_eval(self, gate_seq: Sequence[int], x: np.ndarray, target_of: Optional[np.ndarray] = None, want_grad=True, want_unitary=False):
        """Loss, gradient w.r.t. all n = 6 (k + 1) + QN k parameters and (optionally) W(x) for ``x[M, n]``."""
        return self._v2_like_eval(self._lib.slam_v2_eval_loss_grad, self.v2_qn, gate_seq, x, target_of, want_grad, want_unitary)

    def v2_minimize_stage(self, gate_seq: Sequence[int], params: OptParams, exit_loss: float, init_lo, init_hi, bound_lo=None,
                          bound_hi=None, active: Optional[np.ndarray] = None, x0: Optional[np.ndarray] = None, want_items: bool = True) -> dict:
        return self._stage_call(self._lib.slam_v2_minimize_stage, self.v2_qn, gate_seq, params, active, x0,
                                (init_lo, init_hi, bound_lo, bound_hi), exit_loss, want_items=want_items)

    def v2_decompose_range(self, first: int, count: int, k_min: int, k_max: int, gate_seqs, layouts, params: OptParams, threshold: float):
        """The span loop of a V2 template on the device (``slam_v2_decompose_range``).  ``layouts[i]`` = (init_lo, init_hi, bound_lo,
        bound_hi) of span ``k_min + i`` in device order.  Returns (best_loss [count], best_x [count, n_kmax], best_cycles [count]); a
        row holds the n_k parameters of its target's span k in front, zeros behind."""
        qn = self.v2_qn
        nmax = 6 * (k_max + 1) + qn * k_max
        gs = np.ascontiguousarray(np.concatenate([np.asarray(g, dtype=np.int32) for g in gate_seqs]))
        cat = [np.ascontiguousarray(np.concatenate([np.asarray(l[j], dtype=np.float64) for l in layouts])) for j in range(4)]
        n_tot = sum(6 * (k + 1) + qn * k for k in range(k_min, k_max + 1))
        if len(gs) != sum(range(k_min, k_max + 1)) or any(len(v) != n_tot for v in cat):
            raise ValueError("gate_seqs / layouts do not match the span range")
        best_loss, best_x, best_cycles = _result_triple(pageable_pool.empty, count, nmax)
        _check(self._lib.slam_v2_decompose_range(self._h, int(first), int(count), int(k_min), int(k_max), _ptr(gs), _ptr(cat[0]), _ptr(cat[1]),
                                                 _ptr(cat[2]), _ptr(cat[3]), C.byref(params), float(threshold), _ptr(best_loss), _ptr(best_x),
                                                 _ptr(best_cycles)))
        return best_loss, best_x, best_cycles

    def v2_minimize_stage_trace(self, gate_seq: Sequence[int], params: OptParams, exit_loss: float, trace_cap: int, init_lo, init_hi,
                                bound_lo=None, bound_hi=None, active: Optional[np.ndarray] = None) -> dict:
        """``v2_minimize_stage`` plus the loss / parameters after every accepted iteration of every restart
        (``trace_loss`` [na, R, cap], ``trace_x`` [na, R, cap, n]; NaN beyond an item's iterations).  No ``x0``: NULL goes in its place."""
        return self._stage_call(self._lib.slam_v2_minimize_stage_trace, self.v2_qn, gate_seq, params, active, None,
                                (init_lo, init_hi, bound_lo, bound_hi), exit_loss, trace_cap)

    # -- parallel-drive ("smush") gates: the same calls as the V2 family -------------------------
    def smush_set_gates(self, gates: Sequence["SmushGate"]) -> None:
        arr = (SmushGate * len(gates))(*gates)
        _check(self._lib.slam_smush_set_gates(self._h, arr, len(gates)))
        self.smush_qn = int(gates[0].n_params)

    def smush_eval(self, gate_seq, x, target_of=None, want_grad=True, want_unitary=False):
        """As ``v2_eval`` for a smush gate table (n = 6 (k + 1) + QN k)."""
        return self._v2_like_eval(self._lib.slam_smush_eval_loss_grad, self.smush_qn, gate_seq, x, target_of, want_grad, want_unitary)

    def smush_minimize_stage(self, gate_seq, params: OptParams, exit_loss: float, init_lo, init_hi, bound_lo=None, bound_hi=None,
                             active=None, x0=None, want_items: bool = True) -> dict:
        """As ``v2_minimize_stage`` for a smush gate table."""
        return self._stage_call(self._lib.slam_smush_minimize_stage, self.smush_qn, gate_seq, params, active, x0,
                                (init_lo, init_hi, bound_lo, bound_hi), exit_loss, want_items=want_items)

    def smush_minimize_stage_trace(self, gate_seq, params: OptParams, exit_loss: float, trace_cap: int, init_lo, init_hi, bound_lo=None,
                                   bound_hi=None, active=None) -> dict:
        """As ``v2_minimize_stage_trace`` for a smush gate table."""
        return self._stage_call(self._lib.slam_smush_minimize_stage_trace, self.smush_qn, gate_seq, params, active, None,
                                (init_lo, init_hi, bound_lo, bound_hi), exit_loss, trace_cap)

    def _v2_like_eval(self, fn, qn, gate_seq, x, target_of, want_grad, want_unitary):
        k = len(gate_seq)
        n = 6 * (k + 1) + qn * k
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.ndim != 2 or x.shape[1] != n:
            raise ValueError(f"x must have shape [M, {n}]")
        M = x.shape[0]
        tof = np.zeros(M, np.int32) if target_of is None else np.ascontiguousarray(target_of, dtype=np.int32)
        gs = np.ascontiguousarray(gate_seq, dtype=np.int32)
        loss = np.empty(M, dtype=np.float64)
        grad = np.empty((M, n), dtype=np.float64) if want_grad else None
        w = np.empty((M, 4, 4, 2), dtype=np.float64) if want_unitary else None
        _check(fn(self._h, k, _ptr(gs), _ptr(x), _ptr(tof), M, _ptr(loss), _ptr(grad), _ptr(w)))
        return loss, grad, (w.view(np.complex128).reshape(M, 4, 4) if want_unitary else None)

    def set_cost(self, kind: int) -> None:
        """0 = BasicCost (default), 1 = SquareCost, 2 = MakhlinFunctionalCost (per-span launches; not for decompose_multi / V2)."""
        _check(self._lib.slam_set_cost(self._h, int(kind)))

    def synchronize(self) -> None:
        _check(self._lib.slam_synchronize(self._h))

    def stats(self) -> dict:
        s = Stats()
        _check(self._lib.slam_get_stats(self._h, C.byref(s)))
        return {
            "kernel_ms": s.kernel_ms,
            "kernel_launches": s.kernel_launches,
            "evals": list(s.evals),
            "items": list(s.items),
            "total_ms": s.total_ms,
            "kernel_ms_span": list(s.kernel_ms_span),
            "wave_rounds": list(s.wave_rounds),
            "evals_accepted": list(s.evals_accepted),
            "evals_preempted": list(s.evals_preempted),
        }

    def reset_stats(self) -> None:
        _check(self._lib.slam_reset_stats(self._h))

    def best_loss_device_ptr(self) -> Tuple[int, int]:
        p, n = C.c_void_p(), C.c_int64(0)
        _check(self._lib.slam_best_loss_device_ptr(self._h, C.byref(p), C.byref(n)))
        return int(p.value), int(n.value)


def decompose_multi(ctxs: Sequence["Context"], first: int, count: int, k_min: int, k_max: int, gate_seqs, params: OptParams,
                    success_threshold: float) -> None:
    """The span loops of several contexts (same device, same target window, each its own gate table) as ONE chain of kernels
    (``slam_decompose_multi``): per span one multi-queue optimizer launch and one bookkeeping launch for all of them.  Results
    stay resident in each context: ``ctx.fetch_results_range(k_max, first, count)``."""
    lib = load_library()
    flat = Context._flat_gate_seqs(gate_seqs, k_min, k_max)
    arr = (C.c_void_p * len(ctxs))(*[c._h for c in ctxs])
    _check(lib.slam_decompose_multi(arr, len(ctxs), int(first), int(count), k_min, k_max, _ptr(flat), C.byref(params), float(success_threshold)))


class Comm:
    """RCCL communicator of one rank (``slam_comm``): one process per GPU, xGMI underneath.  Only the job's final
    best-loss min-all-reduce and a few scalars go through it."""

    def __init__(self, device: int, rank: int, world: int, unique_id: bytes):
        if len(unique_id) != COMM_ID_BYTES:
            raise ValueError(f"unique_id must be {COMM_ID_BYTES} bytes")
        self._lib = load_library()
        self._h = C.c_void_p()
        buf = C.create_string_buffer(bytes(unique_id), COMM_ID_BYTES)
        _check(self._lib.slam_comm_init(int(device), int(rank), int(world), buf, C.byref(self._h)))
        self.rank, self.world, self.device = int(rank), int(world), int(device)

    @staticmethod
    def unique_id() -> bytes:
        """``ncclGetUniqueId`` (rank 0 calls this and hands the bytes to the other ranks)."""
        buf = C.create_string_buffer(COMM_ID_BYTES)
        _check(load_library().slam_comm_get_unique_id(buf))
        return buf.raw

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.slam_comm_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _allreduce(self, a: np.ndarray, op: int) -> None:
        if a.dtype != np.float64 or not a.flags.c_contiguous:
            raise ValueError("all-reduce buffers must be C-contiguous float64")
        _check(self._lib.slam_comm_allreduce_f64(self._h, _ptr(a), a.size, op))

    def allreduce_min(self, a: np.ndarray) -> None:
        self._allreduce(a, OP_MIN)

    def allreduce_max(self, a: np.ndarray) -> None:
        self._allreduce(a, OP_MAX)

    def allreduce_sum(self, a: np.ndarray) -> None:
        self._allreduce(a, OP_SUM)

    def barrier(self) -> None:
        _check(self._lib.slam_comm_barrier(self._h))

    def rccl_rank_world(self):
        """(rank, world size) as RCCL itself reports them for this communicator (``ncclCommUserRank`` / ``ncclCommCount``)."""
        r, w = C.c_int(-1), C.c_int(-1)
        _check(self._lib.slam_comm_rank(self._h, C.byref(r), C.byref(w)))
        return int(r.value), int(w.value)

    def merge_begin(self, n_global: int) -> None:
        _check(self._lib.slam_comm_merge_begin(self._h, int(n_global)))
        self._merge_n = int(n_global)

    def merge_add(self, ctx: "Context", first_local: int, count: int, first_global: int) -> None:
        """Min-merge the context's resident best_loss window into the job-wide vector, device to device."""
        _check(self._lib.slam_comm_merge_add(self._h, ctx._h, int(first_local), int(count), int(first_global)))

    def merge_add_host(self, loss: np.ndarray, first_global: int) -> None:
        loss = np.ascontiguousarray(loss, dtype=np.float64)
        _check(self._lib.slam_comm_merge_add_host(self._h, _ptr(loss), loss.size, int(first_global)))

    def allreduce_min_merged(self, threshold: float, want_merged: bool = False):
        """The job's one collective.  Returns (number of entries < threshold, merged vector or None).  The host copy is
        sized from the ``n_global`` given to ``merge_begin`` (the library checks the capacity again)."""
        nb = C.c_int64(0)
        n = getattr(self, "_merge_n", 0)
        if n <= 0:
            raise RuntimeError("allreduce_min_merged: call merge_begin first")
        merged = np.empty(n, dtype=np.float64) if want_merged else None
        _check(self._lib.slam_allreduce_min(self._h, float(threshold), C.byref(nb), _ptr(merged), n if want_merged else 0))
        return int(nb.value), merged
