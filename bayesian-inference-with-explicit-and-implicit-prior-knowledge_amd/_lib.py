"""ctypes binding of libpgas_hip.so (C ABI: include/pgas_hip.h) and the Engine wrapper.

There is no CPU fallback: if the library is missing or a call fails, an exception is raised.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PGAS_HIP_LIB") or os.path.join(_HERE, "libpgas_hip.so")  # override: kernel experiments only

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)


class PgasError(RuntimeError):
    pass


class _ModelDesc(C.Structure):
    _fields_ = [
        ("N", C.c_int32), ("T", C.c_int32), ("nx", C.c_int32), ("ny", C.c_int32), ("nu", C.c_int32),
        ("M", C.c_int32), ("D", C.c_int32),
        ("idx", _ip), ("sel", _ip), ("alpha", _dp), ("beta", _dp), ("nrm", C.c_double),
        ("H", _dp), ("LRinv", _dp), ("cR", C.c_double),
        ("m0", _dp), ("L0", _dp), ("y", _dp), ("u", _dp),
        ("device", C.c_int32), ("keep_logw_trace", C.c_int32), ("no_fast_variant", C.c_int32),
    ]


EXPORTS = [
    "pgas_create", "pgas_destroy", "pgas_last_error", "pgas_segment_size", "pgas_set_params", "pgas_set_params_dev", "pgas_get_params", "pgas_basis_eval",
    "pgas_aux_states", "pgas_init_state", "pgas_step", "pgas_sweep", "pgas_get_traces", "pgas_last_final_index", "pgas_scan_status",
    "pgas_suffstats", "pgas_set_profiling", "pgas_get_profile", "pgas_set_option",
    "pgas_systematic_resample", "pgas_reconstruct_trajectory",
    "pgas_trace_layout", "pgas_trace_row",
    "pgas_shard_setup", "pgas_shard_buffers", "pgas_shard_layout", "pgas_shard_block", "pgas_shard_set_peer_block", "pgas_shard_run", "pgas_ipc_export", "pgas_ipc_open",
    "pgas_hip_runtime_version", "pgas_shard_unique_id", "pgas_shard_comm_init", "pgas_shard_sweep", "pgas_shard_set_collective", "pgas_get_launch_info", "pgas_shard_probe_collective", "pgas_detmath_eval",
    "pgas_m_rng_uniform", "pgas_m_rng_normal", "pgas_m_rng_student_t", "pgas_m_rng_student_t_host", "pgas_m_rng_chi2", "pgas_m_set_time_source", "pgas_m_rng_uniform_dev", "pgas_systematic_resample_dev", "pgas_m_mniw_solve", "pgas_m_mniw_trisolve", "pgas_m_check", "pgas_m_stats_gather_update", "pgas_m_weighted_stats",
    "pgas_m_mniw_solve_n", "pgas_m_mniw_trisolve_n", "pgas_m_stats_gather_update_n", "pgas_m_weighted_stats_n", "pgas_m_expr_eval",
    "pgas_m_rng_student_t_df", "pgas_m_mniw_draw", "pgas_m_hilbert_basis", "pgas_m_lbm_diff",
    "pgas_chains_set_params_dev", "pgas_chains_sweep", "pgas_chains_get_traces", "pgas_chains_final_index", "pgas_chains_keys",
    "pgas_chains_param_draws", "pgas_chains_suffstats", "pgas_rollout", "pgas_rollout_stats", "pgas_filter",
    "pgas_forecast", "pgas_forecast_origins_per_block", "pgas_rollout_cdf", "pgas_forecast_cdf", "pgas_smooth",
    "pgas_m_runs_rng_normal", "pgas_m_runs_rng_student_t", "pgas_m_runs_rng_student_t_df", "pgas_m_runs_rng_uniform", "pgas_m_runs_systematic",
    "pgas_m_runs_weighted_stats", "pgas_m_runs_mniw_solve_n", "pgas_m_runs_lbm_diff", "pgas_m_runs_categorical", "pgas_m_runs_backtrace",
    "pgas_m_rollout", "pgas_m_rollout_stats", "pgas_m_filter",
    "pgas_m_forecast", "pgas_m_forecast_origins_per_block", "pgas_m_rollout_cdf", "pgas_m_forecast_cdf", "pgas_m_smooth",
    "pgas_records_set", "pgas_records_seeds", "pgas_records_sweep", "pgas_records_get_traces", "pgas_records_final_index", "pgas_records_suffstats",
]



class RolloutLatent(C.Structure):   # pgas_m_rollout_latent (include/pgas_marginal.h)
    _fields_ = [("M", C.c_int32), ("D", C.c_int32), ("n", C.c_int32), ("feat", C.c_int32), ("sel", C.c_int32 * 4),
                ("div", C.c_double * 4), ("center", C.c_double * 4), ("L", C.c_double * 4), ("size", C.c_double * 4),
                ("idx_dev", C.c_void_p), ("A_dev", C.c_void_p), ("Lrow_dev", C.c_void_p), ("fcode_dev", C.c_void_p), ("fcode_host", C.c_void_p),
                ("f_ninstr", C.c_int32), ("reserved", C.c_int32)]


class RolloutDesc(C.Structure):   # pgas_m_rollout_desc
    _fields_ = [(k, C.c_int32) for k in ("K", "T", "P", "L", "nx", "nu", "ny", "n_in", "nconst", "nreg", "x0_mode", "f_ninstr", "g_ninstr", "reserved")] + \
               [("f_out", C.c_int32 * 8), ("g_out", C.c_int32 * 8), ("p0", C.c_int64)] + \
               [(k, C.c_void_p) for k in ("consts_dev", "fcode_dev", "gcode_dev", "fcode_host", "gcode_host", "inputs_dev", "seeds_dev", "Qc_dev", "x0_dev",
                                          "m0L0_dev", "out_x_dev", "out_y_dev")] + \
               [("lat", RolloutLatent * 4)]


class RolloutStatsDesc(C.Structure):   # pgas_m_rollout_stats_desc
    _fields_ = [(k, C.c_void_p) for k in ("y_dev", "sum_dev", "sumsq_dev", "lpd_dev", "part_dev")] + \
               [("part_bytes", C.c_uint64), ("cR", C.c_double), ("noise", C.c_int32), ("reserved", C.c_int32), ("LR", C.c_double * 64), ("LRinv", C.c_double * 64)]


class ModelFilterDesc(C.Structure):   # pgas_m_filter_desc
    _fields_ = [(k, C.c_void_p) for k in ("y_dev", "ell_dev", "loglik_dev", "ess_dev", "pred_sum_dev", "pred_sumsq_dev", "filt_sum_dev", "wtot_dev", "x_dev",
                                          "anc_dev", "lw_dev", "yhat_dev")] + \
               [("cR", C.c_double), ("LRinv", C.c_double * 64)]


class ModelForecastDesc(C.Structure):   # pgas_m_forecast_desc
    _fields_ = [(k, C.c_void_p) for k in ("x_dev", "y_dev", "sum_dev", "sumsq_dev", "lpd_dev", "cloud_x_dev", "cloud_y_dev")] + \
               [("H", C.c_int32), ("reserved", C.c_int32), ("cR", C.c_double), ("LRinv", C.c_double * 64)]


class ModelRolloutCdfDesc(C.Structure):   # pgas_m_rollout_cdf_desc
    _fields_ = [("thr_dev", C.c_void_p), ("count_dev", C.c_void_p), ("J", C.c_int32), ("noise", C.c_int32), ("LR", C.c_double * 64)]


class ModelForecastCdfDesc(C.Structure):   # pgas_m_forecast_cdf_desc
    _fields_ = [("x_dev", C.c_void_p), ("thr_dev", C.c_void_p), ("count_dev", C.c_void_p)] + \
               [(k, C.c_int32) for k in ("H", "J", "noise", "reserved")] + [("LR", C.c_double * 64)]


class ModelSmoothDesc(C.Structure):   # pgas_m_smooth_desc
    _fields_ = [(k, C.c_void_p) for k in ("x_dev", "anc_dev", "lw_dev", "yhat_dev", "y_dev", "idx_dev", "xs_dev", "xis_dev", "sum_dev", "sumsq_dev",
                                          "xi_sum_dev", "xi_sumsq_dev", "fmean_dev", "xi_dev")] + \
               [("b0", C.c_int64), ("B", C.c_int32), ("reserved", C.c_int32), ("cQ", C.c_double), ("LQinv", C.c_double * 64)]


ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.c_void_p)   # pgas_allgather_fn (include/pgas_hip.h)

_lib = None


def load():
    """Load libpgas_hip.so; raises PgasError if it has not been built (python __graft_entry__.py)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PgasError(f"{LIB_PATH} not found: build it with `python __graft_entry__.py` (hipcc, gfx950); there is no CPU fallback")
    L = C.CDLL(LIB_PATH)

    class _Missing:   # an older build (tools/ab_bench.py variants) may lack newer entry points: they fail when called, not at load time
        restype = argtypes = None

        def __init__(self, name):
            self.name = name

        def __call__(self, *a):
            raise PgasError(f"{LIB_PATH} does not export {self.name}")

    for name in EXPORTS:
        if not hasattr(L, name):
            setattr(L, name, _Missing(name))
    vp, u64, i32, i64 = C.c_void_p, C.c_uint64, C.c_int32, C.c_int64
    L.pgas_create.restype = C.c_int
    L.pgas_create.argtypes = [C.POINTER(_ModelDesc), C.POINTER(vp)]
    L.pgas_destroy.restype = None
    L.pgas_destroy.argtypes = [vp]
    L.pgas_last_error.restype = C.c_char_p
    L.pgas_last_error.argtypes = [vp]
    L.pgas_segment_size.restype = i32
    L.pgas_set_params.restype = C.c_int
    L.pgas_set_params.argtypes = [vp, vp, _dp, _dp, C.c_double, vp]
    L.pgas_set_params_dev.restype = C.c_int
    L.pgas_set_params_dev.argtypes = [vp, vp, vp, vp]
    L.pgas_get_params.restype = C.c_int
    L.pgas_get_params.argtypes = [vp, _dp, _dp, _dp, vp]
    L.pgas_basis_eval.restype = C.c_int
    L.pgas_basis_eval.argtypes = [vp, vp, i64, i32, vp, vp]
    L.pgas_aux_states.restype = C.c_int
    L.pgas_aux_states.argtypes = [vp, vp, i32, vp, vp]
    L.pgas_init_state.restype = C.c_int
    L.pgas_init_state.argtypes = [vp, u64, _dp, vp, vp]
    L.pgas_step.restype = C.c_int
    L.pgas_step.argtypes = [vp, i32, u64, vp, vp, _dp, vp, vp, vp, vp]
    L.pgas_sweep.restype = C.c_int
    L.pgas_sweep.argtypes = [vp, u64, vp, vp, vp]
    L.pgas_get_traces.restype = C.c_int
    L.pgas_get_traces.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.pgas_last_final_index.restype = C.c_int
    L.pgas_last_final_index.argtypes = [vp, C.POINTER(i64), vp]
    L.pgas_scan_status.restype = C.c_int
    L.pgas_scan_status.argtypes = [vp, C.POINTER(i32), vp]
    L.pgas_suffstats.restype = C.c_int
    L.pgas_suffstats.argtypes = [vp, vp, vp, vp, vp, vp]
    L.pgas_set_profiling.restype = C.c_int
    L.pgas_set_profiling.argtypes = [vp, i32]
    L.pgas_get_profile.restype = C.c_int
    L.pgas_get_profile.argtypes = [vp, C.POINTER(i64), C.POINTER(C.c_double), C.POINTER(i64), C.POINTER(C.c_double), vp]
    L.pgas_set_option.restype = C.c_int
    L.pgas_set_option.argtypes = [vp, i32, i64]
    L.pgas_systematic_resample.restype = C.c_int
    L.pgas_systematic_resample.argtypes = [vp, C.c_double, vp, vp, vp]
    L.pgas_reconstruct_trajectory.restype = C.c_int
    L.pgas_reconstruct_trajectory.argtypes = [vp, vp, vp, i32, i32, i64, vp, vp]
    L.pgas_shard_setup.restype = C.c_int
    L.pgas_shard_setup.argtypes = [vp, i32, i32]
    L.pgas_shard_buffers.restype = C.c_int
    L.pgas_shard_buffers.argtypes = [vp, C.POINTER(vp), C.POINTER(i64)]
    L.pgas_shard_layout.restype = C.c_int
    L.pgas_shard_layout.argtypes = [vp, i32, C.POINTER(i64)]
    L.pgas_shard_block.restype = C.c_int
    L.pgas_shard_block.argtypes = [vp, i32, i32, C.POINTER(vp), C.POINTER(i64)]
    L.pgas_shard_set_peer_block.restype = C.c_int
    L.pgas_shard_set_peer_block.argtypes = [vp, i32, i32, i32, vp]
    L.pgas_trace_layout.restype = C.c_int
    L.pgas_trace_layout.argtypes = [vp, i32, C.POINTER(i64)]
    L.pgas_trace_row.restype = C.c_int
    L.pgas_trace_row.argtypes = [vp, i32, i32, C.POINTER(vp)]
    L.pgas_shard_run.restype = C.c_int
    L.pgas_shard_run.argtypes = [vp, i32, i32, i32, u64, vp, vp, vp]
    L.pgas_shard_unique_id.restype = C.c_int
    L.pgas_shard_unique_id.argtypes = [C.c_char_p]
    L.pgas_shard_comm_init.restype = C.c_int
    L.pgas_shard_comm_init.argtypes = [vp, C.c_char_p]
    L.pgas_shard_sweep.restype = C.c_int
    L.pgas_shard_sweep.argtypes = [vp, u64, vp, vp, i32, vp]
    L.pgas_shard_set_collective.restype = C.c_int
    L.pgas_shard_set_collective.argtypes = [vp, ALLGATHER_FN, vp]
    L.pgas_detmath_eval.restype = C.c_int
    L.pgas_detmath_eval.argtypes = [i32, i32, vp, vp, vp, i64, vp, vp, vp, vp]
    L.pgas_shard_probe_collective.restype = C.c_int
    L.pgas_shard_probe_collective.argtypes = [vp, i32, vp]
    L.pgas_get_launch_info.restype = C.c_int
    L.pgas_get_launch_info.argtypes = [vp, C.POINTER(i32)]
    L.pgas_ipc_export.restype = C.c_int
    L.pgas_ipc_export.argtypes = [vp, i32, i32, C.c_char_p]
    L.pgas_hip_runtime_version.restype = C.c_int32
    L.pgas_hip_runtime_version.argtypes = []
    L.pgas_ipc_open.restype = C.c_int
    L.pgas_ipc_open.argtypes = [vp, C.c_char_p, C.POINTER(vp)]
    u32 = C.c_uint32
    L.pgas_m_rng_uniform.restype = C.c_double
    L.pgas_m_rng_uniform.argtypes = [u64, u32, u32]
    L.pgas_m_rng_normal.restype = C.c_int
    L.pgas_m_rng_normal.argtypes = [vp, u64, u32, u32, i64, i64, i32, vp, vp]
    L.pgas_m_rng_student_t.restype = C.c_int
    L.pgas_m_rng_student_t.argtypes = [vp, u64, u32, u32, i64, i64, vp, vp, vp]
    L.pgas_m_rng_student_t_host.restype = C.c_int
    L.pgas_m_rng_student_t_host.argtypes = [u64, u32, u32, i64, i64, _dp, _dp]
    L.pgas_m_set_time_source.restype = C.c_int
    L.pgas_m_set_time_source.argtypes = [vp, vp]
    L.pgas_m_rng_uniform_dev.restype = C.c_int
    L.pgas_m_rng_uniform_dev.argtypes = [vp, u64, u32, u32, vp, vp]
    L.pgas_systematic_resample_dev.restype = C.c_int
    L.pgas_systematic_resample_dev.argtypes = [vp, vp, vp, vp, vp]
    L.pgas_m_rng_chi2.restype = C.c_int
    L.pgas_m_rng_chi2.argtypes = [vp, u64, u32, u32, i64, i64, vp, vp, vp]
    L.pgas_m_mniw_solve.restype = C.c_int
    L.pgas_m_mniw_solve.argtypes = [vp, i64, i32, C.c_double, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.pgas_m_mniw_trisolve.restype = C.c_int
    L.pgas_m_mniw_trisolve.argtypes = [vp, i64, i32, vp, vp, vp, vp, vp, vp]
    L.pgas_m_rng_student_t_df.restype = C.c_int
    L.pgas_m_rng_student_t_df.argtypes = [vp, u64, C.c_uint32, C.c_uint32, i64, i64, vp, vp, C.c_double, C.c_double, vp, vp]
    L.pgas_m_mniw_draw.restype = C.c_int
    L.pgas_m_mniw_draw.argtypes = [vp, i64, C.c_double, vp, vp, vp, vp, vp, vp, C.c_double, C.c_double, vp, vp, vp]
    L.pgas_m_lbm_diff.restype = C.c_int
    L.pgas_m_lbm_diff.argtypes = [vp, i64, i32, vp, vp, vp, vp, vp, vp, C.c_double, C.c_double, vp, vp, vp, vp]
    L.pgas_m_hilbert_basis.restype = C.c_int
    L.pgas_m_hilbert_basis.argtypes = [vp, i64, i32, i32, vp, i32, vp, i32, C.POINTER(i32), _dp, _dp, _dp, _dp, vp, vp, vp]
    L.pgas_m_expr_eval.restype = C.c_int
    L.pgas_m_expr_eval.argtypes = [vp, i64, vp, i32, vp, i32, i32, i32, C.POINTER(i32), i32, vp, i32, vp, vp, i32, C.POINTER(vp), C.POINTER(i32), i32, i32,
                                   vp, vp, C.c_double, vp, vp]
    L.pgas_m_mniw_solve_n.restype = C.c_int
    L.pgas_m_mniw_solve_n.argtypes = [vp, i64, i32, i32, C.c_double, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.pgas_m_mniw_trisolve_n.restype = C.c_int
    L.pgas_m_mniw_trisolve_n.argtypes = [vp, i64, i32, i32, vp, vp, vp, vp, vp, vp]
    L.pgas_m_weighted_stats_n.restype = C.c_int
    L.pgas_m_weighted_stats_n.argtypes = [vp, i64, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.pgas_m_stats_gather_update_n.restype = C.c_int
    L.pgas_m_stats_gather_update_n.argtypes = [vp, i64, i32, i32, C.c_double, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.pgas_m_weighted_stats.restype = C.c_int
    L.pgas_m_weighted_stats.argtypes = [vp, i64, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.pgas_m_check.restype = C.c_int
    L.pgas_m_check.argtypes = [vp, vp]
    L.pgas_m_stats_gather_update.restype = C.c_int
    L.pgas_m_stats_gather_update.argtypes = [vp, i64, i32, C.c_double, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    for name, args in (("pgas_chains_set_params_dev", [vp, i32, vp, vp, vp]), ("pgas_chains_sweep", [vp, i32, vp, vp, vp, vp]),
                       ("pgas_chains_get_traces", [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]),
                       ("pgas_chains_final_index", [vp, i32, C.POINTER(i64), vp]), ("pgas_chains_keys", [vp, i32, vp, i32, vp, vp]),
                       ("pgas_chains_param_draws", [vp, i32, vp, C.c_double, vp, vp, vp, vp]), ("pgas_chains_suffstats", [vp, i32, vp, vp, vp, vp, vp]),
                       ("pgas_records_set", [vp, i32, C.POINTER(i32), _dp, _dp]), ("pgas_records_seeds", [vp, i32, vp, vp, vp]),
                       ("pgas_records_sweep", [vp, i32, vp, vp, vp, vp]),
                       ("pgas_records_get_traces", [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]),
                       ("pgas_records_final_index", [vp, i32, C.POINTER(i64), vp]), ("pgas_records_suffstats", [vp, i32, vp, vp, vp, vp, vp]),
                       ("pgas_rollout", [vp, i32, i32, i64, vp, vp, vp, vp, i32, vp, vp]),
                       ("pgas_rollout_stats", [vp, i32, i32, i64, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp]),
                       ("pgas_filter", [vp, i32, vp, vp, vp, vp, i32] + [vp] * 10),
                       ("pgas_forecast", [vp, i32, i32] + [vp] * 8), ("pgas_forecast_origins_per_block", []),
                       ("pgas_rollout_cdf", [vp, i32, i32, i64, vp, vp, vp, vp, i32, vp, vp, i32, vp, vp]),
                       ("pgas_forecast_cdf", [vp, i32, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp]),
                       ("pgas_smooth", [vp, i32, i32, i64] + [vp] * 10)):
        getattr(L, name).restype = C.c_int
        getattr(L, name).argtypes = args
    for name, args in (("pgas_m_runs_rng_normal", [vp, vp, i32, i64, u32, u32, i32, vp, vp]), ("pgas_m_runs_rng_student_t", [vp, vp, i32, i64, u32, u32, vp, vp, vp]),
                       ("pgas_m_runs_rng_student_t_df", [vp, vp, i32, i64, u32, u32, vp, vp, C.c_double, C.c_double, vp, vp]),
                       ("pgas_m_runs_rng_uniform", [vp, vp, i32, u32, u32, vp, vp]), ("pgas_m_runs_systematic", [vp, i32, i32, vp, vp, vp, vp, vp]),
                       ("pgas_m_runs_weighted_stats", [vp, i32, i64, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
                       ("pgas_m_runs_mniw_solve_n", [vp, i32, i64, i32, i32, C.c_double] + [vp] * 14),
                       ("pgas_m_runs_lbm_diff", [vp, i32, i64, i32, vp, vp, vp, vp, vp, vp, C.c_double, C.c_double, vp, vp, vp, vp]),
                       ("pgas_m_runs_categorical", [vp, i32, i32, vp, vp, vp, vp, vp, vp]),
                       ("pgas_m_runs_backtrace", [vp, i32, i32, i32, i32, vp, vp, vp, vp, vp])):
        getattr(L, name).restype = C.c_int
        getattr(L, name).argtypes = args
    L.pgas_m_rollout.restype = C.c_int
    L.pgas_m_rollout.argtypes = [vp, C.POINTER(RolloutDesc), vp]
    L.pgas_m_rollout_stats.restype = C.c_int
    L.pgas_m_rollout_stats.argtypes = [vp, C.POINTER(RolloutDesc), C.POINTER(RolloutStatsDesc), vp]
    L.pgas_m_filter.restype = C.c_int
    L.pgas_m_filter.argtypes = [vp, C.POINTER(RolloutDesc), C.POINTER(ModelFilterDesc), vp]
    L.pgas_m_forecast.restype = C.c_int
    L.pgas_m_forecast.argtypes = [vp, C.POINTER(RolloutDesc), C.POINTER(ModelForecastDesc), vp]
    L.pgas_m_forecast_origins_per_block.restype = C.c_int
    L.pgas_m_forecast_origins_per_block.argtypes = []
    L.pgas_m_rollout_cdf.restype = C.c_int
    L.pgas_m_rollout_cdf.argtypes = [vp, C.POINTER(RolloutDesc), C.POINTER(ModelRolloutCdfDesc), vp]
    L.pgas_m_forecast_cdf.restype = C.c_int
    L.pgas_m_forecast_cdf.argtypes = [vp, C.POINTER(RolloutDesc), C.POINTER(ModelForecastCdfDesc), vp]
    L.pgas_m_smooth.restype = C.c_int
    L.pgas_m_smooth.argtypes = [vp, C.POINTER(RolloutDesc), C.POINTER(ModelSmoothDesc), vp]
    _lib = L
    return L


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _ptr(t):
    """a device tensor's address, None (NULL) for None"""
    return None if t is None else t.data_ptr()


def _hp(a):
    return a.ctypes.data_as(_dp)


def detmath_eval(which, x=None, y=None, words=None, device=None):
    """Test hook (pgas_detmath_eval): the shared arithmetic primitives evaluated on the device; returns numpy arrays (out0, out1, words).
    which = 0 exp(x), 1 log(x), 2 sin(pi x) / cos(pi x), 3 Philox4x32-10 of `words` (6 per element), 4 pgas_seg_ref(x), 5 pgas_seg_arg(x, y),
    6 pgas_lvl_scale(x, y), 7 Box-Muller pair of the Philox block of `words`, 8 the segment scans' quantised numerator dev_exp_q51_n(x) =
    rint(exp(x) 2^51) for x <= 0.25 (NaN and -inf give 0), returned as a double (q < 2^52 is exact), 9 the device-only Box-Muller chain of the
    SingleMassOscillator k_propagate on GIVEN Philox output blocks (`words`: 6 per element, the first four are the block), 10 the
    device-only guarded sin(pi x) / cos(pi x)."""
    L = load()
    dev = torch.device("cuda", torch.cuda.current_device() if device is None else torch.device(device).index or 0)
    f = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)  # noqa: E731
    xd, yd = f(x), f(y)
    wd = None if words is None else torch.as_tensor(np.ascontiguousarray(words, dtype=np.uint32).view(np.int32), device=dev)
    n = int(xd.numel()) if xd is not None else int(wd.numel() // 6)
    o0 = torch.empty(n, dtype=torch.float64, device=dev)
    o1 = torch.empty(n, dtype=torch.float64, device=dev)
    ow = torch.empty(4 * n, dtype=torch.int32, device=dev)
    p = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
    rc = L.pgas_detmath_eval(dev.index, int(which), p(xd), p(yd), p(wd), n, o0.data_ptr(), o1.data_ptr(), ow.data_ptr(),
                             C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc != 0:
        raise PgasError(f"pgas_detmath_eval failed ({rc})")
    torch.cuda.synchronize(dev)
    return o0.cpu().numpy(), o1.cpu().numpy(), ow.cpu().numpy().view(np.uint32).reshape(n, 4)


def student_t_host(seed, stream, t, nu, p0=0):
    """Student-t variates of counters (particle p0 .. p0 + len(nu) - 1, t, stream) computed on the HOST by the library's own arithmetic:
    bit-identical to what k_rng_student_t produces on the device (pgas_m_rng_student_t_host)."""
    nu = np.ascontiguousarray(np.atleast_1d(nu), dtype=np.float64)
    out = np.empty_like(nu)
    rc = load().pgas_m_rng_student_t_host(int(seed), int(stream), int(t), int(p0), nu.size, _hp(nu), _hp(out))
    if rc != 0:
        raise PgasError(f"pgas_m_rng_student_t_host failed ({rc})")
    return out


class _DevView:
    """Minimal __cuda_array_interface__ carrier so torch can wrap library-owned device memory."""

    def __init__(self, ptr, shape, typestr, owner):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2}
        self._owner = owner


class Engine:
    """One pgas_ctx: model tables on the device + launch methods on torch tensors."""

    def __init__(self, N, observations, inputs, init_state_mean, init_state_cov, likelihood, basis_map, device=None, keep_logw_trace=False):
        if not torch.cuda.is_available():
            raise PgasError("no HIP device visible: the engine has no CPU path")
        self.lib = load()
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else torch.device(device).index or 0)
        y = _f64(observations)
        self.T = y.shape[0]
        y = y.reshape(self.T, -1)
        u = _f64(inputs).reshape(self.T, -1) if inputs is not None and np.size(inputs) else np.zeros((self.T, 0))
        m0 = _f64(init_state_mean).reshape(-1)
        self.N, self.nx, self.ny, self.nu = int(N), m0.shape[0], y.shape[1], u.shape[1]
        if likelihood.nx != self.nx or likelihood.ny != self.ny:
            raise ValueError("likelihood dimensions do not match the state / observation dimensions")
        b = basis_map.basis
        self.M, self.D = b.M, b.D
        self._keep = dict(
            idx=np.ascontiguousarray(b.indices, dtype=np.int32), sel=np.ascontiguousarray(basis_map.sel, dtype=np.int32),
            alpha=_f64(basis_map.alpha), beta=_f64(basis_map.beta), H=_f64(likelihood.H), LRinv=_f64(likelihood.LRinv),
            m0=m0, L0=_f64(np.linalg.cholesky(np.atleast_2d(_f64(init_state_cov)))), y=y, u=u if self.nu else np.zeros(1),
        )
        self.LR = _f64(likelihood.LR if hasattr(likelihood, "LR") else np.linalg.inv(likelihood.LRinv)).reshape(self.ny, self.ny)   # rollout_stats
        k = self._keep
        d = _ModelDesc(
            self.N, self.T, self.nx, self.ny, self.nu, self.M, self.D,
            k["idx"].ctypes.data_as(_ip), k["sel"].ctypes.data_as(_ip), _hp(k["alpha"]), _hp(k["beta"]), b.norm,
            _hp(k["H"]), _hp(k["LRinv"]), likelihood.cR, _hp(k["m0"]), _hp(k["L0"]), _hp(k["y"]),
            _hp(k["u"]) if self.nu else None, self.device.index, 1 if keep_logw_trace else 0,
            1 if os.environ.get("PGAS_NO_FAST_VARIANT", "0") == "1" else 0,
        )
        h = C.c_void_p()
        rc = self.lib.pgas_create(C.byref(d), C.byref(h))
        if rc != 0:
            raise PgasError(f"pgas_create failed ({rc}): {self.lib.pgas_last_error(None).decode()}")
        self._h = h
        self.keep_logw_trace = bool(keep_logw_trace)
        if os.environ.get("PGAS_STEP_GENERIC", "0") == "1":   # A/B switch for programs that set no options of their own (tools/ab_bench.py)
            self._chk(self.lib.pgas_set_option(self._h, self.OPT_STEP_GENERIC, 1), "pgas_set_option")

    def close(self):
        if getattr(self, "_h", None):
            self.lib.pgas_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -------------------------------------------------------------- helpers
    def _chk(self, rc, what):
        if rc != 0:
            raise PgasError(f"{what} failed ({rc}): {self.lib.pgas_last_error(self._h).decode()}")

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _dev(self, t, dtype=torch.float64, shape=None):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous()):
            t = torch.as_tensor(np.asarray(t) if not isinstance(t, torch.Tensor) else t, dtype=dtype, device=self.device).contiguous()
        if shape is not None and tuple(t.shape) != tuple(shape):
            t = t.reshape(shape).contiguous()
        return t

    # -------------------------------------------------------------- calls
    def set_params(self, coeff_mat, error_cov):
        """coeff_mat (nx,M) tensor/array, error_cov (nx,nx).  An error_cov that already lives on the engine's device is factored THERE
        (pgas_set_params_dev: no synchronisation, no host round trip -- the Gibbs loop's case) and None is returned; a host array is
        factored with NumPy and (LS, LSinv, cS) returned.  The two factorisations agree to rounding, not bit for bit: get_params() reads
        back what the kernels use."""
        A = self._dev(coeff_mat, shape=(self.nx, self.M))
        if isinstance(error_cov, torch.Tensor) and error_cov.is_cuda and error_cov.device == self.device and os.environ.get("PGAS_HOST_PARAMS", "0") != "1":
            Sd = error_cov.detach().to(torch.float64).reshape(self.nx, self.nx).contiguous()
            self._A, self._S = A, Sd   # keep alive until the pack kernel has run
            self._chk(self.lib.pgas_set_params_dev(self._h, A.data_ptr(), Sd.data_ptr(), self._stream()), "pgas_set_params_dev")
            return None
        S = np.atleast_2d(np.asarray(error_cov.detach().cpu() if isinstance(error_cov, torch.Tensor) else error_cov, dtype=np.float64))
        LS = _f64(np.linalg.cholesky(S))
        LSinv = _f64(np.linalg.inv(LS))
        cS = float(-0.5 * self.nx * np.log(2 * np.pi) - np.sum(np.log(np.diag(LS))))
        self._A = A  # keep alive until the pack kernel has run
        self._chk(self.lib.pgas_set_params(self._h, A.data_ptr(), _hp(LS), _hp(LSinv), cS, self._stream()), "pgas_set_params")
        return LS, LSinv, cS

    def get_params(self):
        """(LS, LSinv, cS) the kernels currently use (synchronises): Cholesky factor of error_cov, its inverse, the normalising constant."""
        LS, LSinv, cS = np.zeros((self.nx, self.nx)), np.zeros((self.nx, self.nx)), C.c_double()
        self._chk(self.lib.pgas_get_params(self._h, _hp(LS), _hp(LSinv), C.byref(cS), self._stream()), "pgas_get_params")
        return LS, LSinv, float(cS.value)

    def basis_eval(self, x, t):
        x = self._dev(x).reshape(-1, self.nx)
        phi = torch.empty((x.shape[0], self.M), dtype=torch.float64, device=self.device)
        self._chk(self.lib.pgas_basis_eval(self._h, x.data_ptr(), x.shape[0], t, phi.data_ptr(), self._stream()), "pgas_basis_eval")
        return phi

    def aux_states(self, x, t):
        x = self._dev(x, shape=(self.N, self.nx))
        aux = torch.empty_like(x)
        self._chk(self.lib.pgas_aux_states(self._h, x.data_ptr(), t, aux.data_ptr(), self._stream()), "pgas_aux_states")
        return aux

    def init_state(self, seed, ref0):
        x0 = torch.empty((self.N, self.nx), dtype=torch.float64, device=self.device)
        r = _f64(ref0).reshape(self.nx)
        self._chk(self.lib.pgas_init_state(self._h, seed, _hp(r), x0.data_ptr(), self._stream()), "pgas_init_state")
        torch.cuda.current_stream(self.device).synchronize()  # r is host memory read asynchronously
        return x0

    def step(self, t, seed, log_weights, state, ref_t):
        x = self._dev(state, shape=(self.N, self.nx))
        lw = None if log_weights is None else self._dev(log_weights, shape=(self.N,))
        r = _f64(ref_t.detach().cpu() if isinstance(ref_t, torch.Tensor) else ref_t).reshape(self.nx)
        lw_new = torch.empty(self.N, dtype=torch.float64, device=self.device)
        x_new = torch.empty((self.N, self.nx), dtype=torch.float64, device=self.device)
        anc = torch.empty(self.N, dtype=torch.int32, device=self.device)
        self._chk(
            self.lib.pgas_step(self._h, t, seed, None if lw is None else lw.data_ptr(), x.data_ptr(), _hp(r), lw_new.data_ptr(),
                               x_new.data_ptr(), anc.data_ptr(), self._stream()),
            "pgas_step",
        )
        torch.cuda.current_stream(self.device).synchronize()
        return lw_new, x_new, anc

    def sweep(self, seed, ref_state):
        ref = self._dev(ref_state, shape=(self.T, self.nx))
        traj = torch.empty((self.T, self.nx), dtype=torch.float64, device=self.device)
        self._chk(self.lib.pgas_sweep(self._h, seed, ref.data_ptr(), traj.data_ptr(), self._stream()), "pgas_sweep")
        self._ref_keepalive = ref
        return traj

    TRACE_X, TRACE_LA, TRACE_H, TRACE_LN, TRACE_ANC = range(5)

    def trace_layout(self, kind):
        """(rows, rows per block, blocks, bytes per row) of trace `kind` (pgas_trace_layout)."""
        v = (C.c_int64 * 4)()
        self._chk(self.lib.pgas_trace_layout(self._h, int(kind), v), "pgas_trace_layout")
        return tuple(int(x) for x in v)

    def trace_row(self, kind, t):
        """Device pointer of time row t of trace `kind` (pgas_trace_row)."""
        p = C.c_void_p()
        self._chk(self.lib.pgas_trace_row(self._h, int(kind), int(t), C.byref(p)), "pgas_trace_row")
        return int(p.value)

    def traces_blocks(self, kind, row_shape, dtype):
        """The row blocks of trace `kind` as torch views of library-owned memory, in time order."""
        rows, rpb, nblk, _ = self.trace_layout(kind)
        return [self.dev_tensor(self.trace_row(kind, b * rpb), (min(rpb, rows - b * rpb),) + tuple(row_shape), dtype) for b in range(nblk)]

    def traces(self, copy_blocks=True):
        """(state_trace (T,N,nx), ancestor_trace (T-1,N) int32, logw_last (N), logw_trace (T,N)|None).  Views of library-owned memory on
        an unsharded context; a context that keeps its traces in row blocks (shards, PGAS_OPT_TRACE_BLOCK_BYTES) returns concatenated
        COPIES of x / ancestors (None with copy_blocks=False: use traces_blocks for views of the blocks)."""
        px, pa, pl, pt = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        if self.trace_layout(self.TRACE_X)[2] == 1 and self.trace_layout(self.TRACE_ANC)[2] == 1:
            px.value, pa.value = self.trace_row(self.TRACE_X, 0), self.trace_row(self.TRACE_ANC, 0)
            X = torch.as_tensor(_DevView(px.value, (self.T, self.N, self.nx), "<f8", self), device=self.device)
            A = torch.as_tensor(_DevView(pa.value, (max(self.T - 1, 1), self.N), "<i4", self), device=self.device)
        elif copy_blocks:
            X = torch.cat(self.traces_blocks(self.TRACE_X, (self.N, self.nx), torch.float64))
            A = torch.cat(self.traces_blocks(self.TRACE_ANC, (self.N,), torch.int32))
        else:
            X = A = None
        self._chk(self.lib.pgas_get_traces(self._h, None, None, C.byref(pl), C.byref(pt)), "pgas_get_traces")
        Lw = torch.as_tensor(_DevView(pl.value, (self.N,), "<f8", self), device=self.device)
        Lt = torch.as_tensor(_DevView(pt.value, (self.T, self.N), "<f8", self), device=self.device) if pt.value else None
        return X, A, Lw, Lt

    def last_final_index(self):
        v = C.c_int64()
        self._chk(self.lib.pgas_last_final_index(self._h, C.byref(v), self._stream()), "pgas_last_final_index")
        return int(v.value)

    def scan_gave_up(self):
        """True when a scanner wave of k_step (PGAS_OPT_TAIL_GROUPS) ever ran out of its bounded wait on this context (synchronises)."""
        v = C.c_int32()
        self._chk(self.lib.pgas_scan_status(self._h, C.byref(v), self._stream()), "pgas_scan_status")
        return bool(v.value)

    def set_profiling(self, on):
        """False/0 = off, True/1 = on at the default sampling stride, n > 1 = time every n-th launch."""
        self._chk(self.lib.pgas_set_profiling(self._h, int(on)), "pgas_set_profiling")

    def profile(self):
        """(k_step launches, their total ms, k_propagate launches, their total ms) of the last sweep (synchronises)."""
        n, ms, pn, pm = C.c_int64(), C.c_double(), C.c_int64(), C.c_double()
        self._chk(self.lib.pgas_get_profile(self._h, C.byref(n), C.byref(ms), C.byref(pn), C.byref(pm), self._stream()), "pgas_get_profile")
        return int(n.value), float(ms.value), int(pn.value), float(pm.value)

    OPT_STEP_GENERIC = 16   # PGAS_OPT_STEP_GENERIC: 1 = k_step's and k_propagate's general instances also where the whole-segment ones apply

    def set_option(self, option, value):
        self._chk(self.lib.pgas_set_option(self._h, int(option), int(value)), "pgas_set_option")

    # -------------------------------------------------------------- src/Filtering.py free functions
    _utility = {}

    @classmethod
    def utility(cls, N, device=None):
        """A context that only serves pgas_systematic_resample / pgas_reconstruct_trajectory for N particles (trivial model)."""
        from .descriptors import BasisMap, GaussianLikelihood, HilbertBasis

        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        key = (dev.index or 0, int(N))
        if key not in cls._utility:
            basis = HilbertBasis(np.array([[1]], dtype=np.int32), np.array([[-1.0, 1.0]]))
            cls._utility[key] = cls(int(N), np.zeros((1, 1)), None, np.zeros(1), np.eye(1), GaussianLikelihood(np.eye(1), np.eye(1)),
                                    BasisMap(basis, [0]), device=dev)
        return cls._utility[key]

    def systematic_resample(self, u, logw):
        """u: a float, or a device tensor holding the uniform (read at execution time: graph-captured steps)."""
        lw = self._dev(logw, shape=(self.N,))
        idx = torch.empty(self.N, dtype=torch.int32, device=self.device)
        if isinstance(u, torch.Tensor):
            self._chk(self.lib.pgas_systematic_resample_dev(self._h, u.data_ptr(), lw.data_ptr(), idx.data_ptr(), self._stream()), "pgas_systematic_resample_dev")
        else:
            self._chk(self.lib.pgas_systematic_resample(self._h, float(u), lw.data_ptr(), idx.data_ptr(), self._stream()), "pgas_systematic_resample")
        return idx

    def reconstruct_trajectory(self, particles, ancestry, idx):
        P = particles if isinstance(particles, torch.Tensor) else torch.as_tensor(np.asarray(particles, dtype=np.float64))
        P = P.to(device=self.device, dtype=torch.float64)
        if P.dim() == 2:
            P = P.unsqueeze(-1)
        P = P.contiguous()
        T, N, nx = P.shape
        if N != self.N:
            raise ValueError(f"particle count {N} does not match the context ({self.N})")
        A = ancestry if isinstance(ancestry, torch.Tensor) else torch.as_tensor(np.asarray(ancestry))
        A = A.to(device=self.device, dtype=torch.int32).contiguous()   # the reference stores float64 indices (Q2)
        traj = torch.empty((T, nx), dtype=torch.float64, device=self.device)
        self._chk(self.lib.pgas_reconstruct_trajectory(self._h, P.data_ptr(), A.data_ptr(), T, nx, int(idx), traj.data_ptr(), self._stream()),
                  "pgas_reconstruct_trajectory")
        return traj

    # -------------------------------------------------------------- particle sharding (pgas_amd/sharded.py)
    def shard_setup(self, rank, world):
        self._chk(self.lib.pgas_shard_setup(self._h, rank, world), "pgas_shard_setup")
        self.rank, self.world = rank, world

    def shard_buffers(self):
        """(list of 17 device pointers, (nsegp, N_local, T)) -- see include/pgas_hip.h."""
        out = (C.c_void_p * 17)()
        sz = (C.c_int64 * 3)()
        self._chk(self.lib.pgas_shard_buffers(self._h, out, sz), "pgas_shard_buffers")
        return [int(p or 0) for p in out], tuple(int(v) for v in sz)

    def shard_layout(self, which):
        """(blocks, rows per block) of peer-visible buffer `which` (0, 1: segment cumsums; 2..6: la, h, ln, x, anc)."""
        v = (C.c_int64 * 2)()
        self._chk(self.lib.pgas_shard_layout(self._h, int(which), v), "pgas_shard_layout")
        return int(v[0]), int(v[1])

    def shard_block(self, which, blk):
        """(device pointer, bytes) of block `blk` of this rank's buffer `which`."""
        p, n = C.c_void_p(), C.c_int64()
        self._chk(self.lib.pgas_shard_block(self._h, int(which), int(blk), C.byref(p), C.byref(n)), "pgas_shard_block")
        return int(p.value), int(n.value)

    def shard_set_peer_block(self, peer, which, blk, ptr):
        self._chk(self.lib.pgas_shard_set_peer_block(self._h, int(peer), int(which), int(blk), C.c_void_p(int(ptr))), "pgas_shard_set_peer_block")

    def shard_run(self, phase, t=0, t_aux=0, seed=0, ref=None, traj=None):
        self._chk(
            self.lib.pgas_shard_run(self._h, phase, t, t_aux, seed, None if ref is None else ref.data_ptr(),
                                    None if traj is None else traj.data_ptr(), self._stream()),
            "pgas_shard_run",
        )

    def shard_unique_id(self):
        buf = C.create_string_buffer(128)
        rc = self.lib.pgas_shard_unique_id(buf)
        if rc:
            raise PgasError("pgas_shard_unique_id failed (librccl.so not loadable?)")
        return bytes(buf.raw)

    def shard_comm_init(self, id128):
        self._chk(self.lib.pgas_shard_comm_init(self._h, id128), "pgas_shard_comm_init")

    def shard_set_collective(self, fn):
        """Install a host all-gather `fn(parity, stream_ptr) -> int` in place of RCCL for pgas_shard_sweep (tests); None removes it."""
        if fn is None:
            self._ag_cb = None
            self._chk(self.lib.pgas_shard_set_collective(self._h, C.cast(None, ALLGATHER_FN), None), "pgas_shard_set_collective")
            return

        def tramp(user, parity, stream):
            try:
                return int(fn(int(parity), stream) or 0)
            except Exception as exc:  # an exception must not unwind through the C frames
                import traceback

                self._ag_error = "".join(traceback.format_exception(type(exc), exc, exc.__traceback__))
                return -1

        self._ag_cb = ALLGATHER_FN(tramp)   # keep the trampoline alive as long as the library may call it
        self._chk(self.lib.pgas_shard_set_collective(self._h, self._ag_cb, None), "pgas_shard_set_collective")

    def shard_probe_collective(self, reps=200):
        """Mean duration (us) of the step's RCCL all-gather issued `reps` times back to back on an idle stream; None without RCCL."""
        if getattr(self, "_ag_cb", None) is not None:
            return None
        torch.cuda.synchronize(self.device)
        self._chk(self.lib.pgas_shard_probe_collective(self._h, 3, self._stream()), "pgas_shard_probe_collective")   # warm-up
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        self._chk(self.lib.pgas_shard_probe_collective(self._h, int(reps), self._stream()), "pgas_shard_probe_collective")
        e1.record()
        torch.cuda.synchronize(self.device)
        return e0.elapsed_time(e1) * 1e3 / reps

    def launch_info(self):
        """dict(chunk, local_groups, JP, P) of the last sweep (pgas_get_launch_info)."""
        v = (C.c_int32 * 4)()
        self._chk(self.lib.pgas_get_launch_info(self._h, v), "pgas_get_launch_info")
        g = int(v[1]) & 15
        return dict(chunk=int(v[0]), local_groups=g == 1, groups={0: "k_groups", 1: "local", 2: "tail", 3: "small"}[g], small=g == 3, graph=bool(int(v[1]) & 16), mfma=bool(int(v[1]) & 32),
                    step_instance="full" if int(v[1]) & 64 else "generic", propagate_instance="full" if int(v[1]) & 128 else "generic", JP=int(v[2]), P=int(v[3]))

    def shard_sweep(self, seed, ref, traj, propagate_chunk=0):
        self._ag_error = None
        rc = self.lib.pgas_shard_sweep(self._h, int(seed), ref.data_ptr(), traj.data_ptr(), int(propagate_chunk), self._stream())
        if rc != 0 and getattr(self, "_ag_error", None):
            raise PgasError(f"pgas_shard_sweep: the all-gather callback raised:\n{self._ag_error}")
        self._chk(rc, "pgas_shard_sweep")

    def ipc_export(self, which, blk=0):
        buf = C.create_string_buffer(64)
        self._chk(self.lib.pgas_ipc_export(self._h, int(which), int(blk), buf), "pgas_ipc_export")
        return bytes(buf.raw)

    def ipc_open(self, handle):
        p = C.c_void_p()
        self._chk(self.lib.pgas_ipc_open(self._h, handle, C.byref(p)), "pgas_ipc_open")
        return int(p.value)

    def dev_tensor(self, ptr, shape, dtype):
        """torch view of library-owned device memory."""
        typestr = {torch.float64: "<f8", torch.int64: "<i8", torch.int32: "<i4"}[dtype]
        return torch.as_tensor(_DevView(ptr, shape, typestr, self), device=self.device)

    def rng_normal(self, seed, stream, t, n, ncol=1):
        """(n, ncol) standard normals of counters (particle 0..n-1, t, stream) -- Philox + Box-Muller on the device (k_rng_normal)."""
        out = torch.empty((int(n), int(ncol)), dtype=torch.float64, device=self.device)
        self._chk(self.lib.pgas_m_rng_normal(self._h, int(seed), int(stream), int(t), 0, int(n), int(ncol), out.data_ptr(), self._stream()), "pgas_m_rng_normal")
        return out

    def rng_chi2(self, seed, stream, t, nu):
        """chi^2(nu_p) variates for a device vector nu (k_rng_chi2)."""
        nu = nu.to(device=self.device, dtype=torch.float64).contiguous()
        out = torch.empty_like(nu)
        self._chk(self.lib.pgas_m_rng_chi2(self._h, int(seed), int(stream), int(t), 0, nu.numel(), nu.data_ptr(), out.data_ptr(), self._stream()), "pgas_m_rng_chi2")
        return out

    def suffstats(self, traj):
        traj = self._dev(traj, shape=(self.T, self.nx))
        T0 = torch.empty((self.M, self.nx), dtype=torch.float64, device=self.device)
        T1 = torch.empty((self.M, self.M), dtype=torch.float64, device=self.device)
        T2 = torch.empty((self.nx, self.nx), dtype=torch.float64, device=self.device)
        self._chk(self.lib.pgas_suffstats(self._h, traj.data_ptr(), T0.data_ptr(), T1.data_ptr(), T2.data_ptr(), self._stream()), "pgas_suffstats")
        return T0, T1, T2, float(self.T - 1)

    # -------------------------------------------------------------- C independent chains (pgas_chains_*; pgas_amd/chains.py)
    # Keys travel as int64 tensors holding the u64 bit patterns.
    def chains_set_params(self, coeff_mat, error_cov):
        """coeff_mat (C, nx, M), error_cov (C, nx, nx) device tensors: chain c's transition parameters, factored on the device."""
        n = int(coeff_mat.shape[0])
        A = self._dev(coeff_mat, shape=(n, self.nx, self.M))
        S = self._dev(error_cov, shape=(n, self.nx, self.nx))
        self._ch_params = (A, S)   # keep alive until the pack kernel has run
        self._chk(self.lib.pgas_chains_set_params_dev(self._h, n, A.data_ptr(), S.data_ptr(), self._stream()), "pgas_chains_set_params_dev")

    def chains_sweep(self, seeds, ref):
        """seeds (C,) int64 device tensor, ref (C, T, nx) -> traj (C, T, nx): one sweep per chain, all in one launch."""
        n = int(seeds.shape[0])
        seeds = self._dev(seeds, dtype=torch.int64, shape=(n,))
        ref = self._dev(ref, shape=(n, self.T, self.nx))
        traj = torch.empty((n, self.T, self.nx), dtype=torch.float64, device=self.device)
        self._chk(self.lib.pgas_chains_sweep(self._h, n, seeds.data_ptr(), ref.data_ptr(), traj.data_ptr(), self._stream()), "pgas_chains_sweep")
        self._ch_keepalive = (seeds, ref)
        return traj

    def chains_traces(self, n):
        """(state traces (C, T, N, nx), ancestor traces (C, T-1, N) int32, last log-weights (C, N)) of the last batched sweep: views of
        library-owned memory, valid until the next batched sweep."""
        px, pa, pl = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._chk(self.lib.pgas_chains_get_traces(self._h, C.byref(px), C.byref(pa), C.byref(pl)), "pgas_chains_get_traces")
        n = int(n)
        return (self.dev_tensor(px.value, (n, self.T, self.N, self.nx), torch.float64),
                self.dev_tensor(pa.value, (n, max(self.T - 1, 1), self.N), torch.int32),
                self.dev_tensor(pl.value, (n, self.N), torch.float64))

    def chains_final_index(self, n):
        """Final indices of the last batched sweep's chains (synchronises)."""
        v = (C.c_int64 * int(n))()
        self._chk(self.lib.pgas_chains_final_index(self._h, int(n), v, self._stream()), "pgas_chains_final_index")
        return np.array(v[:], dtype=np.int64)

    def chains_keys(self, keys, first):
        """keys (C,) int64 device tensor -> (6, C): next key, step key, parameter key, key_A, key_chi, key_norm (pgas_chains_keys)."""
        n = int(keys.shape[0])
        keys = self._dev(keys, dtype=torch.int64, shape=(n,))
        out = torch.empty((6, n), dtype=torch.int64, device=self.device)
        self._chk(self.lib.pgas_chains_keys(self._h, n, keys.data_ptr(), 1 if first else 0, out.data_ptr(), self._stream()), "pgas_chains_keys")
        return out

    def chains_param_draws(self, keys6, df):
        """dict(chi2 (C, nx), normals_T (C, nx, nx), normals_A (C, nx, M)) from the parameter keys of a chains_keys block."""
        n = int(keys6.shape[1])
        keys6 = self._dev(keys6, dtype=torch.int64, shape=(6, n))
        f = lambda *s: torch.empty(s, dtype=torch.float64, device=self.device)  # noqa: E731
        d = dict(chi2=f(n, self.nx), normals_T=f(n, self.nx, self.nx), normals_A=f(n, self.nx, self.M))
        self._chk(self.lib.pgas_chains_param_draws(self._h, n, keys6.data_ptr(), float(df), d["chi2"].data_ptr(), d["normals_T"].data_ptr(),
                                                   d["normals_A"].data_ptr(), self._stream()), "pgas_chains_param_draws")
        return d

    def chains_suffstats(self, traj):
        """traj (C, T, nx) -> T0 (C, M, nx), T1 (C, M, M), T2 (C, nx, nx), T3 = T - 1 in one set of launches."""
        n = int(traj.shape[0])
        traj = self._dev(traj, shape=(n, self.T, self.nx))
        T0 = torch.empty((n, self.M, self.nx), dtype=torch.float64, device=self.device)
        T1 = torch.empty((n, self.M, self.M), dtype=torch.float64, device=self.device)
        T2 = torch.empty((n, self.nx, self.nx), dtype=torch.float64, device=self.device)
        self._chk(self.lib.pgas_chains_suffstats(self._h, n, traj.data_ptr(), T0.data_ptr(), T1.data_ptr(), T2.data_ptr(), self._stream()),
                  "pgas_chains_suffstats")
        return T0, T1, T2, float(self.T - 1)

    # -------------------------------------------------------------- E records that share the model (pgas_records_*; pgas_amd/records.py)
    def records_set(self, row0, init_state_mean=None, init_state_cov=None):
        """row0 (E + 1,): record e is rows row0[e] .. row0[e + 1] - 1 of this context's observations / inputs (row0[0] = 0, row0[E] = T,
        every record at least 2 rows); init_state_mean (E, nx) / init_state_cov (E, nx, nx) per record, or None for the context's own."""
        r = np.ascontiguousarray(np.asarray(row0).reshape(-1), dtype=np.int32)
        if r.shape[0] < 2 or not np.array_equal(r, np.asarray(row0).reshape(-1)):
            raise ValueError("row0: expected E + 1 >= 2 integer row numbers")
        E = r.shape[0] - 1
        m0 = P0 = None
        if init_state_mean is not None:
            m0 = _f64(init_state_mean)
            if m0.shape != (E, self.nx):
                raise ValueError(f"init_state_mean: expected shape {(E, self.nx)}, got {m0.shape}")
        if init_state_cov is not None:
            P0 = _f64(init_state_cov)
            if P0.shape != (E, self.nx, self.nx):
                raise ValueError(f"init_state_cov: expected shape {(E, self.nx, self.nx)}, got {P0.shape}")
        self._chk(self.lib.pgas_records_set(self._h, E, r.ctypes.data_as(_ip), None if m0 is None else _hp(m0), None if P0 is None else _hp(P0)),
                  "pgas_records_set")
        self.E, self.row0 = E, r.astype(np.int64)

    def _records(self):
        E = getattr(self, "E", 0)
        if not E:   # let the library refuse (PGAS_E_STATE) with its own message; the shapes below then do not matter
            return 1
        return E

    def records_seeds(self, step_keys):
        """step_keys (C,) int64 device tensor -> seeds (C, E): column 0 the step keys, column e >= 1 child e of the step key."""
        n = int(step_keys.shape[0])
        step_keys = self._dev(step_keys, dtype=torch.int64, shape=(n,))
        out = torch.empty((n, self._records()), dtype=torch.int64, device=self.device)
        self._chk(self.lib.pgas_records_seeds(self._h, n, step_keys.data_ptr(), out.data_ptr(), self._stream()), "pgas_records_seeds")
        return out

    def records_sweep(self, seeds, ref):
        """seeds (C, E) int64 device tensor, ref (C, T, nx) -> traj (C, T, nx): one sweep per (chain, record), all in one launch."""
        n, E = int(seeds.shape[0]), self._records()
        seeds = self._dev(seeds, dtype=torch.int64, shape=(n, E))
        ref = self._dev(ref, shape=(n, self.T, self.nx))
        traj = torch.empty((n, self.T, self.nx), dtype=torch.float64, device=self.device)
        self._chk(self.lib.pgas_records_sweep(self._h, n, seeds.data_ptr(), ref.data_ptr(), traj.data_ptr(), self._stream()), "pgas_records_sweep")
        self._rc_keepalive = (seeds, ref)
        return traj

    def records_traces(self, n):
        """(state traces (C, T, N, nx), ancestor traces (C, T, N) int32 -- record e's T_e - 1 rows start at row0[e], the last row of each
        record is unused --, last log-weights (C, E, N)) of the last record sweep: views of library-owned memory, valid until the next
        sweep or parameter call."""
        px, pa, pl = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._chk(self.lib.pgas_records_get_traces(self._h, C.byref(px), C.byref(pa), C.byref(pl)), "pgas_records_get_traces")
        n = int(n)
        return (self.dev_tensor(px.value, (n, self.T, self.N, self.nx), torch.float64),
                self.dev_tensor(pa.value, (n, self.T, self.N), torch.int32),
                self.dev_tensor(pl.value, (n, self._records(), self.N), torch.float64))

    def records_final_index(self, n):
        """Final indices (C, E) of the last record sweep (synchronises)."""
        n, E = int(n), self._records()
        v = (C.c_int64 * (n * E))()
        self._chk(self.lib.pgas_records_final_index(self._h, n, v, self._stream()), "pgas_records_final_index")
        return np.array(v[:], dtype=np.int64).reshape(n, E)

    def records_suffstats(self, traj):
        """traj (C, T, nx) -> T0 (C, M, nx), T1 (C, M, M), T2 (C, nx, nx) summed over the records (no pair across a seam), T3 = sum (T_e - 1)."""
        n = int(traj.shape[0])
        traj = self._dev(traj, shape=(n, self.T, self.nx))
        T0 = torch.empty((n, self.M, self.nx), dtype=torch.float64, device=self.device)
        T1 = torch.empty((n, self.M, self.M), dtype=torch.float64, device=self.device)
        T2 = torch.empty((n, self.nx, self.nx), dtype=torch.float64, device=self.device)
        self._chk(self.lib.pgas_records_suffstats(self._h, n, traj.data_ptr(), T0.data_ptr(), T1.data_ptr(), T2.data_ptr(), self._stream()),
                  "pgas_records_suffstats")
        return T0, T1, T2, float(self.T - self._records())

    # -------------------------------------------------------------- the draw-batch entry points' operands, on the device in their shapes
    def _draw_operands(self, coeff_mat, error_cov, seeds):
        """(K, coeff_mat (K, nx, M), error_cov (K, nx, nx) or None, seeds (K,) int64 or None)"""
        n = int(coeff_mat.shape[0])
        A = self._dev(coeff_mat, shape=(n, self.nx, self.M))
        S = None if error_cov is None else self._dev(error_cov, shape=(n, self.nx, self.nx))
        sd = None if seeds is None else self._dev(seeds, dtype=torch.int64, shape=(n,))
        return n, A, S, sd

    def _x0_operand(self, x0, x0_mode, n, P):
        return None if x0 is None else self._dev(x0, shape={1: (self.nx,), 2: (n, self.nx), 3: (n, P, self.nx)}[int(x0_mode)])

    def _thresholds_operand(self, thresholds):
        """(thresholds (T, nx + ny, J) or None, J)"""
        th = None if thresholds is None else self._dev(thresholds)
        J, nv = 0 if th is None else int(th.shape[-1]), self.nx + self.ny
        if th is not None and tuple(th.shape) != (self.T, nv, J):
            raise ValueError(f"thresholds: expected ({self.T}, {nv}, J), got {tuple(th.shape)}")
        return th, J

    # -------------------------------------------------------------- open-loop simulation under K parameter draws (pgas_amd/rollout.py)
    def rollout(self, coeff_mat, error_cov=None, seeds=None, replicates=1, p0=0, x0=None, x0_mode=0):
        """pgas_rollout: coeff_mat (K, nx, M); error_cov (K, nx, nx) and seeds (K,) int64 together, or neither (noise-free); replicates
        P <= 1024 with global indices p0 .. p0 + P - 1; x0_mode 0 (drawn), 1 x0 (nx), 2 (K, nx), 3 (K, P, nx) -> (K, T, P, nx).  Enqueues work only."""
        P = int(replicates)
        n, A, S, sd = self._draw_operands(coeff_mat, error_cov, seeds)
        xs = self._x0_operand(x0, x0_mode, n, P)
        out = torch.empty((n, self.T, max(P, 0), self.nx), dtype=torch.float64, device=self.device)
        self._chk(self.lib.pgas_rollout(self._h, n, P, int(p0), _ptr(sd), A.data_ptr(), _ptr(S), _ptr(xs), int(x0_mode), out.data_ptr(), self._stream()),
                  "pgas_rollout")
        self._ro_keepalive = (A, S, sd, xs)   # until the kernels have run
        return out

    def rollout_stats(self, coeff_mat, error_cov=None, seeds=None, replicates=1, p0=0, x0=None, x0_mode=0, observation_noise=False, log_score=False):
        """pgas_rollout_stats: the rollout of `rollout` (same arguments, replicates P <= 2^20 in one call) reduced over its replicates in
        the kernel -> (sum (K, T, nx + ny), sumsq (K, T, nx + ny), lpd (K, T) or None): per step the sums of the state and of the predicted
        observation H x (+ LR e with observation_noise) and of their squares, and with log_score the log predictive density of the
        context's observation row under the context's likelihood.  Enqueues work only."""
        P = int(replicates)
        n, A, S, sd = self._draw_operands(coeff_mat, error_cov, seeds)
        xs = self._x0_operand(x0, x0_mode, n, P)
        nv = self.nx + self.ny
        s1 = torch.empty((n, self.T, nv), dtype=torch.float64, device=self.device)
        s2 = torch.empty((n, self.T, nv), dtype=torch.float64, device=self.device)
        lpd = torch.empty((n, self.T), dtype=torch.float64, device=self.device) if log_score else None
        self._chk(self.lib.pgas_rollout_stats(self._h, n, P, int(p0), _ptr(sd), A.data_ptr(), _ptr(S), _ptr(xs), int(x0_mode),
                                              _hp(self.LR) if observation_noise else None, s1.data_ptr(), s2.data_ptr(), _ptr(lpd), self._stream()),
                  "pgas_rollout_stats")
        self._ro_keepalive = (A, S, sd, xs)   # until the kernels have run
        return s1, s2, lpd

    def rollout_cdf(self, coeff_mat, error_cov=None, seeds=None, replicates=1, p0=0, x0=None, x0_mode=0, observation_noise=False, thresholds=None):
        """pgas_rollout_cdf: the rollout of `rollout_stats` (same arguments) counted against thresholds (T, nx + ny, J) fp64, J <= 16 ->
        count (K, T, nx + ny, J) int32, the number of replicates whose value channel (the state, then the predicted observation H x
        (+ LR e with observation_noise)) is <= the threshold; a NaN on either side counts nothing.  Enqueues work only."""
        P = int(replicates)
        n, A, S, sd = self._draw_operands(coeff_mat, error_cov, seeds)
        xs = self._x0_operand(x0, x0_mode, n, P)
        nv = self.nx + self.ny
        th, J = self._thresholds_operand(thresholds)
        count = torch.empty((n, self.T, nv, max(J, 0)), dtype=torch.int32, device=self.device)
        self._chk(self.lib.pgas_rollout_cdf(self._h, n, P, int(p0), _ptr(sd), A.data_ptr(), _ptr(S), _ptr(xs), int(x0_mode),
                                            _hp(self.LR) if observation_noise else None, _ptr(th), J, count.data_ptr(), self._stream()),
                  "pgas_rollout_cdf")
        self._ro_keepalive = (A, S, sd, xs, th)   # until the kernels have run
        return count

    # -------------------------------------------------------------- a bootstrap particle filter per parameter draw (pgas_amd/heldout.py)
    def filter(self, coeff_mat, error_cov, seeds, x0=None, x0_mode=0, moments=True, traces=False):
        """pgas_filter with the context's N particles: coeff_mat (K, nx, M), error_cov (K, nx, nx), seeds (K,) int64; x0_mode 0 (drawn),
        1 x0 (nx), 2 (K, nx), 3 (K, N, nx) -> dict(loglik (K), ell (K, T), and with moments ess (K, T), pred_sum / pred_sumsq
        (K, T, nx + ny), filt_sum (K, T, nx), wtot (K, T), with traces x (K, T, N, nx), anc (K, T, N) int32; None otherwise).
        Enqueues work only."""
        n, A, S, sd = self._draw_operands(coeff_mat, error_cov, seeds)
        xs = self._x0_operand(x0, x0_mode, n, self.N)
        f = lambda *s: torch.empty(s, dtype=torch.float64, device=self.device)  # noqa: E731
        T, nv = self.T, self.nx + self.ny
        o = dict(loglik=f(n), ell=f(n, T), ess=None, pred_sum=None, pred_sumsq=None, filt_sum=None, wtot=None, x=None, anc=None)
        if moments:
            o.update(ess=f(n, T), pred_sum=f(n, T, nv), pred_sumsq=f(n, T, nv), filt_sum=f(n, T, self.nx), wtot=f(n, T))
        if traces:
            o.update(x=f(n, T, self.N, self.nx), anc=torch.empty((n, T, self.N), dtype=torch.int32, device=self.device))
        self._chk(self.lib.pgas_filter(self._h, n, _ptr(sd), A.data_ptr(), _ptr(S), _ptr(xs), int(x0_mode), _ptr(o["ell"]), _ptr(o["loglik"]), _ptr(o["ess"]),
                                       _ptr(o["pred_sum"]), _ptr(o["pred_sumsq"]), _ptr(o["filt_sum"]), _ptr(o["wtot"]), _ptr(o["x"]), _ptr(o["anc"]),
                                       self._stream()), "pgas_filter")
        self._fl_keepalive = (A, S, sd, xs)   # until the kernels have run
        return o

    def forecast(self, coeff_mat, error_cov, seeds, x_trace, horizon, log_score=True):
        """pgas_forecast from the trace x_trace (K, T, N, nx) of a `filter` call with the same parameters and seeds: the h-step-ahead
        clouds for h = 1 .. horizon from every origin row -> (sum (K, H, T, nx + ny), sumsq (K, H, T, nx + ny), lpd (K, H, T) or None) at
        [k, h - 1, target row]; NaN where the target row is < h - 1.  Enqueues work only."""
        H = int(horizon)
        n, A, S, sd = self._draw_operands(coeff_mat, error_cov, seeds)
        xt = None if x_trace is None else self._dev(x_trace, shape=(n, self.T, self.N, self.nx))
        Hs, nv = max(H, 0), self.nx + self.ny
        s1 = torch.empty((n, Hs, self.T, nv), dtype=torch.float64, device=self.device)
        s2 = torch.empty((n, Hs, self.T, nv), dtype=torch.float64, device=self.device)
        lpd = torch.empty((n, Hs, self.T), dtype=torch.float64, device=self.device) if log_score else None
        self._chk(self.lib.pgas_forecast(self._h, n, H, _ptr(sd), A.data_ptr(), _ptr(S), _ptr(xt), s1.data_ptr(), s2.data_ptr(), _ptr(lpd), self._stream()),
                  "pgas_forecast")
        self._fc_keepalive = (A, S, sd, xt)   # until the kernels have run
        return s1, s2, lpd

    def forecast_cdf(self, coeff_mat, error_cov, seeds, x_trace, horizon, thresholds, observation_noise=True):
        """pgas_forecast_cdf: the h-step-ahead clouds of `forecast` (same arguments) counted against the target row's thresholds
        (T, nx + ny, J) fp64, J <= 16 -> count (K, H, T, nx + ny, J) int32 at [k, h - 1, target row]; -1 where the target row is < h - 1.
        observation_noise adds LR e to the predicted observation.  Enqueues work only."""
        H = int(horizon)
        n, A, S, sd = self._draw_operands(coeff_mat, error_cov, seeds)
        xt = None if x_trace is None else self._dev(x_trace, shape=(n, self.T, self.N, self.nx))
        nv = self.nx + self.ny
        th, J = self._thresholds_operand(thresholds)
        count = torch.empty((n, max(H, 0), self.T, nv, max(J, 0)), dtype=torch.int32, device=self.device)
        self._chk(self.lib.pgas_forecast_cdf(self._h, n, H, _ptr(sd), A.data_ptr(), _ptr(S), _ptr(xt), _hp(self.LR) if observation_noise else None, _ptr(th), J,
                                             count.data_ptr(), self._stream()), "pgas_forecast_cdf")
        self._fc_keepalive = (A, S, sd, xt, th)   # until the kernels have run
        return count

    def smooth(self, coeff_mat, error_cov, seeds, x_trace, anc_trace, trajectories, b0=0, moments=True, states=False, indices=False):
        """pgas_smooth from the traces x_trace (K, T, N, nx), anc_trace (K, T, N) int32 of a `filter` call with the same parameters and
        seeds: `trajectories` <= 256 backward-simulation trajectories b0 .. b0 + trajectories - 1 per draw -> (sum (K, T, nx + ny),
        sumsq (K, T, nx + ny), xs (K, B, T, nx), idx (K, B, T) int32), None for what was not asked for.  Enqueues work only."""
        B = int(trajectories)
        n, A, S, sd = self._draw_operands(coeff_mat, error_cov, seeds)
        xt = None if x_trace is None else self._dev(x_trace, shape=(n, self.T, self.N, self.nx))
        at = None if anc_trace is None else self._dev(anc_trace, dtype=torch.int32, shape=(n, self.T, self.N))
        Bs, nv = max(B, 0), self.nx + self.ny
        s1 = torch.empty((n, self.T, nv), dtype=torch.float64, device=self.device) if moments else None
        s2 = torch.empty((n, self.T, nv), dtype=torch.float64, device=self.device) if moments else None
        xs = torch.empty((n, Bs, self.T, self.nx), dtype=torch.float64, device=self.device) if states else None
        idx = torch.empty((n, Bs, self.T), dtype=torch.int32, device=self.device) if indices else None
        self._chk(self.lib.pgas_smooth(self._h, n, B, int(b0), _ptr(sd), A.data_ptr(), _ptr(S), _ptr(xt), _ptr(at), _ptr(idx), _ptr(xs), _ptr(s1), _ptr(s2),
                                       self._stream()), "pgas_smooth")
        self._sm_keepalive = (A, S, sd, xt, at)   # until the kernels have run
        return s1, s2, xs, idx


class MarginalOps:
    """Device primitives of the marginalised family (include/pgas_marginal.h) for N particles on one device: Philox normals /
    uniforms / Student-t variates, batched MNIW solves, statistics gather + update, systematic resampling.  Hand-written HIP
    through the C ABI; there is no CPU path."""

    def __init__(self, N, device=None):
        self.eng = Engine.utility(int(N), device)
        self.N, self.device, self.lib = int(N), self.eng.device, self.eng.lib

    def _ptr(self, t):
        return 0 if t is None else t.data_ptr()

    def _vec(self, n=None, cols=None):
        shape = (self.N if n is None else n,) if cols is None else (self.N if n is None else n, cols)
        return torch.empty(shape, dtype=torch.float64, device=self.device)

    def uniform(self, seed, stream, t):
        return float(self.lib.pgas_m_rng_uniform(int(seed), int(stream), int(t)))

    def set_time_source(self, t_dev):
        """t_dev: a uint32-sized device tensor (int32 works) the random-number kernels read their time index from, or None."""
        self._t_dev = t_dev   # keep it alive
        self.eng._chk(self.lib.pgas_m_set_time_source(self.eng._h, 0 if t_dev is None else t_dev.data_ptr()), "pgas_m_set_time_source")

    def uniform_dev(self, seed, stream, t):
        """The same uniform as `uniform`, produced on the device into a one-element tensor (time index from the time source if set)."""
        out = torch.empty(1, dtype=torch.float64, device=self.device)
        self.eng._chk(self.lib.pgas_m_rng_uniform_dev(self.eng._h, int(seed), int(stream), int(t), out.data_ptr(), self.eng._stream()), "pgas_m_rng_uniform_dev")
        return out

    def normal(self, seed, stream, t, ncol):
        out = self._vec(cols=int(ncol))
        self.eng._chk(self.lib.pgas_m_rng_normal(self.eng._h, int(seed), int(stream), int(t), 0, self.N, int(ncol), out.data_ptr(), self.eng._stream()),
                      "pgas_m_rng_normal")
        return out

    def student_t(self, seed, stream, t, nu):
        nu = nu.to(device=self.device, dtype=torch.float64).contiguous()
        out = self._vec()
        self.eng._chk(self.lib.pgas_m_rng_student_t(self.eng._h, int(seed), int(stream), int(t), 0, self.N, nu.data_ptr(), out.data_ptr(),
                                                    self.eng._stream()), "pgas_m_rng_student_t")
        return out

    def student_t_df(self, seed, stream, t, anc, src, nu0, nu_scale):
        """Student-t variates with nu[p] = nu0 + nu_scale * src[anc[p]] formed inside the kernel."""
        out = self._vec()
        a = anc.to(device=self.device, dtype=torch.int32).contiguous()
        self.eng._chk(self.lib.pgas_m_rng_student_t_df(self.eng._h, int(seed), int(stream), int(t), 0, self.N, a.data_ptr(), src.contiguous().data_ptr(),
                                                       float(nu0), float(nu_scale), out.data_ptr(), self.eng._stream()), "pgas_m_rng_student_t_df")
        return out

    def mniw_draw(self, scale, anc, m, c, q, T2, T3, P2, P3, t):
        """xi = m + sqrt((P2 + scale T2[a] - q[a]) / (P3 + scale T3[a])) t sqrt(c + 1) in one launch (pgas_m_mniw_draw)."""
        n = m.shape[0]
        out = self._vec(n)
        a = anc.to(device=self.device, dtype=torch.int32).contiguous()
        self.eng._chk(self.lib.pgas_m_mniw_draw(self.eng._h, n, float(scale), a.data_ptr(), m.contiguous().data_ptr(), c.contiguous().data_ptr(),
                                                q.contiguous().data_ptr(), T2.contiguous().data_ptr(), T3.contiguous().data_ptr(), float(P2), float(P3),
                                                t.contiguous().data_ptr(), out.data_ptr(), self.eng._stream()), "pgas_m_mniw_draw")
        return out

    def lbm_diff(self, M, T2, T3, sol1, sol2, P2, P3, r2, r3):
        """lbm(prior + T) - lbm(prior + T + R) per particle from the two solves' q / logdet (pgas_m_lbm_diff; n = 1)."""
        n = T2.shape[0]
        out = self._vec(n)
        r2, r3 = r2.reshape(-1).contiguous(), r3.reshape(-1).contiguous()
        self.eng._chk(self.lib.pgas_m_lbm_diff(self.eng._h, n, int(M), T2.contiguous().data_ptr(), T3.contiguous().data_ptr(), sol1["q"].data_ptr(),
                                               sol1["logdet"].data_ptr(), sol2["q"].data_ptr(), sol2["logdet"].data_ptr(), float(P2), float(P3),
                                               r2.data_ptr(), r3.data_ptr(), out.data_ptr(), self.eng._stream()), "pgas_m_lbm_diff")
        return out

    def hilbert_basis(self, bmap, state, input=None):
        """descriptors.BasisMap.batch for (n, n_x) states and one (n_u,) input in one launch (pgas_m_hilbert_basis) -> (n, M)."""
        b = bmap.basis
        n = state.shape[0]
        state = state.reshape(n, -1).contiguous()
        nx = state.shape[1]
        inp = None if input is None or input.numel() == 0 else input.reshape(-1).contiguous()
        nu = 0 if inp is None else inp.numel()
        cache = bmap.__dict__.setdefault("_idx_dev", {})
        if self.device not in cache:
            cache[self.device] = torch.as_tensor(np.ascontiguousarray(b.indices, dtype=np.int32), device=self.device)
        host = [np.ascontiguousarray(a, dtype=np.float64) for a in (bmap.div, b.center, b.L, b.size)]   # kept alive over the call
        sel = np.ascontiguousarray(bmap.sel, dtype=np.int32)
        out = torch.empty((n, b.M), dtype=torch.float64, device=self.device)
        self.eng._chk(self.lib.pgas_m_hilbert_basis(self.eng._h, n, b.M, b.D, state.data_ptr(), nx, self._ptr(inp), nu, sel.ctypes.data_as(C.POINTER(C.c_int32)),
                                                    *[a.ctypes.data_as(_dp) for a in host], cache[self.device].data_ptr(), out.data_ptr(),
                                                    self.eng._stream()), "pgas_m_hilbert_basis")
        return out

    def mniw_solve(self, P0, P1, T0, T1, scale=1.0, anc=None, R0=None, R1=None, phi=None, want=("m", "c", "q", "logdet"), keep_factor=False, runs=None):
        """eta0 = P0 + scale T0[anc] (+R0), eta1 = P1 + scale T1[anc] (+R1) per particle -> dict of (n,) tensors (see pgas_m_mniw_solve).
        keep_factor=True adds "L" (n, (M+2)(M+3)/2), the packed factor with the right-hand-side rows, for mniw_trisolve.
        T0 (n, M, nvar) with P0 (M, nvar): an interface variable of nvar components (pgas_m_mniw_solve_n) -- "m" is then (n, nvar), "q"
        (n, nvar, nvar) and "L" (n, (M+1+nvar)(M+2+nvar)/2).
        runs=R: the n particles are R runs of n / R and R0 (R, M[, nvar]), R1 (R, M, M) hold one reference per run (pgas_m_runs_mniw_solve_n)."""
        n, M = T0.shape[0], T0.shape[1]
        nv = T0.shape[2] if T0.dim() == 3 else 0   # 0: the scalar layout (T0 (n, M))
        if runs is not None:
            runs = int(runs)
            if runs < 1 or n % runs or R0 is None or R1 is None or R0.shape != ((runs, M, nv) if nv else (runs, M)) or R1.shape != (runs, M, M):
                raise ValueError("mniw_solve: runs=R needs n divisible by R, R0 (R, M[, nvar]) and R1 (R, M, M)")
        if nv:
            if P0.shape != (M, nv) or (runs is None and R0 is not None and R0.shape != (M, nv)):
                raise ValueError("mniw_solve: P0 / R0 must be (M, nvar) when T0 is (n, M, nvar)")
            shp = {"m": (n, nv), "q": (n, nv, nv)}
            out = {k: torch.empty(shp.get(k, (n,)), dtype=torch.float64, device=self.device) for k in want}
        else:
            out = {k: self._vec(n) for k in want}
        if keep_factor:
            R = M + 1 + max(nv, 1)
            out["L"] = torch.empty((n, R * (R + 1) // 2), dtype=torch.float64, device=self.device)
            if nv:
                out["nvar"] = nv
        a = None if anc is None else anc.to(device=self.device, dtype=torch.int32).contiguous()
        for arr in (P0, P1, T0, T1, R0, R1, phi):
            if arr is not None and not (arr.is_contiguous() and arr.dtype == torch.float64 and arr.device == self.device):
                raise ValueError("mniw_solve: operands must be contiguous fp64 tensors on the engine's device")
        if a is not None and a.numel() != n:
            raise ValueError("mniw_solve: one ancestor index per particle expected")
        if runs is not None:
            self.eng._chk(self.lib.pgas_m_runs_mniw_solve_n(self.eng._h, runs, n // runs, M, max(nv, 1), float(scale), self._ptr(a), P0.data_ptr(), P1.data_ptr(),
                                                            T0.data_ptr(), T1.data_ptr(), R0.data_ptr(), R1.data_ptr(), self._ptr(phi), self._ptr(out.get("m")),
                                                            self._ptr(out.get("c")), self._ptr(out.get("q")), self._ptr(out.get("logdet")),
                                                            self._ptr(out.get("L")), self.eng._stream()), "pgas_m_runs_mniw_solve_n")
            return out
        self.eng._chk(self.lib.pgas_m_mniw_solve_n(self.eng._h, n, M, max(nv, 1), float(scale), self._ptr(a), P0.data_ptr(), P1.data_ptr(), T0.data_ptr(),
                                                   T1.data_ptr(), self._ptr(R0), self._ptr(R1), self._ptr(phi), self._ptr(out.get("m")), self._ptr(out.get("c")),
                                                   self._ptr(out.get("q")), self._ptr(out.get("logdet")), self._ptr(out.get("L")), self.eng._stream()),
                      "pgas_m_mniw_solve")
        return out

    def mniw_trisolve(self, fac, anc, phi):
        """m = w[anc] . v, c = v . v with v = L[anc]^-1 phi for a factor kept by mniw_solve(keep_factor=True)."""
        n, M = phi.shape
        nv = int(fac.get("nvar", 0))
        R = M + 1 + max(nv, 1)
        a = None if anc is None else anc.to(device=self.device, dtype=torch.int32).contiguous()
        if fac["L"].shape != (n, R * (R + 1) // 2) or (a is not None and a.numel() != n):
            raise ValueError("mniw_trisolve: operand shapes do not match")
        m, c = (torch.empty((n, nv), dtype=torch.float64, device=self.device) if nv else self._vec(n)), self._vec(n)
        self.eng._chk(self.lib.pgas_m_mniw_trisolve_n(self.eng._h, n, M, max(nv, 1), self._ptr(a), fac["L"].data_ptr(), phi.contiguous().data_ptr(),
                                                      m.data_ptr(), c.data_ptr(), self.eng._stream()), "pgas_m_mniw_trisolve")
        return {"m": m, "c": c}

    def expr_eval(self, prog, state, inp, ivs, mode=0, anc=None, aux=None, mat=None, cR=0.0):
        """Run a traced model program (pgas_amd.exprs.Program) for every particle in one launch (pgas_m_expr_eval): mode 0 -> (n, n_out)
        values, 1 -> values + aux @ mat.T (draw_state), 2 -> cR - |mat (aux - values)|^2 / 2 per particle (log_likelihood)."""
        dev = self.device
        cache = prog.__dict__.setdefault("_dev", {})
        if dev not in cache:
            cache[dev] = (torch.as_tensor(prog.code.reshape(-1), dtype=torch.int32, device=dev), torch.as_tensor(prog.consts, dtype=torch.float64, device=dev))
        code_t, const_t = cache[dev]
        nx, nu, ivw = prog.widths
        n = state.shape[0]
        state = state.reshape(n, nx).contiguous()
        inp = inp.reshape(-1).contiguous() if nu else None
        ivs = [v.reshape(n, w).contiguous() for v, w in zip(ivs, ivw)]
        if state.dtype != torch.float64 or state.device != dev or len(ivs) != len(ivw) or (nu and inp.numel() != nu):
            raise ValueError("expr_eval: operands do not match the traced program")
        nout = len(prog.out_regs)
        out = torch.empty((n,) if mode == 2 else (n, nout), dtype=torch.float64, device=dev)
        a = None if anc is None else anc.to(device=dev, dtype=torch.int32).contiguous()
        regs = (C.c_int32 * nout)(*prog.out_regs)
        ptrs = (C.c_void_p * max(len(ivs), 1))(*[v.data_ptr() for v in ivs])
        wid = (C.c_int32 * max(len(ivs), 1))(*ivw)
        aux_c = None if aux is None else aux.reshape(-1).contiguous()
        mat_c = None if mat is None else mat.contiguous()
        self.eng._chk(self.lib.pgas_m_expr_eval(self.eng._h, n, code_t.data_ptr(), prog.code.shape[0], self._ptr(const_t) if prog.consts.size else None,
                                                int(prog.consts.size), prog.n_in, prog.n_reg, regs, nout, state.data_ptr(), nx, self._ptr(a),
                                                self._ptr(inp), nu, ptrs, wid, len(ivs), int(mode), self._ptr(aux_c), self._ptr(mat_c), float(cR),
                                                out.data_ptr(), self.eng._stream()), "pgas_m_expr_eval")
        return out

    def model_rollout(self, desc):
        """pgas_m_rollout on a filled RolloutDesc (pgas_amd/model_rollout.py builds it and keeps its arrays alive).  Enqueues work only."""
        self.eng._chk(self.lib.pgas_m_rollout(self.eng._h, C.byref(desc), self.eng._stream()), "pgas_m_rollout")

    def model_rollout_stats(self, desc, stats):
        """pgas_m_rollout_stats on a filled RolloutDesc and RolloutStatsDesc (ModelRollout.predict builds both and keeps their arrays
        alive, the partial-sum buffer included).  Enqueues work only."""
        self.eng._chk(self.lib.pgas_m_rollout_stats(self.eng._h, C.byref(desc), C.byref(stats), self.eng._stream()), "pgas_m_rollout_stats")

    def model_filter(self, desc, fl):
        """pgas_m_filter on a filled RolloutDesc and ModelFilterDesc (ModelRollout.filter builds both and keeps their arrays alive).
        Enqueues work only."""
        self.eng._chk(self.lib.pgas_m_filter(self.eng._h, C.byref(desc), C.byref(fl), self.eng._stream()), "pgas_m_filter")

    def model_forecast(self, desc, fc):
        """pgas_m_forecast on a filled RolloutDesc and ModelForecastDesc (ModelRollout.forecast builds both and keeps their arrays
        alive): the h-step-ahead predictions from the trace of a model_filter call with the same descriptor.  Enqueues work only."""
        self.eng._chk(self.lib.pgas_m_forecast(self.eng._h, C.byref(desc), C.byref(fc), self.eng._stream()), "pgas_m_forecast")

    def model_rollout_cdf(self, desc, cd):
        """pgas_m_rollout_cdf on a filled RolloutDesc and ModelRolloutCdfDesc (ModelRollout.cdf builds both and keeps their arrays alive).
        Enqueues work only."""
        self.eng._chk(self.lib.pgas_m_rollout_cdf(self.eng._h, C.byref(desc), C.byref(cd), self.eng._stream()), "pgas_m_rollout_cdf")

    def model_forecast_cdf(self, desc, fc):
        """pgas_m_forecast_cdf on a filled RolloutDesc and ModelForecastCdfDesc (ModelRollout.forecast_cdf builds both and keeps their
        arrays alive): the threshold counts of the h-step-ahead clouds from the trace of a model_filter call with the same descriptor.
        Enqueues work only."""
        self.eng._chk(self.lib.pgas_m_forecast_cdf(self.eng._h, C.byref(desc), C.byref(fc), self.eng._stream()), "pgas_m_forecast_cdf")

    def model_smooth(self, desc, sm):
        """pgas_m_smooth on a filled RolloutDesc and ModelSmoothDesc (ModelRollout.smooth builds both and keeps their arrays alive): up
        to 256 backward-simulation trajectories per draw over the traces of a model_filter call with the same descriptor.  Enqueues
        work only."""
        self.eng._chk(self.lib.pgas_m_smooth(self.eng._h, C.byref(desc), C.byref(sm), self.eng._stream()), "pgas_m_smooth")

    def check(self):
        """Synchronises; raises if a matrix handed to mniw_solve since the last check was not positive definite."""
        self.eng._chk(self.lib.pgas_m_check(self.eng._h, self.eng._stream()), "pgas_m_check")

    def stats_gather_update(self, scale, anc, T, phi, xi):
        """T = (T0 (n,M), T1 (n,M,M), T2 (n,), T3 (n,)) -> scale * T[anc] + statistics of (xi, phi); new tensors."""
        T0, T1, T2, T3 = T
        n, M = T0.shape[0], T0.shape[1]
        nv = T0.shape[2] if T0.dim() == 3 else 1   # T0 (n, M, nvar), T2 (n, nvar, nvar), xi (n, nvar): several components
        out = (torch.empty_like(T0), torch.empty_like(T1), torch.empty_like(T2), torch.empty_like(T3))
        a = None if anc is None else anc.to(device=self.device, dtype=torch.int32).contiguous()
        if a is not None and a.numel() != n:
            raise ValueError("stats_gather_update: one ancestor index per particle expected")
        if phi.shape != (n, M) or xi.numel() != n * nv or T1.shape != (n, M, M) or T2.numel() != n * nv * nv:
            raise ValueError("stats_gather_update: operand shapes do not match (n, M[, nvar])")
        for arr in (T0, T1, T2, T3):
            if not arr.is_contiguous():
                raise ValueError("stats_gather_update: the statistics must be contiguous")
        self.eng._chk(self.lib.pgas_m_stats_gather_update_n(self.eng._h, n, M, nv, float(scale), self._ptr(a), T0.data_ptr(), T1.data_ptr(), T2.data_ptr(),
                                                            T3.data_ptr(), phi.contiguous().data_ptr(), xi.contiguous().data_ptr(), out[0].data_ptr(),
                                                            out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), self.eng._stream()),
                      "pgas_m_stats_gather_update")
        return out

    def weighted_stats(self, w, T):
        """sum_p w[p] T[p] for T = (T0 (n,M), T1 (n,M,M), T2 (n,), T3 (n,)) -> (S0 (M,), S1 (M,M), S2 (), S3 ())."""
        T0, T1, T2, T3 = T
        n, M = T0.shape[0], T0.shape[1]
        nv = T0.shape[2] if T0.dim() == 3 else 0
        w = w.contiguous()
        S0 = torch.empty((M, nv) if nv else (M,), dtype=torch.float64, device=self.device)
        S1 = torch.empty((M, M), dtype=torch.float64, device=self.device)
        k = max(nv, 1)
        S23 = torch.empty(k * k + 1, dtype=torch.float64, device=self.device)
        self.eng._chk(self.lib.pgas_m_weighted_stats_n(self.eng._h, n, M, k, w.data_ptr(), T0.data_ptr(), T1.data_ptr(), T2.data_ptr(), T3.data_ptr(),
                                                       S0.data_ptr(), S1.data_ptr(), S23.data_ptr(), S23.data_ptr() + 8 * k * k, self.eng._stream()),
                      "pgas_m_weighted_stats")
        return S0, S1, (S23[: k * k].reshape(k, k) if nv else S23[0]), S23[k * k]

    def systematic_resample(self, u, logw):
        return self.eng.systematic_resample(u, logw)

    # -------------------------------------------------------------- R independent runs (pgas_m_runs_*; pgas_amd/runs.py)
    # self.N = R * n particles, run r at [r n, (r + 1) n); keys: (R,) int64 device tensor holding the u64 bit patterns of the runs' root keys.
    def _runs(self, keys):
        R = int(keys.shape[0])
        if keys.dtype != torch.int64 or keys.dim() != 1 or keys.device != self.device or not keys.is_contiguous() or R < 1 or self.N % R:
            raise ValueError(f"keys: expected a contiguous (R,) int64 tensor on {self.device} with R dividing the {self.N} particles")
        return R, self.N // R

    def runs_normal(self, keys, stream, t, ncol):
        """(R n, ncol): rows [r n, (r + 1) n) are normal(keys[r], stream, t, ncol) of an n-particle context."""
        R, n = self._runs(keys)
        out = self._vec(cols=int(ncol))
        self.eng._chk(self.lib.pgas_m_runs_rng_normal(self.eng._h, keys.data_ptr(), R, n, int(stream), int(t), int(ncol), out.data_ptr(), self.eng._stream()),
                      "pgas_m_runs_rng_normal")
        return out

    def runs_student_t(self, keys, stream, t, nu):
        R, n = self._runs(keys)
        nu = nu.to(device=self.device, dtype=torch.float64).contiguous()
        if nu.numel() != self.N:
            raise ValueError("runs_student_t: one nu per particle expected")
        out = self._vec()
        self.eng._chk(self.lib.pgas_m_runs_rng_student_t(self.eng._h, keys.data_ptr(), R, n, int(stream), int(t), nu.data_ptr(), out.data_ptr(), self.eng._stream()),
                      "pgas_m_runs_rng_student_t")
        return out

    def runs_student_t_df(self, keys, stream, t, anc, src, nu0, nu_scale):
        """Student-t variates with nu[p] = nu0 + nu_scale * src[anc[p]], anc a global index into the R n axis."""
        R, n = self._runs(keys)
        a = anc.to(device=self.device, dtype=torch.int32).contiguous()
        src = src.contiguous()
        if a.numel() != self.N or src.numel() != self.N or src.dtype != torch.float64:
            raise ValueError("runs_student_t_df: one ancestor and one fp64 source value per particle expected")
        out = self._vec()
        self.eng._chk(self.lib.pgas_m_runs_rng_student_t_df(self.eng._h, keys.data_ptr(), R, n, int(stream), int(t), a.data_ptr(), src.data_ptr(), float(nu0),
                                                            float(nu_scale), out.data_ptr(), self.eng._stream()), "pgas_m_runs_rng_student_t_df")
        return out

    def runs_uniform(self, keys, stream, t):
        """(R,): uniform_dev(keys[r], stream, t) of every run."""
        R, _ = self._runs(keys)
        out = torch.empty(R, dtype=torch.float64, device=self.device)
        self.eng._chk(self.lib.pgas_m_runs_rng_uniform(self.eng._h, keys.data_ptr(), R, int(stream), int(t), out.data_ptr(), self.eng._stream()),
                      "pgas_m_runs_rng_uniform")
        return out

    def runs_systematic(self, R, u, logw, want_global=True):
        """u (R,), logw (R, n) -> (idx_local (R, n), idx_global (R, n) or None) int32: systematic resampling of every run in one launch,
        idx_local[r] what systematic_resample(u[r], logw[r]) gives on an n-particle context, idx_global = r n + idx_local.  n <= 1024."""
        R = int(R)
        if R < 1 or logw.numel() % R or u.numel() != R:
            raise ValueError("runs_systematic: u (R,) and logw (R, n) expected")
        n = logw.numel() // R
        u = u.to(device=self.device, dtype=torch.float64).contiguous()
        lw = logw.to(device=self.device, dtype=torch.float64).contiguous()
        loc = torch.empty((R, n), dtype=torch.int32, device=self.device)
        glo = torch.empty((R, n), dtype=torch.int32, device=self.device) if want_global else None
        self.eng._chk(self.lib.pgas_m_runs_systematic(self.eng._h, R, n, u.data_ptr(), lw.data_ptr(), loc.data_ptr(), self._ptr(glo), self.eng._stream()),
                      "pgas_m_runs_systematic")
        return loc, glo

    def runs_weighted_stats(self, R, w, T):
        """weighted_stats per run: w (R n,), T over R n particles -> (S0 (R, M[, nvar]), S1 (R, M, M), S2 (R[, nvar, nvar]), S3 (R,))."""
        T0, T1, T2, T3 = T
        R, tot, M = int(R), T0.shape[0], T0.shape[1]
        nv = T0.shape[2] if T0.dim() == 3 else 0
        k = max(nv, 1)
        w = w.contiguous()
        if R < 1 or tot % R or w.numel() != tot or T1.shape != (tot, M, M) or T2.numel() != tot * k * k or T3.numel() != tot:
            raise ValueError("runs_weighted_stats: operand shapes do not match (R n, M[, nvar])")
        for arr in (w, T0, T1, T2, T3):
            if not (arr.is_contiguous() and arr.dtype == torch.float64 and arr.device == self.device):
                raise ValueError("runs_weighted_stats: operands must be contiguous fp64 tensors on the engine's device")
        S0 = torch.empty((R, M, nv) if nv else (R, M), dtype=torch.float64, device=self.device)
        S1 = torch.empty((R, M, M), dtype=torch.float64, device=self.device)
        S2 = torch.empty((R, nv, nv) if nv else (R,), dtype=torch.float64, device=self.device)
        S3 = torch.empty(R, dtype=torch.float64, device=self.device)
        self.eng._chk(self.lib.pgas_m_runs_weighted_stats(self.eng._h, R, tot // R, M, k, w.data_ptr(), T0.data_ptr(), T1.data_ptr(), T2.data_ptr(), T3.data_ptr(),
                                                          S0.data_ptr(), S1.data_ptr(), S2.data_ptr(), S3.data_ptr(), self.eng._stream()),
                      "pgas_m_runs_weighted_stats")
        return S0, S1, S2, S3

    # -------------------------------------------------------------- R conditional filters (pgas_amd/marginal_chains.py)
    def runs_lbm_diff(self, R, M, T2, T3, sol1, sol2, P2, P3, r2, r3):
        """lbm_diff over R runs: r2 (R,), r3 (R,) hold the reference statistics' T2 / T3 of every run (pgas_m_runs_lbm_diff; n = 1)."""
        R, n = int(R), T2.shape[0]
        r2, r3 = r2.reshape(-1).contiguous(), r3.reshape(-1).contiguous()
        if R < 1 or n % R or r2.numel() != R or r3.numel() != R:
            raise ValueError("runs_lbm_diff: r2 (R,), r3 (R,) and R n particles expected")
        out = self._vec(n)
        self.eng._chk(self.lib.pgas_m_runs_lbm_diff(self.eng._h, R, n // R, int(M), T2.contiguous().data_ptr(), T3.contiguous().data_ptr(), sol1["q"].data_ptr(),
                                                    sol1["logdet"].data_ptr(), sol2["q"].data_ptr(), sol2["logdet"].data_ptr(), float(P2), float(P3),
                                                    r2.data_ptr(), r3.data_ptr(), out.data_ptr(), self.eng._stream()), "pgas_m_runs_lbm_diff")
        return out

    def runs_categorical(self, R, logw, u, anc_local=None, anc_global=None):
        """logw (R, n), u (R,) -> idx (R,) int32 = min(searchsorted(cumsum(softmax(logw[r])), u[r]), n - 1) in one launch (pgas_m_runs_categorical;
        n <= 1024; a row with a NaN or without a finite maximum gives n - 1).  anc_local / anc_global: contiguous (R, n) int32 tensors whose slot
        n - 1 of every row receives idx[r] and r n + idx[r], in place."""
        R = int(R)
        if R < 1 or logw.numel() % R or u.numel() != R:
            raise ValueError("runs_categorical: logw (R, n) and u (R,) expected")
        n = logw.numel() // R
        lw = logw.to(device=self.device, dtype=torch.float64).contiguous()
        u = u.to(device=self.device, dtype=torch.float64).contiguous()
        for a in (anc_local, anc_global):
            if a is not None and not (a.dtype == torch.int32 and a.is_contiguous() and a.numel() == R * n and a.device == self.device):
                raise ValueError("runs_categorical: the ancestor arrays must be contiguous (R, n) int32 tensors on the engine's device")
        idx = torch.empty(R, dtype=torch.int32, device=self.device)
        self.eng._chk(self.lib.pgas_m_runs_categorical(self.eng._h, R, n, lw.data_ptr(), u.data_ptr(), idx.data_ptr(), self._ptr(anc_local), self._ptr(anc_global),
                                                       self.eng._stream()), "pgas_m_runs_categorical")
        return idx

    def runs_backtrace(self, R, trace, anc, idx):
        """trace (T, R n, w) or (T, R n), anc (T-1, R n) int32 (every run's own indices), idx (R,) int32 on the device -> (R, T, w): row r is
        reconstruct_trajectory on run r's slices (pgas_m_runs_backtrace)."""
        R, T = int(R), trace.shape[0]
        x = trace.reshape(T, trace.shape[1], -1)
        tot, w = x.shape[1], x.shape[2]
        if R < 1 or tot % R or idx.numel() != R or idx.dtype != torch.int32 or anc.dtype != torch.int32 or anc.numel() != (T - 1) * tot:
            raise ValueError("runs_backtrace: trace (T, R n, w), anc (T-1, R n) int32 and idx (R,) int32 expected")
        x = x.to(device=self.device, dtype=torch.float64).contiguous()
        anc, idx = anc.to(self.device).contiguous(), idx.to(self.device).contiguous()
        out = torch.empty((R, T, w), dtype=torch.float64, device=self.device)
        self.eng._chk(self.lib.pgas_m_runs_backtrace(self.eng._h, R, tot // R, T, w, x.data_ptr(), anc.data_ptr() if T > 1 else 0, idx.data_ptr(), out.data_ptr(),
                                                     self.eng._stream()), "pgas_m_runs_backtrace")
        return out
