"""ctypes binding of libsmchip.so (C ABI: include/smc_hip.h).

The HIP extension is the product: if it is missing or cannot be loaded this module raises.
There is no CPU fallback anywhere in this package.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SMC_LIB") or os.path.join(_HERE, "lib", "libsmchip.so")   # SMC_LIB: profiling builds

MODEL_LG1D, MODEL_SV1D, MODEL_UCSV3D, MODEL_UCSV_RB = 1, 2, 3, 4
MODEL_LG2D, LG2_NRAW = 16, 15   # a two-state linear row of the exact-Kalman side (no particle-filter family)
FLAG_ANCESTORS, FLAG_NO_RESIDENT, FLAG_SYSTEMATIC, FLAG_NAN_MISSING, FLAG_CONDITIONAL = 1, 2, 4, 8, 16
FLAG_ANCESTOR_SAMPLING = 32   # with FLAG_CONDITIONAL: the record keeps the ancestors and ancestor_sweep draws the next reference

# every symbol include/smc_hip.h declares
EXPORTS = [
    "smc_create", "smc_destroy", "smc_set_params", "smc_set_streams", "smc_reseed", "smc_step_by_value", "smc_get_launch_geometry", "smc_init", "smc_step",
    "smc_log_likelihood", "smc_get_state", "smc_get_logZ", "smc_permute", "smc_copy_from", "smc_slot_bytes", "smc_pack_slots", "smc_unpack_slots", "smc_get_weights_raw", "smc_get_geometry",
    "smc_last_elapsed_ms", "smc_synchronize", "smc_time_step_kernel", "smc_event_overhead_ms", "smc_normalize", "smc_resample", "smc_kalman_log_likelihood", "smc_get_moments", "smc_get_quantiles", "smc_simulate", "smc_simulate_dim", "smc_model_dim",
    "smc_model_nraw", "smc_auto_seg", "smc_device_count", "smc_host_exp", "smc_host_log", "smc_host_philox4x32_10",
    "smc_host_box_muller", "smc_sys_targets", "smc_device_math", "smc_last_error", "smc_version",
    "smc_set_skip", "smc_pmmh_configure", "smc_pmmh_rejuvenate", "smc_host_pmmh_propose", "smc_host_pmmh_log_uniform",
    "smc_host_prior_logpdf", "smc_step_window", "smc_step_commit",
    "smc_comm_unique_id", "smc_comm_create", "smc_comm_destroy", "smc_comm_rank", "smc_comm_all_gather", "smc_outer_reweight",
    "smc_comm_exchange_slots", "smc_host_reweight", "smc_comm_plan_exchange",
    "smc_outer_seg", "smc_host_outer_records", "smc_host_outer_combine", "smc_host_outer_window", "smc_host_outer_walk",
    "smc_host_outer_advance", "smc_host_outer_temper", "smc_host_outer_resample", "smc_host_rw_factor",
    "smc_set_summaries", "smc_get_summaries", "smc_set_summary_mode", "smc_host_quantile7", "smc_host_sample_moments",
    "smc_set_proposal", "smc_host_optimal_proposal", "smc_host_guided_step", "smc_device_guided_step",
    "smc_host_rb_step", "smc_device_rb_step", "smc_host_guided_steps", "smc_host_rb_steps",
    "smc_ibis_create", "smc_ibis_destroy", "smc_ibis_configure", "smc_ibis_set_theta", "smc_ibis_window", "smc_ibis_commit",
    "smc_ibis_filter", "smc_ibis_permute", "smc_ibis_set_logw", "smc_ibis_rejuvenate", "smc_ibis_get",
    "smc_ibis_summary", "smc_ibis_set_summaries", "smc_ibis_get_summaries", "smc_host_ibis_summary",
    "smc_ibis_window_ess", "smc_ibis_resample", "smc_ibis_theta_moments", "smc_ibis_get_moved", "smc_host_theta_moments",
    "smc_host_rw_factor_cov",
    "smc_ibis_smooth", "smc_ibis_sample_paths", "smc_ibis_last_elapsed_ms", "smc_kalman_smooth", "smc_host_ibis_smooth", "smc_host_ibis_sample_paths",
    "smc_history_begin", "smc_history_len", "smc_history_get", "smc_history_put", "smc_history_end", "smc_smooth", "smc_host_transition_logpdf",
    "smc_host_smooth", "smc_sample_paths", "smc_host_sample_paths", "smc_rb_sample_paths", "smc_host_rb_sample_paths",
    "smc_forecast", "smc_forecast_cloud", "smc_host_forecast",
    "smc_get_flags", "smc_host_filter_steps", "smc_device_filter_steps",
    "smc_ibis_set_flags", "smc_ibis_get_flags", "smc_kalman_log_likelihood_flags", "smc_kalman_smooth_flags",
    "smc_host_ibis_smooth_flags", "smc_host_ibis_sample_paths_flags", "smc_host_kalman_steps",
    "smc_set_reference", "smc_reference_from_paths", "smc_get_reference", "smc_host_conditional_slot", "smc_host_logobs",
    "smc_smooth_pairs", "smc_host_smooth_pairs",
    "smc_live_bytes",
    "smc_kalman2_log_likelihood", "smc_kalman2_smooth", "smc_host_kalman2_steps", "smc_host_kalman2_smooth", "smc_simulate_lg2",
    "smc_ibis_create_rows",
    "smc_history_get_ancestors", "smc_history_put_ancestors", "smc_ancestor_sweep", "smc_host_ancestor_sweep",
    "smc_ibis_theta_quantiles", "smc_ibis_theta_histogram", "smc_host_theta_weights", "smc_host_theta_quantiles", "smc_host_theta_histogram",
    "smc_smooth_quantiles", "smc_host_smooth_quantiles", "smc_smooth_quantiles_info",
    "smc_get_predictive", "smc_predictive", "smc_host_predictive", "smc_host_normcdf", "smc_device_normcdf", "smc_predictive_info",
    "smc_kalman_predictive_flags", "smc_host_kalman_predictive",
]
PROP_NONE, PROP_AFFINE, PROP_OPTIMAL, PROP_NPAR = 0, 1, 2, 4
SUMM_WEIGHTED, SUMM_UNWEIGHTED = 0, 1
_SUMM_MODES = {"weighted": SUMM_WEIGHTED, "unweighted": SUMM_UNWEIGHTED}
COMM_ID_BYTES = 128
PRIOR_UNIFORM, PRIOR_NORMAL, PRIOR_TRUNCNORMAL, PRIOR_LOGNORMAL, PRIOR_NPAR, MAX_DTHETA = 1, 2, 3, 4, 5, 8

_dp = C.POINTER(C.c_double)
_u64p = C.POINTER(C.c_uint64)
_u32p = C.POINTER(C.c_uint32)
_i32p = C.POINTER(C.c_int32)
_ip = C.POINTER(C.c_int)


class SmcError(RuntimeError):
    pass


_lib = None


def _share_hip_runtime_with_torch():
    """One HIP/HSA runtime per process.  PyTorch-ROCm wheels bundle their own libamdhip64.so (same soname
    as /opt/rocm's); whichever copy is loaded first serves both users, but if OUR library pulls in the system
    copy first and torch initialises later, torch's bundled HSA runtime finds "No HIP GPUs".  So when a
    torch wheel is installed we pre-load ITS runtime (a dlopen of one file, torch itself is not imported);
    libsmchip.so's DT_NEEDED libamdhip64.so.7 then binds to it.  SMC_HIP_RUNTIME=system opts out."""
    if os.environ.get("SMC_HIP_RUNTIME", "") == "system":
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return
        cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
    except Exception:   # noqa: BLE001  (fall back to the system runtime)
        pass


def lib():
    """Load libsmchip.so (built by `__graft_entry__.build()` / csrc/Makefile). Fails loudly."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SmcError("HIP extension %s not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(hipcc --offload-arch=gfx950). There is no CPU fallback." % LIB_PATH)
    _share_hip_runtime_with_torch()
    L = C.CDLL(LIB_PATH)
    h = C.c_void_p
    L.smc_create.argtypes = [C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_uint64, C.c_int, C.c_uint32, C.POINTER(h)]
    L.smc_destroy.argtypes = [h]
    L.smc_set_params.argtypes = [h, _dp]
    L.smc_set_streams.argtypes = [h, _u32p]
    L.smc_reseed.argtypes = [h, C.c_uint64]
    L.smc_step_by_value.argtypes = [h, C.POINTER(C.c_int)]
    L.smc_get_launch_geometry.argtypes = [h, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.smc_init.argtypes = [h, C.c_double, _dp]
    L.smc_step.argtypes = [h, C.c_double, _dp, _dp]
    L.smc_log_likelihood.argtypes = [h, _dp, C.c_int64, _dp, _dp, _dp]
    L.smc_get_state.argtypes = [h, _dp, _dp, _i32p]
    L.smc_get_logZ.argtypes = [h, _dp, _dp]
    L.smc_permute.argtypes = [h, _i32p]
    L.smc_copy_from.argtypes = [h, h, C.POINTER(C.c_uint8)]
    L.smc_slot_bytes.argtypes = [h, C.POINTER(C.c_int64)]
    L.smc_pack_slots.argtypes = [h, _i32p, C.c_int64, C.c_void_p]
    L.smc_unpack_slots.argtypes = [h, _i32p, C.c_int64, C.c_void_p]
    L.smc_get_weights_raw.argtypes = [h, _u64p, _dp, _u64p, _u64p, _u64p]
    L.smc_get_geometry.argtypes = [h, _ip, _ip, _ip, _ip]
    L.smc_last_elapsed_ms.argtypes = [h, _dp]
    L.smc_synchronize.argtypes = [h]
    L.smc_time_step_kernel.argtypes = [h, _dp, C.c_int64, C.c_int, _dp, _dp]
    L.smc_event_overhead_ms.argtypes = [h, C.c_int, _dp]
    L.smc_normalize.argtypes = [_dp, C.c_int64, _dp, _dp, _dp, C.c_int]
    L.smc_resample.argtypes = [_dp, C.c_int64, C.c_int64, C.c_uint64, C.c_uint32, C.c_uint32, _i32p, C.c_int]
    L.smc_kalman_log_likelihood.argtypes = [_dp, C.c_int64, _dp, C.c_int64, C.c_int, _dp, C.c_int]
    L.smc_get_moments.argtypes = [h, _dp, _dp]
    L.smc_get_quantiles.argtypes = [h, C.c_int, _dp, C.c_int, _dp]
    L.smc_set_summaries.argtypes = [h, C.c_int, _dp, C.c_int, C.c_int]
    L.smc_set_summary_mode.argtypes = [h, C.c_int]
    L.smc_host_quantile7.argtypes = [_dp, C.c_int64, _dp, C.c_int, _dp]
    L.smc_host_sample_moments.argtypes = [_dp, C.c_int64, _dp, _dp]
    L.smc_set_proposal.argtypes = [h, C.c_int, _dp]
    L.smc_host_optimal_proposal.argtypes = [C.c_int, _dp, _dp]
    L.smc_host_guided_step.argtypes = [C.c_int, _dp, C.c_int, _dp, _dp, _dp, C.c_double, _dp, _dp]
    L.smc_device_guided_step.argtypes = [C.c_int, _dp, C.c_int, _dp, _dp, _dp, C.c_double, C.c_int64, _dp, _dp, C.c_int]
    L.smc_host_rb_step.argtypes = [_dp, _dp, _dp, C.c_double, C.c_int, _dp, _dp]
    L.smc_device_rb_step.argtypes = [_dp, _dp, _dp, C.c_double, C.c_int, C.c_int64, _dp, _dp, C.c_int]
    L.smc_host_guided_steps.argtypes = [C.c_int, _dp, C.c_int, _dp, _dp, _dp, C.c_double, C.c_int64, _dp, _dp]
    L.smc_get_flags.argtypes = [h, _u32p]
    L.smc_live_bytes.argtypes = [C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.smc_set_reference.argtypes = [h, _dp, C.c_int64]
    L.smc_reference_from_paths.argtypes = [h, C.c_int64, C.POINTER(C.c_int64)]
    L.smc_get_reference.argtypes = [h, _dp, C.POINTER(C.c_int64)]
    L.smc_host_conditional_slot.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_int64, C.POINTER(C.c_int64)]
    L.smc_history_get_ancestors.argtypes = [h, C.c_int64, _i32p]
    L.smc_history_put_ancestors.argtypes = [h, C.c_int64, _i32p]
    L.smc_ancestor_sweep.argtypes = [h, C.c_uint64, _i32p, _i32p, C.POINTER(C.c_int64)]
    L.smc_host_ancestor_sweep.argtypes = [C.c_int, _dp, C.c_int64, C.c_int64, _dp, _dp, _i32p, _dp, C.c_uint64, C.c_uint64, C.c_uint32, _i32p, _i32p, _dp]
    L.smc_host_logobs.argtypes = [C.c_int, _dp, _dp, C.c_double, _dp]
    L.smc_host_filter_steps.argtypes = [C.c_int, _dp, C.c_int, _dp, _dp, _dp, C.c_double, C.c_int, C.c_int, C.c_int64, _dp, _dp]
    L.smc_device_filter_steps.argtypes = [C.c_int, _dp, C.c_int, _dp, _dp, _dp, C.c_double, C.c_int, C.c_int, C.c_int64, _dp, _dp, C.c_int]
    L.smc_host_rb_steps.argtypes = [_dp, _dp, _dp, C.c_double, C.c_int, C.c_int64, _dp, _dp]
    L.smc_get_summaries.argtypes = [h, C.c_int64, _dp, _dp, _dp]
    L.smc_sys_targets.argtypes = [C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int, C.POINTER(C.c_uint64), C.c_int]
    L.smc_simulate.argtypes = [C.c_int, _dp, C.c_int64, C.c_uint64, _dp, _dp]
    L.smc_model_dim.argtypes = [C.c_int]
    L.smc_simulate_dim.argtypes = [C.c_int]
    L.smc_model_nraw.argtypes = [C.c_int]
    L.smc_auto_seg.argtypes = [C.c_int, C.c_int64]
    L.smc_host_exp.restype = C.c_double
    L.smc_host_exp.argtypes = [C.c_double]
    L.smc_host_log.restype = C.c_double
    L.smc_host_log.argtypes = [C.c_double]
    L.smc_host_philox4x32_10.restype = None
    L.smc_host_philox4x32_10.argtypes = [_u32p, _u32p, _u32p]
    L.smc_host_box_muller.restype = None
    L.smc_host_box_muller.argtypes = [_u32p, _dp, _dp]
    L.smc_device_math.argtypes = [C.c_int, _dp, _dp, C.c_int64, _dp, C.c_int]
    L.smc_step_window.argtypes = [h, _dp, C.c_int, _dp, _dp]
    L.smc_step_commit.argtypes = [h, C.c_int]
    L.smc_set_skip.argtypes = [h, C.POINTER(C.c_uint8)]
    L.smc_pmmh_configure.argtypes = [h, C.c_int, _i32p, _dp, _i32p, _dp]
    L.smc_pmmh_rejuvenate.argtypes = [h, h, _dp, C.c_int64, C.c_double, _dp, _dp, C.c_int, _u64p, C.c_uint64, _dp, _dp,
                                      C.POINTER(C.c_uint8), C.POINTER(C.c_int64)]
    L.smc_host_pmmh_propose.argtypes = [C.c_int, C.c_uint64, C.c_uint32, C.c_uint32, _dp, _dp, C.c_double, _dp]
    L.smc_host_pmmh_log_uniform.restype = C.c_double
    L.smc_host_pmmh_log_uniform.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32]
    L.smc_host_prior_logpdf.restype = C.c_double
    L.smc_host_prior_logpdf.argtypes = [C.c_int, _dp, C.c_double]
    L.smc_host_reweight.argtypes = [_dp, C.c_int64, _dp, _dp, _dp]
    L.smc_host_outer_records.argtypes = [_dp, C.c_int64, _u64p]
    L.smc_host_outer_combine.argtypes = [_u64p, C.c_int64, C.c_int64, _dp, _dp]
    L.smc_host_outer_window.argtypes = [_dp, _dp, C.c_int, C.c_int64, _u64p]
    L.smc_host_outer_walk.argtypes = [_u64p, C.c_int, C.c_int64, C.c_int64, C.c_double, _dp, _ip]
    L.smc_host_outer_advance.argtypes = [_dp, _dp, _dp, C.c_int, C.c_int64]
    L.smc_host_outer_temper.argtypes = [_dp, C.c_int64, C.c_double, C.c_double, _dp, _dp, _ip, _dp]
    L.smc_host_outer_resample.argtypes = [_dp, C.c_int64, C.c_int64, C.c_uint64, _i32p]
    L.smc_host_rw_factor.argtypes = [_dp, C.c_int64, C.c_int, _dp, _ip]
    L.smc_comm_unique_id.argtypes = [C.c_void_p]
    L.smc_comm_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(h)]
    L.smc_comm_destroy.argtypes = [h]
    L.smc_comm_rank.argtypes = [h, _ip, _ip]
    L.smc_comm_all_gather.argtypes = [h, _dp, C.c_int64, _dp]
    L.smc_outer_reweight.argtypes = [h, _dp, C.c_int64, _dp, _dp, _dp, _dp]
    L.smc_comm_exchange_slots.argtypes = [h, h, _i32p, C.c_int64]
    L.smc_comm_plan_exchange.argtypes = [_i32p, C.c_int64, C.c_int, C.c_int, _i32p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), _i32p,
                                         C.POINTER(C.c_int64)]
    L.smc_ibis_create.argtypes = [C.c_int64, C.c_uint64, C.c_int, C.c_int, C.POINTER(h)]
    L.smc_ibis_destroy.argtypes = [h]
    L.smc_ibis_configure.argtypes = [h, C.c_int, _i32p, _dp, _i32p, _dp]
    L.smc_ibis_set_theta.argtypes = [h, _dp]
    L.smc_ibis_window.argtypes = [h, _dp, C.c_int, _dp, _u64p]
    L.smc_ibis_commit.argtypes = [h, C.c_int]
    L.smc_ibis_filter.argtypes = [h, _dp, C.c_int64]
    L.smc_ibis_permute.argtypes = [h, _i32p]
    L.smc_ibis_set_logw.argtypes = [h, _dp]
    L.smc_ibis_rejuvenate.argtypes = [h, _dp, C.c_int64, C.c_double, _dp, _dp, C.c_int, C.c_uint64, C.POINTER(C.c_int64),
                                      C.POINTER(C.c_uint8)]
    L.smc_ibis_get.argtypes = [h, _dp, _dp, _dp, _dp, _dp]
    L.smc_ibis_summary.argtypes = [h, C.c_int, _dp]
    L.smc_ibis_set_summaries.argtypes = [h, C.c_int, C.c_int]
    L.smc_ibis_get_summaries.argtypes = [h, C.c_int, _dp]
    L.smc_host_ibis_summary.argtypes = [_dp, _dp, _dp, _dp, C.c_int64, C.c_int, _dp]
    L.smc_ibis_window_ess.argtypes = [h, _dp, C.c_int, C.c_double, _dp, _ip]
    L.smc_ibis_resample.argtypes = [h, C.c_uint64, _i32p]
    L.smc_ibis_theta_moments.argtypes = [h, C.c_int, _dp, _dp]
    L.smc_ibis_get_moved.argtypes = [h, C.POINTER(C.c_uint8)]
    L.smc_ibis_smooth.argtypes = [h, _dp, C.c_int64, _dp, _dp, _dp]
    L.smc_ibis_sample_paths.argtypes = [h, _dp, C.c_int64, C.c_int64, C.c_uint64, _i32p, _dp]
    L.smc_ibis_last_elapsed_ms.argtypes = [h, _dp]
    L.smc_kalman_smooth.argtypes = [_dp, C.c_int64, _dp, C.c_int64, C.c_int, _dp, _dp, C.c_int]
    L.smc_host_ibis_smooth.argtypes = [_dp, _dp, C.c_int64, _dp, C.c_int64, C.c_int, _dp, _dp, _dp, _dp, _dp]
    L.smc_host_ibis_sample_paths.argtypes = [_dp, C.c_int64, _dp, C.c_int64, C.c_int, C.c_int64, C.c_uint64, _i32p, _dp, _dp]
    L.smc_ibis_set_flags.argtypes = [h, C.c_uint32]
    L.smc_ibis_get_flags.argtypes = [h, _u32p]
    L.smc_kalman_log_likelihood_flags.argtypes = L.smc_kalman_log_likelihood.argtypes + [C.c_uint32]
    L.smc_kalman_smooth_flags.argtypes = L.smc_kalman_smooth.argtypes + [C.c_uint32]
    L.smc_host_ibis_smooth_flags.argtypes = L.smc_host_ibis_smooth.argtypes + [C.c_uint32]
    L.smc_host_ibis_sample_paths_flags.argtypes = L.smc_host_ibis_sample_paths.argtypes + [C.c_uint32]
    L.smc_host_kalman_steps.argtypes = [_dp, _dp, C.c_int64, C.c_int, C.c_uint32, _dp, _dp, _dp]
    L.smc_host_theta_moments.argtypes = [_dp, _dp, C.c_int64, C.c_int, C.c_int, _dp, _dp]
    L.smc_host_rw_factor_cov.argtypes = [_dp, C.c_int, _dp, _ip]
    L.smc_ibis_theta_quantiles.argtypes = [h, _dp, C.c_int, _dp]
    L.smc_ibis_theta_histogram.argtypes = [h, C.c_int, C.c_double, C.c_double, C.c_int, _u64p, _u64p]
    L.smc_host_theta_weights.argtypes = [_dp, C.c_int64, _u64p, _i32p, _u64p]
    L.smc_host_theta_quantiles.argtypes = [_dp, _dp, C.c_int64, C.c_int, _dp, C.c_int, _dp]
    L.smc_host_theta_histogram.argtypes = [_dp, _dp, C.c_int64, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, _u64p, _u64p]
    L.smc_history_begin.argtypes = [h, C.c_int64]
    L.smc_history_len.argtypes = [h, C.POINTER(C.c_int64)]
    L.smc_history_get.argtypes = [h, C.c_int64, _dp, _dp]
    L.smc_history_put.argtypes = [h, C.c_int64, _dp, _dp]
    L.smc_history_end.argtypes = [h]
    L.smc_smooth.argtypes = [h, _dp, _dp, _dp]
    L.smc_host_transition_logpdf.argtypes = [C.c_int, _dp, _dp, _dp, _dp]
    L.smc_host_smooth.argtypes = [C.c_int, _dp, C.c_int64, C.c_int64, _dp, _dp, _dp, _dp, _dp]
    L.smc_smooth_pairs.argtypes = [h, _dp, _dp, _dp, _dp, _dp]
    L.smc_host_smooth_pairs.argtypes = L.smc_host_smooth.argtypes + [_dp, _dp]
    L.smc_smooth_quantiles.argtypes = L.smc_smooth_pairs.argtypes + [C.c_int, _dp, C.c_int, _dp]
    L.smc_host_smooth_quantiles.argtypes = [C.c_int64, C.c_int64, _dp, _dp, _dp, C.c_int, _dp]
    L.smc_smooth_quantiles_info.argtypes = [h, C.POINTER(C.c_int64), _i32p, C.POINTER(C.c_int64)]
    L.smc_get_predictive.argtypes = [h, C.c_double, _dp, _dp, _dp]
    L.smc_predictive.argtypes = [h, _dp, C.c_int64, _dp, _dp, _dp]
    L.smc_host_predictive.argtypes = [C.c_int, _dp, _dp, C.c_int64, C.c_double, _dp]
    L.smc_host_normcdf.restype = C.c_double
    L.smc_host_normcdf.argtypes = [C.c_double]
    L.smc_device_normcdf.argtypes = [_dp, C.c_int64, _dp, C.c_int]
    L.smc_predictive_info.argtypes = [C.POINTER(C.c_int64), _ip]
    L.smc_kalman_predictive_flags.argtypes = [_dp, C.c_int64, _dp, C.c_int64, C.c_int, _dp, _dp, _dp, C.c_int, C.c_uint32]
    L.smc_host_kalman_predictive.argtypes = [_dp, _dp, C.c_int64, C.c_int, C.c_uint32, _dp, _dp, _dp]
    L.smc_sample_paths.argtypes = [h, C.c_int64, C.c_uint64, _i32p, _i32p, _dp]
    L.smc_host_sample_paths.argtypes = [C.c_int, _dp, C.c_int64, C.c_int64, _dp, _dp, C.c_int64, C.c_uint64, C.c_uint32, _i32p, _dp]
    L.smc_rb_sample_paths.argtypes = [h, _dp, C.c_int64, C.c_int64, C.c_uint64, _i32p, _i32p, _dp, _dp, _dp, _dp, _dp]
    L.smc_host_rb_sample_paths.argtypes = [_dp, C.c_int64, C.c_int64, _dp, _dp, _dp, C.c_int64, C.c_uint64, C.c_uint32, _i32p, _dp, _dp, _dp, _dp, _dp]
    L.smc_forecast.argtypes = [h, C.c_int64, C.c_uint64, C.c_int, _dp, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp]
    L.smc_forecast_cloud.argtypes = [h, C.c_int64, C.c_uint64, _dp, _dp]
    L.smc_host_forecast.argtypes = [C.c_int, _dp, _dp, C.c_int64, C.c_int64, C.c_uint64, C.c_uint32, _dp, _dp, _dp, _dp]
    L.smc_kalman2_log_likelihood.argtypes = [_dp, C.c_int64, _dp, C.c_int64, C.c_int, _dp, C.c_int]
    L.smc_kalman2_smooth.argtypes = [_dp, C.c_int64, _dp, C.c_int64, C.c_int, _dp, _dp, C.c_int]
    L.smc_host_kalman2_steps.argtypes = [_dp, _dp, C.c_int64, C.c_int, _dp, _dp, _dp]
    L.smc_host_kalman2_smooth.argtypes = [_dp, _dp, C.c_int64, C.c_int, _dp, _dp]
    L.smc_simulate_lg2.argtypes = [_dp, C.c_int64, C.c_uint64, _dp, _dp]
    L.smc_ibis_create_rows.argtypes = [C.c_int64, C.c_uint64, C.c_int, C.c_int, C.c_int, C.POINTER(h)]
    L.smc_last_error.restype = C.c_char_p
    L.smc_version.restype = C.c_char_p
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise SmcError("libsmchip error %d: %s" % (rc, lib().smc_last_error().decode()))


def _d(a):
    return a.ctypes.data_as(_dp) if a is not None else None


def device_count():
    return lib().smc_device_count()


def sys_targets(Dtot, n, u, j0, nk, device=-1):
    """T_{j0+k}, k < nk, of systematic resampling (smc_sys_targets); device < 0: host evaluation."""
    out = np.zeros(nk, dtype=np.uint64)
    check(lib().smc_sys_targets(int(Dtot), int(n), int(u), int(j0), int(nk), out.ctypes.data_as(C.POINTER(C.c_uint64)), device))
    return out


def simulate(model_id, raw, T, seed):
    """simulate(rng, model, T) -> (x [d][T], y [T])   src/state_space_models.jl:11-26 (host code)."""
    raw = np.ascontiguousarray(raw, dtype=np.float64)
    d = lib().smc_simulate_dim(model_id)   # rows of the simulated state: smc_model_dim, except UCSV's 3 for the marginal family
    x = np.zeros((d, T))
    y = np.zeros(T)
    check(lib().smc_simulate(model_id, _d(raw), T, seed, _d(x), _d(y)))
    return x, y


def normalize(logw, device=0):
    logw = np.ascontiguousarray(logw, dtype=np.float64)
    w = np.zeros_like(logw)
    lm, ess = C.c_double(), C.c_double()
    check(lib().smc_normalize(_d(logw), logw.size, _d(w), C.byref(lm), C.byref(ess), device))
    return lm.value, w, ess.value


def resample(w, ndraw=None, seed=0, stream=0, t=0, device=0):
    w = np.ascontiguousarray(w, dtype=np.float64)
    ndraw = w.size if ndraw is None else int(ndraw)
    a = np.zeros(ndraw, dtype=np.int32)
    check(lib().smc_resample(_d(w), w.size, ndraw, seed, stream, t, a.ctypes.data_as(_i32p), device))
    return a


def _kalman_flags(missing):
    """the `flags` word of the exact-Kalman calls: missing=True reads a NaN observation as a missing one"""
    return FLAG_NAN_MISSING if missing else 0


def kalman_log_likelihood(raw, y, predict_first=False, device=0, missing=False):
    """Batched exact scalar Kalman filter (src/kalman_filter.jl:29-70): rows of (x_T, Sigma_T, logZ)."""
    raw = np.ascontiguousarray(raw, dtype=np.float64).reshape(-1, 6)
    y = np.ascontiguousarray(y, dtype=np.float64)
    out = np.zeros((raw.shape[0], 3))
    check(lib().smc_kalman_log_likelihood_flags(_d(raw), raw.shape[0], _d(y), y.size, int(predict_first), _d(out), device,
                                                _kalman_flags(missing)))
    return out


def host_kalman_steps(row, y, predict_first=False, missing=False):
    """(xf, Sf, lik), each [T]: the filtered record and the value of every Kalman step of ONE LG1D row over y on the host
    (smc_host_kalman_steps; no GPU) - the loop every exact-Kalman kernel runs per lane"""
    row = np.ascontiguousarray(row, dtype=np.float64).reshape(6)
    y = np.ascontiguousarray(y, dtype=np.float64).ravel()
    xf, Sf, lik = np.zeros(y.size), np.zeros(y.size), np.zeros(y.size)
    check(lib().smc_host_kalman_steps(_d(row), _d(y), y.size, int(bool(predict_first)), _kalman_flags(missing), _d(xf), _d(Sf), _d(lik)))
    return xf, Sf, lik


def kalman_predictive(raw, y, predict_first=False, device=0, missing=False):
    """(pit, ym, yv), each [T][n_theta]: the exact one-step predictive law of y_t under every LG1D row and its probability integral
    transform (smc_kalman_predictive_flags; at a gap of a missing=True call the pit is NaN)"""
    raw = np.ascontiguousarray(raw, dtype=np.float64).reshape(-1, 6)
    y = np.ascontiguousarray(y, dtype=np.float64).ravel()
    out = np.zeros((3, y.size, raw.shape[0]))
    check(lib().smc_kalman_predictive_flags(_d(raw), raw.shape[0], _d(y), y.size, int(bool(predict_first)), _d(out[0]), _d(out[1]), _d(out[2]),
                                            device, _kalman_flags(missing)))
    return out[0], out[1], out[2]


def host_kalman_predictive(row, y, predict_first=False, missing=False):
    """the same rows for ONE LG1D row on the host (smc_host_kalman_predictive; no GPU): (pit, ym, yv), each [T]"""
    row = np.ascontiguousarray(row, dtype=np.float64).reshape(6)
    y = np.ascontiguousarray(y, dtype=np.float64).ravel()
    out = np.zeros((3, y.size))
    check(lib().smc_host_kalman_predictive(_d(row), _d(y), y.size, int(bool(predict_first)), _kalman_flags(missing), _d(out[0]), _d(out[1]), _d(out[2])))
    return out[0], out[1], out[2]


def host_normcdf(z):
    """sp_normcdf on the host (smc_host_normcdf), elementwise"""
    z = np.ascontiguousarray(z, dtype=np.float64)
    f = lib().smc_host_normcdf
    return np.array([f(float(v)) for v in z.ravel()]).reshape(z.shape)


def device_normcdf(z, device=0):
    """sp_normcdf on the device (smc_device_normcdf), elementwise: the same bits"""
    z = np.ascontiguousarray(z, dtype=np.float64)
    out = np.zeros(z.size)
    check(lib().smc_device_normcdf(_d(z.ravel()), z.size, _d(out), device))
    return out.reshape(z.shape)


def host_predictive(model_id, raw, x, y):
    """(pit, obs_mean, obs_var) of ONE cloud x [d][n] for the observation y on the host (smc_host_predictive; no GPU)"""
    raw = np.ascontiguousarray(raw, dtype=np.float64).ravel()
    x = np.ascontiguousarray(x, dtype=np.float64)
    x = x.reshape(-1, x.shape[-1])
    out = np.zeros(3)
    check(lib().smc_host_predictive(int(model_id), _d(raw), _d(x), x.shape[1], float(y), _d(out)))
    return out[0], out[1], out[2]


def predictive_constants():
    """(small_max, chunk) of the predictive checks (smc_predictive_info): the largest cloud one workgroup finishes, the chunk of pred_sum"""
    sm, ch = C.c_int64(), C.c_int()
    check(lib().smc_predictive_info(C.byref(sm), C.byref(ch)))
    return sm.value, ch.value


def kalman_smooth(raw, y, predict_first=False, device=0, missing=False):
    """Batched exact RTS smoother of LG1D rows (smc_kalman_smooth): (xs, Ps), each [T][n_theta]."""
    raw = np.ascontiguousarray(raw, dtype=np.float64).reshape(-1, 6)
    y = np.ascontiguousarray(y, dtype=np.float64).ravel()
    xs, Ps = np.zeros((y.size, raw.shape[0])), np.zeros((y.size, raw.shape[0]))
    check(lib().smc_kalman_smooth_flags(_d(raw), raw.shape[0], _d(y), y.size, int(bool(predict_first)), _d(xs), _d(Ps), int(device),
                                        _kalman_flags(missing)))
    return xs, Ps


def kalman2_log_likelihood(raw, y, predict_first=False, device=0):
    """Batched exact Kalman filter of two-state rows [n][15] (smc_kalman2_log_likelihood): rows of (x1, x2, S11, S21, S22, logZ)."""
    raw = np.ascontiguousarray(raw, dtype=np.float64).reshape(-1, LG2_NRAW)
    y = np.ascontiguousarray(y, dtype=np.float64).ravel()
    out = np.zeros((raw.shape[0], 6))
    check(lib().smc_kalman2_log_likelihood(_d(raw), raw.shape[0], _d(y), y.size, int(bool(predict_first)), _d(out), int(device)))
    return out


def kalman2_smooth(raw, y, predict_first=False, device=0):
    """Batched exact RTS smoother of two-state rows (smc_kalman2_smooth): (xs [T][n][2], Ps [T][n][3], the lower triangle)."""
    raw = np.ascontiguousarray(raw, dtype=np.float64).reshape(-1, LG2_NRAW)
    y = np.ascontiguousarray(y, dtype=np.float64).ravel()
    xs, Ps = np.zeros((y.size, raw.shape[0], 2)), np.zeros((y.size, raw.shape[0], 3))
    check(lib().smc_kalman2_smooth(_d(raw), raw.shape[0], _d(y), y.size, int(bool(predict_first)), _d(xs), _d(Ps), int(device)))
    return xs, Ps


def host_kalman2_steps(row, y, predict_first=False):
    """(xf [T][2], Sf [T][3], lik [T]): the filtered record and the value of every Kalman step of ONE two-state row over y on the
    host (smc_host_kalman2_steps; no GPU) - the loop every two-state kernel runs per lane"""
    row = np.ascontiguousarray(row, dtype=np.float64).reshape(LG2_NRAW)
    y = np.ascontiguousarray(y, dtype=np.float64).ravel()
    xf, Sf, lik = np.zeros((y.size, 2)), np.zeros((y.size, 3)), np.zeros(y.size)
    check(lib().smc_host_kalman2_steps(_d(row), _d(y), y.size, int(bool(predict_first)), _d(xf), _d(Sf), _d(lik)))
    return xf, Sf, lik


def host_kalman2_smooth(row, y, predict_first=False):
    """(xs [T][2], Ps [T][3]) of ONE two-state row on the host (smc_host_kalman2_smooth; no GPU)"""
    row = np.ascontiguousarray(row, dtype=np.float64).reshape(LG2_NRAW)
    y = np.ascontiguousarray(y, dtype=np.float64).ravel()
    xs, Ps = np.zeros((y.size, 2)), np.zeros((y.size, 3))
    check(lib().smc_host_kalman2_smooth(_d(row), _d(y), y.size, int(bool(predict_first)), _d(xs), _d(Ps)))
    return xs, Ps


def simulate_lg2(row, T, seed):
    """simulate(rng, model, T) for a two-state row -> (x [2][T], y [T]) (smc_simulate_lg2; host code)"""
    row = np.ascontiguousarray(row, dtype=np.float64).reshape(LG2_NRAW)
    x, y = np.zeros((2, int(T))), np.zeros(int(T))
    check(lib().smc_simulate_lg2(_d(row), int(T), int(seed) & 0xFFFFFFFFFFFFFFFF, _d(x), _d(y)))
    return x, y


def device_math(which, a, b=None, device=0):
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64) if b is not None else None
    out = np.zeros_like(a)
    check(lib().smc_device_math(which, _d(a), _d(b), a.size, _d(out), device))
    return out


def host_optimal_proposal(model_id, raw):
    """the locally optimal proposal of an LG1D parameter row as an AFFINE row (c0, c1, c2, s2) (smc_host_optimal_proposal; no GPU)"""
    raw = np.ascontiguousarray(raw, dtype=np.float64).ravel()
    par = np.zeros(PROP_NPAR)
    check(lib().smc_host_optimal_proposal(int(model_id), _d(raw), _d(par)))
    return par


def _row_or_none(par):
    return None if par is None else np.ascontiguousarray(par, dtype=np.float64).ravel()


def host_guided_step(model_id, raw, kind, par, xp, z, y):
    """one particle, one guided step by the specification on the host: (x [d], logw) (smc_host_guided_step; no GPU)"""
    raw = np.ascontiguousarray(raw, dtype=np.float64).ravel()
    par = _row_or_none(par)
    xp = np.ascontiguousarray(xp, dtype=np.float64).ravel()
    z = np.ascontiguousarray(z, dtype=np.float64).ravel()
    d = lib().smc_model_dim(int(model_id))
    assert d > 0 and xp.size == d and z.size == d
    x = np.zeros(d)
    lw = C.c_double()
    check(lib().smc_host_guided_step(int(model_id), _d(raw), int(kind), _d(par), _d(xp), _d(z), float(y), _d(x), C.byref(lw)))
    return x, lw.value


def host_guided_steps(model_id, raw, kind, par, xp, z, y):
    """host_guided_step for n particles in one call: xp, z [d][n] -> (x [d][n], logw [n]) (smc_host_guided_steps; no GPU)"""
    raw = np.ascontiguousarray(raw, dtype=np.float64).ravel()
    par = _row_or_none(par)
    d = lib().smc_model_dim(int(model_id))
    xp = np.ascontiguousarray(xp, dtype=np.float64).reshape(d, -1)
    z = np.ascontiguousarray(z, dtype=np.float64).reshape(d, -1)
    assert xp.shape == z.shape
    n = xp.shape[1]
    x = np.zeros((d, n))
    lw = np.zeros(n)
    check(lib().smc_host_guided_steps(int(model_id), _d(raw), int(kind), _d(par), _d(xp), _d(z), float(y), n, _d(x), _d(lw)))
    return x, lw


def live_bytes():
    """(device bytes, pinned host bytes) the handles, communicators and cached bundles of this process hold (smc_live_bytes)"""
    dev, pin = C.c_int64(0), C.c_int64(0)
    check(lib().smc_live_bytes(C.byref(dev), C.byref(pin)))
    return int(dev.value), int(pin.value)


def device_guided_step(model_id, raw, kind, par, xp, z, y, device=0):
    """the same for n particles on the device: xp, z [d][n] -> (x [d][n], logw [n]) (smc_device_guided_step)"""
    raw = np.ascontiguousarray(raw, dtype=np.float64).ravel()
    par = _row_or_none(par)
    d = lib().smc_model_dim(int(model_id))
    xp = np.ascontiguousarray(xp, dtype=np.float64).reshape(d, -1)
    z = np.ascontiguousarray(z, dtype=np.float64).reshape(d, -1)
    assert xp.shape == z.shape
    n = xp.shape[1]
    x = np.zeros((d, n))
    lw = np.zeros(n)
    check(lib().smc_device_guided_step(int(model_id), _d(raw), int(kind), _d(par), _d(xp), _d(z), float(y), n, _d(x), _d(lw), device))
    return x, lw


def _filter_steps(fn, model_id, raw, kind, par, xp, z, y, first, missing, *tail):
    raw = np.ascontiguousarray(raw, dtype=np.float64).ravel()
    par = _row_or_none(par)
    d = lib().smc_model_dim(int(model_id))
    if d < 1:
        raise SmcError("unknown model id %d" % int(model_id))
    nz = 2 if int(model_id) == MODEL_UCSV_RB else d
    z = np.ascontiguousarray(z, dtype=np.float64).reshape(nz, -1)
    n = z.shape[1]
    xp = np.zeros((d, n)) if xp is None else np.ascontiguousarray(xp, dtype=np.float64).reshape(d, -1)
    assert xp.shape[1] == n
    x = np.zeros((d, n))
    lw = np.zeros(n)
    check(fn(int(model_id), _d(raw), int(kind), _d(par), _d(xp), _d(z), float(y), int(bool(first)), int(bool(missing)), n, _d(x), _d(lw), *tail))
    return x, lw


def host_filter_steps(model_id, raw, kind, par, xp, z, y, first=False, missing=False):
    """the whole step of n particles by the specification on the host, every family and proposal: xp [d][n] (None at the first
    step), z [nz][n] -> (x [d][n], logw [n]); kind = PROP_NONE: the bootstrap (or marginal) step.  missing=True and a NaN y: the
    missing step, logw = +0.0 (smc_host_filter_steps; no GPU)"""
    return _filter_steps(lib().smc_host_filter_steps, model_id, raw, kind, par, xp, z, y, first, missing)


def device_filter_steps(model_id, raw, kind, par, xp, z, y, first=False, missing=False, device=0):
    """the same on the device in one launch (smc_device_filter_steps)"""
    return _filter_steps(lib().smc_device_filter_steps, model_id, raw, kind, par, xp, z, y, first, missing, device)


def host_conditional_slot(seed, stream, t, n_x):
    """the retained slot k*_t of a conditional step (smc_host_conditional_slot; no GPU): a function of (seed, stream, t, n_x)"""
    k = C.c_int64()
    check(lib().smc_host_conditional_slot(int(seed), int(stream), int(t), int(n_x), C.byref(k)))
    return k.value


def host_logobs(model_id, raw, x, y):
    """logpdf(observation(x), y) of one state x [d] by the specification on the host (smc_host_logobs; LG1D, SV1D, UCSV3D)"""
    raw = np.ascontiguousarray(raw, dtype=np.float64).ravel()
    x = np.ascontiguousarray(x, dtype=np.float64).ravel()
    if x.size != lib().smc_model_dim(int(model_id)):
        raise ValueError("x must be [d]")
    out = np.zeros(1)
    check(lib().smc_host_logobs(int(model_id), _d(raw), _d(x), float(y), _d(out)))
    return float(out[0])


def host_rb_step(raw, sp, z, y, first=False):
    """one particle, one step of the marginal UCSV family by the specification on the host: state (m, lse, lsn, P) [4] and two
    normals -> (state [4], logw) (smc_host_rb_step; no GPU).  first=True: the step at t = 1, which does not read sp"""
    raw = np.ascontiguousarray(raw, dtype=np.float64).ravel()
    sp = np.ascontiguousarray(sp, dtype=np.float64).ravel()
    z = np.ascontiguousarray(z, dtype=np.float64).ravel()
    assert raw.size == 5 and sp.size == 4 and z.size == 2
    s = np.zeros(4)
    lw = C.c_double()
    check(lib().smc_host_rb_step(_d(raw), _d(sp), _d(z), float(y), int(bool(first)), _d(s), C.byref(lw)))
    return s, lw.value


def host_rb_steps(raw, sp, z, y, first=False):
    """host_rb_step for n particles in one call: sp [4][n], z [2][n] -> (state [4][n], logw [n]) (smc_host_rb_steps; no GPU)"""
    raw = np.ascontiguousarray(raw, dtype=np.float64).ravel()
    sp = np.ascontiguousarray(sp, dtype=np.float64).reshape(4, -1)
    z = np.ascontiguousarray(z, dtype=np.float64).reshape(2, -1)
    assert raw.size == 5 and sp.shape[1] == z.shape[1]
    n = sp.shape[1]
    s = np.zeros((4, n))
    lw = np.zeros(n)
    check(lib().smc_host_rb_steps(_d(raw), _d(sp), _d(z), float(y), int(bool(first)), n, _d(s), _d(lw)))
    return s, lw


def device_rb_step(raw, sp, z, y, first=False, device=0):
    """the same for n particles on the device: sp [4][n], z [2][n] -> (state [4][n], logw [n]) (smc_device_rb_step)"""
    raw = np.ascontiguousarray(raw, dtype=np.float64).ravel()
    sp = np.ascontiguousarray(sp, dtype=np.float64).reshape(4, -1)
    z = np.ascontiguousarray(z, dtype=np.float64).reshape(2, -1)
    assert raw.size == 5 and sp.shape[1] == z.shape[1]
    n = sp.shape[1]
    s = np.zeros((4, n))
    lw = np.zeros(n)
    check(lib().smc_device_rb_step(_d(raw), _d(sp), _d(z), float(y), int(bool(first)), n, _d(s), _d(lw), device))
    return s, lw


SMOOTH_CH = 128   # SMOOTH_CH of csrc/smc_spec.h: particles per chunk of the smoother's sums (part of its numerical contract)
OUTER_SEG = 8     # SMC_OUTER_SEG: entries per segment of the outer level's integer normalisation


def host_reweight(logw, want_w=True):
    """reweight(logw) -> (logmu, w, ess): the outer level's integer normalize (smc_host_reweight; no GPU needed)"""
    logw = np.ascontiguousarray(logw, dtype=np.float64)
    w = np.empty_like(logw) if want_w else None
    lm, ess = C.c_double(), C.c_double()
    check(lib().smc_host_reweight(_d(logw), logw.size, _d(w), C.byref(lm), C.byref(ess)))
    return lm.value, w, ess.value


def host_quantile7(x, p):
    """the unweighted type-7 quantiles of x at the levels p (smc_host_quantile7: the unweighted summary mode's definition; no GPU)"""
    x = np.ascontiguousarray(x, dtype=np.float64).ravel()
    p = np.ascontiguousarray(p, dtype=np.float64).ravel()
    out = np.zeros(p.size)
    check(lib().smc_host_quantile7(_d(x), x.size, _d(p), p.size, _d(out)))
    return out


def host_sample_moments(x):
    """(mean, corrected variance) of x (smc_host_sample_moments; no GPU)"""
    x = np.ascontiguousarray(x, dtype=np.float64).ravel()
    m, v = C.c_double(), C.c_double()
    check(lib().smc_host_sample_moments(_d(x), x.size, C.byref(m), C.byref(v)))
    return m.value, v.value


def host_outer_records(logw_local):
    """segment records [nseg_local][4] (uint64 words) of the whole segments a rank holds (smc_host_outer_records)"""
    lw = np.ascontiguousarray(logw_local, dtype=np.float64)
    rec = np.zeros(((lw.size + OUTER_SEG - 1) // OUTER_SEG, 4), dtype=np.uint64)
    check(lib().smc_host_outer_records(_d(lw), lw.size, rec.ctypes.data_as(_u64p)))
    return rec


def host_outer_combine(rec, n_total):
    """(logmu, ess) from the records of ALL segments (smc_host_outer_combine)"""
    rec = np.ascontiguousarray(rec, dtype=np.uint64).reshape(-1, 4)
    lm, ess = C.c_double(), C.c_double()
    check(lib().smc_host_outer_combine(rec.ctypes.data_as(_u64p), rec.shape[0], int(n_total), C.byref(lm), C.byref(ess)))
    return lm.value, ess.value


def host_outer_window(logw_local, lik):
    """records [k][nseg_local][4] of the k steps of a window over this rank's entries (smc_host_outer_window)"""
    lw = np.ascontiguousarray(logw_local, dtype=np.float64)
    lik = np.ascontiguousarray(lik, dtype=np.float64)
    k, n = lik.shape
    assert n == lw.size
    rec = np.zeros((k, (n + OUTER_SEG - 1) // OUTER_SEG, 4), dtype=np.uint64)
    check(lib().smc_host_outer_window(_d(lw), _d(lik), k, n, rec.ctypes.data_as(_u64p)))
    return rec


def host_outer_walk(rec, n_total, ess_min):
    """(ess [j], j): walk through the steps of a window from the records of ALL segments [k][nseg][4] (smc_host_outer_walk)"""
    rec = np.ascontiguousarray(rec, dtype=np.uint64)
    k, nseg = rec.shape[0], rec.shape[1]
    ess = np.zeros(k)
    j = C.c_int()
    check(lib().smc_host_outer_walk(rec.ctypes.data_as(_u64p), k, nseg, int(n_total), float(ess_min), _d(ess), C.byref(j)))
    return ess[:j.value], j.value


def host_outer_advance(logw, logZ, lik, j):
    """keep the first j steps of a window: (logw, logZ) advanced (new arrays)   (smc_host_outer_advance)"""
    lik = np.ascontiguousarray(lik, dtype=np.float64)
    logw = np.array(logw, dtype=np.float64, order="C")
    logZ = np.array(logZ, dtype=np.float64, order="C")
    assert lik.shape[1] == logw.size == logZ.size and 0 <= j <= lik.shape[0]
    check(lib().smc_host_outer_advance(_d(logw), _d(logZ), _d(lik), int(j), logw.size))
    return logw, logZ


def host_outer_temper(logZ, xi, ess_min):
    """the tempering bisection (smc_samplers.jl:240-266): -> (xi_new, ess, resample_flag, logw)   (smc_host_outer_temper)"""
    logZ = np.ascontiguousarray(logZ, dtype=np.float64)
    lw = np.empty_like(logZ)
    nx, e, flag = C.c_double(), C.c_double(), C.c_int()
    check(lib().smc_host_outer_temper(_d(logZ), logZ.size, float(xi), float(ess_min), C.byref(nx), C.byref(e), C.byref(flag), _d(lw)))
    return nx.value, e.value, bool(flag.value), lw


def host_outer_resample(logw, m, seed):
    """ancestors (ascending, 0-based) of m iid draws from the weights exp(logw)   (smc_host_outer_resample)"""
    logw = np.ascontiguousarray(logw, dtype=np.float64)
    a = np.empty(int(m), dtype=np.int32)
    check(lib().smc_host_outer_resample(_d(logw), logw.size, int(m), int(seed), a.ctypes.data_as(_i32p)))
    return a


def host_rw_factor(theta):
    """(L [d][d], univariate) of random_walk_kernel(theta)   (smc_host_rw_factor)"""
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    n, d = theta.shape
    L = np.zeros((d, d))
    uni = C.c_int()
    check(lib().smc_host_rw_factor(_d(theta), n, d, _d(L), C.byref(uni)))
    return L, bool(uni.value)


def host_rw_factor_cov(cov):
    """(L [d][d], univariate): the tail of random_walk_kernel from a covariance [d][d]   (smc_host_rw_factor_cov)"""
    cov = np.ascontiguousarray(cov, dtype=np.float64)
    d = cov.shape[0]
    assert cov.shape == (d, d)
    L = np.zeros((d, d))
    uni = C.c_int()
    check(lib().smc_host_rw_factor_cov(_d(cov), d, _d(L), C.byref(uni)))
    return L, bool(uni.value)


def host_theta_moments(theta, logw=None, weighted=False):
    """(mean [d], cov [d][d]) of a theta cloud [M][d]: the sample moments (divisor M - 1), or with weighted=True the moments
    under the normalised weights of logw (smc_host_theta_moments: the device's specification on the host; no GPU)"""
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    M, d = theta.shape
    if weighted:
        logw = np.ascontiguousarray(logw, dtype=np.float64)
        assert logw.size == M
    mean, cov = np.zeros(d), np.zeros((d, d))
    check(lib().smc_host_theta_moments(_d(theta), _d(logw) if weighted else None, M, d, int(bool(weighted)), _d(mean), _d(cov)))
    return mean, cov


def host_theta_weights(logw):
    """(q [M] uint64, K, W): the integer weights of logw [M], their exponent maximum and their sum (smc_host_theta_weights)"""
    logw = np.ascontiguousarray(logw, dtype=np.float64).reshape(-1)
    q = np.zeros(logw.size, dtype=np.uint64)
    K, W = C.c_int32(), C.c_uint64()
    check(lib().smc_host_theta_weights(_d(logw), logw.size, q.ctypes.data_as(_u64p), C.byref(K), C.byref(W)))
    return q, K.value, W.value


def _theta_cloud(theta, logw):
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    logw = np.ascontiguousarray(logw, dtype=np.float64).reshape(-1)
    assert theta.ndim == 2 and logw.size == theta.shape[0]
    return theta, logw


def host_theta_quantiles(theta, logw, p):
    """out [d][np]: the weighted quantiles of every coordinate of a theta cloud [M][d] under logw [M] at the levels p
    (smc_host_theta_quantiles: the device's specification on the host; no GPU)"""
    theta, logw = _theta_cloud(theta, logw)
    p = np.ascontiguousarray(p, dtype=np.float64).reshape(-1)
    M, d = theta.shape
    out = np.zeros((d, p.size))
    check(lib().smc_host_theta_quantiles(_d(theta), _d(logw), M, d, _d(p), p.size, _d(out)))
    return out


def host_theta_histogram(theta, logw, component, lo, hi, nbins):
    """(counts [nbins + 3] uint64 = under | bins | over | nan, W) of one coordinate of a theta cloud (smc_host_theta_histogram)"""
    theta, logw = _theta_cloud(theta, logw)
    M, d = theta.shape
    counts = np.zeros(max(int(nbins), 0) + 3, dtype=np.uint64)
    W = C.c_uint64()
    check(lib().smc_host_theta_histogram(_d(theta), _d(logw), M, d, int(component), float(lo), float(hi), int(nbins),
                                         counts.ctypes.data_as(_u64p), C.byref(W)))
    return counts, W.value


def comm_unique_id():
    """the bytes rank 0 hands to the other ranks (smc_comm_unique_id)"""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    check(lib().smc_comm_unique_id(buf))
    return buf.raw


class Comm:
    """The samplers' collectives inside libsmchip.so over RCCL (smc_comm_*): what a host without torch.distributed
    binds to shard theta over the GPUs of a node.  Same interface as distributed.ThetaComm."""

    def __init__(self, unique_id, rank, world, device=0):
        self._c = C.c_void_p()
        self.rank, self.world = int(rank), int(world)
        check(lib().smc_comm_create(C.c_char_p(bytes(unique_id)), self.rank, self.world, int(device), C.byref(self._c)))

    def close(self):
        if getattr(self, "_c", None):
            lib().smc_comm_destroy(self._c)
            self._c = None

    def slice(self, M):
        if M % self.world:
            raise ValueError("n_theta (%d) must be a multiple of the number of ranks (%d)" % (M, self.world))
        per = M // self.world
        return self.rank * per, (self.rank + 1) * per

    def all_gather(self, local):
        local = np.ascontiguousarray(local, dtype=np.float64).ravel()
        out = np.zeros(local.size * self.world)
        check(lib().smc_comm_all_gather(self._c, _d(local), local.size, _d(out)))
        return out

    def outer_reweight(self, logw_local, want_w=True):
        """(logmu, w [n_local*world], ess, logw_all) of the sharded log-weights: smc_host_reweight of the concatenated vector,
        bit for bit; want_w=False: (logmu, None, ess, None) - whole-segment slices then exchange segment records only"""
        lw = np.ascontiguousarray(logw_local, dtype=np.float64).ravel()
        allw, w = (np.zeros(lw.size * self.world), np.zeros(lw.size * self.world)) if want_w else (None, None)
        lm, ess = C.c_double(), C.c_double()
        check(lib().smc_outer_reweight(self._c, _d(lw), lw.size, _d(allw), _d(w), C.byref(lm), C.byref(ess)))
        return lm.value, w, ess.value, allw

    def exchange_slots(self, h, a, M):
        a = np.ascontiguousarray(a, dtype=np.int32)
        check(lib().smc_comm_exchange_slots(self._c, h._h, a.ctypes.data_as(_i32p), int(M)))


class Handle:
    """n_theta bootstrap filters of n_x particles on one GPU (opaque smc_handle)."""

    def __init__(self, model_id, n_theta, n_x, seg=0, seed=1, device=0, flags=0):
        self._h = C.c_void_p()
        self.summary_mode = "weighted"
        self.model_id, self.n_theta, self.n_x = model_id, int(n_theta), int(n_x)
        check(lib().smc_create(model_id, self.n_theta, self.n_x, seg, seed, device, flags, C.byref(self._h)))
        seg_, nseg, d, res = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        check(lib().smc_get_geometry(self._h, C.byref(seg_), C.byref(nseg), C.byref(d), C.byref(res)))
        self.seg, self.nseg, self.d, self.resident = seg_.value, nseg.value, d.value, bool(res.value)
        self.flags = flags | (FLAG_ANCESTORS if flags & FLAG_ANCESTOR_SAMPLING else 0)   # (the library's own rule: smc_get_flags)

    @property
    def missing(self):
        """the handle reads a NaN observation as a missing one (FLAG_NAN_MISSING, read back from the library)"""
        f = C.c_uint32()
        check(lib().smc_get_flags(self._h, C.byref(f)))
        return bool(f.value & FLAG_NAN_MISSING)

    @property
    def conditional(self):
        """the handle runs the conditional particle filter (FLAG_CONDITIONAL, read back from the library)"""
        f = C.c_uint32()
        check(lib().smc_get_flags(self._h, C.byref(f)))
        return bool(f.value & FLAG_CONDITIONAL)

    def set_reference(self, xref):
        """the reference trajectory of a conditional handle, xref [T][d][n_theta] (smc_set_reference); replaces any earlier one"""
        xref = np.ascontiguousarray(xref, dtype=np.float64)
        if xref.ndim != 3 or xref.shape[1:] != (self.d, self.n_theta):
            raise ValueError("xref must be [T][d][n_theta]")
        check(lib().smc_set_reference(self._h, _d(xref), xref.shape[0]))

    def get_reference(self):
        """the reference [T][d][n_theta] as the device holds it (smc_get_reference)"""
        T = C.c_int64()
        check(lib().smc_get_reference(self._h, None, C.byref(T)))
        xref = np.zeros((T.value, self.d, self.n_theta))
        check(lib().smc_get_reference(self._h, _d(xref), None))
        return xref

    def reference_from_paths(self, p=0):
        """path p of the last sample_paths walk becomes the reference, gathered on the device (smc_reference_from_paths); returns
        the number of filters whose path was dead and that kept their reference"""
        kept = C.c_int64()
        check(lib().smc_reference_from_paths(self._h, int(p), C.byref(kept)))
        return kept.value

    @property
    def ancestor_sampling(self):
        """the handle draws its next reference by ancestor sampling (FLAG_ANCESTOR_SAMPLING, read back from the library)"""
        f = C.c_uint32()
        check(lib().smc_get_flags(self._h, C.byref(f)))
        return bool(f.value & FLAG_ANCESTOR_SAMPLING)

    def history_get_ancestors(self, t):
        """the ancestor vector [n_theta][n_x] (int32) of recorded step t of an ancestor-sampling handle: what state() gave after
        that step; row 0 reads -1 (smc_history_get_ancestors)"""
        a = np.zeros((self.n_theta, self.n_x), dtype=np.int32)
        check(lib().smc_history_get_ancestors(self._h, int(t), a.ctypes.data_as(_i32p)))
        return a

    def history_put_ancestors(self, t, a):
        """overwrite the ancestor vector of recorded step t (smc_history_put_ancestors): the planted cases of the tests"""
        a = np.ascontiguousarray(a, dtype=np.int32)
        if a.shape != (self.n_theta, self.n_x):
            raise ValueError("a must be [n_theta][n_x]")
        check(lib().smc_history_put_ancestors(self._h, int(t), a.ctypes.data_as(_i32p)))

    def ancestor_sweep(self, path_seed):
        """the ancestor-sampling sweep over the record (smc_ancestor_sweep): the new reference replaces the old one on the device
        (get_reference); returns (J [T][n_theta] the ancestor draws, idx [T][n_theta] the particles the new path passes through,
        both int32, and the number of dead filters that kept their reference)"""
        T = self.history_len()
        J = np.zeros((T, self.n_theta), dtype=np.int32)
        idx = np.zeros((T, self.n_theta), dtype=np.int32)
        kept = C.c_int64()
        check(lib().smc_ancestor_sweep(self._h, int(path_seed), J.ctypes.data_as(_i32p), idx.ctypes.data_as(_i32p), C.byref(kept)))
        return J, idx, kept.value

    def close(self):
        if getattr(self, "_h", None):
            lib().smc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_params(self, raw):
        raw = np.ascontiguousarray(raw, dtype=np.float64).reshape(self.n_theta, -1)
        assert raw.shape[1] == lib().smc_model_nraw(self.model_id)
        check(lib().smc_set_params(self._h, _d(raw)))

    def set_proposal(self, kind, par=None):
        """the proposal of the handle's filters from the next step on (smc_set_proposal): PROP_NONE (bootstrap, the default),
        PROP_AFFINE with rows par [n_theta][4] = (c0, c1, c2, s2) (LG1D), or PROP_OPTIMAL (LG1D, UCSV3D; derived from the
        parameter rows, also after later set_params calls)"""
        if par is not None:
            par = np.ascontiguousarray(par, dtype=np.float64)
            if par.size == PROP_NPAR and self.n_theta > 1:
                par = np.tile(par.reshape(1, PROP_NPAR), (self.n_theta, 1))
            if par.size != self.n_theta * PROP_NPAR:
                raise ValueError("proposal rows must be [n_theta][4]")
            par = np.ascontiguousarray(par)
        check(lib().smc_set_proposal(self._h, int(kind), _d(par)))
        self.proposal_kind = int(kind)

    def set_streams(self, streams):
        """the stream ids of the filters (smc_set_streams, which drops a pending window).  Ids equal to the ones this object set
        last are not handed to the library: such a call changes nothing, a pending window included."""
        s = np.ascontiguousarray(streams, dtype=np.uint32)
        assert s.size == self.n_theta
        if getattr(self, "_streams_set", None) is not None and np.array_equal(self._streams_set, s):
            return                     # unchanged (the samplers hand over the same global indices at every round): no upload, no wait
        check(lib().smc_set_streams(self._h, s.ctypes.data_as(_u32p)))
        self._streams_set = s.copy()

    def reseed(self, seed):
        check(lib().smc_reseed(self._h, seed))

    @property
    def step_by_value(self):
        """diagnostic: the next step launches take the filter's row by value in the kernel arguments (smc_step_by_value)"""
        b = C.c_int()
        check(lib().smc_step_by_value(self._h, C.byref(b)))
        return bool(b.value)

    def launch_geometry(self):
        """diagnostic: (threads, np, resident_np) - the workgroup geometry of the step launches as SMC_NP left it at smc_create, and
        the pairs per thread the LDS-resident kernels would be asked for now (SMC_RES_NP read at this call; 0 = their own choice)
        (smc_get_launch_geometry)"""
        t, k, r = C.c_int(), C.c_int(), C.c_int()
        check(lib().smc_get_launch_geometry(self._h, C.byref(t), C.byref(k), C.byref(r)))
        return t.value, k.value, r.value

    def init(self, y1):
        lm = np.zeros(self.n_theta)
        check(lib().smc_init(self._h, float(y1), _d(lm)))
        return lm

    def step(self, y):
        lm = np.zeros(self.n_theta)
        ess = np.zeros(self.n_theta)
        check(lib().smc_step(self._h, float(y), _d(lm), _d(ess)))
        return lm, ess

    def step_window(self, y):
        """len(y) bootstrap_filter! steps in one launch, not yet kept: ([k][n_theta] logmu, [k][n_theta] ess);
        follow with step_commit(j)."""
        y = np.ascontiguousarray(y, dtype=np.float64)
        lm = np.zeros((y.size, self.n_theta))
        ess = np.zeros((y.size, self.n_theta))
        check(lib().smc_step_window(self._h, _d(y), y.size, _d(lm), _d(ess)))
        return lm, ess

    def step_commit(self, j):
        check(lib().smc_step_commit(self._h, int(j)))

    @property
    def can_window(self):
        return self.nseg == 1 and self.resident

    def log_likelihood(self, y, trace=False):
        y = np.ascontiguousarray(y, dtype=np.float64)
        logZ = np.zeros(self.n_theta)
        if trace:
            lm = np.zeros((y.size, self.n_theta))
            es = np.zeros((y.size, self.n_theta))
            check(lib().smc_log_likelihood(self._h, _d(y), y.size, _d(logZ), _d(lm), _d(es)))
            return logZ, lm, es
        check(lib().smc_log_likelihood(self._h, _d(y), y.size, _d(logZ), None, None))
        return logZ

    def state(self, want_w=True, want_anc=None):
        x = np.zeros((self.d, self.n_theta, self.n_x))
        w = np.zeros((self.n_theta, self.n_x)) if want_w else None
        if want_anc is None:
            want_anc = bool(self.flags & FLAG_ANCESTORS)
        a = np.zeros((self.n_theta, self.n_x), dtype=np.int32) if want_anc else None
        check(lib().smc_get_state(self._h, _d(x), _d(w), a.ctypes.data_as(_i32p) if a is not None else None))
        return x, w, a

    def logZ(self):
        z = np.zeros(self.n_theta)
        e = np.zeros(self.n_theta)
        check(lib().smc_get_logZ(self._h, _d(z), _d(e)))
        return z, e

    def permute(self, a):
        a = np.ascontiguousarray(a, dtype=np.int32)
        assert a.size == self.n_theta
        check(lib().smc_permute(self._h, a.ctypes.data_as(_i32p)))

    def set_summary_mode(self, mode):
        """"weighted" (the default) or "unweighted": which statistics quantiles(), moments() and the per-step summaries compute from
        now on (smc_set_summary_mode).  "unweighted" is the README loop's quantile(x, p) (type 7, interpolating) and var(x)
        (corrected) of the cloud whatever its weights."""
        if mode not in _SUMM_MODES:
            raise ValueError("summary mode must be 'weighted' or 'unweighted'")
        check(lib().smc_set_summary_mode(self._h, _SUMM_MODES[mode]))
        self.summary_mode = mode

    def moments(self):
        """filtered (mean, variance) of every state coordinate, [d][n_theta] each, computed on the device (in the handle's summary
        mode: weighted mean and uncorrected variance, or the cloud's sample mean and corrected variance)."""
        m = np.zeros((self.d, self.n_theta))
        v = np.zeros((self.d, self.n_theta))
        check(lib().smc_get_moments(self._h, _d(m), _d(v)))
        return m, v

    def predictive(self, y_t):
        """(pit, obs_mean, obs_var), each [n_theta]: the probability integral transform of y_t and the mean and variance of the
        one-step predictive law of the observation, from the current cloud whatever its weights (smc_get_predictive; y_t is the
        observation the last step assimilated).  Bootstrap handles of LG1D, SV1D, UCSV3D."""
        out = np.zeros((3, self.n_theta))
        check(lib().smc_get_predictive(self._h, float(y_t), _d(out[0]), _d(out[1]), _d(out[2])))
        return out[0], out[1], out[2]

    def predictive_record(self, y):
        """the same rows for every step of the record (smc_predictive, one launch): (pit, obs_mean, obs_var), each [T][n_theta]"""
        y = np.ascontiguousarray(y, dtype=np.float64).ravel()
        out = np.zeros((3, y.size, self.n_theta))
        check(lib().smc_predictive(self._h, _d(y), y.size, _d(out[0]), _d(out[1]), _d(out[2])))
        return out[0], out[1], out[2]

    def quantiles(self, p, component=0):
        """quantiles of one state coordinate, [n_theta][len(p)], on the device (in the handle's summary mode: the inverse of the
        weighted empirical CDF, or the cloud's unweighted type-7 quantiles)."""
        p = np.ascontiguousarray(p, dtype=np.float64).ravel()
        out = np.zeros((self.n_theta, p.size))
        check(lib().smc_get_quantiles(self._h, int(component), _d(p), p.size, _d(out)))
        return out

    def set_summaries(self, p=None, component=0, moments=False):
        """per-step summaries inside the following log_likelihood / step_window calls (smc_set_summaries): quantiles of one state
        coordinate at the levels p (<= 8) and / or mean and variance of every coordinate, in the handle's summary mode
        (set_summary_mode); set_summaries() switches it off"""
        p = np.ascontiguousarray([] if p is None else p, dtype=np.float64).ravel()
        check(lib().smc_set_summaries(self._h, int(component), _d(p) if p.size else None, p.size, int(bool(moments))))
        self._sum_np, self._sum_mom = int(p.size), bool(moments)

    def get_summaries(self, T):
        """(q [T][n_theta][np] or None, mean [T][d][n_theta] or None, var or None) of the first T steps of the last such call"""
        nq, mom = getattr(self, "_sum_np", 0), getattr(self, "_sum_mom", False)
        q = np.zeros((T, self.n_theta, nq)) if nq else None
        mean = np.zeros((T, self.d, self.n_theta)) if mom else None
        var = np.zeros((T, self.d, self.n_theta)) if mom else None
        check(lib().smc_get_summaries(self._h, int(T), _d(q), _d(mean), _d(var)))
        return q, mean, var

    def forecast(self, H, seed, p=None, component=0, obs=True):
        """the cloud propagated H steps past the last observation, summarised per horizon on the device under the current weights
        (smc_forecast; always the weighted definitions): a dict of mean, var [H][d][n_theta], q [H][n_theta][len(p)] (p given) and,
        with obs, obs_mean, obs_var [H][n_theta] and obs_q of the predictive law of y.  seed: the Philox key of the forecast draws."""
        H = int(H)
        p = np.ascontiguousarray([] if p is None else p, dtype=np.float64).ravel()
        out = {"mean": np.zeros((H, self.d, self.n_theta)), "var": np.zeros((H, self.d, self.n_theta))}
        if p.size:
            out["q"] = np.zeros((H, self.n_theta, p.size))
        if obs:
            out["obs_mean"], out["obs_var"] = np.zeros((H, self.n_theta)), np.zeros((H, self.n_theta))
            if p.size:
                out["obs_q"] = np.zeros((H, self.n_theta, p.size))
        check(lib().smc_forecast(self._h, H, int(seed) & 0xFFFFFFFFFFFFFFFF, int(component), _d(p) if p.size else None, p.size, _d(out["mean"]),
                                 _d(out["var"]), _d(out.get("q")), _d(out.get("obs_mean")), _d(out.get("obs_var")), _d(out.get("obs_q"))))
        return out

    def forecast_cloud(self, H, seed, want_y=True):
        """(xf [H][d][n_theta][n_x], yf [H][n_theta][n_x] or None): the propagated clouds themselves and the predictive draws of y
        (smc_forecast_cloud); with the w of state() they are weighted trajectories"""
        H = int(H)
        xf = np.zeros((H, self.d, self.n_theta, self.n_x))
        yf = np.zeros((H, self.n_theta, self.n_x)) if want_y else None
        check(lib().smc_forecast_cloud(self._h, H, int(seed) & 0xFFFFFFFFFFFFFFFF, _d(xf), _d(yf)))
        return xf, yf

    def copy_from(self, src, mask):
        m = np.ascontiguousarray(mask, dtype=np.uint8)
        assert m.size == self.n_theta
        check(lib().smc_copy_from(self._h, src._h, m.ctypes.data_as(C.POINTER(C.c_uint8))))

    def set_skip(self, skip):
        """filters the following log_likelihood calls leave out; None: run all again.  A skipped filter reads logZ = -inf,
        NaN in its trace columns and summary rows, and keeps its x, w, ancestors and raw weights (include/smc_hip.h)"""
        if skip is None:
            check(lib().smc_set_skip(self._h, None))
            return
        m = np.ascontiguousarray(skip, dtype=np.uint8)
        assert m.size == self.n_theta
        check(lib().smc_set_skip(self._h, m.ctypes.data_as(C.POINTER(C.c_uint8))))

    def pmmh_configure(self, families, pars, raw_from, raw_const):
        """prior components and the theta -> parameter-row map of smc_pmmh_rejuvenate (see include/smc_hip.h)"""
        fam = np.ascontiguousarray(families, dtype=np.int32)
        par = np.ascontiguousarray(pars, dtype=np.float64).reshape(fam.size, PRIOR_NPAR)
        rf = np.ascontiguousarray(raw_from, dtype=np.int32)
        rc = np.ascontiguousarray(raw_const, dtype=np.float64)
        assert rf.size == rc.size == lib().smc_model_nraw(self.model_id)
        check(lib().smc_pmmh_configure(self._h, fam.size, fam.ctypes.data_as(_i32p), _d(par), rf.ctypes.data_as(_i32p), _d(rc)))
        self._pmmh_d = int(fam.size)

    def pmmh_rejuvenate(self, main, y, xi, chol, scales, filter_seeds, move_seed, theta, logZ):
        """rejuvenate!(smc, y, xi) for this handle's parameter particles, on the device.
        Returns (theta, logZ, accepted, filters_run); theta / logZ are new arrays."""
        y = np.ascontiguousarray(y, dtype=np.float64)
        d = self._pmmh_d
        theta = np.array(theta, dtype=np.float64, order="C").reshape(self.n_theta, d)
        logZ = np.array(logZ, dtype=np.float64, order="C").reshape(self.n_theta)
        chol = np.ascontiguousarray(chol, dtype=np.float64).reshape(d, d)
        scales = np.ascontiguousarray(scales, dtype=np.float64)
        seeds = np.ascontiguousarray(filter_seeds, dtype=np.uint64)
        assert seeds.size == scales.size
        acc = np.zeros(self.n_theta, dtype=np.uint8)
        nrun = C.c_int64()
        check(lib().smc_pmmh_rejuvenate(self._h, main._h if main is not None else None, _d(y), y.size, float(xi), _d(chol),
                                        _d(scales), scales.size, seeds.ctypes.data_as(_u64p), int(move_seed), _d(theta), _d(logZ),
                                        acc.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(nrun)))
        return theta, logZ, acc.astype(bool), int(nrun.value)

    def slot_bytes(self):
        b = C.c_int64()
        check(lib().smc_slot_bytes(self._h, C.byref(b)))
        return b.value

    def pack_slots(self, idx, device_ptr):
        """idx: local slot indices; device_ptr: integer address of a device buffer of len(idx)*slot_bytes() bytes."""
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        check(lib().smc_pack_slots(self._h, idx.ctypes.data_as(_i32p), idx.size, C.c_void_p(int(device_ptr))))

    def unpack_slots(self, idx, device_ptr):
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        check(lib().smc_unpack_slots(self._h, idx.ctypes.data_as(_i32p), idx.size, C.c_void_p(int(device_ptr))))

    def weights_raw(self):
        npad = self.nseg * self.seg
        Cc = np.zeros((self.n_theta, npad), dtype=np.uint64)
        m = np.zeros((self.n_theta, self.nseg))
        S = np.zeros((self.n_theta, self.nseg), dtype=np.uint64)
        hi = np.zeros_like(S)
        lo = np.zeros_like(S)
        check(lib().smc_get_weights_raw(self._h, Cc.ctypes.data_as(_u64p), _d(m), S.ctypes.data_as(_u64p),
                                        hi.ctypes.data_as(_u64p), lo.ctypes.data_as(_u64p)))
        return Cc, m, S, hi, lo

    def elapsed_ms(self):
        ms = C.c_double()
        check(lib().smc_last_elapsed_ms(self._h, C.byref(ms)))
        return ms.value

    def time_step_kernel(self, y, nsample=64):
        """(avg_ms, min_ms) of one k_step launch, HIP events on the kernel's own stream."""
        y = np.ascontiguousarray(y, dtype=np.float64)
        a, m = C.c_double(), C.c_double()
        check(lib().smc_time_step_kernel(self._h, _d(y), y.size, nsample, C.byref(a), C.byref(m)))
        return a.value, m.value

    def event_overhead_ms(self, nsample=64):
        a = C.c_double()
        check(lib().smc_event_overhead_ms(self._h, nsample, C.byref(a)))
        return a.value

    def synchronize(self):
        check(lib().smc_synchronize(self._h))

    def history_begin(self, T_cap):
        """record the state every following init / step leaves, up to T_cap steps (smc_history_begin); init restarts the record"""
        check(lib().smc_history_begin(self._h, int(T_cap)))

    def history_len(self):
        n = C.c_int64()
        check(lib().smc_history_len(self._h, C.byref(n)))
        return n.value

    def history_get(self, t):
        """(x [d][n_theta][n_x], w [n_theta][n_x]) of recorded step t (0-based): what state() gave after that step"""
        x = np.zeros((self.d, self.n_theta, self.n_x))
        w = np.zeros((self.n_theta, self.n_x))
        check(lib().smc_history_get(self._h, int(t), _d(x), _d(w)))
        return x, w

    def history_put(self, t, x=None, w=None):
        """overwrite recorded step t with x [d][n_theta][n_x] and / or w [n_theta][n_x] (smc_history_put; None: left alone):
        clouds that no filter run leaves, for the tests of the backward pass"""
        if x is not None:
            x = np.ascontiguousarray(x, dtype=np.float64)
            if x.shape != (self.d, self.n_theta, self.n_x):
                raise ValueError("x must be [d][n_theta][n_x]")
        if w is not None:
            w = np.ascontiguousarray(w, dtype=np.float64)
            if w.shape != (self.n_theta, self.n_x):
                raise ValueError("w must be [n_theta][n_x]")
        check(lib().smc_history_put(self._h, int(t), _d(x), _d(w)))

    def history_end(self):
        check(lib().smc_history_end(self._h))

    def smooth(self, weights=True, moments=True, pairs=False, quantiles=None):
        """the FFBS backward pass over the recorded steps (smc_smooth): (ws [T][n_theta][n_x] or None, mean [T][d][n_theta] or
        None, var or None); pairs=True (smc_smooth_pairs): the lag-one pair moments follow, (..., cross [T-1][d][d][n_theta],
        resid2 [T-1][d][n_theta]); quantiles=(component, p) (smc_smooth_quantiles, the same pass): the weighted quantiles of that
        state coordinate at the levels p come last, (..., q [T][n_theta][len(p)])"""
        T = self.history_len()
        ws = np.zeros((T, self.n_theta, self.n_x)) if weights else None
        mean = np.zeros((T, self.d, self.n_theta)) if moments else None
        var = np.zeros((T, self.d, self.n_theta)) if moments else None
        if not pairs and quantiles is None:
            check(lib().smc_smooth(self._h, _d(ws), _d(mean), _d(var)))
            return ws, mean, var
        cross = np.zeros((max(T - 1, 0), self.d, self.d, self.n_theta)) if pairs else None
        resid2 = np.zeros((max(T - 1, 0), self.d, self.n_theta)) if pairs else None
        if quantiles is None:
            check(lib().smc_smooth_pairs(self._h, _d(ws), _d(mean), _d(var), _d(cross), _d(resid2)))
            return ws, mean, var, cross, resid2
        component, p = quantiles
        p = np.ascontiguousarray(p, dtype=np.float64).ravel()
        q = np.zeros((T, self.n_theta, p.size))
        check(lib().smc_smooth_quantiles(self._h, _d(ws), _d(mean), _d(var), _d(cross), _d(resid2), int(component), _d(p), int(p.size), _d(q)))
        return (ws, mean, var, cross, resid2, q) if pairs else (ws, mean, var, q)

    def smooth_quantiles_scratch(self):
        """bytes of the handle's quantile block (smc_smooth_quantiles_info): 0 until smooth(quantiles=...) was asked for"""
        b = C.c_int64()
        check(lib().smc_smooth_quantiles_info(self._h, C.byref(b), None, None))
        return b.value

    def sample_paths(self, M, seed, counts=None, want_x=True):
        """M backward-simulated paths per filter over the recorded steps (smc_sample_paths): (idx [T][n_theta][M] int32, xs
        [T][d][n_theta][M] or None).  counts [n_theta]: only the first counts[th] paths of filter th are drawn, the other slots
        read -1 / NaN"""
        T = self.history_len()
        M, counts, cp = self._path_args(M, counts)
        idx = np.zeros((T, self.n_theta, M), dtype=np.int32)
        xs = np.zeros((T, self.d, self.n_theta, M)) if want_x else None
        check(lib().smc_sample_paths(self._h, M, int(seed), cp, idx.ctypes.data_as(_i32p), _d(xs)))
        return idx, xs

    def _path_args(self, M, counts):
        """the checks the two path calls share: (M, counts as int32 [n_theta] or None, its pointer or None)"""
        M = int(M)
        if M < 1:
            raise ValueError("M must be positive")
        if counts is None:
            return M, None, None
        counts = np.ascontiguousarray(counts, dtype=np.int32)
        if counts.shape != (self.n_theta,):
            raise ValueError("counts must be [n_theta]")
        return M, counts, counts.ctypes.data_as(_i32p)

    def rb_sample_paths(self, y, M, seed, counts=None, draws=False, per_path=True, summary=True):
        """M Rao-Blackwellised backward-simulated paths per filter over the record of a MODEL_UCSV_RB handle
        (smc_rb_sample_paths; y [T]: the observations the recorded steps saw): a dict with "idx" [T][n_theta][M] int32, "vol"
        [T][2][n_theta][M] the (lse, lsn) of every path, "tmean", "tvar" [T][n_theta][M] the exact trend moments given each path
        (per_path=False leaves these four out), "tdraw" [T][n_theta][M] a joint trend draw per path (draws=True) and "out"
        [T][n_theta][8] the summary over the paths (summary=True).  counts as in sample_paths"""
        y = np.ascontiguousarray(y, dtype=np.float64).ravel()
        T = y.size
        M, counts, cp = self._path_args(M, counts)
        r = {}
        if per_path:
            r["idx"] = np.zeros((T, self.n_theta, M), dtype=np.int32)
            r["vol"] = np.zeros((T, 2, self.n_theta, M))
            r["tmean"], r["tvar"] = np.zeros((T, self.n_theta, M)), np.zeros((T, self.n_theta, M))
        if draws:
            r["tdraw"] = np.zeros((T, self.n_theta, M))
            if "vol" not in r:
                r["vol"] = np.zeros((T, 2, self.n_theta, M))
        if summary:
            r["out"] = np.zeros((T, self.n_theta, 8))
        check(lib().smc_rb_sample_paths(self._h, _d(y), T, M, int(seed), cp, r["idx"].ctypes.data_as(_i32p) if "idx" in r else None,
                                        _d(r.get("vol")), _d(r.get("tmean")), _d(r.get("tvar")), _d(r.get("tdraw")), _d(r.get("out"))))
        return r


def host_rb_sample_paths(raw, x, w, y, M, seed, stream=0, draws=True, summary=True):
    """M Rao-Blackwellised backward-simulated paths of ONE MODEL_UCSV_RB filter by the specification on the host
    (smc_host_rb_sample_paths; no GPU): raw [5], x [T][4][n], w [T][n], y [T] -> a dict with "idx" [T][M] int32, "vol" [T][2][M],
    "tmean", "tvar" [T][M], "tdraw" [T][M] (draws) and "out" [T][8] (summary)"""
    raw = np.ascontiguousarray(raw, dtype=np.float64).ravel()
    if raw.size != 5:
        raise ValueError("raw must be UCSV's five parameters")
    w = np.ascontiguousarray(w, dtype=np.float64)
    T, n = w.shape
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(T, 4, n)
    y = np.ascontiguousarray(y, dtype=np.float64).ravel()
    if y.size != T:
        raise ValueError("y must be [T]")
    Mz = max(int(M), 0)
    r = {"idx": np.zeros((T, Mz), dtype=np.int32), "vol": np.zeros((T, 2, Mz)), "tmean": np.zeros((T, Mz)), "tvar": np.zeros((T, Mz))}
    if draws:
        r["tdraw"] = np.zeros((T, Mz))
    if summary:
        r["out"] = np.zeros((T, 8))
    check(lib().smc_host_rb_sample_paths(_d(raw), T, n, _d(x), _d(w), _d(y), int(M), int(seed), int(stream), r["idx"].ctypes.data_as(_i32p),
                                         _d(r["vol"]), _d(r["tmean"]), _d(r["tvar"]), _d(r.get("tdraw")), _d(r.get("out"))))
    return r


def host_forecast(model_id, raw, x, H, seed, stream=0):
    """the forecast specification on the host (smc_host_forecast): x [d][n] (or [n] for a scalar state) of ONE filter ->
    (xf [H][d][n], yf, ym, yv [H][n]); the device clouds equal it bit for bit"""
    raw = np.ascontiguousarray(raw, dtype=np.float64).ravel()
    d = lib().smc_model_dim(model_id)
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(d, -1)
    n, H = x.shape[1], int(H)
    xf = np.zeros((H, d, n))
    yf, ym, yv = np.zeros((H, n)), np.zeros((H, n)), np.zeros((H, n))
    check(lib().smc_host_forecast(model_id, _d(raw), _d(x), n, H, int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream), _d(xf), _d(yf), _d(ym), _d(yv)))
    return xf, yf, ym, yv


def host_sample_paths(model_id, raw, x, w, M, seed, stream=0, want_x=True):
    """M backward-simulated paths of ONE filter by the specification on the host (smc_host_sample_paths; no GPU): x [T][d][n],
    w [T][n] -> (idx [T][M] int32, xs [T][d][M] or None)"""
    raw = np.ascontiguousarray(raw, dtype=np.float64).ravel()
    d = lib().smc_model_dim(int(model_id))
    w = np.ascontiguousarray(w, dtype=np.float64)
    T, n = w.shape
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(T, d, n) if d > 0 else np.ascontiguousarray(x, dtype=np.float64)
    idx = np.zeros((T, max(int(M), 0)), dtype=np.int32)
    xs = np.zeros((T, d, max(int(M), 0))) if want_x else None
    check(lib().smc_host_sample_paths(int(model_id), _d(raw), T, n, _d(x), _d(w), int(M), int(seed), int(stream),
                                      idx.ctypes.data_as(_i32p), _d(xs)))
    return idx, xs


def host_ancestor_sweep(model_id, raw, x, w, a, xref, seed, path_seed, stream=0):
    """the ancestor-sampling sweep of ONE filter by the specification on the host (smc_host_ancestor_sweep; no GPU): x [T][d][n],
    w [T][n], a [T][n] int32 (row 0 is not read), xref [T][d] -> (J [T] int32, idx [T] int32, xref_out [T][d])"""
    raw = np.ascontiguousarray(raw, dtype=np.float64).ravel()
    d = lib().smc_model_dim(int(model_id))
    w = np.ascontiguousarray(w, dtype=np.float64)
    T, n = w.shape
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(T, max(d, 1), n)
    a = np.ascontiguousarray(a, dtype=np.int32).reshape(T, n)
    xref = np.ascontiguousarray(xref, dtype=np.float64).reshape(T, max(d, 1))
    J, idx, out = np.zeros(T, dtype=np.int32), np.zeros(T, dtype=np.int32), np.zeros((T, max(d, 1)))
    check(lib().smc_host_ancestor_sweep(int(model_id), _d(raw), T, n, _d(x), _d(w), a.ctypes.data_as(_i32p), _d(xref), int(seed), int(path_seed),
                                        int(stream), J.ctypes.data_as(_i32p), idx.ctypes.data_as(_i32p), _d(out)))
    return J, idx, out


def host_transition_logpdf(model_id, raw, xp, x):
    """logpdf(transition(model, xp), x) by the specification on the host (smc_host_transition_logpdf; no GPU)"""
    raw = np.ascontiguousarray(raw, dtype=np.float64).ravel()
    xp = np.ascontiguousarray(xp, dtype=np.float64).ravel()
    x = np.ascontiguousarray(x, dtype=np.float64).ravel()
    d = lib().smc_model_dim(int(model_id))
    assert xp.size == d and x.size == d
    out = C.c_double()
    check(lib().smc_host_transition_logpdf(int(model_id), _d(raw), _d(xp), _d(x), C.byref(out)))
    return out.value


def host_smooth(model_id, raw, x, w, moments=True):
    """the FFBS smoother of ONE filter by the specification on the host (smc_host_smooth; no GPU): x [T][d][n], w [T][n] ->
    (ws [T][n], mean [T][d], var [T][d]); moments=False: (ws, None, None)"""
    raw = np.ascontiguousarray(raw, dtype=np.float64).ravel()
    d = lib().smc_model_dim(int(model_id))
    w = np.ascontiguousarray(w, dtype=np.float64)
    T, n = w.shape
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(T, d, n)
    ws = np.zeros((T, n))
    mean, var = (np.zeros((T, d)), np.zeros((T, d))) if moments else (None, None)
    check(lib().smc_host_smooth(int(model_id), _d(raw), T, n, _d(x), _d(w), _d(ws), _d(mean), _d(var)))
    return ws, mean, var


def host_smooth_pairs(model_id, raw, x, w):
    """host_smooth with the lag-one pair moments of the same filter (smc_host_smooth_pairs; no GPU): (ws [T][n], mean [T][d],
    var [T][d], cross [T-1][d][d], resid2 [T-1][d])"""
    raw = np.ascontiguousarray(raw, dtype=np.float64).ravel()
    d = lib().smc_model_dim(int(model_id))
    w = np.ascontiguousarray(w, dtype=np.float64)
    T, n = w.shape
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(T, d, n)
    ws, mean, var = np.zeros((T, n)), np.zeros((T, d)), np.zeros((T, d))
    cross, resid2 = np.zeros((max(T - 1, 0), d, d)), np.zeros((max(T - 1, 0), d))
    check(lib().smc_host_smooth_pairs(int(model_id), _d(raw), T, n, _d(x), _d(w), _d(ws), _d(mean), _d(var), _d(cross), _d(resid2)))
    return ws, mean, var, cross, resid2


def host_smooth_quantiles(x, ws, p):
    """the weighted quantiles of ONE state coordinate of ONE filter under the smoothed weights by the specification on the host
    (smc_host_smooth_quantiles; no GPU): x, ws [T][n], levels p -> q [T][len(p)]"""
    ws = np.ascontiguousarray(ws, dtype=np.float64)
    T, n = ws.shape
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(T, n)
    p = np.ascontiguousarray(p, dtype=np.float64).ravel()
    q = np.zeros((T, p.size))
    check(lib().smc_host_smooth_quantiles(T, n, _d(x), _d(ws), _d(p), int(p.size), _d(q)))
    return q


def smooth_quantiles_constants():
    """(SMOOTH_Q_BITS, SMOOTH_Q_LDS_MAX) of the library (smc_smooth_quantiles_info): the bits of an integer weight, and the
    largest n_x whose cloud k_smooth_quantiles stages in LDS"""
    bits, lds = C.c_int32(), C.c_int64()
    check(lib().smc_smooth_quantiles_info(None, None, C.byref(bits), C.byref(lds)))
    return bits.value, lds.value


def host_ibis_summary(rows, x, S, logw, ahead=0):
    """(y, Sigma, between, xbar, Sbar, between_x, K, D) of a cloud of LG1D rows [M][6] with Kalman state (x, S) and outer
    log-weights logw (smc_host_ibis_summary: the device's specification on the host; no GPU)"""
    rows = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, 6)
    x, S, logw = (np.ascontiguousarray(v, dtype=np.float64) for v in (x, S, logw))
    assert x.size == S.size == logw.size == rows.shape[0]
    out = np.zeros(8)
    check(lib().smc_host_ibis_summary(_d(rows), _d(x), _d(S), _d(logw), x.size, int(ahead), _d(out)))
    return out


def host_ibis_smooth(rows, logw, y, predict_first=False, states=False, filtered=False, missing=False):
    """the RTS smoother of a cloud of LG1D rows [M][6] with outer log-weights logw over y (smc_host_ibis_smooth: the device's
    specification on the host; no GPU) -> out [T][8], the rows of host_ibis_summary per period; with states also xs, Ps [T][M];
    with filtered also the filtered record xf, Sf [T][M] the backward pass ran over"""
    rows = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, 6)
    logw, y = np.ascontiguousarray(logw, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64).ravel()
    M, T = rows.shape[0], y.size
    assert logw.size == M
    out = np.zeros((T, 8))
    xs, Ps = (np.zeros((T, M)), np.zeros((T, M))) if states else (None, None)
    xf, Sf = (np.zeros((T, M)), np.zeros((T, M))) if filtered else (None, None)
    check(lib().smc_host_ibis_smooth_flags(_d(rows), _d(logw), M, _d(y), T, int(bool(predict_first)), _d(out), _d(xs), _d(Ps), _d(xf), _d(Sf),
                                           _kalman_flags(missing)))
    return (out,) + ((xs, Ps) if states else ()) + ((xf, Sf) if filtered else ()) if states or filtered else out


def host_ibis_sample_paths(rows, y, which, path_seed, predict_first=False, want_z=False, missing=False):
    """paths [T][Mp] of smc_host_ibis_sample_paths: path p under row which[p] (no GPU); with want_z also the normals z [T][Mp]"""
    rows = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, 6)
    y = np.ascontiguousarray(y, dtype=np.float64).ravel()
    which = np.ascontiguousarray(which, dtype=np.int32).ravel()
    paths = np.zeros((y.size, which.size))
    z = np.zeros((y.size, which.size)) if want_z else None
    check(lib().smc_host_ibis_sample_paths_flags(_d(rows), rows.shape[0], _d(y), y.size, int(bool(predict_first)), which.size, int(path_seed),
                                                 which.ctypes.data_as(_i32p), _d(paths), _d(z), _kalman_flags(missing)))
    return (paths, z) if want_z else paths


class IbisHandle:
    """The device half of the IBIS sampler (smc_ibis_*): M parameter particles with their exact Kalman state, resident on one
    GPU.  d: parameter dimension; families / pars: the prior (distributions.py spec()); raw_from / raw_const: ThetaMap to LG1D rows.
    row_id=MODEL_LG2D: two-state rows of 15 entries (smc_ibis_create_rows); x is then [M][2] and S [M][3], the lower triangle."""

    def __init__(self, M, d, families, pars, raw_from, raw_const, seed=1, device=0, predict_first=False, flags=0, row_id=MODEL_LG1D):
        self._h = C.c_void_p()
        self.M, self.d = int(M), int(d)
        self.nseg = (self.M + OUTER_SEG - 1) // OUTER_SEG
        self.row_id = int(row_id)
        self.nraw, self.nx, self.nS = (LG2_NRAW, 2, 3) if self.row_id == MODEL_LG2D else (6, 1, 1)
        if self.row_id == MODEL_LG1D:                      # (a scalar handle makes the calls it made before)
            check(lib().smc_ibis_create(self.M, int(seed), int(device), int(bool(predict_first)), C.byref(self._h)))
        else:
            check(lib().smc_ibis_create_rows(self.M, int(seed), int(device), int(bool(predict_first)), self.row_id, C.byref(self._h)))
        fam = np.ascontiguousarray(families, dtype=np.int32)
        par = np.ascontiguousarray(pars, dtype=np.float64).reshape(fam.size, PRIOR_NPAR)
        rf = np.ascontiguousarray(raw_from, dtype=np.int32)
        rc = np.ascontiguousarray(raw_const, dtype=np.float64)
        assert fam.size == self.d and rf.size == rc.size == self.nraw
        check(lib().smc_ibis_configure(self._h, self.d, fam.ctypes.data_as(_i32p), _d(par), rf.ctypes.data_as(_i32p), _d(rc)))
        if flags:                                          # (an unflagged handle makes the calls it made before)
            self.set_flags(flags)

    def set_flags(self, flags):
        """0 or FLAG_NAN_MISSING: a NaN observation is a missing Kalman step (smc_ibis_set_flags; only at t = 0)"""
        check(lib().smc_ibis_set_flags(self._h, int(flags)))

    @property
    def flags(self):
        f = C.c_uint32()
        check(lib().smc_ibis_get_flags(self._h, C.byref(f)))
        return int(f.value)

    def close(self):
        if getattr(self, "_h", None):
            lib().smc_ibis_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_theta(self, theta):
        theta = np.ascontiguousarray(theta, dtype=np.float64).reshape(self.M, self.d)
        check(lib().smc_ibis_set_theta(self._h, _d(theta)))

    def window(self, y, want_lik=False):
        """len(y) online steps in one launch, not yet kept: (records [k][nseg][4] uint64, lik [k][M] or None); follow with commit(j)"""
        y = np.ascontiguousarray(y, dtype=np.float64)
        rec = np.zeros((y.size, self.nseg, 4), dtype=np.uint64)
        lik = np.zeros((y.size, self.M)) if want_lik else None
        check(lib().smc_ibis_window(self._h, _d(y), y.size, _d(lik), rec.ctypes.data_as(_u64p)))
        return rec, lik

    def commit(self, j):
        check(lib().smc_ibis_commit(self._h, int(j)))

    def filter(self, y):
        y = np.ascontiguousarray(y, dtype=np.float64)
        check(lib().smc_ibis_filter(self._h, _d(y), y.size))

    def permute(self, a):
        a = np.ascontiguousarray(a, dtype=np.int32)
        assert a.size == self.M
        check(lib().smc_ibis_permute(self._h, a.ctypes.data_as(_i32p)))

    def set_logw(self, logw):
        logw = np.ascontiguousarray(logw, dtype=np.float64)
        assert logw.size == self.M
        check(lib().smc_ibis_set_logw(self._h, _d(logw)))

    def window_ess(self, y, ess_min):
        """window(y) with the walk's integers reduced on the device: (ess [j], j) of host_outer_walk on its records, which stay
        on the device (smc_ibis_window_ess); follow with commit(j)"""
        y = np.ascontiguousarray(y, dtype=np.float64)
        ess = np.zeros(y.size)
        j = C.c_int()
        check(lib().smc_ibis_window_ess(self._h, _d(y), y.size, float(ess_min), _d(ess), C.byref(j)))
        return ess[:j.value], j.value

    def resample(self, seed, want_a=False):
        """resample!(ibis) on the device: the ancestors of host_outer_resample(logw, M, seed) and their gather
        (smc_ibis_resample) -> the ancestors [M] when asked for, else None"""
        a = np.empty(self.M, dtype=np.int32) if want_a else None
        check(lib().smc_ibis_resample(self._h, int(seed), a.ctypes.data_as(_i32p) if want_a else None))
        return a

    def theta_moments(self, weighted=False):
        """(mean [d], cov [d][d]) of the committed theta cloud, reduced on the device (smc_ibis_theta_moments)"""
        mean, cov = np.zeros(self.d), np.zeros((self.d, self.d))
        check(lib().smc_ibis_theta_moments(self._h, int(bool(weighted)), _d(mean), _d(cov)))
        return mean, cov

    def theta_quantiles(self, p):
        """out [d][np]: the weighted quantiles of every coordinate of the committed theta cloud at the levels p, selected on
        the device (smc_ibis_theta_quantiles)"""
        p = np.ascontiguousarray(p, dtype=np.float64).reshape(-1)
        out = np.zeros((self.d, p.size))
        check(lib().smc_ibis_theta_quantiles(self._h, _d(p), p.size, _d(out)))
        return out

    def theta_histogram(self, component, lo, hi, nbins):
        """(counts [nbins + 3] uint64 = under | bins | over | nan, W) of one coordinate of the committed theta cloud, binned on
        the device (smc_ibis_theta_histogram)"""
        counts = np.zeros(max(int(nbins), 0) + 3, dtype=np.uint64)
        W = C.c_uint64()
        check(lib().smc_ibis_theta_histogram(self._h, int(component), float(lo), float(hi), int(nbins), counts.ctypes.data_as(_u64p), C.byref(W)))
        return counts, W.value

    def get_moved(self):
        """the moved mask [M] of the last rejuvenate (smc_ibis_get_moved)"""
        moved = np.zeros(self.M, dtype=np.uint8)
        check(lib().smc_ibis_get_moved(self._h, moved.ctypes.data_as(C.POINTER(C.c_uint8))))
        return moved.astype(bool)

    def rejuvenate(self, y, xi, chol, scales, move_seed, want_moved=True):
        """rejuvenate!(ibis, y, xi) in one launch -> (number of particles that moved, moved mask [M] or None)"""
        y = np.ascontiguousarray(y, dtype=np.float64)
        chol = np.ascontiguousarray(chol, dtype=np.float64).reshape(self.d, self.d)
        scales = np.ascontiguousarray(scales, dtype=np.float64)
        n = C.c_int64()
        moved = np.zeros(self.M, dtype=np.uint8) if want_moved else None
        check(lib().smc_ibis_rejuvenate(self._h, _d(y), y.size, float(xi), _d(chol), _d(scales), scales.size, int(move_seed), C.byref(n),
                                        moved.ctypes.data_as(C.POINTER(C.c_uint8)) if want_moved else None))
        return int(n.value), (moved.astype(bool) if want_moved else None)

    def get(self, theta=False, x=False, S=False, logZ=False, logw=False):
        """the requested arrays from the device, as a dict"""
        out = {}
        if theta:
            out["theta"] = np.zeros((self.M, self.d))
        for name, want, n in (("x", x, self.nx), ("S", S, self.nS), ("logZ", logZ, 1), ("logw", logw, 1)):
            if want:
                out[name] = np.zeros(self.M) if n == 1 else np.zeros((self.M, n))
        check(lib().smc_ibis_get(self._h, _d(out.get("theta")), _d(out.get("x")), _d(out.get("S")), _d(out.get("logZ")), _d(out.get("logw"))))
        return out

    def summary(self, ahead=0):
        """(y, Sigma, between, xbar, Sbar, between_x, K, D) of the committed cloud, reduced on the device (smc_ibis_summary)"""
        out = np.zeros(8)
        check(lib().smc_ibis_summary(self._h, int(ahead), _d(out)))
        return out

    def smooth(self, y, states=False):
        """the RTS smoother of the committed cloud over y (smc_ibis_smooth): out [T][8], the rows of summary() per period for the
        smoothed state; with states also xs, Ps [T][M] per particle.  The handle is not changed."""
        y = np.ascontiguousarray(y, dtype=np.float64).ravel()
        out = np.zeros((y.size, 8))
        xs, Ps = (np.zeros((y.size, self.M)), np.zeros((y.size, self.M))) if states else (None, None)
        check(lib().smc_ibis_smooth(self._h, _d(y), y.size, _d(out), _d(xs), _d(Ps)))
        return (out, xs, Ps) if states else out

    def sample_paths(self, y, which, path_seed):
        """paths [T][Mp] from p(x_1:T | y_1:T), path p under the row of parameter particle which[p] (smc_ibis_sample_paths)"""
        y = np.ascontiguousarray(y, dtype=np.float64).ravel()
        which = np.ascontiguousarray(which, dtype=np.int32).ravel()
        paths = np.zeros((y.size, which.size))
        check(lib().smc_ibis_sample_paths(self._h, _d(y), y.size, which.size, int(path_seed), which.ctypes.data_as(_i32p), _d(paths)))
        return paths

    def last_elapsed_ms(self):
        """device-event time of the kernels of the last smooth / sample_paths call (smc_ibis_last_elapsed_ms)"""
        ms = C.c_double()
        check(lib().smc_ibis_last_elapsed_ms(self._h, C.byref(ms)))
        return ms.value

    def set_summaries(self, on, ahead=0):
        """record the row of summaries after every step of the windows that follow (smc_ibis_set_summaries)"""
        check(lib().smc_ibis_set_summaries(self._h, int(bool(on)), int(ahead)))

    def get_summaries(self, j):
        """rows [j][8] of the first j steps of the last recorded window"""
        out = np.zeros((int(j), 8))
        check(lib().smc_ibis_get_summaries(self._h, int(j), _d(out)))
        return out
