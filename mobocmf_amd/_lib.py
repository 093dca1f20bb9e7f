"""ctypes binding of the C-ABI in include/mobocmf_hip.h (libmobocmf_hip.so, built by csrc/build.sh).

The product path has NO CPU fallback: if the shared library is missing or the device is not a
gfx950, every compute entry point raises.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MOBOCMF_HIP_LIB") or os.path.join(_HERE, "csrc", "libmobocmf_hip.so")   # override: A/B builds

OK, BAD_ARG, WORKSPACE_TOO_SMALL, HIP_ERROR, NOT_PD, BAD_ARCH = range(6)
_ERR = {1: "MOBOCMF_BAD_ARG", 2: "MOBOCMF_WORKSPACE_TOO_SMALL", 3: "MOBOCMF_HIP_ERROR", 4: "MOBOCMF_NOT_PD",
        5: "MOBOCMF_BAD_ARCH"}


class Tuning(ctypes.Structure):
    """mobocmf_tuning of include/mobocmf_hip.h: the kernel-selection knobs that travel with a call (NULL = defaults)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("small_gemm_max", ctypes.c_int32), ("small_panel_max", ctypes.c_int32),
                ("tile_rows", ctypes.c_int32), ("pair_mode", ctypes.c_int32), ("mid_gemm_max", ctypes.c_int32),
                ("mid_gemm_waves", ctypes.c_int32), ("syrk_workgroups", ctypes.c_int32), ("sparse_backward", ctypes.c_int32),
                ("potrf_cols", ctypes.c_int32)]
    KNOBS = tuple(n for n, _ in _fields_[1:])

    def copy(self):
        t = Tuning()
        ctypes.memmove(ctypes.byref(t), ctypes.byref(self), ctypes.sizeof(Tuning))
        return t


PROBE_EVENTS = 11      # MOBOCMF_PROBE_EVENTS


class LayerDesc(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int32), ("d", ctypes.c_int32), ("M", ctypes.c_int32), ("xdiv", ctypes.c_int32),
                ("Np", ctypes.c_int64), ("branch", ctypes.c_int32), ("want_dx", ctypes.c_int32),
                ("jitter", ctypes.c_double), ("min_var", ctypes.c_double), ("params_const", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("tuning", ctypes.POINTER(Tuning)), ("probe_events", ctypes.c_void_p)]


TINY_MAX_LAYERS, TINY_MAX_M, TINY_MAX_D = 3, 32, 8      # MOBOCMF_TINY_MAX_* of include/mobocmf_hip.h
COOP_MAX_M = 128                                         # MOBOCMF_COOP_MAX_M
FROZEN_MAX_M = 512                                       # MOBOCMF_FROZEN_MAX_M
FROZEN_SPLIT_MAX_M = 1024                                # MOBOCMF_FROZEN_SPLIT_MAX_M
# MOBOCMF_STEP_*: do_update of mobocmf_tiny_elbo_step / mobocmf_coop_elbo_step
STEP_GRADIENTS, STEP_UPDATE, STEP_FORWARD, STEP_INPUT_GRADIENTS, STEP_COUPLED = range(5)
STEP_CHAIN_VALID = 16                                    # MOBOCMF_STEP_CHAIN_VALID


class TinyModel(ctypes.Structure):
    """mobocmf_tiny_model: one small surrogate of mobocmf_tiny_elbo_step (the kernel reads the array from DEVICE memory)."""
    _L = TINY_MAX_LAYERS
    _fields_ = [("L", ctypes.c_int32), ("M", ctypes.c_int32), ("d", ctypes.c_int32), ("S", ctypes.c_int32),
                ("N", ctypes.c_int32), ("rows", ctypes.c_int32 * _L), ("trainable", ctypes.c_uint32 * _L),
                ("branch", ctypes.c_int32),
                ("x", ctypes.c_void_p), ("y", ctypes.c_void_p), ("fid", ctypes.c_void_p), ("Zx", ctypes.c_void_p),
                ("raw", (ctypes.c_void_p * 7) * _L), ("m", ctypes.c_void_p * _L), ("L_S", ctypes.c_void_p * _L),
                ("raw_noise", ctypes.c_void_p * _L), ("noise_lo", ctypes.c_double * _L), ("noise_hi", ctypes.c_double * _L),
                ("rng", ctypes.c_void_p * _L), ("eps", ctypes.c_void_p * _L),
                ("adam_m", ctypes.c_void_p), ("adam_v", ctypes.c_void_p), ("steps_done", ctypes.c_void_p),
                ("work", ctypes.c_void_p), ("grad", ctypes.c_void_p), ("out", ctypes.c_void_p), ("info", ctypes.c_void_p),
                ("kl_scale", ctypes.c_double), ("jitter", ctypes.c_double),
                ("row_weight", ctypes.c_void_p), ("seed_gmean", ctypes.c_void_p), ("seed_gvar", ctypes.c_void_p),
                ("seed_scale", ctypes.c_double), ("top_mean", ctypes.c_void_p), ("top_var", ctypes.c_void_p),
                ("xrng", ctypes.c_void_p), ("rand_row0", ctypes.c_int32), ("rand_rows", ctypes.c_int32),
                ("coupling", ctypes.c_void_p), ("role", ctypes.c_int32), ("role_index", ctypes.c_int32)]


class TinyCoupling(ctypes.Structure):
    """mobocmf_tiny_coupling: the theta / omega factors over the models of one mode-4 launch (device-resident)."""
    _fields_ = [("n_obj", ctypes.c_int32), ("n_con", ctypes.c_int32), ("P", ctypes.c_int32), ("T", ctypes.c_int32),
                ("obj_model", ctypes.c_int32 * 8), ("con_model", ctypes.c_int32 * 8),
                ("front", ctypes.c_void_p), ("thresholds", ctypes.c_void_p),
                ("log_eps", ctypes.c_double), ("log_1m_eps", ctypes.c_double), ("losses", ctypes.c_void_p),
                ("barrier", ctypes.c_void_p), ("status", ctypes.c_void_p), ("n_models", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


class FrozenPredictModel(ctypes.Structure):
    """mobocmf_frozen_predict_model: one surrogate of mobocmf_frozen_predict[_split] (the kernel reads the array from DEVICE memory)."""
    _L = TINY_MAX_LAYERS
    _fields_ = [("L", ctypes.c_int32), ("M", ctypes.c_int32), ("d", ctypes.c_int32), ("S", ctypes.c_int32),
                ("T", ctypes.c_int32), ("kind", ctypes.c_int32 * _L),
                ("chain", ctypes.c_void_p * _L), ("Zx", ctypes.c_void_p * _L), ("zf", ctypes.c_void_p * _L),
                ("hyp", ctypes.c_void_p * _L), ("samples", ctypes.c_void_p * _L),
                ("x", ctypes.c_void_p), ("top_mean", ctypes.c_void_p), ("top_var", ctypes.c_void_p),
                ("seed_gmean", ctypes.c_void_p), ("seed_gvar", ctypes.c_void_p), ("grad", ctypes.c_void_p),
                ("work", ctypes.c_void_p)]


EXACT_PREDICT_MAX_N, EXACT_PREDICT_MAX_LEVELS = 512, 8      # MOBOCMF_EXACT_PREDICT_MAX_N / MOBOCMF_EXACT_PREDICT_MAX_LEVELS


class ExactPredictModel(ctypes.Structure):
    """mobocmf_exact_predict_model: one exact-GP surrogate of mobocmf_exact_predict (the kernel reads the array from DEVICE memory)."""
    _fields_ = [("n", ctypes.c_int32), ("d", ctypes.c_int32), ("T", ctypes.c_int32), ("n_levels", ctypes.c_int32),
                ("level", ctypes.c_int32), ("reserved", ctypes.c_int32), ("ld", ctypes.c_int64),
                ("xtr", ctypes.c_void_p), ("lev", ctypes.c_void_p), ("sig", ctypes.c_void_p), ("ntab", ctypes.c_void_p),
                ("hyp_s", ctypes.c_void_p), ("hyp_n", ctypes.c_void_p), ("Linv", ctypes.c_void_p), ("a", ctypes.c_void_p),
                ("kss", ctypes.c_double),
                ("x", ctypes.c_void_p), ("top_mean", ctypes.c_void_p), ("top_var", ctypes.c_void_p),
                ("seed_gmean", ctypes.c_void_p), ("seed_gvar", ctypes.c_void_p), ("grad", ctypes.c_void_p),
                ("work", ctypes.c_void_p)]


# MOBOCMF_EXACT_FIT_*: limits, the positions of the sums in the slab, parameter slots, constraint kinds, modes, words
EXACT_FIT_MAX_N, EXACT_FIT_MAX_LEVELS, EXACT_FIT_MAX_MODELS, EXACT_FIT_STRIP, EXACT_FIT_SUMS = 512, 8, 64, 16, 83
EXACT_FIT_KERNEL_MIN, EXACT_FIT_KERNEL_LIN = 0, 1
EXACT_FIT_IDENTITY, EXACT_FIT_SOFTPLUS, EXACT_FIT_SIGMOID = 0, 1, 2
EXACT_FIT_PARAMS = 6
EXACT_FIT_P_NOISE, EXACT_FIT_P_OS_S, EXACT_FIT_P_LS_S, EXACT_FIT_P_OS_N, EXACT_FIT_P_LS_N, EXACT_FIT_P_RHO = range(6)
EXACT_FIT_STEP, EXACT_FIT_FINISH = 0, 1
EXACT_FIT_WORDS = 8
(EXACT_FIT_W_IT, EXACT_FIT_W_STOPPED_AT, EXACT_FIT_W_BEST_IT, EXACT_FIT_W_RESTORED, EXACT_FIT_W_ABANDONED,
 EXACT_FIT_W_FINAL_INFO) = range(6)
EXACT_FIT_S_OS_S, EXACT_FIT_S_LS_S, EXACT_FIT_S_OS_N, EXACT_FIT_S_LS_N, EXACT_FIT_S_TAU, EXACT_FIT_S_SIG, EXACT_FIT_S_NTAB = \
    0, 1, 33, 34, 66, 67, 75


class ExactFitParam(ctypes.Structure):
    """mobocmf_exact_fit_param: one raw parameter tensor of a model of the device fit, its constraint and its optimiser state."""
    _fields_ = [("raw", ctypes.c_void_p), ("best", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p), ("exp_avg_sq", ctypes.c_void_p),
                ("grad", ctypes.c_void_p), ("numel", ctypes.c_int32), ("kind", ctypes.c_int32), ("lo", ctypes.c_double),
                ("hi", ctypes.c_double)]


class ExactFitModel(ctypes.Structure):
    """mobocmf_exact_fit_model: one exact-GP surrogate of the mobocmf_exact_fit_* launches (read from DEVICE memory)."""
    _fields_ = [("n", ctypes.c_int32), ("d", ctypes.c_int32), ("n_levels", ctypes.c_int32), ("kernel", ctypes.c_int32),
                ("cap", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("x", ctypes.c_void_p), ("lev", ctypes.c_void_p), ("y", ctypes.c_void_p),
                ("params", ExactFitParam * EXACT_FIT_PARAMS),
                ("Linv", ctypes.c_void_p), ("a", ctypes.c_void_p), ("mll", ctypes.c_void_p), ("info", ctypes.c_void_p),
                ("losses", ctypes.c_void_p), ("stats", ctypes.c_void_p), ("words", ctypes.c_void_p), ("work", ctypes.c_void_p)]


# MOBOCMF_EXACT_SAMPLE_*: limits and the feature chunk of the gram launch
EXACT_SAMPLE_MAX_N, EXACT_SAMPLE_MAX_LEVELS, EXACT_SAMPLE_MAX_F, EXACT_SAMPLE_MAX_PROBLEMS, EXACT_SAMPLE_CHUNK = 512, 8, 65536, 64, 16


class ExactSampleProblem(ctypes.Structure):
    """mobocmf_exact_sample_problem: one (model, sample) of the mobocmf_exact_sample_* launches (read from DEVICE memory)."""
    _fields_ = [("n", ctypes.c_int32), ("d", ctypes.c_int32), ("n_levels", ctypes.c_int32), ("F", ctypes.c_int32),
                ("n_out", ctypes.c_int32), ("reserved", ctypes.c_int32), ("out_level", ctypes.c_int32 * EXACT_SAMPLE_MAX_LEVELS),
                ("x", ctypes.c_void_p), ("lev", ctypes.c_void_p), ("y", ctypes.c_void_p), ("sig", ctypes.c_void_p),
                ("ntab", ctypes.c_void_p), ("sqd", ctypes.c_void_p), ("scal", ctypes.c_void_p),
                ("W_sig", ctypes.c_void_p), ("b_sig", ctypes.c_void_p), ("W_noi", ctypes.c_void_p), ("b_noi", ctypes.c_void_p),
                ("theta0", ctypes.c_void_p), ("e", ctypes.c_void_p), ("G", ctypes.c_void_p), ("r", ctypes.c_void_p),
                ("Linv", ctypes.c_void_p), ("a", ctypes.c_void_p), ("info", ctypes.c_void_p), ("w", ctypes.c_void_p),
                ("theta", ctypes.c_void_p), ("chain", ctypes.c_void_p), ("info_out", ctypes.c_void_p)]


class NatgradSmallLayer(ctypes.Structure):
    """mobocmf_natgrad_small_layer: one layer of mobocmf_natgrad_small_step (the kernel reads the array from DEVICE memory)."""
    _fields_ = [("M", ctypes.c_int32), ("n_guard_info", ctypes.c_int32), ("m", ctypes.c_void_p), ("L_S", ctypes.c_void_p),
                ("g_m", ctypes.c_void_p), ("g_LS", ctypes.c_void_p), ("scale", ctypes.c_double),
                ("step_count", ctypes.c_void_p), ("skipped", ctypes.c_void_p), ("info", ctypes.c_void_p),
                ("guard_info", ctypes.c_void_p), ("guard_status", ctypes.c_void_p), ("guard_loss", ctypes.c_void_p),
                ("work", ctypes.c_void_p)]


RFF_MAX_LAYERS = 3        # MOBOCMF_RFF_MAX_LAYERS


class RffLayerDesc(ctypes.Structure):
    """mobocmf_rff_layer_desc: one layer of one chain sample of mobocmf_rff_eval_chains (the kernel reads the table from
    DEVICE memory)."""
    _fields_ = [("kind", ctypes.c_int32), ("F", ctypes.c_int32), ("W1", ctypes.c_int64), ("b1", ctypes.c_int64),
                ("theta", ctypes.c_int64), ("Wf", ctypes.c_int64), ("W2", ctypes.c_int64), ("b2", ctypes.c_int64),
                ("s0", ctypes.c_double), ("s1", ctypes.c_double), ("s2", ctypes.c_double)]


REFINE_MAX_PROBLEMS, REFINE_MAX_CON = 64, 32      # MOBOCMF_REFINE_MAX_PROBLEMS / MOBOCMF_REFINE_MAX_CON
REFINE_STATUS = {0: "refinement moved away from the best start", 1: "the best start itself is returned",
                 2: "no start has a feasible result"}            # status of mobocmf_rff_refine


class RffRefineOptions(ctypes.Structure):
    """mobocmf_rff_refine_options: the settings of mobocmf_rff_refine, passed with the call (NULL = defaults)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("outer", ctypes.c_int32), ("inner", ctypes.c_int32),
                ("backtracks", ctypes.c_int32), ("restore", ctypes.c_int32), ("recentre", ctypes.c_int32),
                ("step0", ctypes.c_double),
                ("step_shrink", ctypes.c_double), ("step_grow", ctypes.c_double), ("rho0", ctypes.c_double),
                ("rho_growth", ctypes.c_double), ("armijo", ctypes.c_double), ("restore_margin", ctypes.c_double)]
    KNOBS = tuple(n for n, _ in _fields_[1:])


NSGA_MAX_ROWS = 1024      # MOBOCMF_NSGA_MAX_ROWS


class NsgaOptions(ctypes.Structure):
    """mobocmf_nsga_options: the settings of mobocmf_nsga_vary, passed with the call (NULL = defaults)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("eta_c", ctypes.c_double),
                ("p_c", ctypes.c_double), ("eta_m", ctypes.c_double), ("p_m", ctypes.c_double)]
    KNOBS = tuple(n for n, _ in _fields_[2:])


class MobocmfError(RuntimeError):
    pass


_P = ctypes.c_void_p
_I64 = ctypes.c_int64
_I32 = ctypes.c_int32
_D = ctypes.c_double
_SZ = ctypes.c_size_t

# name -> argtypes   (every symbol include/mobocmf_hip.h declares)
SYMBOLS = {
    "mobocmf_version": [],
    "mobocmf_device_arch_ok": [],
    "mobocmf_layer_workspace_bytes": [ctypes.POINTER(LayerDesc), ctypes.POINTER(_SZ), ctypes.POINTER(_SZ)],
    "mobocmf_layer_forward": [ctypes.POINTER(LayerDesc)] + [_P] * 11 + [_P, _SZ, _P, _SZ, _P],
    "mobocmf_layer_backward": [ctypes.POINTER(LayerDesc)] + [_P] * 16 + [_P, _SZ, _P, _SZ, _P],
    "mobocmf_chain_block_bytes": [ctypes.POINTER(LayerDesc), ctypes.POINTER(_SZ), ctypes.POINTER(_SZ)],
    "mobocmf_panel_workspace_bytes": [ctypes.POINTER(LayerDesc), ctypes.POINTER(_SZ), ctypes.POINTER(_SZ)],
    "mobocmf_layers_chain_forward": [_I32] + [_P] * 8 + [_P, _SZ, _SZ, _P],
    "mobocmf_layers_chain_backward": [_I32] + [_P] * 10 + [_P, _SZ, _SZ, _P],
    "mobocmf_layer_panel_forward": [ctypes.POINTER(LayerDesc)] + [_P] * 7 + [_P, _SZ, _P, _SZ, _P, _SZ, _P],
    "mobocmf_layer_panel_backward": [ctypes.POINTER(LayerDesc)] + [_P] * 11 + [_P, _SZ, _P, _SZ, _P, _SZ, _P],
    "mobocmf_predictive_covariance_workspace_bytes": [ctypes.POINTER(LayerDesc), ctypes.POINTER(_SZ)],
    "mobocmf_predictive_covariance": [ctypes.POINTER(LayerDesc), _P, _P, _P, _P, _P, _P, _I64, _P, _SZ, _P, _SZ, _P],
    "mobocmf_propagate_forward": [_P, _P, _P, _P, _I64, _I32, _P],
    "mobocmf_propagate_rng_forward": [_P, _P, _P, _P, _P, _I64, _I32, _P],
    "mobocmf_propagate_backward": [_P, _P, _P, _P, _P, _I64, _I32, _P],
    "mobocmf_propagate_backward_prefix": [_P, _P, _P, _P, _P, _I64, _I32, _I64, _P, _P, _P],
    "mobocmf_elbo_data_forward": [_P, _P, _P, _P, _P, _D, _I64, _I32, _P, _P, _SZ, _P],
    "mobocmf_elbo_data_backward": [_P, _P, _P, _P, _P, _D, _I64, _I32, _P, _P, _P, _P, _P, _SZ, _P],
    "mobocmf_elbo_data_interval_forward": [_P, _P, _P, _P, _P, _D, _D, _D, _I64, _I32, _P, _P, _SZ, _P],
    "mobocmf_elbo_data_interval_backward": [_P, _P, _P, _P, _P, _D, _D, _D, _I64, _I32, _P, _P, _P, _P, _P, _SZ, _P],
    "mobocmf_elbo_forward": [_I32, _P, _P, _P, _P, _P, _P, _P, _P, _I64, _P, _I32, _P, _D, _P, _P, _SZ, _P],
    "mobocmf_elbo_backward": [_I32, _P, _P, _P, _P, _P, _P, _P, _P, _I64, _P, _D, _P, _P, _P, _P, _P, _P, _P, _SZ, _P],
    "mobocmf_acq_moments_forward": [_P, _P, _P, _P, _I64, _I32, _P],
    "mobocmf_acq_moments_backward": [_P, _P, _P, _P, _P, _I64, _I32, _P],
    "mobocmf_jes_forward": [_P, _P, _P, _I64, _P],
    "mobocmf_shortcut_var_forward": [_P, _I32, _D, _P, _P],
    "mobocmf_shortcut_var_backward": [_P, _P, _P, _I32, _D, _P, _P],
    "mobocmf_elbo_combine_forward": [_I32, _P, _I32, _P, _D, _P, _P],
    "mobocmf_elbo_combine_backward": [_P, _P, _D, _P, _P],
    "mobocmf_adam_multi": [_I32, _P, _P, _P, _P, _P, _D, _D, _D, _D, _P, _P],
    "mobocmf_adam_step": [_P, _P, _P, _P, _P, _I64, _D, _D, _D, _D, _I64, _P],
    "mobocmf_tuning_init": [ctypes.POINTER(Tuning)],
    "mobocmf_gemm_f64": [_I32, _I32, _I32, _I64, _I64, _P, _I64, _P, _I64, _P, _I64, _D, _I32, ctypes.POINTER(Tuning), _P],
    "mobocmf_gemm_f64_epilogue": [_I32, _I32, _I32, _I64, _I64, _P, _I64, _P, _I64, _P, _I64, _D, _I32] + [_P] * 8 +
                                 [_P, ctypes.POINTER(Tuning), _P],
    "mobocmf_mf_kernel_combine": [_I64, _I64, _P, _P, _I64, _P, _P, _P, _P, _P, _D, _P, _I64, _I64, _I64, _P],
    "mobocmf_exact_gp_workspace_bytes": [_I32, _I64, ctypes.POINTER(_SZ), ctypes.POINTER(_SZ)],
    "mobocmf_exact_gp_factor": [_I32, _P, _I64, _P, _P, _P, _P, _SZ, _P, _SZ, ctypes.POINTER(Tuning), _P],
    "mobocmf_exact_gp_predict": [_I32, _I64, _P, _I64, _P, _P, _P, _P, _SZ, _P, _SZ, ctypes.POINTER(Tuning), _P],
    "mobocmf_gemm_colstat_rows": [_I32, _I32, _I64, _I64, ctypes.POINTER(Tuning), ctypes.POINTER(_I32)],
    "mobocmf_syrk_workspace_bytes": [_I32, _I64, ctypes.POINTER(Tuning), ctypes.POINTER(_SZ)],
    "mobocmf_syrk_weighted_f64": [_I32, _I64, _P, _I64, _P, _P, _P, _I64, _P, ctypes.POINTER(Tuning), _P],
    "mobocmf_softplus_pack": [_I32, _P, _P, _P, _P],
    "mobocmf_softplus_pack_backward": [_I32, _P, _P, _P, _P, _P],
    "mobocmf_softplus_pack_backward_v": [_I32, _P, _P, _P, _P, _P],
    "mobocmf_cond_factors_forward": [_I32, _I32, _I32, _I32, _P, _P, _P, _P, _P, _P, _D, _D, _P, _P, _P, _P, _P, _P],
    "mobocmf_scale_segments": [_I32, _P, _P, _P, _P, _P, _P],
    "mobocmf_gather_segments": [_I32, _P, _P, _P, _P],
    "mobocmf_scalar_combine": [_I32, _P, _P, _P, _P],
    "mobocmf_tiny_flat_len": [ctypes.POINTER(TinyModel), ctypes.POINTER(_I64)],
    "mobocmf_tiny_work_bytes": [ctypes.POINTER(TinyModel), ctypes.POINTER(_SZ)],
    "mobocmf_tiny_elbo_step": [_P, _P, _I32, _D, _D, _D, _D, _I32, _P],
    "mobocmf_coop_work_bytes": [ctypes.POINTER(TinyModel), ctypes.POINTER(_SZ)],
    "mobocmf_coop_elbo_step": [_P, _P, _I32, _I32, _P, _D, _D, _D, _D, _I32, ctypes.POINTER(_I32), _P],
    "mobocmf_rff_eval": [_I32, _I32, _I32, _I64] + [_P] * 8 + [_D, _D, _D, _P, _P],
    "mobocmf_rff_eval_chains": [_I32, _I32, _I64, _P, _P, _I64, _P, _P, _P],
    "mobocmf_rff_feasibility": [_I32, _I64, _P, _I64, _P, _P, _P, _P],
    "mobocmf_rff_chains_value_grad": [_I32, _I32, _I64, _P, _P, _I64, _P, _P, _P, _P],
    "mobocmf_rff_refine_options_init": [ctypes.POINTER(RffRefineOptions)],
    "mobocmf_rff_refine": [_I32, _I32, _I32, _I32, _P, _P, _P, _I32, _P, _P, _P, _P, _I64, _P,
                           ctypes.POINTER(RffRefineOptions)] + [_P] * 7 + [_P],
    "mobocmf_pareto_mask": [_I32, _I64, _P, _I64, _I32, _P, _P, _I64, _P, _D, _P, _P, _P],
    "mobocmf_hypervolume_workspace_bytes": [_I32, _I64, ctypes.POINTER(_SZ)],
    "mobocmf_hypervolume": [_I32, _I64, _P, _I64, _P, ctypes.POINTER(_D), _P, _SZ, _P],
    "mobocmf_nsga_options_init": [ctypes.POINTER(NsgaOptions)],
    "mobocmf_nsga_survive": [_I32, _I32, _I32, _I32, _P, _P, _I64, _P, _P, _P, _I64, _P, _P, _P, _P, _P, _P],
    "mobocmf_nsga_vary": [_I32, _I32, _P, _P, _P, ctypes.c_uint64, _P, ctypes.POINTER(NsgaOptions), _P, _P, _P],
    "mobocmf_recommend_scores": [_P, _I32, _I32, _I32, _I32, _P, _D, _D, _P, _I64, _P, _P],
    "mobocmf_select_inducing_workspace_bytes": [_I64, _I32, ctypes.POINTER(_SZ)],
    "mobocmf_select_inducing": [_I64, _I32, _P, _P, _I32, _D, _I32, _P, _P, _P, _P, _P, _P, _SZ, _P],
    "mobocmf_minibatch_permutation_host": [_I64, _I64, _I64, _P],
    "mobocmf_minibatch_indices": [_I64, _I64, _I32, _P, _I32, _I64, _P, _P, _P, _P],
    "mobocmf_minibatch_gather": [_I64, _I32, _I64] + [_P] * 9,
    "mobocmf_minibatch_accumulate": [_I64, _I64, _P, _P, _P, _P, _P],
    "mobocmf_gram_forward": [_I32, _I32, _P, _P, _I64, _P, _P, _I64, _P, _P, _I64, _P],
    "mobocmf_gram_forward_rep": [_I32, _I32, _P, _P, _I64, _P, _P, _I64, _I32, _P, _P, _I64, _P, _P],
    "mobocmf_gram_backward_workspace_bytes": [_I32, _I32, _I64, _I64, _I32, _I32, ctypes.POINTER(_SZ), ctypes.POINTER(_I32)],
    "mobocmf_gram_backward": [_I32, _I32, _P, _P, _I64, _P, _P, _I64, _I32, _P, _P, _I64, _P, _P, _P, _P, _P, _P, _P, _SZ, _P],
    "mobocmf_gram_backward_rows_workspace_bytes": [_I32, _I32, _I64, _I64, _I32, ctypes.POINTER(_SZ), ctypes.POINTER(_I32)],
    "mobocmf_gram_backward_rows": [_I32, _I32, _P, _P, _I64, _P, _P, _I64, _I32, _P, _P, _I64, _P, _I32, _P, _P, _SZ, _P],
    "mobocmf_inducing_grad_workspace_bytes": [ctypes.POINTER(LayerDesc), ctypes.POINTER(_SZ), ctypes.POINTER(_SZ)],
    "mobocmf_layer_backward_z": [ctypes.POINTER(LayerDesc)] + [_P] * 17 + [_P, _SZ, _P, _SZ, _P, _SZ, _P],
    "mobocmf_layer_panel_backward_z": [ctypes.POINTER(LayerDesc)] + [_P] * 12 + [_P, _SZ, _P, _SZ, _P, _SZ, _P, _SZ, _P],
    "mobocmf_layers_chain_backward_z": [_I32] + [_P] * 11 + [_P, _SZ, _SZ, _P, _SZ, _P],
    "mobocmf_check_info": [_P, ctypes.POINTER(_I32), _P],
    "mobocmf_natgrad_workspace_bytes": [_I32, _I32, ctypes.POINTER(_SZ)],
    "mobocmf_natgrad_step": [_I32, _I32, _P, _P, _P, _P, _D, _D, _I32, _D, _P, _P, _P, _P, _SZ, ctypes.POINTER(Tuning), _P],
    "mobocmf_natgrad_small_work_bytes": [_I32, ctypes.POINTER(_SZ)],
    "mobocmf_natgrad_small_step": [_P, _P, _I32, _D, _D, _I32, _P],
    "mobocmf_jes_group_forward": [_P, _P, _I32, _I32, _I32, _P, _I32, _P, _I32, _P, _I32, _P, _P, _P],
    "mobocmf_jes_mc_group_forward": [_P, _P, _I32, _I32, _I32, _I32, _P, _I32, _P, _I32, _P, _I32, _P, _P, _P],
    "mobocmf_jes_mc_box_forward": [_P, _P, _I32, _I32, _I32, _I32, _P, _P, _I32, _I32, _P, _I32, _P, _I32, _P, _P, _P],
    "mobocmf_ascent_adam_step": [_P, _P, _I32, _I32, _I32, _P, _P, _P, _P, _D, _D, _D, _D, _P, _P],
    "mobocmf_select_topk": [_P, _I32, _I32, _P, _I32, _P, _P, _P, _P],
    "mobocmf_frozen_predict_work_bytes": [ctypes.POINTER(FrozenPredictModel), _I32, ctypes.POINTER(_SZ)],
    "mobocmf_frozen_predict": [_P, _P, _I32, _I32, _P],
    "mobocmf_frozen_predict_split_work_bytes": [ctypes.POINTER(FrozenPredictModel), _I32, ctypes.POINTER(_SZ)],
    "mobocmf_frozen_predict_split": [_P, _P, _I32, _I32, _P],
    "mobocmf_exact_predict_work_bytes": [ctypes.POINTER(ExactPredictModel), _I32, ctypes.POINTER(_SZ)],
    "mobocmf_exact_predict": [_P, _P, _I32, _I32, _P],
    "mobocmf_exact_fit_work_bytes": [ctypes.POINTER(ExactFitModel), _I32, ctypes.POINTER(_SZ)],
    "mobocmf_exact_fit_covariance": [_P, _P, _I32, _P],
    "mobocmf_exact_fit_prepare": [_P, _P, _I32, _P],
    "mobocmf_exact_fit_gradient": [_P, _P, _I32, _P],
    "mobocmf_exact_fit_update": [_P, _P, _I32, _I32, _D, _D, _D, _D, _P],
    "mobocmf_mes_group_forward": [_P, _P, _P, _I32, _I32, _I32, _P, _I32, _P, _I32, _P, _I32, _P, _P, _P],
    "mobocmf_exact_sample_gram": [_P, _P, _I32, _P],
    "mobocmf_exact_sample_weights": [_P, _P, _I32, _P],
}
ACQ_MAX_PAIRS, TOPK_MAX_K, TOPK_MAX_N = 32, 64, 4096      # MOBOCMF_ACQ_MAX_PAIRS / MOBOCMF_TOPK_MAX_K / MOBOCMF_TOPK_MAX_N
ACQ_MAX_COLUMNS = 1 << 24                                 # MOBOCMF_ACQ_MAX_COLUMNS
NATGRAD_MAX_M, NATGRAD_MAX_LAYERS = 1024, 4      # MOBOCMF_NATGRAD_MAX_M, layers per mobocmf_natgrad_step call
NATGRAD_SMALL_MAX_M = 128                        # MOBOCMF_NATGRAD_SMALL_MAX_M
MAX_D, MAX_XDIV = 32, 48        # MOBOCMF_MAX_D / MOBOCMF_MAX_XDIV of include/mobocmf_hip.h
PARETO_MAX_K, HV_MAX_K = 16, 5   # MOBOCMF_PARETO_MAX_K / MOBOCMF_HV_MAX_K
HV_MAX_POINTS = {1: 65536, 2: 65536, 3: 65536, 4: 1024, 5: 256}   # the work bound of mobocmf_hypervolume
INDUCING_MAX_POINTS, INDUCING_MAX_ROWS = 4096, 262144             # MOBOCMF_INDUCING_MAX_POINTS / MOBOCMF_INDUCING_MAX_ROWS
INDUCING_ONE_WG_MAX_ROWS = 32768                                  # MOBOCMF_INDUCING_ONE_WG_MAX_ROWS (form 1 beyond it is refused)
INDUCING_INFO = {1: "a non-finite entry of x", 2: "a non-finite or non-positive hyper-parameter"}   # info of mobocmf_select_inducing

MINIBATCH_MAX_ROWS, MINIBATCH_MAX_LEVELS = 2 ** 31, 8              # MOBOCMF_MINIBATCH_MAX_ROWS / MOBOCMF_MINIBATCH_MAX_LEVELS
MINIBATCH_STATUS = {1: "the batch does not have the rows the step was built for (host and device step counts differ)",
                    2: "a negative step count"}                   # status word of mobocmf_minibatch_indices

_lib = None


def load():
    """Loads the shared library (no GPU needed for loading / symbol checks)."""
    global _lib
    if _lib is None:
        import torch  # noqa: F401  -- first: the HIP runtime torch ships must be the one this library binds to
        if not os.path.exists(LIB_PATH):
            raise MobocmfError(f"HIP extension missing: {LIB_PATH} (run mobocmf_amd/csrc/build.sh or "
                               "__graft_entry__.build()); there is no CPU fallback")
        lib = ctypes.CDLL(LIB_PATH)
        for name, argtypes in SYMBOLS.items():
            fn = getattr(lib, name)
            fn.argtypes = argtypes
            fn.restype = ctypes.c_int
        _lib = lib
    return _lib


def check(rc, what):
    if rc != OK:
        raise MobocmfError(f"{what} failed: {_ERR.get(rc, rc)}")


_arch_checked = False


def require_device():
    """Fail loudly unless a gfx950 device is current."""
    global _arch_checked
    lib = load()
    if not _arch_checked:
        import torch
        if not torch.cuda.is_available():
            raise MobocmfError("mobocmf_amd needs an MI355X (gfx950) device: no GPU visible, and there is no CPU fallback")
        if not lib.mobocmf_device_arch_ok():
            raise MobocmfError("mobocmf_amd kernels are built for gfx950 only")
        _arch_checked = True
    return lib
