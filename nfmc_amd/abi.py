"""The hand-written ctypes mirror of include/nfmc_hip.h: its words (NFMC_X here is X), its structs and, in SYMBOLS, its
prototypes.  This module's whole namespace is the mirror -- it imports ctypes alone and loads nothing -- so that
tests/test_host_abi.py can hold every name in it against the header, and a tool can read the ABI without torch.
nfmc_amd/hip.py loads the library and re-exports these names: call sites say `hip.NAME`."""
import ctypes as C

OK, EINVAL, ESHAPE, EALIGN, EUNSUPPORTED, ESCRATCH = 0, -1, -2, -3, -4, -5
POT_QUADRATIC, POT_FUNNEL, POT_GAUSSIAN_MIXTURE, POT_LOGISTIC_REGRESSION, POT_GAUSSIAN_FULL, POT_ROSENBROCK = 0, 1, 2, 3, 4, 5
POT_STOCHASTIC_VOLATILITY = 6
POT_SPARSE_LOGISTIC_REGRESSION = 7
POT_LATTICE_PHI4 = 8
POT_ITEM_RESPONSE = 9
POT_VARYING_EFFECTS = 10
POT_PARTICLES = 11
POT_LATENT_GAUSSIAN = 12
POT_LATENT_GMRF = 13
POT_DIFFUSION_BRIDGE = 14
MIXTURE_MAX_COMPONENTS = 8   # kMixMaxK (csrc/pot_kinds.hpp)
TAG_NOISE, TAG_ACCEPT, TAG_LATENT, TAG_JUMP = 0, 1, 2, 3
CNT_ACCEPTED, CNT_ATTEMPTED, CNT_NONFINITE, CNT_WORDS = 0, 1, 2, 4
MAX_STEPS_PER_CALL = 512
IMH_PARALLEL_MAX_STEPS = 65536

c_fp = C.c_void_p  # all device pointers travel as void*
NFMC_ABI_VERSION = 4   # include/nfmc_hip.h


class NfmcPotential(C.Structure):
    _fields_ = [('kind', C.c_int32), ('n_components', C.c_int32), ('a', c_fp), ('b', c_fp),
                ('a_scalar', C.c_float), ('b_scalar', C.c_float)]


class NfmcRng(C.Structure):
    _fields_ = [('seed', C.c_uint64), ('chain_offset', C.c_uint64), ('step0', C.c_uint32), ('rounds', C.c_uint32),
                ('replay_normals', c_fp), ('replay_uniforms', c_fp)]


class NfmcStats(C.Structure):
    _fields_ = [('sum_x', c_fp), ('sum_x2', c_fp), ('counters', c_fp), ('scratch', c_fp),
                ('scratch_bytes', C.c_int64), ('defer', C.c_int32), ('tail_slot', C.c_int32)]


class NfmcRealNVP(C.Structure):
    _fields_ = [('d', C.c_int32), ('n_coupling', C.c_int32), ('n_hidden', C.c_int32), ('n_hidden_layers', C.c_int32),
                ('min_scale', C.c_float), ('n_bins', C.c_int32),
                ('ea0_log_scale', c_fp), ('ea0_shift', c_fp), ('ea1_log_scale', c_fp), ('ea1_shift', c_fp),
                ('weights', c_fp), ('layer_stride', C.c_int64), ('spline_bound', C.c_float), ('reserved', C.c_int32),
                ('scratch', c_fp), ('scratch_bytes', C.c_int64)]


class NfmcSampleStore(C.Structure):
    _fields_ = [('base', c_fp), ('stride', C.c_int32), ('countdown', C.c_int32), ('ring_rows', C.c_int32), ('row', C.c_int32)]


class NfmcJumpTail(C.Structure):
    _fields_ = [('flow', NfmcRealNVP), ('adjusted', C.c_int32), ('reserved', C.c_int32), ('counters', c_fp),
                ('replay_latent', c_fp), ('replay_uniform', c_fp), ('mask_out', c_fp), ('log_ratio_out', c_fp)]


class NfmcTune(C.Structure):
    _fields_ = [('state', c_fp), ('inv_mass_diag', c_fp), ('tune_step_size', C.c_int32), ('tune_inv_mass_diag', C.c_int32),
                ('every', C.c_int32), ('trajectory', C.c_int32)]


TUNE_STEP_SIZE, TUNE_LOG_SMOOTH, TUNE_ERROR_SUM, TUNE_ITERATION, TUNE_ANCHOR, TUNE_LOG_RAW = 0, 1, 2, 3, 4, 5
TUNE_TARGET, TUNE_KAPPA, TUNE_GAMMA, TUNE_IMD_ADJUSTMENT, TUNE_TICKET, TUNE_WORDS = 6, 7, 8, 9, 10, 12
STAT_TAIL = 4
# NfmcTune.trajectory and the words of the trajectory block behind the tuning state (include/nfmc_hip.h: NFMC_TRAJ_*)
TRAJECTORY_OFF, TRAJECTORY_ADAPT, TRAJECTORY_FROZEN = 0, 1, 2
(TRAJ_LENGTH, TRAJ_LOG_LENGTH, TRAJ_LOG_AVERAGED, TRAJ_V, TRAJ_COUNT, TRAJ_LEARNING_RATE, TRAJ_BETA2, TRAJ_CLIP,
 TRAJ_MAX_LEAPFROG, TRAJ_LEAPFROG_TOTAL, TRAJ_G_HAT, TRAJ_ALPHA_SUM, TRAJ_HISTORY_ROWS, TRAJ_HISTORY_USED) = range(14)
TRAJ_WORDS = 16
# columns of a history row: what the pool ran with, what it measured, and the controller state its update left
(TRAJ_ROW_LENGTH, TRAJ_ROW_STEP_SIZE, TRAJ_ROW_G_HAT, TRAJ_ROW_ALPHA_SUM, TRAJ_ROW_LEAPFROGS, TRAJ_ROW_LOG_LENGTH,
 TRAJ_ROW_V, TRAJ_ROW_LOG_AVERAGED, TRAJ_ROW_NEXT_STEP_SIZE) = range(9)
TRAJ_ROW_WORDS = 9


class NfmcMalaArgs(C.Structure):
    _fields_ = [('x', c_fp), ('n', C.c_int64), ('d', C.c_int32), ('n_steps', C.c_int32),
                ('step_size', C.c_float), ('adjust', C.c_int32), ('inv_mass_diag', c_fp),
                ('pot', NfmcPotential), ('rng', NfmcRng), ('stats', NfmcStats),
                ('samples', NfmcSampleStore), ('masks_out', c_fp), ('log_ratio_out', c_fp), ('jump', C.POINTER(NfmcJumpTail)),
                ('tune', NfmcTune)]


class NfmcHmcArgs(C.Structure):
    _fields_ = [('x', c_fp), ('n', C.c_int64), ('d', C.c_int32), ('n_steps', C.c_int32),
                ('step_size', C.c_float), ('n_leapfrog', C.c_int32), ('adjust', C.c_int32), ('reserved', C.c_int32),
                ('inv_mass_diag', c_fp), ('pot', NfmcPotential), ('rng', NfmcRng), ('stats', NfmcStats),
                ('samples', NfmcSampleStore), ('masks_out', c_fp), ('log_ratio_out', c_fp), ('jump', C.POINTER(NfmcJumpTail)),
                ('tune', NfmcTune)]


class NfmcMclmcTune(C.Structure):
    _fields_ = [('state', c_fp), ('inv_mass_diag', c_fp), ('tune_step_size', C.c_int32),
                ('tune_decoherence_length', C.c_int32), ('tune_inv_mass_diag', C.c_int32), ('every', C.c_int32)]


class NfmcMclmcArgs(C.Structure):
    _fields_ = [('x', c_fp), ('velocity', c_fp), ('n', C.c_int64), ('d', C.c_int32), ('n_steps', C.c_int32),
                ('step_size', C.c_float), ('decoherence_length', C.c_float), ('inv_mass_diag', c_fp),
                ('pot', NfmcPotential), ('rng', NfmcRng), ('stats', NfmcStats), ('samples', NfmcSampleStore),
                ('energy_out', c_fp), ('energy_sums', c_fp), ('tune', NfmcMclmcTune)]


# words of the mclmc tuning state and of its history rows (include/nfmc_hip.h: NFMC_MCLMC_*); the column totals and the
# shift follow the words as in the mala / hmc tuning state (tune_shift_offset), the history follows the shift
(MCLMC_STEP_SIZE, MCLMC_DECOHERENCE_LENGTH, MCLMC_TARGET, MCLMC_IMD_ADJUSTMENT, MCLMC_DECOHERENCE_FACTOR,
 MCLMC_ENERGY_VARIANCE, MCLMC_COUNT, MCLMC_HISTORY_ROWS, MCLMC_HISTORY_USED) = range(9)
MCLMC_WORDS = 12
(MCLMC_ROW_STEP_SIZE, MCLMC_ROW_DECOHERENCE_LENGTH, MCLMC_ROW_ENERGY_VARIANCE, MCLMC_ROW_COUNT, MCLMC_ROW_NEXT_STEP_SIZE,
 MCLMC_ROW_NEXT_DECOHERENCE_LENGTH) = range(6)
MCLMC_ROW_WORDS = 6
TAG_VELOCITY = 4   # Philox stream of the initial velocity of an mclmc run (nfmc_philox_normals_f32)


class NfmcFlowMhArgs(C.Structure):
    _fields_ = [('x', c_fp), ('logq', c_fp), ('n', C.c_int64), ('n_steps', C.c_int32), ('logq_cached', C.c_int32),
                ('adjusted', C.c_int32), ('reserved', C.c_int32), ('flow', NfmcRealNVP), ('pot', NfmcPotential),
                ('rng', NfmcRng), ('stats', NfmcStats), ('samples', NfmcSampleStore), ('masks_out', c_fp),
                ('log_ratio_out', c_fp)]


INNER_MALA, INNER_HMC = 0, 1
JUMP_RUN_MAX_PARTS = 4


class NfmcJumpRun(C.Structure):
    _fields_ = [('inner_kind', C.c_int32), ('n_parts', C.c_int32), ('inner', c_fp), ('jump', C.POINTER(NfmcFlowMhArgs)),
                ('n_outer', C.c_int32), ('n_inner', C.c_int32)]


class NfmcNeutraHmcArgs(C.Structure):
    _fields_ = [('z', c_fp), ('n', C.c_int64), ('n_steps', C.c_int32), ('n_leapfrog', C.c_int32),
                ('step_size', C.c_float), ('adjust', C.c_int32), ('inv_mass_diag', c_fp),
                ('flow', NfmcRealNVP), ('pot', NfmcPotential), ('rng', NfmcRng), ('stats', NfmcStats),
                ('samples', NfmcSampleStore), ('masks_out', c_fp), ('log_ratio_out', c_fp), ('scratch', c_fp),
                ('scratch_bytes', C.c_int64)]


class NfmcNeutraMhArgs(C.Structure):
    _fields_ = [('z', c_fp), ('n', C.c_int64), ('n_steps', C.c_int32), ('adjust', C.c_int32), ('inv_mass_diag', c_fp),
                ('flow', NfmcRealNVP), ('pot', NfmcPotential), ('rng', NfmcRng), ('stats', NfmcStats),
                ('samples', NfmcSampleStore), ('masks_out', c_fp), ('log_ratio_out', c_fp)]


class NfmcFlowLogqGradArgs(C.Structure):
    _fields_ = [('flow', NfmcRealNVP), ('x', c_fp), ('n', C.c_int64), ('grad_out', c_fp), ('logq_out', c_fp)]


class NfmcDlmcStepArgs(C.Structure):
    _fields_ = [('flow', NfmcRealNVP), ('pot', NfmcPotential), ('x', c_fp), ('grad_u', c_fp), ('logq_out', c_fp),
                ('n', C.c_int64), ('step_size', C.c_float), ('reserved', C.c_int32)]


class NfmcSelectArgs(C.Structure):
    _fields_ = [('x', c_fp), ('x_prime', c_fp), ('n', C.c_int64), ('d', C.c_int32), ('n_carry', C.c_int32),
                ('log_ratio', c_fp), ('uniforms', c_fp), ('carry', c_fp * 2), ('carry_prime', c_fp * 2),
                ('rng', NfmcRng), ('rng_tag', C.c_int32), ('reserved', C.c_int32), ('stats', NfmcStats),
                ('mask_out', c_fp)]


class NfmcAdamW(C.Structure):
    _fields_ = [('lr', C.c_float), ('beta1', C.c_float), ('beta2', C.c_float), ('eps', C.c_float),
                ('weight_decay', C.c_float), ('step', C.c_int32)]


class NfmcFlowFit(C.Structure):
    _fields_ = [('flow', NfmcRealNVP), ('params', c_fp), ('adam_m', c_fp), ('adam_v', c_fp), ('n_params', C.c_int64),
                ('ea_off', C.c_int64), ('partial', c_fp), ('partial_floats', C.c_int64), ('status', c_fp),
                ('x_val', c_fp), ('n_val', C.c_int64), ('params_prev', c_fp), ('best', c_fp), ('run_state', c_fp),
                ('scratch', c_fp), ('scratch_bytes', C.c_int64)]


class NfmcBlobPiece(C.Structure):
    _fields_ = [('param', c_fp), ('vec_off', C.c_int64), ('rows', C.c_int32), ('cols', C.c_int32),
                ('vec_row_stride', C.c_int32), ('vec_col_stride', C.c_int32)]


class NfmcFitControl(C.Structure):
    _fields_ = [('n_epochs', C.c_int32), ('early_stopping', C.c_int32), ('early_stopping_threshold', C.c_int32),
                ('keep_best_weights', C.c_int32), ('skip_nonfinite', C.c_int32), ('reserved', C.c_int32)]


# indices into NfmcFlowFit.run_state (include/nfmc_hip.h: NFMC_FIT_*)
FIT_BEST_LOSS, FIT_SINCE_BEST, FIT_APPLIED, FIT_STOPPED, FIT_DIVERGED, FIT_LAST_LOSS, FIT_LAST_VAL, FIT_BOOKED = range(8)
FIT_STATE_FLOATS = 8


class NfmcDiagArgs(C.Structure):
    _fields_ = [('x', c_fp), ('n_draws', C.c_int64), ('n', C.c_int64), ('d', C.c_int32), ('max_lag', C.c_int32),
                ('group', C.c_int32), ('reserved', C.c_int32), ('sums', c_fp), ('work', c_fp), ('work_bytes', C.c_int64)]


# rows of NfmcDiagArgs.sums (include/nfmc_hip.h: NFMC_DIAG_*); the lags follow from DIAG_ACOV
DIAG_MAX_LAG = 127
DIAG_ROWS = ('sum_m', 'sum_m2', 'sum_mh', 'sum_mh2', 'sum_s2h', 'sum_mu', 'sum_mu2', 'sum_bt')
DIAG_ACOV = len(DIAG_ROWS)


class NfmcDiagStream(C.Structure):
    _fields_ = [('state', c_fp), ('state_bytes', C.c_int64), ('n', C.c_int64), ('d', C.c_int32), ('max_lag', C.c_int32),
                ('n_draws_planned', C.c_int64), ('n_seen', C.c_int64)]


class NfmcDiagStreamArgs(C.Structure):
    _fields_ = [('acc', C.POINTER(NfmcDiagStream)), ('ring', c_fp), ('ring_rows', C.c_int32), ('row', C.c_int32),
                ('n_rows', C.c_int32), ('reserved', C.c_int32), ('first_draw', C.c_int64)]


class NfmcDiagStreamSumsArgs(C.Structure):
    _fields_ = [('acc', C.POINTER(NfmcDiagStream)), ('group', C.c_int32), ('reserved', C.c_int32), ('sums', c_fp),
                ('work', c_fp), ('work_bytes', C.c_int64)]


class NfmcRankArgs(C.Structure):
    _fields_ = [('x', c_fp), ('n_draws', C.c_int64), ('n', C.c_int64), ('d', C.c_int32), ('series', C.c_int32),
                ('out', c_fp), ('order_stats', c_fp), ('nonfinite', c_fp), ('work', c_fp), ('work_bytes', C.c_int64)]


# NfmcRankArgs.series (include/nfmc_hip.h: NFMC_RANK_*)
RANK_BULK, RANK_FOLDED, RANK_TAIL_LOW, RANK_TAIL_HIGH = range(4)
RANK_SERIES = {'bulk': RANK_BULK, 'folded': RANK_FOLDED, 'tail_low': RANK_TAIL_LOW, 'tail_high': RANK_TAIL_HIGH}


class NfmcLimits(C.Structure):
    _fields_ = [('abi_version', C.c_int32), ('max_d_sampler', C.c_int32), ('max_d_flow', C.c_int32),
                ('max_hidden_valu', C.c_int32), ('max_hidden', C.c_int32), ('max_steps_per_call', C.c_int32)]


# every symbol include/nfmc_hip.h declares: (name, restype, argtypes)
SYMBOLS = [
    ('nfmc_stats_scratch_bytes', C.c_int64, [C.c_int32]),
    ('nfmc_tune_state_doubles', C.c_int64, [C.c_int32]),
    ('nfmc_tune_trajectory_doubles', C.c_int64, [C.c_int32]),
    ('nfmc_sampler_layout', C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ('nfmc_mala_steps_f32', C.c_int, [C.POINTER(NfmcMalaArgs), c_fp]),
    ('nfmc_hmc_steps_f32', C.c_int, [C.POINTER(NfmcHmcArgs), c_fp]),
    ('nfmc_mclmc_state_doubles', C.c_int64, [C.c_int32, C.c_int32]),
    ('nfmc_mclmc_steps_f32', C.c_int, [C.POINTER(NfmcMclmcArgs), c_fp]),
    ('nfmc_realnvp_padded_hidden', C.c_int32, [C.c_int32]),
    ('nfmc_realnvp_layer_floats', C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    ('nfmc_coupling_layer_floats', C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    ('nfmc_flow_scratch_bytes', C.c_int64, [C.POINTER(NfmcRealNVP), C.c_int64, C.c_int32]),
    ('nfmc_realnvp_forward_f32', C.c_int, [C.POINTER(NfmcRealNVP), c_fp, C.c_int64, c_fp, c_fp, c_fp, c_fp]),
    ('nfmc_realnvp_inverse_f32', C.c_int, [C.POINTER(NfmcRealNVP), c_fp, C.c_int64, c_fp, c_fp, c_fp,
                                           C.POINTER(NfmcRng), c_fp]),
    ('nfmc_flow_mh_steps_f32', C.c_int, [C.POINTER(NfmcFlowMhArgs), c_fp]),
    ('nfmc_flow_mh_supported_f32', C.c_int, [C.POINTER(NfmcFlowMhArgs)]),
    ('nfmc_jump_run_f32', C.c_int, [C.POINTER(NfmcJumpRun), c_fp]),
    ('nfmc_imh_parallel_supported_f32', C.c_int, [C.POINTER(NfmcFlowMhArgs)]),
    ('nfmc_imh_parallel_work_bytes', C.c_int64, [C.c_int64, C.c_int32, C.c_int32]),
    ('nfmc_imh_parallel_f32', C.c_int, [C.POINTER(NfmcFlowMhArgs), c_fp, C.c_int64, c_fp]),
    ('nfmc_neutra_scratch_bytes', C.c_int64, [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    ('nfmc_neutra_hmc_steps_f32', C.c_int, [C.POINTER(NfmcNeutraHmcArgs), c_fp]),
    ('nfmc_neutra_potential_grad_f32', C.c_int, [C.POINTER(NfmcRealNVP), C.POINTER(NfmcPotential), c_fp, C.c_int64,
                                                 c_fp, c_fp, c_fp]),
    ('nfmc_neutra_mh_steps_f32', C.c_int, [C.POINTER(NfmcNeutraMhArgs), c_fp]),
    ('nfmc_flow_logq_grad_f32', C.c_int, [C.POINTER(NfmcFlowLogqGradArgs), c_fp]),
    ('nfmc_flow_logq_grad_supported_f32', C.c_int, [C.POINTER(NfmcFlowLogqGradArgs)]),
    ('nfmc_dlmc_step_f32', C.c_int, [C.POINTER(NfmcDlmcStepArgs), c_fp]),
    ('nfmc_dlmc_step_supported_f32', C.c_int, [C.POINTER(NfmcDlmcStepArgs)]),
    ('nfmc_mh_accept_select_f32', C.c_int, [C.POINTER(NfmcSelectArgs), c_fp]),
    ('nfmc_langevin_propose_f32', C.c_int, [c_fp, c_fp, c_fp, C.c_float, C.c_int64, C.c_int32, C.POINTER(NfmcRng),
                                            c_fp, c_fp]),
    ('nfmc_langevin_log_ratio_f32', C.c_int, [c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, C.c_float, C.c_int64,
                                              C.c_int32, c_fp, c_fp]),
    ('nfmc_moments_update_f32', C.c_int, [c_fp, C.c_int64, C.c_int32, C.POINTER(NfmcStats), c_fp]),
    ('nfmc_stats_fold_f32', C.c_int, [C.POINTER(NfmcStats), C.c_int32, C.c_uint64, c_fp, C.c_uint64, c_fp]),
    ('nfmc_diag_sums_doubles', C.c_int64, [C.c_int32, C.c_int32]),
    ('nfmc_diag_work_bytes', C.c_int64, [C.c_int64, C.c_int32, C.c_int32]),
    ('nfmc_chain_diagnostics_f32', C.c_int, [C.POINTER(NfmcDiagArgs), c_fp]),
    ('nfmc_diag_stream_state_bytes', C.c_int64, [C.c_int64, C.c_int32, C.c_int32]),
    ('nfmc_diag_stream_work_bytes', C.c_int64, [C.c_int64, C.c_int32, C.c_int32]),
    ('nfmc_diag_stream_reset_f32', C.c_int, [C.POINTER(NfmcDiagStream), c_fp]),
    ('nfmc_diag_stream_update_f32', C.c_int, [C.POINTER(NfmcDiagStreamArgs), c_fp]),
    ('nfmc_diag_stream_sums_f32', C.c_int, [C.POINTER(NfmcDiagStreamSumsArgs), c_fp]),
    ('nfmc_rank_work_bytes', C.c_int64, [C.c_int64, C.c_int64, C.c_int32]),
    ('nfmc_rank_series_f32', C.c_int, [C.POINTER(NfmcRankArgs), c_fp]),
    ('nfmc_philox_normals_f32', C.c_int, [C.POINTER(NfmcRng), C.c_int32, C.c_int64, C.c_int32, c_fp, c_fp]),
    ('nfmc_philox_uniforms_f32', C.c_int, [C.POINTER(NfmcRng), C.c_int32, C.c_int64, c_fp, c_fp]),
    ('nfmc_flow_fit_supported_f32', C.c_int, [C.POINTER(NfmcRealNVP)]),
    ('nfmc_flow_fit_partial_floats', C.c_int64, [C.c_int64, C.c_int64]),
    ('nfmc_flow_fit_workspace', C.c_int64, [C.POINTER(NfmcRealNVP), C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_int64)]),
    ('nfmc_flow_fit_step_f32', C.c_int, [C.POINTER(NfmcFlowFit), c_fp, C.c_int64, C.POINTER(NfmcAdamW), c_fp]),
    ('nfmc_flow_variational_fit_step_f32', C.c_int, [C.POINTER(NfmcFlowFit), C.POINTER(NfmcPotential), c_fp, C.c_int64,
                                                    C.POINTER(NfmcAdamW), c_fp]),
    ('nfmc_flow_fit_epochs_f32', C.c_int, [C.POINTER(NfmcFlowFit), C.POINTER(NfmcPotential), c_fp, C.c_int64, C.c_int64,
                                          C.POINTER(NfmcAdamW), C.POINTER(NfmcFitControl), C.c_int32, C.c_int32, c_fp]),
    ('nfmc_flow_blob_copy_f32', C.c_int, [c_fp, C.POINTER(NfmcBlobPiece), C.c_int32, C.c_int32, c_fp]),
    ('nfmc_rows_sample_f32', C.c_int, [c_fp, C.c_int64, C.c_int32, C.c_uint64, C.c_int64, c_fp, C.c_int64, c_fp, c_fp]),
    ('nfmc_rows_sample_index', C.c_int64, [C.c_int64, C.c_uint64, C.c_int64]),
    ('nfmc_limits', C.c_int, [C.POINTER(NfmcLimits)]),
    ('nfmc_error_string', C.c_char_p, [C.c_int]),
    ('nfmc_build_digest', C.c_char_p, []),
]
