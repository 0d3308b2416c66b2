"""ctypes binding of libgomoku_hip.so (include/gomoku_hip.h)."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "libgomoku_hip.so")
# tools/*.sh ask for the profiling flavour of the library explicitly (GMK_HIP_LIB=prof; built by `python -m gomokuai_amd.build
# --profile`): only that one reads GMK_*_PHASE_MASK / GMK_*_PROFILE.  Anything else loads the production library, which ignores them.
if os.environ.get("GMK_HIP_LIB") == "prof":
    _SO = os.path.join(_HERE, "libgomoku_hip_prof.so")
elif os.environ.get("GMK_HIP_LIB", "").endswith(".so"):          # an experiment build of tools/k1_variants.py, by path
    _SO = os.environ["GMK_HIP_LIB"]

N = 225


class GmkError(RuntimeError):
    pass


class TrainGemmDesc(C.Structure):
    """gmk_train_gemm_desc (include/gomoku_hip.h): train_gemm_kernel's argument block and the extent, in floats, of every buffer it names."""
    _fields_ = [("A", C.c_void_p), ("sam", C.c_int64), ("sak", C.c_int64), ("a_floats", C.c_int64),
                ("B", C.c_void_p), ("sbk", C.c_int64), ("sbn", C.c_int64), ("b_floats", C.c_int64),
                ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
                ("kslab", C.c_int32), ("nz", C.c_int32), ("z0", C.c_int32),
                ("part", C.c_void_p), ("part_floats", C.c_int64),
                ("C", C.c_void_p), ("ldc", C.c_int64), ("cs", C.c_int64), ("c_floats", C.c_int64),
                ("C2", C.c_void_p), ("ldc2", C.c_int64), ("c2_floats", C.c_int64),
                ("cq", C.c_int32), ("nsplit", C.c_int32),
                ("bias", C.c_void_p), ("bias_floats", C.c_int64),
                ("mask", C.c_void_p), ("ldm", C.c_int64), ("mask_floats", C.c_int64),
                ("relu", C.c_int32)]


class TableInfo(C.Structure):
    _fields_ = [("n_patterns", C.c_int32), ("n_states", C.c_int32), ("dat_size", C.c_int32),
                ("max_emissions", C.c_int32), ("trans_words", C.c_int32), ("emit_words", C.c_int32),
                ("invariants", C.c_int32 * 5)]


_lib = None

# gmk_*_set_option (include/gomoku_hip.h)
OPT_NOISE_SAMPLER, OPT_LOCKSTEP, OPT_AZ_LEAVES = 1, 2, 3
OPT_AZ_VCF_DEPTH, OPT_AZ_VCF_BUDGET = 4, 5     # K7 + K14: forced wins by fours solved at the leaves (AlphaZeroMCTS(vcf_depth=, vcf_budget=))
OPT_AZ_PROOF = 6                               # K7 + proofs: proven wins and losses carried up the tree (AlphaZeroMCTS(proof=))
AZ_PROOF_NONE, AZ_PROOF_WINS, AZ_PROOF_LOSES = 0, 1, 2
OPT_AZ_VCF_DEFEND = 7                          # K7 + K15: the replies that lose to a forced win by fours, proven at the leaves (AlphaZeroMCTS(vcf_defend=))
PVNET_F32, PVNET_BF16 = 0, 1                   # GMK_PVNET_*: gmk_pvnet_set_precision (FusedPolicyValueNetwork(precision=))
PVNET_PRECISIONS = {"f32": PVNET_F32, "bf16": PVNET_BF16}
PVNET_SYMMETRIES = {"none": 0, "all": 1, "random": 2}      # GMK_PVNET_SYM_*: gmk_pvnet_evaluate_sym (FusedPolicyValueNetwork.symmetric(mode); K22)
AZ_MAX_LEAVES = 8                              # GMK_AZ_MAX_LEAVES: leaves per game per step of a K7 handle (AlphaZeroMCTS(leaves=))
NOISE_SAMPLERS = {"std": 0, "counter": 1}      # std::gamma_distribution on the host / the counter-based sampler of include/gomoku_noise.h on the device

# every symbol include/gomoku_hip.h declares (checked by tests/test_cabi.py)
EXPORTS = [
    "gmk_init", "gmk_shutdown", "gmk_pool_release", "gmk_pool_poison", "gmk_last_error", "gmk_device_info",
    "gmk_tables_info", "gmk_tables_pattern", "gmk_tables_copy", "gmk_tables_copy_dat", "gmk_tables_scan",
    "gmk_synth_boards", "gmk_moves_to_planes",
    "gmk_eval_batch", "gmk_eval_batch_host", "gmk_eval_launch_info", "gmk_eval_lane_records",
    "gmk_mcts_create", "gmk_mcts_destroy", "gmk_mcts_set_roots", "gmk_mcts_set_game_ids", "gmk_mcts_run", "gmk_mcts_root_stats",
    "gmk_mcts_alg_bytes", "gmk_mcts_launch_info", "gmk_visits_to_pi", "gmk_mcts_advance", "gmk_mcts_step", "gmk_mcts_step_host", "gmk_mcts_add_root_noise", "gmk_mcts_set_option", "gmk_mcts_reserve", "gmk_selfplay_run", "gmk_samples_from_records",
    "gmk_records_scan", "gmk_records_packed_bytes", "gmk_records_pack", "gmk_records_unpack", "gmk_samples_from_packed",
    "gmk_evalstate_create", "gmk_evalstate_destroy", "gmk_evalstate_reset", "gmk_evalstate_update", "gmk_evalstate_update_host", "gmk_evalstate_read",
    "gmk_az_create", "gmk_az_destroy", "gmk_az_set_roots", "gmk_az_select", "gmk_az_expand", "gmk_az_select_host", "gmk_az_expand_host", "gmk_az_read_node_host", "gmk_az_read_children_host", "gmk_az_set_leaf_host", "gmk_az_rollout_host", "gmk_az_expand_stages_host", "gmk_az_write_stats_host", "gmk_az_step", "gmk_az_root_choice", "gmk_az_step_device", "gmk_az_advance", "gmk_az_set_slots", "gmk_az_live_games", "gmk_az_set_game_ids", "gmk_az_add_root_noise", "gmk_az_set_option", "gmk_az_add_playouts", "gmk_az_playouts_owed", "gmk_az_root_stats", "gmk_az_vcf_stats", "gmk_az_vcf_verdicts_host", "gmk_az_defend_stats", "gmk_az_defend_verdicts_host", "gmk_az_root_proofs", "gmk_az_proof_stats",
    "gmk_az_advance_sampled", "gmk_az_root_choice_sampled", "gmk_move_sample_host",
    "gmk_az_set_gumbel", "gmk_az_advance_gumbel", "gmk_az_root_choice_gumbel",
    "gmk_gumbel_sequence_host", "gmk_gumbel_setup_host", "gmk_gumbel_pick_host", "gmk_gumbel_move_host", "gmk_gumbel_row_host",
    "gmk_samples_from_records_target", "gmk_samples_from_packed_target", "gmk_replay_sample_target",
    "gmk_mcts_advance_sampled", "gmk_selfplay_run_sampled", "gmk_trad_selfplay_run_sampled", "gmk_trad_root_choice_sampled",
    "gmk_trad_create", "gmk_trad_destroy", "gmk_trad_reset_evaluators", "gmk_trad_set_game_ids", "gmk_trad_set_positions", "gmk_trad_run", "gmk_trad_step", "gmk_trad_root_choice", "gmk_trad_step_device", "gmk_trad_add_root_noise", "gmk_trad_set_option", "gmk_trad_reserve", "gmk_trad_root_stats", "gmk_trad_read_evaluators", "gmk_trad_run_poolrave", "gmk_trad_run_rave", "gmk_trad_root_amaf", "gmk_trad_selfplay_run", "gmk_pvnet_create", "gmk_pvnet_destroy", "gmk_pvnet_forward", "gmk_pvnet_set_dense", "gmk_pvnet_evaluate",
    "gmk_pvnet_set_precision", "gmk_pvnet_get_precision", "gmk_bf16_round_host",
    "gmk_pvnet_evaluate_sym", "gmk_pvnet_sym_pick_host",
    "gmk_pattern_policy", "gmk_pattern_policy_host", "gmk_pattern_play",
    "gmk_pattern_evaluate_states", "gmk_pattern_evaluate_states_host", "gmk_pattern_states_list_host", "gmk_pattern_states_finish_host",
    "gmk_vcf_solve", "gmk_vcf_solve_host", "gmk_vcf_defend", "gmk_vcf_defend_host",
    "gmk_vcf_threats", "gmk_vcf_threats_host", "gmk_vct_solve", "gmk_vct_solve_host",
    "gmk_match_referee", "gmk_mcts_root_choice", "gmk_mcts_step_device",
    "gmk_mcts_ensemble_merge", "gmk_trad_ensemble_merge", "gmk_ensemble_merge_host",
    "gmk_replay_create", "gmk_replay_destroy", "gmk_replay_reset", "gmk_replay_append", "gmk_replay_append_packed", "gmk_replay_size",
    "gmk_replay_sample", "gmk_replay_draw_host", "gmk_replay_image_bytes", "gmk_replay_snapshot", "gmk_replay_restore", "gmk_replay_image_check_host",
    "gmk_train_create", "gmk_train_destroy", "gmk_train_forward", "gmk_train_grads", "gmk_train_step", "gmk_train_params", "gmk_train_set_params",
    "gmk_train_get_block", "gmk_train_set_block", "gmk_train_set_step_count", "gmk_train_export", "gmk_train_info",
    "gmk_train_kernel_gemm", "gmk_train_kernel_reduce", "gmk_train_kernel_im2col", "gmk_train_kernel_col2im",
    "gmk_noise_mix_rows",
]


def _torch_first():
    """PyTorch-ROCm bundles its own copy of the HIP runtime (torch/lib/libamdhip64.so) next to the system one this
    library links (libamdhip64.so.7).  Both can serve one process, but only when torch's copy brings the GPU up
    first; the other order leaves torch with "No HIP GPUs are available".  So: initialise torch.cuda before the
    first HIP call of this library whenever torch is importable (it provides device memory and streams here)."""
    try:
        import torch
    except ImportError:
        return
    if torch.cuda.is_available():
        torch.cuda.init()


def load():
    """Loads the HIP library; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    _torch_first()
    if not os.path.exists(_SO):
        raise GmkError("libgomoku_hip.so is missing: run `python -m gomokuai_amd.build` "
                       "(there is no CPU fallback for the compute path)")
    L = C.CDLL(_SO)
    vp = C.c_void_p
    L.gmk_last_error.restype = C.c_char_p
    L.gmk_init.argtypes = [C.c_int]
    L.gmk_device_info.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_size_t), C.c_char_p, C.c_int]
    L.gmk_tables_info.argtypes = [C.POINTER(TableInfo)]
    L.gmk_tables_pattern.argtypes = [C.c_int, C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.gmk_tables_copy.argtypes = [vp, vp, vp]
    L.gmk_tables_copy_dat.argtypes = [vp, vp, vp]
    L.gmk_tables_scan.argtypes = [vp, C.c_int, vp, vp, C.c_int]
    L.gmk_synth_boards.argtypes = [C.c_uint64, C.c_uint32, C.c_int, C.c_int, vp, C.c_int, vp, vp]
    L.gmk_moves_to_planes.argtypes = [vp, C.c_int, vp, C.c_int, vp]
    L.gmk_eval_batch.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp]
    L.gmk_eval_batch_host.argtypes = [vp, C.c_int, vp, vp, vp, vp]
    L.gmk_eval_launch_info.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.gmk_eval_lane_records.argtypes = [vp]
    L.gmk_mcts_create.argtypes = [C.c_int, C.c_int, C.c_double, C.c_int, C.c_uint64, C.POINTER(vp)]
    L.gmk_mcts_destroy.argtypes = [vp]
    L.gmk_mcts_set_roots.argtypes = [vp, vp, vp, C.c_uint32]
    L.gmk_mcts_set_game_ids.argtypes = [vp, vp]
    L.gmk_trad_set_game_ids.argtypes = [vp, vp]
    L.gmk_az_set_game_ids.argtypes = [vp, vp]
    L.gmk_mcts_run.argtypes = [vp, C.c_int, vp]
    L.gmk_mcts_root_stats.argtypes = [vp, vp, vp, vp, vp, vp]
    L.gmk_mcts_alg_bytes.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.gmk_mcts_launch_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.gmk_visits_to_pi.argtypes = [vp, C.c_int, vp]
    L.gmk_mcts_advance.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, vp]
    L.gmk_mcts_step.argtypes = [vp, vp, vp, vp, vp, vp, vp, C.c_int, vp]
    L.gmk_mcts_step_host.argtypes = [vp, vp, C.c_int]
    L.gmk_mcts_root_choice.argtypes = [vp, vp, vp, vp]
    L.gmk_mcts_step_device.argtypes = [vp, vp, vp, C.c_int, vp]
    L.gmk_selfplay_run.argtypes = [vp, C.c_int, C.c_uint32, C.c_int, C.c_int, C.c_float, C.c_float, vp, C.c_int, vp, vp, vp, vp, vp, C.POINTER(C.c_int32), vp]
    L.gmk_mcts_advance_sampled.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp]
    L.gmk_selfplay_run_sampled.argtypes = [vp, C.c_int, C.c_uint32, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp, vp, vp, C.POINTER(C.c_int32), vp]
    L.gmk_trad_root_choice_sampled.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_uint64, C.c_uint32, vp]
    L.gmk_mcts_add_root_noise.argtypes = [vp, C.c_float, C.c_float, vp]
    L.gmk_noise_mix_rows.argtypes = [vp, vp, vp, vp, C.c_int, C.c_float, C.c_float, C.c_uint64, vp]
    L.gmk_mcts_set_option.argtypes = [vp, C.c_int, C.c_int]
    L.gmk_mcts_reserve.argtypes = [vp, C.c_int]
    L.gmk_trad_reserve.argtypes = [vp, C.c_int]
    L.gmk_evalstate_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.gmk_evalstate_destroy.argtypes = [vp]
    L.gmk_evalstate_reset.argtypes = [vp]
    L.gmk_evalstate_update.argtypes = [vp, vp, C.c_int, vp]
    L.gmk_evalstate_update_host.argtypes = [vp, vp, C.c_int]
    L.gmk_evalstate_read.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.gmk_az_create.argtypes = [C.c_int, C.c_int, C.c_double, C.POINTER(vp)]
    L.gmk_az_destroy.argtypes = [vp]
    L.gmk_az_set_roots.argtypes = [vp, vp, vp]
    L.gmk_az_select.argtypes = [vp, vp, vp]
    L.gmk_az_expand.argtypes = [vp, vp, vp, vp]
    L.gmk_az_select_host.argtypes = [vp, vp, vp]
    L.gmk_az_step.argtypes = [vp, vp]
    L.gmk_az_root_choice.argtypes = [vp, vp, vp, vp]
    L.gmk_az_step_device.argtypes = [vp, vp, vp, C.c_int, vp, C.POINTER(C.c_int32), vp]
    L.gmk_az_live_games.argtypes = [vp, C.POINTER(C.c_int32)]
    L.gmk_az_set_slots.argtypes = [vp, C.c_int, vp, C.c_int, vp]
    L.gmk_az_advance.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.POINTER(C.c_int32), vp]
    L.gmk_az_advance_sampled.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint32, C.POINTER(C.c_int32), vp]
    L.gmk_az_root_choice_sampled.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_uint64, C.c_uint32, vp]
    L.gmk_move_sample_host.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_uint64, vp]
    L.gmk_az_set_gumbel.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_uint64, C.c_uint32]
    L.gmk_az_advance_gumbel.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.POINTER(C.c_int32), vp]
    L.gmk_az_root_choice_gumbel.argtypes = [vp, vp, vp, vp]
    L.gmk_gumbel_sequence_host.argtypes = [C.c_int, C.c_int, vp]
    L.gmk_gumbel_setup_host.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.c_uint64, vp, vp, vp, vp, vp]
    L.gmk_gumbel_pick_host.argtypes = [vp] * 8 + [C.c_int, C.c_int, C.c_double, C.c_double, vp]
    L.gmk_gumbel_move_host.argtypes = [vp] * 7 + [C.c_int, C.c_double, C.c_double, vp]
    L.gmk_gumbel_row_host.argtypes = [vp] * 4 + [C.c_int, C.c_double, C.c_double, vp]
    L.gmk_samples_from_records_target.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
    L.gmk_samples_from_packed_target.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
    L.gmk_replay_sample_target.argtypes = [vp, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]
    L.gmk_az_add_root_noise.argtypes = [vp, C.c_float, C.c_float, C.c_uint64, C.c_uint32, vp]
    L.gmk_az_set_option.argtypes = [vp, C.c_int, C.c_int]
    L.gmk_az_add_playouts.argtypes = [vp, C.c_int, vp]
    L.gmk_az_playouts_owed.argtypes = [vp, C.POINTER(C.c_int32), vp]
    L.gmk_az_expand_host.argtypes = [vp, vp, vp]
    L.gmk_az_root_stats.argtypes = [vp] * 8
    L.gmk_az_vcf_stats.argtypes = [vp] * 5
    L.gmk_az_root_proofs.argtypes = [vp] * 3
    L.gmk_az_proof_stats.argtypes = [vp] * 3
    L.gmk_az_vcf_verdicts_host.argtypes = [vp] * 5
    L.gmk_az_defend_stats.argtypes = [vp] * 5
    L.gmk_az_defend_verdicts_host.argtypes = [vp] * 5
    L.gmk_trad_create.argtypes = [C.c_int, C.c_int, C.POINTER(vp)]
    L.gmk_trad_destroy.argtypes = [vp]
    L.gmk_trad_reset_evaluators.argtypes = [vp]
    L.gmk_trad_set_positions.argtypes = [vp, vp, vp]
    L.gmk_trad_run.argtypes = [vp, C.c_int, C.c_double, vp]
    L.gmk_trad_step.argtypes = [vp, vp]
    L.gmk_trad_root_choice.argtypes = [vp, vp, vp, vp]
    L.gmk_trad_step_device.argtypes = [vp, vp, vp, C.c_int, vp]
    L.gmk_match_referee.argtypes = [C.c_int, C.c_int] + [vp] * 11
    L.gmk_mcts_ensemble_merge.argtypes = [vp, C.c_int] + [vp] * 8
    L.gmk_trad_ensemble_merge.argtypes = [vp, C.c_int] + [vp] * 8
    L.gmk_ensemble_merge_host.argtypes = [C.c_int, C.c_int] + [vp] * 10
    L.gmk_trad_add_root_noise.argtypes = [vp, C.c_float, C.c_float, C.c_uint64, C.c_uint32, vp]
    L.gmk_trad_set_option.argtypes = [vp, C.c_int, C.c_int]
    L.gmk_trad_root_stats.argtypes = [vp] * 10
    L.gmk_trad_read_evaluators.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.gmk_trad_run_poolrave.argtypes = [vp, C.c_int, C.c_double, C.c_uint64, C.c_uint32, vp]
    L.gmk_trad_run_rave.argtypes = [vp, C.c_int, C.c_double, vp]
    L.gmk_trad_selfplay_run.argtypes = [vp, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_double, C.c_uint64, C.c_int, C.c_float, C.c_float,
                                        vp, C.c_int, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), vp]
    L.gmk_trad_selfplay_run_sampled.argtypes = [vp, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_double, C.c_uint64, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int,
                                                vp, C.c_int, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), vp]
    L.gmk_trad_root_amaf.argtypes = [vp, vp, vp]
    L.gmk_pvnet_create.argtypes = [vp] * 10 + [C.POINTER(vp)]
    L.gmk_pvnet_destroy.argtypes = [vp]
    L.gmk_pvnet_forward.argtypes = [vp, vp, C.c_int, vp, vp, vp]
    L.gmk_pvnet_set_dense.argtypes = [vp] * 6 + [C.c_float]
    L.gmk_pvnet_evaluate.argtypes = [vp, vp, C.c_int, vp, vp, vp]
    L.gmk_pvnet_set_precision.argtypes = [vp, C.c_int]
    L.gmk_pvnet_get_precision.argtypes = [vp, C.POINTER(C.c_int)]
    L.gmk_bf16_round_host.argtypes = [vp, C.c_size_t, vp]
    L.gmk_pvnet_evaluate_sym.argtypes = [vp, vp, C.c_int, C.c_int, C.c_uint64, vp, vp, vp]
    L.gmk_pvnet_sym_pick_host.argtypes = [vp, C.c_int, C.c_uint64, vp]
    L.gmk_samples_from_records.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp]
    L.gmk_records_scan.argtypes = [vp, C.c_int, vp, vp]
    L.gmk_records_packed_bytes.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_uint64), vp]
    L.gmk_records_pack.argtypes = [vp, vp, vp, vp, C.c_int, vp, vp, C.c_uint64, vp, vp]
    L.gmk_records_unpack.argtypes = [vp, C.c_uint64, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp]
    L.gmk_samples_from_packed.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp]
    L.gmk_pattern_policy.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp]
    L.gmk_pattern_policy_host.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, vp, vp]
    L.gmk_pattern_play.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
    L.gmk_pattern_evaluate_states.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
    L.gmk_pattern_evaluate_states_host.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp]
    L.gmk_pattern_states_list_host.argtypes = [vp, C.c_int, vp, vp, vp]
    L.gmk_pattern_states_finish_host.argtypes = [vp, vp, C.c_int, C.c_int, vp]
    L.gmk_vcf_solve.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_uint32, C.c_int, vp, vp, vp, vp, vp, vp]
    L.gmk_vcf_solve_host.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_uint32, C.c_int, vp, vp, vp, vp, vp]
    L.gmk_vcf_defend.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_uint32, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]
    L.gmk_vcf_defend_host.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_uint32, C.c_int, vp, vp, vp, vp, vp, vp, vp]
    L.gmk_vcf_threats.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_uint32, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.gmk_vcf_threats_host.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_uint32, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]
    L.gmk_vct_solve.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]
    L.gmk_vct_solve_host.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp]
    L.gmk_replay_create.argtypes = [C.c_int64, C.c_int64, C.c_uint64, C.POINTER(vp)]
    L.gmk_replay_destroy.argtypes = [vp]
    L.gmk_replay_reset.argtypes = [vp, vp]
    L.gmk_replay_append.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.c_int, vp, vp]
    L.gmk_replay_append_packed.argtypes = [vp, vp, C.c_int, vp, C.c_int, vp, vp]
    L.gmk_replay_size.argtypes = [vp] + [C.POINTER(C.c_int64)] * 4 + [vp]
    L.gmk_replay_sample.argtypes = [vp, C.c_int, C.c_int64, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]
    L.gmk_replay_draw_host.argtypes = [C.c_uint64, C.c_int64, C.c_int64, C.c_int64, vp]
    L.gmk_replay_image_bytes.argtypes = [vp, C.POINTER(C.c_int64), vp]
    L.gmk_replay_snapshot.argtypes = [vp, vp, C.c_int64, vp, vp]
    L.gmk_replay_restore.argtypes = [vp, vp, C.c_int64, vp, vp]
    L.gmk_replay_image_check_host.argtypes = [vp, C.c_int64, vp]
    L.gmk_train_create.argtypes = [vp] * 16 + [C.c_int, C.POINTER(vp)]
    L.gmk_train_destroy.argtypes = [vp]
    L.gmk_train_forward.argtypes = [vp, vp, C.c_int, vp, vp, vp]
    L.gmk_train_grads.argtypes = [vp, vp, vp, vp, C.c_int, vp, vp, vp]
    L.gmk_train_step.argtypes = [vp, vp, vp, vp, C.c_int, C.c_float, vp, vp, vp, vp]
    L.gmk_train_params.argtypes = [vp] * 17
    L.gmk_train_set_params.argtypes = [vp] * 17
    L.gmk_train_get_block.argtypes = [vp, C.c_int, vp]
    L.gmk_train_set_block.argtypes = [vp, C.c_int, vp]
    L.gmk_train_set_step_count.argtypes = [vp, C.c_int64]
    L.gmk_train_export.argtypes = [vp, vp, vp]
    L.gmk_train_info.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.gmk_train_kernel_gemm.argtypes = [C.POINTER(TrainGemmDesc), vp]
    L.gmk_train_kernel_reduce.argtypes = [vp, C.c_int, C.c_int64, vp, vp]
    L.gmk_train_kernel_im2col.argtypes = [vp, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int, vp, vp]
    L.gmk_train_kernel_col2im.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp]
    _lib = L
    return L


def _check(rc):
    if rc < 0:
        raise GmkError("libgomoku_hip: %s (status %d)" % (load().gmk_last_error().decode(), rc))
    return rc


def init(device=0):
    _check(load().gmk_init(device))


def pool_poison(on=True):
    """Diagnostic: reused device blocks of the library's pool are filled with 0xA5 before the next handle gets them (gmk_pool_poison)."""
    _check(load().gmk_pool_poison(1 if on else 0))


def release_pool():
    """Returns the device blocks the library keeps from destroyed handles (up to 224 GB of tree arenas) to the driver."""
    _check(load().gmk_pool_release())


def device_info():
    cu = C.c_int()
    mem = C.c_size_t()
    name = C.create_string_buffer(256)
    _check(load().gmk_device_info(C.byref(cu), C.byref(mem), name, 256))
    return {"cu_count": cu.value, "hbm_bytes": mem.value, "name": name.value.decode()}


# ---------------- pattern tables (host) ----------------
def tables_info():
    info = TableInfo()
    _check(load().gmk_tables_info(C.byref(info)))
    return info


def tables_pattern(i):
    s = C.create_string_buffer(8)
    fav, typ, score = C.c_int(), C.c_int(), C.c_int()
    _check(load().gmk_tables_pattern(i, s, C.byref(fav), C.byref(typ), C.byref(score)))
    return s.value.decode(), fav.value, typ.value, score.value


def tables_copy():
    info = tables_info()
    trans = np.zeros(info.trans_words, dtype=np.uint32)
    emit = np.zeros(info.emit_words, dtype=np.uint16)
    pinfo = np.zeros(info.n_patterns * 2, dtype=np.uint32)
    _check(load().gmk_tables_copy(trans.ctypes.data, emit.ctypes.data, pinfo.ctypes.data))
    return trans, emit, pinfo


def tables_copy_dat():
    info = tables_info()
    base = np.zeros(info.dat_size, dtype=np.int32)
    check = np.zeros(info.dat_size, dtype=np.int32)
    fail = np.zeros(info.dat_size, dtype=np.int32)
    _check(load().gmk_tables_copy_dat(base.ctypes.data, check.ctypes.data, fail.ctypes.data))
    return base, check, fail


def tables_scan(codes):
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    pats = np.zeros(512, dtype=np.int32)
    offs = np.zeros(512, dtype=np.int32)
    m = _check(load().gmk_tables_scan(codes.ctypes.data, len(codes), pats.ctypes.data, offs.ctypes.data, 512))
    return list(zip(pats[:m].tolist(), offs[:m].tolist()))


# ---------------- synthetic workloads (host) ----------------
DEFAULT_SEED = 0x9E3779B97F4A7C15


def synth_boards(n, kind=0, seed=DEFAULT_SEED, first_board=0, stride=64):
    """-> (moves u8[n,stride], lens i32[n], planes u16[n,2,16])."""
    moves = np.zeros((n, stride), dtype=np.uint8)
    lens = np.zeros(n, dtype=np.int32)
    planes = np.zeros((n, 2, 16), dtype=np.uint16)
    _check(load().gmk_synth_boards(seed, first_board, n, kind, moves.ctypes.data, stride, lens.ctypes.data, planes.ctypes.data))
    return moves, lens, planes


def moves_to_planes(moves, lens):
    moves = np.ascontiguousarray(moves, dtype=np.uint8)
    lens = np.ascontiguousarray(lens, dtype=np.int32)
    n, stride = moves.shape
    planes = np.zeros((n, 2, 16), dtype=np.uint16)
    _check(load().gmk_moves_to_planes(moves.ctypes.data, stride, lens.ctypes.data, n, planes.ctypes.data))
    return planes


# ---------------- K1: batched position evaluation ----------------
def eval_batch_host(planes):
    """planes u16[n,2,16] (host) -> scores i32[n,4,225], density i32[n,2,2,225], totals u32[n,11], status i32[n].
    Runs on the GPU through gmk_eval_batch_host; raises without one."""
    init()
    planes = np.ascontiguousarray(planes, dtype=np.uint16)
    n = planes.shape[0]
    scores = np.zeros((n, 4, N), dtype=np.int32)
    density = np.zeros((n, 2, 2, N), dtype=np.int32)
    totals = np.zeros((n, 11), dtype=np.uint32)
    status = np.zeros(n, dtype=np.int32)
    _check(load().gmk_eval_batch_host(planes.ctypes.data, n, scores.ctypes.data, density.ctypes.data,
                                      totals.ctypes.data, status.ctypes.data))
    return scores, density, totals, status


def eval_batch(d_planes, n, d_scores=None, d_density=None, d_totals=None, d_status=None, stream=None):
    """Device-pointer form (ints, e.g. torch.Tensor.data_ptr()); asynchronous on `stream`."""
    _check(load().gmk_eval_batch(d_planes, n, d_scores, d_density, d_totals, d_status, stream))


def eval_launch_info(n):
    g, b, l = C.c_int(), C.c_int(), C.c_int()
    _check(load().gmk_eval_launch_info(n, C.byref(g), C.byref(b), C.byref(l)))
    return {"grid": g.value, "block": b.value, "lds_bytes": l.value}


def eval_lane_records():
    """K1's 64 lane records as the host builds and checks them, [64, 8] uint32: [:, 0] the lines word, [:, 1] the place word (host only)."""
    rec = np.zeros((64, 8), dtype=np.uint32)
    _check(load().gmk_eval_lane_records(rec.ctypes.data))
    return rec


# ---------------- K3: batched MCTS (RandomPolicy) ----------------
class BatchedMCTS:
    """n_games independent searches on the GPU (gmk_mcts_*).  Fresh roots per set_roots()."""

    def __init__(self, n_games, playouts_capacity=800, c_puct=5.0, c_rollouts=5, seed=DEFAULT_SEED, node_capacity=None):
        init()
        self.n = n_games
        self.cap = node_capacity if node_capacity is not None else playouts_capacity * 225 + 1
        h = C.c_void_p()
        _check(load().gmk_mcts_create(n_games, self.cap, c_puct, c_rollouts, seed, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None) and load is not None:
            load().gmk_mcts_destroy(self.h)
            self.h = None

    __del__ = close

    def set_roots(self, planes, last_moves, first_game_id=0):
        planes = np.ascontiguousarray(planes, dtype=np.uint16)
        last = np.ascontiguousarray(last_moves, dtype=np.int16)
        assert planes.shape == (self.n, 2, 16) and last.shape == (self.n,)
        _check(load().gmk_mcts_set_roots(self.h, planes.ctypes.data, last.ctypes.data, first_game_id))

    STATUS_TERMINAL, STATUS_ARENA_FULL, STATUS_ILLEGAL_STEP = 1, 2, 4      # bits of root_stats()[4]

    def set_game_ids(self, ids):
        """Global id of every game (uint32[n]) instead of first_game_id + g: the id keys the game's random streams."""
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        assert ids.shape == (self.n,)
        _check(load().gmk_mcts_set_game_ids(self.h, ids.ctypes.data))

    def run(self, playouts, stream=None):
        _check(load().gmk_mcts_run(self.h, playouts, stream))

    def root_stats(self):
        visits = np.zeros((self.n, N), dtype=np.uint32)
        q = np.zeros(self.n, dtype=np.float32)
        rv = np.zeros(self.n, dtype=np.uint32)
        nodes = np.zeros(self.n, dtype=np.uint32)
        status = np.zeros(self.n, dtype=np.int32)
        _check(load().gmk_mcts_root_stats(self.h, visits.ctypes.data, q.ctypes.data, rv.ctypes.data, nodes.ctypes.data, status.ctypes.data))
        return visits, q, rv, nodes, status

    def advance(self, d_moves, d_visits, d_lens, d_winner, d_unfinished, reuse_subtree=False, stream=None, sample=None):
        """One self-play move for every unfinished game (device pointers as ints).  sample = (plies, power): gmk_mcts_advance_sampled -- a
        game with fewer than `plies` stones on its root board plays a child drawn in proportion to visits^power (power 1..3;
        include/gomoku_sample.h), keyed by the handle's seed, the game's global id and its stones."""
        if sample is None:
            _check(load().gmk_mcts_advance(self.h, d_moves, d_visits, d_lens, d_winner, d_unfinished, int(reuse_subtree), stream))
        else:
            _check(load().gmk_mcts_advance_sampled(self.h, d_moves, d_visits, d_lens, d_winner, d_unfinished, int(reuse_subtree), int(sample[0]), int(sample[1]), stream))

    def step(self, d_forced_moves, d_moves, d_visits, d_lens, d_winner, d_unfinished, reuse_subtree=False, stream=None):
        """MCTS::stepForward(move) per game: d_forced_moves int16[n] on the device, -1 = the most visited child."""
        _check(load().gmk_mcts_step(self.h, d_forced_moves, d_moves, d_visits, d_lens, d_winner, d_unfinished, int(reuse_subtree), stream))

    def step_host(self, moves, reuse_subtree=False):
        """gmk_mcts_step_host: step() with the moves from the host (int16[n], -1 = the most visited child), synchronous, without game records."""
        m = np.ascontiguousarray(moves, dtype=np.int16)
        assert m.shape == (self.n,)
        _check(load().gmk_mcts_step_host(self.h, m.ctypes.data, int(bool(reuse_subtree))))

    def root_choice(self, cells, visits=None, stream=None):
        """gmk_mcts_root_choice: the most visited root child (first maximum in cell order; -1 without a visited one or in a finished game) into
        cells (torch int16[n] on the GPU) and the root children's visit counts by cell, saturated at 65 535, into visits (2-byte torch
        [n, 225], or None); nothing comes to the host."""
        _root_choice(load().gmk_mcts_root_choice, self, cells, visits, stream)

    def step_device(self, cells, verdict, fresh_root=False, stream=None):
        """gmk_mcts_step_device: step() with the cells (torch int16[n]) and the referee's verdicts (torch int32[n], MATCH_*) on the GPU; the
        subtree is kept unless fresh_root."""
        _check_step_device(self, cells, verdict)
        _check(load().gmk_mcts_step_device(self.h, cells.data_ptr(), verdict.data_ptr(), int(bool(fresh_root)), _current_stream(stream)))

    def add_root_noise(self, alpha=0.05, epsilon=0.25, stream=None):
        _check(load().gmk_mcts_add_root_noise(self.h, alpha, epsilon, stream))

    def set_option(self, option, value):
        """gmk_mcts_set_option: OPT_NOISE_SAMPLER -> NOISE_SAMPLERS["std" | "counter"], OPT_LOCKSTEP -> 0 / 1."""
        _check(load().gmk_mcts_set_option(self.h, int(option), int(value)))

    def reserve(self, two_arenas=False):
        """gmk_mcts_reserve: allocate the tree arenas now (two per game for the persistent loop with kept subtrees)."""
        _check(load().gmk_mcts_reserve(self.h, int(bool(two_arenas))))

    def selfplay_run(self, n_total, first_game_id, playouts, d_moves, d_visits, d_lens, d_winner, open_moves=None, open_lens=None,
                     reuse_subtree=False, root_noise=None, stream=None, sample=None):
        """gmk_selfplay_run: the handle's games are slots that play n_total whole games between them (continuous batching on the
        device).  open_moves uint8[n_total, stride] / open_lens int32[n_total] (host) or None; outputs are device pointers (ints),
        indexed by game.  sample = (plies, power): gmk_selfplay_run_sampled, the games advance(sample=) plays.  Returns the number of
        search launches it took."""
        played = C.c_int32()
        om = ol = None
        stride = 0
        if open_moves is not None:
            om = np.ascontiguousarray(open_moves, dtype=np.uint8)
            ol = np.ascontiguousarray(open_lens, dtype=np.int32)
            assert om.ndim == 2 and om.shape[0] == n_total and ol.shape == (n_total,)
            stride = om.shape[1]
        alpha, eps = root_noise if root_noise is not None else (0.0, 0.0)
        opening = (None if om is None else om.ctypes.data, stride, None if ol is None else ol.ctypes.data)
        if sample is None:
            _check(load().gmk_selfplay_run(self.h, int(n_total), int(first_game_id), int(playouts), int(reuse_subtree), float(alpha), float(eps),
                                           *opening, d_moves, d_visits, d_lens, d_winner, C.byref(played), stream))
        else:
            _check(load().gmk_selfplay_run_sampled(self.h, int(n_total), int(first_game_id), int(playouts), int(reuse_subtree), float(alpha), float(eps),
                                                   int(sample[0]), int(sample[1]), *opening, d_moves, d_visits, d_lens, d_winner, C.byref(played), stream))
        return played.value

    def ensemble_merge(self, group, visits=None, values=None, cells=None, cells_per_game=None, root_visits=None, root_value=None, status=None, stream=None):
        """gmk_mcts_ensemble_merge: the games read as n // group ensembles of `group` replicas, their root tables merged on the device into
        torch tensors on the GPU (any may be None): visits int32 / uint32 [E, 225], values float32 [E, 225], cells int16[E], cells_per_game
        int16[n], root_visits int32[E], root_value float32[E], status int32[E] (ENSEMBLE_* bits).  Asynchronous on the stream."""
        _ensemble_merge(load().gmk_mcts_ensemble_merge, self, group, visits, values, cells, cells_per_game, root_visits, root_value, status, stream)

    def alg_bytes(self):
        b = C.c_uint64()
        _check(load().gmk_mcts_alg_bytes(self.h, C.byref(b)))
        return b.value

    def launch_info(self):
        g, b, l = C.c_int(), C.c_int(), C.c_int()
        _check(load().gmk_mcts_launch_info(self.h, C.byref(g), C.byref(b), C.byref(l)))
        return {"grid": g.value, "block": b.value, "lds_bytes": l.value}


def visits_to_pi(visits, stones):
    v = np.ascontiguousarray(visits, dtype=np.uint32)
    pi = np.zeros(N, dtype=np.float32)
    _check(load().gmk_visits_to_pi(v.ctypes.data, int(stones), pi.ctypes.data))
    return pi


TARGET_VISITS, TARGET_POLICY = 0, 1             # GMK_TARGET_*: how a record's row becomes pi (K21: TARGET_POLICY for the rows of the Gumbel entries)
TARGETS = {"visits": TARGET_VISITS, "policy": TARGET_POLICY}


def _target(target):
    """"visits" / "policy" / None (visits) or a GMK_TARGET_* value -> the value; anything else is handed to the library, which refuses it"""
    return TARGET_VISITS if target is None else TARGETS[target] if isinstance(target, str) else int(target)


def samples_from_records(d_moves, d_lens, d_visits, d_winner, d_sample_game, d_sample_move, n_samples, augment,
                         d_states, d_values, d_pi, stream=None, target=None):
    """Device-pointer form of gmk_samples_from_records (K4 + K5); target: gmk_samples_from_records_target with that mode."""
    if target is None:
        _check(load().gmk_samples_from_records(d_moves, d_lens, d_visits, d_winner, d_sample_game, d_sample_move, n_samples,
                                               int(augment), d_states, d_values, d_pi, stream))
    else:
        _check(load().gmk_samples_from_records_target(d_moves, d_lens, d_visits, d_winner, d_sample_game, d_sample_move, n_samples,
                                                      int(augment), _target(target), d_states, d_values, d_pi, stream))


# ---------------- game records on the wire (device pointers; include/gomoku_hip.h) ----------------
WIRE_BAD_LENGTH, WIRE_BAD_SIZE = 1, 2       # the *d_status codes of records_pack / records_unpack


def records_scan(d_lens, n, d_offsets, stream=None):
    """gmk_records_scan: d_offsets int64[n+1] = exclusive prefix sum of d_lens (offsets[n] = -1 if a length is outside [0, 225])."""
    _check(load().gmk_records_scan(d_lens, int(n), d_offsets, stream))


def records_packed_bytes(d_offsets, n, has_visits, stream=None):
    """gmk_records_packed_bytes: the wire size 5n + T (1 + 450 has_visits); synchronises `stream`; raises on a length outside [0, 225]."""
    b = C.c_uint64()
    _check(load().gmk_records_packed_bytes(d_offsets, int(n), int(bool(has_visits)), C.byref(b), stream))
    return b.value


def records_pack(d_moves, d_lens, d_winner, d_visits, n, d_offsets, d_out, out_bytes, d_status, stream=None):
    """gmk_records_pack (d_visits None = no visit section); *d_status != 0: nothing was written."""
    _check(load().gmk_records_pack(d_moves, d_lens, d_winner, d_visits, int(n), d_offsets, d_out, int(out_bytes), d_status, stream))


def records_unpack(d_buf, n_bytes, n, has_visits, d_offsets, d_moves, d_lens, d_winner, d_visits, d_status, stream=None):
    """gmk_records_unpack: whole fixed-stride rows (zeros past each length); *d_status != 0: the records were not touched."""
    _check(load().gmk_records_unpack(d_buf, int(n_bytes), int(n), int(bool(has_visits)), d_offsets, d_moves, d_lens, d_winner, d_visits,
                                     d_status, stream))


def samples_from_packed(d_buf, n, d_offsets, d_sample_game, d_sample_move, n_samples, augment, d_states, d_values, d_pi, stream=None, target=None):
    """Device-pointer form of gmk_samples_from_packed (K4 + K5 on the wire form); target: gmk_samples_from_packed_target with that mode."""
    if target is None:
        _check(load().gmk_samples_from_packed(d_buf, int(n), d_offsets, d_sample_game, d_sample_move, int(n_samples), int(augment),
                                              d_states, d_values, d_pi, stream))
    else:
        _check(load().gmk_samples_from_packed_target(d_buf, int(n), d_offsets, d_sample_game, d_sample_move, int(n_samples), int(augment), _target(target),
                                                     d_states, d_values, d_pi, stream))


# ---------------- replay buffer (device pointers; include/gomoku_hip.h) ----------------
REPLAY_BAD_LENGTH, REPLAY_TOO_FEW, REPLAY_BAD_IMAGE, REPLAY_NO_ROOM = 1, 2, 3, 4      # the *d_status codes of replay append / sample / snapshot / restore


def replay_draw_host(seed, step, population, batch):
    """gmk_replay_draw_host: the population indices perm(0 .. batch-1) of the batch of (seed, step), int64[batch]; needs no GPU."""
    out = np.zeros(int(batch) if batch > 0 else 0, dtype=np.int64)
    _check(load().gmk_replay_draw_host(int(seed) & 0xFFFFFFFFFFFFFFFF, int(step), int(population), int(batch), out.ctypes.data))
    return out


def replay_image_check_host(image):
    """gmk_replay_image_check_host on a buffer image (bytes, or a uint8 numpy array): -> {"games", "plies", "population", "head"}.
    Raises ValueError, naming the broken rule, if the image is not valid, and GmkError if it has fewer than 64 bytes; needs no GPU."""
    image = np.ascontiguousarray(np.frombuffer(image, dtype=np.uint8) if isinstance(image, (bytes, bytearray, memoryview)) else image)
    if image.dtype != np.uint8 or image.ndim != 1:
        raise ValueError("replay_image_check_host: the image must be a flat uint8 array")
    info = np.zeros(5, dtype=np.int64)
    rc = load().gmk_replay_image_check_host(image.ctypes.data, int(image.size), info.ctypes.data)
    if rc == REPLAY_BAD_IMAGE:
        raise ValueError(load().gmk_last_error().decode())
    _check(rc)
    return {"games": int(info[0]), "plies": int(info[1]), "population": int(info[2]), "head": int(info[3])}


class ReplayHandle:
    """A gmk_replay handle: game records in HBM (ring of plies, ring of visit rows, ring of game descriptors); device pointers as ints."""

    def __init__(self, capacity_plies, max_games, seed=DEFAULT_SEED):
        init()
        h = C.c_void_p()
        _check(load().gmk_replay_create(int(capacity_plies), int(max_games), int(seed) & 0xFFFFFFFFFFFFFFFF, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None) and load is not None:
            load().gmk_replay_destroy(self.h)
            self.h = None

    __del__ = close

    def reset(self, stream=None):
        _check(load().gmk_replay_reset(self.h, stream))

    def append(self, d_moves, d_lens, d_winner, d_visits, n, first_move, d_status, stream=None):
        _check(load().gmk_replay_append(self.h, d_moves, d_lens, d_winner, d_visits, int(n), int(first_move), d_status, stream))

    def append_packed(self, d_buf, n, d_offsets, first_move, d_status, stream=None):
        _check(load().gmk_replay_append_packed(self.h, d_buf, int(n), d_offsets, int(first_move), d_status, stream))

    def size(self, stream=None):
        """-> (games, stored plies, sampled plies, evicted games); synchronises `stream`."""
        v = [C.c_int64() for _ in range(4)]
        _check(load().gmk_replay_size(self.h, *[C.byref(x) for x in v], stream))
        return tuple(x.value for x in v)

    def sample(self, batch, step, augment, states_float, d_states, d_values, d_pi, d_picked, d_status, stream=None, target=None):
        """gmk_replay_sample; target ("visits" / "policy" / a TARGET_* value): gmk_replay_sample_target with that mode."""
        if target is None:
            _check(load().gmk_replay_sample(self.h, int(batch), int(step), int(bool(augment)), int(bool(states_float)), d_states, d_values, d_pi,
                                            d_picked, d_status, stream))
        else:
            _check(load().gmk_replay_sample_target(self.h, int(batch), int(step), int(bool(augment)), _target(target), int(bool(states_float)), d_states, d_values,
                                                   d_pi, d_picked, d_status, stream))

    def image_bytes(self, stream=None):
        """The size of the image of what is held now; synchronises `stream`."""
        v = C.c_int64()
        _check(load().gmk_replay_image_bytes(self.h, C.byref(v), stream))
        return v.value

    def snapshot(self, d_image, capacity_bytes, d_status, stream=None):
        """gmk_replay_snapshot: the image into d_image (8-byte aligned); *d_status = REPLAY_NO_ROOM: nothing was written.  Drains `stream` once."""
        _check(load().gmk_replay_snapshot(self.h, d_image, int(capacity_bytes), d_status, stream))

    def restore(self, d_image, n_bytes, d_status, stream=None):
        """gmk_replay_restore: the image's games replace what is held; *d_status = REPLAY_BAD_IMAGE / REPLAY_NO_ROOM: nothing changed.
        Drains `stream` once."""
        _check(load().gmk_replay_restore(self.h, d_image, int(n_bytes), d_status, stream))


# ---------------- K11: the trainer (device pointers; include/gomoku_hip.h) ----------------
# the sixteen tensors: (name, shape) in the ARGUMENT order of gmk_train_create / gmk_train_params (gmk_pvnet_create's ten, gmk_pvnet_set_dense's six)
TRAIN_TENSORS = (("w1", (32, 6, 3, 3)), ("b1", (32,)), ("w2", (64, 32, 3, 3)), ("b2", (64,)), ("w3", (128, 64, 3, 3)), ("b3", (128,)),
                 ("w_policy_conv", (4, 128)), ("b_policy_conv", (4,)), ("w_value_conv", (2, 128)), ("b_value_conv", (2,)),
                 ("w_policy", (225, 900)), ("b_policy", (225,)), ("w_hidden", (64, 450)), ("b_hidden", (64,)), ("w_out", (64,)), ("b_out", (1,)))
# ... and their order inside a block (d_grads, the moments): the two 1x1 heads side by side
TRAIN_BLOCK_ORDER = ("w1", "b1", "w2", "b2", "w3", "b3", "w_policy_conv", "w_value_conv", "b_policy_conv", "b_value_conv",
                     "w_policy", "b_policy", "w_hidden", "b_hidden", "w_out", "b_out")
TRAIN_BIASES = tuple(name for name, _ in TRAIN_TENSORS if name.startswith("b"))
TRAIN_PARAMS = sum(int(np.prod(shape)) for _, shape in TRAIN_TENSORS)
BLOCK_PARAMS, BLOCK_M, BLOCK_V, BLOCK_UPDATE = 0, 1, 2, 3


def split_block(block):
    """A block in TRAIN_BLOCK_ORDER (numpy or torch, 1-D) -> {name: view of the tensor's shape}."""
    shapes, out, at = dict(TRAIN_TENSORS), {}, 0
    for name in TRAIN_BLOCK_ORDER:
        size = int(np.prod(shapes[name]))
        out[name] = block[at:at + size].reshape(shapes[name])
        at += size
    assert at == TRAIN_PARAMS == block.shape[0]
    return out


def join_block(tensors):
    """{name: array} -> one float32 numpy block in TRAIN_BLOCK_ORDER."""
    shapes = dict(TRAIN_TENSORS)
    parts = [np.ascontiguousarray(np.asarray(tensors[name], dtype=np.float32)).reshape(-1) for name in TRAIN_BLOCK_ORDER]
    assert all(p.size == int(np.prod(shapes[name])) for p, name in zip(parts, TRAIN_BLOCK_ORDER))
    return np.concatenate(parts)


class TrainerHandle:
    """A gmk_trainer handle: the parameters, Adam's moments and the activations of up to max_batch positions in HBM; device pointers as ints."""

    def __init__(self, arrays, max_batch):
        """arrays: {name: float32 array} for every name of TRAIN_TENSORS."""
        init()
        host = self._host(arrays)
        h = C.c_void_p()
        _check(load().gmk_train_create(*[a.ctypes.data for a in host], int(max_batch), C.byref(h)))
        self.h, self.max_batch = h, int(max_batch)

    @staticmethod
    def _host(arrays):
        host = [np.ascontiguousarray(np.asarray(arrays[name], dtype=np.float32)) for name, _ in TRAIN_TENSORS]
        for a, (name, shape) in zip(host, TRAIN_TENSORS):
            if a.size != int(np.prod(shape)):
                raise ValueError("TrainerHandle: %s must hold %d floats" % (name, int(np.prod(shape))))
        return host

    def close(self):
        if getattr(self, "h", None) and load is not None:
            load().gmk_train_destroy(self.h)
            self.h = None

    __del__ = close

    def forward(self, d_states, n, d_value, d_probs, stream=None):
        _check(load().gmk_train_forward(self.h, d_states, int(n), d_value, d_probs, stream))

    def grads(self, d_states, d_values, d_pi, n, d_grads, d_metrics, stream=None):
        _check(load().gmk_train_grads(self.h, d_states, d_values, d_pi, int(n), d_grads, d_metrics, stream))

    def step(self, d_states, d_values, d_pi, n, lr, d_old_probs, d_probs_out, d_metrics, stream=None):
        _check(load().gmk_train_step(self.h, d_states, d_values, d_pi, int(n), float(lr), d_old_probs, d_probs_out, d_metrics, stream))

    def params(self):
        """-> {name: float32 array}; synchronises the device."""
        out = {name: np.empty(shape, dtype=np.float32) for name, shape in TRAIN_TENSORS}
        _check(load().gmk_train_params(self.h, *[out[name].ctypes.data for name, _ in TRAIN_TENSORS]))
        return out

    def set_params(self, arrays):
        host = self._host(arrays)
        _check(load().gmk_train_set_params(self.h, *[a.ctypes.data for a in host]))

    def get_block(self, which):
        out = np.empty(TRAIN_PARAMS, dtype=np.float32)
        _check(load().gmk_train_get_block(self.h, int(which), out.ctypes.data))
        return out

    def set_block(self, which, block):
        block = np.ascontiguousarray(np.asarray(block, dtype=np.float32)).reshape(-1)
        if block.size != TRAIN_PARAMS:
            raise ValueError("TrainerHandle.set_block: a block holds %d floats" % TRAIN_PARAMS)
        _check(load().gmk_train_set_block(self.h, int(which), block.ctypes.data))

    def set_step_count(self, step):
        _check(load().gmk_train_set_step_count(self.h, int(step)))

    def export(self, pvnet_handle, stream=None):
        _check(load().gmk_train_export(self.h, pvnet_handle, stream))

    def info(self):
        """-> {"step", "scratch_bytes", "max_batch", "param_floats"}"""
        step, scratch, mb, pf = C.c_int64(), C.c_int64(), C.c_int32(), C.c_int32()
        _check(load().gmk_train_info(self.h, C.byref(step), C.byref(scratch), C.byref(mb), C.byref(pf)))
        return {"step": step.value, "scratch_bytes": scratch.value, "max_batch": mb.value, "param_floats": pf.value}


# K11's kernels on their own (gmk_train_kernel_*): a buffer is a float32 torch tensor on the device, or a device pointer as an int
TRAIN_GEMM_NONE = 2 ** 31 - 1          # cq / nsplit: "no grouping" / "no split", as the trainer's own descriptors have them
_GEMM_BUFFERS = {"A": "a_floats", "B": "b_floats", "part": "part_floats", "C": "c_floats", "C2": "c2_floats", "bias": "bias_floats", "mask": "mask_floats"}


def _dev_ptr(buf):
    if buf is None:
        return None
    return int(buf.data_ptr()) if hasattr(buf, "data_ptr") else int(buf)


def train_gemm_desc(**fields):
    """-> TrainGemmDesc.  Buffers (A, B, part, C, C2, bias, mask) are torch tensors -- the extent is then what is left of the tensor's storage
    from its first element on -- or device pointers as ints with the `*_floats` field given.  Defaults: one k slab that holds every k, no
    grouping, no split, no bias, no ReLU, no mask: the direct form as the trainer's gemm() sets it up."""
    d = TrainGemmDesc()
    d.kslab, d.nz, d.cq, d.nsplit = max(int(fields.get("K", 1)), 1), 1, TRAIN_GEMM_NONE, TRAIN_GEMM_NONE
    for name, value in fields.items():
        if name in _GEMM_BUFFERS:
            setattr(d, name, _dev_ptr(value))
            if hasattr(value, "data_ptr") and _GEMM_BUFFERS[name] not in fields:
                setattr(d, _GEMM_BUFFERS[name], value.untyped_storage().nbytes() // 4 - value.storage_offset())
        else:
            setattr(d, name, int(value))
    return d


def train_kernel_gemm(desc, stream=None):
    """train_gemm_kernel through the trainer's launcher; GmkError (status -3, the field named) if the descriptor's addressing does not fit."""
    _check(load().gmk_train_kernel_gemm(C.byref(desc), stream))


def train_kernel_reduce(part, nz, mn, out, stream=None):
    _check(load().gmk_train_kernel_reduce(_dev_ptr(part), int(nz), int(mn), _dev_ptr(out), stream))


def train_kernel_im2col(inp, in_floats, sb, sp, sc, channels, npos, col, stream=None):
    _check(load().gmk_train_kernel_im2col(_dev_ptr(inp), int(in_floats), int(sb), int(sp), int(sc), int(channels), int(npos), _dev_ptr(col), stream))


def train_kernel_col2im(dcol, channels, npos, mask, out, stream=None):
    _check(load().gmk_train_kernel_col2im(_dev_ptr(dcol), int(channels), int(npos), _dev_ptr(mask), _dev_ptr(out), stream))


# ---------------- K2: incrementally maintained evaluator states ----------------
class EvaluatorStates:
    """n_games device-resident Evaluator objects (gmk_evalstate_*): apply / revert moves, read the members back."""

    APPLY_NONE, REVERT = -1, -2

    def __init__(self, n_games):
        init()
        self.n = n_games
        h = C.c_void_p()
        _check(load().gmk_evalstate_create(n_games, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None) and load is not None:
            load().gmk_evalstate_destroy(self.h)
            self.h = None

    __del__ = close

    def reset(self):
        _check(load().gmk_evalstate_reset(self.h))

    def update(self, moves):
        """moves int16[n, k]: per game k entries (cell >= 0 apply, -1 nothing, -2 revert the last move)."""
        moves = np.ascontiguousarray(moves, dtype=np.int16)
        assert moves.ndim == 2 and moves.shape[0] == self.n
        _check(load().gmk_evalstate_update_host(self.h, moves.ctypes.data, moves.shape[1]))

    def read(self):
        out = {"scores": np.zeros((self.n, 4, N), np.int32), "density": np.zeros((self.n, 2, 2, N), np.int32),
               "pattern_dist": np.zeros((self.n, 226, 8), np.uint32), "compound_dist": np.zeros((self.n, 226, 3), np.uint32),
               "meta": np.zeros((self.n, 4), np.int32), "record": np.zeros((self.n, 228), np.uint8)}
        _check(load().gmk_evalstate_read(self.h, out["scores"].ctypes.data, out["density"].ctypes.data, out["pattern_dist"].ctypes.data,
                                         out["compound_dist"].ctypes.data, out["meta"].ctypes.data, out["record"].ctypes.data))
        return out


# ---------------- K10: the pattern heuristic on its own (EvaluationProbs, DecisiveFilter, EvaluationValue) ----------------
PATTERN_OVER, PATTERN_EVALUATOR_ERROR, PATTERN_ILLEGAL, PATTERN_STALLED = 1, 2, 4, 8      # status bits of gmk_pattern_policy / gmk_pattern_play


def _move_lists(moves, lens):
    """The host front ends' move lists: moves u8[n, stride] and lens i32[n], contiguous -> (moves, lens, n, stride); the library is initialised."""
    init()
    moves = np.ascontiguousarray(moves, dtype=np.uint8)
    lens = np.ascontiguousarray(lens, dtype=np.int32)
    assert moves.ndim == 2 and lens.shape == (moves.shape[0],)
    return (moves, lens) + moves.shape


def pattern_policy(moves, lens, filter=True):
    """moves u8[n, stride] (host), lens i32[n]: one move list per position, black first -> {"probs" f32[n,225], "value" f32[n], "best" i32[n],
    "status" i32[n]} for the player to move: what PatternEvalAgent (filter=True) or MaxEvaluatedRollout (filter=False) sees there.
    Runs on the GPU through gmk_pattern_policy_host; raises without one."""
    moves, lens, n, stride = _move_lists(moves, lens)
    out = {"probs": np.zeros((n, N), np.float32), "value": np.zeros(n, np.float32), "best": np.zeros(n, np.int32), "status": np.zeros(n, np.int32)}
    _check(load().gmk_pattern_policy_host(moves.ctypes.data, stride, lens.ctypes.data, n, int(bool(filter)),
                                          out["probs"].ctypes.data, out["value"].ctypes.data, out["best"].ctypes.data, out["status"].ctypes.data))
    return out


def pattern_policy_device(d_moves, stride, d_lens, n, filter=True, d_probs=None, d_value=None, d_best=None, d_status=None, stream=None):
    """Device-pointer form (ints, e.g. torch.Tensor.data_ptr()) of gmk_pattern_policy; asynchronous on `stream`."""
    _check(load().gmk_pattern_policy(d_moves, int(stride), d_lens, int(n), int(bool(filter)), d_probs, d_value, d_best, d_status, stream))


def pattern_play(d_moves, d_lens, n, filter=True, max_moves=0, d_winner=None, d_values=None, d_status=None, stream=None):
    """gmk_pattern_play: the n openings in d_moves u8[n,225] / d_lens i32[n] (device pointers) are played out greedily in one launch."""
    _check(load().gmk_pattern_play(d_moves, d_lens, int(n), int(bool(filter)), int(max_moves), d_winner, d_values, d_status, stream))


# ---------------- K23: the pattern heuristic for rows of network planes (include/gomoku_pattern_states.h) ----------------
PATTERN_NORM_L2, PATTERN_NORM_SUM = 0, 1                     # GMK_PATTERN_NORM_*
PATTERN_NORMS = {"l2": PATTERN_NORM_L2, "sum": PATTERN_NORM_SUM}


def _pattern_norm(norm):
    if norm in PATTERN_NORMS:
        return PATTERN_NORMS[norm]
    if norm in (PATTERN_NORM_L2, PATTERN_NORM_SUM) and not isinstance(norm, bool):
        return int(norm)
    raise ValueError("norm is 'l2' or 'sum', not %r" % (norm,))


def _state_rows(states):
    """Host rows of planes: anything of n x 6 x 225 float32 values -> (contiguous f32[n, 6, 225], n)."""
    states = np.ascontiguousarray(states, dtype=np.float32)
    if states.size % (6 * N) or (states.ndim < 2 and states.size):
        raise ValueError("states hold n x 6 x 225 values")
    states = states.reshape(-1, 6, N)
    return states, states.shape[0]


def pattern_evaluate_states(states, filter=True, norm="sum", value=None, probs=None, status=None, stream=None):
    """gmk_pattern_evaluate_states on torch tensors on the GPU: states f32 [n, 6, 15, 15] (or [n, 6, 225]), contiguous -> (value f32[n],
    probs f32[n, 225], status i32[n]).  Outputs that are passed in are written in place (status=False: no status is asked for and None is
    returned for it).  Asynchronous on `stream` (an int handle; None: torch's current stream); nothing is synchronised."""
    import torch
    norm = _pattern_norm(norm)
    if not (isinstance(states, torch.Tensor) and states.is_cuda and states.dtype == torch.float32 and states.is_contiguous()):
        raise ValueError("states is a contiguous float32 tensor on the GPU")
    if states.numel() % (6 * N) or (states.dim() < 2 and states.numel()):
        raise ValueError("states hold n x 6 x 225 values")
    n = states.numel() // (6 * N)
    init()
    dev = states.device
    if value is None:
        value = torch.empty(n, dtype=torch.float32, device=dev)
    if probs is None:
        probs = torch.empty((n, N), dtype=torch.float32, device=dev)
    if status is None:
        status = torch.empty(n, dtype=torch.int32, device=dev)
    elif status is False:
        status = None
    for t, dt, count in ((value, torch.float32, n), (probs, torch.float32, n * N), (status, torch.int32, n)):
        if t is not None and not (t.is_cuda and t.dtype == dt and t.is_contiguous() and t.numel() >= count):
            raise ValueError("the outputs are contiguous GPU tensors: value f32[n], probs f32[n, 225], status i32[n]")
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    _check(load().gmk_pattern_evaluate_states(states.data_ptr(), n, int(bool(filter)), norm, value.data_ptr(), probs.data_ptr(),
                                              None if status is None else status.data_ptr(), stream))
    return value, probs, status


def pattern_evaluate_states_host(states, filter=True, norm="sum"):
    """gmk_pattern_evaluate_states_host: host rows f32 [n, 6, 225] -> {"value" f32[n], "probs" f32[n, 225], "status" i32[n]}.  Runs on the GPU;
    raises without one."""
    norm = _pattern_norm(norm)
    states, n = _state_rows(states)
    init()
    out = {"value": np.zeros(n, np.float32), "probs": np.zeros((n, N), np.float32), "status": np.zeros(n, np.int32)}
    _check(load().gmk_pattern_evaluate_states_host(states.ctypes.data, n, int(bool(filter)), norm, out["value"].ctypes.data, out["probs"].ctypes.data,
                                                   out["status"].ctypes.data))
    return out


def pattern_states_list_host(states):
    """gmk_pattern_states_list_host: the canonical move lists of host rows f32 [n, 6, 225] -> (moves u8[n, 225], zero past the length, lens i32[n],
    status i32[n] = 0 or PATTERN_ILLEGAL).  Needs no GPU and no init()."""
    states, n = _state_rows(states)
    moves, lens, status = np.zeros((n, N), np.uint8), np.zeros(n, np.int32), np.zeros(n, np.int32)
    _check(load().gmk_pattern_states_list_host(states.ctypes.data, n, moves.ctypes.data, lens.ctypes.data, status.ctypes.data))
    return moves, lens, status


def pattern_states_finish_host(vec, states, norm="sum"):
    """gmk_pattern_states_finish_host: K10's vectors f32[n, 225] of the rows' canonical lists -> the priors f32[n, 225] under `norm` (a row that is
    no position: zeros).  Needs no GPU and no init()."""
    norm = _pattern_norm(norm)
    states, n = _state_rows(states)
    vec = np.ascontiguousarray(vec, dtype=np.float32)
    if vec.shape != (n, N):
        raise ValueError("vec is f32[n, 225], one row per row of states")
    probs = np.zeros((n, N), np.float32)
    _check(load().gmk_pattern_states_finish_host(vec.ctypes.data, states.ctypes.data, n, norm, probs.ctypes.data))
    return probs


# ---------------- K14: the forced-win solver by continuous fours (gmk_vcf_solve) ----------------
VCF_NONE, VCF_WIN, VCF_DEPTH, VCF_BUDGET, VCF_OVER, VCF_BAD = 0, 1, 2, 3, 4, 5      # the status of a position (include/gomoku_hip.h)
VCF_STATUS_NAMES = ("NONE", "WIN", "DEPTH", "BUDGET", "OVER", "BAD")
VCF_OPPONENT, VCF_ITERATIVE = 1, 2                                                 # flags
VCF_MAX_DEPTH, VCF_PV = 32, 64


def _vcf_flags(opponent, iterative):
    return (VCF_OPPONENT if opponent else 0) | (VCF_ITERATIVE if iterative else 0)


def vcf_solve(moves, lens, max_depth=16, budget=100000, opponent=False, iterative=False):
    """moves u8[n, stride] (host), lens i32[n]: one move list per position, black first -> {"status" i32[n], "move" i32[n], "length" i32[n],
    "nodes" u32[n], "pv" u8[n, 64]}: is there a forced win by continuous fours for the side to move (opponent=True: for the other side, moving
    first), within max_depth attacker moves and `budget` four-making candidates?  Exact; the contract is in include/gomoku_hip.h.
    Runs on the GPU through gmk_vcf_solve_host; raises without one."""
    moves, lens, n, stride = _move_lists(moves, lens)
    out = {"status": np.zeros(n, np.int32), "move": np.zeros(n, np.int32), "length": np.zeros(n, np.int32), "nodes": np.zeros(n, np.uint32),
           "pv": np.full((n, VCF_PV), 255, np.uint8)}
    if n:
        _check(load().gmk_vcf_solve_host(moves.ctypes.data, stride, lens.ctypes.data, n, int(max_depth), int(budget), _vcf_flags(opponent, iterative),
                                         out["status"].ctypes.data, out["move"].ctypes.data, out["length"].ctypes.data, out["nodes"].ctypes.data,
                                         out["pv"].ctypes.data))
    return out


def vcf_solve_device(d_moves, stride, d_lens, n, max_depth=16, budget=100000, opponent=False, iterative=False,
                     d_status=None, d_move=None, d_length=None, d_nodes=None, d_pv=None, stream=None):
    """Device-pointer form (ints, e.g. torch.Tensor.data_ptr()) of gmk_vcf_solve; asynchronous on `stream`, allocates nothing."""
    _check(load().gmk_vcf_solve(d_moves, int(stride), d_lens, int(n), int(max_depth), int(budget), _vcf_flags(opponent, iterative),
                                d_status, d_move, d_length, d_nodes, d_pv, stream))


# ---------------- K15: the moves that refute a forced win by continuous fours (gmk_vcf_defend) ----------------
VCF_CELL_NONE, VCF_CELL_HOLDS, VCF_CELL_LOSES, VCF_CELL_UNKNOWN, VCF_CELL_FIVE = 0, 1, 2, 3, 4      # the verdict of a cell (include/gomoku_hip.h)
VCF_CELL_NAMES = ("NONE", "HOLDS", "LOSES", "UNKNOWN", "FIVE")


def vcf_defend(moves, lens, max_depth=16, budget=100000, iterative=False):
    """moves u8[n, stride] (host), lens i32[n]: one move list per position, black first -> the threat against the side to move, which is
    vcf_solve(opponent=True) ("threat_status" i32[n], "threat_length" i32[n], "threat_pv" u8[n, 64], "threat_nodes" u32[n]), and for each of
    the 225 cells what a stone of the side to move there does about it: "verdict" u8[n, 225] (VCF_CELL_*), "length" u8[n, 225] (the
    attacker's moves where the cell LOSES) and "nodes" u32[n, 225] (the candidates tried where the cell was searched).  Exact; the contract is
    in include/gomoku_hip.h ("K15").  Runs on the GPU through gmk_vcf_defend_host; raises without one."""
    moves, lens, n, stride = _move_lists(moves, lens)
    out = {"threat_status": np.zeros(n, np.int32), "threat_length": np.zeros(n, np.int32), "threat_pv": np.full((n, VCF_PV), 255, np.uint8),
           "threat_nodes": np.zeros(n, np.uint32), "verdict": np.zeros((n, 225), np.uint8), "length": np.zeros((n, 225), np.uint8),
           "nodes": np.zeros((n, 225), np.uint32)}
    if n:
        _check(load().gmk_vcf_defend_host(moves.ctypes.data, stride, lens.ctypes.data, n, int(max_depth), int(budget), _vcf_flags(False, iterative),
                                          out["threat_status"].ctypes.data, out["threat_length"].ctypes.data, out["threat_pv"].ctypes.data,
                                          out["threat_nodes"].ctypes.data, out["verdict"].ctypes.data, out["length"].ctypes.data,
                                          out["nodes"].ctypes.data))
    return out


def vcf_defend_device(d_moves, stride, d_lens, n, max_depth=16, budget=100000, iterative=False, d_threat_status=None, d_threat_length=None,
                      d_threat_pv=None, d_threat_nodes=None, d_verdict=None, d_cell_length=None, d_cell_nodes=None, stream=None):
    """Device-pointer form (ints, e.g. torch.Tensor.data_ptr()) of gmk_vcf_defend; asynchronous on `stream`, allocates nothing.  The threat's
    status, length and pv and the verdicts are required."""
    _check(load().gmk_vcf_defend(d_moves, int(stride), d_lens, int(n), int(max_depth), int(budget), _vcf_flags(False, iterative),
                                 d_threat_status, d_threat_length, d_threat_pv, d_threat_nodes, d_verdict, d_cell_length, d_cell_nodes, stream))


# ---------------- K17: what a stone of the side to move threatens (gmk_vcf_threats), and the forced win by threats (gmk_vct_solve) ----------------
VCF_THREAT_NONE, VCF_THREAT_QUIET, VCF_THREAT_WINS, VCF_THREAT_UNKNOWN, VCF_THREAT_FIVE, VCF_THREAT_FOUR, VCF_THREAT_IGNORES = 0, 1, 2, 3, 4, 5, 6
VCF_THREAT_NAMES = ("NONE", "QUIET", "WINS", "UNKNOWN", "FIVE", "FOUR", "IGNORES")
VCT_MAX_THREATS, VCT_PV = 8, 80
VCT_BUDGET = 6                                                                      # a status of vct_solve beside the VCF_* ones
VCT_STATUS_NAMES = VCF_STATUS_NAMES + ("VCT_BUDGET",)


def vcf_threats(moves, lens, max_depth=16, budget=100000, iterative=False):
    """moves u8[n, stride] (host), lens i32[n]: one move list per position, black first -> the own verdict of the side to move, which is
    vcf_solve's ("own_status" i32[n], "own_move" i32[n], "own_length" i32[n], "own_nodes" u32[n], "own_pv" u8[n, 64]), and for each of the 225
    cells what a stone of the side to move there threatens: "verdict" u8[n, 225] (VCF_THREAT_*), "length" u8[n, 225] (the moves of the win by
    fours that a WINS cell threatens; 1 or 2 for a FOUR) and "nodes" u32[n, 225] (the candidates tried where the cell was searched).  Exact;
    the contract is in include/gomoku_hip.h ("K17").  Runs on the GPU through gmk_vcf_threats_host; raises without one."""
    moves, lens, n, stride = _move_lists(moves, lens)
    out = {"own_status": np.zeros(n, np.int32), "own_move": np.zeros(n, np.int32), "own_length": np.zeros(n, np.int32),
           "own_nodes": np.zeros(n, np.uint32), "own_pv": np.full((n, VCF_PV), 255, np.uint8), "verdict": np.zeros((n, 225), np.uint8),
           "length": np.zeros((n, 225), np.uint8), "nodes": np.zeros((n, 225), np.uint32)}
    if n:
        _check(load().gmk_vcf_threats_host(moves.ctypes.data, stride, lens.ctypes.data, n, int(max_depth), int(budget), _vcf_flags(False, iterative),
                                           *[out[k].ctypes.data for k in ("own_status", "own_move", "own_length", "own_nodes", "own_pv", "verdict",
                                                                          "length", "nodes")]))
    return out


def vcf_threats_device(d_moves, stride, d_lens, n, max_depth=16, budget=100000, iterative=False, d_own_status=None, d_own_move=None,
                       d_own_length=None, d_own_nodes=None, d_own_pv=None, d_verdict=None, d_cell_length=None, d_cell_nodes=None, stream=None):
    """Device-pointer form (ints, e.g. torch.Tensor.data_ptr()) of gmk_vcf_threats; asynchronous on `stream`, allocates nothing.  The own
    status and the verdicts are required."""
    _check(load().gmk_vcf_threats(d_moves, int(stride), d_lens, int(n), int(max_depth), int(budget), _vcf_flags(False, iterative),
                                  d_own_status, d_own_move, d_own_length, d_own_nodes, d_own_pv, d_verdict, d_cell_length, d_cell_nodes, stream))


def vct_solve(moves, lens, max_depth=16, budget=100000, iterative=False, max_threats=1, max_positions=4096):
    """moves u8[n, stride] (host), lens i32[n]: one move list per root, black first -> {"status" i32[n] (VCF_* or VCT_BUDGET), "move" i32[n],
    "threats" i32[n], "positions" u32[n], "pv" u8[n, 80]}: does the side to move have a forced win by continuous threats, at most max_threats
    moves that threaten a win by fours (each answered by every reply that holds) and then a win by fours?  max_depth, budget and iterative are
    those of every inner vcf_solve; max_positions caps the positions of one root on one level.  Exact; the contract is in
    include/gomoku_hip.h ("K17").  Runs on the GPU through gmk_vct_solve_host; raises without one."""
    moves, lens, n, stride = _move_lists(moves, lens)
    out = {"status": np.zeros(n, np.int32), "move": np.full(n, -1, np.int32), "threats": np.zeros(n, np.int32), "positions": np.zeros(n, np.uint32),
           "pv": np.full((n, VCT_PV), 255, np.uint8)}
    if n:
        _check(load().gmk_vct_solve_host(moves.ctypes.data, stride, lens.ctypes.data, n, int(max_depth), int(budget), _vcf_flags(False, iterative),
                                         int(max_threats), int(max_positions), *[out[k].ctypes.data for k in ("status", "move", "threats", "positions", "pv")]))
    return out


def vct_solve_device(d_moves, stride, d_lens, n, max_depth=16, budget=100000, iterative=False, max_threats=1, max_positions=4096,
                     d_status=None, d_move=None, d_threats=None, d_positions=None, d_pv=None, stream=None):
    """Device-pointer form (ints, e.g. torch.Tensor.data_ptr()) of gmk_vct_solve.  It allocates its workspace and synchronises `stream`
    between the levels: when it returns, the outputs are written."""
    _check(load().gmk_vct_solve(d_moves, int(stride), d_lens, int(n), int(max_depth), int(budget), _vcf_flags(False, iterative), int(max_threats),
                                int(max_positions), d_status, d_move, d_threats, d_positions, d_pv, stream))


# ---------------- K12: the referee of a match between two search handles (gmk_match_referee) and what its callers share ----------------
MATCH_MOVED, MATCH_REFUSED, MATCH_ENDED, MATCH_OVER = 0, 1, 2, 3      # the referee's verdicts (include/gomoku_hip.h)
MATCH_STATUS_REFUSED, MATCH_STATUS_BAD_ROW = 1, 2                      # bits of the referee's status words


def _current_stream(stream):
    import torch
    return torch.cuda.current_stream().cuda_stream if stream is None else stream


def noise_mix_rows(priors, game_ids, stones, alpha, epsilon, seed, draws=None, stream=None):
    """gmk_noise_mix_rows, a diagnostic entry: Default::AddNoise with the counter-based sampler on n rows of priors by cell, in place, one
    wavefront per row, on `stream` (default: torch's current stream); the call does not wait.  priors float32[n, 225] (0: no child), game_ids and
    stones uint32[n] (any 4-byte integer tensor: the bits count), draws None or float32[n, 225] for the gamma variates before the normalisation;
    all on the device and contiguous.  alpha finite and > 0, 0 <= epsilon <= 1, else GmkError."""
    import torch
    n = priors.shape[0]
    assert priors.is_cuda and priors.dtype == torch.float32 and tuple(priors.shape) == (n, N) and priors.is_contiguous()
    for ids in (game_ids, stones):
        assert ids.is_cuda and ids.element_size() == 4 and tuple(ids.shape) == (n,) and ids.is_contiguous()
    assert draws is None or (draws.is_cuda and draws.dtype == torch.float32 and tuple(draws.shape) == (n, N) and draws.is_contiguous())
    _check(load().gmk_noise_mix_rows(priors.data_ptr(), None if draws is None else draws.data_ptr(), game_ids.data_ptr(), stones.data_ptr(), n,
                                     float(alpha), float(epsilon), int(seed) & 0xFFFFFFFFFFFFFFFF, _current_stream(stream)))


def _root_choice(entry, tree, cells, visits, stream):
    import torch
    assert cells.is_cuda and cells.dtype == torch.int16 and cells.shape == (tree.n,) and cells.is_contiguous()
    assert visits is None or (visits.is_cuda and visits.element_size() == 2 and visits.shape == (tree.n, N) and visits.is_contiguous())
    _check(entry(tree.h, cells.data_ptr(), None if visits is None else visits.data_ptr(), _current_stream(stream)))


def _sample_args(sample):
    """sample = (plies, power, seed, first_game_id) -> the four arguments of the sampled entries"""
    plies, power, seed, first_game_id = sample
    return int(plies), int(power), int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_game_id) & 0xFFFFFFFF


def move_sample_host(visits, stones, game_ids, plies, power, seed, proofs=None):
    """gmk_move_sample_host: the cell each of n roots plays under the sampling rule of include/gomoku_sample.h, int16[n] (-1: none); needs no
    GPU.  visits uint32[n, 225] by cell, not saturated (root_stats()["visits"]); stones int32[n] on the root boards; game_ids uint32[n], GLOBAL
    (first_game_id + the game's number); plies, power: a root with fewer than `plies` stones is drawn in proportion to visits^power (1..3), any
    other plays the most visited child; proofs int8[n, 225] (AlphaZeroMCTS.root_proofs()["children"]) or None."""
    visits = np.ascontiguousarray(visits, dtype=np.uint32)
    n = visits.shape[0]
    stones = np.ascontiguousarray(stones, dtype=np.int32)
    game_ids = np.ascontiguousarray(game_ids, dtype=np.uint32)
    assert visits.shape == (n, N) and stones.shape == (n,) and game_ids.shape == (n,)
    if proofs is not None:
        proofs = np.ascontiguousarray(proofs, dtype=np.int8)
        assert proofs.shape == (n, N)
    cells = np.zeros(n, dtype=np.int16)
    _check(load().gmk_move_sample_host(visits.ctypes.data, None if proofs is None else proofs.ctypes.data, stones.ctypes.data, game_ids.ctypes.data, n,
                                       int(plies), int(power), int(seed) & 0xFFFFFFFFFFFFFFFF, cells.ctypes.data))
    return cells


# ---------------- K21: the Gumbel root rule on the host (include/gomoku_gumbel.h; no GPU) ----------------
GUMBEL_MAX_SIMS = 4096
GUMBEL_C_VISIT, GUMBEL_C_SCALE = 50.0, 1.0      # the paper's; parameters, not tuned here


def _rows(a, dtype, n=None, width=N):
    a = np.ascontiguousarray(a, dtype=dtype)
    assert a.ndim == (2 if width else 1) and (n is None or a.shape[0] == n) and (not width or a.shape[1] == width), a.shape
    return a


def gumbel_sequence_host(m_eff, n_sims):
    """gmk_gumbel_sequence_host: the sequential-halving schedule seq[0 .. n_sims) for m_eff considered children, uint32[n_sims]."""
    seq = np.zeros(max(int(n_sims), 0), dtype=np.uint32)
    _check(load().gmk_gumbel_sequence_host(int(m_eff), int(n_sims), seq.ctypes.data))
    return seq


def gumbel_setup_host(prior, visits, stones, game_ids, max_considered, seed):
    """gmk_gumbel_setup_host: the set-up of n roots given by rows by cell (prior float32[n, 225], 0 = no child; visits uint32[n, 225]; stones
    int32[n]; game_ids uint32[n], GLOBAL) -> {"draws" float64[n, 225] (g_c of every cell), "score" float64[n, 225] (s_c, 0 without a child), "base"
    uint32[n, 225], "considered" uint8[n, 225], "m_eff" int32[n]}."""
    prior = _rows(prior, np.float32)
    n = prior.shape[0]
    visits, stones, game_ids = _rows(visits, np.uint32, n), _rows(stones, np.int32, n, 0), _rows(game_ids, np.uint32, n, 0)
    out = {"draws": np.zeros((n, N), np.float64), "score": np.zeros((n, N), np.float64), "base": np.zeros((n, N), np.uint32),
           "considered": np.zeros((n, N), np.uint8), "m_eff": np.zeros(n, np.int32)}
    _check(load().gmk_gumbel_setup_host(prior.ctypes.data, visits.ctypes.data, stones.ctypes.data, game_ids.ctypes.data, n, int(max_considered),
                                        int(seed) & 0xFFFFFFFFFFFFFFFF, *[out[k].ctypes.data for k in ("draws", "score", "base", "considered", "m_eff")]))
    return out


def _gumbel_state(prior, visits, value, root_value, setup):
    prior = _rows(prior, np.float32)
    n = prior.shape[0]
    rows = [prior, _rows(visits, np.uint32, n), _rows(value, np.float32, n), _rows(root_value, np.float32, n, 0)]
    if setup is not None:
        rows += [_rows(setup["score"], np.float64, n), _rows(setup["base"], np.uint32, n), _rows(setup["considered"], np.uint8, n)]
    return n, rows


def gumbel_pick_host(prior, visits, value, root_value, setup, n_sims, c_visit=GUMBEL_C_VISIT, c_scale=GUMBEL_C_SCALE):
    """gmk_gumbel_pick_host: the cell the next playout's root step descends into, int16[n] (-1: a root without children).  value float32[n, 225]
    the children's stored means, root_value float32[n] the roots' own; setup: what gumbel_setup_host returned."""
    n, rows = _gumbel_state(prior, visits, value, root_value, setup)
    m_eff = _rows(setup["m_eff"], np.int32, n, 0)
    cells = np.zeros(n, dtype=np.int16)
    _check(load().gmk_gumbel_pick_host(*[r.ctypes.data for r in rows], m_eff.ctypes.data, n, int(n_sims), float(c_visit), float(c_scale), cells.ctypes.data))
    return cells


def gumbel_move_host(prior, visits, value, root_value, setup, c_visit=GUMBEL_C_VISIT, c_scale=GUMBEL_C_SCALE):
    """gmk_gumbel_move_host: the move, int16[n] (-1: a root without children)."""
    n, rows = _gumbel_state(prior, visits, value, root_value, setup)
    cells = np.zeros(n, dtype=np.int16)
    _check(load().gmk_gumbel_move_host(*[r.ctypes.data for r in rows], n, float(c_visit), float(c_scale), cells.ctypes.data))
    return cells


def gumbel_row_host(prior, visits, value, root_value, c_visit=GUMBEL_C_VISIT, c_scale=GUMBEL_C_SCALE):
    """gmk_gumbel_row_host: the improved-policy rows, uint16[n, 225]: what the Gumbel entries write where the plain ones write visit counts."""
    n, rows = _gumbel_state(prior, visits, value, root_value, None)
    out = np.zeros((n, N), dtype=np.uint16)
    _check(load().gmk_gumbel_row_host(*[r.ctypes.data for r in rows], n, float(c_visit), float(c_scale), out.ctypes.data))
    return out


def pvnet_sym_pick_host(states, seed=DEFAULT_SEED):
    """gmk_pvnet_sym_pick_host: the symmetry 0..7 that gmk_pvnet_evaluate_sym's "random" mode evaluates each position in, int32[n]; needs no GPU.
    states float32 [n, 6, 15, 15] (Board.encoded_states()); the pick depends on a row's content and the seed only (include/gomoku_symmetry.h)."""
    states = np.ascontiguousarray(states, dtype=np.float32)
    n = states.shape[0]
    assert states.size == n * 6 * N
    sym = np.zeros(n, dtype=np.int32)
    _check(load().gmk_pvnet_sym_pick_host(states.ctypes.data, n, int(seed) & 0xFFFFFFFFFFFFFFFF, sym.ctypes.data))
    return sym


def _check_step_device(tree, cells, verdict):
    import torch
    assert cells.is_cuda and cells.dtype == torch.int16 and cells.shape == (tree.n,) and cells.is_contiguous()
    assert verdict.is_cuda and verdict.dtype == torch.int32 and verdict.shape == (tree.n,) and verdict.is_contiguous()


# ---------------- K13: root-parallel ensembles (gmk_*_ensemble_merge) ----------------
ENSEMBLE_MISMATCH, ENSEMBLE_RANGE, ENSEMBLE_SATURATED = 1, 2, 4      # bits of the merge's status words
ENSEMBLE_MAX_GROUP = 4096


def _ensemble_merge(entry, tree, group, visits, values, cells, cells_per_game, root_visits, root_value, status, stream):
    import torch
    group = int(group)
    n_ens = tree.n // group if group > 0 and tree.n % group == 0 else 0      # (a bad group: the library refuses it; no shape to hold the tensors to)
    def ptr(t, size, shape):
        if t is None:
            return None
        assert t.is_cuda and t.is_contiguous() and t.element_size() == size and (n_ens == 0 or tuple(t.shape) == shape), "ensemble_merge: a tensor of the wrong shape or type"
        return t.data_ptr()
    _check(entry(tree.h, group, ptr(visits, 4, (n_ens, N)), ptr(values, 4, (n_ens, N)), ptr(cells, 2, (n_ens,)), ptr(cells_per_game, 2, (tree.n,)),
                 ptr(root_visits, 4, (n_ens,)), ptr(root_value, 4, (n_ens,)), ptr(status, 4, (n_ens,)), _current_stream(stream)))


def ensemble_merge_host(group, visits, values, root_visits=None, root_values=None):
    """gmk_ensemble_merge_host: the merge of gmk_*_ensemble_merge on host tables -- visits uint32[n, 225], values float32[n, 225], and
    optionally root_visits uint32[n], root_values float32[n] of n = E * group replicas -> {"visits" u32[E,225], "values" f32[E,225],
    "cells" i16[E], "root_visits" u32[E], "root_value" f32[E], "status" i32[E]}.  Needs no GPU."""
    visits = np.ascontiguousarray(visits, dtype=np.uint32)
    values = np.ascontiguousarray(values, dtype=np.float32)
    group = int(group)
    if visits.ndim != 2 or visits.shape[1] != N or values.shape != visits.shape:
        raise ValueError("ensemble_merge_host: visits and values are [n, 225] tables")
    n = visits.shape[0]
    if group >= 1 and n % group != 0:
        raise GmkError("ensemble_merge_host: group %d does not divide the %d games" % (group, n))
    rv = rq = None
    if root_visits is not None:
        rv = np.ascontiguousarray(root_visits, dtype=np.uint32)
        rq = np.ascontiguousarray(root_values, dtype=np.float32)
        assert rv.shape == (n,) and rq.shape == (n,)
    n_ens = n // group if group >= 1 else 0
    out = {"visits": np.zeros((n_ens, N), np.uint32), "values": np.zeros((n_ens, N), np.float32), "cells": np.zeros(n_ens, np.int16),
           "root_visits": np.zeros(n_ens, np.uint32), "root_value": np.zeros(n_ens, np.float32), "status": np.zeros(n_ens, np.int32)}
    _check(load().gmk_ensemble_merge_host(n_ens, group, visits.ctypes.data, values.ctypes.data, None if rv is None else rv.ctypes.data,
                                          None if rq is None else rq.ctypes.data, *[out[k].ctypes.data for k in
                                          ("visits", "values", "cells", "root_visits", "root_value", "status")]))
    return out


def match_referee(cells, visit_rows, row_of, moves, lens, winner, visits, verdict, status, unfinished, stream=None):
    """gmk_match_referee: one ply of n games on the device.  cells int16[n], visit_rows 2-byte [n, 225] or None, row_of int32[n] or None
    (slot -> record row), the records moves uint8[rows, 225] / lens int32[rows] / winner int8[rows] / visits 2-byte [rows, 225, 225] or None,
    verdict int32[n] (MATCH_*, in and out), status int32[n], unfinished int32[1]: torch tensors on the GPU."""
    import torch
    n, rows = int(cells.shape[0]), int(lens.shape[0])
    assert cells.dtype == torch.int16 and cells.is_contiguous() and verdict.dtype == torch.int32 and verdict.shape == (n,) and status.dtype == torch.int32 and status.shape == (n,)
    assert unfinished.dtype == torch.int32 and unfinished.numel() == 1
    assert moves.dtype == torch.uint8 and moves.shape == (rows, N) and moves.is_contiguous() and lens.dtype == torch.int32 and winner.dtype == torch.int8 and winner.shape == (rows,)
    assert visit_rows is None or (visit_rows.element_size() == 2 and visit_rows.shape == (n, N) and visit_rows.is_contiguous())
    assert visits is None or (visits.element_size() == 2 and visits.shape == (rows, N, N) and visits.is_contiguous())
    assert row_of is None or (row_of.dtype == torch.int32 and row_of.shape == (n,) and row_of.is_contiguous())
    assert all(t is None or t.is_cuda for t in (cells, visit_rows, row_of, moves, lens, winner, visits, verdict, status, unfinished))
    opt = lambda t: None if t is None else t.data_ptr()
    _check(load().gmk_match_referee(n, rows, cells.data_ptr(), opt(visit_rows), opt(row_of), moves.data_ptr(), lens.data_ptr(), winner.data_ptr(), opt(visits),
                                    verdict.data_ptr(), status.data_ptr(), unfinished.data_ptr(), _current_stream(stream)))


# ---------------- K6: pattern-guided search (TraditionalPolicy), one tree + one evaluator per game ----------------
class TraditionalMCTS:
    """n_games searches of MCTS(policy=TraditionalPolicy(c_puct)) run side by side on the GPU (gmk_trad_*).
    set_positions(move lists) = a fresh root at that position (the games' evaluators persist and are synchronised, like
    the reference's policy object); run(playouts) iterates MCTS::playout; root_stats() reads the roots."""

    def __init__(self, n_games, node_capacity=1 << 20, c_puct=5.0):
        init()
        self.n, self.c_puct = n_games, float(c_puct)
        h = C.c_void_p()
        _check(load().gmk_trad_create(n_games, int(node_capacity), C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None) and load is not None:       # (module globals are gone at interpreter shutdown)
            load().gmk_trad_destroy(self.h)
            self.h = None

    __del__ = close

    STATUS_ARENA_FULL, STATUS_EVALUATOR_ERROR, STATUS_BOARD_ONLY_REVERT, STATUS_ILLEGAL_STEP = 1, 2, 4, 8      # bits of root_stats()["status"]

    def reset_evaluators(self):
        _check(load().gmk_trad_reset_evaluators(self.h))

    def set_game_ids(self, ids):
        """The game each slot is playing, relative to the first_game_id of add_root_noise / PoolRAVEMCTS (uint32[n]; default: the
        slot number): random streams belong to the game, not to the slot it runs in."""
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        assert ids.shape == (self.n,)
        _check(load().gmk_trad_set_game_ids(self.h, ids.ctypes.data))

    def set_positions(self, move_lists, lens=None):
        """One move list per game, or (with lens) the arrays themselves: moves uint8[n, 225], lens int32[n]; a negative length
        leaves that game's position and tree as they are (not on the first call)."""
        if lens is not None:
            moves = np.ascontiguousarray(move_lists, dtype=np.uint8)
            lens = np.ascontiguousarray(lens, dtype=np.int32)
            assert moves.shape == (self.n, N) and lens.shape == (self.n,)
        else:
            moves = np.zeros((self.n, N), np.uint8)
            lens = np.zeros(self.n, np.int32)
            assert len(move_lists) == self.n
            for g, ml in enumerate(move_lists):
                lens[g] = len(ml)
                moves[g, :len(ml)] = ml
        _check(load().gmk_trad_set_positions(self.h, moves.ctypes.data, lens.ctypes.data))

    def run(self, playouts, stream=0):
        _check(load().gmk_trad_run(self.h, int(playouts), self.c_puct, stream))

    def step(self, moves=None):
        """MCTS::stepForward: per game the cell to step to (int16[n]), -1 / None = the most visited child; the subtree is kept."""
        if moves is None:
            _check(load().gmk_trad_step(self.h, None))
        else:
            m = np.ascontiguousarray(moves, dtype=np.int16)
            assert m.shape == (self.n,)
            _check(load().gmk_trad_step(self.h, m.ctypes.data))

    def root_choice(self, cells, visits=None, stream=None, sample=None):
        """gmk_trad_root_choice: root_stats()["best"] into cells (torch int16[n] on the GPU) and the root children's visit counts by cell,
        saturated at 65 535, into visits (2-byte torch [n, 225], or None); nothing comes to the host.
        sample = (plies, power, seed, first_game_id): gmk_trad_root_choice_sampled, the choice selfplay_run(sample=) makes for the games of
        set_game_ids at the stones of their positions."""
        if sample is None:
            _root_choice(load().gmk_trad_root_choice, self, cells, visits, stream)
        else:
            args = _sample_args(sample)
            _root_choice(lambda h, c, v, s: load().gmk_trad_root_choice_sampled(h, c, v, *args, s), self, cells, visits, stream)

    def step_device(self, cells, verdict, fresh_root=False, stream=None):
        """gmk_trad_step_device: step() with the cells (torch int16[n]) and the referee's verdicts (torch int32[n], MATCH_*) on the GPU."""
        _check_step_device(self, cells, verdict)
        _check(load().gmk_trad_step_device(self.h, cells.data_ptr(), verdict.data_ptr(), int(bool(fresh_root)), _current_stream(stream)))

    def ensemble_merge(self, group, visits=None, values=None, cells=None, cells_per_game=None, root_visits=None, root_value=None, status=None, stream=None):
        """gmk_trad_ensemble_merge: BatchedMCTS.ensemble_merge for a K6 / K6 + RAVE / K8 handle."""
        _ensemble_merge(load().gmk_trad_ensemble_merge, self, group, visits, values, cells, cells_per_game, root_visits, root_value, status, stream)

    def add_root_noise(self, alpha=0.05, epsilon=0.25, seed=DEFAULT_SEED, first_game_id=0, stream=None):
        """gmk_trad_add_root_noise on `stream` (default: torch's current stream): the counter sampler is one launch there, the std sampler waits for it."""
        _check(load().gmk_trad_add_root_noise(self.h, alpha, epsilon, seed, first_game_id, _current_stream(stream)))

    _POOLRAVE = 0

    def set_option(self, option, value):
        """gmk_trad_set_option: OPT_NOISE_SAMPLER -> NOISE_SAMPLERS["std" | "counter"], OPT_LOCKSTEP -> 0 / 1."""
        _check(load().gmk_trad_set_option(self.h, int(option), int(value)))

    def reserve(self, two_arenas=False):
        """gmk_trad_reserve: the two arenas per slot of the persistent loop with kept subtrees, now."""
        _check(load().gmk_trad_reserve(self.h, int(bool(two_arenas))))

    def selfplay_run(self, n_total, first_game_id, playouts, d_moves, d_visits, d_lens, d_winner, open_moves=None, open_lens=None,
                     reuse_subtree=False, root_noise=None, seed=DEFAULT_SEED, stream=None, max_steps=0, persistent=False, sample=None):
        """gmk_trad_selfplay_run: the handle's games are slots that play n_total whole games between them, the loop resident on the
        device (search, MCTS::stepForward's move, end-of-game check and slot hand-over are kernels).  open_moves uint8[n_total, stride] /
        open_lens int32[n_total] (host) or None; the outputs are device pointers (ints), indexed by game.
        sample = (plies, power): gmk_trad_selfplay_run_sampled -- a game with fewer than `plies` stones plays a cell drawn in proportion to
        visits^power (include/gomoku_sample.h), keyed by this call's seed and first_game_id.
        Returns (search launches, whether a search stopped at its node capacity)."""
        steps, overflow = C.c_int32(), C.c_int32()
        om = ol = None
        stride = 0
        if open_moves is not None:
            om = np.ascontiguousarray(open_moves, dtype=np.uint8)
            ol = np.ascontiguousarray(open_lens, dtype=np.int32)
            assert om.ndim == 2 and om.shape[0] == n_total and ol.shape == (n_total,)
            stride = om.shape[1]
        alpha, eps = root_noise if root_noise is not None else (0.0, 0.0)
        head = (self.h, self._POOLRAVE, int(n_total), int(first_game_id), int(playouts), self.c_puct, int(seed), int(bool(reuse_subtree)), float(alpha), float(eps))
        tail = (None if om is None else om.ctypes.data, stride, None if ol is None else ol.ctypes.data,
                d_moves, d_visits, d_lens, d_winner, int(bool(persistent)), int(max_steps), C.byref(overflow), C.byref(steps), stream)
        if sample is None:
            _check(load().gmk_trad_selfplay_run(*head, *tail))
        else:
            _check(load().gmk_trad_selfplay_run_sampled(*head, int(sample[0]), int(sample[1]), *tail))
        return steps.value, bool(overflow.value)

    def root_stats(self):
        out = {"visits": np.zeros((self.n, N), np.uint32), "values": np.zeros((self.n, N), np.float32), "priors": np.zeros((self.n, N), np.float32),
               "best": np.zeros(self.n, np.int32), "root_visits": np.zeros(self.n, np.uint32), "root_value": np.zeros(self.n, np.float32),
               "n_nodes": np.zeros(self.n, np.int32), "status": np.zeros(self.n, np.int32), "evaluator_updates": np.zeros(self.n, np.uint64)}
        _check(load().gmk_trad_root_stats(self.h, *[out[k].ctypes.data for k in
               ("visits", "values", "priors", "best", "root_visits", "root_value", "n_nodes", "status", "evaluator_updates")]))
        return out

    def read_evaluators(self):
        out = {"scores": np.zeros((self.n, 4, N), np.int32), "density": np.zeros((self.n, 2, 2, N), np.int32),
               "pattern_dist": np.zeros((self.n, 226, 8), np.uint32), "compound_dist": np.zeros((self.n, 226, 3), np.uint32),
               "meta": np.zeros((self.n, 4), np.int32), "record": np.zeros((self.n, 228), np.uint8)}
        _check(load().gmk_trad_read_evaluators(self.h, out["scores"].ctypes.data, out["density"].ctypes.data, out["pattern_dist"].ctypes.data,
                                               out["compound_dist"].ctypes.data, out["meta"].ctypes.data, out["record"].ctypes.data))
        return out


def _root_stats_with_amaf(self):
    """root_stats() of the two RAVE searchers: TraditionalMCTS's, and the root children's AMAF statistics."""
    out = TraditionalMCTS.root_stats(self)
    out["amaf_visits"] = np.zeros((self.n, N), np.uint32)
    out["amaf_values"] = np.zeros((self.n, N), np.float32)
    _check(load().gmk_trad_root_amaf(self.h, out["amaf_visits"].ctypes.data, out["amaf_values"].ctypes.data))
    return out


class PoolRAVEMCTS(TraditionalMCTS):
    """n_games searches of MCTS(policy=PoolRAVEPolicy(c_puct)) side by side on the GPU (K8): the tree, step, noise and root
    statistics of TraditionalMCTS, playouts with one random rollout each and RAVE::BackPropogate<true>."""

    _POOLRAVE = 1

    def __init__(self, n_games, node_capacity=1 << 20, c_puct=2.0, seed=DEFAULT_SEED, first_game_id=0):
        super().__init__(n_games, node_capacity, c_puct)
        self.seed, self.first_game_id = int(seed), int(first_game_id)

    def run(self, playouts, stream=0):
        _check(load().gmk_trad_run_poolrave(self.h, int(playouts), self.c_puct, self.seed, self.first_game_id, stream))

    def add_root_noise(self, alpha=0.05, epsilon=0.25, seed=None, first_game_id=None, stream=None):
        super().add_root_noise(alpha, epsilon, self.seed if seed is None else seed, self.first_game_id if first_game_id is None else first_game_id, stream)

    root_stats = _root_stats_with_amaf


class TraditionalRAVEMCTS(TraditionalMCTS):
    """n_games searches of MCTS(policy=TraditionalPolicy(c_puct, use_rave=True)) side by side on the GPU (agents/mcts.py:44-47): K6's
    playout with RAVE::BackPropogate<true> against the leaf position (gmk_trad_run_rave); root_stats() adds the root children's
    AMAF statistics.  c_bias is accepted and unused, as in the reference (HandSelect, not MinMSE)."""

    _POOLRAVE = 2                                        # gmk_trad_selfplay_run's policy

    def __init__(self, n_games, node_capacity=1 << 20, c_puct=5.0, c_bias=0.0):
        super().__init__(n_games, node_capacity, c_puct)
        self.c_bias = float(c_bias)

    def run(self, playouts, stream=0):
        _check(load().gmk_trad_run_rave(self.h, int(playouts), self.c_puct, stream))

    root_stats = _root_stats_with_amaf


# ---------------- K7: network-guided search, many games in lock step ----------------
class AlphaZeroMCTS:
    """n_games searches of MCTS(policy=Policy(eval_state=network.eval_state, c_puct)) (agents/alphazero.py:5-9) advancing one
    playout per step: select() writes the leaves' feature planes into `states` (torch float32 [n, 6, 15, 15] on the GPU), the
    caller's network maps them to (value [n], probs [n, 225]), expand() grows the trees and backs the values up.
    leaves = L > 1 (at most AZ_MAX_LEAVES): a step takes up to L leaves from every game, steered apart by virtual loss (OPT_AZ_LEAVES, see
    gmk_az_set_option); the batch then has live x L rows, game g's k-th leaf in row g L + k, and search() takes about playouts / L steps.
    vcf_depth = D > 0 (at most VCF_MAX_DEPTH): select() also hands every pending leaf to the forced-win solver (vcf_solve's walk, plain mode, the side
    to move attacks, at most vcf_budget nodes), and expand() answers a leaf with a forced win by fours itself: value 1, all the probability on
    the winning move (OPT_AZ_VCF_DEPTH / OPT_AZ_VCF_BUDGET; include/gomoku_hip.h, "K7 + K14").  vcf_stats() and vcf_verdicts() read it out.
    proof = True: nodes carry proven wins and losses (a five on the board, a leaf the solver answers WIN) up the tree, descents stop at proven
    nodes without a network row, and the root plays a proven win and avoids proven losses (OPT_AZ_PROOF; include/gomoku_hip.h, "K7 + proofs").
    root_proofs() and proof_stats() read it out.
    vcf_defend = True (it acts only with vcf_depth > 0 and proof): select() also asks what the opponent threatens at every pending leaf the solver
    did not answer, and under a forced win by fours which replies lose to it (vcf_defend's table); expand() marks those children as the
    opponent's proven wins and proves a leaf without a holding reply lost (OPT_AZ_VCF_DEFEND; include/gomoku_hip.h, "K7 + K15").
    defend_stats() and defend_verdicts() read it out.
    gumbel = (max_considered, n_sims, c_visit, c_scale, seed, first_game_id): the root step of select() is Gumbel AlphaZero's (gmk_az_set_gumbel;
    include/gomoku_gumbel.h, "K21"): sequential halving over the Gumbel-top-m root children, PUCB below; advance(gumbel=True) and
    root_choice(gumbel=True) then move by the rule and write the improved-policy row where the visit counts went.  leaves = 1 and proof = False only."""

    def __init__(self, n_games, node_capacity=1 << 16, c_puct=5.0, leaves=1, vcf_depth=0, vcf_budget=64, proof=False, vcf_defend=False, gumbel=None):
        import torch
        init()
        self.n = n_games
        h = C.c_void_p()
        _check(load().gmk_az_create(n_games, int(node_capacity), float(c_puct), C.byref(h)))
        self.h = h
        self.leaves = 1
        self.states = torch.zeros((n_games, 6, 15, 15), dtype=torch.float32, device="cuda")
        self.live = n_games                                        # games with rows in the leaf batch (see select)
        if leaves != 1:
            self.set_option(OPT_AZ_LEAVES, leaves)
        if vcf_depth != 0:
            self.set_option(OPT_AZ_VCF_BUDGET, vcf_budget)
            self.set_option(OPT_AZ_VCF_DEPTH, vcf_depth)
        if proof:
            self.set_option(OPT_AZ_PROOF, 1)
        if vcf_defend:
            self.set_option(OPT_AZ_VCF_DEFEND, 1)
        if gumbel is not None:
            self.set_gumbel(*gumbel)

    def set_gumbel(self, max_considered, n_sims=1, c_visit=GUMBEL_C_VISIT, c_scale=GUMBEL_C_SCALE, seed=DEFAULT_SEED, first_game_id=0):
        """gmk_az_set_gumbel: max_considered = 0 switches the Gumbel root search off, 1 .. 225 on with n_sims (1 .. 4096) playouts per move to
        schedule; waits for the device and voids every root's set-up."""
        _check(load().gmk_az_set_gumbel(self.h, int(max_considered), int(n_sims), float(c_visit), float(c_scale), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                        int(first_game_id) & 0xFFFFFFFF))

    def close(self):
        if getattr(self, "h", None) and load is not None:
            load().gmk_az_destroy(self.h)
            self.h = None

    __del__ = close

    STATUS_OVER, STATUS_ARENA_FULL, STATUS_ILLEGAL_STEP = 1, 2, 4      # bits of root_stats()["status"]

    def set_game_ids(self, ids):
        """The game each slot is playing, relative to add_root_noise's first_game_id (uint32[n]; default: the slot number)."""
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        assert ids.shape == (self.n,)
        _check(load().gmk_az_set_game_ids(self.h, ids.ctypes.data))

    def set_roots(self, planes, last_moves):
        """planes uint16[n,2,16]; last_moves int16[n,2] = (last move, the one before), -1 where there is none."""
        planes = np.ascontiguousarray(planes, dtype=np.uint16)
        last_moves = np.ascontiguousarray(last_moves, dtype=np.int16)
        assert planes.shape == (self.n, 2, 16) and last_moves.shape == (self.n, 2)
        _check(load().gmk_az_set_roots(self.h, planes.ctypes.data, last_moves.ctypes.data))
        self.n_total = None
        self._refresh_live()

    def _refresh_live(self):
        """self.live = rows of the leaf batch: the games still played, in slot order (gmk_az_live_games)"""
        n = C.c_int32(0)
        _check(load().gmk_az_live_games(self.h, C.byref(n)))
        self.live = n.value

    def select(self, stream=None):
        import torch
        stream = torch.cuda.current_stream().cuda_stream if stream is None else stream
        _check(load().gmk_az_select(self.h, self.states.data_ptr(), stream))
        return self.states[:self.live * self.leaves]               # the games still played (all of them until advance() ends one), `leaves` rows each

    def expand(self, values, probs, stream=None):
        import torch
        assert values.dtype == torch.float32 and probs.dtype == torch.float32 and values.is_contiguous() and probs.is_contiguous()
        assert values.numel() == self.live * self.leaves and probs.numel() == self.live * self.leaves * N
        stream = torch.cuda.current_stream().cuda_stream if stream is None else stream
        _check(load().gmk_az_expand(self.h, values.data_ptr(), probs.data_ptr(), stream))

    def step(self, moves=None):
        """MCTS::stepForward for every game: int16[n] cells, -1 / None = the most visited child; the subtree is kept."""
        if moves is None:
            _check(load().gmk_az_step(self.h, None))
        else:
            m = np.ascontiguousarray(moves, dtype=np.int16)
            assert m.shape == (self.n,)
            _check(load().gmk_az_step(self.h, m.ctypes.data))

    def root_choice(self, cells, visits=None, stream=None, sample=None, gumbel=False):
        """gmk_az_root_choice: the most visited root child (first maximum in cell order, -1 without one) into cells (torch int16[n] on the
        GPU) and the root children's visit counts by cell, saturated at 65 535, into visits (2-byte torch [n, 225], or None).
        sample = (plies, power, seed, first_game_id): gmk_az_root_choice_sampled, the choice advance(sample=) makes.
        gumbel = True: gmk_az_root_choice_gumbel, the choice advance(gumbel=True) makes; visits gets the improved-policy row, and the roots'
        set-ups are void afterwards (the choice is taken once per root)."""
        if gumbel:
            assert sample is None
            _root_choice(load().gmk_az_root_choice_gumbel, self, cells, visits, stream)
        elif sample is None:
            _root_choice(load().gmk_az_root_choice, self, cells, visits, stream)
        else:
            args = _sample_args(sample)
            _root_choice(lambda h, c, v, s: load().gmk_az_root_choice_sampled(h, c, v, *args, s), self, cells, visits, stream)

    def step_device(self, cells, verdict, fresh_root=False, unfinished=None, stream=None):
        """gmk_az_step_device: step() with the cells (torch int16[n]) and the referee's verdicts (torch int32[n], MATCH_*) on the GPU; games that
        ended leave the leaf batch.  unfinished: the referee's counter (torch int32[1]); its value is returned (else None)."""
        _check_step_device(self, cells, verdict)
        count = C.c_int32(0)
        _check(load().gmk_az_step_device(self.h, cells.data_ptr(), verdict.data_ptr(), int(bool(fresh_root)), None if unfinished is None else unfinished.data_ptr(),
                                         None if unfinished is None else C.byref(count), _current_stream(stream)))
        self._refresh_live()
        return None if unfinished is None else count.value

    def set_slots(self, n_total, open_moves=None, open_lens=None):
        """Continuous batching (gmk_az_set_slots): the n slots of this handle play n_total games between them, from their openings
        (uint8[n_total, stride], int32[n_total]); takes set_roots's place.  advance() then wants records of n_total rows."""
        self.n_total = int(n_total)
        if open_moves is None:
            _check(load().gmk_az_set_slots(self.h, int(n_total), None, 0, None))
        else:
            m = np.ascontiguousarray(open_moves, dtype=np.uint8)
            l = np.ascontiguousarray(open_lens, dtype=np.int32)
            assert m.ndim == 2 and m.shape[0] == n_total and l.shape == (n_total,)
            _check(load().gmk_az_set_slots(self.h, int(n_total), m.ctypes.data, m.shape[1], l.ctypes.data))
        self._refresh_live()

    def advance(self, moves, visits, lens, winner, reuse_subtree=True, stream=None, sample=None, gumbel=False):
        """One self-play move for every game still played, on the device (gmk_az_advance): moves uint8[n,225], visits int16/uint16
        [n,225,225] or None, lens int32[n], winner int8[n] are torch tensors on the GPU (the games' records, openings included);
        returns the number of games that go on.  sample = (plies, power, seed, first_game_id): gmk_az_advance_sampled -- a game with fewer
        than `plies` stones on its root board plays a child drawn in proportion to visits^power (power 1..3; include/gomoku_sample.h), keyed by
        seed and the game's global id as add_root_noise keys its draws; None: every game plays its most visited child.
        gumbel = True: gmk_az_advance_gumbel -- the move is the Gumbel rule's and `visits` gets the improved-policy row (set_gumbel must be on)."""
        import torch
        stream = torch.cuda.current_stream().cuda_stream if stream is None else stream
        rows = getattr(self, "n_total", None) or self.n
        assert moves.dtype == torch.uint8 and moves.shape == (rows, N) and lens.dtype == torch.int32 and lens.shape == (rows,) and winner.dtype == torch.int8 and winner.shape == (rows,)
        assert visits is None or (visits.element_size() == 2 and visits.shape == (rows, N, N))
        unfinished = C.c_int32(0)
        if gumbel:
            assert sample is None
            _check(load().gmk_az_advance_gumbel(self.h, moves.data_ptr(), visits.data_ptr() if visits is not None else None, lens.data_ptr(), winner.data_ptr(),
                                                int(bool(reuse_subtree)), C.byref(unfinished), stream))
        elif sample is None:
            _check(load().gmk_az_advance(self.h, moves.data_ptr(), visits.data_ptr() if visits is not None else None, lens.data_ptr(), winner.data_ptr(),
                                         int(bool(reuse_subtree)), C.byref(unfinished), stream))
        else:
            _check(load().gmk_az_advance_sampled(self.h, moves.data_ptr(), visits.data_ptr() if visits is not None else None, lens.data_ptr(), winner.data_ptr(),
                                                 int(bool(reuse_subtree)), *_sample_args(sample), C.byref(unfinished), stream))
        self._refresh_live()
        return unfinished.value

    def add_root_noise(self, alpha=0.05, epsilon=0.25, seed=DEFAULT_SEED, first_game_id=0, stream=None):
        """gmk_az_add_root_noise on `stream` (default: torch's current stream): the counter sampler is one launch there, the std sampler waits for it."""
        _check(load().gmk_az_add_root_noise(self.h, alpha, epsilon, seed, first_game_id, _current_stream(stream)))

    def set_option(self, option, value):
        """gmk_az_set_option: OPT_NOISE_SAMPLER -> NOISE_SAMPLERS["std" | "counter"]; OPT_AZ_LEAVES -> 1 .. AZ_MAX_LEAVES leaves per game per step;
        OPT_AZ_VCF_DEPTH -> 0 (off) .. VCF_MAX_DEPTH and OPT_AZ_VCF_BUDGET -> 1 .. 2^20 for the solver at the leaves; OPT_AZ_PROOF -> 0 / 1;
        OPT_AZ_VCF_DEFEND -> 0 / 1."""
        import torch
        _check(load().gmk_az_set_option(self.h, int(option), int(value)))
        if int(option) == OPT_AZ_LEAVES:
            self.leaves = int(value)
            if self.states.shape[0] < self.n * self.leaves:
                self.states = torch.zeros((self.n * self.leaves, 6, 15, 15), dtype=torch.float32, device="cuda")

    def add_playouts(self, playouts, stream=None):
        """gmk_az_add_playouts: every game that is not over owes `playouts` more (leaves > 1: select() takes them off as it completes them)."""
        _check(load().gmk_az_add_playouts(self.h, int(playouts), _current_stream(stream)))

    def playouts_owed(self, stream=None):
        """gmk_az_playouts_owed: the largest number of playouts a game still owes (waits for the stream)."""
        owed = C.c_int32(0)
        _check(load().gmk_az_playouts_owed(self.h, C.byref(owed), _current_stream(stream)))
        return owed.value

    def search(self, network, playouts, graph=False):
        """`playouts` lock-step playouts; network(states) -> (value [n], probs [n, 225]) on the GPU.  graph=True: the first playout
        runs eagerly, then ONE playout step (select kernel, the network's kernels, expand kernel) is captured into a hipGraph and
        replayed for the rest, which removes the launch gaps between the ~10 kernels of a step; the network must be capturable
        (no host synchronisation; PolicyValueNetwork and FusedPolicyValueNetwork are).
        leaves > 1: every game is given `playouts` more to complete (add_playouts), ceil(playouts / leaves) steps are taken without looking,
        then steps until no game owes any (playouts_owed: collisions cut steps short); every game ends with exactly `playouts` more."""
        import torch

        def step():
            values, probs = network(self.select())
            self.expand(values.contiguous(), probs.contiguous())

        if self.leaves > 1:
            if playouts <= 0:
                return
            self.add_playouts(playouts)
            blind = -(-playouts // self.leaves)
            if not graph or blind < 3:
                for _ in range(blind):
                    step()
                while self.playouts_owed() > 0:
                    step()
                return
            step()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                step()
            for _ in range(blind - 1):
                g.replay()
            while self.playouts_owed() > 0:
                g.replay()
            return
        if not graph or playouts < 3:
            for _ in range(playouts):
                step()
            return
        step()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            step()
        for _ in range(playouts - 1):
            g.replay()

    def vcf_stats(self):
        """gmk_az_vcf_stats: per game, since set_roots / set_slots: pending leaves solved, those answered WIN, those cut by BUDGET or DEPTH, and the
        nodes the walks counted."""
        out = {"leaves": np.zeros(self.n, np.uint32), "wins": np.zeros(self.n, np.uint32), "cut": np.zeros(self.n, np.uint32), "nodes": np.zeros(self.n, np.uint64)}
        _check(load().gmk_az_vcf_stats(self.h, *[out[k].ctypes.data for k in ("leaves", "wins", "cut", "nodes")]))
        return out

    def root_proofs(self):
        """gmk_az_root_proofs: the root's proof (AZ_PROOF_*) int8[n] and its children's by cell int8[n, 225], 0 where there is no child."""
        out = {"root": np.zeros(self.n, np.int8), "children": np.zeros((self.n, N), np.int8)}
        _check(load().gmk_az_root_proofs(self.h, out["root"].ctypes.data, out["children"].ctypes.data))
        return out

    def proof_stats(self):
        """gmk_az_proof_stats: per game, since set_roots / set_slots: nodes given a proof, and descents ended at a node already proven."""
        out = {"proved": np.zeros(self.n, np.uint32), "stops": np.zeros(self.n, np.uint32)}
        _check(load().gmk_az_proof_stats(self.h, out["proved"].ctypes.data, out["stops"].ctypes.data))
        return out

    def defend_stats(self):
        """gmk_az_defend_stats: per game, since set_roots / set_slots: leaves expanded under a forced win by fours of the opponent, children marked
        as his proven wins, cells that were solved in full, and the nodes of those solves."""
        out = {"threatened": np.zeros(self.n, np.uint32), "marked": np.zeros(self.n, np.uint32), "searched": np.zeros(self.n, np.uint32), "nodes": np.zeros(self.n, np.uint64)}
        _check(load().gmk_az_defend_stats(self.h, *[out[k].ctypes.data for k in ("threatened", "marked", "searched", "nodes")]))
        return out

    def defend_verdicts(self):
        """gmk_az_defend_verdicts_host: for the live x leaves rows of the last select(), the threat against the leaf ("threat_status" i32[rows] as
        vcf_solve names it, "threat_length" i32[rows]) and vcf_defend's table for it ("verdict" i8[rows, 225] VCF_CELL_*, "nodes" u32[rows, 225]); a
        row without a pending leaf, or one the solver answered itself, reads VCF_NONE / 0 and zeros."""
        rows = self.live * self.leaves
        out = {"threat_status": np.zeros(rows, np.int32), "threat_length": np.zeros(rows, np.int32), "verdict": np.zeros((rows, N), np.int8), "nodes": np.zeros((rows, N), np.uint32)}
        _check(load().gmk_az_defend_verdicts_host(self.h, *[out[k].ctypes.data for k in ("threat_status", "threat_length", "verdict", "nodes")]))
        return out

    def vcf_verdicts(self):
        """gmk_az_vcf_verdicts_host: the verdicts of the last select() for the live x leaves rows of the leaf batch, as vcf_solve names them; a row
        without a pending leaf reads VCF_NONE / -1 / 0 / 0."""
        rows = self.live * self.leaves
        out = {"status": np.zeros(rows, np.int32), "move": np.zeros(rows, np.int32), "length": np.zeros(rows, np.int32), "nodes": np.zeros(rows, np.uint32)}
        _check(load().gmk_az_vcf_verdicts_host(self.h, *[out[k].ctypes.data for k in ("status", "move", "length", "nodes")]))
        return out

    def root_stats(self):
        out = {"visits": np.zeros((self.n, N), np.uint32), "values": np.zeros((self.n, N), np.float32), "priors": np.zeros((self.n, N), np.float32),
               "root_visits": np.zeros(self.n, np.uint32), "root_value": np.zeros(self.n, np.float32),
               "n_nodes": np.zeros(self.n, np.int32), "status": np.zeros(self.n, np.int32)}
        _check(load().gmk_az_root_stats(self.h, *[out[k].ctypes.data for k in ("visits", "values", "priors", "root_visits", "root_value", "n_nodes", "status")]))
        return out
