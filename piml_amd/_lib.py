"""ctypes binding of libpiml_hip.so (include/piml_hip.h).  Loading fails loudly: there is no
CPU fallback for the product path."""
import ctypes
import os

# torch must be loaded first: libpiml_hip.so needs libamdhip64.so.7 and has to bind to the
# HIP runtime instance torch already loaded (device pointers and streams come from torch);
# loading it before torch would pull a second runtime from /opt/rocm into the process.
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
# PIML_LIB=<path>: an experimental build of the same ABI beside the shipped library (piml_amd.build.variant; tools/ A/B timings)
LIB_PATH = os.environ.get('PIML_LIB') or os.path.join(_HERE, 'libpiml_hip.so')
ABI_VERSION = 35
COMPACT_MAX_AGENTS = 16384      # PIML_COMPACT_MAX_AGENTS / PIML_COMPACT_SLOTS (include/piml_hip.h: compact rows)
COMPACT_SLOTS = 256

_lib = None

_i, _f, _p, _z = ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t
_ll = ctypes.c_longlong
_d = ctypes.c_double


class EncoderBranch(ctypes.Structure):
    """piml_encoder_branch (include/piml_hip.h)."""
    _fields_ = [('x', _p), ('rows', _ll), ('in_dim', _i), ('k', _i),
                ('w1', _p), ('b1', _p), ('w2', _p), ('b2', _p), ('w3', _p), ('b3', _p),
                ('scale', _f), ('h1', _p), ('h2', _p), ('msgs', _p), ('g_pooled', _p), ('g_msgs', _p),
                ('g2', _p), ('g1', _p), ('g_x', _p), ('partials', _p), ('grads', _p), ('packed', _p), ('relu_mask', _p),
                ('keep_bits', _p), ('drop_state', _p), ('drop_p', _f), ('sum_a', _p), ('sum_b', _p),
                ('nbr_idx', _p), ('plan', _p)]


class DecoderBranch(ctypes.Structure):
    """piml_decoder_branch (include/piml_hip.h)."""
    _fields_ = [('msgs', _p), ('agents', _ll), ('k', _i),
                ('w1', _p), ('b1', _p), ('w2', _p), ('b2', _p), ('w3', _p), ('b3', _p),
                ('pooled', _p), ('h1', _p), ('d2', _p), ('g_pre2', _p), ('g_pre1', _p), ('g_pooled', _p),
                ('partials', _p), ('grads', _p), ('packed', _p), ('pred', _p), ('g_pred_rows', _p), ('g_d2', _p),
                ('fold_w3', _p), ('fold_b3', _p), ('fold_scale', _f), ('dw1_out', _p)]


class CollisionHead(ctypes.Structure):
    """piml_collision_head (include/piml_hip.h)."""
    _fields_ = [('msgs', _p), ('rows', _ll), ('w1', _p), ('b1', _p), ('w2', _p), ('b2', _p), ('packed', _p), ('out', _p),
                ('fold_w3', _p), ('fold_b3', _p), ('fold_scale', _f)]


class Head64(ctypes.Structure):
    """piml_head64 (include/piml_hip.h)."""
    _fields_ = [('x', _p), ('rows', _ll), ('w1', _p), ('b1', _p), ('w2', _p), ('b2', _p), ('hidden', _p), ('out', _p),
                ('g_out', _p), ('g_x', _p), ('partials', _p), ('grads', _p)]


class Corrector(ctypes.Structure):
    """piml_corrector (include/piml_hip.h)."""
    _fields_ = [('agents', _ll), ('k', _i), ('scale', _f), ('enc', _p), ('keep_bits', _p),
                ('wa', _p), ('ba', _p), ('wb', _p), ('bb', _p), ('wc', _p), ('bc', _p), ('wd', _p), ('bd', _p),
                ('hid', _p), ('score', _p), ('attn', _p), ('pooled', _p), ('chid', _p), ('out', _p),
                ('g_out', _p), ('g_pooled', _p), ('g_score', _p), ('g_chid', _p), ('g_enc', _p),
                ('partials_a', _p), ('partials_b', _p), ('grads', _p)]


class Scenario(ctypes.Structure):
    """piml_scenario (include/piml_hip.h)."""
    _fields_ = [('position', _p), ('velocity', _p), ('acceleration', _p), ('destination', _p), ('hist_velocity', _p),
                ('self_features', _p), ('desired_speed', _p), ('mask', _p), ('flag', _p), ('waypoints', _p), ('exit_idx', _p),
                ('spawn_iters', _p), ('position_out', _p), ('velocity_out', _p), ('acceleration_out', _p),
                ('destination_out', _p), ('mask_out', _p), ('spawn_out', _p), ('frame_counter', _p), ('spawned', _p),
                ('dropped', _p), ('entries', _p), ('route_polyline', _p),
                ('hist_width', _i), ('F', _i), ('D', _i), ('E', _i), ('P', _i), ('R', _i), ('capacity', _i), ('T', _i),
                ('n_initial', _i), ('route_max_iters', _i), ('spawn_cap', _i), ('uniform_speed', _i),
                ('dt', _f), ('spawn_offset', _f), ('route_clearance', _f), ('arrival_radius', _f), ('speed_mean', _f),
                ('speed_std', _f), ('speed_min', _f), ('seed', ctypes.c_uint64), ('poisson_thresholds', ctypes.c_uint32 * 8)]


class ScenarioRules(ctypes.Structure):
    """piml_scenario_rules (include/piml_hip.h)."""
    _fields_ = [('spawn_law', _i), ('arrival_rule', _i), ('initial_velocity', _i), ('speed_clamp', _i), ('spawn_cap2', _i),
                ('grid', _i), ('length', _f), ('width', _f), ('side_ratio', _f), ('direction_ratio', _f),
                ('poisson_thresholds2', ctypes.c_uint32 * 8), ('square_grid', _f * 32)]


class MlapmLaw(ctypes.Structure):
    """piml_mlapm_law (include/piml_hip.h)."""
    _fields_ = [('variant', _i), ('tau', _f), ('A', _f), ('B', _f), ('C', _f), ('D', _f), ('theta_deg', _f), ('radius', _f)]


class WallGrid(ctypes.Structure):
    """piml_wall_grid (include/piml_hip.h)."""
    _fields_ = [('points', _p), ('cell_start', _p), ('n_points', _i), ('gx', _i), ('gy', _i),
                ('x0', _f), ('y0', _f), ('cell', _f), ('cutoff', _f)]


class WallLaw(ctypes.Structure):
    """piml_wall_law (include/piml_hip.h)."""
    _fields_ = [('A', _f), ('B', _f)]


class GroupLaw(ctypes.Structure):
    """piml_group_law (include/piml_hip.h)."""
    _fields_ = [('A', _f), ('dist', _f)]


class SceneGroups(ctypes.Structure):
    """piml_scene_groups (include/piml_hip.h)."""
    _fields_ = [('row_unit', _p), ('unit_rows', _p), ('n_units', _i), ('group_first', _p), ('group_size', _p)]


class NoiseLaw(ctypes.Structure):
    """piml_noise_law (include/piml_hip.h)."""
    _fields_ = [('rho', _f), ('amp', _f)]


class NoiseArgs(ctypes.Structure):
    """piml_noise_args (include/piml_hip.h)."""
    _fields_ = [('state', _p), ('law', NoiseLaw), ('law_table', _p)]


class NavGrid(ctypes.Structure):
    """piml_nav_grid (include/piml_hip.h)."""
    _fields_ = [('u', _p), ('G', _i), ('gx', _i), ('gy', _i), ('x0', _f), ('y0', _f), ('cell', _f), ('near', _f)]


class NavSight(ctypes.Structure):
    """piml_nav_sight (include/piml_hip.h)."""
    _fields_ = [('parent', _p), ('G', _i), ('gx', _i), ('gy', _i)]


class ExitChoice(ctypes.Structure):
    """piml_exit_choice (include/piml_hip.h)."""
    _fields_ = [('margin', _f), ('commit', _f), ('every', _i)]


SPAWN_LAWS = {'gc': 0, 'crosswalk': 1, 'square': 2, 'unit1': 3, 'unit2': 4, 'unit3': 5, 'clip': 6}     # PIML_SPAWN_*
SPAWN_CLIP_GROUPS = 7          # PIML_SPAWN_CLIP_GROUPS ('clip_groups'): piml_scenario_step_mlapm_groups only, so not in SPAWN_LAWS
ARRIVAL_RULES = {'gc': 0, 'radius': 1, 'x_band': 2, 'x_exit': 3}                             # PIML_ARRIVE_*


PACKED_VALID, FORK, ACCUMULATE, DEFER_SLOT_SUMS, DEFER_PACK, POOL_H2, POOL_TRAIN, POOL_MSGS, DEFER_UNFOLD = 1, 2, 4, 8, 16, 32, 64, 128, 256   # piml_pinnsf_* flags

# name -> argtypes, in the order of include/piml_hip.h
SIGNATURES = {
    'piml_abi_version': [],
    'piml_heading_fwd': [_p, _i, _i, _i, _p, _p],
    'piml_relfeat_fwd': [_p, _p, _p, _p, _i, _p, _p, _i, _i, _i, _i, _i, _i, _i, _f, _f, _f, _f,
                         _p, _p, _p, _i, _p, _p, _p],
    'piml_mlapm_step_fwd': [_p, _p, _p, _p, _i, _i, _f, _f, _f, _f, _f, _f, _f, _f, _i, _p, _p, _p],
    'piml_mlapm_step_bwd': [_p, _p, _p, _p, _p, _i, _i, _f, _f, _f, _f, _f, _f, _f, _f, _p, _p, _p, _p, _p],
    'piml_mlapm_rollout_step': [_p, _p, _p, _p, _ll, _i, _i, _f, _f, _f, _f, _f, _f, _f, _f, _p, _p, _p],
    'piml_mlapm_bwd_workspace_floats': [_i, _i],
    'piml_mlapm_step_bwd_ws': [_p, _p, _p, _p, _p, _i, _i, _f, _f, _f, _f, _f, _f, _f, _f, _p, _p, _p, _p, _p, _ll, _p],
    'piml_mlapm_fit_workspace_doubles': [_i, _i],
    'piml_mlapm_fit_loss_grad': [_p, _p, _p, _p, _p, _p, _i, _i, _p, _i, _p, _i, _p, _i, _f, _f, _p, _ll, _p, _p, _p],
    'piml_mlapm_rollout_fit_workspace_doubles': [_i, _i, _ll],
    'piml_mlapm_rollout_fit_loss_grad': [_p, _p, _p, _p, _p, _i, _ll, _i, _p, _i, _p, _p, _i, _ll, _p, _i, _f, _f, _d,
                                         _p, _ll, _p, _p, _p, _p],
    'piml_collision_matrix': [_p, _i, _i, _f, _i, _p, _p],
    'piml_collision_friends': [_p, _p, _i, _i, _i, _i, _p],
    'piml_collision_counts': [_p, _i, _i, _p, _i, _p, _p],
    'piml_collision_counts_frames': [_p, _i, _i, _i, _p, _i, _p, _p],
    'piml_collision_counts_scratch': [_p, _i, _i, _p, _i, _p, _p, _p],
    'piml_collision_counts_grid': [_p, _i, _i, _p, _i, _p, _p, _p],
    'piml_collision_label': [_p, _z, _i, _p, _p],
    'piml_sinkhorn_frames': [_p, _p, _p, _p, _i, _i, _i, _f, _i, _f, _p, _p, _p, _p, _p],
    'piml_mmd_frames': [_p, _p, _p, _p, _i, _i, _i, _d, _i, _d, _p, _p],
    'piml_crowd_stats_workspace_bytes': [_i, _i, _i],
    'piml_crowd_stats': [_p, _p, _p, _p, _i, _i, _i, _i, _i, _f, _i, _f, _f, _f, _f, _f, _i, _i, _f, _i,
                         _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _ll, _p],
    'piml_crowd_stats_voronoi_workspace_bytes': [_i, _i, _i, _i],
    'piml_crowd_stats_voronoi': [_p, _p, _p, _p, _i, _i, _i, _i, _i, _f, _p, _i, _i, _f, _f, _f, _f, _i, _f, _f, _f, _f, _f,
                                 _i, _i, _f, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _ll, _p],
    'piml_pair_stats_workspace_bytes': [_i, _i, _i, _i],
    'piml_pair_stats': [_p, _p, _p, _p, _i, _i, _i, _i, _i, _p, _i, _f, _f, _i, _f, _f, _f, _f, _f, _i, _f, _i,
                        _p, _p, _p, _p, _p, _p, _p, _p, _ll, _p],
    'piml_flow_stats_workspace_bytes': [_i, _i, _i, _i],
    'piml_flow_stats': [_p, _p, _p, _p, _i, _i, _i, _i, _i, _f, _f, _i, _f, _f, _f, _f, _f, _i, _f, _f, _f, _f, _f, _i, _i,
                        _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _ll, _p],
    'piml_view_stats_workspace_bytes': [_i, _i, _i, _i],
    'piml_view_stats': [_p, _p, _p, _p, _i, _i, _i, _i, _i, _p, _i, _f, _f, _i, _f, _f, _f, _f, _i, _i, _f, _f, _f, _f,
                        _p, _p, _p, _p, _p, _p, _p, _ll, _p],
    'piml_track_stats_workspace_bytes': [_i, _i, _i],
    'piml_track_stats': [_p, _p, _p, _i, _i, _i, _i, _i, _f, _f, _i, _f, _f, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p,
                         _p, _p, _ll, _p],
    'piml_obstacle_stats_workspace_bytes': [_i, _i, _i, _i],
    'piml_obstacle_stats': [_p, _p, _p, _p, _i, _i, _i, _i, _i, _p, _i, _f, _f, _f, _i, _f, _f, _f, _f, _f, _i, _f, _i,
                            _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _ll, _p],
    'piml_line_stats_workspace_bytes': [_i, _i, _i, _i, _i, _i],
    'piml_line_stats': [_p, _p, _p, _i, _i, _i, _i, _i, _p, _i, _f, _f, _i, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _ll,
                        _p],
    'piml_group_pairs': [_p, _p, _p, _i, _i, _i, _i, _i, _f, _f, _f, _i, _i, _p, _p, _p, _p, _p, _p, _p],
    'piml_group_members': [_p, _p, _i, _i, _i, _i, _i, _p, _i, _f, _f, _f, _f, _i, _i, _p, _p, _p, _p, _p, _p],
    'piml_group_components': [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p],
    'piml_calc_acceleration': [_p, _z, _i, _i, _f, _f, _f, _f, _f, _f, _p, _p],
    'piml_rollout_step': [_p, _p, _p, _p, _p, _p, _i, _p, _p, _i, _i, _p, _p, _p, _p, _p, _p, _p, _i, _p, _p, _p,
                          _p, _p, _p, _p, _p, _i, _i, _i, _f, _i, _p],
    'piml_rollout_step_ksum': [_p, _i, _p, _i, _f, _p, _p, _p, _p, _p, _p, _i, _p, _p, _i, _i, _p, _p, _p, _p, _p, _p, _p, _i, _p, _p, _p,
                               _p, _p, _p, _p, _p, _i, _i, _i, _f, _i, _p],
    'piml_scenario_step': [_p, _p, _i, _p],
    'piml_scenario_step_rules': [_p, _p, _p, _i, _p],
    'piml_scenario_step_members': [_p, _p, _i, _p, _p, _i, _p],
    'piml_scenario_step_mlapm': [_p, _p, _i, _p, _p, _i, _p],
    'piml_mlapm_law_table_bytes': [_i],
    'piml_mlapm_law_table_fill': [_p, _i, _p],
    'piml_scenario_step_mlapm_laws': [_p, _p, _i, _p, _p, _i, _p],
    'piml_wall_force': [_p, _ll, _p, _f, _f, _p, _p, _p, _p],
    'piml_scenario_step_mlapm_walls': [_p, _p, _i, _p, _p, _p, _p, _p, _p, _i, _p],
    'piml_group_force': [_p, _p, _p, _ll, _f, _f, _p, _p],
    'piml_scenario_step_mlapm_groups': [_p, _p, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _p],
    'piml_noise_force': [_p, _p, _p, _p, _p, _i, _i, _ll, _f, _f, _p],
    'piml_scenario_step_mlapm_noise': [_p, _p, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _p],
    'piml_nav_relax': [_p, _p, _p, _p, _i, _i, _i, _i, _p, _p],
    'piml_nav_direction': [_p, _p, _p, _ll, _p, _p, _p, _p, _p],
    'piml_scenario_step_mlapm_nav': [_p, _p, _i, _p, _p, _p, _p, _p, _p, _p, _p, _i, _p],
    'piml_nav_density': [_p, _p, _i, _i, _f, _f, _f, _i, _i, _p, _p],
    'piml_nav_cost': [_p, _i, _i, _i, _f, _i, _f, _f, _f, _p, _p],
    'piml_nav_relax_cost': [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _p, _p],
    'piml_scenario_step_mlapm_navdyn': [_p, _p, _i, _p, _p, _p, _p, _p, _p, _p, _ll, _p, _i, _p],
    'piml_nav_descent': [_p, _i, _i, _i, _p, _p],
    'piml_nav_flow': [_p, _p, _p, _i, _i, _f, _f, _f, _i, _i, _p, _p, _p],
    'piml_nav_cost_flow': [_p, _p, _p, _i, _i, _i, _i, _f, _i, _f, _f, _f, _f, _f, _p, _p],
    'piml_nav_relax_cost_gates': [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _p, _p],
    'piml_nav_relax_active': [_p, _p, _p, _i, _p, _p, _i, _i, _i, _i, _i, _p, _p, _p, _p],
    'piml_nav_choose_exit': [_p, _i, _p, _p, _ll, _p, _p, _p, _i, _p],
    'piml_nav_sight_relax': [_p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _p, _p],
    'piml_nav_direction_sight': [_p, _p, _p, _ll, _p, _p, _p, _p, _p, _p],
    'piml_scenario_step_mlapm_sight': [_p, _p, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i, _p],
    'piml_scenario_step_nav': [_p, _p, _i, _p, _p, _i, _p, _p, _p, _p],
    'piml_scenario_route': [_p, _p, _i, _p, _i, _i, _f, _p, _p, _p],
    'piml_collision_correction_fwd': [_p, _p, _p, _z, _i, _i, _f, _f, _p, _p],
    'piml_collision_correction_bwd': [_p, _p, _p, _p, _z, _i, _i, _f, _f, _p, _p, _p, _p],
    'piml_train_step_fwd': [_p] * 7 + [_i, _i, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _f, _p, _p, _p, _p, _p, _p, _p, _p],
    'piml_train_step_fwd_copy': [_p] * 7 + [_i, _i, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _f, _p, _p, _p, _p, _p, _p, _p, _p, _ll, _p],
    'piml_train_step_bwd': [_p, _p, _p, _p, _p, _i, _i, _i, _i, _f, _p, _p, _p, _p, _p],
    'piml_train_step_bwd6': [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _f, _p, _p, _p, _p, _p],
    'piml_pinnsf_unfold_defer': [_i, _p],
    'piml_train_step_bwd7': [_p, _ll, _p, _p, _p, _p, _ll, _p, _p, _i, _i, _i, _i, _f, _p, _p, _p, _p, _p],
    'piml_train_step_tail_fwd': [_p, _p, _p, _p, _i, _p, _i, _p, _f, _p, _p, _p, _i, _i, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _f,
                                 _p, _p, _p, _p, _p, _p, _p, _p, _ll, _p],
    'piml_train_step_tail_bwd': [_p, _ll, _p, _p, _p, _p, _ll, _p, _p, _i, _i, _i, _i, _f, _p, _p, _p, _p, _p, _f, _i, _i, _p, _p, _p, _p],
    'piml_pinnsf_epilogue_fwd': [_p, _p, _p, _z, _f, _p, _p],
    'piml_pinnsf_epilogue_bwd': [_p, _p, _z, _f, _p, _p],
    'piml_pinnsf_epilogue_ksum_fwd': [_p, _i, _p, _i, _p, _z, _f, _p, _p],
    'piml_pinnsf_epilogue_ksum_bwd': [_p, _p, _z, _f, _i, _i, _p, _p, _p, _p],
    'piml_pinnsf_epilogue_agentnorm_fwd': [_p, _p, _p, _i, _i, _f, _p, _p],
    'piml_pinnsf_epilogue_ksum_agentnorm_fwd': [_p, _i, _p, _i, _p, _i, _i, _f, _p, _p],
    'piml_pinnsf_epilogue_agentnorm_bwd': [_p, _p, _i, _i, _f, _p, _p],
    'piml_self_features_fwd': [_p, _i, _p, _p, _z, _p, _p],
    'piml_self_features_bwd': [_p, _z, _p, _p, _p, _p],
    'piml_colsum_blocks': [_z, _i],
    'piml_act_bwd_colsum': [_p, _p, _z, _i, _p, _p, _p, _p],
    'piml_sum_leading': [_p, _i, _z, _p, _p],
    'piml_act_bwd_colsum_stage1': [_p, _p, _z, _i, _p, _p, _p, _p],
    'piml_layer_reduce': [_p, _i, _z, _p, _p, _i, _i, _p, _p],
    'piml_scale_ksum_fwd': [_p, _p, _z, _i, _i, _f, _p, _p, _p, _p],
    'piml_ksum_blocks': [_z, _i],
    'piml_scale_ksum_bwd': [_p, _p, _z, _i, _i, _f, _p, _p, _p, _p],
    'piml_dropout_keep_bits': [_p, _ll, _i, _f, _i, _p, _p],
    'piml_timer_create': [ctypes.POINTER(_p)],
    'piml_timer_record': [_p, _p],
    'piml_timer_elapsed_ms': [_p, _p, ctypes.POINTER(_f)],
    'piml_timer_destroy': [_p],
    'piml_trace_begin': [],
    'piml_trace_mark': [ctypes.c_char_p, _p],
    'piml_trace_end': [ctypes.c_char_p, _i, ctypes.POINTER(_f), _i],
    'piml_probe_arith': [_p, _p, _p, _p, _p, _p, _i, _p],
    'piml_encoder_partial_floats': [],
    'piml_encoder_pack_floats': [],
    'piml_encoder_split_tiles': [_ll],
    'piml_encoder_split_tiles_train': [_ll],
    'piml_multi_copy': [ctypes.POINTER(_p), ctypes.POINTER(_p), ctypes.POINTER(_z), _i, _p],
    'piml_rollout_prologue': [_p] * 8 + [_i] * 4 + [_p] * 11 + [_p],
    'piml_rollout_losses_blocks': [_i, _i],
    'piml_rollout_losses': [_p, _p, _ll, _p, _p, _p, _p, _p, _i, _i, _i, _f, _p, _p, _p, _p, _p, _p, _p],
    'piml_rollout_losses_bwd': [_p, _p, _p, _p, _p, _p, _ll, _p, _p],
    'piml_rollout_losses_frames': [_p, _p, _ll, _p, _p, ctypes.POINTER(_p), _i, _p, _i, _i, _i, _f, _f, _f, _p, _p, _p, _p, _p, _p, _p],
    'piml_rollout_losses_frames_bwd': [_p, _p, _p, _p, _f, _f, _p, _p, _p, _ll, _p, _p],
    'piml_collision_pred_loss_blocks': [_ll, _i],
    'piml_collision_pred_loss': [ctypes.POINTER(_p), ctypes.POINTER(_p), _i, _ll, _i, _i, _p, _i, _i, _f, _p, _p, _p, _p, _p],
    'piml_collision_pred_loss_bwd': [_p, _p, _ll, _p, _p],
    'piml_adam_tickets': [],
    'piml_adam_step': [ctypes.POINTER(_p)] * 5 + [ctypes.POINTER(_ll), _i, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, _p, _p],
    'piml_pointwise_losses_blocks': [_ll, _ll, _i],
    'piml_pointwise_losses': [_p, _p, _ll, _ll, _p, _ll, _f, _p, _i, _p, _p, _p, _p, _p],
    'piml_p2p_alloc': [_z, ctypes.POINTER(_p)],
    'piml_p2p_free': [_p],
    'piml_p2p_export': [_p, _p],
    'piml_p2p_open': [_p, ctypes.POINTER(_p)],
    'piml_p2p_close': [_p],
    'piml_p2p_copy': [_p, _p, _z, _p],
    'piml_allgather_state_p2p': [_p, _z, _i, _i, ctypes.POINTER(_p), ctypes.POINTER(_p), ctypes.c_uint, ctypes.c_uint, _p, _p],
    'piml_encoder_products': [_i],
    'piml_relfeat_pack_form': [_i],
    'piml_relfeat_pack_plan': [_i, _i, _i, _i, _i, _i, _i, ctypes.POINTER(_i), ctypes.POINTER(_i)],
    'piml_relfeat_pack_tail_blocks': [_i, _i, _i, ctypes.POINTER(_i), _i],
    'piml_relfeat_plan': [_i] * 8 + [ctypes.POINTER(_i)] * 5,
    'piml_rowdecoder_products': [_i],
    'piml_encoder_dw2': [_i],
    'piml_encoder_fused_bwd': [_i],
    'piml_encoder_sums_bwd': [_i],
    'piml_encoder_sums_dec_slots': [_i],
    'piml_encoder_compact_rows': [_i],
    'piml_encoder_pack': [ctypes.POINTER(EncoderBranch), _i, _p],
    'piml_encoder_workgroups': [ctypes.POINTER(EncoderBranch), _i, ctypes.POINTER(_i)],
    'piml_encoder_fwd': [ctypes.POINTER(EncoderBranch), _i, _p],
    'piml_encoder_fwd_packed': [ctypes.POINTER(EncoderBranch), _i, _p],
    'piml_encoder_bwd': [ctypes.POINTER(EncoderBranch), _i, _p],
    'piml_encoder_bwd_acc': [ctypes.POINTER(EncoderBranch), _i, _i, _p],
    'piml_encoder_ksum': [_p, _ll, _i, _p, _p],
    'piml_decoder_pack_floats': [],
    'piml_decoder_partial_floats': [],
    'piml_decoder_workgroups': [_ll],
    'piml_decoder_fwd': [ctypes.POINTER(DecoderBranch), _i, _p, _f, _p, _p],
    'piml_decoder_bwd': [ctypes.POINTER(DecoderBranch), _i, _p, _p, _f, _p, _p],
    'piml_rowdecoder_slots': [_ll],
    'piml_rowdecoder_fwd': [ctypes.POINTER(DecoderBranch), _i, _p],
    'piml_rowdecoder_fwd_packed': [ctypes.POINTER(DecoderBranch), _i, _p],
    'piml_rowdecoder_bwd': [ctypes.POINTER(DecoderBranch), _i, _p],
    'piml_rowdecoder_bwd_acc': [ctypes.POINTER(DecoderBranch), _i, _i, _p],
    'piml_collision_head_pack_floats': [],
    'piml_collision_head_fwd': [_p, _ll, _p, _p, _p, _p, _p, _p, _p],
    'piml_head64_partial_floats': [],
    'piml_head64_slots': [_ll],
    'piml_head64_fwd': [ctypes.POINTER(Head64), _p],
    'piml_head64_bwd': [ctypes.POINTER(Head64), _p],
    'piml_head64_bwd_acc': [ctypes.POINTER(Head64), _i, _p],
    'piml_corrector_partial_floats': [_i],
    'piml_corrector_slots': [_i, _ll, _i],
    'piml_corrector_fwd': [ctypes.POINTER(Corrector), _p],
    'piml_corrector_bwd': [ctypes.POINTER(Corrector), _i, _p],
    'piml_pinnsf_pool_h2_ok': [ctypes.POINTER(EncoderBranch), _i],
    'piml_pinnsf_pool_train_ok': [ctypes.POINTER(EncoderBranch), _i],
    'piml_pinnsf_pool_msgs_ok': [ctypes.POINTER(EncoderBranch), _i],
    'piml_pinnsf_streams_init': [],
    'piml_pinnsf_pack_flush': [],
    'piml_pinnsf_slot_sums_flush': [],
    'piml_pinnsf_pack': [ctypes.POINTER(EncoderBranch), ctypes.POINTER(DecoderBranch), _i, ctypes.POINTER(CollisionHead),
                         _i, _p],
    'piml_pinnsf_fwd': [ctypes.POINTER(EncoderBranch), ctypes.POINTER(DecoderBranch), _i, ctypes.POINTER(CollisionHead),
                        _p, _f, _p, _i, _p],
    'piml_pinnsf_bwd': [ctypes.POINTER(EncoderBranch), ctypes.POINTER(DecoderBranch), _i, _p, _p, _f, _p, _i, _p],
    'piml_comm_available': [],
    'piml_comm_unique_id': [_p],
    'piml_comm_init': [ctypes.POINTER(_p), _i, _i, _p],
    'piml_comm_destroy': [_p],
    'piml_allgather_state': [_p, _p, _z, _p, _p],
    'piml_reducescatter_grad': [_p, _p, _p, _z, _p],
    'piml_allreduce_sum': [_p, _p, _z, _p],
    'piml_relfeat_fwd_self': [_p, _p, _p, _p, _i, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _f, _f, _f, _f, _p, _p, _p, _p, _p, _p, _p],
    'piml_relfeat_bwd_self': [_p, _p, _p, _p, _p, _p, _i, _p, _i, _i, _i, _i, _i, _i, _p, _p, _p, _p],
    'piml_relfeat_fwd_tick': [_p, _p, _p, _p, _i, _p, _p, _i, _i, _i, _i, _i, _i, _i, _f, _f, _f, _f,
                              _p, _p, _p, _i, _p, _p, _p, _p],
    'piml_relfeat_self_fwd': [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _f, _f, _f, _f, _p, _p, _p, _p, _p, _p, _p],
    'piml_relfeat_self_fwd_part': [_i, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _f, _f, _f, _f, _p, _p, _p, _p, _p, _p, _p],
    'piml_relfeat_self_bwd': [_p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _p, _p, _p, _p],
    'piml_relfeat_bwd_det': [_p, _p, _p, _p, _p, _p, _p, _p, _i, _p, _i, _i, _i, _i, _i, _i, _i, _p, _p, _p],
    'piml_relfeat_bwd': [_p, _p, _p, _p, _p, _p, _i, _p, _i, _i, _i, _i, _i, _i, _p, _p, _p],
}


class P2PMsg(ctypes.Structure):
    """piml_p2p_msg (include/piml_hip.h)."""
    _fields_ = [('scatter_src', _p), ('scatter_floats', _z), ('out_scatter', _p), ('n_bcast', _i),
                ('bcast_src', _p * 8), ('bcast_floats', _z * 8), ('out_bcast', _p * 8), ('sum', _i)]


SIGNATURES['piml_p2p_exchange'] = [ctypes.POINTER(P2PMsg), _i, _i, ctypes.POINTER(_p), ctypes.POINTER(_p), _z, _p, ctypes.c_uint, _p, _p]


class PimlHipError(RuntimeError):
    pass


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise PimlHipError(
                f'{LIB_PATH} is missing: build it with `python -m piml_amd.build` '
                '(hipcc --offload-arch=gfx950). piml_amd has no CPU fallback.')
        L = ctypes.CDLL(LIB_PATH)
        for name, args in SIGNATURES.items():
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = _i
        L.piml_encoder_split_tiles.restype = _ll
        L.piml_encoder_split_tiles_train.restype = _ll
        L.piml_mlapm_bwd_workspace_floats.restype = _ll
        L.piml_mlapm_fit_workspace_doubles.restype = _ll
        L.piml_mlapm_rollout_fit_workspace_doubles.restype = _ll
        L.piml_crowd_stats_workspace_bytes.restype = _ll
        L.piml_crowd_stats_voronoi_workspace_bytes.restype = _ll
        L.piml_pair_stats_workspace_bytes.restype = _ll
        L.piml_flow_stats_workspace_bytes.restype = _ll
        L.piml_view_stats_workspace_bytes.restype = _ll
        L.piml_track_stats_workspace_bytes.restype = _ll
        L.piml_obstacle_stats_workspace_bytes.restype = _ll
        L.piml_line_stats_workspace_bytes.restype = _ll
        L.piml_mlapm_law_table_bytes.restype = _ll
        L.piml_error_string.argtypes = [_i]
        L.piml_error_string.restype = ctypes.c_char_p
        if L.piml_abi_version() != ABI_VERSION:
            raise PimlHipError(f'{LIB_PATH}: ABI {L.piml_abi_version()} != expected {ABI_VERSION}; rebuild')
        _lib = L
    return _lib


def _demangle_lite(sym):
    """`_ZN4piml23enc_fwd_x3_kernelILi0EEEvNS_7EncArgsE` -> `enc_fwd_x3_kernel<0>`: the nested name's last component and
    its literal template arguments (bool / int), which is all this library's kernels use."""
    import re
    i = 2
    if sym[i:i + 1] == 'N':
        i += 1
    name = None
    while i < len(sym) and sym[i].isdigit():
        m = re.match(r'\d+', sym[i:])
        n = int(m.group())
        name = sym[i + m.end():i + m.end() + n]
        i += m.end() + n
    if name is None:
        return sym
    if sym[i:i + 1] == 'I':
        args, i = [], i + 1
        while sym[i:i + 1] == 'L':
            m = re.match(r'L([bi])(n?\d+)E', sym[i:])
            if not m:
                break
            v = int(m.group(2).replace('n', '-'))
            args.append(('true' if v else 'false') if m.group(1) == 'b' else str(v))
            i += m.end()
        if args:
            name += '<' + ', '.join(args) + '>'
    return name


def kernel_resource_usage(path=None):
    """{kernel name: {vgprs, agprs, vgpr_spill, sgpr_spill, scratch_bytes, lds_bytes, symbol}} of every kernel IN the library
    file (default: the one this process loads), read from the code objects' own metadata -- the NT_AMDGPU_METADATA notes of
    the gfx950 ELFs in the file's offload bundles -- not from a build log.  bench.py prints the entries of the step's kernels;
    tests/test_abi.py holds every kernel the default dispatch reaches to vgpr_spill == 0."""
    import struct
    import msgpack
    blob = open(path or LIB_PATH, 'rb').read()
    magic, out, at = b'__CLANG_OFFLOAD_BUNDLE__', {}, 0
    while True:
        at = blob.find(magic, at)
        if at < 0:
            break
        n, = struct.unpack_from('<Q', blob, at + 24)
        off = at + 32
        for _ in range(n):
            o, size, tl = struct.unpack_from('<QQQ', blob, off)
            triple = blob[off + 24:off + 24 + tl]
            off += 24 + tl
            elf = blob[at + o:at + o + size]
            if b'gfx950' not in triple or elf[:4] != b'\x7fELF':
                continue
            shoff, = struct.unpack_from('<Q', elf, 0x28)
            shentsize, shnum = struct.unpack_from('<HH', elf, 0x3A)
            for k in range(shnum):
                sh_type, = struct.unpack_from('<I', elf, shoff + k * shentsize + 4)
                if sh_type != 7:      # SHT_NOTE
                    continue
                q, sz = struct.unpack_from('<QQ', elf, shoff + k * shentsize + 0x18)
                end = q + sz
                while q + 12 <= end:
                    namesz, descsz, typ = struct.unpack_from('<III', elf, q)
                    q += 12 + ((namesz + 3) & ~3)
                    desc = elf[q:q + descsz]
                    q += (descsz + 3) & ~3
                    if typ != 32:     # NT_AMDGPU_METADATA
                        continue
                    for kd in msgpack.unpackb(desc, raw=False).get('amdhsa.kernels', []):
                        out[_demangle_lite(kd['.name'])] = {
                            'vgprs': kd.get('.vgpr_count'), 'agprs': kd.get('.agpr_count'),
                            'vgpr_spill': kd.get('.vgpr_spill_count'), 'sgpr_spill': kd.get('.sgpr_spill_count'),
                            'scratch_bytes': kd.get('.private_segment_fixed_size'),
                            'lds_bytes': kd.get('.group_segment_fixed_size'), 'symbol': kd['.name']}
        at += len(magic)
    return out


def check(err, what):
    if err != 0:
        raise PimlHipError(f'{what} failed: hipError {err} ({lib().piml_error_string(err).decode()})')


class StageTrace:
    """piml_trace_*: live time of every launch stage between `start()` and `stop()` on torch's current stream.
    stop() -> [(stage name, microseconds), ...] in launch order."""
    _START = ctypes.c_char_p(b'start')

    def start(self):
        check(lib().piml_trace_begin(), 'piml_trace_begin')
        lib().piml_trace_mark(self._START, torch.cuda.current_stream().cuda_stream)

    def stop(self):
        names = ctypes.create_string_buffer(4096)
        us = (_f * 64)()
        n = lib().piml_trace_end(names, 4096, us, 64)
        if n < 0:
            check(-n, 'piml_trace_end')
        return list(zip(names.value.decode().split('\n')[:n], [float(us[i]) for i in range(n)]))


class StreamTimer:
    """A pair of HIP events recorded on torch's current stream through the C ABI; works
    inside HIP-graph capture (torch.cuda.Event(external=True) is refused on ROCm)."""

    def __init__(self):
        self._e = [_p(), _p()]
        for e in self._e:
            check(lib().piml_timer_create(ctypes.byref(e)), 'piml_timer_create')

    def start(self):
        check(lib().piml_timer_record(self._e[0], torch.cuda.current_stream().cuda_stream), 'piml_timer_record')

    def stop(self):
        check(lib().piml_timer_record(self._e[1], torch.cuda.current_stream().cuda_stream), 'piml_timer_record')

    def elapsed_ms(self):
        ms = _f()
        check(lib().piml_timer_elapsed_ms(self._e[0], self._e[1], ctypes.byref(ms)), 'piml_timer_elapsed_ms')
        return float(ms.value)

    def __del__(self):
        try:
            for e in self._e:
                lib().piml_timer_destroy(e)
        except Exception:   # interpreter shutdown
            pass
