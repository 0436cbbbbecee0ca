/*
 * piml_hip.h -- C ABI of libpiml_hip.so, the MI355X (gfx950) implementation of PIML's
 * per-timestep pairwise hot path.
 *
 * The reference (tsinghua-fib-lab/PIML) is pure Python/PyTorch and has no FFI layer; the
 * entry points below are what a binding for this path binds (ctypes stub: INTEGRATION.md).
 * Each entry cites the reference interface it replaces (paths relative to the reference
 * repository root).
 *
 * Conventions
 *  - every pointer is a DEVICE pointer owned by the caller (torch allocates); float32,
 *    C-contiguous; `stream` is a hipStream_t passed as void* (NULL = default stream);
 *  - nothing is allocated, freed or synchronised inside: every call only enqueues work on
 *    `stream`, so calls are re-entrant and capturable into a hipGraph;
 *  - return value is a hipError_t as int (0 = hipSuccess, 1 = hipErrorInvalidValue for a
 *    rejected argument); no exceptions cross the boundary;
 *  - absent agents are NaN positions (the reference's sentinel, src/data/data.py:141-143),
 *    never compacted;
 *  - leading dimensions (channels, time) are flattened by the caller into C "slices".
 *
 * Where to start.  A host that replaces the reference's per-timestep path binds FIFTEEN of the entries below (INTEGRATION.md
 * sections 2 - 4); everything else in this header is the same path cut into components (for hosts that keep parts of the
 * reference's torch.nn network, and for the parity tests), and measurement plumbing / A-B switches live in piml_hip_tuning.h:
 *   features      piml_relfeat_self_fwd / piml_relfeat_self_bwd   (get_relative_features + the self_features cat, both ways)
 *                 piml_heading_fwd                                 (multi-frame windows: the temporal heading fill)
 *   network       piml_pinnsf_pack / piml_pinnsf_fwd / piml_pinnsf_bwd   (PINNSF.forward and its autograd, three calls)
 *   closed form   piml_mlapm_step_fwd / piml_mlapm_step_bwd_ws    (MLAPM.step and its analytic gradient)
 *   collisions    piml_collision_counts / piml_collision_label     (collision_detection(...).sum(-1), calculate_collision_label)
 *   integrator    piml_rollout_step / piml_train_step_fwd / piml_train_step_bwd   (the frame bodies of the two rollout loops)
 *   multi-GPU     piml_allgather_state + piml_reducescatter_grad (RCCL), or piml_p2p_exchange (P2P stores, capturable)
 */
#ifndef PIML_HIP_H
#define PIML_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped when a declared function changes its signature or a struct changes a field that exists.  Fields APPENDED to a struct and
 * added functions leave it alone (35 since the scenario structs): a caller built against an older header of the same version
 * must zero-fill the structs it passes to a newer library to their CURRENT size -- piml_amd/_lib.py and the library travel together. */
#define PIML_HIP_ABI_VERSION 35
#define PIML_MAX_TOPK 32 /* topk_ped / topk_obs upper bound (reference defaults 6 / 10) */

/* ABI version of the loaded library (== PIML_HIP_ABI_VERSION). */
int piml_abi_version(void);

/* hipGetErrorString for the codes returned below. */
const char* piml_error_string(int err);

/*
 * Heading direction.  Replaces Pedestrians.get_heading_direction
 * (src/data/data.py:350-395): zero-velocity frames are filled from the temporally nearest
 * non-zero frame (backward sweep then forward sweep), then h/|h| (|h| == 0 -> h/0.1).
 * velocity, heading: (C, T, N, 2).
 */
int piml_heading_fwd(const float* velocity, int C, int T, int N, float* heading, void* stream);

/*
 * Relative features, forward.  Replaces Pedestrians.get_relative_features
 * (src/data/data.py:466-512) = get_nearby_obj_in_sight (:416-447) + get_relative_quantity
 * (:397-414) + get_filtered_features (:449-464), for C slices of N agents and M shared
 * obstacle points, without materialising any N x N tensor.
 *
 *   position, velocity, acceleration : (C, N, .) per-agent records whose consecutive agents
 *             are `state_ld` floats apart: state_ld = 2 for three separate (C, N, 2) arrays,
 *             6 for one interleaved (C, N, 6) = (p, v, a) buffer (pass base, base+2, base+4),
 *             which is what the per-step all-gather of agent-block sharding produces
 *   destination : (C, focal_count, 2), destinations of the focal rows only
 *   heading : (C, N, 2) unit heading from piml_heading_fwd, or NULL = derive it from
 *             `velocity` (the T == 1 per-step case, where heading = v/|v|)
 *   obstacles : (M, 2), may be NULL when M == 0
 *   focal_begin, focal_count : the block of focal agents this call computes (multi-GPU
 *             agent-block sharding; single GPU: 0, N).  Sources are always all N agents.
 *   topk_ped/topk_obs : k (<= PIML_MAX_TOPK); effective k is min(k, N) / min(k, M)
 *   cos_thr_* : float32(cos(3.14 * sight_angle / 180))  (the reference's 3.14, quirk Q1)
 *   dist_thr_* : neighbours farther than this (strict >) are zero-padded
 * Outputs (row i = focal_begin + i):
 *   ped_feat (C, focal_count, kp_eff, 6) = (p_j - p_i, v_j - v_i, a_j - a_i), zero-padded
 *   obs_feat (C, focal_count, ko_eff, 6) = (o_j - p_i, -v_i, -a_i), zero-padded
 *   dest_feat (C, focal_count, 2) = destination - position, NaN -> 0; rows `dest_feat_ld` floats
 *             apart (2 = dense; 7 writes columns 0..1 of a (C, focal_count, 7) self_features buffer)
 *   ped_idx / obs_idx (int32, same leading shape, k_eff) : source index per slot, -1 = empty
 * NaN velocity / acceleration entries are read as 0 (the reference zeroes them in place
 * first, data.py:483-484; the host wrapper performs that in-place write).
 * Ordering rule: slots ascend by (distance, index); exact distance ties resolve to the
 * lower index (torch.sort leaves ties unspecified).
 */
int piml_relfeat_fwd(const float* position, const float* heading, const float* velocity,
                     const float* acceleration, int state_ld, const float* destination,
                     const float* obstacles, int C, int N, int M, int focal_begin,
                     int focal_count, int topk_ped, int topk_obs, float cos_thr_ped,
                     float cos_thr_obs, float dist_thr_ped, float dist_thr_obs,
                     float* ped_feat, float* obs_feat, float* dest_feat, int dest_feat_ld,
                     int32_t* ped_idx, int32_t* obs_idx, void* stream);

/* piml_relfeat_fwd + `*tick += 1` (a device-side int64 frame counter the kernel never reads): the captured inference
 * rollout frame (src/models/simulators.py:595-652) ends with this launch. */
int piml_relfeat_fwd_tick(const float* position, const float* heading, const float* velocity, const float* acceleration,
                          int state_ld, const float* destination, const float* obstacles, int C, int N, int M,
                          int focal_begin, int focal_count, int topk_ped, int topk_obs, float cos_thr_ped,
                          float cos_thr_obs, float dist_thr_ped, float dist_thr_obs, float* ped_feat, float* obs_feat,
                          float* dest_feat, int dest_feat_ld, int32_t* ped_idx, int32_t* obs_idx, long long* tick,
                          void* stream);
/* piml_relfeat_fwd / piml_relfeat_bwd with the model's self_features rows [dest - p, v, a, v0] (C, n, 7) in place of the
 * destination features: the per-frame torch.cat of the training rollout (src/models/simulators.py:778-779) inside the launch.
 * desired_speed (C, n); g_state_zero (C, N, 6; may be NULL): cleared by the forward launch for the backward to accumulate into.
 * bwd: g_self (C, n, 7); ACCUMULATES into g_state (C, N, 6) = d/d(p, v, a) (cleared by the caller / by the forward);
 * writes g_destination (C, n, 2) and g_speed (C, n; may be NULL). */
int piml_relfeat_fwd_self(const float* position, const float* heading, const float* velocity, const float* acceleration,
                          int state_ld, const float* destination, const float* obstacles, const float* desired_speed, int C,
                          int N, int M, int focal_begin, int focal_count, int topk_ped, int topk_obs, float cos_thr_ped,
                          float cos_thr_obs, float dist_thr_ped, float dist_thr_obs, float* ped_feat, float* obs_feat,
                          float* self_features, int32_t* ped_idx, int32_t* obs_idx, float* g_state_zero, void* stream);
int piml_relfeat_bwd_self(const float* g_ped_feat, const float* g_obs_feat, const float* g_self, const int32_t* ped_idx,
                          const int32_t* obs_idx, const float* position, int state_ld, const float* destination, int C, int N,
                          int focal_begin, int focal_count, int kp_eff, int ko_eff, float* g_state, float* g_destination,
                          float* g_speed, void* stream);


/*
 * piml_relfeat_fwd for ONE scene of packed (N, 6) = (p, v, a) records that also writes the model's self_features rows
 * [dest - p, v, a, v0] (n, 7) (src/models/simulators.py:169-173 builds them with a torch.cat per frame) and, when
 * `g_state_zero` (N * 6 floats) is given, clears it for the backward to accumulate into: one launch instead of three.
 * piml_relfeat_self_bwd is its backward in one launch: g_self (n, 7) = d/d(self_features); ACCUMULATES into the cleared
 * g_state (N, 6); writes g_destination (n, 2) and g_speed (n, may be NULL).
 */
int piml_relfeat_self_fwd(const float* state, const float* destination_rows, const float* obstacles,
                          const float* desired_speed, int N, int M, int focal_begin, int focal_count, int topk_ped,
                          int topk_obs, float cos_thr_ped, float cos_thr_obs, float dist_thr_ped, float dist_thr_obs,
                          float* ped_feat, float* obs_feat, float* self_features, int32_t* ped_idx, int32_t* obs_idx,
                          float* g_state_zero, void* stream);
/* The same in two launches for agent-block sharding: PIML_RELFEAT_LOCAL reads only the focal block's own records (and the
 * obstacles), so it can run while the all-gather of the other blocks is in flight; it writes obs_feat, self_features,
 * obs_idx and leaves its pedestrian list in ped_idx.  PIML_RELFEAT_REMOTE continues from that list over the agents either
 * side of the block and writes ped_feat / ped_idx.  Bit-identical to the single launch (part 0). */
#define PIML_RELFEAT_LOCAL 1
#define PIML_RELFEAT_REMOTE 2
int piml_relfeat_self_fwd_part(int part, const float* state, const float* destination_rows, const float* obstacles,
                               const float* desired_speed, int N, int M, int focal_begin, int focal_count, int topk_ped,
                               int topk_obs, float cos_thr_ped, float cos_thr_obs, float dist_thr_ped, float dist_thr_obs,
                               float* ped_feat, float* obs_feat, float* self_features, int32_t* ped_idx,
                               int32_t* obs_idx, float* g_state_zero, void* stream);
int piml_relfeat_self_bwd(const float* g_ped_feat, const float* g_obs_feat, const float* g_self, const int* ped_idx,
                          const int* obs_idx, const float* state, const float* destination_rows, int N, int focal_begin,
                          int focal_count, int kp_eff, int ko_eff, float* g_state, float* g_destination, float* g_speed,
                          void* stream);

/*
 * Relative features, backward: what autograd computes through gather / repeat / masked
 * zeroing in src/data/data.py:397-414, 449-464, 491-510.
 *   g_ped_feat (C, focal_count, kp_eff, 6), g_obs_feat (C, focal_count, ko_eff, 6),
 *   g_dest_feat (C, focal_count, 2) : upstream gradients
 *   ped_idx, obs_idx : as written by piml_relfeat_fwd
 *   position (stride state_ld), destination (focal rows) : forward inputs (only their NaN
 *             pattern is used)
 * Outputs:
 *   g_state (C, N, 6) : d/d(position, velocity, acceleration) concatenated per agent, for
 *             ALL N sources (a rank's partial sum under agent-block sharding); the kernel
 *             ACCUMULATES into it with float atomics, the caller zeroes it first;
 *   g_destination (C, focal_count, 2) : overwritten.
 */
int piml_relfeat_bwd(const float* g_ped_feat, const float* g_obs_feat, const float* g_dest_feat,
                     const int32_t* ped_idx, const int32_t* obs_idx, const float* position,
                     int state_ld, const float* destination, int C, int N, int focal_begin, int focal_count,
                     int kp_eff, int ko_eff, float* g_state, float* g_destination, void* stream);

/*
 * Deterministic piml_relfeat_bwd (same gradient, no atomics, bit-reproducible; slower -- opt-in): the caller supplies the
 * neighbour-list entries sorted by source: sorted_keys[e] = slice * N + ped_idx of entry e (C * N for an empty slot),
 * ascending, and order[e] = row * kp_eff + slot of that entry, in a STABLE order (C * focal_count * kp_eff int64 each).
 * accumulate != 0: g_state (C, N, 6) is added to instead of overwritten.  Every g_state element is written.
 */
int piml_relfeat_bwd_det(const float* g_ped_feat, const float* g_obs_feat, const float* g_dest_feat, const int* ped_idx,
                         const int* obs_idx, const long long* sorted_keys, const long long* order, const float* position,
                         int state_ld, const float* destination, int C, int N, int focal_begin, int focal_count,
                         int kp_eff, int ko_eff, int accumulate, float* g_state, float* g_destination, void* stream);

/*
 * Closed-form social-force step.  Replaces MLAPM.step (src/models/mlapm.py:10-58).
 *   position, velocity, destination (N, 2); desired_speed (N); variant 0 = 'raw', 1 = 'GC',
 *   2 = 'UCY' (with the one-line coll.unsqueeze(-1) fix the shipped code needs for N > 2);
 *   tau, A, B, C, D, theta_deg = self.args[...]; radius, dt = step() arguments.
 * Outputs: action (N, 2) = velocity + force * dt; force (N, 2) optional (NULL to skip).
 * skip_absent = 0: like the reference, a NaN position poisons every row (its callers filter absent
 * agents first, src/main_mlapm.py:19-25).  skip_absent = 1: agents with a NaN position are treated
 * as absent -- they exert no force and their own action is NaN -- which replaces that host-side
 * compaction and keeps shapes static (graph-capturable simulation loop).
 */
int piml_mlapm_step_fwd(const float* position, const float* velocity, const float* desired_speed,
                        const float* destination, int N, int variant, float tau, float A, float B,
                        float C, float D, float theta_deg, float radius, float dt, int skip_absent,
                        float* action, float* force, void* stream);

/*
 * One frame of the simulation loop of src/main_mlapm.py:18-36 in ONE launch: the state of frame t - 1 = *frame_counter - 1 is
 * read from the trajectories (frames, N, 2) themselves -- an agent within `radius` of its destination in a frame >= 1 is absent
 * (NaN) from the next frame on, absent agents contribute nothing (skip_absent) -- MLAPM.step's velocity and p + v dt are
 * written to frame t, and the last workgroup to finish sets *frame_counter = t + 1 (done_counter: a zeroed device word).
 * Frame 0 is the caller's initial state.  A launch with *frame_counter outside [1, frames) does nothing.
 */
int piml_mlapm_rollout_step(float* traj_position, float* traj_velocity, const float* desired_speed,
                            const float* destination, long long frames, int N, int variant, float tau, float A,
                            float B, float C, float D, float theta_deg, float radius, float dt,
                            long long* frame_counter, unsigned* done_counter, void* stream);

/*
 * Analytic gradient of piml_mlapm_step_fwd (what autograd gives through mlapm.py:10-58):
 * g_action (N, 2) -> g_position, g_velocity, g_destination (N, 2), g_desired_speed (N), all
 * overwritten.  view / rotation sign / collision flags are piecewise constant (no gradient).
 * No atomics: every pair is evaluated in both roles by the owning wavefront.
 */
int piml_mlapm_step_bwd(const float* g_action, const float* position, const float* velocity,
                        const float* desired_speed, const float* destination, int N, int variant,
                        float tau, float A, float B, float C, float D, float theta_deg, float radius,
                        float dt, float* g_position, float* g_velocity, float* g_desired_speed,
                        float* g_destination, void* stream);

/*
 * The same gradient with every ordered pair evaluated ONCE (N >= 512): a wavefront keeps 128 source agents in its lanes and
 * rotates 64 focal agents -- with their focal-side sums -- through them, the two sides leave as partial rows in `workspace`
 * (piml_mlapm_bwd_workspace_floats(N, variant) floats, 0 = this form does not apply) and a second launch adds an agent's
 * rows in a fixed order (UCY: the rotating pass gives every pair its flag-off term, the second launch -- a wavefront per
 * agent -- adds [flag on] - [flag off] for the pairs the exact predicate flags).  No atomics.  With workspace == NULL or a
 * small scene this IS piml_mlapm_step_bwd; a non-NULL workspace that is too small is hipErrorInvalidValue.
 */
long long piml_mlapm_bwd_workspace_floats(int N, int variant);
int piml_mlapm_step_bwd_ws(const float* g_action, const float* position, const float* velocity,
                           const float* desired_speed, const float* destination, int N, int variant,
                           float tau, float A, float B, float C, float D, float theta_deg, float radius,
                           float dt, float* g_position, float* g_velocity, float* g_desired_speed,
                           float* g_destination, float* workspace, long long workspace_floats, void* stream);

/*
 * Calibration of MLAPM's constants to a clip: loss and parameter gradient in one pass (mlapm_fit.hip).
 *   The clip is packed frame-major: entry e (E of them) is one agent present in one frame, state (E, 4) = (p, v),
 *   destination (E, 2), desired_speed (E), target (E, 2) (normally v of the next frame; NaN = no target).
 *   offsets (F + 1) int32: frame f holds entries [offsets[f], offsets[f + 1]), which are also its only sources;
 *   frame_of (E) int32.  small_focal (n_small) / big_focal (n_big): the entries with a target, of frames with
 *   <= 64 / > 64 entries (a lane / a wave per focal entry).  params (6) on the device = (tau, A, B, C, D, theta_deg).
 *   For every focal entry, pred = MLAPM.step of its frame (piml_mlapm_step_fwd's variants and arithmetic), and
 *   loss (1, float64) = sum |pred - target|^2 / focal count (0 without focal entries), grad (6, float32) = d loss / d params
 *   (view, rotation sign and the UCY flag are constant; constants a variant does not use get exactly 0).
 *   workspace: piml_mlapm_fit_workspace_doubles(n_small, n_big) float64 (-1 for negative counts).  Deterministic (no
 *   atomics, fixed-order float64 sums).  hipErrorInvalidValue before any launch for negative sizes,
 *   n_small + n_big > E, a variant outside 0..2, non-finite dt / radius, a NULL buffer that is needed, or a small workspace.
 */
long long piml_mlapm_fit_workspace_doubles(int n_small, int n_big);
int piml_mlapm_fit_loss_grad(const float* state, const float* destination, const float* desired_speed,
                             const float* target, const int* offsets, const int* frame_of, int E, int F,
                             const int* small_focal, int n_small, const int* big_focal, int n_big,
                             const float* params, int variant, float dt, float radius, double* workspace,
                             long long workspace_doubles, double* loss, float* grad, void* stream);

/*
 * Calibration of MLAPM's constants on multi-frame rollouts: loss and parameter gradient of H closed-loop steps per window,
 * forward and adjoint in one launch (mlapm_rollout_fit.hip).  Extends the one-step loss above to the reference's
 * multi-frame rollout training (multiple_rollout_mse_loss with time_decay, src/models/simulators.py:172-193, 659-832) on
 * the MLAPM law (src/models/mlapm.py:10-58, explicit Euler of src/main_mlapm.py:25).
 *   The windows are packed (piml_amd/calibrate.py pack_windows): window w (W of them) owns the slots
 *   [slot_offsets[w], slot_offsets[w + 1]) (S in all); entry (w, k, s) = (H + 1) slot_offsets[w] + k n_w + s, k = 0 .. H,
 *   holds rec_state (4) = the recorded (p, v) of frame t0 + k, destination (2) and flags (1 byte: bit 0 present, bit 1
 *   injected, bit 2 carried from k - 1); desired_speed (S) per slot.  small_windows (n_small): windows of <= 64 slots,
 *   H <= 48 (a lane per slot, states in LDS); big_windows (n_big) with big_base (n_big) = the prefix sum of their slot
 *   counts (big_slots in all): a wave per focal slot, states in the workspace.  params (6) on the device.
 *   Carried slots step v' = MLAPM.step over the slots present in k (piml_mlapm_step_fwd's variants and arithmetic),
 *   p' = p + v' dt; entering slots take their recorded state.  loss (1, float64) = sum_k,s w_k |p^ - P|^2 / sum w_k over
 *   the carried (k >= 1, slot), w_k = time_decay^(H - k) (0 without terms); grad (6, float32) = d loss / d params through
 *   the whole chain (view, rotation sign and the UCY flag are constant; unused constants exactly 0).  per_step (2 H
 *   float64, optional): the squared-error sums, then the term counts, of k = 1 .. H.
 *   workspace: piml_mlapm_rollout_fit_workspace_doubles(n_small + n_big, H, big_slots) float64 (-1 for negative sizes or
 *   H < 1).  Deterministic (no atomics, fixed-order float64 sums).  hipErrorInvalidValue before any launch for negative
 *   sizes, H < 1, small windows with H > 48, n_small + n_big > W, a variant outside 0..2, dt not finite and > 0, radius
 *   not finite and >= 0, time_decay not finite and >= 0, a NULL buffer that is needed, or a short workspace.
 */
long long piml_mlapm_rollout_fit_workspace_doubles(int n_windows, int horizon, long long big_slots);
int piml_mlapm_rollout_fit_loss_grad(const float* rec_state, const float* destination, const unsigned char* flags,
                                     const float* desired_speed, const int* slot_offsets, int W, long long S, int horizon,
                                     const int* small_windows, int n_small, const int* big_windows, const int* big_base,
                                     int n_big, long long big_slots, const float* params, int variant, float dt,
                                     float radius, double time_decay, double* workspace, long long workspace_doubles,
                                     double* loss, float* grad, double* per_step, void* stream);

/*
 * Collision matrix, pair part of Pedestrians.collision_detection (src/data/data.py:549-564):
 * coll (S, N, N) = [|p_j - p_i| < threshold] (- I when minus_identity), NaN -> 0; S slices.
 * With minus_identity = 0 it is the `real_position` matrix of data.py:576-581.
 */
int piml_collision_matrix(const float* position, int S, int N, float threshold, int minus_identity,
                          float* coll, void* stream);

/*
 * "Friends" filter of collision_detection, in place on coll (C, T, N, N):
 *   base != NULL : 3-D rule (data.py:573-591), C must be 1: pairs whose `base` (S_base, N, N)
 *                  sum over slices exceeds 25 are zeroed in all T slices (base may be coll);
 *   base == NULL : 4-D rule (data.py:592-598): per channel, pairs colliding in any of the first
 *                  4 frames are zeroed in every frame.
 */
int piml_collision_friends(float* coll, const float* base, int C, int T, int S_base, int N, void* stream);

/*
 * Fused collision_detection(position (S,N,2), thr_h).sum(-1) for n_thresholds thresholds
 * (device array) with the 3-D friends rule, without materialising (S,N,N):
 * counts (n_thresholds, S, N), overwritten.  Callers: src/models/simulators.py:708-724,
 * src/functions/metrics.py:16-26.
 */
/*
 * Rollout losses of the fine-tuning step (src/models/simulators.py:172-249 as assembled at :790-819), forward and the
 * gradient fields in ONE launch:  p (C, T, N, 2) predicted positions; labels (C, T, N, labels_ld) with the label position in
 * columns 0-1; mask_pred (C, T, N) int64 (!= 0: the agent is predicted in that frame); gates (T) bytes (!= 0: the frame has
 * a predicted agent at all); collisions / hard_collisions (C, T, N) counts or NULL; abnormal_mask (N) or NULL.
 *   p_res = where(mask & gate, p, 0), lab = where(mask, labels[..., :2], 0), decay_t = time_decay^(T - 1 - t)
 *   out[0] = sum (p_res - lab)^2 decay_t                                       (multiple_rollout_mse_loss, reduction 'sum')
 *   out[1] = sum [sum_t collisions > 0] abnormal ((p_res - (p_res.n) n) - (lab - (lab.n) n))^2 decay_t,
 *            n = (lab[T-1] - lab[0]) / (|.| + 1e-6)                            (multiple_rollout_collision_loss, 'sum')
 *   out[2] = the same with hard_collisions
 * g_mse / g_coll / g_hard (C, T, N, 2) = d out[i] / d p.  piml_rollout_losses_bwd: g_p = sum_i *g_out_i * g_i, the three
 * upstream gradients as device scalars (NULL = 0).  The sums
 * run in a fixed order.  partial: 6 * piml_rollout_losses_blocks(C, N) floats, ticket: one zeroed unsigned (left zero);
 * both only used when piml_rollout_losses_blocks(C, N) > 1.
 */
/* n device-to-device copies (dst[i] <- src[i], bytes[i] bytes; the ranges of one pair do not overlap) in one launch per 24
 * pairs: the tensors of a training batch into the static inputs of the captured step (src/models/simulators.py:699-779). */
int piml_multi_copy(void* const* dst, const void* const* src, const size_t* bytes, int n, void* stream);
/* The prologue of the differentiable training rollout in one launch (src/models/simulators.py:672-697, :707): frame t_start of
 * position / velocity / acceleration / destination (C, T, N, 2) and dest_idx (C, T, N) int64 copied out, new_flag =
 * (long(mask_p - mask_p_pred) == 1) as bytes, mask_pred = long(mask_p_pred), gates[t] = (sum over (c, n) of mask_pred > 0) as
 * bytes and as floats, speed = self_features[..., t_start, :, 6], *nan_flag = 0. */
int piml_rollout_prologue(const float* position, const float* velocity, const float* acceleration, const float* destination,
                          const long long* dest_idx, const float* mask_p, const float* mask_p_pred, const float* self_features,
                          int C, int T, int N, int t_start, float* p0, float* v0, float* a0, float* d0, long long* di0,
                          unsigned char* new_flag, long long* mask_pred, unsigned char* gates, float* gates_f, float* speed,
                          int* nan_flag, void* stream);
int piml_rollout_losses_blocks(int C, int N);
int piml_rollout_losses(const float* p, const float* labels, long long labels_ld, const long long* mask_pred,
                        const unsigned char* gates, const float* collisions, const float* hard_collisions,
                        const float* abnormal_mask, int C, int T, int N, float time_decay, float* out, float* g_mse,
                        float* g_coll, float* g_hard, float* partial, unsigned* ticket, void* stream);
int piml_rollout_losses_bwd(const float* g_out0, const float* g_out1, const float* g_out2, const float* g_mse,
                            const float* g_coll, const float* g_hard, long long n, float* g_p, void* stream);
/* piml_rollout_losses on the collision count records of the frames AS PRODUCED, with the statistics the step logs and the
 * weighted total: count_frames = HOST array of T device pointers, frame t's (2, C, N) floats [collisions | hard collisions]
 * (piml_collision_counts of its positions; NULL = zeros), gated here by gates[t] (src/models/simulators.py:708-715, :728);
 * focus != 0: they also weight the two collision-focus sums (:800-819).  out (12 floats): [0] mse, [1] focus sum of the
 * collisions, [2] of the hard collisions, [3] sum of the gated collisions, [4] of the hard ones, [5] number of entries with
 * mask_pred == 1, [6] total = mse + w_coll [1] + w_hard [2], [7] w_coll [1], [8] w_hard [2].  T <= 32.
 * bwd: upstream gradients of [0], [7], [8] and [6] (device scalars; the first three may be NULL, the last not). */
int piml_rollout_losses_frames(const float* p, const float* labels, long long labels_ld, const long long* mask_pred,
                               const unsigned char* gates, const float* const* count_frames, int focus,
                               const float* abnormal_mask, int C, int T, int N, float time_decay, float w_coll, float w_hard,
                               float* out, float* g_mse, float* g_coll, float* g_hard, float* partial, unsigned* ticket,
                               void* stream);
int piml_rollout_losses_frames_bwd(const float* g_mse_out, const float* g_collw_out, const float* g_hardw_out,
                                   const float* g_total_out, float w_coll, float w_hard, const float* g_mse, const float* g_coll,
                                   const float* g_hard, long long n, float* g_p, void* stream);

/* The collision-prediction loss of `pinnsf_bm` over the frames of a training rollout (src/models/simulators.py:731-733 per frame,
 * :826-830 behind the loop) in ONE launch: pred_frames / feature_frames = HOST arrays of nframes (<= 32) device pointers, frame f's
 * predictions (n = windows * agents * k values in (0, 1), the model's last output) and pedestrian features (n rows of feature_ld >= 4
 * floats: relative position, relative velocity -- the label is calculate_collision_label of them, src/data/data.py:514-535); frame f
 * is rollout frame t_start + f of T_total, gates (T_total floats, 0 / 1) = the reference's per-frame `if torch.sum(mask) > 0`.
 *     out[0] = weight * F.binary_cross_entropy(pred * gate, label * gate, reduction='sum')   (logarithms clamped at -100)
 *     out[1] = sum(round(pred * gate) == label * gate) / (T_total * n)                         (frames outside the rollout: equal)
 * grad (nframes, n) = d out[0] / d pred (binary_cross_entropy_backward's (p - y) / max((1 - p) p, 1e-12)).  partial (2 floats per
 * workgroup of piml_collision_pred_loss_blocks) and a zeroed ticket are needed when that is > 1.  bwd: g_pred = *g_loss * grad
 * (g_loss NULL = 1), n = nframes * n values. */
int piml_collision_pred_loss_blocks(long long n, int nframes);
int piml_collision_pred_loss(const float* const* pred_frames, const float* const* feature_frames, int nframes, long long n, int k,
                             int feature_ld, const float* gates, int t_start, int T_total, float weight, float* out, float* grad,
                             float* partial, unsigned* ticket, void* stream);
int piml_collision_pred_loss_bwd(const float* g_loss, const float* grad, long long n, float* g_pred, void* stream);

/* The losses of a pointwise pre-training batch (src/models/simulators.py:333-352, pinnsf_interaction 'sim') and their gradients in ONE
 * launch: pred (rows, 2), labels (rows, labels_ld >= 6 [+ k]) -- columns 4, 5 the acceleration label, 6 .. 6 + k - 1 the collision labels
 * --, msgs (nmsg values, the model's second output) or NULL (reg_weight == 0), coll_pred (rows, k) (the model's last output,
 * `pinnsf_bm` under collision_pred_weight > 0) or NULL.
 *     out[1] = F.mse_loss(pred, labels[:, 4:6], 'sum')   out[2] = sum(reg_weight |msgs|)   out[3] = F.binary_cross_entropy(coll_pred,
 *     labels[:, 6:], 'sum')   out[0] = out[1] (+ out[2]) (+ out[3])
 * grad = [2 rows | nmsg | rows k] floats: d out[0] / d (pred | msgs | coll_pred); its backward is piml_collision_pred_loss_bwd (a copy
 * scaled by the upstream gradient).  partial (3 floats per workgroup of piml_pointwise_losses_blocks) and a zeroed ticket when > 1. */
/* One Adam step of n parameter tensors in ONE launch (the optimiser of both training loops: torch.optim.Adam(model.parameters(), lr,
 * weight_decay), src/models/simulators.py:69-71, :104-129, stepped at :319 / :358-359): params / grads / exp_avg / exp_avg_sq / steps =
 * HOST arrays of n device pointers (float32, contiguous; steps: one float counter per tensor, as torch keeps them with
 * capturable=True), sizes their element counts.  Per tensor: step += 1; grad += weight_decay * param; exp_avg = beta1 exp_avg +
 * (1 - beta1) grad; exp_avg_sq = beta2 exp_avg_sq + (1 - beta2) grad^2; param -= (lr / (1 - beta1^step)) exp_avg / (sqrt(exp_avg_sq) /
 * sqrt(1 - beta2^step) + eps) -- torch's fused kernel operation for operation (doubles for the hyper-parameters), bitwise equal to it.
 * A tensor is cut into pieces of 1024 elements, one workgroup each; the tensor's last workgroup out (tickets) writes its counter. */
int piml_adam_tickets(void);   /* unsigned counters `tickets` must hold (zeroed once; every launch leaves them zero) */
int piml_adam_step(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq, float* const* steps,
                   const long long* sizes, int n, double lr, double beta1, double beta2, double weight_decay, double eps,
                   unsigned* tickets, void* stream);

int piml_pointwise_losses_blocks(long long rows, long long nmsg, int k);
int piml_pointwise_losses(const float* pred, const float* labels, long long labels_ld, long long rows, const float* msgs, long long nmsg,
                          float reg_weight, const float* coll_pred, int k, float* out, float* grad, float* partial, unsigned* ticket,
                          void* stream);


int piml_collision_counts(const float* position, int S, int N, const float* thresholds, int n_thresholds,
                          float* counts, void* stream);
/* The same for up to 32 frames of a training rollout in ONE launch (src/models/simulators.py:708-715 counts every frame on its
 * own): frames[f] = a HOST array of device pointers to (S, N, 2) tensors, S <= 25 slices each (independent slices, as in
 * piml_collision_counts below 26); counts (nframes, n_thresholds, S, N): record f is what a call on frame f alone writes. */
int piml_collision_counts_frames(const float* const* frames, int nframes, int S, int N, const float* thresholds,
                                 int n_thresholds, float* counts, void* stream);

/*
 * The same counts for stacks of MORE than 25 slices (the evaluation's (t, N, 2) rollouts) in parallel form: needs
 * `totals_zeroed`, n_thresholds * N * N int32 of caller scratch, zero on entry (it holds the per-pair collision totals
 * of the friends rule afterwards).  n_thresholds <= 4.  piml_collision_counts itself needs no scratch (one wavefront
 * per agent) and is the slower choice there.
 */
int piml_collision_counts_scratch(const float* position, int S, int N, const float* thresholds, int n_thresholds,
                                  int* totals_zeroed, float* counts, void* stream);
/* The same result from a per-frame cell grid (N <= 8192): one workgroup per slice bins its positions into cells of 1.02 x the
 * largest threshold and tests the 3 x 3 block around every agent -- O(N x occupancy) pair tests per slice instead of N^2;
 * two launches (totals, then counts), totals_zeroed as above. */
int piml_collision_counts_grid(const float* position, int S, int N, const float* thresholds, int n_thresholds,
                               int* totals_zeroed, float* counts, void* stream);


/*
 * Pedestrians.calculate_collision_label (src/data/data.py:514-535): rows of >= 4 floats
 * (dp, dv, ...), `row_stride` floats apart -> label[rows] in {0, 1}.
 */
int piml_collision_label(const float* ped_features, size_t rows, int row_stride, float* label, void* stream);

/*
 * Evaluation metrics, every frame in ONE launch (one workgroup per frame, no host sync).  x: (F, n, 2), y: (F, m, 2)
 * positions; mask_x (F, n) / mask_y (F, m): uint8 presence (non-zero = present), NULL = every point present.  Each frame's
 * present points are compacted in slot order, as the reference's p[mask == 1] does; absent slots are never read (they may
 * hold NaN).  A NaN in a present point makes that frame's result NaN.  Limits: 0 <= n, m <= 4096 (n != m allowed).
 * Deterministic: no atomics, the same inputs give the same bits.
 *
 * Entropic OT.  Replaces SinkhornDistance.forward (src/functions/metrics.py:129-187) as ot_with_time_mask (:45-67) and
 * wasserstein_distance_2d (:94-97) call it on one frame: log-domain Sinkhorn with uniform marginals, the cost
 * C_ij = |x_i - y_j|^2 recomputed (never stored), at most max_iter iterations, the frame stopping after the iteration whose
 * err = sum_i |u_i - u_i'| is < thresh (the reference's break, :161-172, 2-D input).  Float32 arithmetic as the reference's,
 * the final sum(exp(M) * C) accumulated in float64.  cost (F) float32, iters (F) int32 = iterations run; u (F, n) and
 * v (F, m) (each may be NULL) = the final potentials at the frame's slots, 0 at absent ones.
 * A frame with an empty side (the reference cannot run one) returns, leaves the other frames alone and has cost 0.  No
 * present point in x: err is 0, so with thresh > 0 the loop stops after its first iteration (iters = min(1, max_iter)), and
 * that iteration sets v to +inf at y's present slots.  Points in x but none in y: err is inf, then NaN, so iters = max_iter,
 * and u is +inf at x's present slots (max_iter >= 1).  One point a side: the squared distance, u + v = it.
 * hipErrorInvalidValue: F, n or m < 0, n or m > 4096, eps <= 0 (or NaN), max_iter < 0, a NULL x / y (with points) or
 * cost / iters.  F == 0 is a no-op.
 */
int piml_sinkhorn_frames(const float* x, const float* y, const unsigned char* mask_x, const unsigned char* mask_y, int F,
                         int n, int m, float eps, int max_iter, float thresh, float* cost, int* iters, float* u, float* v,
                         void* stream);

/*
 * Multi-kernel Gaussian MMD.  Replaces MaximumMeanDiscrepancy.__call__ / guassian_kernel (src/functions/metrics.py:207-273)
 * as mmd_with_time_mask (:70-91) and mmd_loss (:100-104) call it on one frame: bandwidth = sum L2 / ((n+m)^2 - (n+m)) over
 * the frame's (n+m)^2 pairs unless fix_sigma != 0 (Python truthiness: 0 means "computed"), divided by
 * kernel_mul^(kernel_num // 2); K = sum_i exp(-L2 / (bandwidth * kernel_mul^i)), i < kernel_num <= 8;
 * out[f] = XX / n^2 + YY / m^2 - XY / (n m) - YX / (m n) (an empty block adds 0).  float64 from the float32 positions on,
 * out (F) float32.  All points coinciding give bandwidth 0 and NaN, as in the reference.  With one side empty the result is
 * the other side's block alone (YY / m^2 or XX / n^2, the bandwidth from its points); one point in total gives NaN
 * ((n+m)^2 - (n+m) == 0), no point at all gives 0.
 * hipErrorInvalidValue: F, n or m < 0, n or m > 4096, kernel_num outside 1..8, a NULL x / y (with points) or out.
 * F == 0 is a no-op.
 */
int piml_mmd_frames(const float* x, const float* y, const unsigned char* mask_x, const unsigned char* mask_y, int F, int n,
                    int m, double kernel_mul, int kernel_num, double fix_sigma, float* out, void* stream);

/*
 * Crowd-dynamics statistics without agent pairing (crowdstats.hip), S members x T frames in one call.
 * P, V (S, T, N, 2) positions / velocities, M (S, T, N) presence, float32.  Agent i is present in slice (s, t) when
 * M == 1 and both coordinates of P are finite; it has a speed when both components of V are finite too.  n_active (S)
 * int32 or NULL: member s's slots at or past n_active[s] are not swept (they never held an agent).  Frames [t0, t1)
 * (T' = t1 - t0).  A present agent is focal when has_box == 0 or x0 <= x < x1 and y0 <= y < y1.  For every focal agent:
 *   rho = sum_j exp(-|p_j - p_i|^2 / R^2) / (pi R^2) over the slice's present j (j = i included), no cut-off;
 *   u = sqrt(vx^2 + vy^2); bin = min(floor(rho / rho_bin), rho_bins - 1); cell (floor((x - x0) / cell),
 *   floor((y - y0) / cell)), dropped outside [0, gx) x [0, gy); all of these in float32, the divisions true divisions.
 * Outputs: n, n_speed (S, T') int64 focal agents / those with a speed; sum_speed, sum_density (S, T') float64;
 * fd_count (S, rho_bins) int64, fd_sum, fd_sum2 (S, rho_bins) float64 = count, sum u, sum u^2 over the focal agents with a
 * speed of every frame; map (S, gy, gx) int64 focal agent-frames per cell (has_box only; zeroed by the call);
 * density (S, T', N) float32 or NULL: rho at focal agents, NaN elsewhere.  workspace: at least
 * piml_crowd_stats_workspace_bytes(S, T', rho_bins) bytes (-1 for negative arguments).  One memset (map) and two launches,
 * no host synchronisation (capturable).  Deterministic: no float atomics (the map counts are 64-bit integer atomics);
 * member s's results are bitwise those of an S = 1 call on member s alone.
 * hipErrorInvalidValue: S, T or N <= 0, frames outside [0, T] or empty, R <= 0 or not finite, rho_bin <= 0, rho_bins
 * outside 1..256, with a box: a non-finite or empty box, cell <= 0, gx or gy < 1 or a NULL map; a NULL input, output or
 * workspace, or a workspace too small.
 */
long long piml_crowd_stats_workspace_bytes(int S, int frames, int rho_bins);
int piml_crowd_stats(const float* P, const float* V, const float* M, const int* n_active, int S, int T, int N, int t0, int t1,
                     float radius, int has_box, float x0, float x1, float y0, float y1, float cell, int gx, int gy,
                     float rho_bin, int rho_bins, long long* n, long long* n_speed, double* sum_speed, double* sum_density,
                     long long* fd_count, double* fd_sum, double* fd_sum2, long long* map, float* density, void* workspace,
                     long long workspace_bytes, void* stream);

/*
 * The same statistics on the Voronoi local density of Steffen and Seyfried (2010) (voronoi.hip).  Inputs,
 * presence, frames, the focal box, speed, bin, map cell, every sum and every output are those of piml_crowd_stats; with
 * has_bounds a focal agent must also lie inside the walkable rectangle (bx0 <= x < bx1, by0 <= y < by1).  rho = 1 / area
 * of the agent's cell.  dirs: a host array of `sides` (3..32) unit vectors (x, y pairs, counter-clockwise), copied into the
 * kernel arguments.  In coordinates relative to p_i, in float32 without contraction:
 *   the cell starts as the polygon with vertices cutoff * dirs[k];
 *   with has_bounds it is clipped by x >= bx0 - x_i, x <= bx1 - x_i, y >= by0 - y_i, y <= by1 - y_i, in this order;
 *   then, in slot order, by q . d <= |d|^2 / 2, d = p_j - p_i, for every present agent j of the slice below the member's
 *   bound; pairs with |d|^2 >= 4 cutoff^2 (they cannot cut) or |d|^2 == 0 (i itself; coincident agents share one cell) are
 *   skipped.  Obstacles do not bound cells.
 * A clip keeps the vertices with signed distance s <= 0 and adds, on every edge whose ends differ in that, the point
 * v_in + t (v_out - v_in), t = s_in / (s_in - s_out); on a side of the rectangle that point's coordinate along the normal
 * is the side's own.  The area is the shoelace sum over the final vertices with float64 products and a float64 sum,
 * rounded to float32; rho = 1 / area is a float32 true division.  The polygon holds 64 vertices: an agent whose polygon
 * would pass that in the course of the clips, or whose area is not > 0, is left out of every statistic, has density NaN
 * and adds 1 to dropped[s].  dropped (S) int64, zeroed by the call.  workspace: at least
 * piml_crowd_stats_voronoi_workspace_bytes(S, T', N, rho_bins) bytes (-1 for negative arguments).  Two memsets and three
 * launches, no host synchronisation (capturable).  Deterministic: no float atomics (map and dropped are 64-bit integer
 * atomics); member s's results are bitwise those of an S = 1 call on member s alone.
 * hipErrorInvalidValue: everything piml_crowd_stats refuses (its radius aside); cutoff <= 0 or not finite; sides outside
 * 3..32; a NULL dirs or dropped; with has_bounds, a non-finite or empty rectangle.
 */
long long piml_crowd_stats_voronoi_workspace_bytes(int S, int frames, int N, int rho_bins);
int piml_crowd_stats_voronoi(const float* P, const float* V, const float* M, const int* n_active, int S, int T, int N, int t0,
                             int t1, float cutoff, const float* dirs, int sides, int has_bounds, float bx0, float bx1,
                             float by0, float by1, int has_box, float x0, float x1, float y0, float y1, float cell, int gx,
                             int gy, float rho_bin, int rho_bins, long long* n, long long* n_speed, double* sum_speed,
                             double* sum_density, long long* fd_count, double* fd_sum, double* fd_sum2, long long* map,
                             float* density, long long* dropped, void* workspace, long long workspace_bytes, void* stream);

/*
 * Time-to-collision and pair-distance statistics without agent pairing (pairstats.hip), S members in one
 * call.  P, V (S, T, N, 2), M (S, T, N) float32; n_active (S) int32 or NULL as for piml_crowd_stats.  Agent i takes part
 * in slice (s, t) when M == 1 and both coordinates of P and both components of V are finite (slots at or past
 * n_active[s] are not swept); it is focal when it takes part and has_box == 0 or x0 <= x < x1 and y0 <= y < y1.  lags:
 * a host array of K (0..8) positive, ascending frame counts, copied into the kernel arguments; lag index 0 is L = 0.
 * Pair slice (s, t, k) for t0 <= t and t + L_k < t1 pairs every focal i of frame t with every participant j != i (as a
 * slot) of frame t + L_k, ordered pairs.  Per pair in float32 (true divisions and square roots, no contraction):
 * d = p_j - p_i, w = v_j - v_i, c = |d|^2 - R^2, b = d.w, a = |w|^2; distance sqrt(|d|^2); pairs with distance >= r_max
 * are skipped entirely (r_max <= 0: no cut-off); overlap when c < 0; otherwise a collision course when b < 0 and
 * disc = b^2 - a c >= 0, tau = c / (-b + sqrt(disc)).  Outputs, int64, zeroed by the call:
 *   focal, pairs, overlap (S, K + 1): focal agent-frames, ordered pairs evaluated, overlapping pairs;
 *   ttc (S, K + 1, tau_bins): collision-course pairs by floor(tau / tau_bin), where that is < tau_bins;
 *   dist (S, K + 1, r_bins): pairs by floor(distance / r_bin), where that is < r_bins;
 *   nn (S, r_bins + 1): lag 0, each focal agent's smallest distance bin, r_bins when none is below r_bins * r_bin;
 *   min_ttc (S, tau_bins + 1): lag 0, each focal agent's smallest tau bin, tau_bins when none is below tau_bins * tau_bin.
 * A lag that reaches past the frames has no slices and zero counts.  workspace: at least
 * piml_pair_stats_workspace_bytes(S, K, tau_bins, r_bins) bytes (-1 for negative arguments).  One memset and two
 * launches, no host synchronisation (capturable).  Deterministic: integer counts only, added with integer atomics;
 * member s's results are bitwise those of an S = 1 call on member s alone.
 * hipErrorInvalidValue: S, T or N <= 0, N > 65536 (the per-slice u32 counters), frames outside [0, T] or empty, K outside
 * 0..8, lags NULL (K > 0), not positive or not ascending, R <= 0 or not finite, r_max NaN, tau_bin or r_bin <= 0 or not
 * finite, tau_bins or r_bins outside 1..256, a non-finite or empty box, a NULL input, output or workspace, or a
 * workspace too small.
 */
long long piml_pair_stats_workspace_bytes(int S, int K, int tau_bins, int r_bins);
int piml_pair_stats(const float* P, const float* V, const float* M, const int* n_active, int S, int T, int N, int t0, int t1,
                    const int* lags, int K, float radius, float r_max, int has_box, float x0, float x1, float y0, float y1,
                    float tau_bin, int tau_bins, float r_bin, int r_bins, long long* focal, long long* pairs,
                    long long* overlap, long long* ttc, long long* dist, long long* nn, long long* min_ttc, void* workspace,
                    long long workspace_bytes, void* stream);

/*
 * Collective-motion statistics (flowstats.hip), S members in one call: the velocity-velocity correlation over
 * distance, the lane order parameter of Rex and Loewen (2007) and the velocity field.  P, V, M, n_active, the frames
 * [t0, t1) and the box as for piml_pair_stats.  Agent i takes part in slice (s, t) when M == 1, both coordinates of P are
 * finite and both components of V are finite and below 1024 in magnitude; it is focal when it takes part and has_box == 0
 * or x0 <= x < x1 and y0 <= y < y1.  A mover has s = sqrt(vx^2 + vy^2) >= v_min and the heading h = v / s; a lane mover has
 * |v.e| >= v_min along e = (ex, ey) and the direction sign(v.e).  Same-frame ordered pairs only, in float32 (true divisions
 * and square roots, no contraction), d = p_j - p_i, Q = 2^20.  Outputs, int64:
 *   corr_pairs, corr_sum (S, r_bins): focal mover i, mover j != i (as a slot), r = sqrt(|d|^2) < r_max, by floor(r / r_bin)
 *     where that is < r_bins: the pairs and the sum of llrintf((h_i.h_j) Q);
 *   lane_n, lane_sum, lane_same, lane_opp, dir_plus, dir_minus (S, T'): focal lane mover i counts the lane movers j != i
 *     with |d.(-ey, ex)| < lane_width and |d.e| < lane_length as n_same (equal direction) or n_opp; dir_plus / dir_minus
 *     count the focal lane movers by direction; those with n_same + n_opp > 0 add 1 to lane_n, llrintf(phi Q) with
 *     phi = ((n_same - n_opp) / (n_same + n_opp))^2 to lane_sum, n_same to lane_same and n_opp to lane_opp;
 *   map_n, map_vx, map_vy (S, gy, gx), has_box only: every focal participant adds 1, llrintf(vx Q), llrintf(vy Q) to the cell
 *     (floor((x - x0) / cell), floor((y - y0) / cell)) of piml_crowd_stats when it lies in the grid.
 * workspace: at least piml_flow_stats_workspace_bytes(S, r_bins, gx, gy) bytes (gx = gy = 0 without a box; -1 for negative
 * arguments).  One memset and two launches, no host synchronisation (capturable).  Deterministic: integer outputs only,
 * added with integer atomics; member s's results are bitwise those of an S = 1 call on member s alone.  S, T' or N == 0:
 * success, nothing is done.
 * hipErrorInvalidValue, before any HIP call: S, T or N < 0, N > 65536 (the per-slice u32 counters), frames outside [0, T]
 * or t1 < t0, v_min, r_bin, r_max, lane_width or lane_length <= 0 or not finite, r_bins outside 1..256,
 * | |e|^2 - 1 | > 1e-4, a non-finite or empty box, cell <= 0, gx or gy < 1; then, unless there is nothing to do, a NULL
 * input, output (the maps with a box only) or workspace, or a workspace too small.
 */
long long piml_flow_stats_workspace_bytes(int S, int r_bins, int gx, int gy);
int piml_flow_stats(const float* P, const float* V, const float* M, const int* n_active, int S, int T, int N, int t0, int t1,
                    float v_min, float r_bin, int r_bins, float r_max, float ex, float ey, float lane_width,
                    float lane_length, int has_box, float x0, float x1, float y0, float y1, float cell, int gx, int gy,
                    long long* corr_pairs, long long* corr_sum, long long* lane_n, long long* lane_sum, long long* lane_same,
                    long long* lane_opp, long long* dir_plus, long long* dir_minus, long long* map_n, long long* map_vx,
                    long long* map_vy, void* workspace, long long workspace_bytes, void* stream);

/*
 * Heading-frame pair statistics (viewstats.hip), S members in one call: where the others are in a walking
 * agent's own frame.  P, V, M, n_active, the frames [t0, t1), the lags and the box as for piml_pair_stats.  Agent i takes
 * part in slice (s, t) as for piml_flow_stats (M == 1, P finite, both components of V below 1024 in magnitude, slot below
 * n_active[s]); a mover has sp = sqrt(vx^2 + vy^2) >= v_min and the heading h = v / sp.  Focal: a participant mover of frame t
 * with has_box == 0 or x0 <= x < x1 and y0 <= y < y1.  Pair slice (s, t, k) for t0 <= t and t + L_k < t1 pairs every focal i of
 * frame t with every participant j != i (as a slot) of frame t + L_k, mover or not, ordered pairs.  Per pair in float32 (true
 * divisions and square roots, no contraction): d = p_j - p_i, r = sqrt(dx^2 + dy^2); pairs with r >= r_max are skipped
 * entirely (r_max <= 0: no cut-off); a = dx hx + dy hy is the distance ahead, l = dy hx - dx hy the distance to the left;
 * class c = 0 when j is not a mover, otherwise with q = h_i.h_j: 1 (with) if q >= cos_same, 2 (against) if q <= -cos_same, 3
 * (across) else; with X = (float)(cell * half) formed on the host, cx = floor((a + X) / cell), cy = floor((l + X) / cell) and
 * G = 2 half.  Outputs, int64, zeroed by the call, Q = 2^20:
 *   focal, pairs (S, K + 1): focal agent-frames, ordered pairs evaluated;
 *   map (S, K + 1, 4, G, G): pairs by [c][cy][cx] where 0 <= cx, cy < G;
 *   nn_map (S, G G + 1): lag 0, each focal agent's nearest source (smallest r, ties to the lowest slot) by cy G + cx; G G when
 *     it lies outside the map or the agent has no source;
 *   front_gap (S, gap_bins + 1): lag 0, per focal agent the smallest a over the sources with a > 0 and |l| < corridor by
 *     b = floor(a / gap_bin); gap_bins when b >= gap_bins or nobody is in front;
 *   front_speed (S, gap_bins): the sum of llrintf(sp_i Q) over the focal agents of front_gap's bin b < gap_bins.
 * A lag that reaches past the frames has no slices and zero counts.  workspace: at least
 * piml_view_stats_workspace_bytes(S, K, half, gap_bins) bytes (-1 for negative arguments).  One memset and two launches, no
 * host synchronisation (capturable).  Deterministic: integer outputs only, added with integer atomics; member s's results
 * are bitwise those of an S = 1 call on member s alone.
 * hipErrorInvalidValue, before any HIP call: S, T or N <= 0, N > 65536 (the per-slice u32 counters), frames outside [0, T] or
 * empty, K outside 0..8, lags NULL (K > 0), not positive or not ascending, v_min, cell, corridor or gap_bin <= 0 or not
 * finite, half outside 1..16, cos_same outside [0, 1], r_max NaN, gap_bins outside 1..256, a non-finite or empty box, a NULL
 * input, output or workspace, or a workspace too small.
 */
long long piml_view_stats_workspace_bytes(int S, int K, int half, int gap_bins);
int piml_view_stats(const float* P, const float* V, const float* M, const int* n_active, int S, int T, int N, int t0, int t1,
                    const int* lags, int K, float v_min, float cell, int half, float cos_same, float r_max, float corridor,
                    float gap_bin, int gap_bins, int has_box, float x0, float x1, float y0, float y1, long long* focal,
                    long long* pairs, long long* map, long long* nn_map, long long* front_gap, long long* front_speed,
                    void* workspace, long long workspace_bytes, void* stream);

/*
 * Track statistics (trackstats.hip), S members in one call: what an agent does along its own track.  Slot n of
 * member s is one agent for the whole run; P (S, T, N, 2) and M (S, T, N) float32, n_active (S) int32 or NULL and the frames
 * [t0, t1) as for piml_pair_stats; velocities are not an input.  Agent i takes part at (s, t) when M == 1 and both
 * coordinates of P are finite and below 65536 in magnitude; slots at or past n_active[s] are not swept.  float32 (true
 * divisions and square roots, no contraction), Q = 2^20, t an index into the window (T' = t1 - t0 frames):
 *   step (i, t): i takes part at t and t + 1; u = p(t+1) - p(t), l = sqrt(ux^2 + uy^2); a mover when l / dt >= v_min, with the
 *     heading h = u / l.  Nothing requires presence between two frames that are compared.
 * Outputs, int64:
 *   ac_n, ac_sum (S, n_lags): lag L = 1 .. n_lags, every t where steps t and t + L are movers: 1 and llrintf((h_t.h_{t+L}) Q);
 *   msd_n, msd_sum, msd_far (S, n_lags): every t where i takes part at t and t + L, d = p(t+L) - p(t), d2 = dx^2 + dy^2:
 *     sqrt(d2) < d_max adds 1 to msd_n and llrintf(d2 Q) to msd_sum, otherwise 1 to msd_far;
 *   acc (S, acc_bins + 1), acc_sum (S): every t where steps t and t + 1 exist, a = sqrt(|u_{t+1} - u_t|^2) / dt / dt: bin
 *     min(floor(a / acc_bin), acc_bins) (the last bin is open), and llrintf(a Q) where a < acc_bin * acc_bins;
 *   trk_frames, trk_steps, trk_first, trk_last, trk_path, trk_net (S, N): per track the frames taking part, the steps, the
 *     first and last participating frame (-1 without one), sum llrintf(l Q) over its steps, and llrintf(|p(last) - p(first)| Q)
 *     (0 with fewer than two frames).
 * One workgroup per track; the span [first, last] is staged in LDS tiles of PIML_TRACK_TILE frames with a halo of n_lags,
 * PIML_TRACK_LAG_LANES lags per pass, one lag per lane.
 * workspace: at least piml_track_stats_workspace_bytes(S, n_lags, acc_bins) = S (5 n_lags + acc_bins + 2) 8 bytes (-1 for
 * negative arguments).  One memset and two launches, no host synchronisation (capturable).  Deterministic: integer outputs
 * only, added with integer atomics; member s's results are bitwise those of an S = 1 call on member s alone.  S, T' or
 * N == 0: success, nothing is done.
 * hipErrorInvalidValue, before any HIP call: S, T or N < 0, N > 65536, frames outside [0, T] or t1 < t0, T' > 2^25, dt, v_min, d_max or
 * acc_bin <= 0 or not finite, d_max > 1024, n_lags outside 1..PIML_TRACK_MAX_LAGS, acc_bins outside 1..256,
 * d_max^2 Q N T' >= 2^63 or acc_bin acc_bins Q N T' >= 2^63 (the 64-bit sums); then, unless there is nothing to do, a NULL
 * input, output or workspace, or a workspace too small.
 */
#define PIML_TRACK_TILE 1024
#define PIML_TRACK_LAG_LANES 128
#define PIML_TRACK_MAX_LAGS 512
long long piml_track_stats_workspace_bytes(int S, int n_lags, int acc_bins);
int piml_track_stats(const float* P, const float* M, const int* n_active, int S, int T, int N, int t0, int t1, float dt,
                     float v_min, int n_lags, float d_max, float acc_bin, int acc_bins, long long* ac_n, long long* ac_sum,
                     long long* msd_n, long long* msd_sum, long long* msd_far, long long* acc, long long* acc_sum,
                     long long* trk_frames, long long* trk_steps, long long* trk_first, long long* trk_last,
                     long long* trk_path, long long* trk_net, void* workspace, long long workspace_bytes, void* stream);

/*
 * Obstacle statistics (obstaclestats.hip), S members in one call against one shared list of obstacle points:
 * clearance, contacts, crossings and time to wall.  P, V, M, n_active, the frames [t0, t1) and the box as for
 * piml_pair_stats; obs (O, 2) float32.  Agent i takes part at (s, t) when M == 1, both coordinates of P are finite and below
 * 65536 in magnitude and both components of V are finite and below 1024 in magnitude (slots at or past n_active[s] are not
 * swept); it is focal when it takes part and has_box == 0 or x0 <= x < x1 and y0 <= y < y1.  An obstacle point is valid when
 * both coordinates are finite; the others are skipped, and with no valid point only focal and steps count.  float32 (true
 * divisions and square roots, no contraction), Q = 2^20, t an index into the window (T' = t1 - t0 frames).  For a focal
 * (i, t) and every valid point q, e = q - p(t):
 *   clearance r = sqrt(min_q |e|^2); a contact when r < radius;
 *   time to wall: c = |e|^2 - radius^2, b = -(e.v), a = |v|^2; on a collision course when c >= 0, b < 0 and
 *     disc = b^2 - a c >= 0, then tau = c / (-b + sqrt(disc)); tau_min = min_q tau;
 *   a step (i, t) exists when i is focal at t, takes part at t + 1 and t + 1 < T': u = p(t+1) - p(t), len2 = |u|^2,
 *     s = min(max((e.u) / len2, 0), 1) (0 when len2 == 0), m = sqrt(min_q |e - s u|^2); a hit when m < hit_radius (the
 *     step's segment touches the obstacle, even when neither end is in contact).
 * The minima are exact in float32 whatever the order of the points.  Outputs, int64:
 *   focal, steps, contact, hit (S): the focal agent-frames, the steps, the contacts and the hits;
 *   clear (S, r_bins + 1): every focal agent-frame by min(floor(r / r_bin), r_bins) (the last bin is open); clear_speed (S,
 *     r_bins + 1): the sum of llrintf(sqrt(|v|^2) Q) over the same items per bin; clear_sum (S): the sum of llrintf(r Q) over
 *     the items with r < r_bin * r_bins;
 *   swept (S, r_bins + 1): every step by min(floor(m / r_bin), r_bins);
 *   min_ttc (S, tau_bins + 1): every focal agent-frame by floor(tau_min / tau_bin) where that is < tau_bins, else (no
 *     collision course, or beyond the range) bin tau_bins;
 *   trk_frames, trk_contacts, trk_hits, trk_min (S, N): per track its focal frames, contacts and hits, and
 *     llrintf(Q min(r, 2^24)) of its smallest r (-1 without a focal frame).
 * One lane per focal agent-frame; the points are staged in LDS tiles of PIML_OBS_TILE, the skipped ones filtered out while
 * staging.  dt (seconds per frame) is checked and recorded by the callers; no device quantity depends on it.
 * workspace: at least piml_obstacle_stats_workspace_bytes(S, N, r_bins, tau_bins) = S (3 r_bins + tau_bins + 9 + 4 N) 8
 * bytes (-1 for negative arguments).  One memset and two launches, no host synchronisation (capturable).  Deterministic:
 * integer outputs only, added with integer atomics; member s's results are bitwise those of an S = 1 call on member s
 * alone.  S, T', N or O == 0: success, nothing is done (the outputs are left alone).
 * hipErrorInvalidValue, before any HIP call: S, T, N or O < 0, N > 65536, O > 2^24, frames outside [0, T] or t1 < t0, dt,
 * radius, hit_radius, r_bin or tau_bin <= 0 or not finite, r_bins or tau_bins outside 1..256, a non-finite or empty box,
 * 1449 Q N T' >= 2^63 (clear_speed: a speed is below sqrt(2) 1024 < 1449) or r_bin r_bins Q N T' >= 2^63 (clear_sum); then,
 * unless there is nothing to do, a NULL input, output or workspace, or a workspace too small.
 */
#define PIML_OBS_TILE 4096
long long piml_obstacle_stats_workspace_bytes(int S, int N, int r_bins, int tau_bins);
int piml_obstacle_stats(const float* P, const float* V, const float* M, const int* n_active, int S, int T, int N, int t0,
                        int t1, const float* obs, int O, float dt, float radius, float hit_radius, int has_box, float x0,
                        float x1, float y0, float y1, float r_bin, int r_bins, float tau_bin, int tau_bins, long long* focal,
                        long long* steps, long long* contact, long long* hit, long long* clear_sum, long long* clear,
                        long long* clear_speed, long long* swept, long long* min_ttc, long long* trk_frames,
                        long long* trk_contacts, long long* trk_hits, long long* trk_min, void* workspace,
                        long long workspace_bytes, void* stream);

/*
 * Measurement-line statistics (linestats.hip), S members in one call against L shared lines: crossings, the
 * N-t curve, crossing speed, lateral profile and per track the first crossing.  P (S, T, N, 2), M (S, T, N), n_active and
 * the frames [t0, t1) as for piml_track_stats (velocities are not an input; slot n of a member is one agent for the whole
 * run); lines (L, 4) float32, each row (ax, ay, bx, by).  Agent i takes part at (s, t) when M == 1 and both coordinates of
 * P are finite and below 65536 in magnitude (slots at or past n_active[s] are not swept).  A step (i, t) exists when i takes
 * part at t and t + 1 and t + 1 < T' (T' = t1 - t0; no step spans a gap).  float32 (true divisions and square roots, no
 * contraction), Q = 2^20.  Per line, d = b - a, len2 = dx dx + dy dy, side(p) = dx (py - ay) - dy (px - ax); for a step
 * s0 = side(p(t)), s1 = side(p(t+1)):
 *   direction 0 when s0 < 0 and s1 >= 0, direction 1 when s0 >= 0 and s1 < 0 (a point on the line is on the left side);
 *   f = s0 / (s0 - s1), u = p(t+1) - p(t), c = p(t) + f u, w = ((cx - ax) dx + (cy - ay) dy) / len2;
 *   a crossing when 0 <= w < 1 (half-open: collinear lines sharing an end point count a crossing once between them);
 *   vn = |s1 - s0| / sqrt(len2) / dt; tc = t Q + llrintf(f Q).
 * Outputs, int64:
 *   cross (S, L, 2): crossings per direction; nt (S, L, 2, T'): crossings whose step starts at frame t (entry T' - 1 is 0);
 *   speed (S, L, 2, v_bins + 1): by min(floor(vn / v_bin), v_bins) (the last bin is open); speed_sum (S, L, 2): the sum of
 *     llrintf(vn Q) over the crossings with vn < v_bin * v_bins;
 *   profile (S, L, 2, w_bins): by min(floor(w w_bins), w_bins - 1);
 *   steps (S): the steps swept; trk_steps (S, N): the steps of each track;
 *   trk_count (S, L, N): the track's crossings of the line, both directions; trk_first (S, L, N): its smallest tc (-1
 *     without a crossing); trk_dir (S, L, N): the direction of that crossing (-1 without one): the minimum is taken over
 *     2 tc + dir, so time and direction come from the same step and direction 0 is the first of two at the same tc.
 * A line the host has not checked (a == b, non-finite) counts no crossing.  One lane per track over PIML_LINE_CHUNK steps,
 * the lanes of a workgroup on neighbouring slots; the lines are held in LDS; every row takes integer atomics directly.
 * workspace: at least piml_line_stats_workspace_bytes(S, N, L, T', v_bins, w_bins) =
 * S (2 L (T' + v_bins + w_bins + 3) + 1 + N + 2 L N) 8 bytes (-1 for negative arguments).  One memset and two launches (one
 * when T' == 1), no host synchronisation (capturable).  Deterministic: integer outputs only, added with integer atomics;
 * member s's results are bitwise those of an S = 1 call on member s alone.  S, T', N or L == 0: success, nothing is done
 * (the outputs are left alone).
 * hipErrorInvalidValue, before any HIP call: S, T or N < 0, N > 65536, L outside 0..PIML_LINE_MAX_L, frames outside [0, T]
 * or t1 < t0, T' > 2^25 (tc and the packed word stay far below 2^63), dt or v_bin <= 0 or not finite, v_bins or w_bins outside
 * 1..256, v_bin v_bins Q N T' >= 2^63 (speed_sum); then, unless there is nothing to do, a NULL input, output or workspace,
 * or a workspace too small.
 */
#define PIML_LINE_MAX_L 16
#define PIML_LINE_CHUNK 32
long long piml_line_stats_workspace_bytes(int S, int N, int L, int frames, int v_bins, int w_bins);
int piml_line_stats(const float* P, const float* M, const int* n_active, int S, int T, int N, int t0, int t1,
                    const float* lines, int L, float dt, float v_bin, int v_bins, int w_bins, long long* cross, long long* nt,
                    long long* speed, long long* speed_sum, long long* profile, long long* steps, long long* trk_steps,
                    long long* trk_count, long long* trk_first, long long* trk_dir, void* workspace,
                    long long workspace_bytes, void* stream);

/*
 * Group statistics (groupstats.hip), S members in one call: who walks with whom.  P (S, T, N, 2), M (S, T, N),
 * n_active and the frames [t0, t1) as for piml_line_stats (velocities are not an input; slot n of a member is one agent for
 * the whole run).  Agent i takes part at (s, t) when M == 1, both coordinates of P are finite and below 65536 in magnitude
 * and i < n_active[s].  A step (i, t) exists when i takes part at t and t + 1 and t + 1 < T' (T' = t1 - t0); its
 * displacement is u_i(t) = p_i(t+1) - p_i(t), metres per frame.  float32 with separately rounded products, true square
 * roots and divisions and no contraction, Q = 2^20.  The caller makes each threshold once in float64 and rounds it once:
 * r2 = radius^2, dv2 = (dv_max dt)^2, vm2 = (v_min dt)^2.  A pair-frame (i, j, t), i < j, exists when both steps exist at
 * t; with e = p_j(t) - p_i(t) and g = u_j(t) - u_i(t) it is together when ex ex + ey ey < r2, gx gx + gy gy < dv2,
 * |u_i|^2 >= vm2 and |u_j|^2 >= vm2 (each sum the x term plus the y term).  co[i, j] counts the pair-frames, near[i, j] the
 * together ones; a pair is a candidate when near >= min_frames.
 *
 * piml_group_pairs (pass 1): edges (S, max_edges, 4) int32 rows (i, j, co, near), one per candidate, in any order; n_edges
 * (S) int32 the true number of candidates, also when it exceeds max_edges (rows past max_edges are not written; rows past
 * n_edges are left alone); trk_steps, trk_path (S, N) int64 the steps of each track and the sum of llrintf(sqrtf(|u|^2) Q)
 * over them; pairs, together (S) int64 the pair-frames swept and the together ones.  One workgroup per (member, focal
 * track), the focal staged in LDS in tiles of PIML_GROUP_TILE frames, one lane per partner, one integer atomic per wave to
 * append.  Three memsets and one launch, no host synchronisation (capturable).  The cost grows as S N^2 times the frames
 * present.
 *
 * piml_group_members (pass 2): links (K, 3) int32 rows (member, i, j); over every together pair-frame of a link, with
 * d2 = ex ex + ey ey, d = sqrtf(d2), w = u_i + u_j, w2 = wx wx + wy wy:
 *   dist (S, r_bins + 1): by min(floor(d / r_bin), r_bins); dist_sum (S): the sum of llrintf(d Q);
 *   abreast (S, a_bins): by min(floor(c a_bins), a_bins - 1), c = fabsf(ex wx + ey wy) / (sqrtf(d2) sqrtf(w2)) (bin 0: side
 *     by side; the last bin: in file); abreast_skipped (S): the pair-frames with d2 == 0 or w2 == 0 instead;
 *   link_frames (S): the together pair-frames of the member's links.
 * All int64; a member without links gives zeros; a link with an index out of range is skipped.  Five memsets and one
 * launch (none for K == 0 or T' == 1).
 *
 * Deterministic: integer outputs, integer atomics; member s's results are bitwise those of an S = 1 call on member s alone
 * (its edge rows up to their order).  S, T' or N == 0: success, nothing is done (the outputs are left alone).
 * hipErrorInvalidValue, before any HIP call: S, T or N < 0, N > 65536, frames outside [0, T] or t1 < t0, T' > 2^25, r2 or
 * dv2 <= 0 or not finite, vm2 < 0 or not finite, sqrt(r2) Q N^2 / 2 T' >= 2^63 (dist_sum), min_frames < 1, max_edges < 0,
 * n_links < 0, r_bin <= 0 or not finite, r_bins or a_bins outside 1..256; then, unless there is nothing to do, a NULL
 * input or output (edges may be NULL when max_edges == 0, links when K == 0).
 */
#define PIML_GROUP_TILE 256
int piml_group_pairs(const float* P, const float* M, const int* n_active, int S, int T, int N, int t0, int t1, float r2,
                     float dv2, float vm2, int min_frames, int max_edges, int* edges, int* n_edges, long long* trk_steps,
                     long long* trk_path, long long* pairs, long long* together, void* stream);
int piml_group_members(const float* P, const float* M, int S, int T, int N, int t0, int t1, const int* links, int n_links,
                       float r2, float dv2, float vm2, float r_bin, int r_bins, int a_bins, long long* dist,
                       long long* dist_sum, long long* abreast, long long* abreast_skipped, long long* link_frames,
                       void* stream);

/*
 * The host half of the group statistics on the device (groupstats.hip): the link rule, the connected
 * components of the links and the sizes of the groups, for S members in ONE launch with no host read -- what stands between
 * piml_group_pairs and piml_group_members.  edges (S, cap, 4) int32 rows (i, j, co, near) in any order, as piml_group_pairs
 * writes them, and n_edges (S) int32 its true counts: min(max(n_edges[s], 0), cap) rows of member s are read, the others
 * never.  trk_steps, trk_path (S, N) int64 as piml_group_pairs writes them.  A row is a link when
 * near 1024 >= share_q co in 64-bit integers (and both indices lie in [0, N): any other row is no link); a track is eligible
 * when trk_steps >= min_frames; the groups are the connected components of the links.
 *   candidates (S) int64 = n_edges; links (S) int64 the rows that are links;
 *   group_id (S, N) int32: the smallest slot of the track's component, -1 for a track that is not eligible;
 *   size_tracks, size_path, size_steps (S, g_max + 1) int64: at index k = min(size, g_max) the eligible tracks in groups of
 *     that many eligible tracks and the sums of their trk_path and trk_steps (index 0 stays 0);
 *   workspace (S, N) int32 scratch; status (S) int32: 0, or 1 when member s's labels had not settled after N rounds (they
 *     always do: a non-zero word is a defect of the kernel and its rows are not to be used).
 * Every output element is written by the launch itself: nothing is zeroed before and nothing accumulates across calls.
 * One workgroup of 256 lanes per member: labels start at their own slot in the group_id row; a round lowers both ends of
 * every link to the smaller label (integer atomic minimum) and then jumps label[x] to label[label[x]], until a round
 * changes nothing; the sizes by integer atomics, the tables in LDS.  Integers only, so the result is the same bit for bit
 * whatever the order of the rows and of the lanes, and equal to piml_amd.groupstats.host_rows on the same rows.  One launch,
 * capturable.  S or N == 0: success, nothing is done.
 * hipErrorInvalidValue, before any HIP call: S, N or cap < 0, N > 65536, g_max outside 1..64, min_frames < 1, share_q
 * outside 1..1024; then, unless there is nothing to do, a NULL pointer (edges may be NULL when cap == 0).
 */
int piml_group_components(const int* edges, const int* n_edges, const long long* trk_steps, const long long* trk_path, int S,
                          int N, int cap, int min_frames, int share_q, int g_max, long long* candidates, long long* links,
                          int* group_id, long long* size_tracks, long long* size_path, long long* size_steps, int* workspace,
                          int* status, void* stream);

/*
 * utils.calc_acceleration (src/utils/utils.py:31-100): version 0/1/2 = 'v0'/'v1'/'v2' with the
 * caller-supplied constants (A, B, C, D, theta [rad]); rows of >= 2 floats -> acc (rows, 2).
 */
int piml_calc_acceleration(const float* relative_data, size_t rows, int row_stride, int version, float A,
                           float B, float C, float D, float theta, float eps, float* acc, void* stream);

/*
 * Fused per-frame epilogue of the inference rollout: the body of
 * BaseSimulator.get_multiple_rollouts between the model call and the feature recomputation
 * (src/models/simulators.py:596-639, 651) in one launch.  For every (slice, agent):
 *   record (p, v, a) and the presence mask of frame t; v' = v + a dt, p' = p + v dt (lagged
 *   Euler); waypoint switch when |p - dest| < 0.5; past the last waypoint the agent leaves the
 *   scene (p' = NaN, only if remove_arrived); agents entering at frame t+1 are re-initialised
 *   from the ground-truth series; history-velocity shift; columns 2.. of the next self_features
 *   row = (history, a', desired speed)  [columns 0..1 are written by piml_relfeat_fwd].  NaN
 *   components of v', a' are stored as 0 in the state and in the row's a' columns, as the feature
 *   recomputation writes them into its arguments (src/data/data.py:483-484); the history keeps them.
 * State (C,N,.) is updated IN PLACE; a_next (C,N,2) is the model's prediction.  Series are
 * (C,T,N,.); new_flag (C,T+1,N) uint8 (frame T all zero); F = hist_width + 5; waypoints
 * (D,N,2) shared (waypoints_per_slice = 0) or (C,D,N,2).  The frame index t is read from DEVICE
 * memory (frame_counter), so one captured launch serves every frame of a replayed hipGraph.
 */
int piml_rollout_step(float* position, float* velocity, float* acceleration, float* destination,
                      int64_t* dest_idx, float* hist_velocity, int hist_width, const float* a_next,
                      const float* waypoints, int D, int waypoints_per_slice, const int64_t* dest_num,
                      const float* position_series, const float* velocity_series,
                      const float* acceleration_series, const float* destination_series,
                      const int64_t* dest_idx_series, const float* self_features_series, int F,
                      const uint8_t* new_flag, float* position_out, float* velocity_out,
                      float* acceleration_out, float* mask_out, float* self_features_next,
                      const float* desired_speed, const int64_t* frame_counter, int C, int T, int N,
                      float dt, int remove_arrived, void* stream);

/* piml_rollout_step with the bottleneck variants' network epilogue in front of it (piml_pinnsf_epilogue_ksum_fwd's arithmetic: the sum
 * of the agent's kp / ko per-neighbour predictions pred_ped (C N kp, 2) [+ pred_obs (C N ko, 2) or NULL] + the desired-force
 * term of its self_features row, per-row norm): an inference frame of `pinnsf_bm` / `pinnsf_bottleneck` needs one launch for
 * both.  The self_features read are the rows of `self_features_next` BEFORE this launch rewrites them (F must be 7); a_next is
 * ignored (may be NULL). */
int piml_rollout_step_ksum(const float* pred_ped, int kp, const float* pred_obs, int ko, float tau, float* position,
                           float* velocity, float* acceleration, float* destination, int64_t* dest_idx, float* hist_velocity,
                           int hist_width, const float* a_next, const float* waypoints, int D, int waypoints_per_slice,
                           const int64_t* dest_num, const float* position_series, const float* velocity_series,
                           const float* acceleration_series, const float* destination_series,
                           const int64_t* dest_idx_series, const float* self_features_series, int F, const uint8_t* new_flag,
                           float* position_out, float* velocity_out, float* acceleration_out, float* mask_out,
                           float* self_features_next, const float* desired_speed, const int64_t* frame_counter, int C, int T,
                           int N, float dt, int remove_arrived, void* stream);

/*
 * Open-world scenario frame (ABI 35).  Replaces the simulation loop the reference stubs (BaseSimulator.run /
 * run_single_step, src/models/simulators.py:834-838) around a scenario's update function -- GC's arrival rule and Poisson
 * arrivals (src/data/scenarios.py:313-401), utils.route (src/utils/utils.py:141-165) -- and the frame protocol of
 * RawData.add_frame / add_pedestrians (src/data/data.py:206-303), one launch per frame.  Storage is append-only: the agent
 * of global ordinal n lives in slot n (as add_pedestrians appends); ordinals >= capacity are dropped, counted, never written.
 * This block is the frame that piml_scenario_step, piml_scenario_step_rules and piml_scenario_step_members share (one
 * kernel); piml_scenario_step runs it under GC's rule, the other two state what they change.
 *
 * init == 0, frame t -> t+1 (t = *frame_counter, read on the device):
 *   every slot i < min(spawned[t & 1], capacity) with mask[i] == 1: v' = v + a dt, p' = p + v dt, a' = a_next[i]; the
 *   history shift and columns 2.. of its self_features row (history, a', v0) as piml_rollout_step; flag += 1 when
 *   |p' - dest| or the distance from p' to entry exit_idx[flag] is < arrival_radius; then flag == D or a NaN
 *   waypoint[flag] retires the agent for good (p, dest = NaN, v, a = 0, mask 0), otherwise dest = waypoint[flag];
 *   k = Poisson(rate dt) draw of frame t+1 (k = #{j < spawn_cap : u24 >= poisson_thresholds[j]}) new agents of ordinals
 *   spawned[t & 1] + j, one wave each: distinct uniform origin / destination entries, uniform point + U[0,1)^2 spawn_offset,
 *   waypoints (route(o, d), d, NaN...), exit_idx of each, v0 = max(speed_min, speed_mean + speed_std z) (speed_mean if
 *   uniform_speed), v = a = history = 0, flag 0, mask 1; spawned[(t+1) & 1] = spawned[t & 1] + k,
 *   *dropped = max(0, spawned - capacity), spawn_out[t+1] = k;
 *   frame t+1's p, v, a, dest, mask are written to the (T, capacity, .) outputs when t+1 < T.
 * init == 1: the n_initial agents (ordinals 0 ..) spawn into frame t through the same path; a_next unused.
 * The Philox word layout of the draws is documented in piml_amd/csrc/scenario.hip.  Columns 0..1 of self_features (the
 * destination features) are piml_relfeat_fwd's.  Slots nobody has written (absent, not yet spawned) are the caller's to
 * initialise (NaN positions / destinations, zero masks).  No atomics; the spawned count is ping-ponged by frame parity.
 * hipErrorInvalidValue: capacity or T < 1, hist_width < 2, F != hist_width + 5, D outside 2..8, E < 2, P < 1, R < 2,
 * n_initial outside 0..4096, route_max_iters outside 0..64, spawn_cap outside 0..8, dt <= 0, thresholds above 2^24 or
 * decreasing, init not 0 / 1, a NULL buffer (spawn_out and spawn_iters may be NULL), a NULL a_next with init == 0.
 */
typedef struct piml_scenario {
    float *position, *velocity, *acceleration, *destination; /* (capacity, 2) state, in place */
    float* hist_velocity;                                   /* (capacity, hist_width) */
    float* self_features;                                   /* (capacity, F) */
    float* desired_speed;                                   /* (capacity) */
    float* mask;                                            /* (capacity) 1 = present */
    int* flag;                                              /* (capacity) index of the current waypoint */
    float* waypoints;                                       /* (D, capacity, 2) */
    int* exit_idx;                                          /* (D, capacity) entry nearest each waypoint */
    int* spawn_iters;                                       /* (capacity) route iterations of each agent, or NULL */
    float *position_out, *velocity_out, *acceleration_out, *destination_out; /* (T, capacity, 2) */
    float* mask_out;                                        /* (T, capacity) */
    int* spawn_out;                                         /* (T) agents spawned per frame, or NULL */
    const int64_t* frame_counter;                           /* t */
    int64_t* spawned;                                       /* [2], by frame parity: agents spawned through the frame */
    int64_t* dropped;                                       /* [1] */
    const float* entries;                                   /* (E, P, 2) */
    const float* route_polyline;                            /* (R, 2) */
    int hist_width, F, D, E, P, R, capacity, T, n_initial, route_max_iters, spawn_cap, uniform_speed;
    float dt, spawn_offset, route_clearance, arrival_radius, speed_mean, speed_std, speed_min;
    uint64_t seed;
    uint32_t poisson_thresholds[8];                         /* ceil(2^24 P(K <= j)), j < spawn_cap */
} piml_scenario;
int piml_scenario_step(const piml_scenario* s, const float* a_next, int init, void* stream);

/*
 * Scene rules of piml_scenario_step_rules (ABI 35, additive): piml_scenario_step's frame with the reference's synthetic
 * scenes (src/data/scenarios.py:9-311, crosswalk / four_directional_square / basic_unit1..3) in place of GC's entry pairs,
 * route and exit distance.
 * spawn_law (what a new agent of ordinal n looks like; word layout in piml_amd/csrc/scenario.hip):
 *   PIML_SPAWN_GC          GC (scenarios.py:369-387): piml_scenario_step, arrival_rule must be PIML_ARRIVE_GC
 *   PIML_SPAWN_CROSSWALK   scenarios.py:36-65: |x| = length/2 + 3u on a coin side, y = +-width/2 on a coin side,
 *                          waypoints (-side_x length/2, +-width/2 by a coin) and (same x, 3 y), heading (0, -side_y)
 *   PIML_SPAWN_SQUARE      scenarios.py:87-134: the init launch's n_initial = 4 grid^2 agents on the four blocks of
 *                          square_grid (+-length, the block length), destinations at rank(cell) of grid^2 Philox keys
 *                          (randperm), heading 0; no arrivals afterwards (spawn_cap 0)
 *   PIML_SPAWN_UNIT1       scenarios.py:140-156: (0, width u) -> (length, y + 2u - 1), heading (1, 0)
 *   PIML_SPAWN_UNIT2       scenarios.py:189-215: side / direction by u < side_ratio / u < direction_ratio, heading (+-1, 0)
 *   PIML_SPAWN_UNIT3       scenarios.py:248-282: stream 1 as UNIT1; stream 2 (0..spawn_cap2 per frame, thresholds2) from
 *                          (length u, 0) -> (x + 2u - 1, width), heading (0, 1)
 *   PIML_SPAWN_CLIP        a recorded clip's arrivals resampled (a bootstrap of its tracks; no reference counterpart).
 *                          s->entries is the track table, (E, P, 2) float32 with P = 3 + D, one row per recorded track:
 *                          point 0 the position at the track's first frame inside the window, point 1 the velocity at that
 *                          frame, point 2 (desired_speed, 0), points 3 .. 3+D-1 the waypoints from that frame on (NaN =
 *                          none; the last non-NaN one is the destination).  Rows [0, n_initial) are the tracks present at
 *                          the window's first frame: the init launch places row i in slot i, nothing drawn.  Rows
 *                          [n_initial, E) are the Ka = E - n_initial arrival rows: a new agent of ordinal n takes row
 *                          n_initial + ((u24 Ka) >> 24) of its own Philox draw (integer arithmetic), origin = the row's +
 *                          spawn_offset (2u - 1, 2u - 1) (the row's bitwise when spawn_offset == 0), velocity the row's
 *                          (0 unless initial_velocity), desired speed the row's: uniform_speed, speed_mean, speed_std,
 *                          speed_min and speed_clamp are not read.  The per-frame count is stream 1's, as every law's.
 *                          Any arrival rule but PIML_ARRIVE_GC.
 *   PIML_SPAWN_CLIP_GROUPS the clip law with arrival units (groups that appear together): piml_scenario_step_mlapm_groups
 *                          below, the only entry that takes it.
 * arrival_rule: PIML_ARRIVE_RADIUS |p' - dest| < arrival_radius -> flag += 1; PIML_ARRIVE_XBAND |p'.x - dest.x| <
 * arrival_radius -> flag += 1; PIML_ARRIVE_XEXIT p'.x > length retires the agent (flag unchanged).  Retirement as
 * piml_scenario_step (flag == D or waypoint[flag] NaN; or the x exit).
 * initial_velocity: 0 = v0 vector 0, 1 = heading * v0 (the velocity of the spawn frame and the newest history slot; older
 * slots 0).  speed_clamp: 1 = v0 = max(speed_min, speed_mean + speed_std z), 0 = no clamp (uniform_speed: v0 = speed_mean).
 * entries (but for PIML_SPAWN_CLIP's table), route_polyline and exit_idx are not read (may be NULL).
 * hipErrorInvalidValue: s or r NULL; the checks of piml_scenario_step except D (1..8 here, >= 2 for the crosswalk) and
 * E, P, R, route_max_iters, entries, route_polyline, exit_idx; spawn_law / arrival_rule unknown or one GC and the other
 * not; initial_velocity or speed_clamp not 0 / 1; spawn_cap2 outside 0..8 or non-zero for a law other than UNIT3;
 * thresholds2 above 2^24 or decreasing; the square's grid outside 1..32 or n_initial != 4 grid^2; for PIML_SPAWN_CLIP a
 * NULL entries, P != 3 + D, n_initial > E, no arrival row (E == n_initial) with spawn_cap > 0, more than 2^24 arrival rows.
 */
enum { PIML_SPAWN_GC = 0, PIML_SPAWN_CROSSWALK = 1, PIML_SPAWN_SQUARE = 2, PIML_SPAWN_UNIT1 = 3, PIML_SPAWN_UNIT2 = 4,
       PIML_SPAWN_UNIT3 = 5, PIML_SPAWN_CLIP = 6,
       PIML_SPAWN_CLIP_GROUPS = 7 /* piml_scenario_step_mlapm_groups only: every other entry rejects it */ };
enum { PIML_ARRIVE_GC = 0, PIML_ARRIVE_RADIUS = 1, PIML_ARRIVE_XBAND = 2, PIML_ARRIVE_XEXIT = 3 };
typedef struct piml_scenario_rules {
    int spawn_law, arrival_rule, initial_velocity, speed_clamp;
    int spawn_cap2;                                         /* second Poisson stream's cap (UNIT3) */
    int grid;                                               /* SQUARE: cells per side */
    float length, width;                                    /* scene size (SQUARE: length = block length) */
    float side_ratio, direction_ratio;                      /* UNIT2 */
    uint32_t poisson_thresholds2[8];                        /* second stream's ceil(2^24 P(K <= j)), j < spawn_cap2 */
    float square_grid[32];                                  /* SQUARE: the grid coordinates, grid of them */
} piml_scenario_rules;
int piml_scenario_step_rules(const piml_scenario* s, const piml_scenario_rules* r, const float* a_next, int init,
                             void* stream);

/*
 * Ensembles (ABI 35, additive): piml_scenario_step's frame for `members` simulations of one scene in one launch
 * (grid.y = member; the single-run entries are one member).
 * s's per-member pointers are the bases of member-major buffers whose member-m slice has exactly the single-scene layout:
 * state (members, capacity, .) -- position, velocity, acceleration, destination, hist_velocity, self_features,
 * desired_speed, mask, flag, spawn_iters --, waypoints (members, D, capacity, 2), exit_idx (members, D, capacity),
 * the recorded outputs (members, T, capacity, .), spawn_out (members, T), spawned (members, 2), dropped (members);
 * a_next (members, capacity, 2).  frame_counter, entries, route_polyline, both threshold tables and every scalar are
 * shared.  s->seed is ignored: member m's Philox key is seeds[m] (device memory, (members)).  r = NULL is GC's rule
 * (piml_scenario_step); otherwise as piml_scenario_step_rules.  Member m is bitwise what piml_scenario_step[_rules]
 * gives with seed = seeds[m]; the parity ping-pong is per member.
 * hipErrorInvalidValue (before any launch): every check of piml_scenario_step / piml_scenario_step_rules, members
 * outside 1..65535, NULL seeds.
 */
int piml_scenario_step_members(const piml_scenario* s, const piml_scenario_rules* r, int members, const uint64_t* seeds,
                               const float* a_next, int init, void* stream);

/*
 * MLAPM drives the scene (ABI 35, additive): one frame t -> t+1 of every member under the closed-form law instead of a
 * network's a_next -- the simulation loop of src/main_mlapm.py:18-36 around the scene's arrivals, routing and exits.
 * Buffers, members, seeds and r exactly as piml_scenario_step_members (members = 1 with one seed is the single run; r = NULL
 * is GC); frame 0's spawn stays with that entry's init launch, which does not depend on the law.
 * t = *frame_counter + frame_offset; the counter is read, not written (the caller adds the frames it ran: a captured graph
 * of K frames takes offsets 0 .. K-1 and one add of K).  From t + 1 >= T on a call does nothing.
 * Every slot i < min(spawned[t & 1], capacity) with mask[i] == 1:
 *   F = MLAPM.step's force (src/models/mlapm.py:10-58, with the coll.unsqueeze(-1) fix for UCY) on (p, v, v0 =
 *   desired_speed[i], dest = the current waypoint), the sources being the member's agents present in frame t as RECORDED
 *   (position_out[t], velocity_out[t]; absent ones skipped, as main_mlapm.py:19-23 compacts them);
 *   v' = v + F dt (mlapm.py:57), p' = p + v' dt (main_mlapm.py:25, explicit Euler), a' = F; then the history /
 *   self_features update, arrival, retirement and record of piml_scenario_step (GC) or piml_scenario_step_rules.
 * Spawns, waypoints, exit_idx, desired_speed, spawned, dropped and spawn_out are bitwise those of a piml_scenario_step_members
 * run of the same seeds (they depend on (seed, frame, ordinal) only).  law->radius is MLAPM's UCY collision radius
 * (mlapm.py:42-46), not the scene's arrival_radius.  This entry has no obstacle or wall term (the reference's law has
 * none); piml_scenario_step_mlapm_walls below adds one.
 * No atomics; capturable.
 * hipErrorInvalidValue (before any launch): every check of piml_scenario_step_members except a_next / init; frame_offset < 0;
 * NULL law; variant not 0 / 1 / 2; tau not finite and > 0; A, B, C, D or theta_deg not finite; radius not finite and > 0.
 */
typedef struct piml_mlapm_law {
    int variant;                                            /* 0 raw, 1 GC, 2 UCY (piml_mlapm_step_fwd's) */
    float tau, A, B, C, D, theta_deg;                       /* MLAPM(version, tau, A, B, C, D, theta) */
    float radius;                                           /* UCY collision radius (MLAPM.step's radius) */
} piml_mlapm_law;
int piml_scenario_step_mlapm(const piml_scenario* s, const piml_scenario_rules* r, int members, const uint64_t* seeds,
                             const piml_mlapm_law* law, int frame_offset, void* stream);

/*
 * One law per ensemble member (ABI 35, additive): piml_scenario_step_mlapm with member m stepping under row m of a table
 * of laws, so a parameter sweep, a sensitivity study or a population of candidates is ONE ensemble run -- in place of one
 * run of the loop of src/main_mlapm.py:18-36 per parameter set, which is what the reference's src/utils/grid_search.py
 * does (one process per grid point).
 * The table holds each law's DERIVED constants (cos / sin of theta, B, C, D times log2 e, twice the radius, the absent-source
 * switch), formed on the host by the same code as piml_scenario_step_mlapm's launch, so member m of a table run is bitwise
 * the member of a piml_scenario_step_mlapm run under laws[m].  The row layout is private: size it with
 * piml_mlapm_law_table_bytes(n) (n rows; -1 for n < 0) and fill it with piml_mlapm_law_table_fill.
 * piml_mlapm_law_table_fill(laws, n, table_host): HOST to HOST, no stream and no GPU call (it runs on a machine without a
 * GPU).  hipErrorInvalidValue with table_host untouched: n < 0, a NULL pointer with n > 0, or any law that
 * piml_scenario_step_mlapm rejects (variant not 0 / 1 / 2; tau not finite and > 0; A, B, C, D or theta_deg not finite;
 * radius not finite and > 0); every law is checked before the first row is written.
 * piml_scenario_step_mlapm_laws: table_device = the filled bytes in device memory (the caller's upload), `members` rows.
 * The kernel reads member m's row on every launch (scalar loads; members may differ in variant): overwriting the buffer
 * in place between two replays of a captured graph changes the law of the later frames, with no re-capture.
 * hipErrorInvalidValue (before any launch): every frame check of piml_scenario_step_mlapm, NULL table_device.  The entry
 * CANNOT validate the table's contents, which live in device memory: that is piml_mlapm_law_table_fill's job, and bytes
 * from anywhere else are undefined behaviour of the force law (not of memory: a row indexes nothing).
 * No atomics; capturable; no scratch.
 */
long long piml_mlapm_law_table_bytes(int n);
int piml_mlapm_law_table_fill(const piml_mlapm_law* laws, int n, void* table_host);
int piml_scenario_step_mlapm_laws(const piml_scenario* s, const piml_scenario_rules* r, int members, const uint64_t* seeds,
                                  const void* table_device, int frame_offset, void* stream);

/*
 * A wall term for the MLAPM scenario frame (ABI 35, additive): the repulsion of the scene's nearest obstacle point.
 * p is the agent position; the VALID obstacle points are those with both coordinates finite; q* is the valid point nearest
 * p under d2 = fadd(fmul(e.x, e.x), fmul(e.y, e.y)), e = q - p, in exact float32, ties to the point that comes first in the
 * grid's sorted order.  The agent feels the wall when d2 < c2, c2 = fl(cutoff cutoff) formed once on the host:
 *   W = A exp(B d) (p - q*) / d,  d = sqrt(d2);  W = 0 when d2 == 0 (F.normalize's convention, as the pair law's).
 * Otherwise (no valid point within the cutoff, a NaN position) W = 0, index -1 and dist2 +inf.  The term is isotropic: it has
 * no view factor, so a resting agent still feels the wall.  Its value jumps by A exp(B cutoff) at the cutoff; this is
 * documented, not smoothed.  A = 50, B = -5 is Helbing and Molnar's 1995 boundary potential (U0 = 10 m^2/s^2, R = 0.2 m), the
 * literature's starting point for a fit -- not a default: the entries below are the only ones with a wall term.
 * The value uses the fast reciprocal-sqrt / exp2 units (1e-5 relative, as the pair law); the selection (index, dist2, the
 * cutoff predicate) is exact float32.
 *
 * piml_wall_grid: a static uniform cell grid over the valid points, built once per scene by the host
 * (piml_amd.ops_scenario.wall_grid).  cell >= cutoff (1 + 2^-5) is the cell side, (x0, y0) the points' minimum, a point's
 * cell (floor((q.x - x0) / cell), floor((q.y - y0) / cell)) in float32, `points` the valid points sorted stably by
 * cy gx + cx, cell_start the CSR offsets of the gx gy cells into them.  The kernel finds the agent's cell by the same
 * formula, clamps it to [-1, gx] x [-1, gy] and searches its 3 x 3 neighbourhood, one wave per agent; with gx, gy <= 1024
 * the float32 cell quotients are off by less than 2^-7 cells and the margin 2^-5 makes that search exact.  Every range
 * read from cell_start is clamped to [0, n_points]: a corrupt table gives a wrong force, never a read outside `points`.
 *
 * piml_wall_force: position (rows, 2) -> force (rows, 2) and optionally the selection dist2 (rows), index (rows; into
 * `points`, -1 for none), one wave per row.  rows == 0 or n_points == 0: success without a launch (with n_points == 0 the
 * outputs are the caller's to fill: force 0, dist2 +inf, index -1).
 * hipErrorInvalidValue (before any HIP call): rows < 0; NULL g or force; NULL position with rows > 0 and n_points > 0;
 * n_points < 0; NULL points / cell_start with n_points > 0; gx or gy outside 1..1024; cell or cutoff not finite and > 0;
 * cell < cutoff (1 + 2^-5); x0 or y0 not finite; A or B not finite; A < 0; B > 0.
 *
 * piml_scenario_step_mlapm_walls: piml_scenario_step_mlapm (law != NULL, table_device == NULL) or
 * piml_scenario_step_mlapm_laws (law == NULL, table_device != NULL) with the frame's force
 *   F = ((v0 e - v) / tau - sum over pairs) + W,  componentwise, the wall added last,
 * W evaluated at the agent's position of frame t by the code of piml_wall_force.  Integration, history, arrival, retirement,
 * spawns and records are exactly piml_scenario_step_mlapm's.  The wall law is `wall` by value, or member m's row of
 * wall_table_device ((members) piml_wall_law in device memory, read on every launch: overwriting it between two replays of
 * a captured graph changes the later frames, with no re-capture).
 * hipErrorInvalidValue (before any launch): every check of piml_scenario_step_mlapm / piml_scenario_step_mlapm_laws for the
 * form used; law and table_device both NULL or both given; wall and wall_table_device both NULL or both given; the grid
 * checks of piml_wall_force; the A / B checks on a by-value wall.  The entry CANNOT validate a wall table's contents, which
 * live in device memory (A >= 0, B <= 0, finite, are the caller's to keep; other values are undefined behaviour of the
 * force, not of memory: a row indexes nothing).  No atomics, no scratch, no host synchronisation; capturable.
 */
typedef struct piml_wall_grid {
    const float* points;                                    /* (n_points, 2) device; the valid points in sorted order */
    const int* cell_start;                                  /* (gx*gy + 1) device */
    int n_points, gx, gy;
    float x0, y0, cell, cutoff;
} piml_wall_grid;
typedef struct piml_wall_law { float A, B; } piml_wall_law;
int piml_wall_force(const float* position, long long rows, const piml_wall_grid* g, float A, float B,
                    float* force, float* dist2, int* index, void* stream);
int piml_scenario_step_mlapm_walls(const piml_scenario* s, const piml_scenario_rules* r, int members, const uint64_t* seeds,
                                   const piml_mlapm_law* law, const void* table_device, const piml_wall_grid* g,
                                   const piml_wall_law* wall, const piml_wall_law* wall_table_device, int frame_offset,
                                   void* stream);

/*
 * Group arrivals and a group cohesion term for the MLAPM scenario frame (ABI 35, additive).
 *
 * PIML_SPAWN_CLIP_GROUPS is PIML_SPAWN_CLIP's track table (s->entries, (E, 3 + D, 2), rows [0, n_initial) the first frame)
 * whose rows are bundled into UNITS of 1 .. 4 consecutive rows that appear together -- the recorded clip's groups
 * (piml_amd.scenarios.clip_scenario(groups=)).  piml_scene_groups describes the bundling and holds the per-slot bookkeeping:
 *   row_unit   (E, 2) int32, device: per table row (its index inside its unit, the unit's size)
 *   unit_rows  (n_units) int32, device: the first row of each ARRIVAL unit (rows >= n_initial)
 *   group_first, group_size  (members, capacity) int32, device, member-major like the state: for a slot that holds an agent,
 *              the slot of its unit's first member and the unit's size; the caller zeroes them (size 0 = never spawned).
 * init == 1: the init launch.  Slot i < n_initial is row i, nothing is drawn; group_first[i] = i - row_unit[i][0],
 * group_size[i] = row_unit[i][1].  The laws, the wall arguments and frame_offset are not read.
 * init == 0: frame t -> t + 1 as piml_scenario_step_mlapm (law != NULL, law_table_device == NULL),
 * piml_scenario_step_mlapm_laws (the other way round) or, with wall_grid != NULL, piml_scenario_step_mlapm_walls.  The spawn
 * count of the frame -- the scene rules' stream-1 draw against poisson_thresholds, as for every law -- is a number of UNITS
 * k.  Unit j < k draws u = ((u24 n_units) >> 24) from its own Philox call (word layout in piml_amd/csrc/scenario.hip),
 * first = unit_rows[u], size = row_unit[first][1], and one offset spawn_offset (2u - 1, 2u - 1) shared by its members (none
 * when spawn_offset == 0).  With n the agents spawned through frame t, member q of unit j takes row first + q into slot
 * n + (the sizes of units 0 .. j-1) + q; slots >= capacity are dropped and never written; group_first / group_size are
 * written for every member that is.  spawned grows by the sum of the sizes, spawn_out[t + 1] is that sum, dropped the agents
 * past the capacity.  The arrivals depend on (seed, frame, index in frame) only, never on a law.
 *
 * The group term (glaw or glaw_table_device given; both NULL: none, the units still arrive together).  For slot i the
 * mates are the slots j in [group_first[i], group_first[i] + group_size[i]) clamped to [0, n_t), n_t = min(spawned, capacity);
 * a mate is present when its RECORDED position of frame t is not NaN.  In float32, every operation rounded on its own:
 *   n = the present mates (i among them); n < 2: G = 0;  c = (sum of p_j, ascending j) / (float)n;  e = c - p_i;
 *   d = sqrt(ex ex + ey ey);  thr = dist (float)(n - 1);  G = d > thr ? ((A ex) / d, (A ey) / d) : 0,
 * the attraction term of Moussaid et al. 2010 (their threshold is (n - 1) / 2 m: dist = 0.5); their gaze term is not built.
 * The frame adds it last: F = ((v0 e - v) / tau - sum [+ W]) + G.  glaw_table_device: (members) piml_group_law in device
 * memory, read on every launch, as the wall table.  A has no default (about 3 m/s^2 in the paper: a starting point for a fit).
 *
 * piml_group_force: G for every row of position (rows, 2) with its own group_first / group_size (rows) (the clamp is to
 * [0, rows)), one thread per row; bitwise what the frame adds.  A NaN position[i] gives 0.
 * hipErrorInvalidValue (before any launch) -- piml_group_force: rows < 0; A or dist not finite or negative; a NULL pointer
 * with rows > 0.  piml_scenario_step_mlapm_groups: s, r, seeds or g NULL; members outside 1..65535; frame_offset < 0; init not
 * 0 / 1; r->spawn_law != PIML_SPAWN_CLIP_GROUPS; any frame check of PIML_SPAWN_CLIP on the same descriptor; a NULL pointer
 * inside g; n_units < 0, n_units == 0 with spawn_cap > 0, n_units > 2^24; glaw and glaw_table_device both given; glaw's A or
 * dist not finite or negative; and with init == 0: law and law_table_device both NULL or both given, a law
 * piml_scenario_step_mlapm rejects, wall / wall_table_device not exactly one with a wall_grid or any of them without one, a
 * grid or by-value wall law piml_scenario_step_mlapm_walls rejects.  The tables' contents (row_unit, unit_rows, a law table)
 * live in device memory and cannot be checked: rows and sizes read from them are clamped to the track table, so a corrupt
 * table spawns the wrong rows and reads or writes nothing outside the buffers.  No atomics, no scratch, capturable.
 */
typedef struct piml_group_law { float A, dist; } piml_group_law;
typedef struct piml_scene_groups {
    const int* row_unit;                                    /* (E, 2) */
    const int* unit_rows;                                   /* (n_units) */
    int n_units;
    int *group_first, *group_size;                          /* (members, capacity) */
} piml_scene_groups;
int piml_group_force(const float* position, const int* group_first, const int* group_size, long long rows, float A,
                     float dist, float* force, void* stream);
int piml_scenario_step_mlapm_groups(const piml_scenario* s, const piml_scenario_rules* r, int members, const uint64_t* seeds,
                                    const piml_mlapm_law* law, const void* law_table_device,
                                    const piml_wall_grid* wall_grid /* NULL: no wall term */, const piml_wall_law* wall,
                                    const piml_wall_law* wall_table_device, const piml_scene_groups* g,
                                    const piml_group_law* glaw /* both NULL: no group term */,
                                    const piml_group_law* glaw_table_device, int init, int frame_offset, void* stream);

/*
 * A fluctuation term for the MLAPM scenario frame (ABI 35, additive): the fluctuation of Helbing and Molnar 1995 as an
 * Ornstein-Uhlenbeck acceleration eta per agent, added to the force last, after the wall and group terms:
 *   F = (((v0 e - v) / tau - sum) [+ W]) [+ G]) + eta',    eta' = rho eta + amp z   (float32, every operation rounded alone),
 *   rho = exp(-dt / noise_tau) (0 for noise_tau == 0: white noise),  amp = An sqrt(1 - rho^2),
 * An (m/s^2) the stationary standard deviation of each component.  The caller forms (rho, amp) in float64 and rounds them
 * to float32 (piml_amd.ops_scenario.noise_law): piml_noise_law holds the two floats.
 *
 * z: two standard normals from Philox4x32-10, key = the member's seed, counter = (t lo, t hi, slot, 0x5CE40001), t =
 * *frame_counter + frame_offset the frame stepped from; z_x from the words (w0, w1), z_y from (w2, w3), each
 * (float)(sqrt(-2 ln u1) cos(2 pi u2)) in double with u1 = ((wa >> 8) + 1) 2^-24, u2 = (wb >> 8) 2^-24.  The draws depend
 * on (seed, frame, slot) only, never on the dynamics, and the arrivals never on the noise.
 *
 * piml_noise_args.state: (members, capacity, 2) float32 in device memory, member-major like the state, eta of every slot;
 * the caller zeroes it before frame 0 (a slot is one agent for the whole run: eta = 0 at birth, nothing is written at
 * spawn).  Only the wave that steps live slot i of member m reads and writes state[m capacity + i]; absent and retired
 * slots are not touched and draw nothing.  law: the term by value; law_table: (members) piml_noise_law in device memory,
 * row m for member m, read on every launch (law is then not read).  A row with amp == 0 skips the draw, the state update and
 * the add: that member's frame is piml_scenario_step_mlapm_groups' / _walls' / _laws' / piml_scenario_step_mlapm's bit for bit.
 *
 * piml_scenario_step_mlapm_noise takes what piml_scenario_step_mlapm_groups takes and steps the same frame: with g != NULL
 * a grouped clip scene (r->spawn_law == PIML_SPAWN_CLIP_GROUPS), with g == NULL (then glaw and glaw_table_device NULL too)
 * every other scene as piml_scenario_step_mlapm / _laws / _walls.  init == 1 is the grouped scene's init launch (g != NULL;
 * the state is not read); every other scene's init launch is piml_scenario_step_members'.
 *
 * piml_noise_force: one OU step for every row of eta_in (members, N, 2): row (m, i) draws z with key seeds[m], frame
 * `frame`, slot i, and eta_out = rho eta_in + amp z; z_out (may be NULL) gets z.  present (may be NULL: all) (members, N)
 * bytes: a row with present == 0 is copied unchanged and its z is 0.  One thread per row; eta_out may be eta_in.  Bitwise the
 * state the frame leaves and the value it adds.
 * hipErrorInvalidValue (before any launch) -- both: rho not finite or outside [0, 1), amp not finite or negative (a by-value
 * law; a table's rows live in device memory and cannot be checked).  piml_noise_force: members, N or frame < 0; eta_out,
 * eta_in or seeds NULL with members N > 0.  piml_scenario_step_mlapm_noise: noise or noise->state NULL; with g != NULL every
 * check of piml_scenario_step_mlapm_groups; with g == NULL: glaw or glaw_table_device given, init != 0, and the checks of
 * piml_scenario_step_mlapm (law), piml_scenario_step_mlapm_laws (law_table_device) -- exactly one of the two -- and, with
 * wall_grid != NULL, piml_scenario_step_mlapm_walls; wall or wall_table_device without a grid.  No atomics, capturable.
 */
typedef struct piml_noise_law { float rho, amp; } piml_noise_law;
typedef struct piml_noise_args {
    float* state;                                           /* (members, capacity, 2) */
    piml_noise_law law;
    const piml_noise_law* law_table;                        /* (members), device; NULL: `law` for every member */
} piml_noise_args;
int piml_noise_force(float* eta_out, float* z_out /* may be NULL */, const float* eta_in,
                     const unsigned char* present /* may be NULL */, const uint64_t* seeds, int members, int N, long long frame,
                     float rho, float amp, void* stream);
int piml_scenario_step_mlapm_noise(const piml_scenario* s, const piml_scenario_rules* r, int members, const uint64_t* seeds,
                                   const piml_mlapm_law* law, const void* law_table_device,
                                   const piml_wall_grid* wall_grid /* NULL: no wall term */, const piml_wall_law* wall,
                                   const piml_wall_law* wall_table_device, const piml_scene_groups* g /* NULL: no groups */,
                                   const piml_group_law* glaw /* both NULL: no group term */,
                                   const piml_group_law* glaw_table_device, const piml_noise_args* noise, int init,
                                   int frame_offset, void* stream);

/*
 * Routing by a static floor field for the MLAPM scenario frame (ABI 35, additive): for every gate g of a scene of gates
 * (GC's spawn law: entries (E, P, 2), exit_idx) the geodesic distance u[g] to the gate over the free cells of a grid, which
 * the agents descend instead of walking the straight line to their destination.
 *
 * The grid: gx x gy cells of side `cell` from the origin (x0, y0), 1 <= gx, gy <= 1024, a point's cell
 * (floor((q.x - x0) / cell), floor((q.y - y0) / cell)) in float32 as in piml_wall_grid, planes row-major (gy, gx).
 * blocked (gy, gx) bytes: the cells no agent may enter; cells outside the grid count as blocked.  goal (G, gy, gx) bytes:
 * gate g's cells; a goal cell is free whatever `blocked` says.  u (G, gy, gx) float32 IN CELL UNITS.
 *
 * piml_nav_relax: `launches` launches of K = 8 Jacobi steps each of the first-order Godunov upwind update with h = 1,
 *   a = min(left, right), b = min(down, up), lo = min(a, b), hi = max(a, b),
 *   cand = lo + 1                                       when hi is not finite or hi - lo >= 1,
 *        = 0.5 ((lo + hi) + sqrt(2 - (hi - lo)^2))      otherwise,
 *   u' = cand < u ? cand : u;  a goal cell is 0 and any other blocked cell +inf, before and after,
 * every operation one correctly rounded float32 operation, so a numpy float32 run is the same function bit for bit
 * (tests/nav_ref.py).  Launch j reads u_a and writes u_b for even j and the other way round for odd j (ping-pong; every
 * cell of the written buffer is written), so after an even number of launches the result is in u_a.  The caller
 * initialises u_a (0 on goal cells, +inf elsewhere is the field's start; any state is stepped as it stands).  A workgroup
 * of 256 threads takes a 32 x 32 tile of one gate's plane, stages it with a halo of K cells in LDS, steps K times on the
 * shrinking region (trapezoidal blocking: bitwise K steps of the whole plane) and writes the tile.  changed (G) int32: a
 * thread whose output cell differs from its input cell stores 1 into changed[g] (a plain store; never cleared here).  u
 * only decreases, so a launch that changed nothing left a fixed point.  No atomics, no host synchronisation; capturable.
 * hipErrorInvalidValue (before any launch): a NULL buffer; u_a == u_b; G outside 1..64; gx or gy outside 1..1024;
 * launches < 0.  launches == 0 is a no-op.
 *
 * piml_nav_grid: the field as the lookup reads it.  near (cell units, >= 0): within it the agent walks to its own
 * destination point.
 *
 * piml_nav_direction: for every row a unit vector e and a branch code, one wave per row (the loads are wave-uniform):
 *   0, straight: e = (dest - p) / max(|dest - p|, 1e-12), bitwise the frame's own line -- when p is NaN, the gate is outside
 *      0..G-1, p's cell c is outside the grid, u[c] is not finite, u[c] <= near, or neither branch below applies;
 *   1, bilinear: the four cell centres around p are inside the grid and their u finite: e = -grad of their bilinear
 *      interpolant at p, normalised; a gradient whose squared norm is 0 falls through to
 *   2, descent: e points from p to the centre of the 8-neighbour n of c that maximises (u[c] - u[n]) / |n - c| > 0, u[n]
 *      finite; a diagonal n is skipped when either orthogonal cell beside it is not finite (no corner is cut); ties go to
 *      the first in the order E, W, N, S, NE, NW, SE, SW (N = +y); `neighbour` gets its position in that order, -1 in
 *      the other branches.
 * The selection (branch, neighbour) is exact float32; the value uses the fast reciprocal square root (1e-5 relative).
 * position, destination, direction (rows, 2); gate, branch, neighbour (rows) int32; branch and neighbour may be NULL.
 * rows == 0: success without a launch.
 * hipErrorInvalidValue (before any launch): rows < 0; NULL g, g->u or direction; NULL position, gate or destination with
 * rows > 0; G outside 1..64; gx or gy outside 1..1024; cell not finite and > 0; x0 or y0 not finite; near not finite or < 0.
 *
 * piml_scenario_step_mlapm_nav: the frame of piml_scenario_step_mlapm_noise for a scene without groups, with e of
 *   F = ((v0 e - v) / tau - sum) [+ W] [+ eta']
 * the frame's own line e = (target - p) / max(|target - p|, 1e-12) for the steering target fl(p + n.e), n = piml_nav_direction's
 * result for (p, gate = exit_idx[flag], destination) of the slot, in its branches 1 and 2, and for the destination itself in
 * branch 0: the frame is bitwise piml_scenario_step_mlapm_noise on a state whose destination was overwritten by p + n.e, and e is
 * n.e to within ulp(p).  Everything else, arrival against the slot's destination included, is the same code.  noise == NULL:
 * no fluctuation term (amp == 0).
 * hipErrorInvalidValue (before any launch): the checks of piml_scenario_step_mlapm_noise with g == NULL and init == 0 (a
 * NULL noise excepted) and of piml_nav_direction's grid; a scene rule other than GC's (r != NULL with another spawn law:
 * only GC's law has gates and exit_idx); s->route_max_iters != 0 (with a detour point the waypoint's gate is not the
 * destination's and the agent would never arrive); nav->G != s->E.  No atomics, capturable.
 */
typedef struct piml_nav_grid {
    const float* u;                                         /* (G, gy, gx) device, cell units */
    int G, gx, gy;
    float x0, y0, cell, near;
} piml_nav_grid;
int piml_nav_relax(const unsigned char* blocked, const unsigned char* goal, float* u_a, float* u_b, int G, int gx, int gy,
                   int launches, int* changed, void* stream);
int piml_nav_direction(const float* position, const int* gate, const float* destination, long long rows,
                       const piml_nav_grid* g, float* direction, int* branch /* may be NULL */,
                       int* neighbour /* may be NULL */, void* stream);
int piml_scenario_step_mlapm_nav(const piml_scenario* s, const piml_scenario_rules* r, int members, const uint64_t* seeds,
                                 const piml_mlapm_law* law, const void* law_table_device,
                                 const piml_wall_grid* wall_grid /* NULL: no wall term */, const piml_wall_law* wall,
                                 const piml_wall_law* wall_table_device, const piml_nav_grid* nav,
                                 const piml_noise_args* noise /* NULL: no fluctuation */, int frame_offset, void* stream);

/*
 * The density-aware floor field (ABI 35, additive): the travel cost of a cell grows with the crowd in and around it, and the
 * field is solved again per ensemble member while the scene runs, so routed agents use a second door when the first is
 * congested (the dynamic navigation field of Hartmann et al. 2014).  The grid, blocked and goal are piml_nav_relax's and are
 * shared by all members; count, cost (members, gy, gx) and u (members, G, gy, gx) have a member axis, 1 <= members <= 65535.
 *
 * piml_nav_density: count[m][c] = the number of present slots of member m whose cell is c.  position (members, capacity, 2),
 * mask (members, capacity) float32 (a slot is present when its mask is not 0), count (members, gy, gx) int32.  A slot's cell is
 * piml_nav_direction's, (floor(fdiv(fsub(p.x, x0), cell)), floor(fdiv(fsub(p.y, y0), cell))) in float32; an absent slot, a NaN
 * position and a cell outside the grid deposit nothing.  The entry zeroes count itself (hipMemsetAsync on the stream) and
 * then launches one thread per slot, grid.y = member: integer atomics only, so the result is deterministic, and two members
 * never touch the same plane.  Capturable.
 * hipErrorInvalidValue (before any launch): a NULL buffer; members outside 1..65535; capacity < 1; gx or gy outside 1..1024;
 * cell not finite and > 0; x0 or y0 not finite.
 *
 * piml_nav_cost: the slowness f (members, gy, gx) float32 from the counts.  With s the integer sum of count over the
 * (2r + 1)^2 window of the cell, r = radius_cells, cells outside the grid counting 0,
 *   area = fmul((float)((2r + 1)^2), fmul(cell, cell)),
 *   f = fminf(fadd(1, fmul(kd, fmaxf(fsub(fdiv((float)s, area), rho0), 0))), fmax),
 * every operation one correctly rounded float32 operation (tests/navcost_ref.py gives the same bits).  A workgroup of 256
 * threads stages a 32 x 32 tile of one member's counts with a halo of r cells in LDS and sums rows, then columns.  Known limit:
 * blocked cells count in the window's area, so the density beside a wall reads low.
 * hipErrorInvalidValue (before any launch): a NULL buffer; members outside 1..65535; gx or gy outside 1..1024; cell not finite
 * and > 0; radius_cells outside 0..8; kd < 0, rho0 < 0, fmax < 1, or any of the three not finite.
 *
 * piml_nav_relax_cost: piml_nav_relax with the slowness in the update and a member axis.  One step is
 *   cand = lo + f                                         when hi is not finite or hi - lo >= f,
 *        = 0.5 ((lo + hi) + sqrt(2 f f - (hi - lo)^2))    otherwise (fmul(2, fmul(f, f)), then fsub),
 *   u' = cand < u ? cand : u, goal cells 0 and other blocked cells +inf as in piml_nav_relax,
 * with f = cost[member][cell] >= 1, each operation one correctly rounded float32 operation: bitwise tests/navcost_ref.py, and
 * with cost == 1 everywhere bitwise piml_nav_relax.  cost (members, gy, gx); u_a, u_b (members, G, gy, gx), ping-pong as in
 * piml_nav_relax; changed (members * G) int32, plane member * G + gate.  The same temporal blocking: K = 8 steps per launch on
 * a 32 x 32 tile staged with a halo of 8 in two LDS planes, the member's cost tile staged once into a third (29952 bytes of
 * LDS a workgroup: 5 workgroups a CU against piml_nav_relax's 7); grid.z = member * G + gate.  From the cold start (0 on goal
 * cells, +inf elsewhere) u only decreases, so a launch that changed nothing left the fixed point, and
 * u_static <= u <= max(f) u_static.  A warm start from a field of lower cost does NOT reach it (the minimum keeps stale low
 * values): start cold.  No atomics, no host synchronisation; capturable.
 * hipErrorInvalidValue (before any launch): members < 1; a NULL buffer; u_a == u_b; G outside 1..64; gx or gy outside
 * 1..1024; launches < 0; members * G > 65535; more than 2^31 - 1 cells in u.  launches == 0 is a no-op.
 *
 * piml_scenario_step_mlapm_navdyn: piml_scenario_step_mlapm_nav with a field per member: member m looks its directions up in
 * nav->u + m * member_stride (elements; G * gy * gx for the u of piml_nav_relax_cost), 0 meaning one field shared by all
 * members -- then the frame is piml_scenario_step_mlapm_nav's bit for bit.  The caller guarantees members fields behind nav->u.
 * There is no form with the any-angle table: that table is a uniform-cost construction.
 * hipErrorInvalidValue (before any launch): piml_scenario_step_mlapm_nav's refusals; member_stride < 0.  No atomics, capturable.
 */
int piml_nav_density(const float* position, const float* mask, int members, int capacity, float x0, float y0, float cell,
                     int gx, int gy, int* count, void* stream);
int piml_nav_cost(const int* count, int members, int gx, int gy, float cell, int radius_cells, float kd, float rho0, float fmax,
                  float* cost, void* stream);
int piml_nav_relax_cost(const unsigned char* blocked, const unsigned char* goal, const float* cost, float* u_a, float* u_b,
                        int members, int G, int gx, int gy, int launches, int* changed, void* stream);
int piml_scenario_step_mlapm_navdyn(const piml_scenario* s, const piml_scenario_rules* r, int members, const uint64_t* seeds,
                                    const piml_mlapm_law* law, const void* law_table_device,
                                    const piml_wall_grid* wall_grid /* NULL: no wall term */, const piml_wall_law* wall,
                                    const piml_wall_law* wall_table_device, const piml_nav_grid* nav, long long member_stride,
                                    const piml_noise_args* noise /* NULL: no fluctuation */, int frame_offset, void* stream);

/*
 * The direction-aware density (ABI 35, additive): a counted person weighs 1 - flow (v . d) / vref, d the way to the walker's
 * gate, so each gate has a cost plane of its own: cost (members, G, gy, gx).  A standing person weighs 1 as in piml_nav_cost,
 * one walking the walker's way at vref weighs 0, one coming at the walker at vref weighs 1 + flow.  Every operation below is
 * one correctly rounded float32 operation and every sum an integer (tests/navflow_ref.py gives the same bits).
 *
 * piml_nav_descent: d (G, gy, gx, 2) float32 from the STATIC field u (G, gy, gx) of piml_nav_relax, once per scene: the upwind
 * unit direction of steepest descent.  With L, R, D, U the four neighbours (+inf outside the grid), a = L < R ? L : R,
 * b = D < U ? D : U: rx = (u, a finite and a < u) ? fsub(u, a) : 0, negated when L < R; ry likewise with b and D < U;
 * n = sqrtf(fadd(fmul(rx, rx), fmul(ry, ry))); d = (fdiv(rx, n), fdiv(ry, n)) when n > 0, else (0, 0) -- goal cells, cells
 * with u = +inf and blocked cells.  The static field, not the one being solved: the field under construction cannot define
 * its own cost without an outer fixed-point loop.  One thread per cell.
 * hipErrorInvalidValue (before any launch): a NULL buffer; G outside 1..64; gx or gy outside 1..1024.
 *
 * piml_nav_flow: piml_nav_density's deposit -- the same slots, cell formula and count -- which also adds the slot's velocity
 * (members, capacity, 2) into mom (members, 2, gy, gx) int32, per component
 *   q = isfinite(v) ? (int)rintf(fmul(fminf(fmaxf(v, -8), 8), 1024)) : 0            (2^-10 m/s; halves round to even).
 * A slot that deposits no count deposits no momentum.  The entry zeroes count and mom itself (hipMemsetAsync on the stream);
 * integer atomics only: deterministic.  Capturable.
 * hipErrorInvalidValue (before any launch): piml_nav_density's refusals; a NULL velocity or mom; capacity >= 1 << 18 (a window
 * sum of momenta stays inside int32).
 *
 * piml_nav_cost_flow: cost[m][g][c] from count, mom and d.  With s, px, py the integer sums of count, mom[0], mom[1] over
 * piml_nav_cost's window and area piml_nav_cost's,
 *   pd    = fadd(fmul((float)px, dx), fmul((float)py, dy)),      along = fdiv(pd, fmul(1024, vref)),
 *   s_eff = fsub((float)s, fmul(flow, along)),
 *   f     = fminf(fadd(1, fmul(kd, fmaxf(fsub(fdiv(s_eff, area), rho0), 0))), fmax)  >= 1.
 * flow == 0 gives s_eff == s exactly: every gate's plane is piml_nav_cost's bit for bit, whatever the velocities.  A workgroup
 * stages each of the member's three integer tiles with its halo once, takes the separable window sums into registers and
 * loops over the gates (15360 bytes of LDS, piml_nav_cost's).
 * hipErrorInvalidValue (before any launch): piml_nav_cost's refusals; a NULL mom or d; G outside 1..64; members * G > 65535 or
 * more than 2^31 - 1 cells in cost (piml_nav_relax_cost_gates' limits); flow or vref not finite, flow < 0, vref <= 0.
 *
 * piml_nav_relax_cost_gates: piml_nav_relax_cost with the cost read from plane member * G + gate of cost (members, G, gy, gx)
 * in place of plane member: the same update, temporal blocking, LDS, changed flags and refusals, and with the same cost in
 * every gate's plane piml_nav_relax_cost bit for bit.
 */
int piml_nav_descent(const float* u, int G, int gx, int gy, float* d, void* stream);
int piml_nav_flow(const float* position, const float* velocity, const float* mask, int members, int capacity, float x0,
                  float y0, float cell, int gx, int gy, int* count, int* mom, void* stream);
int piml_nav_cost_flow(const int* count, const int* mom, const float* d, int members, int G, int gx, int gy, float cell,
                       int radius_cells, float kd, float rho0, float fmax, float flow, float vref, float* cost, void* stream);
int piml_nav_relax_cost_gates(const unsigned char* blocked, const unsigned char* goal, const float* cost, float* u_a,
                              float* u_b, int members, int G, int gx, int gy, int launches, int* changed, void* stream);

/*
 * The weighted solve by active tiles (ABI 35, additive; csrc/navactive.hip): piml_nav_relax_cost's (cost_per_gate = 0: cost
 * (members, gy, gx), plane member) or piml_nav_relax_cost_gates' (cost_per_gate = 1: cost (members, G, gy, gx), plane
 * member * G + gate) Jacobi sequence bit for bit -- the same grid (tiles x, tiles y, member * G + gate), temporal blocking,
 * LDS planes and per-cell arithmetic --, skipping the tiles whose step reproduces what the written buffer already holds.
 * u_a holds the cold start (0 on goal cells, +inf elsewhere); u_b may hold anything.  flags: device int32, two planes of
 * members * G * ty * tx words (tx = ceil(gx / 32), ty = ceil(gy / 32)), ping-ponged per launch; they need no clearing.
 * Launch 0 steps every tile; in a later launch a block reads the nine flags of its 3 x 3 tile neighbourhood from the launch
 * before (outside the tile grid: 0); none set: it writes its own flag 0 and returns; otherwise it steps and writes the tile
 * and its flag is whether any word of the tile differs from its input.  The buffer a launch writes always holds the whole
 * next iterate, so after `launches` launches u_a is exactly what the dense entries leave there after the same number.
 * work: NULL or device int32 (members * G): every block that stepped its tile adds 1 (integer atomics; the entry does not
 * clear it).  stalled: device int32, one word: a block whose tile changed in the LAST launch stores 1 -- the launches were
 * too few for the fixed point; the entry never clears it.  While it stays 0 after a call, u_a == u_b is the fixed point.
 * The entry queues `launches` launches on `stream` and nothing else: no host read, no allocation, no memset; capturable.
 * hipErrorInvalidValue (before any launch): piml_nav_relax_cost_gates' refusals (a NULL blocked, goal, cost, u_a or u_b;
 * u_a == u_b; members < 1; G outside 1..64; gx or gy outside 1..1024; members * G > 65535; more than 2^31 - 1 cells in u);
 * launches odd or < 2 (the result is in u_a); cost_per_gate neither 0 nor 1; a NULL flags or stalled.
 */
int piml_nav_relax_active(const unsigned char* blocked, const unsigned char* goal, const float* cost, int cost_per_gate,
                          float* u_a, float* u_b, int members, int G, int gx, int gy, int launches, int* flags, int* work,
                          int* stalled, void* stream);

/*
 * Exit choice (ABI 35, additive): a routed agent re-decides which of a class of equivalent gates it is bound for.  The spawn
 * law draws the destination gate uniformly at birth; u[g] at the agent's cell is the walking distance to gate g under the
 * static field and a travel-time proxy under the density-weighted one, so the least u over a class is the nearest exit under
 * the former and the quickest under the latter.
 *
 * piml_nav_choose_exit: ONE launch, in front of a scenario frame (network-driven or MLAPM), that re-decides the gate of every
 * present slot of every member.  s, members and seeds are the frame entries' (seeds NULL: one member, key s->seed); nav and
 * member_stride are piml_scenario_step_mlapm_navdyn's (0: one static field for all members); gate_class (G) device int32, the
 * class of each gate, -1 = in no class; law->margin and law->commit in CELL units (metres / nav->cell, divided in float32 by
 * the host); switch_count (members, capacity) device int32 or NULL; frame_offset as the MLAPM frame's.
 * Schedule: with t = *frame_counter + frame_offset the kernel returns at once unless t >= 1 and (t - 1) % every == 0 -- the
 * density update's schedule, tested on the device, so the launch can sit in front of every captured frame and eager and
 * captured runs are bitwise each other; where an update falls on the same t the choice runs after it and reads the fresh field.
 * Per slot i < min(spawned[t & 1], capacity) with mask != 0 and f = flag[i] in 0..1, cur = exit_idx[f][i]:
 *   1. the spawn draws of calls 1 and 2 (stream 0x5CE00001 / 2, key = the member's seed, counter = ordinal i) are recomputed:
 *      the origin gate oe, the destination point index di, the destination's offset words (w2.z, w2.w).  Nothing new is drawn
 *      and no per-agent state is kept: slot = ordinal.
 *   2. candidates: gates g with gate_class[g] == gate_class[cur] >= 0, g != oe and u[g][c] finite, c the agent's cell by
 *      piml_nav_direction's cell formula.
 *   3. the slot is left untouched when the position is NaN, c is outside the grid, cur is outside 0..G-1 or in no class, there
 *      is no candidate, or u[cur][c] is finite and <= commit.
 *   4. best = the candidate of least u, the lowest gate on a tie.  Switch iff u[cur][c] is not finite or
 *      fadd(u[best][c], margin) < u[cur][c]: equality stays, best == cur never switches.  (An unreachable current gate is
 *      left whatever the margin, +inf included.)
 *   5. on a switch d' = entries[best][di] + unit24(w2.z, w2.w) spawn_offset, the spawn's formula operation for operation;
 *      waypoints[q][i] = d' and exit_idx[q][i] = the entry nearest d' for q = f .. 1, destination[i] = d', switch_count[m][i]
 *      += 1.  Rows below f, the recorded *_out buffers and every other field are not written.
 * After a switch rows >= f are bitwise what the spawn would have written had its destination draw been `best`; a switch back
 * restores the original destination bit for bit.  One wave per slot, lane g holding u[g]; no atomics, a slot's rows are
 * written by its own wave only.  Every predicate is one correctly rounded float32 operation after another
 * (tests/navchoice_ref.py gives the same bits).  Capturable.
 * Known limits: a gate is both origin and destination under GC's law and only the agent's own origin gate is excluded; the
 * class is looked up through exit_idx, the entry nearest the waypoint, not the drawn gate; the field may be up to `every`
 * frames old; there is no per-agent preference or familiarity term.
 * hipErrorInvalidValue (before any launch): a NULL s, nav, gate_class or law; the frame checks of piml_scenario_step on s;
 * members outside 1..65535, a NULL seeds with members != 1; piml_nav_direction's grid checks; nav->G != s->E;
 * s->route_max_iters != 0 or s->D < 2; law->every < 1; margin or commit negative or NaN; member_stride < 0; frame_offset < 0.
 * gate_class is device memory: its values are the caller's to validate.
 */
typedef struct piml_exit_choice {
    float margin, commit;                                   /* cell units */
    int every;                                              /* frames between two passes, >= 1 */
} piml_exit_choice;
int piml_nav_choose_exit(const piml_scenario* s, int members, const uint64_t* seeds, const piml_nav_grid* nav,
                         long long member_stride, const int* gate_class, const piml_exit_choice* law,
                         int* switch_count /* may be NULL */, int frame_offset, void* stream);

/*
 * The any-angle floor field: a second table beside u.  For every cell c of gate g, parent[g][c] is the next turning point
 * of the taut string from c to the gate -- the gate cell itself in open space, a corner cell round a wall -- and w[g][c]
 * the string's length in cells.  An agent in c steers at the centre of its parent along a straight segment that enters no
 * blocked cell wherever in c it stands, so routed agents walk straight where piml_nav_direction's first-order gradient curves
 * (3 degrees off on average in open space) and keep off the walls where it falls back to a neighbour's centre.
 *
 * The grid, blocked (gy, gx) and goal (G, gy, gx) are piml_nav_relax's: a cell outside the grid counts as blocked, a goal
 * cell is free whatever `blocked` says (gate g sees the mask blocked & !goal[g]).  w (G, gy, gx) float32 in cell units;
 * parent (G, gy, gx) int32, the linear index y gx + x, or -1.
 *
 * Start: goal cells w = 0, parent = self; every other cell w = +inf, parent = -1.  Goal and blocked cells never change.
 * One Jacobi step k -> k + 1, for every free cell c = (x, y) that is no goal cell:
 *   best = +inf, bp = -1; if parent_k[c] = q >= 0: best = fadd(w_k[q], dist(c, q)), bp = q.
 *   For the neighbours n in the order E, W, N, S, NE, NW, SE, SW (N = +y): skip n outside the grid, blocked, or with w_k[n]
 *   not finite; skip a diagonal n when either orthogonal cell beside it is blocked or outside (no corner is cut).
 *   q = parent_k[n] (n itself for a goal cell); if !visible(c, q): q = n.  cand = fadd(w_k[q], dist(c, q)) replaces
 *   (best, bp) only when cand < best strictly.
 *   w_{k+1}[c] = best, parent_{k+1}[c] = bp.
 * dist(c, q) = sqrtf((float)(dx dx + dy dy)): the integer is exact below 2^24, the root correctly rounded, so a numpy float32
 * run with Python integers is the same function bit for bit (tests/navsight_ref.py).  w never increases; a step that changed
 * nothing is a fixed point.
 *
 * visible(c, q), D = q - c: a cell X = c + a OBSTRUCTS when it is blocked (or outside) and there is a t in [0, 1] with
 * |a.x - t D.x| < 1 - t / 2 and |a.y - t D.y| < 1 - t / 2: the open square of X meets the convex hull of c's square and q's
 * centre, which at t is a square of half-width (1 - t) / 2 around c + t D.  visible is true when no cell obstructs.  Each
 * inequality is two strict linear constraints on t with odd integer coefficients, t (2 D - 1) > 2 a - 2 and
 * t (2 D + 1) < 2 a + 2, compared by integer cross-multiplication: no float is involved.  Walking along the face of a wall is
 * visible; a diagonal pinch between two blocked cells never is.
 *
 * piml_nav_sight_relax: `launches` launches of ONE Jacobi step each, one wave per cell.  Launch j reads (w_a, parent_a) and
 * writes (w_b, parent_b) for even j and the other way round for odd j (every cell of the written planes is written), so
 * after an even number of launches the result is in the a planes.  The caller initialises the a planes (the start above;
 * any state whose parents are -1 or cells with a finite w is stepped as it stands).  cache (G, gy, gx, 8) int32, filled with
 * -1 by the caller before the first launch and kept between launches on the same mask: per cell and neighbour slot the last
 * parent tested and whether c sees it, (q << 1) | visible.  It only saves walks: visible(c, q) is a property of the mask, so
 * the planes are bitwise those of the plain step whatever valid entries it holds.  changed (G) int32: a wave whose cell's
 * w or parent differs from its input stores 1 into changed[g] (a plain store; never cleared here).  No atomics, no host
 * synchronisation; capturable.
 * hipErrorInvalidValue (before any launch): a NULL buffer; w_a == w_b or parent_a == parent_b; G outside 1..64; gx or gy
 * outside 1..1024; launches < 0.  launches == 0 is a no-op.
 *
 * piml_nav_sight: the parent planes as the lookup reads them, beside the piml_nav_grid of the same scene.
 *
 * piml_nav_direction_sight: piml_nav_direction with one branch in front of its branches 1 and 2:
 *   3, sight: where the field applies (p inside the grid, the gate valid, u[c] finite and > near) and q = parent[g][c] >= 0
 *      is not c itself: T = origin + (q + 0.5) cell per axis (branch 2's centre formula), h = T - p,
 *      h2 = fadd(fmul(h.x, h.x), fmul(h.y, h.y)) > 0: e = h rsq(h2), neighbour -1.
 * Otherwise branches 1, 2 and 0 as in piml_nav_direction, bit for bit.  Arguments and refusals are piml_nav_direction's, and
 * hipErrorInvalidValue also for a NULL sight or sight->parent, or sight->G, gx, gy other than the grid's.
 *
 * piml_scenario_step_mlapm_sight: piml_scenario_step_mlapm_nav with n = piml_nav_direction_sight's result: the steering
 * target is fl(p + n.e) in branches 1, 2 and 3, the destination in branch 0.  A parent plane that is all -1 gives
 * piml_scenario_step_mlapm_nav bit for bit.  hipErrorInvalidValue (before any launch): everything piml_scenario_step_mlapm_nav
 * refuses; a NULL sight or sight->parent; sight->G, gx, gy other than the grid's.  No atomics, capturable.
 *
 * Known limits: the agent heads for the centre of the gate CELL until `near`, not for its own destination point; parents are
 * cell centres, so a path rounds a corner at half a cell plus the mask's clearance; the field is static.
 */
typedef struct piml_nav_sight {
    const int* parent;                                      /* (G, gy, gx) device: y gx + x of the parent cell, or -1 */
    int G, gx, gy;
} piml_nav_sight;
int piml_nav_sight_relax(const unsigned char* blocked, const unsigned char* goal, float* w_a, int* parent_a, float* w_b,
                         int* parent_b, int* cache, int G, int gx, int gy, int launches, int* changed, void* stream);
int piml_nav_direction_sight(const float* position, const int* gate, const float* destination, long long rows,
                             const piml_nav_grid* g, const piml_nav_sight* sight, float* direction,
                             int* branch /* may be NULL */, int* neighbour /* may be NULL */, void* stream);
int piml_scenario_step_mlapm_sight(const piml_scenario* s, const piml_scenario_rules* r, int members, const uint64_t* seeds,
                                   const piml_mlapm_law* law, const void* law_table_device,
                                   const piml_wall_grid* wall_grid /* NULL: no wall term */, const piml_wall_law* wall,
                                   const piml_wall_law* wall_table_device, const piml_nav_grid* nav,
                                   const piml_nav_sight* sight, const piml_noise_args* noise /* NULL: no fluctuation */,
                                   int frame_offset, void* stream);

/*
 * The floor field under the network-driven frame (ABI 35, additive): piml_scenario_step_members' frame for a scene of gates,
 * which also writes, per slot, the point the network should be steered to.  A PINNSF reads the destination only as a unit
 * direction (columns 0..1 of self_features, the desired-force term), so the caller hands `steer` to the relative-feature
 * launch in the place of the destination and the network follows the field; nothing else of its inputs changes.
 * Buffers, r, members, a_next and init exactly as piml_scenario_step_members; seeds == NULL is the single run (members == 1,
 * key s->seed, as piml_scenario_step).  steer (members, capacity, 2) float32, member-major as the state.
 * With p', flag' and dest' the slot's position, flag and destination AFTER this frame's integration, arrival and retirement:
 *   a slot that stays present:  steer = fl(p' + n.e) per component in n's branches 1, 2 (and 3), dest' in branch 0 --
 *                               piml_scenario_step_mlapm_nav's target formula -- with n = piml_nav_direction's result (sight !=
 *                               NULL: piml_nav_direction_sight's) for (p', gate = exit_idx[flag'], dest');
 *   a slot that retires in this frame or was retired earlier: steer = (NaN, NaN); exit_idx is never read with flag' >= D;
 *   a spawned agent (the init launch's too): steer from (origin, exit_idx[0], its first waypoint);
 *   slots >= capacity and dropped ordinals: never written, as every other buffer.
 * Position, velocity, history, arrival against the slot's destination, retirement, records, spawns and the Philox schedule
 * are piml_scenario_step_members' bit for bit: the field moves nothing but `steer`.  One thread per slot, the lookup a gather
 * of 13 words (14 with the table); one wave per spawned agent.  No atomics, capturable.
 * hipErrorInvalidValue (before any launch): everything piml_scenario_step_members refuses (seeds == NULL is refused only with
 * members != 1); everything piml_nav_direction refuses about the grid and, with sight != NULL, piml_nav_direction_sight about
 * the table; a scene rule other than GC's (r != NULL with another spawn law); s->route_max_iters != 0; nav->G != s->E; a
 * NULL steer.
 */
int piml_scenario_step_nav(const piml_scenario* s, const piml_scenario_rules* r /* NULL or GC's */, int members,
                           const uint64_t* seeds /* NULL: members == 1, key s->seed */, const float* a_next, int init,
                           const piml_nav_grid* nav, const piml_nav_sight* sight /* NULL: no any-angle table */,
                           float* steer, void* stream);

/*
 * utils.route (src/utils/utils.py:141-165) for n (o, d) pairs, one wave each, the device function the spawn path uses:
 * the segment o -> r is tested against the polyline's R-1 segments, the hit with the smallest alpha moves r to
 * crossing + clearance * normal, until nothing is hit or max_iters moves were made.  float32 in the reference's order.
 * origin / destination / waypoint (n, 2), polyline (R, 2), iters (n) int32 = moves made.
 * hipErrorInvalidValue: n < 0, R < 2, max_iters outside 0..64, a NULL buffer with n > 0.  n == 0 is a no-op.
 */
int piml_scenario_route(const float* origin, const float* destination, int n, const float* polyline, int R, int max_iters,
                        float clearance, float* waypoint, int* iters, void* stream);

/*
 * The hand-written collision handling that closes PINNSF_polar_bottleneck_collision.forward
 * (`--model pinnsf_pbc`, src/models/model.py:1383-1444), on the k gathered neighbours of every
 * agent: rows of ped_features (row_stride floats: p_j - p_i, v_j - v_i, ...), the agent's velocity v_i
 * (self_features[..., 2:4]) and the predicted acceleration.  Reaction radius = collision_threshold +
 * 1.34 * 2 * time_unit; a neighbour inside it is "head-on" when (v_i . p_ji)(v_j . -p_ji) > 0, else "chasing";
 * for the nearest of each kind the approaching normal component of the prediction is removed and the
 * acceleration that cancels the normal closing speed within one time unit is added (step 2, then step 3 on
 * the result).  bwd is the analytic gradient w.r.t. predictions, velocity and the (p_ji, v_ji) columns of the
 * two selected neighbour rows (flags / selections are piecewise constant); any gradient output may be NULL.
 * NaN: a NaN offset component reads as 0 (the reference's nan_to_num) and receives no gradient; a flagged chasing row's
 * NaN velocity makes the agent NaN as in the reference; an unflagged row's never does (the reference lets slot 0's through
 * when nobody is chasing).  k == 0 (ped_features may be NULL): out = predictions, the gradient passes through.
 */
int piml_collision_correction_fwd(const float* predictions, const float* ped_features, const float* velocity,
                                  size_t rows, int k, int row_stride, float collision_threshold, float time_unit,
                                  float* out, void* stream);
int piml_collision_correction_bwd(const float* g_out, const float* predictions, const float* ped_features,
                                  const float* velocity, size_t rows, int k, int row_stride,
                                  float collision_threshold, float time_unit, float* g_predictions,
                                  float* g_ped_features, float* g_velocity, void* stream);

/*
 * Differentiable frame step of the fine-tuning rollout, BaseSimulator.test_multiple_rollouts_for_training
 * between the model call and the feature recomputation (src/models/simulators.py:741-769), one launch:
 *   v' = v + a dt, p' = p + v dt (lagged Euler), a' = a_pred; waypoint switch when |p - dest| < 0.5 (the
 *   index is clamped at the last waypoint: nobody leaves the scene here); agents flagged in
 *   new_flag[c, t_next, i] are re-initialised from the (C,T,N,.) ground-truth series of frame t_next
 *   (new_flag NULL or t_next >= T: no injection).  nan_flag (optional) is OR-ed with 1 when a_pred has a NaN
 *   (the assert at :745, kept on the device).  State (C,N,.) in, new state out; waypoints as in
 *   piml_rollout_step.  bwd: with keep = not re-initialised,
 *   g_p = keep g_p', g_v = keep (g_v' + dt g_p'), g_a = keep dt g_v', g_a_pred = keep g_a'
 *   (any g_*_out may be NULL = zero; any output may be NULL = not wanted).
 * zero_mask (C,N) uint8, optional: when given, NaN components of v' and a' are replaced by 0 -- what the
 * next Pedestrians.get_relative_features call would do to them in place (src/data/data.py:483-484) -- and
 * the mask records which (bits 0-1: v'.xy, bits 2-3: a'.xy); bwd passes no gradient through those.
 */
int piml_train_step_fwd(const float* position, const float* velocity, const float* acceleration,
                        const float* a_pred, const float* destination, const int64_t* dest_idx,
                        const float* waypoints, int D, int waypoints_per_slice, const int64_t* dest_num,
                        const uint8_t* new_flag, const float* position_series, const float* velocity_series,
                        const float* acceleration_series, const float* destination_series,
                        const int64_t* dest_idx_series, int C, int T, int N, int t_next, float dt,
                        float* position_out, float* velocity_out, float* acceleration_out,
                        float* destination_out, int64_t* dest_idx_out, int* nan_flag, uint8_t* zero_mask,
                        void* stream);
/* piml_train_step_fwd that also leaves the frame's INPUT position in a caller's buffer (position_copy: C slices of (N, 2)
 * floats, position_copy_slice_stride floats apart -- frame t of the (C, T, N, 2) array of predicted positions the rollout loss
 * reads, src/models/simulators.py:728, :790): the frames write that array themselves instead of a concatenation behind the loop.
 * position_copy may be NULL (= piml_train_step_fwd). */
int piml_train_step_fwd_copy(const float* position, const float* velocity, const float* acceleration, const float* a_pred,
                             const float* destination, const int64_t* dest_idx, const float* waypoints, int D,
                             int waypoints_per_slice, const int64_t* dest_num, const uint8_t* new_flag,
                             const float* position_series, const float* velocity_series, const float* acceleration_series,
                             const float* destination_series, const int64_t* dest_idx_series, int C, int T, int N, int t_next,
                             float dt, float* position_out, float* velocity_out, float* acceleration_out, float* destination_out,
                             int64_t* dest_idx_out, int* nan_flag, uint8_t* zero_mask, float* position_copy,
                             long long position_copy_slice_stride, void* stream);
int piml_train_step_bwd(const float* g_position_out, const float* g_velocity_out, const float* g_acceleration_out,
                        const uint8_t* new_flag, const uint8_t* zero_mask, int C, int T, int N, int t_next, float dt,
                        float* g_position, float* g_velocity, float* g_acceleration, float* g_a_pred, void* stream);
/* piml_train_step_bwd with a second source of d/d(outputs): g_state6 (C, N, 6; may be NULL) = d/d(p', v', a') interleaved, as
 * piml_relfeat_bwd_self leaves it, is ADDED to the three separate gradients (each may be NULL) before the frame's backward --
 * the two consumers of a frame's state (the next frame's step and its features) without a gradient accumulation in between. */
int piml_train_step_bwd6(const float* g_position_out, const float* g_velocity_out, const float* g_acceleration_out,
                         const float* g_state6, const unsigned char* new_flag, const unsigned char* zero_mask, int C, int T, int N,
                         int t_next, float dt, float* g_position, float* g_velocity, float* g_acceleration, float* g_a_pred,
                         void* stream);
/* piml_train_step_bwd6 with a third source: g_position_in (may be NULL) = a gradient that arrives on the frame's INPUT position
 * itself -- the rollout loss reads every frame's position (src/models/simulators.py:728, :790-819) and the next frame's step
 * reads it too; handed in here (C slices of (N, 2) contiguous floats, g_position_in_slice_stride floats apart: a time slice of
 * the loss's (C, T, N, 2) gradient as it stands) it is added to g_position inside the launch instead of by a strided addition
 * of the autograd engine per frame.  g_position_out_slice_stride != 0: g_position_out is laid out the same way (0: C * N
 * contiguous rows). */
int piml_train_step_bwd7(const float* g_position_out, long long g_position_out_slice_stride, const float* g_velocity_out,
                         const float* g_acceleration_out,
                         const float* g_state6, const float* g_position_in, long long g_position_in_slice_stride,
                         const unsigned char* new_flag, const unsigned char* zero_mask, int C, int T, int N, int t_next, float dt,
                         float* g_position, float* g_velocity, float* g_acceleration, float* g_a_pred, void* stream);
/* The frame step with the model's TAIL in front of it, one launch each way.  In the training rollout the network sees channelled
 * (C, N, .) input, where the reference's desired-force term takes its norm over the AGENT axis (quirk Q2: `torch.norm(self_features[...,
 * :2], p=2, dim=1, keepdim=True)`, src/models/model.py:1290 / :1125 as evaluated at src/models/simulators.py:701), so the tail
 *     predictions = sum_k acc_ped[c, n, k] (+ sum_k acc_obs[c, n, k]) + (v0 d / t - v) / tau,   t[c, comp] = || d[c, :, comp] ||_2 (0 -> 0.1)
 * is a reduction over a slice's agents followed by piml_train_step_fwd_copy on the result (a_pred = predictions).  acc_ped (C, N, kp, 2):
 * the decoder tails' sum (kp = 1) or the bottleneck variants' per-neighbour predictions; acc_obs likewise or NULL; self_features
 * (C, N, 7).  Backward = piml_train_step_bwd7, then with g = d/d(predictions) (written to g_prediction (C, N, 2), required):
 * g_acc_ped (C, N, kp, 2) / g_acc_obs = g broadcast over k (NULL: not written -- for kp = 1 g_prediction IS that gradient), g_self
 * (C, N, 7) = piml_pinnsf_epilogue_agentnorm_bwd's (may be NULL).  Bitwise what the separate launches produce. */
int piml_train_step_tail_fwd(const float* position, const float* velocity, const float* acceleration, const float* acc_ped, int kp,
                             const float* acc_obs, int ko, const float* self_features, float tau, const float* destination,
                             const int64_t* dest_idx, const float* waypoints, int D, int waypoints_per_slice, const int64_t* dest_num,
                             const uint8_t* new_flag, const float* position_series, const float* velocity_series,
                             const float* acceleration_series, const float* destination_series, const int64_t* dest_idx_series, int C,
                             int T, int N, int t_next, float dt, float* position_out, float* velocity_out, float* acceleration_out,
                             float* destination_out, int64_t* dest_idx_out, int* nan_flag, uint8_t* zero_mask, float* position_copy,
                             long long position_copy_slice_stride, void* stream);
int piml_train_step_tail_bwd(const float* g_position_out, long long g_position_out_slice_stride, const float* g_velocity_out,
                             const float* g_acceleration_out, const float* g_state6, const float* g_position_in,
                             long long g_position_in_slice_stride, const unsigned char* new_flag, const unsigned char* zero_mask, int C,
                             int T, int N, int t_next, float dt, float* g_position, float* g_velocity, float* g_acceleration,
                             float* g_prediction, const float* self_features, float tau, int kp, int ko, float* g_acc_ped,
                             float* g_acc_obs, float* g_self, void* stream);


/*
 * Glue of the PINNSF network around its (PyTorch-ROCm / rocBLAS) GEMMs -- SURVEY.md row a8:
 * "only the desired-force term and k-sum are candidates to fuse".  The GEMMs stay in torch.
 *
 * piml_pinnsf_epilogue_fwd/bwd: the tail of every PINNSF.forward,
 *   predictions = acc_ped + acc_obs + (v0 * dest/|dest| - v) / tau     (src/models/model.py:1289-1294)
 * on rows of self_features = [dest - p (2), v (2), a (2), v0 (1)] (7 floats, contiguous), with the
 * reference's guard |dest| == 0 -> |dest| + 0.1.  The per-row norm only (2-D input, or
 * fix_dest_norm): the channelled dim=1 quirk (Q2) stays a torch expression.  acc_obs may be NULL.
 * bwd: g_self (rows,7) from g_out (rows,2); d/d(acc_ped) = d/d(acc_obs) = g_out (no kernel).
 */
int piml_pinnsf_epilogue_fwd(const float* acc_ped, const float* acc_obs, const float* self_features,
                             size_t rows, float tau, float* out, void* stream);
int piml_pinnsf_epilogue_bwd(const float* g_out, const float* self_features, size_t rows, float tau,
                             float* g_self, void* stream);
/*
 * The same tail for the bottleneck variants (src/models/model.py:1116-1134): predictions = sum over the neighbour axis of
 * the per-row predictor outputs pred_ped (rows, kp, 2) [+ pred_obs (rows, ko, 2), may be NULL] + the desired-force term;
 * backward: g_self (may be NULL) and the upstream gradient broadcast to every neighbour row (either may be NULL).
 */
int piml_pinnsf_epilogue_ksum_fwd(const float* pred_ped, int kp, const float* pred_obs, int ko, const float* self_features,
                                  size_t rows, float tau, float* out, void* stream);
int piml_pinnsf_epilogue_ksum_bwd(const float* g_out, const float* self_features, size_t rows, float tau, int kp, int ko,
                                  float* g_self, float* g_pred_ped, float* g_pred_obs, void* stream);

/*
 * The same tail for channelled (C, N, 7) input with the reference's literal `dim=1` norm (quirk Q2): the
 * norm of each destination component is taken over the N AGENTS of slice c,
 * t[c, comp] = || self_features[c, :, comp] ||_2 (+0.1 where 0), as src/models/model.py:1290 computes it in
 * the fine-tuning rollouts (src/models/simulators.py:701).  One workgroup per slice.
 */
int piml_pinnsf_epilogue_agentnorm_fwd(const float* acc_ped, const float* acc_obs, const float* self_features,
                                       int C, int N, float tau, float* out, void* stream);
/* piml_pinnsf_epilogue_ksum_fwd with the agent-axis norm of piml_pinnsf_epilogue_agentnorm_fwd (quirk Q2): the bottleneck
 * variants' tail on the channelled (C, N, .) frames of the training rollout -- neighbour-axis sums + desired force in one launch.
 * Backward: piml_pinnsf_epilogue_ksum_bwd with g_self = NULL (the broadcasts) + piml_pinnsf_epilogue_agentnorm_bwd. */
int piml_pinnsf_epilogue_ksum_agentnorm_fwd(const float* pred_ped, int kp, const float* pred_obs, int ko, const float* self_features,
                                            int C, int N, float tau, float* out, void* stream);
int piml_pinnsf_epilogue_agentnorm_bwd(const float* g_out, const float* self_features, int C, int N, float tau,
                                       float* g_self, void* stream);

/*
 * self_features rows for the model from the packed state: out (rows,7) = [dest_feat (ld dest_ld),
 * state[:, 2:6] (v, a; interleaved (p,v,a) records, 6 floats), desired_speed] -- the torch.cat at
 * src/models/simulators.py:648-650 / 777-779.  dest_feat NULL: columns 0-1 of `out` are left as they
 * are (piml_relfeat_fwd wrote them in place with dest_feat_ld = 7).  bwd splits g_self into g_dest (rows,2),
 * g_state (rows,6; position columns zero) and g_speed (rows).
 */
int piml_self_features_fwd(const float* dest_feat, int dest_ld, const float* state, const float* desired_speed,
                           size_t rows, float* out, void* stream);
int piml_self_features_bwd(const float* g_self, size_t rows, float* g_dest, float* g_state, float* g_speed,
                           void* stream);

/*
 * Backward glue of one Linear(+ReLU) layer: g_pre = g * [y > 0] (y = the layer's output; NULL: no
 * activation, g_pre is not written) and bias gradient db[c] = sum_r g_pre[r,c], in ONE pass over
 * g (replaces torch's threshold_backward + column reduce_kernel + its semaphore memset).
 * g, y, g_pre: (rows, cols) row-major.  Deterministic two-level sum in a fixed order: slabs of rows ->
 * `partials` (piml_colsum_blocks(rows, cols) * cols floats, caller-owned scratch; may be NULL when
 * that count is 1), then one small second launch over the partials.  No atomics, no global state.
 * cols <= 1024 when cols % 4 == 0, else cols <= 256.
 */
int piml_colsum_blocks(size_t rows, int cols);
int piml_act_bwd_colsum(const float* g, const float* y, size_t rows, int cols, float* g_pre, float* partials,
                        float* db, void* stream);

/*
 * out[j] = sum_b parts[b, j] for parts (B, n) row-major, n % 4 == 0, in a fixed order: the reduction step of
 * the chunked weight-gradient formulation dW = sum_b G_b^T X_b (the per-chunk products are one strided-batched
 * library GEMM; see ops._MLPChain), replacing the library's split-K GEMM + its reduction kernel.
 */
int piml_sum_leading(const float* parts, int B, size_t n, float* out, void* stream);
/*
 * The two small reductions that close one layer's backward in ONE launch: piml_sum_leading on (parts, B, n,
 * out) and the second stage of the bias-gradient sum on the `col_partials` (nb, cols) that
 * piml_act_bwd_colsum_stage1 left behind (same contract as piml_act_bwd_colsum minus its second launch; with
 * piml_colsum_blocks(rows, cols) == 1 it has already written db and there is nothing left to do).
 * Either half may be absent (parts NULL / col_partials NULL or nb <= 1).
 */
int piml_act_bwd_colsum_stage1(const float* g, const float* y, size_t rows, int cols, float* g_pre, float* partials,
                               float* db, void* stream);
int piml_layer_reduce(const float* parts, int B, size_t n, float* out, const float* col_partials, int nb, int cols,
                      float* db, void* stream);

/*
 * Neighbour-axis sum of the PINNSF processor output (src/models/model.py:1279-1283 with quirk Q3:
 * processor(x) = scale * x, scale = 2 in eval mode): msgs = scale * e (rows,cols) and
 * pooled[r / k] = sum over the k rows of one agent of msgs.  bwd: g_e = scale * (g_pooled[r / k] +
 * g_msgs[r]) with g_msgs optional (NULL).  cols % 4 == 0.
 * col_partials (optional, piml_ksum_blocks(agents, cols) * cols floats, needs 256 % (cols / 4) == 0): per-block
 * column sums of g_e, i.e. the first stage of the bias gradient of the Linear that produced e (finish with
 * piml_layer_reduce) -- saves that layer's own pass over g_e.
 * bias (cols, optional): msgs = scale * (e + bias) -- the bias of the encoder's last Linear, when that layer was
 * run as a plain GEMM (its bias-epilogue variant is the slower kernel); the gradient w.r.t. that bias is still
 * the column sum of g_e, which the layer's own backward computes.
 * keep_bits (optional, piml_dropout_keep_bits layout): the processor's train-mode dropout, msgs = keep * scale * (..)
 * with scale = 2 / (1 - p) chosen by the caller; bwd: g_e = keep * scale * (..).
 */
int piml_scale_ksum_fwd(const float* e, const float* bias, size_t agents, int k, int cols, float scale,
                        const unsigned* keep_bits, float* msgs, float* pooled, void* stream);
int piml_ksum_blocks(size_t agents, int cols);
int piml_scale_ksum_bwd(const float* g_pooled, const float* g_msgs, size_t agents, int k, int cols, float scale,
                        const unsigned* keep_bits, float* g_e, float* col_partials, void* stream);

/*
 * Keep-mask of the PINNSF processor's dropout.  The reference's processor is Dropout_p(2 x) in train mode
 * (src/models/model.py:82-119 with quirk Q3; model.train() at src/models/simulators.py:311; --dropout 0.5 at
 * src/main.py:45): the fused kernels take the mask as bits -- keep_bits (rows, ceil(cols / 32)) dwords, bit (c & 31)
 * of word (c >> 5) of a row = feature c of that row is kept -- and the caller folds 1 / (1 - p) into `scale`.
 *   state: 4 x uint64 on the device: [seed, offset, ticket, unused].  Every call draws with draw number `offset` and
 *          advances `offset` by one ON THE DEVICE (last block out), so a call captured into a hipGraph draws a fresh
 *          mask on every replay.  Philox4x32-10, counter = (offset lo, offset hi, row, (stream_id << 16) | sub),
 *          key = (seed lo, seed hi).  p == 0.5: keep word w of a row = output word w & 3 of the call
 *          sub = 0xFFFF - (w >> 2) (one call per 128 features).  Other p: feature c takes 16 bits -- call sub = c >> 3,
 *          output word (c >> 1) & 3, half c & 1 -- and is kept iff they are >= round(p * 65536).
 *   stream_id (0 .. 65535) tells masks of the same draw apart (the two branches of one encoder launch use 0 and 1).
 *   p in [0, 1]; p = 1 keeps nothing.
 */
int piml_dropout_keep_bits(unsigned long long* state, long long rows, int cols, float p, int stream_id, unsigned* keep_bits,
                           void* stream);

/*
 * Fused PINNSF encoder on the matrix cores (piml_amd/csrc/encoder_x3.hip: f32 products as split bf16 products, the
 * default; piml_amd/csrc/encoder.hip: the f32 matrix instruction; see piml_encoder_products): the reference's
 *   ped_encoder / obs_encoder = MLP(in, [128, 128, 128]) (src/models/model.py:40-65, built at :1232-1236),
 *   the processor in its effective form `scale * x` (ResDNN with >= 2 "layers" and inactive dropout, :82-119,
 *   SURVEY quirk Q3) and the neighbour-axis sum (:1279-1283),
 * i.e. msgs = scale * (W3 relu(W2 relu(W1 x + b1) + b2) + b3) for every neighbour row and pooled = sum over the k
 * rows of an agent.  Weights use the nn.Linear layout (out, in), row-major.  Up to two encoders (pedestrian and
 * obstacle branch) run in ONE launch, workgroups split in proportion to their rows.
 *
 * fwd:  x (rows, in_dim <= 8) -> msgs (rows, 128); h1 / h2 (rows, 128): post-ReLU activations of layers 1 / 2,
 *       saved for the backward (NULL for inference).  pooled comes from piml_encoder_ksum.
 *       h1 may be NULL in forward AND backward (every branch) when the backward does without it: relu_mask given, split
 *       products, more than piml_encoder_split_tiles() tiles (the dX chain then masks with the sign bits), layer-split
 *       weight gradients (piml_encoder_dw2, which recompute h1 from x on the matrix cores) and at least two workgroups per
 *       branch (piml_encoder_workgroups) -- 33 MB less to write and 33 MB less to read at the 4096-agent scene.
 * bwd:  upstream g_pooled (rows / k, 128) and / or g_msgs (rows, 128) (one may be NULL)
 *       -> g2, g1 (rows, 128): caller-provided scratch, the gradients at the pre-activations of layers 2 and 1;
 *          g_x (rows, in_dim) or NULL when the inputs need no gradient;
 *          partials: piml_encoder_workgroups() slots of piml_encoder_partial_floats() floats for THIS branch, slot p
 *          = [dW3 128x128 | dW2 128x128 | dW1 128 x in_dim (row-major, in a 1024-float field) | db3 | db2 | db1] of workgroup p's
 *          row slab; piml_encoder_bwd sums them into `grads` itself (one extra launch for both branches).
 */
typedef struct piml_encoder_branch {
    const float* x;
    long long rows;
    int in_dim;
    int k;
    const float *w1, *b1, *w2, *b2, *w3, *b3;
    float scale;
    float *h1, *h2, *msgs;
    const float *g_pooled, *g_msgs;
    float *g2, *g1, *g_x;
    float* partials;
    float* grads;  /* bwd out: piml_encoder_partial_floats() floats = the slots of `partials` summed (same layout) */
    float* packed; /* piml_encoder_pack_floats() floats of caller-provided scratch: the weights re-ordered into MFMA
                      operand fragments; written by piml_encoder_fwd (or piml_encoder_pack), read by piml_encoder_bwd */
    unsigned* relu_mask; /* optional scratch, 256 dwords per 32-row tile (ceil(rows / 32) tiles): the signs of h1 and h2 as
                      bits.  A forward on the split-product kernels with more than piml_encoder_split_tiles() tiles writes
                      it, and the backward of the SAME configuration then reads these 2 MB instead of h1 and h2 (2 x 33 MB at
                      the 4096-agent scene) in its dX chain; pass the same pointer to both, or NULL to both */
    unsigned* keep_bits; /* optional (rows, 4) dwords, piml_dropout_keep_bits layout: the processor's train-mode
                      dropout.  msgs = keep * scale * (...) in the forward, g3 = keep * scale * (g_pooled + g_msgs) in the
                      backward (dX chain and dW3 / db3); the caller passes scale = 2 / (1 - p) and the same bits to both */
    unsigned long long* drop_state; /* forward only, optional: a piml_dropout_keep_bits state.  Non-NULL: the forward DRAWS the
                      mask of this launch (stream_id = index of the branch) with probability drop_p and leaves it in keep_bits
                      for the backward: for drop_p == 0.5 on the split-product kernels inside the forward kernel itself (one
                      Philox call per row, no extra launch), otherwise by one generator launch for all branches in front of it.
                      The draw counter advances once per launch.  Same state for every branch.  NULL: keep_bits is given */
    float drop_p;
    /* PIML_POOL_TRAIN (piml_pinnsf_fwd / bwd): the branch on the agents' SUMS of h2 instead of on message rows.
     * fwd out: sum_a / sum_b (agents, 128) = the agents' sums of h2 over their k rows, in two parts: sum_a from the 32-row tile
     * the agent's first row lies in, sum_b from the next tile (only for agents whose rows straddle two tiles:
     * (a k) >> 5 != (a k + k - 1) >> 5; undefined for the others).  `relu_mask` is required and holds the signs of h2 in the
     * layout of the exchanged layer (dwords 128 .. 255 of a tile: lane l = (feature j, half h) owns dwords 128 + 2 l, + 1;
     * bit 16 (blk & 1) + r of dword blk >> 1 = h2[row rho(r) + 4 h][32 blk + j] > 0).  `h2` (rows, 128) is written when
     * non-NULL (the collision head reads the rows), `msgs` is not written.  bwd in: g_pooled = d/d(sums) (agents, 128);
     * dW3 / db3 are not produced here (they follow from the decoder's folded first layer: piml_pinnsf_bwd). */
    float *sum_a, *sum_b;
    /* PIML_POOL_TRAIN, optional, branch 1 of a two-branch call only (a branch whose rows nothing reads one by one): COMPACT ROWS.
     * An agent whose first neighbour slot is empty (nbr_idx[agent * k] < 0: the relative-feature kernels fill the slots of a row
     * front to back, and an empty slot is an all-zero feature row) has k identical zero rows, whose layers give one constant.  With
     * nbr_idx (rows ints: the branch's neighbour indices) and plan (PIML_COMPACT_PLAN_INTS(rows / k) ints of scratch) the forward
     * runs only the agents that have a neighbour, 32 / k of them per tile, writes the constant for the others and leaves the
     * lists of both kinds and the backward's workgroup split in `plan`; the backward (same `plan`, nbr_idx not read) follows it and
     * adds the other agents' share of the weight gradients in closed form.  relu_mask must then hold
     * PIML_COMPACT_TILES(rows / k, k) tiles when that is more than ceil(rows / 32), `partials` PIML_COMPACT_SLOTS slots in BOTH
     * branches (the split between them follows the data), and g_x rows of agents without a neighbour are NOT written (they keep
     * whatever the caller's buffer held; the relative-feature backward reads no row whose index is negative).  `packed` must come
     * from piml_pinnsf_pack or piml_encoder_pack of this library version (both write the zero row's constants behind the images).
     * Serves k = 2, 6 or 10 in branch 1, k <= 16 in branch 0, in_dim = 6 in both, rows / k <= PIML_COMPACT_MAX_AGENTS, the two-crew
     * backward (piml_encoder_sums_bwd(2), the default); anything else with these pointers set is hipErrorInvalidValue, in the
     * forward already.  Both NULL: every row goes through the layers. */
    const int* nbr_idx;
    int* plan;
} piml_encoder_branch;
#define PIML_COMPACT_MAX_AGENTS 16384
#define PIML_COMPACT_PLAN_INTS(agents) (16 + 2 * (((agents) + 3) / 4 * 4))
#define PIML_COMPACT_TILES(agents, k) (((agents) + 32 / (k) - 1) / (32 / (k)))
#define PIML_COMPACT_SLOTS 256

/* floats of one partial slot / of one `packed` buffer */
int piml_encoder_partial_floats(void);
int piml_encoder_pack_floats(void);
/* (re)fill `packed` from the weights; piml_encoder_fwd does this itself, piml_encoder_bwd expects it done */
int piml_encoder_pack(const piml_encoder_branch* branches, int nbranches, void* stream);
/* total workgroups of a launch over these branches; *wg_branch0 = how many of them serve branch 0 (the rest serve
 * branch 1): the number of partial slots each branch's `partials` must hold. */
int piml_encoder_workgroups(const piml_encoder_branch* branches, int nbranches, int* wg_branch0);
int piml_encoder_fwd(const piml_encoder_branch* branches, int nbranches, void* stream);
/* the forward alone: `packed` already holds the images of these weights (piml_encoder_pack / piml_pinnsf_pack), e.g. one
 * pack per rollout or per back-propagated window instead of one per frame */
int piml_encoder_fwd_packed(const piml_encoder_branch* branches, int nbranches, void* stream);
int piml_encoder_bwd(const piml_encoder_branch* branches, int nbranches, void* stream);
/* accumulate = 1 (or PIML_ACCUMULATE): `grads` += the slot sums instead of = (a further backward pass through the same weights
 * within one optimiser step -- the frames of a training rollout; cf. PIML_ACCUMULATE of piml_pinnsf_bwd).  | PIML_DEFER_SLOT_SUMS:
 * the slot sums are not launched here but left for the next piml_relfeat_self_bwd on the stream (or piml_pinnsf_slot_sums_flush),
 * which runs them as leading workgroups of its launch -- together with those a piml_rowdecoder_bwd_acc of the same backward pass
 * left (the bottleneck variants: three launches become one); `partials` and `grads` must stay alive until then. */
int piml_encoder_bwd_acc(const piml_encoder_branch* branches, int nbranches, int accumulate, void* stream);
/* pooled (agents, 128) = sum over k consecutive rows of msgs (agents * k, 128) */
int piml_encoder_ksum(const float* msgs, long long agents, int k, float* pooled, void* stream);

/*
 * Fused PINNSF decoder tail on the f32 matrix cores (piml_amd/csrc/decoder.hip), reference
 * src/models/model.py:1283-1294 (`pinnsf_m`, same in `pinnsf`):
 *   pooled = sum over the k neighbour rows of msgs;  acc_branch = predictor(decoder(pooled)) with
 *   decoder = Linear(128, 64) ReLU Linear(64, 64), predictor = Linear(64, 2);
 *   acc = acc_ped [+ acc_obs] [+ (v0 * dest / |dest| - v) / tau when self_features (agents, 7) is given].
 * Both branches have the same number of agents.  Weights: nn.Linear layouts w1 (64,128) b1 (64) w2 (64,64) b2 (64)
 * w3 (2,64) b3 (2).  fwd writes pooled (agents,128), h1 (agents,64: post-ReLU), d2 (agents,64: decoder output) when
 * the pointers are given (needed by bwd) and `packed` (piml_decoder_pack_floats() floats, re-used by bwd).
 * bwd: g_pred (agents,2) -> g_pooled (agents,128) per branch; g_pre2 / g_pre1 (agents,64) are caller scratch;
 * g_self (agents,7, optional) = gradient of the desired-force term; partials: piml_decoder_workgroups(agents) slots of
 * piml_decoder_partial_floats() floats per branch = [dW1 64x128 | dW2 64x64 | dW3 2x64 | db1 64 | db2 64 | db3 2 +
 * 6 pad]; piml_decoder_bwd sums the slots into `grads` (same layout) itself.
 */
typedef struct piml_decoder_branch {
    const float* msgs;
    long long agents;
    int k;
    const float *w1, *b1, *w2, *b2, *w3, *b3;
    float *pooled, *h1, *d2;
    float *g_pre2, *g_pre1, *g_pooled;
    float* partials;
    float* grads; /* bwd out: piml_decoder_partial_floats() floats, the partial slots summed */
    float* packed;
    /* per-ROW use of the same network (the bottleneck variants, piml_rowdecoder_*): */
    float* pred;              /* fwd out (rows, 2): predictor output of every row */
    const float* g_pred_rows; /* bwd in (rows, 2) */
    const float* g_d2;        /* bwd in (rows, 64) or NULL: extra gradient on the decoder output (the `decoded` collision head) */
    /* PIML_POOL_TRAIN: the encoder's last layer folded into this decoder's first (msgs = scale (W3 h2 + b3) is linear in h2, so
     * W_d1 sum_r msgs_r + b_d1 = (scale W_d1 W3) sum_r h2_r + (b_d1 + k scale W_d1 b3)).  Non-NULL fold_w3 (128, 128) / fold_b3
     * (128) = that encoder's w3 / b3, fold_scale = its processor scale: the pack ALSO writes the folded images (float64
     * products, rounded once) behind the plain ones in `packed`; forward and backward use them under PIML_POOL_TRAIN.
     * `w1` / `b1` stay the raw decoder weights.  Then pooled = the agents' sums of h2 (first parts in, completed sums out),
     * msgs = their second parts (agents, 128), g_pooled = d/d(sums); in `grads` the dW1 / db1 fields hold the gradient of the
     * FOLDED layer until the slot sums' epilogue has unfolded them (dw1_out below). */
    const float *fold_w3, *fold_b3;
    float fold_scale;
    float* dw1_out; /* PIML_POOL_TRAIN bwd out (64, 128): d/d(w1) of the raw first layer (`grads`' dW1 field keeps d/d(W1')) */
} piml_decoder_branch;

int piml_decoder_pack_floats(void);
int piml_decoder_partial_floats(void);
int piml_decoder_workgroups(long long agents);
int piml_decoder_fwd(const piml_decoder_branch* branches, int nbranches, const float* self_features, float tau,
                     float* acc, void* stream);
int piml_decoder_bwd(const piml_decoder_branch* branches, int nbranches, const float* g_pred,
                     const float* self_features, float tau, float* g_self, void* stream);

/*
 * Collision head of `pinnsf_m` (src/models/model.py:1246, 1296-1300): out[row] = sigmoid(w2 . relu(W1 msgs[row] + b1)
 * + b2), msgs (rows, 128), W1 (64, 128), w2 (1, 64); forward only.  `packed`: piml_collision_head_pack_floats()
 * floats of scratch.  The 128 -> 64 layer runs as f32 arithmetic on split bf16 products like the encoder layers
 * (piml_amd/csrc/decoder.hip: head_fwd_body_x3; environment PIML_HEAD_PRODUCTS=f32 at load time: the f32 matrix
 * instruction); both stay within 1e-6 of float64 (tests/test_encoder_gpu.py).
 */
/*
 * The bottleneck variants (`pinnsf_bottleneck`, `pinnsf_bm`, src/models/model.py:1062-1221) apply decoder + predictor to
 * every NEIGHBOUR row and sum the (rows, 2) outputs over the neighbour axis afterwards (:1116-1122).  Same kernels, the
 * rows in the role of the agents: `msgs` = the (rows, 128) embeddings (read directly, no pooling; `pooled` unused),
 * `agents` = rows of the branch (the two branches may differ), `pred` / `h1` / `d2` per row; backward: `g_pred_rows`
 * (+ `g_d2`), `g_pooled` = d/d(embeddings) (rows, 128), weight-gradient partials in piml_rowdecoder_slots(rows) slots per
 * branch (slabs of a multiple of 32 rows), summed into `grads`.  One launch forward, three backward (dX, dW, slot sum).
 */
int piml_rowdecoder_slots(long long rows);
int piml_rowdecoder_fwd(const piml_decoder_branch* branches, int nbranches, void* stream);
int piml_rowdecoder_fwd_packed(const piml_decoder_branch* branches, int nbranches, void* stream); /* without the pack launch */
int piml_rowdecoder_bwd(const piml_decoder_branch* branches, int nbranches, void* stream);
int piml_rowdecoder_bwd_acc(const piml_decoder_branch* branches, int nbranches, int accumulate, void* stream);   /* grads +=, see piml_encoder_bwd_acc */

typedef struct piml_collision_head {
    const float* msgs; /* (rows, 128) */
    long long rows;
    const float *w1, *b1, *w2, *b2;
    float* packed; /* piml_collision_head_pack_floats() floats */
    float* out;    /* (rows) */
    /* PIML_POOL_TRAIN: the head on h2 rows (msgs = that array) with the encoder's last layer folded into W1:
     * W1' = fold_scale W1 fold_w3, b1' = b1 + fold_scale W1 fold_b3 (packed behind the plain images when fold_w3 is given) */
    const float *fold_w3, *fold_b3;
    float fold_scale;
} piml_collision_head;

int piml_collision_head_pack_floats(void);
int piml_collision_head_fwd(const float* msgs, long long rows, const float* w1, const float* b1, const float* w2,
                            const float* b2, float* packed, float* out, void* stream);

/*
 * Collision head of `pinnsf_bm`, forward and backward (piml_amd/csrc/head64.hip).  Reference: src/models/model.py:1183
 * `ped_collision_predictor = MLP(64, [64, 1])`, :1214-1215 `sigmoid(...)` on the decoder output of every pedestrian
 * neighbour row; trained with BCE against the 1-s collision labels (src/models/simulators.py:348-355).
 *   out[row] = sigmoid(w2 . relu(W1 x[row] + b1) + b2),   x (rows, 64), W1 (64, 64), w2 (1, 64), nn.Linear layouts.
 * fwd: x -> out (rows), hidden (rows, 64: post-ReLU, saved for bwd; NULL for inference).
 * bwd: g_out (rows), out, hidden, x -> g_x (rows, 64; NULL = not wanted); partials = piml_head64_slots(rows) slots of
 *      piml_head64_partial_floats() floats of scratch; grads (same layout as one slot) = [dW1 64x64 | db1 64 | dw2 64 |
 *      db2 1 | 3 pad].  Two launches (tiles + slot sum), no atomics.  One slot per workgroup: four 32-row tiles per workgroup above
 *      2048 tiles, below that ONE tile per workgroup with its four waves on disjoint blocks of the tile's products (the training
 *      loops' few thousand rows: 14.6 -> 6 us per launch).
 */
typedef struct piml_head64 {
    const float* x;
    long long rows;
    const float *w1, *b1, *w2, *b2;
    float* hidden;
    float* out;
    const float* g_out;
    float* g_x;
    float* partials;
    float* grads;
} piml_head64;
int piml_head64_partial_floats(void);
int piml_head64_slots(long long rows);
int piml_head64_fwd(const piml_head64* head, void* stream);
int piml_head64_bwd(const piml_head64* head, void* stream);
int piml_head64_bwd_acc(const piml_head64* head, int accumulate, void* stream);   /* grads +=, | PIML_DEFER_SLOT_SUMS: see piml_encoder_bwd_acc */

/*
 * The corrector of `pinnsf_res` (src/models/model.py:1016-1020, :1050-1052; attn_pooling :950-970; ResDNN :82-119) on
 * hand-written kernels (piml_amd/csrc/corrector.hip), forward and backward:
 *     r = keep * scale * enc,  hid = relu(Wa r + ba),  s = wb . hid + bb,  attn = softmax_k(exp(s)),
 *     pooled = sum_k attn r,   out = Wd relu(Wc pooled + bc) + bd
 * enc (agents * k, 128): the pedestrian encoder's raw output, an agent's k neighbour rows consecutive; scale / keep_bits:
 * what corrector[0] (a ResDNN of >= 2 "layers" = Dropout(2 x)) does to it -- scale 2 in eval mode, 2 / (1 - p) and the
 * keep-mask bits (rows, 4) int32 of piml_dropout_keep_bits in train mode (NULL: keep everything); weights in nn.Linear
 * layouts: wa (128, 128), ba (128), wb (1, 128), bb (1), wc (64, 128), bc (64), wd (2, 64), bd (2).
 * fwd writes hid (rows, 128; NULL for inference), score / attn (rows), pooled (agents, 128), chid (agents, 64), out (agents, 2).
 * bwd reads them (not `out`, which may be NULL there) and g_out (agents, 2); writes g_enc (rows, 128; NULL = not wanted); scratch g_pooled (agents, 128),
 *     g_score (rows), g_chid (agents, 64), partials_a = piml_corrector_slots(0, ..) x piml_corrector_partial_floats(0) floats, partials_b likewise
 *     with 1; grads = [dWa 128x128 | dba 128 | dwb 128 | dbb 1 | 3 pad | dWc 64x128 | dbc 64 | dWd 2x64 | dbd 2 | 2 pad];
 *     accumulate != 0: grads += (see piml_encoder_bwd_acc).  No atomics: bit-reproducible.
 */
typedef struct piml_corrector {
    long long agents;
    int k;
    float scale;
    const float* enc;
    const unsigned* keep_bits;
    const float *wa, *ba, *wb, *bb, *wc, *bc, *wd, *bd;
    float *hid, *score, *attn, *pooled, *chid, *out;
    const float* g_out;
    float *g_pooled, *g_score, *g_chid, *g_enc;
    float *partials_a, *partials_b, *grads;
} piml_corrector;
int piml_corrector_partial_floats(int which);
int piml_corrector_slots(int which, long long agents, int k);
int piml_corrector_fwd(const piml_corrector* c, void* stream);
int piml_corrector_bwd(const piml_corrector* c, int accumulate, void* stream);

/*
 * The whole non-bottleneck PINNSF network (src/models/model.py:1271-1305: both encoders, the decoder tails, the
 * desired-force epilogue and, for `pinnsf_m`, the collision head) as ONE call per direction.  Default: the stages run in
 * program order on `stream` -- what a captured HIP graph wants:
 *
 *   piml_pinnsf_pack   ONE launch for the MFMA operand images of every weight (encoder x 2, decoder x 2, head) -> the
 *                      `packed` fields.  Weights that did not change since the last pack (rollouts, evaluation, the frames
 *                      of one back-propagated window) need no repack: pass PIML_PACKED_VALID to fwd.  flags: reserved (0).
 *   piml_pinnsf_fwd    [pack unless PIML_PACKED_VALID] -> encoders (both branches, one launch; draws the dropout masks
 *                      itself when the branches carry drop_state) -> [neighbour-axis sums + decoder tails + desired force +
 *                      collision head] (one launch).  head may be NULL.
 *   piml_pinnsf_bwd    [decoder dX chain + decoder dW partials] -> encoder dX -> encoder dW -> ONE slot sum for all four
 *                      partial sets.  Same fields as piml_decoder_bwd / piml_encoder_bwd.
 * flags: PIML_PACKED_VALID (fwd: skip the pack); PIML_FORK (opt-in: the independent stages on library-owned side streams
 * with event fork / join -- packs and collision head beside the encoders, decoder dW beside the encoder chain.  Measured
 * SLOWER inside captured graphs on ROCm 7.2, where every cross-stream edge of a replayed graph costs more than the ~5 us
 * stage it hides: 0.247 ms/step serial vs 0.295 forked at cfg3, DESIGN.md.  The side streams are created per device on
 * first use, outside any capture: piml_pinnsf_streams_init, idempotent).
 */
/* piml_pinnsf_unfold_defer(1, NULL): from now on (this device) a PIML_POOL_TRAIN backward does not launch the unfold of its folded
 * layers' gradients behind its slot sums but leaves it with the library; piml_pinnsf_unfold_defer(0, stream) launches what is
 * waiting (on `stream`, or on the stream it was left on when NULL) and ends the deferral.  For the backward passes of ONE
 * optimiser step that accumulate into the same buffers (PIML_ACCUMULATE: the frames of the rollout of
 * src/models/simulators.py:699-779): the unfold reads the folded layers' summed gradients and overwrites the unfolded ones, so
 * only the last pass's matters -- one launch per step instead of one per pass.  Another network's backward in between launches
 * what is waiting first.  Until the closing call dw1_out and the dW3 / db3 fields of the encoders' `grads` are NOT valid.  Only
 * backward passes that ask for it with PIML_DEFER_UNFOLD are deferred; every other one launches its unfold behind its sums as
 * outside the deferral. */
int piml_pinnsf_unfold_defer(int on, void* stream);
#define PIML_PACKED_VALID 1
#define PIML_FORK 2
#define PIML_ACCUMULATE 4 /* piml_pinnsf_bwd: every branch's `grads` += the slot sums instead of = (a further backward pass through
                             the same weights inside one optimiser step: the frames of a training rollout); not with PIML_FORK */
#define PIML_DEFER_SLOT_SUMS 8 /* piml_pinnsf_bwd: do NOT launch the slot sums; leave them with the library, which runs them as the
                                  leading workgroups of the next piml_relfeat_self_bwd on the same stream (the two kernels are
                                  independent and small: one launch boundary, ~5 us, less per step), or -- whichever comes first
                                  -- at piml_pinnsf_slot_sums_flush / at the next deferring piml_pinnsf_bwd.  Until then the
                                  branches' `grads` are NOT valid: for callers that know a relfeat backward follows (the step of
                                  src/models/simulators.py:699-779: network backward, then the features' backward); not with PIML_FORK */
#define PIML_DEFER_PACK 16 /* piml_pinnsf_pack: do NOT launch; the next relfeat FORWARD launch on the same stream (piml_relfeat_self_fwd,
                              piml_relfeat_self_fwd_part, piml_relfeat_fwd_self) runs the pack as its trailing workgroups -- the
                              pack depends on the weights only and is a ~4 us launch in front of the step's chain by itself.
                              Whichever comes first: every consumer of packed images (piml_pinnsf_fwd, piml_encoder_fwd_packed,
                              piml_rowdecoder_fwd_packed) and piml_pinnsf_pack_flush launch a pack that is still waiting */
#define PIML_POOL_H2 32 /* piml_pinnsf_fwd, INFERENCE only (no head, no dropout, no backward): msgs = scale (W3 h2 + b3) is linear in
                           h2, so the neighbour-axis sum is taken BEFORE the last encoder layer.  The encoder launch stops after layer 2
                           and writes the agents' sums of h2: enc[i].msgs (agents, 128) = the part from the 32-row tile the agent's
                           first row lies in, enc[i].h2 (agents, 128) = the part from the next tile (agents whose k rows straddle two
                           tiles: (a k) >> 5 != (a k + k - 1) >> 5; undefined for the others).  dec[i].pooled = the same buffer as
                           enc[i].msgs, dec[i].msgs = the same as enc[i].h2; the decoder tails run on their sum.  The CALLER folds
                           the skipped layer into the decoder's first layer -- dec[i].w1 = scale * W_d1 * W3 (64 x 128),
                           dec[i].b1 = b_d1 + scale * k * W_d1 * b3 -- when it packs; enc[i].w3 / b3 / scale are not read.
                           Served when piml_pinnsf_pool_h2_ok(enc, nbranches): k = 6 or 10, split products, more than 32 tiles of
                           32 rows (environment PIML_POOL_H2_MIN_TILES); hipErrorInvalidValue otherwise */
#define PIML_POOL_TRAIN 64 /* piml_pinnsf_fwd AND piml_pinnsf_bwd (the same call pair): TRAINING on the agents' sums of h2 -- for
                           processors without an active dropout mask (eval mode, or p = 0) and callers that read neither branch's
                           per-row messages (the reference's training loops read predictions[0] only unless reg_weight > 0:
                           src/models/simulators.py:331-347, :702-737).  The messages are linear in h2, so the neighbour-axis sum moves
                           in front of the encoders' last layer (layer 2 runs with exchanged operands: a tile's rows sit on registers
                           and an agent's sum is register additions), that layer is folded into the decoders' first layer and into
                           the collision head's (fold_w3 / fold_b3 / fold_scale of piml_decoder_branch / piml_collision_head, packed
                           by piml_pinnsf_pack), and its gradient is recovered from the folded layers' gradients after the slot sums:
                               dW_d1 = s (G W3^T + k g_b b3^T),  dW3 = s W_d1^T G,  db3 = s k W_d1^T g_b     (G = d/d(W_d1'), g_b = d/d(b_d1')).
                           Backward: every row of an agent sees the same upstream gradient g = d/d(sum), so G2 = g[agent] * [h2 > 0]
                           directly -- the W3^T chain layer and the dW3 = G3^T H2 product over all rows (half of the backward's
                           matrix work, and the 33 MB of saved h2) are gone.  enc[i].sum_a / sum_b / relu_mask, dec[i].pooled =
                           enc[i].sum_a, dec[i].msgs = enc[i].sum_b, dec[i].fold_*, head->msgs = enc[0].h2, head->fold_*.
                           Served when piml_pinnsf_pool_train_ok(enc, nbranches): k in {2, 6, 10}, whole agents, split products,
                           more than piml_encoder_split_tiles() tiles, no keep_bits / drop_state; hipErrorInvalidValue otherwise */
#define PIML_POOL_MSGS 128 /* piml_pinnsf_fwd only (the backward is the plain one): the agents' sums of the MESSAGES written by the
                           encoder forward itself -- for training passes whose dropout mask keeps the sum from moving in front of the
                           last layer (PIML_POOL_TRAIN) and whose caller does not read the per-row messages.  The last encoder layer
                           runs with exchanged operands (a tile's rows on registers), the keep bits of a row travel from the lane that
                           drew / loaded them to the lanes that own its features, and the sums leave as enc[i].sum_a / sum_b
                           (dec[i].pooled = enc[i].sum_a, dec[i].msgs = enc[i].sum_b; the decoder completes them in `pooled`, where
                           the backward's dW1 reads them).  enc[i].msgs may be NULL: the rows of a branch are stored only where it is
                           not (the collision head's input: head->msgs = enc[0].msgs).  Everything the plain backward reads is left
                           as by the plain forward (h2, relu_mask, keep_bits, the decoders' h1 / d2).  Reference arithmetic:
                           src/models/model.py:82-119 (processor), :1279-1283 (the sum).  Served when
                           piml_pinnsf_pool_msgs_ok(enc, nbranches): k in {2, 6, 10}, whole agents, split products, relu_mask given,
                           more than piml_encoder_split_tiles_train() tiles; hipErrorInvalidValue otherwise */
#define PIML_DEFER_UNFOLD 256 /* piml_pinnsf_bwd with PIML_POOL_TRAIN: this pass's unfold may wait for piml_pinnsf_unfold_defer(0, ...)
                                 while a deferral is on.  The decision travels with the pass (its slot sums too, when PIML_DEFER_SLOT_SUMS
                                 leaves them to a later launch): a pass without the flag launches its unfold behind its sums even while
                                 the device defers -- for callers whose gradient buffers are read, or freed, before the deferral
                                 ends (a pass whose buffers are not the ones the deferring step accumulates into) */
int piml_pinnsf_pool_train_ok(const piml_encoder_branch* enc, int nbranches);
int piml_pinnsf_pool_msgs_ok(const piml_encoder_branch* enc, int nbranches);
int piml_pinnsf_pool_h2_ok(const piml_encoder_branch* enc, int nbranches);
int piml_pinnsf_pack_flush(void);
int piml_pinnsf_slot_sums_flush(void);   /* launch the deferred slot sums of the current device, if any are waiting (on their stream) */
int piml_pinnsf_pack(const piml_encoder_branch* enc, const piml_decoder_branch* dec, int nbranches,
                     const piml_collision_head* head, int flags, void* stream);
int piml_pinnsf_fwd(const piml_encoder_branch* enc, const piml_decoder_branch* dec, int nbranches,
                    const piml_collision_head* head, const float* self_features, float tau, float* acc, int flags,
                    void* stream);
int piml_pinnsf_bwd(const piml_encoder_branch* enc, const piml_decoder_branch* dec, int nbranches, const float* g_pred,
                    const float* self_features, float tau, float* g_self, int flags, void* stream);

/*
 * RCCL exchange of agent-block sharding (the reference's only multi-GPU mechanism is
 * nn.DataParallel, src/models/simulators.py:64-67).  `comm` is an ncclComm_t (as void*): either one the host already
 * owns, or one made with piml_comm_unique_id (one rank) + piml_comm_init (every rank, after the 128-byte id has been
 * distributed by the host, e.g. through the torch.distributed store).  RCCL is bound at run time (dlopen of the
 * librccl already in the process); piml_comm_available() == 0 when there is none.  Return: 0, a hipError_t, or
 * 10000 + ncclResult_t.
 *   piml_allgather_state     own (floats_per_rank) -> full (world * floats_per_rank): the (p, v, a) records, 6 floats / agent
 *   piml_reducescatter_grad  full (world * floats_per_rank) partial d/d(state) -> own (floats_per_rank), summed over ranks
 *   piml_allreduce_sum       in place, e.g. the flat bucket [d/d(state) | weight gradients]
 */
typedef struct piml_comm_id { char internal[128]; } piml_comm_id;
int piml_comm_available(void);
int piml_comm_unique_id(piml_comm_id* id);
int piml_comm_init(void** comm, int world, int rank, const piml_comm_id* id);
int piml_comm_destroy(void* comm);
int piml_allgather_state(void* comm, const float* own, size_t floats_per_rank, float* full, void* stream);
int piml_reducescatter_grad(void* comm, const float* full, float* own, size_t floats_per_rank, void* stream);
int piml_allreduce_sum(void* comm, float* buf, size_t count, void* stream);

/*
 * P2P-store all-gather of the state records ("fall back to / compare with a P2P-store epilogue ... into peers'
 * double-buffered state arrays"; piml_amd/csrc/p2p.hip; the reference has no counterpart, src/models/simulators.py:64-67 is
 * nn.DataParallel).  No collective library in the data path: every rank stores its block into every peer's receive buffer
 * (xGMI stores between GPUs of a node, plain stores when ranks share a GPU) and raises a flag word per (receiver, sender).
 *   Per rank: recv = piml_p2p_alloc(2 * world * floats_per_rank * 4) and flags = piml_p2p_alloc(2 * world * 4) (zeroed);
 *   both exported (piml_p2p_export -> 64 opaque bytes, carried to the peers by the host: a pipe, the torch.distributed store)
 *   and opened there (piml_p2p_open); a rank's own buffers enter the tables as they are.
 *   piml_allgather_state_p2p(own, floats_per_rank (multiple of 4), rank, world, peer_recv[world], peer_flags[world], seq, ...):
 *   step seq = 1, 2, 3, ... (the same on every rank); on return of the launch's completion recv[seq & 1][s] holds rank s's
 *   block for every s, i.e. recv + (seq & 1) * world * floats_per_rank is the gathered (N, 6) array.  spin_limit: rounds of
 *   ~4 us the wait for the peers' flags may take (0: ~0.5 s); when it runs out status[0] (a device int the caller zeroed) is
 *   set to 1 and the launch ends -- a lost peer is an error to read back, never a hang.
 */
typedef struct piml_ipc_handle { char internal[64]; } piml_ipc_handle;
int piml_p2p_alloc(size_t bytes, void** devptr);
int piml_p2p_free(void* devptr);
int piml_p2p_export(void* devptr, piml_ipc_handle* out);
int piml_p2p_open(const piml_ipc_handle* in, void** devptr);
int piml_p2p_close(void* devptr);
int piml_p2p_copy(void* dst, const void* src, size_t bytes, void* stream);
/* The general exchange step, step counter ON THE DEVICE (no argument changes from step to step: the launch sits inside a captured
 * HIP graph and is replayed with it).  Every rank sends to every receiver r the message [scatter part | broadcast parts ...]:
 *   scatter part    = scatter_src + r * scatter_floats   (the partial d/d(state) rows of r's agent block: reduce-scatter input)
 *   broadcast parts = bcast_src[j], bcast_floats[j] floats, j < n_bcast <= PIML_P2P_MAX_PARTS
 *                     (the rank's own records forward; its weight-gradient buffers backward)
 * into recv_r[parity][rank] (parity = step & 1), raises r's flag, waits for its own `world` flags, then writes
 *   sum == 0: out_scatter[s * scatter_floats + e] / out_bcast[j][s * bcast_floats[j] + e] = what sender s sent (all-gather layout);
 *   sum == 1: out_scatter[e] / out_bcast[j][e] = the senders' parts added IN RANK ORDER (the same sum on every rank).
 * An out pointer may be NULL (that part is not wanted) and may EQUAL its source (in-place sums: no result is written before every
 * workgroup of the launch has read its sources).  Every count is a multiple of 4 floats; slot_floats >= the sum of the parts is
 * the capacity of one (parity, sender) slot of the receive buffers (piml_p2p_alloc(2 * world * slot_floats * 4)).
 * ctr: 3 + world dwords of device memory the host zeroed ONCE (ctr[0] = completed steps).  status: a device int the host zeroed;
 * STICKY -- once a wait ran out (spin_limit rounds of ~0.5 us, 0: ~0.5 s) it is 1 and every later step returns at once, on this
 * rank; the exchange is dead until the hosts rebuild it.  Reference: none (nn.DataParallel, src/models/simulators.py:64-67). */
#define PIML_P2P_MAX_PARTS 8
typedef struct piml_p2p_msg {
    const float* scatter_src;
    size_t scatter_floats;
    float* out_scatter;
    int n_bcast;
    const float* bcast_src[PIML_P2P_MAX_PARTS];
    size_t bcast_floats[PIML_P2P_MAX_PARTS];
    float* out_bcast[PIML_P2P_MAX_PARTS];
    int sum;
} piml_p2p_msg;
int piml_p2p_exchange(const piml_p2p_msg* msg, int rank, int world, float* const* peer_recv, unsigned* const* peer_flags,
                      size_t slot_floats, unsigned* ctr, unsigned spin_limit, int* status, void* stream);
int piml_allgather_state_p2p(const float* own, size_t floats_per_rank, int rank, int world, float* const* peer_recv,
                             unsigned* const* peer_flags, unsigned seq, unsigned spin_limit, int* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PIML_HIP_H */
