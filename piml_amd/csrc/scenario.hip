// Open-world scenario frame: integrate, arrive, retire, spawn and record one simulated frame of a scene whose agents are not
// recorded but generated -- the Grand Central hall of the reference (src/data/scenarios.py:313-401, GC()) and its synthetic
// scenes (scenarios.py:9-311), driven by the frame protocol of RawData.add_frame / add_pedestrians (src/data/data.py:206-303).
// One launch per frame, no host sync: a whole simulation replays as one captured frame (the frame counter and the spawn
// count live in device memory).
//
// Every network-driven entry (piml_scenario_step, piml_scenario_step_rules, piml_scenario_step_members) launches the one
// frame kernel, scenario_frame_kernel<kGC>: kGC is GC's rule (entry points, route, exit distance), otherwise a scene rule of
// piml_scenario_rules.  piml_scenario_step_nav launches the same body as scenario_frame_nav_kernel<kSight>: GC's frame, which
// also writes every slot's steering target from the floor field of nav.hpp (kNav in agent_step and spawn_block).  Grid (agent blocks + spawn blocks, members): a single run is one member whose Philox key is S.seed,
// member m of an ensemble has key seeds[m] (member_view below).
// Frame t -> t+1 (init == 0):
//   agents   (one thread per slot i < min(n_t, capacity), n_t = agents spawned through frame t)
//     1. integrate  v' = v + a dt, p' = p + v dt (the lagged Euler of rollout_step_agent, pairwise.hip), a' = a_next; the
//                   velocity history shifts and columns 2.. of the self_features row get (history, a', v0);
//     2. arrive     GC (scenarios.py:376-384): dis2des = |p' - dest|, dis2exit = min over the points of entry exit(dest) of
//                   |p' - e|, exit(w) = the entry whose points come nearest waypoint w (computed once at spawn); flag += 1
//                   if either is below arrival_radius (at most once per frame).  A scene rule: |p' - dest| < r or
//                   |p'.x - dest.x| < r -> flag += 1, or retire when p'.x > length;
//     3. retire     add_frame (data.py:236-247): flag == D or waypoint[flag] NaN -> p, dest = NaN, v, a = 0, mask 0, for
//                   good; otherwise dest = waypoint[flag];
//   spawn    (one wave per new agent j < k_{t+1}, ordinal n_t + j; ordinals >= capacity are dropped)
//     4. GC: k ~ Poisson(rate dt) by inversion, origin / destination entries distinct and uniform (random.sample(entry, 2)),
//        a point index uniform in 0..P-1 and an offset U[0,1)^2 * spawn_offset for each, waypoints (r, d) = route(o, d)
//        (lanes over the polyline's segments), v0 = max(speed_min, speed_mean + speed_std z) (or speed_mean), v = a = 0.
//        A scene rule: k1 + k2 agents of its spawn law (below);
//   5. record frame t+1's p, v, a, dest, mask into the (T, capacity, .) buffers (skipped from t+1 = T on).
// init == 1 spawns the n_initial agents (ordinals 0 .. n_initial-1) into frame t through the same path (GC's generate(20)).
//
// GC's randomness: Philox4x32-10 (philox.hpp), key = (seed lo, seed hi).  Counter words (c0, c1, c2, c3):
//   spawn count of frame f      (f lo, f hi, 0, 0x5CE00000): word 0 >> 8 = u24; k = #{j < spawn_cap : u24 >= thr[j]},
//                               thr[j] = ceil(2^24 P(K <= j)) computed by the host (the documented cap: P(K > 8 | 0.4) ~ 1e-10)
//   agent of ordinal n, call 1  (n lo, n hi, 0, 0x5CE00001): origin entry (w0 E) >> 32; destination entry (w1 (E-1)) >> 32,
//                               shifted past the origin; origin point (w2 P) >> 32; destination point (w3 P) >> 32
//                      call 2  (n lo, n hi, 0, 0x5CE00002): offsets (w0, w1) of the origin, (w2, w3) of the destination,
//                               each (w >> 8) 2^-24
//                      call 3  (n lo, n hi, 0, 0x5CE00003): z = sqrt(-2 ln u1) cos(2 pi u2) in double, u1 = ((w0 >> 8) + 1)
//                               2^-24, u2 = (w1 >> 8) 2^-24
// The exit choice (piml_nav_choose_exit, scenario_choose_exit_kernel below) draws nothing new: it re-reads calls 1 and 2 of
// the slot's ordinal -- the origin entry, the destination point index and the destination's offset words.
// The dropout keep-mask stream uses c3 = (stream_id << 16) | sub with stream ids 0 and 1: stream 0x5CE0 is never one of
// them.  The schedule depends on (seed, frame, ordinal) only, not on the dynamics; tests/scenario_ref.py restates it.
//
// A scene rule's randomness: c3 = 0x5CE10000 | sub (key = (seed lo, seed hi), the float of a word is (w >> 8) 2^-24 =: u(w),
// a coin is w >> 31):
//   spawn counts of frame f     (f lo, f hi, 0, 0x5CE10000): stream 1 k1 from word 0 >> 8 against thresholds,
//                               stream 2 k2 (UNIT3) from word 1 >> 8 against thresholds2; the frame's first k1 new
//                               ordinals are stream 1's, the next k2 stream 2's (torch.cat of generate(k1, k2))
//   agent of ordinal n, call 1  (n lo, n hi, 0, 0x5CE10001):
//       CROSSWALK       side_x = 2 coin(w0) - 1, side_y = 2 coin(w1) - 1, x = side_x (length/2 + 3 u(w2)),
//                       waypoint y = -width/2 + width coin(w3)
//       UNIT1, UNIT3/1  y = width u(w0), destination y = y + (2 u(w1) - 1)
//       UNIT2           left side u(w0) < side_ratio, right-to-left u(w1) < direction_ratio, y = width/2 u(w2),
//                       destination y = y + (2 u(w3) - 1)
//       UNIT3/2         x = length u(w0), destination x = x + (2 u(w1) - 1)
//       SQUARE          none
//                      call 2  (n lo, n hi, 0, 0x5CE10002): z from (w0, w1) as GC's call 3 (double), when not uniform_speed
//   square cell c's key         (c, 0, 0, 0x5CE10003) word 0: randperm(grid^2)[c] = rank of key c among the grid^2 keys,
//                               ties by cell index (each init wave counts its own cell's rank)
//
// The clip law's randomness (PIML_SPAWN_CLIP, a bootstrap of a recorded clip's arrivals; the table layout is in
// include/piml_hip.h): c3 = 0x5CE20000 | sub, key = (seed lo, seed hi).  The spawn count of a frame is the scene rules'
// stream-1 draw above (0x5CE10000 word 0); there is no second stream.
//   agent of ordinal n, call 1  (n lo, n hi, 0, 0x5CE20001): arrival row n_initial + (((w0 >> 8) Ka) >> 24) (64-bit integer
//                               product, Ka = E - n_initial <= 2^24 arrival rows: exact, every row reachable), origin =
//                               the row's + spawn_offset (2 u(w1) - 1, 2 u(w2) - 1) (not added when spawn_offset == 0)
// The init launch draws nothing: slot i < n_initial is row i.
//
// The grouped clip law's randomness (PIML_SPAWN_CLIP_GROUPS, piml_scenario_step_mlapm_groups only: the clip law whose
// arrivals are UNITS of 1 .. 4 table rows that appear together; row_unit / unit_rows in include/piml_hip.h): c3 =
// 0x5CE30000 | sub, key = (seed lo, seed hi).  The UNIT count k of a frame is again the scene rules' stream-1 draw
// (0x5CE10000 word 0 against poisson_thresholds).
//   unit j < k of frame f       (f lo, f hi, j, 0x5CE30001): unit u = ((w0 >> 8) Ua) >> 24 (64-bit integer product, Ua <= 2^24
//                               units: exact, every unit reachable), first row unit_rows[u], size row_unit[first][1]; one
//                               offset spawn_offset (2 u(w1) - 1, 2 u(w2) - 1) for the whole unit, so that its members keep
//                               their relative geometry (not added when spawn_offset == 0)
// Slots: base_j = n + the sizes of units 0 .. j-1 of the frame; member q takes row first + q into slot base_j + q (dropped,
// never written, from the capacity on) and group_first = base_j, group_size = size.  Block j of the spawn blocks serves unit
// j, its wave q member q; every wave redraws units 0 .. j to find its base (at most 8 Philox calls) and the bookkeeping
// thread all k for the total, so nothing is exchanged between waves.  The init launch draws nothing: slot i is row i,
// group_first = i - row_unit[i][0], group_size = row_unit[i][1].  The draws depend on (seed, frame, unit) only.
//
// The fluctuation term's randomness (piml_scenario_step_mlapm_noise; noise.hpp): c3 = 0x5CE40000 | sub, key = (seed lo,
// seed hi).
//   slot i, step from frame t   (t lo, t hi, i, 0x5CE40001): z_x from (w0, w1), z_y from (w2, w3), each as GC's call 3 (double)
// One call per live slot and frame, by one lane of the slot's wave; absent and retired slots draw nothing.  The draws depend
// on (seed, frame, slot) only, never on the dynamics.
//
// Members: the descriptor's per-member pointers are the bases of member-major buffers, member m's slice of each having
// exactly the single-run layout -- state (members, capacity, .), waypoints (members, D, capacity, 2), exit_idx
// (members, D, capacity), recorded outputs (members, T, capacity, .), spawn_out (members, T), spawned (members, 2),
// dropped (members), a_next (members, capacity, 2).  frame_counter, entries, route_polyline, both threshold tables and
// every scalar are shared.  A block builds member blockIdx.y's view of the descriptor (member_view; a no-op for member 0)
// and runs the frame on it, so member m is bitwise the single run with seed = seeds[m].
//
// Determinism: no atomics.  The spawned count is ping-ponged by frame parity per member (spawned[t & 1] read,
// spawned[(t+1) & 1] written by one thread of block agent_blocks), so no workgroup reads a value another one writes in the
// same launch; spawned agents take slots >= n_t, which no agent thread touches, and no block touches another member's slices.
// The fluctuation term's state eta (members, capacity, 2) keeps the rule: element (m, i) is read and written by lane 0 of the
// one wave that steps live slot i of member m, and by nobody else in the launch -- spawn blocks never touch it (eta = 0 at
// birth is the caller's zero fill), other waves never read it (the pair sum, the wall and the group term read positions).
#include "common.hpp"
#include "groups.hpp"
#include "mlapm.hpp"
#include "nav.hpp"
#include "noise.hpp"
#include "philox.hpp"
#include "walls.hpp"
#include "../../include/piml_hip.h"

#include <cmath>

namespace piml {

constexpr unsigned kScenarioStream = 0x5CE00000u;
constexpr unsigned kRulesStream = 0x5CE10000u;
constexpr unsigned kClipStream = 0x5CE20000u;
constexpr unsigned kGroupStream = 0x5CE30000u;
constexpr unsigned kClipMaxArrivals = 1u << 24; // arrival rows the 24-bit row draw reaches
constexpr int kRulesMaxGrid = 32;
constexpr int kScenarioMaxSpawn = 8;       // spawn_cap bound (the Poisson inversion's cap)
constexpr int kScenarioMaxD = 8;
constexpr int kScenarioMaxIters = 64;
constexpr int kScenarioMaxInitial = 4096;
constexpr int kScenarioLdsPoints = 2048;   // entry points staged in LDS (16 KB) when E * P fits

__device__ __forceinline__ unsigned pick(unsigned w, unsigned n) { return (unsigned)(((unsigned long long)w * n) >> 32); }
__device__ __forceinline__ float unit24(unsigned w) { return (float)(w >> 8) * 5.9604644775390625e-8f; }
__device__ __forceinline__ float qnan() { return __uint_as_float(0x7fc00000u); }

// wave-wide lexicographic minimum of (alpha, j)
__device__ __forceinline__ void wave_argmin(float& a, int& j) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float oa = __shfl_xor(a, o, 64);
        const int oj = __shfl_xor(j, o, 64);
        if (oa < a || (oa == a && oj < j)) { a = oa; j = oj; }
    }
}

__device__ __forceinline__ float wave_min(float x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = fminf(x, __shfl_xor(x, o, 64));
    return x;
}

__device__ __forceinline__ int wave_sum(int x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

// the spawn count of a Poisson draw u24 by inversion: #{j < cap : u >= thr[j]}
__device__ __forceinline__ int threshold_count(unsigned u, const uint32_t* thr, int cap) {
    int k = 0;
    for (int j = 0; j < cap; ++j) k += u >= thr[j];
    return k;
}

// utils.route (src/utils/utils.py:141-165) for one (o, d) pair, one wave: every iteration tests the segment o -> r against
// the polyline's R-1 segments (lanes strided over them), takes the hit with the smallest alpha (lowest segment on a tie, as
// torch.argmin over the ascending hit indices), and moves r to the crossing + clearance * normal.  float32 in the
// reference's operation order (cross_dot_z: product, product, one add).  Returns r; *iters = moves made (<= max_iters).
// Wave-uniform result.
__device__ float2 route_wave(float2 o, float2 d, const float2* __restrict__ poly, int R, int max_iters, float clearance, int* iters) {
    const int lane = lane_id();
    float2 r = d;
    int it = 0;
    for (; it < max_iters; ++it) {
        const float Ax = __fsub_rn(r.x, o.x), Ay = __fsub_rn(r.y, o.y);
        float best = INFINITY;
        int bj = 0x7fffffff;
        for (int j = lane; j < R - 1; j += 64) {
            const float2 p0 = poly[j], p1 = poly[j + 1];
            const float Bx = __fsub_rn(p1.x, p0.x), By = __fsub_rn(p1.y, p0.y);
            const float Cx = __fsub_rn(p0.x, o.x), Cy = __fsub_rn(p0.y, o.y);
            const float det = __fadd_rn(__fmul_rn(Ay, Bx), __fmul_rn(-Ax, By));
            const float alpha = __fdiv_rn(__fadd_rn(__fmul_rn(Cy, Bx), __fmul_rn(-Cx, By)), det);
            const float beta = __fdiv_rn(__fadd_rn(__fmul_rn(Cy, Ax), __fmul_rn(-Cx, Ay)), det);
            if (0.f < alpha && alpha < 1.f && 0.f < beta && beta < 1.f && alpha < best) { best = alpha; bj = j; }
        }
        wave_argmin(best, bj);
        if (bj == 0x7fffffff) break;
        const float al = best;
        const float2 p0 = poly[bj], p1 = poly[bj + 1];
        const float Bx = __fsub_rn(p1.x, p0.x), By = __fsub_rn(p1.y, p0.y);
        const float om = __fsub_rn(1.f, al);
        const float cx = __fadd_rn(__fmul_rn(al, r.x), __fmul_rn(om, o.x));
        const float cy = __fadd_rn(__fmul_rn(al, r.y), __fmul_rn(om, o.y));
        const float s = -__fadd_rn(__fmul_rn(By, Ax), __fmul_rn(-Bx, Ay));
        float nx = __fmul_rn(s, Ay), ny = __fmul_rn(s, -Ax);
        const float nn = norm2(nx, ny);
        nx = __fdiv_rn(nx, nn);
        ny = __fdiv_rn(ny, nn);
        r = make_float2(__fadd_rn(cx, __fmul_rn(clearance, nx)), __fadd_rn(cy, __fmul_rn(clearance, ny)));
    }
    *iters = it;
    return r;
}

// the entry whose points come nearest q (argmin over entries of the min over their points of |q - e|, first entry on a
// tie); one wave.  min_p sqrt_rn(s_p) = sqrt_rn(min_p s_p): the correctly rounded square root is monotonic, so the
// per-entry minimum is taken on the squared distances and rooted once.
__device__ int nearest_entry_wave(float2 q, const float2* entries, int E, int P) {
    const int lane = lane_id();
    float best = INFINITY;
    int be = 0;
    for (int e = 0; e < E; ++e) {
        float m = INFINITY;
        for (int p = lane; p < P; p += 64) {
            const float2 x = entries[(size_t)e * P + p];
            m = fminf(m, sq2(__fsub_rn(q.x, x.x), __fsub_rn(q.y, x.y)));
        }
        m = sqrtf(wave_min(m));
        if (m < best) { best = m; be = e; }
    }
    return be;
}

// frame t+1's record of a slot retired for good
__device__ __forceinline__ void record_retired(const piml_scenario& S, int i, long long t) {
    const long long tn = t + 1;
    if (tn >= S.T) return;
    const size_t fr = (size_t)tn * S.capacity + i;
    ((float2*)S.position_out)[fr] = make_float2(qnan(), qnan());
    ((float2*)S.velocity_out)[fr] = make_float2(0.f, 0.f);
    ((float2*)S.acceleration_out)[fr] = make_float2(0.f, 0.f);
    ((float2*)S.destination_out)[fr] = make_float2(qnan(), qnan());
    S.mask_out[fr] = 0.f;
}

// the velocity history shift and columns 2.. of slot i's self_features row (history, a', v0) after a step to (v', a')
__device__ __forceinline__ void agent_history(const piml_scenario& S, int i, float2 vn, float2 an) {
    const int hw = S.hist_width;
    float* h = S.hist_velocity + (size_t)i * hw;
    float* so = S.self_features + (size_t)i * S.F;
    for (int q = 0; q + 2 < hw; ++q) h[q] = h[q + 2];
    h[hw - 2] = vn.x; h[hw - 1] = vn.y;
    for (int q = 0; q < hw; ++q) so[2 + q] = h[q];
    so[2 + hw] = an.x; so[3 + hw] = an.y; so[4 + hw] = S.desired_speed[i];
}

// 2. arrive, GC's rule (scenarios.py:376-384): m2 = the minimum over the exit entry's points of |p' - e|^2
__device__ __forceinline__ int gc_arrive(const piml_scenario& S, int f, float2 pn, float2 d, float m2) {
    const bool near = norm2(__fsub_rn(pn.x, d.x), __fsub_rn(pn.y, d.y)) < S.arrival_radius || sqrtf(m2) < S.arrival_radius;
    return near ? f + 1 : f;
}

// 2. arrive, a scene rule (scenarios.py:67-69, 128-130, 159-160, 218-219, 286-287); gone: PIML_ARRIVE_XEXIT's exit
__device__ __forceinline__ int rules_arrive(const piml_scenario& S, const piml_scenario_rules& R, int f, float2 pn, float2 d,
                                            bool& gone) {
    gone = false;
    if (R.arrival_rule == PIML_ARRIVE_RADIUS) f += norm2(__fsub_rn(pn.x, d.x), __fsub_rn(pn.y, d.y)) < S.arrival_radius;
    else if (R.arrival_rule == PIML_ARRIVE_XBAND) f += fabsf(__fsub_rn(pn.x, d.x)) < S.arrival_radius;
    else gone = pn.x > R.length;                             // PIML_ARRIVE_XEXIT: mask_p = 0
    return f;
}

// what agent_retire_record left in slot i: whether it is still present, and its destination (NaN when not)
struct SlotAfter {
    bool present;
    float2 dest;
};

// 3. retire (data.py:236-247) with the flag f after step 2 (gone: the rule retired the agent itself), then slot i's state
// and frame t+1's record
__device__ __forceinline__ SlotAfter agent_retire_record(const piml_scenario& S, int i, long long t, int f, bool gone, float2 pn,
                                                    float2 vn, float2 an) {
    const long long tn = t + 1;
    const bool rec = tn < S.T;
    const size_t fr = (size_t)tn * S.capacity + i;
    float2 dn = make_float2(qnan(), qnan());
    gone = gone || f >= S.D;
    if (!gone) {
        dn = ((const float2*)S.waypoints)[(size_t)f * S.capacity + i];
        gone = dn.x != dn.x || dn.y != dn.y;
    }
    float m = 1.f;
    if (gone) {
        pn = make_float2(qnan(), qnan());
        dn = make_float2(qnan(), qnan());
        vn = make_float2(0.f, 0.f);
        an = make_float2(0.f, 0.f);
        m = 0.f;
    }
    ((float2*)S.position)[i] = pn; ((float2*)S.velocity)[i] = vn; ((float2*)S.acceleration)[i] = an;
    ((float2*)S.destination)[i] = dn;
    S.flag[i] = f;
    S.mask[i] = m;
    if (rec) {
        ((float2*)S.position_out)[fr] = pn;
        ((float2*)S.velocity_out)[fr] = vn;
        ((float2*)S.acceleration_out)[fr] = an;
        ((float2*)S.destination_out)[fr] = dn;
        S.mask_out[fr] = m;
    }
    return SlotAfter{!gone, dn};
}

// The routed frame's arguments (piml_scenario_step_nav): the floor field, its any-angle table (read with kSight only) and
// the steering targets it writes, (members, capacity, 2); member_view's layout.
struct SteerArgs {
    piml_nav_grid NV;
    const int* parent;
    float2* steer;
};

// the steering target of an agent at p bound for dest through `gate`: one metre down the field in the lookup's branches 1, 2
// and 3, the destination in branch 0 (scenario_mlapm_body's kNav formula).  One thread per agent here, one wave there: the
// lookup has no cross-lane operation.
template <bool kSight>
__device__ __forceinline__ float2 steer_target(const SteerArgs& A, int gate, float2 p, float2 dest) {
    const NavDir nd = nav_direction<kSight>(A.NV, gate, p, dest, A.parent);
    return make_float2(nd.branch ? __fadd_rn(p.x, nd.e.x) : dest.x, nd.branch ? __fadd_rn(p.y, nd.e.y) : dest.y);
}

// steps 1-3 and the record of slot i (member view S, the network's a_next); entries: GC's entry points (LDS or global).
// kNav: then slot i's steering target, from what step 3 left -- the lookup for a slot that stays present (its flag is < D),
// NaN for one that retires now or was retired earlier.  kNav == false reads neither the field nor steer.
template <bool kGC, bool kNav = false, bool kSight = false>
__device__ __forceinline__ void agent_step(const piml_scenario& S, const piml_scenario_rules& R, const float2* a_next,
                                           const float2* entries, int i, long long t, const SteerArgs* A = nullptr) {
    if (S.mask[i] == 0.f) {                                  // retired for good
        record_retired(S, i, t);
        if constexpr (kNav) A->steer[i] = make_float2(qnan(), qnan());
        return;
    }
    const float dt = S.dt;
    const float2 p = ((const float2*)S.position)[i], v = ((const float2*)S.velocity)[i];
    const float2 a = ((const float2*)S.acceleration)[i], d = ((const float2*)S.destination)[i];
    const float2 an = a_next[i];
    const float2 vn = make_float2(__fadd_rn(v.x, __fmul_rn(a.x, dt)), __fadd_rn(v.y, __fmul_rn(a.y, dt)));
    const float2 pn = make_float2(__fadd_rn(p.x, __fmul_rn(v.x, dt)), __fadd_rn(p.y, __fmul_rn(v.y, dt)));
    agent_history(S, i, vn, an);
    const int f = S.flag[i];
    bool gone = false;
    int fn;
    if (kGC) {
        const float2* ent = entries + (size_t)S.exit_idx[(size_t)f * S.capacity + i] * S.P;
        float m2 = INFINITY;                                 // min over the exit's points of the squared distance
#pragma unroll 10
        for (int q = 0; q < S.P; ++q) m2 = fminf(m2, sq2(__fsub_rn(pn.x, ent[q].x), __fsub_rn(pn.y, ent[q].y)));
        fn = gc_arrive(S, f, pn, d, m2);
    } else {
        fn = rules_arrive(S, R, f, pn, d, gone);
    }
    const SlotAfter after = agent_retire_record(S, i, t, fn, gone, pn, vn, an);   // 3. retire (data.py:236-247)
    if constexpr (kNav) {
        float2 target = make_float2(qnan(), qnan());
        if (after.present) target = steer_target<kSight>(*A, S.exit_idx[(size_t)fn * S.capacity + i], pn, after.dest);
        A->steer[i] = target;
    }
}

// one wave: agent of ordinal `ord` (< capacity) appears in frame `f`
__device__ void spawn_agent(const piml_scenario& S, const float2* ent, long long ord, long long f) {
    const int lane = lane_id();
    const unsigned k0 = (unsigned)S.seed, k1 = (unsigned)(S.seed >> 32);
    const unsigned c0 = (unsigned)ord, c1 = (unsigned)((unsigned long long)ord >> 32);
    const PhiloxOut w1 = philox4x32_10(c0, c1, 0u, kScenarioStream | 1u, k0, k1);
    const PhiloxOut w2 = philox4x32_10(c0, c1, 0u, kScenarioStream | 2u, k0, k1);
    const unsigned oe = pick(w1.x, (unsigned)S.E);
    unsigned de = pick(w1.y, (unsigned)S.E - 1u);
    de += de >= oe;
    const unsigned oi = pick(w1.z, (unsigned)S.P), di = pick(w1.w, (unsigned)S.P);
    const float2 eo = ent[(size_t)oe * S.P + oi], ed = ent[(size_t)de * S.P + di];
    const float2 o = make_float2(__fadd_rn(eo.x, __fmul_rn(unit24(w2.x), S.spawn_offset)),
                                 __fadd_rn(eo.y, __fmul_rn(unit24(w2.y), S.spawn_offset)));
    const float2 d = make_float2(__fadd_rn(ed.x, __fmul_rn(unit24(w2.z), S.spawn_offset)),
                                 __fadd_rn(ed.y, __fmul_rn(unit24(w2.w), S.spawn_offset)));
    int iters;
    const float2 r = route_wave(o, d, (const float2*)S.route_polyline, S.R, S.route_max_iters, S.route_clearance, &iters);
    float v0 = S.speed_mean;
    if (!S.uniform_speed) {
        const PhiloxOut w3 = philox4x32_10(c0, c1, 0u, kScenarioStream | 3u, k0, k1);
        const double u1 = (double)((w3.x >> 8) + 1u) * 5.9604644775390625e-8, u2 = (double)(w3.y >> 8) * 5.9604644775390625e-8;
        const float z = (float)(sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2));
        v0 = __fadd_rn(S.speed_mean, __fmul_rn(S.speed_std, z));
        if (v0 < S.speed_min) v0 = S.speed_min;
    }
    // waypoints (r, d, NaN ...) and the exit entry of each, once
    const size_t cap = (size_t)S.capacity, i = (size_t)ord;
    for (int q = 0; q < S.D; ++q) {
        const float2 wq = q == 0 ? r : (q == 1 ? d : make_float2(qnan(), qnan()));
        const int ex = q < 2 ? nearest_entry_wave(wq, ent, S.E, S.P) : 0;
        if (lane == 0) {
            ((float2*)S.waypoints)[q * cap + i] = wq;
            S.exit_idx[q * cap + i] = ex;
        }
    }
    if (lane == 0) {
        ((float2*)S.position)[i] = o;
        ((float2*)S.velocity)[i] = make_float2(0.f, 0.f);
        ((float2*)S.acceleration)[i] = make_float2(0.f, 0.f);
        ((float2*)S.destination)[i] = r;
        S.desired_speed[i] = v0;
        S.flag[i] = 0;
        S.mask[i] = 1.f;
        if (S.spawn_iters) S.spawn_iters[i] = iters;
        if (f < S.T) {
            const size_t fr = (size_t)f * cap + i;
            ((float2*)S.position_out)[fr] = o;
            ((float2*)S.velocity_out)[fr] = make_float2(0.f, 0.f);
            ((float2*)S.acceleration_out)[fr] = make_float2(0.f, 0.f);
            ((float2*)S.destination_out)[fr] = r;
            S.mask_out[fr] = 1.f;
        }
    }
    for (int q = lane; q < S.hist_width; q += 64) S.hist_velocity[i * S.hist_width + q] = 0.f;
    for (int q = 2 + lane; q < S.F; q += 64) S.self_features[i * S.F + q] = q == S.F - 1 ? v0 : 0.f;
}

__global__ __launch_bounds__(256) void scenario_route_kernel(const float2* __restrict__ o, const float2* __restrict__ d, int n,
                                                             const float2* __restrict__ poly, int R, int max_iters, float clearance,
                                                             float2* __restrict__ out, int* __restrict__ iters) {
    const int j = (int)blockIdx.x * (int)(blockDim.x >> 6) + (int)(threadIdx.x >> 6);
    if (j >= n) return;
    int it;
    const float2 r = route_wave(o[j], d[j], poly, R, max_iters, clearance, &it);
    if (lane_id() == 0) {
        out[j] = r;
        iters[j] = it;
    }
}


// ---- scene rules (piml_scenario_rules): the synthetic scenes' spawn laws ----

// 2 u - 1 of torch's (2 * torch.rand(n) - 1)
__device__ __forceinline__ float jitter(unsigned w) { return __fsub_rn(__fmul_rn(2.f, unit24(w)), 1.f); }

// what a scene rule's spawn writes, one wave: slot `ord`'s state (flag 0, mask 1, a = 0, destination = waypoint 0), its
// waypoints way(q), q < D, the record of frame f, and the history / self_features row -- the spawn frame's velocity in the
// newest slot, older slots 0 (make_dataset on add_pedestrians' zero fill)
template <class Way>
__device__ __forceinline__ void rules_spawn_write(const piml_scenario& S, long long ord, long long f, float2 o, float2 vel,
                                                  float v0, Way way) {
    const int lane = lane_id();
    const size_t cap = (size_t)S.capacity, i = (size_t)ord;
    for (int q = lane; q < S.D; q += 64) ((float2*)S.waypoints)[q * cap + i] = way(q);
    if (lane == 0) {
        const float2 d0 = way(0);
        ((float2*)S.position)[i] = o;
        ((float2*)S.velocity)[i] = vel;
        ((float2*)S.acceleration)[i] = make_float2(0.f, 0.f);
        ((float2*)S.destination)[i] = d0;
        S.desired_speed[i] = v0;
        S.flag[i] = 0;
        S.mask[i] = 1.f;
        if (S.spawn_iters) S.spawn_iters[i] = 0;
        if (f < S.T) {
            const size_t fr = (size_t)f * cap + i;
            ((float2*)S.position_out)[fr] = o;
            ((float2*)S.velocity_out)[fr] = vel;
            ((float2*)S.acceleration_out)[fr] = make_float2(0.f, 0.f);
            ((float2*)S.destination_out)[fr] = d0;
            S.mask_out[fr] = 1.f;
        }
    }
    const int hw = S.hist_width;
    for (int q = lane; q < hw; q += 64) S.hist_velocity[i * hw + q] = q == hw - 2 ? vel.x : (q == hw - 1 ? vel.y : 0.f);
    for (int q = 2 + lane; q < S.F; q += 64)
        S.self_features[i * S.F + q] = q == S.F - 1 ? v0 : (q == hw ? vel.x : (q == hw + 1 ? vel.y : 0.f));
}

// one wave: agent of ordinal `ord` (< capacity) of spawn stream `group` (0 / 1) appears in frame `f`
__device__ void rules_spawn_agent(const piml_scenario& S, const piml_scenario_rules& R, long long ord, int group, long long f) {
    const int lane = lane_id();
    const unsigned k0 = (unsigned)S.seed, k1 = (unsigned)(S.seed >> 32);
    const unsigned c0 = (unsigned)ord, c1 = (unsigned)((unsigned long long)ord >> 32);
    const float L = R.length, W = R.width;
    float2 o, d0, d1 = make_float2(qnan(), qnan()), head = make_float2(0.f, 0.f);
    if (R.spawn_law == PIML_SPAWN_SQUARE) {
        const int cells = R.grid * R.grid, c = (int)(ord % cells), g = (int)(ord / cells);
        const unsigned mine = philox4x32_10((unsigned)c, 0u, 0u, kRulesStream | 3u, k0, k1).x;
        int below = 0;
        for (int q = lane; q < cells; q += 64) {
            const unsigned other = philox4x32_10((unsigned)q, 0u, 0u, kRulesStream | 3u, k0, k1).x;
            below += other < mine || (other == mine && q < c);
        }
        const int s = wave_sum(below);                       // randperm(grid^2)[c]
        const float gx = R.square_grid[c / R.grid], gy = R.square_grid[c % R.grid];
        const float hx = R.square_grid[s / R.grid], hy = R.square_grid[s % R.grid];
        if (g == 0)      { o = make_float2(__fsub_rn(gx, L), gy); d0 = make_float2(__fadd_rn(hx, L), hy); }
        else if (g == 1) { o = make_float2(__fadd_rn(gx, L), gy); d0 = make_float2(__fsub_rn(hx, L), hy); }
        else if (g == 2) { o = make_float2(gx, __fsub_rn(gy, L)); d0 = make_float2(hx, __fadd_rn(hy, L)); }
        else             { o = make_float2(gx, __fadd_rn(gy, L)); d0 = make_float2(hx, __fsub_rn(hy, L)); }
    } else {
        const PhiloxOut w = philox4x32_10(c0, c1, 0u, kRulesStream | 1u, k0, k1);
        if (R.spawn_law == PIML_SPAWN_CROSSWALK) {
            const float sx = (w.x >> 31) ? 1.f : -1.f, sy = (w.y >> 31) ? 1.f : -1.f;
            o = make_float2(sx * __fadd_rn(0.5f * L, __fmul_rn(3.f, unit24(w.z))), 0.5f * W * sy);
            d0 = make_float2(-sx * (0.5f * L), __fadd_rn(-0.5f * W, (w.w >> 31) ? W : 0.f));
            d1 = make_float2(d0.x, __fmul_rn(d0.y, 3.f));
            head = make_float2(0.f, -sy);
        } else if (R.spawn_law == PIML_SPAWN_UNIT2) {
            const bool left = unit24(w.x) < R.side_ratio, rtl = unit24(w.y) < R.direction_ratio;
            float y = __fmul_rn(0.5f * W, unit24(w.z));
            if (left) y = __fadd_rn(y, 0.5f * W);
            if (rtl) y = __fsub_rn(W, y);
            o = make_float2(rtl ? L : 0.f, y);
            d0 = make_float2(rtl ? 0.f : L, __fadd_rn(y, jitter(w.w)));
            head = make_float2(rtl ? -1.f : 1.f, 0.f);
        } else if (R.spawn_law == PIML_SPAWN_UNIT3 && group == 1) {
            const float x = __fmul_rn(L, unit24(w.x));
            o = make_float2(x, 0.f);
            d0 = make_float2(__fadd_rn(x, jitter(w.y)), W);
            head = make_float2(0.f, 1.f);
        } else {                                             // UNIT1, UNIT3's first stream
            const float y = __fmul_rn(W, unit24(w.x));
            o = make_float2(0.f, y);
            d0 = make_float2(L, __fadd_rn(y, jitter(w.y)));
            head = make_float2(1.f, 0.f);
        }
    }
    float v0 = S.speed_mean;
    if (!S.uniform_speed) {
        const PhiloxOut w2 = philox4x32_10(c0, c1, 0u, kRulesStream | 2u, k0, k1);
        const double u1 = (double)((w2.x >> 8) + 1u) * 5.9604644775390625e-8, u2 = (double)(w2.y >> 8) * 5.9604644775390625e-8;
        const float z = (float)(sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2));
        v0 = __fadd_rn(S.speed_mean, __fmul_rn(S.speed_std, z));
        if (R.speed_clamp && v0 < S.speed_min) v0 = S.speed_min;
    }
    // (a zero heading component stays +0, as torch.zeros_like, also for the crosswalk's v0 <= 0)
    const float2 vel = R.initial_velocity ? make_float2(head.x != 0.f ? head.x * v0 : 0.f, head.y != 0.f ? head.y * v0 : 0.f)
                                          : make_float2(0.f, 0.f);
    rules_spawn_write(S, ord, f, o, vel, v0,
                      [&](int q) { return q == 0 ? d0 : (q == 1 ? d1 : make_float2(qnan(), qnan())); });
}

// one wave: agent of ordinal `ord` (< capacity) of the clip law appears in frame `f`: row `ord` of the track table in the
// init launch, otherwise an arrival row drawn from stream kClipStream (the file header's word layout)
__device__ void clip_spawn_agent(const piml_scenario& S, const piml_scenario_rules& R, int init, long long ord, long long f) {
    size_t row = (size_t)ord;
    float2 off = make_float2(0.f, 0.f);
    const bool moved = !init && S.spawn_offset != 0.f;       // (x + 0 would turn a -0 coordinate into +0)
    if (!init) {
        const PhiloxOut w = philox4x32_10((unsigned)ord, (unsigned)((unsigned long long)ord >> 32), 0u, kClipStream | 1u,
                                          (unsigned)S.seed, (unsigned)(S.seed >> 32));
        const unsigned long long Ka = (unsigned long long)(S.E - S.n_initial);
        row = (size_t)S.n_initial + (size_t)(((unsigned long long)(w.x >> 8) * Ka) >> 24);
        off = make_float2(__fmul_rn(S.spawn_offset, jitter(w.y)), __fmul_rn(S.spawn_offset, jitter(w.z)));
    }
    const float2* r = (const float2*)S.entries + row * (size_t)S.P;
    float2 o = r[0];
    if (moved) o = make_float2(__fadd_rn(o.x, off.x), __fadd_rn(o.y, off.y));
    const float2 vel = R.initial_velocity ? r[1] : make_float2(0.f, 0.f);
    rules_spawn_write(S, ord, f, o, vel, r[2].x, [&](int q) { return r[3 + q]; });
}

// ---- the grouped clip law (PIML_SPAWN_CLIP_GROUPS): arrival units of the track table (the file header's word layout) ----

struct GroupArgs {
    const int* row_unit;                                     // (E, 2) per table row: index inside its unit, the unit's size
    const int* unit_rows;                                    // (n_units) first row of each arrival unit
    int n_units;
    int *group_first, *group_size;                           // (members, capacity); member_view's layout
    piml_group_law law;                                      // the group term, by value ...
    const piml_group_law* law_table;                         // ... or row blockIdx.y of this table when not NULL
    int term;                                                // 0: no group term (the units still arrive together)
};

__device__ __forceinline__ void group_view(GroupArgs& G, int capacity, int m) {
    G.group_first += (size_t)m * (size_t)capacity;
    G.group_size += (size_t)m * (size_t)capacity;
}

// one wave: table row `row` appears in slot `slot` (< capacity) in frame f, moved by `off` when `moved`
__device__ void group_spawn_member(const piml_scenario& S, const piml_scenario_rules& R, size_t row, long long slot, long long f,
                                   bool moved, float2 off) {
    const float2* r = (const float2*)S.entries + row * (size_t)S.P;
    float2 o = r[0];
    if (moved) o = make_float2(__fadd_rn(o.x, off.x), __fadd_rn(o.y, off.y));   // (x + 0 would turn a -0 coordinate into +0)
    const float2 vel = R.initial_velocity ? r[1] : make_float2(0.f, 0.f);
    rules_spawn_write(S, slot, f, o, vel, r[2].x, [&](int q) { return r[3 + q]; });
}

struct GroupUnit {
    int first, size;                                         // table rows first .. first + size - 1
    unsigned w1, w2;                                         // the unit's offset words
};

// unit j of frame f.  first and size come from device tables: they are clamped to the table (a corrupt table spawns the
// wrong rows, it never reads outside `entries` or writes more than kGroupMaxSize slots)
__device__ __forceinline__ GroupUnit group_unit_draw(const piml_scenario& S, const GroupArgs& G, long long f, int j) {
    const PhiloxOut w = philox4x32_10((unsigned)f, (unsigned)((unsigned long long)f >> 32), (unsigned)j, kGroupStream | 1u,
                                      (unsigned)S.seed, (unsigned)(S.seed >> 32));
    const int u = (int)(((unsigned long long)(w.x >> 8) * (unsigned long long)G.n_units) >> 24);
    GroupUnit un;
    un.first = min(max(G.unit_rows[u], 0), S.E - 1);
    un.size = min(max(G.row_unit[2 * (size_t)un.first + 1], 1), min(kGroupMaxSize, S.E - un.first));
    un.w1 = w.y;
    un.w2 = w.z;
    return un;
}

// spawn block b of the grouped law: unit b of frame f, one wave per member; block 0's first thread does the bookkeeping
__device__ __forceinline__ void group_spawn_block(const piml_scenario& S, const piml_scenario_rules& R, const GroupArgs& G,
                                                  const uint32_t* thr, long long n, long long f, int b) {
    const PhiloxOut w = philox4x32_10((unsigned)f, (unsigned)((unsigned long long)f >> 32), 0u, kRulesStream, (unsigned)S.seed,
                                      (unsigned)(S.seed >> 32));
    const int k = threshold_count(w.x >> 8, thr, S.spawn_cap);
    if (b == 0 && threadIdx.x == 0) {
        long long total = 0;
        for (int j = 0; j < k; ++j) total += group_unit_draw(S, G, f, j).size;
        S.spawned[f & 1] = n + total;
        *S.dropped = n + total > S.capacity ? n + total - S.capacity : 0;
        if (S.spawn_out && f < S.T) S.spawn_out[f] = (int)total;
    }
    const int q = (int)(threadIdx.x >> 6);
    if (b >= k) return;
    long long base = n;
    GroupUnit un = group_unit_draw(S, G, f, 0);
    for (int j = 0; j < b; ++j) {
        base += un.size;
        un = group_unit_draw(S, G, f, j + 1);
    }
    const long long slot = base + q;
    if (q >= un.size || slot >= S.capacity) return;          // members past the capacity are dropped, never written
    const float2 off = make_float2(__fmul_rn(S.spawn_offset, jitter(un.w1)), __fmul_rn(S.spawn_offset, jitter(un.w2)));
    group_spawn_member(S, R, (size_t)(un.first + q), slot, f, S.spawn_offset != 0.f, off);
    if (lane_id() == 0) {
        G.group_first[slot] = (int)base;
        G.group_size[slot] = un.size;
    }
}

// ---- the frame ----

// a spawn block (b = blockIdx.x - agent_blocks) of member view S: the spawn count of frame f -- init: n_initial; GC: k of
// stream 0x5CE0; a scene rule (the clip law too): k1 + k2 of stream 0x5CE1 --, its bookkeeping by one thread of block 0,
// then one wave per new agent of ordinal n + j.  thr / R are the kernel arguments' (an indexed read of a local copy's table
// would put the whole descriptor in scratch); ent: GC's entry points (LDS or global).
// kNav (GC only): lane 0 of the new agent's wave then writes its steering target from what it has just written itself --
// the origin, exit_idx[0] and the first waypoint.  kNav == false reads neither the field nor steer.
template <bool kNav = false, bool kSight = false>
__device__ __forceinline__ void spawn_block(bool gc, const piml_scenario& S, const piml_scenario_rules& R, const uint32_t* thr,
                                            const float2* ent, int init, long long n, long long f, int b,
                                            const SteerArgs* A = nullptr) {
    int k1 = S.n_initial, k2 = 0;
    if (!init) {
        const PhiloxOut w = philox4x32_10((unsigned)f, (unsigned)((unsigned long long)f >> 32), 0u,
                                          gc ? kScenarioStream : kRulesStream, (unsigned)S.seed, (unsigned)(S.seed >> 32));
        k1 = threshold_count(w.x >> 8, thr, S.spawn_cap);
        if (!gc) k2 = threshold_count(w.y >> 8, R.poisson_thresholds2, R.spawn_cap2);
    }
    const int k = k1 + k2;
    if (b == 0 && threadIdx.x == 0) {
        S.spawned[f & 1] = n + k;
        *S.dropped = n + k > S.capacity ? n + k - S.capacity : 0;
        if (S.spawn_out && f < S.T) S.spawn_out[f] = k;
    }
    const int j = b * (int)(blockDim.x >> 6) + (int)(threadIdx.x >> 6);
    if (j >= k || n + j >= S.capacity) return;               // ordinals past the capacity are dropped, never written
    if (gc) spawn_agent(S, ent, n + j, f);
    else if (R.spawn_law == PIML_SPAWN_CLIP) clip_spawn_agent(S, R, init, n + j, f);
    else rules_spawn_agent(S, R, n + j, j >= k1, f);
    if constexpr (kNav) {
        if (lane_id() == 0) {                                // the lane that wrote them (flag 0: exit_idx row 0)
            const size_t i = (size_t)(n + j);
            A->steer[i] = steer_target<kSight>(*A, S.exit_idx[i], ((const float2*)S.position)[i], ((const float2*)S.destination)[i]);
        }
    }
}

// member m's view of the descriptor (the file header's layout); member 0's pointers are the bases
__device__ __forceinline__ void member_view(piml_scenario& S, const float2*& a_next, int m) {
    const size_t mm = (size_t)m, cap = (size_t)S.capacity, T = (size_t)S.T, D = (size_t)S.D;
    S.position += mm * cap * 2;
    S.velocity += mm * cap * 2;
    S.acceleration += mm * cap * 2;
    S.destination += mm * cap * 2;
    S.hist_velocity += mm * cap * (size_t)S.hist_width;
    S.self_features += mm * cap * (size_t)S.F;
    S.desired_speed += mm * cap;
    S.mask += mm * cap;
    S.flag += mm * cap;
    S.waypoints += mm * D * cap * 2;
    if (S.exit_idx) S.exit_idx += mm * D * cap;
    if (S.spawn_iters) S.spawn_iters += mm * cap;
    S.position_out += mm * T * cap * 2;
    S.velocity_out += mm * T * cap * 2;
    S.acceleration_out += mm * T * cap * 2;
    S.destination_out += mm * T * cap * 2;
    S.mask_out += mm * T * cap;
    if (S.spawn_out) S.spawn_out += mm * T;
    S.spawned += mm * 2;
    S.dropped += mm;
    if (a_next) a_next += mm * cap;
}

// the init launch of a grouped scene: slot i < n_initial is table row i, nothing is drawn (grid: waves over n_initial, members)
__global__ __launch_bounds__(256) void scenario_groups_init_kernel(const piml_scenario S0, const piml_scenario_rules R,
                                                                   const GroupArgs G0) {
    piml_scenario S = S0;
    GroupArgs G = G0;
    const float2* no_a = nullptr;
    member_view(S, no_a, (int)blockIdx.y);
    group_view(G, S.capacity, (int)blockIdx.y);
    const long long f = *S.frame_counter;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        S.spawned[f & 1] = S.n_initial;
        *S.dropped = S.n_initial > S.capacity ? S.n_initial - S.capacity : 0;
        if (S.spawn_out && f < S.T) S.spawn_out[f] = S.n_initial;
    }
    const int i = (int)blockIdx.x * (int)(blockDim.x >> 6) + (int)(threadIdx.x >> 6);
    if (i >= S.n_initial || i >= S.capacity) return;
    group_spawn_member(S, R, (size_t)i, i, f, false, make_float2(0.f, 0.f));
    if (lane_id() == 0) {
        G.group_first[i] = i - G.row_unit[2 * (size_t)i];
        G.group_size[i] = G.row_unit[2 * (size_t)i + 1];
    }
}

struct FrameArgs {
    piml_scenario S;
    piml_scenario_rules R;                                   // a scene rule's; not read by GC's frame
    const float2* a_next;
    int init, agent_blocks;
};

// Blocks 0 .. agent_blocks-1: one thread per slot; the rest spawn (spawn_block).  seeds NULL: the single run, key S.seed.
template <bool kGC>
__global__ __launch_bounds__(256) void scenario_frame_kernel(const FrameArgs K0, const unsigned long long* __restrict__ seeds) {
    __shared__ float2 lds_entries[kScenarioLdsPoints];
    piml_scenario S = K0.S;
    const float2* a_next = K0.a_next;
    member_view(S, a_next, (int)blockIdx.y);
    if (seeds) S.seed = seeds[blockIdx.y];                   // (a select of the key in one expression cost 19 VGPRs)
    const float2* ent = (const float2*)S.entries;
    const bool lds = kGC && S.E * S.P <= kScenarioLdsPoints; // kernel-uniform: every GC block stages the entry points
    if (lds) {
        for (int q = threadIdx.x; q < S.E * S.P; q += blockDim.x) lds_entries[q] = ent[q];
        __syncthreads();
        ent = lds_entries;
    }
    const long long t = *S.frame_counter;
    const long long n = K0.init ? 0 : S.spawned[t & 1];
    const long long f = K0.init ? t : t + 1;                 // the frame the new agents appear in
    if ((int)blockIdx.x < K0.agent_blocks) {
        const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
        if (i < n && i < S.capacity) {                       // (two inlined copies: LDS reads where the points fit)
            if (lds) agent_step<kGC>(S, K0.R, a_next, lds_entries, (int)i, t);
            else agent_step<kGC>(S, K0.R, a_next, (const float2*)S.entries, (int)i, t);
        }
        return;
    }
    spawn_block(kGC, S, K0.R, K0.S.poisson_thresholds, ent, K0.init, n, f, (int)blockIdx.x - K0.agent_blocks);
}

// The frame routed by the floor field (piml_scenario_step_nav): scenario_frame_kernel<true>'s grid and steps -- GC's frame, bit
// for bit -- with kNav in agent_step and spawn_block, so every slot the launch writes also gets its steering target: one
// lookup of nav.hpp per slot that stays present, one per spawned agent.  kSight: the lookup with the any-angle table
// (nav_direction<true>, branch 3).  A kernel of its own and not a third form of the one above: handing that kernel's body its
// arguments by reference changed the instructions of the two existing kernels.
template <bool kSight>
__global__ __launch_bounds__(256) void scenario_frame_nav_kernel(const FrameArgs K0, const unsigned long long* __restrict__ seeds,
                                                                 const SteerArgs A0) {
    __shared__ float2 lds_entries[kScenarioLdsPoints];
    piml_scenario S = K0.S;
    const float2* a_next = K0.a_next;
    member_view(S, a_next, (int)blockIdx.y);
    SteerArgs A = A0;
    A.steer += (size_t)blockIdx.y * (size_t)S.capacity;      // member_view's layout
    if (seeds) S.seed = seeds[blockIdx.y];
    const float2* ent = (const float2*)S.entries;
    const bool lds = S.E * S.P <= kScenarioLdsPoints;        // kernel-uniform: every block stages the entry points
    if (lds) {
        for (int q = threadIdx.x; q < S.E * S.P; q += blockDim.x) lds_entries[q] = ent[q];
        __syncthreads();
        ent = lds_entries;
    }
    const long long t = *S.frame_counter;
    const long long n = K0.init ? 0 : S.spawned[t & 1];
    const long long f = K0.init ? t : t + 1;                 // the frame the new agents appear in
    if ((int)blockIdx.x < K0.agent_blocks) {
        const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
        if (i < n && i < S.capacity) agent_step<true, true, kSight>(S, K0.R, a_next, ent, (int)i, t, &A);
        return;
    }
    spawn_block<true, kSight>(true, S, K0.R, K0.S.poisson_thresholds, ent, K0.init, n, f, (int)blockIdx.x - K0.agent_blocks, &A);
}


// ---- the MLAPM frame (piml_scenario_step_mlapm): the closed-form law of src/main_mlapm.py:18-36 drives the scene ----
//
// One launch per frame t -> t+1, every scene, grid.y = member (one member and its seed is the single run).  Blocks
// 0 .. agent_blocks-1 hold one wave per slot i (4 per block); the rest are scenario_frame_kernel's spawn blocks (spawn_block).
// Per present slot i of member m: the member's sources are read from the RECORDS of frame t (position_out[t],
// velocity_out[t]; the init launch or the previous frame wrote them), never from the state other waves overwrite in this
// launch -- mlapm_fwd_kernel<ROLL> reads traj[t-1] and writes traj[t] the same way.  Sources: slots j < n_t = min(spawned,
// capacity), retired ones NaN and skipped (skip_absent, main_mlapm's compaction); slots >= n_t are staged as NaN, the first
// min(capacity, n_t + 64) of them, which puts every present source in the same packed / scalar lane of mlapm_tile_sum as a
// piml_mlapm_step_fwd over all capacity rows, so the force is bitwise that call's.  Then
//   F = (v0 e - v) / tau - sum (mlapm.py:21-58), v' = v + F dt (:57), p' = p + v' dt (main_mlapm.py:25, explicit Euler),
//   a' = F; the history / self_features update, arrival, retirement and record of agent_step.
// GC's exit distance is spread over the wave's lanes (the minimum is exact, so the order does not matter).
// The frame index is *frame_counter + frame_offset, read and never written here: a captured graph of K frames carries
// offsets 0 .. K-1 and one counter add of K, so a frame is one launch and nothing needs a grid-wide "last block" count.
// Past the records (t + 1 >= T) a launch does nothing.  No atomics: the same parity ping-pong of the spawned count.

constexpr int kMlScWaves = 4;

struct MlapmScenarioArgs {
    piml_scenario S;
    piml_scenario_rules R;                                   // scenes other than GC
    MlapmParams P;
    int gc, agent_blocks, frame_offset;
};

// One body, two forms.  kTable == false (piml_scenario_step_mlapm): every member steps under the launch's by-value law K0.P;
// `table` is not read.  kTable == true (piml_scenario_step_mlapm_laws): member m steps under table[m], a row of derived
// constants that piml_mlapm_law_table_fill formed on the host with make_params (K0.P is not read).  The row is read on every
// launch -- a captured graph follows what the table's buffer holds at replay time -- and its index is the block's member,
// so the 56 bytes arrive by scalar loads.  The tile loop, the NaN staging of absent sources, GC's exit distance and the
// spawn blocks are the same code in both; the kTable == false code is instruction for instruction what it was before the
// table existed (the extra pointer moved one hidden-argument offset).
//
// kWalls (piml_scenario_step_mlapm_walls): the frame with the wall term of walls.hpp, F = ((v0 e - v) / tau - sum) + W, W
// from the agent's position in the state (frame t's) and added last, one float32 add per component; everything else is the
// same code.  The wall law is the by-value `wall`, or row blockIdx.y of `wall_table` when that is not NULL (read on every
// launch, as the law table).  kWalls == false is the two plain kernels below, whose names and arguments did not change.
//
// kGroups (piml_scenario_step_mlapm_groups): the frame of a grouped clip scene.  Its spawn blocks are group_spawn_block's
// (one block per arrival unit), and with GA.term the force gains the group term of groups.hpp, F = (the above) + G, added
// last, one float32 add per component.  G reads the mates' positions from the RECORDS of frame t, as the pair sum does its
// sources -- never from S.position or S.mask, which other waves overwrite in this launch.  The group law is GA.law, or row
// blockIdx.y of GA.law_table when that is not NULL.  kGroups == false does not read GA: those kernels are what they were.
//
// kNoise (piml_scenario_step_mlapm_noise): any of the forms above with the fluctuation term of noise.hpp, F = (the above) +
// eta', added last, one float32 add per component.  Lane 0 of the slot's wave draws z for (seed, t, i), steps eta = NA.state[m
// capacity + i] and writes it back -- before the pair sum, where few values are live; it depends on nothing the sum makes --
// and the wave takes eta' from lane 0 when it adds.  The law is NA.law, or row blockIdx.y of NA.law_table when that is not
// NULL (amp is read again at the add: a flag kept across the tile loop cost the one scalar register that gave a kernel a
// stack frame); amp == 0 skips the draw, the state and the add.  kNoise == false does not read NA: the kernels above compile
// to the instructions they had.
//
// kNav (piml_scenario_step_mlapm_nav): the agent steers by the floor field of nav.hpp.  n = nav_direction(NV, the gate of the
// slot's current waypoint, p, destination); in its branches 1 and 2 the steering TARGET is the point one metre down the
// field, fl(p + n.e) per component, and e is the frame's own line for that target in place of the destination -- so the frame
// is bitwise the frame without the field run on a state whose destination was overwritten by p + n.e, and e is n.e to within
// ulp(p).  In branch 0 the target is the destination: the straight line, bit for bit.  Everything else -- the force, the terms
// above, integration, arrival against S.destination -- is the same code.  kNav == false does not read NV: the kernels above
// compile to the instructions they had.
//
// kSight (piml_scenario_step_mlapm_sight, with kNav): the lookup with its sight branch, nav_direction<true>(..., SV.parent): in
// branch 3 the target is fl(p + n.e) as in branches 1 and 2.  One more load per agent; kSight == false does not read SV.
template <bool kTable, bool kWalls, bool kGroups, bool kNoise = false, bool kNav = false, bool kSight = false>
__device__ __forceinline__ void scenario_mlapm_body(const MlapmScenarioArgs& K0, const unsigned long long* __restrict__ seeds,
                                                    const MlapmParams* __restrict__ table, const WallArgs& WG,
                                                    const piml_wall_law& wall, const piml_wall_law* __restrict__ wall_table,
                                                    const GroupArgs& GA, const piml_noise_args& NA = piml_noise_args{},
                                                    const piml_nav_grid& NV = piml_nav_grid{},
                                                    const piml_nav_sight& SV = piml_nav_sight{}) {
    __shared__ float4 tile[kMlTile];                         // agent blocks: the sources (px, py, vx, vy); spawn blocks: entries
    __shared__ unsigned short ucy_ring[kMlScWaves][256];
    static_assert(kScenarioLdsPoints * sizeof(float2) <= sizeof(tile), "the entry points fit the source tile");
    piml_scenario S = K0.S;
    const float2* no_a = nullptr;
    member_view(S, no_a, (int)blockIdx.y);
    S.seed = seeds[blockIdx.y];
    MlapmParams row;
    if (kTable) row = table[blockIdx.y];                     // block-uniform index: scalar loads
    const MlapmParams& P = kTable ? row : K0.P;
    const long long t = *S.frame_counter + K0.frame_offset;
    if (t + 1 >= S.T) return;                                // past the records: nothing to do
    const long long n = S.spawned[t & 1];
    const int cap = S.capacity;
    if ((int)blockIdx.x < K0.agent_blocks) {
        const int n_t = (int)min(n, (long long)cap);
        if ((int)blockIdx.x * kMlScWaves >= n_t) return;     // (block-uniform) no slot of this block holds an agent yet
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const int i = (int)blockIdx.x * kMlScWaves + wave;
        const bool live = i < n_t && S.mask[i] != 0.f;       // wave-uniform
        float2 pi = make_float2(0.f, 0.f), vi = pi, di = pi;
        if (live) { pi = ((const float2*)S.position)[i]; vi = ((const float2*)S.velocity)[i]; di = ((const float2*)S.destination)[i]; }
        float2 ti = di;                                      // what the agent steers to
        if constexpr (kNav) {
            if (live) {                                      // wave-uniform; the gate is range-checked by the lookup
                const int gate = S.exit_idx[(size_t)S.flag[i] * cap + i];
                const NavDir nd = nav_direction<kSight>(NV, gate, pi, di, SV.parent);
                const float tx = nd.branch ? __fadd_rn(pi.x, nd.e.x) : di.x, ty = nd.branch ? __fadd_rn(pi.y, nd.e.y) : di.y;
                ti = make_float2(tx, ty);
            }
        }
        // the fluctuation of this step, drawn before the pair sum while few values are live (it depends on (seed, t, i) and
        // the slot's own state only); added to the force last, below
        float2 eta = make_float2(0.f, 0.f);
        if constexpr (kNoise) {
            const float rho = NA.law_table ? NA.law_table[blockIdx.y].rho : NA.law.rho;       // block-uniform index
            const float amp = NA.law_table ? NA.law_table[blockIdx.y].amp : NA.law.amp;
            if (amp != 0.f && live && lane == 0) {
                float2* st = (float2*)NA.state + ((size_t)blockIdx.y * (size_t)cap + (size_t)i);   // member_view's layout
                eta = noise_step(*st, rho, amp, noise_draw(S.seed, t, (unsigned)i));
                *st = eta;
            }
        }
        float ex = ti.x - pi.x, ey = ti.y - pi.y;
        const float en = fmaxf(norm2(ex, ey), 1e-12f);      // mlapm.py:21
        ex /= en; ey /= en;
        const float2* pt = (const float2*)S.position_out + (size_t)t * cap;
        const float2* vt = (const float2*)S.velocity_out + (size_t)t * cap;
        const int ns = min(cap, n_t + 64);
        float sx = 0.f, sy = 0.f;
        v2f acc2x = {0.f, 0.f}, acc2y = {0.f, 0.f};
        for (int base = 0; base < ns; base += kMlTile) {
            const int tn = min(kMlTile, ns - base);
            __syncthreads();
            for (int q = threadIdx.x; q < tn; q += kMlScWaves * 64) {
                const int j = base + q;
                float4 s = make_float4(qnan(), qnan(), qnan(), qnan());
                if (j < n_t) {
                    const float2 a = pt[j], b = vt[j];
                    s = make_float4(a.x, a.y, b.x, b.y);
                }
                tile[q] = s;
            }
            __syncthreads();
            if (!live) continue;
            mlapm_tile_sum(P, tile, tn, lane, ucy_ring[uniform(wave)], pi, vi, ex, ey, sx, sy, acc2x, acc2y);
        }
        if (i >= n_t) return;
        if (!live) {                                         // retired for good
            if (lane == 0) record_retired(S, i, t);
            return;
        }
        sx += acc2x.x + acc2x.y; sy += acc2y.x + acc2y.y;
        sx = wave_sum(sx); sy = wave_sum(sy);
        const float dt = S.dt;
        const float v0i = S.desired_speed[i];
        float fx = (v0i * ex - vi.x) / P.tau - sx;           // :22, :29/:40/:53
        float fy = (v0i * ey - vi.y) / P.tau - sy;
        if constexpr (kWalls) {
            const piml_wall_law w = wall_table ? wall_table[blockIdx.y] : wall;   // block-uniform index: scalar loads
            const WallHit h = wall_force_wave(WG, w.A, w.B, make_float2(uniform(pi.x), uniform(pi.y)), lane);
            fx += h.force.x; fy += h.force.y;
        }
        if constexpr (kGroups) {
            if (GA.term) {
                const piml_group_law gl = GA.law_table ? GA.law_table[blockIdx.y] : GA.law;   // block-uniform index
                const size_t mo = (size_t)blockIdx.y * (size_t)cap + (size_t)i;               // member_view's layout
                const float2 g = group_force_row(pt, n_t, i, GA.group_first[mo], GA.group_size[mo], gl.A, gl.dist);
                fx = __fadd_rn(fx, g.x); fy = __fadd_rn(fy, g.y);
            }
        }
        if constexpr (kNoise) {
            const float amp = NA.law_table ? NA.law_table[blockIdx.y].amp : NA.law.amp;       // (read again: nothing is kept)
            if (amp != 0.f) { fx = __fadd_rn(fx, __shfl(eta.x, 0, 64)); fy = __fadd_rn(fy, __shfl(eta.y, 0, 64)); }
        }
        const float2 vn = make_float2(vi.x + fx * dt, vi.y + fy * dt);          // :57
        const float2 pn = make_float2(pi.x + vn.x * dt, pi.y + vn.y * dt);      // main_mlapm.py:25
        const float2 an = make_float2(fx, fy);
        const int f = S.flag[i];
        float m2 = INFINITY;
        if (K0.gc) {
            const float2* ent = (const float2*)S.entries + (size_t)S.exit_idx[(size_t)f * cap + i] * S.P;
            for (int q = lane; q < S.P; q += 64) m2 = fminf(m2, sq2(__fsub_rn(pn.x, ent[q].x), __fsub_rn(pn.y, ent[q].y)));
            m2 = wave_min(m2);
        }
        if (lane == 0) {
            agent_history(S, i, vn, an);
            bool gone = false;
            const int fn = K0.gc ? gc_arrive(S, f, pn, di, m2) : rules_arrive(S, K0.R, f, pn, di, gone);
            agent_retire_record(S, i, t, fn, gone, pn, vn, an);
        }
        return;
    }
    if constexpr (kGroups) {                                 // the grouped law's spawn blocks: one per arrival unit
        GroupArgs G = GA;
        group_view(G, cap, (int)blockIdx.y);
        group_spawn_block(S, K0.R, G, K0.S.poisson_thresholds, n, t + 1, (int)blockIdx.x - K0.agent_blocks);
        return;
    }
    // spawn blocks: the frame kernel's, from the same thresholds of the kernel arguments
    const float2* ent = (const float2*)S.entries;
    if (K0.gc && S.E * S.P <= kScenarioLdsPoints) {          // block-uniform, before any wave leaves
        float2* lds_entries = (float2*)tile;
        for (int q = threadIdx.x; q < S.E * S.P; q += blockDim.x) lds_entries[q] = ent[q];
        __syncthreads();
        ent = lds_entries;
    }
    spawn_block(K0.gc, S, K0.R, K0.S.poisson_thresholds, ent, 0, n, t + 1, (int)blockIdx.x - K0.agent_blocks);
}

template <bool kTable>
__global__ __launch_bounds__(kMlScWaves * 64) void scenario_mlapm_kernel(const MlapmScenarioArgs K0,
                                                                        const unsigned long long* __restrict__ seeds,
                                                                        const MlapmParams* __restrict__ table) {
    scenario_mlapm_body<kTable, false, false>(K0, seeds, table, WallArgs{}, piml_wall_law{}, nullptr, GroupArgs{});
}

template <bool kTable>
__global__ __launch_bounds__(kMlScWaves * 64) void scenario_mlapm_walls_kernel(const MlapmScenarioArgs K0,
                                                                              const unsigned long long* __restrict__ seeds,
                                                                              const MlapmParams* __restrict__ table,
                                                                              const WallArgs WG, const piml_wall_law wall,
                                                                              const piml_wall_law* __restrict__ wall_table) {
    scenario_mlapm_body<kTable, true, false>(K0, seeds, table, WG, wall, wall_table, GroupArgs{});
}

static_assert(kMlScWaves == kGroupMaxSize, "a spawn block of the grouped law holds one wave per member of a unit");

template <bool kTable, bool kWalls>
__global__ __launch_bounds__(kMlScWaves * 64) void scenario_mlapm_groups_kernel(const MlapmScenarioArgs K0,
                                                                               const unsigned long long* __restrict__ seeds,
                                                                               const MlapmParams* __restrict__ table,
                                                                               const WallArgs WG, const piml_wall_law wall,
                                                                               const piml_wall_law* __restrict__ wall_table,
                                                                               const GroupArgs GA) {
    scenario_mlapm_body<kTable, kWalls, true>(K0, seeds, table, WG, wall, wall_table, GA);
}

// every form of the frame with the fluctuation term; kGroups == false does not read GA, kWalls == false neither WG nor the laws
template <bool kTable, bool kWalls, bool kGroups>
__global__ __launch_bounds__(kMlScWaves * 64) void scenario_mlapm_noise_kernel(const MlapmScenarioArgs K0,
                                                                              const unsigned long long* __restrict__ seeds,
                                                                              const MlapmParams* __restrict__ table,
                                                                              const WallArgs WG, const piml_wall_law wall,
                                                                              const piml_wall_law* __restrict__ wall_table,
                                                                              const GroupArgs GA, const piml_noise_args NA) {
    scenario_mlapm_body<kTable, kWalls, kGroups, true>(K0, seeds, table, WG, wall, wall_table, GA, NA);
}

// the frame routed by the floor field: a scene of gates without groups, the fluctuation term compiled in (amp == 0 skips it)
template <bool kTable, bool kWalls>
__global__ __launch_bounds__(kMlScWaves * 64) void scenario_mlapm_nav_kernel(const MlapmScenarioArgs K0,
                                                                            const unsigned long long* __restrict__ seeds,
                                                                            const MlapmParams* __restrict__ table,
                                                                            const WallArgs WG, const piml_wall_law wall,
                                                                            const piml_wall_law* __restrict__ wall_table,
                                                                            const piml_noise_args NA, const piml_nav_grid NV) {
    scenario_mlapm_body<kTable, kWalls, false, true, true>(K0, seeds, table, WG, wall, wall_table, GroupArgs{}, NA, NV);
}

// the frame routed by the floor field and its any-angle table (nav.hpp, branch 3)
template <bool kTable, bool kWalls>
__global__ __launch_bounds__(kMlScWaves * 64) void scenario_mlapm_sight_kernel(const MlapmScenarioArgs K0,
                                                                              const unsigned long long* __restrict__ seeds,
                                                                              const MlapmParams* __restrict__ table,
                                                                              const WallArgs WG, const piml_wall_law wall,
                                                                              const piml_wall_law* __restrict__ wall_table,
                                                                              const piml_noise_args NA, const piml_nav_grid NV,
                                                                              const piml_nav_sight SV) {
    scenario_mlapm_body<kTable, kWalls, false, true, true, true>(K0, seeds, table, WG, wall, wall_table, GroupArgs{}, NA, NV, SV);
}

// the frame routed by a floor field per member (piml_scenario_step_mlapm_navdyn; navdensity.hip solves the fields): member
// blockIdx.y looks its directions up in the planes member_stride elements further on.  The body is the nav kernel's, called
// with a copy of the grid whose u was advanced; stride 0 is the nav kernel's frame bit for bit
template <bool kTable, bool kWalls>
__global__ __launch_bounds__(kMlScWaves * 64) void scenario_mlapm_navdyn_kernel(const MlapmScenarioArgs K0,
                                                                               const unsigned long long* __restrict__ seeds,
                                                                               const MlapmParams* __restrict__ table,
                                                                               const WallArgs WG, const piml_wall_law wall,
                                                                               const piml_wall_law* __restrict__ wall_table,
                                                                               const piml_noise_args NA, const piml_nav_grid NV0,
                                                                               const long long member_stride) {
    piml_nav_grid NV = NV0;
    NV.u = NV0.u + (long long)blockIdx.y * member_stride;
    scenario_mlapm_body<kTable, kWalls, false, true, true>(K0, seeds, table, WG, wall, wall_table, GroupArgs{}, NA, NV);
}

// ---- exit choice (piml_nav_choose_exit): a routed agent re-decides which gate of its class it is bound for ----
//
// One launch in front of a frame, grid (agent blocks of 4 waves, members), one wave per slot.  It reads the frame counter t
// (+ frame_offset, as the MLAPM frame) and returns at once unless t >= 1 and (t - 1) % every == 0 -- the density update's
// schedule, on the device, so that the launch sits in front of every captured frame.  Lane g < G <= 64 holds u[g] at the
// agent's cell (nav_direction's cell formula), the candidates -- gates of the current gate's class, the agent's own origin gate
// excepted, u finite -- go through wave_argmin (least u, lowest gate on a tie), and the agent switches when its current gate
// is unreachable or fadd(u[best], margin) < u[cur].  The origin gate, the destination point index and the offset words are
// spawn_agent's draws of calls 1 and 2, recomputed from (seed, ordinal = slot): nothing new is drawn and nothing per agent is
// stored.  On a switch rows flag .. 1 of waypoints / exit_idx and the destination are rewritten by lane 0 of the slot's own
// wave, operation for operation as spawn_agent writes them (route_max_iters == 0: the waypoint is the destination); rows
// below the flag, the records and every other field are not touched.  No atomics.
struct ExitChoiceArgs {
    piml_nav_grid NV;
    long long member_stride;                                 // elements between two members' fields; 0: one field
    const int* gate_class;                                   // (G), -1: in no class
    piml_exit_choice law;                                    // margin, commit in cell units
    int* switch_count;                                       // (members, capacity) or NULL
    int frame_offset;
};

__global__ __launch_bounds__(kMlScWaves * 64) void scenario_choose_exit_kernel(const piml_scenario S0,
                                                                              const unsigned long long* __restrict__ seeds,
                                                                              const ExitChoiceArgs A) {
    piml_scenario S = S0;
    const float2* no_a = nullptr;
    member_view(S, no_a, (int)blockIdx.y);
    if (seeds) S.seed = seeds[blockIdx.y];
    const long long t = *S.frame_counter + A.frame_offset;
    if (t < 1 || (t - 1) % A.law.every != 0) return;         // (kernel-uniform) not a scheduled frame
    const long long n = S.spawned[t & 1];
    const int cap = S.capacity;
    const int lane = threadIdx.x & 63;
    const int i = (int)blockIdx.x * kMlScWaves + (int)(threadIdx.x >> 6);
    if (i >= n || i >= cap) return;                          // wave-uniform from here on
    if (S.mask[i] == 0.f) return;
    const int f = S.flag[i];
    if (f < 0 || f >= 2) return;
    const piml_nav_grid& N = A.NV;
    const int cur = S.exit_idx[(size_t)f * cap + i];
    if (cur < 0 || cur >= N.G) return;
    const int cls = A.gate_class[cur];
    if (cls < 0) return;
    const float2 p = ((const float2*)S.position)[i];
    const float fcx = floorf(__fdiv_rn(__fsub_rn(p.x, N.x0), N.cell)), fcy = floorf(__fdiv_rn(__fsub_rn(p.y, N.y0), N.cell));
    if (!(p.x == p.x && p.y == p.y && fcx >= 0.f && fcx < (float)N.gx && fcy >= 0.f && fcy < (float)N.gy)) return;
    const size_t cells = (size_t)(N.gy * N.gx), c = (size_t)((int)fcy * N.gx + (int)fcx);
    const float* __restrict__ u = N.u + (long long)blockIdx.y * A.member_stride;
    const unsigned k0 = (unsigned)S.seed, k1 = (unsigned)(S.seed >> 32);
    const PhiloxOut w1 = philox4x32_10((unsigned)i, 0u, 0u, kScenarioStream | 1u, k0, k1);
    const int oe = (int)pick(w1.x, (unsigned)S.E);
    const bool gate = lane < N.G;
    const float ug = gate ? u[(size_t)lane * cells + c] : INFINITY;
    const float ucur = __shfl(ug, cur, 64);
    const bool cand = gate && lane != oe && nav_finite(ug) && A.gate_class[gate ? lane : 0] == cls;
    float ub = cand ? ug : INFINITY;
    int best = cand ? lane : 0x7fffffff;
    wave_argmin(ub, best);
    if (best == 0x7fffffff) return;                          // no candidate
    const bool bound = nav_finite(ucur);
    if (bound && ucur <= A.law.commit) return;               // committed to the gate in front of it
    if (best == cur || !(!bound || __fadd_rn(ub, A.law.margin) < ucur)) return;
    // the switch: spawn_agent's destination for the entry `best`, from the same point index and offset words
    const PhiloxOut w2 = philox4x32_10((unsigned)i, 0u, 0u, kScenarioStream | 2u, k0, k1);
    const unsigned di = pick(w1.w, (unsigned)S.P);
    const float2* ent = (const float2*)S.entries;
    const float2 ed = ent[(size_t)best * S.P + di];
    const float2 d = make_float2(__fadd_rn(ed.x, __fmul_rn(unit24(w2.z), S.spawn_offset)),
                                 __fadd_rn(ed.y, __fmul_rn(unit24(w2.w), S.spawn_offset)));
    const int ex = nearest_entry_wave(d, ent, S.E, S.P);
    if (lane == 0) {
        for (int q = f; q < 2; ++q) {
            ((float2*)S.waypoints)[(size_t)q * cap + i] = d;
            S.exit_idx[(size_t)q * cap + i] = ex;
        }
        ((float2*)S.destination)[i] = d;
        if (A.switch_count) A.switch_count[(size_t)blockIdx.y * (size_t)cap + (size_t)i] += 1;
    }
}

}  // namespace piml

namespace {

bool thresholds_ok(const uint32_t* thr, int cap) {
    for (int j = 0; j < cap; ++j)
        if (thr[j] > (1u << 24) || (j && thr[j] < thr[j - 1])) return false;
    return true;
}

// the checks of every frame entry (include/piml_hip.h); r == NULL is GC
bool frame_args_ok(const piml_scenario& S, const piml_scenario_rules* r, const float* a_next, int init) {
    const bool gc = !r || r->spawn_law == PIML_SPAWN_GC;
    if (r && (r->spawn_law < PIML_SPAWN_GC || r->spawn_law > PIML_SPAWN_CLIP || r->arrival_rule < PIML_ARRIVE_GC ||
              r->arrival_rule > PIML_ARRIVE_XEXIT || gc != (r->arrival_rule == PIML_ARRIVE_GC)))
        return false;
    if (S.capacity < 1 || S.T < 1 || S.hist_width < 2 || S.F != S.hist_width + 5 || S.D > piml::kScenarioMaxD ||
        S.n_initial < 0 || S.n_initial > piml::kScenarioMaxInitial || S.spawn_cap < 0 || S.spawn_cap > piml::kScenarioMaxSpawn ||
        !(S.dt > 0.f) || (init != 0 && init != 1) || (!init && !a_next))
        return false;
    if (!S.position || !S.velocity || !S.acceleration || !S.destination || !S.hist_velocity || !S.self_features ||
        !S.desired_speed || !S.flag || !S.mask || !S.waypoints || !S.position_out || !S.velocity_out ||
        !S.acceleration_out || !S.destination_out || !S.mask_out || !S.frame_counter || !S.spawned || !S.dropped ||
        !thresholds_ok(S.poisson_thresholds, S.spawn_cap))
        return false;
    if (gc)
        return S.D >= 2 && S.E >= 2 && S.P >= 1 && S.R >= 2 && S.route_max_iters >= 0 &&
               S.route_max_iters <= piml::kScenarioMaxIters && S.exit_idx && S.entries && S.route_polyline;
    const piml_scenario_rules& R = *r;
    if (S.D < 1 || (R.spawn_law == PIML_SPAWN_CROSSWALK && S.D < 2) || R.spawn_cap2 < 0 ||
        R.spawn_cap2 > piml::kScenarioMaxSpawn || (R.spawn_cap2 && R.spawn_law != PIML_SPAWN_UNIT3) ||
        (R.initial_velocity != 0 && R.initial_velocity != 1) || (R.speed_clamp != 0 && R.speed_clamp != 1))
        return false;
    if (R.spawn_law == PIML_SPAWN_SQUARE && (R.grid < 1 || R.grid > piml::kRulesMaxGrid || S.n_initial != 4 * R.grid * R.grid))
        return false;
    if (R.spawn_law == PIML_SPAWN_CLIP &&                    // the track table: (E, 3 + D, 2), rows n_initial.. the arrivals
        (!S.entries || S.P != 3 + S.D || S.n_initial > S.E || (S.spawn_cap > 0 && S.E == S.n_initial) ||
         (unsigned)(S.E - S.n_initial) > piml::kClipMaxArrivals))
        return false;
    return thresholds_ok(R.poisson_thresholds2, R.spawn_cap2);
}

// >= 1: block agent_blocks writes each member's spawned count
int spawn_blocks(const piml_scenario& S, const piml_scenario_rules* r, int init) {
    const int waves = init ? S.n_initial : S.spawn_cap + (r && r->spawn_law != PIML_SPAWN_GC ? r->spawn_cap2 : 0);
    return waves > 0 ? (waves + 3) / 4 : 1;
}

// one scenario_frame_kernel launch over frame_args_ok's arguments; seeds NULL: one member, key S.seed
int launch_frame(const piml_scenario& S, const piml_scenario_rules* r, int members, const uint64_t* seeds,
                 const float* a_next, int init, void* stream) {
    piml::FrameArgs K;
    K.S = S;
    K.R = r ? *r : piml_scenario_rules{};
    K.a_next = (const float2*)a_next;
    K.init = init;
    K.agent_blocks = init ? 0 : (S.capacity + 255) / 256;
    const dim3 grid((unsigned)(K.agent_blocks + spawn_blocks(S, r, init)), (unsigned)members);
    const unsigned long long* sd = (const unsigned long long*)seeds;
    if (K.R.spawn_law == PIML_SPAWN_GC)
        hipLaunchKernelGGL(piml::scenario_frame_kernel<true>, grid, dim3(256), 0, piml::as_stream(stream), K, sd);
    else
        hipLaunchKernelGGL(piml::scenario_frame_kernel<false>, grid, dim3(256), 0, piml::as_stream(stream), K, sd);
    return hipGetLastError();
}

}  // namespace

PIML_API int piml_scenario_step(const piml_scenario* s, const float* a_next, int init, void* stream) {
    if (!s || !frame_args_ok(*s, nullptr, a_next, init)) return hipErrorInvalidValue;
    return launch_frame(*s, nullptr, 1, nullptr, a_next, init, stream);
}

PIML_API int piml_scenario_step_rules(const piml_scenario* s, const piml_scenario_rules* r, const float* a_next, int init,
                                      void* stream) {
    if (!s || !r || !frame_args_ok(*s, r, a_next, init)) return hipErrorInvalidValue;
    return launch_frame(*s, r, 1, nullptr, a_next, init, stream);
}

PIML_API int piml_scenario_step_members(const piml_scenario* s, const piml_scenario_rules* r, int members,
                                        const uint64_t* seeds, const float* a_next, int init, void* stream) {
    if (!s || !seeds || members < 1 || members > 65535 || !frame_args_ok(*s, r, a_next, init)) return hipErrorInvalidValue;
    return launch_frame(*s, r, members, seeds, a_next, init, stream);
}

PIML_API int piml_scenario_step_nav(const piml_scenario* s, const piml_scenario_rules* r, int members, const uint64_t* seeds,
                                    const float* a_next, int init, const piml_nav_grid* nav, const piml_nav_sight* sight,
                                    float* steer, void* stream) {
    if (!s || !steer || members < 1 || members > 65535 || (!seeds && members != 1) || !frame_args_ok(*s, r, a_next, init))
        return hipErrorInvalidValue;
    if (r && r->spawn_law != PIML_SPAWN_GC) return hipErrorInvalidValue;      // only GC's law has gates and exit_idx
    if (s->route_max_iters != 0) return hipErrorInvalidValue;                 // a detour point's gate is not the destination's
    if (!piml::nav_grid_ok(nav) || nav->G != s->E || (sight && !piml::nav_sight_ok(sight, nav))) return hipErrorInvalidValue;
    piml::FrameArgs K;
    K.S = *s;
    K.R = piml_scenario_rules{};
    K.a_next = (const float2*)a_next;
    K.init = init;
    K.agent_blocks = init ? 0 : (s->capacity + 255) / 256;
    const dim3 grid((unsigned)(K.agent_blocks + spawn_blocks(*s, nullptr, init)), (unsigned)members);
    const piml::SteerArgs A{*nav, sight ? sight->parent : nullptr, (float2*)steer};
    const unsigned long long* sd = (const unsigned long long*)seeds;
    if (sight)
        hipLaunchKernelGGL(piml::scenario_frame_nav_kernel<true>, grid, dim3(256), 0, piml::as_stream(stream), K, sd, A);
    else
        hipLaunchKernelGGL(piml::scenario_frame_nav_kernel<false>, grid, dim3(256), 0, piml::as_stream(stream), K, sd, A);
    return hipGetLastError();
}

// the law checks of the MLAPM frame entries (include/piml_hip.h)
static bool mlapm_law_ok(const piml_mlapm_law& L) {
    return L.variant >= 0 && L.variant <= 2 && std::isfinite(L.tau) && L.tau > 0.f && std::isfinite(L.A) &&
           std::isfinite(L.B) && std::isfinite(L.C) && std::isfinite(L.D) && std::isfinite(L.theta_deg) &&
           std::isfinite(L.radius) && L.radius > 0.f;
}

// the arguments of an MLAPM frame launch (K.P left to the caller) and its grid
static dim3 mlapm_frame_launch(piml::MlapmScenarioArgs& K, const piml_scenario& S, const piml_scenario_rules* r, int members,
                               int frame_offset) {
    K.S = S;
    K.R = r ? *r : piml_scenario_rules{};
    K.gc = K.R.spawn_law == PIML_SPAWN_GC;
    K.agent_blocks = (S.capacity + piml::kMlScWaves - 1) / piml::kMlScWaves;
    K.frame_offset = frame_offset;
    return dim3((unsigned)(K.agent_blocks + spawn_blocks(S, r, 0)), (unsigned)members);
}

PIML_API int piml_scenario_step_mlapm(const piml_scenario* s, const piml_scenario_rules* r, int members, const uint64_t* seeds,
                                      const piml_mlapm_law* law, int frame_offset, void* stream) {
    // the frame checks (init = 1 only waives a_next, which this frame does not take)
    if (!s || !seeds || !law || members < 1 || members > 65535 || frame_offset < 0 || !frame_args_ok(*s, r, nullptr, 1))
        return hipErrorInvalidValue;
    const piml_mlapm_law& L = *law;
    if (!mlapm_law_ok(L)) return hipErrorInvalidValue;
    piml::MlapmScenarioArgs K;
    const dim3 grid = mlapm_frame_launch(K, *s, r, members, frame_offset);
    K.P = piml::make_params(L.variant, L.tau, L.A, L.B, L.C, L.D, L.theta_deg, L.radius, 1);
    hipLaunchKernelGGL(piml::scenario_mlapm_kernel<false>, grid, dim3(piml::kMlScWaves * 64), 0, piml::as_stream(stream), K,
                       (const unsigned long long*)seeds, (const piml::MlapmParams*)nullptr);
    return hipGetLastError();
}

PIML_API long long piml_mlapm_law_table_bytes(int n) { return n < 0 ? -1 : (long long)n * (long long)sizeof(piml::MlapmParams); }

PIML_API int piml_mlapm_law_table_fill(const piml_mlapm_law* laws, int n, void* table_host) {
    if (n < 0 || (n > 0 && (!laws || !table_host))) return hipErrorInvalidValue;
    for (int m = 0; m < n; ++m)                              // every law before the first byte is written
        if (!mlapm_law_ok(laws[m])) return hipErrorInvalidValue;
    piml::MlapmParams* rows = (piml::MlapmParams*)table_host;
    for (int m = 0; m < n; ++m) {
        const piml_mlapm_law& L = laws[m];
        rows[m] = piml::make_params(L.variant, L.tau, L.A, L.B, L.C, L.D, L.theta_deg, L.radius, 1);
    }
    return hipSuccess;
}

PIML_API int piml_scenario_step_mlapm_laws(const piml_scenario* s, const piml_scenario_rules* r, int members,
                                           const uint64_t* seeds, const void* table_device, int frame_offset, void* stream) {
    if (!s || !seeds || !table_device || members < 1 || members > 65535 || frame_offset < 0 ||
        !frame_args_ok(*s, r, nullptr, 1))
        return hipErrorInvalidValue;
    piml::MlapmScenarioArgs K;
    const dim3 grid = mlapm_frame_launch(K, *s, r, members, frame_offset);
    K.P = piml::MlapmParams{};                               // not read: the rows are the table's
    hipLaunchKernelGGL(piml::scenario_mlapm_kernel<true>, grid, dim3(piml::kMlScWaves * 64), 0, piml::as_stream(stream), K,
                       (const unsigned long long*)seeds, (const piml::MlapmParams*)table_device);
    return hipGetLastError();
}

PIML_API int piml_scenario_step_mlapm_walls(const piml_scenario* s, const piml_scenario_rules* r, int members,
                                            const uint64_t* seeds, const piml_mlapm_law* law, const void* table_device,
                                            const piml_wall_grid* g, const piml_wall_law* wall,
                                            const piml_wall_law* wall_table_device, int frame_offset, void* stream) {
    if (!s || !seeds || members < 1 || members > 65535 || frame_offset < 0 || !frame_args_ok(*s, r, nullptr, 1))
        return hipErrorInvalidValue;
    if (!law == !table_device || !wall == !wall_table_device) return hipErrorInvalidValue;   // exactly one of each pair
    if (law && !mlapm_law_ok(*law)) return hipErrorInvalidValue;
    if (!piml::wall_grid_ok(g) || (wall && !piml::wall_law_ok(wall->A, wall->B))) return hipErrorInvalidValue;
    piml::MlapmScenarioArgs K;
    const dim3 grid = mlapm_frame_launch(K, *s, r, members, frame_offset);
    const piml::WallArgs WG = piml::wall_args(*g);
    const piml_wall_law w = wall ? *wall : piml_wall_law{};
    if (law) {
        const piml_mlapm_law& L = *law;
        K.P = piml::make_params(L.variant, L.tau, L.A, L.B, L.C, L.D, L.theta_deg, L.radius, 1);
        hipLaunchKernelGGL(piml::scenario_mlapm_walls_kernel<false>, grid, dim3(piml::kMlScWaves * 64), 0,
                           piml::as_stream(stream), K, (const unsigned long long*)seeds, (const piml::MlapmParams*)nullptr, WG,
                           w, wall_table_device);
    } else {
        K.P = piml::MlapmParams{};                           // not read: the rows are the table's
        hipLaunchKernelGGL(piml::scenario_mlapm_walls_kernel<true>, grid, dim3(piml::kMlScWaves * 64), 0,
                           piml::as_stream(stream), K, (const unsigned long long*)seeds,
                           (const piml::MlapmParams*)table_device, WG, w, wall_table_device);
    }
    return hipGetLastError();
}

PIML_API int piml_scenario_step_mlapm_groups(const piml_scenario* s, const piml_scenario_rules* r, int members,
                                             const uint64_t* seeds, const piml_mlapm_law* law, const void* law_table_device,
                                             const piml_wall_grid* wall_grid, const piml_wall_law* wall,
                                             const piml_wall_law* wall_table_device, const piml_scene_groups* g,
                                             const piml_group_law* glaw, const piml_group_law* glaw_table_device, int init,
                                             int frame_offset, void* stream) {
    if (!s || !r || !seeds || !g || members < 1 || members > 65535 || frame_offset < 0 || (init != 0 && init != 1) ||
        r->spawn_law != PIML_SPAWN_CLIP_GROUPS)
        return hipErrorInvalidValue;
    piml_scenario_rules clip = *r;                           // the frame checks of the clip law: the table is the same
    clip.spawn_law = PIML_SPAWN_CLIP;
    if (!frame_args_ok(*s, &clip, nullptr, 1)) return hipErrorInvalidValue;
    if (!g->row_unit || !g->unit_rows || !g->group_first || !g->group_size || g->n_units < 0 ||
        (g->n_units == 0 && s->spawn_cap > 0) || (unsigned)g->n_units > piml::kGroupMaxUnits)
        return hipErrorInvalidValue;
    if (glaw && glaw_table_device) return hipErrorInvalidValue;
    if (glaw && !piml::group_law_ok(glaw->A, glaw->dist)) return hipErrorInvalidValue;
    piml::GroupArgs GA;
    GA.row_unit = g->row_unit;
    GA.unit_rows = g->unit_rows;
    GA.n_units = g->n_units;
    GA.group_first = g->group_first;
    GA.group_size = g->group_size;
    GA.law = glaw ? *glaw : piml_group_law{};
    GA.law_table = glaw_table_device;
    GA.term = glaw || glaw_table_device;
    if (init) {                                              // the laws are not read
        const dim3 grid((unsigned)(s->n_initial > 0 ? (s->n_initial + 3) / 4 : 1), (unsigned)members);
        hipLaunchKernelGGL(piml::scenario_groups_init_kernel, grid, dim3(256), 0, piml::as_stream(stream), *s, *r, GA);
        return hipGetLastError();
    }
    if (!law == !law_table_device) return hipErrorInvalidValue;                               // exactly one
    if (law && !mlapm_law_ok(*law)) return hipErrorInvalidValue;
    if (wall_grid ? (!wall == !wall_table_device) : (wall || wall_table_device)) return hipErrorInvalidValue;
    if (wall_grid && (!piml::wall_grid_ok(wall_grid) || (wall && !piml::wall_law_ok(wall->A, wall->B))))
        return hipErrorInvalidValue;
    piml::MlapmScenarioArgs K;
    mlapm_frame_launch(K, *s, r, members, frame_offset);
    const dim3 grid((unsigned)(K.agent_blocks + (s->spawn_cap > 0 ? s->spawn_cap : 1)), (unsigned)members);   // a block per unit
    K.P = piml::MlapmParams{};                               // (not read with a table)
    if (law) K.P = piml::make_params(law->variant, law->tau, law->A, law->B, law->C, law->D, law->theta_deg, law->radius, 1);
    const piml::WallArgs WG = wall_grid ? piml::wall_args(*wall_grid) : piml::WallArgs{};
    const piml_wall_law w = wall ? *wall : piml_wall_law{};
    const unsigned long long* sd = (const unsigned long long*)seeds;
    const piml::MlapmParams* tb = (const piml::MlapmParams*)law_table_device;
    const dim3 block(piml::kMlScWaves * 64);
    hipStream_t st = piml::as_stream(stream);
    if (wall_grid) {
        if (law) hipLaunchKernelGGL((piml::scenario_mlapm_groups_kernel<false, true>), grid, block, 0, st, K, sd, tb, WG, w,
                                    wall_table_device, GA);
        else hipLaunchKernelGGL((piml::scenario_mlapm_groups_kernel<true, true>), grid, block, 0, st, K, sd, tb, WG, w,
                                wall_table_device, GA);
    } else {
        if (law) hipLaunchKernelGGL((piml::scenario_mlapm_groups_kernel<false, false>), grid, block, 0, st, K, sd, tb, WG, w,
                                    wall_table_device, GA);
        else hipLaunchKernelGGL((piml::scenario_mlapm_groups_kernel<true, false>), grid, block, 0, st, K, sd, tb, WG, w,
                                wall_table_device, GA);
    }
    return hipGetLastError();
}

template <bool kTable, bool kWalls, bool kGroups>
static void launch_mlapm_noise(dim3 grid, hipStream_t st, const piml::MlapmScenarioArgs& K, const unsigned long long* sd,
                               const piml::MlapmParams* tb, const piml::WallArgs& WG, const piml_wall_law& w,
                               const piml_wall_law* wt, const piml::GroupArgs& GA, const piml_noise_args& NA) {
    hipLaunchKernelGGL((piml::scenario_mlapm_noise_kernel<kTable, kWalls, kGroups>), grid, dim3(piml::kMlScWaves * 64), 0, st, K,
                       sd, tb, WG, w, wt, GA, NA);
}

PIML_API int piml_scenario_step_mlapm_noise(const piml_scenario* s, const piml_scenario_rules* r, int members,
                                            const uint64_t* seeds, const piml_mlapm_law* law, const void* law_table_device,
                                            const piml_wall_grid* wall_grid, const piml_wall_law* wall,
                                            const piml_wall_law* wall_table_device, const piml_scene_groups* g,
                                            const piml_group_law* glaw, const piml_group_law* glaw_table_device,
                                            const piml_noise_args* noise, int init, int frame_offset, void* stream) {
    if (!noise || !noise->state || (!noise->law_table && !piml::noise_law_ok(noise->law.rho, noise->law.amp)))
        return hipErrorInvalidValue;
    if (init)                                                // the grouped scene's init launch: no law, no state is read
        return g ? piml_scenario_step_mlapm_groups(s, r, members, seeds, law, law_table_device, wall_grid, wall,
                                                   wall_table_device, g, glaw, glaw_table_device, init, frame_offset, stream)
                 : (int)hipErrorInvalidValue;
    if (!s || !seeds || members < 1 || members > 65535 || frame_offset < 0) return hipErrorInvalidValue;
    piml::GroupArgs GA{};
    if (g) {                                                 // piml_scenario_step_mlapm_groups' checks
        if (!r || r->spawn_law != PIML_SPAWN_CLIP_GROUPS) return hipErrorInvalidValue;
        piml_scenario_rules clip = *r;
        clip.spawn_law = PIML_SPAWN_CLIP;
        if (!frame_args_ok(*s, &clip, nullptr, 1)) return hipErrorInvalidValue;
        if (!g->row_unit || !g->unit_rows || !g->group_first || !g->group_size || g->n_units < 0 ||
            (g->n_units == 0 && s->spawn_cap > 0) || (unsigned)g->n_units > piml::kGroupMaxUnits)
            return hipErrorInvalidValue;
        if (glaw && glaw_table_device) return hipErrorInvalidValue;
        if (glaw && !piml::group_law_ok(glaw->A, glaw->dist)) return hipErrorInvalidValue;
        GA.row_unit = g->row_unit;
        GA.unit_rows = g->unit_rows;
        GA.n_units = g->n_units;
        GA.group_first = g->group_first;
        GA.group_size = g->group_size;
        GA.law = glaw ? *glaw : piml_group_law{};
        GA.law_table = glaw_table_device;
        GA.term = glaw || glaw_table_device;
    } else if (glaw || glaw_table_device || !frame_args_ok(*s, r, nullptr, 1)) {
        return hipErrorInvalidValue;
    }
    if (!law == !law_table_device) return hipErrorInvalidValue;                               // exactly one
    if (law && !mlapm_law_ok(*law)) return hipErrorInvalidValue;
    if (wall_grid ? (!wall == !wall_table_device) : (wall || wall_table_device)) return hipErrorInvalidValue;
    if (wall_grid && (!piml::wall_grid_ok(wall_grid) || (wall && !piml::wall_law_ok(wall->A, wall->B))))
        return hipErrorInvalidValue;
    piml::MlapmScenarioArgs K;
    dim3 grid = mlapm_frame_launch(K, *s, r, members, frame_offset);
    if (g) grid = dim3((unsigned)(K.agent_blocks + (s->spawn_cap > 0 ? s->spawn_cap : 1)), (unsigned)members);   // a block per unit
    K.P = piml::MlapmParams{};                               // (not read with a table)
    if (law) K.P = piml::make_params(law->variant, law->tau, law->A, law->B, law->C, law->D, law->theta_deg, law->radius, 1);
    const piml::WallArgs WG = wall_grid ? piml::wall_args(*wall_grid) : piml::WallArgs{};
    const piml_wall_law w = wall ? *wall : piml_wall_law{};
    const unsigned long long* sd = (const unsigned long long*)seeds;
    const piml::MlapmParams* tb = (const piml::MlapmParams*)law_table_device;
    hipStream_t st = piml::as_stream(stream);
    const int form = (law ? 0 : 4) | (wall_grid ? 2 : 0) | (g ? 1 : 0);
    switch (form) {
    case 0: launch_mlapm_noise<false, false, false>(grid, st, K, sd, tb, WG, w, wall_table_device, GA, *noise); break;
    case 1: launch_mlapm_noise<false, false, true>(grid, st, K, sd, tb, WG, w, wall_table_device, GA, *noise); break;
    case 2: launch_mlapm_noise<false, true, false>(grid, st, K, sd, tb, WG, w, wall_table_device, GA, *noise); break;
    case 3: launch_mlapm_noise<false, true, true>(grid, st, K, sd, tb, WG, w, wall_table_device, GA, *noise); break;
    case 4: launch_mlapm_noise<true, false, false>(grid, st, K, sd, tb, WG, w, wall_table_device, GA, *noise); break;
    case 5: launch_mlapm_noise<true, false, true>(grid, st, K, sd, tb, WG, w, wall_table_device, GA, *noise); break;
    case 6: launch_mlapm_noise<true, true, false>(grid, st, K, sd, tb, WG, w, wall_table_device, GA, *noise); break;
    default: launch_mlapm_noise<true, true, true>(grid, st, K, sd, tb, WG, w, wall_table_device, GA, *noise); break;
    }
    return hipGetLastError();
}

// sight == NULL: the nav frame's kernels; stride >= 0: those of the frame with a field per member
template <bool kTable, bool kWalls>
static void launch_mlapm_nav(dim3 grid, hipStream_t st, const piml::MlapmScenarioArgs& K, const unsigned long long* sd,
                             const piml::MlapmParams* tb, const piml::WallArgs& WG, const piml_wall_law& w,
                             const piml_wall_law* wt, const piml_noise_args& NA, const piml_nav_grid& NV,
                             const piml_nav_sight* sight, long long stride) {
    if (stride >= 0)                                         // a field per member (sight == NULL)
        hipLaunchKernelGGL((piml::scenario_mlapm_navdyn_kernel<kTable, kWalls>), grid, dim3(piml::kMlScWaves * 64), 0, st, K, sd,
                           tb, WG, w, wt, NA, NV, stride);
    else if (sight)
        hipLaunchKernelGGL((piml::scenario_mlapm_sight_kernel<kTable, kWalls>), grid, dim3(piml::kMlScWaves * 64), 0, st, K, sd,
                           tb, WG, w, wt, NA, NV, *sight);
    else
        hipLaunchKernelGGL((piml::scenario_mlapm_nav_kernel<kTable, kWalls>), grid, dim3(piml::kMlScWaves * 64), 0, st, K, sd, tb,
                           WG, w, wt, NA, NV);
}

// piml_scenario_step_mlapm_nav (sight == NULL), piml_scenario_step_mlapm_sight and piml_scenario_step_mlapm_navdyn (stride >= 0,
// the elements between two members' fields; -1 otherwise): one set of checks, one dispatch
static int step_mlapm_nav(const piml_scenario* s, const piml_scenario_rules* r, int members, const uint64_t* seeds,
                          const piml_mlapm_law* law, const void* law_table_device, const piml_wall_grid* wall_grid,
                          const piml_wall_law* wall, const piml_wall_law* wall_table_device, const piml_nav_grid* nav,
                          const piml_nav_sight* sight, const piml_noise_args* noise, int frame_offset, void* stream,
                          long long stride = -1) {
    if (noise && (!noise->state || (!noise->law_table && !piml::noise_law_ok(noise->law.rho, noise->law.amp))))
        return hipErrorInvalidValue;
    if (!s || !seeds || members < 1 || members > 65535 || frame_offset < 0) return hipErrorInvalidValue;
    if (r && r->spawn_law != PIML_SPAWN_GC) return hipErrorInvalidValue;      // only GC's law has gates and exit_idx
    if (!frame_args_ok(*s, r, nullptr, 1)) return hipErrorInvalidValue;
    if (s->route_max_iters != 0) return hipErrorInvalidValue;                 // a detour point's gate is not the destination's
    if (!piml::nav_grid_ok(nav) || nav->G != s->E) return hipErrorInvalidValue;
    if (!law == !law_table_device) return hipErrorInvalidValue;               // exactly one
    if (law && !mlapm_law_ok(*law)) return hipErrorInvalidValue;
    if (wall_grid ? (!wall == !wall_table_device) : (wall || wall_table_device)) return hipErrorInvalidValue;
    if (wall_grid && (!piml::wall_grid_ok(wall_grid) || (wall && !piml::wall_law_ok(wall->A, wall->B))))
        return hipErrorInvalidValue;
    piml::MlapmScenarioArgs K;
    const dim3 grid = mlapm_frame_launch(K, *s, r, members, frame_offset);
    K.P = piml::MlapmParams{};                               // (not read with a table)
    if (law) K.P = piml::make_params(law->variant, law->tau, law->A, law->B, law->C, law->D, law->theta_deg, law->radius, 1);
    const piml::WallArgs WG = wall_grid ? piml::wall_args(*wall_grid) : piml::WallArgs{};
    const piml_wall_law w = wall ? *wall : piml_wall_law{};
    const piml_noise_args NA = noise ? *noise : piml_noise_args{};            // amp == 0: the term is skipped
    const unsigned long long* sd = (const unsigned long long*)seeds;
    const piml::MlapmParams* tb = (const piml::MlapmParams*)law_table_device;
    hipStream_t st = piml::as_stream(stream);
    if (law) {
        if (wall_grid) launch_mlapm_nav<false, true>(grid, st, K, sd, tb, WG, w, wall_table_device, NA, *nav, sight, stride);
        else launch_mlapm_nav<false, false>(grid, st, K, sd, tb, WG, w, wall_table_device, NA, *nav, sight, stride);
    } else {
        if (wall_grid) launch_mlapm_nav<true, true>(grid, st, K, sd, tb, WG, w, wall_table_device, NA, *nav, sight, stride);
        else launch_mlapm_nav<true, false>(grid, st, K, sd, tb, WG, w, wall_table_device, NA, *nav, sight, stride);
    }
    return hipGetLastError();
}

PIML_API int piml_scenario_step_mlapm_nav(const piml_scenario* s, const piml_scenario_rules* r, int members,
                                          const uint64_t* seeds, const piml_mlapm_law* law, const void* law_table_device,
                                          const piml_wall_grid* wall_grid, const piml_wall_law* wall,
                                          const piml_wall_law* wall_table_device, const piml_nav_grid* nav,
                                          const piml_noise_args* noise, int frame_offset, void* stream) {
    return step_mlapm_nav(s, r, members, seeds, law, law_table_device, wall_grid, wall, wall_table_device, nav, nullptr, noise,
                          frame_offset, stream);
}

PIML_API int piml_scenario_step_mlapm_sight(const piml_scenario* s, const piml_scenario_rules* r, int members,
                                            const uint64_t* seeds, const piml_mlapm_law* law, const void* law_table_device,
                                            const piml_wall_grid* wall_grid, const piml_wall_law* wall,
                                            const piml_wall_law* wall_table_device, const piml_nav_grid* nav,
                                            const piml_nav_sight* sight, const piml_noise_args* noise, int frame_offset,
                                            void* stream) {
    if (!piml::nav_grid_ok(nav) || !piml::nav_sight_ok(sight, nav)) return hipErrorInvalidValue;
    return step_mlapm_nav(s, r, members, seeds, law, law_table_device, wall_grid, wall, wall_table_device, nav, sight, noise,
                          frame_offset, stream);
}

PIML_API int piml_scenario_step_mlapm_navdyn(const piml_scenario* s, const piml_scenario_rules* r, int members,
                                             const uint64_t* seeds, const piml_mlapm_law* law, const void* law_table_device,
                                             const piml_wall_grid* wall_grid, const piml_wall_law* wall,
                                             const piml_wall_law* wall_table_device, const piml_nav_grid* nav,
                                             long long member_stride, const piml_noise_args* noise, int frame_offset,
                                             void* stream) {
    if (member_stride < 0) return hipErrorInvalidValue;
    return step_mlapm_nav(s, r, members, seeds, law, law_table_device, wall_grid, wall, wall_table_device, nav, nullptr, noise,
                          frame_offset, stream, member_stride);
}

PIML_API int piml_nav_choose_exit(const piml_scenario* s, int members, const uint64_t* seeds, const piml_nav_grid* nav,
                                  long long member_stride, const int* gate_class, const piml_exit_choice* law,
                                  int* switch_count, int frame_offset, void* stream) {
    if (!s || !gate_class || !law || members < 1 || members > 65535 || (!seeds && members != 1) || frame_offset < 0 ||
        member_stride < 0)
        return hipErrorInvalidValue;
    if (!frame_args_ok(*s, nullptr, nullptr, 1)) return hipErrorInvalidValue;  // GC's descriptor (init = 1 waives a_next)
    if (s->route_max_iters != 0 || s->D < 2) return hipErrorInvalidValue;      // the waypoint is the destination
    if (!piml::nav_grid_ok(nav) || nav->G != s->E) return hipErrorInvalidValue;
    if (law->every < 1 || !(law->margin >= 0.f) || !(law->commit >= 0.f)) return hipErrorInvalidValue;   // (NaN fails both)
    piml::ExitChoiceArgs A;
    A.NV = *nav;
    A.member_stride = member_stride;
    A.gate_class = gate_class;
    A.law = *law;
    A.switch_count = switch_count;
    A.frame_offset = frame_offset;
    const dim3 grid((unsigned)((s->capacity + piml::kMlScWaves - 1) / piml::kMlScWaves), (unsigned)members);
    hipLaunchKernelGGL(piml::scenario_choose_exit_kernel, grid, dim3(piml::kMlScWaves * 64), 0, piml::as_stream(stream), *s,
                       (const unsigned long long*)seeds, A);
    return hipGetLastError();
}

PIML_API int piml_scenario_route(const float* origin, const float* destination, int n, const float* polyline, int R,
                                 int max_iters, float clearance, float* waypoint, int* iters, void* stream) {
    if (n < 0 || R < 2 || max_iters < 0 || max_iters > piml::kScenarioMaxIters) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    if (!origin || !destination || !polyline || !waypoint || !iters) return hipErrorInvalidValue;
    hipLaunchKernelGGL(piml::scenario_route_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, piml::as_stream(stream),
                       (const float2*)origin, (const float2*)destination, n, (const float2*)polyline, R, max_iters, clearance,
                       (float2*)waypoint, iters);
    return hipGetLastError();
}
