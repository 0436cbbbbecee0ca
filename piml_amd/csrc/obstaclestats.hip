// Obstacle statistics of crowds: what the agents do next to the scene's walls and pillars, which no sibling
// (crowdstats, pairstats, flowstats, trackstats) looks at -- each focal agent-frame's clearance to the nearest obstacle
// point, the contacts, the smallest time to an obstacle, and per step the clearance of the swept segment p(t) .. p(t+1)
// with the crossings ("hits": tunnelling between frames) -- for S members against one shared list of O obstacle points.
//
// Agent i takes part at (s, t) when M == 1, both coordinates of P are finite and below 65536 in magnitude and both
// components of V are finite and below 1024 in magnitude; slots at or past n_active[s] are not swept.  Focal: it takes part
// and lies in the optional box [x0, x1) x [y0, y1).  An obstacle point is valid when both coordinates are finite; the others
// are skipped, and with no valid point only `focal` and `steps` count.  Window frames t = 0 .. T' - 1, float32 with true
// divisions and square roots and no contraction, Q = 2^20.  For a focal (i, t) and every valid point q, e = q - p(t):
//   clearance r = sqrt(min_q |e|^2); contact when r < radius;
//   time to wall (pairstats' formula for a point at rest): c = |e|^2 - radius^2, b = -(e.v), a = |v|^2; on a collision
//       course when c >= 0, b < 0 and disc = b^2 - a c >= 0, then tau = c / (-b + sqrt(disc)); tau_min = min_q tau;
//   a step (i, t) exists when i is focal at t, takes part at t + 1 and t + 1 < T': u = p(t+1) - p(t), len2 = |u|^2,
//       s = min(max((e.u) / len2, 0), 1) (s = 0 when len2 == 0), m = sqrt(min_q |e - s u|^2); a hit when m < hit_radius.
// The minima are exact in float32 whatever the order of the points (fminf; every lane visits the points in list order).
//
// obstacle_stats_kernel: one workgroup of OS_THREADS lanes takes a run of consecutive slices (s, t).  The focal agents of a
// slice are compacted in slot order into LDS (tiles of OS_FOCAL_TILE candidate slots) and taken one per lane in chunks of
// OS_THREADS, so that absent slots and agents outside the box occupy no lane; a lane keeps p, v, u and its three running
// minima in registers.  The obstacle points are staged into LDS in tiles of PIML_OBS_TILE points, 8 B each, the skipped
// ones filtered out while staging (a ballot compaction, in list order; an odd count is made even with a copy of the last
// point, which changes no minimum); every lane reads the same two points per 16-byte read, a broadcast without bank
// conflicts (13 % faster at the GC ensemble shape than one point per 8-byte read).  A list of at most one tile (GC: 4094 points) is staged once per workgroup and serves all its
// slices.  An item's bins and counts go into the workgroup's u64 LDS accumulator with integer LDS atomics (a handful per
// item, against O point evaluations); the accumulator is added to the member's rows of the workspace with 64-bit integer
// atomics when the member changes and at the end of the run.  The track rows (frames, contacts, hits, the smallest
// llrintf(Q r)) live in the workspace too, several workgroups sharing a track: integer atomic adds, and an atomic max of
// 2^62 - value for the minimum (0 = no focal frame).  obstacle_stats_copy_kernel moves the workspace into the outputs.  No
// float atomics: every output is an integer, so the results are bitwise reproducible whatever the order of the adds.
//
// LDS: 32 KiB of points + 4 KiB of focal slots + 8.1 KiB of accumulator = 44.2 KiB, three workgroups (12 waves) per CU; the
// sweep is bound by its ~45 vector instructions per point (the IEEE division of s among them), not by the broadcast read,
// and the registers stay far below the 128 that 12 waves per CU allow.
#include "stats.hpp"
#include "../../include/piml_hip.h"

#include <cmath>

namespace piml {

constexpr int OS_THREADS = 256;
constexpr int OS_WAVES = OS_THREADS / 64;
constexpr int OS_TILE = PIML_OBS_TILE;        // obstacle points per LDS tile (32 KiB)
static_assert(OS_TILE % 2 == 0, "the sweep reads the points in pairs");
constexpr int OS_FOCAL_TILE = 1024;           // candidate slots per focal compaction
constexpr int OS_MAX_BINS = 256;
constexpr int OS_MAX_N = 65536;
constexpr int OS_MAX_O = 1 << 24;
constexpr float OS_Q = 1048576.f;             // 2^20
constexpr float OS_MAX_COORD = 65536.f;
constexpr float OS_MAX_SPEED = 1024.f;
constexpr float OS_MAX_R = 16777216.f;        // trk_min holds llrintf(Q min(r, 2^24))
constexpr unsigned long long OS_MIN_BASE = 1ull << 62;
constexpr int OS_COUNTERS = 5;                // focal, steps, contact, hit, clear_sum
constexpr int OS_ACC = OS_COUNTERS + 4 * (OS_MAX_BINS + 1);
constexpr long long OS_MAX_GRID = 1 << 20;
constexpr long long OS_TARGET_WG = 4096;      // runs are sized so that about this many workgroups start
constexpr int OS_MAX_RUN = 64;

struct ObstacleArgs {
    const float *P, *V, *M;                   // (S, T, N, 2), (S, T, N, 2), (S, T, N)
    const int* n_active;                      // (S) or NULL
    const float* obs;                         // (O, 2)
    int S, T, N, O, t0, Tp, RB, TB, run, has_box;
    float radius, r2, hit_radius, r_bin, r_top, tau_bin, x0, x1, y0, y1;
    long long slices;
    unsigned long long* ws;                   // counters (5, S) | clear, clear_speed, swept (S, RB + 1) | min_ttc (S, TB + 1) |
                                              // trk_frames, trk_contacts, trk_hits, trk_min (S, N)
    long long *focal, *steps, *contact, *hit, *clear_sum, *clear, *clear_speed, *swept, *min_ttc;
    long long *trk_frames, *trk_contacts, *trk_hits, *trk_min;
};

__device__ __forceinline__ bool os_participant(float m, float2 p, float2 v) {
    return m == 1.f && fabsf(p.x) < OS_MAX_COORD && fabsf(p.y) < OS_MAX_COORD && fabsf(v.x) < OS_MAX_SPEED &&
           fabsf(v.y) < OS_MAX_SPEED;
}

// Compacts the valid points of obs[lo, hi) (hi - lo <= OS_TILE) into pts in list order; returns their number, rounded up to
// an even one (wg_compact: every thread calls it, and the tile may still be read on entry).
__device__ int os_stage_points(const float2* obs, int lo, int hi, float2* pts, int* wave_cnt) {
    float2 pt;
    int cnt = wg_compact<OS_THREADS>(
        lo, hi, wave_cnt, [&](int j) { return pt = obs[j], isfinite(pt.x) && isfinite(pt.y); },
        [&](int q, int) { pts[q] = pt; });
    // an odd number is made even with a copy of the last point, which changes no minimum: the sweep reads pairs
    if (cnt & 1) {
        if (threadIdx.x == 0) pts[cnt] = pts[cnt - 1];
        ++cnt;
        __syncthreads();
    }
    return cnt;
}

struct OsLane {
    float px, py, vx, vy, ux, uy, aa, len2;   // aa = |v|^2
    float min_d2, min_tau, min_m2;
};

// One point against one focal agent.
__device__ __forceinline__ void os_point(float qx, float qy, float r2, bool moves, OsLane& l) {
    const float ex = qx - l.px, ey = qy - l.py;
    const float d2 = ex * ex + ey * ey;
    l.min_d2 = fminf(l.min_d2, d2);
    float s = 0.f;
    if (moves) s = fminf(fmaxf((ex * l.ux + ey * l.uy) / l.len2, 0.f), 1.f);
    const float fx = ex - s * l.ux, fy = ey - s * l.uy;
    l.min_m2 = fminf(l.min_m2, fx * fx + fy * fy);
    const float c = d2 - r2;
    const float b = -(ex * l.vx + ey * l.vy);
    if (c >= 0.f && b < 0.f) {
        const float disc = b * b - l.aa * c;
        if (disc >= 0.f) l.min_tau = fminf(l.min_tau, c / (-b + sqrtf(disc)));
    }
}

// The sweep of one focal agent over cnt staged points (cnt even: os_stage_points pads), two points per 16-byte read.
__device__ __forceinline__ void os_sweep(const float2* pts, int cnt, float r2, OsLane& l) {
    const bool moves = l.len2 != 0.f;
    const float4* pairs = reinterpret_cast<const float4*>(pts);
    for (int k = 0; k < cnt / 2; ++k) {
        const float4 q = pairs[k];
        os_point(q.x, q.y, r2, moves, l);
        os_point(q.z, q.w, r2, moves, l);
    }
}

__device__ __forceinline__ int os_bin(float x, float width, int bins) {
    const float q = floorf(x / width);
    return q < (float)bins ? (int)q : bins;
}

__global__ void __launch_bounds__(OS_THREADS) obstacle_stats_kernel(ObstacleArgs a) {
    __shared__ __align__(16) float2 pts[OS_TILE];
    __shared__ int fslot[OS_FOCAL_TILE];
    __shared__ int wave_cnt[OS_WAVES];
    __shared__ unsigned long long acc[OS_ACC];
    const int tid = threadIdx.x;
    const int RB = a.RB, TB = a.TB, N = a.N;
    // rows of the accumulator: counters, clear, clear_speed, swept (RB + 1 each), min_ttc (TB + 1)
    const int o_clear = OS_COUNTERS, o_speed = o_clear + RB + 1, o_swept = o_speed + RB + 1, o_ttc = o_swept + RB + 1;
    const int n_acc = o_ttc + TB + 1;
    for (int k = tid; k < OS_ACC; k += OS_THREADS) acc[k] = 0ull;
    const float2* obs = reinterpret_cast<const float2*>(a.obs);
    const bool one_tile = a.O <= OS_TILE;
    int cnt = one_tile ? os_stage_points(obs, 0, a.O, pts, wave_cnt) : 0;
    __syncthreads();
    const long long SN = (long long)a.S * N;
    unsigned long long* w_rows = a.ws + (long long)OS_COUNTERS * a.S;
    unsigned long long* w_ttc = w_rows + 3ll * a.S * (RB + 1);
    unsigned long long* w_trk = w_ttc + (long long)a.S * (TB + 1);
    const long long runs = (a.slices + a.run - 1) / a.run;
    for (long long r = blockIdx.x; r < runs; r += gridDim.x) {
        const long long lo = r * a.run, hi = min(lo + (long long)a.run, a.slices);
        int cur_s = -1;
        for (long long sl = lo; sl <= hi; ++sl) {
            const int s = sl < hi ? (int)(sl / a.Tp) : -1;
            if (cur_s >= 0 && s != cur_s) {
                // flush the accumulator into member cur_s's workspace rows
                for (int e = tid; e < n_acc; e += OS_THREADS) {
                    const unsigned long long v = acc[e];
                    if (!v) continue;
                    unsigned long long* dst;
                    if (e < OS_COUNTERS) dst = a.ws + (long long)e * a.S + cur_s;
                    else if (e < o_ttc) {
                        const int row = (e - o_clear) / (RB + 1);
                        dst = w_rows + ((long long)row * a.S + cur_s) * (RB + 1) + (e - o_clear - row * (RB + 1));
                    } else dst = w_ttc + (long long)cur_s * (TB + 1) + (e - o_ttc);
                    atomicAdd(dst, v);
                    acc[e] = 0ull;
                }
                __syncthreads();
            }
            if (sl == hi) break;
            cur_s = s;
            const int t = (int)(sl - (long long)s * a.Tp);
            const bool has_next = t + 1 < a.Tp;
            const long long f0 = ((long long)s * a.T + a.t0 + t) * N;
            const float2* P0 = reinterpret_cast<const float2*>(a.P) + f0;
            const float2* V0 = reinterpret_cast<const float2*>(a.V) + f0;
            const float* M0 = a.M + f0;
            int bound = N;
            if (a.n_active) bound = min(max(a.n_active[s], 0), N);
            unsigned long long* trk = w_trk + (long long)s * N;
            for (int f_lo = 0; f_lo < bound; f_lo += OS_FOCAL_TILE) {
                const int nf = wg_compact<OS_THREADS>(
                    f_lo, min(f_lo + OS_FOCAL_TILE, bound), wave_cnt,
                    [&](int j) {
                        const float2 p = P0[j];
                        return os_participant(M0[j], p, V0[j]) && in_box(a.has_box, a.x0, a.x1, a.y0, a.y1, p);
                    },
                    [&](int q, int j) { fslot[q] = j; });
                for (int c0 = 0; c0 < nf; c0 += OS_THREADS) {
                    const bool focal = c0 + tid < nf;
                    const int i = focal ? fslot[c0 + tid] : 0;
                    OsLane l{};
                    l.min_d2 = l.min_tau = l.min_m2 = INFINITY;
                    bool step = false;
                    if (focal) {
                        const float2 p = P0[i], v = V0[i];
                        l.px = p.x, l.py = p.y, l.vx = v.x, l.vy = v.y;
                        l.aa = v.x * v.x + v.y * v.y;
                        if (has_next) {
                            const float2 p1 = P0[N + i];      // frame t + 1 of the same member
                            step = os_participant(M0[N + i], p1, V0[N + i]);
                            if (step) {
                                l.ux = p1.x - p.x, l.uy = p1.y - p.y;
                                l.len2 = l.ux * l.ux + l.uy * l.uy;
                            }
                        }
                    }
                    int n_valid = cnt;
                    if (one_tile) {
                        if (focal) os_sweep(pts, cnt, a.r2, l);
                    } else {
                        n_valid = 0;
                        for (int o_lo = 0; o_lo < a.O; o_lo += OS_TILE) {
                            cnt = os_stage_points(obs, o_lo, min(o_lo + OS_TILE, a.O), pts, wave_cnt);
                            n_valid += cnt;
                            if (focal) os_sweep(pts, cnt, a.r2, l);
                            __syncthreads();  // every lane is done with this tile before the next one is staged
                        }
                    }
                    if (!focal) continue;
                    atomicAdd(acc + 0, 1ull);
                    if (step) atomicAdd(acc + 1, 1ull);
                    if (n_valid == 0) continue;
                    const float rr = sqrtf(l.min_d2);
                    const int rb = os_bin(rr, a.r_bin, RB);
                    const bool contact = rr < a.radius;
                    atomicAdd(acc + o_clear + rb, 1ull);
                    atomicAdd(acc + o_speed + rb, (unsigned long long)llrintf(sqrtf(l.aa) * OS_Q));
                    if (rr < a.r_top) atomicAdd(acc + 4, (unsigned long long)llrintf(rr * OS_Q));
                    if (contact) atomicAdd(acc + 2, 1ull);
                    atomicAdd(acc + o_ttc + os_bin(l.min_tau, a.tau_bin, TB), 1ull);
                    bool hit = false;
                    if (step) {
                        const float m = sqrtf(l.min_m2);
                        hit = m < a.hit_radius;
                        atomicAdd(acc + o_swept + os_bin(m, a.r_bin, RB), 1ull);
                        if (hit) atomicAdd(acc + 3, 1ull);
                    }
                    atomicAdd(trk + i, 1ull);
                    if (contact) atomicAdd(trk + SN + i, 1ull);
                    if (hit) atomicAdd(trk + 2 * SN + i, 1ull);
                    atomicMax(trk + 3 * SN + i, OS_MIN_BASE - (unsigned long long)llrintf(fminf(rr, OS_MAX_R) * OS_Q));
                }
                __syncthreads();              // fslot is rewritten by the next focal tile
            }
        }
    }
}

__global__ void __launch_bounds__(OS_THREADS) obstacle_stats_copy_kernel(ObstacleArgs a) {
    const long long S = a.S, nr = S * (a.RB + 1), nt = S * (a.TB + 1), SN = S * a.N;
    const long long total = OS_COUNTERS * S + 3 * nr + nt + 4 * SN;
    for (long long e = (long long)blockIdx.x * OS_THREADS + threadIdx.x; e < total; e += (long long)gridDim.x * OS_THREADS) {
        const unsigned long long u = a.ws[e];
        const long long v = (long long)u;
        long long q = e;
        if (q < S) { a.focal[q] = v; continue; }
        q -= S;
        if (q < S) { a.steps[q] = v; continue; }
        q -= S;
        if (q < S) { a.contact[q] = v; continue; }
        q -= S;
        if (q < S) { a.hit[q] = v; continue; }
        q -= S;
        if (q < S) { a.clear_sum[q] = v; continue; }
        q -= S;
        if (q < nr) { a.clear[q] = v; continue; }
        q -= nr;
        if (q < nr) { a.clear_speed[q] = v; continue; }
        q -= nr;
        if (q < nr) { a.swept[q] = v; continue; }
        q -= nr;
        if (q < nt) { a.min_ttc[q] = v; continue; }
        q -= nt;
        if (q < SN) { a.trk_frames[q] = v; continue; }
        q -= SN;
        if (q < SN) { a.trk_contacts[q] = v; continue; }
        q -= SN;
        if (q < SN) { a.trk_hits[q] = v; continue; }
        q -= SN;
        a.trk_min[q] = u ? (long long)(OS_MIN_BASE - u) : -1;
    }
}

static long long os_workspace_elems(long long S, long long N, long long RB, long long TB) {
    return S * (OS_COUNTERS + 3 * (RB + 1) + (TB + 1) + 4 * N);
}

}  // namespace piml

using namespace piml;

PIML_API long long piml_obstacle_stats_workspace_bytes(int S, int N, int r_bins, int tau_bins) {
    if (S < 0 || N < 0 || r_bins < 0 || tau_bins < 0) return -1;
    return os_workspace_elems(S, N, r_bins, tau_bins) * (long long)sizeof(unsigned long long);
}

PIML_API int piml_obstacle_stats(const float* P, const float* V, const float* M, const int* n_active, int S, int T, int N,
                                 int t0, int t1, const float* obs, int O, float dt, float radius, float hit_radius,
                                 int has_box, float x0, float x1, float y0, float y1, float r_bin, int r_bins, float tau_bin,
                                 int tau_bins, long long* focal, long long* steps, long long* contact, long long* hit,
                                 long long* clear_sum, long long* clear, long long* clear_speed, long long* swept,
                                 long long* min_ttc, long long* trk_frames, long long* trk_contacts, long long* trk_hits,
                                 long long* trk_min, void* workspace, long long workspace_bytes, void* stream) {
    const auto positive = [](float x) { return x > 0.f && std::isfinite(x); };
    if (S < 0 || T < 0 || N < 0 || O < 0 || N > OS_MAX_N || O > OS_MAX_O || t0 < 0 || t1 > T || t1 < t0 || !positive(dt) ||
        !positive(radius) || !positive(hit_radius) || !positive(r_bin) || !positive(tau_bin) || r_bins < 1 ||
        r_bins > OS_MAX_BINS || tau_bins < 1 || tau_bins > OS_MAX_BINS)
        return hipErrorInvalidValue;
    if (has_box && (!std::isfinite(x0) || !std::isfinite(x1) || !std::isfinite(y0) || !std::isfinite(y1) || !(x0 < x1) ||
                    !(y0 < y1)))
        return hipErrorInvalidValue;
    // No 64-bit sum overflows: a member's clear_speed row adds at most N T' terms below sqrt(2) 1024 Q < 1449 Q, its clear_sum
    // at most N T' terms below r_bin r_bins Q (DESIGN 4.23 "No overflow").
    const float r_top = r_bin * (float)r_bins;
    const double items = (double)N * (double)(t1 - t0), two63 = 9223372036854775808.0;
    if (!std::isfinite(r_top) || !(1449.0 * (double)OS_Q * items < two63) || !((double)r_top * (double)OS_Q * items < two63))
        return hipErrorInvalidValue;
    if (S == 0 || t1 == t0 || N == 0 || O == 0) return hipSuccess;
    if (!P || !V || !M || !obs || !focal || !steps || !contact || !hit || !clear_sum || !clear || !clear_speed || !swept ||
        !min_ttc || !trk_frames || !trk_contacts || !trk_hits || !trk_min || !workspace)
        return hipErrorInvalidValue;
    const long long need = piml_obstacle_stats_workspace_bytes(S, N, r_bins, tau_bins);
    if (workspace_bytes < need) return hipErrorInvalidValue;
    ObstacleArgs a{};
    a.P = P, a.V = V, a.M = M, a.n_active = n_active, a.obs = obs;
    a.S = S, a.T = T, a.N = N, a.O = O, a.t0 = t0, a.Tp = t1 - t0, a.RB = r_bins, a.TB = tau_bins;
    a.slices = (long long)S * a.Tp;
    const unsigned grid = stats_run_grid(a.slices, OS_TARGET_WG, OS_MAX_RUN, OS_MAX_GRID, &a.run);
    a.has_box = has_box ? 1 : 0;
    a.x0 = x0, a.x1 = x1, a.y0 = y0, a.y1 = y1;
    a.radius = radius, a.r2 = radius * radius, a.hit_radius = hit_radius;
    a.r_bin = r_bin, a.r_top = r_top, a.tau_bin = tau_bin;
    a.ws = static_cast<unsigned long long*>(workspace);
    a.focal = focal, a.steps = steps, a.contact = contact, a.hit = hit, a.clear_sum = clear_sum;
    a.clear = clear, a.clear_speed = clear_speed, a.swept = swept, a.min_ttc = min_ttc;
    a.trk_frames = trk_frames, a.trk_contacts = trk_contacts, a.trk_hits = trk_hits, a.trk_min = trk_min;
    hipStream_t st = as_stream(stream);
    hipError_t e = hipMemsetAsync(workspace, 0, (size_t)need, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(obstacle_stats_kernel, dim3(grid), dim3(OS_THREADS), 0, st, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const long long elems = need / (long long)sizeof(unsigned long long);
    const long long blocks = (elems + OS_THREADS - 1) / OS_THREADS;
    hipLaunchKernelGGL(obstacle_stats_copy_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(OS_THREADS), 0, st, a);
    return hipGetLastError();
}
