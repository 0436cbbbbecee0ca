// Calibration of MLAPM's six constants on multi-frame rollouts: the weighted mean squared POSITION error of H closed-loop
// MLAPM steps per window and its gradient with respect to (tau, A, B, C, D, theta_deg), by an adjoint sweep in the same
// launch.  The one-step loss of mlapm_fit.hip never sees errors that feed back through the neighbours; this one does
// (the reference trains its network the same way: multiple_rollout_mse_loss, src/models/simulators.py:172-193, 659-832).
//
// The windows arrive packed (piml_amd/calibrate.py pack_windows).  Window w owns the slots [slot_off[w], slot_off[w + 1)),
// n of them: every agent present in any of its H + 1 frames.  Entry (w, k, s) = (H + 1) slot_off[w] + k n + s holds the
// recorded (p, v), the destination and a flag byte (bit 0 present, bit 1 injected, bit 2 carried from k - 1).
//   forward   k = 0 .. H-1: a slot present in k and k + 1 steps v' = MLAPM.step over the slots present in k, p' = p + v' dt;
//             a slot that enters in k + 1 takes its recorded (p, v) (the reference's new_peds_flag) and no gradient.
//   loss      w_k |p^_k - P_k|^2 over the carried (k, slot), w_k = time_decay^(H - k), divided by sum w_k (float64).
//   adjoint   k = H-1 .. 0: g = lambda_v + dt lambda_p at k + 1 is d loss / d v'; the pair backward (mlapm_pair_grad, both
//             roles of every pair, as mlapm_bwd_kernel) gives d / d(p, v) at k, lambda_p passes through the Euler update, and
//             the per-focal parameter sums of mlapm_fit.hip (fit_pair) dotted with g give the parameter gradient.
// Positions are carried as an offset from the recording, d = p^ - P (float32): a pair's relative position is
// (P_j - P_i) + (d_j - d_i) and the error is d itself, so the float32 state keeps the precision of the small numbers the
// loss is made of rather than that of coordinates of ~20 m.
//
// Forms, by the window's slot count n (the host sorts the windows into two lists):
//   n <= 64  mlapm_rollout_small_kernel: one wave per window, a lane per slot, every saved state (H + 1) x 64 x 16 B in LDS
//            (recorded GC frames hold ~21 agents; (H + 3) KiB, H <= 48);
//   n >  64  mlapm_rollout_big_kernel: four waves per window, a wave per focal slot with the lanes striding the sources
//            (mlapm_fit_wave_kernel's decomposition, for open-world clips), the saved states and the adjoint in the
//            workspace (L2-resident: a step of a 500-agent window is 8 KiB).
// Every window writes one float64 row (weight, weighted squared error, 6 gradients, then H squared-error sums and H term
// counts by k); mlapm_rollout_reduce_kernel (ONE workgroup, a second launch) adds the rows in a fixed order.  No atomics:
// two calls are bitwise equal.  The constants are read from device memory, so a fit iteration can be captured.
#include "common.hpp"
#include "mlapm.hpp"
#include "../../include/piml_hip.h"

#include <cmath>

namespace piml {

constexpr int kRollRow = 8;            // weight, sum w |d|^2, d/d(tau, A, B, C, D, theta); then 2 H per-step columns
constexpr int kRollSmall = 64;         // slots of a window of the small form
constexpr int kRollSmallMaxH = 48;     // LDS (H + 3) KiB of the small form
constexpr int kRollWaves = 4;          // waves of the big form
constexpr unsigned char kPresent = 1, kCarried = 4;

struct RollPack {
    const float4* rec;                 // (R) recorded px, py, vx, vy per (window, k, slot)
    const float2* dest;                // (R)
    const unsigned char* flags;        // (R)
    const float* v0;                   // (S) desired speed per slot
    const int* slot_off;               // (W + 1)
    int W, H;
};

struct RollOut {
    double* rows;                      // (windows, 8 + 2 H)
    float4* big;                       // big-form state: per slot (H + 1) saved (d, v), stage (e, g), adjoint (lp, lv)
    float dt, radius;
    double decay;
    long long big_slots;               // float4 blocks of (H + 4) in `big`
    int variant;
};

__device__ __forceinline__ MlapmParams roll_params(const FitConst& K, const float* __restrict__ params) {
    MlapmParams P;
    P.variant = K.variant; P.tau = K.tau; P.A = K.A; P.B = params[2]; P.Cc = params[3]; P.D = params[4];
    P.cth = K.cth; P.sth = K.sth; P.r2 = K.r2; P.B2 = K.B2; P.C2 = K.C2; P.D2 = K.D2;
    P.skip_absent = 0; P.ucy_two_phase = 0;
    return P;
}

__device__ __forceinline__ double decay_weight(double g, int e) {    // time_decay^e, the same products everywhere
    double w = 1.0;
    for (int q = 0; q < e; ++q) w *= g;
    return w;
}

// desired direction e = normalize(D - p^) with p^ = P + d (mlapm.py:21), and |D - p^|
__device__ __forceinline__ void roll_dir(float2 D, float4 rc, float4 cur, float& ex, float& ey, float& dn) {
    ex = (D.x - rc.x) - cur.x; ey = (D.y - rc.y) - cur.y;
    dn = norm2(ex, ey);
    const float en = fmaxf(dn, 1e-12f);
    ex /= en; ey /= en;
}

// one step of a carried slot: v' = v + F dt (mlapm.py:57), d' = d + (v' dt - (P_{k+1} - P_k)) (explicit Euler)
__device__ __forceinline__ float4 roll_advance(const MlapmParams& P, float dt, float v0, float ex, float ey, float4 rc,
                                               float4 rc1, float4 cur, float sx, float sy) {
    const float fx = (v0 * ex - cur.z) / P.tau - sx, fy = (v0 * ey - cur.w) / P.tau - sy;
    const float vx = cur.z + fx * dt, vy = cur.w + fy * dt;
    return make_float4(cur.x + (vx * dt - (rc1.x - rc.x)), cur.y + (vy * dt - (rc1.y - rc.y)), vx, vy);
}

// the state adjoint of one step for a focal slot, from its sums (sp, sv) over the pairs (mlapm_bwd_kernel's tail):
// lambda_p(k) = [carried] lambda_p(k + 1) + sp - d(desired force)/dp . G,  lambda_v(k) = sv + g - G / tau
__device__ __forceinline__ float4 roll_adjoint(const MlapmParams& P, float dt, float v0, float ex, float ey, float dn,
                                               float gx, float gy, float4 lam, bool carried, float spx, float spy,
                                               float svx, float svy) {
    const float Gx = gx * dt, Gy = gy * dt;
    const float ge = Gx * ex + Gy * ey;
    float tdx, tdy;
    if (dn > 1e-12f) {
        tdx = v0 / P.tau * (Gx - ge * ex) / dn;
        tdy = v0 / P.tau * (Gy - ge * ey) / dn;
    } else {
        tdx = v0 / P.tau * Gx / 1e-12f; tdy = v0 / P.tau * Gy / 1e-12f;
    }
    const float lpx = carried ? lam.x : 0.f, lpy = carried ? lam.y : 0.f;
    return make_float4(lpx + spx - tdx, lpy + spy - tdy, svx + gx - Gx / P.tau, svy + gy - Gy / P.tau);
}

// d v' / d params dotted with g (fit_focal_row with g in place of 2 r); constants a variant does not use stay 0
__device__ __forceinline__ void roll_param_grad(const FitConst& K, float dt, float v0, float ex, float ey, float4 cur,
                                                float gx, float gy, const FitAcc& a, double* acc) {
    const float fdx = (v0 * ex - cur.z) / K.tau, fdy = (v0 * ey - cur.w) / K.tau;
    const double ddt = dt, A = K.A, x = gx, y = gy;
    acc[0] += ddt * (x * (-(double)fdx) + y * (-(double)fdy)) / (double)K.tau;
    acc[1] += -ddt * (x * a.ux + y * a.uy);
    acc[2] += -ddt * A * (x * a.bx + y * a.by);
    if (K.variant != 0) acc[3] += -ddt * A * (x * a.cx + y * a.cy);
    if (K.variant == 1) acc[4] += -ddt * A * (x * a.dx + y * a.dy);
    if (K.variant != 0) acc[5] += -ddt * A * (x * a.tx + y * a.ty);
}

__device__ __forceinline__ bool window_of(const RollPack& Q, const int* __restrict__ wins, int idx, int cap, int& s0, int& n) {
    const int w = wins[idx];
    if (w < 0 || w >= Q.W) return false;
    s0 = Q.slot_off[w];
    n = Q.slot_off[w + 1] - s0;
    return s0 >= 0 && n >= 0 && n <= cap;
}

// ---- small form: one wave per window, lane = slot ----
__global__ __launch_bounds__(kRollSmall) void mlapm_rollout_small_kernel(RollPack Q, const int* __restrict__ wins,
                                                                         const float* __restrict__ params, RollOut O) {
    extern __shared__ __align__(16) float4 roll_lds[];
    const int H = Q.H, width = kRollRow + 2 * H;
    float4* saved = roll_lds;                                   // (H + 1) x 64: (d, v)
    float4* stA = roll_lds + (size_t)(H + 1) * kRollSmall;       // forward: (P, -, -); backward: (P, e)
    float4* stB = stA + kRollSmall;                              // backward: (g, -, -)
    const FitConst K = fit_const(params, O.variant, O.radius);
    const MlapmParams MP = roll_params(K, params);
    const float dt = O.dt;
    const int lane = threadIdx.x;
    double* row = O.rows + (size_t)blockIdx.x * width;
    int s0 = 0, n = 0;
    if (!window_of(Q, wins, blockIdx.x, kRollSmall, s0, n)) n = 0;
    const bool has = lane < n;
    const size_t base = (size_t)(H + 1) * s0;
    auto at = [&](int k) { return base + (size_t)k * n + lane; };
    const float v0 = has ? Q.v0[s0 + lane] : 0.f;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    double lw = 0.0, le = 0.0;
    {
        const float4 rc = has ? Q.rec[at(0)] : float4(zero4);
        saved[lane] = make_float4(0.f, 0.f, rc.z, rc.w);
    }
    for (int k = 0; k < H; ++k) {
        const unsigned char fk = has ? Q.flags[at(k)] : 0, fk1 = has ? Q.flags[at(k + 1)] : 0;
        const float4 rc = has ? Q.rec[at(k)] : float4(zero4);
        const u64 mask = __builtin_amdgcn_ballot_w64((fk & kPresent) != 0);
        stA[lane] = rc;
        __syncthreads();
        const float4 cur = saved[k * kRollSmall + lane];
        float4 nxt = zero4;
        double e2 = 0.0, cnt = 0.0;
        if (fk1 & kCarried) {
            const float4 rc1 = Q.rec[at(k + 1)];
            float ex, ey, dn;
            roll_dir(Q.dest[at(k)], rc, cur, ex, ey, dn);
            float sx = 0.f, sy = 0.f;
            for (u64 m = mask; m; m &= m - 1) {
                const int j = __builtin_ctzll(m);
                if (j == lane) continue;
                const float4 pj = stA[j], cj = saved[k * kRollSmall + j];
                const float2 f = mlapm_pair(MP, (pj.x - rc.x) + (cj.x - cur.x), (pj.y - rc.y) + (cj.y - cur.y),
                                            cj.z - cur.z, cj.w - cur.w, cur.z, cur.w, ex, ey);
                sx += f.x; sy += f.y;
            }
            nxt = roll_advance(MP, dt, v0, ex, ey, rc, rc1, cur, sx, sy);
            e2 = (double)nxt.x * nxt.x + (double)nxt.y * nxt.y;
            cnt = 1.0;
            const double w = decay_weight(O.decay, H - k - 1);
            lw += w; le += w * e2;
        } else if (fk1 & kPresent) {
            const float4 rc1 = Q.rec[at(k + 1)];
            nxt = make_float4(0.f, 0.f, rc1.z, rc1.w);              // injected: the recorded state
        }
        saved[(k + 1) * kRollSmall + lane] = nxt;
        e2 = wave_sum_d(e2); cnt = wave_sum_d(cnt);
        if (lane == 0) { row[kRollRow + k] = e2; row[kRollRow + H + k] = cnt; }
        __syncthreads();
    }
    // adjoint at H: d (sum w |d|^2) / d p^_H
    float4 lam = zero4;
    if (has && (Q.flags[at(H)] & kCarried)) {
        const float4 c = saved[H * kRollSmall + lane];
        lam = make_float4(2.f * c.x, 2.f * c.y, 0.f, 0.f);
    }
    double ga[6] = {0, 0, 0, 0, 0, 0};
    for (int k = H - 1; k >= 0; --k) {
        const unsigned char fk = has ? Q.flags[at(k)] : 0, fk1 = has ? Q.flags[at(k + 1)] : 0;
        const bool present = (fk & kPresent) != 0, carried = (fk1 & kCarried) != 0;
        const u64 mask = __builtin_amdgcn_ballot_w64(present);
        const float4 rc = has ? Q.rec[at(k)] : float4(zero4);
        const float4 cur = saved[k * kRollSmall + lane];
        float ex = 0.f, ey = 0.f, dn = 0.f;
        if (present) roll_dir(Q.dest[at(k)], rc, cur, ex, ey, dn);
        const float gx = carried ? lam.z + dt * lam.x : 0.f, gy = carried ? lam.w + dt * lam.y : 0.f;
        stA[lane] = make_float4(rc.x, rc.y, ex, ey);
        stB[lane] = make_float4(gx * dt, gy * dt, 0.f, 0.f);
        __syncthreads();
        float4 nl = zero4;
        if (present) {
            const float Gx = gx * dt, Gy = gy * dt;
            FitAcc a = {};
            float spx = 0.f, spy = 0.f, svx = 0.f, svy = 0.f;
            for (u64 m = mask; m; m &= m - 1) {
                const int j = __builtin_ctzll(m);
                if (j == lane) continue;
                const float4 pj = stA[j], tj = stB[j], cj = saved[k * kRollSmall + j];
                const float rx = (pj.x - rc.x) + (cj.x - cur.x), ry = (pj.y - rc.y) + (cj.y - cur.y);
                const float wx = cj.z - cur.z, wy = cj.w - cur.w;
                float ax, ay, bx, by;
                if (carried) {                                  // focal side: this slot's own step
                    fit_pair(K, rx, ry, wx, wy, cur.z, cur.w, ex, ey, a);
                    mlapm_pair_grad(MP, rx, ry, wx, wy, cur.z, cur.w, ex, ey, Gx, Gy, ax, ay, bx, by);
                    spx -= ax; spy -= ay; svx -= bx; svy -= by;
                }
                if (tj.x != 0.f || tj.y != 0.f) {               // source side: slot j's step (j is wave-uniform)
                    mlapm_pair_grad(MP, -rx, -ry, -wx, -wy, cj.z, cj.w, pj.z, pj.w, tj.x, tj.y, ax, ay, bx, by);
                    spx += ax; spy += ay; svx += bx; svy += by;
                }
            }
            nl = roll_adjoint(MP, dt, v0, ex, ey, dn, gx, gy, lam, carried, spx, spy, svx, svy);
            if (k >= 1 && (fk & kCarried)) {                    // the loss term of this slot at k
                const float w2 = (float)(2.0 * decay_weight(O.decay, H - k));
                nl.x += w2 * cur.x; nl.y += w2 * cur.y;
            }
            if (carried) roll_param_grad(K, dt, v0, ex, ey, cur, gx, gy, a, ga);
        }
        lam = nl;
        __syncthreads();
    }
    lw = wave_sum_d(lw); le = wave_sum_d(le);
#pragma unroll
    for (int q = 0; q < 6; ++q) ga[q] = wave_sum_d(ga[q]);
    if (lane == 0) {
        row[0] = lw; row[1] = le;
#pragma unroll
        for (int q = 0; q < 6; ++q) row[2 + q] = ga[q];
    }
}

// ---- big form: four waves per window, a wave per focal slot, state in the workspace ----
__global__ __launch_bounds__(kRollWaves * 64) void mlapm_rollout_big_kernel(RollPack Q, const int* __restrict__ wins,
                                                                            const int* __restrict__ big_base,
                                                                            const float* __restrict__ params, RollOut O,
                                                                            int row0) {
    __shared__ double red[kRollWaves][kRollRow];
    const int H = Q.H, width = kRollRow + 2 * H;
    const FitConst K = fit_const(params, O.variant, O.radius);
    const MlapmParams MP = roll_params(K, params);
    const float dt = O.dt;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double* row = O.rows + (size_t)(row0 + blockIdx.x) * width;
    int s0 = 0, n = 0;
    if (!window_of(Q, wins, blockIdx.x, 1 << 30, s0, n)) n = 0;
    const int bb = big_base[blockIdx.x];
    if (bb < 0 || (long long)bb + n > O.big_slots) n = 0;      // outside the workspace: an empty row
    const size_t base = (size_t)(H + 1) * s0;
    float4* saved = O.big + (size_t)(H + 4) * (n ? bb : 0);   // (H + 1) x n, then stage n, adjoint n
    float4* stage = saved + (size_t)(H + 1) * n;
    float4* lamv = stage + n;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    double lw = 0.0, le = 0.0;                                  // lane 0 of each wave
    for (int s = threadIdx.x; s < n; s += kRollWaves * 64) {
        const float4 rc = Q.rec[base + s];
        saved[s] = make_float4(0.f, 0.f, rc.z, rc.w);
    }
    __syncthreads();
    for (int k = 0; k < H; ++k) {
        const float4* sk = saved + (size_t)k * n;
        const size_t ek = base + (size_t)k * n, ek1 = ek + n;
        double e2 = 0.0, cnt = 0.0;
        for (int i = wave; i < n; i += kRollWaves) {
            const unsigned char fk1 = Q.flags[ek1 + i];
            float4 nxt = zero4;
            if (fk1 & kCarried) {
                const float4 rc = Q.rec[ek + i], cur = sk[i];
                float ex, ey, dn;
                roll_dir(Q.dest[ek + i], rc, cur, ex, ey, dn);
                float sx = 0.f, sy = 0.f;
                for (int j = lane; j < n; j += 64) {
                    if (j == i || !(Q.flags[ek + j] & kPresent)) continue;
                    const float4 pj = Q.rec[ek + j], cj = sk[j];
                    const float2 f = mlapm_pair(MP, (pj.x - rc.x) + (cj.x - cur.x), (pj.y - rc.y) + (cj.y - cur.y),
                                                cj.z - cur.z, cj.w - cur.w, cur.z, cur.w, ex, ey);
                    sx += f.x; sy += f.y;
                }
                sx = wave_sum(sx); sy = wave_sum(sy);
                nxt = roll_advance(MP, dt, Q.v0[s0 + i], ex, ey, rc, Q.rec[ek1 + i], cur, sx, sy);
                const double d2 = (double)nxt.x * nxt.x + (double)nxt.y * nxt.y;
                const double w = decay_weight(O.decay, H - k - 1);
                e2 += d2; cnt += 1.0; lw += w; le += w * d2;
            } else if (fk1 & kPresent) {
                const float4 rc1 = Q.rec[ek1 + i];
                nxt = make_float4(0.f, 0.f, rc1.z, rc1.w);
            }
            if (lane == 0) saved[(size_t)(k + 1) * n + i] = nxt;
        }
        if (lane == 0) { red[wave][0] = e2; red[wave][1] = cnt; }
        __syncthreads();
        if (threadIdx.x == 0) {
            double a = 0.0, c = 0.0;
            for (int q = 0; q < kRollWaves; ++q) { a += red[q][0]; c += red[q][1]; }
            row[kRollRow + k] = a; row[kRollRow + H + k] = c;
        }
        __syncthreads();
    }
    for (int s = threadIdx.x; s < n; s += kRollWaves * 64) {
        float4 lam = zero4;
        if (Q.flags[base + (size_t)H * n + s] & kCarried) {
            const float4 c = saved[(size_t)H * n + s];
            lam = make_float4(2.f * c.x, 2.f * c.y, 0.f, 0.f);
        }
        lamv[s] = lam;
    }
    double ga[6] = {0, 0, 0, 0, 0, 0};
    __syncthreads();
    for (int k = H - 1; k >= 0; --k) {
        const float4* sk = saved + (size_t)k * n;
        const size_t ek = base + (size_t)k * n, ek1 = ek + n;
        // stage every slot's desired direction and d loss / d v' for the source side of the pairs
        for (int s = threadIdx.x; s < n; s += kRollWaves * 64) {
            float ex = 0.f, ey = 0.f, dn = 0.f, gx = 0.f, gy = 0.f;
            if (Q.flags[ek + s] & kPresent) roll_dir(Q.dest[ek + s], Q.rec[ek + s], sk[s], ex, ey, dn);
            if (Q.flags[ek1 + s] & kCarried) {
                const float4 lam = lamv[s];
                gx = lam.z + dt * lam.x; gy = lam.w + dt * lam.y;
            }
            stage[s] = make_float4(ex, ey, gx * dt, gy * dt);
        }
        __syncthreads();
        for (int i = wave; i < n; i += kRollWaves) {
            const unsigned char fk = Q.flags[ek + i];
            if (!(fk & kPresent)) {
                if (lane == 0) lamv[i] = zero4;
                continue;
            }
            const bool carried = (Q.flags[ek1 + i] & kCarried) != 0;
            const float4 rc = Q.rec[ek + i], cur = sk[i], lam = lamv[i];
            float ex, ey, dn;
            roll_dir(Q.dest[ek + i], rc, cur, ex, ey, dn);
            const float gx = carried ? lam.z + dt * lam.x : 0.f, gy = carried ? lam.w + dt * lam.y : 0.f;
            const float Gx = gx * dt, Gy = gy * dt;
            FitAcc a = {};
            float spx = 0.f, spy = 0.f, svx = 0.f, svy = 0.f;
            for (int j = lane; j < n; j += 64) {
                if (j == i || !(Q.flags[ek + j] & kPresent)) continue;
                const float4 pj = Q.rec[ek + j], tj = stage[j], cj = sk[j];
                const float rx = (pj.x - rc.x) + (cj.x - cur.x), ry = (pj.y - rc.y) + (cj.y - cur.y);
                const float wx = cj.z - cur.z, wy = cj.w - cur.w;
                float ax, ay, bx, by;
                if (carried) {
                    fit_pair(K, rx, ry, wx, wy, cur.z, cur.w, ex, ey, a);
                    mlapm_pair_grad(MP, rx, ry, wx, wy, cur.z, cur.w, ex, ey, Gx, Gy, ax, ay, bx, by);
                    spx -= ax; spy -= ay; svx -= bx; svy -= by;
                }
                if (tj.z != 0.f || tj.w != 0.f) {
                    mlapm_pair_grad(MP, -rx, -ry, -wx, -wy, cj.z, cj.w, tj.x, tj.y, tj.z, tj.w, ax, ay, bx, by);
                    spx += ax; spy += ay; svx += bx; svy += by;
                }
            }
            spx = wave_sum(spx); spy = wave_sum(spy); svx = wave_sum(svx); svy = wave_sum(svy);
            if (carried) {
                a.ux = wave_sum(a.ux); a.uy = wave_sum(a.uy);
                a.bx = wave_sum(a.bx); a.by = wave_sum(a.by);
                if (K.variant != 0) {
                    a.cx = wave_sum(a.cx); a.cy = wave_sum(a.cy);
                    a.tx = wave_sum(a.tx); a.ty = wave_sum(a.ty);
                }
                if (K.variant == 1) { a.dx = wave_sum(a.dx); a.dy = wave_sum(a.dy); }
            }
            if (lane == 0) {
                const float v0 = Q.v0[s0 + i];
                float4 nl = roll_adjoint(MP, dt, v0, ex, ey, dn, gx, gy, lam, carried, spx, spy, svx, svy);
                if (k >= 1 && (fk & kCarried)) {
                    const float w2 = (float)(2.0 * decay_weight(O.decay, H - k));
                    nl.x += w2 * cur.x; nl.y += w2 * cur.y;
                }
                if (carried) roll_param_grad(K, dt, v0, ex, ey, cur, gx, gy, a, ga);
                lamv[i] = nl;
            }
        }
        __syncthreads();
    }
    if (lane == 0) {
        red[wave][0] = lw; red[wave][1] = le;
#pragma unroll
        for (int q = 0; q < 6; ++q) red[wave][2 + q] = ga[q];
    }
    __syncthreads();
    if (threadIdx.x < kRollRow) {
        double t = 0.0;
        for (int q = 0; q < kRollWaves; ++q) t += red[q][threadIdx.x];
        row[threadIdx.x] = t;
    }
}

// ONE workgroup: thread t adds rows t, t + 256, ... in order, then a fixed tree over the 256 threads, eight columns at a time
__global__ __launch_bounds__(256) void mlapm_rollout_reduce_kernel(const double* __restrict__ rows, int n_rows, int width,
                                                                   int cols, double* __restrict__ loss,
                                                                   float* __restrict__ grad, double* __restrict__ per_step) {
    __shared__ double red[kRollRow][256];
    __shared__ double head[kRollRow];
    for (int c0 = 0; c0 < cols; c0 += kRollRow) {
        double acc[kRollRow] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int r = threadIdx.x; r < n_rows; r += 256) {
#pragma unroll
            for (int q = 0; q < kRollRow; ++q)
                if (c0 + q < cols) acc[q] += rows[(size_t)r * width + c0 + q];
        }
#pragma unroll
        for (int q = 0; q < kRollRow; ++q) red[q][threadIdx.x] = acc[q];
        __syncthreads();
        for (int h = 128; h > 0; h >>= 1) {
            if ((int)threadIdx.x < h) {
#pragma unroll
                for (int q = 0; q < kRollRow; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + h];
            }
            __syncthreads();
        }
        if (threadIdx.x < kRollRow && c0 + (int)threadIdx.x < cols) {
            if (c0 == 0) head[threadIdx.x] = red[threadIdx.x][0];
            else per_step[c0 - kRollRow + threadIdx.x] = red[threadIdx.x][0];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double w = head[0];
        const double inv = w > 0.0 ? 1.0 / w : 0.0;             // no term: loss and gradient 0
        *loss = head[1] * inv;
        for (int q = 0; q < 6; ++q) grad[q] = (float)(head[2 + q] * inv);
    }
}

static long long roll_row_doubles(long long windows, int H) {
    const long long d = windows * (kRollRow + 2LL * H);
    return (d + 1) & ~1LL;                                      // the big-form state after it is 16-byte aligned
}

}  // namespace piml

using namespace piml;

PIML_API long long piml_mlapm_rollout_fit_workspace_doubles(int n_windows, int horizon, long long big_slots) {
    if (n_windows < 0 || horizon < 1 || big_slots < 0) return -1;
    return roll_row_doubles(n_windows, horizon) + big_slots * (horizon + 4LL) * 2;
}

PIML_API int piml_mlapm_rollout_fit_loss_grad(const float* rec_state, const float* destination, const unsigned char* flags,
                                              const float* desired_speed, const int* slot_offsets, int W, long long S,
                                              int horizon, const int* small_windows, int n_small,
                                              const int* big_windows, const int* big_base, int n_big, long long big_slots,
                                              const float* params, int variant, float dt, float radius, double time_decay,
                                              double* workspace, long long workspace_doubles, double* loss, float* grad,
                                              double* per_step, void* stream) {
    if (W < 0 || S < 0 || horizon < 1 || n_small < 0 || n_big < 0 || big_slots < 0) return hipErrorInvalidValue;
    if ((long long)n_small + n_big > W || (n_small > 0 && horizon > kRollSmallMaxH)) return hipErrorInvalidValue;
    if ((horizon + 1LL) * S >= (1LL << 40)) return hipErrorInvalidValue;
    if (variant < 0 || variant > 2 || !std::isfinite(dt) || !(dt > 0.f) || !std::isfinite(radius) || !(radius >= 0.f))
        return hipErrorInvalidValue;
    if (!std::isfinite(time_decay) || !(time_decay >= 0.f)) return hipErrorInvalidValue;
    if (!params || !loss || !grad || !slot_offsets) return hipErrorInvalidValue;
    if (S > 0 && (!rec_state || !destination || !flags || !desired_speed)) return hipErrorInvalidValue;
    if ((n_small > 0 && !small_windows) || (n_big > 0 && (!big_windows || !big_base))) return hipErrorInvalidValue;
    const long long need = piml_mlapm_rollout_fit_workspace_doubles(n_small + n_big, horizon, n_big > 0 ? big_slots : 0);
    if (!workspace || workspace_doubles < need) return hipErrorInvalidValue;
    const RollPack Q = {(const float4*)rec_state, (const float2*)destination, flags, desired_speed, slot_offsets, W, horizon};
    const RollOut O = {workspace, (float4*)(workspace + roll_row_doubles(n_small + n_big, horizon)), dt, radius,
                       time_decay, n_big > 0 ? big_slots : 0, variant};
    hipStream_t st = as_stream(stream);
    if (n_small > 0) {
        const size_t lds = (size_t)(horizon + 3) * kRollSmall * sizeof(float4);
        hipLaunchKernelGGL(mlapm_rollout_small_kernel, dim3(n_small), dim3(kRollSmall), lds, st, Q, small_windows, params, O);
    }
    if (n_big > 0)
        hipLaunchKernelGGL(mlapm_rollout_big_kernel, dim3(n_big), dim3(kRollWaves * 64), 0, st, Q, big_windows, big_base,
                           params, O, n_small);
    const int width = kRollRow + 2 * horizon;
    hipLaunchKernelGGL(mlapm_rollout_reduce_kernel, dim3(1), dim3(256), 0, st, workspace, n_small + n_big, width,
                       per_step ? width : kRollRow, loss, grad, per_step);
    return hipGetLastError();
}
