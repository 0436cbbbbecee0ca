// Calibration of MLAPM's six constants (tau, A, B, C, D, theta) to a clip: the mean squared velocity residual of one
// MLAPM.step per (frame, agent) and its analytic gradient with respect to the constants, in one sweep over the pairs.
//
// The clip arrives packed frame-major (piml_amd/calibrate.py pack_clip): entry e = one agent present in one frame, the
// entries of frame f are [offsets[f], offsets[f + 1]) and they are also that frame's sources (as with skip_absent).
// Focal entries -- the ones with a finite target -- come in two lists, by the size n of their frame:
//   n <= 64  mlapm_fit_lane_kernel: one LANE per focal entry, 256 consecutive focal entries per workgroup (a recorded
//            GC frame holds ~21 agents: a wave per focal agent would leave two thirds of its lanes idle);
//   n >  64  mlapm_fit_wave_kernel: one WAVE per focal entry, the lanes stride over the frame's sources, wave sums (the
//            decomposition of mlapm_fwd_kernel, for open-world clips with hundreds to thousands of agents per frame).
// Both write one float64 row of 8 per workgroup (weight, squared residual, 6 gradients), the focal values converted to
// float64 and summed in a fixed order; mlapm_fit_reduce_kernel (ONE workgroup, a second launch) adds the rows in a fixed
// order.  No atomics: the result is bitwise reproducible.  The constants are read from device memory, so a whole fit
// iteration (this + an optimiser update of the same 6-vector) can be captured once and replayed.
#include "common.hpp"
#include "mlapm.hpp"
#include "../../include/piml_hip.h"

#include <cmath>

namespace piml {

constexpr int kFitRow = 8;        // weight, sum |r|^2, d/d(tau, A, B, C, D, theta)
constexpr int kFitLaneBlock = 256;
constexpr int kFitWaves = 4;

struct FitPack {
    const float4* state;          // (E) px, py, vx, vy
    const float2* dest;           // (E)
    const float* v0;              // (E)
    const float2* target;         // (E)
    const int* offsets;           // (F + 1)
    const int* frame_of;          // (E)
    int E, F;
};

// One focal entry's row: prediction v + dt ((v0 e - v) / tau - A U) (mlapm.py:21-22, :57), residual against the target,
// and 2 r . d pred / d param, in float64 from the float32 sums.  Unused constants get exactly 0.
__device__ __forceinline__ void fit_focal_row(const FitConst& K, float dt, float4 s, float2 d, float v0, float2 tg,
                                              float ex, float ey, const FitAcc& a, double* row) {
    const float fdx = (v0 * ex - s.z) / K.tau, fdy = (v0 * ey - s.w) / K.tau;
    const float px = s.z + (fdx - K.A * a.ux) * dt, py = s.w + (fdy - K.A * a.uy) * dt;
    const double rx = (double)px - (double)tg.x, ry = (double)py - (double)tg.y;
    const double ddt = dt, A = K.A;
    row[0] = 1.0;
    row[1] = rx * rx + ry * ry;
    row[2] = 2.0 * ddt * (rx * (-(double)fdx) + ry * (-(double)fdy)) / (double)K.tau;          // d((v0 e - v)/tau)/dtau
    row[3] = -2.0 * ddt * (rx * a.ux + ry * a.uy);
    row[4] = -2.0 * ddt * A * (rx * a.bx + ry * a.by);
    row[5] = K.variant == 0 ? 0.0 : -2.0 * ddt * A * (rx * a.cx + ry * a.cy);
    row[6] = K.variant == 1 ? -2.0 * ddt * A * (rx * a.dx + ry * a.dy) : 0.0;
    row[7] = K.variant == 0 ? 0.0 : -2.0 * ddt * A * (rx * a.tx + ry * a.ty);
}

__device__ __forceinline__ void focal_setup(const FitPack& Q, int e, float4& s, float2& d, float& ex, float& ey) {
    s = Q.state[e]; d = Q.dest[e];
    ex = d.x - s.x; ey = d.y - s.y;
    const float en = fmaxf(norm2(ex, ey), 1e-12f);                  // :21, as mlapm_fwd_kernel
    ex /= en; ey /= en;
}

__device__ __forceinline__ bool frame_range(const FitPack& Q, int e, int& lo, int& hi) {
    const int f = Q.frame_of[e];
    if (f < 0 || f >= Q.F) return false;
    lo = max(Q.offsets[f], 0); hi = min(Q.offsets[f + 1], Q.E);
    return true;
}

// lanes = focal entries of frames with <= 64 agents
__global__ __launch_bounds__(kFitLaneBlock) void mlapm_fit_lane_kernel(FitPack Q, const int* __restrict__ focal, int n_focal,
                                                                       const float* __restrict__ params, int variant,
                                                                       float dt, float radius, double* __restrict__ part) {
    __shared__ double red[kFitLaneBlock / 64][kFitRow];
    const FitConst K = fit_const(params, variant, radius);
    const int k = blockIdx.x * kFitLaneBlock + threadIdx.x;
    double row[kFitRow] = {0, 0, 0, 0, 0, 0, 0, 0};
    int lo = 0, hi = 0;
    const int e = k < n_focal ? focal[k] : -1;
    if (e >= 0 && e < Q.E && frame_range(Q, e, lo, hi)) {
        const float2 tg = Q.target[e];
        if (tg.x == tg.x && tg.y == tg.y) {
            float4 s; float2 d; float ex, ey;
            focal_setup(Q, e, s, d, ex, ey);
            FitAcc a = {};
            for (int j = lo; j < hi; ++j) {
                if (j == e) continue;                               // the self pair has view = 0
                const float4 o = Q.state[j];
                fit_pair(K, o.x - s.x, o.y - s.y, o.z - s.z, o.w - s.w, s.z, s.w, ex, ey, a);
            }
            fit_focal_row(K, dt, s, d, Q.v0[e], tg, ex, ey, a, row);
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < kFitRow; ++q) {
        const double t = wave_sum_d(row[q]);
        if (lane == 0) red[wave][q] = t;
    }
    __syncthreads();
    if (threadIdx.x < kFitRow) {
        double t = 0.0;
        for (int w = 0; w < kFitLaneBlock / 64; ++w) t += red[w][threadIdx.x];
        part[(size_t)blockIdx.x * kFitRow + threadIdx.x] = t;
    }
}

// a wave per focal entry of frames with > 64 agents; the lanes stride over the sources
__global__ __launch_bounds__(kFitWaves * 64) void mlapm_fit_wave_kernel(FitPack Q, const int* __restrict__ focal, int n_focal,
                                                                        const float* __restrict__ params, int variant,
                                                                        float dt, float radius, double* __restrict__ part) {
    __shared__ double red[kFitWaves][kFitRow];
    const FitConst K = fit_const(params, variant, radius);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int k = blockIdx.x * kFitWaves + wave;
    double row[kFitRow] = {0, 0, 0, 0, 0, 0, 0, 0};
    int lo = 0, hi = 0;
    const int e = k < n_focal ? focal[k] : -1;
    if (e >= 0 && e < Q.E && frame_range(Q, e, lo, hi)) {
        const float2 tg = Q.target[e];
        if (tg.x == tg.x && tg.y == tg.y) {
            float4 s; float2 d; float ex, ey;
            focal_setup(Q, e, s, d, ex, ey);
            FitAcc a = {};
            for (int j = lo + lane; j < hi; j += 64) {
                if (j == e) continue;
                const float4 o = Q.state[j];
                fit_pair(K, o.x - s.x, o.y - s.y, o.z - s.z, o.w - s.w, s.z, s.w, ex, ey, a);
            }
            a.ux = wave_sum(a.ux); a.uy = wave_sum(a.uy);
            a.bx = wave_sum(a.bx); a.by = wave_sum(a.by);
            if (K.variant != 0) {
                a.cx = wave_sum(a.cx); a.cy = wave_sum(a.cy);
                a.tx = wave_sum(a.tx); a.ty = wave_sum(a.ty);
            }
            if (K.variant == 1) { a.dx = wave_sum(a.dx); a.dy = wave_sum(a.dy); }
            fit_focal_row(K, dt, s, d, Q.v0[e], tg, ex, ey, a, row);
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < kFitRow; ++q) red[wave][q] = row[q];
    }
    __syncthreads();
    if (threadIdx.x < kFitRow) {
        double t = 0.0;
        for (int w = 0; w < kFitWaves; ++w) t += red[w][threadIdx.x];
        part[(size_t)blockIdx.x * kFitRow + threadIdx.x] = t;
    }
}

// ONE workgroup: thread t adds rows t, t + 256, ... in order, then a fixed tree over the 256 threads
__global__ __launch_bounds__(256) void mlapm_fit_reduce_kernel(const double* __restrict__ part, int rows,
                                                               double* __restrict__ loss, float* __restrict__ grad) {
    __shared__ double red[kFitRow][256];
    double acc[kFitRow] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int r = threadIdx.x; r < rows; r += 256) {
#pragma unroll
        for (int q = 0; q < kFitRow; ++q) acc[q] += part[(size_t)r * kFitRow + q];
    }
#pragma unroll
    for (int q = 0; q < kFitRow; ++q) red[q][threadIdx.x] = acc[q];
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
#pragma unroll
            for (int q = 0; q < kFitRow; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + h];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double w = red[0][0];
        const double inv = w > 0.0 ? 1.0 / w : 0.0;                 // no focal entry: loss and gradient 0
        *loss = red[1][0] * inv;
        for (int q = 0; q < 6; ++q) grad[q] = (float)(red[2 + q][0] * inv);
    }
}

static long long fit_rows(int n_small, int n_big) {
    return (long long)(n_small + kFitLaneBlock - 1) / kFitLaneBlock + (long long)(n_big + kFitWaves - 1) / kFitWaves;
}

}  // namespace piml

using namespace piml;

PIML_API long long piml_mlapm_fit_workspace_doubles(int n_small, int n_big) {
    if (n_small < 0 || n_big < 0) return -1;
    return fit_rows(n_small, n_big) * kFitRow;
}

PIML_API int piml_mlapm_fit_loss_grad(const float* state, const float* destination, const float* desired_speed,
                                      const float* target, const int* offsets, const int* frame_of, int E, int F,
                                      const int* small_focal, int n_small, const int* big_focal, int n_big,
                                      const float* params, int variant, float dt, float radius, double* workspace,
                                      long long workspace_doubles, double* loss, float* grad, void* stream) {
    if (E < 0 || F < 0 || n_small < 0 || n_big < 0 || (long long)n_small + n_big > E) return hipErrorInvalidValue;
    if (variant < 0 || variant > 2 || !std::isfinite(dt) || !std::isfinite(radius)) return hipErrorInvalidValue;
    if (!params || !loss || !grad) return hipErrorInvalidValue;
    if (E > 0 && (!state || !destination || !desired_speed || !target || !offsets || !frame_of)) return hipErrorInvalidValue;
    if ((n_small > 0 && !small_focal) || (n_big > 0 && !big_focal)) return hipErrorInvalidValue;
    const long long rows = fit_rows(n_small, n_big);
    if (rows > 0 && (!workspace || workspace_doubles < rows * kFitRow)) return hipErrorInvalidValue;
    const FitPack Q = {(const float4*)state, (const float2*)destination, desired_speed, (const float2*)target, offsets,
                       frame_of, E, F};
    const int lane_blocks = (n_small + kFitLaneBlock - 1) / kFitLaneBlock;
    const int wave_blocks = (n_big + kFitWaves - 1) / kFitWaves;
    if (lane_blocks > 0)
        hipLaunchKernelGGL(mlapm_fit_lane_kernel, dim3(lane_blocks), dim3(kFitLaneBlock), 0, as_stream(stream), Q, small_focal,
                           n_small, params, variant, dt, radius, workspace);
    if (wave_blocks > 0)
        hipLaunchKernelGGL(mlapm_fit_wave_kernel, dim3(wave_blocks), dim3(kFitWaves * 64), 0, as_stream(stream), Q, big_focal,
                           n_big, params, variant, dt, radius, workspace + (size_t)lane_blocks * kFitRow);
    hipLaunchKernelGGL(mlapm_fit_reduce_kernel, dim3(1), dim3(256), 0, as_stream(stream), workspace, (int)rows, loss, grad);
    return hipGetLastError();
}
