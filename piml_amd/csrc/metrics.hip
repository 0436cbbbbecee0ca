// Evaluation metrics per frame: entropic OT (log-domain Sinkhorn) and multi-kernel Gaussian MMD, every frame of an
// evaluation in ONE launch each, one workgroup per frame.
//
// Reference: src/functions/metrics.py:45-104 (ot_with_time_mask, mmd_with_time_mask, wasserstein_distance_2d, mmd_loss) and
// the two classes behind them, SinkhornDistance.forward (:129-187) and MaximumMeanDiscrepancy (:207-273).  The reference
// compacts the present agents of a frame (p[mask == 1]) and runs its Python loop of ~10 library launches per Sinkhorn
// iteration, with a host sync (err.item()) at the end of each; MMD builds five (n+m)^2 Gram matrices.  Here a workgroup
// compacts its frame's present points into LDS (absent slots are never read, so they may hold NaN), recomputes the cost
// C_ij = |x_i - y_j|^2 from LDS instead of storing it, and stops the frame where the reference's per-frame loop breaks.
//
// Numerics.  Sinkhorn is the reference's float32 arithmetic entry by entry: M_ij = ((-C_ij + u_i) + v_j) / eps as a true
// division, each log-sum-exp max-first as torch evaluates it (log(sum(exp(M - max))) + max, max := 0 when infinite), accurate
// expf / logf.  Only the order of the float32 sums differs (64-lane strided partials, then a butterfly).  The final cost
// sum(exp(M) * C) is accumulated in float64.  MMD is float64 from the float32 positions on: XX + YY - XY - YX cancels ~4
// digits (block sums ~5 against a result ~1e-3), so a float32 evaluation carries ~4e-5 of rounding in its result.
// Every sum runs in a fixed order (no atomics): two runs give the same bits.
#include "common.hpp"
#include "../../include/piml_hip.h"

#include <cmath>

namespace piml {

constexpr int MET_MAX_POINTS = 4096;
constexpr int MET_MAX_WAVES = 16;
constexpr int MET_MAX_KERNELS = 8;

// 4 waves for small frames (each wave owns whole rows), up to 16 so a 4096-point frame has 4 waves per SIMD to hide the
// 8-cycle v_exp_f32 / v_log_f32 behind one another
static int metric_threads(int n, int m) {
    const int p = n > m ? n : m;
    const int t = (p + 63) / 64 * 64;
    return t < 256 ? 256 : (t > 1024 ? 1024 : t);
}


// f(slot, compacted index or -1) for every slot of an n-point frame, in slot order; returns the number of present slots.
// `wave_cnt` is MET_MAX_WAVES ints of LDS; every thread of the workgroup must call it.
template <class Fn>
__device__ int for_slots(const unsigned char* mask, int n, int* wave_cnt, Fn f) {
    const int tid = threadIdx.x, w = tid >> 6, W = blockDim.x >> 6;
    int base = 0;
    for (int s0 = 0; s0 < n; s0 += blockDim.x) {
        const int s = s0 + tid;
        const bool present = s < n && (mask == nullptr || mask[s] != 0);
        const u64 b = __ballot(present);
        if ((tid & 63) == 0) wave_cnt[w] = __popcll(b);
        __syncthreads();
        int before = base, total = base;
        for (int k = 0; k < W; ++k) {
            before += k < w ? wave_cnt[k] : 0;
            total += wave_cnt[k];
        }
        if (s < n) f(s, present ? before + (int)mbcnt(b) : -1);
        __syncthreads();                      // wave_cnt is rewritten by the next chunk
        base = total;
    }
    return base;
}

__device__ __forceinline__ int compact(const float* pts, const unsigned char* mask, int n, float2* out, int* wave_cnt) {
    return for_slots(mask, n, wave_cnt, [&](int s, int k) {
        if (k >= 0) out[k] = make_float2(pts[2 * s], pts[2 * s + 1]);
    });
}

// fixed-order sum over the waves of the workgroup of one value per wave (lane 0's); every thread returns the total
__device__ __forceinline__ double block_sum_d(double x, double* red) {
    const int w = threadIdx.x >> 6, W = blockDim.x >> 6;
    x = wave_sum(x);
    __syncthreads();                          // red may still be read by a previous call
    if ((threadIdx.x & 63) == 0) red[w] = x;
    __syncthreads();
    double t = 0.0;
    for (int k = 0; k < W; ++k) t += red[k];
    return t;
}

// ---------------------------------------------------------------------------------------------------------------------
// Sinkhorn
struct SinkArgs {
    const float *x, *y;                       // (F, n, 2), (F, m, 2)
    const unsigned char *mx, *my;             // (F, n), (F, m) or NULL = all present
    int n, m, max_iter;
    float eps, thresh;
    float* cost;                              // (F)
    int* iters;                               // (F)
    float *u, *v;                             // (F, n), (F, m) or NULL
};

// M_ij = ((-C_ij + u_i) + v_j) / eps with C_ij = |dx|^2 + |dy|^2 (SinkhornDistance.M and _cost_matrix, float32)
__device__ __forceinline__ float cost_entry(float2 a, float2 b) {
    const float dx = a.x - b.x, dy = a.y - b.y;
    return dx * dx + dy * dy;
}
__device__ __forceinline__ float m_entry(float c, float ui, float vj, float eps) { return ((-c + ui) + vj) / eps; }

// torch.logsumexp over a row (or column) whose entries one wave visits 64 apart: the max first (max := 0 when infinite),
// then log(sum(exp(M - max))) + max.  A NaN entry reaches the sum through exp even where fmaxf skipped it.
template <class Entry>
__device__ __forceinline__ float wave_lse(int len, Entry entry) {
    const int lane = threadIdx.x & 63;
    float mx = -INFINITY;
    for (int j = lane; j < len; j += 64) mx = fmaxf(mx, entry(j));
    mx = wave_max(mx);
    if (isinf(mx)) mx = 0.f;
    float s = 0.f;
    for (int j = lane; j < len; j += 64) s += expf(entry(j) - mx);
    return logf(wave_sum(s)) + mx;
}

__global__ void __launch_bounds__(1024) sinkhorn_frames_kernel(SinkArgs a) {
    extern __shared__ __attribute__((aligned(16))) float met_lds[];
    __shared__ int wave_cnt[MET_MAX_WAVES];
    __shared__ float err_part[2][MET_MAX_WAVES];
    __shared__ double red[MET_MAX_WAVES];
    float2* X = reinterpret_cast<float2*>(met_lds);
    float2* Y = X + a.n;
    float* U = reinterpret_cast<float*>(Y + a.m);
    float* V = U + a.n;
    const long long f = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, W = blockDim.x >> 6;
    const unsigned char* mx = a.mx ? a.mx + f * a.n : nullptr;
    const unsigned char* my = a.my ? a.my + f * a.m : nullptr;
    const int n = compact(a.x + f * a.n * 2, mx, a.n, X, wave_cnt);
    const int m = compact(a.y + f * a.m * 2, my, a.m, Y, wave_cnt);
    for (int i = tid; i < n; i += blockDim.x) U[i] = 0.f;
    for (int j = tid; j < m; j += blockDim.x) V[j] = 0.f;
    __syncthreads();
    const float eps = a.eps;
    // log(mu + 1e-8), mu = fill_(1.0 / points) in float32
    const float lmu = logf((float)(1.0 / n) + 1e-8f), lnu = logf((float)(1.0 / m) + 1e-8f);
    int it = 0;
    while (it < a.max_iter) {
        // row half: u_i = eps * (log mu - lse_j M_ij) + u_i, each wave a row at a time
        float e = 0.f;
        for (int i = w; i < n; i += W) {
            const float2 xi = X[i];
            const float ui = U[i];
            const float lse = wave_lse(m, [&](int j) { return m_entry(cost_entry(xi, Y[j]), ui, V[j], eps); });
            const float un = eps * (lmu - lse) + ui;
            e += fabsf(un - ui);
            if (lane == 0) U[i] = un;
        }
        if (lane == 0) err_part[it & 1][w] = e;      // double-buffered: a wave may run ahead into the next iteration
        __syncthreads();
        // column half on the new u
        for (int j = w; j < m; j += W) {
            const float2 yj = Y[j];
            const float vj = V[j];
            const float lse = wave_lse(n, [&](int i) { return m_entry(cost_entry(X[i], yj), U[i], vj, eps); });
            if (lane == 0) V[j] = eps * (lnu - lse) + vj;
        }
        __syncthreads();
        float err = 0.f;
        for (int k = 0; k < W; ++k) err += err_part[it & 1][k];
        ++it;
        if (err < a.thresh) break;                   // uniform: every thread summed the same partials in the same order
    }
    // cost = sum_ij exp(M_ij) * C_ij, the products in float32 (pi * C), the sum in float64
    double acc = 0.0;
    for (int i = w; i < n; i += W) {
        const float2 xi = X[i];
        const float ui = U[i];
        for (int j = lane; j < m; j += 64) {
            const float c = cost_entry(xi, Y[j]);
            acc += (double)(expf(m_entry(c, ui, V[j], eps)) * c);
        }
    }
    acc = block_sum_d(acc, red);
    if (tid == 0) {
        a.cost[f] = (float)acc;
        a.iters[f] = it;
    }
    if (a.u) for_slots(mx, a.n, wave_cnt, [&](int s, int k) { a.u[f * a.n + s] = k >= 0 ? U[k] : 0.f; });
    if (a.v) for_slots(my, a.m, wave_cnt, [&](int s, int k) { a.v[f * a.m + s] = k >= 0 ? V[k] : 0.f; });
}

// ---------------------------------------------------------------------------------------------------------------------
// MMD
struct MmdArgs {
    const float *x, *y;
    const unsigned char *mx, *my;
    int n, m, kernel_num;
    double pow_mul[MET_MAX_KERNELS];          // kernel_mul ** i, as Python evaluates it (host pow)
    double div_mul;                           // kernel_mul ** (kernel_num // 2)
    double fix_sigma;                         // 0 = the bandwidth of the data (Python truthiness of fix_sigma)
    float* out;                               // (F)
};

__device__ __forceinline__ double l2_d(float2 a, float2 b) {
    const double dx = (double)a.x - (double)b.x, dy = (double)a.y - (double)b.y;
    return dx * dx + dy * dy;
}

__global__ void __launch_bounds__(1024) mmd_frames_kernel(MmdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float met_lds[];
    __shared__ int wave_cnt[MET_MAX_WAVES];
    __shared__ double red[MET_MAX_WAVES];
    float2* P = reinterpret_cast<float2*>(met_lds);    // [x present | y present], guassian_kernel's `total`
    const long long f = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, W = blockDim.x >> 6;
    const int n = compact(a.x + f * a.n * 2, a.mx ? a.mx + f * a.n : nullptr, a.n, P, wave_cnt);
    const int m = compact(a.y + f * a.m * 2, a.my ? a.my + f * a.m : nullptr, a.m, P + n, wave_cnt);
    __syncthreads();
    const int N = n + m;
    // pass 1: bandwidth = sum L2 / (N^2 - N) over the full symmetric (N, N) matrix = 2 x the upper triangle
    double bw = a.fix_sigma;
    if (bw == 0.0) {
        double s = 0.0;
        for (int i = w; i < N; i += W) {
            const float2 pi = P[i];
            for (int j = i + 1 + lane; j < N; j += 64) s += l2_d(pi, P[j]);
        }
        s = block_sum_d(s, red);
        bw = 2.0 * s / ((double)N * N - N);
    }
    bw /= a.div_mul;
    double neg_inv[MET_MAX_KERNELS];                    // -1 / bandwidth_i (unrolled: stays in registers)
#pragma unroll
    for (int k = 0; k < MET_MAX_KERNELS; ++k) neg_inv[k] = -1.0 / (bw * a.pow_mul[k]);
    const int kn = a.kernel_num;
    auto kern = [&](double l2) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < MET_MAX_KERNELS; ++k)
            if (k < kn) s += exp(l2 * neg_inv[k]);
        return s;
    };
    // pass 2: the strict upper triangle by block; K is symmetric, so YX = XY and the diagonal blocks are 2 x their upper
    // triangle + their diagonal (K(0): kernel_num, or NaN when the bandwidth is 0 or NaN, as in the reference)
    double sxx = 0.0, sxy = 0.0, syy = 0.0;
    for (int i = w; i < N; i += W) {
        const float2 pi = P[i];
        for (int j = i + 1 + lane; j < N; j += 64) {
            const double k = kern(l2_d(pi, P[j]));
            if (j < n) sxx += k;
            else if (i < n) sxy += k;
            else syy += k;
        }
    }
    sxx = block_sum_d(sxx, red);
    sxy = block_sum_d(sxy, red);
    syy = block_sum_d(syy, red);
    if (tid == 0) {
        const double kd = kern(0.0), dn = n, dm = m;
        // an empty block contributes nothing (the reference sums empty slices)
        const double xx = n ? (dn * kd + 2.0 * sxx) / (dn * dn) : 0.0;
        const double yy = m ? (dm * kd + 2.0 * syy) / (dm * dm) : 0.0;
        const double xy = n && m ? sxy / (dn * dm) : 0.0;
        a.out[f] = (float)(xx + yy - 2.0 * xy);
    }
}

static size_t points_lds(int n, int m, int floats_per_point) { return (size_t)(n + m) * floats_per_point * sizeof(float); }

template <class K>
static hipError_t allow_lds(K kernel, size_t bytes) {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

}  // namespace piml

using namespace piml;

PIML_API int piml_sinkhorn_frames(const float* x, const float* y, const unsigned char* mask_x, const unsigned char* mask_y,
                                  int F, int n, int m, float eps, int max_iter, float thresh, float* cost, int* iters,
                                  float* u, float* v, void* stream) {
    if (F < 0 || n < 0 || m < 0 || n > MET_MAX_POINTS || m > MET_MAX_POINTS || !(eps > 0.f) || max_iter < 0)
        return hipErrorInvalidValue;
    if (F == 0) return hipSuccess;
    if ((n && !x) || (m && !y) || !cost || !iters) return hipErrorInvalidValue;
    static hipError_t attr = allow_lds(sinkhorn_frames_kernel, points_lds(MET_MAX_POINTS, MET_MAX_POINTS, 3));
    if (attr != hipSuccess) return attr;
    SinkArgs A{x, y, mask_x, mask_y, n, m, max_iter, eps, thresh, cost, iters, u, v};
    hipLaunchKernelGGL(sinkhorn_frames_kernel, dim3((unsigned)F), dim3(metric_threads(n, m)), points_lds(n, m, 3),
                       as_stream(stream), A);
    return hipGetLastError();
}

PIML_API int piml_mmd_frames(const float* x, const float* y, const unsigned char* mask_x, const unsigned char* mask_y,
                             int F, int n, int m, double kernel_mul, int kernel_num, double fix_sigma, float* out,
                             void* stream) {
    if (F < 0 || n < 0 || m < 0 || n > MET_MAX_POINTS || m > MET_MAX_POINTS || kernel_num < 1 ||
        kernel_num > MET_MAX_KERNELS)
        return hipErrorInvalidValue;
    if (F == 0) return hipSuccess;
    if ((n && !x) || (m && !y) || !out) return hipErrorInvalidValue;
    static hipError_t attr = allow_lds(mmd_frames_kernel, points_lds(MET_MAX_POINTS, MET_MAX_POINTS, 2));
    if (attr != hipSuccess) return attr;
    MmdArgs A{};
    A.x = x, A.y = y, A.mx = mask_x, A.my = mask_y, A.n = n, A.m = m, A.kernel_num = kernel_num, A.out = out;
    for (int k = 0; k < kernel_num; ++k) A.pow_mul[k] = std::pow(kernel_mul, (double)k);
    A.div_mul = std::pow(kernel_mul, (double)(kernel_num / 2));
    A.fix_sigma = fix_sigma;
    hipLaunchKernelGGL(mmd_frames_kernel, dim3((unsigned)F), dim3(metric_threads(n, m)), points_lds(n, m, 2),
                       as_stream(stream), A);
    return hipGetLastError();
}
