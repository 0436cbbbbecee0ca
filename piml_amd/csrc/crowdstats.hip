// Crowd-dynamics statistics that need no agent pairing: the Gaussian local density of every focal agent (Helbing, Johansson
// and Al-Abideen 2007), per-frame occupancy / speed / density series, the speed-density relation (fundamental diagram) in
// density bins and a density map, for S members x T' frames in one call.
//
// Density pass (crowd_density_kernel): one workgroup of 256 lanes per (member, frame) slice, grid-stride over the slices.
// Agent per lane: the workgroup walks the slice's slots below the member's bound in chunks of 256 focal candidates (slot
// c0 + lane), and for each chunk sweeps the slice's present agents, staged in LDS tiles of CD_TILE slots compacted in slot
// order (absent slots are never staged).  Every lane sums exp(-d^2 / R^2) over the staged sources in slot order into a
// float64 accumulator, so a focal agent's density depends on nothing but the slice's present positions: not on the bound,
// the member count, the chunk or the tile.  A slice with at most CD_TILE slots below its bound is staged once.
// The epilogue of a chunk computes speed, density bin and map cell; per lane series terms accumulate in registers, the
// fundamental diagram per wave into LDS rows (one wave-wide float64 butterfly per distinct bin present in the wave), the map
// through 64-bit integer atomics.  At the end of the slice the series are reduced over the lanes (butterfly, then the
// waves in order) and written, and the diagram's per-bin sums of the slice go to a fixed workspace slot.
// Reduce pass (crowd_fd_reduce_kernel): one workgroup per (member, bin) sums its T' slots in a fixed tree (lane strides over
// the frames, butterfly, waves in order).  No float atomics anywhere: two calls give the same bits, and member m of an
// S-member call gives the bits of an S = 1 call on that member alone.
// The statistics pass exists twice from one body (crowd_density_body): crowd_density_kernel as above, and
// crowd_given_density_kernel, which takes every agent's density from a.rho_in (voronoi.hip fills it) and neither stages
// nor sweeps.  The shared declarations and the host half both entries use are in crowdstats.hpp.
#include "crowdstats.hpp"
#include "../../include/piml_hip.h"

#include <cmath>

namespace piml {

__device__ __forceinline__ double cd_sweep(const float2* src, int cnt, float2 pi, float inv_r2) {
    double acc = 0.0;
#pragma unroll 4
    for (int k = 0; k < cnt; ++k) {
        const float2 q = src[k];
        const float dx = q.x - pi.x, dy = q.y - pi.y;
        acc += (double)expf(-((dx * dx + dy * dy) * inv_r2));
    }
    return acc;
}

// The statistics pass.  GIVEN: every agent's density was computed beforehand (a.rho_in, NaN where the agent is to be left
// out); nothing is staged or swept, everything else is the same code.
template <bool GIVEN>
__device__ __forceinline__ void crowd_density_body(const CrowdArgs& a) {
    __shared__ float2 src[GIVEN ? 1 : CD_TILE];
    __shared__ int wave_cnt[CD_WAVES];
    __shared__ double w_sum[CD_WAVES][CD_MAX_BINS], w_sum2[CD_WAVES][CD_MAX_BINS];
    __shared__ int w_cnt[CD_WAVES][CD_MAX_BINS];
    __shared__ double red_d[2][CD_WAVES];
    __shared__ long long red_i[2][CD_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, B = a.B;
    const long long slices = (long long)a.S * a.Tp;
    for (long long sl = blockIdx.x; sl < slices; sl += gridDim.x) {
        const int s = (int)(sl / a.Tp), tp = (int)(sl - (long long)s * a.Tp);
        const long long frame = (long long)s * a.T + a.t0 + tp;
        const float2* P = reinterpret_cast<const float2*>(a.P) + frame * a.N;
        const float2* V = reinterpret_cast<const float2*>(a.V) + frame * a.N;
        const float* M = a.M + frame * a.N;
        int bound = a.N;
        if (a.n_active) bound = min(max(a.n_active[s], 0), a.N);
        for (int k = tid; k < CD_WAVES * B; k += CD_THREADS) {
            (&w_sum[0][0])[(k / B) * CD_MAX_BINS + k % B] = 0.0;
            (&w_sum2[0][0])[(k / B) * CD_MAX_BINS + k % B] = 0.0;
            (&w_cnt[0][0])[(k / B) * CD_MAX_BINS + k % B] = 0;
        }
        const bool one_tile = GIVEN || bound <= CD_TILE;
        int cnt = 0;
        if constexpr (GIVEN)
            __syncthreads();                  // the zeroing
        else
            cnt = one_tile ? cd_stage(P, M, 0, bound, src, wave_cnt) : 0;     // (its barriers also cover the zeroing)
        long long n_focal = 0, n_spd = 0;
        double s_speed = 0.0, s_dens = 0.0;
        for (int c0 = 0; c0 < bound; c0 += CD_THREADS) {
            const int i = c0 + tid;
            float2 pi = make_float2(0.f, 0.f);
            bool focal = false;
            if (i < bound) {
                pi = P[i];
                focal = cd_present(M[i], pi) && in_box(a.has_box, a.x0, a.x1, a.y0, a.y1, pi);
            }
            float rho_given = 0.f;
            if constexpr (GIVEN) {
                if (focal) rho_given = a.rho_in[sl * a.N + i];
                focal = focal && !isnan(rho_given);
            }
            if (!__syncthreads_or(focal)) {
                if (a.density && i < a.N) a.density[sl * a.N + i] = NAN;
                continue;
            }
            double acc = 0.0;
            if (!GIVEN && one_tile) {
                acc = cd_sweep(src, cnt, pi, a.inv_r2);
            } else if (!GIVEN) {
                for (int lo = 0; lo < bound; lo += CD_TILE) {
                    cnt = cd_stage(P, M, lo, min(lo + CD_TILE, bound), src, wave_cnt);
                    acc += cd_sweep(src, cnt, pi, a.inv_r2);
                    __syncthreads();          // every lane is done with this tile before the next one is staged
                }
            }
            // epilogue: density, speed, bin, cell
            const float rho = GIVEN ? rho_given : (float)(acc / a.area);
            int bin = -1;
            float u = 0.f;
            if (focal) {
                const float2 v = V[i];
                ++n_focal;
                s_dens += (double)rho;
                if (isfinite(v.x) && isfinite(v.y)) {
                    u = sqrtf(v.x * v.x + v.y * v.y);
                    const float q = floorf(rho / a.rho_bin);
                    bin = q >= (float)(B - 1) ? B - 1 : (int)q;
                    ++n_spd;
                    s_speed += (double)u;
                }
                if (a.has_box) {
                    const float cx = floorf((pi.x - a.x0) / a.cell), cy = floorf((pi.y - a.y0) / a.cell);
                    if (a.map && cx >= 0.f && cx < (float)a.gx && cy >= 0.f && cy < (float)a.gy)
                        atomicAdd(reinterpret_cast<unsigned long long*>(a.map) +
                                      ((long long)s * a.gy + (int)cy) * a.gx + (int)cx, 1ull);
                }
            }
            if (a.density && i < a.N) a.density[sl * a.N + i] = focal ? rho : NAN;
            // the diagram: one butterfly per distinct bin of the wave, added to the wave's own LDS row in chunk order
            u64 pending = __ballot(bin >= 0);
            while (pending) {
                const int bb = __shfl(bin, (int)__builtin_ctzll(pending), 64);
                const bool mine = bin == bb;
                const u64 mm = __ballot(mine);
                const double su = wave_sum(mine ? (double)u : 0.0);
                const double su2 = wave_sum(mine ? (double)u * (double)u : 0.0);
                if (lane == 0) {
                    w_sum[w][bb] += su;
                    w_sum2[w][bb] += su2;
                    w_cnt[w][bb] += __popcll(mm);
                }
                pending &= ~mm;
            }
        }
        if (a.density)
            for (int i = max(bound, 0) + tid; i < a.N; i += CD_THREADS) a.density[sl * a.N + i] = NAN;
        // the slice's series: lanes in butterfly order, then the waves in order
        n_focal = wave_sum(n_focal);
        n_spd = wave_sum(n_spd);
        s_speed = wave_sum(s_speed);
        s_dens = wave_sum(s_dens);
        if (lane == 0) {
            red_i[0][w] = n_focal;
            red_i[1][w] = n_spd;
            red_d[0][w] = s_speed;
            red_d[1][w] = s_dens;
        }
        __syncthreads();
        if (tid == 0) {
            long long t0 = 0, t1 = 0;
            double d0 = 0.0, d1 = 0.0;
            for (int k = 0; k < CD_WAVES; ++k) {
                t0 += red_i[0][k];
                t1 += red_i[1][k];
                d0 += red_d[0][k];
                d1 += red_d[1][k];
            }
            a.n[sl] = t0;
            a.n_speed[sl] = t1;
            a.sum_speed[sl] = d0;
            a.sum_density[sl] = d1;
        }
        for (int b = tid; b < B; b += CD_THREADS) {
            double su = 0.0, su2 = 0.0;
            int c = 0;
            for (int k = 0; k < CD_WAVES; ++k) {
                su += w_sum[k][b];
                su2 += w_sum2[k][b];
                c += w_cnt[k][b];
            }
            a.ws_sum[sl * B + b] = su;
            a.ws_sum2[sl * B + b] = su2;
            a.ws_count[sl * B + b] = c;
        }
        __syncthreads();                      // LDS rows and red_* are reused by the next slice
    }
}

__global__ void __launch_bounds__(CD_THREADS) crowd_density_kernel(CrowdArgs a) { crowd_density_body<false>(a); }
__global__ void __launch_bounds__(CD_THREADS) crowd_given_density_kernel(CrowdArgs a) { crowd_density_body<true>(a); }

__global__ void __launch_bounds__(CD_THREADS) crowd_fd_reduce_kernel(CrowdArgs a) {
    __shared__ double red[2][CD_WAVES];
    __shared__ long long red_c[CD_WAVES];
    const int s = blockIdx.x / a.B, b = blockIdx.x % a.B;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    double su = 0.0, su2 = 0.0;
    long long c = 0;
    for (int tp = tid; tp < a.Tp; tp += CD_THREADS) {
        const long long k = ((long long)s * a.Tp + tp) * a.B + b;
        su += a.ws_sum[k];
        su2 += a.ws_sum2[k];
        c += a.ws_count[k];
    }
    su = wave_sum(su);
    su2 = wave_sum(su2);
    c = wave_sum(c);
    if (lane == 0) {
        red[0][w] = su;
        red[1][w] = su2;
        red_c[w] = c;
    }
    __syncthreads();
    if (tid == 0) {
        double t0 = 0.0, t1 = 0.0;
        long long tc = 0;
        for (int k = 0; k < CD_WAVES; ++k) {
            t0 += red[0][k];
            t1 += red[1][k];
            tc += red_c[k];
        }
        a.fd_count[blockIdx.x] = tc;
        a.fd_sum[blockIdx.x] = t0;
        a.fd_sum2[blockIdx.x] = t1;
    }
}

long long cd_workspace_bytes(long long slices, int B) { return slices * B * (long long)(2 * sizeof(double) + sizeof(int)); }

hipError_t cd_prepare(CrowdArgs& a, const float* P, const float* V, const float* M, const int* n_active, int S, int T, int N,
                      int t0, int t1, int has_box, float x0, float x1, float y0, float y1, float cell, int gx, int gy,
                      float rho_bin, int rho_bins, long long* n, long long* n_speed, double* sum_speed, double* sum_density,
                      long long* fd_count, double* fd_sum, double* fd_sum2, long long* map, float* density, void* workspace,
                      long long workspace_bytes, long long extra_bytes, void** extra) {
    if (S <= 0 || T <= 0 || N <= 0 || t0 < 0 || t1 > T || t1 <= t0 || !(rho_bin > 0.f) || !std::isfinite(rho_bin) ||
        rho_bins < 1 || rho_bins > CD_MAX_BINS)
        return hipErrorInvalidValue;
    if (has_box && (!std::isfinite(x0) || !std::isfinite(x1) || !std::isfinite(y0) || !std::isfinite(y1) || !(x0 < x1) ||
                    !(y0 < y1) || !(cell > 0.f) || !std::isfinite(cell) || gx < 1 || gy < 1 || !map))
        return hipErrorInvalidValue;
    if (!P || !V || !M || !n || !n_speed || !sum_speed || !sum_density || !fd_count || !fd_sum || !fd_sum2 || !workspace)
        return hipErrorInvalidValue;
    const int Tp = t1 - t0;
    const long long slices = (long long)S * Tp;
    if (workspace_bytes < cd_workspace_bytes(slices, rho_bins) + extra_bytes) return hipErrorInvalidValue;
    a = CrowdArgs{};
    a.P = P, a.V = V, a.M = M, a.n_active = n_active;
    a.S = S, a.T = T, a.N = N, a.t0 = t0, a.Tp = Tp, a.B = rho_bins;
    a.rho_bin = rho_bin;
    a.has_box = has_box ? 1 : 0, a.gx = gx, a.gy = gy;
    a.x0 = x0, a.x1 = x1, a.y0 = y0, a.y1 = y1, a.cell = cell;
    a.n = n, a.n_speed = n_speed, a.sum_speed = sum_speed, a.sum_density = sum_density;
    a.map = has_box ? map : nullptr;
    a.density = density;
    a.ws_sum = static_cast<double*>(workspace);
    a.ws_sum2 = a.ws_sum + slices * rho_bins;
    a.ws_count = reinterpret_cast<int*>(a.ws_sum2 + slices * rho_bins);
    a.fd_count = fd_count, a.fd_sum = fd_sum, a.fd_sum2 = fd_sum2;
    if (extra) *extra = a.ws_count + slices * rho_bins;
    return hipSuccess;
}

hipError_t cd_run(const CrowdArgs& a, bool given_density, hipStream_t st) {
    const long long slices = (long long)a.S * a.Tp;
    if (a.map) {
        const hipError_t e = hipMemsetAsync(a.map, 0, (size_t)a.S * a.gy * a.gx * sizeof(long long), st);
        if (e != hipSuccess) return e;
    }
    const dim3 grid((unsigned)(slices < CD_MAX_GRID ? slices : CD_MAX_GRID));
    if (given_density)
        hipLaunchKernelGGL(crowd_given_density_kernel, grid, dim3(CD_THREADS), 0, st, a);
    else
        hipLaunchKernelGGL(crowd_density_kernel, grid, dim3(CD_THREADS), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(crowd_fd_reduce_kernel, dim3((unsigned)(a.S * a.B)), dim3(CD_THREADS), 0, st, a);
    return hipGetLastError();
}

}  // namespace piml

using namespace piml;

PIML_API long long piml_crowd_stats_workspace_bytes(int S, int frames, int rho_bins) {
    if (S < 0 || frames < 0 || rho_bins < 0) return -1;
    return cd_workspace_bytes((long long)S * frames, rho_bins);
}

PIML_API int piml_crowd_stats(const float* P, const float* V, const float* M, const int* n_active, int S, int T, int N,
                              int t0, int t1, float radius, int has_box, float x0, float x1, float y0, float y1, float cell,
                              int gx, int gy, float rho_bin, int rho_bins, long long* n, long long* n_speed,
                              double* sum_speed, double* sum_density, long long* fd_count, double* fd_sum, double* fd_sum2,
                              long long* map, float* density, void* workspace, long long workspace_bytes, void* stream) {
    if (!(radius > 0.f) || !std::isfinite(radius)) return hipErrorInvalidValue;
    CrowdArgs a;
    const hipError_t e = cd_prepare(a, P, V, M, n_active, S, T, N, t0, t1, has_box, x0, x1, y0, y1, cell, gx, gy, rho_bin,
                                    rho_bins, n, n_speed, sum_speed, sum_density, fd_count, fd_sum, fd_sum2, map, density,
                                    workspace, workspace_bytes, 0, nullptr);
    if (e != hipSuccess) return e;
    a.inv_r2 = 1.f / (radius * radius);
    a.area = M_PI * (double)radius * (double)radius;
    return cd_run(a, false, as_stream(stream));
}
