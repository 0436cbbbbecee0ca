// Collective-motion statistics of crowds: the velocity-velocity correlation over distance, the lane-formation
// order parameter of Rex and Loewen (Phys. Rev. E 75, 051402, 2007) with the same / opposite counts that a chance level
// needs, and the velocity field on the cells of piml_crowd_stats, for S members in one call.
//
// Participant of slice (s, t): M == 1, both coordinates of P finite, both components of V finite and below 1024 in
// magnitude, slot below n_active[s].  Focal: a participant inside the optional box [x0, x1) x [y0, y1).  Mover: a participant
// with s = sqrt(vx^2 + vy^2) >= v_min; its heading h = v / s.  Lane mover: a participant with |v.e| >= v_min along the unit
// axis e; its direction is the sign of v.e.  Only same-frame pairs, float32 with true divisions and square roots and no
// contraction, d = p_j - p_i:
//   (a) every focal mover i against every mover j != i (as a slot) with r = sqrt(|d|^2) < r_max: bin floor(r / r_bin) (below
//       r_bins) counts the pair and adds llrintf((h_i.h_j) Q), Q = 2^20;
//   (b) every focal lane mover i counts the lane movers j != i with |d.e_perp| < lane_width and |d.e| < lane_length,
//       e_perp = (-e_y, e_x), as n_same (equal direction) or n_opp; with a non-empty band phi = ((n_same - n_opp) /
//       (n_same + n_opp))^2 and the slice adds llrintf(phi Q);
//   (c) every focal participant adds 1, llrintf(vx Q), llrintf(vy Q) to its cell (floor((x - x0) / cell), floor((y - y0) / cell))
//       when a box is given and the cell lies in the grid.
//
// flow_stats_kernel: one workgroup of 256 lanes per slice, a run of consecutive slices per workgroup.  The slice's
// participants are compacted in slot order into LDS tiles of FS_TILE sources (position and heading 16 B -- heading x NaN:
// not a mover --, v.e 4 B -- 0: not a lane mover --, slot 4 B); the focal agents are compacted too and taken one per lane in
// chunks of 256.  One sweep over the sources serves (a) and (b); a pair whose |d|^2 is beyond both r_max and the band's
// diagonal leaves it after the subtraction and the squares.  n_same / n_opp live in registers, the distance histogram in
// per-wave LDS rows (u32 counts, 64-bit sums: |q| <= 2^20 + 1 times up to 2^30 pairs does not fit 32 bits).  After a slice
// the waves' rows are added into the workgroup's 64-bit LDS accumulator, which goes to the member's workspace rows with
// 64-bit integer atomics when the member changes and at the end of the run; the per-slice series are written directly (one
// workgroup owns a slice); the map goes to the workspace with 64-bit integer atomics per focal agent.
// flow_stats_copy_kernel moves the workspace into the outputs.  Every output is an integer and every atomic an integer
// add, so the results are bitwise reproducible whatever the order of the adds.
//
// No u32 counter overflows: per slice a wave's bin holds at most (ceil(N / 256) * 64) * N <= 2^30 pairs for N <= FS_MAX_N,
// a lane's band at most N agents, and the u32 rows are folded into u64 after every slice.
#include "stats.hpp"
#include "../../include/piml_hip.h"

#include <cmath>

namespace piml {

constexpr int FS_THREADS = 256;
constexpr int FS_WAVES = FS_THREADS / 64;
constexpr int FS_TILE = 1024;                 // sources per LDS tile (24 KiB)
constexpr int FS_MAX_BINS = 256;
constexpr int FS_MAX_N = 65536;
constexpr float FS_Q = 1048576.f;             // 2^20
constexpr float FS_MAX_V = 1024.f;
constexpr long long FS_MAX_GRID = 1 << 20;
constexpr long long FS_TARGET_WG = 2048;      // runs are sized so that about this many workgroups start
constexpr int FS_MAX_RUN = 64;
constexpr int FS_SERIES = 6;                  // lane_n, lane_sum, lane_same, lane_opp, dir_plus, dir_minus

struct FlowArgs {
    const float *P, *V, *M;                   // (S, T, N, 2), (S, T, N, 2), (S, T, N)
    const int* n_active;                      // (S) or NULL
    int S, T, N, t0, Tp, RB, run, has_box, gx, gy;
    float v_min, r_bin, r_max, ex, ey, lane_width, lane_length, x0, x1, y0, y1, cell;
    float far2;                               // |d|^2 above this: beyond r_max and outside every band
    long long slices;
    unsigned long long* ws;                   // corr_pairs, corr_sum (S, RB) | map_n, map_vx, map_vy (S, gy, gx)
    long long *corr_pairs, *corr_sum;         // (S, RB)
    long long* series[FS_SERIES];             // (S, T')
    long long *map_n, *map_vx, *map_vy;       // (S, gy, gx) or NULL
};

__device__ __forceinline__ bool fs_participant(float m, float2 p, float2 v) {
    return m == 1.f && isfinite(p.x) && isfinite(p.y) && fabsf(v.x) < FS_MAX_V && fabsf(v.y) < FS_MAX_V;
}

struct FsAgent {
    float hx, hy;                             // heading; hx NaN: not a mover
    float ve;                                 // v.e; 0: not a lane mover
};

__device__ __forceinline__ FsAgent fs_agent(const FlowArgs& a, float2 v) {
    FsAgent g;
    const float s = sqrtf(v.x * v.x + v.y * v.y);
    const bool mover = s >= a.v_min;
    g.hx = mover ? v.x / s : NAN;
    g.hy = mover ? v.y / s : 0.f;
    const float ve = v.x * a.ex + v.y * a.ey;
    g.ve = fabsf(ve) >= a.v_min ? ve : 0.f;
    return g;
}

// Compacts the participants of slots [lo, hi) (hi - lo <= FS_TILE) into ph / ve / slot in slot order; returns their
// number (wg_compact: every thread calls it, and the tile may still be read on entry).
__device__ int fs_stage(const FlowArgs& a, const float2* P, const float2* V, const float* M, int lo, int hi, float4* ph,
                        float* ve, int* slot, int* wave_cnt) {
    float2 p, v;
    return wg_compact<FS_THREADS>(
        lo, hi, wave_cnt, [&](int j) { return p = P[j], v = V[j], fs_participant(M[j], p, v); },
        [&](int q, int j) {
            const FsAgent g = fs_agent(a, v);
            ph[q] = make_float4(p.x, p.y, g.hx, g.hy);
            ve[q] = g.ve;
            slot[q] = j;
        });
}

// The sweep of one focal agent (slot i at pi, heading / v.e in g) over cnt staged sources: (a) into the wave's rows, (b)
// into n_same / n_opp.
__device__ __forceinline__ void fs_sweep(const FlowArgs& a, const float4* ph, const float* ve, const int* slot, int cnt, int i,
                                         float2 pi, FsAgent g, unsigned* h_cnt, unsigned long long* h_sum, unsigned& n_same,
                                         unsigned& n_opp) {
    const float r_max = a.r_max, r_bin = a.r_bin, frb = (float)a.RB, far2 = a.far2;
    const float ex = a.ex, ey = a.ey, nex = -a.ey, lw = a.lane_width, ll = a.lane_length;
    const bool mover = !isnan(g.hx), lane = g.ve != 0.f, plus = g.ve > 0.f;
    for (int q = 0; q < cnt; ++q) {
        const float4 s = ph[q];
        const float vej = ve[q];
        if (slot[q] == i) continue;
        const float dx = s.x - pi.x, dy = s.y - pi.y;
        const float d2 = dx * dx + dy * dy;
        if (!(d2 <= far2)) continue;          // neither test below can pass (see piml_flow_stats): most pairs leave here
        if (lane && vej != 0.f) {
            const float across = dx * nex + dy * ex, along = dx * ex + dy * ey;
            if (fabsf(across) < lw && fabsf(along) < ll) {
                const bool same = (vej > 0.f) == plus;
                n_same += same ? 1u : 0u;
                n_opp += same ? 0u : 1u;
            }
        }
        if (mover && !isnan(s.z)) {
            const float r = sqrtf(d2);
            if (!(r < r_max)) continue;
            const float qd = floorf(r / r_bin);
            if (!(qd < frb)) continue;
            const float c = g.hx * s.z + g.hy * s.w;
            const long long qc = llrintf(c * FS_Q);
            atomicAdd(h_cnt + (int)qd, 1u);
            atomicAdd(h_sum + (int)qd, (unsigned long long)qc);
        }
    }
}

__global__ void __launch_bounds__(FS_THREADS) flow_stats_kernel(FlowArgs a) {
    __shared__ float4 ph[FS_TILE];
    __shared__ float ve[FS_TILE];
    __shared__ int slot[FS_TILE];
    __shared__ int fslot[FS_TILE];
    __shared__ int wave_cnt[FS_WAVES];
    __shared__ unsigned h_cnt[FS_WAVES][FS_MAX_BINS];
    __shared__ unsigned long long h_sum[FS_WAVES][FS_MAX_BINS];
    __shared__ unsigned long long acc[2][FS_MAX_BINS];
    __shared__ long long red[FS_SERIES][FS_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int RB = a.RB;
    for (int k = tid; k < FS_WAVES * FS_MAX_BINS; k += FS_THREADS) {
        (&h_cnt[0][0])[k] = 0u;
        (&h_sum[0][0])[k] = 0ull;
    }
    for (int k = tid; k < 2 * FS_MAX_BINS; k += FS_THREADS) (&acc[0][0])[k] = 0ull;
    __syncthreads();
    const long long G = a.has_box ? (long long)a.gx * a.gy : 0;
    unsigned long long* w_map = a.ws + 2ll * a.S * RB;
    const long long runs = (a.slices + a.run - 1) / a.run;
    for (long long r = blockIdx.x; r < runs; r += gridDim.x) {
        const long long lo = r * a.run, hi = min(lo + (long long)a.run, a.slices);
        int cur_s = -1;
        for (long long sl = lo; sl <= hi; ++sl) {
            const int s = sl < hi ? (int)(sl / a.Tp) : -1;
            if (cur_s >= 0 && s != cur_s) {
                // flush the accumulator of member cur_s into its workspace rows
                for (int e = tid; e < 2 * RB; e += FS_THREADS) {
                    const int row = e / RB, b = e - row * RB;
                    const unsigned long long v = acc[row][b];
                    if (!v) continue;
                    atomicAdd(a.ws + ((long long)row * a.S + cur_s) * RB + b, v);
                    acc[row][b] = 0ull;
                }
                __syncthreads();
            }
            if (sl == hi) break;
            cur_s = s;
            const int tp = (int)(sl - (long long)s * a.Tp);
            const long long frame = (long long)s * a.T + a.t0 + tp;
            const float2* P = reinterpret_cast<const float2*>(a.P) + frame * a.N;
            const float2* V = reinterpret_cast<const float2*>(a.V) + frame * a.N;
            const float* M = a.M + frame * a.N;
            int bound = a.N;
            if (a.n_active) bound = min(max(a.n_active[s], 0), a.N);
            unsigned* hc = h_cnt[w];
            unsigned long long* hs = h_sum[w];
            const bool one_tile = bound <= FS_TILE;
            int cnt = one_tile ? fs_stage(a, P, V, M, 0, bound, ph, ve, slot, wave_cnt) : 0;
            long long l_n = 0, l_sum = 0, l_same = 0, l_opp = 0, d_plus = 0, d_minus = 0;
            // focal agents: each tile of FS_TILE candidate slots compacted into fslot, then one per lane in chunks of 256
            for (int f_lo = 0; f_lo < bound; f_lo += FS_TILE) {
                const int nf = wg_compact<FS_THREADS>(
                    f_lo, min(f_lo + FS_TILE, bound), wave_cnt,
                    [&](int j) {
                        const float2 p = P[j];
                        return fs_participant(M[j], p, V[j]) && in_box(a.has_box, a.x0, a.x1, a.y0, a.y1, p);
                    },
                    [&](int q, int j) { fslot[q] = j; });
                for (int c0 = 0; c0 < nf; c0 += FS_THREADS) {
                    const bool focal = c0 + tid < nf;
                    const int i = focal ? fslot[c0 + tid] : -1;
                    float2 pi = make_float2(0.f, 0.f), vi = make_float2(0.f, 0.f);
                    FsAgent g{NAN, 0.f, 0.f};
                    if (focal) {
                        pi = P[i];
                        vi = V[i];
                        g = fs_agent(a, vi);
                    }
                    const bool sweeps = focal && (!isnan(g.hx) || g.ve != 0.f);
                    unsigned n_same = 0, n_opp = 0;
                    if (one_tile) {
                        if (sweeps) fs_sweep(a, ph, ve, slot, cnt, i, pi, g, hc, hs, n_same, n_opp);
                    } else {
                        for (int t_lo = 0; t_lo < bound; t_lo += FS_TILE) {
                            cnt = fs_stage(a, P, V, M, t_lo, min(t_lo + FS_TILE, bound), ph, ve, slot, wave_cnt);
                            if (sweeps) fs_sweep(a, ph, ve, slot, cnt, i, pi, g, hc, hs, n_same, n_opp);
                            __syncthreads();  // every lane is done with this tile before the next one is staged
                        }
                    }
                    if (focal) {
                        if (g.ve != 0.f) {
                            d_plus += g.ve > 0.f ? 1 : 0;
                            d_minus += g.ve > 0.f ? 0 : 1;
                            const unsigned band = n_same + n_opp;
                            if (band > 0u) {
                                const float ratio = ((float)n_same - (float)n_opp) / (float)band;
                                ++l_n;
                                l_sum += llrintf(ratio * ratio * FS_Q);
                                l_same += n_same;
                                l_opp += n_opp;
                            }
                        }
                        if (a.has_box) {
                            const float cx = floorf((pi.x - a.x0) / a.cell), cy = floorf((pi.y - a.y0) / a.cell);
                            if (cx >= 0.f && cx < (float)a.gx && cy >= 0.f && cy < (float)a.gy) {
                                unsigned long long* m = w_map + (long long)s * G + (long long)(int)cy * a.gx + (int)cx;
                                atomicAdd(m, 1ull);
                                atomicAdd(m + (long long)a.S * G, (unsigned long long)llrintf(vi.x * FS_Q));
                                atomicAdd(m + 2ll * a.S * G, (unsigned long long)llrintf(vi.y * FS_Q));
                            }
                        }
                    }
                }
                __syncthreads();              // fslot is rewritten by the next focal tile
            }
            // the slice's series: lanes, then waves; its rows: the waves' rows added into the 64-bit accumulator
            const long long ser[FS_SERIES] = {wave_sum(l_n),    wave_sum(l_sum),  wave_sum(l_same),
                                              wave_sum(l_opp),  wave_sum(d_plus), wave_sum(d_minus)};
            if (lane == 0) {
#pragma unroll
                for (int k = 0; k < FS_SERIES; ++k) red[k][w] = ser[k];
            }
            __syncthreads();                  // red and every wave's rows complete
            if (tid < FS_SERIES) {
                long long x = 0;
                for (int q = 0; q < FS_WAVES; ++q) x += red[tid][q];
                long long* dst = a.series[0];
#pragma unroll
                for (int k = 1; k < FS_SERIES; ++k) dst = tid == k ? a.series[k] : dst;
                dst[sl] = x;
            }
            for (int b = tid; b < RB; b += FS_THREADS) {
                unsigned long long c = 0, x = 0;
                for (int q = 0; q < FS_WAVES; ++q) {
                    c += h_cnt[q][b];
                    x += h_sum[q][b];
                    h_cnt[q][b] = 0u;
                    h_sum[q][b] = 0ull;
                }
                acc[0][b] += c;
                acc[1][b] += x;
            }
            __syncthreads();                  // rows zeroed, tile and red free for the next slice
        }
    }
}

__global__ void __launch_bounds__(FS_THREADS) flow_stats_copy_kernel(FlowArgs a) {
    const long long n0 = (long long)a.S * a.RB, n1 = a.has_box ? (long long)a.S * a.gx * a.gy : 0;
    const long long total = 2 * n0 + 3 * n1;
    for (long long e = (long long)blockIdx.x * FS_THREADS + threadIdx.x; e < total; e += (long long)gridDim.x * FS_THREADS) {
        const long long v = (long long)a.ws[e];
        long long q = e;
        if (q < n0) { a.corr_pairs[q] = v; continue; }
        q -= n0;
        if (q < n0) { a.corr_sum[q] = v; continue; }
        q -= n0;
        if (q < n1) { a.map_n[q] = v; continue; }
        q -= n1;
        if (q < n1) { a.map_vx[q] = v; continue; }
        q -= n1;
        a.map_vy[q] = v;
    }
}

}  // namespace piml

using namespace piml;

PIML_API long long piml_flow_stats_workspace_bytes(int S, int r_bins, int gx, int gy) {
    if (S < 0 || r_bins < 0 || gx < 0 || gy < 0) return -1;
    return (long long)S * (2ll * r_bins + 3ll * gx * gy) * (long long)sizeof(unsigned long long);
}

PIML_API int piml_flow_stats(const float* P, const float* V, const float* M, const int* n_active, int S, int T, int N,
                             int t0, int t1, float v_min, float r_bin, int r_bins, float r_max, float ex, float ey,
                             float lane_width, float lane_length, int has_box, float x0, float x1, float y0, float y1,
                             float cell, int gx, int gy, long long* corr_pairs, long long* corr_sum, long long* lane_n,
                             long long* lane_sum, long long* lane_same, long long* lane_opp, long long* dir_plus,
                             long long* dir_minus, long long* map_n, long long* map_vx, long long* map_vy, void* workspace,
                             long long workspace_bytes, void* stream) {
    const auto positive = [](float x) { return x > 0.f && std::isfinite(x); };
    if (S < 0 || T < 0 || N < 0 || N > FS_MAX_N || t0 < 0 || t1 > T || t1 < t0 || !positive(v_min) || !positive(r_bin) ||
        r_bins < 1 || r_bins > FS_MAX_BINS || !positive(r_max) || !positive(lane_width) || !positive(lane_length))
        return hipErrorInvalidValue;
    const double norm2 = (double)ex * (double)ex + (double)ey * (double)ey;
    if (!(std::fabs(norm2 - 1.0) <= 1e-4)) return hipErrorInvalidValue;
    if (has_box && (!std::isfinite(x0) || !std::isfinite(x1) || !std::isfinite(y0) || !std::isfinite(y1) || !(x0 < x1) ||
                    !(y0 < y1) || !positive(cell) || gx < 1 || gy < 1))
        return hipErrorInvalidValue;
    if (S == 0 || t1 == t0 || N == 0) return hipSuccess;
    if (!P || !V || !M || !corr_pairs || !corr_sum || !lane_n || !lane_sum || !lane_same || !lane_opp || !dir_plus ||
        !dir_minus || !workspace || (has_box && (!map_n || !map_vx || !map_vy)))
        return hipErrorInvalidValue;
    const long long need = piml_flow_stats_workspace_bytes(S, r_bins, has_box ? gx : 0, has_box ? gy : 0);
    if (workspace_bytes < need) return hipErrorInvalidValue;
    FlowArgs a{};
    a.P = P, a.V = V, a.M = M, a.n_active = n_active;
    a.S = S, a.T = T, a.N = N, a.t0 = t0, a.Tp = t1 - t0, a.RB = r_bins;
    a.slices = (long long)S * a.Tp;
    const unsigned grid = stats_run_grid(a.slices, FS_TARGET_WG, FS_MAX_RUN, FS_MAX_GRID, &a.run);
    a.has_box = has_box ? 1 : 0, a.gx = has_box ? gx : 0, a.gy = has_box ? gy : 0;
    a.v_min = v_min, a.r_bin = r_bin, a.r_max = r_max, a.ex = ex, a.ey = ey;
    a.lane_width = lane_width, a.lane_length = lane_length;
    // The pre-filter changes no result.  r = sqrtf(d2) < r_max needs d2 < r_max^2 (1 + 2^-22).  A band member has computed
    // |d.e_perp| < lane_width and |d.e| < lane_length; their squares sum to |e|^2 |d|^2 up to the float32 error of two dot
    // products (a few 1e-7 relative) and | |e|^2 - 1 | <= 1e-4, so d2 <= (lane_width^2 + lane_length^2) (1 + 2e-4).  The
    // factor 1.001 covers both with room.
    const double reach2 = std::fmax((double)r_max * r_max, (double)lane_width * lane_width + (double)lane_length * lane_length);
    a.far2 = (float)(reach2 * 1.001);
    a.x0 = x0, a.x1 = x1, a.y0 = y0, a.y1 = y1, a.cell = cell;
    a.ws = static_cast<unsigned long long*>(workspace);
    a.corr_pairs = corr_pairs, a.corr_sum = corr_sum;
    a.series[0] = lane_n, a.series[1] = lane_sum, a.series[2] = lane_same, a.series[3] = lane_opp;
    a.series[4] = dir_plus, a.series[5] = dir_minus;
    a.map_n = map_n, a.map_vx = map_vx, a.map_vy = map_vy;
    hipStream_t st = as_stream(stream);
    hipError_t e = hipMemsetAsync(workspace, 0, (size_t)need, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(flow_stats_kernel, dim3(grid), dim3(FS_THREADS), 0, st, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const long long elems = need / (long long)sizeof(unsigned long long);
    const long long blocks = (elems + FS_THREADS - 1) / FS_THREADS;
    hipLaunchKernelGGL(flow_stats_copy_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(FS_THREADS), 0, st, a);
    return hipGetLastError();
}
