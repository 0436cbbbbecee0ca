// Pair statistics of crowds that need no pairing of a simulated agent with a recorded one: the
// time-to-collision pair histogram of Karamouzas, Skinner and Guy (Phys. Rev. Lett. 113, 238701, 2014) at lag 0 and at
// time-scrambled lags, the pair-distance histogram, the overlap count and, at lag 0, each focal agent's nearest-neighbour
// distance and smallest time to collision, for S members in one call.
//
// Participant of slice (s, t): M == 1, both coordinates of P finite, both components of V finite, slot below n_active[s].
// Focal: a participant inside the optional box [x0, x1) x [y0, y1).  Pair slice (s, t, k), t0 <= t, t + L_k < t1 (L_0 = 0):
// every focal i of frame t against every participant j != i (as a slot) of frame t + L_k.  Per pair, float32 with true
// divisions and no contraction: d = p_j - p_i, w = v_j - v_i, c = |d|^2 - R^2, b = d.w, a = |w|^2; the distance sqrt(|d|^2)
// (pairs with distance >= r_max skipped entirely when r_max is given); overlap when c < 0; otherwise a collision course when
// b < 0 and disc = b^2 - a c >= 0, with tau = c / (-b + sqrt(disc)); bins floor(tau / tau_bin), floor(distance / r_bin).
//
// pair_stats_kernel: one workgroup of 256 lanes per pair slice.  The participants of frame t + L_k are compacted in slot
// order into LDS tiles of PS_TILE sources (position + velocity 16 B, slot 4 B); the focal agents of frame t are compacted
// too (slots, in tiles of PS_TILE candidates) and taken one per lane in chunks of 256, so that absent slots and agents
// outside the box occupy no lane.  Each wave counts into its own u32 histograms in LDS (ds_add_u32); per-lane registers
// hold the pair / overlap counts and, at lag 0, the minimum distance and tau.  After a slice the waves' rows are added
// into the workgroup's u64 LDS accumulator; a workgroup takes a run of consecutive slices (same member and lag for most
// of it) and adds the accumulator to the member's rows of the workspace with 64-bit integer atomics when the member or
// lag changes and at the end of the run.  pair_stats_copy_kernel moves the workspace rows into the outputs.  No float
// atomics: every output is an integer count, so the results are bitwise reproducible whatever the order of the adds.
//
// No u32 counter overflows: per slice a wave's bin holds at most (ceil(N / 256) * 64) * N < 2^32 pairs for N <= PS_MAX_N,
// and the u32 rows are folded into u64 after every slice.
#include "stats.hpp"
#include "../../include/piml_hip.h"

#include <cmath>

namespace piml {

constexpr int PS_THREADS = 256;
constexpr int PS_WAVES = PS_THREADS / 64;
constexpr int PS_TILE = 1024;                 // sources per LDS tile (20 KiB)
constexpr int PS_MAX_BINS = 256;
constexpr int PS_MAX_LAGS = 8;
constexpr int PS_MAX_N = 65536;
constexpr int PS_HIST = 2 * PS_MAX_BINS + 2 * (PS_MAX_BINS + 1);      // ttc, dist, nn, min_ttc of one slice
constexpr long long PS_MAX_GRID = 1 << 20;
constexpr long long PS_TARGET_WG = 2048;      // runs are sized so that about this many workgroups start
constexpr int PS_MAX_RUN = 64;

struct PairArgs {
    const float *P, *V, *M;                   // (S, T, N, 2), (S, T, N, 2), (S, T, N)
    const int* n_active;                      // (S) or NULL
    int S, T, N, t0, Tp, K1, TB, RB;
    int lag[PS_MAX_LAGS + 1];                 // lag[0] = 0
    int off[PS_MAX_LAGS + 2];                 // first slice of lag k within a member (k-major, then t)
    int per_member, run, has_box, has_rmax;
    float r2, r_max, x0, x1, y0, y1, tau_bin, r_bin;
    long long slices;
    unsigned long long* ws;                   // focal, pairs, overlap (S, K1) | ttc (S, K1, TB) | dist (S, K1, RB) |
                                              // nn (S, RB + 1) | min_ttc (S, TB + 1)
    long long *focal, *pairs, *overlap, *ttc, *dist, *nn, *min_ttc;
};

__device__ __forceinline__ bool ps_participant(float m, float2 p, float2 v) {
    return m == 1.f && isfinite(p.x) && isfinite(p.y) && isfinite(v.x) && isfinite(v.y);
}

// Compacts the participants of slots [lo, hi) (hi - lo <= PS_TILE) into pv / slot in slot order; returns their number
// (wg_compact: every thread calls it, and the tile may still be read on entry).
__device__ int ps_stage(const float2* P, const float2* V, const float* M, int lo, int hi, float4* pv, int* slot,
                        int* wave_cnt) {
    float2 p, v;
    return wg_compact<PS_THREADS>(
        lo, hi, wave_cnt, [&](int j) { return p = P[j], v = V[j], ps_participant(M[j], p, v); },
        [&](int q, int j) { pv[q] = make_float4(p.x, p.y, v.x, v.y), slot[q] = j; });
}

struct PsLane {
    unsigned pairs, overlap;
    float min_d, min_tau;
};

// The sweep of one focal agent (slot i, position / velocity pi) over cnt staged sources: counts into the wave's rows.
__device__ __forceinline__ void ps_sweep(const PairArgs& a, const float4* pv, const int* slot, int cnt, int i, float4 pi,
                                         unsigned* h_ttc, unsigned* h_dist, PsLane& l) {
    const float r2 = a.r2, r_max = a.r_max, tau_bin = a.tau_bin, r_bin = a.r_bin;
    const float ftb = (float)a.TB, frb = (float)a.RB;
    const bool has_rmax = a.has_rmax != 0;
    for (int q = 0; q < cnt; ++q) {
        const float4 s = pv[q];
        if (slot[q] == i) continue;
        const float dx = s.x - pi.x, dy = s.y - pi.y;
        const float d2 = dx * dx + dy * dy;
        const float dist = sqrtf(d2);
        if (has_rmax && dist >= r_max) continue;
        ++l.pairs;
        l.min_d = fminf(l.min_d, dist);
        const float qd = floorf(dist / r_bin);
        if (qd < frb) atomicAdd(h_dist + (int)qd, 1u);
        const float c = d2 - r2;
        if (c < 0.f) {
            ++l.overlap;
            continue;
        }
        const float wx = s.z - pi.z, wy = s.w - pi.w;
        const float b = dx * wx + dy * wy;
        if (!(b < 0.f)) continue;
        const float aa = wx * wx + wy * wy;
        const float disc = b * b - aa * c;
        if (!(disc >= 0.f)) continue;
        const float tau = c / (-b + sqrtf(disc));
        l.min_tau = fminf(l.min_tau, tau);
        const float qt = floorf(tau / tau_bin);
        if (qt < ftb) atomicAdd(h_ttc + (int)qt, 1u);
    }
}

__global__ void __launch_bounds__(PS_THREADS) pair_stats_kernel(PairArgs a) {
    __shared__ float4 pv[PS_TILE];
    __shared__ int slot[PS_TILE];
    __shared__ int fslot[PS_TILE];
    __shared__ int wave_cnt[PS_WAVES];
    __shared__ unsigned hist[PS_WAVES][PS_HIST];
    __shared__ unsigned long long acc[3 + PS_HIST];
    __shared__ unsigned long long red[3][PS_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int TB = a.TB, RB = a.RB;
    // row offsets inside a slice's histogram: ttc [0, TB), dist [TB, TB + RB), nn (RB + 1), min_ttc (TB + 1)
    const int o_dist = TB, o_nn = TB + RB, o_mt = TB + 2 * RB + 1, n_hist = 2 * TB + 2 * RB + 2;
    for (int k = tid; k < PS_WAVES * PS_HIST; k += PS_THREADS) (&hist[0][0])[k] = 0u;
    for (int k = tid; k < 3 + PS_HIST; k += PS_THREADS) acc[k] = 0ull;
    __syncthreads();
    const long long runs = (a.slices + a.run - 1) / a.run;
    for (long long r = blockIdx.x; r < runs; r += gridDim.x) {
        const long long lo = r * a.run, hi = min(lo + (long long)a.run, a.slices);
        int cur_s = -1, cur_k = -1;
        for (long long sl = lo; sl <= hi; ++sl) {
            int s = -1, k = -1, t = 0, lag = 0;
            if (sl < hi) {
                s = (int)(sl / a.per_member);
                const int rem = (int)(sl - (long long)s * a.per_member);
                // the last lag whose first slice is at or before rem (lags without slices share the next one's offset);
                // unrolled selects, so the argument arrays are never indexed at run time
                int base = 0;
                k = 0;
#pragma unroll
                for (int q = 1; q <= PS_MAX_LAGS; ++q)
                    if (a.off[q] <= rem) k = q, base = a.off[q], lag = a.lag[q];
                t = rem - base;
            }
            if (cur_s >= 0 && (s != cur_s || k != cur_k)) {
                // flush the accumulator of (cur_s, cur_k) into the member's workspace rows
                const long long S = a.S, K1 = a.K1;
                unsigned long long* ws = a.ws;
                unsigned long long* w_ttc = ws + 3 * S * K1;
                unsigned long long* w_dist = w_ttc + S * K1 * TB;
                unsigned long long* w_nn = w_dist + S * K1 * RB;
                unsigned long long* w_mt = w_nn + S * (RB + 1);
                const int n_acc = 3 + (cur_k == 0 ? n_hist : TB + RB);
                for (int e = tid; e < n_acc; e += PS_THREADS) {
                    const unsigned long long v = acc[e];
                    if (!v) continue;
                    unsigned long long* dst;
                    if (e < 3) dst = ws + (e * S + cur_s) * K1 + cur_k;
                    else if (e < 3 + TB) dst = w_ttc + ((long long)cur_s * K1 + cur_k) * TB + (e - 3);
                    else if (e < 3 + TB + RB) dst = w_dist + ((long long)cur_s * K1 + cur_k) * RB + (e - 3 - TB);
                    else if (e < 3 + o_mt) dst = w_nn + (long long)cur_s * (RB + 1) + (e - 3 - o_nn);
                    else dst = w_mt + (long long)cur_s * (TB + 1) + (e - 3 - o_mt);
                    atomicAdd(dst, v);
                    acc[e] = 0ull;
                }
                __syncthreads();
            }
            if (sl == hi) break;
            cur_s = s, cur_k = k;
            const bool lag0 = k == 0;
            const long long fi = (long long)s * a.T + a.t0 + t, fj = fi + lag;
            const float2* Pi = reinterpret_cast<const float2*>(a.P) + fi * a.N;
            const float2* Vi = reinterpret_cast<const float2*>(a.V) + fi * a.N;
            const float* Mi = a.M + fi * a.N;
            const float2* Pj = reinterpret_cast<const float2*>(a.P) + fj * a.N;
            const float2* Vj = reinterpret_cast<const float2*>(a.V) + fj * a.N;
            const float* Mj = a.M + fj * a.N;
            int bound = a.N;
            if (a.n_active) bound = min(max(a.n_active[s], 0), a.N);
            unsigned* hw = hist[w];
            const bool one_tile = bound <= PS_TILE;
            int cnt = one_tile ? ps_stage(Pj, Vj, Mj, 0, bound, pv, slot, wave_cnt) : 0;
            PsLane l{0u, 0u, INFINITY, INFINITY};
            unsigned n_focal = 0;
            // focal agents: each tile of PS_TILE candidate slots compacted into fslot, then one per lane in chunks of 256
            for (int f_lo = 0; f_lo < bound; f_lo += PS_TILE) {
                const int nf = wg_compact<PS_THREADS>(
                    f_lo, min(f_lo + PS_TILE, bound), wave_cnt,
                    [&](int j) {
                        const float2 p = Pi[j];
                        return ps_participant(Mi[j], p, Vi[j]) && in_box(a.has_box, a.x0, a.x1, a.y0, a.y1, p);
                    },
                    [&](int q, int j) { fslot[q] = j; });
                for (int c0 = 0; c0 < nf; c0 += PS_THREADS) {
                    const bool focal = c0 + tid < nf;
                    const int i = focal ? fslot[c0 + tid] : -1;
                    float4 pi = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (focal) {
                        const float2 p = Pi[i], v = Vi[i];
                        pi = make_float4(p.x, p.y, v.x, v.y);
                    }
                    l.min_d = INFINITY;
                    l.min_tau = INFINITY;
                    if (one_tile) {
                        if (focal) ps_sweep(a, pv, slot, cnt, i, pi, hw, hw + o_dist, l);
                    } else {
                        for (int t_lo = 0; t_lo < bound; t_lo += PS_TILE) {
                            cnt = ps_stage(Pj, Vj, Mj, t_lo, min(t_lo + PS_TILE, bound), pv, slot, wave_cnt);
                            if (focal) ps_sweep(a, pv, slot, cnt, i, pi, hw, hw + o_dist, l);
                            __syncthreads();  // every lane is done with this tile before the next one is staged
                        }
                    }
                    if (focal) {
                        ++n_focal;
                        if (lag0) {
                            const float qd = floorf(l.min_d / a.r_bin), qt = floorf(l.min_tau / a.tau_bin);
                            atomicAdd(hw + o_nn + (qd < (float)RB ? (int)qd : RB), 1u);
                            atomicAdd(hw + o_mt + (qt < (float)TB ? (int)qt : TB), 1u);
                        }
                    }
                }
                __syncthreads();              // fslot is rewritten by the next focal tile
            }
            // the slice's counters: lanes, then waves; its rows: the waves' u32 rows added into the u64 accumulator
            const unsigned long long f = wave_sum((unsigned long long)n_focal);
            const unsigned long long p = wave_sum((unsigned long long)l.pairs);
            const unsigned long long o = wave_sum((unsigned long long)l.overlap);
            if (lane == 0) {
                red[0][w] = f;
                red[1][w] = p;
                red[2][w] = o;
            }
            __syncthreads();                  // red and every wave's rows complete
            if (tid < 3) {
                unsigned long long x = 0;
                for (int q = 0; q < PS_WAVES; ++q) x += red[tid][q];
                acc[tid] += x;
            }
            const int n_used = lag0 ? n_hist : TB + RB;
            for (int e = tid; e < n_used; e += PS_THREADS) {
                unsigned long long x = 0;
                for (int q = 0; q < PS_WAVES; ++q) {
                    x += hist[q][e];
                    hist[q][e] = 0u;
                }
                acc[3 + e] += x;
            }
            __syncthreads();                  // rows zeroed, tile and red free for the next slice
        }
    }
}

__global__ void __launch_bounds__(PS_THREADS) pair_stats_copy_kernel(PairArgs a) {
    const long long S = a.S, K1 = a.K1;
    const long long n0 = S * K1, n3 = n0 * a.TB, n4 = n0 * a.RB, n5 = S * (a.RB + 1), n6 = S * (a.TB + 1);
    const long long total = 3 * n0 + n3 + n4 + n5 + n6;
    for (long long e = (long long)blockIdx.x * PS_THREADS + threadIdx.x; e < total; e += (long long)gridDim.x * PS_THREADS) {
        const long long v = (long long)a.ws[e];
        long long q = e;
        if (q < n0) { a.focal[q] = v; continue; }
        q -= n0;
        if (q < n0) { a.pairs[q] = v; continue; }
        q -= n0;
        if (q < n0) { a.overlap[q] = v; continue; }
        q -= n0;
        if (q < n3) { a.ttc[q] = v; continue; }
        q -= n3;
        if (q < n4) { a.dist[q] = v; continue; }
        q -= n4;
        if (q < n5) { a.nn[q] = v; continue; }
        q -= n5;
        a.min_ttc[q] = v;
    }
}

static long long ps_workspace_elems(long long S, long long K1, long long TB, long long RB) {
    return S * (3 * K1 + K1 * TB + K1 * RB + (RB + 1) + (TB + 1));
}

}  // namespace piml

using namespace piml;

PIML_API long long piml_pair_stats_workspace_bytes(int S, int K, int tau_bins, int r_bins) {
    if (S < 0 || K < 0 || tau_bins < 0 || r_bins < 0) return -1;
    return ps_workspace_elems(S, (long long)K + 1, tau_bins, r_bins) * (long long)sizeof(unsigned long long);
}

PIML_API int piml_pair_stats(const float* P, const float* V, const float* M, const int* n_active, int S, int T, int N,
                             int t0, int t1, const int* lags, int K, float radius, float r_max, int has_box, float x0,
                             float x1, float y0, float y1, float tau_bin, int tau_bins, float r_bin, int r_bins,
                             long long* focal, long long* pairs, long long* overlap, long long* ttc, long long* dist,
                             long long* nn, long long* min_ttc, void* workspace, long long workspace_bytes, void* stream) {
    if (S <= 0 || T <= 0 || N <= 0 || N > PS_MAX_N || t0 < 0 || t1 > T || t1 <= t0 || K < 0 || K > PS_MAX_LAGS ||
        (K > 0 && !lags) || !(radius > 0.f) || !std::isfinite(radius) || std::isnan(r_max) ||
        !(tau_bin > 0.f) || !std::isfinite(tau_bin) || tau_bins < 1 || tau_bins > PS_MAX_BINS ||
        !(r_bin > 0.f) || !std::isfinite(r_bin) || r_bins < 1 || r_bins > PS_MAX_BINS)
        return hipErrorInvalidValue;
    for (int k = 0; k < K; ++k)
        if (lags[k] <= 0 || (k > 0 && lags[k] <= lags[k - 1])) return hipErrorInvalidValue;
    if (has_box && (!std::isfinite(x0) || !std::isfinite(x1) || !std::isfinite(y0) || !std::isfinite(y1) || !(x0 < x1) ||
                    !(y0 < y1)))
        return hipErrorInvalidValue;
    if (!P || !V || !M || !focal || !pairs || !overlap || !ttc || !dist || !nn || !min_ttc || !workspace)
        return hipErrorInvalidValue;
    const long long need = piml_pair_stats_workspace_bytes(S, K, tau_bins, r_bins);
    if (workspace_bytes < need) return hipErrorInvalidValue;
    PairArgs a{};
    a.P = P, a.V = V, a.M = M, a.n_active = n_active;
    a.S = S, a.T = T, a.N = N, a.t0 = t0, a.Tp = t1 - t0, a.K1 = K + 1, a.TB = tau_bins, a.RB = r_bins;
    a.lag[0] = 0;
    for (int k = 0; k < K; ++k) a.lag[k + 1] = lags[k];
    a.off[0] = 0;
    for (int k = 0; k <= K; ++k) a.off[k + 1] = a.off[k] + (a.Tp > a.lag[k] ? a.Tp - a.lag[k] : 0);
    for (int k = K + 2; k < PS_MAX_LAGS + 2; ++k) a.off[k] = a.off[K + 1];
    a.per_member = a.off[K + 1];
    a.slices = (long long)S * a.per_member;
    const unsigned grid = stats_run_grid(a.slices, PS_TARGET_WG, PS_MAX_RUN, PS_MAX_GRID, &a.run);
    a.has_box = has_box ? 1 : 0;
    a.x0 = x0, a.x1 = x1, a.y0 = y0, a.y1 = y1;
    a.has_rmax = r_max > 0.f ? 1 : 0;
    a.r_max = r_max;
    a.r2 = radius * radius;
    a.tau_bin = tau_bin, a.r_bin = r_bin;
    a.ws = static_cast<unsigned long long*>(workspace);
    a.focal = focal, a.pairs = pairs, a.overlap = overlap, a.ttc = ttc, a.dist = dist, a.nn = nn, a.min_ttc = min_ttc;
    hipStream_t st = as_stream(stream);
    hipError_t e = hipMemsetAsync(workspace, 0, (size_t)need, st);
    if (e != hipSuccess) return e;
    if (grid > 0) {
        hipLaunchKernelGGL(pair_stats_kernel, dim3(grid), dim3(PS_THREADS), 0, st, a);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const long long elems = need / (long long)sizeof(unsigned long long);
    const long long blocks = (elems + PS_THREADS - 1) / PS_THREADS;
    hipLaunchKernelGGL(pair_stats_copy_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(PS_THREADS), 0, st, a);
    return hipGetLastError();
}
