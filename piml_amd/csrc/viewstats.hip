// Heading-frame pair statistics of crowds: where the others are in a walking agent's own frame.  The pair
// distribution over (distance ahead, distance to the left) at lag 0 and at time-scrambled lags, split by the other agent's
// direction relative to the focal one, and, at lag 0, the cell of each focal agent's nearest neighbour and its front gap
// with the speed walked at that gap (the distance-headway / speed relation of Seyfried et al., J. Stat. Mech. P10002,
// 2005), for S members in one call.
//
// Participant of slice (s, t): M == 1, both coordinates of P finite, both components of V finite and below 1024 in
// magnitude, slot below n_active[s].  Mover: a participant with sp = sqrt(vx^2 + vy^2) >= v_min; its heading h = v / sp.
// Focal: a participant mover of frame t inside the optional box [x0, x1) x [y0, y1).  Source: every participant j != i (as a
// slot) of frame t + L_k, mover or not.  Pair slice (s, t, k), t0 <= t, t + L_k < t1 (L_0 = 0), numbered as in pairstats.hip.
// Per pair, float32 with true divisions and square roots and no contraction: d = p_j - p_i, r = sqrt(dx^2 + dy^2) (pairs with
// r >= r_max skipped entirely when r_max is given); a = dx hx + dy hy the distance ahead, l = dy hx - dx hy the distance to
// the left; class 0 when j is not a mover, otherwise with q = h_i.h_j: 1 (with) if q >= cos_same, 2 (against) if
// q <= -cos_same, 3 (across) else; cell cx = floor((a + X) / cell), cy = floor((l + X) / cell) with X = cell * half formed on
// the host, counted when 0 <= cx, cy < G = 2 half.  At lag 0 per focal agent: the cell of its nearest source (smallest r, ties
// to the lowest slot; G G when that lies outside the map or there is no source) and, over the sources with a > 0 and
// |l| < corridor, the smallest a as b = floor(a / gap_bin) (gap_bins: at or beyond the range, or nobody in front), with
// llrintf(sp_i 2^20) added to the speed sum of a bin b < gap_bins.
//
// view_stats_kernel: one workgroup of 256 lanes per pair slice, a run of consecutive slices per workgroup.  The participants
// of frame t + L_k are compacted in slot order into LDS tiles of VS_TILE sources (position and heading 16 B -- heading x NaN:
// not a mover --, slot 4 B); the focal agents of frame t are compacted too and taken one per lane in chunks of 256.  The
// sources are swept in slot order, so a strict comparison keeps the lowest slot among equally near ones.  All waves count
// into ONE set of u32 LDS rows (ds_add_u32: the four-class map, the nearest-neighbour map, the front gaps) and one u64 row
// (the speed sums); the rows stay in LDS over the slices of a run that share member and lag and go to the member's workspace
// rows with 64-bit integer atomics when the member or lag changes, at the end of the run, and before a slice that could
// overflow a u32 bin.  view_stats_copy_kernel moves the workspace into the outputs.  No float atomics: every output is an
// integer, so the results are bitwise reproducible whatever the order of the adds.
//
// No u32 counter overflows: a slice adds at most n (n - 1) pairs (n >= 2 participants; n <= VS_MAX_N gives < 2^32) to a map
// bin and at most n agents to a bin of the other rows; the kernel sums this bound over the slices since the last flush and
// flushes before it would pass 2^32 - 1.  A lane's pair count of one slice is at most ceil(n / 256) n <= 2^24.
//
// LDS per workgroup (static): tile 16 KiB + slots 4 KiB + focal slots 4 KiB + u32 rows (4 G G + G G + 1 + gap_bins + 1
// <= 5378) 21.0 KiB + speed sums 2 KiB + counters: 47.0 KiB, three workgroups per CU.
#include "stats.hpp"
#include "../../include/piml_hip.h"

#include <cmath>

namespace piml {

constexpr int VS_THREADS = 256;
constexpr int VS_WAVES = VS_THREADS / 64;
constexpr int VS_TILE = 1024;                 // sources per LDS tile (20 KiB)
constexpr int VS_MAX_HALF = 16;
constexpr int VS_MAX_CELLS = 4 * VS_MAX_HALF * VS_MAX_HALF;           // G G
constexpr int VS_MAX_BINS = 256;
constexpr int VS_MAX_LAGS = 8;
constexpr int VS_MAX_N = 65536;
constexpr int VS_ROWS = 4 * VS_MAX_CELLS + (VS_MAX_CELLS + 1) + (VS_MAX_BINS + 1);   // map, nn_map, front_gap
constexpr float VS_Q = 1048576.f;             // 2^20
constexpr float VS_MAX_V = 1024.f;
constexpr long long VS_MAX_GRID = 1 << 20;
constexpr long long VS_TARGET_WG = 2048;      // runs are sized so that about this many workgroups start
constexpr int VS_MAX_RUN = 64;

struct ViewArgs {
    const float *P, *V, *M;                   // (S, T, N, 2), (S, T, N, 2), (S, T, N)
    const int* n_active;                      // (S) or NULL
    int S, T, N, t0, Tp, K1, G, GB;
    int lag[VS_MAX_LAGS + 1];                 // lag[0] = 0
    int off[VS_MAX_LAGS + 2];                 // first slice of lag k within a member (k-major, then t)
    int per_member, run, has_box, has_rmax;
    float v_min, cell, X, cos_same, r_max, corridor, gap_bin, x0, x1, y0, y1;
    long long slices;
    unsigned long long* ws;                   // focal, pairs (S, K1) | map (S, K1, 4, G, G) | nn_map (S, G G + 1) |
                                              // front_gap (S, GB + 1) | front_speed (S, GB)
    long long *focal, *pairs, *map, *nn_map, *front_gap, *front_speed;
};

__device__ __forceinline__ bool vs_participant(float m, float2 p, float2 v) {
    return m == 1.f && isfinite(p.x) && isfinite(p.y) && fabsf(v.x) < VS_MAX_V && fabsf(v.y) < VS_MAX_V;
}

// Compacts the participants of slots [lo, hi) (hi - lo <= VS_TILE) into ph / slot in slot order; returns their number
// (wg_compact: every thread calls it, and the tile may still be read on entry).
__device__ int vs_stage(const ViewArgs& a, const float2* P, const float2* V, const float* M, int lo, int hi, float4* ph,
                        int* slot, int* wave_cnt) {
    float2 p, v;
    return wg_compact<VS_THREADS>(
        lo, hi, wave_cnt, [&](int j) { return p = P[j], v = V[j], vs_participant(M[j], p, v); },
        [&](int q, int j) {
            const float sp = sqrtf(v.x * v.x + v.y * v.y);
            const bool mover = sp >= a.v_min;
            ph[q] = make_float4(p.x, p.y, mover ? v.x / sp : NAN, mover ? v.y / sp : 0.f);
            slot[q] = j;
        });
}

struct VsLane {
    unsigned pairs;
    float min_r, min_a;
    int nn_cell;                              // the nearest source's cell so far; G G: outside the map, or no source
};

// The sweep of one focal agent (slot i at pi, heading h) over cnt staged sources in slot order: the pair maps into h_map,
// the nearest source and the front gap into l.
__device__ __forceinline__ void vs_sweep(const ViewArgs& a, const float4* ph, const int* slot, int cnt, int i, float2 pi,
                                         float2 h, unsigned* h_map, VsLane& l) {
    const float r_max = a.r_max, cell = a.cell, X = a.X, cs = a.cos_same, corridor = a.corridor;
    const int G = a.G, GG = G * G;
    const float fG = (float)G;
    const bool has_rmax = a.has_rmax != 0;
    for (int q = 0; q < cnt; ++q) {
        const float4 s = ph[q];
        if (slot[q] == i) continue;
        const float dx = s.x - pi.x, dy = s.y - pi.y;
        const float r = sqrtf(dx * dx + dy * dy);
        if (has_rmax && r >= r_max) continue;
        ++l.pairs;
        const float ahead = dx * h.x + dy * h.y, left = dy * h.x - dx * h.y;
        const float cx = floorf((ahead + X) / cell), cy = floorf((left + X) / cell);
        const bool in_map = cx >= 0.f && cx < fG && cy >= 0.f && cy < fG;
        const int c = in_map ? (int)cy * G + (int)cx : GG;
        if (in_map) {
            int cls = 0;
            if (!isnan(s.z)) {
                const float d = h.x * s.z + h.y * s.w;
                cls = d >= cs ? 1 : d <= -cs ? 2 : 3;
            }
            atomicAdd(h_map + cls * GG + c, 1u);
        }
        if (r < l.min_r) l.min_r = r, l.nn_cell = c;
        if (ahead > 0.f && fabsf(left) < corridor) l.min_a = fminf(l.min_a, ahead);
    }
}

// Adds the workgroup's LDS rows of (member s, lag index k) to the member's workspace rows and zeroes them.  Every thread of
// the workgroup calls it after a barrier that completed the rows; it ends with one.
__device__ void vs_flush(const ViewArgs& a, int s, int k, unsigned* rows, unsigned long long* spd, unsigned long long* cnt) {
    const int tid = threadIdx.x;
    const long long S = a.S, K1 = a.K1, GG = (long long)a.G * a.G, GB = a.GB;
    const int n_map = 4 * (int)GG, o_gap = n_map + (int)GG + 1;
    unsigned long long* w_map = a.ws + 2 * S * K1;
    unsigned long long* w_nn = w_map + S * K1 * 4 * GG;
    unsigned long long* w_gap = w_nn + S * (GG + 1);
    unsigned long long* w_spd = w_gap + S * (GB + 1);
    const int n_rows = k == 0 ? o_gap + (int)GB + 1 : n_map;
    for (int e = tid; e < n_rows; e += VS_THREADS) {
        const unsigned v = rows[e];
        if (!v) continue;
        rows[e] = 0u;
        unsigned long long* dst;
        if (e < n_map) dst = w_map + ((long long)s * K1 + k) * n_map + e;
        else if (e < o_gap) dst = w_nn + (long long)s * (GG + 1) + (e - n_map);
        else dst = w_gap + (long long)s * (GB + 1) + (e - o_gap);
        atomicAdd(dst, (unsigned long long)v);
    }
    if (k == 0) {
        for (int e = tid; e < (int)GB; e += VS_THREADS) {
            const unsigned long long v = spd[e];
            if (!v) continue;
            spd[e] = 0ull;
            atomicAdd(w_spd + (long long)s * GB + e, v);
        }
    }
    if (tid < 2) {
        const unsigned long long v = cnt[tid];
        if (v) atomicAdd(a.ws + ((long long)tid * S + s) * K1 + k, v);
        cnt[tid] = 0ull;
    }
    __syncthreads();
}

__global__ void __launch_bounds__(VS_THREADS) view_stats_kernel(ViewArgs a) {
    __shared__ float4 ph[VS_TILE];
    __shared__ int slot[VS_TILE];
    __shared__ int fslot[VS_TILE];
    __shared__ int wave_cnt[VS_WAVES];
    __shared__ unsigned rows[VS_ROWS];
    __shared__ unsigned long long spd[VS_MAX_BINS];
    __shared__ unsigned long long cnt[2];     // focal agent-frames, pairs
    const int tid = threadIdx.x, lane = tid & 63;
    const int G = a.G, GG = G * G, GB = a.GB;
    const int o_nn = 4 * GG, o_gap = o_nn + GG + 1;
    for (int k = tid; k < VS_ROWS; k += VS_THREADS) rows[k] = 0u;
    for (int k = tid; k < VS_MAX_BINS; k += VS_THREADS) spd[k] = 0ull;
    if (tid < 2) cnt[tid] = 0ull;
    __syncthreads();
    const long long runs = (a.slices + a.run - 1) / a.run;
    for (long long r = blockIdx.x; r < runs; r += gridDim.x) {
        const long long lo = r * a.run, hi = min(lo + (long long)a.run, a.slices);
        int cur_s = -1, cur_k = -1;
        unsigned long long pending = 0;       // the largest count a u32 bin can hold since the last flush
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
                for (int q = 1; q <= VS_MAX_LAGS; ++q)
                    if (a.off[q] <= rem) k = q, base = a.off[q], lag = a.lag[q];
                t = rem - base;
            }
            int bound = a.N;
            if (sl < hi && a.n_active) bound = min(max(a.n_active[s], 0), a.N);
            const unsigned long long most = (unsigned long long)bound * (unsigned long long)max(bound - 1, 1);
            if (cur_s >= 0 && (s != cur_s || k != cur_k || pending + most > 0xffffffffull)) {
                vs_flush(a, cur_s, cur_k, rows, spd, cnt);
                pending = 0;
            }
            if (sl == hi) break;
            cur_s = s, cur_k = k;
            pending += most;
            const bool lag0 = k == 0;
            const long long fi = (long long)s * a.T + a.t0 + t, fj = fi + lag;
            const float2* Pi = reinterpret_cast<const float2*>(a.P) + fi * a.N;
            const float2* Vi = reinterpret_cast<const float2*>(a.V) + fi * a.N;
            const float* Mi = a.M + fi * a.N;
            const float2* Pj = reinterpret_cast<const float2*>(a.P) + fj * a.N;
            const float2* Vj = reinterpret_cast<const float2*>(a.V) + fj * a.N;
            const float* Mj = a.M + fj * a.N;
            const bool one_tile = bound <= VS_TILE;
            int n_src = one_tile ? vs_stage(a, Pj, Vj, Mj, 0, bound, ph, slot, wave_cnt) : 0;
            unsigned n_focal = 0, n_pairs = 0;
            // focal agents: each tile of VS_TILE candidate slots compacted into fslot, then one per lane in chunks of 256
            for (int f_lo = 0; f_lo < bound; f_lo += VS_TILE) {
                const int nf = wg_compact<VS_THREADS>(
                    f_lo, min(f_lo + VS_TILE, bound), wave_cnt,
                    [&](int j) {
                        const float2 p = Pi[j], v = Vi[j];
                        return vs_participant(Mi[j], p, v) && sqrtf(v.x * v.x + v.y * v.y) >= a.v_min &&
                               in_box(a.has_box, a.x0, a.x1, a.y0, a.y1, p);
                    },
                    [&](int q, int j) { fslot[q] = j; });
                for (int c0 = 0; c0 < nf; c0 += VS_THREADS) {
                    const bool focal = c0 + tid < nf;
                    const int i = focal ? fslot[c0 + tid] : -1;
                    float2 pi = make_float2(0.f, 0.f), h = make_float2(1.f, 0.f);
                    float sp = 1.f;
                    if (focal) {
                        pi = Pi[i];
                        const float2 v = Vi[i];
                        sp = sqrtf(v.x * v.x + v.y * v.y);
                        h = make_float2(v.x / sp, v.y / sp);
                    }
                    VsLane l{0u, INFINITY, INFINITY, GG};
                    if (one_tile) {
                        if (focal) vs_sweep(a, ph, slot, n_src, i, pi, h, rows, l);
                    } else {
                        for (int t_lo = 0; t_lo < bound; t_lo += VS_TILE) {
                            n_src = vs_stage(a, Pj, Vj, Mj, t_lo, min(t_lo + VS_TILE, bound), ph, slot, wave_cnt);
                            if (focal) vs_sweep(a, ph, slot, n_src, i, pi, h, rows, l);
                            __syncthreads();  // every lane is done with this tile before the next one is staged
                        }
                    }
                    if (focal) {
                        ++n_focal;
                        n_pairs += l.pairs;
                        if (lag0) {
                            atomicAdd(rows + o_nn + l.nn_cell, 1u);
                            const float b = floorf(l.min_a / a.gap_bin);
                            const bool in_range = b < (float)GB;
                            atomicAdd(rows + o_gap + (in_range ? (int)b : GB), 1u);
                            if (in_range) atomicAdd(spd + (int)b, (unsigned long long)llrintf(sp * VS_Q));
                        }
                    }
                }
                __syncthreads();              // fslot is rewritten by the next focal tile
            }
            // the slice's counters: lanes, then one 64-bit LDS add per wave
            const unsigned long long f = wave_sum((unsigned long long)n_focal);
            const unsigned long long p = wave_sum((unsigned long long)n_pairs);
            if (lane == 0) {
                atomicAdd(cnt, f);
                atomicAdd(cnt + 1, p);
            }
            __syncthreads();                  // rows and counters complete; the tile is free for the next slice
        }
    }
}

__global__ void __launch_bounds__(VS_THREADS) view_stats_copy_kernel(ViewArgs a) {
    const long long S = a.S, K1 = a.K1, GG = (long long)a.G * a.G, GB = a.GB;
    const long long n0 = S * K1, n2 = n0 * 4 * GG, n3 = S * (GG + 1), n4 = S * (GB + 1), n5 = S * GB;
    const long long total = 2 * n0 + n2 + n3 + n4 + n5;
    for (long long e = (long long)blockIdx.x * VS_THREADS + threadIdx.x; e < total; e += (long long)gridDim.x * VS_THREADS) {
        const long long v = (long long)a.ws[e];
        long long q = e;
        if (q < n0) { a.focal[q] = v; continue; }
        q -= n0;
        if (q < n0) { a.pairs[q] = v; continue; }
        q -= n0;
        if (q < n2) { a.map[q] = v; continue; }
        q -= n2;
        if (q < n3) { a.nn_map[q] = v; continue; }
        q -= n3;
        if (q < n4) { a.front_gap[q] = v; continue; }
        q -= n4;
        a.front_speed[q] = v;
    }
}

static long long vs_workspace_elems(long long S, long long K1, long long GG, long long GB) {
    return S * (2 * K1 + K1 * 4 * GG + (GG + 1) + (GB + 1) + GB);
}

}  // namespace piml

using namespace piml;

PIML_API long long piml_view_stats_workspace_bytes(int S, int K, int half, int gap_bins) {
    if (S < 0 || K < 0 || half < 0 || gap_bins < 0) return -1;
    return vs_workspace_elems(S, (long long)K + 1, 4ll * half * half, gap_bins) * (long long)sizeof(unsigned long long);
}

PIML_API int piml_view_stats(const float* P, const float* V, const float* M, const int* n_active, int S, int T, int N,
                             int t0, int t1, const int* lags, int K, float v_min, float cell, int half, float cos_same,
                             float r_max, float corridor, float gap_bin, int gap_bins, int has_box, float x0, float x1,
                             float y0, float y1, long long* focal, long long* pairs, long long* map, long long* nn_map,
                             long long* front_gap, long long* front_speed, void* workspace, long long workspace_bytes,
                             void* stream) {
    const auto positive = [](float x) { return x > 0.f && std::isfinite(x); };
    if (S <= 0 || T <= 0 || N <= 0 || N > VS_MAX_N || t0 < 0 || t1 > T || t1 <= t0 || K < 0 || K > VS_MAX_LAGS ||
        (K > 0 && !lags) || !positive(v_min) || !positive(cell) || half < 1 || half > VS_MAX_HALF ||
        !(cos_same >= 0.f && cos_same <= 1.f) || std::isnan(r_max) || !positive(corridor) || !positive(gap_bin) ||
        gap_bins < 1 || gap_bins > VS_MAX_BINS)
        return hipErrorInvalidValue;
    for (int k = 0; k < K; ++k)
        if (lags[k] <= 0 || (k > 0 && lags[k] <= lags[k - 1])) return hipErrorInvalidValue;
    if (has_box && (!std::isfinite(x0) || !std::isfinite(x1) || !std::isfinite(y0) || !std::isfinite(y1) || !(x0 < x1) ||
                    !(y0 < y1)))
        return hipErrorInvalidValue;
    if (!P || !V || !M || !focal || !pairs || !map || !nn_map || !front_gap || !front_speed || !workspace)
        return hipErrorInvalidValue;
    const long long need = piml_view_stats_workspace_bytes(S, K, half, gap_bins);
    if (workspace_bytes < need) return hipErrorInvalidValue;
    ViewArgs a{};
    a.P = P, a.V = V, a.M = M, a.n_active = n_active;
    a.S = S, a.T = T, a.N = N, a.t0 = t0, a.Tp = t1 - t0, a.K1 = K + 1, a.G = 2 * half, a.GB = gap_bins;
    a.lag[0] = 0;
    for (int k = 0; k < K; ++k) a.lag[k + 1] = lags[k];
    a.off[0] = 0;
    for (int k = 0; k <= K; ++k) a.off[k + 1] = a.off[k] + (a.Tp > a.lag[k] ? a.Tp - a.lag[k] : 0);
    for (int k = K + 2; k < VS_MAX_LAGS + 2; ++k) a.off[k] = a.off[K + 1];
    a.per_member = a.off[K + 1];
    a.slices = (long long)S * a.per_member;
    const unsigned grid = stats_run_grid(a.slices, VS_TARGET_WG, VS_MAX_RUN, VS_MAX_GRID, &a.run);
    a.has_box = has_box ? 1 : 0;
    a.x0 = x0, a.x1 = x1, a.y0 = y0, a.y1 = y1;
    a.has_rmax = r_max > 0.f ? 1 : 0;
    a.r_max = r_max;
    a.v_min = v_min, a.cell = cell, a.X = cell * (float)half, a.cos_same = cos_same, a.corridor = corridor;
    a.gap_bin = gap_bin;
    a.ws = static_cast<unsigned long long*>(workspace);
    a.focal = focal, a.pairs = pairs, a.map = map, a.nn_map = nn_map, a.front_gap = front_gap, a.front_speed = front_speed;
    hipStream_t st = as_stream(stream);
    hipError_t e = hipMemsetAsync(workspace, 0, (size_t)need, st);
    if (e != hipSuccess) return e;
    if (grid > 0) {
        hipLaunchKernelGGL(view_stats_kernel, dim3(grid), dim3(VS_THREADS), 0, st, a);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const long long elems = need / (long long)sizeof(unsigned long long);
    const long long blocks = (elems + VS_THREADS - 1) / VS_THREADS;
    hipLaunchKernelGGL(view_stats_copy_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(VS_THREADS), 0, st, a);
    return hipGetLastError();
}
