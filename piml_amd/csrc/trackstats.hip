// Track (Lagrangian) statistics of crowds: what an agent does along its own track -- the autocorrelation of
// its heading and its mean squared displacement over n_lags frame lags, the histogram of its frame-to-frame acceleration,
// and one row per track (frames, steps, first and last frame, path length, net displacement) -- for S members in one call.
// Slot n of member s is one agent for the whole run, so a track is column (s, :, n) of P and M; velocities are not an input.
//
// Agent i takes part at (s, t) when M == 1 and both coordinates of P are finite and below 65536 in magnitude; slots at or
// past n_active[s] are not swept.  Window frames t = 0 .. T' - 1, float32 with true divisions and square roots and no
// contraction, Q = 2^20:
//   step (i, t): i takes part at t and t + 1; u = p(t+1) - p(t), l = sqrt(ux^2 + uy^2); a mover when l / dt >= v_min, with
//       the heading h = u / l;
//   (a) lags L = 1 .. n_lags, every t where steps t and t + L are movers: ac_n[L-1] += 1, ac_sum[L-1] += llrintf((h_t.h_{t+L}) Q);
//   (b) every t where i takes part at t and t + L: d = p(t+L) - p(t), d2 = dx^2 + dy^2; sqrt(d2) < d_max: msd_n[L-1] += 1,
//       msd_sum[L-1] += llrintf(d2 Q); otherwise msd_far[L-1] += 1;
//   (c) every t where steps t and t + 1 exist: a = sqrt(|u_{t+1} - u_t|^2) / dt / dt, acc[min(floor(a / acc_bin), acc_bins)] += 1,
//       and acc_sum += llrintf(a Q) when a < acc_bin * acc_bins;
//   (d) per track: frames, steps, first and last participating frame (-1 without one), path = sum llrintf(l Q), net =
//       llrintf(|p(last) - p(first)| Q) (0 with fewer than two frames).
//
// track_stats_kernel: one workgroup of TS_THREADS lanes per track (member, slot), tracks taken grid-stride.  A scan of the
// window's mask (and the positions where the mask is 1) gives first, last and the frame count; frames outside [first, last]
// are not looked at again.  The span is staged into LDS in tiles of TS_TILE frames plus a halo of n_lags + 1, 16 B per frame:
// position, then heading of the step that starts there (position x NaN: absent; heading x NaN: no mover), the headings
// computed once per step from the staged positions.  Lanes own lags: in a pass lane k owns lag L = pass * TS_THREADS + k + 1;
// for frame t it reads entry t as a broadcast and entry t + L at unit stride (16 B per lane: the b128 read's four-bank
// groups do not collide), and keeps ac_n, ac_sum, msd_n, msd_sum, msd_far in registers over all tiles of the pass; they
// reach the member's workspace row once per track and lag, with 64-bit integer atomics, only when non-zero.  A lane stops at
// t = last - L, so a short track costs its own span squared, not the window.  In pass 0 the same staged tile serves (c) and
// the sums of (d) in one O(span) sweep: the acceleration histogram in an LDS row (u32), flushed per track.
// track_stats_copy_kernel moves the workspace into the outputs.  Every output is an integer and every atomic an integer
// add, so the results are bitwise reproducible whatever the order of the adds.
//
// sqrt(d2) < d_max is evaluated as d2 < near2, near2 the smallest float32 whose correctly rounded square root is >= d_max
// (found on the host; sqrtf is monotonic): the same predicate without a square root per pair.
#include "common.hpp"
#include "../../include/piml_hip.h"

#include <cmath>

namespace piml {

constexpr int TS_THREADS = PIML_TRACK_LAG_LANES;   // lags per pass
constexpr int TS_WAVES = TS_THREADS / 64;
constexpr int TS_TILE = PIML_TRACK_TILE;           // frames per staged tile (without the halo)
constexpr int TS_MAX_LAGS = PIML_TRACK_MAX_LAGS;
constexpr int TS_ENTRIES = TS_TILE + TS_MAX_LAGS + 1;
constexpr int TS_MAX_BINS = 256;
constexpr int TS_MAX_N = 65536;
constexpr float TS_Q = 1048576.f;                  // 2^20
constexpr float TS_MAX_COORD = 65536.f;
constexpr float TS_MAX_D = 1024.f;
constexpr int TS_MAX_FRAMES = 1 << 25;            // a track's path: fewer than 2^25 steps below 2^37.5 units each
constexpr long long TS_MAX_GRID = 1 << 20;
constexpr int TS_ROWS = 5;                         // ac_n, ac_sum, msd_n, msd_sum, msd_far

struct TrackArgs {
    const float *P, *M;                            // (S, T, N, 2), (S, T, N)
    const int* n_active;                           // (S) or NULL
    int S, T, N, t0, Tp, NL, AB;
    float dt, v_min, near2, acc_bin, acc_top;      // acc_top = acc_bin * acc_bins
    unsigned long long* ws;                        // 5 rows (S, NL) | acc (S, AB + 1) | acc_sum (S)
    long long* lag[TS_ROWS];                       // (S, NL)
    long long *acc, *acc_sum;                      // (S, AB + 1), (S)
    long long *trk_frames, *trk_steps, *trk_first, *trk_last, *trk_path, *trk_net;      // (S, N)
};

__device__ __forceinline__ bool ts_participant(float m, float2 p) {
    return m == 1.f && fabsf(p.x) < TS_MAX_COORD && fabsf(p.y) < TS_MAX_COORD;
}


__global__ void __launch_bounds__(TS_THREADS) track_stats_kernel(TrackArgs a) {
    __shared__ float4 e[TS_ENTRIES];
    __shared__ unsigned h_acc[TS_MAX_BINS + 1];
    __shared__ long long red[3][TS_WAVES];
    __shared__ int span[3][TS_WAVES];
    float2* e2 = reinterpret_cast<float2*>(e);    // entry k: position e2[2 k], heading e2[2 k + 1]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int NL = a.NL, AB = a.AB, Tp = a.Tp;
    for (int k = tid; k <= TS_MAX_BINS; k += TS_THREADS) h_acc[k] = 0u;
    __syncthreads();
    const long long tracks = (long long)a.S * a.N;
    unsigned long long* w_acc = a.ws + (long long)TS_ROWS * a.S * NL;
    unsigned long long* w_acc_sum = w_acc + (long long)a.S * (AB + 1);
    for (long long tr = blockIdx.x; tr < tracks; tr += gridDim.x) {
        const int s = (int)(tr / a.N), i = (int)(tr - (long long)s * a.N);
        int bound = a.N;
        if (a.n_active) bound = min(max(a.n_active[s], 0), a.N);
        const long long frame0 = (long long)s * a.T + a.t0;
        const float2* P = reinterpret_cast<const float2*>(a.P) + frame0 * a.N + i;      // frame t of the window: P[t * N]
        const float* M = a.M + frame0 * a.N + i;
        // the track's span: first, last, frames
        int first = Tp, last = -1, frames = 0;
        if (i < bound) {
            for (int t = tid; t < Tp; t += TS_THREADS) {
                const float m = M[(long long)t * a.N];
                if (m == 1.f && ts_participant(m, P[(long long)t * a.N])) {
                    first = min(first, t);
                    last = t;
                    ++frames;
                }
            }
        }
        first = wave_min(first), last = wave_max(last), frames = (int)wave_sum(frames);
        if (lane == 0) span[0][w] = first, span[1][w] = last, span[2][w] = frames;
        __syncthreads();
        first = span[0][0], last = span[1][0], frames = span[2][0];
#pragma unroll
        for (int q = 1; q < TS_WAVES; ++q) first = min(first, span[0][q]), last = max(last, span[1][q]), frames += span[2][q];
        __syncthreads();                           // span is rewritten by the next track
        if (frames == 0) {
            if (tid == 0) {
                a.trk_frames[tr] = 0, a.trk_steps[tr] = 0, a.trk_first[tr] = -1, a.trk_last[tr] = -1;
                a.trk_path[tr] = 0, a.trk_net[tr] = 0;
            }
            continue;
        }
        long long steps = 0, path = 0, acc_sum = 0;
        for (int L0 = 0; L0 < NL; L0 += TS_THREADS) {
            const int L = L0 + tid + 1;
            const bool owns = L <= NL;
            unsigned ac_n = 0, msd_n = 0, msd_far = 0;
            long long ac_sum = 0, msd_sum = 0;
            for (int c0 = first; c0 <= last; c0 += TS_TILE) {
                // positions of frames c0 .. c0 + TS_TILE + NL (NaN past `last`), then the headings of the steps
                const int staged = TS_TILE + NL + 1;
                for (int k = tid; k < staged; k += TS_THREADS) {
                    const int t = c0 + k;
                    float2 p = make_float2(NAN, NAN);
                    if (t <= last) {
                        const float m = M[(long long)t * a.N];
                        const float2 q = m == 1.f ? P[(long long)t * a.N] : p;
                        if (ts_participant(m, q)) p = q;
                    }
                    e[k] = make_float4(p.x, p.y, NAN, 0.f);
                }
                __syncthreads();
                for (int k = tid; k < staged - 1; k += TS_THREADS) {
                    const float2 p0 = e2[2 * k], p1 = e2[2 * k + 2];          // positions only: the headings are being written
                    if (isnan(p0.x) || isnan(p1.x)) continue;
                    const float ux = p1.x - p0.x, uy = p1.y - p0.y;
                    const float l = sqrtf(ux * ux + uy * uy);
                    if (l / a.dt >= a.v_min) e2[2 * k + 1] = make_float2(ux / l, uy / l);
                }
                __syncthreads();
                const int core = min(TS_TILE, last - c0 + 1);
                // the lag sweep: frames t = c0 .. c0 + core - 1 with t + L <= last
                if (owns) {
                    const int n_t = min(core, last - L - c0 + 1);
                    const float near2 = a.near2;
                    for (int k = 0; k < n_t; ++k) {
                        const float4 p = e[k];
                        if (isnan(p.x)) continue;
                        const float4 q = e[k + L];
                        if (isnan(q.x)) continue;
                        const float dx = q.x - p.x, dy = q.y - p.y;
                        const float d2 = dx * dx + dy * dy;
                        if (d2 < near2) {
                            ++msd_n;
                            msd_sum += llrintf(d2 * TS_Q);
                        } else {
                            ++msd_far;
                        }
                        if (!isnan(p.z) && !isnan(q.z)) {
                            const float c = p.z * q.z + p.w * q.w;
                            ++ac_n;
                            ac_sum += llrintf(c * TS_Q);
                        }
                    }
                }
                // steps, path and acceleration items of the core frames
                if (L0 == 0) {
                    for (int k = tid; k < core; k += TS_THREADS) {
                        const float2 p0 = e2[2 * k], p1 = e2[2 * k + 2], p2 = e2[2 * k + 4];
                        if (isnan(p0.x) || isnan(p1.x)) continue;
                        const float ux = p1.x - p0.x, uy = p1.y - p0.y;
                        const float l = sqrtf(ux * ux + uy * uy);
                        ++steps;
                        path += llrintf(l * TS_Q);
                        if (isnan(p2.x)) continue;
                        const float gx = (p2.x - p1.x) - ux, gy = (p2.y - p1.y) - uy;
                        const float acc = sqrtf(gx * gx + gy * gy) / a.dt / a.dt;
                        const float qb = floorf(acc / a.acc_bin);
                        atomicAdd(h_acc + (qb < (float)AB ? (int)qb : AB), 1u);
                        if (acc < a.acc_top) acc_sum += llrintf(acc * TS_Q);
                    }
                }
                __syncthreads();                   // every lane is done with this tile before the next one is staged
            }
            if (owns) {
                unsigned long long* row = a.ws + (long long)s * NL + (L - 1);
                const long long stride = (long long)a.S * NL;
                if (ac_n) atomicAdd(row, (unsigned long long)ac_n);
                if (ac_sum) atomicAdd(row + stride, (unsigned long long)ac_sum);
                if (msd_n) atomicAdd(row + 2 * stride, (unsigned long long)msd_n);
                if (msd_sum) atomicAdd(row + 3 * stride, (unsigned long long)msd_sum);
                if (msd_far) atomicAdd(row + 4 * stride, (unsigned long long)msd_far);
            }
        }
        // the track's row and its acceleration items
        steps = wave_sum(steps), path = wave_sum(path), acc_sum = wave_sum(acc_sum);
        if (lane == 0) red[0][w] = steps, red[1][w] = path, red[2][w] = acc_sum;
        __syncthreads();                           // red and h_acc complete
        if (tid == 0) {
            steps = path = acc_sum = 0;
            for (int q = 0; q < TS_WAVES; ++q) steps += red[0][q], path += red[1][q], acc_sum += red[2][q];
            long long net = 0;
            if (frames >= 2) {
                const float2 pf = P[(long long)first * a.N], pl = P[(long long)last * a.N];
                const float dx = pl.x - pf.x, dy = pl.y - pf.y;
                net = llrintf(sqrtf(dx * dx + dy * dy) * TS_Q);
            }
            a.trk_frames[tr] = frames, a.trk_steps[tr] = steps, a.trk_first[tr] = first, a.trk_last[tr] = last;
            a.trk_path[tr] = path, a.trk_net[tr] = net;
            if (acc_sum) atomicAdd(w_acc_sum + s, (unsigned long long)acc_sum);
        }
        for (int b = tid; b <= AB; b += TS_THREADS) {
            const unsigned c = h_acc[b];
            if (!c) continue;
            atomicAdd(w_acc + (long long)s * (AB + 1) + b, (unsigned long long)c);
            h_acc[b] = 0u;
        }
        __syncthreads();                           // red and h_acc free for the next track
    }
}

__global__ void __launch_bounds__(256) track_stats_copy_kernel(TrackArgs a) {
    const long long n0 = (long long)a.S * a.NL, n1 = (long long)a.S * (a.AB + 1);
    const long long total = TS_ROWS * n0 + n1 + a.S;
    for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < total; k += (long long)gridDim.x * 256) {
        const long long v = (long long)a.ws[k];
        if (k < TS_ROWS * n0) {
            const int row = (int)(k / n0);
            long long* dst = a.lag[0];
#pragma unroll
            for (int r = 1; r < TS_ROWS; ++r) dst = row == r ? a.lag[r] : dst;
            dst[k - row * n0] = v;
        } else if (k < TS_ROWS * n0 + n1) {
            a.acc[k - TS_ROWS * n0] = v;
        } else {
            a.acc_sum[k - TS_ROWS * n0 - n1] = v;
        }
    }
}

}  // namespace piml

using namespace piml;

PIML_API long long piml_track_stats_workspace_bytes(int S, int n_lags, int acc_bins) {
    if (S < 0 || n_lags < 0 || acc_bins < 0) return -1;
    return (long long)S * (5ll * n_lags + acc_bins + 2ll) * (long long)sizeof(unsigned long long);
}

PIML_API int piml_track_stats(const float* P, const float* M, const int* n_active, int S, int T, int N, int t0, int t1, float dt,
                              float v_min, int n_lags, float d_max, float acc_bin, int acc_bins, long long* ac_n,
                              long long* ac_sum, long long* msd_n, long long* msd_sum, long long* msd_far, long long* acc,
                              long long* acc_sum, long long* trk_frames, long long* trk_steps, long long* trk_first,
                              long long* trk_last, long long* trk_path, long long* trk_net, void* workspace,
                              long long workspace_bytes, void* stream) {
    const auto positive = [](float x) { return x > 0.f && std::isfinite(x); };
    if (S < 0 || T < 0 || N < 0 || N > TS_MAX_N || t0 < 0 || t1 > T || t1 < t0 || !positive(dt) || !positive(v_min) ||
        !positive(d_max) || d_max > TS_MAX_D || !positive(acc_bin) || n_lags < 1 || n_lags > TS_MAX_LAGS || acc_bins < 1 ||
        acc_bins > TS_MAX_BINS || t1 - t0 > TS_MAX_FRAMES)
        return hipErrorInvalidValue;
    // No 64-bit sum overflows: a member's msd_sum row adds at most N T' terms below d_max^2 Q, its acc_sum at most N T' terms
    // below acc_bin acc_bins Q; T' <= 2^25 bounds trk_path and, with N <= 2^16, ac_sum (DESIGN 4.22 "No overflow").
    const float acc_top = acc_bin * (float)acc_bins;
    const double items = (double)N * (double)(t1 - t0), two63 = 9223372036854775808.0;
    if (!std::isfinite(acc_top) || !((double)d_max * d_max * (double)TS_Q * items < two63) ||
        !((double)acc_top * (double)TS_Q * items < two63))
        return hipErrorInvalidValue;
    if (S == 0 || t1 == t0 || N == 0) return hipSuccess;
    if (!P || !M || !ac_n || !ac_sum || !msd_n || !msd_sum || !msd_far || !acc || !acc_sum || !trk_frames || !trk_steps ||
        !trk_first || !trk_last || !trk_path || !trk_net || !workspace)
        return hipErrorInvalidValue;
    const long long need = piml_track_stats_workspace_bytes(S, n_lags, acc_bins);
    if (workspace_bytes < need) return hipErrorInvalidValue;
    TrackArgs a{};
    a.P = P, a.M = M, a.n_active = n_active;
    a.S = S, a.T = T, a.N = N, a.t0 = t0, a.Tp = t1 - t0, a.NL = n_lags, a.AB = acc_bins;
    a.dt = dt, a.v_min = v_min, a.acc_bin = acc_bin, a.acc_top = acc_top;
    // near2: the smallest float32 whose correctly rounded square root is >= d_max, so sqrtf(d2) < d_max <=> d2 < near2
    float near2 = (float)((double)d_max * (double)d_max);
    while (near2 > 0.f && std::sqrt(near2) >= d_max) near2 = std::nextafter(near2, 0.f);
    while (std::sqrt(near2) < d_max) near2 = std::nextafter(near2, INFINITY);
    a.near2 = near2;
    a.ws = static_cast<unsigned long long*>(workspace);
    a.lag[0] = ac_n, a.lag[1] = ac_sum, a.lag[2] = msd_n, a.lag[3] = msd_sum, a.lag[4] = msd_far;
    a.acc = acc, a.acc_sum = acc_sum;
    a.trk_frames = trk_frames, a.trk_steps = trk_steps, a.trk_first = trk_first, a.trk_last = trk_last;
    a.trk_path = trk_path, a.trk_net = trk_net;
    hipStream_t st = as_stream(stream);
    hipError_t err = hipMemsetAsync(workspace, 0, (size_t)need, st);
    if (err != hipSuccess) return err;
    const long long tracks = (long long)S * N;
    hipLaunchKernelGGL(track_stats_kernel, dim3((unsigned)(tracks < TS_MAX_GRID ? tracks : TS_MAX_GRID)), dim3(TS_THREADS), 0,
                       st, a);
    err = hipGetLastError();
    if (err != hipSuccess) return err;
    const long long elems = need / (long long)sizeof(unsigned long long);
    const long long blocks = (elems + 255) / 256;
    hipLaunchKernelGGL(track_stats_copy_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, a);
    return hipGetLastError();
}
