// Measurement-line statistics of crowds: who crosses a line, when, how fast and where along it -- the N-t curve,
// the flow, the crossing speed and the lateral profile per line and direction, and per track and line the number of
// crossings and the time and direction of the first one -- for S members in one call against L <= 16 shared lines.  Slot n of
// member s is one agent for the whole run; velocities are not an input.
//
// Agent i takes part at (s, t) when M == 1 and both coordinates of P are finite and below 65536 in magnitude; slots at or
// past n_active[s] are not swept.  Window frames t = 0 .. T' - 1.  A step (i, t) exists when i takes part at t and t + 1 and
// t + 1 < T': no step spans a gap.  float32 with true divisions and square roots and no contraction, Q = 2^20.  Per line
// (ax, ay, bx, by), d = b - a, len2 = dx dx + dy dy, side(p) = dx (py - ay) - dy (px - ax), and for a step s0 = side(p(t)),
// s1 = side(p(t+1)):
//   direction 0 when s0 < 0 and s1 >= 0, direction 1 when s0 >= 0 and s1 < 0 (a point on the line belongs to the left side);
//   f = s0 / (s0 - s1), u = p(t+1) - p(t), c = p(t) + f u, w = ((cx - ax) dx + (cy - ay) dy) / len2;
//   a crossing when 0 <= w < 1; vn = |s1 - s0| / sqrt(len2) / dt; tc = t Q + llrintf(f Q).
// Per crossing: cross[dir] += 1, nt[dir][t] += 1, speed[dir][min(floor(vn / v_bin), v_bins)] += 1, speed_sum[dir] +=
// llrintf(vn Q) when vn < v_bin v_bins, profile[dir][min(floor(w w_bins), w_bins - 1)] += 1, the track's count += 1 and its
// first-crossing word = min(word, 2 tc + dir): time and direction of the first crossing come from the same step, and of two
// crossings at the same tc (a step that ends on the line and the next that leaves it backwards) direction 0 is the first.
//
// line_stats_kernel: one lane per track over a chunk of LS_CHUNK steps -- lanes of a workgroup are neighbouring slots, so
// every frame is read at unit stride --, work items (member, chunk, block of slots) taken grid-stride.  The lines and what
// derives from them (d, len2, sqrt(len2)) are computed once per workgroup into LDS and read as broadcasts.  A lane carries
// p(t+1) over to the next step.  Crossings are sparse, so every row takes 64-bit integer atomics in the member's workspace
// directly; the first-crossing word is kept as 2^62 - word under an atomic maximum, so that the zeroed workspace means
// "none".  line_stats_copy_kernel moves the workspace into the outputs and unpacks the word.  Every output is an integer and
// every atomic an integer add or maximum, so the results are bitwise reproducible whatever the order.
#include "common.hpp"
#include "../../include/piml_hip.h"

#include <cmath>

namespace piml {

constexpr int LS_THREADS = 256;
constexpr int LS_CHUNK = PIML_LINE_CHUNK;          // steps per lane and work item
constexpr int LS_MAX_L = PIML_LINE_MAX_L;
constexpr int LS_MAX_BINS = 256;
constexpr int LS_MAX_N = 65536;
constexpr float LS_Q = 1048576.f;                  // 2^20
constexpr float LS_MAX_COORD = 65536.f;
constexpr int LS_MAX_FRAMES = 1 << 25;             // tc < 2^45, the packed word below 2^46
constexpr long long LS_MAX_GRID = 1 << 20;
constexpr unsigned long long LS_KEY_TOP = 1ull << 62;

struct LineArgs {
    const float *P, *M, *lines;                    // (S, T, N, 2), (S, T, N), (L, 4)
    const int* n_active;                           // (S) or NULL
    int S, T, N, t0, Tp, L, VB, WB;
    int NB, NC;                                    // blocks of slots, chunks of steps
    float dt, v_bin, v_top;                        // v_top = v_bin * v_bins
    unsigned long long* ws;
    // workspace segments, each laid out as its output: cross (S, L, 2) | nt (S, L, 2, T') | speed (S, L, 2, VB + 1) |
    // speed_sum (S, L, 2) | profile (S, L, 2, WB) | steps (S) | trk_steps (S, N) | trk_count (S, L, N) | key (S, L, N)
    long long o_nt, o_speed, o_ssum, o_prof, o_steps, o_tsteps, o_count, o_key, total;
    long long *cross, *nt, *speed, *speed_sum, *profile, *steps, *trk_steps, *trk_count, *trk_first, *trk_dir;
};

__device__ __forceinline__ bool ls_participant(float m, float2 p) {
    return m == 1.f && fabsf(p.x) < LS_MAX_COORD && fabsf(p.y) < LS_MAX_COORD;
}


__global__ void __launch_bounds__(LS_THREADS) line_stats_kernel(LineArgs a) {
    __shared__ float ln[LS_MAX_L][8];              // ax, ay, dx, dy, len2, sqrt(len2)
    const int tid = threadIdx.x, lane = tid & 63;
    const int L = a.L, Tp = a.Tp, VB = a.VB, WB = a.WB;
    if (tid < L) {
        const float ax = a.lines[4 * tid], ay = a.lines[4 * tid + 1];
        const float dx = a.lines[4 * tid + 2] - ax, dy = a.lines[4 * tid + 3] - ay;
        const float len2 = dx * dx + dy * dy;
        ln[tid][0] = ax, ln[tid][1] = ay, ln[tid][2] = dx, ln[tid][3] = dy, ln[tid][4] = len2, ln[tid][5] = sqrtf(len2);
    }
    __syncthreads();
    const long long items = (long long)a.S * a.NC * a.NB;
    for (long long w = blockIdx.x; w < items; w += gridDim.x) {
        const int ab = (int)(w % a.NB);
        const long long r = w / a.NB;
        const int c = (int)(r % a.NC), s = (int)(r / a.NC);
        const int i = ab * LS_THREADS + tid;
        int bound = a.N;
        if (a.n_active) bound = min(max(a.n_active[s], 0), a.N);
        const int c0 = c * LS_CHUNK, c1 = min(c0 + LS_CHUNK, Tp - 1);        // steps t = c0 .. c1 - 1
        long long steps = 0;
        if (i < bound) {
            const long long frame0 = (long long)s * a.T + a.t0;
            const float2* P = reinterpret_cast<const float2*>(a.P) + frame0 * a.N + i;  // frame t of the window: P[t * N]
            const float* M = a.M + frame0 * a.N + i;
            float2 p0 = P[(long long)c0 * a.N];
            bool part0 = ls_participant(M[(long long)c0 * a.N], p0);
            const long long row = (long long)s * L;                         // (s, l) = row + l
            for (int t = c0; t < c1; ++t) {
                const float2 p1 = P[(long long)(t + 1) * a.N];
                const bool part1 = ls_participant(M[(long long)(t + 1) * a.N], p1);
                if (part0 && part1) {
                    ++steps;
                    const float ux = p1.x - p0.x, uy = p1.y - p0.y;
                    for (int l = 0; l < L; ++l) {
                        const float ax = ln[l][0], ay = ln[l][1], dx = ln[l][2], dy = ln[l][3];
                        const float s0 = dx * (p0.y - ay) - dy * (p0.x - ax);
                        const float s1 = dx * (p1.y - ay) - dy * (p1.x - ax);
                        const bool fwd = s0 < 0.f && s1 >= 0.f, back = s0 >= 0.f && s1 < 0.f;
                        if (!(fwd || back)) continue;
                        const float f = s0 / (s0 - s1);
                        const float cx = p0.x + f * ux, cy = p0.y + f * uy;
                        const float len2 = ln[l][4];
                        const float wl = ((cx - ax) * dx + (cy - ay) * dy) / len2;
                        if (!(wl >= 0.f && wl < 1.f)) continue;
                        const int dir = fwd ? 0 : 1;
                        const float vn = fabsf(s1 - s0) / ln[l][5] / a.dt;
                        const long long tc = (long long)t * (long long)LS_Q + llrintf(f * LS_Q);
                        const long long rd = (row + l) * 2 + dir;
                        atomicAdd(a.ws + rd, 1ull);
                        atomicAdd(a.ws + a.o_nt + rd * Tp + t, 1ull);
                        const float qv = floorf(vn / a.v_bin);
                        atomicAdd(a.ws + a.o_speed + rd * (VB + 1) + (qv < (float)VB ? (int)qv : VB), 1ull);
                        if (vn < a.v_top) atomicAdd(a.ws + a.o_ssum + rd, (unsigned long long)llrintf(vn * LS_Q));
                        const float qw = floorf(wl * (float)WB);
                        atomicAdd(a.ws + a.o_prof + rd * WB + (qw < (float)(WB - 1) ? (int)qw : WB - 1), 1ull);
                        const long long trk = (row + l) * a.N + i;
                        atomicAdd(a.ws + a.o_count + trk, 1ull);
                        atomicMax(a.ws + a.o_key + trk, LS_KEY_TOP - (unsigned long long)(2 * tc + dir));
                    }
                }
                p0 = p1, part0 = part1;
            }
            if (steps) atomicAdd(a.ws + a.o_tsteps + (long long)s * a.N + i, (unsigned long long)steps);
        }
        steps = wave_sum(steps);
        if (lane == 0 && steps) atomicAdd(a.ws + a.o_steps + s, (unsigned long long)steps);
    }
}

__global__ void __launch_bounds__(256) line_stats_copy_kernel(LineArgs a) {
    for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < a.total; k += (long long)gridDim.x * 256) {
        const unsigned long long v = a.ws[k];
        if (k < a.o_nt) {
            a.cross[k] = (long long)v;
        } else if (k < a.o_speed) {
            a.nt[k - a.o_nt] = (long long)v;
        } else if (k < a.o_ssum) {
            a.speed[k - a.o_speed] = (long long)v;
        } else if (k < a.o_prof) {
            a.speed_sum[k - a.o_ssum] = (long long)v;
        } else if (k < a.o_steps) {
            a.profile[k - a.o_prof] = (long long)v;
        } else if (k < a.o_tsteps) {
            a.steps[k - a.o_steps] = (long long)v;
        } else if (k < a.o_count) {
            a.trk_steps[k - a.o_tsteps] = (long long)v;
        } else if (k < a.o_key) {
            a.trk_count[k - a.o_count] = (long long)v;
        } else {
            const unsigned long long word = LS_KEY_TOP - v;                  // v == 0: no crossing
            a.trk_first[k - a.o_key] = v ? (long long)(word >> 1) : -1ll;
            a.trk_dir[k - a.o_key] = v ? (long long)(word & 1ull) : -1ll;
        }
    }
}

}  // namespace piml

using namespace piml;

PIML_API long long piml_line_stats_workspace_bytes(int S, int N, int L, int frames, int v_bins, int w_bins) {
    if (S < 0 || N < 0 || L < 0 || frames < 0 || v_bins < 0 || w_bins < 0) return -1;
    const long long per_dir = 2ll + frames + (v_bins + 1ll) + w_bins;       // cross, speed_sum | nt | speed | profile
    return (long long)S * (2ll * L * per_dir + 1ll + N + 2ll * L * N) * (long long)sizeof(unsigned long long);
}

PIML_API int piml_line_stats(const float* P, const float* M, const int* n_active, int S, int T, int N, int t0, int t1,
                             const float* lines, int L, float dt, float v_bin, int v_bins, int w_bins, long long* cross,
                             long long* nt, long long* speed, long long* speed_sum, long long* profile, long long* steps,
                             long long* trk_steps, long long* trk_count, long long* trk_first, long long* trk_dir,
                             void* workspace, long long workspace_bytes, void* stream) {
    const auto positive = [](float x) { return x > 0.f && std::isfinite(x); };
    if (S < 0 || T < 0 || N < 0 || N > LS_MAX_N || L < 0 || L > LS_MAX_L || t0 < 0 || t1 > T || t1 < t0 || !positive(dt) ||
        !positive(v_bin) || v_bins < 1 || v_bins > LS_MAX_BINS || w_bins < 1 || w_bins > LS_MAX_BINS ||
        t1 - t0 > LS_MAX_FRAMES)
        return hipErrorInvalidValue;
    // No 64-bit sum overflows: a (member, line, direction) speed_sum adds at most N T' terms below v_bin v_bins Q.
    const float v_top = v_bin * (float)v_bins;
    const double items = (double)N * (double)(t1 - t0), two63 = 9223372036854775808.0;
    if (!std::isfinite(v_top) || !((double)v_top * (double)LS_Q * items < two63)) return hipErrorInvalidValue;
    if (S == 0 || t1 == t0 || N == 0 || L == 0) return hipSuccess;
    if (!P || !M || !lines || !cross || !nt || !speed || !speed_sum || !profile || !steps || !trk_steps || !trk_count ||
        !trk_first || !trk_dir || !workspace)
        return hipErrorInvalidValue;
    const int Tp = t1 - t0;
    const long long need = piml_line_stats_workspace_bytes(S, N, L, Tp, v_bins, w_bins);
    if (workspace_bytes < need) return hipErrorInvalidValue;
    LineArgs a{};
    a.P = P, a.M = M, a.lines = lines, a.n_active = n_active;
    a.S = S, a.T = T, a.N = N, a.t0 = t0, a.Tp = Tp, a.L = L, a.VB = v_bins, a.WB = w_bins;
    a.NB = (N + LS_THREADS - 1) / LS_THREADS, a.NC = (Tp - 1 + LS_CHUNK - 1) / LS_CHUNK;
    a.dt = dt, a.v_bin = v_bin, a.v_top = v_top;
    a.ws = static_cast<unsigned long long*>(workspace);
    const long long rows = 2ll * S * L;
    a.o_nt = rows;
    a.o_speed = a.o_nt + rows * Tp;
    a.o_ssum = a.o_speed + rows * (v_bins + 1);
    a.o_prof = a.o_ssum + rows;
    a.o_steps = a.o_prof + rows * w_bins;
    a.o_tsteps = a.o_steps + S;
    a.o_count = a.o_tsteps + (long long)S * N;
    a.o_key = a.o_count + (long long)S * L * N;
    a.total = a.o_key + (long long)S * L * N;
    a.cross = cross, a.nt = nt, a.speed = speed, a.speed_sum = speed_sum, a.profile = profile, a.steps = steps;
    a.trk_steps = trk_steps, a.trk_count = trk_count, a.trk_first = trk_first, a.trk_dir = trk_dir;
    hipStream_t st = as_stream(stream);
    hipError_t err = hipMemsetAsync(workspace, 0, (size_t)need, st);
    if (err != hipSuccess) return err;
    const long long items_n = (long long)S * a.NC * a.NB;
    if (items_n > 0) {                             // T' == 1: no step, the copy alone writes the empty rows
        hipLaunchKernelGGL(line_stats_kernel, dim3((unsigned)(items_n < LS_MAX_GRID ? items_n : LS_MAX_GRID)),
                           dim3(LS_THREADS), 0, st, a);
        err = hipGetLastError();
        if (err != hipSuccess) return err;
    }
    const long long blocks = (a.total + 255) / 256;
    hipLaunchKernelGGL(line_stats_copy_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, a);
    return hipGetLastError();
}
