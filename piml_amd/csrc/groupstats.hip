// Group statistics of crowds: who walks with whom.  Two passes over S members in one call each.  Slot n of
// member s is one agent for the whole run; velocities are not an input.
//
// Agent i takes part at (s, t) when M == 1, both coordinates of P are finite and below 65536 in magnitude and
// i < n_active[s].  Window frames t = 0 .. T' - 1.  A step (i, t) exists when i takes part at t and t + 1 and t + 1 < T';
// u_i(t) = p_i(t+1) - p_i(t).  float32 with separately rounded products, true square roots and divisions and no
// contraction, Q = 2^20.  A pair-frame (i, j, t), i < j, exists when both steps exist at t; with e = p_j(t) - p_i(t) and
// g = u_j(t) - u_i(t) it is "together" when ex ex + ey ey < r2, gx gx + gy gy < dv2, |u_i|^2 >= vm2 and |u_j|^2 >= vm2
// (r2, dv2, vm2 made once on the host).
//
// group_pairs_kernel (pass 1): one workgroup per (member, focal track i), tracks taken grid-stride.  A scan of the focal's
// column gives its first and last participating frame; nothing outside is looked at.  The focal's positions and steps
// are staged in LDS in tiles of GS_TILE frames, 16 B per frame (position, displacement; displacement x NaN: no step),
// and read back as broadcasts.  Lane k owns partner j = i + 1 + chunk GS_THREADS + k, so the lanes of a wave read
// consecutive slots of one frame; a lane carries p_j(t+1) into the next iteration, so every position is read once per
// focal, and keeps co (pair-frames) and near (together pair-frames) in registers over all tiles.  The lanes whose pair is
// a candidate (near >= min_frames) append a row (i, j, co, near) with one integer atomic per wave (ballot, prefix count);
// rows past max_edges are counted and not written.  Per track the steps and sum llrintf(sqrtf(|u|^2) Q) are written by
// the track's own workgroup; pairs and together take one 64-bit integer atomic per wave.
//
// group_members_kernel (pass 2): one workgroup per link (s, i, j), links taken grid-stride, lanes over frames.  Every
// together pair-frame (the predicate of pass 1) goes into LDS histograms of the member distance and of the formation
// cosine, flushed per link with 64-bit integer atomics where non-zero.  A link with an index out of range is skipped.
//
// Every output is an integer and every atomic an integer add, so the results are bitwise reproducible whatever the order
// of the adds; only the order of the edge rows depends on it, and the operator sorts them.
#include "common.hpp"
#include "../../include/piml_hip.h"

#include <cmath>

namespace piml {

constexpr int GS_THREADS = 256;
constexpr int GS_WAVES = GS_THREADS / 64;
constexpr int GS_TILE = PIML_GROUP_TILE;           // focal frames per staged tile
constexpr int GS_MAX_BINS = 256;
constexpr int GS_MAX_N = 65536;
constexpr float GS_Q = 1048576.f;                  // 2^20
constexpr float GS_MAX_COORD = 65536.f;
constexpr int GS_MAX_FRAMES = 1 << 25;
constexpr long long GS_MAX_GRID = 1 << 20;

struct GroupPairArgs {
    const float *P, *M;                            // (S, T, N, 2), (S, T, N)
    const int* n_active;                           // (S) or NULL
    int S, T, N, t0, Tp, min_frames, max_edges;
    float r2, dv2, vm2;
    int *edges, *n_edges;                          // (S, max_edges, 4), (S)
    long long *trk_steps, *trk_path;               // (S, N)
    unsigned long long *pairs, *together;          // (S)
};

struct GroupMemberArgs {
    const float *P, *M;
    const int* links;                              // (K, 3): member, i, j
    int S, T, N, t0, Tp, K, RB, AB;
    float r2, dv2, vm2, r_bin;
    unsigned long long *dist, *dist_sum, *abreast, *skipped, *frames;
};

__device__ __forceinline__ bool gs_participant(float m, float2 p) {
    return m == 1.f && fabsf(p.x) < GS_MAX_COORD && fabsf(p.y) < GS_MAX_COORD;
}


// the pair-frame predicate, shared by both passes: e = p_j - p_i, u_i, u_j
__device__ __forceinline__ bool gs_together(float ex, float ey, float uix, float uiy, float ujx, float ujy, float r2,
                                            float dv2, float vm2) {
    const float gx = ujx - uix, gy = ujy - uiy;
    return ex * ex + ey * ey < r2 && gx * gx + gy * gy < dv2 && uix * uix + uiy * uiy >= vm2 && ujx * ujx + ujy * ujy >= vm2;
}

__global__ void __launch_bounds__(GS_THREADS) group_pairs_kernel(GroupPairArgs a) {
    __shared__ float4 foc[GS_TILE];                // p_i(t), u_i(t); u x NaN: no step
    __shared__ long long red[2][GS_WAVES];
    __shared__ int span[2][GS_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int Tp = a.Tp;
    const long long N = a.N;
    const long long tracks = (long long)a.S * a.N;
    for (long long tr = blockIdx.x; tr < tracks; tr += gridDim.x) {
        const int s = (int)(tr / a.N), i = (int)(tr - (long long)s * a.N);
        int bound = a.N;
        if (a.n_active) bound = min(max(a.n_active[s], 0), a.N);
        const long long frame0 = (long long)s * a.T + a.t0;
        const float2* P = reinterpret_cast<const float2*>(a.P) + frame0 * N;     // frame t of the window, slot n: P[t * N + n]
        const float* M = a.M + frame0 * N;
        // the focal's span
        int first = Tp, last = -1;
        if (i < bound) {
            for (int t = tid; t < Tp; t += GS_THREADS) {
                if (gs_participant(M[t * N + i], P[t * N + i])) {
                    first = min(first, t);
                    last = t;
                }
            }
        }
        first = wave_min(first), last = wave_max(last);
        if (lane == 0) span[0][w] = first, span[1][w] = last;
        __syncthreads();
        first = span[0][0], last = span[1][0];
#pragma unroll
        for (int q = 1; q < GS_WAVES; ++q) first = min(first, span[0][q]), last = max(last, span[1][q]);
        __syncthreads();                           // span is rewritten by the next track
        if (last <= first) {                       // no step
            if (tid == 0) a.trk_steps[tr] = 0, a.trk_path[tr] = 0;
            continue;
        }
        long long steps = 0, path = 0, pairs = 0, tog = 0;
        const int partners = bound - 1 - i;
        const int chunks = max((partners + GS_THREADS - 1) / GS_THREADS, 1);      // one pass at least: the focal's own row
        for (int c = 0; c < chunks; ++c) {
            const int j = i + 1 + c * GS_THREADS + tid;
            const bool owns = j < bound;
            int co = 0, near = 0;
            float2 q0 = make_float2(0.f, 0.f);
            bool part0 = false;
            if (owns) {
                q0 = P[first * N + j];
                part0 = gs_participant(M[first * N + j], q0);
            }
            for (int c0 = first; c0 < last; c0 += GS_TILE) {
                const int core = min(GS_TILE, last - c0);                         // steps t = c0 .. c0 + core - 1
                __syncthreads();                   // every lane is done with the tile staged before
                for (int k = tid; k < core; k += GS_THREADS) {
                    const long long t = c0 + k;
                    const float2 p0 = P[t * N + i], p1 = P[(t + 1) * N + i];
                    const bool ok = gs_participant(M[t * N + i], p0) && gs_participant(M[(t + 1) * N + i], p1);
                    const float ux = p1.x - p0.x, uy = p1.y - p0.y;
                    foc[k] = ok ? make_float4(p0.x, p0.y, ux, uy) : make_float4(0.f, 0.f, NAN, 0.f);
                    if (ok && c == 0) {
                        ++steps;
                        path += llrintf(sqrtf(ux * ux + uy * uy) * GS_Q);
                    }
                }
                __syncthreads();
                if (owns) {
                    const float2* Pj = P + (long long)(c0 + 1) * N + j;           // p_j(t + 1), t = c0 + k: Pj[k * N]
                    const float* Mj = M + (long long)(c0 + 1) * N + j;
                    for (int k = 0; k < core; ++k) {
                        const float2 q1 = Pj[k * N];
                        const bool part1 = gs_participant(Mj[k * N], q1);
                        const float4 f = foc[k];
                        if (part0 && part1 && !isnan(f.z)) {
                            ++co;
                            if (gs_together(q0.x - f.x, q0.y - f.y, f.z, f.w, q1.x - q0.x, q1.y - q0.y, a.r2, a.dv2, a.vm2))
                                ++near;
                        }
                        q0 = q1, part0 = part1;
                    }
                }
            }
            pairs += co, tog += near;
            // the candidates of this chunk: one atomic per wave
            const bool cand = owns && near >= a.min_frames;
            const unsigned long long mask = __ballot(cand);
            if (mask) {
                int base = 0;
                if (lane == 0) base = atomicAdd(a.n_edges + s, (int)__popcll(mask));
                base = __shfl(base, 0, 64);
                const long long pos = (long long)base + __popcll(mask & ((1ull << lane) - 1ull));
                if (cand && pos < a.max_edges)
                    reinterpret_cast<int4*>(a.edges)[(long long)s * a.max_edges + pos] = make_int4(i, j, co, near);
            }
        }
        steps = wave_sum(steps), path = wave_sum(path), pairs = wave_sum(pairs), tog = wave_sum(tog);
        if (lane == 0) {
            red[0][w] = steps, red[1][w] = path;
            if (pairs) atomicAdd(a.pairs + s, (unsigned long long)pairs);
            if (tog) atomicAdd(a.together + s, (unsigned long long)tog);
        }
        __syncthreads();
        if (tid == 0) {
            steps = path = 0;
            for (int q = 0; q < GS_WAVES; ++q) steps += red[0][q], path += red[1][q];
            a.trk_steps[tr] = steps, a.trk_path[tr] = path;
        }
        __syncthreads();                           // red free for the next track
    }
}

__global__ void __launch_bounds__(GS_THREADS) group_members_kernel(GroupMemberArgs a) {
    __shared__ unsigned h_dist[GS_MAX_BINS + 1], h_abr[GS_MAX_BINS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int RB = a.RB, AB = a.AB;
    const long long N = a.N;
    for (int k = tid; k <= GS_MAX_BINS; k += GS_THREADS) {
        h_dist[k] = 0u;
        if (k < GS_MAX_BINS) h_abr[k] = 0u;
    }
    __syncthreads();
    for (long long l = blockIdx.x; l < a.K; l += gridDim.x) {
        const int s = a.links[3 * l], i = a.links[3 * l + 1], j = a.links[3 * l + 2];
        if (s < 0 || s >= a.S || i < 0 || j <= i || j >= a.N) continue;           // the same for the whole workgroup
        const long long frame0 = (long long)s * a.T + a.t0;
        const float2* P = reinterpret_cast<const float2*>(a.P) + frame0 * N;
        const float* M = a.M + frame0 * N;
        long long dsum = 0, skipped = 0, n = 0;
        for (long long t = tid; t < a.Tp - 1; t += GS_THREADS) {
            const float2 pi0 = P[t * N + i], pi1 = P[(t + 1) * N + i], pj0 = P[t * N + j], pj1 = P[(t + 1) * N + j];
            if (!(gs_participant(M[t * N + i], pi0) && gs_participant(M[(t + 1) * N + i], pi1) &&
                  gs_participant(M[t * N + j], pj0) && gs_participant(M[(t + 1) * N + j], pj1)))
                continue;
            const float ex = pj0.x - pi0.x, ey = pj0.y - pi0.y;
            const float uix = pi1.x - pi0.x, uiy = pi1.y - pi0.y, ujx = pj1.x - pj0.x, ujy = pj1.y - pj0.y;
            if (!gs_together(ex, ey, uix, uiy, ujx, ujy, a.r2, a.dv2, a.vm2)) continue;
            ++n;
            const float d2 = ex * ex + ey * ey;
            const float d = sqrtf(d2);
            const float qb = floorf(d / a.r_bin);
            atomicAdd(h_dist + (qb < (float)RB ? (int)qb : RB), 1u);
            dsum += llrintf(d * GS_Q);
            const float wx = uix + ujx, wy = uiy + ujy;
            const float w2 = wx * wx + wy * wy;
            if (d2 == 0.f || w2 == 0.f) {
                ++skipped;
            } else {
                const float c = fabsf(ex * wx + ey * wy) / (sqrtf(d2) * sqrtf(w2));
                const float qa = floorf(c * (float)AB);
                atomicAdd(h_abr + (qa < (float)(AB - 1) ? (int)qa : AB - 1), 1u);
            }
        }
        dsum = wave_sum(dsum), skipped = wave_sum(skipped), n = wave_sum(n);
        if (lane == 0) {
            if (dsum) atomicAdd(a.dist_sum + s, (unsigned long long)dsum);
            if (skipped) atomicAdd(a.skipped + s, (unsigned long long)skipped);
            if (n) atomicAdd(a.frames + s, (unsigned long long)n);
        }
        __syncthreads();                           // the histograms are complete
        for (int b = tid; b <= RB; b += GS_THREADS) {
            const unsigned c = h_dist[b];
            if (!c) continue;
            atomicAdd(a.dist + (long long)s * (RB + 1) + b, (unsigned long long)c);
            h_dist[b] = 0u;
        }
        for (int b = tid; b < AB; b += GS_THREADS) {
            const unsigned c = h_abr[b];
            if (!c) continue;
            atomicAdd(a.abreast + (long long)s * AB + b, (unsigned long long)c);
            h_abr[b] = 0u;
        }
        __syncthreads();                           // and free for the next link
    }
}

// group_components_kernel: the link rule, the connected components and the sizes between the passes, one
// workgroup per member.  label (the group_id row) starts at label[x] = x; a round is an edge sweep -- every link lowers the
// larger of its two ends' labels to the smaller with an integer atomic minimum -- and a pointer-jumping sweep
// label[x] = min(label[x], label[label[x]]).  Labels only decrease, label[x] <= x, and a label never leaves its component,
// so when a round changes nothing every track of a component carries the component's smallest slot, whatever the order of
// the rows and of the lanes.  After k edge sweeps the tracks within k links of that slot carry it, so N rounds always
// suffice; `status` is 1 if they did not (a logic error, never a spin).  Every access to a label another lane may be
// lowering is an atomic of agent scope, and a fence and a barrier stand between the sweeps.  The sizes: count[root] over the
// eligible tracks in the int32 workspace row, then the three tables by 64-bit integer atomics in LDS, stored once.
struct GroupCompArgs {
    const int* edges;                              // (S, cap, 4)
    const int* n_edges;                            // (S)
    const long long *trk_steps, *trk_path;         // (S, N)
    int S, N, cap, min_frames, share_q, G;
    long long *candidates, *links;                 // (S)
    int* group_id;                                 // (S, N): the labels
    long long *size_tracks, *size_path, *size_steps;                              // (S, G + 1)
    int *work, *status;                            // (S, N), (S)
};

constexpr int GS_MAX_G = 64;

__device__ __forceinline__ int gs_label(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ void gs_sweep_end() {   // what this sweep lowered is seen by every lane of the next
    __threadfence();
    __syncthreads();
}

__global__ void __launch_bounds__(GS_THREADS) group_components_kernel(GroupCompArgs a) {
    __shared__ unsigned long long table[3][GS_MAX_G + 1];
    __shared__ int n_links, changed;
    const int tid = threadIdx.x, s = blockIdx.x, N = a.N, G = a.G;
    const int4* rows = reinterpret_cast<const int4*>(a.edges) + (long long)s * a.cap;
    const int listed = a.n_edges[s];
    const int ne = min(max(listed, 0), a.cap);
    int* label = a.group_id + (long long)s * N;
    int* count = a.work + (long long)s * N;
    const long long* steps = a.trk_steps + (long long)s * N;
    const long long* path = a.trk_path + (long long)s * N;
    const auto is_link = [&](int4 r) {             // (i, j, co, near): the share rule in 64-bit integers, both ends in range
        return (long long)r.w * 1024 >= (long long)a.share_q * r.z && r.x >= 0 && r.x < N && r.y >= 0 && r.y < N;
    };
    if (tid == 0) n_links = 0, changed = 0;
    for (int k = tid; k < 3 * (GS_MAX_G + 1); k += GS_THREADS) (&table[0][0])[k] = 0ull;
    for (int x = tid; x < N; x += GS_THREADS) {
        __hip_atomic_store(label + x, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(count + x, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    int mine = 0;
    for (int e = tid; e < ne; e += GS_THREADS) mine += is_link(rows[e]) ? 1 : 0;
    if (mine) atomicAdd(&n_links, mine);
    gs_sweep_end();
    const int links = n_links;
    bool settled = links == 0;
    for (int round = 0; round < N && !settled; ++round) {
        int ch = 0;
        for (int e = tid; e < ne; e += GS_THREADS) {
            const int4 r = rows[e];
            if (!is_link(r)) continue;
            const int li = gs_label(label + r.x), lj = gs_label(label + r.y);
            if (li < lj) atomicMin(label + r.y, li), ch = 1;
            else if (lj < li) atomicMin(label + r.x, lj), ch = 1;
        }
        gs_sweep_end();
        for (int x = tid; x < N; x += GS_THREADS) {
            const int l = gs_label(label + x);     // 0 <= label[x] <= x < N always
            const int ll = gs_label(label + l);
            if (ll < l) atomicMin(label + x, ll), ch = 1;
        }
        if (ch) atomicOr(&changed, 1);
        gs_sweep_end();
        settled = changed == 0;
        __syncthreads();                           // every lane has read the word
        if (tid == 0) changed = 0;
        __syncthreads();
    }
    // the sizes of the components over the eligible tracks
    for (int x = tid; x < N; x += GS_THREADS)
        if (steps[x] >= a.min_frames) atomicAdd(count + gs_label(label + x), 1);
    gs_sweep_end();
    for (int x = tid; x < N; x += GS_THREADS) {
        const long long st = steps[x];
        if (st >= a.min_frames) {
            const int k = min(gs_label(count + gs_label(label + x)), G);
            atomicAdd(&table[0][k], 1ull);
            atomicAdd(&table[1][k], (unsigned long long)path[x]);
            atomicAdd(&table[2][k], (unsigned long long)st);
        } else {
            label[x] = -1;                         // nobody else reads label[x] any more: the others read their own and a count
        }
    }
    __syncthreads();
    for (int k = tid; k <= G; k += GS_THREADS) {
        a.size_tracks[(long long)s * (G + 1) + k] = (long long)table[0][k];
        a.size_path[(long long)s * (G + 1) + k] = (long long)table[1][k];
        a.size_steps[(long long)s * (G + 1) + k] = (long long)table[2][k];
    }
    if (tid == 0) {
        a.candidates[s] = listed;
        a.links[s] = links;
        a.status[s] = settled ? 0 : 1;
    }
}

// the arguments both entries share; no 64-bit sum overflows: dist_sum adds at most N (N - 1) / 2 T' terms below sqrt(r2) Q
// (trk_path: T' <= 2^25 steps below 2^37.5 each)
static bool gs_bad_common(int S, int T, int N, int t0, int t1, float r2, float dv2, float vm2) {
    const auto positive = [](float x) { return x > 0.f && std::isfinite(x); };
    if (S < 0 || T < 0 || N < 0 || N > GS_MAX_N || t0 < 0 || t1 > T || t1 < t0 || t1 - t0 > GS_MAX_FRAMES || !positive(r2) ||
        !positive(dv2) || !(vm2 >= 0.f) || !std::isfinite(vm2))
        return true;
    const double items = 0.5 * (double)N * (double)N * (double)(t1 - t0), two63 = 9223372036854775808.0;
    return !(std::sqrt((double)r2) * (double)GS_Q * items < two63);
}

}  // namespace piml

using namespace piml;

PIML_API int piml_group_pairs(const float* P, const float* M, const int* n_active, int S, int T, int N, int t0, int t1, float r2,
                              float dv2, float vm2, int min_frames, int max_edges, int* edges, int* n_edges,
                              long long* trk_steps, long long* trk_path, long long* pairs, long long* together, void* stream) {
    if (gs_bad_common(S, T, N, t0, t1, r2, dv2, vm2) || min_frames < 1 || max_edges < 0) return hipErrorInvalidValue;
    if (S == 0 || t1 == t0 || N == 0) return hipSuccess;
    if (!P || !M || (max_edges > 0 && !edges) || !n_edges || !trk_steps || !trk_path || !pairs || !together)
        return hipErrorInvalidValue;
    GroupPairArgs a{};
    a.P = P, a.M = M, a.n_active = n_active;
    a.S = S, a.T = T, a.N = N, a.t0 = t0, a.Tp = t1 - t0, a.min_frames = min_frames, a.max_edges = max_edges;
    a.r2 = r2, a.dv2 = dv2, a.vm2 = vm2;
    a.edges = edges, a.n_edges = n_edges, a.trk_steps = trk_steps, a.trk_path = trk_path;
    a.pairs = reinterpret_cast<unsigned long long*>(pairs), a.together = reinterpret_cast<unsigned long long*>(together);
    hipStream_t st = as_stream(stream);
    hipError_t err = hipMemsetAsync(n_edges, 0, (size_t)S * sizeof(int), st);
    if (err == hipSuccess) err = hipMemsetAsync(pairs, 0, (size_t)S * sizeof(long long), st);
    if (err == hipSuccess) err = hipMemsetAsync(together, 0, (size_t)S * sizeof(long long), st);
    if (err != hipSuccess) return err;
    const long long tracks = (long long)S * N;
    hipLaunchKernelGGL(group_pairs_kernel, dim3((unsigned)(tracks < GS_MAX_GRID ? tracks : GS_MAX_GRID)), dim3(GS_THREADS), 0, st,
                       a);
    return hipGetLastError();
}

PIML_API int piml_group_members(const float* P, const float* M, int S, int T, int N, int t0, int t1, const int* links,
                                int n_links, float r2, float dv2, float vm2, float r_bin, int r_bins, int a_bins,
                                long long* dist, long long* dist_sum, long long* abreast, long long* abreast_skipped,
                                long long* link_frames, void* stream) {
    if (gs_bad_common(S, T, N, t0, t1, r2, dv2, vm2) || n_links < 0 || !(r_bin > 0.f) || !std::isfinite(r_bin) || r_bins < 1 ||
        r_bins > GS_MAX_BINS || a_bins < 1 || a_bins > GS_MAX_BINS)
        return hipErrorInvalidValue;
    if (S == 0 || t1 == t0 || N == 0) return hipSuccess;
    if (!P || !M || (n_links > 0 && !links) || !dist || !dist_sum || !abreast || !abreast_skipped || !link_frames)
        return hipErrorInvalidValue;
    GroupMemberArgs a{};
    a.P = P, a.M = M, a.links = links;
    a.S = S, a.T = T, a.N = N, a.t0 = t0, a.Tp = t1 - t0, a.K = n_links, a.RB = r_bins, a.AB = a_bins;
    a.r2 = r2, a.dv2 = dv2, a.vm2 = vm2, a.r_bin = r_bin;
    a.dist = reinterpret_cast<unsigned long long*>(dist), a.dist_sum = reinterpret_cast<unsigned long long*>(dist_sum);
    a.abreast = reinterpret_cast<unsigned long long*>(abreast), a.skipped = reinterpret_cast<unsigned long long*>(abreast_skipped);
    a.frames = reinterpret_cast<unsigned long long*>(link_frames);
    hipStream_t st = as_stream(stream);
    hipError_t err = hipMemsetAsync(dist, 0, (size_t)S * (r_bins + 1) * sizeof(long long), st);
    if (err == hipSuccess) err = hipMemsetAsync(dist_sum, 0, (size_t)S * sizeof(long long), st);
    if (err == hipSuccess) err = hipMemsetAsync(abreast, 0, (size_t)S * a_bins * sizeof(long long), st);
    if (err == hipSuccess) err = hipMemsetAsync(abreast_skipped, 0, (size_t)S * sizeof(long long), st);
    if (err == hipSuccess) err = hipMemsetAsync(link_frames, 0, (size_t)S * sizeof(long long), st);
    if (err != hipSuccess || n_links == 0 || t1 - t0 < 2) return err;
    hipLaunchKernelGGL(group_members_kernel, dim3((unsigned)(n_links < 65536 ? n_links : 65536)), dim3(GS_THREADS), 0, st, a);
    return hipGetLastError();
}

PIML_API int piml_group_components(const int* edges, const int* n_edges, const long long* trk_steps, const long long* trk_path,
                                   int S, int N, int cap, int min_frames, int share_q, int g_max, long long* candidates,
                                   long long* links, int* group_id, long long* size_tracks, long long* size_path,
                                   long long* size_steps, int* workspace, int* status, void* stream) {
    if (S < 0 || N < 0 || cap < 0 || N > GS_MAX_N || g_max < 1 || g_max > GS_MAX_G || min_frames < 1 || share_q < 1 ||
        share_q > 1024)
        return hipErrorInvalidValue;
    if (S == 0 || N == 0) return hipSuccess;
    if ((cap > 0 && !edges) || !n_edges || !trk_steps || !trk_path || !candidates || !links || !group_id || !size_tracks ||
        !size_path || !size_steps || !workspace || !status)
        return hipErrorInvalidValue;
    GroupCompArgs a{};
    a.edges = edges, a.n_edges = n_edges, a.trk_steps = trk_steps, a.trk_path = trk_path;
    a.S = S, a.N = N, a.cap = cap, a.min_frames = min_frames, a.share_q = share_q, a.G = g_max;
    a.candidates = candidates, a.links = links, a.group_id = group_id;
    a.size_tracks = size_tracks, a.size_path = size_path, a.size_steps = size_steps;
    a.work = workspace, a.status = status;
    hipLaunchKernelGGL(group_components_kernel, dim3((unsigned)S), dim3(GS_THREADS), 0, as_stream(stream), a);
    return hipGetLastError();
}
