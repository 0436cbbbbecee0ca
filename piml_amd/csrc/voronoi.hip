// Voronoi local density (Steffen and Seyfried 2010) for the crowd statistics: every focal agent's cell is the part of the
// plane closer to it than to any other present agent of its slice, cut off at a regular polygon of radius `cutoff` around
// the agent and, optionally, at a walkable rectangle; its density is 1 / area of the cell.
//
// Cell pass (voronoi_cell_kernel): one workgroup of 256 lanes per (member, frame) slice, grid-stride over the slices; the
// slice's present agents are staged in LDS in slot order (cd_stage, as the Gaussian pass does).  One WAVE per focal agent,
// one polygon vertex per lane (capacity VD_CAP = 64), coordinates relative to the agent.  The wave tests 64 staged agents
// at a time (one per lane: |d|^2 < 4 cutoff^2 and != 0), and clips by the survivors in slot order.  A clip is a signed
// distance per lane and one Sutherland-Hodgman round over the edges (lane l owns edge l -> l + 1): a lane emits its vertex
// when it is inside and the edge's intersection when the sign changes along the edge, at the position a ballot and a
// lane-prefix count give it; the new vertices pass through a per-wave LDS row.  An intersection is interpolated from the
// edge's INSIDE end, t = s_in / (s_in - s_out) in [0, 1] (no cancellation: the signs differ); on a side of the rectangle
// its coordinate along the normal is the side's own.  Geometry is float32 (no contraction); the shoelace terms are float64
// products of the float32 vertices, summed over the wave in a fixed butterfly, the area is rounded to float32 and
// rho = 1 / area is a float32 true division.  A cell whose polygon would pass VD_CAP vertices or whose area is not > 0
// gets NaN and adds 1 to dropped[s] (64-bit integer atomic).  With at most CD_TILE slots below the member's bound the slice
// is staged once and the four waves run through the agents (slot w, w + 4, ...) without a barrier; with more, the four
// agents of a round keep their polygons in registers while the tiles are staged one after the other.
// The densities go to the workspace, and crowdstats.hip's statistics pass (crowd_given_density_kernel) and reduce pass
// take it from there: speed, bin, map, series and diagram are the very code of the Gaussian entry.  A cell depends on
// nothing but the slice's present positions in slot order: two calls give the same bits, and member m of an S-member call
// the bits of an S = 1 call on member m.
#include "crowdstats.hpp"
#include "../../include/piml_hip.h"

#include <cmath>

namespace piml {

constexpr int VD_CAP = 64;                    // vertices per polygon: one per lane
constexpr int VD_MAX_SIDES = 32;

struct VoronoiArgs {
    const float *P, *M;                       // (S, T, N, 2), (S, T, N)
    const int* n_active;                      // (S) or NULL
    int S, T, N, t0, Tp;
    int has_box, has_bounds, sides;
    float x0, x1, y0, y1;                     // the focal box
    float bx0, bx1, by0, by1;                 // the walkable rectangle
    float cutoff, four_c2;
    float dirs[2 * VD_MAX_SIDES];
    float* rho;                               // (S T', N)
    long long* dropped;                       // (S)
};

// One polygon per wave: lane l < n holds vertex l (relative to the agent), counter-clockwise as the directions are.
struct VdPoly {
    float x, y;
    int n;                                    // wave-uniform; -1 once the polygon passed VD_CAP
};

// Keeps the part of the polygon where s <= 0 (s: this lane's signed distance).  axis 0 / 1: the line is x = snap / y = snap
// and an intersection takes that coordinate as it is; axis < 0: a general line.  row: the wave's VD_CAP LDS slots.
__device__ __forceinline__ void vd_clip(VdPoly& g, float s, int axis, float snap, float2* row, int lane) {
    const bool live = lane < g.n;
    const bool in = live && s <= 0.f;
    const u64 in_mask = __ballot(in);
    if (in_mask == __ballot(live)) return;                        // the line misses the polygon
    const int nx = lane + 1 == g.n ? 0 : lane + 1;
    const float xn = __shfl(g.x, nx, 64), yn = __shfl(g.y, nx, 64), sn = __shfl(s, nx, 64);
    const bool in_next = (in_mask >> nx) & 1;
    const bool cross = live && in != in_next;
    const u64 cross_mask = __ballot(cross);
    const int total = __popcll(in_mask) + __popcll(cross_mask);
    if (total > VD_CAP) {
        g.n = -1;
        return;
    }
    const int at = (int)mbcnt(in_mask) + (int)mbcnt(cross_mask);
    if (in) row[at] = make_float2(g.x, g.y);
    if (cross) {
        const float xa = in ? g.x : xn, ya = in ? g.y : yn, sa = in ? s : sn;       // the inside end
        const float xb = in ? xn : g.x, yb = in ? yn : g.y, sb = in ? sn : s;
        const float t = sa / (sa - sb);
        float ix = xa + t * (xb - xa), iy = ya + t * (yb - ya);
        if (axis == 0) ix = snap;
        if (axis == 1) iy = snap;
        row[at + (in ? 1 : 0)] = make_float2(ix, iy);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    g.n = total;
    if (lane < total) {
        const float2 v = row[lane];
        g.x = v.x, g.y = v.y;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();                              // the row is rewritten by the next clip
}

// The cut-off polygon around pi, clipped by the rectangle.
__device__ __forceinline__ VdPoly vd_begin(const VoronoiArgs& a, const float* dirs, float2 pi, float2* row, int lane) {
    VdPoly g;
    g.n = a.sides;
    g.x = g.y = 0.f;
    if (lane < a.sides) {
        g.x = a.cutoff * dirs[2 * lane];
        g.y = a.cutoff * dirs[2 * lane + 1];
    }
    if (a.has_bounds) {
        const float hx0 = a.bx0 - pi.x, hx1 = a.bx1 - pi.x, hy0 = a.by0 - pi.y, hy1 = a.by1 - pi.y;
        vd_clip(g, hx0 - g.x, 0, hx0, row, lane);
        if (g.n > 0) vd_clip(g, g.x - hx1, 0, hx1, row, lane);
        if (g.n > 0) vd_clip(g, hy0 - g.y, 1, hy0, row, lane);
        if (g.n > 0) vd_clip(g, g.y - hy1, 1, hy1, row, lane);
    }
    return g;
}

// Clips by the bisectors of the cnt staged agents, in their order.
__device__ __forceinline__ void vd_clip_tile(VdPoly& g, const float2* src, int cnt, float2 pi, float four_c2, float2* row,
                                             int lane) {
    for (int k0 = 0; k0 < cnt && g.n > 0; k0 += 64) {
        float dx = 0.f, dy = 0.f, d2 = 0.f;
        if (k0 + lane < cnt) {
            const float2 q = src[k0 + lane];
            dx = q.x - pi.x, dy = q.y - pi.y;
            d2 = dx * dx + dy * dy;
        }
        u64 cuts = __ballot(d2 != 0.f && d2 < four_c2);           // (a lane past cnt has d2 == 0)
        while (cuts && g.n > 0) {
            const int k = (int)__builtin_ctzll(cuts);
            cuts &= cuts - 1;
            const float ex = __shfl(dx, k, 64), ey = __shfl(dy, k, 64), h = 0.5f * __shfl(d2, k, 64);
            vd_clip(g, (g.x * ex + g.y * ey) - h, -1, 0.f, row, lane);
        }
    }
}

// 1 / area (NaN for a polygon that passed VD_CAP or has no area), written by lane 0; counts the NaN in dropped[s].
__device__ __forceinline__ void vd_finish(const VoronoiArgs& a, const VdPoly& g, int s, long long at, int lane) {
    const int nx = lane + 1 < g.n ? lane + 1 : 0;
    const float xn = __shfl(g.x, nx, 64), yn = __shfl(g.y, nx, 64);
    const double term = lane < g.n ? (double)g.x * (double)yn - (double)xn * (double)g.y : 0.0;
    const float area = (float)(0.5 * wave_sum(term));
    const bool ok = g.n > 0 && area > 0.f;
    if (lane == 0) {
        a.rho[at] = ok ? 1.f / area : NAN;
        if (!ok) atomicAdd(reinterpret_cast<unsigned long long*>(a.dropped) + s, 1ull);
    }
}

__device__ __forceinline__ bool vd_focal(const VoronoiArgs& a, float m, float2 p) {
    return cd_present(m, p) && in_box(a.has_box, a.x0, a.x1, a.y0, a.y1, p) &&
           (!a.has_bounds || (a.bx0 <= p.x && p.x < a.bx1 && a.by0 <= p.y && p.y < a.by1));
}

__global__ void __launch_bounds__(CD_THREADS) voronoi_cell_kernel(VoronoiArgs a) {
    __shared__ float2 src[CD_TILE];
    __shared__ int wave_cnt[CD_WAVES];
    __shared__ float2 rows[CD_WAVES][VD_CAP];
    __shared__ float dirs[2 * VD_MAX_SIDES];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid < 2 * VD_MAX_SIDES) dirs[tid] = a.dirs[tid];          // (a load from the argument segment, no private copy)
    __syncthreads();
    float2* row = rows[w];
    const long long slices = (long long)a.S * a.Tp;
    for (long long sl = blockIdx.x; sl < slices; sl += gridDim.x) {
        const int s = (int)(sl / a.Tp), tp = (int)(sl - (long long)s * a.Tp);
        const long long frame = (long long)s * a.T + a.t0 + tp;
        const float2* P = reinterpret_cast<const float2*>(a.P) + frame * a.N;
        const float* M = a.M + frame * a.N;
        int bound = a.N;
        if (a.n_active) bound = min(max(a.n_active[s], 0), a.N);
        if (bound <= CD_TILE) {
            const int cnt = cd_stage(P, M, 0, bound, src, wave_cnt);
            for (int i = w; i < bound; i += CD_WAVES) {
                const float2 pi = P[i];
                if (!vd_focal(a, M[i], pi)) {
                    if (lane == 0) a.rho[sl * a.N + i] = NAN;
                    continue;
                }
                VdPoly g = vd_begin(a, dirs, pi, row, lane);
                vd_clip_tile(g, src, cnt, pi, a.four_c2, row, lane);
                vd_finish(a, g, s, sl * a.N + i, lane);
            }
            __syncthreads();                  // every wave is done with src before the next slice is staged
        } else {
            for (int i0 = 0; i0 < bound; i0 += CD_WAVES) {
                const int i = i0 + w;
                float2 pi = make_float2(0.f, 0.f);
                bool focal = false;
                if (i < bound) {
                    pi = P[i];
                    focal = vd_focal(a, M[i], pi);
                }
                VdPoly g;
                g.x = g.y = 0.f, g.n = 0;
                if (focal) g = vd_begin(a, dirs, pi, row, lane);
                for (int lo = 0; lo < bound; lo += CD_TILE) {
                    const int cnt = cd_stage(P, M, lo, min(lo + CD_TILE, bound), src, wave_cnt);
                    if (focal) vd_clip_tile(g, src, cnt, pi, a.four_c2, row, lane);
                    __syncthreads();          // every wave is done with this tile before the next one is staged
                }
                if (focal)
                    vd_finish(a, g, s, sl * a.N + i, lane);
                else if (i < bound && lane == 0)
                    a.rho[sl * a.N + i] = NAN;
            }
        }
    }
}

}  // namespace piml

using namespace piml;

PIML_API long long piml_crowd_stats_voronoi_workspace_bytes(int S, int frames, int N, int rho_bins) {
    if (S < 0 || frames < 0 || N < 0 || rho_bins < 0) return -1;
    const long long slices = (long long)S * frames;
    return cd_workspace_bytes(slices, rho_bins) + slices * N * (long long)sizeof(float);
}

PIML_API int piml_crowd_stats_voronoi(const float* P, const float* V, const float* M, const int* n_active, int S, int T, int N,
                                      int t0, int t1, float cutoff, const float* dirs, int sides, int has_bounds, float bx0,
                                      float bx1, float by0, float by1, int has_box, float x0, float x1, float y0, float y1,
                                      float cell, int gx, int gy, float rho_bin, int rho_bins, long long* n,
                                      long long* n_speed, double* sum_speed, double* sum_density, long long* fd_count,
                                      double* fd_sum, double* fd_sum2, long long* map, float* density, long long* dropped,
                                      void* workspace, long long workspace_bytes, void* stream) {
    if (!(cutoff > 0.f) || !std::isfinite(cutoff) || sides < 3 || sides > VD_MAX_SIDES || !dirs || !dropped)
        return hipErrorInvalidValue;
    if (has_bounds && (!std::isfinite(bx0) || !std::isfinite(bx1) || !std::isfinite(by0) || !std::isfinite(by1) ||
                       !(bx0 < bx1) || !(by0 < by1)))
        return hipErrorInvalidValue;
    CrowdArgs c;
    void* extra = nullptr;
    const long long rho_bytes = S > 0 && N > 0 && t1 > t0 ? (long long)S * (t1 - t0) * N * (long long)sizeof(float) : 0;
    hipError_t e = cd_prepare(c, P, V, M, n_active, S, T, N, t0, t1, has_box, x0, x1, y0, y1, cell, gx, gy, rho_bin, rho_bins,
                              n, n_speed, sum_speed, sum_density, fd_count, fd_sum, fd_sum2, map, density, workspace,
                              workspace_bytes, rho_bytes, &extra);
    if (e != hipSuccess) return e;
    VoronoiArgs a{};
    a.P = P, a.M = M, a.n_active = n_active;
    a.S = S, a.T = T, a.N = N, a.t0 = t0, a.Tp = c.Tp;
    a.has_box = c.has_box, a.has_bounds = has_bounds ? 1 : 0, a.sides = sides;
    a.x0 = x0, a.x1 = x1, a.y0 = y0, a.y1 = y1;
    a.bx0 = bx0, a.bx1 = bx1, a.by0 = by0, a.by1 = by1;
    a.cutoff = cutoff, a.four_c2 = 4.f * (cutoff * cutoff);
    for (int k = 0; k < 2 * sides; ++k) a.dirs[k] = dirs[k];
    a.rho = static_cast<float*>(extra);
    a.dropped = dropped;
    c.rho_in = a.rho;
    hipStream_t st = as_stream(stream);
    e = hipMemsetAsync(dropped, 0, (size_t)S * sizeof(long long), st);
    if (e != hipSuccess) return e;
    const long long slices = (long long)S * c.Tp;
    hipLaunchKernelGGL(voronoi_cell_kernel, dim3((unsigned)(slices < CD_MAX_GRID ? slices : CD_MAX_GRID)), dim3(CD_THREADS), 0,
                       st, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return cd_run(c, true, st);
}
