// The wall term of the MLAPM scenario frame (piml_scenario_step_mlapm_walls) and of its stand-alone operator
// (piml_wall_force): the repulsion of the scene's nearest obstacle point, found through a static uniform cell grid.
//
//   q* = the valid obstacle point nearest p, d2 = fadd(fmul(e.x, e.x), fmul(e.y, e.y)), e = q - p, exact float32; ties go
//   to the point that comes first in the grid's sorted order.  Felt when d2 < c2 = fl(cutoff cutoff) (formed by the host):
//   W = A exp(B d) (p - q*) / d, d = sqrt(d2); W = 0 for d2 == 0 (F.normalize's convention, as the pair law's).
//   Not felt (no point within the cutoff, a NaN position, an empty grid): W = 0, index -1, d2 = +inf.
//
// The grid (piml_wall_grid, built once per scene by the host): cells of side `cell` >= cutoff (1 + 2^-5) from the points'
// minimum (x0, y0), a point's cell floor((q - origin) / cell) in float32, points sorted by cy gx + cx (stably), cell_start
// the CSR offsets.  The agent's cell comes from the same float32 formula, clamped to [-1, gx] x [-1, gy] while still a
// float; its 3 x 3 neighbourhood is three row-runs, each contiguous in the sorted list.  One wave serves an agent: the
// lanes stride over the runs, each keeps the minimum of the 64-bit key (bits(d2) << 32) | sorted index (d2 >= 0, so its
// bit pattern orders as its value), and one wave-wide minimum of the key yields the point and the tie rule together.
// Exactness: a point within the cutoff lies less than 1 / (1 + 2^-5) cells away per axis and the float32 quotients are off
// by less than 2^-7 cells for grids of at most 1024 cells per axis, so the nearest point within the cutoff is always in
// the 3 x 3 neighbourhood (tests/test_wallforce.py checks it adversarially).
// Every range read from cell_start is clamped to [0, n_points]: a corrupt table gives a wrong force, never a read outside
// `points`.  The value uses the hardware rsq / exp2 units as mlapm.hpp does (a smooth term, 1e-5 relative); the selection
// (index, d2, the cutoff predicate) is exact.
#pragma once
#include "common.hpp"
#include "mlapm.hpp"
#include "../../include/piml_hip.h"

#include <cmath>

namespace piml {

constexpr int kWallMaxCells = 1024;              // per axis: the bound of the exactness argument
constexpr float kWallCellMargin = 1.03125f;      // 1 + 2^-5
constexpr int kWallWaves = 4;                    // waves (rows) per block of the operator

struct WallArgs {
    piml_wall_grid G;
    float c2;                                    // fl(cutoff * cutoff), formed once by the host
};

struct WallHit {
    float2 force;
    float d2;
    int index;
};

__device__ __forceinline__ u64 wave_min_key(u64 k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)k, o, 64);
        const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(k >> 32), o, 64);
        const u64 ok = ((u64)hi << 32) | lo;
        k = ok < k ? ok : k;
    }
    return k;
}

// the cell coordinate of p along one axis, clamped to [-1, g] before the integer conversion (wave-uniform)
__device__ __forceinline__ int wall_cell(float p, float origin, float cell, int g) {
    const float c = floorf(__fdiv_rn(__fsub_rn(p, origin), cell));
    return uniform((int)fminf(fmaxf(c, -1.f), (float)g));
}

// One wave, one agent at p (the same in every lane).  Wave-uniform result.
__device__ __forceinline__ WallHit wall_force_wave(const WallArgs& W, float A, float B, float2 p, int lane) {
    WallHit h;
    h.force = make_float2(0.f, 0.f);
    h.d2 = INFINITY;
    h.index = -1;
    const piml_wall_grid& G = W.G;
    if (p.x != p.x || p.y != p.y || G.n_points <= 0) return h;
    const float2* pts = (const float2*)G.points;
    const int cx = wall_cell(p.x, G.x0, G.cell, G.gx), cy = wall_cell(p.y, G.y0, G.cell, G.gy);
    const int lo = max(cx - 1, 0), hi = min(cx + 1, G.gx - 1);
    u64 best = kEmptyKey;
    if (lo <= hi) {
        for (int r = max(cy - 1, 0); r <= min(cy + 1, G.gy - 1); ++r) {
            int b = G.cell_start[r * G.gx + lo], e = G.cell_start[r * G.gx + hi + 1];
            b = min(max(b, 0), G.n_points);
            e = min(max(e, 0), G.n_points);
            for (int j = b + lane; j < e; j += 64) {
                const float2 q = pts[j];
                const float ex = __fsub_rn(q.x, p.x), ey = __fsub_rn(q.y, p.y);
                const float d2 = __fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey));
                const u64 key = ((u64)__float_as_uint(d2) << 32) | (unsigned)j;
                best = key < best ? key : best;
            }
        }
    }
    best = wave_min_key(best);
    if (best == kEmptyKey) return h;
    const float d2 = __uint_as_float((unsigned)(best >> 32));
    if (!(d2 < W.c2)) return h;                  // the cutoff predicate, exact
    h.d2 = d2;
    h.index = (int)(unsigned)best;
    if (d2 > 0.f) {
        const float2 q = pts[h.index];
        const float rinv = fast_rsq(d2);
        const float d = d2 * rinv;
        const float g = A * fast_exp2((B * 1.4426950408889634f) * d) * rinv;
        h.force = make_float2(g * (p.x - q.x), g * (p.y - q.y));
    }
    return h;
}

// ---- host: the checks of both entries (include/piml_hip.h) ----

static inline bool wall_grid_ok(const piml_wall_grid* g) {
    if (!g || g->n_points < 0 || (g->n_points > 0 && (!g->points || !g->cell_start))) return false;
    if (g->gx < 1 || g->gx > kWallMaxCells || g->gy < 1 || g->gy > kWallMaxCells) return false;
    if (!std::isfinite(g->cell) || !(g->cell > 0.f) || !std::isfinite(g->cutoff) || !(g->cutoff > 0.f)) return false;
    if (g->cell < g->cutoff * kWallCellMargin) return false;
    return std::isfinite(g->x0) && std::isfinite(g->y0);
}

static inline bool wall_law_ok(float A, float B) { return std::isfinite(A) && std::isfinite(B) && A >= 0.f && B <= 0.f; }

static inline WallArgs wall_args(const piml_wall_grid& g) {
    WallArgs W;
    W.G = g;
    W.c2 = g.cutoff * g.cutoff;
    return W;
}

}  // namespace piml
