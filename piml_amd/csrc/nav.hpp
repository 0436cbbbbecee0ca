// The floor field's lookup of the MLAPM scenario frame (piml_scenario_step_mlapm_nav) and of its stand-alone operator
// (piml_nav_direction): the desired direction e of an agent at p bound for gate g, from u[g], the gate's geodesic distance
// over the free cells of a static grid in CELL units (piml_nav_relax, nav.hip; +inf on blocked and unreachable cells).
//
//   c = the agent's cell, (floor((p.x - x0) / cell), floor((p.y - y0) / cell)) in float32 (the wall grid's formula).
//   0 straight:  e = (dest - p) / max(|dest - p|, 1e-12), the frame's own line (nav_straight), when p is NaN, g is outside
//                0..G-1, c is outside the grid, u[c] is not finite, u[c] <= near, or neither branch below applies.
//   1 bilinear:  f = (p - origin) / cell - 0.5 per axis, i0 = floor(f), t = f - i0: the centres of the cells i0, i0 + 1 per
//                axis surround p.  All four inside the grid and finite: grad = ((1 - ty)(u10 - u00) + ty (u11 - u01),
//                (1 - tx)(u01 - u00) + tx (u11 - u10)), n2 = fadd(fmul(gx, gx), fmul(gy, gy)); n2 > 0: e = -grad rsq(n2).
//                n2 == 0 (a plateau or a saddle of the interpolant) falls through to
//   2 descent:   the 8-neighbour n of c that maximises s = (u[c] - u[n]) w > 0, w = 1 for the four orthogonal ones and
//                fl(1 / sqrt 2) for the diagonals, u[n] finite; a diagonal is skipped when either orthogonal cell beside it
//                is not finite (no corner is cut); ORDER: E, W, N, S, NE, NW, SE, SW, N = +y, and a later
//                neighbour replaces an earlier one only when its s is strictly larger, so ties go to the first.  e points
//                from p to n's centre origin + (n + 0.5) cell.  No neighbour qualifies: branch 0.
//   3 sight:     (nav_direction<true> only) in front of 1 and 2: the centre of parent[g][c], the next turning point of the
//                shortest path from c (piml_nav_sight_relax, navsight.hip); see kSight below.
// Every predicate above is one correctly rounded float32 operation after another (tests/nav_ref.py restates them in numpy),
// so branch and neighbour are exact; e uses the hardware rsq (1e-5 relative, as the pair law and the wall term).
// Cells outside the grid read as +inf (the load is from the cell clamped into the grid) and g is range-checked: no index
// leaves u.  The frame steers to the point fl(p + e) in branches 1 and 2 (scenario.hip, kNav), to the destination in branch 0.
// Known limit: the first-order scheme is anisotropic.  On an empty grid with a point goal the bilinear direction is off the
// straight line by 3 degrees on average, 16 degrees at worst beyond 2 cells and 8.7 degrees beyond 8.
#pragma once
#include "common.hpp"
#include "mlapm.hpp"
#include "../../include/piml_hip.h"

#include <cmath>

namespace piml {

constexpr int kNavMaxCells = 1024;               // per axis
constexpr int kNavMaxGates = 64;
constexpr int kNavWaves = 4;                     // waves (rows) per block of the operator
constexpr float kNavDiag = 0.70710678118654752f; // fl(1 / sqrt 2)

struct NavDir {
    float2 e;
    int branch, neighbour;
};

// the frame's own desired direction (scenario_mlapm_body; mlapm.py:21)
__device__ __forceinline__ float2 nav_straight(float2 p, float2 dest) {
    float ex = dest.x - p.x, ey = dest.y - p.y;
    const float en = fmaxf(norm2(ex, ey), 1e-12f);
    ex /= en; ey /= en;
    return make_float2(ex, ey);
}

// u[g] at cell (x, y); +inf outside the grid.  The load is unconditional, from the cell clamped into the grid: no index
// leaves the plane, and nothing branches
__device__ __forceinline__ float nav_u(const piml_nav_grid& N, const float* __restrict__ plane, int x, int y) {
    const bool in = x >= 0 && x < N.gx && y >= 0 && y < N.gy;
    const int xc = min(max(x, 0), N.gx - 1), yc = min(max(y, 0), N.gy - 1);
    const float v = plane[(size_t)(yc * N.gx + xc)];
    return in ? v : INFINITY;
}

__device__ __forceinline__ bool nav_finite(float x) { return fabsf(x) < INFINITY; }

// One wave, one agent: p, dest and g are the same in every lane, and so is the result.  Written without branches: the three
// candidates are all computed (13 loads of words every lane shares) and the result is selected, which keeps the frame's
// scalar registers free of saved execution masks; what a refused branch computed (inf - inf, say) is never selected.
//
// kSight (piml_nav_direction_sight, piml_scenario_step_mlapm_sight): branch 3 in front of the other two.  parent (G, gy, gx) is
// the any-angle table of piml_nav_sight_relax; where the field applies and q = parent[g][c] >= 0 is not c itself, e points
// from p to q's centre (branch 2's centre formula), whose segment from any point of c enters no blocked cell.  One more load,
// two integer divisions by gx, the same selects.  kSight == false does not read `parent` and compiles to what it was.
template <bool kSight = false>
__device__ __forceinline__ NavDir nav_direction(const piml_nav_grid& N, int g, float2 p, float2 dest,
                                                const int* __restrict__ parent = nullptr) {
    const float2 e0 = nav_straight(p, dest);
    const float qx = __fdiv_rn(__fsub_rn(p.x, N.x0), N.cell), qy = __fdiv_rn(__fsub_rn(p.y, N.y0), N.cell);
    const float fcx = floorf(qx), fcy = floorf(qy);
    const bool inside = p.x == p.x && p.y == p.y && g >= 0 && g < N.G &&
                        fcx >= 0.f && fcx < (float)N.gx && fcy >= 0.f && fcy < (float)N.gy;
    const int cx = (int)fminf(fmaxf(fcx, -1.f), (float)N.gx), cy = (int)fminf(fmaxf(fcy, -1.f), (float)N.gy);
    const float* __restrict__ plane = N.u + (size_t)min(max(g, 0), N.G - 1) * (size_t)(N.gy * N.gx);
    const float uc = nav_u(N, plane, cx, cy);
    const bool field = inside && nav_finite(uc) && uc > N.near;
    // 1: the bilinear interpolant of the four surrounding centres
    const float fx = __fsub_rn(qx, 0.5f), fy = __fsub_rn(qy, 0.5f);
    const float fi = floorf(fx), fj = floorf(fy);
    const bool around = fi >= 0.f && fi <= (float)(N.gx - 2) && fj >= 0.f && fj <= (float)(N.gy - 2);
    const int i0 = (int)fminf(fmaxf(fi, -1.f), (float)N.gx), j0 = (int)fminf(fmaxf(fj, -1.f), (float)N.gy);
    const float u00 = nav_u(N, plane, i0, j0), u10 = nav_u(N, plane, i0 + 1, j0);
    const float u01 = nav_u(N, plane, i0, j0 + 1), u11 = nav_u(N, plane, i0 + 1, j0 + 1);
    const float tx = __fsub_rn(fx, fi), ty = __fsub_rn(fy, fj);
    const float gx = __fadd_rn(__fmul_rn(__fsub_rn(1.f, ty), __fsub_rn(u10, u00)), __fmul_rn(ty, __fsub_rn(u11, u01)));
    const float gy = __fadd_rn(__fmul_rn(__fsub_rn(1.f, tx), __fsub_rn(u01, u00)), __fmul_rn(tx, __fsub_rn(u11, u10)));
    const float g2 = __fadd_rn(__fmul_rn(gx, gx), __fmul_rn(gy, gy));
    const bool bilinear = field && around && nav_finite(u00) && nav_finite(u10) && nav_finite(u01) && nav_finite(u11) && g2 > 0.f;
    // 2: steepest descent over the 8 neighbours, E W N S NE NW SE SW; a later one wins only when strictly better
    const float uE = nav_u(N, plane, cx + 1, cy), uW = nav_u(N, plane, cx - 1, cy);
    const float uN = nav_u(N, plane, cx, cy + 1), uS = nav_u(N, plane, cx, cy - 1);
    const float uNE = nav_u(N, plane, cx + 1, cy + 1), uNW = nav_u(N, plane, cx - 1, cy + 1);
    const float uSE = nav_u(N, plane, cx + 1, cy - 1), uSW = nav_u(N, plane, cx - 1, cy - 1);
    const bool okE = nav_finite(uE), okW = nav_finite(uW), okN = nav_finite(uN), okS = nav_finite(uS);
    float best = 0.f, s;
    int k = -1;
    bool take;
    s = __fsub_rn(uc, uE); take = okE && s > best; best = take ? s : best; k = take ? 0 : k;
    s = __fsub_rn(uc, uW); take = okW && s > best; best = take ? s : best; k = take ? 1 : k;
    s = __fsub_rn(uc, uN); take = okN && s > best; best = take ? s : best; k = take ? 2 : k;
    s = __fsub_rn(uc, uS); take = okS && s > best; best = take ? s : best; k = take ? 3 : k;
    s = __fmul_rn(__fsub_rn(uc, uNE), kNavDiag); take = okN && okE && nav_finite(uNE) && s > best; best = take ? s : best; k = take ? 4 : k;
    s = __fmul_rn(__fsub_rn(uc, uNW), kNavDiag); take = okN && okW && nav_finite(uNW) && s > best; best = take ? s : best; k = take ? 5 : k;
    s = __fmul_rn(__fsub_rn(uc, uSE), kNavDiag); take = okS && okE && nav_finite(uSE) && s > best; best = take ? s : best; k = take ? 6 : k;
    s = __fmul_rn(__fsub_rn(uc, uSW), kNavDiag); take = okS && okW && nav_finite(uSW) && s > best; best = take ? s : best; k = take ? 7 : k;
    const int dx = (k == 0 || k == 4 || k == 6) ? 1 : (k == 2 || k == 3) ? 0 : -1;
    const int dy = (k == 2 || k == 4 || k == 5) ? 1 : (k == 0 || k == 1) ? 0 : -1;
    const float hx = __fsub_rn(__fadd_rn(N.x0, __fmul_rn(__fadd_rn((float)(cx + dx), 0.5f), N.cell)), p.x);
    const float hy = __fsub_rn(__fadd_rn(N.y0, __fmul_rn(__fadd_rn((float)(cy + dy), 0.5f), N.cell)), p.y);
    const float h2 = __fadd_rn(__fmul_rn(hx, hx), __fmul_rn(hy, hy));
    const bool descent = field && !bilinear && k >= 0 && h2 > 0.f;
    if constexpr (kSight) {
        // 3: the parent's centre.  The load is from the cell clamped into the grid, the parent clamped into the plane
        const int cells = N.gy * N.gx;
        const int lin = min(max(cy, 0), N.gy - 1) * N.gx + min(max(cx, 0), N.gx - 1);
        const int q = parent[(size_t)min(max(g, 0), N.G - 1) * (size_t)cells + (size_t)lin];
        const int qc = min(max(q, 0), cells - 1);
        const float sx = __fsub_rn(__fadd_rn(N.x0, __fmul_rn(__fadd_rn((float)(qc % N.gx), 0.5f), N.cell)), p.x);
        const float sy = __fsub_rn(__fadd_rn(N.y0, __fmul_rn(__fadd_rn((float)(qc / N.gx), 0.5f), N.cell)), p.y);
        const float s2 = __fadd_rn(__fmul_rn(sx, sx), __fmul_rn(sy, sy));
        const bool sight = field && q >= 0 && q < cells && q != lin && s2 > 0.f;
        const float rinv = fast_rsq(sight ? s2 : bilinear ? g2 : h2);
        NavDir d;
        d.e.x = sight ? sx * rinv : bilinear ? -gx * rinv : descent ? hx * rinv : e0.x;
        d.e.y = sight ? sy * rinv : bilinear ? -gy * rinv : descent ? hy * rinv : e0.y;
        d.branch = sight ? 3 : bilinear ? 1 : descent ? 2 : 0;
        d.neighbour = descent && !sight ? k : -1;
        return d;
    } else {
        const float rinv = fast_rsq(bilinear ? g2 : h2);
        NavDir d;
        d.e.x = bilinear ? -gx * rinv : descent ? hx * rinv : e0.x;
        d.e.y = bilinear ? -gy * rinv : descent ? hy * rinv : e0.y;
        d.branch = bilinear ? 1 : descent ? 2 : 0;
        d.neighbour = descent ? k : -1;
        return d;
    }
}

// ---- host: the grid checks of piml_nav_direction and piml_scenario_step_mlapm_nav (include/piml_hip.h) ----

static inline bool nav_dims_ok(int G, int gx, int gy) {
    return G >= 1 && G <= kNavMaxGates && gx >= 1 && gx <= kNavMaxCells && gy >= 1 && gy <= kNavMaxCells;
}

static inline bool nav_grid_ok(const piml_nav_grid* g) {
    if (!g || !g->u || !nav_dims_ok(g->G, g->gx, g->gy)) return false;
    if (!std::isfinite(g->cell) || !(g->cell > 0.f) || !std::isfinite(g->near) || g->near < 0.f) return false;
    return std::isfinite(g->x0) && std::isfinite(g->y0);
}

// the table of the sight branch against the grid it goes with
static inline bool nav_sight_ok(const piml_nav_sight* s, const piml_nav_grid* g) {
    return s && g && s->parent && s->G == g->G && s->gx == g->gx && s->gy == g->gy;
}

}  // namespace piml
