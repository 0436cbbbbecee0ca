// What the weighted floor-field solvers of navdensity.hip (one cost plane per member) and navflow.hip (one per member and
// gate) share: the tile constants, the weighted step and the host-side checks.  The two kernels are written out in their own
// translation units: nav_relax_cost_kernel keeps its compiled code that way.
#pragma once
#include "nav.hpp"

namespace piml {

constexpr int kNdK = 8;                                      // Jacobi steps per launch (nav.hip's kNavK)
constexpr int kNdTile = 32;                                  // output tile side
constexpr int kNdSide = kNdTile + 2 * kNdK;                  // staged side
constexpr int kNdCells = kNdSide * kNdSide;
constexpr int kNdThreads = 256;
constexpr int kNdMaxRadius = 8;                              // the cost window's radius in cells
constexpr int kNdMaxMembers = 65535;

// one cell's weighted step from its four neighbours; f is the cell's slowness
__device__ __forceinline__ float nav_update_cost(float u, float left, float right, float down, float up, float f) {
    const float a = left < right ? left : right, b = down < up ? down : up;
    const float lo = a < b ? a : b, hi = a < b ? b : a;
    const float d = __fsub_rn(hi, lo);
    float cand;
    if (!nav_finite(hi) || d >= f) cand = __fadd_rn(lo, f);
    else cand = __fmul_rn(0.5f, __fadd_rn(__fadd_rn(lo, hi), sqrtf(__fsub_rn(__fmul_rn(2.f, __fmul_rn(f, f)), __fmul_rn(d, d)))));
    return cand < u ? cand : u;
}

static inline bool nd_grid_ok(int members, int gx, int gy) {
    return members >= 1 && members <= kNdMaxMembers && gx >= 1 && gx <= kNavMaxCells && gy >= 1 && gy <= kNavMaxCells;
}

// the plane checks the two weighted solvers share: grid.z = members * G planes, and the cells of u fit an int
static inline bool nd_planes_ok(int members, int G, int gx, int gy) {
    if (members < 1 || !nav_dims_ok(G, gx, gy)) return false;
    const long long planes = (long long)members * G;
    return planes <= kNdMaxMembers && planes * gx * gy <= 0x7fffffffLL;
}

}  // namespace piml
