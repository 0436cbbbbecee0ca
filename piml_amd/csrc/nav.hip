// The static floor field of a scene of gates: piml_nav_relax, a Jacobi eikonal solver with temporal blocking, and
// piml_nav_direction, the lookup of nav.hpp as a stand-alone operator -- one wave per row of `position`.  The MLAPM scenario
// frame (scenario.hip, kNav) runs the same device function on the same field: position[i] + direction[i] is bitwise the point
// the frame steers an agent at position[i] bound for gate[i] to.
//
// The solver.  One step is the first-order Godunov upwind update with h = 1 (nav_update below), every operation a single
// correctly rounded float32 operation: sqrtf under -fhip-fp32-correctly-rounded-divide-sqrt is correctly rounded on gfx950,
// __fsqrt_rn is not (common.hpp), so the root is sqrtf.  A launch is K = 8 steps: a workgroup stages its 32 x 32 tile with
// a halo of K cells (48 x 48, cells outside the grid as blocked) into two LDS planes, and step s = 1 .. K updates the
// cells at least s cells inside the staged square from the plane step s - 1 wrote.  A cell's value after step s depends on
// its 4-neighbourhood after step s - 1 only, so by induction every cell at least s cells inside holds exactly u_s of the
// whole plane; after K steps that is the tile.  Fixed cells (goal: 0, blocked or outside: +inf) are staged into both
// planes and never written again.  Nothing is read from the output buffer and no block reads what another writes in the
// launch: the planes ping-pong across launches (the host alternates them).
#include "nav.hpp"

namespace piml {

constexpr int kNavK = 8;                                     // Jacobi steps per launch
constexpr int kNavTile = 32;                                 // output tile side
constexpr int kNavSide = kNavTile + 2 * kNavK;               // staged side
constexpr int kNavCells = kNavSide * kNavSide;
constexpr int kNavThreads = 256;

// one cell's step from its four neighbours (include/piml_hip.h; tests/nav_ref.py is the same function in numpy float32)
__device__ __forceinline__ float nav_update(float u, float left, float right, float down, float up) {
    const float a = left < right ? left : right, b = down < up ? down : up;
    const float lo = a < b ? a : b, hi = a < b ? b : a;
    const float d = __fsub_rn(hi, lo);
    float cand;
    if (!nav_finite(hi) || d >= 1.f) cand = __fadd_rn(lo, 1.f);
    else cand = __fmul_rn(0.5f, __fadd_rn(__fadd_rn(lo, hi), sqrtf(__fsub_rn(2.f, __fmul_rn(d, d)))));
    return cand < u ? cand : u;
}

__global__ __launch_bounds__(kNavThreads) void nav_relax_kernel(const unsigned char* __restrict__ blocked,
                                                               const unsigned char* __restrict__ goal,
                                                               const float* __restrict__ u_in, float* __restrict__ u_out,
                                                               int gx, int gy, int* __restrict__ changed) {
    __shared__ float plane[2][kNavCells];
    __shared__ unsigned char fixed[kNavCells];
    const int g = (int)blockIdx.z;
    const int X0 = (int)blockIdx.x * kNavTile - kNavK, Y0 = (int)blockIdx.y * kNavTile - kNavK;
    const size_t po = (size_t)g * (size_t)gy * (size_t)gx;
    for (int q = threadIdx.x; q < kNavCells; q += kNavThreads) {
        const int lx = q % kNavSide, ly = q / kNavSide;
        const int x = X0 + lx, y = Y0 + ly;
        float v = INFINITY;
        unsigned char fx = 1;
        if (x >= 0 && x < gx && y >= 0 && y < gy) {
            const size_t c = (size_t)y * (size_t)gx + (size_t)x;
            if (goal[po + c]) v = 0.f;
            else if (!blocked[c]) { v = u_in[po + c]; fx = 0; }
        }
        plane[0][q] = v;
        plane[1][q] = v;
        fixed[q] = fx;
    }
    __syncthreads();
#pragma unroll 1
    for (int s = 1; s <= kNavK; ++s) {
        const float* src = plane[(s - 1) & 1];
        float* dst = plane[s & 1];
        for (int q = threadIdx.x; q < kNavCells; q += kNavThreads) {
            const int lx = q % kNavSide, ly = q / kNavSide;
            if (lx < s || lx >= kNavSide - s || ly < s || ly >= kNavSide - s || fixed[q]) continue;
            dst[q] = nav_update(src[q], src[q - 1], src[q + 1], src[q - kNavSide], src[q + kNavSide]);
        }
        __syncthreads();
    }
    static_assert((kNavK & 1) == 0, "the result of an even number of steps is in plane 0");
    bool diff = false;
    for (int q = threadIdx.x; q < kNavTile * kNavTile; q += kNavThreads) {
        const int lx = q % kNavTile, ly = q / kNavTile;
        const int x = X0 + kNavK + lx, y = Y0 + kNavK + ly;
        if (x >= gx || y >= gy) continue;
        const size_t c = po + (size_t)y * (size_t)gx + (size_t)x;
        const float v = plane[0][(ly + kNavK) * kNavSide + lx + kNavK];
        u_out[c] = v;
        diff |= __float_as_uint(v) != __float_as_uint(u_in[c]);
    }
    if (diff) changed[g] = 1;                                // a plain store; every writer stores the same value
}

__global__ __launch_bounds__(kNavWaves * 64) void nav_direction_kernel(const float2* __restrict__ position,
                                                                      const int* __restrict__ gate,
                                                                      const float2* __restrict__ destination, long long rows,
                                                                      const piml_nav_grid N, float2* __restrict__ direction,
                                                                      int* __restrict__ branch, int* __restrict__ neighbour) {
    const long long i = (long long)blockIdx.x * kNavWaves + (threadIdx.x >> 6);
    if (i >= rows) return;                                   // wave-uniform
    const float2 p = position[i], t = destination[i];
    const NavDir d = nav_direction(N, gate[i], p, t);
    if ((threadIdx.x & 63) == 0) {
        direction[i] = d.e;
        if (branch) branch[i] = d.branch;
        if (neighbour) neighbour[i] = d.neighbour;
    }
}

}  // namespace piml

PIML_API int piml_nav_relax(const unsigned char* blocked, const unsigned char* goal, float* u_a, float* u_b, int G, int gx,
                            int gy, int launches, int* changed, void* stream) {
    if (!blocked || !goal || !u_a || !u_b || u_a == u_b || !changed || !piml::nav_dims_ok(G, gx, gy) || launches < 0)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)((gx + piml::kNavTile - 1) / piml::kNavTile), (unsigned)((gy + piml::kNavTile - 1) / piml::kNavTile),
                    (unsigned)G);
    for (int j = 0; j < launches; ++j) {
        hipLaunchKernelGGL(piml::nav_relax_kernel, grid, dim3(piml::kNavThreads), 0, piml::as_stream(stream), blocked, goal,
                           (const float*)(j & 1 ? u_b : u_a), j & 1 ? u_a : u_b, gx, gy, changed);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

PIML_API int piml_nav_direction(const float* position, const int* gate, const float* destination, long long rows,
                                const piml_nav_grid* g, float* direction, int* branch, int* neighbour, void* stream) {
    if (rows < 0 || !direction || !piml::nav_grid_ok(g)) return hipErrorInvalidValue;
    if (rows == 0) return hipSuccess;
    if (!position || !gate || !destination) return hipErrorInvalidValue;
    const long long blocks = (rows + piml::kNavWaves - 1) / piml::kNavWaves;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(piml::nav_direction_kernel, dim3((unsigned)blocks), dim3(piml::kNavWaves * 64), 0, piml::as_stream(stream),
                       (const float2*)position, gate, (const float2*)destination, rows, *g, (float2*)direction, branch,
                       neighbour);
    return hipGetLastError();
}
