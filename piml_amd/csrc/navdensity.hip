// The density-aware floor field of a scene of gates: the travel cost of a cell grows with the crowd standing in and around it,
// and the field is solved again, per ensemble member, while the scene runs (the dynamic navigation field of Hartmann et al.
// 2014; Kretz's quickest path on an eikonal solver).  Three steps, each an entry of its own (include/piml_hip.h):
//
//   piml_nav_density     count[m][c] = the present agents of member m in cell c (integer atomics: deterministic);
//   piml_nav_cost        f[m][c] = min(1 + kd max(s / area - rho0, 0), fmax), s the window sum of count: the slowness;
//   piml_nav_relax_cost  piml_nav_relax (nav.hip) with f in the Godunov update and a member axis.
//
// The weighted step (nav_update_cost, navcost.hpp; tests/navcost_ref.py is the same function in numpy float32): with the slowness
// f >= 1 of the cell, cand = lo + f when hi is not finite or hi - lo >= f, else 0.5 ((lo + hi) + sqrt(2 f f - d d)).  f == 1
// gives nav_update's operations on the same values (2 * (1 * 1) is exactly 2), so cost == 1 is piml_nav_relax bit for bit.
// Every update restarts from the cold start (0 on goal cells, +inf elsewhere): min(cand, u) keeps a stale low value where
// the cost rose, so a warm start does not reach the fixed point (tests/test_navdensity.py shows it).
//
// The solver keeps nav_relax_kernel's temporal blocking -- K = 8 steps per launch on a 32 x 32 tile staged with a halo of 8,
// two ping-pong LDS planes, no block reads what another writes -- and stages the member's cost tile once into a third plane:
// 3 x 9216 + 2304 = 29952 bytes of LDS against 20736, so 5 workgroups (20 waves) fit a CU's 160 KB where nav_relax_kernel
// fits 7; the kernel is bound by its LDS round trips and barriers, not by latency it would need more waves to hide.
// nav_relax_kernel itself is untouched: this is a kernel of its own in a translation unit of its own.
#include "navcost.hpp"                                      // the tile constants and nav_update_cost

namespace piml {

// ---- the deposit: one thread per slot, grid (slot blocks, members) ----
__global__ __launch_bounds__(kNdThreads) void nav_density_kernel(const float2* __restrict__ position,
                                                                const float* __restrict__ mask, int capacity, float x0,
                                                                float y0, float cell, int gx, int gy,
                                                                int* __restrict__ count) {
    const int i = (int)blockIdx.x * kNdThreads + (int)threadIdx.x;
    if (i >= capacity) return;
    const size_t m = blockIdx.y;
    if (mask[m * (size_t)capacity + (size_t)i] == 0.f) return;
    const float2 p = position[m * (size_t)capacity + (size_t)i];
    // nav_direction's cell (nav.hpp); a NaN fails every comparison
    const float fcx = floorf(__fdiv_rn(__fsub_rn(p.x, x0), cell)), fcy = floorf(__fdiv_rn(__fsub_rn(p.y, y0), cell));
    if (!(fcx >= 0.f && fcx < (float)gx && fcy >= 0.f && fcy < (float)gy)) return;
    atomicAdd(count + m * (size_t)gy * (size_t)gx + (size_t)((int)fcy * gx + (int)fcx), 1);
}

// ---- the slowness: a 32 x 32 tile of one member's counts, staged with a halo of r cells; the window sum is separable ----
__global__ __launch_bounds__(kNdThreads) void nav_cost_kernel(const int* __restrict__ count, int gx, int gy, int r, float area,
                                                             float kd, float rho0, float fmax, float* __restrict__ cost) {
    __shared__ int staged[kNdSide * kNdSide];                // (32 + 2r)^2 of it used, row pitch 32 + 2r
    __shared__ int rows[kNdSide * kNdTile];                  // horizontal sums: 32 + 2r rows of 32
    const int side = kNdTile + 2 * r;
    const int X0 = (int)blockIdx.x * kNdTile - r, Y0 = (int)blockIdx.y * kNdTile - r;
    const size_t po = (size_t)blockIdx.z * (size_t)gy * (size_t)gx;
    for (int q = threadIdx.x; q < side * side; q += kNdThreads) {
        const int x = X0 + q % side, y = Y0 + q / side;
        staged[q] = x >= 0 && x < gx && y >= 0 && y < gy ? count[po + (size_t)y * (size_t)gx + (size_t)x] : 0;
    }
    __syncthreads();
    for (int q = threadIdx.x; q < side * kNdTile; q += kNdThreads) {
        const int lx = q % kNdTile, ly = q / kNdTile;
        int s = 0;
        for (int k = 0; k <= 2 * r; ++k) s += staged[ly * side + lx + k];
        rows[q] = s;
    }
    __syncthreads();
    for (int q = threadIdx.x; q < kNdTile * kNdTile; q += kNdThreads) {
        const int lx = q % kNdTile, ly = q / kNdTile;
        const int x = X0 + r + lx, y = Y0 + r + ly;
        if (x >= gx || y >= gy) continue;
        int s = 0;
        for (int k = 0; k <= 2 * r; ++k) s += rows[(ly + k) * kNdTile + lx];
        const float over = fmaxf(__fsub_rn(__fdiv_rn((float)s, area), rho0), 0.f);
        cost[po + (size_t)y * (size_t)gx + (size_t)x] = fminf(__fadd_rn(1.f, __fmul_rn(kd, over)), fmax);
    }
}

// grid (tiles x, tiles y, member * G + gate): blocked and goal are the scene's, cost the member's, u and changed the plane's
__global__ __launch_bounds__(kNdThreads) void nav_relax_cost_kernel(const unsigned char* __restrict__ blocked,
                                                                   const unsigned char* __restrict__ goal,
                                                                   const float* __restrict__ cost,
                                                                   const float* __restrict__ u_in, float* __restrict__ u_out,
                                                                   int G, int gx, int gy, int* __restrict__ changed) {
    __shared__ float plane[2][kNdCells];
    __shared__ float slow[kNdCells];
    __shared__ unsigned char fixed[kNdCells];
    const int z = (int)blockIdx.z;
    const int X0 = (int)blockIdx.x * kNdTile - kNdK, Y0 = (int)blockIdx.y * kNdTile - kNdK;
    const size_t cells = (size_t)gy * (size_t)gx;
    const size_t po = (size_t)z * cells, go = (size_t)(z % G) * cells, co = (size_t)(z / G) * cells;
    for (int q = threadIdx.x; q < kNdCells; q += kNdThreads) {
        const int lx = q % kNdSide, ly = q / kNdSide;
        const int x = X0 + lx, y = Y0 + ly;
        float v = INFINITY, f = 1.f;
        unsigned char fx = 1;
        if (x >= 0 && x < gx && y >= 0 && y < gy) {
            const size_t c = (size_t)y * (size_t)gx + (size_t)x;
            f = cost[co + c];
            if (goal[go + c]) v = 0.f;
            else if (!blocked[c]) { v = u_in[po + c]; fx = 0; }
        }
        plane[0][q] = v;
        plane[1][q] = v;
        slow[q] = f;
        fixed[q] = fx;
    }
    __syncthreads();
#pragma unroll 1
    for (int s = 1; s <= kNdK; ++s) {
        const float* src = plane[(s - 1) & 1];
        float* dst = plane[s & 1];
        for (int q = threadIdx.x; q < kNdCells; q += kNdThreads) {
            const int lx = q % kNdSide, ly = q / kNdSide;
            if (lx < s || lx >= kNdSide - s || ly < s || ly >= kNdSide - s || fixed[q]) continue;
            dst[q] = nav_update_cost(src[q], src[q - 1], src[q + 1], src[q - kNdSide], src[q + kNdSide], slow[q]);
        }
        __syncthreads();
    }
    static_assert((kNdK & 1) == 0, "the result of an even number of steps is in plane 0");
    bool diff = false;
    for (int q = threadIdx.x; q < kNdTile * kNdTile; q += kNdThreads) {
        const int lx = q % kNdTile, ly = q / kNdTile;
        const int x = X0 + kNdK + lx, y = Y0 + kNdK + ly;
        if (x >= gx || y >= gy) continue;
        const size_t c = po + (size_t)y * (size_t)gx + (size_t)x;
        const float v = plane[0][(ly + kNdK) * kNdSide + lx + kNdK];
        u_out[c] = v;
        diff |= __float_as_uint(v) != __float_as_uint(u_in[c]);
    }
    if (diff) changed[z] = 1;                                // a plain store; every writer stores the same value
}

}  // namespace piml

PIML_API int piml_nav_density(const float* position, const float* mask, int members, int capacity, float x0, float y0,
                              float cell, int gx, int gy, int* count, void* stream) {
    if (!position || !mask || !count || capacity < 1 || !piml::nd_grid_ok(members, gx, gy)) return hipErrorInvalidValue;
    if (!std::isfinite(cell) || !(cell > 0.f) || !std::isfinite(x0) || !std::isfinite(y0)) return hipErrorInvalidValue;
    hipStream_t st = piml::as_stream(stream);
    const hipError_t e = hipMemsetAsync(count, 0, (size_t)members * (size_t)gy * (size_t)gx * sizeof(int), st);
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)((capacity + piml::kNdThreads - 1) / piml::kNdThreads), (unsigned)members);
    hipLaunchKernelGGL(piml::nav_density_kernel, grid, dim3(piml::kNdThreads), 0, st, (const float2*)position, mask, capacity,
                       x0, y0, cell, gx, gy, count);
    return hipGetLastError();
}

PIML_API int piml_nav_cost(const int* count, int members, int gx, int gy, float cell, int radius_cells, float kd, float rho0,
                           float fmax, float* cost, void* stream) {
    if (!count || !cost || !piml::nd_grid_ok(members, gx, gy) || radius_cells < 0 || radius_cells > piml::kNdMaxRadius)
        return hipErrorInvalidValue;
    if (!std::isfinite(cell) || !(cell > 0.f)) return hipErrorInvalidValue;
    if (!std::isfinite(kd) || kd < 0.f || !std::isfinite(rho0) || rho0 < 0.f || !std::isfinite(fmax) || fmax < 1.f)
        return hipErrorInvalidValue;
    const int w = 2 * radius_cells + 1;
    const float area = (float)(w * w) * (cell * cell);       // host float32: one rounding per operation (-ffp-contract=off)
    if (!std::isfinite(area) || !(area > 0.f)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((gx + piml::kNdTile - 1) / piml::kNdTile), (unsigned)((gy + piml::kNdTile - 1) / piml::kNdTile),
                    (unsigned)members);
    hipLaunchKernelGGL(piml::nav_cost_kernel, grid, dim3(piml::kNdThreads), 0, piml::as_stream(stream), count, gx, gy,
                       radius_cells, area, kd, rho0, fmax, cost);
    return hipGetLastError();
}

PIML_API int piml_nav_relax_cost(const unsigned char* blocked, const unsigned char* goal, const float* cost, float* u_a,
                                 float* u_b, int members, int G, int gx, int gy, int launches, int* changed, void* stream) {
    if (!blocked || !goal || !cost || !u_a || !u_b || u_a == u_b || !changed || members < 1 || !piml::nav_dims_ok(G, gx, gy) ||
        launches < 0)
        return hipErrorInvalidValue;
    const long long planes = (long long)members * G;
    if (planes > piml::kNdMaxMembers || planes * gx * gy > 0x7fffffffLL) return hipErrorInvalidValue;   // grid.z; cells of u
    const dim3 grid((unsigned)((gx + piml::kNdTile - 1) / piml::kNdTile), (unsigned)((gy + piml::kNdTile - 1) / piml::kNdTile),
                    (unsigned)planes);
    for (int j = 0; j < launches; ++j) {
        hipLaunchKernelGGL(piml::nav_relax_cost_kernel, grid, dim3(piml::kNdThreads), 0, piml::as_stream(stream), blocked, goal,
                           cost, (const float*)(j & 1 ? u_b : u_a), j & 1 ? u_a : u_b, G, gx, gy, changed);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
