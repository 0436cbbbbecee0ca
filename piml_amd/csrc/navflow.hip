// The direction-aware density of the floor field: a counted person weighs by how much slower than the walker they move along
// the walker's way to its gate (Hartmann et al. 2014; Kretz's dynamic distance potential), so a column walking through a door
// towards my gate does not close it to me, and the same column coming at me closes it twice.  Four entries
// (include/piml_hip.h), beside navdensity.hip's three, which stay what they were:
//
//   piml_nav_descent           d[g][c] = the upwind unit direction of steepest descent of the STATIC field u[g], once per scene;
//   piml_nav_flow              navdensity's deposit, and beside count two int32 planes of velocity components in 2^-10 m/s;
//   piml_nav_cost_flow         per (member, gate, cell): s_eff = s - flow (p . d) / (1024 vref) in place of the head count s;
//   piml_nav_relax_cost_gates  piml_nav_relax_cost with the cost read from plane member * G + gate.
//
// Every operation of the three rules is a single correctly rounded float32 operation (tests/navflow_ref.py restates them in
// numpy) and the sums are integers, so the planes are the restatement's bit for bit; flow == 0 gives s_eff == s exactly
// (fmul(0, along) is a zero of either sign, and s - (+-0) is s), so every gate's plane is then piml_nav_cost's.
//
// The cost kernel stages one member's tile of count with its halo of r cells in LDS, takes the separable window sum (rows, then
// columns) into registers -- four cells a thread --, does the same for the two momentum planes through the SAME two LDS
// buffers (15360 bytes, nav_cost_kernel's: the three sums are needed together only in registers), and then loops over the
// gates: a gate costs one float2 load and one store per cell, not a staging.  The solver is nav_relax_cost_kernel written out
// again with the cost plane's offset changed: a shared body, a template over that offset inlined into both kernels, gave
// nav_relax_cost_kernel other instructions in each of the three forms tried, and that kernel keeps its compiled code.
#include "navcost.hpp"

namespace piml {

constexpr int kNfMaxCapacity = 1 << 18;                      // a window sum of momenta (|q| <= 2^13 each) stays inside int32
constexpr int kNfPerThread = kNdTile * kNdTile / kNdThreads; // cells of the output tile a thread holds

// ---- the descent direction: one thread per cell, grid (cell blocks, gates) ----
__global__ __launch_bounds__(kNdThreads) void nav_descent_kernel(const float* __restrict__ u, int gx, int gy,
                                                                float2* __restrict__ d) {
    const int c = (int)blockIdx.x * kNdThreads + (int)threadIdx.x;
    if (c >= gx * gy) return;
    const int x = c % gx, y = c / gx;
    const float* __restrict__ plane = u + (size_t)blockIdx.y * (size_t)gy * (size_t)gx;
    const float uc = plane[c];
    const float L = x > 0 ? plane[c - 1] : INFINITY, R = x < gx - 1 ? plane[c + 1] : INFINITY;
    const float D = y > 0 ? plane[c - gx] : INFINITY, U = y < gy - 1 ? plane[c + gx] : INFINITY;
    const float a = L < R ? L : R, b = D < U ? D : U;
    float rx = nav_finite(uc) && nav_finite(a) && a < uc ? __fsub_rn(uc, a) : 0.f;
    float ry = nav_finite(uc) && nav_finite(b) && b < uc ? __fsub_rn(uc, b) : 0.f;
    if (L < R) rx = -rx;                                     // the lower neighbour lies towards -x
    if (D < U) ry = -ry;
    const float n = sqrtf(__fadd_rn(__fmul_rn(rx, rx), __fmul_rn(ry, ry)));
    d[(size_t)blockIdx.y * (size_t)gy * (size_t)gx + (size_t)c] =
        n > 0.f ? make_float2(__fdiv_rn(rx, n), __fdiv_rn(ry, n)) : make_float2(0.f, 0.f);
}

// a velocity component in 2^-10 m/s, clamped to +-8 m/s; rintf rounds halves to even
__device__ __forceinline__ int nav_flow_q(float v) {
    return nav_finite(v) ? (int)rintf(__fmul_rn(fminf(fmaxf(v, -8.f), 8.f), 1024.f)) : 0;
}

// ---- the deposit: nav_density_kernel's slot, cell and count, and the slot's velocity into the member's two momentum planes ----
__global__ __launch_bounds__(kNdThreads) void nav_flow_kernel(const float2* __restrict__ position,
                                                             const float2* __restrict__ velocity,
                                                             const float* __restrict__ mask, int capacity, float x0, float y0,
                                                             float cell, int gx, int gy, int* __restrict__ count,
                                                             int* __restrict__ mom) {
    const int i = (int)blockIdx.x * kNdThreads + (int)threadIdx.x;
    if (i >= capacity) return;
    const size_t m = blockIdx.y;
    if (mask[m * (size_t)capacity + (size_t)i] == 0.f) return;
    const float2 p = position[m * (size_t)capacity + (size_t)i];
    const float fcx = floorf(__fdiv_rn(__fsub_rn(p.x, x0), cell)), fcy = floorf(__fdiv_rn(__fsub_rn(p.y, y0), cell));
    if (!(fcx >= 0.f && fcx < (float)gx && fcy >= 0.f && fcy < (float)gy)) return;
    const size_t cells = (size_t)gy * (size_t)gx, c = (size_t)((int)fcy * gx + (int)fcx);
    atomicAdd(count + m * cells + c, 1);
    const float2 v = velocity[m * (size_t)capacity + (size_t)i];
    const int qx = nav_flow_q(v.x), qy = nav_flow_q(v.y);
    if (qx) atomicAdd(mom + (2 * m) * cells + c, qx);
    if (qy) atomicAdd(mom + (2 * m + 1) * cells + c, qy);
}

// ---- the slowness per gate: grid (tiles x, tiles y, members) ----
__global__ __launch_bounds__(kNdThreads) void nav_cost_flow_kernel(const int* __restrict__ count, const int* __restrict__ mom,
                                                                  const float2* __restrict__ d, int G, int gx, int gy, int r,
                                                                  float area, float kd, float rho0, float fmax, float flow,
                                                                  float unit, float* __restrict__ cost) {
    __shared__ int staged[kNdSide * kNdSide];                // (32 + 2r)^2 of it used, row pitch 32 + 2r
    __shared__ int rows[kNdSide * kNdTile];                  // horizontal sums: 32 + 2r rows of 32
    const int side = kNdTile + 2 * r;
    const int X0 = (int)blockIdx.x * kNdTile - r, Y0 = (int)blockIdx.y * kNdTile - r;
    const size_t cells = (size_t)gy * (size_t)gx, m = blockIdx.z;
    int sum[3][kNfPerThread];                                // the window sums of count, mom x, mom y at this thread's cells
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int* __restrict__ src = k == 0 ? count + m * cells : mom + (2 * m + (size_t)(k - 1)) * cells;
        // (staged was last read before the previous plane's second barrier, rows before this plane's first)
        for (int q = threadIdx.x; q < side * side; q += kNdThreads) {
            const int x = X0 + q % side, y = Y0 + q / side;
            staged[q] = x >= 0 && x < gx && y >= 0 && y < gy ? src[(size_t)y * (size_t)gx + (size_t)x] : 0;
        }
        __syncthreads();
        for (int q = threadIdx.x; q < side * kNdTile; q += kNdThreads) {
            const int lx = q % kNdTile, ly = q / kNdTile;
            int s = 0;
            for (int j = 0; j <= 2 * r; ++j) s += staged[ly * side + lx + j];
            rows[q] = s;
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < kNfPerThread; ++t) {
            const int q = (int)threadIdx.x + t * kNdThreads;
            const int lx = q % kNdTile, ly = q / kNdTile;
            int s = 0;
            for (int j = 0; j <= 2 * r; ++j) s += rows[(ly + j) * kNdTile + lx];
            sum[k][t] = s;
        }
    }
    for (int g = 0; g < G; ++g) {
#pragma unroll
        for (int t = 0; t < kNfPerThread; ++t) {
            const int q = (int)threadIdx.x + t * kNdThreads;
            const int x = X0 + r + q % kNdTile, y = Y0 + r + q / kNdTile;
            if (x >= gx || y >= gy) continue;
            const size_t c = (size_t)y * (size_t)gx + (size_t)x;
            const float2 e = d[(size_t)g * cells + c];
            const float pd = __fadd_rn(__fmul_rn((float)sum[1][t], e.x), __fmul_rn((float)sum[2][t], e.y));
            const float s_eff = __fsub_rn((float)sum[0][t], __fmul_rn(flow, __fdiv_rn(pd, unit)));
            const float over = fmaxf(__fsub_rn(__fdiv_rn(s_eff, area), rho0), 0.f);
            cost[(m * (size_t)G + (size_t)g) * cells + c] = fminf(__fadd_rn(1.f, __fmul_rn(kd, over)), fmax);
        }
    }
}

// grid (tiles x, tiles y, member * G + gate): nav_relax_cost_kernel (navdensity.hip) statement for statement, but for the cost
// plane, which is the plane's own: blocked and goal are the scene's; cost, u and changed the plane's
__global__ __launch_bounds__(kNdThreads) void nav_relax_cost_gates_kernel(const unsigned char* __restrict__ blocked,
                                                                         const unsigned char* __restrict__ goal,
                                                                         const float* __restrict__ cost,
                                                                         const float* __restrict__ u_in,
                                                                         float* __restrict__ u_out, int G, int gx, int gy,
                                                                         int* __restrict__ changed) {
    __shared__ float plane[2][kNdCells];
    __shared__ float slow[kNdCells];
    __shared__ unsigned char fixed[kNdCells];
    const int z = (int)blockIdx.z;
    const int X0 = (int)blockIdx.x * kNdTile - kNdK, Y0 = (int)blockIdx.y * kNdTile - kNdK;
    const size_t cells = (size_t)gy * (size_t)gx;
    const size_t po = (size_t)z * cells, go = (size_t)(z % G) * cells;
    for (int q = threadIdx.x; q < kNdCells; q += kNdThreads) {
        const int lx = q % kNdSide, ly = q / kNdSide;
        const int x = X0 + lx, y = Y0 + ly;
        float v = INFINITY, f = 1.f;
        unsigned char fx = 1;
        if (x >= 0 && x < gx && y >= 0 && y < gy) {
            const size_t c = (size_t)y * (size_t)gx + (size_t)x;
            f = cost[po + c];
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

PIML_API int piml_nav_descent(const float* u, int G, int gx, int gy, float* d, void* stream) {
    if (!u || !d || !piml::nav_dims_ok(G, gx, gy)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((gx * gy + piml::kNdThreads - 1) / piml::kNdThreads), (unsigned)G);
    hipLaunchKernelGGL(piml::nav_descent_kernel, grid, dim3(piml::kNdThreads), 0, piml::as_stream(stream), u, gx, gy, (float2*)d);
    return hipGetLastError();
}

PIML_API int piml_nav_flow(const float* position, const float* velocity, const float* mask, int members, int capacity, float x0,
                           float y0, float cell, int gx, int gy, int* count, int* mom, void* stream) {
    if (!position || !velocity || !mask || !count || !mom || capacity < 1 || capacity >= piml::kNfMaxCapacity ||
        !piml::nd_grid_ok(members, gx, gy))
        return hipErrorInvalidValue;
    if (!std::isfinite(cell) || !(cell > 0.f) || !std::isfinite(x0) || !std::isfinite(y0)) return hipErrorInvalidValue;
    hipStream_t st = piml::as_stream(stream);
    const size_t plane = (size_t)members * (size_t)gy * (size_t)gx * sizeof(int);
    hipError_t e = hipMemsetAsync(count, 0, plane, st);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(mom, 0, 2 * plane, st);
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)((capacity + piml::kNdThreads - 1) / piml::kNdThreads), (unsigned)members);
    hipLaunchKernelGGL(piml::nav_flow_kernel, grid, dim3(piml::kNdThreads), 0, st, (const float2*)position,
                       (const float2*)velocity, mask, capacity, x0, y0, cell, gx, gy, count, mom);
    return hipGetLastError();
}

PIML_API int piml_nav_cost_flow(const int* count, const int* mom, const float* d, int members, int G, int gx, int gy, float cell,
                                int radius_cells, float kd, float rho0, float fmax, float flow, float vref, float* cost,
                                void* stream) {
    if (!count || !mom || !d || !cost || !piml::nd_grid_ok(members, gx, gy) || !piml::nd_planes_ok(members, G, gx, gy) ||
        radius_cells < 0 || radius_cells > piml::kNdMaxRadius)
        return hipErrorInvalidValue;
    if (!std::isfinite(cell) || !(cell > 0.f)) return hipErrorInvalidValue;
    if (!std::isfinite(kd) || kd < 0.f || !std::isfinite(rho0) || rho0 < 0.f || !std::isfinite(fmax) || fmax < 1.f)
        return hipErrorInvalidValue;
    if (!std::isfinite(flow) || flow < 0.f || !std::isfinite(vref) || !(vref > 0.f)) return hipErrorInvalidValue;
    const int w = 2 * radius_cells + 1;
    const float area = (float)(w * w) * (cell * cell);       // host float32: one rounding per operation (-ffp-contract=off)
    if (!std::isfinite(area) || !(area > 0.f)) return hipErrorInvalidValue;
    const float unit = 1024.f * vref;                        // a momentum of vref in the planes' unit
    const dim3 grid((unsigned)((gx + piml::kNdTile - 1) / piml::kNdTile), (unsigned)((gy + piml::kNdTile - 1) / piml::kNdTile),
                    (unsigned)members);
    hipLaunchKernelGGL(piml::nav_cost_flow_kernel, grid, dim3(piml::kNdThreads), 0, piml::as_stream(stream), count, mom,
                       (const float2*)d, G, gx, gy, radius_cells, area, kd, rho0, fmax, flow, unit, cost);
    return hipGetLastError();
}

PIML_API int piml_nav_relax_cost_gates(const unsigned char* blocked, const unsigned char* goal, const float* cost, float* u_a,
                                       float* u_b, int members, int G, int gx, int gy, int launches, int* changed,
                                       void* stream) {
    if (!blocked || !goal || !cost || !u_a || !u_b || u_a == u_b || !changed || launches < 0 ||
        !piml::nd_planes_ok(members, G, gx, gy))
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)((gx + piml::kNdTile - 1) / piml::kNdTile), (unsigned)((gy + piml::kNdTile - 1) / piml::kNdTile),
                    (unsigned)(members * G));
    for (int j = 0; j < launches; ++j) {
        hipLaunchKernelGGL(piml::nav_relax_cost_gates_kernel, grid, dim3(piml::kNdThreads), 0, piml::as_stream(stream), blocked,
                           goal, cost, (const float*)(j & 1 ? u_b : u_a), j & 1 ? u_a : u_b, G, gx, gy, changed);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
