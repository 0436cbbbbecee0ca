// The any-angle floor field: piml_nav_sight_relax, a Theta*-style propagation of (w, parent) run as a Jacobi relaxation, and
// piml_nav_direction_sight, the lookup of nav.hpp with its sight branch as a stand-alone operator.  parent[g][c] is the next
// turning point of the taut string from cell c to gate g; w[g][c] the string's length in cells (include/piml_hip.h has the
// definitions; tests/navsight_ref.py is the same function in numpy float32 and Python integers, bit for bit).
//
// One launch is ONE Jacobi step, one wave per cell (the cell comes from blockIdx and the wave's number read into a scalar).
// Lanes 0 .. 7 take the eight neighbour slots side by side -- a slot's chain of dependent loads, w[n], parent[n], the cache,
// w[q], is what a step costs once the field stands, and one after the other the eight chains cost a step of GC's 0.125 m
// grid 0.9 ms, walks or no walks -- and the candidates are then compared in slot order.  A candidate's parent q is the
// neighbour's parent when c sees it and the neighbour otherwise; visible(c, q) depends on the static mask alone, so the wave
// keeps the last (q, result) of each slot in `cache` and walks a sight line, all 64 lanes on it, only where a neighbour's
// parent moved: on the front.  A slot is read and written by its own cell's wave only, and what it holds is true in any
// step, so the cache needs no second plane and a replayed graph of launches finds it valid.
//
// The walk (sight_visible).  X = c + a obstructs when it is blocked and some t in [0, 1] has |a - t D| < 1 - t / 2 on both
// axes, D = q - c.  1 - t / 2 <= 1, so on the major axis M (|D_M| >= |D_m|) t lies within 1 / |D_M| of a_M / D_M, where the
// line's minor coordinate t D_m stays within 1 of r = a_M D_m / D_M: |a_m - r| < 2, the four cells floor(r) - 1 .. floor(r) + 2.
// The lanes stride a_M over the bounding box grown by one cell, test those four cells each with the exact integer test,
// and a wave vote gives the result; testing a cell too many changes nothing.  Products stay below 2^23 for 1024 cells.
#include "nav.hpp"

namespace piml {

constexpr int kSightWaves = 4;                               // waves (cells) per block

// the mask gate g sees: outside the grid, or blocked and not one of its goal cells (a goal cell is free, as in nav_relax)
__device__ __forceinline__ bool sight_blocked(const unsigned char* __restrict__ blocked, const unsigned char* __restrict__ goal,
                                              int gx, int gy, int x, int y) {
    if (x < 0 || x >= gx || y < 0 || y >= gy) return true;
    const int c = y * gx + x;
    return blocked[c] != 0 && goal[c] == 0;
}

// the bounds l < t < u that |a - t D| < 1 - t / 2 puts on t: t (2 D - 1) > 2 a - 2 and t (2 D + 1) < 2 a + 2, as fractions with
// positive denominators.  D < 0 mirrors the axis; D == 0 leaves t < 2 - 2 |a| and no lower bound (-1 stands for it)
__device__ __forceinline__ void sight_axis(int a, int D, int& ln, int& ld, int& un, int& ud) {
    if (D < 0) { a = -a; D = -D; }
    const bool flat = D == 0;
    ln = flat ? -1 : 2 * a - 2;
    ld = flat ? 1 : 2 * D - 1;
    un = flat ? 2 - 2 * abs(a) : 2 * a + 2;
    ud = flat ? 1 : 2 * D + 1;
}

__device__ __forceinline__ bool sight_obstructs(int ax, int ay, int Dx, int Dy) {
    int lxn, lxd, uxn, uxd, lyn, lyd, uyn, uyd;
    sight_axis(ax, Dx, lxn, lxd, uxn, uxd);
    sight_axis(ay, Dy, lyn, lyd, uyn, uyd);
    return lxn * uxd < uxn * lxd && lxn * uyd < uyn * lxd && lyn * uxd < uxn * lyd && lyn * uyd < uyn * lyd &&
           lxn < lxd && lyn < lyd && uxn > 0 && uyn > 0;
}

// every lane of the wave calls this with the same cells; the result is the same in every lane
__device__ __forceinline__ bool sight_visible(const unsigned char* __restrict__ blocked, const unsigned char* __restrict__ goal,
                                              int gx, int gy, int cx, int cy, int qx, int qy, int lane) {
    const int Dx = qx - cx, Dy = qy - cy;
    const bool xmajor = abs(Dx) >= abs(Dy);
    const int DM = xmajor ? Dx : Dy, Dm = xmajor ? Dy : Dx;
    const int lo = min(0, DM) - 1, count = abs(DM) + 3, den = abs(DM), sgn = DM < 0 ? -1 : 1;
    bool hit = false;
    for (int k = lane; k < count; k += 64) {
        const int aM = lo + k;
        int f = 0;                                           // floor(aM Dm / DM)
        if (den) {
            const int num = aM * Dm * sgn;
            f = num / den;
            if (num % den < 0) --f;
        }
#pragma unroll
        for (int j = -1; j <= 2; ++j) {
            const int am = f + j;
            const int ax = xmajor ? aM : am, ay = xmajor ? am : aM;
            if (sight_blocked(blocked, goal, gx, gy, cx + ax, cy + ay) && sight_obstructs(ax, ay, Dx, Dy)) hit = true;
        }
    }
    return __ballot(hit) == 0ull;
}

// sqrtf of an integer below 2^24: one conversion (exact) and one correctly rounded root (common.hpp)
__device__ __forceinline__ float sight_dist(int cx, int cy, int qx, int qy) {
    const int dx = qx - cx, dy = qy - cy;
    return sqrtf((float)(dx * dx + dy * dy));
}

__global__ __launch_bounds__(kSightWaves * 64) void nav_sight_relax_kernel(const unsigned char* __restrict__ blocked,
                                                                          const unsigned char* __restrict__ goal_all,
                                                                          const float* __restrict__ w_in,
                                                                          const int* __restrict__ parent_in,
                                                                          float* __restrict__ w_out, int* __restrict__ parent_out,
                                                                          int* __restrict__ cache, int gx, int gy,
                                                                          int* __restrict__ changed) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int cells = gx * gy;
    const long long cl = (long long)blockIdx.x * kSightWaves + wave;
    if (cl >= cells) return;                                 // wave-uniform
    const int c = (int)cl, cx = c % gx, cy = c / gx;
    const int g = (int)blockIdx.y;
    const size_t po = (size_t)g * (size_t)cells;
    const unsigned char* __restrict__ goal = goal_all + po;
    const float* __restrict__ w = w_in + po;
    const int* __restrict__ parent = parent_in + po;
    const float wc = w[c];
    const int pc = parent[c];
    float best = wc;
    int bp = pc;
    if (!goal[c] && !blocked[c]) {                           // goal and blocked cells are copied through
        best = INFINITY;
        bp = -1;
        if (pc >= 0 && pc < cells) {
            best = __fadd_rn(w[pc], sight_dist(cx, cy, pc % gx, pc / gx));
            bp = pc;
        }
        // lanes 0 .. 7 take the neighbour slots E W N S NE NW SE SW side by side (every candidate reads state k only)
        const int s = lane & 7;
        const int dx = (s == 0 || s == 4 || s == 6) ? 1 : (s == 2 || s == 3) ? 0 : -1;
        const int dy = (s == 2 || s == 4 || s == 5) ? 1 : (s == 0 || s == 1) ? 0 : -1;
        const int nx = cx + dx, ny = cy + dy, n = ny * gx + nx;
        bool ok = lane < 8 && !sight_blocked(blocked, goal, gx, gy, nx, ny);
        if (ok && s >= 4)                                    // no corner is cut
            ok = !sight_blocked(blocked, goal, gx, gy, nx, cy) && !sight_blocked(blocked, goal, gx, gy, cx, ny);
        if (ok) ok = nav_finite(w[n]);
        int q = n;
        if (ok) {
            q = parent[n];
            if (q < 0 || q >= cells) q = n;
        }
        int* slot = cache + (po + (size_t)c) * 8 + s;
        const bool need = ok && q != n;
        const int e = need ? *slot : -1;
        const bool hit = need && e >= 0 && (e >> 1) == q;
        bool vis = hit && (e & 1) != 0;
        unsigned long long miss = __ballot(need && !hit);    // the slots whose parent moved: the whole wave walks each line
        while (miss) {                                       // wave-uniform
            const int j = __ffsll(miss) - 1;
            miss &= miss - 1;
            const int qj = __shfl(q, j);
            const bool v = sight_visible(blocked, goal, gx, gy, cx, cy, qj % gx, qj / gx, lane);
            if (lane == j) {
                vis = v;
                *slot = (q << 1) | (v ? 1 : 0);
            }
        }
        if (need && !vis) q = n;
        const float cand = ok ? __fadd_rn(w[q], sight_dist(cx, cy, q % gx, q / gx)) : INFINITY;
#pragma unroll
        for (int k = 0; k < 8; ++k) {                        // in slot order; a later one wins only when strictly better
            const float ck = __shfl(cand, k);
            const int qk = __shfl(q, k);
            if (ck < best) { best = ck; bp = qk; }
        }
    }
    if (lane == 0) {
        w_out[po + c] = best;
        parent_out[po + c] = bp;
        if (__float_as_uint(best) != __float_as_uint(wc) || bp != pc) changed[g] = 1;   // a plain store; every writer stores 1
    }
}

__global__ __launch_bounds__(kNavWaves * 64) void nav_direction_sight_kernel(const float2* __restrict__ position,
                                                                            const int* __restrict__ gate,
                                                                            const float2* __restrict__ destination,
                                                                            long long rows, const piml_nav_grid N,
                                                                            const int* __restrict__ parent,
                                                                            float2* __restrict__ direction,
                                                                            int* __restrict__ branch, int* __restrict__ neighbour) {
    const long long i = (long long)blockIdx.x * kNavWaves + (threadIdx.x >> 6);
    if (i >= rows) return;                                   // wave-uniform
    const float2 p = position[i], t = destination[i];
    const NavDir d = nav_direction<true>(N, gate[i], p, t, parent);
    if ((threadIdx.x & 63) == 0) {
        direction[i] = d.e;
        if (branch) branch[i] = d.branch;
        if (neighbour) neighbour[i] = d.neighbour;
    }
}

}  // namespace piml

PIML_API int piml_nav_sight_relax(const unsigned char* blocked, const unsigned char* goal, float* w_a, int* parent_a, float* w_b,
                                  int* parent_b, int* cache, int G, int gx, int gy, int launches, int* changed, void* stream) {
    if (!blocked || !goal || !w_a || !parent_a || !w_b || !parent_b || !cache || w_a == w_b || parent_a == parent_b ||
        !changed || !piml::nav_dims_ok(G, gx, gy) || launches < 0)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)((gx * gy + piml::kSightWaves - 1) / piml::kSightWaves), (unsigned)G);
    for (int j = 0; j < launches; ++j) {
        hipLaunchKernelGGL(piml::nav_sight_relax_kernel, grid, dim3(piml::kSightWaves * 64), 0, piml::as_stream(stream), blocked,
                           goal, (const float*)(j & 1 ? w_b : w_a), (const int*)(j & 1 ? parent_b : parent_a), j & 1 ? w_a : w_b,
                           j & 1 ? parent_a : parent_b, cache, gx, gy, changed);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

PIML_API int piml_nav_direction_sight(const float* position, const int* gate, const float* destination, long long rows,
                                      const piml_nav_grid* g, const piml_nav_sight* sight, float* direction, int* branch,
                                      int* neighbour, void* stream) {
    if (rows < 0 || !direction || !piml::nav_grid_ok(g) || !piml::nav_sight_ok(sight, g)) return hipErrorInvalidValue;
    if (rows == 0) return hipSuccess;
    if (!position || !gate || !destination) return hipErrorInvalidValue;
    const long long blocks = (rows + piml::kNavWaves - 1) / piml::kNavWaves;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(piml::nav_direction_sight_kernel, dim3((unsigned)blocks), dim3(piml::kNavWaves * 64), 0,
                       piml::as_stream(stream), (const float2*)position, gate, (const float2*)destination, rows, *g, sight->parent,
                       (float2*)direction, branch, neighbour);
    return hipGetLastError();
}
