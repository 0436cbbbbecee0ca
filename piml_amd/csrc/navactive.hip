// The weighted floor-field solve by active tiles (piml_nav_relax_active, include/piml_hip.h): the Jacobi sequence of
// piml_nav_relax_cost / piml_nav_relax_cost_gates bit for bit, with the tiles skipped whose step provably reproduces what the
// buffer it would write already holds, and with no word the host has to read between launches, so the whole solve is
// capturable.
//
// Why a skipped tile is exact.  S_n is the field after n launches; launch n reads buffer A (S_n) and writes B (S_n+1),
// launch n + 1 reads B and writes A.  A launch computes a tile's 32 x 32 outputs from the tile and a halo of kNdK = 8 <= 32
// cells: the tile and its eight neighbour tiles in the buffer it reads.  If no tile of T's 3 x 3 neighbourhood changed during
// launch n, then S_n+2(T) = S_n+1(T) = S_n(T), which A holds at T already: launch n + 1 may leave T alone.  By induction the
// written buffer always holds the whole next iterate, and when no tile changed in a launch both buffers are equal and hold
// the fixed point.  Launch 0 steps every tile, so only the buffer it reads (u_a) needs the cold start; u_b, the flags and
// work may hold anything.
//
// flags: two int32 planes of planes * ty * tx words; launch j writes plane j & 1 -- every block its own word, stepped or
// not -- and reads the other.  A block reads the nine words of its neighbourhood (those outside the tile grid count 0) as
// addresses every lane shares; none set: it writes its word 0 and returns before staging anything.  Otherwise the step is
// nav_relax_cost_kernel's statement for statement (navdensity.hip: K = 8 steps on a tile staged with a halo of 8, two
// ping-pong LDS planes and the cost tile in a third, 29952 bytes), the bitwise difference against the input is OR-ed across
// the block, and that is the block's word.  work[plane] counts the stepped blocks (an integer atomic: the sum is
// deterministic); in the last launch a block whose tile changed stores 1 to *stalled (a plain store; every writer stores the
// same value), which says the launches were too few.  The kernels of navdensity.hip and navflow.hip are untouched.
#include "navcost.hpp"                                      // the tile constants and nav_update_cost

namespace piml {

// grid (tiles x, tiles y, member * G + gate): blocked and goal are the scene's; u, the flags and work the plane's; cost the
// member's (per_gate == 0) or the plane's
__global__ __launch_bounds__(kNdThreads) void nav_relax_active_kernel(const unsigned char* __restrict__ blocked,
                                                                     const unsigned char* __restrict__ goal,
                                                                     const float* __restrict__ cost, int per_gate,
                                                                     const float* __restrict__ u_in, float* __restrict__ u_out,
                                                                     int G, int gx, int gy, const int* __restrict__ flag_in,
                                                                     int* __restrict__ flag_out, int first, int last,
                                                                     int* __restrict__ work, int* __restrict__ stalled) {
    __shared__ float plane[2][kNdCells];
    __shared__ float slow[kNdCells];
    __shared__ unsigned char fixed[kNdCells];
    const int z = (int)blockIdx.z;
    const int bx = (int)blockIdx.x, by = (int)blockIdx.y, tx = (int)gridDim.x, ty = (int)gridDim.y;
    const size_t fo = (size_t)z * (size_t)(ty * tx);        // the plane's flags
    if (!first) {
        int any = 0;
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const int nx = bx + dx, ny = by + dy;
                if (nx >= 0 && nx < tx && ny >= 0 && ny < ty) any |= flag_in[fo + (size_t)(ny * tx + nx)];
            }
        if (!any) {                                          // the same in every lane: the whole block leaves
            if (threadIdx.x == 0) flag_out[fo + (size_t)(by * tx + bx)] = 0;
            return;
        }
    }
    const int X0 = bx * kNdTile - kNdK, Y0 = by * kNdTile - kNdK;
    const size_t cells = (size_t)gy * (size_t)gx;
    const size_t po = (size_t)z * cells, go = (size_t)(z % G) * cells, co = per_gate ? po : (size_t)(z / G) * cells;
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
    int diff = 0;
    for (int q = threadIdx.x; q < kNdTile * kNdTile; q += kNdThreads) {
        const int lx = q % kNdTile, ly = q / kNdTile;
        const int x = X0 + kNdK + lx, y = Y0 + kNdK + ly;
        if (x >= gx || y >= gy) continue;
        const size_t c = po + (size_t)y * (size_t)gx + (size_t)x;
        const float v = plane[0][(ly + kNdK) * kNdSide + lx + kNdK];
        u_out[c] = v;
        diff |= __float_as_uint(v) != __float_as_uint(u_in[c]);
    }
    diff = __syncthreads_or(diff);
    if (threadIdx.x == 0) {
        flag_out[fo + (size_t)(by * tx + bx)] = diff ? 1 : 0;
        if (work) atomicAdd(work + z, 1);
        if (last && diff) *stalled = 1;                      // a plain store; every writer stores the same value
    }
}

}  // namespace piml

PIML_API int piml_nav_relax_active(const unsigned char* blocked, const unsigned char* goal, const float* cost, int cost_per_gate,
                                   float* u_a, float* u_b, int members, int G, int gx, int gy, int launches, int* flags,
                                   int* work, int* stalled, void* stream) {
    if (!blocked || !goal || !cost || !u_a || !u_b || u_a == u_b || !flags || !stalled || launches < 2 || (launches & 1) ||
        (cost_per_gate != 0 && cost_per_gate != 1) || !piml::nd_planes_ok(members, G, gx, gy))
        return hipErrorInvalidValue;
    const int tx = (gx + piml::kNdTile - 1) / piml::kNdTile, ty = (gy + piml::kNdTile - 1) / piml::kNdTile;
    const dim3 grid((unsigned)tx, (unsigned)ty, (unsigned)(members * G));
    const size_t words = (size_t)(members * G) * (size_t)(ty * tx);     // one plane of flags
    for (int j = 0; j < launches; ++j) {
        int* out = flags + (size_t)(j & 1) * words;
        const int* in = flags + (size_t)((j + 1) & 1) * words;
        hipLaunchKernelGGL(piml::nav_relax_active_kernel, grid, dim3(piml::kNdThreads), 0, piml::as_stream(stream), blocked, goal,
                           cost, cost_per_gate, (const float*)(j & 1 ? u_b : u_a), j & 1 ? u_a : u_b, G, gx, gy, in, out,
                           j == 0 ? 1 : 0, j == launches - 1 ? 1 : 0, work, stalled);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
