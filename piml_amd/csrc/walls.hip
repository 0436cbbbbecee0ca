// piml_wall_force: the wall term of walls.hpp as a stand-alone operator -- one wave per row of `position`, any number of
// rows (every slot of every frame of an ensemble, for instance).  The MLAPM scenario frame (scenario.hip) runs the same
// wave function on the same grid, so force[i] is bitwise what the frame adds for an agent at position[i].
#include "walls.hpp"

namespace piml {

__global__ __launch_bounds__(kWallWaves * 64) void wall_force_kernel(const float2* __restrict__ position, long long rows,
                                                                    const WallArgs W, float A, float B,
                                                                    float2* __restrict__ force, float* __restrict__ dist2,
                                                                    int* __restrict__ index) {
    const long long i = (long long)blockIdx.x * kWallWaves + (threadIdx.x >> 6);
    if (i >= rows) return;                                   // wave-uniform
    const int lane = threadIdx.x & 63;
    const float2 p = position[i];
    const WallHit h = wall_force_wave(W, A, B, make_float2(uniform(p.x), uniform(p.y)), lane);
    if (lane == 0) {
        force[i] = h.force;
        if (dist2) dist2[i] = h.d2;
        if (index) index[i] = h.index;
    }
}

}  // namespace piml

PIML_API int piml_wall_force(const float* position, long long rows, const piml_wall_grid* g, float A, float B, float* force,
                             float* dist2, int* index, void* stream) {
    if (rows < 0 || !force || !piml::wall_grid_ok(g) || !piml::wall_law_ok(A, B)) return hipErrorInvalidValue;
    if (rows == 0 || g->n_points == 0) return hipSuccess;    // nothing to launch (the caller fills the empty outputs)
    if (!position) return hipErrorInvalidValue;
    const long long blocks = (rows + piml::kWallWaves - 1) / piml::kWallWaves;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(piml::wall_force_kernel, dim3((unsigned)blocks), dim3(piml::kWallWaves * 64), 0, piml::as_stream(stream),
                       (const float2*)position, rows, piml::wall_args(*g), A, B, (float2*)force, dist2, index);
    return hipGetLastError();
}
