// piml_group_force: the group term of groups.hpp as a stand-alone operator -- one thread per row of `position`, any number
// of rows.  The MLAPM scenario frame (scenario.hip) calls the same function on frame t's records, so force[i] is bitwise
// what the frame adds for slot i of a frame whose recorded positions are `position`.
#include "groups.hpp"

namespace piml {

__global__ __launch_bounds__(256) void group_force_kernel(const float2* __restrict__ position, const int* __restrict__ group_first,
                                                          const int* __restrict__ group_size, long long rows, float A,
                                                          float dist, float2* __restrict__ force) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    force[i] = group_force_row(position, rows, i, group_first[i], group_size[i], A, dist);
}

}  // namespace piml

PIML_API int piml_group_force(const float* position, const int* group_first, const int* group_size, long long rows, float A,
                              float dist, float* force, void* stream) {
    if (rows < 0 || !piml::group_law_ok(A, dist)) return hipErrorInvalidValue;
    if (rows == 0) return hipSuccess;
    if (!position || !group_first || !group_size || !force) return hipErrorInvalidValue;
    const long long blocks = (rows + 255) / 256;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(piml::group_force_kernel, dim3((unsigned)blocks), dim3(256), 0, piml::as_stream(stream),
                       (const float2*)position, group_first, group_size, rows, A, dist, (float2*)force);
    return hipGetLastError();
}
