// piml_noise_force: the fluctuation term of noise.hpp as a stand-alone operator -- one thread per row of (members, N),
// row m N + i being slot i of the member whose key is seeds[m].  The MLAPM scenario frame (scenario.hip) calls the same two
// functions for its live slots, so eta_out is bitwise the state the frame leaves, and what it adds to the force, for the
// step from frame `frame`.  A row with present == 0 draws nothing: its eta is copied and its z is 0.  In place is allowed:
// a thread reads and writes its own row only.
#include "noise.hpp"

namespace piml {

__global__ __launch_bounds__(256) void noise_force_kernel(float2* eta_out, float2* z_out, const float2* eta_in,
                                                          const unsigned char* __restrict__ present,
                                                          const unsigned long long* __restrict__ seeds, long long rows, int N,
                                                          long long frame, float rho, float amp) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    float2 eta = eta_in[r], z = make_float2(0.f, 0.f);
    if (!present || present[r]) {
        z = noise_draw(seeds[r / N], frame, (unsigned)(r % N));
        eta = noise_step(eta, rho, amp, z);
    }
    eta_out[r] = eta;
    if (z_out) z_out[r] = z;
}

}  // namespace piml

PIML_API int piml_noise_force(float* eta_out, float* z_out, const float* eta_in, const unsigned char* present,
                              const uint64_t* seeds, int members, int N, long long frame, float rho, float amp, void* stream) {
    if (members < 0 || N < 0 || frame < 0 || !piml::noise_law_ok(rho, amp)) return hipErrorInvalidValue;
    const long long rows = (long long)members * (long long)N;
    if (rows == 0) return hipSuccess;
    if (!eta_out || !eta_in || !seeds) return hipErrorInvalidValue;
    const long long blocks = (rows + 255) / 256;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(piml::noise_force_kernel, dim3((unsigned)blocks), dim3(256), 0, piml::as_stream(stream), (float2*)eta_out,
                       (float2*)z_out, (const float2*)eta_in, present, (const unsigned long long*)seeds, rows, N, frame, rho, amp);
    return hipGetLastError();
}
