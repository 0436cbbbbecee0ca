// The fluctuation term of the MLAPM scenario frame (piml_scenario_step_mlapm_noise) and of its stand-alone operator
// (piml_noise_force): the fluctuation of Helbing and Molnar 1995 as an Ornstein-Uhlenbeck acceleration eta per agent,
//   eta' = rho eta + amp z,   rho = exp(-dt / noise_tau) (0: white noise),   amp = An sqrt(1 - rho^2),
// z two independent standard normals per (seed, frame, slot).  The host forms (rho, amp) once in float64 and rounds them to
// float32 (ops_scenario.noise_law); the device sees only the two floats, so everything but z is float32 arithmetic with
// every operation rounded on its own (the library is built without contraction) and restated bit for bit in numpy.
//
// The draws: Philox4x32-10 (philox.hpp), key = (seed lo, seed hi), counter = (t lo, t hi, slot, 0x5CE40001), t the frame
// stepped FROM.  z_x comes from the words (w0, w1), z_y from (w2, w3), each as GC's speed draw (scenario.hip, call 3):
//   u1 = ((wa >> 8) + 1) 2^-24,  u2 = (wb >> 8) 2^-24,  z = (float)(sqrt(-2 ln u1) cos(2 pi u2))  in double.
// |z| <= sqrt(48 ln 2) = 5.77.  The draws depend on (seed, frame, slot) only, never on the dynamics.
#pragma once
#include "common.hpp"
#include "philox.hpp"
#include "../../include/piml_hip.h"

#include <cmath>

namespace piml {

constexpr unsigned kNoiseStream = 0x5CE40000u;

__device__ __forceinline__ float noise_normal(unsigned wa, unsigned wb) {
    const double u1 = (double)((wa >> 8) + 1u) * 5.9604644775390625e-8, u2 = (double)(wb >> 8) * 5.9604644775390625e-8;
    return (float)(sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2));
}

// the two normals of slot `slot` for the step from frame t
__device__ __forceinline__ float2 noise_draw(unsigned long long seed, long long t, unsigned slot) {
    const PhiloxOut w = philox4x32_10((unsigned)t, (unsigned)((unsigned long long)t >> 32), slot, kNoiseStream | 1u,
                                      (unsigned)seed, (unsigned)(seed >> 32));
    return make_float2(noise_normal(w.x, w.y), noise_normal(w.z, w.w));
}

__device__ __forceinline__ float2 noise_step(float2 eta, float rho, float amp, float2 z) {
    return make_float2(__fadd_rn(__fmul_rn(rho, eta.x), __fmul_rn(amp, z.x)), __fadd_rn(__fmul_rn(rho, eta.y), __fmul_rn(amp, z.y)));
}

// ---- host: the checks of both entries (include/piml_hip.h) ----

static inline bool noise_law_ok(float rho, float amp) {
    return std::isfinite(rho) && std::isfinite(amp) && rho >= 0.f && rho < 1.f && amp >= 0.f;
}

}  // namespace piml
