// The group cohesion term of the MLAPM scenario frame (piml_scenario_step_mlapm_groups) and of its stand-alone operator
// (piml_group_force): the attraction term of Moussaid et al. 2010, a constant pull towards the centroid of the agent's
// group once the agent is further from it than dist (n - 1) metres.
//
//   mates of row i: the rows j in [group_first[i], group_first[i] + group_size[i]) clamped to [0, rows), i among them; a
//   mate is present when position[j] is not NaN.  n = the present mates; n < 2 or position[i] NaN: G = 0.  Otherwise, every
//   operation a float32 one rounded on its own (no contraction):
//     c = (sum of p_j over the present mates in ascending j, from 0) / (float)n,  e = c - p_i,
//     d = sqrt(ex ex + ey ey),  thr = dist (float)(n - 1),  G = d > thr ? ((A ex) / d, (A ey) / d) : 0.
//
// The range is clamped before any read: whatever group_first / group_size hold, nothing outside `position` is read.  The
// function is scalar -- at most four mates for a scene of scenarios.clip_scenario -- and gives the same value in every
// lane that calls it with the same arguments, so the frame's waves call it as it stands.
#pragma once
#include "common.hpp"
#include "../../include/piml_hip.h"

#include <cmath>

namespace piml {

constexpr int kGroupMaxSize = 4;                 // members per arrival unit (scenarios.CLIP_MAX_GROUP)
constexpr unsigned kGroupMaxUnits = 1u << 24;    // arrival units the 24-bit unit draw reaches

__device__ __forceinline__ float2 group_force_row(const float2* __restrict__ position, long long rows, long long i, int first,
                                                  int size, float A, float dist) {
    const float2 zero = make_float2(0.f, 0.f);
    const float2 pi = position[i];
    if (pi.x != pi.x || pi.y != pi.y) return zero;
    const long long lo = first > 0 ? (long long)first : 0;
    long long hi = (long long)first + (long long)size;
    hi = hi < rows ? hi : rows;
    float sx = 0.f, sy = 0.f;
    int n = 0;
    for (long long j = lo; j < hi; ++j) {
        const float2 p = position[j];
        if (p.x != p.x || p.y != p.y) continue;
        sx = __fadd_rn(sx, p.x);
        sy = __fadd_rn(sy, p.y);
        ++n;
    }
    if (n < 2) return zero;
    const float fn = (float)n;
    const float ex = __fsub_rn(__fdiv_rn(sx, fn), pi.x), ey = __fsub_rn(__fdiv_rn(sy, fn), pi.y);
    const float d = sqrtf(__fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey)));   // (correctly rounded: common.hpp)
    const float thr = __fmul_rn(dist, (float)(n - 1));
    if (!(d > thr)) return zero;
    return make_float2(__fdiv_rn(__fmul_rn(A, ex), d), __fdiv_rn(__fmul_rn(A, ey), d));
}

// ---- host: the checks of both entries (include/piml_hip.h) ----

static inline bool group_law_ok(float A, float dist) {
    return std::isfinite(A) && std::isfinite(dist) && A >= 0.f && dist >= 0.f;
}

}  // namespace piml
