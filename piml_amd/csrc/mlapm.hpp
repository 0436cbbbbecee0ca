// Pair arithmetic shared by the MLAPM kernels (pairwise.hip: step / rollout / state gradient; mlapm_fit.hip: loss and
// parameter gradient for calibration).
#pragma once
#include "common.hpp"

namespace piml {

// MLAPM is a smooth force law checked to 1e-5 relative (not a discrete selection like relfeat), so
// its pair arithmetic uses the hardware reciprocal-sqrt / reciprocal / exp2 units (<= 1 ulp
// each) instead of the multi-instruction IEEE division / sqrt / expf expansions.
__device__ __forceinline__ float fast_rsq(float x) { return __builtin_amdgcn_rsqf(x); }
__device__ __forceinline__ float fast_rcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// UCY collision flag (mlapm.py:43-47) with EXACTLY the reference's float32 operations -- it is a discrete decision,
// so the fast reciprocal / squared-domain shortcuts of the smooth terms do not apply here:
//   |vr| < 2R  or  |vr + vv| < 2R  or  (0 < tmin < 1 and dmin < 2R),
//   tmin = -(vr.vv) / (vv.vv),  dmin = sqrt(vr.vr - (vr.vv)^2 / (vv.vv)),  dots = x*x' + y*y' (two products, one add),
//   norms = torch.norm on 2-vectors = sqrt(fma(y, y, x*x)).  A NaN dmin (negative argument) compares false.
__device__ __forceinline__ bool ucy_collision(float rx, float ry, float wx, float wy, float two_r) {
    bool coll = norm2(rx, ry) < two_r;
    coll |= norm2(__fadd_rn(rx, wx), __fadd_rn(ry, wy)) < two_r;
    const float rw = __fadd_rn(__fmul_rn(rx, wx), __fmul_rn(ry, wy));
    const float ww = __fadd_rn(__fmul_rn(wx, wx), __fmul_rn(wy, wy));
    const float rr = __fadd_rn(__fmul_rn(rx, rx), __fmul_rn(ry, ry));
    const float tmin = __fdiv_rn(-rw, ww);
    const float dmin = sqrtf(__fsub_rn(rr, __fdiv_rn(__fmul_rn(rw, rw), ww)));
    coll |= (tmin > 0.f) && (tmin < 1.f) && (dmin < two_r);
    return coll;
}

}  // namespace piml
