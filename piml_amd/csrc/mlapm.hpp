// Pair arithmetic shared by the MLAPM kernels (pairwise.hip: step / rollout / state gradient; mlapm_fit.hip: loss and
// parameter gradient for calibration; mlapm_rollout_fit.hip: the same over multi-frame rollouts; scenario.hip: the MLAPM
// scenario frame).
#pragma once
#include "common.hpp"

#include <cmath>
#include <cstdlib>

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


constexpr int kMlTile = 2048;   // agents per LDS tile (fwd 32 KiB, bwd 64 KiB)

struct MlapmParams {
    int variant;                 // 0 raw, 1 GC, 2 UCY (mlapm.py:28-53)
    float tau, A, B, Cc, D, cth, sth, r2;   // cos/sin of theta, 2*radius
    float B2, C2, D2;            // B, C, D pre-multiplied by log2(e): exp(x) = exp2(x * log2 e)
    int skip_absent;             // 1: sources with a NaN position contribute nothing (absent agents)
    int ucy_two_phase;           // backward, UCY: the two-phase form (PIML_MLAPM_UCY_TWO_PHASE=0 keeps the scalar loop)
};

// One ordered pair: focal (vix, viy, ex, ey) at the origin, source at (rx, ry) with
// relative velocity (wx, wy).  Returns view * A * g * direction (mlapm.py:25-53).
__device__ __forceinline__ float2 mlapm_pair(const MlapmParams& P, float rx, float ry, float wx, float wy,
                                             float vix, float viy, float ex, float ey) {
    const float d2 = rx * rx + ry * ry;
    const bool pos = d2 > 0.f;                                      // NaN -> false, handled below
    const float rinv = fast_rsq(d2);
    const float r = pos ? d2 * rinv : d2;                           // :26 (0 stays 0, NaN stays NaN)
    const float view = (vix * rx + viy * ry > 0.f) ? 1.f : 0.f;     // :27
    const float ninv = pos ? rinv : 0.f;                            // F.normalize: 0 / eps = 0
    const float nx = rx * ninv, ny = ry * ninv;
    float g, dx, dy;
    if (P.variant == 0) {
        g = fast_exp2(P.B2 * r);                                    // :29
        dx = nx; dy = ny;
    } else {
        const float cr = rx * ey - ry * ex;                         // :34 / :48
        // theta = -sign(cr) * theta, 0 -> +theta; sign(NaN) = NaN propagates like the reference
        const float st = cr > 0.f ? -P.sth : (cr <= 0.f ? P.sth : cr);
        dx = P.cth * nx - st * ny; dy = st * nx + P.cth * ny;       // :36-39
        if (P.variant == 1) {
            const float w2 = wx * wx + wy * wy;
            // cosine_similarity clamps both norms at 1e-8 (:32)
            const float cs = (rx * wx + ry * wy) * fminf(rinv, 1e8f) * fminf(fast_rsq(w2), 1e8f);
            g = fast_exp2(P.B2 * r + P.C2 * cs + P.D2 * r * cs);    // :40
        } else {
            const bool coll = ucy_collision(rx, ry, wx, wy, P.r2);      // :43-47, exact
            g = coll ? fast_exp2(P.B2 * r + P.C2) : 1.f;            // :53 (with coll.unsqueeze(-1), Q8)
            if (r != r) g = r;                                      // NaN poisons like the reference
        }
    }
    const float s = view * P.A * g;
    return make_float2(s * dx, s * dy);
}

// Two ordered pairs per lane with packed fp32 (v_pk_mul / v_pk_add / v_pk_fma_f32): the raw and GC force laws
// (variants 0, 1).  Same expressions as mlapm_pair, element-wise on 2-vectors; products feeding sums are fused
// (fma), which the 1e-5 relative bar of this smooth force law allows (the selections are unaffected).
// (The variant stays a run-time value on purpose: a kernel specialised per variant at compile time measured
// slower -- GC forward 38.7 us against 26.1 us at N = 4096; round 4, again, on the rollout frame: 47.5 against 34.1 us.)
typedef float v2f __attribute__((ext_vector_type(2)));

__device__ __forceinline__ v2f pk_fma(v2f a, v2f b, v2f c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ v2f pk_sel(bool c0, bool c1, v2f a, v2f b) { return v2f{c0 ? a.x : b.x, c1 ? a.y : b.y}; }

__device__ __forceinline__ void mlapm_pair2(const MlapmParams& P, v2f rx, v2f ry, v2f wx, v2f wy, float vix, float viy,
                                            float ex, float ey, v2f& fx, v2f& fy) {
    const v2f zero = {0.f, 0.f}, one = {1.f, 1.f};
    const v2f d2 = pk_fma(ry, ry, rx * rx);
    const bool p0 = d2.x > 0.f, p1 = d2.y > 0.f;                                  // NaN -> false
    const v2f rinv = {fast_rsq(d2.x), fast_rsq(d2.y)};
    const v2f r = pk_sel(p0, p1, d2 * rinv, d2);                                  // :26
    const v2f dot = pk_fma(v2f{viy, viy}, ry, v2f{vix, vix} * rx);
    const v2f view = pk_sel(dot.x > 0.f, dot.y > 0.f, one, zero);                 // :27
    const v2f ninv = pk_sel(p0, p1, rinv, zero);
    const v2f nx = rx * ninv, ny = ry * ninv;
    v2f g, dx, dy;
    if (P.variant == 0) {
        const v2f a = v2f{P.B2, P.B2} * r;
        g = v2f{fast_exp2(a.x), fast_exp2(a.y)};                                  // :29
        dx = nx; dy = ny;
    } else {
        const v2f cr = pk_fma(rx, v2f{ey, ey}, -(ry * v2f{ex, ex}));              // :34
        const v2f st = {cr.x > 0.f ? -P.sth : (cr.x <= 0.f ? P.sth : cr.x),
                        cr.y > 0.f ? -P.sth : (cr.y <= 0.f ? P.sth : cr.y)};
        const v2f cth = {P.cth, P.cth};
        dx = pk_fma(cth, nx, -(st * ny));                                         // :36-39
        dy = pk_fma(st, nx, cth * ny);
        const v2f w2 = pk_fma(wy, wy, wx * wx);
        const v2f ri8 = {fminf(rinv.x, 1e8f), fminf(rinv.y, 1e8f)};
        const v2f qi8 = {fminf(fast_rsq(w2.x), 1e8f), fminf(fast_rsq(w2.y), 1e8f)};
        const v2f cs = pk_fma(ry, wy, rx * wx) * ri8 * qi8;                       // :32
        const v2f a = pk_fma(v2f{P.D2, P.D2} * r, cs, pk_fma(v2f{P.C2, P.C2}, cs, v2f{P.B2, P.B2} * r));
        g = v2f{fast_exp2(a.x), fast_exp2(a.y)};                                  // :40
    }
    const v2f sc = view * v2f{P.A, P.A} * g;
    fx = sc * dx;
    fy = sc * dy;
}

// UCY (variant 2) in two phases (round 4).  g = exp(B r + C) only for pairs the collision predicate flags, 1 otherwise
// (mlapm.py:43-53), and the predicate -- three square roots and two divisions in the reference's exact float32 operations --
// cost more than the rest of the pair.  Phase 1 gives every pair its g = 1 term on packed arithmetic and a CONSERVATIVE
// distance test: every clause of the predicate implies that the relative position comes within 2R of the origin for some
// t in [0, 1] of r + t w, hence |r| - |w| < 2R; a pair with (|r| - |w|)^2 - (2R)^2 > 1e-6 (|r|^2 + 1) (the slack covers the
// roundings of both sides, 1e-7 relative, with a factor of ten) cannot be flagged.  The others -- ~4 % of the pairs of a
// 4096-agent hall -- are compacted into a per-wave ring and get the exact predicate 64 at a time; a flagged pair adds the
// difference (g - 1) x its g = 1 term.  Same sums up to the order of the additions.
__device__ __forceinline__ void mlapm_pair2_ucy(const MlapmParams& P, v2f rx, v2f ry, v2f wx, v2f wy, float vix, float viy,
                                                float ex, float ey, v2f& fx, v2f& fy, bool& near0, bool& near1) {
    const v2f zero = {0.f, 0.f}, one = {1.f, 1.f};
    const v2f d2 = pk_fma(ry, ry, rx * rx);
    const bool p0 = d2.x > 0.f, p1 = d2.y > 0.f;                                  // NaN -> false
    const v2f rinv = {fast_rsq(d2.x), fast_rsq(d2.y)};
    const v2f r = pk_sel(p0, p1, d2 * rinv, d2);
    const v2f dot = pk_fma(v2f{viy, viy}, ry, v2f{vix, vix} * rx);
    const v2f view = pk_sel(dot.x > 0.f, dot.y > 0.f, one, zero);                 // :27
    const v2f ninv = pk_sel(p0, p1, rinv, zero);
    const v2f nx = rx * ninv, ny = ry * ninv;
    const v2f cr = pk_fma(rx, v2f{ey, ey}, -(ry * v2f{ex, ex}));                  // :48
    const v2f st = {cr.x > 0.f ? -P.sth : (cr.x <= 0.f ? P.sth : cr.x),
                    cr.y > 0.f ? -P.sth : (cr.y <= 0.f ? P.sth : cr.y)};
    const v2f cth = {P.cth, P.cth};
    const v2f sc = view * v2f{P.A, P.A};                                          // g = 1
    fx = sc * pk_fma(cth, nx, -(st * ny));
    fy = sc * pk_fma(st, nx, cth * ny);
    // conservative test: far = certainly not flagged
    const v2f w2 = pk_fma(wy, wy, wx * wx);
    const v2f wn = w2 * v2f{fast_rsq(fmaxf(w2.x, 1e-30f)), fast_rsq(fmaxf(w2.y, 1e-30f))};
    const v2f a = r - wn;
    const v2f slack = pk_fma(v2f{1e-6f, 1e-6f}, d2, v2f{1e-6f + P.r2 * P.r2, 1e-6f + P.r2 * P.r2});
    near0 = !(a.x > 0.f && a.x * a.x > slack.x);                                  // (NaN: near)
    near1 = !(a.y > 0.f && a.y * a.y > slack.y);
}

// exact second phase of one candidate: the difference between its flagged term and the g = 1 term phase 1 added
__device__ __forceinline__ float2 mlapm_ucy_correction(const MlapmParams& P, float rx, float ry, float wx, float wy,
                                                       float vix, float viy, float ex, float ey) {
    if (!ucy_collision(rx, ry, wx, wy, P.r2)) return make_float2(0.f, 0.f);       // :43-47, exact
    const float d2 = rx * rx + ry * ry;
    const bool pos = d2 > 0.f;
    const float rinv = fast_rsq(d2);
    const float r = pos ? d2 * rinv : d2;
    const float view = (vix * rx + viy * ry > 0.f) ? 1.f : 0.f;
    const float ninv = pos ? rinv : 0.f;
    const float nx = rx * ninv, ny = ry * ninv;
    const float cr = rx * ey - ry * ex;
    const float st = cr > 0.f ? -P.sth : (cr <= 0.f ? P.sth : cr);
    const float s = view * P.A * (fast_exp2(P.B2 * r + P.C2) - 1.f);              // :53 minus the g = 1 term
    return make_float2(s * (P.cth * nx - st * ny), s * (st * nx + P.cth * ny));
}

// The sources of one LDS tile (tile[0 .. tn), (px, py, vx, vy); absent ones NaN) against the focal agent (pi, vi) with
// desired direction (ex, ey), one wave: lane-strided pair terms into the lane's scalar (sx, sy) and packed (acc2x, acc2y)
// partial sums (the caller adds them, sx + acc2.x + acc2.y, and takes the wave sum).  `ring` is the wave's 256-entry UCY
// candidate ring.  mlapm_fwd_kernel (pairwise.hip) and the MLAPM scenario frame (scenario.hip) share it, so a frame of
// either adds the same terms in the same order.
__device__ __forceinline__ void mlapm_tile_sum(const MlapmParams& P, const float4* tile, int tn, int lane, unsigned short* ring,
                                               float2 pi, float2 vi, float ex, float ey, float& sx, float& sy,
                                               v2f& acc2x, v2f& acc2y) {
    int j = lane;
    if (P.variant != 2) {
        // two sources per lane and iteration (j, j + 64), packed arithmetic
        const v2f pix = {pi.x, pi.x}, piy = {pi.y, pi.y}, vix2 = {vi.x, vi.x}, viy2 = {vi.y, vi.y};
        for (; j + 64 < tn; j += 128) {
            const float4 a = tile[j], b = tile[j + 64];
            v2f fx, fy;
            mlapm_pair2(P, v2f{a.x, b.x} - pix, v2f{a.y, b.y} - piy, v2f{a.z, b.z} - vix2, v2f{a.w, b.w} - viy2,
                        vi.x, vi.y, ex, ey, fx, fy);
            if (P.skip_absent) {                                        // absent sources contribute nothing
                if (a.x != a.x || a.y != a.y) { fx.x = 0.f; fy.x = 0.f; }
                if (b.x != b.x || b.y != b.y) { fx.y = 0.f; fy.y = 0.f; }
            }
            acc2x += fx; acc2y += fy;
        }
    }
    if (P.variant == 2) {
        // phase 1 on two sources per lane (j, j + 64; the second clamped and masked at the tile's end), candidates into
        // the ring; phase 2 whenever 64 are waiting, and for what is left at the end of the tile
        const v2f pix = {pi.x, pi.x}, piy = {pi.y, pi.y}, vix2 = {vi.x, vi.x}, viy2 = {vi.y, vi.y};
        unsigned head = 0, tail = 0;
        for (int j0 = 0;; j0 += 128) {
            const bool more = j0 < tn;
            if (more) {
                const int ja = j0 + lane, jb = j0 + 64 + lane;
                const bool va = ja < tn, vb = jb < tn;
                const float4 a = tile[va ? ja : 0], b = tile[vb ? jb : 0];
                v2f fx, fy;
                bool na, nb;
                mlapm_pair2_ucy(P, v2f{a.x, b.x} - pix, v2f{a.y, b.y} - piy, v2f{a.z, b.z} - vix2, v2f{a.w, b.w} - viy2,
                                vi.x, vi.y, ex, ey, fx, fy, na, nb);
                const bool absent_a = P.skip_absent && (a.x != a.x || a.y != a.y);
                const bool absent_b = P.skip_absent && (b.x != b.x || b.y != b.y);
                if (!va || absent_a) { fx.x = 0.f; fy.x = 0.f; na = false; }
                if (!vb || absent_b) { fx.y = 0.f; fy.y = 0.f; nb = false; }
                acc2x += fx; acc2y += fy;
                const u64 ma = __builtin_amdgcn_ballot_w64(na);
                if (ma) {
                    if (na) ring[(tail + mbcnt(ma)) & 255] = (unsigned short)ja;
                    tail += (unsigned)__builtin_popcountll(ma);
                }
                const u64 mb = __builtin_amdgcn_ballot_w64(nb);
                if (mb) {
                    if (nb) ring[(tail + mbcnt(mb)) & 255] = (unsigned short)jb;
                    tail += (unsigned)__builtin_popcountll(mb);
                }
            }
            while (tail - head >= (more ? 64u : 1u)) {
                const unsigned n = min(64u, tail - head);
                __builtin_amdgcn_wave_barrier();
                if ((unsigned)lane < n) {
                    const float4 c = tile[ring[(head + lane) & 255]];
                    const float2 t = mlapm_ucy_correction(P, c.x - pi.x, c.y - pi.y, c.z - vi.x, c.w - vi.y, vi.x, vi.y, ex, ey);
                    sx += t.x; sy += t.y;
                }
                head += n;
            }
            if (!more) break;
        }
        return;
    }
    for (; j < tn; j += 64) {
        const float4 s = tile[j];
        if (P.skip_absent && (s.x != s.x || s.y != s.y)) continue;      // absent source
        const float2 t = mlapm_pair(P, s.x - pi.x, s.y - pi.y, s.z - vi.x, s.w - vi.y, vi.x, vi.y, ex, ey);
        sx += t.x; sy += t.y;
    }
}

// d(-G . T)/d(vr), d(-G . T)/d(vv) of one ordered pair, T the pair term of mlapm_pair and
// (Gx, Gy) the upstream gradient on the focal agent's force.  view, the rotation sign and the
// UCY collision flag are piecewise constant and carry no gradient (as in autograd).
__device__ __forceinline__ void mlapm_pair_grad(const MlapmParams& P, float rx, float ry, float wx, float wy,
                                                float vix, float viy, float ex, float ey, float Gx, float Gy,
                                                float& ax, float& ay, float& bx, float& by, int ucy_flag = -1) {
    ax = ay = bx = by = 0.f;
    const float d2 = rx * rx + ry * ry;
    if (!(d2 > 0.f) || !(vix * rx + viy * ry > 0.f)) return;
    const float rinv = fast_rsq(d2), r = d2 * rinv;
    const float nx = rx * rinv, ny = ry * rinv;
    float st = 0.f, ct = 1.f;
    if (P.variant != 0) {
        const float cr = rx * ey - ry * ex;
        st = cr > 0.f ? -P.sth : P.sth; ct = P.cth;
    }
    const float ux = ct * Gx + st * Gy, uy = -st * Gx + ct * Gy;   // R^T G
    const float un = ux * nx + uy * ny;
    float phi2, fx, fy, hx = 0.f, hy = 0.f;                        // phi*log2e, d(phi)/d(vr), d(phi)/d(vv)
    if (P.variant == 0) {
        phi2 = P.B2 * r; fx = P.B * nx; fy = P.B * ny;
    } else if (P.variant == 1) {
        const float w2 = wx * wx + wy * wy;
        const float ri8 = fminf(rinv, 1e8f), qi8 = fminf(fast_rsq(w2), 1e8f);
        const float n8x = rx * ri8, n8y = ry * ri8, mx = wx * qi8, my = wy * qi8;
        const float cs = n8x * mx + n8y * my;
        phi2 = P.B2 * r + P.C2 * cs + P.D2 * r * cs;
        const float k1 = P.Cc + P.D * r;
        const bool r_ok = r > 1e-8f, q_ok = w2 > 1e-16f;
        const float csx = (r_ok ? mx - cs * n8x : mx) * ri8;       // d(cs)/d(vr)
        const float csy = (r_ok ? my - cs * n8y : my) * ri8;
        fx = P.B * nx + k1 * csx + P.D * cs * nx;
        fy = P.B * ny + k1 * csy + P.D * cs * ny;
        hx = k1 * (q_ok ? n8x - cs * mx : n8x) * qi8;              // d(cs)/d(vv)
        hy = k1 * (q_ok ? n8y - cs * my : n8y) * qi8;
    } else {
        const float cf = (ucy_flag >= 0 ? ucy_flag != 0 : ucy_collision(rx, ry, wx, wy, P.r2)) ? 1.f : 0.f;      // the forward's exact flag
        phi2 = (P.B2 * r + P.C2) * cf; fx = P.B * cf * nx; fy = P.B * cf * ny;
    }
    const float AE = -P.A * fast_exp2(phi2);
    ax = AE * (un * fx + (ux - un * nx) * rinv);
    ay = AE * (un * fy + (uy - un * ny) * rinv);
    bx = AE * un * hx;
    by = AE * un * hy;
}

// The constants of a calibration launch, read from device memory (mlapm_fit.hip, mlapm_rollout_fit.hip), and the
// per-focal parameter sums of the calibration kernels.
struct FitConst {
    float tau, A, B2, C2, D2, cth, sth, r2;
    int variant;
};

__device__ __forceinline__ FitConst fit_const(const float* __restrict__ params, int variant, float radius) {
    FitConst K;
    K.variant = variant;
    K.tau = params[0]; K.A = params[1];
    const float log2e = 1.4426950408889634f;
    K.B2 = params[2] * log2e; K.C2 = params[3] * log2e; K.D2 = params[4] * log2e;
    // cos / sin of theta pi / 180 by sincospif (make_params forms theta / 180 * pi and calls cosf / sinf on the host; the two
    // agree to an ulp, and sincospif needs no large-argument reduction, which would put an array in scratch memory)
    sincospif(params[5] / 180.f, &K.sth, &K.cth);
    K.r2 = radius * 2.f;
    return K;
}

// The focal agent's sums over its sources, with u = view * g (mlapm.py:25-53) and dir the (rotated) unit direction:
//   U = sum u dir            (force = A U;            d force / dA = U)
//   UB = sum u kB dir        (d force / dB = A UB;    kB = r, UCY r [coll])
//   UC = sum u kC dir        (d force / dC = A UC;    kC = cos (GC), [coll] (UCY))
//   UD = sum u r cos dir     (d force / dD = A UD;    GC)
//   UT = sum u d dir / d theta_deg   (rotation R(s theta pi / 180), GC and UCY)
struct FitAcc {
    float ux, uy, bx, by, cx, cy, dx, dy, tx, ty;
};

__device__ __forceinline__ void fit_pair(const FitConst& K, float rx, float ry, float wx, float wy, float vix, float viy,
                                         float ex, float ey, FitAcc& a) {
    // (every sum is updated unconditionally, with zero factors where a term does not apply: selects rather than branches
    // keep the accumulators in registers)
    const float d2 = rx * rx + ry * ry;
    const bool pos = d2 > 0.f;
    const float rinv = fast_rsq(d2);
    const float r = pos ? d2 * rinv : d2;                           // :26
    const float view = (vix * rx + viy * ry > 0.f) ? 1.f : 0.f;     // :27
    const float ninv = pos ? rinv : 0.f;
    const float nx = rx * ninv, ny = ry * ninv;
    float u, kB = r, kC = 0.f, kD = 0.f, dirx = nx, diry = ny, ddx = 0.f, ddy = 0.f;
    if (K.variant == 0) {
        u = fast_exp2(K.B2 * r);                                    // :29
    } else {
        const float cr = rx * ey - ry * ex;                         // :34 / :48
        const float sg = cr > 0.f ? -1.f : 1.f;                     // theta_ij = -sign(cr) theta, 0 -> +theta
        const float st = sg * K.sth;
        dirx = K.cth * nx - st * ny; diry = st * nx + K.cth * ny;   // :36-39
        // d dir / d theta_deg = (pi / 180) sg (-sin nx - cos ny, cos nx - sin ny) at theta_ij
        const float k = sg * 0.017453292519943295f;
        ddx = k * (-st * nx - K.cth * ny); ddy = k * (K.cth * nx - st * ny);
        if (K.variant == 1) {
            const float w2 = wx * wx + wy * wy;
            const float cs = (rx * wx + ry * wy) * fminf(rinv, 1e8f) * fminf(fast_rsq(w2), 1e8f);   // :32
            u = fast_exp2(K.B2 * r + K.C2 * cs + K.D2 * r * cs);     // :40
            kC = cs; kD = r * cs;
        } else {
            const bool coll = ucy_collision(rx, ry, wx, wy, K.r2);  // :43-47, exact; no gradient
            u = coll ? fast_exp2(K.B2 * r + K.C2) : 1.f;            // :53 (coll.unsqueeze(-1))
            kB = coll ? r : 0.f; kC = coll ? 1.f : 0.f;
        }
    }
    u *= view;
    const float ux = u * dirx, uy = u * diry;
    a.ux += ux; a.uy += uy;
    a.bx += kB * ux; a.by += kB * uy;
    a.cx += kC * ux; a.cy += kC * uy;
    a.dx += kD * ux; a.dy += kD * uy;
    a.tx += u * ddx; a.ty += u * ddy;
}

// float64 sum over the 64 lanes of a wave (fixed butterfly order)
__device__ __forceinline__ double wave_sum_d(double x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

// the constants of a launch (host)
static inline MlapmParams make_params(int variant, float tau, float A, float B, float Cc, float D, float theta_deg,
                               float radius, int skip_absent = 0) {
    MlapmParams P;
    P.skip_absent = skip_absent;
    static const bool two_phase_off = getenv("PIML_MLAPM_UCY_TWO_PHASE") && atoi(getenv("PIML_MLAPM_UCY_TWO_PHASE")) == 0;
    P.ucy_two_phase = two_phase_off ? 0 : 1;
    P.variant = variant; P.tau = tau; P.A = A; P.B = B; P.Cc = Cc; P.D = D;
    // the reference forms theta = sign * theta / 180 * pi in float32 (mlapm.py:34)
    const float th = theta_deg / 180.f * 3.14159265358979323846f;
    P.cth = cosf(th); P.sth = sinf(th);
    P.r2 = radius * 2.f;
    const float log2e = 1.4426950408889634f;
    P.B2 = B * log2e; P.C2 = Cc * log2e; P.D2 = D * log2e;
    return P;
}

}  // namespace piml
