// What the two crowd-statistics entries share (crowdstats.hip: Gaussian density; voronoi.hip: Voronoi density): the kernel
// arguments, the presence rule, the LDS staging of a slice's present agents, and the host half that checks
// the common arguments and launches the statistics pass and the diagram's reduce pass.
#pragma once
#include "stats.hpp"

namespace piml {

constexpr int CD_THREADS = 256;
constexpr int CD_WAVES = CD_THREADS / 64;
constexpr int CD_TILE = 1024;                 // source slots per LDS tile (8 KiB of positions)
constexpr int CD_MAX_BINS = 256;
constexpr long long CD_MAX_GRID = 1 << 20;

struct CrowdArgs {
    const float *P, *V, *M;                   // (S, T, N, 2), (S, T, N, 2), (S, T, N)
    const int* n_active;                      // (S) or NULL
    int S, T, N, t0, Tp, B;
    float inv_r2, rho_bin;
    double area;                              // pi R^2
    int has_box, gx, gy;
    float x0, x1, y0, y1, cell;
    long long *n, *n_speed;                   // (S, T')
    double *sum_speed, *sum_density;          // (S, T')
    long long* map;                           // (S, gy, gx) or NULL
    float* density;                           // (S, T', N) or NULL
    double *ws_sum, *ws_sum2;                 // (S T', B)
    int* ws_count;                            // (S T', B)
    long long *fd_count;                      // (S, B)
    double *fd_sum, *fd_sum2;                 // (S, B)
    const float* rho_in;                      // (S T', N) densities computed beforehand (NaN: not focal), or NULL
};

__device__ __forceinline__ bool cd_present(float m, float2 p) { return m == 1.f && isfinite(p.x) && isfinite(p.y); }

// Compacts the present agents of slots [lo, hi) (hi - lo <= CD_TILE) into src in slot order; returns their number
// (wg_compact: every thread calls it, and src may still be read on entry).
__device__ inline int cd_stage(const float2* P, const float* M, int lo, int hi, float2* src, int* wave_cnt) {
    float2 p;
    return wg_compact<CD_THREADS>(
        lo, hi, wave_cnt, [&](int j) { return p = P[j], cd_present(M[j], p); }, [&](int q, int) { src[q] = p; });
}

// crowdstats.hip.  cd_prepare: checks every argument the two entries share and fills `a` (workspace: the diagram's slots
// first, then `extra_bytes` for the caller at *extra); hipSuccess or hipErrorInvalidValue.  cd_run: the map's memset, the
// statistics pass -- sweeping the Gaussian density, or taking each agent's density from a.rho_in when given_density --
// and the reduce pass.
long long cd_workspace_bytes(long long slices, int B);
hipError_t cd_prepare(CrowdArgs& a, const float* P, const float* V, const float* M, const int* n_active, int S, int T, int N,
                      int t0, int t1, int has_box, float x0, float x1, float y0, float y1, float cell, int gx, int gy,
                      float rho_bin, int rho_bins, long long* n, long long* n_speed, double* sum_speed, double* sum_density,
                      long long* fd_count, double* fd_sum, double* fd_sum2, long long* map, float* density, void* workspace,
                      long long workspace_bytes, long long extra_bytes, void** extra);
hipError_t cd_run(const CrowdArgs& a, bool given_density, hipStream_t st);

}  // namespace piml
