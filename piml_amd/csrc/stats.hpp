// What the crowd-statistics kernels share: the workgroup compaction that stages a tile in LDS, the focal box
// test and the host's sizing of runs of slices.  The wave reductions are in common.hpp.
#pragma once
#include "common.hpp"

namespace piml {

// Compacts the kept slots of [lo, hi) in slot order; returns their number.  keep(j) loads slot j and says whether it stays;
// put(q, j) stores it at place q of the tile (what keep loaded reaches put through the callers' captures).  Every thread
// of a workgroup of THREADS lanes calls it; wave_cnt is THREADS / 64 ints of LDS.
// The barrier contract, stated here once: the tile may still be read by other waves on entry, so nothing is written before
// the first barrier of a round; the second barrier of a round completes the tile (the caller may read it on return) and
// frees wave_cnt, which the next round and the next call rewrite.
template <int THREADS, class Keep, class Put>
__device__ __forceinline__ int wg_compact(int lo, int hi, int* wave_cnt, Keep keep, Put put) {
    const int tid = threadIdx.x, w = tid >> 6;
    int base = 0;
    for (int s0 = lo; s0 < hi; s0 += THREADS) {
        const int j = s0 + tid;
        const bool kept = j < hi && keep(j);
        const u64 b = __ballot(kept);
        if ((tid & 63) == 0) wave_cnt[w] = __popcll(b);
        __syncthreads();
        int before = base, total = base;
        for (int k = 0; k < THREADS / 64; ++k) {
            before += k < w ? wave_cnt[k] : 0;
            total += wave_cnt[k];
        }
        if (kept) put(before + (int)mbcnt(b), j);
        __syncthreads();
        base = total;
    }
    return base;
}

// the focal box [x0, x1) x [y0, y1), when there is one
__device__ __forceinline__ bool in_box(int has_box, float x0, float x1, float y0, float y1, float2 p) {
    return !has_box || (x0 <= p.x && p.x < x1 && y0 <= p.y && p.y < y1);
}

// Host: a workgroup takes `run` consecutive slices, sized so that about target_wg workgroups start (1 <= run <= max_run).
// Returns the grid, capped at max_grid (0: no slices, nothing to launch).
inline unsigned stats_run_grid(long long slices, long long target_wg, int max_run, long long max_grid, int* run) {
    const long long r = slices / target_wg;
    *run = (int)(r < 1 ? 1 : r > max_run ? max_run : r);
    const long long runs = (slices + *run - 1) / *run;
    return (unsigned)(runs < max_grid ? runs : max_grid);
}

}  // namespace piml
