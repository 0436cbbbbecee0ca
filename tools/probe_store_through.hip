// What does a launch pay at its end for the lines its stores left dirty in the L2s, and what does the NEXT launch pay when it
// finds those bytes in memory instead?  (profiles/r12_store_through.md; piml_amd/csrc/store.hpp.)
//
// producer<MODE, MB>: 256 workgroups of 256 threads; each spins a few microseconds of arithmetic, then stores its share
//   (MB MiB / 256, contiguous: the shape of a gradient slot) as its LAST action.
//     MODE 0  plain 16-byte stores                  MODE 1  write-through (sc1) 16-byte stores
//     MODE 2  plain 4-byte stores                   MODE 3  write-through 4-byte stores
//   (a 4-byte wave instruction writes 256 contiguous bytes = two whole 128-byte lines, a 16-byte one eight)
// consumer<MODE, MB, SHIFT>: follows the producer in a captured graph; workgroup c reads the share of producer (c + SHIFT) % 256
//   once, 16 bytes per lane, and leaves one sum.  SHIFT 0: the reader sits on the XCD that stored the bytes (workgroups are
//   dealt round-robin over the XCDs); SHIFT 3: on another one.  MODE and MB only name the kernel for the trace.
// Plain kernels, no flag, poll, fence or spin on memory: the launch boundary is the only publication.
//
// The host captures PAIRS (producer, consumer) pairs into one graph and replays it; `pair us` = HIP events around the replays /
// pairs (tools/probe_store_through.py makes the table).
// build: hipcc -O3 --offload-arch=gfx950 -I piml_amd/csrc -o tools/probe_store_through tools/probe_store_through.hip
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "store.hpp"

#define CK(x)                                                                                 \
    do {                                                                                      \
        hipError_t e_ = (x);                                                                  \
        if (e_ != hipSuccess) {                                                               \
            fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
            exit(1);                                                                          \
        }                                                                                     \
    } while (0)

constexpr int WG = 256, THREADS = 256, PAIRS = 20, REPLAYS = 20;

template <int MODE, int MB>
__global__ __launch_bounds__(THREADS) void producer(float* __restrict__ buf, float seed) {
    constexpr size_t SHARE = (size_t)MB * 1024 * 1024 / 4 / WG;       // floats per workgroup (a multiple of 1024)
    float a = seed + threadIdx.x;
    for (int i = 0; i < 1500; ++i) a = __fmaf_rn(a, 1.0001f, 0.5f);
    float* p = buf + (size_t)blockIdx.x * SHARE;
    if constexpr (MODE < 2) {
        float4* q = reinterpret_cast<float4*>(p);
        const float4 v = make_float4(a, a + 1.f, a + 2.f, a + 3.f);
#pragma unroll
        for (int j = 0; j < (int)(SHARE / 4 / THREADS); ++j) piml::store16<MODE == 1>(q + j * THREADS + threadIdx.x, v);
    } else {
#pragma unroll 8
        for (int j = 0; j < (int)(SHARE / THREADS); ++j) {
            const int i = j * THREADS + threadIdx.x;
            if constexpr (MODE == 3) __hip_atomic_store(p + i, a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);       // global_store_dword ... sc1
            else p[i] = a;
        }
    }
}

template <int MODE, int MB, int SHIFT>
__global__ __launch_bounds__(THREADS) void consumer(const float* __restrict__ buf, float* __restrict__ out) {
    constexpr size_t SHARE = (size_t)MB * 1024 * 1024 / 4 / WG;
    const float4* q = reinterpret_cast<const float4*>(buf + (size_t)((blockIdx.x + SHIFT) % WG) * SHARE);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < (int)(SHARE / 4 / THREADS); ++j) {
        const float4 v = q[j * THREADS + threadIdx.x];
        s += (v.x + v.y) + (v.z + v.w);
    }
    if (s == 12345.678f) out[blockIdx.x] = s;       // (keeps the loads; one workgroup's store would not matter to the next producer)
}

template <int MODE, int MB, int SHIFT>
static void run(float* buf, float* out, hipStream_t s) {
    hipGraph_t g;
    hipGraphExec_t e;
    CK(hipStreamBeginCapture(s, hipStreamCaptureModeGlobal));
    for (int i = 0; i < PAIRS; ++i) {
        hipLaunchKernelGGL((producer<MODE, MB>), dim3(WG), dim3(THREADS), 0, s, buf, (float)i);
        hipLaunchKernelGGL((consumer<MODE, MB, SHIFT>), dim3(WG), dim3(THREADS), 0, s, buf, out);
    }
    CK(hipStreamEndCapture(s, &g));
    CK(hipGraphInstantiate(&e, g, nullptr, nullptr, 0));
    hipEvent_t t0, t1;
    CK(hipEventCreate(&t0));
    CK(hipEventCreate(&t1));
    for (int i = 0; i < 3; ++i) CK(hipGraphLaunch(e, s));
    CK(hipStreamSynchronize(s));
    CK(hipEventRecord(t0, s));
    for (int i = 0; i < REPLAYS; ++i) CK(hipGraphLaunch(e, s));
    CK(hipEventRecord(t1, s));
    CK(hipStreamSynchronize(s));
    float ms = 0.f;
    CK(hipEventElapsedTime(&ms, t0, t1));
    static const char* names[4] = {"plain 16 B", "write-through 16 B", "plain 4 B", "write-through 4 B"};
    printf("PAIR mode=%d MB=%d shift=%d pair_us=%.3f  # %s, %d MiB, reader on %s XCD\n", MODE, MB, SHIFT,
           ms * 1e3 / (PAIRS * REPLAYS), names[MODE], MB, SHIFT ? "another" : "the storing");
    fflush(stdout);
    CK(hipEventDestroy(t0));
    CK(hipEventDestroy(t1));
    CK(hipGraphExecDestroy(e));
    CK(hipGraphDestroy(g));
}

template <int MB>
static void sizes(float* buf, float* out, hipStream_t s) {
    run<0, MB, 0>(buf, out, s); run<1, MB, 0>(buf, out, s); run<2, MB, 0>(buf, out, s); run<3, MB, 0>(buf, out, s);
    run<0, MB, 3>(buf, out, s); run<1, MB, 3>(buf, out, s); run<2, MB, 3>(buf, out, s); run<3, MB, 3>(buf, out, s);
}

int main() {
    float *buf, *out;
    CK(hipMalloc(&buf, (size_t)18 * 1024 * 1024));
    CK(hipMalloc(&out, WG * sizeof(float)));
    hipStream_t s;
    CK(hipStreamCreate(&s));
    sizes<4>(buf, out, s);
    sizes<13>(buf, out, s);
    sizes<18>(buf, out, s);
    CK(hipStreamDestroy(s));
    CK(hipFree(buf));
    CK(hipFree(out));
    return 0;
}
