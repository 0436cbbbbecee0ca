// Write-through stores for a launch's bulk outputs (profiles/r12_store_through.md).
//
// A plain store leaves its line dirty in the storing XCD's L2; what is still dirty when the launch ends is written back before
// the next launch of the stream starts.  An `sc1` store goes to memory at once and drops the line, so a stream written with it
// leaves nothing for the end of the launch; its reader finds the bytes in memory (the Infinity Cache), not in an L2.  Measured
// (tools/probe_store_through.hip, 13 - 18 MiB stored as the producer's last action): the pair producer + consumer is 0.9 us
// shorter when the reader sits on another XCD than the writer, as seven of eight readers of a slot array do, and 0.4 - 0.9 us
// longer when it sits on the same one.  So a stream qualifies only if no workgroup of the same launch reads it back and its
// reader is spread over the XCDs.  A 4-byte sc1 store costs what a 16-byte one does as long as every wave instruction writes
// whole 128-byte lines -- the slot stores do, as they stand -- so no stream is widened for it (forms 1 and 2 below were built for
// that question and lost: the transposition costs more than the fewer instructions save).  The launch boundary stays the only
// publication: no fence, flag or ticket belongs to these stores.
//
// One compile-time switch per stream, the form of its stores (an A/B pair is two builds of the library, piml_amd.build.variant):
// 0 = 4 bytes per lane, plain (what the stream was); 1 = 16 bytes per lane, plain; 2 = 16 bytes per lane, write-through;
// 3 = 4 bytes per lane, write-through (the default).
#pragma once
#include <hip/hip_runtime.h>

#ifndef PIML_WT_ENC_BWD_SLOTS            // encoder_bwd5.hip: a workgroup's dW2 slot, stored behind its last tile
#define PIML_WT_ENC_BWD_SLOTS 3
#endif
#ifndef PIML_WT_DEC_BWD_SLOTS            // decoder.hip: dec_bwd_dw_body4's dW1 / dW2 slots
#define PIML_WT_DEC_BWD_SLOTS 3
#endif

namespace piml {

typedef unsigned st_u32x4 __attribute__((ext_vector_type(4)));
typedef float st_f32x4 __attribute__((ext_vector_type(4)));

// 16 bytes per lane to a global pointer (16-byte aligned); WT: global_store_dwordx4 ... sc1.
// The s_nop belongs to the store: a store of more than 8 bytes per lane still reads its data registers for two wait states after
// it issues, the compiler keeps a vector instruction that overwrites them away from a store it knows, and it does not look into
// an asm statement (without the s_nop the next block's first add landed in the registers of the store before it: wrong slots).
template <bool WT>
__device__ __forceinline__ void store16(float4* p, const float4 v) {
    if constexpr (WT) {
        const st_f32x4 r = {v.x, v.y, v.z, v.w};
        asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(r) : "memory");
    } else *p = v;
}

// 16 bytes per lane through a buffer resource (an offset past its range is not stored); WT: buffer_store_dwordx4 ... sc1
template <bool WT>
__device__ __forceinline__ void store16(const __amdgpu_buffer_rsrc_t rs, unsigned voff, unsigned soff, const st_u32x4 v) {
    if constexpr (WT) __builtin_amdgcn_raw_buffer_store_b128(v, rs, (int)voff, (int)soff, 16);
    else __builtin_amdgcn_raw_buffer_store_b128(v, rs, (int)voff, (int)soff, 0);
}

// 4 x 4 transposition inside every quad of lanes (DPP quad_perm, no LDS): lane q of a quad comes in with m[i] = M[i][q] and leaves
// with M[q][0 .. 3] -- four registers that hold one column of four rows become four consecutive columns of one row, the shape
// of a 16-byte store.  Moves only: every value keeps its bits.
__device__ __forceinline__ float st_quad_xor1(float v) {
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xf, 0xf, false));       // quad_perm [1, 0, 3, 2]
}
__device__ __forceinline__ float st_quad_xor2(float v) {
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x4E, 0xf, 0xf, false));       // quad_perm [2, 3, 0, 1]
}
__device__ __forceinline__ float4 quad_transpose(float m0, float m1, float m2, float m3, int lane) {
    const bool odd = lane & 1, hi = lane & 2;
    // lanes q ^ 1: the even lane keeps row 0 / 2 and receives its neighbour's column of it, the odd lane row 1 / 3
    const float r01 = st_quad_xor1(odd ? m0 : m1), r23 = st_quad_xor1(odd ? m2 : m3);
    const float a0 = odd ? r01 : m0, a1 = odd ? m1 : r01;      // row (q & 1), columns (q & 2), (q & 2) + 1
    const float a2 = odd ? r23 : m2, a3 = odd ? m3 : r23;      // row 2 + (q & 1), the same columns
    // lanes q ^ 2: the low pair of lanes keeps rows 0 / 1 and receives their columns 2, 3; the high pair rows 2 / 3, columns 0, 1
    const float s0 = st_quad_xor2(hi ? a0 : a2), s1 = st_quad_xor2(hi ? a1 : a3);
    return hi ? make_float4(s0, s1, a2, a3) : make_float4(a0, a1, s0, s1);
}

// 4 bytes per lane to a global pointer; WT: global_store_dword ... sc1 (an instruction the compiler knows: no wait states to add)
template <bool WT>
__device__ __forceinline__ void store4(float* p, float v) {
    if constexpr (WT) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *p = v;
}

// One 32 x 32 block of a 32x32 matrix instruction's accumulators (register r of lane (i = lane & 31, h = lane >> 5) holds row
// rho(r) + 4 h, rho(r) = (r & 3) + 8 (r >> 2), column i) to row-major memory: `block` = its row 0, column 0 (16-byte aligned), ld
// floats per row (a multiple of 32: a row of the block is one 128-byte line).
// FORM 0 / 3: sixteen 4-byte stores, each wave instruction two whole lines (rows rho(r) and rho(r) + 4), plain / written through.
// FORM 1 / 2: registers 4 g .. 4 g + 3 of a lane are four consecutive rows of one column, so a quad transposition turns them into
// row 8 g + 4 h + (i & 3), columns 4 (i >> 2) .. + 3: four 16-byte stores, each wave instruction eight whole lines, plain / written
// through.
template <int FORM, class F>
__device__ __forceinline__ void store_acc32(float* block, int ld, int lane, F&& value) {
    const int i = lane & 31, h = lane >> 5;
    if constexpr (FORM == 0 || FORM == 3) {
#pragma unroll
        for (int r = 0; r < 16; ++r) store4<FORM == 3>(block + (size_t)((r & 3) + 8 * (r >> 2) + 4 * h) * ld + i, value(r));
    } else {
        float* p = block + (size_t)(4 * h + (i & 3)) * ld + 4 * (i >> 2);
#pragma unroll
        for (int g = 0; g < 4; ++g)
            store16<FORM == 2>(reinterpret_cast<float4*>(p + (size_t)(8 * g) * ld),
                               quad_transpose(value(4 * g), value(4 * g + 1), value(4 * g + 2), value(4 * g + 3), lane));
    }
}

}  // namespace piml
