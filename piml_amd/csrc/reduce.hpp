// The slot sums of a backward pass (one launch for every partial set) and their DEFERRED form: a piml_pinnsf_bwd called with
// PIML_DEFER_SLOT_SUMS leaves the description of its sums here instead of launching them, and the next piml_relfeat_self_bwd
// on the same stream runs them as the leading workgroups of ITS launch (relfeat.hip): the two kernels are independent (the
// sums read the weight-gradient slots, the relfeat backward the feature gradients), each is small next to the chip, and a
// launch boundary on gfx950 costs ~4.5 us.  Private to libpiml_hip.so.
#pragma once
#include <hip/hip_runtime.h>

#include "pack.hpp"

namespace piml {

struct ReduceSet {
    const float* parts;
    float* grads;
    int slots, lanes, split, off0, off1;       // float4 geometry: sum_slots_16x16 (pack.hpp)
    const int* dev_slots;                      // non-NULL: the slot count is read here (compact rows: the split of the encoder
                                               // backward's workgroups between the branches follows the plan, encoder_bwd5.hip)
};
// PIML_POOL_TRAIN: behind the slot sums, the gradient of a decoder's FOLDED first layer W1' = s W1 W3, b1' = b1 + k s W1 b3
// (G = d/d(W1'), g_b = d/d(b1'), both in the decoder's summed `grads`) is unfolded into the gradients of its factors:
//     dW1 = s (G W3^T + k g_b b3^T)   -> dw1_out (64, 128)
//     dW3 = s W1^T G, db3 = s k W1^T g_b   -> the dW3 / db3 fields of the encoder's `grads`
struct UnfoldSet {
    const float* dgrads;   // decoder `grads` (DEC_PART floats)
    const float *w1, *w3, *b3;
    float scale;
    int k;
    float* dw1_out;
    float* egrads;         // encoder `grads` (ENC_PART layout)
};
constexpr int REDUCE_SETS = 8;   // (the bottleneck variants leave 4 encoder + 2 row decoder + 1 head sets in one backward pass)
struct ReduceAll {
    ReduceSet set[REDUCE_SETS];
    int nsets;
    int accumulate;       // PIML_ACCUMULATE: grads += the sums
    int gx;               // workgroups per set (the widest set's (lanes + 15) / 16)
    UnfoldSet unf[2];
    int nunf;             // > 0: the unfold behind the sums
    int defer_unfold;     // PIML_DEFER_UNFOLD of the pass: its unfold may wait while the device defers (piml_pinnsf_unfold_defer)
    int dec_upstream;     // the decoder sets were summed by the encoder backward's launch (DecSlotSums, encoder_bwd5.hip): nothing in
                          // this launch writes what the unfold reads, so its workgroups may ride in it (unfold_begin)
    int unf_blocks;       // set by unfold_begin: the launch's leading workgroups that run the unfold (nunf * kUnfoldBlocks, or 0)
};
constexpr int kUnfoldBlocks = 64 + 64 + 1;       // per set: rows of dW1 | row pairs of dW3 | db3

// The unfold of R at the launch that sums R's slots, decided once (network.hip).  While the device defers (piml_pinnsf_unfold_defer)
// a pass that asked for it, R's unfold is recorded and waits; otherwise with R.dec_upstream it rides in the sums launch (the
// returned description carries unf_blocks), else it is a launch of its own behind it.  unfold_end, behind the sums launch,
// launches what is left: R's own unfold, or the entry of another network that R's recording replaced.
struct UnfoldTail {
    ReduceAll R;
    hipStream_t stream = nullptr;
    bool go = false;
};
ReduceAll unfold_begin(const ReduceAll& R, hipStream_t s, UnfoldTail* t);
int unfold_end(const UnfoldTail& t);

// unfold workgroup `bid` of nunf * kUnfoldBlocks: set bid / kUnfoldBlocks, block bid % kUnfoldBlocks.  float64 accumulation (4 M
// multiply-adds in all: its time was the launch); one thread per output element.  Reads the decoder's summed `grads` (G = the FOLDED
// dW1' field, g_b = its db1' field), W1, W3, b3; writes dw1_out and the dW3 / db3 fields of the encoder's `grads` -- [0, EH EH) and
// [2 EH EH + 8 EH, + EH), disjoint from the layer-1 set (DW2_L1_OFF0 / OFF1) the same launch sums into that buffer.  (Unrolled
// to stay within 64 registers: as leading workgroups of the relfeat backward the body sets that launch's occupancy.)
__device__ __forceinline__ void unfold_block(const ReduceAll& R, int bid) {
    const int y = bid / kUnfoldBlocks, x = bid - y * kUnfoldBlocks, tid = (int)threadIdx.x;
    const UnfoldSet U = R.unf[y];
    const float* __restrict__ G = U.dgrads;
    const float* __restrict__ gb = U.dgrads + DD * DH + DD * DD + 2 * DD;
    const double sc = (double)U.scale;
    if (x < 64) {                     // row x of dW1: s (G[x][:] W3^T + k g_b[x] b3)
        __shared__ float g[DH];
        __shared__ double part[256];
        if (tid < DH) g[tid] = G[(size_t)x * DH + tid];
        __syncthreads();
        const int m = tid & 127, half = tid >> 7;
        const float4* wr = reinterpret_cast<const float4*>(U.w3 + (size_t)m * EH + 64 * half);
        double a = 0.0;
#pragma unroll 8
        for (int q = 0; q < 16; ++q) {
            const float4 wv = wr[q];
            const float* gq = g + 64 * half + 4 * q;
            a += (double)gq[0] * wv.x + (double)gq[1] * wv.y + (double)gq[2] * wv.z + (double)gq[3] * wv.w;
        }
        part[tid] = a;
        __syncthreads();
        if (tid < DH)
            U.dw1_out[(size_t)x * DH + tid] = (float)(sc * ((part[tid] + part[tid + 128]) + (double)U.k * (double)gb[x] * (double)U.b3[tid]));
    } else if (x < 128) {             // rows 2 (x - 64), + 1 of dW3 = s W1^T G (the terms in order of i, 8 loads of each factor in flight)
        const int m = __builtin_amdgcn_readfirstlane(2 * (x - 64) + (tid >> 7)), j = tid & 127;
        double a = 0.0;
        for (int i0 = 0; i0 < DD; i0 += 8) {
            float wv[8], gv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) { wv[u] = U.w1[(size_t)(i0 + u) * DH + m]; gv[u] = G[(size_t)(i0 + u) * DH + j]; }
#pragma unroll
            for (int u = 0; u < 8; ++u) a += (double)wv[u] * (double)gv[u];
        }
        U.egrads[(size_t)m * EH + j] = (float)(sc * a);
    } else if (tid < EH) {            // db3 = s k W1^T g_b (the same way)
        double a = 0.0;
        for (int i0 = 0; i0 < DD; i0 += 8) {
            float wv[8], gv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) { wv[u] = U.w1[(size_t)(i0 + u) * DH + tid]; gv[u] = gb[i0 + u]; }
#pragma unroll
            for (int u = 0; u < 8; ++u) a += (double)wv[u] * (double)gv[u];
        }
        U.egrads[2 * EH * EH + 8 * EH + tid] = (float)(sc * (double)U.k * a);
    }
}
static_assert(2 * EH * EH + 8 * EH >= (DW2_L1_OFF0 + DW2_L1_SPLIT) * 4 && 2 * EH * EH + 9 * EH <= DW2_L1_OFF1 * 4 && EH * EH <= DW2_L1_OFF0 * 4,
              "the unfold's dW3 / db3 fields lie outside the encoder layer-1 set's targets");

// workgroup `bid` of gx * nsets: set bid / gx, column block bid % gx
__device__ __forceinline__ void reduce_block(const ReduceAll& A, int bid) {
    const int y = bid / A.gx, x = bid - y * A.gx;
    const ReduceSet S = A.set[y];
    if (x * 16 < S.lanes) sum_slots_16x16_at(x, S.parts, S.grads, S.dev_slots ? *S.dev_slots : S.slots, S.lanes, S.split, S.off0, S.off1, A.accumulate != 0);
}
// workgroup `bid` of a slot-sum launch of A.unf_blocks + gx * nsets: the unfold's workgroups lead (their f64 chains are the longest)
__device__ __forceinline__ void reduce_launch_block(const ReduceAll& A, int bid) {
    if (bid < A.unf_blocks) unfold_block(A, bid);
    else reduce_block(A, bid - A.unf_blocks);
}
__host__ __device__ inline int reduce_launch_blocks(const ReduceAll& A) { return A.unf_blocks + A.gx * A.nsets; }

// ---- the weight pack of the network (every operand image in one launch, network.hip) and its deferred form: a
// piml_pinnsf_pack called with PIML_DEFER_PACK leaves its description here, and the next relfeat FORWARD launch on the same
// stream runs it as its trailing workgroups (the pack depends on the weights only; alone it is a ~4 us launch in front of
// the step's chain).  Every consumer of packed images (piml_pinnsf_fwd with PIML_PACKED_VALID, piml_encoder_fwd_packed,
// piml_rowdecoder_fwd_packed) first launches a pack that is still waiting. ----
struct PackAll {
    piml_encoder_branch enc[2];
    piml_decoder_branch dec[2];
    piml_collision_head head;
    int nbr, has_head;
    int has_fold;         // a decoder branch or the head carries fold_w3: nbr + has_head fold sets ride behind the image sets
    int skip_f32;         // the encoders' f32-instruction fragment images (4 x 16384 floats per branch) are not written: every
                          // kernel the library would launch reads the split-product images (piml_encoder_products(1), the default)
};
// live elements of an encoder set: with skip_f32 the two f32 fragment blocks [0, 32768) and [PACK_FWD, PACK_FWD + 32768) are left out
constexpr int ENC_LIVE_X3 = PACK_FLOATS - 2 * 32768;
__host__ __device__ inline int enc_set_elems(const PackAll& A) { return A.skip_f32 ? ENC_LIVE_X3 : PACK_FLOATS; }
__host__ __device__ inline int pack_elems_total(const PackAll& A) {
    return A.nbr * (enc_set_elems(A) + DEC_PACK_PLAIN) + (A.has_head ? HEAD_PACK_PLAIN : 0);
}

// element t of the concatenated image sets (encoder branches, decoder branches, head)
__device__ __forceinline__ void pack_flat(const PackAll& A, int t) {
    const int ne = enc_set_elems(A);
    for (int y = 0; y < A.nbr; ++y) {
        if (t < ne) {
            int e = t;
            if (A.skip_f32) e = t < PACK_FWD - 32768 ? t + 32768 : t + 2 * 32768;      // [32768, PACK_FWD) | [PACK_FWD + 32768, PACK_FLOATS)
            const piml_encoder_branch& J = A.enc[y];
            J.packed[e] = pack_value(J, e);
            return;
        }
        t -= ne;
    }
    for (int y = 0; y < A.nbr; ++y) {
        if (t < DEC_PACK_PLAIN) {
            const piml_decoder_branch& J = A.dec[y];
            J.packed[t] = dec_pack_value(J, t);
            return;
        }
        t -= DEC_PACK_PLAIN;
    }
    if (A.has_head && t < HEAD_PACK_PLAIN) A.head.packed[t] = head_pack_value(A.head, t);
}
__host__ __device__ inline int fold_sets(const PackAll& A) { return A.has_fold ? A.nbr + (A.has_head ? 1 : 0) : 0; }
// the folded images (pack.hpp): a workgroup of `threads` threads takes (threads / 64) / CH groups, CH = 8 waves per group (4 for
// 256 threads)
__host__ __device__ inline int fold_groups_per_block(int threads) { return threads >= 512 ? threads / 512 : 1; }
__host__ __device__ inline int fold_blocks(const PackAll& A, int threads) {
    const int g = fold_groups_per_block(threads);
    return (fold_sets(A) * FOLD_GROUPS + g - 1) / g;
}
// workgroup fb of fold_blocks(A, threads); red: threads doubles of LDS.  EVERY thread of the workgroup must call it (barrier).
template <int CH>
__device__ __forceinline__ void fold_block(const PackAll& A, int fb, int threads, double* red, int tid) {
    const int wave = tid >> 6, lane = tid & 63;
    const int grp = fb * ((threads >> 6) / CH) + wave / CH, chunk = wave % CH;
    const int f = grp / FOLD_GROUPS, r = grp - f * FOLD_GROUPS, i = r / 3, hc = r - 3 * i;
    const bool live = f < fold_sets(A);
    const bool is_head = f >= A.nbr;
    const piml_decoder_branch& J = A.dec[is_head ? 0 : f];
    const float* w1 = is_head ? A.head.w1 : J.w1;
    const float* w3 = is_head ? A.head.fold_w3 : J.fold_w3;
    const float* b3 = is_head ? A.head.fold_b3 : J.fold_b3;
    const bool have = live && w3 != nullptr;
    double part = 0.0;
    if (have && (hc < 2 || lane == 0))
        part = fold_partial<CH>(w1 + (size_t)i * DH, hc < 2 ? w3 + 64 * hc + lane : b3, hc < 2 ? EH : 1, chunk);
    red[tid] = part;
    __syncthreads();
    if (have && chunk == 0) {
        double sum = 0.0;
#pragma unroll
        for (int c = 0; c < CH; ++c) sum += red[tid + 64 * c];
        if (is_head) head_fold_store(A.head, i, hc, lane, sum);
        else dec_fold_store(J, i, hc, lane, sum);
    }
}
// the pack inside another launch, cut into "pack blocks" of `threads` threads, kPackPerThread elements per thread (a
// thread's elements are `threads` apart: coalesced stores, independent gathers in flight together; fewer, fatter blocks
// -- 1 100 workgroups of one element per thread cost the relfeat forward 4 us of tail), then the fold blocks.  Two forms carry
// them (relfeat.hip: relfeat_go; piml_relfeat_pack_form selects, TRAILING is the default and the faster one at every measured shape):
//   TRAILING  every pack block is a workgroup of its own behind the launch's search workgroups (first_block >= 0).  A CU takes one
//             only when a search workgroup has left it -- whichever CU is free first, which balances the launch's tail;
//   TAIL      split launches only: obstacle workgroup b of nb -- the short half of the grid -- runs pack blocks b, b + nb, ...
//             behind the epilogue of its own rows and a workgroup barrier per block (tail_stride = nb > 0, no extra workgroups):
//             a fixed share per workgroup, kept for A/B and the tests (profiles/r13_pack_placement.md).
// Same block decomposition, thread count and arithmetic either way: the images are bitwise the same.
constexpr int kPackPerThread = 4;
struct PackWork {
    PackAll A;
    int first_block;          // TRAILING: blockIdx.x of the first pack workgroup; < 0: the launch has no pack workgroups
    int tail_stride;          // TAIL: the number of obstacle workgroups, each takes every tail_stride-th pack block; 0: not this form
};
// TAIL: the pack blocks of obstacle workgroup b of nb are pack_tail_first(b), + pack_tail_stride(nb), ... below the total -- every
// block exactly once over b = 0 .. nb - 1; pack_tail_share is the longest such chain
__host__ __device__ inline int pack_tail_first(int b) { return b; }
__host__ __device__ inline int pack_tail_stride(int nb) { return nb; }
__host__ __device__ inline int pack_tail_share(int nb, int total) { return nb > 0 ? (total + nb - 1) / nb : total; }
__host__ __device__ inline int pack_plain_blocks(const PackAll& A, int threads) {
    return (pack_elems_total(A) + threads * kPackPerThread - 1) / (threads * kPackPerThread);
}
// the zero-row constants of encoder branch y (pack.hpp: PACK_ZROW), one workgroup each: thread (feature j, part p of threads / 128)
// sums 128 / parts terms of W2[j] . relu(b1) in float64, sixteen loads in flight; the parts meet in LDS in order.  The whole
// workgroup calls it (barrier); red: `threads` doubles
__device__ __forceinline__ void zrow_block(const PackAll& A, int y, int threads, double* red, int tid) {
    const piml_encoder_branch& J = A.enc[y];
    const int t = tid, parts = threads >= 512 ? 4 : 2, per = EH / parts;
    double part = 0.0;
    if (t < parts * EH) {
        const int j = t & (EH - 1), p = t >> 7;
        const float* __restrict__ wr = J.w2 + (size_t)j * EH + p * per;
        const float* __restrict__ br = J.b1 + p * per;
        for (int q0 = 0; q0 < per; q0 += 16) {
            float wv[16], bv[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) { wv[u] = wr[q0 + u]; bv[u] = br[q0 + u]; }
#pragma unroll
            for (int u = 0; u < 16; ++u) part += (double)wv[u] * (double)fmaxf(bv[u], 0.f);
        }
    }
    red[t] = part;
    __syncthreads();
    if (t < EH) {
        double sum = 0.0;
        for (int p = 0; p < parts; ++p) sum += red[t + p * EH];
        J.packed[PACK_ZROW + t] = fmaxf(J.b1[t], 0.f);
        J.packed[PACK_ZROW + EH + t] = fmaxf((float)((double)J.b2[t] + sum), 0.f);
    }
}
__host__ __device__ inline int pack_blocks_total(const PackAll& A, int threads) { return pack_plain_blocks(A, threads) + fold_blocks(A, threads) + A.nbr; }
// red: `threads` doubles of LDS (the folded images' partial sums); the whole workgroup calls this.  tid: the caller's threadIdx.x (a
// caller that runs several blocks in a loop hands over a copy the compiler cannot see through, so that a block's per-thread address
// arithmetic is not hoisted out of the loop and held in registers: relfeat_fwd_kernel)
__device__ __forceinline__ void pack_block(const PackAll& A, int bid, int threads, double* red, int tid) {
    const int plain = pack_plain_blocks(A, threads);
    if (bid < plain) {
        const int total = pack_elems_total(A);
#pragma unroll
        for (int j = 0; j < kPackPerThread; ++j) {
            const int t = (bid * kPackPerThread + j) * threads + tid;
            if (t < total) pack_flat(A, t);
        }
    } else if (bid >= plain + fold_blocks(A, threads)) {
        zrow_block(A, bid - plain - fold_blocks(A, threads), threads, red, tid);
    } else if (threads >= 512) {
        fold_block<8>(A, bid - plain, threads, red, tid);
    } else {
        fold_block<4>(A, bid - plain, threads, red, tid);
    }
}
int launch_pack(const PackAll& A, hipStream_t s);
int pending_pack_leave(const PackAll& A, hipStream_t s);
bool pending_pack_take(hipStream_t s, PackAll* out);
int pending_pack_flush(hipStream_t consumer);

int launch_slot_sums(const ReduceAll& R, hipStream_t s);          // the stand-alone launch (pinnsf_reduce_kernel)
// deferred sums of the current device: leave (a second deferral first launches the one already waiting, on ITS stream),
// take (true: *out holds sums deferred on stream s, the entry is cleared), flush (launch what is waiting, if anything)
int pending_slot_sums_leave(const ReduceAll& R, hipStream_t s);
bool pending_slot_sums_take(hipStream_t s, ReduceAll* out);
int pending_slot_sums_flush();
bool pending_slot_sums_write(const float* grads);                  // deferred sums waiting that write into `grads`

}  // namespace piml
