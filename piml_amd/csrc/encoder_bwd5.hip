// Backward of the PINNSF encoder on the agents' sums of h2 (PIML_POOL_TRAIN) as TWO CREWS of four waves (round 6).
//
// Reference arithmetic: the autograd of MLP(in, [128, 128, 128]) (src/models/model.py:40-65) below the neighbour-axis sum
// (:1279-1283) with the last layer folded into the decoder:
//     G2 = g_sum[row / k] * [h2 > 0]     dW2 = G2^T H1, db2 = colsum G2        H1 = relu(W1 x + b1)
//     G1 = (G2 W2) * [h1 > 0]            dW1 = G1^T X,  db1 = colsum G1        g_x = G1 W1
//
// encoder_bwd3.hip runs this as ONE wave per SIMD (368 registers): every vector, LDS and scalar instruction of a tile is issued
// by the wave that also issues its 96 matrix instructions, a lone wave issues one instruction per four cycles whatever its
// kind, and its stamps read 8.5 k cycles per tile for 3.1 k cycles of products.  Here a workgroup is EIGHT waves, two per SIMD
// (a SIMD issues the vector instructions of two waves at twice the rate of one, and one wave's LDS / memory latency is the
// other's issue time), cut by ROLE, not by data -- the persistent state of a tile's work (weight fragments 96 registers, dW2
// accumulators 128) does not fit one wave of 256 registers, but it falls into two halves that never meet in a register:
//   crew A (waves 0-3, wave w = feature block w): the CHAIN.  Gathers g_sum of the next tile, masks it with the signs of h2,
//     splits it into bf16 pieces and lays them into the G2 image (LDS); layer B = 48 products on the W2^T fragments it holds
//     in registers for the whole slab (hi, mid AND lo: no weight traffic per tile); masks G1, lays it into the G1 tile (LDS);
//     recomputes H1 of the next tile (f32 matrix instruction) and lays its pieces into the H1 image; db2, db1.
//   crew B (waves 4-7): the WEIGHT GRADIENTS.  dW2 += G2^T H1 = 48 products from the two images into 128 accumulator
//     registers; one tile behind, from the G1 tile: dW1 (vector FMAs) and g_x (the per-wave partials through LDS, fixed
//     order).
// Every buffer between the crews is double-buffered (the x rows three deep), so a tile costs ONE workgroup barrier -- a bare
// s_barrier behind lgkmcnt(0): __syncthreads() would also wait for the loads that are in flight for the next tile.
// Everything is plain VGPRs and builtin matrix instructions (<= 256 registers: no accumulator-file operands, no asm hazards).
// Arithmetic, product order and summation order of every WEIGHT gradient are those of enc_bwd_fused_x3_kernel<..., SUMS>: the two
// kernels agree BITWISE there; g_x is the same f32 arithmetic in another summation order (f32 matrix instruction, below)
// (tests/test_sums_gpu.py::test_two_crew_backward_against_the_one_wave_kernel).
// Fragment element order, images and the slot layout: encoder_bwd3.hip / pack.hpp.
#include "common.hpp"
#include "encoder.hpp"
#include "x3.hpp"
#include "store.hpp"

namespace piml {

typedef short f5_s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) f5_s16x4 f5_lds_s16x4;

constexpr int F5_THREADS = 512;
constexpr int F5_IMG = 3 * 128 * 64;                         // one G2 image [piece 3][feature 128][row 32] bf16 = one H1 image = 24576 B
constexpr int F5_M = 0;                                      // G2 images [parity 2]
constexpr int F5_H = F5_M + 2 * F5_IMG;                      // H1 images [parity 2]: B fragments [block 4][k-step 2][piece 3][lane 64] u32x4
constexpr int F5_TROW = 36;                                  // floats per feature of the G1 tile (32 rows + 4: conflict-free both ways)
constexpr int F5_TBYTES = 128 * F5_TROW * 4;
constexpr int F5_T = F5_H + 2 * F5_IMG;                      // G1 tiles [parity 2][feature 128][36] floats
constexpr int F5_XS = F5_T + 2 * F5_TBYTES;                  // x rows [ring 3][32][8] floats
constexpr int F5_MK = F5_XS + 3 * 1024;                      // sign words of h1 [parity 2][128 dwords]
constexpr int F5_W1 = F5_MK + 2 * 512;                       // 4096 bytes: zeros, or (compact rows) the 128 floats of S, written by crew B, read by both crews
constexpr int F5_GXP = F5_W1 + 4096;                         // g_x partials [parity 2][wave 4][row 32][16] floats
constexpr int F5_GXP_BYTES = 4 * 32 * 16 * 4;                // one parity
constexpr int F5_TAB = F5_GXP + 2 * F5_GXP_BYTES;            // gather table [rem < 16][half 2][register 16] byte offsets
constexpr int F5_KMAX = 16;
constexpr int F5_LDS_BYTES = F5_TAB + F5_KMAX * 2 * 16 * 4;
constexpr int F5_LDS_LAUNCH = F5_LDS_BYTES;
static_assert(F5_LDS_LAUNCH <= 160 * 1024, "fits the CU");
constexpr int F5_PART1 = EH * EH + 1024 + 2 * EH;            // = F3_PART1 (encoder_bwd3.hip): dW2 | dW1 (1024-float field) | db2 | db1

struct F5Args {
    EncArgs A;
    int nA[2];          // workgroups of branch 0 / branch 1 (grid = their sum)
    DecSlotSums D;      // the decoder's slot sets, summed by this launch's workgroups (D.nsets = 0: left to the slot-sum launch)
};

// row_shl:C of a DPP row (16 lanes): lane i reads lane i + C
template <int C>
__device__ __forceinline__ float f5_row_shl(float v) {
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x100 + C, 0xf, 0xf, false));
}
// lane 0 of the row: s (its own chain 0) += the chains of lanes 1 .. 15, in that order
template <int C>
__device__ __forceinline__ void f5_chains_add(float4& s, const float4 v) {
    if constexpr (C < 16) {
        slot_chains_add(s, make_float4(f5_row_shl<C>(v.x), f5_row_shl<C>(v.y), f5_row_shl<C>(v.z), f5_row_shl<C>(v.w)));
        f5_chains_add<C + 1>(s, v);
    }
}
// The decoder sets' slot sums (pack.hpp: slot_chains, the summation order of the slot-sum launch): workgroup wg of nwg owns float4
// columns [wg per, (wg + 1) per) of the sets' concatenation; thread t of nthr takes chain t & 15 of columns t >> 4 and t >> 4 +
// nthr / 16 of every round of nthr / 8 columns (all 16 loads in flight: at cfg3 one round for crew A), so the 16 chains of a
// column are one DPP row and meet in its lane 0 without LDS.
__device__ __forceinline__ void f5_dec_sums(const DecSlotSums& D, int wg, int nwg, int t, int nthr) {
    const int total = D.nsets * D.lanes, per = (total + nwg - 1) / nwg;
    const int e1 = min(wg * per + per, total), half = nthr >> 4;
    for (int e = wg * per + (t >> 4); e < e1; e += 2 * half) {          // (the 16 lanes of a row share e: a row is active or not)
        const bool two = e + half < e1;
        const int ea = e, eb = two ? e + half : e;
        const int sa = ea >= D.lanes ? 1 : 0, sb = eb >= D.lanes ? 1 : 0;
        const float4* const p[2] = {reinterpret_cast<const float4*>(sa ? D.parts[1] : D.parts[0]),
                                    reinterpret_cast<const float4*>(sb ? D.parts[1] : D.parts[0])};
        const int j[2] = {ea - sa * D.lanes, eb - sb * D.lanes};
        float4 s[2];
        slot_chains<2>(p, D.slots, D.lanes, j, t & 15, s);
        const float4 va = s[0], vb = s[1];
        f5_chains_add<1>(s[0], va);
        f5_chains_add<1>(s[1], vb);
        if ((t & 15) == 0) {
            slot_sum_store(reinterpret_cast<float4*>(sa ? D.grads[1] : D.grads[0]) + j[0], s[0], D.accumulate != 0);
            if (two) slot_sum_store(reinterpret_cast<float4*>(sb ? D.grads[1] : D.grads[0]) + j[1], s[1], D.accumulate != 0);
        }
    }
}

#ifdef PIML_F5_STAMPS
// diagnostic build only (tools/f5_stamps.py): cycles between the stamps of every wave, summed over the workgroup's tiles
__device__ unsigned long long g_f5_stamps[256 * 8 * 16];      // [workgroup][wave 8][stamp 16]
#define F5_STAMP(i)                                                        \
    do {                                                                   \
        __builtin_amdgcn_sched_barrier(0);                                 \
        {                                                                  \
            const unsigned long long t_ = __builtin_amdgcn_s_memtime();    \
            st[i] += t_ - tprev;                                           \
            tprev = t_;                                                    \
        }                                                                  \
        __builtin_amdgcn_sched_barrier(0);                                 \
    } while (0)
#else
#define F5_STAMP(i)
#endif

// the workgroup barrier of the tile loop: this wave's LDS operations done, nothing said about its loads in flight
#define F5_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

__device__ __forceinline__ float f5_relu(float x) { return __int_as_float(max(__float_as_int(x), 0)); }
__device__ __forceinline__ constexpr int f5_rho(int r) { return (r & 3) + 8 * (r >> 2); }      // row of accumulator register r in lane half 0 (half 1: + 4)

#define F5_SLOT(MF, FILL)                        \
    do {                                         \
        MF;                                      \
        __builtin_amdgcn_sched_barrier(0);       \
        FILL;                                    \
        __builtin_amdgcn_sched_barrier(0);       \
    } while (0)

// INC: the columns of x the vector loops run over -- 6 when in_dim == 6 (every PINNSF encoder of the reference:
// ped_feature_dim = obs_feature_dim = 6, src/main.py:60-62), else 8 (in_dim <= 8, padded with zeros)
// CP: compact rows (piml_encoder_branch.plan of branch 1; the plan, its tiles and the constants of the zero row: encoder_x3.hip /
// pack.hpp).  The split of the grid between the branches, the tiles of branch 1 and the agents behind their rows come from the plan
// the forward left; the agents WITHOUT a neighbour -- k identical zero rows each, G2 = g_sum[agent] * [h2c > 0] on every one -- enter
// in closed form behind the tile loop: with S = k * (sum of g_sum over the workgroup's share of them) * [h2c > 0],
//     dW2 += S (x) h1c      db2 += S      db1 += (W2^T S) * [h1c > 0]      dW1 += 0 (their x is zero)
// in a fixed order (share = agents e = bx, bx + nwg, ... of empty_of, lane half h the even / odd ones of them; dW2's accumulators
// START from S (x) h1c), and their rows of g_x
// are not written (the relative-feature backward reads no row whose index is negative).
// CPM: 0 = no plan; 1 / 2 = a workgroup of branch 0 / 1 of a launch with one (two copies of the body in that kernel: the compact
// requests beside the dense ones in ONE copy cost more registers than a wave has)
template <bool GX, int INC, int CPM>
__device__ __forceinline__ void enc_bwd_sums2_body(const F5Args& F) {
    constexpr bool CP = CPM != 0;
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int crew = wv >> 2, w = wv & 3;                     // waves w and w + 4 share a SIMD
    const int ctid = tid & 255;                               // thread index within the crew
    const int n = lane & 31, h = lane >> 5;
    int bx = (int)blockIdx.x, b = 0;
    const int* __restrict__ plan = CP ? F.A.br[1].plan : nullptr;
    int nA0 = F.nA[0], nA1 = F.nA[1], nne = 0, nemp = 0, ctiles = 0;
    if (CP) {
        nne = __builtin_amdgcn_readfirstlane(plan[0]); nemp = __builtin_amdgcn_readfirstlane(plan[1]);
        ctiles = __builtin_amdgcn_readfirstlane(plan[2]);
        nA0 = __builtin_amdgcn_readfirstlane(plan[3]); nA1 = __builtin_amdgcn_readfirstlane(plan[4]);
    }
    if (CPM == 2 || (CPM == 0 && bx >= nA0)) { b = 1; bx -= nA0; }
    const piml_encoder_branch J = b ? F.A.br[1] : F.A.br[0];
    const int nwg = b ? nA1 : nA0;
    constexpr bool cp = CPM == 2;                              // this workgroup's tiles are compact
    const bool cpe = cp && nemp > 0;                           // ... and it has a share of the agents without a neighbour
    const unsigned R = (unsigned)J.rows;                      // rows < 2^22 (checked on the host): byte offsets fit 32 bits
    const unsigned IN = __builtin_amdgcn_readfirstlane((unsigned)J.in_dim), K = __builtin_amdgcn_readfirstlane((unsigned)J.k);
    const unsigned kmagic = __builtin_amdgcn_readfirstlane((unsigned)((0x100000000ull + K - 1) / K));      // row / K == umulhi(row, kmagic)
    const int ntiles = cp ? ctiles : (int)((R + 31) >> 5);
    const int nit = bx < ntiles ? (ntiles - bx + nwg - 1) / nwg : 0;      // tiles of this workgroup: bx, bx + nwg, ...
    float* P = J.partials + (size_t)bx * F5_PART1;
    constexpr int NS = INC == 6 ? 3 : 4;                      // column pairs of x

    // Buffer resources: an offset past the range reads as zero / is not stored (rows and tiles past the end cost no branch)
    auto rsrc = [&](const void* base, unsigned bytes) {
        return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, 0x00020000);
    };
    constexpr unsigned kOut = 0x80000000u;       // (+ a table offset: no wrap)
    const __amdgpu_buffer_rsrc_t rs_gp = rsrc(J.g_pooled, (R / K) * EH * 4);
    const __amdgpu_buffer_rsrc_t rs_x = rsrc(J.x, R * IN * 4);
    const __amdgpu_buffer_rsrc_t rs_mk = rsrc(J.relu_mask, (unsigned)ntiles * 1024);
    const __amdgpu_buffer_rsrc_t rs_gx = rsrc(J.g_x, GX ? R * IN * 4 : 0u);
    const unsigned cS = CP ? 32u / K : 1u;                     // agents of a compact tile
    const __amdgpu_buffer_rsrc_t rs_pl = rsrc(CP ? plan + CP_LISTS : nullptr, CP ? (unsigned)nne * 4u : 0u);      // agent_of
    auto ld1 = [&](const __amdgpu_buffer_rsrc_t& rs, unsigned voff, unsigned soff) {
        return (unsigned)__builtin_amdgcn_raw_buffer_load_b32(rs, (int)voff, (int)soff, 0);
    };

#ifdef PIML_F5_STAMPS
    unsigned long long st[16], tprev = __builtin_amdgcn_s_memtime();
#pragma unroll
    for (int i = 0; i < 16; ++i) st[i] = 0;
#endif

    // ---- LDS: the buffers the lagging work of the first iterations reads must hold zeros; the gather table ----
    {
        float4* z = reinterpret_cast<float4*>(smem + F5_T);
        constexpr int NZ = (F5_W1 - F5_T) / 16;               // G1 tiles | x ring | sign words
#pragma unroll
        for (int i = 0; i < (NZ + F5_THREADS - 1) / F5_THREADS; ++i)
            if (i * F5_THREADS + tid < NZ) z[i * F5_THREADS + tid] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int i = 0; i < 2 * F5_GXP_BYTES / 16 / F5_THREADS; ++i) reinterpret_cast<float4*>(smem + F5_GXP)[i * F5_THREADS + tid] = make_float4(0.f, 0.f, 0.f, 0.f);
        // agent of tile row m relative to the tile's first agent: (rem + m) / K with rem = (32 tile) % K; entry = byte offset of
        // that agent's 512-byte row of g_sum; register r of lane half hh holds row rho(r) + 4 hh
        if ((unsigned)tid < K * 32u) {
            const unsigned rem = (unsigned)tid >> 5, hh = ((unsigned)tid >> 4) & 1u, r = (unsigned)tid & 15u;
            reinterpret_cast<unsigned*>(smem + F5_TAB)[tid] = ((rem + 4u * hh + (unsigned)f5_rho((int)r)) / K) * (EH * 4);
        }
        if (tid < 256) reinterpret_cast<float4*>(smem + F5_W1)[tid] = make_float4(0.f, 0.f, 0.f, 0.f);      // (read only in the compact copy, behind crew B's S)
    }

    if (crew == 0) {
        // =================================================== crew A: the chain ===================================================
        // W2^T fragments of block w, all eight k-blocks, three pieces: 96 registers for the whole slab
        u32x4 wh[8], wm[8], wl[8];
        {
            const u32x4* imgB = reinterpret_cast<const u32x4*>(J.packed + PACK_F32 + 3 * X3_IMG) + lane;
#pragma unroll
            for (int kb = 0; kb < 8; ++kb) {
                const int fb = w * 8 + kb;
                wh[kb] = imgB[(fb * 2) * 64];
                wm[kb] = imgB[(fb * 2 + 1) * 64];
                wl[kb] = imgB[X3_HM / 4 + fb * 64];
            }
        }
        const float* W1rows = J.packed + PACK_FWD + 32768;
        float w1v[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) w1v[s] = W1rows[(32 * w + n) * 8 + 2 * s + h];
        const float b1v = J.b1[32 * w + n];

        // ---- per-lane LDS addresses (encoder_bwd3.hip) ----
        const int fw = 32 * w + n;
        const int swz_w = (fw >> 1) & 7;
        const int mw_off = F5_M + fw * 64;                     // writer of the G2 image: feature fw, chunk c at slot (c ^ swz_w)
        int mr[2];                                             // reader (ds_read_b64_tr_b16): + kb * 1024 + piece * 8192
        {
            const int g16 = lane >> 4, q = (lane >> 2) & 3, pp = lane & 3, hh = g16 >> 1;
            const int chunk = 4 * (g16 & 1) + pp;
#pragma unroll
            for (int half2 = 0; half2 < 2; ++half2)
                mr[half2] = F5_M + (8 * half2 + 4 * hh + q) * 64 + ((chunk ^ (4 * half2 + 2 * hh + (q >> 1))) * 8);
        }
        // sign words of h1: lane (n, h), register r needs bit bp of word (w >> 1) of source lane rho(r) + 4 h + 32 h', h' = (n >> 2) & 1
        const int bp = 16 * (w & 1) + (n & 3) + 4 * (n >> 3);
        const int mk_off = F5_MK + ((4 * h + 32 * ((n >> 2) & 1)) * 2 + (w >> 1)) * 4;
        const int t_off = F5_T + fw * (F5_TROW * 4) + (4 * h) * 4;       // + parity * F5_TBYTES + 32 g: rows 8 g + 4 h .. + 3
        const int h_off = F5_H + ((w * 2) * 3 * 64 + lane) * 16;         // + parity * F5_IMG + ((s * 3 + piece) * 64) * 16
        const unsigned gbase = (unsigned)(32 * w + n) * 4u;              // this lane's feature within a row of g_sum

        // requests of a tile: g_sum rows through the table (16 loads), the lane's sign word of h2, its x values for H1, and
        // (threads 0 .. 127 of the crew) the tile's sign words of h1
        float g2[16];
        unsigned m2 = 0, mkv = 0;
        float xa[NS];
        // (every offset that must be range-checked travels in the VECTOR offset: the scalar offset of a buffer access is not part
        // of the check)
        // compact tiles: the agent behind row n of the tile requested NEXT (-1: a dead row), fetched one request ahead
        const unsigned slot_n = CP ? (unsigned)n / K : 0u, kn = (unsigned)n - slot_n * K;
        int av = -1;
        auto plan_req = [&](int tile) {
            const unsigned idx = cS * (unsigned)tile + slot_n;
            const bool ok = (tile < ntiles) & (slot_n < cS) & (idx < (unsigned)nne);
            const unsigned v = ld1(rs_pl, ok ? idx * 4u : kOut, 0u);
            av = ok ? (int)v : -1;
        };
        auto req_g = [&](int tile) {
            if (CP && cp) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int sa = __builtin_amdgcn_readlane(av, f5_rho(r)), sb = __builtin_amdgcn_readlane(av, f5_rho(r) + 4);
                    const int a_ = h ? sb : sa;
                    g2[r] = __uint_as_float(ld1(rs_gp, a_ >= 0 ? gbase + (unsigned)a_ * (EH * 4) : kOut, 0u));
                }
                m2 = ld1(rs_mk, tile < ntiles ? (unsigned)tile * 1024u + (128u + 2u * (unsigned)lane + (unsigned)(w >> 1)) * 4u : kOut, 0u);
                return;
            }
            const unsigned t32 = __builtin_amdgcn_readfirstlane((unsigned)tile * 32u);
            const unsigned a0 = __builtin_amdgcn_readfirstlane(__umulhi(t32, kmagic)), rem = t32 - a0 * K;
            const bool live = tile < ntiles;
            const unsigned gb = live ? gbase + a0 * (EH * 4) : kOut;      // (an agent past the end is out of the resource's range)
            const uint4* tab = reinterpret_cast<const uint4*>(smem + F5_TAB + (rem * 32u + 16u * (unsigned)h) * 4u);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint4 o = tab[i];
                g2[4 * i + 0] = __uint_as_float(ld1(rs_gp, gb + o.x, 0u));
                g2[4 * i + 1] = __uint_as_float(ld1(rs_gp, gb + o.y, 0u));
                g2[4 * i + 2] = __uint_as_float(ld1(rs_gp, gb + o.z, 0u));
                g2[4 * i + 3] = __uint_as_float(ld1(rs_gp, gb + o.w, 0u));
            }
            m2 = ld1(rs_mk, live ? (unsigned)tile * 1024u + (128u + 2u * (unsigned)lane + (unsigned)(w >> 1)) * 4u : kOut, 0u);
        };
        auto req_x = [&](int tile) {
            const unsigned row = (CP && cp) ? (unsigned)av * K + kn : (unsigned)tile * 32u + (unsigned)n;
            const bool valid = (CP && cp) ? av >= 0 : (tile < ntiles) & (row < R);
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const unsigned cx = 2u * s + h;
                xa[s] = __uint_as_float(ld1(rs_x, (valid & (cx < IN)) ? (row * IN + cx) * 4u : kOut, 0u));
            }
            mkv = ld1(rs_mk, tile < ntiles ? (unsigned)tile * 1024u + (unsigned)(ctid & 127) * 4u : kOut, 0u);
            if (CP && cp) plan_req(tile + nwg);               // (the requests come in tile order: bx, bx + nwg, ...)
        };
        // G2 of the requested tile = g2 * [h2 > 0] -> db2 -> bf16 pieces -> image `pm`; 16 steps (k-step s = j >> 3)
        float db1 = 0.f, db2 = 0.f;
        unsigned phi[4], pmid[4], plo[4];
        float sp_ra = 0.f, sp_rb = 0.f;
        auto split_a = [&](float a_, float b_, unsigned& hi) {
            hi = bf16_pair(a_, b_);
            sp_ra = a_ - __uint_as_float(hi << 16);
            sp_rb = b_ - __uint_as_float(hi & 0xffff0000u);
        };
        auto split_b = [&](unsigned& mid, unsigned& lo) {
            mid = bf16_pair(sp_ra, sp_rb);
            lo = bf16_pair(sp_ra - __uint_as_float(mid << 16), sp_rb - __uint_as_float(mid & 0xffff0000u));
        };
        auto g2_step = [&](int j, int pm) {
            const int s = j >> 3, q = j & 7;
            if (q < 2) {
                const unsigned m2w = m2 >> (16 * (w & 1));
#pragma unroll
                for (int r = 8 * s + 4 * q; r < 8 * s + 4 * q + 4; ++r) {
                    const int t = __builtin_amdgcn_sbfe(m2w, r, 1);
                    g2[r] = __uint_as_float(__float_as_uint(g2[r]) & (unsigned)t);
                    db2 += g2[r];
                }
            } else if (q < 6) {
                const int d = q - 2;
                split_a(g2[8 * s + 2 * d], g2[8 * s + 2 * d + 1], phi[d]);
                split_b(pmid[d], plo[d]);
            } else {
                const int g = 2 * s + (q - 6), d = 2 * (g & 1);
                unsigned char* dst = smem + mw_off + pm * F5_IMG + (((2 * g + h) ^ swz_w) * 8);
                *reinterpret_cast<uint2*>(dst) = make_uint2(phi[d], phi[d + 1]);
                *reinterpret_cast<uint2*>(dst + 8192) = make_uint2(pmid[d], pmid[d + 1]);
                *reinterpret_cast<uint2*>(dst + 16384) = make_uint2(plo[d], plo[d + 1]);
            }
        };
        // H1 = relu(W1 x + b1) of the requested tile -> pieces -> image `pm`; h1_mma, then 10 steps (k-step s = j / 5)
        f32x16 hacc;
        auto h1_mma = [&]() {
#pragma unroll
            for (int r = 0; r < 16; ++r) hacc[r] = b1v;
#pragma unroll
            for (int s = 0; s < NS; ++s) hacc = mfma32(xa[s], w1v[s], hacc);
        };
        auto h1_step = [&](int j, int pm) {
            const int s = j / 5, q = j % 5;
            if (q < 4) {
                split_a(f5_relu(hacc[8 * s + 2 * q]), f5_relu(hacc[8 * s + 2 * q + 1]), phi[q]);
                split_b(pmid[q], plo[q]);
            } else {
                u32x4* dst = reinterpret_cast<u32x4*>(smem + h_off + pm * F5_IMG + (s * 3 * 64) * 16);
                dst[0] = (u32x4){phi[0], phi[1], phi[2], phi[3]};
                dst[64] = (u32x4){pmid[0], pmid[1], pmid[2], pmid[3]};
                dst[128] = (u32x4){plo[0], plo[1], plo[2], plo[3]};
            }
        };
        // the x values (wave s: column pair s) and the sign words of the requested tile -> LDS
        auto stage = [&](int xslot, int pm) {
            if (w < NS) reinterpret_cast<float*>(smem + F5_XS + xslot * 1024)[n * 8 + 2 * w + h] = w == 0 ? xa[0] : (w == 1 ? xa[1] : (w == 2 ? xa[2] : xa[NS - 1]));
            if (ctid < 128) reinterpret_cast<unsigned*>(smem + F5_MK + pm * 512)[ctid] = mkv;
        };
        auto load_b = [&](u32x4 (&o)[3], int kb, int pm) {
#pragma unroll
            for (int p = 0; p < 3; ++p) {
                const f5_s16x4 lo4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((f5_lds_s16x4*)(smem + mr[0] + pm * F5_IMG + kb * 1024 + p * 8192));
                const f5_s16x4 hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((f5_lds_s16x4*)(smem + mr[1] + pm * F5_IMG + kb * 1024 + p * 8192));
                const uint2 x = __builtin_bit_cast(uint2, lo4), y = __builtin_bit_cast(uint2, hi4);
                o[p] = (u32x4){x.x, x.y, y.x, y.y};
            }
        };

        F5_BARRIER();                                          // the table
        // ---- prologue: the first tile's images, the second tile's requests ----
        if (CP && cp) plan_req(bx);
        req_g(bx);
        req_x(bx);
#pragma unroll
        for (int j = 0; j < 16; ++j) g2_step(j, 0);
        h1_mma();
#pragma unroll
        for (int j = 0; j < 10; ++j) h1_step(j, 0);
        stage(0, 0);
        req_g(bx + nwg);
        req_x(bx + nwg);
        F5_STAMP(15);
        F5_BARRIER();

        for (int it = 0; it < nit; ++it) {
            const int par = it & 1, tile = bx + it * nwg;
            F5_STAMP(0);
            // layer B: G1 = (G2 W2) * [h1 > 0], 48 products into one accumulator (the five small products of every k-block first,
            // the eight hi x hi on top: encoder_bwd3.hip); between them the operand loads and this tile's sign words of h1
            f32x16 acc;
            u32x4 opa[2][3], ahi[8];                          // (ahi: the activations' hi pieces, kept for the eight hi x hi products)
            unsigned mkw[16];
            const unsigned* mk1 = reinterpret_cast<const unsigned*>(smem + mk_off + par * 512);
            auto fill_a = [&](int sl) {
                if (sl < 40 && sl % 5 == 0) {                  // the next k-block's operands
                    const int kb = sl / 5 + 1;
                    if (kb < 8) load_b(opa[kb & 1], kb, par);
                    return;
                }
                if (sl == 38 || sl == 39) return;
                const int f = sl < 40 ? sl - sl / 5 - 1 : sl - 10;     // free steps: 0 .. 29 under the small products, 30 .. 37 under the hi x hi ones
                (void)it;      // (keeps the capture of a dropped branch: without it the same instructions come out in another order)
                if (f >= 30 && f < 34) {                       // this tile's sign words (late: used right behind)
#pragma unroll
                    for (int i = 4 * (f - 30); i < 4 * (f - 30) + 4; ++i) mkw[i] = mk1[2 * f5_rho(i)];
                }
            };
            load_b(opa[0], 0, par);
            const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kb = 0; kb < 8; ++kb) {
                const u32x4 (&o)[3] = opa[kb & 1];
                ahi[kb] = o[0];
                F5_SLOT(acc = mfma_bf(o[2], wh[kb], kb == 0 ? zero16 : acc), fill_a(kb * 5 + 0));
                F5_SLOT(acc = mfma_bf(o[1], wm[kb], acc), fill_a(kb * 5 + 1));
                F5_SLOT(acc = mfma_bf(o[0], wl[kb], acc), fill_a(kb * 5 + 2));
                F5_SLOT(acc = mfma_bf(o[1], wh[kb], acc), fill_a(kb * 5 + 3));
                F5_SLOT(acc = mfma_bf(o[0], wm[kb], acc), fill_a(kb * 5 + 4));
            }
#pragma unroll
            for (int kb = 0; kb < 8; ++kb) F5_SLOT(acc = mfma_bf(ahi[kb], wh[kb], acc), fill_a(40 + kb));
            F5_STAMP(1);
            // G1: mask, db1, the lane's 16 rows of its feature -> the G1 tile
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int t = __builtin_amdgcn_sbfe(mkw[r], bp, 1);
                acc[r] = __uint_as_float(__float_as_uint(acc[r]) & (unsigned)t);
                db1 += acc[r];
            }
            {
                float4* dst = reinterpret_cast<float4*>(smem + t_off + par * F5_TBYTES);
#pragma unroll
                for (int g = 0; g < 4; ++g) dst[2 * g] = make_float4(acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]);
            }
            F5_STAMP(2);
            // the vector half of the tile, while crew B's products hold the matrix pipe: the NEXT tile's H1 (its three f32
            // products first: they queue behind crew B's) and G2 images, the requests of the tile after it
            h1_mma();
#pragma unroll
            for (int j = 0; j < 16; ++j) g2_step(j, par ^ 1);
            F5_STAMP(6);
#pragma unroll
            for (int j = 0; j < 10; ++j) h1_step(j, par ^ 1);
            F5_STAMP(7);
            stage((it + 1) % 3, par ^ 1);
            req_g(tile + 2 * nwg);
            req_x(tile + 2 * nwg);
            F5_STAMP(5);
            F5_BARRIER();
        }
        F5_STAMP(3);
        // the decoder slot sums: crew A alone, while crew B works on the last tile and stores its slot (crew A only waits there)
        if (F.D.nsets > 0) {
            f5_dec_sums(F.D, (int)blockIdx.x, (int)gridDim.x, ctid, 256);
            F5_STAMP(12);
        }
        // compact rows: db2 += S, db1 += (W2^T S) * [h1c > 0] -- the lane half's 64 terms in order, the halves added (S: crew B's
        // prologue left it in LDS)
        if (CP && cpe) {
            const float* sv = reinterpret_cast<const float*>(smem + F5_W1);
            const float* __restrict__ wc = J.w2 + (size_t)(64 * h) * EH + 32 * w + n;      // the W2 column of the lane's feature
            float pacc = 0.f;
#pragma unroll 1
            for (int q0 = 0; q0 < 64; q0 += 16) {
                float w2c[16];
#pragma unroll
                for (int q = 0; q < 16; ++q) w2c[q] = wc[(size_t)(q0 + q) * EH];
#pragma unroll
                for (int q = 0; q < 16; ++q) pacc = __fmaf_rn(w2c[q], sv[64 * h + q0 + q], pacc);
            }
            pacc += __shfl_xor(pacc, 32, 64);
            if (h == 0) {
                db1 += J.packed[PACK_ZROW + 32 * w + n] > 0.f ? pacc : 0.f;
                db2 += sv[32 * w + n];
            }
        }
        F5_BARRIER();                                          // (crew B's two trailing barriers)
        F5_BARRIER();
        db1 += __shfl_xor(db1, 32, 64);
        db2 += __shfl_xor(db2, 32, 64);
        if (h == 0) {
            P[EH * EH + 1024 + 32 * w + n] = db2;
            P[EH * EH + 1024 + EH + 32 * w + n] = db1;
        }
        for (unsigned cc = IN * 128 + ctid; cc < 1024; cc += 256) P[EH * EH + cc] = 0.f;        // the unused tail of the dW1 field
        F5_STAMP(11);
    } else {
        // =========================================== crew B: the weight gradients ===========================================
        f32x16 c[4], sm[4];
#pragma unroll
        for (int jb = 0; jb < 4; ++jb)
#pragma unroll
            for (int r = 0; r < 16; ++r) { c[jb][r] = 0.f; sm[jb][r] = 0.f; }
        float w1acc[INC];
#pragma unroll
        for (int cc = 0; cc < INC; ++cc) w1acc[cc] = 0.f;
        float w1g[8];                                          // B operand of the g_x products: W1[32 w + 4 j + (lane >> 4)][lane & 15]
        {
            const float* W1r = J.packed + PACK_FWD + 32768;     // W1 rows padded to 8 columns (zeros beyond in_dim)
#pragma unroll
            for (int j = 0; j < 8; ++j) w1g[j] = (lane & 15) < 8 ? W1r[(32 * w + 4 * j + (lane >> 4)) * 8 + (lane & 15)] : 0.f;
        }
        const int fw = 32 * w + n;
        const int swz_w = (fw >> 1) & 7;
        const int mw_off = F5_M + fw * 64;                     // this lane's own feature of the G2 image (A fragments of dW2)
        const int t_row = F5_T + fw * (F5_TROW * 4) + (4 * h) * 4;        // this lane's feature of the G1 tile, rows 4 h ..
        const int xs_off = F5_XS + (4 * h) * 32;                          // dW1: x rows 4 h ..

        auto load_g2 = [&](u32x4 (&g)[3], int s_, int pm) {
#pragma unroll
            for (int p = 0; p < 3; ++p) {
                const uint2 x = *reinterpret_cast<const uint2*>(smem + mw_off + pm * F5_IMG + p * 8192 + (((4 * s_ + h) ^ swz_w) * 8));
                const uint2 y = *reinterpret_cast<const uint2*>(smem + mw_off + pm * F5_IMG + p * 8192 + (((4 * s_ + 2 + h) ^ swz_w) * 8));
                g[p] = (u32x4){x.x, x.y, y.x, y.y};
            }
        };
        auto load_h = [&](u32x4 (&o)[3], int u_, int pm) {
            const int s_ = u_ >> 2, jb_ = u_ & 3;
            const u32x4* hr = reinterpret_cast<const u32x4*>(smem + F5_H + pm * F5_IMG) + lane;
#pragma unroll
            for (int p = 0; p < 3; ++p) o[p] = hr[((jb_ * 2 + s_) * 3 + p) * 64];
        };
        // g_x of a finished tile: the four waves' partials, fixed order; crew thread (row ctid >> 3, column ctid & 7)
        // compact tiles: the agent behind this thread's row (ctid >> 3) of the tile stored NEXT, fetched one store ahead
        const unsigned slot_m = CP ? (unsigned)(ctid >> 3) / K : 0u, km = (unsigned)(ctid >> 3) - slot_m * K;
        int bav = -1;
        auto gx_store = [&](int tile, int pm) {
            const unsigned grow = (CP && cp) ? (unsigned)bav * K + km : (unsigned)tile * 32u + (unsigned)(ctid >> 3), cs = (unsigned)ctid & 7u;
            const float* gp = reinterpret_cast<const float*>(smem + F5_GXP + pm * F5_GXP_BYTES) + (ctid >> 3) * 16 + (ctid & 7);      // [wave][row][16]: column = slot
            const float v = ((gp[0] + gp[512]) + gp[1024]) + gp[1536];
            const bool cok = cs < IN;
            const unsigned off = (grow * IN + cs) * 4u;
            const bool rok = (CP && cp) ? bav >= 0 : (tile >= 0) & (tile < ntiles) & (grow < R);
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rs_gx, (int)((rok & cok) ? off : kOut), 0, 0);
            if (CP && cp) {                                    // (the stores come in tile order: bx - 2 nwg, bx - nwg, bx, ...)
                const int nt = tile + nwg;
                const unsigned idx = cS * (unsigned)nt + slot_m;
                const bool ok = (nt >= 0) & (nt < ntiles) & (slot_m < cS) & (idx < (unsigned)nne);
                const unsigned pv = ld1(rs_pl, ok ? idx * 4u : kOut, 0u);
                bav = ok ? (int)pv : -1;
            }
        };
        // the lagging vector work on the G1 tile `pm` and x ring slot `xslot`
        float g1[16];
        float4 xv[2][4];
        auto g1_load = [&](int half_, int pm) {
            const float4* src = reinterpret_cast<const float4*>(smem + t_row + pm * F5_TBYTES);
#pragma unroll
            for (int g = 2 * half_; g < 2 * half_ + 2; ++g) {
                const float4 v = src[2 * g];
                g1[4 * g] = v.x; g1[4 * g + 1] = v.y; g1[4 * g + 2] = v.z; g1[4 * g + 3] = v.w;
            }
        };
        auto x_load = [&](int k, int xslot) {                  // rows (registers) 2 k, 2 k + 1
            const float4* xr = reinterpret_cast<const float4*>(smem + xs_off + xslot * 1024);
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                xv[k & 1][2 * e] = xr[2 * f5_rho(2 * k + e)];
                if (INC == 8) xv[k & 1][2 * e + 1] = xr[2 * f5_rho(2 * k + e) + 1];
                else {
                    const float2 t2 = *reinterpret_cast<const float2*>(&xr[2 * f5_rho(2 * k + e) + 1]);
                    xv[k & 1][2 * e + 1] = make_float4(t2.x, t2.y, 0.f, 0.f);
                }
            }
        };
        auto x_fma = [&](int k) {
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const float4 xa4 = xv[k & 1][2 * e], xb4 = xv[k & 1][2 * e + 1];
                const float g = g1[2 * k + e];
                w1acc[0] = __fmaf_rn(g, xa4.x, w1acc[0]); w1acc[1] = __fmaf_rn(g, xa4.y, w1acc[1]);
                w1acc[2] = __fmaf_rn(g, xa4.z, w1acc[2]); w1acc[3] = __fmaf_rn(g, xa4.w, w1acc[3]);
                w1acc[4] = __fmaf_rn(g, xb4.x, w1acc[4]); w1acc[5] = __fmaf_rn(g, xb4.y, w1acc[5]);
                if (INC == 8) { w1acc[INC - 2] = __fmaf_rn(g, xb4.z, w1acc[INC - 2]); w1acc[INC - 1] = __fmaf_rn(g, xb4.w, w1acc[INC - 1]); }
            }
        };
        // g_x on the f32 matrix instruction: D[row][c] = sum over the wave's 32 features of G1[row][f] W1[f][c], two chains (rows
        // 0 .. 15 / 16 .. 31) of eight products (four features each); operand A: lane (m = row & 15, k = lane >> 4) reads
        // G1[feature 4 j + k][row] from the tile, operand B: lane (k, n = column) holds W1[4 j + k][n] (0 beyond column 7)
        f32x4 gd[2];
        float ga[8][2];                                        // (all sixteen operands requested up front: 8 ds_read2_b32)
        const int ga_off = F5_T + (32 * w + (lane >> 4)) * (F5_TROW * 4) + (lane & 15) * 4;      // + 4 j features, + 16 r rows
        auto gm_load = [&](int j, int pm) {
#pragma unroll
            for (int r = 0; r < 2; ++r) ga[j][r] = *reinterpret_cast<const float*>(smem + ga_off + pm * F5_TBYTES + j * (4 * F5_TROW * 4) + r * 64);
        };
        // (these products ride between crew B's OWN products, not in its vector half: there crew A's chain of 51 dependent products
        // owns the matrix pipe -- the older wave wins the arbitration every time -- and crew B's in-order stream stood behind its
        // first g_x product for the whole of crew A's chain: 4.5 k cycles for the vector half instead of 3.5 k)
        auto gxm_step = [&](int f, int pm) {                  // 0 .. 9; pm: the G1 tile
            if (!GX) return;
            if (f == 0) {
                gd[0] = gd[1] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int j = 0; j < 8; ++j) gm_load(j, pm);
            } else if (f <= 8) {
                const int j = f - 1;
#pragma unroll
                for (int r = 0; r < 2; ++r) gd[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(ga[j][r], w1g[j], gd[r], 0, 0, 0);
            } else if (f == 9) {                              // rows 16 r + 4 (lane >> 4) + i, column lane & 15
                float* dst = reinterpret_cast<float*>(smem + F5_GXP + (pm ^ 1) * F5_GXP_BYTES) + (w * 32 + 4 * (lane >> 4)) * 16 + (lane & 15);
#pragma unroll
                for (int r = 0; r < 2; ++r)
#pragma unroll
                    for (int i = 0; i < 4; ++i) dst[(16 * r + i) * 16] = gd[r][i];
            }
        };
        auto lag_step = [&](int f, int pm, int xslot) {       // dW1: 0 .. 9 (rows two by two, loads a step ahead; step 9 is empty)
            if (f == 0) { g1_load(0, pm); g1_load(1, pm); x_load(0, xslot); }
            else if (f == 1) { x_load(1, xslot); x_fma(0); }
            else if (f < 9) { if (f < 8) x_load(f, xslot); x_fma(f - 1); }
        };

        F5_BARRIER();                                          // the table (crew A's prologue barrier)
        // compact rows, while crew A prepares the first tile: S of this workgroup's share (lane half h: every second agent of it)
        // -> LDS (the 4096 bytes at F5_W1 nothing else uses; crew A reads it behind its loop)
        if (CP && cpe) {
            const int* __restrict__ eo = plan + CP_LISTS + (((int)(R / K) + 3) & ~3);
            const float* __restrict__ gp = J.g_pooled + 32 * w + n;
            float sacc = 0.f;
            for (int e0 = bx + h * nwg; e0 < nemp; e0 += 16 * nwg) {
                int ai[8];
                float gv[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) ai[u] = eo[min(e0 + 2 * u * nwg, nemp - 1)];
#pragma unroll
                for (int u = 0; u < 8; ++u) gv[u] = gp[(size_t)ai[u] * EH];
#pragma unroll
                for (int u = 0; u < 8; ++u) sacc += e0 + 2 * u * nwg < nemp ? gv[u] : 0.f;
            }
            sacc += __shfl_xor(sacc, 32, 64);
            if (h == 0) reinterpret_cast<float*>(smem + F5_W1)[32 * w + n] = J.packed[PACK_ZROW + EH + 32 * w + n] > 0.f ? (float)K * sacc : 0.f;
        }
        F5_STAMP(15);
        F5_BARRIER();
        if (CP && cpe) {                                       // dW2 starts from S (x) h1c
            const float* sv = reinterpret_cast<const float*>(smem + F5_W1) + 32 * w + 4 * h;
#pragma unroll
            for (int jb = 0; jb < 4; ++jb) {
                const float h1v = J.packed[PACK_ZROW + 32 * jb + n];
#pragma unroll
                for (int r = 0; r < 16; ++r) c[jb][r] = sv[f5_rho(r)] * h1v;
            }
        }
        for (int it = 0; it < nit; ++it) {
            const int par = it & 1, tile = bx + it * nwg;
            F5_STAMP(0);
            // dW2 += G2^T H1: 48 products (8 groups u = 4 s + jb of six) into the slab's accumulators; between them the g_x products
            // of the tile BEFORE (its G1 tile is in the other buffer)
            u32x4 g2f[3], opb[2][3];
            const int lpm = par ^ 1, xslot = (it + 2) % 3;
            auto fill_b = [&](int sl) {
                if (sl % 6 == 0) {
                    const int u_ = sl / 6 + 1;
                    if (u_ < 8) load_h(opb[u_ & 1], u_, par);
                    return;
                }
                if (sl == 23) { load_g2(g2f, 1, par); return; }   // (behind the last product of k-step 0)
                const int f = sl - sl / 6 - 1 - (sl > 23);         // 39 free steps
                if (f == 1) gxm_step(0, lpm);
                else if (f >= 6 && f < 14) gxm_step(f - 5, lpm);
                else if (f == 22) gxm_step(9, lpm);
            };
            // the vector half first, while crew A's products hold the matrix pipe: the g_x store of the tile two back, dW1 of
            // the tile before (its x rows two ring slots back)
            if (GX) gx_store(tile - 2 * nwg, par ^ 1);
#pragma unroll
            for (int f = 0; f < 10; ++f) lag_step(f, lpm, xslot);
            F5_STAMP(6);
            F5_STAMP(5);
            load_g2(g2f, 0, par);
            load_h(opb[0], 0, par);
#pragma unroll
            for (int u = 0; u < 8; ++u) {                          // u = 4 s + jb
                const int jb = u & 3;
                const u32x4 (&o)[3] = opb[u & 1];
                F5_SLOT(sm[jb] = mfma_bf(g2f[2], o[0], sm[jb]), fill_b(u * 6 + 0));
                F5_SLOT(sm[jb] = mfma_bf(g2f[1], o[1], sm[jb]), fill_b(u * 6 + 1));
                F5_SLOT(sm[jb] = mfma_bf(g2f[0], o[2], sm[jb]), fill_b(u * 6 + 2));
                F5_SLOT(sm[jb] = mfma_bf(g2f[1], o[0], sm[jb]), fill_b(u * 6 + 3));
                F5_SLOT(sm[jb] = mfma_bf(g2f[0], o[1], sm[jb]), fill_b(u * 6 + 4));
                F5_SLOT(c[jb] = mfma_bf(g2f[0], o[0], c[jb]), fill_b(u * 6 + 5));
            }
            F5_STAMP(1);
            F5_BARRIER();
        }
        F5_STAMP(3);
        // the last tile's vector work, the last two g_x stores
        {
            const int it = nit, par = it & 1, tile = bx + it * nwg;
            if (GX) gx_store(tile - 2 * nwg, par ^ 1);
#pragma unroll
            for (int f = 0; f < 10; ++f) lag_step(f, par ^ 1, (it + 2) % 3);
#pragma unroll
            for (int f = 0; f < 10; ++f) gxm_step(f, par ^ 1);
            F5_BARRIER();
            if (GX) gx_store(tile - nwg, par);
            F5_BARRIER();
        }
        F5_STAMP(4);
        // ---- the slot: dW2 | dW1 ----
        // (store.hpp: written through -- the slot is this workgroup's last action, all of it would be dirty in the XCD's L2 when
        // the launch ends, and its readers are the slot sums of the NEXT launch)
#pragma unroll
        for (int jb = 0; jb < 4; ++jb)
            store_acc32<PIML_WT_ENC_BWD_SLOTS>(P + (size_t)(32 * w) * EH + 32 * jb, EH, lane, [&](int r) { return c[jb][r] + sm[jb][r]; });
#pragma unroll
        for (int cc = 0; cc < INC; ++cc) w1acc[cc] += __shfl_xor(w1acc[cc], 32, 64);
        if (h == 0) {
            float* o = P + EH * EH + (size_t)(32 * w + n) * IN;
#pragma unroll
            for (int cc = 0; cc < INC; ++cc)
                if ((unsigned)cc < IN) o[cc] = w1acc[cc];
        }
        F5_STAMP(11);
    }
#ifdef PIML_F5_STAMPS
    if (lane == 0)
        for (int i = 0; i < 16; ++i) g_f5_stamps[(blockIdx.x * 8 + wv) * 16 + i] = st[i];
#endif
}
template <bool GX, int INC>
__global__ __launch_bounds__(F5_THREADS) void enc_bwd_sums2_kernel(F5Args F) { enc_bwd_sums2_body<GX, INC, 0>(F); }
template <bool GX>
__global__ __launch_bounds__(F5_THREADS) void enc_bwd_sums2_cp_kernel(F5Args F) {
    if ((int)blockIdx.x < __builtin_amdgcn_readfirstlane(F.A.br[1].plan[3])) enc_bwd_sums2_body<GX, 6, 1>(F);
    else enc_bwd_sums2_body<GX, 6, 2>(F);
}

#ifdef PIML_F5_STAMPS
extern "C" __attribute__((visibility("default"))) int piml_f5_stamps(unsigned long long* out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_f5_stamps), sizeof(unsigned long long) * 256 * 8 * 16);
}
#endif

int enc_f5_set_attributes() {
    auto set = [&](const void* f) { return (int)hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, F5_LDS_LAUNCH); };
    if (int e = set(reinterpret_cast<const void*>(enc_bwd_sums2_kernel<false, 6>))) return e;
    if (int e = set(reinterpret_cast<const void*>(enc_bwd_sums2_kernel<true, 6>))) return e;
    if (int e = set(reinterpret_cast<const void*>(enc_bwd_sums2_kernel<false, 8>))) return e;
    if (int e = set(reinterpret_cast<const void*>(enc_bwd_sums2_cp_kernel<false>))) return e;
    if (int e = set(reinterpret_cast<const void*>(enc_bwd_sums2_cp_kernel<true>))) return e;
    return set(reinterpret_cast<const void*>(enc_bwd_sums2_kernel<true, 8>));
}

// the PIML_POOL_TRAIN backward (g_pooled = the gradient of the agents' sums; checked by the caller); false: a shape this kernel
// does not take (k > 16) -- the caller launches enc_f3_launch(..., sums = true)
bool enc_f5_launch(const EncArgs& A, const int* nA, hipStream_t s, const DecSlotSums* D) {
    F5Args F;
    F.A = A;
    F.nA[0] = nA[0]; F.nA[1] = A.nbr > 1 ? nA[1] : 0;
    F.D = D ? *D : DecSlotSums{};
    bool in6 = true;
    for (int i = 0; i < A.nbr; ++i) {
        if (A.br[i].k > F5_KMAX) return false;
        in6 = in6 && A.br[i].in_dim == 6;
    }
    const bool gx = A.br[0].g_x != nullptr;
    const dim3 g((unsigned)(F.nA[0] + F.nA[1])), blk(F5_THREADS);
    if (A.nbr > 1 && A.br[1].plan) {          // compact rows (in_dim = 6 in both branches and the grid = PIML_COMPACT_SLOTS: checked by the caller)
        if (gx) hipLaunchKernelGGL((enc_bwd_sums2_cp_kernel<true>), g, blk, F5_LDS_LAUNCH, s, F);
        else hipLaunchKernelGGL((enc_bwd_sums2_cp_kernel<false>), g, blk, F5_LDS_LAUNCH, s, F);
    } else if (in6) {
        if (gx) hipLaunchKernelGGL((enc_bwd_sums2_kernel<true, 6>), g, blk, F5_LDS_LAUNCH, s, F);
        else hipLaunchKernelGGL((enc_bwd_sums2_kernel<false, 6>), g, blk, F5_LDS_LAUNCH, s, F);
    } else {
        if (gx) hipLaunchKernelGGL((enc_bwd_sums2_kernel<true, 8>), g, blk, F5_LDS_LAUNCH, s, F);
        else hipLaunchKernelGGL((enc_bwd_sums2_kernel<false, 8>), g, blk, F5_LDS_LAUNCH, s, F);
    }
    return true;
}

}  // namespace piml
