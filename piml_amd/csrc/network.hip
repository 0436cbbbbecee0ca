// The fused PINNSF network as one call per direction: the launch stages of encoder.hip / decoder.hip in as few launches
// as their data dependences allow.
//
// Replaces the body of PINNSF.forward / its autograd backward (src/models/model.py:1271-1305: ped_encoder /
// obs_encoder -> sum over neighbours -> decoders -> predictors -> desired force, and the `pinnsf_m` collision head
// :1296-1300).  Most stages of one step are small next to the chip (the decoder tails and the head work on 4096 agents,
// the packs and reductions on < 1 MB), and every dependent launch on gfx950 pays ~4.5 us for the end-of-kernel
// write-back + start-of-kernel invalidate of the eight per-XCD L2s.  Default (serial) order, one stream:
//
//   pack      ONE launch for every weight image (pinnsf_pack_kernel)                 -- skipped with PIML_PACKED_VALID
//   forward   encoders (both branches) -> [neighbour-axis sums + decoder tails + desired force + collision head]
//   backward  [decoder dX chain + dW partials] -> encoder dX -> encoder dW -> ONE slot sum for all four partial sets
//
// PIML_FORK (opt-in, measured SLOWER inside captured graphs on ROCm 7.2: every cross-stream edge of a replayed graph
// costs more than the ~5 us stage it hides) puts the independent stages on library-owned side streams instead:
//
//   forward    main:  [enc pack] -> encoders ----------------> pooling -> decoder tails -> join
//              side0: dec pack, head pack ----\                           ^
//              side1:                          \-> (after encoders) head -/
//   backward   main:  decoder dX -> encoder dX -> encoder dW ------------> join -> encoder reduction
//              side0:            \-> decoder dW -> decoder reduction ----/
//
// The side streams belong to the library (one pair per device, created on first use outside any capture).
#include <cstdio>
#include <cstdlib>
#include <mutex>

#include "common.hpp"
#include "pack.hpp"
#include "reduce.hpp"
#include "stages.hpp"
#include "trace.hpp"

namespace piml {

namespace {

struct Side {
    hipStream_t s[2] = {nullptr, nullptr};
    hipEvent_t ev[6] = {};
    bool ok = false;
};

constexpr int kMaxDevices = 64;
Side g_side[kMaxDevices];
std::mutex g_mu;

int side_streams(Side** out) {
    int dev = 0;
    if (hipError_t e = hipGetDevice(&dev)) return e;
    if (dev < 0 || dev >= kMaxDevices) return hipErrorInvalidDevice;
    std::lock_guard<std::mutex> lock(g_mu);
    Side& S = g_side[dev];
    if (!S.ok) {
        // creating streams / events is not a capturable operation: fail clearly instead of invalidating the capture
        for (auto& s : S.s)
            if (hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking)) return e;
        for (auto& ev : S.ev)
            if (hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming)) return e;
        S.ok = true;
    }
    *out = &S;
    return hipSuccess;
}

// `to` continues after everything enqueued on `from` so far
int edge(hipStream_t from, hipStream_t to, hipEvent_t ev) {
    if (hipError_t e = hipEventRecord(ev, from)) return e;
    return hipStreamWaitEvent(to, ev, 0);
}

// a failing stage names itself on stderr: the hipError_t alone does not say which of the ~10 launches refused
#define PIML_TRY(x)                                                                        \
    do {                                                                                   \
        if (int e_ = (x)) {                                                                \
            fprintf(stderr, "libpiml_hip: %s -> %d (%s:%d)\n", #x, e_, __FILE__, __LINE__); \
            return e_;                                                                     \
        }                                                                                  \
    } while (0)

}  // namespace

// ---- one launch for every weight image of the network: blockIdx.y = encoder branches, decoder branches, head (reduce.hpp) ----
__global__ __launch_bounds__(256) void pinnsf_pack_kernel(PackAll A) {
    __shared__ double red[256];
    pack_block(A, (int)blockIdx.x, 256, red, (int)threadIdx.x);
}

int launch_pack(const PackAll& A, hipStream_t s) {
    hipLaunchKernelGGL(pinnsf_pack_kernel, dim3((unsigned)pack_blocks_total(A, 256)), dim3(256), 0, s, A);
    trace_mark("pinnsf_pack", s);
    return hipGetLastError();
}

// ---- one launch for every slot sum of the backward pass (reduce.hpp): a set of slots per gx workgroups (encoder branches --
// one set each, or two with the layer-split slots of encoder_dw2.hip -- then the decoder branches) ----
// (with A.unf_blocks > 0 the unfold's workgroups lead: reduce_launch_block)
__global__ __launch_bounds__(256) void pinnsf_reduce_kernel(ReduceAll A) { reduce_launch_block(A, (int)blockIdx.x); }

int launch_slot_sums(const ReduceAll& R, hipStream_t s) {
    hipLaunchKernelGGL(pinnsf_reduce_kernel, dim3((unsigned)reduce_launch_blocks(R)), dim3(256), 0, s, R);
    return hipGetLastError();
}

// ---- PIML_POOL_TRAIN: the folded first layers' gradients -> the gradients of their factors (reduce.hpp: UnfoldSet, unfold_block) ----
// A launch of its own where the decoder sets are summed by the same slot-sum launch (it has to see their sums) and for a deferred
// unfold; otherwise the unfold's workgroups ride in the slot-sum launch.
__global__ __launch_bounds__(256) void pinnsf_unfold_kernel(ReduceAll R) { unfold_block(R, (int)(blockIdx.y * kUnfoldBlocks + blockIdx.x)); }

// (Round 5, built, parity green, measured and removed: the unfold as workgroups of the launch that sums the slots, gated by a
// device-side ticket the decoder sets' sum workgroups raise -- sums written with device-scope stores, unfold reads through LDS in
// one round of device-scope loads.  At the tail of the launch the chain [sums, ticket, uncached loads, products] ran 19 - 21 us
// against 9.4 + 4.7 as two launches; dispatched early -- right behind the decoder sets -- the 258 polling workgroups cost the
// launch more still, 33 us; an ACQUIRE in the poll invalidates the XCD's L2 on every round: 49 us.  Two launches it stays.)
static int launch_unfold_now(const ReduceAll& R, hipStream_t s) {
    if (R.nunf <= 0) return hipSuccess;
    hipLaunchKernelGGL(pinnsf_unfold_kernel, dim3(kUnfoldBlocks, (unsigned)R.nunf), dim3(256), 0, s, R);
    trace_mark("pinnsf_unfold", s);
    return hipGetLastError();
}

// ---- deferred unfold (piml_pinnsf_unfold_defer): one waiting entry per device ----
// The unfold READS the folded layers' summed gradients and OVERWRITES the unfolded ones, so of the backward passes of one optimiser
// step that accumulate into the same buffers (PIML_ACCUMULATE: the frames of a training rollout) only the LAST pass's unfold
// matters -- the earlier ones compute from partial sums what the last one computes again.  While deferring, unfold_begin records
// the sets of a pass that asked for it (PIML_DEFER_UNFOLD, carried in R through deferred slot sums) instead of launching; another
// network's sets first launch what is waiting.  A pass without the flag launches at once: its buffers are the caller's to read.
namespace {
struct PendingUnfold {
    ReduceAll R;
    hipStream_t stream = nullptr;
    bool valid = false, deferring = false;
};
PendingUnfold g_pending_unfold[kMaxDevices];
PendingUnfold* pending_unfold_entry() {
    int dev = 0;
    if (hipGetDevice(&dev) || dev < 0 || dev >= kMaxDevices) return nullptr;
    return &g_pending_unfold[dev];
}
bool same_unfold(const ReduceAll& a, const ReduceAll& b) {
    if (a.nunf != b.nunf) return false;
    for (int i = 0; i < a.nunf; ++i)
        if (a.unf[i].dgrads != b.unf[i].dgrads || a.unf[i].dw1_out != b.unf[i].dw1_out || a.unf[i].egrads != b.unf[i].egrads ||
            a.unf[i].w1 != b.unf[i].w1 || a.unf[i].w3 != b.unf[i].w3 || a.unf[i].b3 != b.unf[i].b3 || a.unf[i].k != b.unf[i].k ||
            a.unf[i].scale != b.unf[i].scale)
            return false;
    return true;
}
}  // namespace

ReduceAll unfold_begin(const ReduceAll& R, hipStream_t s, UnfoldTail* t) {
    ReduceAll out = R;
    out.unf_blocks = 0;
    t->go = false;
    if (R.nunf <= 0) return out;
    PendingUnfold* P = pending_unfold_entry();
    bool deferred = false;
    if (P) {
        std::lock_guard<std::mutex> lock(g_mu);
        if (P->deferring && R.defer_unfold) {
            if (P->valid && !same_unfold(P->R, R)) { t->R = P->R; t->stream = P->stream; t->go = true; }
            P->R = R; P->stream = s; P->valid = true;
            deferred = true;
        }
    }
    if (deferred) return out;
    if (R.dec_upstream) out.unf_blocks = R.nunf * kUnfoldBlocks;
    else { t->R = R; t->stream = s; t->go = true; }
    return out;
}

int unfold_end(const UnfoldTail& t) { return t.go ? launch_unfold_now(t.R, t.stream) : (int)hipSuccess; }

PIML_API int piml_pinnsf_unfold_defer(int on, void* stream) {
    PendingUnfold* P = pending_unfold_entry();
    if (!P) return hipErrorInvalidDevice;
    ReduceAll R;
    hipStream_t s = nullptr;
    bool go = false;
    {
        std::lock_guard<std::mutex> lock(g_mu);
        if (P->valid) { R = P->R; s = stream ? as_stream(stream) : P->stream; go = true; P->valid = false; }
        P->deferring = on != 0;
    }
    return go ? launch_unfold_now(R, s) : (int)hipSuccess;
}

// ---- deferred slot sums (PIML_DEFER_SLOT_SUMS): one waiting entry per device ----
namespace {
struct PendingSums {
    ReduceAll R;
    hipStream_t stream = nullptr;
    bool valid = false;
};
PendingSums g_pending[kMaxDevices];

PendingSums* pending_entry() {
    int dev = 0;
    if (hipGetDevice(&dev) || dev < 0 || dev >= kMaxDevices) return nullptr;
    return &g_pending[dev];
}
}  // namespace

namespace {
struct PendingPack {
    PackAll A;
    hipStream_t stream = nullptr;
    bool valid = false;
};
PendingPack g_pending_pack[kMaxDevices];
PendingPack* pending_pack_entry() {
    int dev = 0;
    if (hipGetDevice(&dev) || dev < 0 || dev >= kMaxDevices) return nullptr;
    return &g_pending_pack[dev];
}
}  // namespace

// consumer: the stream of the launch that is about to read the images (nullptr: unknown -- the stream the pack was left on).  A
// pack left on another stream than its consumer's runs on the CONSUMER's stream: there it is ordered in front of the reader
// (and inside the same capture), which the stream it was left on does not promise.
int pending_pack_flush(hipStream_t consumer) {
    PendingPack* P = pending_pack_entry();
    if (!P) return hipErrorInvalidDevice;
    PackAll A;
    hipStream_t s;
    {
        std::lock_guard<std::mutex> lock(g_mu);
        if (!P->valid) return hipSuccess;
        A = P->A; s = P->stream; P->valid = false;
    }
    return launch_pack(A, consumer ? consumer : s);
}

int pending_pack_leave(const PackAll& A, hipStream_t s) {
    if (int e = pending_pack_flush(nullptr)) return e;
    PendingPack* P = pending_pack_entry();
    if (!P) return hipErrorInvalidDevice;
    std::lock_guard<std::mutex> lock(g_mu);
    P->A = A; P->stream = s; P->valid = true;
    return hipSuccess;
}

bool pending_pack_take(hipStream_t s, PackAll* out) {
    PendingPack* P = pending_pack_entry();
    if (!P) return false;
    std::lock_guard<std::mutex> lock(g_mu);
    if (!P->valid || P->stream != s) return false;
    *out = P->A;
    P->valid = false;
    return true;
}

int pending_slot_sums_flush() {
    PendingSums* P = pending_entry();
    if (!P) return hipErrorInvalidDevice;
    ReduceAll R;
    hipStream_t s;
    {
        std::lock_guard<std::mutex> lock(g_mu);
        if (!P->valid) return hipSuccess;
        R = P->R; s = P->stream; P->valid = false;
    }
    UnfoldTail t;
    if (int e = launch_slot_sums(unfold_begin(R, s, &t), s)) return e;
    trace_mark("pinnsf_reduce", s);
    return unfold_end(t);
}

bool pending_slot_sums_write(const float* grads) {
    PendingSums* P = pending_entry();
    if (!P) return false;
    std::lock_guard<std::mutex> lock(g_mu);
    for (int i = 0; P->valid && i < P->R.nsets; ++i)
        if (P->R.set[i].grads == grads) return true;
    return false;
}

int pending_slot_sums_leave(const ReduceAll& R, hipStream_t s) {
    PendingSums* P = pending_entry();
    if (!P) return hipErrorInvalidDevice;
    {
        // Sums of ANOTHER operator of the same backward pass waiting on this stream (the bottleneck variants: row decoder, then
        // encoders, piml_rowdecoder_bwd_acc / piml_encoder_bwd_acc with PIML_DEFER_SLOT_SUMS): the two descriptions become one
        // launch -- when they fit, accumulate alike, carry no unfold, and write DIFFERENT gradient buffers (the same buffer twice
        // is a second pass over the same parameters: its predecessor has to run first).
        std::lock_guard<std::mutex> lock(g_mu);
        ReduceAll& Q = P->R;
        bool merge = P->valid && P->stream == s && Q.accumulate == R.accumulate && Q.nunf == 0 && R.nunf == 0 &&
                     Q.nsets + R.nsets <= (int)(sizeof(Q.set) / sizeof(Q.set[0]));
        for (int i = 0; merge && i < Q.nsets; ++i)
            for (int j = 0; j < R.nsets; ++j)
                if (Q.set[i].grads == R.set[j].grads) { merge = false; break; }
        if (merge) {
            for (int j = 0; j < R.nsets; ++j) Q.set[Q.nsets++] = R.set[j];
            if (R.gx > Q.gx) Q.gx = R.gx;
            return hipSuccess;
        }
    }
    if (int e = pending_slot_sums_flush()) return e;          // sums already waiting: they run now, on the stream they were left on
    std::lock_guard<std::mutex> lock(g_mu);
    P->R = R; P->stream = s; P->valid = true;
    return hipSuccess;
}

bool pending_slot_sums_take(hipStream_t s, ReduceAll* out) {
    PendingSums* P = pending_entry();
    if (!P) return false;
    std::lock_guard<std::mutex> lock(g_mu);
    if (!P->valid || P->stream != s) return false;
    *out = P->R;
    P->valid = false;
    return true;
}

}  // namespace piml

using namespace piml;

PIML_API int piml_pinnsf_streams_init(void) {
    Side* S;
    return side_streams(&S);
}

// One launch on `stream`.  (Not forked internally: a fork nested inside a caller's forked stream crashed
// hipStreamEndCapture on ROCm 7.2, tools/probe_capture_fork.py.)
PIML_API int piml_pinnsf_pack(const piml_encoder_branch* enc, const piml_decoder_branch* dec, int nbr,
                              const piml_collision_head* head, int flags, void* stream) {
    if (!enc || !dec || nbr < 1 || nbr > 2) return hipErrorInvalidValue;
    PackAll A = {};
    A.nbr = nbr;
    A.has_head = head != nullptr;
    A.skip_f32 = enc_f32_images_needed() ? 0 : 1;
    for (int i = 0; i < nbr; ++i) {
        const piml_encoder_branch& e = enc[i];
        const piml_decoder_branch& d = dec[i];
        if (e.in_dim < 1 || e.in_dim > 8 || !e.w1 || !e.b1 || !e.w2 || !e.b2 || !e.w3 || !e.b3 || !e.packed || !d.w1 || !d.b1 ||
            !d.w2 || !d.b2 || !d.w3 || !d.b3 || !d.packed)
            return hipErrorInvalidValue;
        A.enc[i] = e;
        A.dec[i] = d;
    }
    if (head) {
        if (!head->w1 || !head->b1 || !head->w2 || !head->b2 || !head->packed) return hipErrorInvalidValue;
        A.head = *head;
        if (head->fold_w3) {
            if (!head->fold_b3) return hipErrorInvalidValue;
            A.has_fold = 1;
        }
    }
    for (int i = 0; i < nbr; ++i)
        if (dec[i].fold_w3) {
            if (!dec[i].fold_b3) return hipErrorInvalidValue;
            A.has_fold = 1;
        }
    if (flags & PIML_DEFER_PACK) return pending_pack_leave(A, as_stream(stream));      // the next relfeat forward on `stream` runs it
    return launch_pack(A, as_stream(stream));
}

PIML_API int piml_pinnsf_pack_flush(void) { return pending_pack_flush(nullptr); }

// every slot sum of the backward pass (encoder + decoder partials) in one launch on `s`; dec_summed: the decoder sets were summed
// by the encoder backward (PIML_POOL_TRAIN, encoder_bwd5.hip) -- left out here, and the unfold's workgroups ride in this launch
static int reduce_all(const piml_encoder_branch* enc, const piml_decoder_branch* dec, int nbr, hipStream_t s, bool accumulate, bool defer = false,
                      bool sums = false, bool defer_unfold = false, bool dec_summed = false) {
    ReduceAll R = {};
    R.accumulate = accumulate ? 1 : 0;
    R.defer_unfold = defer_unfold ? 1 : 0;
    R.dec_upstream = dec_summed ? 1 : 0;
    int w0 = 0, n = 0, maxl = 0;
    const int total = piml_encoder_workgroups(enc, nbr, &w0);
    const int dslots = piml_decoder_workgroups(dec[0].agents);
    int n0[2] = {0, 0}, n1[2] = {0, 0};
    const bool dw2 = !sums && enc_dw2_used(enc, nbr, n0, n1);
    auto add = [&](const float* parts, float* grads, int slots, int lanes, int split, int off0, int off1) {
        R.set[n++] = ReduceSet{parts, grads, slots, lanes, split, off0, off1};
        if (lanes > maxl) maxl = lanes;
    };
    for (int i = 0; i < nbr; ++i) {
        if (sums) {          // PIML_POOL_TRAIN: one layer-1 slot (dW2 | dW1 | db2 | db1) per workgroup; dW3 / db3 come from the unfold
            add(enc[i].partials, enc[i].grads, nbr == 1 ? total : (i == 0 ? w0 : total - w0), DW2_L1_LANES, DW2_L1_SPLIT, DW2_L1_OFF0, DW2_L1_OFF1);
            // compact rows: the backward's split follows the plan (ints 3 / 4: the workgroups = slots of branch 0 / 1), so the sums read it
            if (nbr == 2 && enc[1].plan) R.set[n - 1].dev_slots = enc[1].plan + 3 + i;
            R.unf[i] = UnfoldSet{dec[i].grads, dec[i].w1, enc[i].w3, enc[i].b3, dec[i].fold_scale, enc[i].k, dec[i].dw1_out, enc[i].grads};
            R.nunf = nbr;
        } else if (dw2) {
            add(enc[i].partials, enc[i].grads, n0[i], DW2_L0_LANES, DW2_L0_SPLIT, 0, DW2_L0_OFF1);
            add(enc[i].partials + (size_t)n0[i] * (DW2_L0_LANES * 4), enc[i].grads, n1[i], DW2_L1_LANES, DW2_L1_SPLIT, DW2_L1_OFF0, DW2_L1_OFF1);
        } else {
            add(enc[i].partials, enc[i].grads, nbr == 1 ? total : (i == 0 ? w0 : total - w0), ENC_PART / 4, 0x7fffffff, 0, 0);
        }
    }
    if (!dec_summed)
        for (int i = 0; i < nbr; ++i) add(dec[i].partials, dec[i].grads, dslots, DEC_PART / 4, 0x7fffffff, 0, 0);
    R.nsets = n;
    R.gx = (maxl + 15) / 16;
    if (defer) return pending_slot_sums_leave(R, s);          // the next piml_relfeat_self_bwd on `s` (or a flush) runs them
    UnfoldTail t;
    if (int e = launch_slot_sums(unfold_begin(R, s, &t), s)) return e;
    trace_mark("pinnsf_reduce", s);
    return unfold_end(t);
}

// Decoder slot sets of the PIML_POOL_TRAIN backward: 1 (default) = summed by the two-crew encoder backward's workgroups (the next
// launch boundary publishes them, and the unfold rides in the slot-sum launch); 0 = by the slot-sum launch, the unfold a launch of
// its own behind it.  PIML_ENC_DEC_SLOTS=0 / 1 at load time
static int g_dec_slots_enc = !(getenv("PIML_ENC_DEC_SLOTS") && atoi(getenv("PIML_ENC_DEC_SLOTS")) == 0);

PIML_API int piml_encoder_sums_dec_slots(int on) {
    const int old = g_dec_slots_enc;
    if (on >= 0) g_dec_slots_enc = on ? 1 : 0;
    return old;
}

// Compact rows on the PIML_POOL_TRAIN path (piml_encoder_branch.nbr_idx / plan): what piml_amd.ops asks before it sets the pointers.
// PIML_ENC_COMPACT=0 / 1 at load time
static int g_compact_rows = !(getenv("PIML_ENC_COMPACT") && atoi(getenv("PIML_ENC_COMPACT")) == 0);

PIML_API int piml_encoder_compact_rows(int on) {
    const int old = g_compact_rows;
    if (on >= 0) g_compact_rows = on ? 1 : 0;
    return old;
}

PIML_API int piml_pinnsf_slot_sums_flush(void) { return pending_slot_sums_flush(); }

PIML_API int piml_pinnsf_pool_h2_ok(const piml_encoder_branch* enc, int nbr) { return enc_pool_h2_ok(enc, nbr) ? 1 : 0; }
PIML_API int piml_pinnsf_pool_train_ok(const piml_encoder_branch* enc, int nbr) { return enc_pool_train_ok(enc, nbr) ? 1 : 0; }
PIML_API int piml_pinnsf_pool_msgs_ok(const piml_encoder_branch* enc, int nbr) { return enc_pool_msgs_ok(enc, nbr) ? 1 : 0; }

PIML_API int piml_pinnsf_fwd(const piml_encoder_branch* enc, const piml_decoder_branch* dec, int nbr,
                             const piml_collision_head* head, const float* self_features, float tau, float* acc,
                             int flags, void* stream) {
    hipStream_t m = as_stream(stream);
    const bool pack = !(flags & PIML_PACKED_VALID);
    PIML_TRY(pending_pack_flush(m));         // a deferred pack nobody took: now, in front of this call's launches (no-op otherwise)
    if (flags & PIML_POOL_TRAIN) {            // training on the agents' sums of h2 (see the header)
        if ((flags & (PIML_FORK | PIML_POOL_H2)) || !enc_pool_train_ok(enc, nbr)) return hipErrorInvalidValue;
        for (int i = 0; i < nbr; ++i)
            if (dec[i].pooled != enc[i].sum_a || dec[i].msgs != enc[i].sum_b) return hipErrorInvalidValue;
        if (pack) PIML_TRY(piml_pinnsf_pack(enc, dec, nbr, head, 0, stream));
        PIML_TRY(enc_stage_fwd_sum(enc, nbr, m, nbr > 1 ? acc : nullptr, nbr > 1 ? dec[0].agents * 2 : 0));
        trace_mark("enc_fwd_sum", m);
        PIML_TRY(dec_stage_fwd_sum(dec, nbr, head, self_features, tau, acc, m));
        trace_mark("dec_fwd_head_sum", m);
        return hipSuccess;
    }
    if (flags & PIML_POOL_MSGS) {             // the agents' sums of the messages from the encoder forward's registers (see the header)
        if ((flags & (PIML_FORK | PIML_POOL_H2)) || !enc_pool_msgs_ok(enc, nbr)) return hipErrorInvalidValue;
        for (int i = 0; i < nbr; ++i)
            if (dec[i].pooled != enc[i].sum_a || dec[i].msgs != enc[i].sum_b) return hipErrorInvalidValue;
        if (head && head->rows > 0 && head->msgs != enc[0].msgs) return hipErrorInvalidValue;      // the head reads the rows the forward stores
        if (pack) PIML_TRY(piml_pinnsf_pack(enc, dec, nbr, head, 0, stream));
        PIML_TRY(enc_stage_fwd(enc, nbr, m, nbr > 1 ? acc : nullptr, nbr > 1 ? dec[0].agents * 2 : 0, true));
        trace_mark("enc_fwd", m);
        PIML_TRY(dec_stage_fwd_sum(dec, nbr, head, self_features, tau, acc, m, false));
        trace_mark("dec_fwd_head_sum", m);
        return hipSuccess;
    }
    if (flags & PIML_POOL_H2) {               // inference: the agents' sums of h2 instead of the messages (see the header)
        if ((flags & PIML_FORK) || head || !enc_pool_h2_ok(enc, nbr)) return hipErrorInvalidValue;
        if (pack) PIML_TRY(piml_pinnsf_pack(enc, dec, nbr, nullptr, 0, stream));
        PIML_TRY(enc_stage_fwd_pool(enc, nbr, m, nbr > 1 ? acc : nullptr, nbr > 1 ? dec[0].agents * 2 : 0));
        trace_mark("enc_fwd", m);
        PIML_TRY(dec_stage_fwd_ph2(dec, nbr, self_features, tau, acc, m));
        trace_mark("dec_fwd_head", m);
        return hipSuccess;
    }
    if (!(flags & PIML_FORK)) {
        if (pack) PIML_TRY(piml_pinnsf_pack(enc, dec, nbr, head, 0, stream));
        // the split decoder tiles accumulate their two branches into `acc`: cleared by the encoder launch
        PIML_TRY(enc_stage_fwd(enc, nbr, m, nbr > 1 ? acc : nullptr, nbr > 1 ? dec[0].agents * 2 : 0));
        trace_mark("enc_fwd", m);
        PIML_TRY(dec_stage_fwd_fused(dec, nbr, head, self_features, tau, acc, m));
        trace_mark("dec_fwd_head", m);
        return hipSuccess;
    }
    Side* S;
    PIML_TRY(side_streams(&S));
    hipStream_t s0 = S->s[0], s1 = S->s[1];
    if (pack) {
        PIML_TRY(edge(m, s0, S->ev[0]));
        PIML_TRY(dec_stage_pack(dec, nbr, s0));
        if (head) PIML_TRY(head_stage_pack(head, s0));
        PIML_TRY(hipEventRecord(S->ev[1], s0));
        PIML_TRY(enc_stage_pack(enc, nbr, m));
    }
    PIML_TRY(enc_stage_fwd(enc, nbr, m));
    if (head) {
        PIML_TRY(edge(m, s1, S->ev[2]));
        if (pack) PIML_TRY(hipStreamWaitEvent(s1, S->ev[1], 0));
        PIML_TRY(head_stage_fwd(head, s1));
        PIML_TRY(hipEventRecord(S->ev[3], s1));
    }
    PIML_TRY(dec_stage_pool(dec, nbr, m));
    if (pack) PIML_TRY(hipStreamWaitEvent(m, S->ev[1], 0));
    PIML_TRY(dec_stage_fwd(dec, nbr, self_features, tau, acc, m));
    if (head) PIML_TRY(hipStreamWaitEvent(m, S->ev[3], 0));
    return hipSuccess;
}

PIML_API int piml_pinnsf_bwd(const piml_encoder_branch* enc, const piml_decoder_branch* dec, int nbr, const float* g_pred,
                             const float* self_features, float tau, float* g_self, int flags, void* stream) {
    hipStream_t m = as_stream(stream);
    if (flags & PIML_POOL_TRAIN) {            // backward of a PIML_POOL_TRAIN forward
        if (flags & PIML_FORK) return hipErrorInvalidValue;
        for (int i = 0; i < nbr; ++i)
            if (!dec[i].dw1_out || !dec[i].fold_w3 || dec[i].g_pooled != enc[i].g_pooled) return hipErrorInvalidValue;
        PIML_TRY(dec_stage_bwd_fused(dec, nbr, g_pred, self_features, tau, g_self, m, true));
        trace_mark("dec_bwd", m);
        // the decoder sets to the encoder backward -- unless deferred sums that write the same gradients still wait: theirs go first
        DecSlotSums D = {};
        if (g_dec_slots_enc) {
            D.nsets = nbr;
            D.slots = piml_decoder_workgroups(dec[0].agents);
            D.lanes = DEC_PART / 4;
            D.accumulate = (flags & PIML_ACCUMULATE) != 0;
            for (int i = 0; i < nbr; ++i) {
                D.parts[i] = dec[i].partials;
                D.grads[i] = dec[i].grads;
                if (pending_slot_sums_write(dec[i].grads)) D.nsets = 0;
            }
        }
        bool dec_summed = false;
        PIML_TRY(enc_stage_bwd_sum(enc, nbr, m, D.nsets > 0 ? &D : nullptr, &dec_summed));
        trace_mark("enc_bwd_dx", m);
        return reduce_all(enc, dec, nbr, m, (flags & PIML_ACCUMULATE) != 0, (flags & PIML_DEFER_SLOT_SUMS) != 0, true,
                          (flags & PIML_DEFER_UNFOLD) != 0, dec_summed);
    }
    if (!(flags & PIML_FORK)) {
        PIML_TRY(dec_stage_bwd_fused(dec, nbr, g_pred, self_features, tau, g_self, m));
        trace_mark("dec_bwd", m);
        PIML_TRY(enc_stage_bwd_dx(enc, nbr, m));
        trace_mark("enc_bwd_dx", m);
        PIML_TRY(enc_stage_bwd_dw(enc, nbr, m));
        trace_mark("enc_bwd_dw", m);
        PIML_TRY(reduce_all(enc, dec, nbr, m, (flags & PIML_ACCUMULATE) != 0, (flags & PIML_DEFER_SLOT_SUMS) != 0));
        return hipSuccess;
    }
    if (flags & (PIML_ACCUMULATE | PIML_DEFER_SLOT_SUMS)) return hipErrorInvalidValue;      // (the forked form sums its slots per stage: not offered there)
    PIML_TRY(dec_stage_bwd_dx(dec, nbr, g_pred, self_features, tau, g_self, m));
    Side* S;
    PIML_TRY(side_streams(&S));
    hipStream_t s0 = S->s[0];
    PIML_TRY(edge(m, s0, S->ev[4]));
    PIML_TRY(dec_stage_bwd_dw(dec, nbr, g_pred, true, s0));
    PIML_TRY(hipEventRecord(S->ev[5], s0));
    PIML_TRY(enc_stage_bwd_dx(enc, nbr, m));
    PIML_TRY(enc_stage_bwd_dw(enc, nbr, m));
    PIML_TRY(hipStreamWaitEvent(m, S->ev[5], 0));
    return enc_stage_reduce(enc, nbr, m);
}
