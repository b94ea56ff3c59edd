// xent.hip — frame-level softmax cross-entropy against one target symbol per frame (the table nnet-align writes).
// No reference counterpart (the reference never finished frame-level training).  DESIGN.md section 3.7.
//
// Contract (include/lstm_ctc_hip.h: lc_xent_loss)
//   logits [T,B,V] time-major fp32; targets [B,T] int32, the layout lc_ctc_align writes; seq_len [B].
//   A frame (t, b) is SCORED when t < seq_len[b] and 0 <= targets[b,t] < V.  Class V-1 (the blank) is a legal target; -1 means
//   "ignore".  loss[b] = sum over scored frames of -log_softmax(logits[t,b,:])[target] (natural log); frames[b] = number of
//   scored frames; correct[b] = scored frames whose argmax (lowest index among equal maxima, the greedy decoder's rule) is the
//   target; grad = d sum_b loss[b] / d logits = softmax - onehot on scored rows, +0 on every other row, un-normalised like
//   lc_ctc_loss.  A live target < -1 or >= V makes loss[b] NaN; its frame counts nowhere and gets a zero row.  -inf logits
//   behave as in float arithmetic: a -inf non-target class contributes 0 and gets gradient 0, a -inf target gives +inf loss, an
//   all -inf row gives NaN.  Every element of loss, frames, correct and grad is written on every call (no memset), and the
//   result is bit-identical from call to call (no atomics).
//
// Two launches:
//   1. xent_rows_kernel<G, NE, VEC> (V <= 1024) or xent_wide_kernel<VEC> (any V): one GROUP of G lanes per frame, waves walk
//      the frames with a grid stride.  A frame's row is loaded ONCE and stays in NE registers per lane between the maximum, the
//      sum of exponentials and the gradient store: logits are read once, the gradient is written once.
//        V <= 64    G = 16: FOUR frames per wave, one per 16-lane DPP row; the reductions are the four row steps of a DPP
//                   butterfly (xor 1, xor 2 by quad_perm, then row_half_mirror, row_mirror), which leave the SAME bits in every
//                   lane of the row (each step adds two operands that both lanes of a pair hold, and fp addition commutes).
//        V <= 1024  G = 64: one frame per wave, 4 / 8 / 16 elements per lane, lc_wave_max / lc_wave_sum.
//        V  > 1024  one frame per wave in three passes over the row (maximum + argmax, sum, gradient); the second and third
//                   find the row in the caches.
//      VEC (V % 4 == 0, 16-byte aligned buffers): 16-byte accesses, lane l of the group holds elements 4 (j G + l) .. + 3;
//      otherwise dwords, element j G + l.  The wide kernel takes 16-byte accesses at ANY V when the buffers are aligned: a row
//      then starts 0 .. 3 elements short of a boundary, and those and the last (V - head) % 4 go as dwords.  Rows that are not
//      scored are never read; their gradient rows are stored as zeros.
//      The lane that holds the target's logit writes the frame's term -log_softmax[target] = lse - x_target (fp32: one
//      log-sum-exp, one subtraction) and a flag word (1 = scored, 2 = argmax is the target, 4 = bad target) as ONE 8-byte
//      word to the workspace, laid out [B,T] like the targets.
//   2. rg_fold_kernel: one workgroup per utterance folds its frames' terms in a FIXED order in double (thread i takes frames
//      i, i + 256, ... in sequence, then a xor butterfly over each wave's lanes, then the four waves) and rounds once to float,
//      like ctc_align.hip's score.
// The walk over the frames, the loads, the argmax, the zero rows, the gradient store, the fold and the launcher with the V
// ladder are row_group.h's, shared with kd.hip and consistency.hip.  The two kernel bodies stay here and are not a two-row
// criterion of that header: a frame has ONE row and a target, the lane that owns the target writes the term, and the bad
// flag comes from the target before any row is read - three hooks that no other criterion would use.
#include "common.h"
#include "row_group.h"
#include <math.h>

namespace {

// what the targets say about frame (t, b); valid: the frame is inside [T, B]
struct XentFrame {
    int tgt;
    bool scored, bad;
    __device__ __forceinline__ XentFrame(const int *targets, const int *seq_len, int t, int b, size_t bt, int V, bool valid)
    {
        int sl = 0;
        tgt = -1;
        if (valid) {
            sl = seq_len[b];
            tgt = targets[bt];
        }
        const bool live = valid && t < sl;
        scored = live && tgt >= 0 && tgt < V;
        bad = live && (tgt < -1 || tgt >= V);
    }
};

// ------------------------------------------------------------------------------------------ 1a. rows that fit registers
template <int G, int NE, bool VEC>
__global__ __launch_bounds__(256) void xent_rows_kernel(const float *__restrict__ logits, int T, int B, int V,
                                                        const int *__restrict__ targets, const int *__restrict__ seq_len,
                                                        int2 *__restrict__ terms, float *__restrict__ grad)
{
    const RgGroup<G, NE, VEC> grp;
    rg_for_frames<64 / G>(T, B, [&](int t, int b, bool valid, size_t bt) {
        const XentFrame f(targets, seq_len, t, b, bt, V, valid);
        const int tgt = f.tgt;
        const bool scored = f.scored;
        const size_t row = ((size_t)t * B + b) * (size_t)V;
        const float *const xb[1] = {logits};
        float *const gb[1] = {grad};
        if (__builtin_amdgcn_ballot_w64(scored) == 0) {          // nothing to score in this wave: zero rows, no logits read
            if (valid) {
                if (grp.l == 0) terms[bt] = make_int2(0, f.bad ? RG_BAD : 0);
                if (grad) grp.zero(gb, row, V);
            }
            return;
        }
        // the row, once (-inf in groups that score nothing), its maximum and argmax
        float x[1][NE], m[1];
        int amax[1];
        grp.load(x, xb, row, V, scored);
        grp.top(x, m, amax);
        // the target's logit in the lane that holds it
        float xt = 0.0f;
        bool owner = false;
#pragma unroll
        for (int j = NE - 1; j >= 0; --j) {
            const bool is_t = grp.idx(j) == tgt;
            xt = is_t ? x[0][j] : xt;
            owner = owner || is_t;
        }
        float s = 0.0f;
#pragma unroll
        for (int j = 0; j < NE; ++j) {
            x[0][j] = __builtin_amdgcn_exp2f((x[0][j] - m[0]) * RG_LOG2E);
            s += x[0][j];
        }
        s = rg_sum<G>(s);
        const float lse = m[0] + __builtin_amdgcn_logf(s) * RG_LN2;
        if (scored ? owner : (valid && grp.l == 0))
            terms[bt] = make_int2(scored ? __float_as_int(lse - xt) : 0,
                                  scored ? (RG_SCORED | (amax[0] == tgt ? RG_AGREE : 0)) : (f.bad ? RG_BAD : 0));
        if (grad && valid) {
            const float inv = __builtin_amdgcn_rcpf(s);
            grp.store(gb, row, V, scored, 0, [&](int j, float (&out)[1]) { out[0] = x[0][j] * inv - (grp.idx(j) == tgt ? 1.0f : 0.0f); });
        }
    });
}

// ------------------------------------------------------------------------------------------ 1b. any row width
template <bool VEC>
__global__ __launch_bounds__(256) void xent_wide_kernel(const float *__restrict__ logits, int T, int B, int V,
                                                        const int *__restrict__ targets, const int *__restrict__ seq_len,
                                                        int2 *__restrict__ terms, float *__restrict__ grad)
{
    const int lane = threadIdx.x & 63;
    rg_for_frames<1>(T, B, [&](int t, int b, bool, size_t bt) {
        const XentFrame f(targets, seq_len, t, b, bt, V, true);
        const int tgt = f.tgt;
        const size_t row = ((size_t)t * B + b) * (size_t)V;
        const int head = (int)((4 - (row & 3)) & 3);
        const float *xr[1] = {logits + row};
        float *gr[1] = {grad ? grad + row : nullptr};
        if (!f.scored) {                                                     // wave-uniform
            if (lane == 0) terms[bt] = make_int2(0, f.bad ? RG_BAD : 0);
            if (grad) rg_wide_zero<VEC>(lane, V, head, gr);
            return;
        }
        float m[1];
        int amax[1];
        rg_wide_top<VEC>(lane, V, head, xr, m, amax);
        // pass 2: sum of exponentials, per lane in the order of its visits, then over the lanes
        float s = 0.0f;
        auto ex = [&](float v) { return __builtin_amdgcn_exp2f((v - m[0]) * RG_LOG2E); };
        rg_wide_pass<VEC>(lane, V, head, xr, [&](int, const float (&x)[1]) { s += ex(x[0]); });
        s = lc_wave_sum(s);
        const float lse = m[0] + __builtin_amdgcn_logf(s) * RG_LN2;
        if (lane == 0)
            terms[bt] = make_int2(__float_as_int(lse - xr[0][tgt]), RG_SCORED | (amax[0] == tgt ? RG_AGREE : 0));
        // pass 3: the gradient row
        if (grad) {
            const float inv = __builtin_amdgcn_rcpf(s);
            rg_wide_grad<VEC>(lane, V, head, xr, gr, true, 0,
                              [&](int e, float (&x)[1], float (&out)[1]) { out[0] = ex(x[0]) * inv - (e == tgt ? 1.0f : 0.0f); });
        }
    });
}

}  // namespace

extern "C" size_t lc_xent_workspace_bytes(int T, int B, int V) { return rg_workspace_bytes(T, B, V); }

extern "C" int lc_xent_loss(const float *logits, int T, int B, int V, const int *targets, const int *seq_len, float *loss,
                            int *frames, int *correct, float *grad, void *workspace, size_t workspace_bytes,
                            lc_stream_t stream)
{
    LC_CHECK_ARG(logits && targets && seq_len && loss && frames && correct && workspace, "lc_xent_loss: null pointer");
    LC_CHECK_ARG(T > 0 && B > 0 && V >= 2, "lc_xent_loss: bad shape T=%d B=%d V=%d", T, B, V);
    const size_t need = lc_xent_workspace_bytes(T, B, V);
    if (workspace_bytes < need) {
        lc_set_error("lc_xent_loss: workspace too small (%zu < %zu)", workspace_bytes, need);
        return LC_EWORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    int2 *terms = (int2 *)workspace;
    const bool aligned = (((uintptr_t)logits | (uintptr_t)grad) & 15) == 0;
    const bool vec = aligned && V % 4 == 0;          // rows in registers: every row starts on a 16-byte boundary
    // no cap for the Infinity Cache on the wide kernel: one row a frame, and the second and third pass find it in the caches
    return rg_launch("xent_rows", "xent_fold", T, B, V, vec, aligned, false, terms, loss, frames, correct, s,
                     [&](auto shape, unsigned nb) {
                         using S = decltype(shape);
                         if constexpr (S::NE == 0)
                             hipLaunchKernelGGL((xent_wide_kernel<S::VEC>), dim3(nb), dim3(256), 0, s, logits, T, B, V, targets,
                                                seq_len, terms, grad);
                         else
                             hipLaunchKernelGGL((xent_rows_kernel<S::G, S::NE, S::VEC>), dim3(nb), dim3(256), 0, s, logits, T, B,
                                                V, targets, seq_len, terms, grad);
                     });
}
