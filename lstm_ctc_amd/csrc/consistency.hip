// consistency.hip — consistency-regularised CTC (CR-CTC): the per-frame symmetric KL between the posteriors of two views of
// one utterance that sit in the two halves of ONE batch, kd.hip's sibling.  No reference counterpart.  DESIGN.md section 3.12.
//
// Contract (include/lstm_ctc_hip.h: lc_consistency_loss)
//   logits, grad [T,2B,V] time-major fp32, B the number of PAIRS: row (t, b) is view a of pair b, row (t, b + B) view b;
//   seq_len [B], one length per pair.  A pair-frame (t, b) is SCORED when t < seq_len[b].  With qa = softmax(za), qb =
//   softmax(zb): loss[b] = sum over scored pair-frames of J = KL(qb || qa) + KL(qa || qb) = sum_k (qa_k - qb_k)(log qa_k -
//   log qb_k) (both probabilities 0: term 0), natural log, not scaled, not clamped; frames[b] = scored pair-frames; agree[b] =
//   those whose two argmaxes (lowest index among equal maxima) coincide; grad row a = grad_scale (qa - qb), row b = grad_scale
//   (qb - qa) - the STOP-GRADIENT form, each view a constant target for the other, NOT the derivative of J - stored (accumulate
//   = 0; every other row +0) or added to what grad holds (accumulate != 0; every other row neither read nor written).  A row of
//   either view whose maximum is not finite (all -inf, a +inf) or that holds a NaN is BAD: loss[b] NaN, the pair-frame counts
//   nowhere and adds nothing to grad.  Unscored pair-frames' rows are never read.  Every element of loss, frames and agree is
//   written on every call, bit-identically from call to call and with and without a gradient (no atomics).
//
// Arithmetic of a pair-frame, all fp32:
//   ma = max za, mb = max zb;  a_k = za_k - ma, b_k = zb_k - mb;  ea_k = exp(a_k), eb_k = exp(b_k);  Sa = sum ea, Sb = sum eb
//   d_k = ea_k / Sa - eb_k / Sb;   J = sum_{d_k != 0} d_k ((a_k - b_k) - (ln Sa - ln Sb))       (no per-element log; equal rows
//   grad a_k = grad_scale d_k,  grad b_k = -(grad_scale d_k)                                      give d = 0, J = 0 exactly)
//   Sa (Sb) is NaN exactly when row a (b) is bad (-inf - -inf, inf - inf, NaN), and >= 1 otherwise: that is the test.
//
// Two launches, kd.hip's, through the two-row skeleton of row_group.h (rg_rows_kernel / rg_wide_kernel over the criterion
// Consistency below, then rg_fold_kernel): one GROUP of G lanes per pair-frame, waves walk the pair-frames with a grid stride.
//        V <= 64    G = 16: four pair-frames per wave, one per 16-lane DPP row, butterfly reductions
//        V <= 1024  G = 64: one pair-frame per wave, 4 / 8 / 16 elements per lane and row; both rows are loaded ONCE and stay
//                   in registers (the exponentials and a_k - b_k: 3 NE per lane) across the two maxima, the two sums, the
//                   term and the two gradient rows
//        V  > 1024  one pair-frame per wave in three passes over the two rows (maxima + argmaxes, sums, term + gradient), on a
//                   grid capped so that the rows in flight stay in the Infinity Cache (RG_WIDE_INFLIGHT_BYTES)
//      VEC: 16-byte accesses when V % 4 == 0 and both buffers are 16-byte aligned (then every row of either half starts on a
//      16-byte boundary: no head), dwords otherwise.  Lane 0 of the group writes the pair-frame's term and a flag word (1 =
//      scored, 2 = argmaxes agree, 4 = bad row) as ONE 8-byte word to the workspace, laid out [B,T]; one workgroup per pair
//      then folds its pair-frames' terms in a FIXED order in double and rounds once.
#include "common.h"
#include "row_group.h"
#include <math.h>

namespace {

// A product that is rounded on its own (no fma).  The two quotients: an fma would leave one product's rounding error as the d
// of two equal rows.  grad_scale d: the accumulated row is then the stored row added to what grad held, in one rounding.
__device__ __forceinline__ float cr_mul(float x, float y)
{
#pragma clang fp contract(off)
    return x * y;
}

// The criterion: row 1 view a, row 2 view b, B V elements on; two gradient rows in the same places.
struct Consistency {
    static constexpr int NG = 2;
    static constexpr bool TWO_LOOPS = true;
    const float *x[2];
    float *g[2];
    const int *seq_len;
    float scale;
    struct Sums { float ma, mb, sa, sb, jt, ia, ib, dl; };

    __device__ __forceinline__ size_t row(int t, int b, int B, int V) const { return ((size_t)t * (2 * (size_t)B) + b) * (size_t)V; }
    // VEC: V % 4 == 0, so every row of either half starts on a boundary and ends on one
    __device__ __forceinline__ int head(size_t, int V) const
    {
        __builtin_assume((V & 3) == 0);
        return 0;
    }
    __device__ __forceinline__ bool scored(int t, int b) const { return t < seq_len[b]; }
    __device__ __forceinline__ Sums open(float ma, float mb) const { return {ma, mb, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}; }
    // first half of an element: the exponentials in the rows' place and a - b kept; the two sums gain theirs
    __device__ __forceinline__ void element(Sums &s, float &za, float &zb, float &ab) const
    {
        const float a = za - s.ma, b = zb - s.mb;
        za = __builtin_amdgcn_exp2f(a * RG_LOG2E);
        zb = __builtin_amdgcn_exp2f(b * RG_LOG2E);
        ab = a - b;
        s.sa += za;
        s.sb += zb;
    }
    template <int G> __device__ __forceinline__ void close(Sums &s) const
    {
        s.sa = rg_sum<G>(s.sa);
        s.sb = rg_sum<G>(s.sb);
        s.ia = __builtin_amdgcn_rcpf(s.sa);
        s.ib = __builtin_amdgcn_rcpf(s.sb);
        s.dl = (__builtin_amdgcn_logf(s.sa) - __builtin_amdgcn_logf(s.sb)) * RG_LN2;
    }
    // NaN exactly when a row's maximum is not finite or it holds a NaN (which slips past the maximum, not the sum)
    __device__ __forceinline__ bool bad(const Sums &s) const { return !(s.sa == s.sa && s.sb == s.sb); }
    // second half: d = qa - qb in row 1's place and its share of J (d = 0, which covers probability 0 in both views: none; no
    // 0 * inf)
    __device__ __forceinline__ void second(Sums &s, float &ea, float eb, float ab) const
    {
        const float d = cr_mul(ea, s.ia) - cr_mul(eb, s.ib);
        s.jt += d != 0.0f ? d * (ab - s.dl) : 0.0f;
        ea = d;
    }
    template <int G> __device__ __forceinline__ float term(const Sums &s) const { return rg_sum<G>(s.jt); }
    __device__ __forceinline__ void grad_open(Sums &, bool) const {}
    __device__ __forceinline__ void grad(const Sums &, float d, float, float (&out)[2]) const
    {
        out[0] = cr_mul(scale, d);
        out[1] = -out[0];
    }
};

}  // namespace

extern "C" size_t lc_consistency_workspace_bytes(int T, int B, int V) { return rg_workspace_bytes(T, B, V); }

extern "C" int lc_consistency_loss(const float *logits, int T, int B, int V, const int *seq_len, float grad_scale, float *loss,
                                   int *frames, int *agree, float *grad, int accumulate, void *workspace,
                                   size_t workspace_bytes, lc_stream_t stream)
{
    LC_CHECK_ARG(logits && seq_len && loss && frames && agree && workspace, "lc_consistency_loss: null pointer");
    LC_CHECK_ARG(T > 0 && B > 0 && V >= 2, "lc_consistency_loss: bad shape T=%d B=%d (pairs) V=%d", T, B, V);
    LC_CHECK_ARG(isfinite(grad_scale), "lc_consistency_loss: grad_scale must be finite, got %g", (double)grad_scale);
    LC_CHECK_ARG(grad || !accumulate, "lc_consistency_loss: accumulate needs a gradient buffer");
    const size_t need = lc_consistency_workspace_bytes(T, B, V);
    if (workspace_bytes < need) {
        lc_set_error("lc_consistency_loss: workspace too small (%zu < %zu)", workspace_bytes, need);
        return LC_EWORKSPACE;
    }
    const bool vec = V % 4 == 0 && (((uintptr_t)logits | (uintptr_t)grad) & 15) == 0;      // then every row of either half is aligned
    const size_t half = (size_t)B * (size_t)V;       // from a row of view a to its partner in view b
    const Consistency cr = {{logits, logits + half}, {grad, grad ? grad + half : nullptr}, seq_len, grad_scale};
    return rg_launch_criterion("cr_rows", "cr_fold", cr, T, B, V, vec, vec, (int2 *)workspace, accumulate != 0, loss, frames,
                               agree, (hipStream_t)stream);
}
