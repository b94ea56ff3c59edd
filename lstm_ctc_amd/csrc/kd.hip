// kd.hip — teacher-student distillation: per-frame KL(softmax(teacher / tau) || softmax(logits / tau)) against a teacher's
// whole posterior, the soft-target relative of xent.hip.  No reference counterpart.  DESIGN.md section 3.9.
//
// Contract (include/lstm_ctc_hip.h: lc_kd_loss)
//   logits, teacher [T,B,V] time-major fp32 (teacher in the log domain; a per-row shift is immaterial, -inf = probability 0);
//   seq_len, teacher_len [B].  A frame (t, b) is SCORED when t < seq_len[b] and t < teacher_len[b].  With p = softmax(teacher
//   / tau), q = softmax(logits / tau): loss[b] = sum over scored frames of sum_k p_k (log p_k - log q_k) (p_k = 0: term 0),
//   natural log, not clamped; frames[b] = scored frames; agree[b] = scored frames whose two argmaxes (lowest index among equal
//   maxima) coincide; grad row = grad_scale (q - p), stored (accumulate = 0; every other row +0) or added to what grad holds
//   (accumulate != 0; every other row neither read nor written).  A teacher row whose maximum is not finite (all -inf, a
//   +inf) or that holds a NaN is BAD: loss[b] NaN, the frame counts nowhere and adds nothing to grad.  Unscored frames' rows
//   are never read.  Every element of loss, frames and agree is written on every call, bit-identically from call to call and
//   with and without a gradient (no atomics).
//
// Arithmetic of a frame, s the teacher row, z the student row, c = log2(e) / tau, all fp32:
//   ms = max s, mz = max z;  a_k = s_k - ms, b_k = z_k - mz;  ep_k = exp2(c a_k), eq_k = exp2(c b_k);  Sp = sum ep, Sq = sum eq
//   KL = (sum_{ep_k > 0} ep_k (a_k - b_k)) / (tau Sp) + ln Sq - ln Sp         (no per-element log, no 0 * inf; the maxima
//   grad_k = grad_scale (eq_k / Sq - ep_k / Sp)                                are taken out BEFORE the difference, so a
//   shift of either row cancels exactly).  Sp is NaN exactly when the row is bad (-inf - -inf, inf - inf, NaN), and >= 1
//   otherwise: that is the test.
//
// Two launches, xent.hip's, through the two-row skeleton of row_group.h (rg_rows_kernel / rg_wide_kernel over the criterion
// Kd below, then rg_fold_kernel): one GROUP of G lanes per frame, waves walk the frames with a grid stride.
//        V <= 64    G = 16: four frames per wave, one per 16-lane DPP row, butterfly reductions (every lane gets the result)
//        V <= 1024  G = 64: one frame per wave, 4 / 8 / 16 elements per lane and row; both rows are loaded ONCE and stay in
//                   2 NE registers per lane across the two maxima, the two sums, the KL sum and the gradient store
//        V  > 1024  one frame per wave in three passes over the two rows (maxima + argmaxes, sums, gradient), on a grid
//                   capped so that the rows in flight stay in the Infinity Cache (RG_WIDE_INFLIGHT_BYTES)
//      VEC as in xent.hip: 16-byte accesses when V % 4 == 0 and all three buffers are 16-byte aligned; the wide kernel takes
//      them at any V with a head / body / tail split.  Lane 0 of the group writes the frame's term and a flag word (1 =
//      scored, 2 = argmaxes agree, 4 = bad teacher row) as ONE 8-byte word to the workspace, laid out [B,T]; one workgroup
//      per utterance then folds its frames' terms in a FIXED order in double and rounds once.
#include "common.h"
#include "row_group.h"
#include <math.h>

namespace {

// The criterion: row 1 the teacher's, row 2 the student's, one gradient row.
struct Kd {
    static constexpr int NG = 1;
    static constexpr bool TWO_LOOPS = false;
    const float *x[2];
    float *g[1];
    const int *seq_len, *teacher_len;
    float c, itau, scale;
    struct Sums { float ms, mz, sp, sq, ka, ip, iq; };

    __device__ __forceinline__ size_t row(int t, int b, int B, int V) const { return ((size_t)t * B + b) * (size_t)V; }
    __device__ __forceinline__ int head(size_t row, int) const { return (int)((4 - (row & 3)) & 3); }
    __device__ __forceinline__ bool scored(int t, int b) const { return t < seq_len[b] && t < teacher_len[b]; }
    __device__ __forceinline__ Sums open(float ms, float mz) const { return {ms, mz, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}; }
    // one element of a frame: the exponentials in the rows' place; the KL sum gains ep (a - b) where ep > 0
    __device__ __forceinline__ void element(Sums &s, float &x1, float &x2, float &) const
    {
        const float a = x1 - s.ms, b = x2 - s.mz;
        const float ep = __builtin_amdgcn_exp2f(a * c), eq = __builtin_amdgcn_exp2f(b * c);
        s.sp += ep;
        s.sq += eq;
        s.ka += ep > 0.0f ? ep * (a - b) : 0.0f;
        x1 = ep;
        x2 = eq;
    }
    template <int G> __device__ __forceinline__ void close(Sums &s) const
    {
        s.sp = rg_sum<G>(s.sp);
        s.sq = rg_sum<G>(s.sq);
        s.ka = rg_sum<G>(s.ka);
    }
    // NaN exactly when the teacher row's maximum is not finite or it holds a NaN (which slips past the maximum, not the sum)
    __device__ __forceinline__ bool bad(const Sums &s) const { return !(s.sp == s.sp); }
    template <int G> __device__ __forceinline__ float term(const Sums &s) const
    {
        return s.ka * itau * __builtin_amdgcn_rcpf(s.sp) + (__builtin_amdgcn_logf(s.sq) - __builtin_amdgcn_logf(s.sp)) * RG_LN2;
    }
    __device__ __forceinline__ void grad_open(Sums &s, bool good) const
    {
        s.ip = good ? scale * __builtin_amdgcn_rcpf(s.sp) : 0.0f;
        s.iq = good ? scale * __builtin_amdgcn_rcpf(s.sq) : 0.0f;
    }
    __device__ __forceinline__ void grad(const Sums &s, float ep, float eq, float (&out)[1]) const { out[0] = eq * s.iq - ep * s.ip; }
};

}  // namespace

extern "C" size_t lc_kd_workspace_bytes(int T, int B, int V) { return rg_workspace_bytes(T, B, V); }

extern "C" int lc_kd_loss(const float *logits, const float *teacher, int T, int B, int V, const int *seq_len,
                          const int *teacher_len, float temperature, float grad_scale, float *loss, int *frames, int *agree,
                          float *grad, int accumulate, void *workspace, size_t workspace_bytes, lc_stream_t stream)
{
    LC_CHECK_ARG(logits && teacher && seq_len && teacher_len && loss && frames && agree && workspace,
                 "lc_kd_loss: null pointer");
    LC_CHECK_ARG(T > 0 && B > 0 && V >= 2, "lc_kd_loss: bad shape T=%d B=%d V=%d", T, B, V);
    const float itau = 1.0f / temperature;
    LC_CHECK_ARG(temperature > 0.0f && isfinite(temperature) && isfinite(itau),
                 "lc_kd_loss: temperature must be finite and > 0, got %g", (double)temperature);
    const size_t need = lc_kd_workspace_bytes(T, B, V);
    if (workspace_bytes < need) {
        lc_set_error("lc_kd_loss: workspace too small (%zu < %zu)", workspace_bytes, need);
        return LC_EWORKSPACE;
    }
    const bool aligned = (((uintptr_t)logits | (uintptr_t)teacher | (uintptr_t)grad) & 15) == 0;
    const bool vec = aligned && V % 4 == 0;          // rows in registers: every row starts on a 16-byte boundary
    const Kd cr = {{teacher, logits}, {grad}, seq_len, teacher_len, RG_LOG2E * itau, itau, grad_scale};
    return rg_launch_criterion("kd_rows", "kd_fold", cr, T, B, V, vec, aligned, (int2 *)workspace, accumulate != 0, loss, frames,
                               agree, (hipStream_t)stream);
}
