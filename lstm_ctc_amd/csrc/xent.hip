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
//   2. xent_fold_kernel: one workgroup per utterance folds its frames' terms in a FIXED order in double (thread i takes frames
//      i, i + 256, ... in sequence, then a xor butterfly over each wave's lanes, then the four waves) and rounds once to float,
//      like ctc_align.hip's score.
#include "common.h"
#include "row_group.h"
#include <math.h>

#define XE_LOG2E 1.4426950408889634f
#define XE_LN2 0.6931471805599453f
#define XE_MAX_GRID 2048                 // blocks of four waves, as stream_grid in misc.hip

namespace {

// ------------------------------------------------------------------------------------------ 1a. rows that fit registers
template <int G, int NE, bool VEC>
__global__ __launch_bounds__(256) void xent_rows_kernel(const float *__restrict__ logits, int T, int B, int V,
                                                        const int *__restrict__ targets, const int *__restrict__ seq_len,
                                                        int2 *__restrict__ terms, float *__restrict__ grad)
{
    constexpr int FW = 64 / G;                       // frames per wave
    constexpr int NQ = NE / 4;                       // 16-byte accesses per lane (VEC)
    const int lane = threadIdx.x & 63, l = lane & (G - 1), g = lane / G;
    const int stride = (int)gridDim.x * 4 * FW;      // <= 2048 * 16 frames per pass
    const int first = ((int)blockIdx.x * 4 + ((int)threadIdx.x >> 6)) * FW;
    const long long TB = (long long)T * B;
    RgWalk w(first, stride, B);
    for (long long fb = first; fb < TB; fb += stride, w.next(B)) {
        int b = w.b0 + g, t = w.t0;
#pragma unroll
        for (int i = 0; i < FW - 1; ++i)             // g < FW: at most FW - 1 wraps (B = 1)
            if (b >= B) { b -= B; ++t; }
        const bool valid = t < T;
        const size_t bt = (size_t)b * T + t;         // the frame's place in targets and in the workspace, both [B,T]
        int tgt = -1, sl = 0;
        if (valid) {
            sl = seq_len[b];
            tgt = targets[bt];
        }
        const bool live = valid && t < sl;
        const bool scored = live && tgt >= 0 && tgt < V;
        const bool bad = live && (tgt < -1 || tgt >= V);
        const size_t row = ((size_t)t * B + b) * (size_t)V;
        if (__builtin_amdgcn_ballot_w64(scored) == 0) {          // nothing to score in this wave: zero rows, no logits read
            if (valid) {
                if (l == 0) terms[bt] = make_int2(0, bad ? RG_BAD : 0);
                if (grad) {
                    if (VEC) {
#pragma unroll
                        for (int jq = 0; jq < NQ; ++jq) {
                            const int q = jq * G + l;
                            if (4 * q < V) *(float4 *)(grad + row + 4 * q) = make_float4(0.f, 0.f, 0.f, 0.f);
                        }
                    } else {
#pragma unroll
                        for (int j = 0; j < NE; ++j) {
                            const int e = j * G + l;
                            if (e < V) grad[row + e] = 0.0f;
                        }
                    }
                }
            }
            continue;
        }
        // the row, once: x[j] is element idx(j) of the frame, -inf beyond V and in groups that score nothing
        float x[NE];
        if (VEC) {
#pragma unroll
            for (int jq = 0; jq < NQ; ++jq) {
                const int q = jq * G + l;
                float4 v = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
                if (scored && 4 * q < V) v = *(const float4 *)(logits + row + 4 * q);
                x[4 * jq] = v.x; x[4 * jq + 1] = v.y; x[4 * jq + 2] = v.z; x[4 * jq + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < NE; ++j) {
                const int e = j * G + l;
                x[j] = (scored && e < V) ? logits[row + e] : -INFINITY;
            }
        }
        auto idx = [&](int j) { return VEC ? 4 * ((j >> 2) * G + l) + (j & 3) : j * G + l; };
        float m = x[0];
#pragma unroll
        for (int j = 1; j < NE; ++j) m = fmaxf(m, x[j]);
        m = rg_max<G>(m);
        // lowest index holding the maximum (idx rises with j inside a lane), and the target's logit in the lane that holds it
        int cand = 0x7fffffff;
        float xt = 0.0f;
        bool owner = false;
#pragma unroll
        for (int j = NE - 1; j >= 0; --j) {
            const int e = idx(j);
            cand = x[j] == m ? e : cand;
            const bool is_t = e == tgt;
            xt = is_t ? x[j] : xt;
            owner = owner || is_t;
        }
        const int amax = rg_min<G>(cand);
        float s = 0.0f;
#pragma unroll
        for (int j = 0; j < NE; ++j) {
            x[j] = __builtin_amdgcn_exp2f((x[j] - m) * XE_LOG2E);
            s += x[j];
        }
        s = rg_sum<G>(s);
        const float lse = m + __builtin_amdgcn_logf(s) * XE_LN2;
        if (scored ? owner : (valid && l == 0))
            terms[bt] = make_int2(scored ? __float_as_int(lse - xt) : 0,
                                  scored ? (RG_SCORED | (amax == tgt ? RG_AGREE : 0)) : (bad ? RG_BAD : 0));
        if (grad && valid) {
            const float inv = scored ? __builtin_amdgcn_rcpf(s) : 0.0f;
            if (VEC) {
#pragma unroll
                for (int jq = 0; jq < NQ; ++jq) {
                    const int q = jq * G + l;
                    float4 v;
                    v.x = scored ? x[4 * jq] * inv - (4 * q == tgt ? 1.0f : 0.0f) : 0.0f;
                    v.y = scored ? x[4 * jq + 1] * inv - (4 * q + 1 == tgt ? 1.0f : 0.0f) : 0.0f;
                    v.z = scored ? x[4 * jq + 2] * inv - (4 * q + 2 == tgt ? 1.0f : 0.0f) : 0.0f;
                    v.w = scored ? x[4 * jq + 3] * inv - (4 * q + 3 == tgt ? 1.0f : 0.0f) : 0.0f;
                    if (4 * q < V) *(float4 *)(grad + row + 4 * q) = v;
                }
            } else {
#pragma unroll
                for (int j = 0; j < NE; ++j) {
                    const int e = j * G + l;
                    if (e < V) grad[row + e] = scored ? x[j] * inv - (e == tgt ? 1.0f : 0.0f) : 0.0f;
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------ 1b. any row width
// rg_walk_row (row_group.h) is one pass of a wave over a row.
template <bool VEC>
__global__ __launch_bounds__(256) void xent_wide_kernel(const float *__restrict__ logits, int T, int B, int V,
                                                        const int *__restrict__ targets, const int *__restrict__ seq_len,
                                                        int2 *__restrict__ terms, float *__restrict__ grad)
{
    const int lane = threadIdx.x & 63;
    const int stride = (int)gridDim.x * 4;
    const int first = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    const long long TB = (long long)T * B;
    RgWalk w(first, stride, B);
    for (long long fb = first; fb < TB; fb += stride, w.next(B)) {
        const int b = w.b0, t = w.t0;
        const size_t bt = (size_t)b * T + t;
        const int sl = seq_len[b], tgt = targets[bt];
        const bool live = t < sl;
        const bool scored = live && tgt >= 0 && tgt < V;
        const bool bad = live && (tgt < -1 || tgt >= V);
        const size_t row = ((size_t)t * B + b) * (size_t)V;
        const int head = (int)((4 - (row & 3)) & 3);
        const float *xr = logits + row;
        float *gr = grad ? grad + row : nullptr;
        if (!scored) {                                                       // wave-uniform
            if (lane == 0) terms[bt] = make_int2(0, bad ? RG_BAD : 0);
            if (gr)
                rg_walk_row<VEC>(lane, V, head, [&](int e) { gr[e] = 0.0f; },
                                 [&](int e) { *(float4 *)(gr + e) = make_float4(0.f, 0.f, 0.f, 0.f); });
            continue;
        }
        // pass 1: maximum and the lowest index that holds it (a lane's indices rise, so strictly-greater keeps its first)
        float m = -INFINITY;
        int cand = 0x7fffffff;
        auto top = [&](float v, int e) {
            if (v > m || (cand == 0x7fffffff && v == m)) { m = v; cand = e; }
        };
        rg_walk_row<VEC>(lane, V, head, [&](int e) { top(xr[e], e); },
                         [&](int e) {
                             const float4 q = *(const float4 *)(xr + e);
                             top(q.x, e); top(q.y, e + 1); top(q.z, e + 2); top(q.w, e + 3);
                         });
        const float lm = m;
        m = lc_wave_max(m);
        const int amax = rg_min<64>(lm == m ? cand : 0x7fffffff);
        // pass 2: sum of exponentials, per lane in the order of its visits, then over the lanes
        float s = 0.0f;
        auto ex = [&](float v) { return __builtin_amdgcn_exp2f((v - m) * XE_LOG2E); };
        rg_walk_row<VEC>(lane, V, head, [&](int e) { s += ex(xr[e]); },
                         [&](int e) {
                             const float4 q = *(const float4 *)(xr + e);
                             s += ex(q.x); s += ex(q.y); s += ex(q.z); s += ex(q.w);
                         });
        s = lc_wave_sum(s);
        const float lse = m + __builtin_amdgcn_logf(s) * XE_LN2;
        if (lane == 0)
            terms[bt] = make_int2(__float_as_int(lse - xr[tgt]), RG_SCORED | (amax == tgt ? RG_AGREE : 0));
        // pass 3: the gradient row
        if (gr) {
            const float inv = __builtin_amdgcn_rcpf(s);
            auto g1 = [&](float v, int e) { return ex(v) * inv - (e == tgt ? 1.0f : 0.0f); };
            rg_walk_row<VEC>(lane, V, head, [&](int e) { gr[e] = g1(xr[e], e); },
                             [&](int e) {
                                 const float4 q = *(const float4 *)(xr + e);
                                 *(float4 *)(gr + e) = make_float4(g1(q.x, e), g1(q.y, e + 1), g1(q.z, e + 2), g1(q.w, e + 3));
                             });
        }
    }
}

// ------------------------------------------------------------------------------------------ 2. per-utterance fold
__global__ __launch_bounds__(256) void xent_fold_kernel(const int2 *__restrict__ terms, int T, float *__restrict__ loss,
                                                        int *__restrict__ frames, int *__restrict__ correct)
{
    rg_fold(terms, T, loss, frames, correct);
}

}  // namespace

extern "C" size_t lc_xent_workspace_bytes(int T, int B, int V)
{
    if (T <= 0 || B <= 0 || V < 2) return 0;
    return lc_align256((size_t)T * B * sizeof(int2));            // per frame: its term (float) and a flag word
}

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
    const long long TB = (long long)T * B;
    const bool aligned = (((uintptr_t)logits | (uintptr_t)grad) & 15) == 0;
    const bool vec = aligned && V % 4 == 0;          // rows in registers: every row starts on a 16-byte boundary
#define LC_XE(KERNEL, FW)                                                                                               \
    do {                                                                                                                \
        long long nb = (TB + 4 * (FW) - 1) / (4 * (FW));                                                                \
        if (nb > XE_MAX_GRID) nb = XE_MAX_GRID;                                                                         \
        hipLaunchKernelGGL(KERNEL, dim3((unsigned)nb), dim3(256), 0, s, logits, T, B, V, targets, seq_len, terms, grad); \
    } while (0)
    if (V <= 64) {
        if (vec) LC_XE((xent_rows_kernel<16, 4, true>), 4); else LC_XE((xent_rows_kernel<16, 4, false>), 4);
    } else if (V <= 256) {
        if (vec) LC_XE((xent_rows_kernel<64, 4, true>), 1); else LC_XE((xent_rows_kernel<64, 4, false>), 1);
    } else if (V <= 512) {
        if (vec) LC_XE((xent_rows_kernel<64, 8, true>), 1); else LC_XE((xent_rows_kernel<64, 8, false>), 1);
    } else if (V <= 1024) {
        if (vec) LC_XE((xent_rows_kernel<64, 16, true>), 1); else LC_XE((xent_rows_kernel<64, 16, false>), 1);
    } else {
        if (aligned) LC_XE((xent_wide_kernel<true>), 1); else LC_XE((xent_wide_kernel<false>), 1);
    }
#undef LC_XE
    LC_CHECK_LAUNCH("xent_rows");
    hipLaunchKernelGGL(xent_fold_kernel, dim3(B), dim3(256), 0, s, terms, T, loss, frames, correct);
    LC_CHECK_LAUNCH("xent_fold");
    return LC_OK;
}
