// ctc_window.hip — alignment-windowed CTC: the CTC loss and gradient summed only over the paths that keep every label inside
// a window of frames (Senior et al. 2015: windows around a forced alignment stop a unidirectional model emitting late).
// No reference counterpart.  DESIGN.md section 3.8.  lc_ctc_loss (ctc.hip) is not touched by this file.
//
// Contract (include/lstm_ctc_hip.h: lc_ctc_loss_windowed): lc_ctc_loss's, plus win_lo / win_hi parallel to the flat labels.
// Label j may sit on frame t only when win_lo[j] <= t <= win_hi[j]; blank positions are never constrained.
//
// Four launches per call (two without a gradient), no LDS atomics, no global atomics, every sum in a fixed order - the result
// is bit-identical from call to call:
//   1. cw_lse_kernel         one wave per live frame (t, b): lse[t, b] = log sum_k exp(logits[t, b, k]), fp32.
//   2. cw_index_kernel       (gradient only) one workgroup per utterance: the label indices ordered by (class, index), and per
//                            class the first rank and the count.  Ranks come from counting, so the order is a pure function
//                            of the labels.
//   3. cw_sweep_kernel<PPL>  one wave per (utterance, direction), 2B waves, no barrier.  ctc_align.hip's geometry: lane l holds
//      the PPL consecutive lattice positions l * PPL .. l * PPL + PPL - 1, the s-1 / s-2 neighbours of its first position come
//      by one DPP wave shift.  BOTH directions are the same forward recursion: direction 1 walks the frames backwards over the
//      REVERSED lattice (position p stands for lattice position S - 1 - p; S is odd, so label positions stay odd and the
//      "s-2 only between different labels" rule is symmetric), which yields beta INCLUDING the frame's own emission.  A cell
//      is a DOUBLE in the log2 domain (v_exp_f32 / v_log_f32 are base 2), as in ctc_align.hip: the log-sum-exp of a cell's
//      predecessors is m + log2(sum 2^(a_i - m)) with the differences rounded to fp32 and the exponentials and the logarithm
//      on the fp32 pipes (a term far below the maximum has no weight, so its rounding does not matter), and m + ., + emission
//      are double additions - a cell's error is a few fp32 ulps of a number below 2, whatever the cell's magnitude, and there
//      is no re-centring and no offset to carry.  (fp32 cells re-centred on the row maximum were built first: the cells that
//      carry the paths lie hundreds of bits below the best PREFIX when windows or a tight T force the path, and the
//      gradient error reached the project's 1e-4 bar at T = 164.)  A cell's emission is the fp32 log-softmax
//      (logits - lse) * log2(e).  "Log zero" is -inf itself: a masked cell (frame outside the label's window) is set to -inf
//      by a select, and the log-sum-exp takes its maximum through fmax(m, -DBL_MAX), so that an all-dead neighbourhood gives
//      -DBL_MAX + log2(0) = -inf and never -inf - -inf: a dead cell stays dead and no NaN can arise, also when every cell of
//      a row is dead.  The rows go to the workspace.  Direction 0 finishes with log2 p = log-sum-exp of the two end cells
//      and the loss, rounded once.
//   4. cw_grad_kernel        one wave per frame.  occupancy(t, s) = 2^(alpha + beta - emission - log2 p), the exponent formed in double; lane k
//      sums the positions of class k, k + 64, ... in the order of cw_index_kernel's list, the blank's positions are summed
//      lane by lane and then by the wave's DPP reduction.  grad = softmax - occupancy.
// The band (only positions whose window contains t are live) is NOT exploited: every position is computed on every frame.
#include "common.h"
#include "ctc_lattice.h"
#include <float.h>
#include <limits.h>
#include <math.h>

#define CW_LOG2E 1.4426950408889634f
#define CW_LN2 0.6931471805599453
#define CW_OK 0
#define CW_ZERO 1                        // loss already written, gradient rows are zeros (skipped utterance, bad label)
#define CW_NOPATH 2                      // loss +inf, gradient = softmax on the live frames

namespace {

// ------------------------------------------------------------------------------------------ 1. per-frame log-sum-exp
__global__ __launch_bounds__(256) void cw_lse_kernel(const float *__restrict__ logits, int T, int B, int V,
                                                     const int *__restrict__ seq_len, float *__restrict__ lse)
{
    const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= (size_t)T * B) return;
    const int t = (int)(row / B), b = (int)(row % B);
    if (t >= seq_len[b]) return;                                  // never read
    const float *x = logits + row * V;
    float m = -INFINITY;
    for (int k = lane; k < V; k += 64) m = fmaxf(m, x[k]);
    m = lc_wave_max(m);
    float s = 0.0f;
    for (int k = lane; k < V; k += 64) s += __builtin_amdgcn_exp2f((x[k] - m) * CW_LOG2E);
    s = lc_wave_sum(s);
    if (lane == 0) lse[row] = m + __builtin_amdgcn_logf(s) * (float)CW_LN2;
}

// ------------------------------------------------------------------------------------------ 2. class -> positions lists
// order[b][r] = index of the label of rank r in (class, index) order; first[b][k] / cnt[b][k] = rank of class k's first
// label / number of its labels.  Labels outside [0, V) take part in the ranking but belong to no class (the sweep gives such
// an utterance a NaN loss and nothing reads its lists); every rank is below L, so nothing is written out of bounds.
__global__ __launch_bounds__(256) void cw_index_kernel(int V, const int *__restrict__ labels, const int *__restrict__ offs,
                                                       int maxL, int pitch, int *__restrict__ order,
                                                       int *__restrict__ first, int *__restrict__ cnt)
{
    __shared__ int lab[1024];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int off = offs[b];
    int L = offs[b + 1] - off;
    if (L < 0 || L > maxL) L = 0;
    for (int i = tid; i < L; i += 256) lab[i] = labels[off + i];
    __syncthreads();
    int *ord = order + (size_t)b * pitch;
    for (int i = tid; i < L; i += 256) {
        const int me = lab[i];
        int rank = 0;
        for (int j = 0; j < L; ++j) {
            const int o = lab[j];
            rank += (o < me || (o == me && j < i)) ? 1 : 0;
        }
        ord[rank] = i;
    }
    for (int k = tid; k < V; k += 256) {
        int lt = 0, eq = 0;
        for (int j = 0; j < L; ++j) {
            const int o = lab[j];
            lt += o < k ? 1 : 0;
            eq += o == k ? 1 : 0;
        }
        first[(size_t)b * V + k] = lt;
        cnt[(size_t)b * V + k] = eq;
    }
}

// ------------------------------------------------------------------------------------------ 3. alpha / beta sweeps
// cw_neg_inf / cw_lse2 / cw_lse3 / cw_shr1 / cw_readlane: ctc_lattice.h (shared with ctc_delay.hip)
template <int PPL>
__global__ __launch_bounds__(64) void cw_sweep_kernel(const float *__restrict__ logits, int T, int B, int V,
                                                      const int *__restrict__ labels, const int *__restrict__ offs,
                                                      const int *__restrict__ seq_len, int maxL,
                                                      const int *__restrict__ win_lo, const int *__restrict__ win_hi,
                                                      const float *__restrict__ lse, double *__restrict__ alpha,
                                                      double *__restrict__ beta, int srow, int want_beta,
                                                      float *__restrict__ loss,
                                                      double *__restrict__ lp2, int *__restrict__ status)
{
    constexpr int K = PPL <= 4 ? 8 : 32 / PPL;            // frames fetched ahead as one chunk: 8, 8, 8, 4, 2, 1
    constexpr int NG = PPL == 1 ? 1 : PPL / 2;            // label positions (gathers, windows) per lane
    const int b = blockIdx.x >> 1, dir = blockIdx.x & 1, lane = threadIdx.x;
    if (dir == 1 && !want_beta) return;
    const int Tb = min(max(seq_len[b], 0), T);
    const int off = offs[b], L = offs[b + 1] - off, S = 2 * L + 1;
    const int blank = V - 1;
    const double NEG = cw_neg_inf();
    if (Tb == 0 || L > Tb) {                              // lc_ctc_loss: the utterance is skipped, loss 0, gradient 0
        if (lane == 0 && dir == 0) { loss[b] = 0.0f; lp2[b] = 0.0; status[b] = CW_ZERO; }
        return;
    }
    {   // a label outside [0, V-1) (or a label count the workspace was not sized for): NaN loss, zero gradient, and the labels
        // never index anything
        int bad = (L < 0 || L > maxL) ? 1 : 0;
        if (!bad)
            for (int i = lane; i < L; i += 64) {
                const int lab = labels[off + i];
                bad |= (lab < 0 || lab >= blank) ? 1 : 0;
            }
        if (__builtin_amdgcn_ballot_w64(bad != 0) != 0) {
            if (lane == 0 && dir == 0) { loss[b] = __int_as_float(0x7fc00000); lp2[b] = 0.0; status[b] = CW_ZERO; }
            return;
        }
    }
    // per position: is it inside the lattice, may it be entered from two positions back; per label position: class, window
    unsigned valid = 0, allow2 = 0;
    int gsym[NG], wlo[NG], whi[NG];
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
        const int p = lane * PPL + j;
        if (p < S) valid |= 1u << j;
        if (PPL == 1 || (j & 1)) {
            int sym = blank, lo = 0, hi = INT_MAX;
            if ((p & 1) && p < S) {
                const int i = dir ? L - 1 - (p >> 1) : (p >> 1);          // the label this position stands for
                sym = labels[off + i];
                lo = win_lo[off + i];
                hi = win_hi[off + i];
                if (p >= 3 && sym != labels[off + (dir ? i + 1 : i - 1)]) allow2 |= 1u << j;
            }
            gsym[PPL == 1 ? 0 : j >> 1] = sym;
            wlo[PPL == 1 ? 0 : j >> 1] = lo;
            whi[PPL == 1 ? 0 : j >> 1] = hi;
        }
    }
    double a[PPL];
#pragma unroll
    for (int j = 0; j < PPL; ++j) a[j] = NEG;
    if (lane == 0) a[0] = 0.0;                            // "before the first frame": it reaches positions 0 (stay) and 1

    float cg[K][NG], cb[K], cl[K], ng[K][NG], nb[K], nl[K];
    auto fetch = [&](int k0, float (&g)[K][NG], float (&gb)[K], float (&gl)[K]) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int kk = min(k0 + k, Tb - 1);
            const int t = dir ? Tb - 1 - kk : kk;
            const size_t row = (size_t)t * B + b;
            const float *x = logits + row * V;
#pragma unroll
            for (int g_ = 0; g_ < NG; ++g_) g[k][g_] = x[gsym[g_]];
            gb[k] = x[blank];
            gl[k] = lse[row];
        }
    };
    fetch(0, cg, cb, cl);
    double *rows = (dir ? beta : alpha) + (size_t)b * T * srow;
    for (int k0 = 0; k0 < Tb; k0 += K) {
        fetch(k0 + K, ng, nb, nl);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int kk = k0 + k;
            if (kk < Tb) {
                const int t = dir ? Tb - 1 - kk : kk;
                const float lz = cl[k];
                const float eb = (cb[k] - lz) * CW_LOG2E;
                const double in1 = cw_shr1(a[PPL - 1]);
                const double in2 = PPL == 1 ? cw_shr1(in1) : in1;            // s-2 of the lane's first label position
#pragma unroll
                for (int j = PPL - 1; j >= 0; --j) {                         // descending: a[j-1], a[j-2] are the old frame's
                    const double p1 = j >= 1 ? a[j - 1] : in1;
                    const int g_ = PPL == 1 ? 0 : j >> 1;
                    double v;
                    float e = eb;
                    bool live = (valid >> j & 1u) != 0;
                    if (PPL == 1) {
                        const double p2 = (allow2 & 1u) ? in2 : NEG;
                        v = cw_lse3(a[0], p1, p2);
                        if (lane & 1) e = (cg[k][0] - lz) * CW_LOG2E;
                        live = live && t >= wlo[0] && t <= whi[0];           // blank lanes: lo = 0, hi = INT_MAX
                    } else if (j & 1) {
                        double p2 = j >= 2 ? a[j - 2] : in2;
                        p2 = (allow2 >> j & 1u) ? p2 : NEG;
                        v = cw_lse3(a[j], p1, p2);
                        e = (cg[k][g_] - lz) * CW_LOG2E;
                        live = live && t >= wlo[g_] && t <= whi[g_];
                    } else {
                        v = cw_lse2(a[j], p1);                               // blanks are never entered from s-2
                    }
                    a[j] = live ? v + (double)e : NEG;
                }
                // the row
                double *dst = rows + (size_t)t * srow;
                if constexpr (PPL == 1) {
                    dst[lane] = a[0];                                        // srow >= 64
                } else {
#pragma unroll
                    for (int c = 0; c < PPL / 2; ++c) {
                        const int p0 = lane * PPL + 2 * c;                   // srow is a multiple of 64: both or none
                        if (p0 < srow) *(double2 *)(dst + p0) = make_double2(a[2 * c], a[2 * c + 1]);
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
#pragma unroll
            for (int g_ = 0; g_ < NG; ++g_) cg[k][g_] = ng[k][g_];
            cb[k] = nb[k];
            cl[k] = nl[k];
        }
    }
    if (dir == 1) return;
    // log2 p: the path ends in S-1 or S-2
    const int s1 = S - 1, s2 = S - 2;
    double m1 = NEG, m2 = NEG;
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
        if (j == (s1 & (PPL - 1))) m1 = a[j];
        if (s2 >= 0 && j == (s2 & (PPL - 1))) m2 = a[j];
    }
    const double v1 = cw_readlane(m1, s1 / PPL);
    const double v2 = s2 >= 0 ? cw_readlane(m2, s2 / PPL) : NEG;
    if (lane == 0) {
        const double hi = fmax(v1, v2), lo = fmin(v1, v2);
        if (!(hi > NEG)) {                                                   // no surviving path
            loss[b] = INFINITY; lp2[b] = 0.0; status[b] = CW_NOPATH;
        } else {
            const double lp = hi + (double)__builtin_amdgcn_logf(1.0f + __builtin_amdgcn_exp2f((float)(lo - hi)));
            loss[b] = (float)(0.0 - lp * CW_LN2);
            lp2[b] = lp; status[b] = CW_OK;
        }
    }
}

// ------------------------------------------------------------------------------------------ 4. gradient
__global__ __launch_bounds__(256) void cw_grad_kernel(const float *__restrict__ logits, int T, int B, int V,
                                                      const int *__restrict__ offs, const int *__restrict__ seq_len,
                                                      const float *__restrict__ lse, const double *__restrict__ alpha,
                                                      const double *__restrict__ beta, int srow,
                                                      const double *__restrict__ lp2, const int *__restrict__ status,
                                                      const int *__restrict__ order, int pitch,
                                                      const int *__restrict__ first, const int *__restrict__ cnt,
                                                      float *__restrict__ grad)
{
    const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= (size_t)T * B) return;
    const int t = (int)(row / B), b = (int)(row % B);
    const int Tb = min(max(seq_len[b], 0), T);
    const int st = status[b];
    const float *x = logits + row * V;
    float *g = grad + row * V;
    if (t >= Tb || st == CW_ZERO) {                                          // wave-uniform
        for (int k = lane; k < V; k += 64) g[k] = 0.0f;
        return;
    }
    const float lz = lse[row];
    if (st == CW_NOPATH) {
        for (int k = lane; k < V; k += 64) g[k] = __builtin_amdgcn_exp2f((x[k] - lz) * CW_LOG2E);
        return;
    }
    const int L = offs[b + 1] - offs[b], S = 2 * L + 1;
    const size_t bt = (size_t)b * T + t;
    const double *A = alpha + bt * srow, *Bt = beta + bt * srow;
    const double lp = lp2[b];
    const int blank = V - 1;
    // the blank: positions 0, 2, .., 2L, lane l takes 2l, 2l + 128, ... in sequence, then the wave's fixed reduction
    const float eb = (x[blank] - lz) * CW_LOG2E;
    {
        const double c = (double)eb + lp;
        float acc = 0.0f;
        for (int s = 2 * lane; s < S; s += 128) acc += __builtin_amdgcn_exp2f((float)((A[s] + Bt[S - 1 - s]) - c));
        acc = lc_wave_sum(acc);
        if (lane == 0) g[blank] = __builtin_amdgcn_exp2f(eb) - acc;
    }
    // the labels: lane k sums the positions of class k in the order of the utterance's list
    const int *ord = order + (size_t)b * pitch;
    const int *fr = first + (size_t)b * V, *cn = cnt + (size_t)b * V;
    for (int k = lane; k < blank; k += 64) {
        const float e = (x[k] - lz) * CW_LOG2E;
        const double c = (double)e + lp;
        const int r0 = fr[k], n = cn[k];
        float acc = 0.0f;
        for (int r = 0; r < n; ++r) {
            const int s = 2 * ord[r0 + r] + 1;
            acc += __builtin_amdgcn_exp2f((float)((A[s] + Bt[S - 1 - s]) - c));
        }
        g[k] = __builtin_amdgcn_exp2f(e) - acc;
    }
}

inline size_t cw_align256(size_t x) { return (x + 255) & ~(size_t)255; }
inline int cw_ppl(int S) { return S <= 64 ? 1 : S <= 128 ? 2 : S <= 256 ? 4 : S <= 512 ? 8 : S <= 1024 ? 16 : 32; }
struct CwLayout {
    size_t lse, status, lp2, order, first, cnt, alpha, beta, total;
    int ppl, srow, pitch;
};
inline CwLayout cw_layout(int T, int B, int V, int max_label_len)
{
    CwLayout m;
    const int S = 2 * max_label_len + 1;
    m.ppl = cw_ppl(S);
    m.srow = (S + 63) / 64 * 64;                         // <= 64 * ppl
    m.pitch = max_label_len > 0 ? max_label_len : 1;
    const size_t TB = (size_t)T * B;
    size_t o = 0;
    m.lse = o; o += cw_align256(TB * sizeof(float));
    m.status = o; o += cw_align256((size_t)B * sizeof(int));
    m.lp2 = o; o += cw_align256((size_t)B * sizeof(double));
    m.order = o; o += cw_align256((size_t)B * m.pitch * sizeof(int));
    m.first = o; o += cw_align256((size_t)B * V * sizeof(int));
    m.cnt = o; o += cw_align256((size_t)B * V * sizeof(int));
    m.alpha = o; o += cw_align256(TB * m.srow * sizeof(double));
    m.beta = o; o += cw_align256(TB * m.srow * sizeof(double));
    m.total = o;
    return m;
}

}  // namespace

extern "C" size_t lc_ctc_window_workspace_bytes(int T, int B, int V, int max_label_len)
{
    if (T <= 0 || B <= 0 || V < 2 || max_label_len < 0 || max_label_len > 1023) return 0;
    return cw_layout(T, B, V, max_label_len).total;
}

extern "C" int lc_ctc_loss_windowed(const float *logits, int T, int B, int V, const int *labels, const int *label_offsets,
                                    const int *seq_len, int max_label_len, const int *win_lo, const int *win_hi,
                                    float *loss, float *grad, void *workspace, size_t workspace_bytes, lc_stream_t stream)
{
    LC_CHECK_ARG(logits && labels && label_offsets && seq_len && win_lo && win_hi && loss && workspace,
                 "lc_ctc_loss_windowed: null pointer");
    LC_CHECK_ARG(T > 0 && B > 0 && V >= 2 && max_label_len >= 0, "lc_ctc_loss_windowed: bad shape T=%d B=%d V=%d L=%d", T, B,
                 V, max_label_len);
    LC_CHECK_ARG(max_label_len <= 1023, "lc_ctc_loss_windowed: label length %d exceeds the supported maximum 1023",
                 max_label_len);
    LC_CHECK_ARG((long long)B * 2 <= 0x7fffffffLL && ((long long)T * B + 3) / 4 <= 0x7fffffffLL,
                 "lc_ctc_loss_windowed: T * B = %lld is beyond the launch grid", (long long)T * B);
    const CwLayout m = cw_layout(T, B, V, max_label_len);
    if (workspace_bytes < m.total) {
        lc_set_error("lc_ctc_loss_windowed: workspace too small (%zu < %zu)", workspace_bytes, m.total);
        return LC_EWORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    char *w = (char *)workspace;
    float *lse = (float *)(w + m.lse);
    int *status = (int *)(w + m.status);
    double *lp2 = (double *)(w + m.lp2);
    int *order = (int *)(w + m.order), *first = (int *)(w + m.first), *cnt = (int *)(w + m.cnt);
    double *alpha = (double *)(w + m.alpha), *beta = (double *)(w + m.beta);
    const unsigned frame_blocks = (unsigned)(((long long)T * B + 3) / 4);
    hipLaunchKernelGGL(cw_lse_kernel, dim3(frame_blocks), dim3(256), 0, s, logits, T, B, V, seq_len, lse);
    LC_CHECK_LAUNCH("ctc_window_lse");
    if (grad) {
        hipLaunchKernelGGL(cw_index_kernel, dim3(B), dim3(256), 0, s, V, labels, label_offsets, max_label_len, m.pitch, order,
                           first, cnt);
        LC_CHECK_LAUNCH("ctc_window_index");
    }
#define LC_CW(PPL)                                                                                                     \
    hipLaunchKernelGGL(cw_sweep_kernel<PPL>, dim3(2 * B), dim3(64), 0, s, logits, T, B, V, labels, label_offsets, seq_len, \
                       max_label_len, win_lo, win_hi, lse, alpha, beta, m.srow, grad ? 1 : 0, loss, lp2, status)
    switch (m.ppl) {
    case 1: LC_CW(1); break;
    case 2: LC_CW(2); break;
    case 4: LC_CW(4); break;
    case 8: LC_CW(8); break;
    case 16: LC_CW(16); break;
    default: LC_CW(32); break;
    }
#undef LC_CW
    LC_CHECK_LAUNCH("ctc_window_sweep");
    if (grad) {
        hipLaunchKernelGGL(cw_grad_kernel, dim3(frame_blocks), dim3(256), 0, s, logits, T, B, V, label_offsets, seq_len, lse,
                           alpha, beta, m.srow, lp2, status, order, m.pitch, first, cnt, grad);
        LC_CHECK_LAUNCH("ctc_window_grad");
    }
    return LC_OK;
}
