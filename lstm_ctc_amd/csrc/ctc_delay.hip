// ctc_delay.hip — delay-penalised CTC (Kang et al. 2023): the CTC criterion over paths weighted by exp(-lambda * E(path)),
// E = sum over the labels of the frame at which the label's run starts, plus E's expectation under that tilted posterior
// (entry_sum: the "expected frame at which a label is entered", summed over the labels).  Optional label windows mask
// emissions as in ctc_window.hip.  No reference counterpart.  DESIGN.md section 3.10.
//
// Contract: include/lstm_ctc_hip.h: lc_ctc_loss_delay.  The lattice is ctc_window.hip's (section 3.8): double cells in the
// log2 domain, one wave per (utterance, direction), PPL positions per lane, neighbours by DPP shift, -inf as "log zero".
// What is new:
//   * the arc weight w(t) = -lambda * log2(e) * t, formed and added in double, on every arc that ENTERS a label position
//     (from s-1 or s-2) at frame t; "stay" arcs and arcs into blanks carry none.  Frame 0 carries none.
//   * the backward sweep is still the forward recursion on the reversed lattice, but an arc's weight belongs to its TARGET
//     in the original orientation, which the reverse walk sees as the arc's SOURCE: a move out of an odd (label) position
//     of the previously processed row t + 1 carries w(t + 1).  (Out of an odd position p - 1 into the blank p, or out of
//     the odd p - 2 into the odd p; the move p - 1 -> p into an odd p leaves a blank and carries nothing.)
//   * cd_grad_kernel<ENTRY> also sums occupancy(t, s) * notyet(s), notyet(s) = L - (s + 1) / 2, per frame in double (each
//     lane its positions in sequence, then a fixed butterfly) into the workspace; without a gradient cd_entry_kernel does
//     the same from the two lattices alone.  cd_fold_kernel, one wave per utterance, folds an utterance's frame terms in a
//     fixed order in double and rounds once.
// Launches: lse, [index], sweep, [grad<ENTRY> | entry], [fold].  No atomics; results are bit-identical from call to call.
#include "common.h"
#include "ctc_lattice.h"
#include <float.h>
#include <limits.h>
#include <math.h>

#define CD_LOG2E 1.4426950408889634f
#define CD_LOG2E_D 1.4426950408889634
#define CD_LN2 0.6931471805599453
#define CD_OK 0
#define CD_ZERO 1                        // skipped utterance: loss 0, gradient rows zeros, entry_sum 0
#define CD_NOPATH 2                      // loss +inf, gradient = softmax on the live frames, entry_sum 0
#define CD_NAN 3                         // bad label: loss NaN, gradient rows zeros, entry_sum NaN

namespace {

// ------------------------------------------------------------------------------------------ 1. per-frame log-sum-exp
// (ctc_window.hip's cw_lse_kernel)
__global__ __launch_bounds__(256) void cd_lse_kernel(const float *__restrict__ logits, int T, int B, int V,
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
    for (int k = lane; k < V; k += 64) s += __builtin_amdgcn_exp2f((x[k] - m) * CD_LOG2E);
    s = lc_wave_sum(s);
    if (lane == 0) lse[row] = m + __builtin_amdgcn_logf(s) * (float)CD_LN2;
}

// ------------------------------------------------------------------------------------------ 2. class -> positions lists
// (ctc_window.hip's cw_index_kernel) order[b][r] = index of the label of rank r in (class, index) order; first[b][k] /
// cnt[b][k] = rank of class k's first label / number of its labels.  Every rank is below L: nothing is written out of bounds.
__global__ __launch_bounds__(256) void cd_index_kernel(int V, const int *__restrict__ labels, const int *__restrict__ offs,
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
template <int PPL>
__global__ __launch_bounds__(64) void cd_sweep_kernel(const float *__restrict__ logits, int T, int B, int V,
                                                      const int *__restrict__ labels, const int *__restrict__ offs,
                                                      const int *__restrict__ seq_len, int maxL,
                                                      const int *__restrict__ win_lo, const int *__restrict__ win_hi,
                                                      float lambda, const float *__restrict__ lse,
                                                      double *__restrict__ alpha, double *__restrict__ beta, int srow,
                                                      int want_beta, float *__restrict__ loss,
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
        if (lane == 0 && dir == 0) { loss[b] = 0.0f; lp2[b] = 0.0; status[b] = CD_ZERO; }
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
            if (lane == 0 && dir == 0) { loss[b] = __int_as_float(0x7fc00000); lp2[b] = 0.0; status[b] = CD_NAN; }
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
                if (win_lo) {
                    lo = win_lo[off + i];
                    hi = win_hi[off + i];
                }
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
    const double wl = -(double)lambda * CD_LOG2E_D;       // w(t) = wl * t

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
                const float eb = (cb[k] - lz) * CD_LOG2E;
                // forward: the arcs into a label position of this row carry w(t).  Backward (reversed lattice): the arcs out
                // of a label position of the row before, frame t + 1, carry w(t + 1) - that is p-1 -> p for an even p and
                // p-2 -> p for an odd p.  An arc p-2 -> p joins two label positions in either direction.
                const double w = wl * (double)(dir ? t + 1 : t);
                const double w1odd = dir ? 0.0 : w, w1even = dir ? w : 0.0;
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
                        const double p2 = (allow2 & 1u) ? in2 + w : NEG;
                        v = cw_lse3(a[0], p1 + ((lane & 1) ? w1odd : w1even), p2);
                        if (lane & 1) e = (cg[k][0] - lz) * CD_LOG2E;
                        live = live && t >= wlo[0] && t <= whi[0];           // blank lanes: lo = 0, hi = INT_MAX
                    } else if (j & 1) {
                        double p2 = j >= 2 ? a[j - 2] : in2;
                        p2 = (allow2 >> j & 1u) ? p2 + w : NEG;
                        v = cw_lse3(a[j], p1 + w1odd, p2);
                        e = (cg[k][g_] - lz) * CD_LOG2E;
                        live = live && t >= wlo[g_] && t <= whi[g_];
                    } else {
                        v = cw_lse2(a[j], p1 + w1even);                      // blanks are never entered from s-2
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
    // log2 of the weighted path sum: the path ends in S-1 or S-2
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
            loss[b] = INFINITY; lp2[b] = 0.0; status[b] = CD_NOPATH;
        } else {
            const double lp = hi + (double)__builtin_amdgcn_logf(1.0f + __builtin_amdgcn_exp2f((float)(lo - hi)));
            loss[b] = (float)(0.0 - lp * CD_LN2);
            lp2[b] = lp; status[b] = CD_OK;
        }
    }
}

// the wave's sum of a double in a fixed order (xor butterfly), the same value in every lane
__device__ __forceinline__ double cd_wave_sum_d(double x)
{
#pragma unroll
    for (int mask = 1; mask < 64; mask <<= 1) {
        const int lo = __shfl_xor(__double2loint(x), mask, 64), hi = __shfl_xor(__double2hiint(x), mask, 64);
        x += __hiloint2double(hi, lo);
    }
    return x;
}

// ------------------------------------------------------------------------------------------ 4. gradient (+ entry terms)
template <bool ENTRY>
__global__ __launch_bounds__(256) void cd_grad_kernel(const float *__restrict__ logits, int T, int B, int V,
                                                      const int *__restrict__ offs, const int *__restrict__ seq_len,
                                                      const float *__restrict__ lse, const double *__restrict__ alpha,
                                                      const double *__restrict__ beta, int srow,
                                                      const double *__restrict__ lp2, const int *__restrict__ status,
                                                      const int *__restrict__ order, int pitch,
                                                      const int *__restrict__ first, const int *__restrict__ cnt,
                                                      float *__restrict__ grad, double *__restrict__ fterm)
{
    const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= (size_t)T * B) return;
    const int t = (int)(row / B), b = (int)(row % B);
    const int Tb = min(max(seq_len[b], 0), T);
    const int st = status[b];
    const float *x = logits + row * V;
    float *g = grad + row * V;
    if (t >= Tb || st == CD_ZERO || st == CD_NAN) {                          // wave-uniform
        for (int k = lane; k < V; k += 64) g[k] = 0.0f;
        return;
    }
    const float lz = lse[row];
    if (st == CD_NOPATH) {
        for (int k = lane; k < V; k += 64) g[k] = __builtin_amdgcn_exp2f((x[k] - lz) * CD_LOG2E);
        return;
    }
    const int L = offs[b + 1] - offs[b], S = 2 * L + 1;
    const size_t bt = (size_t)b * T + t;
    const double *A = alpha + bt * srow, *Bt = beta + bt * srow;
    const double lp = lp2[b];
    const int blank = V - 1;
    double eacc = 0.0;                                                       // this lane's sum of occupancy * notyet
    // the blank: positions 0, 2, .., 2L, lane l takes 2l, 2l + 128, ... in sequence, then the wave's fixed reduction
    const float eb = (x[blank] - lz) * CD_LOG2E;
    {
        const double c = (double)eb + lp;
        float acc = 0.0f;
        for (int s = 2 * lane; s < S; s += 128) {
            const float o = __builtin_amdgcn_exp2f((float)((A[s] + Bt[S - 1 - s]) - c));
            acc += o;
            if (ENTRY) eacc += (double)o * (double)(L - (s >> 1));
        }
        acc = lc_wave_sum(acc);
        if (lane == 0) g[blank] = __builtin_amdgcn_exp2f(eb) - acc;
    }
    // the labels: lane k sums the positions of class k in the order of the utterance's list
    const int *ord = order + (size_t)b * pitch;
    const int *fr = first + (size_t)b * V, *cn = cnt + (size_t)b * V;
    for (int k = lane; k < blank; k += 64) {
        const float e = (x[k] - lz) * CD_LOG2E;
        const double c = (double)e + lp;
        const int r0 = fr[k], n = cn[k];
        float acc = 0.0f;
        for (int r = 0; r < n; ++r) {
            const int i = ord[r0 + r], s = 2 * i + 1;
            const float o = __builtin_amdgcn_exp2f((float)((A[s] + Bt[S - 1 - s]) - c));
            acc += o;
            if (ENTRY) eacc += (double)o * (double)(L - 1 - i);
        }
        g[k] = __builtin_amdgcn_exp2f(e) - acc;
    }
    if (ENTRY) {
        eacc = cd_wave_sum_d(eacc);
        if (lane == 0) fterm[bt] = eacc;
    }
}

// ------------------------------------------------------------------------------------------ 4'. entry terms alone
// One wave per live frame of an utterance with a path: sum_s occupancy(t, s) * notyet(s), lane l takes s = l, l + 64, ...
__global__ __launch_bounds__(256) void cd_entry_kernel(const float *__restrict__ logits, int T, int B, int V,
                                                       const int *__restrict__ labels, const int *__restrict__ offs,
                                                       const int *__restrict__ seq_len, const float *__restrict__ lse,
                                                       const double *__restrict__ alpha, const double *__restrict__ beta,
                                                       int srow, const double *__restrict__ lp2,
                                                       const int *__restrict__ status, double *__restrict__ fterm)
{
    const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= (size_t)T * B) return;
    const int t = (int)(row / B), b = (int)(row % B);
    const int Tb = min(max(seq_len[b], 0), T);
    if (t >= Tb || status[b] != CD_OK) return;                               // wave-uniform; the fold never reads these
    const float *x = logits + row * V;
    const float lz = lse[row];
    const int off = offs[b], L = offs[b + 1] - off, S = 2 * L + 1;
    const size_t bt = (size_t)b * T + t;
    const double *A = alpha + bt * srow, *Bt = beta + bt * srow;
    const double lp = lp2[b];
    double eacc = 0.0;
    for (int s = lane; s < S; s += 64) {
        const int sym = (s & 1) ? labels[off + (s >> 1)] : V - 1;            // status OK: every label lies in [0, V-1)
        const float e = (x[sym] - lz) * CD_LOG2E;
        const float o = __builtin_amdgcn_exp2f((float)((A[s] + Bt[S - 1 - s]) - ((double)e + lp)));
        eacc += (double)o * (double)(L - ((s + 1) >> 1));
    }
    eacc = cd_wave_sum_d(eacc);
    if (lane == 0) fterm[bt] = eacc;
}

// ------------------------------------------------------------------------------------------ 5. per-utterance fold
// One wave per utterance: lane l sums the terms of frames l, l + 64, ... in sequence, then the fixed butterfly; rounded once.
__global__ __launch_bounds__(64) void cd_fold_kernel(const double *__restrict__ fterm, int T, const int *__restrict__ seq_len,
                                                     const int *__restrict__ status, float *__restrict__ entry_sum)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    const int st = status[b];
    if (st != CD_OK) {
        if (lane == 0) entry_sum[b] = st == CD_NAN ? __int_as_float(0x7fc00000) : 0.0f;
        return;
    }
    const int Tb = min(max(seq_len[b], 0), T);
    const double *f = fterm + (size_t)b * T;
    double acc = 0.0;
    for (int t = lane; t < Tb; t += 64) acc += f[t];
    acc = cd_wave_sum_d(acc);
    if (lane == 0) entry_sum[b] = (float)acc;
}

inline size_t cd_align256(size_t x) { return (x + 255) & ~(size_t)255; }
inline int cd_ppl(int S) { return S <= 64 ? 1 : S <= 128 ? 2 : S <= 256 ? 4 : S <= 512 ? 8 : S <= 1024 ? 16 : 32; }
struct CdLayout {
    size_t lse, status, lp2, order, first, cnt, fterm, alpha, beta, total;
    int ppl, srow, pitch;
};
inline CdLayout cd_layout(int T, int B, int V, int max_label_len)
{
    CdLayout m;
    const int S = 2 * max_label_len + 1;
    m.ppl = cd_ppl(S);
    m.srow = (S + 63) / 64 * 64;                         // <= 64 * ppl
    m.pitch = max_label_len > 0 ? max_label_len : 1;
    const size_t TB = (size_t)T * B;
    size_t o = 0;
    m.lse = o; o += cd_align256(TB * sizeof(float));
    m.status = o; o += cd_align256((size_t)B * sizeof(int));
    m.lp2 = o; o += cd_align256((size_t)B * sizeof(double));
    m.order = o; o += cd_align256((size_t)B * m.pitch * sizeof(int));
    m.first = o; o += cd_align256((size_t)B * V * sizeof(int));
    m.cnt = o; o += cd_align256((size_t)B * V * sizeof(int));
    m.fterm = o; o += cd_align256(TB * sizeof(double));
    m.alpha = o; o += cd_align256(TB * m.srow * sizeof(double));
    m.beta = o; o += cd_align256(TB * m.srow * sizeof(double));
    m.total = o;
    return m;
}

}  // namespace

extern "C" size_t lc_ctc_delay_workspace_bytes(int T, int B, int V, int max_label_len)
{
    if (T <= 0 || B <= 0 || V < 2 || max_label_len < 0 || max_label_len > 1023) return 0;
    return cd_layout(T, B, V, max_label_len).total;
}

extern "C" int lc_ctc_loss_delay(const float *logits, int T, int B, int V, const int *labels, const int *label_offsets,
                                 const int *seq_len, int max_label_len, const int *win_lo, const int *win_hi,
                                 float delay_penalty, float *loss, float *entry_sum, float *grad, void *workspace,
                                 size_t workspace_bytes, lc_stream_t stream)
{
    LC_CHECK_ARG(logits && labels && label_offsets && seq_len && loss && workspace, "lc_ctc_loss_delay: null pointer");
    LC_CHECK_ARG((win_lo == nullptr) == (win_hi == nullptr), "lc_ctc_loss_delay: win_lo and win_hi go together (both or none)");
    LC_CHECK_ARG(T > 0 && B > 0 && V >= 2 && max_label_len >= 0, "lc_ctc_loss_delay: bad shape T=%d B=%d V=%d L=%d", T, B, V,
                 max_label_len);
    LC_CHECK_ARG(max_label_len <= 1023, "lc_ctc_loss_delay: label length %d exceeds the supported maximum 1023",
                 max_label_len);
    LC_CHECK_ARG(isfinite(delay_penalty), "lc_ctc_loss_delay: delay_penalty must be finite, got %g", (double)delay_penalty);
    LC_CHECK_ARG((long long)B * 2 <= 0x7fffffffLL && ((long long)T * B + 3) / 4 <= 0x7fffffffLL,
                 "lc_ctc_loss_delay: T * B = %lld is beyond the launch grid", (long long)T * B);
    const CdLayout m = cd_layout(T, B, V, max_label_len);
    if (workspace_bytes < m.total) {
        lc_set_error("lc_ctc_loss_delay: workspace too small (%zu < %zu)", workspace_bytes, m.total);
        return LC_EWORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    char *w = (char *)workspace;
    float *lse = (float *)(w + m.lse);
    int *status = (int *)(w + m.status);
    double *lp2 = (double *)(w + m.lp2);
    int *order = (int *)(w + m.order), *first = (int *)(w + m.first), *cnt = (int *)(w + m.cnt);
    double *fterm = (double *)(w + m.fterm);
    double *alpha = (double *)(w + m.alpha), *beta = (double *)(w + m.beta);
    const unsigned frame_blocks = (unsigned)(((long long)T * B + 3) / 4);
    hipLaunchKernelGGL(cd_lse_kernel, dim3(frame_blocks), dim3(256), 0, s, logits, T, B, V, seq_len, lse);
    LC_CHECK_LAUNCH("ctc_delay_lse");
    if (grad) {
        hipLaunchKernelGGL(cd_index_kernel, dim3(B), dim3(256), 0, s, V, labels, label_offsets, max_label_len, m.pitch, order,
                           first, cnt);
        LC_CHECK_LAUNCH("ctc_delay_index");
    }
#define LC_CD(PPL)                                                                                                     \
    hipLaunchKernelGGL(cd_sweep_kernel<PPL>, dim3(2 * B), dim3(64), 0, s, logits, T, B, V, labels, label_offsets, seq_len, \
                       max_label_len, win_lo, win_hi, delay_penalty, lse, alpha, beta, m.srow, (grad || entry_sum) ? 1 : 0, \
                       loss, lp2, status)
    switch (m.ppl) {
    case 1: LC_CD(1); break;
    case 2: LC_CD(2); break;
    case 4: LC_CD(4); break;
    case 8: LC_CD(8); break;
    case 16: LC_CD(16); break;
    default: LC_CD(32); break;
    }
#undef LC_CD
    LC_CHECK_LAUNCH("ctc_delay_sweep");
    if (grad && entry_sum) {
        hipLaunchKernelGGL(cd_grad_kernel<true>, dim3(frame_blocks), dim3(256), 0, s, logits, T, B, V, label_offsets, seq_len,
                           lse, alpha, beta, m.srow, lp2, status, order, m.pitch, first, cnt, grad, fterm);
        LC_CHECK_LAUNCH("ctc_delay_grad");
    } else if (grad) {
        hipLaunchKernelGGL(cd_grad_kernel<false>, dim3(frame_blocks), dim3(256), 0, s, logits, T, B, V, label_offsets, seq_len,
                           lse, alpha, beta, m.srow, lp2, status, order, m.pitch, first, cnt, grad, fterm);
        LC_CHECK_LAUNCH("ctc_delay_grad");
    } else if (entry_sum) {
        hipLaunchKernelGGL(cd_entry_kernel, dim3(frame_blocks), dim3(256), 0, s, logits, T, B, V, labels, label_offsets,
                           seq_len, lse, alpha, beta, m.srow, lp2, status, fterm);
        LC_CHECK_LAUNCH("ctc_delay_entry");
    }
    if (entry_sum) {
        hipLaunchKernelGGL(cd_fold_kernel, dim3(B), dim3(64), 0, s, fterm, T, seq_len, status, entry_sum);
        LC_CHECK_LAUNCH("ctc_delay_fold");
    }
    return LC_OK;
}
