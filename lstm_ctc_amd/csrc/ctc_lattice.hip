// ctc_lattice.hip — the four CTC criteria that sum over a constrained or re-weighted set of paths, carry a second quantity
// along them, or relax what a lattice cell emits, on one lattice:
//   * alignment-windowed CTC (lc_ctc_loss_windowed): the CTC loss and gradient summed only over the paths that keep every label
//     inside a window of frames (Senior et al. 2015: windows around a forced alignment stop a unidirectional model emitting
//     late).  DESIGN.md section 3.8.
//   * delay-penalised CTC (lc_ctc_loss_delay, Kang et al. 2023): the CTC criterion over paths weighted by exp(-lambda * E(path)),
//     E = sum over the labels of the frame at which the label's run starts, plus E's expectation under that tilted posterior
//     (entry_sum: the "expected frame at which a label is entered", summed over the labels), with optional label windows.
//     DESIGN.md section 3.10.
//   * maximum-entropy CTC (lc_ctc_loss_entropy, Liu et al. 2018): the (windowed) CTC loss, the entropy H = log Z - Ebar of the
//     posterior over the feasible paths (Ebar = the posterior mean of log p(path)), and the exact gradient of loss - eta H,
//     with optional label windows.  DESIGN.md section 3.14.
//   * transcript-tolerant CTC (lc_ctc_loss_star, after OTC / BTC, Gao et al. 2023, and STC, Pratap et al. 2022): every lattice
//     position may explain a frame by a penalised star, "some non-blank class", instead of by its own class; the loss over
//     these mixture emissions, the expected number of frames the star explains (star_frames) and the exact gradient, with
//     optional label windows.  DESIGN.md section 3.15.
// No reference counterpart.  lc_ctc_loss (ctc.hip) is not touched by this file.
//
// Contract (include/lstm_ctc_hip.h): lc_ctc_loss's, plus win_lo / win_hi parallel to the flat labels.  Label j may sit on
// frame t only when win_lo[j] <= t <= win_hi[j]; blank positions are never constrained.
//
// All entries run lat_launch: lse, [index], sweep, [grad<ENTRY, ENT, STAR> | entry], [fold] - four launches for the windowed and
// the entropy loss (two without a gradient), five for the star entry with and without one.  No LDS atomics, no global atomics, every sum in a fixed order - the result is bit-identical from call
// to call:
//   1. lat_lse_kernel        (ctc_lattice.h) one wave per live frame (t, b): lse[t, b] = log sum_k exp(logits[t, b, k]), fp32.
//   2. lat_index_kernel      (gradient only) one workgroup per utterance: the label indices ordered by (class, index), and per
//                            class the first rank and the count.  Ranks come from counting, so the order is a pure function
//                            of the labels.
//   3. lat_sweep_kernel<PPL, DELAY>  one wave per (utterance, direction), 2B waves, no barrier.  ctc_align.hip's geometry: lane l
//      holds the PPL consecutive lattice positions l * PPL .. l * PPL + PPL - 1, the s-1 / s-2 neighbours of its first position
//      come by one DPP wave shift.  BOTH directions are the same forward recursion: direction 1 walks the frames backwards over
//      the REVERSED lattice (position p stands for lattice position S - 1 - p; S is odd, so label positions stay odd and the
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
//      DELAY (lc_ctc_loss_delay; the windowed instantiation carries none of it):
//        * the arc weight w(t) = -lambda * log2(e) * t, formed and added in double, on every arc that ENTERS a label position
//          (from s-1 or s-2) at frame t; "stay" arcs and arcs into blanks carry none.  Frame 0 carries none.
//        * the backward sweep is still the forward recursion on the reversed lattice, but an arc's weight belongs to its
//          TARGET in the original orientation, which the reverse walk sees as the arc's SOURCE: a move out of an odd (label)
//          position of the previously processed row t + 1 carries w(t + 1).  (Out of an odd position p - 1 into the blank p,
//          or out of the odd p - 2 into the odd p; the move p - 1 -> p into an odd p leaves a blank and carries nothing.)
//        * the windows may be NULL (no constraint).
//      ENT (lc_ctc_loss_entropy; the other instantiations carry none of it): the expectation semiring.  Beside each cell a the
//      sweep keeps m, the mean of log2 p(prefix) over the prefixes that end in the cell under their posterior:
//      m = emission + sum_i w_i m_i / sum_i w_i over the cell's predecessors, w_i = 2^(a_i - max) the terms its log-sum-exp
//      forms (lat_lse2_mean / lat_lse3_mean, ctc_lattice.h: the mean relative to the heaviest predecessor's m).  m is a plain
//      double, 0 in a dead cell by a select; its rows go to the workspace beside the cells'.  Direction 0 finishes with Ebar
//      (the end cells' means under the weights of log2 p, to the workspace) and H = (log2 p - Ebar) ln 2 >= 0, in double,
//      rounded once; a single path gives m == a bit for bit and H = +0.  The windows may be NULL.
//      STAR (lc_ctc_loss_star; never with DELAY or ENT, the other instantiations carry none of it): only a cell's emission
//      changes.  The star term of a frame is es = (lse_nb - lse) log2 e - log2(V - 1) - penalty log2 e, lse_nb the frame's
//      non-blank log-sum-exp (lat_lse_kernel<true>: one more float per frame in the prefetch arrays), the constant part formed
//      in double on the host and rounded once, one constant for the label positions (bypass) and one for the blank positions
//      (self-loop); the cell's emission is e' = max(e, es) + log2(1 + 2^-|e - es|) on the fp32 pipes (lat_star_mix), and
//      e' = e by a select when es = -inf (penalty +inf, or no non-blank mass on the frame).  Windows, dead cells, status words
//      and the end cells are the plain instantiation's.  The windows may be NULL.
//   4. lat_grad_kernel<ENTRY, ENT>  one wave per frame.  occupancy(t, s) = 2^(alpha + beta - emission - log2 p), the exponent formed
//      in double; lane k sums the positions of class k, k + 64, ... in the order of lat_index_kernel's list, the blank's
//      positions are summed lane by lane and then by the wave's DPP reduction.  grad = softmax - occupancy.  ENTRY also sums
//      occupancy(t, s) * notyet(s), notyet(s) = L - (s + 1) / 2, per frame in double (each lane its positions in sequence,
//      then a fixed butterfly) into the workspace; without a gradient lat_entry_kernel does the same from the two lattices
//      alone.  ENT subtracts eta * ln 2 * sum occupancy(t, s) * (Ebar - c(t, s)), c = m_alpha + m_beta - emission the mean log2
//      probability of the paths through the cell, from the plain gradient: the plain part is summed as without ENT, the
//      products beside it in double in the same orders.  STAR: the occupancies carry e' in the exponent; the own share
//      rho = 2^(e - e') scales a class's occupancy sum, the star share sigma = 2^(es - e') gives M(t) = sum_k sigma_k occ_k in
//      double (to the frame terms, folded into star_frames), and a second pass subtracts 2^((z_k - lse_nb) log2 e) M(t) from
//      the non-blank classes.  star_frames is required, so this kernel also runs without a gradient and then stores M(t) only.
//   5. lat_fold_kernel       (entry_sum and star_frames) one wave per utterance folds its frame terms in a fixed order in double and rounds
//      once.
// The band (only positions whose window contains t are live) is NOT exploited: every position is computed on every frame.
#include "common.h"
#include "ctc_lattice.h"
#include <float.h>
#include <limits.h>
#include <math.h>

#define LAT_LOG2E_D 1.4426950408889634
#define LAT_OK 0
#define LAT_ZERO 1                       // skipped utterance: loss 0, gradient rows zeros, entry_sum 0
#define LAT_NOPATH 2                     // loss +inf, gradient = softmax on the live frames, entry_sum 0
#define LAT_NAN 3                        // bad label: loss NaN, gradient rows zeros, entry_sum NaN

namespace {

// ------------------------------------------------------------------------------------------ 2. class -> positions lists
// order[b][r] = index of the label of rank r in (class, index) order; first[b][k] / cnt[b][k] = rank of class k's first
// label / number of its labels.  Labels outside [0, V) take part in the ranking but belong to no class (the sweep gives such
// an utterance a NaN loss and nothing reads its lists); every rank is below L, so nothing is written out of bounds.
__global__ __launch_bounds__(256) void lat_index_kernel(int V, const int *__restrict__ labels, const int *__restrict__ offs,
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
// DELAY = ENT = STAR = false: win_lo / win_hi are not NULL (the host checks).  lambda is read by DELAY alone; malpha / mbeta /
// ebar / entropy by ENT alone (nullptr otherwise); lse_nb / star_b / star_s by STAR alone.
// STAR (lc_ctc_loss_star; never with DELAY or ENT): star_b / star_s = log2(V - 1) + penalty * log2(e) of the bypass (label
// positions) and the self-loop (blank positions) star, +inf for a penalty of +inf.
template <int PPL, bool DELAY, bool ENT, bool STAR>
__global__ __launch_bounds__(64) void lat_sweep_kernel(const float *__restrict__ logits, int T, int B, int V,
                                                       const int *__restrict__ labels, const int *__restrict__ offs,
                                                       const int *__restrict__ seq_len, int maxL,
                                                       const int *__restrict__ win_lo, const int *__restrict__ win_hi,
                                                       float lambda, const float *__restrict__ lse,
                                                       double *__restrict__ alpha, double *__restrict__ beta, int srow,
                                                       int want_beta, float *__restrict__ loss,
                                                       double *__restrict__ lp2, int *__restrict__ status,
                                                       double *__restrict__ malpha, double *__restrict__ mbeta,
                                                       double *__restrict__ ebar, float *__restrict__ entropy,
                                                       const float *__restrict__ lse_nb, float star_b, float star_s)
{
    static_assert(!(STAR && (DELAY || ENT)), "the star is built under neither the delay tilt nor the entropy term");
    constexpr int K = PPL <= 4 ? 8 : 32 / PPL;            // frames fetched ahead as one chunk: 8, 8, 8, 4, 2, 1
    constexpr int NG = PPL == 1 ? 1 : PPL / 2;            // label positions (gathers, windows) per lane
    const int b = blockIdx.x >> 1, dir = blockIdx.x & 1, lane = threadIdx.x;
    if (dir == 1 && !want_beta) return;
    const int Tb = min(max(seq_len[b], 0), T);
    const int off = offs[b], L = offs[b + 1] - off, S = 2 * L + 1;
    const int blank = V - 1;
    const double NEG = lat_neg_inf();
    if (Tb == 0 || L > Tb) {                              // lc_ctc_loss: the utterance is skipped, loss 0, gradient 0
        if (lane == 0 && dir == 0) {
            loss[b] = 0.0f; lp2[b] = 0.0; status[b] = LAT_ZERO;
            if (ENT) { entropy[b] = 0.0f; ebar[b] = 0.0; }
        }
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
            if (lane == 0 && dir == 0) {
                loss[b] = __int_as_float(0x7fc00000); lp2[b] = 0.0; status[b] = LAT_NAN;
                if (ENT) { entropy[b] = __int_as_float(0x7fc00000); ebar[b] = 0.0; }
            }
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
                if (!(DELAY || ENT || STAR) || win_lo) {
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
    // ENT: mm[j] = the mean of log2 p(prefix) over the prefixes that end in the cell, under their posterior; 0 in a dead cell
    constexpr int PM = ENT ? PPL : 1;
    double mm[PM];
#pragma unroll
    for (int j = 0; j < PM; ++j) mm[j] = 0.0;
    const double wl = DELAY ? -(double)lambda * LAT_LOG2E_D : 0.0;       // w(t) = wl * t

    constexpr int KS = STAR ? K : 1;                      // STAR: the frame's non-blank log-sum-exp rides with lse
    float cg[K][NG], cb[K], cl[K], cs[KS], ng[K][NG], nb[K], nl[K], ns[KS];
    auto fetch = [&](int k0, float (&g)[K][NG], float (&gb)[K], float (&gl)[K], float (&gs)[KS]) {
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
            if constexpr (STAR) gs[k] = lse_nb[row];
        }
    };
    fetch(0, cg, cb, cl, cs);
    double *rows = (dir ? beta : alpha) + (size_t)b * T * srow;
    double *mrows = ENT ? (dir ? mbeta : malpha) + (size_t)b * T * srow : nullptr;
    for (int k0 = 0; k0 < Tb; k0 += K) {
        fetch(k0 + K, ng, nb, nl, ns);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int kk = k0 + k;
            if (kk < Tb) {
                const int t = dir ? Tb - 1 - kk : kk;
                const float lz = cl[k];
                float eb = (cb[k] - lz) * LAT_LOG2E;
                float esl = 0.0f;                                            // STAR: the star term of a label position
                if constexpr (STAR) {
                    const float nbl = (cs[k] - lz) * LAT_LOG2E;              // log2 of the frame's non-blank mass
                    esl = nbl - star_b;
                    eb = lat_star_mix(eb, nbl - star_s);
                }
                // DELAY, forward: the arcs into a label position of this row carry w(t).  Backward (reversed lattice): the arcs
                // out of a label position of the row before, frame t + 1, carry w(t + 1) - that is p-1 -> p for an even p and
                // p-2 -> p for an odd p.  An arc p-2 -> p joins two label positions in either direction.
                const double w = DELAY ? wl * (double)(dir ? t + 1 : t) : 0.0;
                const double w1odd = dir ? 0.0 : w, w1even = dir ? w : 0.0;
                const double in1 = lat_shr1(a[PPL - 1]);
                const double in2 = PPL == 1 ? lat_shr1(in1) : in1;           // s-2 of the lane's first label position
                const double mi1 = ENT ? lat_shr1_zero(mm[PM - 1]) : 0.0;    // ENT: the neighbours' means, 0 into lane 0
                const double mi2 = ENT && PPL == 1 ? lat_shr1_zero(mi1) : mi1;
#pragma unroll
                for (int j = PPL - 1; j >= 0; --j) {                         // descending: a[j-1], a[j-2] are the old frame's
                    const double p1 = j >= 1 ? a[j - 1] : in1;
                    const int g_ = PPL == 1 ? 0 : j >> 1;
                    double v, mean = 0.0;
                    float e = eb;
                    bool live = (valid >> j & 1u) != 0;
                    if constexpr (ENT) {                                     // the same cells, and the means beside them
                        const double q1 = j >= 1 ? mm[j - 1] : mi1;
                        if (PPL == 1) {
                            const bool two = (allow2 & 1u) != 0;
                            v = lat_lse3_mean(a[0], p1, two ? in2 : NEG, mm[0], q1, two ? mi2 : 0.0, mean);
                            if (lane & 1) e = (cg[k][0] - lz) * LAT_LOG2E;
                            live = live && t >= wlo[0] && t <= whi[0];
                        } else if (j & 1) {
                            const bool two = (allow2 >> j & 1u) != 0;
                            const double p2 = j >= 2 ? a[j - 2] : in2, q2 = j >= 2 ? mm[j - 2] : mi2;
                            v = lat_lse3_mean(a[j], p1, two ? p2 : NEG, mm[j], q1, two ? q2 : 0.0, mean);
                            e = (cg[k][g_] - lz) * LAT_LOG2E;
                            live = live && t >= wlo[g_] && t <= whi[g_];
                        } else {
                            v = lat_lse2_mean(a[j], p1, mm[j], q1, mean);
                        }
                    } else if (PPL == 1) {
                        const double p2 = (allow2 & 1u) ? (DELAY ? in2 + w : in2) : NEG;
                        v = lat_lse3(a[0], DELAY ? p1 + ((lane & 1) ? w1odd : w1even) : p1, p2);
                        if (lane & 1) e = (cg[k][0] - lz) * LAT_LOG2E;
                        if constexpr (STAR)
                            if (lane & 1) e = lat_star_mix(e, esl);
                        live = live && t >= wlo[0] && t <= whi[0];           // blank lanes: lo = 0, hi = INT_MAX
                    } else if (j & 1) {
                        double p2 = j >= 2 ? a[j - 2] : in2;
                        p2 = (allow2 >> j & 1u) ? (DELAY ? p2 + w : p2) : NEG;
                        v = lat_lse3(a[j], DELAY ? p1 + w1odd : p1, p2);
                        e = (cg[k][g_] - lz) * LAT_LOG2E;
                        if constexpr (STAR) e = lat_star_mix(e, esl);
                        live = live && t >= wlo[g_] && t <= whi[g_];
                    } else {
                        v = lat_lse2(a[j], DELAY ? p1 + w1even : p1);        // blanks are never entered from s-2
                    }
                    a[j] = live ? v + (double)e : NEG;
                    if constexpr (ENT) mm[j] = a[j] > NEG ? mean + (double)e : 0.0;      // dead: 0 by a select, also for a NaN mean
                }
                // the row
                double *dst = rows + (size_t)t * srow;
                if constexpr (PPL == 1) {
                    dst[lane] = a[0];                                        // srow >= 64
                    if constexpr (ENT) mrows[(size_t)t * srow + lane] = mm[0];
                } else {
#pragma unroll
                    for (int c = 0; c < PPL / 2; ++c) {
                        const int p0 = lane * PPL + 2 * c;                   // srow is a multiple of 64: both or none
                        if (p0 < srow) *(double2 *)(dst + p0) = make_double2(a[2 * c], a[2 * c + 1]);
                        if constexpr (ENT)
                            if (p0 < srow) *(double2 *)(mrows + (size_t)t * srow + p0) = make_double2(mm[2 * c], mm[2 * c + 1]);
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
            if constexpr (STAR) cs[k] = ns[k];
        }
    }
    if (dir == 1) return;
    // log2 of the (weighted) path sum: the path ends in S-1 or S-2
    const int s1 = S - 1, s2 = S - 2;
    double m1 = NEG, m2 = NEG;
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
        if (j == (s1 & (PPL - 1))) m1 = a[j];
        if (s2 >= 0 && j == (s2 & (PPL - 1))) m2 = a[j];
    }
    const double v1 = lat_readlane(m1, s1 / PPL);
    const double v2 = s2 >= 0 ? lat_readlane(m2, s2 / PPL) : NEG;
    double u1 = 0.0, u2 = 0.0;                                               // ENT: the two end cells' means
    if constexpr (ENT) {
        double n1 = 0.0, n2 = 0.0;
#pragma unroll
        for (int j = 0; j < PPL; ++j) {
            if (j == (s1 & (PPL - 1))) n1 = mm[j];
            if (s2 >= 0 && j == (s2 & (PPL - 1))) n2 = mm[j];
        }
        u1 = lat_readlane(n1, s1 / PPL);
        u2 = s2 >= 0 ? lat_readlane(n2, s2 / PPL) : 0.0;
    }
    if (lane == 0) {
        const double hi = fmax(v1, v2), lo = fmin(v1, v2);
        if (!(hi > NEG)) {                                                   // no surviving path
            loss[b] = INFINITY; lp2[b] = 0.0; status[b] = LAT_NOPATH;
            if constexpr (ENT) { entropy[b] = 0.0f; ebar[b] = 0.0; }
        } else {
            const float wlo = __builtin_amdgcn_exp2f((float)(lo - hi));
            const double lp = hi + (double)__builtin_amdgcn_logf(1.0f + wlo);
            loss[b] = (float)(0.0 - lp * LAT_LN2);
            lp2[b] = lp; status[b] = LAT_OK;
            if constexpr (ENT) {
                // Ebar = the mean of log2 p(path) under the path posterior: the end cells' means under the weights of lp, again
                // relative to the heavier cell; H = (log2 Z - Ebar) ln 2 >= 0, formed in double and rounded once.  One path:
                // its cells and its means are the same sums of the same emissions, and H is +0 exactly.
                const double uhi = v1 >= v2 ? u1 : u2, ulo = v1 >= v2 ? u2 : u1;
                const double eb2 = uhi + (double)wlo * (ulo - uhi) / (1.0 + (double)wlo);
                const double h = (lp - eb2) * LAT_LN2;
                ebar[b] = eb2;
                entropy[b] = h > 0.0 ? (float)h : 0.0f;
            }
        }
    }
}

// the wave's sum of a double in a fixed order (xor butterfly), the same value in every lane
__device__ __forceinline__ double lat_wave_sum_d(double x)
{
#pragma unroll
    for (int mask = 1; mask < 64; mask <<= 1) {
        const int lo = __shfl_xor(__double2loint(x), mask, 64), hi = __shfl_xor(__double2hiint(x), mask, 64);
        x += __hiloint2double(hi, lo);
    }
    return x;
}

// ------------------------------------------------------------------------------------------ 4. gradient (+ entry terms)
// ENT (maximum-entropy CTC; never with ENTRY): the gradient of loss - eta H is the plain one minus eta times
// sum_s occupancy(t, s) * (Ebar - c(t, s)), c = malpha + mbeta - emission the mean log-probability of the paths through the
// cell.  The plain part is summed exactly as without ENT (eta = 0 gives its bits); the products occupancy * (Ebar - c), each
// formed as that product, are summed beside it in double in the same orders and the term is rounded once.
// STAR (transcript-tolerant CTC; never with ENTRY or ENT): a cell's emission is the mixture e' = log2(2^e + 2^es), es the
// star term of its parity.  The occupancies carry e' in the exponent; rho = 2^(e - e') and sigma = 2^(es - e') are the own
// and the star share of the cell, each formed as that power (a dead side is 0 by a select, a cell with e' = -inf is never
// visited).  grad = softmax - rho_k occ_k - [k < V-1] 2^((z_k - lse_nb) log2 e) M(t), M(t) = sum_k sigma_k occ_k in double
// (each lane its classes in sequence, then the fixed butterfly), the last term in a second pass over the lane's own stores
// and only where M(t) != 0.  M(t) goes to fterm; grad may be NULL, then nothing is stored and M(t) is the same sum.
template <bool ENTRY, bool ENT, bool STAR>
__global__ __launch_bounds__(256) void lat_grad_kernel(const float *__restrict__ logits, int T, int B, int V,
                                                       const int *__restrict__ offs, const int *__restrict__ seq_len,
                                                       const float *__restrict__ lse, const double *__restrict__ alpha,
                                                       const double *__restrict__ beta, int srow,
                                                       const double *__restrict__ lp2, const int *__restrict__ status,
                                                       const int *__restrict__ order, int pitch,
                                                       const int *__restrict__ first, const int *__restrict__ cnt,
                                                       float *__restrict__ grad, double *__restrict__ fterm,
                                                       const double *__restrict__ malpha, const double *__restrict__ mbeta,
                                                       const double *__restrict__ ebar, float eta,
                                                       const float *__restrict__ lse_nb, float star_b, float star_s)
{
    static_assert(!(STAR && (ENTRY || ENT)), "the star is built under neither the delay tilt nor the entropy term");
    const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= (size_t)T * B) return;
    const int t = (int)(row / B), b = (int)(row % B);
    const int Tb = min(max(seq_len[b], 0), T);
    const int st = status[b];
    const float *x = logits + row * V;
    const bool store = !STAR || grad != nullptr;                             // wave-uniform; only STAR runs without a gradient
    float *g = store ? grad + row * V : nullptr;
    if (t >= Tb || st == LAT_ZERO || st == LAT_NAN) {                        // wave-uniform
        if (store)
            for (int k = lane; k < V; k += 64) g[k] = 0.0f;
        return;
    }
    const float lz = lse[row];
    if (st == LAT_NOPATH) {
        if (store)
            for (int k = lane; k < V; k += 64) g[k] = __builtin_amdgcn_exp2f((x[k] - lz) * LAT_LOG2E);
        return;
    }
    const int L = offs[b + 1] - offs[b], S = 2 * L + 1;
    const size_t bt = (size_t)b * T + t;
    const double *A = alpha + bt * srow, *Bt = beta + bt * srow;
    const double lp = lp2[b];
    const int blank = V - 1;
    double eacc = 0.0;                                                       // this lane's sum of occupancy * notyet
    const double *MA = ENT ? malpha + bt * srow : nullptr, *MB = ENT ? mbeta + bt * srow : nullptr;
    const double eb2 = ENT ? ebar[b] : 0.0, etal = ENT ? (double)eta * LAT_LN2 : 0.0;      // the means are in log2
    const float lnb = STAR ? lse_nb[row] : 0.0f;
    const float nbl = (lnb - lz) * LAT_LOG2E, esl = nbl - star_b, ess = nbl - star_s;      // STAR: the two star terms
    double macc = 0.0;                                                       // STAR: this lane's sum of sigma_k * occ_k
    // the blank: positions 0, 2, .., 2L, lane l takes 2l, 2l + 128, ... in sequence, then the wave's fixed reduction
    const float eb = (x[blank] - lz) * LAT_LOG2E;
    {
        const float em = STAR ? lat_star_mix(eb, ess) : eb;
        const double c = (double)em + lp;
        float acc = 0.0f;
        double dacc = 0.0;                                                   // ENT: sum of occupancy * (Ebar - c)
        for (int s = 2 * lane; s < (STAR && !(em > -INFINITY) ? 0 : S); s += 128) {
            const float o = __builtin_amdgcn_exp2f((float)((A[s] + Bt[S - 1 - s]) - c));
            acc += o;
            if (ENTRY) eacc += (double)o * (double)(L - (s >> 1));
            if (ENT) dacc += (double)o * (eb2 - ((MA[s] + MB[S - 1 - s]) - (double)eb));
        }
        acc = lc_wave_sum(acc);
        if (ENT) dacc = lat_wave_sum_d(dacc);
        if constexpr (STAR) {
            if (lane == 0) {
                const float rho = eb > -INFINITY ? __builtin_amdgcn_exp2f(eb - em) : 0.0f;
                const float sigma = ess > -INFINITY ? __builtin_amdgcn_exp2f(ess - em) : 0.0f;
                macc = (double)sigma * (double)acc;
                if (store) g[blank] = __builtin_amdgcn_exp2f(eb) - rho * acc;
            }
        } else if (lane == 0) {
            const float plain = __builtin_amdgcn_exp2f(eb) - acc;
            g[blank] = ENT ? plain - (float)(etal * dacc) : plain;
        }
    }
    // the labels: lane k sums the positions of class k in the order of the utterance's list
    const int *ord = order + (size_t)b * pitch;
    const int *fr = first + (size_t)b * V, *cn = cnt + (size_t)b * V;
    for (int k = lane; k < blank; k += 64) {
        const float e = (x[k] - lz) * LAT_LOG2E;
        const float em = STAR ? lat_star_mix(e, esl) : e;
        const double c = (double)em + lp;
        const int r0 = fr[k], n = STAR && !(em > -INFINITY) ? 0 : cn[k];
        float acc = 0.0f;
        double dacc = 0.0;
        for (int r = 0; r < n; ++r) {
            const int i = ord[r0 + r], s = 2 * i + 1;
            const float o = __builtin_amdgcn_exp2f((float)((A[s] + Bt[S - 1 - s]) - c));
            acc += o;
            if (ENTRY) eacc += (double)o * (double)(L - 1 - i);
            if (ENT) dacc += (double)o * (eb2 - ((MA[s] + MB[S - 1 - s]) - (double)e));
        }
        if constexpr (STAR) {
            const float rho = e > -INFINITY ? __builtin_amdgcn_exp2f(e - em) : 0.0f;
            const float sigma = esl > -INFINITY ? __builtin_amdgcn_exp2f(esl - em) : 0.0f;
            macc += (double)sigma * (double)acc;
            if (store) g[k] = __builtin_amdgcn_exp2f(e) - rho * acc;
        } else {
            const float plain = __builtin_amdgcn_exp2f(e) - acc;
            g[k] = ENT ? plain - (float)(etal * dacc) : plain;
        }
    }
    if constexpr (STAR) {
        const double mt = lat_wave_sum_d(macc);                              // M(t), the same value in every lane
        if (lane == 0) fterm[bt] = mt;
        if (store && mt != 0.0)                                              // mt != 0 needs a live star term, so lnb > -inf
            for (int k = lane; k < blank; k += 64)
                g[k] -= (float)((double)__builtin_amdgcn_exp2f((x[k] - lnb) * LAT_LOG2E) * mt);
    }
    if (ENTRY) {
        eacc = lat_wave_sum_d(eacc);
        if (lane == 0) fterm[bt] = eacc;
    }
}

// ------------------------------------------------------------------------------------------ 4'. entry terms alone
// One wave per live frame of an utterance with a path: sum_s occupancy(t, s) * notyet(s), lane l takes s = l, l + 64, ...
__global__ __launch_bounds__(256) void lat_entry_kernel(const float *__restrict__ logits, int T, int B, int V,
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
    if (t >= Tb || status[b] != LAT_OK) return;                              // wave-uniform; the fold never reads these
    const float *x = logits + row * V;
    const float lz = lse[row];
    const int off = offs[b], L = offs[b + 1] - off, S = 2 * L + 1;
    const size_t bt = (size_t)b * T + t;
    const double *A = alpha + bt * srow, *Bt = beta + bt * srow;
    const double lp = lp2[b];
    double eacc = 0.0;
    for (int s = lane; s < S; s += 64) {
        const int sym = (s & 1) ? labels[off + (s >> 1)] : V - 1;            // status OK: every label lies in [0, V-1)
        const float e = (x[sym] - lz) * LAT_LOG2E;
        const float o = __builtin_amdgcn_exp2f((float)((A[s] + Bt[S - 1 - s]) - ((double)e + lp)));
        eacc += (double)o * (double)(L - ((s + 1) >> 1));
    }
    eacc = lat_wave_sum_d(eacc);
    if (lane == 0) fterm[bt] = eacc;
}

// ------------------------------------------------------------------------------------------ 5. per-utterance fold
// One wave per utterance: lane l sums the terms of frames l, l + 64, ... in sequence, then the fixed butterfly; rounded once.
__global__ __launch_bounds__(64) void lat_fold_kernel(const double *__restrict__ fterm, int T, const int *__restrict__ seq_len,
                                                      const int *__restrict__ status, float *__restrict__ entry_sum)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    const int st = status[b];
    if (st != LAT_OK) {
        if (lane == 0) entry_sum[b] = st == LAT_NAN ? __int_as_float(0x7fc00000) : 0.0f;
        return;
    }
    const int Tb = min(max(seq_len[b], 0), T);
    const double *f = fterm + (size_t)b * T;
    double acc = 0.0;
    for (int t = lane; t < Tb; t += 64) acc += f[t];
    acc = lat_wave_sum_d(acc);
    if (lane == 0) entry_sum[b] = (float)acc;
}

// ------------------------------------------------------------------------------------------ host
// the workspace: slabs in this order; only the delay and the star entry have the frame terms, only the entropy entry Ebar and
// the means, only the star entry (last, so that it is the delay entry's layout plus one slab) the non-blank log-sum-exp
struct LatLayout {
    size_t lse, status, lp2, ebar, order, first, cnt, fterm, alpha, beta, malpha, mbeta, lse_nb, total;
    int ppl, srow, pitch;
};
inline LatLayout lat_layout(int T, int B, int V, int max_label_len, bool with_fterm, bool with_means, bool with_nb)
{
    LatLayout m;
    const int S = 2 * max_label_len + 1;
    m.ppl = lat_ppl(S);
    m.srow = (S + 63) / 64 * 64;                         // <= 64 * ppl
    m.pitch = max_label_len > 0 ? max_label_len : 1;
    const size_t TB = (size_t)T * B;
    size_t o = 0;
    m.lse = o; o += lc_align256(TB * sizeof(float));
    m.status = o; o += lc_align256((size_t)B * sizeof(int));
    m.lp2 = o; o += lc_align256((size_t)B * sizeof(double));
    m.ebar = o; o += with_means ? lc_align256((size_t)B * sizeof(double)) : 0;
    m.order = o; o += lc_align256((size_t)B * m.pitch * sizeof(int));
    m.first = o; o += lc_align256((size_t)B * V * sizeof(int));
    m.cnt = o; o += lc_align256((size_t)B * V * sizeof(int));
    m.fterm = o; o += with_fterm ? lc_align256(TB * sizeof(double)) : 0;
    m.alpha = o; o += lc_align256(TB * m.srow * sizeof(double));
    m.beta = o; o += lc_align256(TB * m.srow * sizeof(double));
    m.malpha = o; o += with_means ? lc_align256(TB * m.srow * sizeof(double)) : 0;
    m.mbeta = o; o += with_means ? lc_align256(TB * m.srow * sizeof(double)) : 0;
    m.lse_nb = o; o += with_nb ? lc_align256(TB * sizeof(float)) : 0;
    m.total = o;
    return m;
}
inline size_t lat_workspace_bytes(int T, int B, int V, int max_label_len, bool with_fterm, bool with_means, bool with_nb)
{
    if (T <= 0 || B <= 0 || V < 2 || max_label_len < 0 || max_label_len > 1023) return 0;
    return lat_layout(T, B, V, max_label_len, with_fterm, with_means, with_nb).total;
}

// what tells the four entries apart on the host: the criterion, the names in front of an error, the tags of the launches
struct LatEntry {
    bool delay, entropy, star;
    const char *name, *weight, *lse, *index, *sweep, *grad, *entry, *fold;
};
const LatEntry LAT_WINDOW = {false, false, false, "lc_ctc_loss_windowed", "delay_penalty", "ctc_window_lse", "ctc_window_index",
                             "ctc_window_sweep", "ctc_window_grad", "ctc_window_entry", "ctc_window_fold"};
const LatEntry LAT_DELAY = {true, false, false, "lc_ctc_loss_delay", "delay_penalty", "ctc_delay_lse", "ctc_delay_index",
                            "ctc_delay_sweep", "ctc_delay_grad", "ctc_delay_entry", "ctc_delay_fold"};
const LatEntry LAT_ENTROPY = {false, true, false, "lc_ctc_loss_entropy", "entropy_weight", "ctc_entropy_lse", "ctc_entropy_index",
                              "ctc_entropy_sweep", "ctc_entropy_grad", "ctc_entropy_entry", "ctc_entropy_fold"};
const LatEntry LAT_STAR = {false, false, true, "lc_ctc_loss_star", "bypass_penalty", "ctc_star_lse", "ctc_star_index",
                           "ctc_star_sweep", "ctc_star_grad", "ctc_star_entry", "ctc_star_fold"};

// ``weight`` is the delay penalty, the entropy weight or the bypass penalty, ``weight2`` the star entry's self-loop penalty (0
// otherwise), ``extra`` entry_sum [B] (delay; optional), entropy [B] (entropy; required) or star_frames [B] (star; required:
// it is folded from the frame terms as entry_sum is).  The windowed entry comes with windows, weight 0 and no extra.
int lat_launch(const LatEntry &e, const float *logits, int T, int B, int V, const int *labels, const int *label_offsets,
               const int *seq_len, int max_label_len, const int *win_lo, const int *win_hi, float weight, float weight2,
               float *loss, float *extra, float *grad, void *workspace, size_t workspace_bytes, lc_stream_t stream)
{
    float *entry_sum = e.entropy ? nullptr : extra, *entropy = e.entropy ? extra : nullptr;
    LC_CHECK_ARG(logits && labels && label_offsets && seq_len && loss && workspace && (!(e.entropy || e.star) || extra) &&
                     (e.delay || e.entropy || e.star || (win_lo && win_hi)),
                 "%s: null pointer", e.name);
    LC_CHECK_ARG((win_lo == nullptr) == (win_hi == nullptr), "%s: win_lo and win_hi go together (both or none)", e.name);
    LC_CHECK_ARG(T > 0 && B > 0 && V >= 2 && max_label_len >= 0, "%s: bad shape T=%d B=%d V=%d L=%d", e.name, T, B, V,
                 max_label_len);
    LC_CHECK_ARG(max_label_len <= 1023, "%s: label length %d exceeds the supported maximum 1023", e.name, max_label_len);
    if (e.star) {                                        // +inf is legal: it switches that arc family off
        LC_CHECK_ARG(weight >= 0.0f, "%s: bypass_penalty must be >= 0 or +inf, got %g", e.name, (double)weight);
        LC_CHECK_ARG(weight2 >= 0.0f, "%s: selfloop_penalty must be >= 0 or +inf, got %g", e.name, (double)weight2);
    } else {
        LC_CHECK_ARG(isfinite(weight), "%s: %s must be finite, got %g", e.name, e.weight, (double)weight);
    }
    LC_CHECK_ARG((long long)B * 2 <= 0x7fffffffLL && ((long long)T * B + 3) / 4 <= 0x7fffffffLL,
                 "%s: T * B = %lld is beyond the launch grid", e.name, (long long)T * B);
    const LatLayout m = lat_layout(T, B, V, max_label_len, e.delay || e.star, e.entropy, e.star);
    if (workspace_bytes < m.total) {
        lc_set_error("%s: workspace too small (%zu < %zu)", e.name, workspace_bytes, m.total);
        return LC_EWORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    char *w = (char *)workspace;
    float *lse = (float *)(w + m.lse);
    int *status = (int *)(w + m.status);
    double *lp2 = (double *)(w + m.lp2);
    int *order = (int *)(w + m.order), *first = (int *)(w + m.first), *cnt = (int *)(w + m.cnt);
    double *fterm = (double *)(w + m.fterm);             // only with entry_sum, which only the delay entry has
    double *alpha = (double *)(w + m.alpha), *beta = (double *)(w + m.beta);
    double *ebar = (double *)(w + m.ebar), *malpha = (double *)(w + m.malpha), *mbeta = (double *)(w + m.mbeta);   // entropy only
    float *lse_nb = (float *)(w + m.lse_nb);              // star only
    // star: log2(V - 1) + penalty * log2(e), formed in double and rounded once; +inf with the penalty
    const float star_b = e.star ? (float)(log2((double)(V - 1)) + (double)weight * LAT_LOG2E_D) : 0.0f;
    const float star_s = e.star ? (float)(log2((double)(V - 1)) + (double)weight2 * LAT_LOG2E_D) : 0.0f;
    const unsigned frame_blocks = (unsigned)(((long long)T * B + 3) / 4);
    if (e.star)
        hipLaunchKernelGGL(lat_lse_kernel<true>, dim3(frame_blocks), dim3(256), 0, s, logits, T, B, V, seq_len, lse, lse_nb);
    else
        hipLaunchKernelGGL(lat_lse_kernel<false>, dim3(frame_blocks), dim3(256), 0, s, logits, T, B, V, seq_len, lse,
                           (float *)nullptr);
    LC_CHECK_LAUNCH(e.lse);
    if (grad || e.star) {                                // the star's frame terms are summed in the gradient's order
        hipLaunchKernelGGL(lat_index_kernel, dim3(B), dim3(256), 0, s, V, labels, label_offsets, max_label_len, m.pitch, order,
                           first, cnt);
        LC_CHECK_LAUNCH(e.index);
    }
#define LC_LAT(PPL, DELAY, ENT, STAR)                                                                                   \
    hipLaunchKernelGGL((lat_sweep_kernel<PPL, DELAY, ENT, STAR>), dim3(2 * B), dim3(64), 0, s, logits, T, B, V, labels, \
                       label_offsets, seq_len, max_label_len, win_lo, win_hi, weight, lse, alpha, beta, m.srow,         \
                       (grad || entry_sum) ? 1 : 0, loss, lp2, status, malpha, mbeta, ebar, entropy, lse_nb, star_b,    \
                       star_s)
    // the sign picks the DELAY instantiations, + 64 ENT, + 128 STAR
    switch (e.delay ? -m.ppl : e.entropy ? 64 + m.ppl : e.star ? 128 + m.ppl : m.ppl) {
    case 1: LC_LAT(1, false, false, false); break;
    case 2: LC_LAT(2, false, false, false); break;
    case 4: LC_LAT(4, false, false, false); break;
    case 8: LC_LAT(8, false, false, false); break;
    case 16: LC_LAT(16, false, false, false); break;
    case 32: LC_LAT(32, false, false, false); break;
    case 65: LC_LAT(1, false, true, false); break;
    case 66: LC_LAT(2, false, true, false); break;
    case 68: LC_LAT(4, false, true, false); break;
    case 72: LC_LAT(8, false, true, false); break;
    case 80: LC_LAT(16, false, true, false); break;
    case 96: LC_LAT(32, false, true, false); break;
    case 129: LC_LAT(1, false, false, true); break;
    case 130: LC_LAT(2, false, false, true); break;
    case 132: LC_LAT(4, false, false, true); break;
    case 136: LC_LAT(8, false, false, true); break;
    case 144: LC_LAT(16, false, false, true); break;
    case 160: LC_LAT(32, false, false, true); break;
    case -1: LC_LAT(1, true, false, false); break;
    case -2: LC_LAT(2, true, false, false); break;
    case -4: LC_LAT(4, true, false, false); break;
    case -8: LC_LAT(8, true, false, false); break;
    case -16: LC_LAT(16, true, false, false); break;
    default: LC_LAT(32, true, false, false); break;
    }
#undef LC_LAT
    LC_CHECK_LAUNCH(e.sweep);
#define LC_LAT_GRAD(ENTRY, ENT, STAR)                                                                                   \
    hipLaunchKernelGGL((lat_grad_kernel<ENTRY, ENT, STAR>), dim3(frame_blocks), dim3(256), 0, s, logits, T, B, V,       \
                       label_offsets, seq_len, lse, alpha, beta, m.srow, lp2, status, order, m.pitch, first, cnt, grad, \
                       fterm, malpha, mbeta, ebar, weight, lse_nb, star_b, star_s)
    if (e.star) {                                        // also without a gradient: the same pass, storing only M(t)
        LC_LAT_GRAD(false, false, true);
        LC_CHECK_LAUNCH(e.grad);
    } else if (grad && entropy) {
        LC_LAT_GRAD(false, true, false);
        LC_CHECK_LAUNCH(e.grad);
    } else if (grad && entry_sum) {
        LC_LAT_GRAD(true, false, false);
        LC_CHECK_LAUNCH(e.grad);
    } else if (grad) {
        LC_LAT_GRAD(false, false, false);
        LC_CHECK_LAUNCH(e.grad);
    } else if (entry_sum) {
        hipLaunchKernelGGL(lat_entry_kernel, dim3(frame_blocks), dim3(256), 0, s, logits, T, B, V, labels, label_offsets,
                           seq_len, lse, alpha, beta, m.srow, lp2, status, fterm);
        LC_CHECK_LAUNCH(e.entry);
    }
#undef LC_LAT_GRAD
    if (entry_sum) {
        hipLaunchKernelGGL(lat_fold_kernel, dim3(B), dim3(64), 0, s, fterm, T, seq_len, status, entry_sum);
        LC_CHECK_LAUNCH(e.fold);
    }
    return LC_OK;
}

}  // namespace

extern "C" size_t lc_ctc_window_workspace_bytes(int T, int B, int V, int max_label_len)
{
    return lat_workspace_bytes(T, B, V, max_label_len, false, false, false);
}

extern "C" size_t lc_ctc_delay_workspace_bytes(int T, int B, int V, int max_label_len)
{
    return lat_workspace_bytes(T, B, V, max_label_len, true, false, false);
}

extern "C" size_t lc_ctc_entropy_workspace_bytes(int T, int B, int V, int max_label_len)
{
    return lat_workspace_bytes(T, B, V, max_label_len, false, true, false);
}

extern "C" size_t lc_ctc_star_workspace_bytes(int T, int B, int V, int max_label_len)
{
    return lat_workspace_bytes(T, B, V, max_label_len, true, false, true);
}

extern "C" int lc_ctc_loss_star(const float *logits, int T, int B, int V, const int *labels, const int *label_offsets,
                                const int *seq_len, int max_label_len, const int *win_lo, const int *win_hi,
                                float bypass_penalty, float selfloop_penalty, float *loss, float *star_frames, float *grad,
                                void *workspace, size_t workspace_bytes, lc_stream_t stream)
{
    return lat_launch(LAT_STAR, logits, T, B, V, labels, label_offsets, seq_len, max_label_len, win_lo, win_hi,
                      bypass_penalty, selfloop_penalty, loss, star_frames, grad, workspace, workspace_bytes, stream);
}

extern "C" int lc_ctc_loss_entropy(const float *logits, int T, int B, int V, const int *labels, const int *label_offsets,
                                   const int *seq_len, int max_label_len, const int *win_lo, const int *win_hi,
                                   float entropy_weight, float *loss, float *entropy, float *grad, void *workspace,
                                   size_t workspace_bytes, lc_stream_t stream)
{
    return lat_launch(LAT_ENTROPY, logits, T, B, V, labels, label_offsets, seq_len, max_label_len, win_lo, win_hi,
                      entropy_weight, 0.0f, loss, entropy, grad, workspace, workspace_bytes, stream);
}

extern "C" int lc_ctc_loss_windowed(const float *logits, int T, int B, int V, const int *labels, const int *label_offsets,
                                    const int *seq_len, int max_label_len, const int *win_lo, const int *win_hi,
                                    float *loss, float *grad, void *workspace, size_t workspace_bytes, lc_stream_t stream)
{
    return lat_launch(LAT_WINDOW, logits, T, B, V, labels, label_offsets, seq_len, max_label_len, win_lo, win_hi, 0.0f, 0.0f, loss,
                      nullptr, grad, workspace, workspace_bytes, stream);
}

extern "C" int lc_ctc_loss_delay(const float *logits, int T, int B, int V, const int *labels, const int *label_offsets,
                                 const int *seq_len, int max_label_len, const int *win_lo, const int *win_hi,
                                 float delay_penalty, float *loss, float *entry_sum, float *grad, void *workspace,
                                 size_t workspace_bytes, lc_stream_t stream)
{
    return lat_launch(LAT_DELAY, logits, T, B, V, labels, label_offsets, seq_len, max_label_len, win_lo, win_hi, delay_penalty,
                      0.0f, loss, entry_sum, grad, workspace, workspace_bytes, stream);
}
