// ctc_lattice.h — what the double-cell log2-domain CTC lattices share (ctc_lattice.hip: windowed, delay-penalised,
// maximum-entropy and transcript-tolerant CTC, ctc_align.hip: forced alignment; DESIGN.md sections 3.6, 3.8, 3.14, 3.15): the
// per-frame log-sum-exp kernel (with the non-blank log-sum-exp beside it for the star), -inf as "log zero", the
// log-sum-exp of a cell's predecessors on the fp32 exp2 / log2 pipes relative to their maximum, the DPP neighbour shift.
#pragma once
#include "common.h"
#include <float.h>
#include <math.h>

#define LAT_LOG2E 1.4426950408889634f
#define LAT_LN2 0.6931471805599453

namespace {

// one wave per live frame (t, b): lse[t, b] = log sum_k exp(logits[t, b, k]), fp32.  Grid: ceil(T * B / 4) blocks of 256.
// NB (transcript-tolerant CTC) also writes lse_nb[t, b] = log sum_{k < V-1} exp(logits[t, b, k]) from the same two passes over the
// row: a second log-sum-exp around the non-blank maximum, not log(1 - q_blank), which cancels when the blank dominates.  A row
// whose non-blank logits are all -inf gives -inf (the maximum is clamped to -FLT_MAX, so no -inf - -inf arises).  lse is
// formed by the same operations in the same order with and without NB.
template <bool NB>
__global__ __launch_bounds__(256) void lat_lse_kernel(const float *__restrict__ logits, int T, int B, int V,
                                                      const int *__restrict__ seq_len, float *__restrict__ lse,
                                                      float *__restrict__ lse_nb)
{
    const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= (size_t)T * B) return;
    const int t = (int)(row / B), b = (int)(row % B);
    if (t >= seq_len[b]) return;                                  // never read
    const float *x = logits + row * V;
    float m = -INFINITY, mn = -FLT_MAX;
    for (int k = lane; k < V; k += 64) {
        m = fmaxf(m, x[k]);
        if (NB && k < V - 1) mn = fmaxf(mn, x[k]);
    }
    m = lc_wave_max(m);
    if (NB) mn = lc_wave_max(mn);
    float s = 0.0f, sn = 0.0f;
    for (int k = lane; k < V; k += 64) {
        s += __builtin_amdgcn_exp2f((x[k] - m) * LAT_LOG2E);
        if (NB && k < V - 1) sn += __builtin_amdgcn_exp2f((x[k] - mn) * LAT_LOG2E);
    }
    s = lc_wave_sum(s);
    if (NB) sn = lc_wave_sum(sn);
    if (lane == 0) {
        lse[row] = m + __builtin_amdgcn_logf(s) * (float)LAT_LN2;
        if (NB) lse_nb[row] = mn + __builtin_amdgcn_logf(sn) * (float)LAT_LN2;
    }
}

__device__ __forceinline__ double lat_neg_inf() { return __longlong_as_double(0xfff0000000000000ull); }
// log2(2^a + 2^b [+ 2^c]); -inf operands are "log zero", all of them -inf gives -inf (see ctc_lattice.hip's header)
__device__ __forceinline__ double lat_lse2(double a, double b)
{
    const double m = fmax(fmax(a, b), -DBL_MAX);
    return m + (double)__builtin_amdgcn_logf(__builtin_amdgcn_exp2f((float)(a - m)) + __builtin_amdgcn_exp2f((float)(b - m)));
}
__device__ __forceinline__ double lat_lse3(double a, double b, double c)
{
    const double m = fmax(fmax(fmax(a, b), c), -DBL_MAX);
    return m + (double)__builtin_amdgcn_logf(__builtin_amdgcn_exp2f((float)(a - m)) + __builtin_amdgcn_exp2f((float)(b - m)) +
                                             __builtin_amdgcn_exp2f((float)(c - m)));
}
// lane i receives x of lane i-1, lane 0 receives -inf (two 32-bit DPP wave_shr:1 moves)
__device__ __forceinline__ double lat_shr1(double x)
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), 0x138, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp((int)0xfff00000, __double2hiint(x), 0x138, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
// the same shift for a quantity that is no logarithm: lane 0 receives 0
__device__ __forceinline__ double lat_shr1_zero(double x)
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), 0x138, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), 0x138, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
// lat_lse2 / lat_lse3, bit for bit, and in ``mean`` the mean of ma, mb [, mc] under the same weights 2^(a_i - max) / sum:
// the expectation semiring's second component (maximum-entropy CTC).  The mean is formed relative to the m of the maximal
// operand, whose weight is exactly 1: its error is a few fp32 ulps of the SPREAD of the m_i, not of their magnitude, and a
// cell with one live predecessor copies that predecessor's m exactly.  A "log zero" operand has weight 0 and must come with
// a finite m (0 by convention); all operands dead gives a NaN mean, which the caller discards with the dead cell.
__device__ __forceinline__ double lat_lse2_mean(double a, double b, double ma, double mb, double &mean)
{
    const double m = fmax(fmax(a, b), -DBL_MAX);
    const float wa = __builtin_amdgcn_exp2f((float)(a - m)), wb = __builtin_amdgcn_exp2f((float)(b - m));
    const float sum = wa + wb;
    const double ref = a == m ? ma : mb;
    mean = ref + ((double)wa * (ma - ref) + (double)wb * (mb - ref)) * (double)__builtin_amdgcn_rcpf(sum);
    return m + (double)__builtin_amdgcn_logf(sum);
}
__device__ __forceinline__ double lat_lse3_mean(double a, double b, double c, double ma, double mb, double mc, double &mean)
{
    const double m = fmax(fmax(fmax(a, b), c), -DBL_MAX);
    const float wa = __builtin_amdgcn_exp2f((float)(a - m)), wb = __builtin_amdgcn_exp2f((float)(b - m)),
                wc = __builtin_amdgcn_exp2f((float)(c - m));
    const float sum = wa + wb + wc;
    const double ref = a == m ? ma : b == m ? mb : mc;
    mean = ref + ((double)wa * (ma - ref) + (double)wb * (mb - ref) + (double)wc * (mc - ref)) *
                     (double)__builtin_amdgcn_rcpf(sum);
    return m + (double)__builtin_amdgcn_logf(sum);
}
// transcript-tolerant CTC: log2(2^e + 2^es), a cell's own emission e mixed with its star term es, on the fp32 pipes.  A star
// term of -inf (weight 0, or no non-blank mass on the frame) leaves e by a select, bit for bit; e = -inf gives es.
__device__ __forceinline__ float lat_star_mix(float e, float es)
{
    return es > -INFINITY ? fmaxf(e, es) + __builtin_amdgcn_logf(1.0f + __builtin_amdgcn_exp2f(-fabsf(e - es))) : e;
}
__device__ __forceinline__ double lat_readlane(double x, int lane)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(x), lane);
    return __hiloint2double(hi, lo);
}

// lattice positions per lane for a lattice of S = 2 L + 1 positions
inline int lat_ppl(int S) { return S <= 64 ? 1 : S <= 128 ? 2 : S <= 256 ? 4 : S <= 512 ? 8 : S <= 1024 ? 16 : 32; }

}  // namespace
