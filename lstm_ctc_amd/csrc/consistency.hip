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
// Two launches, kd.hip's:
//   1. cr_rows_kernel<G, NE, VEC> (V <= 1024) or cr_wide_kernel<VEC> (any V): one GROUP of G lanes per pair-frame, waves walk
//      the pair-frames with a grid stride.  Both rows are loaded ONCE and stay in registers (the exponentials and a_k - b_k:
//      3 NE per lane) across the two maxima, the two sums, the term and the two gradient rows.
//        V <= 64    G = 16: four pair-frames per wave, one per 16-lane DPP row, butterfly reductions
//        V <= 1024  G = 64: one pair-frame per wave, 4 / 8 / 16 elements per lane and row
//        V  > 1024  one pair-frame per wave in three passes over the two rows (maxima + argmaxes, sums, term + gradient), on a
//                   grid capped so that the rows in flight stay in the Infinity Cache (CR_WIDE_INFLIGHT_BYTES)
//      VEC: 16-byte accesses when V % 4 == 0 and both buffers are 16-byte aligned (then every row of either half starts on a
//      16-byte boundary), dwords otherwise.  Lane 0 of the group writes the pair-frame's term and a flag word (1 = scored, 2 =
//      argmaxes agree, 4 = bad row) as ONE 8-byte word to the workspace, laid out [B,T].
//   2. cr_fold_kernel: one workgroup per pair folds its pair-frames' terms in a FIXED order in double and rounds once.
#include "common.h"
#include "row_group.h"
#include <math.h>

#define CR_LOG2E 1.4426950408889634f
#define CR_LN2 0.6931471805599453f
#define CR_MAX_GRID 2048                 // blocks of four waves, as stream_grid in misc.hip
// The wide kernel re-reads both rows of a pair-frame twice, and finds them in the Infinity Cache only while the rows of ALL
// waves in flight fit there: 2 rows x 4 V bytes x 4 waves per block.  kd.hip's cap and its measurement.
#define CR_WIDE_INFLIGHT_BYTES (128ll << 20)
#define CR_WIDE_MIN_GRID 256

namespace {

// first half of an element: za, zb on entry; the exponentials in their place and a - b on exit; the two sums gain theirs
__device__ __forceinline__ void cr_exps(float &za, float &zb, float ma, float mb, float &ab, float &sa, float &sb)
{
    const float a = za - ma, b = zb - mb;
    za = __builtin_amdgcn_exp2f(a * CR_LOG2E);
    zb = __builtin_amdgcn_exp2f(b * CR_LOG2E);
    ab = a - b;
    sa += za;
    sb += zb;
}
// A product that is rounded on its own (no fma).  The two quotients: an fma would leave one product's rounding error as the d
// of two equal rows.  grad_scale d: the accumulated row is then the stored row added to what grad held, in one rounding.
__device__ __forceinline__ float cr_mul(float x, float y)
{
#pragma clang fp contract(off)
    return x * y;
}
// second half: d = qa - qb and its share of J (d = 0, which covers probability 0 in both views: none; no 0 * inf)
__device__ __forceinline__ float cr_diff(float ea, float eb, float ab, float ia, float ib, float dl, float &j)
{
    const float d = cr_mul(ea, ia) - cr_mul(eb, ib);
    j += d != 0.0f ? d * (ab - dl) : 0.0f;
    return d;
}
__device__ __forceinline__ float cr_dlog(float sa, float sb)
{
    return (__builtin_amdgcn_logf(sa) - __builtin_amdgcn_logf(sb)) * CR_LN2;
}

// ------------------------------------------------------------------------------------------ 1a. rows that fit registers
template <int G, int NE, bool VEC>
__global__ __launch_bounds__(256) void cr_rows_kernel(const float *__restrict__ logits, int T, int B, int V,
                                                      const int *__restrict__ seq_len, float scale, int2 *__restrict__ terms,
                                                      float *grad, int acc)
{
    constexpr int FW = 64 / G;                       // pair-frames per wave
    constexpr int NQ = NE / 4;                       // 16-byte accesses per lane and row (VEC)
    const int lane = threadIdx.x & 63, l = lane & (G - 1), g = lane / G;
    const int stride = (int)gridDim.x * 4 * FW;      // <= 2048 * 16 pair-frames per pass
    const int first = ((int)blockIdx.x * 4 + ((int)threadIdx.x >> 6)) * FW;
    const long long TB = (long long)T * B;
    const size_t half = (size_t)B * (size_t)V;       // from a row of view a to its partner in view b
    RgWalk w(first, stride, B);
    for (long long fb = first; fb < TB; fb += stride, w.next(B)) {
        int b = w.b0 + g, t = w.t0;
#pragma unroll
        for (int i = 0; i < FW - 1; ++i)             // g < FW: at most FW - 1 wraps (B = 1)
            if (b >= B) { b -= B; ++t; }
        const bool valid = t < T;
        const size_t bt = (size_t)b * T + t;         // the pair-frame's place in the workspace [B,T]
        const bool scored = valid && t < seq_len[valid ? b : 0];
        const size_t row = ((size_t)t * (2 * (size_t)B) + b) * (size_t)V;      // view a; view b is at row + half
        if (__builtin_amdgcn_ballot_w64(scored) == 0) {          // nothing to score in this wave: no row is read
            if (valid) {
                if (l == 0) terms[bt] = make_int2(0, 0);
                if (grad && !acc) {
                    if (VEC) {
#pragma unroll
                        for (int jq = 0; jq < NQ; ++jq) {
                            const int q = jq * G + l;
                            if (4 * q < V) {
                                *(float4 *)(grad + row + 4 * q) = make_float4(0.f, 0.f, 0.f, 0.f);
                                *(float4 *)(grad + row + half + 4 * q) = make_float4(0.f, 0.f, 0.f, 0.f);
                            }
                        }
                    } else {
#pragma unroll
                        for (int j = 0; j < NE; ++j) {
                            const int e = j * G + l;
                            if (e < V) {
                                grad[row + e] = 0.0f;
                                grad[row + half + e] = 0.0f;
                            }
                        }
                    }
                }
            }
            continue;
        }
        // both rows, once: element idx(j) of the pair-frame, -inf beyond V and in groups that score nothing
        float za[NE], zb[NE], ab[NE];
        if (VEC) {
#pragma unroll
            for (int jq = 0; jq < NQ; ++jq) {
                const int q = jq * G + l;
                float4 u = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY), v = u;
                if (scored && 4 * q < V) {
                    u = *(const float4 *)(logits + row + 4 * q);
                    v = *(const float4 *)(logits + row + half + 4 * q);
                }
                za[4 * jq] = u.x; za[4 * jq + 1] = u.y; za[4 * jq + 2] = u.z; za[4 * jq + 3] = u.w;
                zb[4 * jq] = v.x; zb[4 * jq + 1] = v.y; zb[4 * jq + 2] = v.z; zb[4 * jq + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < NE; ++j) {
                const int e = j * G + l;
                const bool in = scored && e < V;
                za[j] = in ? logits[row + e] : -INFINITY;
                zb[j] = in ? logits[row + half + e] : -INFINITY;
            }
        }
        auto idx = [&](int j) { return VEC ? 4 * ((j >> 2) * G + l) + (j & 3) : j * G + l; };
        float ma = za[0], mb = zb[0];
#pragma unroll
        for (int j = 1; j < NE; ++j) {
            ma = fmaxf(ma, za[j]);
            mb = fmaxf(mb, zb[j]);
        }
        ma = rg_max<G>(ma);
        mb = rg_max<G>(mb);
        // lowest index holding each maximum (idx rises with j inside a lane)
        int ca = 0x7fffffff, cb = 0x7fffffff;
#pragma unroll
        for (int j = NE - 1; j >= 0; --j) {
            const int e = idx(j);
            ca = za[j] == ma ? e : ca;
            cb = zb[j] == mb ? e : cb;
        }
        const bool same = rg_min<G>(ca) == rg_min<G>(cb);
        float sa = 0.0f, sb = 0.0f, jt = 0.0f;
#pragma unroll
        for (int j = 0; j < NE; ++j) cr_exps(za[j], zb[j], ma, mb, ab[j], sa, sb);
        sa = rg_sum<G>(sa);
        sb = rg_sum<G>(sb);
        const bool bad = scored && !(sa == sa && sb == sb);      // NaN exactly when a row's maximum is not finite or it holds a NaN
        const bool good = scored && !bad;
        const float ia = __builtin_amdgcn_rcpf(sa), ib = __builtin_amdgcn_rcpf(sb), dl = cr_dlog(sa, sb);
#pragma unroll
        for (int j = 0; j < NE; ++j) za[j] = cr_diff(za[j], zb[j], ab[j], ia, ib, dl, jt);      // za: d = qa - qb from here on
        jt = rg_sum<G>(jt);
        if (valid && l == 0)
            terms[bt] = make_int2(good ? __float_as_int(jt) : 0, good ? (RG_SCORED | (same ? RG_AGREE : 0)) : (bad ? RG_BAD : 0));
        if (grad && valid && (good || !acc)) {
            if (VEC) {
#pragma unroll
                for (int jq = 0; jq < NQ; ++jq) {
                    const int q = jq * G + l;
                    if (4 * q < V) {
                        float4 u = make_float4(0.f, 0.f, 0.f, 0.f), v = u;
                        if (good) {
                            u.x = cr_mul(scale, za[4 * jq]); u.y = cr_mul(scale, za[4 * jq + 1]);
                            u.z = cr_mul(scale, za[4 * jq + 2]); u.w = cr_mul(scale, za[4 * jq + 3]);
                            v.x = -u.x; v.y = -u.y; v.z = -u.z; v.w = -u.w;
                            if (acc) {
                                const float4 o = *(const float4 *)(grad + row + 4 * q);
                                const float4 p = *(const float4 *)(grad + row + half + 4 * q);
                                u.x += o.x; u.y += o.y; u.z += o.z; u.w += o.w;
                                v.x += p.x; v.y += p.y; v.z += p.z; v.w += p.w;
                            }
                        }
                        *(float4 *)(grad + row + 4 * q) = u;
                        *(float4 *)(grad + row + half + 4 * q) = v;
                    }
                }
            } else {
#pragma unroll
                for (int j = 0; j < NE; ++j) {
                    const int e = j * G + l;
                    if (e < V) {
                        float u = 0.0f, v = 0.0f;
                        if (good) {
                            u = cr_mul(scale, za[j]);
                            v = -u;
                            if (acc) {
                                u += grad[row + e];
                                v += grad[row + half + e];
                            }
                        }
                        grad[row + e] = u;
                        grad[row + half + e] = v;
                    }
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------ 1b. any row width
// One pass of a wave over a row of V elements: 16-byte accesses (VEC: V % 4 == 0, rows aligned) or dwords.  A lane's indices
// rise in the order it visits them.
template <bool VEC, class F1, class F4> __device__ __forceinline__ void cr_walk_row(int lane, int V, F1 f1, F4 f4)
{
    if (VEC)
        for (int q = lane; 4 * q < V; q += 64) f4(4 * q);
    else
        for (int e = lane; e < V; e += 64) f1(e);
}

template <bool VEC>
__global__ __launch_bounds__(256) void cr_wide_kernel(const float *__restrict__ logits, int T, int B, int V,
                                                      const int *__restrict__ seq_len, float scale, int2 *__restrict__ terms,
                                                      float *grad, int acc)
{
    const int lane = threadIdx.x & 63;
    const int stride = (int)gridDim.x * 4;
    const int first = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    const long long TB = (long long)T * B;
    const size_t half = (size_t)B * (size_t)V;
    RgWalk w(first, stride, B);
    for (long long fb = first; fb < TB; fb += stride, w.next(B)) {
        const int b = w.b0, t = w.t0;
        const size_t bt = (size_t)b * T + t;
        const bool scored = t < seq_len[b];
        const size_t row = ((size_t)t * (2 * (size_t)B) + b) * (size_t)V;
        const float *ar = logits + row, *br = logits + row + half;
        float *ga = grad ? grad + row : nullptr, *gb = grad ? grad + row + half : nullptr;
        const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (!scored) {                                                       // wave-uniform
            if (lane == 0) terms[bt] = make_int2(0, 0);
            if (ga && !acc)
                cr_walk_row<VEC>(lane, V, [&](int e) { ga[e] = 0.0f; gb[e] = 0.0f; },
                                 [&](int e) { *(float4 *)(ga + e) = zero4; *(float4 *)(gb + e) = zero4; });
            continue;
        }
        // pass 1: both maxima and the lowest index that holds each (a lane's indices rise, so strictly-greater keeps its first)
        float ma = -INFINITY, mb = -INFINITY;
        int ca = 0x7fffffff, cb = 0x7fffffff;
        auto top = [&](float u, float v, int e) {
            if (u > ma || (ca == 0x7fffffff && u == ma)) { ma = u; ca = e; }
            if (v > mb || (cb == 0x7fffffff && v == mb)) { mb = v; cb = e; }
        };
        cr_walk_row<VEC>(lane, V, [&](int e) { top(ar[e], br[e], e); },
                         [&](int e) {
                             const float4 u = *(const float4 *)(ar + e), v = *(const float4 *)(br + e);
                             top(u.x, v.x, e); top(u.y, v.y, e + 1); top(u.z, v.z, e + 2); top(u.w, v.w, e + 3);
                         });
        const float lma = ma, lmb = mb;
        ma = lc_wave_max(ma);
        mb = lc_wave_max(mb);
        const bool same = rg_min<64>(lma == ma ? ca : 0x7fffffff) == rg_min<64>(lmb == mb ? cb : 0x7fffffff);
        // pass 2: the two sums, per lane in the order of its visits, then over the lanes
        float sa = 0.0f, sb = 0.0f, ab;
        cr_walk_row<VEC>(lane, V,
                         [&](int e) {
                             float u = ar[e], v = br[e];
                             cr_exps(u, v, ma, mb, ab, sa, sb);
                         },
                         [&](int e) {
                             float4 u = *(const float4 *)(ar + e), v = *(const float4 *)(br + e);
                             cr_exps(u.x, v.x, ma, mb, ab, sa, sb);
                             cr_exps(u.y, v.y, ma, mb, ab, sa, sb);
                             cr_exps(u.z, v.z, ma, mb, ab, sa, sb);
                             cr_exps(u.w, v.w, ma, mb, ab, sa, sb);
                         });
        sa = lc_wave_sum(sa);
        sb = lc_wave_sum(sb);
        const bool good = sa == sa && sb == sb;      // a NaN slips past the maximum (comparisons), not past the sum
        if (!good) {
            if (lane == 0) terms[bt] = make_int2(0, RG_BAD);
            if (ga && !acc)
                cr_walk_row<VEC>(lane, V, [&](int e) { ga[e] = 0.0f; gb[e] = 0.0f; },
                                 [&](int e) { *(float4 *)(ga + e) = zero4; *(float4 *)(gb + e) = zero4; });
            continue;
        }
        // pass 3: the term and the two gradient rows
        const float ia = __builtin_amdgcn_rcpf(sa), ib = __builtin_amdgcn_rcpf(sb), dl = cr_dlog(sa, sb);
        float jt = 0.0f, dsa = 0.0f, dsb = 0.0f;
        auto d1 = [&](float u, float v) {
            cr_exps(u, v, ma, mb, ab, dsa, dsb);
            return cr_mul(scale, cr_diff(u, v, ab, ia, ib, dl, jt));
        };
        cr_walk_row<VEC>(lane, V,
                         [&](int e) {
                             const float u = d1(ar[e], br[e]);
                             if (ga) {
                                 ga[e] = acc ? u + ga[e] : u;
                                 gb[e] = acc ? -u + gb[e] : -u;
                             }
                         },
                         [&](int e) {
                             const float4 x = *(const float4 *)(ar + e), y = *(const float4 *)(br + e);
                             float4 u = make_float4(d1(x.x, y.x), d1(x.y, y.y), d1(x.z, y.z), d1(x.w, y.w));
                             float4 v = make_float4(-u.x, -u.y, -u.z, -u.w);
                             if (ga) {
                                 if (acc) {
                                     const float4 o = *(const float4 *)(ga + e), p = *(const float4 *)(gb + e);
                                     u.x += o.x; u.y += o.y; u.z += o.z; u.w += o.w;
                                     v.x += p.x; v.y += p.y; v.z += p.z; v.w += p.w;
                                 }
                                 *(float4 *)(ga + e) = u;
                                 *(float4 *)(gb + e) = v;
                             }
                         });
        jt = lc_wave_sum(jt);
        if (lane == 0) terms[bt] = make_int2(__float_as_int(jt), RG_SCORED | (same ? RG_AGREE : 0));
    }
}

// ------------------------------------------------------------------------------------------ 2. per-pair fold
__global__ __launch_bounds__(256) void cr_fold_kernel(const int2 *__restrict__ terms, int T, float *__restrict__ loss,
                                                      int *__restrict__ frames, int *__restrict__ agree)
{
    rg_fold(terms, T, loss, frames, agree);
}

}  // namespace

extern "C" size_t lc_consistency_workspace_bytes(int T, int B, int V)
{
    if (T <= 0 || B <= 0 || V < 2) return 0;
    return lc_align256((size_t)T * B * sizeof(int2));              // per pair-frame: its term (float) and a flag word
}

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
    hipStream_t s = (hipStream_t)stream;
    int2 *terms = (int2 *)workspace;
    const long long TB = (long long)T * B;
    const int acc = accumulate != 0;
    const bool vec = V % 4 == 0 && (((uintptr_t)logits | (uintptr_t)grad) & 15) == 0;      // then every row of either half is aligned
    long long cap = CR_MAX_GRID;
    if (V > 1024) {
        const long long fit = CR_WIDE_INFLIGHT_BYTES / (32ll * V);
        cap = fit < CR_WIDE_MIN_GRID ? CR_WIDE_MIN_GRID : fit < CR_MAX_GRID ? fit : CR_MAX_GRID;
    }
#define LC_CR(KERNEL, FW)                                                                                               \
    do {                                                                                                                \
        long long nb = (TB + 4 * (FW) - 1) / (4 * (FW));                                                                \
        if (nb > cap) nb = cap;                                                                                         \
        hipLaunchKernelGGL(KERNEL, dim3((unsigned)nb), dim3(256), 0, s, logits, T, B, V, seq_len, grad_scale, terms,    \
                           grad, acc);                                                                                  \
    } while (0)
    if (V <= 64) {
        if (vec) LC_CR((cr_rows_kernel<16, 4, true>), 4); else LC_CR((cr_rows_kernel<16, 4, false>), 4);
    } else if (V <= 256) {
        if (vec) LC_CR((cr_rows_kernel<64, 4, true>), 1); else LC_CR((cr_rows_kernel<64, 4, false>), 1);
    } else if (V <= 512) {
        if (vec) LC_CR((cr_rows_kernel<64, 8, true>), 1); else LC_CR((cr_rows_kernel<64, 8, false>), 1);
    } else if (V <= 1024) {
        if (vec) LC_CR((cr_rows_kernel<64, 16, true>), 1); else LC_CR((cr_rows_kernel<64, 16, false>), 1);
    } else {
        if (vec) LC_CR((cr_wide_kernel<true>), 1); else LC_CR((cr_wide_kernel<false>), 1);
    }
#undef LC_CR
    LC_CHECK_LAUNCH("cr_rows");
    hipLaunchKernelGGL(cr_fold_kernel, dim3(B), dim3(256), 0, s, terms, T, loss, frames, agree);
    LC_CHECK_LAUNCH("cr_fold");
    return LC_OK;
}
