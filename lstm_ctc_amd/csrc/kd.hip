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
// Two launches, xent.hip's:
//   1. kd_rows_kernel<G, NE, VEC> (V <= 1024) or kd_wide_kernel<VEC> (any V): one GROUP of G lanes per frame, waves walk the
//      frames with a grid stride.  Both rows are loaded ONCE and stay in 2 NE registers per lane across the two maxima, the two
//      sums, the KL sum and the gradient store.
//        V <= 64    G = 16: four frames per wave, one per 16-lane DPP row, butterfly reductions (every lane gets the result)
//        V <= 1024  G = 64: one frame per wave, 4 / 8 / 16 elements per lane and row
//        V  > 1024  one frame per wave in three passes over the two rows (maxima + argmaxes, sums, gradient), on a grid
//                   capped so that the rows in flight stay in the Infinity Cache (KD_WIDE_INFLIGHT_BYTES)
//      VEC as in xent.hip: 16-byte accesses when V % 4 == 0 and all three buffers are 16-byte aligned; the wide kernel takes
//      them at any V with a head / body / tail split.  Lane 0 of the group writes the frame's term and a flag word (1 =
//      scored, 2 = argmaxes agree, 4 = bad teacher row) as ONE 8-byte word to the workspace, laid out [B,T].
//   2. kd_fold_kernel: one workgroup per utterance folds its frames' terms in a FIXED order in double and rounds once.
#include "common.h"
#include "row_group.h"
#include <math.h>

#define KD_LOG2E 1.4426950408889634f
#define KD_LN2 0.6931471805599453f
#define KD_MAX_GRID 2048                 // blocks of four waves, as stream_grid in misc.hip
// The wide kernel re-reads both rows of a frame twice, and finds them in the Infinity Cache only while the rows of ALL waves
// in flight fit there: 2 rows x 4 V bytes x 4 waves per block.  Its grid is capped so that they take 128 MiB of the 256 (at
// least one block per CU): V = 5000 at 2048 blocks is 328 MB in flight and was measured at 1603 us per call, at 838 blocks
// 1256 us.
#define KD_WIDE_INFLIGHT_BYTES (128ll << 20)
#define KD_WIDE_MIN_GRID 256

namespace {

// one element of a frame: a = s - ms, b = z - mz on entry; the exponentials on exit; the KL sum gains ep (a - b) where ep > 0
__device__ __forceinline__ void kd_element(float &s, float &z, float ms, float mz, float c, float &sp, float &sq, float &ka)
{
    const float a = s - ms, b = z - mz;
    const float ep = __builtin_amdgcn_exp2f(a * c), eq = __builtin_amdgcn_exp2f(b * c);
    sp += ep;
    sq += eq;
    ka += ep > 0.0f ? ep * (a - b) : 0.0f;
    s = ep;
    z = eq;
}
// the frame's term from its three sums (all lanes hold them)
__device__ __forceinline__ float kd_term(float ka, float sp, float sq, float itau)
{
    return ka * itau * __builtin_amdgcn_rcpf(sp) + (__builtin_amdgcn_logf(sq) - __builtin_amdgcn_logf(sp)) * KD_LN2;
}

// ------------------------------------------------------------------------------------------ 1a. rows that fit registers
template <int G, int NE, bool VEC>
__global__ __launch_bounds__(256) void kd_rows_kernel(const float *__restrict__ logits, const float *__restrict__ teacher,
                                                      int T, int B, int V, const int *__restrict__ seq_len,
                                                      const int *__restrict__ teacher_len, float c, float itau, float scale,
                                                      int2 *__restrict__ terms, float *grad, int acc)
{
    constexpr int FW = 64 / G;                       // frames per wave
    constexpr int NQ = NE / 4;                       // 16-byte accesses per lane and row (VEC)
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
        const size_t bt = (size_t)b * T + t;         // the frame's place in the workspace [B,T]
        int sl = 0, tl = 0;
        if (valid) {
            sl = seq_len[b];
            tl = teacher_len[b];
        }
        const bool scored = valid && t < sl && t < tl;
        const size_t row = ((size_t)t * B + b) * (size_t)V;
        if (__builtin_amdgcn_ballot_w64(scored) == 0) {          // nothing to score in this wave: no row is read
            if (valid) {
                if (l == 0) terms[bt] = make_int2(0, 0);
                if (grad && !acc) {
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
        // both rows, once: element idx(j) of the frame, -inf beyond V and in groups that score nothing
        float s[NE], z[NE];
        if (VEC) {
#pragma unroll
            for (int jq = 0; jq < NQ; ++jq) {
                const int q = jq * G + l;
                float4 u = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY), v = u;
                if (scored && 4 * q < V) {
                    u = *(const float4 *)(teacher + row + 4 * q);
                    v = *(const float4 *)(logits + row + 4 * q);
                }
                s[4 * jq] = u.x; s[4 * jq + 1] = u.y; s[4 * jq + 2] = u.z; s[4 * jq + 3] = u.w;
                z[4 * jq] = v.x; z[4 * jq + 1] = v.y; z[4 * jq + 2] = v.z; z[4 * jq + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < NE; ++j) {
                const int e = j * G + l;
                const bool in = scored && e < V;
                s[j] = in ? teacher[row + e] : -INFINITY;
                z[j] = in ? logits[row + e] : -INFINITY;
            }
        }
        auto idx = [&](int j) { return VEC ? 4 * ((j >> 2) * G + l) + (j & 3) : j * G + l; };
        float ms = s[0], mz = z[0];
#pragma unroll
        for (int j = 1; j < NE; ++j) {
            ms = fmaxf(ms, s[j]);
            mz = fmaxf(mz, z[j]);
        }
        ms = rg_max<G>(ms);
        mz = rg_max<G>(mz);
        // lowest index holding each maximum (idx rises with j inside a lane)
        int cs = 0x7fffffff, cz = 0x7fffffff;
#pragma unroll
        for (int j = NE - 1; j >= 0; --j) {
            const int e = idx(j);
            cs = s[j] == ms ? e : cs;
            cz = z[j] == mz ? e : cz;
        }
        const bool same = rg_min<G>(cs) == rg_min<G>(cz);
        float sp = 0.0f, sq = 0.0f, ka = 0.0f;
#pragma unroll
        for (int j = 0; j < NE; ++j) kd_element(s[j], z[j], ms, mz, c, sp, sq, ka);
        sp = rg_sum<G>(sp);
        sq = rg_sum<G>(sq);
        ka = rg_sum<G>(ka);
        const bool bad = scored && !(sp == sp);      // NaN exactly when the teacher row's maximum is not finite or it holds a NaN
        const bool good = scored && !bad;
        if (valid && l == 0)
            terms[bt] = make_int2(good ? __float_as_int(kd_term(ka, sp, sq, itau)) : 0,
                                  good ? (RG_SCORED | (same ? RG_AGREE : 0)) : (bad ? RG_BAD : 0));
        if (grad && valid && (good || !acc)) {
            const float ip = good ? scale * __builtin_amdgcn_rcpf(sp) : 0.0f, iq = good ? scale * __builtin_amdgcn_rcpf(sq) : 0.0f;
            if (VEC) {
#pragma unroll
                for (int jq = 0; jq < NQ; ++jq) {
                    const int q = jq * G + l;
                    if (4 * q < V) {
                        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                        if (good) {
                            v.x = z[4 * jq] * iq - s[4 * jq] * ip;
                            v.y = z[4 * jq + 1] * iq - s[4 * jq + 1] * ip;
                            v.z = z[4 * jq + 2] * iq - s[4 * jq + 2] * ip;
                            v.w = z[4 * jq + 3] * iq - s[4 * jq + 3] * ip;
                            if (acc) {
                                const float4 o = *(const float4 *)(grad + row + 4 * q);
                                v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
                            }
                        }
                        *(float4 *)(grad + row + 4 * q) = v;
                    }
                }
            } else {
#pragma unroll
                for (int j = 0; j < NE; ++j) {
                    const int e = j * G + l;
                    if (e < V) {
                        float v = 0.0f;
                        if (good) {
                            v = z[j] * iq - s[j] * ip;
                            if (acc) v += grad[row + e];
                        }
                        grad[row + e] = v;
                    }
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------ 1b. any row width
// rg_walk_row (row_group.h) is one pass of a wave over a row.
template <bool VEC>
__global__ __launch_bounds__(256) void kd_wide_kernel(const float *__restrict__ logits, const float *__restrict__ teacher,
                                                      int T, int B, int V, const int *__restrict__ seq_len,
                                                      const int *__restrict__ teacher_len, float c, float itau, float scale,
                                                      int2 *__restrict__ terms, float *grad, int acc)
{
    const int lane = threadIdx.x & 63;
    const int stride = (int)gridDim.x * 4;
    const int first = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    const long long TB = (long long)T * B;
    RgWalk w(first, stride, B);
    for (long long fb = first; fb < TB; fb += stride, w.next(B)) {
        const int b = w.b0, t = w.t0;
        const size_t bt = (size_t)b * T + t;
        const bool scored = t < seq_len[b] && t < teacher_len[b];
        const size_t row = ((size_t)t * B + b) * (size_t)V;
        const int head = (int)((4 - (row & 3)) & 3);
        const float *zr = logits + row, *sr = teacher + row;
        float *gr = grad ? grad + row : nullptr;
        if (!scored) {                                                       // wave-uniform
            if (lane == 0) terms[bt] = make_int2(0, 0);
            if (gr && !acc)
                rg_walk_row<VEC>(lane, V, head, [&](int e) { gr[e] = 0.0f; },
                                 [&](int e) { *(float4 *)(gr + e) = make_float4(0.f, 0.f, 0.f, 0.f); });
            continue;
        }
        // pass 1: both maxima and the lowest index that holds each (a lane's indices rise, so strictly-greater keeps its first)
        float ms = -INFINITY, mz = -INFINITY;
        int cs = 0x7fffffff, cz = 0x7fffffff;
        auto top = [&](float u, float v, int e) {
            if (u > ms || (cs == 0x7fffffff && u == ms)) { ms = u; cs = e; }
            if (v > mz || (cz == 0x7fffffff && v == mz)) { mz = v; cz = e; }
        };
        rg_walk_row<VEC>(lane, V, head, [&](int e) { top(sr[e], zr[e], e); },
                         [&](int e) {
                             const float4 u = *(const float4 *)(sr + e), v = *(const float4 *)(zr + e);
                             top(u.x, v.x, e); top(u.y, v.y, e + 1); top(u.z, v.z, e + 2); top(u.w, v.w, e + 3);
                         });
        const float lms = ms, lmz = mz;
        ms = lc_wave_max(ms);
        mz = lc_wave_max(mz);
        const bool same = rg_min<64>(lms == ms ? cs : 0x7fffffff) == rg_min<64>(lmz == mz ? cz : 0x7fffffff);
        // pass 2: the three sums, per lane in the order of its visits, then over the lanes
        float sp = 0.0f, sq = 0.0f, ka = 0.0f;
        rg_walk_row<VEC>(lane, V, head,
                         [&](int e) {
                             float u = sr[e], v = zr[e];
                             kd_element(u, v, ms, mz, c, sp, sq, ka);
                         },
                         [&](int e) {
                             float4 u = *(const float4 *)(sr + e), v = *(const float4 *)(zr + e);
                             kd_element(u.x, v.x, ms, mz, c, sp, sq, ka);
                             kd_element(u.y, v.y, ms, mz, c, sp, sq, ka);
                             kd_element(u.z, v.z, ms, mz, c, sp, sq, ka);
                             kd_element(u.w, v.w, ms, mz, c, sp, sq, ka);
                         });
        sp = lc_wave_sum(sp);
        sq = lc_wave_sum(sq);
        ka = lc_wave_sum(ka);
        const bool good = sp == sp;                  // a NaN teacher slips past the maximum (comparisons), not past the sum
        if (lane == 0)
            terms[bt] = make_int2(good ? __float_as_int(kd_term(ka, sp, sq, itau)) : 0,
                                  good ? (RG_SCORED | (same ? RG_AGREE : 0)) : RG_BAD);
        // pass 3: the gradient row
        if (gr && (good || !acc)) {
            const float ip = good ? scale * __builtin_amdgcn_rcpf(sp) : 0.0f, iq = good ? scale * __builtin_amdgcn_rcpf(sq) : 0.0f;
            auto g1 = [&](float u, float v, float o) {
                if (!good) return 0.0f;
                const float d = __builtin_amdgcn_exp2f((v - mz) * c) * iq - __builtin_amdgcn_exp2f((u - ms) * c) * ip;
                return acc ? d + o : d;
            };
            rg_walk_row<VEC>(lane, V, head,
                             [&](int e) {
                                 float o = 0.0f, u = 0.0f, v = 0.0f;
                                 if (good) { u = sr[e]; v = zr[e]; if (acc) o = gr[e]; }
                                 gr[e] = g1(u, v, o);
                             },
                             [&](int e) {
                                 float4 o = make_float4(0.f, 0.f, 0.f, 0.f), u = o, v = o;
                                 if (good) {
                                     u = *(const float4 *)(sr + e);
                                     v = *(const float4 *)(zr + e);
                                     if (acc) o = *(const float4 *)(gr + e);
                                 }
                                 *(float4 *)(gr + e) = make_float4(g1(u.x, v.x, o.x), g1(u.y, v.y, o.y), g1(u.z, v.z, o.z), g1(u.w, v.w, o.w));
                             });
        }
    }
}

// ------------------------------------------------------------------------------------------ 2. per-utterance fold
__global__ __launch_bounds__(256) void kd_fold_kernel(const int2 *__restrict__ terms, int T, float *__restrict__ loss,
                                                      int *__restrict__ frames, int *__restrict__ agree)
{
    rg_fold(terms, T, loss, frames, agree);
}

}  // namespace

extern "C" size_t lc_kd_workspace_bytes(int T, int B, int V)
{
    if (T <= 0 || B <= 0 || V < 2) return 0;
    return lc_align256((size_t)T * B * sizeof(int2));              // per frame: its term (float) and a flag word
}

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
    hipStream_t s = (hipStream_t)stream;
    int2 *terms = (int2 *)workspace;
    const long long TB = (long long)T * B;
    const float c = KD_LOG2E * itau;
    const int acc = accumulate != 0;
    const bool aligned = (((uintptr_t)logits | (uintptr_t)teacher | (uintptr_t)grad) & 15) == 0;
    const bool vec = aligned && V % 4 == 0;          // rows in registers: every row starts on a 16-byte boundary
    long long cap = KD_MAX_GRID;
    if (V > 1024) {
        const long long fit = KD_WIDE_INFLIGHT_BYTES / (32ll * V);
        cap = fit < KD_WIDE_MIN_GRID ? KD_WIDE_MIN_GRID : fit < KD_MAX_GRID ? fit : KD_MAX_GRID;
    }
#define LC_KD(KERNEL, FW)                                                                                               \
    do {                                                                                                                \
        long long nb = (TB + 4 * (FW) - 1) / (4 * (FW));                                                                \
        if (nb > cap) nb = cap;                                                                                         \
        hipLaunchKernelGGL(KERNEL, dim3((unsigned)nb), dim3(256), 0, s, logits, teacher, T, B, V, seq_len, teacher_len, \
                           c, itau, grad_scale, terms, grad, acc);                                                      \
    } while (0)
    if (V <= 64) {
        if (vec) LC_KD((kd_rows_kernel<16, 4, true>), 4); else LC_KD((kd_rows_kernel<16, 4, false>), 4);
    } else if (V <= 256) {
        if (vec) LC_KD((kd_rows_kernel<64, 4, true>), 1); else LC_KD((kd_rows_kernel<64, 4, false>), 1);
    } else if (V <= 512) {
        if (vec) LC_KD((kd_rows_kernel<64, 8, true>), 1); else LC_KD((kd_rows_kernel<64, 8, false>), 1);
    } else if (V <= 1024) {
        if (vec) LC_KD((kd_rows_kernel<64, 16, true>), 1); else LC_KD((kd_rows_kernel<64, 16, false>), 1);
    } else {
        if (aligned) LC_KD((kd_wide_kernel<true>), 1); else LC_KD((kd_wide_kernel<false>), 1);
    }
#undef LC_KD
    LC_CHECK_LAUNCH("kd_rows");
    hipLaunchKernelGGL(kd_fold_kernel, dim3(B), dim3(256), 0, s, terms, T, loss, frames, agree);
    LC_CHECK_LAUNCH("kd_fold");
    return LC_OK;
}
