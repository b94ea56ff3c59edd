// layer_norm.hip - layer normalisation of a layer's output between the LSTM layers (lc_layer_norm_fwd / lc_layer_norm_bwd,
// include/lstm_ctc_hip.h), with the DropoutWrapper mask behind it.  One streaming pass each on row_stream.h's
// skeleton: a row is read once into registers by LPR lanes of one wave, reduced with cross-lane adds, and written once.  Dead
// rows are written +0 and never read.  No atomics: the parameter gradients go through per-workgroup partials in the workspace.
#include "row_stream.h"

namespace {

enum { LN_MAX_GROUPS = 1024 };       // workgroups per launch (4 per CU), = the most [2, C] partials of the backward
enum { LN_MAX_C = 8192 };            // 128 floats per lane at 64 lanes
enum { LN_REG_C = 2048 };            // up to here the backward's per-lane dgamma / dbeta sums live in registers, beyond in LDS

template <int VW> struct alignas(4 * VW) Vec { float e[VW]; };

// sum over the LPR lanes (a power of two, an aligned part of one wave) that hold a row; every lane gets the same bits
template <int LPR> __device__ __forceinline__ float group_sum(float v)
{
#pragma unroll
    for (int m = LPR / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// the lane's vectors of a row: vector q = k * LPR + lane for k < NP, as far as the row goes (the outer test is wave-uniform)
// LN_FENCE ends an iteration that loads or stores: the compiler keeps the next one's memory accesses (and with them its mask
// hashes) behind it instead of interleaving all NP iterations, which cost the wide kernels hundreds of registers
#define LN_FENCE asm volatile("" ::: "memory")
#define LN_FOR(k, q) _Pragma("unroll") for (int k = 0; k < NP; ++k) if (k * LPR < CV) if (const int q = k * LPR + lane; q < CV)

// The DropoutWrapper factor of the VW elements of vector q in row r: element c of the row belongs to mask stream
// stream0 + c / dw at index r * dw + c % dw - what lc_dropout_scale gives on a [rows, dw] column window.
template <int VW>
__device__ __forceinline__ void mask_of(Vec<VW> &f, int q, long long r, float keep, float inv_keep, uint32_t seed, uint32_t stream0,
                                        int dw)
{
    const int c = q * VW;
    int s = c / dw, cm = c - s * dw;
#pragma unroll
    for (int j = 0; j < VW; ++j) {
        f.e[j] = lc_dropout_factor(seed, stream0 + (uint32_t)s, (uint64_t)r * (uint64_t)dw + (uint64_t)cm, keep, inv_keep);
        if (++cm == dw) { cm = 0; ++s; }
    }
}

// mean and 1 / sqrt(biased variance + eps) of the row held in v: the centred two-pass form on the registers
template <int VW, int LPR, int NP>
__device__ __forceinline__ void row_stats(const Vec<VW> (&v)[NP], int lane, int CV, int C, float eps, float &mean, float &rstd)
{
    float s = 0.f;
    LN_FOR(k, q) {
#pragma unroll
        for (int j = 0; j < VW; ++j) s += v[k].e[j];
    }
    mean = group_sum<LPR>(s) / (float)C;
    float ss = 0.f;
    LN_FOR(k, q) {
#pragma unroll
        for (int j = 0; j < VW; ++j) { const float d = v[k].e[j] - mean; ss += d * d; }
    }
    rstd = 1.0f / sqrtf(group_sum<LPR>(ss) / (float)C + eps);
}

template <int VW, int LPR, int NP>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const float *__restrict__ x, long long ldx, const float *__restrict__ gamma,
                                                     const float *__restrict__ beta, long long nrows, int CV, int C, int T, int B,
                                                     float eps, const int *__restrict__ seq_len, float keep, float inv_keep,
                                                     uint32_t seed, uint32_t stream0, int dw, float *__restrict__ y, long long ldy)
{
    typedef Vec<VW> V;
    constexpr int RPB = 256 / LPR;
    const int lane = threadIdx.x % LPR, sub = threadIdx.x / LPR;
    const long long groups = (nrows + RPB - 1) / RPB;
    for (long long g = blockIdx.x; g < groups; g += gridDim.x) {
        const long long r = g * RPB + sub;
        if (r >= nrows) continue;
        const long long t = r / B;
        int len = seq_len[(int)(r - t * B)];
        len = len < 0 ? 0 : (len > T ? T : len);
        V *dst = reinterpret_cast<V *>(y + r * ldy);
        if (t >= len) {
            zero_row<V, LPR>(dst, CV, lane);
            continue;
        }
        const V *src = reinterpret_cast<const V *>(x + r * ldx);
        V v[NP];
        LN_FOR(k, q) v[k] = src[q];
        float mean, rstd;
        row_stats<VW, LPR, NP>(v, lane, CV, C, eps, mean, rstd);
        LN_FOR(k, q) {
            const V ga = reinterpret_cast<const V *>(gamma)[q], be = reinterpret_cast<const V *>(beta)[q];
            V o;
#pragma unroll
            for (int j = 0; j < VW; ++j) o.e[j] = __fmaf_rn((v[k].e[j] - mean) * rstd, ga.e[j], be.e[j]);
            if (keep < 1.f) {
                V f;
                mask_of<VW>(f, q, r, keep, inv_keep, seed, stream0, dw);
#pragma unroll
                for (int j = 0; j < VW; ++j) o.e[j] *= f.e[j];
            }
            dst[q] = o;
            LN_FENCE;
        }
    }
}

// Workgroup blockIdx.x walks the row groups [blockIdx.x * per, (blockIdx.x + 1) * per) and leaves one [2, C] partial (dgamma
// row, dbeta row) at part + blockIdx.x * 2 * C.  LDSACC (rows wider than LN_REG_C, one wave per workgroup): the lane's sums
// live in its own LDS slots instead of registers.  dx may be dy (same pitch): the row is in registers before it is written.
template <int VW, int LPR, int NP, int BLOCK, bool LDSACC>
__global__ __launch_bounds__(BLOCK) void ln_bwd_kernel(const float *__restrict__ x, long long ldx, const float *dy, long long lddy,
                                                       const float *__restrict__ gamma, long long nrows, int CV, int C, int T, int B,
                                                       float eps, const int *__restrict__ seq_len, float keep, float inv_keep,
                                                       uint32_t seed, uint32_t stream0, int dw, float *dx, long long lddx,
                                                       float *__restrict__ part, long long per)
{
    typedef Vec<VW> V;
    constexpr int RPB = BLOCK / LPR;
    constexpr int CMAX = LDSACC ? LN_MAX_C : LN_REG_C;
    static_assert(!LDSACC || RPB == 1, "LDS sums are one wave's");
    __shared__ float sm[2 * CMAX];
    const int lane = threadIdx.x % LPR, sub = threadIdx.x / LPR;
    const long long groups = (nrows + RPB - 1) / RPB;
    V dg[LDSACC ? 1 : NP], db[LDSACC ? 1 : NP];
    if constexpr (LDSACC) {
        if (part) LN_FOR(k, q) {
#pragma unroll
            for (int j = 0; j < VW; ++j) sm[q * VW + j] = sm[CMAX + q * VW + j] = 0.f;
        }
    } else {
#pragma unroll
        for (int k = 0; k < NP; ++k) dg[k] = db[k] = V{};
    }
    long long g1 = (blockIdx.x + 1) * per;
    g1 = g1 < groups ? g1 : groups;
    for (long long g = blockIdx.x * per; g < g1; ++g) {
        const long long r = g * RPB + sub;
        if (r >= nrows) continue;
        const long long t = r / B;
        int len = seq_len[(int)(r - t * B)];
        len = len < 0 ? 0 : (len > T ? T : len);
        V *dst = reinterpret_cast<V *>(dx + r * lddx);
        if (t >= len) {
            // zero_row written out: called, the wide instantiations of this kernel come out with other registers and spills
            if (dx) for (int q = lane; q < CV; q += LPR) dst[q] = V{};
            continue;
        }
        const V *src = reinterpret_cast<const V *>(x + r * ldx), *gsrc = reinterpret_cast<const V *>(dy + r * lddy);
        V v[NP], gr[NP];
        LN_FOR(k, q) { v[k] = src[q]; gr[k] = gsrc[q]; }
        float mean, rstd;
        row_stats<VW, LPR, NP>(v, lane, CV, C, eps, mean, rstd);
        // v becomes xh, gr the masked dy; the sums of gamma g and gamma g xh
        float s1 = 0.f, s2 = 0.f;
        LN_FOR(k, q) {
            const V ga = reinterpret_cast<const V *>(gamma)[q];
            if (keep < 1.f) {
                V f;
                mask_of<VW>(f, q, r, keep, inv_keep, seed, stream0, dw);
#pragma unroll
                for (int j = 0; j < VW; ++j) gr[k].e[j] *= f.e[j];
            }
#pragma unroll
            for (int j = 0; j < VW; ++j) {
                v[k].e[j] = (v[k].e[j] - mean) * rstd;
                const float a = ga.e[j] * gr[k].e[j];
                s1 += a;
                s2 += a * v[k].e[j];
            }
            LN_FENCE;
        }
        s1 = group_sum<LPR>(s1) / (float)C;
        s2 = group_sum<LPR>(s2) / (float)C;
        LN_FOR(k, q) {
            if (part) {
                if constexpr (LDSACC) {
#pragma unroll
                    for (int j = 0; j < VW; ++j) {
                        sm[q * VW + j] += gr[k].e[j] * v[k].e[j];
                        sm[CMAX + q * VW + j] += gr[k].e[j];
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < VW; ++j) {
                        dg[k].e[j] += gr[k].e[j] * v[k].e[j];
                        db[k].e[j] += gr[k].e[j];
                    }
                }
            }
            if (dx) {
                const V ga = reinterpret_cast<const V *>(gamma)[q];
                V o;
#pragma unroll
                for (int j = 0; j < VW; ++j) o.e[j] = rstd * (ga.e[j] * gr[k].e[j] - s1 - v[k].e[j] * s2);
                dst[q] = o;
            }
            LN_FENCE;
        }
    }
    if (!part) return;
    if constexpr (!LDSACC) {
        // the workgroup's row groups, one after the other in a fixed order
        for (int s = 0; s < RPB; ++s) {
            if (sub == s) LN_FOR(k, q) {
#pragma unroll
                for (int j = 0; j < VW; ++j) {
                    const int c = q * VW + j;
                    sm[c] = s == 0 ? dg[k].e[j] : sm[c] + dg[k].e[j];
                    sm[CMAX + c] = s == 0 ? db[k].e[j] : sm[CMAX + c] + db[k].e[j];
                }
            }
            __syncthreads();
        }
    } else {
        __syncthreads();
    }
    float *p = part + (long long)blockIdx.x * 2 * C;
    for (int c = threadIdx.x; c < C; c += BLOCK) { p[c] = sm[c]; p[C + c] = sm[CMAX + c]; }
}

// dgamma | dbeta = the sum of the nparts [2, C] partials, in a fixed order: 64 outputs per workgroup, four slices of the partials
// side by side, the four slice sums added in order.
__global__ __launch_bounds__(256) void ln_fold_kernel(const float *__restrict__ part, int nparts, int C, float *__restrict__ dgamma,
                                                      float *__restrict__ dbeta)
{
    __shared__ float sm[4][64];
    const int cx = threadIdx.x % 64, sl = threadIdx.x / 64;
    const int o = blockIdx.x * 64 + cx;
    const int per = (nparts + 3) / 4;
    const int p1 = (sl + 1) * per < nparts ? (sl + 1) * per : nparts;
    float s = 0.f;
    if (o < 2 * C)
        for (int p = sl * per; p < p1; ++p) s += part[(long long)p * 2 * C + o];
    sm[sl][cx] = s;
    __syncthreads();
    if (sl == 0 && o < 2 * C) {
        const float v = ((sm[0][cx] + sm[1][cx]) + sm[2][cx]) + sm[3][cx];
        if (o < C) dgamma[o] = v; else dbeta[o - C] = v;
    }
}

// the workgroups of the backward over nrows rows at `rpb` rows per workgroup pass, and the row groups each of them walks
void ln_bwd_shares(long long nrows, int rpb, long long &per, int &nparts)
{
    const long long groups = (nrows + rpb - 1) / rpb;
    per = (groups + LN_MAX_GROUPS - 1) / LN_MAX_GROUPS;
    nparts = (int)((groups + per - 1) / per);
}

size_t ln_workspace_bytes(long long nrows, int C)
{
    // the most partials any lane choice gives: one per workgroup, at most one per row
    const long long parts = nrows < LN_MAX_GROUPS ? nrows : LN_MAX_GROUPS;
    return lc_align256((size_t)parts * 2 * (size_t)C * sizeof(float));
}

#define LN_SHAPE_OK(T, B, C) ((T) > 0 && (B) > 0 && (C) > 0 && (C) <= LN_MAX_C)

}  // namespace

extern "C" size_t lc_layer_norm_workspace_bytes(int T, int B, int C)
{
    if (!LN_SHAPE_OK(T, B, C)) return 0;
    return ln_workspace_bytes((long long)T * B, C);
}

extern "C" int lc_layer_norm_fwd(const float *x, int ldx, const float *gamma, const float *beta, int T, int B, int C, float eps,
                                 const int *seq_len, float keep, uint32_t seed, uint32_t stream0, int drop_width, float *y, int ldy,
                                 lc_stream_t stream)
{
    const char *who = "lc_layer_norm_fwd";
    LC_CHECK_ARG(LN_SHAPE_OK(T, B, C), "%s: bad shape (T %d, B %d, C %d; C in 1..%d)", who, T, B, C, (int)LN_MAX_C);
    LC_CHECK_ARG(x && gamma && beta && seq_len && y, "%s: null pointer", who);
    LC_CHECK_ARG(ldx >= C && ldy >= C, "%s: a row pitch (%d, %d) below C %d", who, ldx, ldy, C);
    LC_CHECK_ARG(eps > 0.f && keep > 0.f && keep <= 1.f, "%s: need eps > 0 and keep in (0, 1], got %g, %g", who, eps, keep);
    LC_CHECK_ARG(drop_width >= 1 && C % drop_width == 0, "%s: drop_width %d does not divide C %d", who, drop_width, C);
    const long long nrows = (long long)T * B;
    LC_CHECK_ARG(!rs_overlap(x, ldx, nrows, C, y, ldy, nrows, C), "%s: x and y overlap", who);
    const bool vec = rs_vec16(C, {ldx, ldy}, {x, y, gamma, beta});
    const int CV = vec ? C / 4 : C, lpr = rs_lanes_fewest_idle(CV, 4, 64), passes = (CV + lpr - 1) / lpr;
    const dim3 grid(rs_grid(nrows, 256 / lpr, LN_MAX_GROUPS)), block(256);
    hipStream_t s = (hipStream_t)stream;
#define LC_LN(VW, L, NP) hipLaunchKernelGGL((ln_fwd_kernel<VW, L, NP>), grid, block, 0, s, x, (long long)ldx, gamma, beta, nrows, CV, \
                                            C, T, B, eps, seq_len, keep, 1.0f / keep, seed, stream0, drop_width, y, (long long)ldy)
    // below 64 lanes a lane holds at most 8 vectors; a whole wave holds the row however many passes that takes
    rs_dispatch_lanes<4, 64>(lpr, [&](auto lanes) {
        constexpr int L = decltype(lanes)::value;
        if constexpr (L < 64) {
            if (vec) LC_LN(4, L, 8); else LC_LN(1, L, 8);
        } else if (vec) {
            if (passes <= 8) LC_LN(4, 64, 8); else LC_LN(4, 64, 32);
        } else {
            if (passes <= 32) LC_LN(1, 64, 32); else LC_LN(1, 64, 128);
        }
    });
#undef LC_LN
    LC_CHECK_LAUNCH(who);
    return LC_OK;
}

extern "C" int lc_layer_norm_bwd(const float *x, int ldx, const float *dy, int lddy, const float *gamma, int T, int B, int C,
                                 float eps, const int *seq_len, float keep, uint32_t seed, uint32_t stream0, int drop_width,
                                 float *dx, int lddx, float *dgamma, float *dbeta, void *workspace, size_t workspace_bytes,
                                 lc_stream_t stream)
{
    const char *who = "lc_layer_norm_bwd";
    LC_CHECK_ARG(LN_SHAPE_OK(T, B, C), "%s: bad shape (T %d, B %d, C %d; C in 1..%d)", who, T, B, C, (int)LN_MAX_C);
    LC_CHECK_ARG(x && dy && gamma && seq_len, "%s: null pointer", who);
    LC_CHECK_ARG((dgamma != nullptr) == (dbeta != nullptr), "%s: dgamma and dbeta go together (both or neither)", who);
    LC_CHECK_ARG(dx || dgamma, "%s: nothing to compute (dx, dgamma and dbeta are all NULL)", who);
    LC_CHECK_ARG(ldx >= C && lddy >= C && (!dx || lddx >= C), "%s: a row pitch (%d, %d, %d) below C %d", who, ldx, lddy, lddx, C);
    LC_CHECK_ARG(eps > 0.f && keep > 0.f && keep <= 1.f, "%s: need eps > 0 and keep in (0, 1], got %g, %g", who, eps, keep);
    LC_CHECK_ARG(drop_width >= 1 && C % drop_width == 0, "%s: drop_width %d does not divide C %d", who, drop_width, C);
    const long long nrows = (long long)T * B;
    if (dx) {
        LC_CHECK_ARG(!rs_overlap(x, ldx, nrows, C, dx, lddx, nrows, C), "%s: x and dx overlap", who);
        LC_CHECK_ARG((dx == dy && lddx == lddy) || !rs_overlap(dy, lddy, nrows, C, dx, lddx, nrows, C),
                     "%s: dy and dx overlap (dx == dy with one pitch is the in-place form)", who);
    }
    if (dgamma) {
        LC_CHECK_ARG(workspace && workspace_bytes >= ln_workspace_bytes(nrows, C),
                     "%s: workspace of %zu bytes, lc_layer_norm_workspace_bytes asks for %zu", who, workspace ? workspace_bytes : 0,
                     ln_workspace_bytes(nrows, C));
        LC_CHECK_ARG(dgamma != dbeta, "%s: dgamma and dbeta are one pointer", who);
    }
    const bool vec = rs_vec16(C, {ldx, lddy, dx ? lddx : 0}, {x, dy, dx, gamma});
    const int CV = vec ? C / 4 : C, lpr = rs_lanes_fewest_idle(CV, 4, 64), passes = (CV + lpr - 1) / lpr;
    const bool wide = C > LN_REG_C;             // one wave per workgroup, its sums in LDS
    long long per;
    int nparts;
    ln_bwd_shares(nrows, wide ? 1 : 256 / lpr, per, nparts);
    float *part = dgamma ? (float *)workspace : nullptr;
    hipStream_t s = (hipStream_t)stream;
#define LC_LN(VW, L, NP, BLOCK, LDSACC) hipLaunchKernelGGL((ln_bwd_kernel<VW, L, NP, BLOCK, LDSACC>), dim3(nparts), dim3(BLOCK), 0, s, \
                                                           x, (long long)ldx, dy, (long long)lddy, gamma, nrows, CV, C, T, B, eps,     \
                                                           seq_len, keep, 1.0f / keep, seed, stream0, drop_width, dx,                 \
                                                           (long long)lddx, part, per)
    // as the forward; past LN_REG_C (more passes than the registers take) one wave per workgroup with its sums in LDS
    rs_dispatch_lanes<4, 64>(lpr, [&](auto lanes) {
        constexpr int L = decltype(lanes)::value;
        if constexpr (L < 64) {
            if (vec) LC_LN(4, L, 8, 256, false); else LC_LN(1, L, 8, 256, false);
        } else if (vec) {
            if (passes <= 8) LC_LN(4, 64, 8, 256, false); else LC_LN(4, 64, 32, 64, true);
        } else {
            if (passes <= 32) LC_LN(1, 64, 32, 256, false); else LC_LN(1, 64, 128, 64, true);
        }
    });
#undef LC_LN
    LC_CHECK_LAUNCH(who);
    if (dgamma) {
        hipLaunchKernelGGL(ln_fold_kernel, dim3((2 * C + 63) / 64), dim3(256), 0, s, part, nparts, C, dgamma, dbeta);
        LC_CHECK_LAUNCH(who);
    }
    return LC_OK;
}
