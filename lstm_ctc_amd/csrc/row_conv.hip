// row_conv.hip - row convolution (lookahead convolution, Amodei et al. 2016, "Deep Speech 2"; no reference counterpart): one
// depthwise filter over the next tau frames of the uni-LSTM's top layer (lc_row_conv_fwd / lc_row_conv_bwd,
// include/lstm_ctc_hip.h).  x, y, dy, dx are time-major [T * B, C] with row pitches, w and dw dense
// [tau + 1, C].  Pure HBM streams: lanes along c, a thread produces ROWCONV_SEG consecutive frames of a fixed (b, c range) from
// one walk over their tau + ROWCONV_SEG source rows - rows B * ld floats apart - so that a row is loaded (tau + 8) / 8 times,
// not tau + 1 times, and the repeats are L2's.  Dead frames are never read.
#include "row_stream.h"

namespace {

constexpr int ROWCONV_MAX_TAU = 32;      // design cap: a column group's weights fit in LDS (33 x 64 float4 = 33 KB)
constexpr int ROWCONV_SEG = 8;           // consecutive frames one thread produces, their sums in registers
constexpr int ROWCONV_SLABS = 512;       // row slabs of the dw reduction at most ...
constexpr int ROWCONV_SLAB_ROWS = 64;    // ... of at least this many rows each
constexpr int ROWCONV_JT = 8;            // kernel rows one dw workgroup accumulates

struct RowConvArgs {
    int T, B, tau;
    int fwd;                // 1: y from x (sources t + j, live ones only); 0: dx from dy (sources t - j >= 0)
    const int *seq_len;
};

__device__ __forceinline__ int rc_len(const RowConvArgs &a, int b)
{
    const int n = a.seq_len[b];
    return n < 0 ? 0 : (n > a.T ? a.T : n);
}

__device__ __forceinline__ float rc_mul(float w, float v) { return w * v; }
__device__ __forceinline__ float4 rc_mul(float4 w, float4 v) { return make_float4(w.x * v.x, w.y * v.y, w.z * v.z, w.w * v.w); }
__device__ __forceinline__ float rc_fma(float w, float v, float s) { return fmaf(w, v, s); }
__device__ __forceinline__ float4 rc_fma(float4 w, float4 v, float4 s)
{
    return make_float4(fmaf(w.x, v.x, s.x), fmaf(w.y, v.y, s.y), fmaf(w.z, v.z, s.z), fmaf(w.w, v.w, s.w));
}
__device__ __forceinline__ float rc_add(float a, float b) { return a + b; }
__device__ __forceinline__ float4 rc_add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// y / dx.  blockIdx.x: a group of LPR column vectors, whose tau + 1 weight vectors sit in LDS; LPR lanes walk one (segment, b)
// item, 256 / LPR items per workgroup pass, items by grid stride over blockIdx.y.  An item is ROWCONV_SEG consecutive frames
// of one utterance; items run b fastest, so a workgroup's rows are neighbours in memory.  Every output row is written exactly
// once: the sum in ascending j, the first term initialising it, or +0 for a dead row.
template <typename V, int LPR>
__global__ __launch_bounds__(256) void row_conv_rows_kernel(const float *__restrict__ x, long long ldx, const float *__restrict__ w,
                                                            int C, int CV, long long items, RowConvArgs a,
                                                            float *__restrict__ out, long long ldo)
{
    constexpr int RPB = 256 / LPR;
    __shared__ V wl[(ROWCONV_MAX_TAU + 1) * LPR];
    const int lane = threadIdx.x % LPR, sub = threadIdx.x / LPR;
    const int q = blockIdx.x * LPR + lane;
    for (int i = threadIdx.x; i < (a.tau + 1) * LPR; i += 256) {
        const int j = i / LPR, qq = blockIdx.x * LPR + i % LPR;
        wl[i] = qq < CV ? reinterpret_cast<const V *>(w + (long long)j * C)[qq] : V{};
    }
    __syncthreads();
    if (q >= CV) return;
    const int dir = a.fwd ? 1 : -1;
    const long long hop = dir * (long long)a.B * ldx;                   // floats from one source row to the next
    const long long groups = (items + RPB - 1) / RPB;
    for (long long g = blockIdx.y; g < groups; g += gridDim.y) {
        const long long it = g * RPB + sub;
        if (it >= items) continue;
        const int seg = (int)(it / a.B), b = (int)(it - (long long)seg * a.B);
        const int len = rc_len(a, b);
        const int t0 = seg * ROWCONV_SEG, t1 = t0 + ROWCONV_SEG < a.T ? t0 + ROWCONV_SEG : a.T;
        const int n = t1 - t0;
        // Slot u is output frame tb + dir * u, source k is frame tb + dir * k: source k is term j = k - u of slot u, so one
        // walk over the sources k = 0 .. tau + n - 1, each row loaded ONCE, gives every slot its terms in ascending j.  Only
        // live sources are loaded: frames 0 <= s < len.  (A live slot's sources are then exactly the formula's: forward
        // t + j < len, backward t - j >= 0.)
        const int tb = a.fwd ? t0 : t1 - 1;
        const int klo = a.fwd ? 0 : (tb > len - 1 ? tb - (len - 1) : 0);
        const int kend = a.tau + n - 1, klast = a.fwd ? len - 1 - tb : tb;
        const int khi = kend < klast ? kend : klast;
        V s[ROWCONV_SEG];
#pragma unroll
        for (int u = 0; u < ROWCONV_SEG; ++u) s[u] = V{};
        const float *p = x + ((long long)(tb + dir * klo) * a.B + b) * ldx;
#pragma unroll 2
        for (int k = klo; k <= khi; ++k) {
            const V v = reinterpret_cast<const V *>(p)[q];
            p += hop;
#pragma unroll
            for (int u = 0; u < ROWCONV_SEG; ++u) {
                const int j = k - u;
                if (j == 0)
                    s[u] = rc_mul(wl[lane], v);                          // the first term initialises the sum
                else if (j > 0 && j <= a.tau)
                    s[u] = rc_fma(wl[j * LPR + lane], v, s[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < ROWCONV_SEG; ++u) {
            const int t = tb + dir * u;
            if (u < n) reinterpret_cast<V *>(out + ((long long)t * a.B + b) * ldo)[q] = t < len ? s[u] : V{};
        }
    }
}

// dw, stage one: workgroup (column group, row slab, group of ROWCONV_JT kernel rows) sums dy[t, b] * x[t + j, b] over the live
// pairs of its slab - 256 / LPR threads per column vector stride the slab's rows, LDS folds them in thread order - and writes
// part[slab][j][C].  Every element of part that stage two reads is written.
template <typename V, int LPR>
__global__ __launch_bounds__(256) void row_conv_dw_partial_kernel(const float *__restrict__ x, long long ldx,
                                                                  const float *__restrict__ dy, long long lddy, int C, int CV,
                                                                  long long rows, long long slab_rows, RowConvArgs a,
                                                                  float *__restrict__ part)
{
    constexpr int RPB = 256 / LPR;
    __shared__ V red[256];
    const int lane = threadIdx.x % LPR, sub = threadIdx.x / LPR;
    const int q = blockIdx.x * LPR + lane, j0 = blockIdx.z * ROWCONV_JT;
    const long long r_lo = blockIdx.y * slab_rows, r_hi = r_lo + slab_rows < rows ? r_lo + slab_rows : rows;
    V acc[ROWCONV_JT];
#pragma unroll
    for (int k = 0; k < ROWCONV_JT; ++k) acc[k] = V{};
    if (q < CV) {
        // two rows a turn: their lengths, then their dy, then their x rows are independent loads in flight together
        for (long long r0 = r_lo + sub; r0 < r_hi; r0 += 2 * RPB) {
            int n[2];                                                    // live kernel rows of this group per row (<= 0: none)
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const long long r = r0 + u * RPB;
                n[u] = 0;
                if (r < r_hi) {
                    const int t = (int)(r / a.B), b = (int)(r - (long long)t * a.B);
                    const int last = rc_len(a, b) - 1 - t;               // < 0: a dead row
                    n[u] = (a.tau < last ? a.tau : last) - j0 + 1;
                }
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                if (n[u] <= 0) continue;
                const long long r = r0 + u * RPB;
                const V d = reinterpret_cast<const V *>(dy + r * lddy)[q];
                const float *p = x + (r + (long long)j0 * a.B) * ldx;
#pragma unroll
                for (int k = 0; k < ROWCONV_JT; ++k) {
                    if (k < n[u]) acc[k] = rc_fma(d, reinterpret_cast<const V *>(p)[q], acc[k]);
                    p += (long long)a.B * ldx;
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < ROWCONV_JT; ++k) {
        red[threadIdx.x] = acc[k];
        __syncthreads();
        if (sub == 0 && q < CV && j0 + k <= a.tau) {
            V s = red[lane];
            for (int i = 1; i < RPB; ++i) s = rc_add(s, red[i * LPR + lane]);
            reinterpret_cast<V *>(part + ((long long)blockIdx.y * (a.tau + 1) + j0 + k) * C)[q] = s;
        }
        __syncthreads();
    }
}

// dw, stage two: the slabs in a fixed order (no float atomics: the same call gives the same bits).  A workgroup owns
// ROWCONV_FOLD_E elements; ROWCONV_FOLD_S threads per element take the slabs s, s + 16, ... with four independent sums (one
// thread adding all 512 slabs one load after the other took 130 us, whatever the shape), and LDS adds the 16 in thread order.
constexpr int ROWCONV_FOLD_E = 16, ROWCONV_FOLD_S = 16;
__global__ __launch_bounds__(256) void row_conv_dw_fold_kernel(const float *__restrict__ part, int nslab, long long n,
                                                               float *__restrict__ dw)
{
    __shared__ float red[ROWCONV_FOLD_S][ROWCONV_FOLD_E];
    const int e = threadIdx.x % ROWCONV_FOLD_E, sl = threadIdx.x / ROWCONV_FOLD_E;
    const long long i = (long long)blockIdx.x * ROWCONV_FOLD_E + e;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    if (i < n) {
        const float *p = part + i;
        int k = sl;
        for (; k + 3 * ROWCONV_FOLD_S < nslab; k += 4 * ROWCONV_FOLD_S) {
            s0 += p[(long long)k * n];
            s1 += p[(long long)(k + ROWCONV_FOLD_S) * n];
            s2 += p[(long long)(k + 2 * ROWCONV_FOLD_S) * n];
            s3 += p[(long long)(k + 3 * ROWCONV_FOLD_S) * n];
        }
        for (; k < nslab; k += ROWCONV_FOLD_S) s0 += p[(long long)k * n];
    }
    red[sl][e] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (sl == 0 && i < n) {
        float s = red[0][e];
        for (int m = 1; m < ROWCONV_FOLD_S; ++m) s += red[m][e];
        dw[i] = s;
    }
}

template <typename V>
void launch_rows(const float *x, int ldx, const float *w, int C, int CV, const RowConvArgs &a, float *out, int ldo, hipStream_t s)
{
    const int lpr = rs_lanes_cover(CV, 4, 64);
    const long long items = (long long)lc_cdiv(a.T, ROWCONV_SEG) * a.B;
    const dim3 grid((unsigned)lc_cdiv(CV, lpr), rs_grid(items, 256 / lpr)), block(256);
    rs_dispatch_lanes<4, 64>(lpr, [&](auto L) {
        hipLaunchKernelGGL((row_conv_rows_kernel<V, decltype(L)::value>), grid, block, 0, s, x, (long long)ldx, w, C, CV, items, a,
                           out, (long long)ldo);
    });
}

int rc_slabs(long long rows)
{
    const long long n = (rows + ROWCONV_SLAB_ROWS - 1) / ROWCONV_SLAB_ROWS;
    return (int)(n < 1 ? 1 : (n > ROWCONV_SLABS ? ROWCONV_SLABS : n));
}

template <typename V>
void launch_dw(const float *x, int ldx, const float *dy, int lddy, int C, int CV, const RowConvArgs &a, float *part, float *dw,
               hipStream_t s)
{
    const int lpr = rs_lanes_cover(CV, 4, 64);
    const long long rows = (long long)a.T * a.B;
    const long long slab_rows = (rows + rc_slabs(rows) - 1) / rc_slabs(rows);
    const int nslab = (int)((rows + slab_rows - 1) / slab_rows);        // no empty slab
    const dim3 grid((unsigned)lc_cdiv(CV, lpr), (unsigned)nslab, (unsigned)lc_cdiv(a.tau + 1, ROWCONV_JT)), block(256);
    rs_dispatch_lanes<4, 64>(lpr, [&](auto L) {
        hipLaunchKernelGGL((row_conv_dw_partial_kernel<V, decltype(L)::value>), grid, block, 0, s, x, (long long)ldx, dy,
                           (long long)lddy, C, CV, rows, slab_rows, a, part);
    });
    const long long n = (long long)(a.tau + 1) * C;
    hipLaunchKernelGGL(row_conv_dw_fold_kernel, dim3((unsigned)((n + ROWCONV_FOLD_E - 1) / ROWCONV_FOLD_E)), dim3(256), 0, s, part,
                       nslab, n, dw);
}

// Whether two [rows, C] windows with pitches lda / ldb share an element.  Two column windows of one buffer (equal pitches, the
// bases less than a pitch apart modulo it, C apart at least) interleave without touching.
bool rc_overlap(const float *a, long long lda, const float *b, long long ldb, long long rows, int C)
{
    if (!rs_overlap(a, lda, rows, C, b, ldb, rows, C)) return false;
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    if (lda == ldb && (a0 > b0 ? a0 - b0 : b0 - a0) % sizeof(float) == 0) {
        const uintptr_t lo = a0 < b0 ? a0 : b0, hi = a0 < b0 ? b0 : a0;
        const long long d = (long long)(((hi - lo) / sizeof(float)) % (uintptr_t)lda);
        if (d >= C && d + C <= lda) return false;
    }
    return true;
}

bool rc_shape_ok(int T, int B, int C, int tau) { return T > 0 && B > 0 && C > 0 && tau >= 0 && tau <= ROWCONV_MAX_TAU; }

}  // namespace

extern "C" size_t lc_row_conv_workspace_bytes(int T, int B, int C, int tau)
{
    if (!rc_shape_ok(T, B, C, tau)) return 0;
    return lc_align256((size_t)rc_slabs((long long)T * B) * (size_t)(tau + 1) * (size_t)C * sizeof(float));
}

extern "C" int lc_row_conv_fwd(const float *x, int ldx, const float *w, int T, int B, int C, int tau, const int *seq_len,
                               float *y, int ldy, lc_stream_t stream)
{
    LC_CHECK_ARG(rc_shape_ok(T, B, C, tau), "lc_row_conv_fwd: bad shape (T %d, B %d, C %d, tau %d; tau in 0..%d)", T, B, C, tau,
                 ROWCONV_MAX_TAU);
    LC_CHECK_ARG(x && w && seq_len && y, "lc_row_conv_fwd: null pointer");
    LC_CHECK_ARG(ldx >= C && ldy >= C, "lc_row_conv_fwd: a row pitch (%d, %d) below C %d", ldx, ldy, C);
    LC_CHECK_ARG(!rc_overlap(x, ldx, y, ldy, (long long)T * B, C), "lc_row_conv_fwd: x and y overlap");
    RowConvArgs a;
    a.T = T; a.B = B; a.tau = tau; a.fwd = 1; a.seq_len = seq_len;
    hipStream_t s = (hipStream_t)stream;
    if (rs_vec16(C, {ldx, ldy}, {x, w, y}))
        launch_rows<float4>(x, ldx, w, C, C / 4, a, y, ldy, s);
    else
        launch_rows<float>(x, ldx, w, C, C, a, y, ldy, s);
    LC_CHECK_LAUNCH("lc_row_conv_fwd");
    return LC_OK;
}

extern "C" int lc_row_conv_bwd(const float *x, int ldx, const float *dy, int lddy, const float *w, int T, int B, int C, int tau,
                               const int *seq_len, float *dx, int lddx, float *dw, void *workspace, size_t workspace_bytes,
                               lc_stream_t stream)
{
    LC_CHECK_ARG(rc_shape_ok(T, B, C, tau), "lc_row_conv_bwd: bad shape (T %d, B %d, C %d, tau %d; tau in 0..%d)", T, B, C, tau,
                 ROWCONV_MAX_TAU);
    LC_CHECK_ARG(dy && w && seq_len, "lc_row_conv_bwd: null pointer");
    LC_CHECK_ARG(dx || dw, "lc_row_conv_bwd: dx and dw are both NULL");
    LC_CHECK_ARG(!dw || x, "lc_row_conv_bwd: dw needs x");
    LC_CHECK_ARG(lddy >= C && (!dx || lddx >= C) && (!dw || ldx >= C), "lc_row_conv_bwd: a row pitch (%d, %d, %d) below C %d",
                 ldx, lddy, lddx, C);
    LC_CHECK_ARG(!dx || !rc_overlap(dy, lddy, dx, lddx, (long long)T * B, C), "lc_row_conv_bwd: dy and dx overlap");
    const size_t need = lc_row_conv_workspace_bytes(T, B, C, tau);
    if (dw && (!workspace || workspace_bytes < need)) {
        lc_set_error("lc_row_conv_bwd: workspace of %zu bytes needed (%zu given)", need, workspace ? workspace_bytes : (size_t)0);
        return LC_EWORKSPACE;
    }
    RowConvArgs a;
    a.T = T; a.B = B; a.tau = tau; a.fwd = 0; a.seq_len = seq_len;
    hipStream_t s = (hipStream_t)stream;
    if (dx) {
        if (rs_vec16(C, {lddy, lddx}, {dy, w, dx}))
            launch_rows<float4>(dy, lddy, w, C, C / 4, a, dx, lddx, s);
        else
            launch_rows<float>(dy, lddy, w, C, C, a, dx, lddx, s);
    }
    if (dw) {
        if (rs_vec16(C, {ldx, lddy}, {x, dy, workspace}))
            launch_dw<float4>(x, ldx, dy, lddy, C, C / 4, a, (float *)workspace, dw, s);
        else
            launch_dw<float>(x, ldx, dy, lddy, C, C, a, (float *)workspace, dw, s);
    }
    LC_CHECK_LAUNCH("lc_row_conv_bwd");
    return LC_OK;
}
