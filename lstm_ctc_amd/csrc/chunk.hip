// chunk.hip - the layout passes of the latency-controlled BiLSTM (lc_chunk_gather / lc_chunk_fold, include/lstm_ctc_hip.h):
// the padded time-major [T, B, C] batch against its chunked form [Tc, Bc, C], Bc = nC * B, chunk row c * B + b, whose rows
// the reverse recurrences of lc_lstm_fwd / lc_lstm_bwd walk from a zero state.  Pure HBM streams: no arithmetic but the
// ordered sum of a frame's chunk copies.
#include "common.h"

namespace {

enum { CHUNK_GATHER = 0, CHUNK_FOLD = 1 };

struct ChunkArgs {
    int T, B, chunk, Tc, nC;
    long long Bc;
    int zero_lookahead, sum_copies;
    const int *seq_len;
};

// The source rows of output row r: n of them, the first at `src`, each next one `step` rows further (n = 0: the row is +0).
//   gather  r = tau * Bc + c * B + b  <-  padded row (c * chunk + tau) * B + b, if that frame exists and is wanted
//   fold    r = t * B + b             <-  chunk rows (t - c * chunk) * Bc + c * B + b over c ascending: the frame's own chunk
//                                          c = t / chunk alone, or (sum_copies) every chunk whose window holds t
template <int MODE>
__device__ __forceinline__ void chunk_sources(const ChunkArgs &a, long long r, long long &src, int &n, long long &step)
{
    if constexpr (MODE == CHUNK_GATHER) {
        const int tau = (int)(r / a.Bc), rc = (int)(r - tau * a.Bc), c = rc / a.B, b = rc - c * a.B;
        const long long t = (long long)c * a.chunk + tau;
        n = (t < a.T && !(a.zero_lookahead && tau >= a.chunk)) ? 1 : 0;
        src = t * a.B + b;
        step = 0;
    } else {
        const int t = (int)(r / a.B), b = (int)(r - (long long)t * a.B), c_own = t / a.chunk;
        // the first chunk whose window [c * chunk, c * chunk + Tc) still holds t
        int c_lo = c_own;
        if (a.sum_copies) c_lo = t < a.Tc ? 0 : (t - a.Tc) / a.chunk + 1;
        // a copy at tau = t - c * chunk is live in its chunk row iff tau < clamp(seq_len[b] - c * chunk, 0, Tc), and with
        // tau < Tc that is t < seq_len[b]: all copies of a frame are live or dead together
        n = (a.seq_len != nullptr && t >= a.seq_len[b]) ? 0 : c_own - c_lo + 1;
        src = (long long)(t - (long long)c_lo * a.chunk) * a.Bc + (long long)c_lo * a.B + b;
        step = (long long)a.B - (long long)a.chunk * a.Bc;
    }
}

__device__ __forceinline__ void chunk_add(float &s, const float v) { s += v; }
__device__ __forceinline__ void chunk_add(float4 &s, const float4 v) { s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w; }

// LPR lanes walk one output row, 256 / LPR rows per workgroup pass, workgroups walk the row groups with a grid stride.  Every
// output row is written exactly once.  V = float4: 16-byte accesses; V = float: any C and pitch.
template <typename V, int LPR, int MODE>
__global__ __launch_bounds__(256) void chunk_rows_kernel(const float *__restrict__ x, long long ldx, long long nrows, int CV,
                                                         ChunkArgs a, float *__restrict__ out, long long ldo)
{
    constexpr int RPB = 256 / LPR;
    const int lane = threadIdx.x % LPR, sub = threadIdx.x / LPR;
    const long long groups = (nrows + RPB - 1) / RPB;
    for (long long g = blockIdx.x; g < groups; g += gridDim.x) {
        const long long r = g * RPB + sub;
        if (r >= nrows) continue;
        long long src, step;
        int n;
        chunk_sources<MODE>(a, r, src, n, step);
        V *dst = reinterpret_cast<V *>(out + r * ldo);
        if (n == 0) {
            for (int q = lane; q < CV; q += LPR) dst[q] = V{};
            continue;
        }
        const V *from = reinterpret_cast<const V *>(x + src * ldx);
        if (n == 1) {
            int q = lane;
            for (; q + 3 * LPR < CV; q += 4 * LPR) {          // four loads in flight per lane before the first store
                const V v0 = from[q], v1 = from[q + LPR], v2 = from[q + 2 * LPR], v3 = from[q + 3 * LPR];
                dst[q] = v0; dst[q + LPR] = v1; dst[q + 2 * LPR] = v2; dst[q + 3 * LPR] = v3;
            }
            for (; q < CV; q += LPR) dst[q] = from[q];
            continue;
        }
        if constexpr (MODE == CHUNK_FOLD) {
            // the frame's copies in ascending chunk order; the first one initialises the sum (no 0 + ...)
            const long long hop = step * ldx;                // floats between two copies of this row
            for (int q = lane; q < CV; q += LPR) {
                const float *p = x + src * ldx;
                V s = reinterpret_cast<const V *>(p)[q];
                for (int k = 1; k < n; ++k) {
                    p += hop;
                    chunk_add(s, reinterpret_cast<const V *>(p)[q]);
                }
                dst[q] = s;
            }
        }
    }
}

template <typename V, int MODE>
void launch_chunk_rows(const float *x, int ldx, long long nrows, int CV, const ChunkArgs &a, float *out, int ldo, hipStream_t s)
{
    // lanes per row: the power of two that covers the row's vectors, 4 .. 256; at most 2048 workgroups (8 per CU), the
    // rest by grid stride
    int lpr = 4;
    while (lpr < 256 && lpr < CV) lpr *= 2;
    const long long groups = (nrows + 256 / lpr - 1) / (256 / lpr);
    const dim3 grid((unsigned)(groups < 2048 ? groups : 2048)), block(256);
#define LC_CHUNK(L) hipLaunchKernelGGL((chunk_rows_kernel<V, L, MODE>), grid, block, 0, s, x, (long long)ldx, nrows, CV, a, out, (long long)ldo)
    switch (lpr) {
    case 4: LC_CHUNK(4); break;
    case 8: LC_CHUNK(8); break;
    case 16: LC_CHUNK(16); break;
    case 32: LC_CHUNK(32); break;
    case 64: LC_CHUNK(64); break;
    case 128: LC_CHUNK(128); break;
    default: LC_CHUNK(256); break;
    }
#undef LC_CHUNK
}

template <int MODE>
int chunk_rows(const char *who, const float *x, int ldx, int T, int B, int C, int chunk, int lookahead, int zero_lookahead,
               int sum_copies, const int *seq_len, float *out, int ldo, lc_stream_t stream)
{
    LC_CHECK_ARG(x && out, "%s: null pointer", who);
    LC_CHECK_ARG(T > 0 && B > 0 && C > 0 && chunk > 0 && lookahead >= 0, "%s: bad shape (T %d, B %d, C %d, chunk %d, lookahead %d)",
                 who, T, B, C, chunk, lookahead);
    LC_CHECK_ARG(ldx >= C && ldo >= C, "%s: a row pitch (%d, %d) below C %d", who, ldx, ldo, C);
    ChunkArgs a;
    a.T = T; a.B = B; a.chunk = chunk;
    a.Tc = (long long)chunk + lookahead < T ? chunk + lookahead : T;
    a.nC = lc_cdiv(T, chunk);
    a.Bc = (long long)a.nC * B;
    a.zero_lookahead = zero_lookahead != 0; a.sum_copies = sum_copies != 0;
    a.seq_len = seq_len;
    const long long nrows = MODE == CHUNK_GATHER ? (long long)a.Tc * a.Bc : (long long)T * B;
    hipStream_t s = (hipStream_t)stream;
    if (C % 4 == 0 && ldx % 4 == 0 && ldo % 4 == 0 && (((uintptr_t)x | (uintptr_t)out) & 15) == 0)
        launch_chunk_rows<float4, MODE>(x, ldx, nrows, C / 4, a, out, ldo, s);
    else
        launch_chunk_rows<float, MODE>(x, ldx, nrows, C, a, out, ldo, s);
    LC_CHECK_LAUNCH(who);
    return LC_OK;
}

}  // namespace

extern "C" int lc_chunk_gather(const float *x, int ldx, int T, int B, int C, int chunk, int lookahead, int zero_lookahead,
                               float *out, int ldo, lc_stream_t stream)
{
    return chunk_rows<CHUNK_GATHER>("lc_chunk_gather", x, ldx, T, B, C, chunk, lookahead, zero_lookahead, 0, nullptr, out, ldo,
                                    stream);
}

extern "C" int lc_chunk_fold(const float *xc, int ldc, int T, int B, int C, int chunk, int lookahead, int sum_copies,
                             const int *seq_len, float *out, int ldo, lc_stream_t stream)
{
    return chunk_rows<CHUNK_FOLD>("lc_chunk_fold", xc, ldc, T, B, C, chunk, lookahead, 0, sum_copies, seq_len, out, ldo, stream);
}
