// time_reduce.hip - the layout passes of the pyramidal BiLSTM (lc_time_reduce_fwd / lc_time_reduce_bwd, include/lstm_ctc_hip.h):
// r consecutive frames of a layer's output [T, B, C] side by side as one frame of the next layer's input [ceil(T / r), B, r * C],
// and the way back for the gradient.  Pure HBM streams with chunk.hip's skeleton: no arithmetic, no LDS, no atomics.
#include "common.h"

namespace {

enum { TR_FWD = 0, TR_BWD = 1 };
enum { TR_MAX_GROUPS = 2048 };        // workgroups per launch (8 per CU), the rest by grid stride

// One C-wide segment per (frame t, utterance b): the narrow side holds it as row t * B + b of [.., C], the wide side as columns
// [(t % r) * C, (t % r + 1) * C) of row (t / r) * B + b of [.., r * C].  fwd copies narrow -> wide for t < ceil(T / r) * r (the
// frames past T are the cut-short last group: dead for every utterance), bwd wide -> narrow for t < T.  A segment is live iff
// t < clamp(seq_len[b], 0, T); a dead one is written +0 and its source is never read.
// LPR lanes walk one segment, 256 / LPR segments per workgroup pass.  V = float4: 16-byte accesses; V = float: any C and pitch.
template <typename V, int LPR, int MODE>
__global__ __launch_bounds__(256) void time_reduce_kernel(const float *__restrict__ in, long long ldi, long long nseg, int CV, int C,
                                                          int T, int B, int r, const int *__restrict__ seq_len,
                                                          float *__restrict__ out, long long ldo)
{
    constexpr int SPB = 256 / LPR;
    const int lane = threadIdx.x % LPR, sub = threadIdx.x / LPR;
    const long long groups = (nseg + SPB - 1) / SPB;
    for (long long g = blockIdx.x; g < groups; g += gridDim.x) {
        const long long s = g * SPB + sub;
        if (s >= nseg) continue;
        // fwd walks the wide side in storage order (to, b, j), bwd the narrow side (t, b): stores of a workgroup are contiguous
        // (32-bit divisions where the segment count allows them were measured at c2's shape: no difference)
        long long t, wide_row;
        int b, j;
        if constexpr (MODE == TR_FWD) {
            wide_row = s / r;
            j = (int)(s - wide_row * r);
            const long long to = wide_row / B;
            b = (int)(wide_row - to * B);
            t = to * r + j;
        } else {
            t = s / B;
            b = (int)(s - t * B);
            const long long to = t / r;
            j = (int)(t - to * r);
            wide_row = to * B + b;
        }
        const long long narrow = (t * B + b), wide_off = (long long)j * C;
        int len = seq_len[b];
        len = len < 0 ? 0 : (len > T ? T : len);
        V *dst = reinterpret_cast<V *>(MODE == TR_FWD ? out + wide_row * ldo + wide_off : out + narrow * ldo);
        if (t >= len) {
            for (int q = lane; q < CV; q += LPR) dst[q] = V{};
            continue;
        }
        const V *from = reinterpret_cast<const V *>(MODE == TR_FWD ? in + narrow * ldi : in + wide_row * ldi + wide_off);
        int q = lane;
        for (; q + 3 * LPR < CV; q += 4 * LPR) {              // four loads in flight per lane before the first store
            const V v0 = from[q], v1 = from[q + LPR], v2 = from[q + 2 * LPR], v3 = from[q + 3 * LPR];
            dst[q] = v0; dst[q + LPR] = v1; dst[q + 2 * LPR] = v2; dst[q + 3 * LPR] = v3;
        }
        for (; q < CV; q += LPR) dst[q] = from[q];
    }
}

template <typename V, int MODE>
void launch_time_reduce(const float *in, int ldi, long long nseg, int CV, int C, int T, int B, int r, const int *seq_len, float *out,
                        int ldo, hipStream_t s)
{
    // lanes per segment: the power of two in 4 .. 256 that leaves the fewest lanes idle over the segment's passes (the widest
    // such, at most 8 passes per lane) - c2's 160 vectors take 32 lanes five times, not 256 lanes once with 96 of them idle
    int lpr = 256;
    long long idle = -1;
    for (int l = 256; l >= 4; l /= 2) {
        const int passes = (CV + l - 1) / l;
        if (passes > 8 && l < 256) break;
        const long long w = (long long)passes * l - CV;
        if (idle < 0 || w < idle) { idle = w; lpr = l; }
    }
    const long long groups = (nseg + 256 / lpr - 1) / (256 / lpr);
    const dim3 grid((unsigned)(groups < TR_MAX_GROUPS ? groups : TR_MAX_GROUPS)), block(256);
#define LC_TR(L) hipLaunchKernelGGL((time_reduce_kernel<V, L, MODE>), grid, block, 0, s, in, (long long)ldi, nseg, CV, C, T, B, r, \
                                    seq_len, out, (long long)ldo)
    switch (lpr) {
    case 4: LC_TR(4); break;
    case 8: LC_TR(8); break;
    case 16: LC_TR(16); break;
    case 32: LC_TR(32); break;
    case 64: LC_TR(64); break;
    case 128: LC_TR(128); break;
    default: LC_TR(256); break;
    }
#undef LC_TR
}

// Whether the byte ranges of an [rows_a, Ca] window at pitch lda and an [rows_b, Cb] window at pitch ldb intersect.
bool tr_overlap(const float *a, long long lda, long long rows_a, long long Ca, const float *b, long long ldb, long long rows_b,
                long long Cb)
{
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + ((rows_a - 1) * lda + Ca) * sizeof(float);
    const uintptr_t b0 = (uintptr_t)b, b1 = b0 + ((rows_b - 1) * ldb + Cb) * sizeof(float);
    return !(a1 <= b0 || b1 <= a0);
}

// narrow: the [T * B, C] side, wide: the [ceil(T / r) * B, r * C] side; MODE says which of them is written.
template <int MODE>
int time_reduce(const char *who, const float *narrow, int ldn, const float *wide, int ldw, int T, int B, int C, int r,
                const int *seq_len, lc_stream_t stream)
{
    LC_CHECK_ARG(T > 0 && B > 0 && C > 0 && r >= 2 && r <= 4, "%s: bad shape (T %d, B %d, C %d, r %d; r in 2..4)", who, T, B, C, r);
    LC_CHECK_ARG(narrow && wide && seq_len, "%s: null pointer", who);
    LC_CHECK_ARG(ldn >= C && (long long)ldw >= (long long)r * C, "%s: a row pitch (%d, %d) below C %d / r * C %lld", who, ldn, ldw, C,
                 (long long)r * C);
    const long long To = ((long long)T + r - 1) / r;
    LC_CHECK_ARG(!tr_overlap(narrow, ldn, (long long)T * B, C, wide, ldw, To * B, (long long)r * C), "%s: input and output overlap",
                 who);
    const long long nseg = MODE == TR_FWD ? To * B * r : (long long)T * B;
    const float *in = MODE == TR_FWD ? narrow : wide;
    float *out = const_cast<float *>(MODE == TR_FWD ? wide : narrow);
    const int ldi = MODE == TR_FWD ? ldn : ldw, ldo = MODE == TR_FWD ? ldw : ldn;
    hipStream_t s = (hipStream_t)stream;
    if (C % 4 == 0 && ldn % 4 == 0 && ldw % 4 == 0 && (((uintptr_t)narrow | (uintptr_t)wide) & 15) == 0)
        launch_time_reduce<float4, MODE>(in, ldi, nseg, C / 4, C, T, B, r, seq_len, out, ldo, s);
    else
        launch_time_reduce<float, MODE>(in, ldi, nseg, C, C, T, B, r, seq_len, out, ldo, s);
    LC_CHECK_LAUNCH(who);
    return LC_OK;
}

}  // namespace

extern "C" int lc_time_reduce_fwd(const float *x, int ldx, int T, int B, int C, int r, const int *seq_len, float *y, int ldy,
                                  lc_stream_t stream)
{
    return time_reduce<TR_FWD>("lc_time_reduce_fwd", x, ldx, y, ldy, T, B, C, r, seq_len, stream);
}

extern "C" int lc_time_reduce_bwd(const float *dy, int lddy, int T, int B, int C, int r, const int *seq_len, float *dx, int lddx,
                                  lc_stream_t stream)
{
    return time_reduce<TR_BWD>("lc_time_reduce_bwd", dx, lddx, dy, lddy, T, B, C, r, seq_len, stream);
}
