// time_reduce.hip - the layout passes of the pyramidal BiLSTM (lc_time_reduce_fwd / lc_time_reduce_bwd, include/lstm_ctc_hip.h):
// r consecutive frames of a layer's output [T, B, C] side by side as one frame of the next layer's input [ceil(T / r), B, r * C],
// and the way back for the gradient.  Pure HBM streams on row_stream.h's skeleton: no arithmetic, no LDS, no atomics.
#include "row_stream.h"

namespace {

enum { TR_FWD = 0, TR_BWD = 1 };

// The row map (row_stream.h).  One C-wide segment per (frame t, utterance b): the narrow side holds it as row t * B + b of
// [.., C], the wide side as columns [(t % r) * C, (t % r + 1) * C) of row (t / r) * B + b of [.., r * C].  fwd copies narrow ->
// wide for t < ceil(T / r) * r (the frames past T are the cut-short last group: dead for every utterance), bwd wide -> narrow
// for t < T.  A segment is live iff t < clamp(seq_len[b], 0, T); a dead one is written +0 and its source is never read.
template <int MODE> struct TimeReduceMap {
    static constexpr bool SUMS = false;
    int C, T, B, r;
    const int *seq_len;

    template <int LPR> __device__ __forceinline__ RsSpan locate(long long s, long long ldi, long long ldo) const
    {
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
        const int n = t >= len ? 0 : 1;
        if constexpr (MODE == TR_FWD) return {wide_row * ldo + wide_off, narrow * ldi, 0, n};
        else return {narrow * ldo, wide_row * ldi + wide_off, 0, n};
    }
};

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
    LC_CHECK_ARG(!rs_overlap(narrow, ldn, (long long)T * B, C, wide, ldw, To * B, (long long)r * C), "%s: input and output overlap",
                 who);
    const long long nseg = MODE == TR_FWD ? To * B * r : (long long)T * B;
    const float *in = MODE == TR_FWD ? narrow : wide;
    float *out = const_cast<float *>(MODE == TR_FWD ? wide : narrow);
    const int ldi = MODE == TR_FWD ? ldn : ldw, ldo = MODE == TR_FWD ? ldw : ldn;
    // lanes per segment: the fewest idle over its passes - c2's 160 vectors take 32 lanes five times
    rs_launch_map(in, ldi, out, ldo, nseg, C, rs_lanes_fewest_idle, TimeReduceMap<MODE>{C, T, B, r, seq_len}, (hipStream_t)stream);
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
