// chunk.hip - the layout passes of the latency-controlled BiLSTM (lc_chunk_gather / lc_chunk_fold, include/lstm_ctc_hip.h):
// the padded time-major [T, B, C] batch against its chunked form [Tc, Bc, C], Bc = nC * B, chunk row c * B + b, whose rows
// the reverse recurrences of lc_lstm_fwd / lc_lstm_bwd walk from a zero state.  Pure HBM streams: no arithmetic but the
// ordered sum of a frame's chunk copies.
#include "row_stream.h"

namespace {

enum { CHUNK_GATHER = 0, CHUNK_FOLD = 1 };

// The row map (row_stream.h) of output row r: its n source rows, the first at row `src`, each next one `step` rows further.
//   gather  r = tau * Bc + c * B + b  <-  padded row (c * chunk + tau) * B + b, if that frame exists and is wanted
//   fold    r = t * B + b             <-  chunk rows (t - c * chunk) * Bc + c * B + b over c ascending: the frame's own chunk
//                                          c = t / chunk alone, or (sum_copies) every chunk whose window holds t
template <int MODE> struct ChunkMap {
    static constexpr bool SUMS = MODE == CHUNK_FOLD;
    int T, B, chunk, Tc, nC;
    long long Bc;
    int zero_lookahead, sum_copies;
    const int *seq_len;

    template <int LPR> __device__ __forceinline__ RsSpan locate(long long r, long long ldx, long long ldo) const
    {
        long long src, step;
        int n;
        if constexpr (MODE == CHUNK_GATHER) {
            const int tau = (int)(r / Bc), rc = (int)(r - tau * Bc), c = rc / B, b = rc - c * B;
            const long long t = (long long)c * chunk + tau;
            n = (t < T && !(zero_lookahead && tau >= chunk)) ? 1 : 0;
            src = t * B + b;
            step = 0;
        } else {
            const int t = (int)(r / B), b = (int)(r - (long long)t * B), c_own = t / chunk;
            // the first chunk whose window [c * chunk, c * chunk + Tc) still holds t
            int c_lo = c_own;
            if (sum_copies) c_lo = t < Tc ? 0 : (t - Tc) / chunk + 1;
            // a copy at tau = t - c * chunk is live in its chunk row iff tau < clamp(seq_len[b] - c * chunk, 0, Tc), and with
            // tau < Tc that is t < seq_len[b]: all copies of a frame are live or dead together
            n = (seq_len != nullptr && t >= seq_len[b]) ? 0 : c_own - c_lo + 1;
            src = (long long)(t - (long long)c_lo * chunk) * Bc + (long long)c_lo * B + b;
            step = (long long)B - (long long)chunk * Bc;
        }
        return {r * ldo, src * ldx, step * ldx, n};
    }
};

template <int MODE>
int chunk_rows(const char *who, const float *x, int ldx, int T, int B, int C, int chunk, int lookahead, int zero_lookahead,
               int sum_copies, const int *seq_len, float *out, int ldo, lc_stream_t stream)
{
    LC_CHECK_ARG(x && out, "%s: null pointer", who);
    LC_CHECK_ARG(T > 0 && B > 0 && C > 0 && chunk > 0 && lookahead >= 0, "%s: bad shape (T %d, B %d, C %d, chunk %d, lookahead %d)",
                 who, T, B, C, chunk, lookahead);
    LC_CHECK_ARG(ldx >= C && ldo >= C, "%s: a row pitch (%d, %d) below C %d", who, ldx, ldo, C);
    ChunkMap<MODE> a;
    a.T = T; a.B = B; a.chunk = chunk;
    a.Tc = (long long)chunk + lookahead < T ? chunk + lookahead : T;
    a.nC = lc_cdiv(T, chunk);
    a.Bc = (long long)a.nC * B;
    a.zero_lookahead = zero_lookahead != 0; a.sum_copies = sum_copies != 0;
    a.seq_len = seq_len;
    const long long nrows = MODE == CHUNK_GATHER ? (long long)a.Tc * a.Bc : (long long)T * B;
    // lanes per row: the power of two that covers the row's vectors
    rs_launch_map(x, ldx, out, ldo, nrows, C, rs_lanes_cover, a, (hipStream_t)stream);
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
