// conv.hip - the 2-D convolutional front-end between the features and the first LSTM layer (lc_conv_fwd / lc_conv_bwd,
// include/lstm_ctc_hip.h): one 3 (time) x 3 (frequency) layer per call, time stride 1, frequency stride 2, zero
// padding 1, bias and ReLU fused, dead frames +0 and never read.  Three direct convolutions on plain FMAs (K is 9 .. 576 and N is
// 8 .. 64: too small for the tuned GEMMs), each over LDS tiles: a workgroup stages a time segment of one or a few utterances -
// its input rows with one halo row on each side, so a row is fetched once per segment, not once per tap - and a chunk of
// CONV_KC input channels of the weights, and every thread keeps a small register tile (4 channels x the segment's frames).
// No atomics: the weight gradient goes through per-workgroup partials in the workspace, folded in a fixed order.
#include "row_stream.h"

namespace {

enum { CONV_TS = 8 };            // frames per segment of the forward pass (32 accumulators per thread)
enum { CONV_TSB = 4 };           // frames per segment of the input gradient (2 bins x 4 channels x 4 frames per thread)
enum { CONV_KC = 8 };            // channels of the reduction staged in LDS at a time
enum { CONV_MAX_POS = 64 };      // output positions (utterance, bin) of a workgroup tile
enum { CONV_MAX_NB = 8 };        // utterances side by side in a tile, when the bins alone do not fill it
enum { CONV_MAX_GROUPS = 1024 }; // workgroups per launch of the forward pass and of the input gradient, the rest by grid stride
enum { CONV_DW_GROUPS = 1024 };  // workgroups of the weight gradient: partials per weight x chunks of input channels
enum { CONV_DW_MIN_PARTS = 128 };
enum { CONV_DW_TS = 8, CONV_DW_FT = 16 };      // its tile: frames x output bins
enum { CONV_MAX_C = 64, CONV_MAX_F = 512 };

// How a pass cuts its output into workgroup tiles: segments of `ts` frames x groups of NB utterances x tiles of FT positions
// along the frequency axis.  CG threads (4 channels each) stand on one position.
struct ConvTiles {
    int CG, FT, NB, nseg, nbg, nft;
    long long items;
};

ConvTiles conv_tiles(int T, int B, int npos_axis, int channels, int ts)
{
    ConvTiles g;
    g.CG = (channels + 3) / 4;
    const int npos = 256 / g.CG < CONV_MAX_POS ? 256 / g.CG : CONV_MAX_POS;
    g.FT = npos_axis < npos ? npos_axis : npos;
    g.NB = npos / g.FT < 1 ? 1 : (npos / g.FT > CONV_MAX_NB ? CONV_MAX_NB : npos / g.FT);
    if (g.NB > B) g.NB = B;
    g.nseg = lc_cdiv(T, ts);
    g.nbg = lc_cdiv(B, g.NB);
    g.nft = lc_cdiv(npos_axis, g.FT);
    g.items = (long long)g.nseg * g.nbg * g.nft;
    return g;
}

__device__ __forceinline__ int conv_len(const int *seq_len, int b, int B, int T)
{
    if (b >= B) return 0;
    const int len = seq_len[b];
    return len < 0 ? 0 : (len > T ? T : len);
}

// column of (bin f, channel ci) in a row of x / dx
__device__ __forceinline__ int conv_xcol(int gm, int f, int ci, int F, int Cin) { return gm ? ci * F + f : f * Cin + ci; }

// ---------------------------------------------------------------------------------------------------------------- forward
// LDS: lens[CONV_MAX_NB] | xs[CONV_TS + 2][NB][CONV_KC][NBINS] | ws[9][CONV_KC][Cout], NBINS = 2 FT + 1 (odd: the channel-minor
// fill walks it at that stride).  Thread (cg, pos): 4 output channels of one (utterance, bin) over the segment's frames.
template <bool VEC>
__global__ __launch_bounds__(256) void conv_fwd_kernel(const float *__restrict__ x, long long ldx, int gm, const float *__restrict__ w,
                                                       const float *__restrict__ bias, int T, int B, int F, int Fo, int Cin, int Cout,
                                                       const int *__restrict__ seq_len, float *__restrict__ y, long long ldy,
                                                       ConvTiles g, int xs_floats)
{
    extern __shared__ float sm[];
    int *lens = reinterpret_cast<int *>(sm);
    float *xs = sm + CONV_MAX_NB, *ws = xs + xs_floats;
    const int tid = threadIdx.x, NB = g.NB, FT = g.FT, NBINS = 2 * FT + 1;
    const int cg = tid % g.CG, pos = tid / g.CG, bb = pos / FT, fl = pos - bb * FT;
    const bool mine = pos < NB * FT && 4 * cg < Cout;
    for (long long item = blockIdx.x; item < g.items; item += gridDim.x) {
        const int ft = (int)(item % g.nft), bg = (int)((item / g.nft) % g.nbg), seg = (int)(item / ((long long)g.nft * g.nbg));
        const int t0 = seg * CONV_TS, b0 = bg * NB, fo0 = ft * FT;
        __syncthreads();
        if (tid < NB) lens[tid] = conv_len(seq_len, b0 + tid, B, T);
        __syncthreads();
        int maxlen = 0;
        for (int k = 0; k < NB; ++k) maxlen = lens[k] > maxlen ? lens[k] : maxlen;
        float acc[CONV_TS][4];
#pragma unroll
        for (int tt = 0; tt < CONV_TS; ++tt) acc[tt][0] = acc[tt][1] = acc[tt][2] = acc[tt][3] = 0.f;
        if (maxlen > t0) {
            for (int c0 = 0; c0 < Cin; c0 += CONV_KC) {
                const int kc = Cin - c0 < CONV_KC ? Cin - c0 : CONV_KC;
                __syncthreads();
                // the input rows t0 - 1 .. t0 + CONV_TS of the tile's utterances, bins 2 fo0 - 1 .. 2 (fo0 + FT) - 1, kc channels;
                // what is dead, padded or out of range is a 0 that is never read from memory
                const int per_row = NB * kc * NBINS, total = (CONV_TS + 2) * per_row;
                for (int e = tid; e < total; e += 256) {
                    const int row = e / per_row, r1 = e - row * per_row, ub = r1 / (kc * NBINS), r2 = r1 - ub * kc * NBINS;
                    int cl, bin;
                    if (gm) { cl = r2 / NBINS; bin = r2 - cl * NBINS; } else { bin = r2 / kc; cl = r2 - bin * kc; }
                    const int t = t0 - 1 + row, f = 2 * fo0 - 1 + bin;
                    float v = 0.f;
                    if (t >= 0 && t < lens[ub] && f >= 0 && f < F)
                        v = x[((long long)t * B + (b0 + ub)) * ldx + conv_xcol(gm, f, c0 + cl, F, Cin)];
                    xs[((row * NB + ub) * CONV_KC + cl) * NBINS + bin] = v;
                }
                for (int e = tid; e < 9 * kc * Cout; e += 256) {
                    const int tap = e / (kc * Cout), r1 = e - tap * kc * Cout;       // r1 = cl * Cout + co
                    ws[tap * CONV_KC * Cout + r1] = w[((long long)tap * Cin + c0) * Cout + r1];
                }
                __syncthreads();
                if (mine) {
                    for (int cl = 0; cl < kc; ++cl) {
#pragma unroll
                        for (int j = 0; j < 3; ++j) {
                            float xv[CONV_TS + 2];
#pragma unroll
                            for (int r = 0; r < CONV_TS + 2; ++r) xv[r] = xs[((r * NB + bb) * CONV_KC + cl) * NBINS + 2 * fl + j];
#pragma unroll
                            for (int i = 0; i < 3; ++i) {
                                const float4 wv = *reinterpret_cast<const float4 *>(ws + ((i * 3 + j) * CONV_KC + cl) * Cout + 4 * cg);
#pragma unroll
                                for (int tt = 0; tt < CONV_TS; ++tt) {
                                    acc[tt][0] = __fmaf_rn(xv[tt + i], wv.x, acc[tt][0]);
                                    acc[tt][1] = __fmaf_rn(xv[tt + i], wv.y, acc[tt][1]);
                                    acc[tt][2] = __fmaf_rn(xv[tt + i], wv.z, acc[tt][2]);
                                    acc[tt][3] = __fmaf_rn(xv[tt + i], wv.w, acc[tt][3]);
                                }
                            }
                        }
                    }
                }
            }
        }
        const int b = b0 + bb, fo = fo0 + fl;
        if (mine && b < B && fo < Fo) {
            const int len = lens[bb];
            float bv[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) bv[k] = bias[4 * cg + k];
#pragma unroll
            for (int tt = 0; tt < CONV_TS; ++tt) {
                const int t = t0 + tt;
                if (t >= T) break;
                float o[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float v = acc[tt][k] + bv[k];
                    o[k] = t < len && v > 0.f ? v : 0.f;
                }
                float *dst = y + ((long long)t * B + b) * ldy + (long long)fo * Cout + 4 * cg;
                if (VEC) {
                    *reinterpret_cast<float4 *>(dst) = make_float4(o[0], o[1], o[2], o[3]);
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) dst[k] = o[k];
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------- input gradient
// The transposed convolution as a gather: position m stands for the bins 2m (tap j = 1 of output bin m) and 2m + 1 (tap j = 2 of
// output bin m, tap j = 0 of output bin m + 1).  LDS: lens | gs[CONV_TSB + 2][NB][CONV_KC][NBG] | ws[9][CONV_KC][CI4], g = dy where
// y > 0, the weights with the input channel contiguous.  Thread (cg, pos): 4 input channels of both bins over the segment.
template <bool VEC>
__global__ __launch_bounds__(256) void conv_dx_kernel(const float *__restrict__ y, long long ldy, const float *__restrict__ dy,
                                                      long long lddy, const float *__restrict__ w, int gm, int T, int B, int F, int Fo,
                                                      int Cin, int Cout, const int *__restrict__ seq_len, float *__restrict__ dx,
                                                      long long lddx, ConvTiles g, int NBG, int gs_floats)
{
    extern __shared__ float sm[];
    int *lens = reinterpret_cast<int *>(sm);
    float *gs = sm + CONV_MAX_NB, *ws = gs + gs_floats;
    const int tid = threadIdx.x, NB = g.NB, FT = g.FT, CI4 = 4 * g.CG;
    const int cg = tid % g.CG, pos = tid / g.CG, bb = pos / FT, ml = pos - bb * FT;
    const bool mine = pos < NB * FT;
    for (long long item = blockIdx.x; item < g.items; item += gridDim.x) {
        const int ft = (int)(item % g.nft), bg = (int)((item / g.nft) % g.nbg), seg = (int)(item / ((long long)g.nft * g.nbg));
        const int t0 = seg * CONV_TSB, b0 = bg * NB, m0 = ft * FT;
        __syncthreads();
        if (tid < NB) lens[tid] = conv_len(seq_len, b0 + tid, B, T);
        __syncthreads();
        int maxlen = 0;
        for (int k = 0; k < NB; ++k) maxlen = lens[k] > maxlen ? lens[k] : maxlen;
        float ae[CONV_TSB][4], ao[CONV_TSB][4];          // bins 2m and 2m + 1
#pragma unroll
        for (int tt = 0; tt < CONV_TSB; ++tt)
#pragma unroll
            for (int k = 0; k < 4; ++k) ae[tt][k] = ao[tt][k] = 0.f;
        if (maxlen > t0) {
            for (int c0 = 0; c0 < Cout; c0 += CONV_KC) {
                const int kc = Cout - c0 < CONV_KC ? Cout - c0 : CONV_KC;
                __syncthreads();
                // g of the rows t0 - 1 .. t0 + CONV_TSB, output bins m0 .. m0 + FT, kc output channels (channel fastest, as in y)
                const int per_row = NB * (FT + 1) * kc, total = (CONV_TSB + 2) * per_row;
                for (int e = tid; e < total; e += 256) {
                    const int row = e / per_row, r1 = e - row * per_row, ub = r1 / ((FT + 1) * kc), r2 = r1 - ub * (FT + 1) * kc;
                    const int bin = r2 / kc, cl = r2 - bin * kc;
                    const int t = t0 - 1 + row, fo = m0 + bin;
                    float v = 0.f;
                    if (t >= 0 && t < lens[ub] && fo < Fo) {
                        const long long r = (long long)t * B + (b0 + ub);
                        const long long c = (long long)fo * Cout + c0 + cl;
                        if (y[r * ldy + c] > 0.f) v = dy[r * lddy + c];
                    }
                    gs[((row * NB + ub) * CONV_KC + cl) * NBG + bin] = v;
                }
                for (int e = tid; e < 9 * CI4 * kc; e += 256) {
                    const int tap = e / (CI4 * kc), r1 = e - tap * CI4 * kc, ci = r1 / kc, cl = r1 - ci * kc;
                    ws[(tap * CONV_KC + cl) * CI4 + ci] = ci < Cin ? w[((long long)tap * Cin + ci) * Cout + c0 + cl] : 0.f;
                }
                __syncthreads();
                if (mine) {
                    for (int cl = 0; cl < kc; ++cl) {
                        float ga[CONV_TSB + 2], gb[CONV_TSB + 2];
#pragma unroll
                        for (int r = 0; r < CONV_TSB + 2; ++r) {
                            const float *p = gs + ((r * NB + bb) * CONV_KC + cl) * NBG + ml;
                            ga[r] = p[0];
                            gb[r] = p[1];
                        }
#pragma unroll
                        for (int i = 0; i < 3; ++i) {
                            const float4 w0 = *reinterpret_cast<const float4 *>(ws + ((i * 3 + 0) * CONV_KC + cl) * CI4 + 4 * cg);
                            const float4 w1 = *reinterpret_cast<const float4 *>(ws + ((i * 3 + 1) * CONV_KC + cl) * CI4 + 4 * cg);
                            const float4 w2 = *reinterpret_cast<const float4 *>(ws + ((i * 3 + 2) * CONV_KC + cl) * CI4 + 4 * cg);
#pragma unroll
                            for (int tt = 0; tt < CONV_TSB; ++tt) {
                                // dx[t] takes tap i from g[t - i + 1]: row tt + 2 - i of the tile
                                const float a = ga[tt + 2 - i], b = gb[tt + 2 - i];
                                ae[tt][0] = __fmaf_rn(a, w1.x, ae[tt][0]);
                                ae[tt][1] = __fmaf_rn(a, w1.y, ae[tt][1]);
                                ae[tt][2] = __fmaf_rn(a, w1.z, ae[tt][2]);
                                ae[tt][3] = __fmaf_rn(a, w1.w, ae[tt][3]);
                                ao[tt][0] = __fmaf_rn(b, w0.x, __fmaf_rn(a, w2.x, ao[tt][0]));
                                ao[tt][1] = __fmaf_rn(b, w0.y, __fmaf_rn(a, w2.y, ao[tt][1]));
                                ao[tt][2] = __fmaf_rn(b, w0.z, __fmaf_rn(a, w2.z, ao[tt][2]));
                                ao[tt][3] = __fmaf_rn(b, w0.w, __fmaf_rn(a, w2.w, ao[tt][3]));
                            }
                        }
                    }
                }
            }
        }
        const int b = b0 + bb, m = m0 + ml;
        if (mine && b < B && m < Fo) {
            const int len = lens[bb];
#pragma unroll
            for (int tt = 0; tt < CONV_TSB; ++tt) {
                const int t = t0 + tt;
                if (t >= T) break;
                const bool live = t < len;
                float *row = dx + ((long long)t * B + b) * lddx;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int f = 2 * m + h;
                    if (f >= F) break;
                    float o[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) o[k] = live ? (h ? ao[tt][k] : ae[tt][k]) : 0.f;
                    if (VEC) {
                        *reinterpret_cast<float4 *>(row + (long long)f * Cin + 4 * cg) = make_float4(o[0], o[1], o[2], o[3]);
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            if (4 * cg + k < Cin) row[conv_xcol(gm, f, 4 * cg + k, F, Cin)] = o[k];
                    }
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------ weight gradient
// Workgroup (p, chunk) walks the tiles [p * per, (p + 1) * per) - CONV_DW_TS frames x CONV_DW_FT output bins of one utterance
// each, in a fixed order - for the input channels chunk * CONV_KC .. and leaves its share of one [9 Cin Cout + Cout] partial at
// part + p * n (dbias behind dw, from chunk 0).  Thread (cl, cg) of sub-group `sub`: the 9 taps of one input channel x 4 output
// channels over every NSUB-th position of the tile; the sub-groups are added in ascending order through LDS at the end.
// LDS: xs[CONV_DW_TS + 2][2 CONV_DW_FT + 1][CONV_KC] | gs[CONV_DW_TS][CONV_DW_FT][Cout], and over it at the end
// red[9][CONV_KC][Cout] | redb[Cout].  VEC: y and dy are read 16 bytes at a time.
template <bool VEC>
__global__ __launch_bounds__(256) void conv_dw_kernel(const float *__restrict__ x, long long ldx, int gm, const float *__restrict__ y,
                                                      long long ldy, const float *__restrict__ dy, long long lddy, int T, int B, int F,
                                                      int Fo, int Cin, int Cout, const int *__restrict__ seq_len,
                                                      float *__restrict__ part, long long items, long long per, int nft)
{
    constexpr int XB = 2 * CONV_DW_FT + 1;
    __shared__ float xs[(CONV_DW_TS + 2) * XB * CONV_KC];
    __shared__ __attribute__((aligned(16))) float gs[CONV_DW_TS * CONV_DW_FT * CONV_MAX_C];
    __shared__ __attribute__((aligned(16))) float redb[CONV_MAX_C];
    static_assert(CONV_DW_TS * CONV_DW_FT >= 9 * CONV_KC, "the partial fits over the g tile");
    float *red = gs;
    const int tid = threadIdx.x, CG = Cout / 4;
    const int c0 = blockIdx.y * CONV_KC, kc = Cin - c0 < CONV_KC ? Cin - c0 : CONV_KC;
    const int kce = Cin < CONV_KC ? Cin : CONV_KC;                  // threads along the channel chunk
    const int tps = kce * CG, NSUB = 256 / tps;
    const int sub = tid / tps, cl = tid % kce, cg = (tid % tps) / kce;
    const bool mine = sub < NSUB && cl < kc;
    float4 acc[9], bacc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    long long i1 = (blockIdx.x + 1) * per;
    i1 = i1 < items ? i1 : items;
    for (long long item = blockIdx.x * per; item < i1; ++item) {
        const int ft = (int)(item % nft), b = (int)((item / nft) % B), seg = (int)(item / ((long long)nft * B));
        const int t0 = seg * CONV_DW_TS, fo0 = ft * CONV_DW_FT;
        const int len = conv_len(seq_len, b, B, T);
        if (len <= t0) continue;                                     // (uniform: the whole workgroup is on one utterance)
        __syncthreads();
        for (int e = tid; e < (CONV_DW_TS + 2) * XB * kc; e += 256) {
            const int row = e / (XB * kc), r1 = e - row * XB * kc;
            int cc, bin;
            if (gm) { cc = r1 / XB; bin = r1 - cc * XB; } else { bin = r1 / kc; cc = r1 - bin * kc; }
            const int t = t0 - 1 + row, f = 2 * fo0 - 1 + bin;
            float v = 0.f;
            if (t >= 0 && t < len && f >= 0 && f < F) v = x[((long long)t * B + b) * ldx + conv_xcol(gm, f, c0 + cc, F, Cin)];
            xs[(row * XB + bin) * CONV_KC + cc] = v;
        }
        // g of the tile: per frame one run of CONV_DW_FT * Cout columns from fo0 * Cout, cut at the row's end
        const int run = CONV_DW_FT * Cout, c_lo = fo0 * Cout, c_hi = Fo * Cout;
        if (VEC) {
            for (int e = tid; e < CONV_DW_TS * run / 4; e += 256) {
                const int tt = e / (run / 4), q = e - tt * (run / 4), t = t0 + tt, c = c_lo + 4 * q;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (t < len && c < c_hi) {
                    const long long r = (long long)t * B + b;
                    const float4 yv = *reinterpret_cast<const float4 *>(y + r * ldy + c);
                    const float4 dv = *reinterpret_cast<const float4 *>(dy + r * lddy + c);
                    v.x = yv.x > 0.f ? dv.x : 0.f;
                    v.y = yv.y > 0.f ? dv.y : 0.f;
                    v.z = yv.z > 0.f ? dv.z : 0.f;
                    v.w = yv.w > 0.f ? dv.w : 0.f;
                }
                *reinterpret_cast<float4 *>(gs + tt * run + 4 * q) = v;
            }
        } else {
            for (int e = tid; e < CONV_DW_TS * run; e += 256) {
                const int tt = e / run, q = e - tt * run, t = t0 + tt, c = c_lo + q;
                float v = 0.f;
                if (t < len && c < c_hi) {
                    const long long r = (long long)t * B + b;
                    const float yv = y[r * ldy + c], dv = dy[r * lddy + c];
                    v = yv > 0.f ? dv : 0.f;
                }
                gs[tt * run + q] = v;
            }
        }
        __syncthreads();
        if (mine) {
            for (int p = sub; p < CONV_DW_TS * CONV_DW_FT; p += NSUB) {
                const int tt = p / CONV_DW_FT, fl = p - tt * CONV_DW_FT;
                if (t0 + tt >= len || fo0 + fl >= Fo) continue;
                const float4 gv = *reinterpret_cast<const float4 *>(gs + p * Cout + 4 * cg);
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        const float xv = xs[((tt + i) * XB + 2 * fl + j) * CONV_KC + cl];
                        float4 &a = acc[i * 3 + j];
                        a.x = __fmaf_rn(xv, gv.x, a.x);
                        a.y = __fmaf_rn(xv, gv.y, a.y);
                        a.z = __fmaf_rn(xv, gv.z, a.z);
                        a.w = __fmaf_rn(xv, gv.w, a.w);
                    }
                bacc.x += gv.x; bacc.y += gv.y; bacc.z += gv.z; bacc.w += gv.w;
            }
        }
    }
    // the sub-groups one after the other, in a fixed order
    for (int s = 0; s < NSUB; ++s) {
        __syncthreads();
        if (mine && sub == s) {
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                float4 *r = reinterpret_cast<float4 *>(red + (k * CONV_KC + cl) * Cout + 4 * cg);
                float4 v = acc[k];
                if (s) { const float4 o = *r; v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w; }
                *r = v;
            }
            if (cl == 0) {
                float4 *r = reinterpret_cast<float4 *>(redb + 4 * cg);
                float4 v = bacc;
                if (s) { const float4 o = *r; v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w; }
                *r = v;
            }
        }
    }
    __syncthreads();
    const long long n = 9LL * Cin * Cout + Cout;
    float *dst = part + (long long)blockIdx.x * n;
    for (int e = tid; e < 9 * kc * Cout; e += 256) {
        const int tap = e / (kc * Cout), r1 = e - tap * kc * Cout;           // r1 = cl * Cout + co
        dst[((long long)tap * Cin + c0) * Cout + r1] = red[tap * CONV_KC * Cout + r1];
    }
    if (blockIdx.y == 0)
        for (int e = tid; e < Cout; e += 256) dst[9LL * Cin * Cout + e] = redb[e];
}

// dw | dbias = the sum of the nparts partials of n elements, in a fixed order: four interleaved running sums, added in order
__global__ __launch_bounds__(256) void conv_fold_kernel(const float *__restrict__ part, int nparts, long long n, long long nw,
                                                        float *__restrict__ dw, float *__restrict__ dbias)
{
    const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
    if (o >= n) return;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    const float *p = part + o;
    int k = 0;
    for (; k + 3 < nparts; k += 4) {
        s0 += p[(long long)k * n];
        s1 += p[(long long)(k + 1) * n];
        s2 += p[(long long)(k + 2) * n];
        s3 += p[(long long)(k + 3) * n];
    }
    for (; k < nparts; ++k) s0 += p[(long long)k * n];
    const float v = (s0 + s1) + (s2 + s3);
    if (o < nw) dw[o] = v; else dbias[o - nw] = v;
}

// the tiles of the weight gradient, the tiles each workgroup walks and the partials that leaves: CONV_DW_GROUPS workgroups
// over the chunks of input channels, at least CONV_DW_MIN_PARTS partials
void conv_dw_shares(int T, int B, int Fo, int Cin, long long &items, long long &per, int &nparts, int &nft)
{
    const int chunks = lc_cdiv(Cin, CONV_KC);
    const int cap = CONV_DW_GROUPS / chunks > CONV_DW_MIN_PARTS ? CONV_DW_GROUPS / chunks : CONV_DW_MIN_PARTS;
    nft = lc_cdiv(Fo, CONV_DW_FT);
    items = (long long)lc_cdiv(T, CONV_DW_TS) * B * nft;
    per = (items + cap - 1) / cap;
    nparts = (int)((items + per - 1) / per);
}

bool conv_shape_ok(int T, int B, int F, int Cin, int Cout)
{
    return T > 0 && B > 0 && F > 0 && F <= CONV_MAX_F && Cin > 0 && Cin <= CONV_MAX_C && Cout > 0 && Cout <= CONV_MAX_C &&
           Cout % 8 == 0;
}

#define CONV_SHAPE_MSG "%s: bad shape (T %d, B %d, F %d, Cin %d, Cout %d; F in 1..%d, Cin in 1..%d, Cout a multiple of 8 in 8..%d)"

}  // namespace

extern "C" size_t lc_conv_workspace_bytes(int T, int B, int F, int Cin, int Cout)
{
    if (!conv_shape_ok(T, B, F, Cin, Cout)) return 0;
    long long items, per;
    int nparts, nft;
    conv_dw_shares(T, B, (F + 1) / 2, Cin, items, per, nparts, nft);
    return lc_align256((size_t)nparts * (size_t)(9 * Cin * Cout + Cout) * sizeof(float));
}

extern "C" int lc_conv_fwd(const float *x, int ldx, int x_group_major, const float *w, const float *bias, int T, int B, int F, int Cin,
                           int Cout, const int *seq_len, float *y, int ldy, lc_stream_t stream)
{
    const char *who = "lc_conv_fwd";
    LC_CHECK_ARG(conv_shape_ok(T, B, F, Cin, Cout), CONV_SHAPE_MSG, who, T, B, F, Cin, Cout, (int)CONV_MAX_F, (int)CONV_MAX_C,
                 (int)CONV_MAX_C);
    LC_CHECK_ARG(x && w && bias && seq_len && y, "%s: null pointer", who);
    const int Fo = (F + 1) / 2, Cx = Cin * F, Cy = Fo * Cout;
    LC_CHECK_ARG(ldx >= Cx && ldy >= Cy, "%s: a row pitch (%d, %d) below the row (%d, %d)", who, ldx, ldy, Cx, Cy);
    const long long nrows = (long long)T * B;
    LC_CHECK_ARG(!rs_overlap(x, ldx, nrows, Cx, y, ldy, nrows, Cy) && !rs_overlap(w, 9 * Cin * Cout, 1, 9 * Cin * Cout, y, ldy, nrows, Cy) &&
                     !rs_overlap(bias, Cout, 1, Cout, y, ldy, nrows, Cy),
                 "%s: y overlaps an input", who);
    const ConvTiles g = conv_tiles(T, B, Fo, Cout, CONV_TS);
    const int NBINS = 2 * g.FT + 1;
    const int xs_floats = ((CONV_TS + 2) * g.NB * CONV_KC * NBINS + 3) / 4 * 4;
    const size_t lds = (size_t)(CONV_MAX_NB + xs_floats + 9 * CONV_KC * Cout) * sizeof(float);
    const dim3 grid((unsigned)(g.items < CONV_MAX_GROUPS ? g.items : CONV_MAX_GROUPS)), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (rs_vec16(Cout, {ldy}, {y}))
        hipLaunchKernelGGL(conv_fwd_kernel<true>, grid, block, lds, s, x, (long long)ldx, x_group_major, w, bias, T, B, F, Fo, Cin, Cout,
                           seq_len, y, (long long)ldy, g, xs_floats);
    else
        hipLaunchKernelGGL(conv_fwd_kernel<false>, grid, block, lds, s, x, (long long)ldx, x_group_major, w, bias, T, B, F, Fo, Cin, Cout,
                           seq_len, y, (long long)ldy, g, xs_floats);
    LC_CHECK_LAUNCH(who);
    return LC_OK;
}

extern "C" int lc_conv_bwd(const float *x, int ldx, int x_group_major, const float *y, int ldy, const float *dy, int lddy, const float *w,
                           int T, int B, int F, int Cin, int Cout, const int *seq_len, float *dx, int lddx, float *dw, float *dbias,
                           void *workspace, size_t workspace_bytes, lc_stream_t stream)
{
    const char *who = "lc_conv_bwd";
    LC_CHECK_ARG(conv_shape_ok(T, B, F, Cin, Cout), CONV_SHAPE_MSG, who, T, B, F, Cin, Cout, (int)CONV_MAX_F, (int)CONV_MAX_C,
                 (int)CONV_MAX_C);
    LC_CHECK_ARG(y && dy && w && seq_len, "%s: null pointer", who);
    LC_CHECK_ARG((dw != nullptr) == (dbias != nullptr), "%s: dw and dbias go together (both or neither)", who);
    LC_CHECK_ARG(dx || dw, "%s: nothing to compute (dx, dw and dbias are all NULL)", who);
    LC_CHECK_ARG(!dw || x, "%s: dw needs x", who);
    const int Fo = (F + 1) / 2, Cx = Cin * F, Cy = Fo * Cout, nw = 9 * Cin * Cout;
    LC_CHECK_ARG(ldy >= Cy && lddy >= Cy && (!dw || ldx >= Cx) && (!dx || lddx >= Cx),
                 "%s: a row pitch (%d, %d, %d, %d) below the row (%d, %d)", who, ldx, ldy, lddy, lddx, Cx, Cy);
    const long long nrows = (long long)T * B;
    if (dx)
        LC_CHECK_ARG(!(x && rs_overlap(x, ldx, nrows, Cx, dx, lddx, nrows, Cx)) && !rs_overlap(y, ldy, nrows, Cy, dx, lddx, nrows, Cx) &&
                         !rs_overlap(dy, lddy, nrows, Cy, dx, lddx, nrows, Cx) && !rs_overlap(w, nw, 1, nw, dx, lddx, nrows, Cx),
                     "%s: dx overlaps an input", who);
    if (dw) {
        const float *outs[2] = {dw, dbias};
        const long long on[2] = {nw, Cout};
        for (int k = 0; k < 2; ++k)
            LC_CHECK_ARG(!rs_overlap(x, ldx, nrows, Cx, outs[k], on[k], 1, on[k]) && !rs_overlap(y, ldy, nrows, Cy, outs[k], on[k], 1, on[k]) &&
                             !rs_overlap(dy, lddy, nrows, Cy, outs[k], on[k], 1, on[k]) && !rs_overlap(w, nw, 1, nw, outs[k], on[k], 1, on[k]) &&
                             !(dx && rs_overlap(dx, lddx, nrows, Cx, outs[k], on[k], 1, on[k])),
                         "%s: dw or dbias overlaps an input or dx", who);
        LC_CHECK_ARG(!rs_overlap(dw, nw, 1, nw, dbias, Cout, 1, Cout), "%s: dw and dbias overlap", who);
        const size_t need = lc_conv_workspace_bytes(T, B, F, Cin, Cout);
        if (!workspace || workspace_bytes < need) {
            lc_set_error("%s: workspace of %zu bytes needed (%zu given)", who, need, workspace ? workspace_bytes : (size_t)0);
            return LC_EWORKSPACE;
        }
    }
    hipStream_t s = (hipStream_t)stream;
    if (dx) {
        const ConvTiles g = conv_tiles(T, B, Fo, Cin, CONV_TSB);
        const int NBG = (g.FT + 1) | 1;
        const int gs_floats = ((CONV_TSB + 2) * g.NB * CONV_KC * NBG + 3) / 4 * 4;
        const size_t lds = (size_t)(CONV_MAX_NB + gs_floats + 9 * CONV_KC * 4 * g.CG) * sizeof(float);
        const dim3 grid((unsigned)(g.items < CONV_MAX_GROUPS ? g.items : CONV_MAX_GROUPS)), block(256);
        if (!x_group_major && rs_vec16(Cin, {lddx}, {dx}))
            hipLaunchKernelGGL(conv_dx_kernel<true>, grid, block, lds, s, y, (long long)ldy, dy, (long long)lddy, w, 0, T, B, F, Fo, Cin,
                               Cout, seq_len, dx, (long long)lddx, g, NBG, gs_floats);
        else
            hipLaunchKernelGGL(conv_dx_kernel<false>, grid, block, lds, s, y, (long long)ldy, dy, (long long)lddy, w, x_group_major, T, B,
                               F, Fo, Cin, Cout, seq_len, dx, (long long)lddx, g, NBG, gs_floats);
        LC_CHECK_LAUNCH(who);
    }
    if (dw) {
        long long items, per;
        int nparts, nft;
        conv_dw_shares(T, B, Fo, Cin, items, per, nparts, nft);
        float *part = (float *)workspace;
        const dim3 grid((unsigned)nparts, (unsigned)lc_cdiv(Cin, CONV_KC)), block(256);
        if (rs_vec16(Cout, {ldy, lddy}, {y, dy}))
            hipLaunchKernelGGL(conv_dw_kernel<true>, grid, block, 0, s, x, (long long)ldx, x_group_major, y, (long long)ldy, dy,
                               (long long)lddy, T, B, F, Fo, Cin, Cout, seq_len, part, items, per, nft);
        else
            hipLaunchKernelGGL(conv_dw_kernel<false>, grid, block, 0, s, x, (long long)ldx, x_group_major, y, (long long)ldy, dy,
                               (long long)lddy, T, B, F, Fo, Cin, Cout, seq_len, part, items, per, nft);
        LC_CHECK_LAUNCH(who);
        const long long n = (long long)nw + Cout;
        hipLaunchKernelGGL(conv_fold_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, part, nparts, n, (long long)nw, dw, dbias);
        LC_CHECK_LAUNCH(who);
    }
    return LC_OK;
}
