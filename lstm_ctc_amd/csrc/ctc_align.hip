// ctc_align.hip — CTC forced alignment: the best (Viterbi) path through the 2L+1 lattice lc_ctc_loss sums over.
// No reference counterpart (TF 1.8 has no such op).  DESIGN.md section 3.6.
//
// Three launches per call, one wave per work item, no LDS, no atomics (the result is bit-identical from call to call):
//   1. lat_lse_kernel          (ctc_lattice.h) one wave per live frame (t, b): lse[t, b] = log sum_k exp(logits[t, b, k]), fp32.
//   2. align_sweep_kernel<PPL> one wave per utterance.  Lane l holds the PPL consecutive lattice positions l * PPL .. l * PPL +
//      PPL - 1 in registers, so the s-1 / s-2 neighbours are in the lane itself except for position l * PPL (and, with one
//      position per lane, its s-2): those come by one DPP wave shift.  The cell values are DOUBLES: a cell's emission is the
//      fp32 log-softmax logits[t, b, k] - lse[t, b] (exact as a double difference), and T_b of them are added at 2^-53 - the
//      accumulation contributes nothing to the error at any T (fp32 sums would add T_b * 2^-24 * |score|, over the project's
//      1e-4 bar from T ~ 840).  The label gathers and the frame's lse are fetched a chunk of K frames ahead into registers.
//      Every cell leaves a 2-bit backpointer (0 = stay, 1 = from s-1, 2 = from s-2); a lane packs its positions' codes of
//      up to 16 frames into one 32-bit word and the wave stores rows of 64 words (256 bytes, coalesced).
//   3. align_trace_kernel<PPL> one wave per utterance.  The backpointer rows do not depend on the path - lane l needs its own
//      words only - so the wave loads them a chunk of frames ahead, all loads independent; the dependent chain is then
//      v_readlane + scalar bit arithmetic per frame, no memory access.  The position of every frame is parked in the lane of
//      that frame (a select, off the chain), and after a chunk the lanes turn positions into symbols (one label gather each,
//      off the chain) and store ali / label_index coalesced.
// Tie rule (fp32 inputs, exact comparisons): at a cell stay wins over s-1 wins over s-2 (a candidate replaces the incumbent only
// when strictly greater); at the end S-1 wins over S-2.
#include "common.h"
#include "ctc_lattice.h"
#include <math.h>

static int g_align_phases = 7;      // development hook: bit 0 = lse pass, bit 1 = sweep, bit 2 = backtrace

// geometry shared by the sweep and the backtrace: words per lane and frame, frames per word
template <int PPL> struct AlGeo {
    static constexpr int JW = PPL < 16 ? PPL : 16;        // positions per word and frame
    static constexpr int NWORD = (PPL + 15) / 16;         // words per lane and frame (2 at 32 positions per lane)
    static constexpr int TPW = 16 / JW;                   // frames per word
};

// ------------------------------------------------------------------------------------------ 2. forward sweep
template <int PPL>
__global__ __launch_bounds__(64) void align_sweep_kernel(const float *__restrict__ logits, int T, int B, int V,
                                                         const int *__restrict__ labels, const int *__restrict__ offs,
                                                         const int *__restrict__ seq_len, const float *__restrict__ lse,
                                                         unsigned *__restrict__ bp, int TG, int *__restrict__ endstate,
                                                         float *__restrict__ score)
{
    constexpr int NWORD = AlGeo<PPL>::NWORD, TPW = AlGeo<PPL>::TPW;
    // frames fetched ahead as one chunk (two chunks ahead in three rotating buffers was measured and is SLOWER: 238 vs 194 us
    // at B = 64, L = 100 - the sweep is bound by its dependent arithmetic, not by the gathers' latency)
    constexpr int K = PPL <= 4 ? 8 : 32 / PPL;
    constexpr int NG = PPL == 1 ? 1 : PPL / 2;            // label gathers per lane and frame
    const int b = blockIdx.x, lane = threadIdx.x;
    const int Tb = min(max(seq_len[b], 0), T);
    const int off = offs[b], L = offs[b + 1] - off, S = 2 * L + 1;
    const int blank = V - 1;
    const double NEG = lat_neg_inf();
    if (Tb == 0 || L < 0 || S > 64 * PPL) {
        if (lane == 0) { score[b] = Tb == 0 ? 0.0f : -INFINITY; endstate[b] = -1; }
        return;
    }
    // per position: is it inside the lattice, may it be entered from s-2; per gather: the class to fetch
    unsigned valid = 0, allow2 = 0;
    int gsym[NG];
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
        const int s = lane * PPL + j;
        if (s < S) valid |= 1u << j;
        if (PPL == 1 || (j & 1)) {
            int sym = blank;
            if ((s & 1) && s < S) {
                sym = min(max(labels[off + (s >> 1)], 0), blank);
                if (s >= 3 && sym != labels[off + (s >> 1) - 1]) allow2 |= 1u << j;
            }
            gsym[PPL == 1 ? 0 : j >> 1] = sym;
        }
    }
    const bool odd1 = (lane & 1) != 0;                    // PPL == 1: this lane's position is a label position

    double a[PPL];
#pragma unroll
    for (int j = 0; j < PPL; ++j) a[j] = NEG;
    if (lane == 0) a[0] = 0.0;                            // "before frame 0": frame 0 reaches positions 0 (stay) and 1 (s-1)

    float cg[K][NG], cb[K], cl[K], ng[K][NG], nb[K], nl[K];
    auto fetch = [&](int t0, float (&g)[K][NG], float (&gb)[K], float (&gl)[K]) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int t = min(t0 + k, Tb - 1);
            const size_t row = (size_t)t * B + b;
            const float *x = logits + row * V;
#pragma unroll
            for (int g_ = 0; g_ < NG; ++g_) g[k][g_] = x[gsym[g_]];
            gb[k] = x[blank];
            gl[k] = lse[row];
        }
    };
    fetch(0, cg, cb, cl);
    unsigned acc = 0;
    unsigned *bprow = bp + (size_t)b * TG * NWORD * 64 + lane;
    for (int t0 = 0; t0 < Tb; t0 += K) {
        fetch(t0 + K, ng, nb, nl);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int t = t0 + k;
            if (t < Tb) {
                const double lz = (double)cl[k];
                const double eb = (double)cb[k] - lz;
                const double in1 = lat_shr1(a[PPL - 1]);
                const double in2 = PPL == 1 ? lat_shr1(in1) : in1;      // s-2 of the lane's first label position
                unsigned bits[NWORD];
#pragma unroll
                for (int w = 0; w < NWORD; ++w) bits[w] = 0;
#pragma unroll
                for (int j = PPL - 1; j >= 0; --j) {                     // descending: a[j-1], a[j-2] are still the old frame's
                    const double p1 = j >= 1 ? a[j - 1] : in1;
                    double best = a[j];
                    unsigned code = 0;
                    if (p1 > best) { best = p1; code = 1; }
                    double e = eb;
                    if (PPL == 1) {
                        const double p2 = (allow2 & 1u) ? in2 : NEG;
                        if (p2 > best) { best = p2; code = 2; }
                        if (odd1) e = (double)cg[k][0] - lz;
                    } else if (j & 1) {
                        double p2 = j >= 2 ? a[j - 2] : in2;
                        p2 = (allow2 >> j & 1u) ? p2 : NEG;
                        if (p2 > best) { best = p2; code = 2; }
                        e = (double)cg[k][j >> 1] - lz;
                    }
                    a[j] = (valid >> j & 1u) ? best + e : NEG;
                    bits[j >> 4] |= code << (2 * (j & 15));
                }
                if (TPW == 1) {
#pragma unroll
                    for (int w = 0; w < NWORD; ++w) bprow[((size_t)t * NWORD + w) * 64] = bits[w];
                } else {
                    acc |= bits[0] << (2 * PPL * (t & (TPW - 1)));
                    if ((t & (TPW - 1)) == TPW - 1 || t == Tb - 1) {
                        bprow[(size_t)(t / TPW) * 64] = acc;
                        acc = 0;
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
#pragma unroll
            for (int g_ = 0; g_ < NG; ++g_) cg[k][g_] = ng[k][g_];
            cb[k] = nb[k];
            cl[k] = nl[k];
        }
    }
    // the path ends in S-1 (preferred) or S-2
    const int s1 = S - 1, s2 = S - 2;
    double m1 = NEG, m2 = NEG;
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
        if (j == (s1 & (PPL - 1))) m1 = a[j];
        if (s2 >= 0 && j == (s2 & (PPL - 1))) m2 = a[j];
    }
    const double v1 = lat_readlane(m1, s1 / PPL);
    const double v2 = s2 >= 0 ? lat_readlane(m2, s2 / PPL) : NEG;
    int end = s1;
    double sc = v1;
    if (v2 > v1) { end = s2; sc = v2; }
    if (!(sc > NEG)) end = -1;
    if (lane == 0) { score[b] = end < 0 ? -INFINITY : (float)sc; endstate[b] = end; }
}

// ------------------------------------------------------------------------------------------ 3. backtrace
template <int PPL>
__global__ __launch_bounds__(64) void align_trace_kernel(int T, int B, int V, const int *__restrict__ labels,
                                                         const int *__restrict__ offs, const int *__restrict__ seq_len,
                                                         const unsigned *__restrict__ bp, int TG,
                                                         const int *__restrict__ endstate, int *__restrict__ ali,
                                                         int *__restrict__ lidx)
{
    constexpr int NWORD = AlGeo<PPL>::NWORD, TPW = AlGeo<PPL>::TPW;
    constexpr int CHF = PPL <= 4 ? 64 : 256 / PPL;         // frames per chunk: 64, 64, 64, 32, 16, 8
    constexpr int R = CHF / TPW * NWORD;                   // backpointer rows per chunk: 4, 8, 16, 16, 16, 16
    const int b = blockIdx.x, lane = threadIdx.x;
    const int Tb = min(max(seq_len[b], 0), T);
    const int off = offs[b];
    const int blank = V - 1;
    int *arow = ali + (size_t)b * T;
    int *lrow = lidx ? lidx + (size_t)b * T : nullptr;
    int s = __builtin_amdgcn_readfirstlane(endstate[b]);
    const int live = s >= 0 ? Tb : 0;                      // no path: everything is -1
    for (int t = live + lane; t < T; t += 64) {
        arow[t] = -1;
        if (lrow) lrow[t] = -1;
    }
    if (live == 0) return;
    const unsigned *bprow = bp + (size_t)b * TG * NWORD * 64 + lane;
    unsigned cur[R], nxt[R];
    auto fetch = [&](int base, unsigned (&r)[R]) {
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const int tg = base / TPW + i / NWORD;
            r[i] = (base >= 0 && tg < TG) ? bprow[((size_t)tg * NWORD + i % NWORD) * 64] : 0u;
        }
    };
    int base = (live - 1) / CHF * CHF;
    fetch(base, cur);
    for (; base >= 0; base -= CHF) {
        fetch(base - CHF, nxt);
        int sv = 0;
#pragma unroll
        for (int k = CHF - 1; k >= 0; --k) {
            const int t = base + k;
            if (t < live) {
                sv = lane == k ? s : sv;                 // off the chain: nothing below reads sv
                if (t > 0) {
                    const int owner = s / PPL, j = s & (PPL - 1);
                    unsigned word;
                    if (NWORD == 2) {
                        const unsigned w0 = __builtin_amdgcn_readlane(cur[(k / TPW) * NWORD], owner);
                        const unsigned w1 = __builtin_amdgcn_readlane(cur[(k / TPW) * NWORD + (NWORD - 1)], owner);
                        word = (j >> 4) ? w1 : w0;
                    } else {
                        word = __builtin_amdgcn_readlane(cur[k / TPW], owner);
                    }
                    const int shift = 2 * ((k % TPW) * AlGeo<PPL>::JW + (j & 15));
                    s -= (int)(word >> shift & 3u);
                    s = max(s, 0);
                }
            }
        }
        const int t = base + lane;
        if (lane < CHF && t < live) {
            const int l = sv >> 1;
            const bool lab = (sv & 1) != 0;
            arow[t] = lab ? labels[off + l] : blank;
            if (lrow) lrow[t] = lab ? l : -1;
        }
#pragma unroll
        for (int i = 0; i < R; ++i) cur[i] = nxt[i];
    }
}

// ------------------------------------------------------------------------------------------ C ABI
struct AlLayout {
    size_t lse, end, bp, total;
    int ppl, tg;
};
static inline AlLayout al_layout(int T, int B, int max_label_len)
{
    AlLayout m;
    m.ppl = lat_ppl(2 * max_label_len + 1);
    const int jw = m.ppl < 16 ? m.ppl : 16, nword = (m.ppl + 15) / 16, tpw = 16 / jw;
    m.tg = (T + tpw - 1) / tpw;
    size_t o = 0;
    m.lse = o; o += lc_align256((size_t)T * B * sizeof(float));
    m.end = o; o += lc_align256((size_t)B * sizeof(int));
    m.bp = o; o += lc_align256((size_t)B * m.tg * nword * 64 * sizeof(unsigned));
    m.total = o;
    return m;
}

extern "C" void lc_debug_ctc_align_phases(int mask) { g_align_phases = mask; }

extern "C" size_t lc_ctc_align_workspace_bytes(int T, int B, int V, int max_label_len)
{
    (void)V;
    if (T <= 0 || B <= 0 || max_label_len < 0 || max_label_len > 1023) return 0;
    return al_layout(T, B, max_label_len).total;
}

extern "C" int lc_ctc_align(const float *logits, int T, int B, int V, const int *labels, const int *label_offsets,
                            const int *seq_len, int max_label_len, int *ali, int *label_index, float *score,
                            void *workspace, size_t workspace_bytes, lc_stream_t stream)
{
    LC_CHECK_ARG(logits && labels && label_offsets && seq_len && ali && score && workspace, "lc_ctc_align: null pointer");
    LC_CHECK_ARG(T > 0 && B > 0 && V >= 2 && max_label_len >= 0, "lc_ctc_align: bad shape T=%d B=%d V=%d L=%d", T, B, V,
                 max_label_len);
    const int S = 2 * max_label_len + 1;
    LC_CHECK_ARG(S <= 64 * 32, "lc_ctc_align: label length %d exceeds the supported maximum 1023", max_label_len);
    const AlLayout m = al_layout(T, B, max_label_len);
    if (workspace_bytes < m.total) {
        lc_set_error("lc_ctc_align: workspace too small (%zu < %zu)", workspace_bytes, m.total);
        return LC_EWORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    char *w = (char *)workspace;
    float *lse = (float *)(w + m.lse);
    int *endstate = (int *)(w + m.end);
    unsigned *bp = (unsigned *)(w + m.bp);
    const int phases = g_align_phases;
    if (phases & 1) {
        hipLaunchKernelGGL(lat_lse_kernel<false>, dim3(lc_cdiv((long long)T * B, 4)), dim3(256), 0, s, logits, T, B, V, seq_len,
                           lse, (float *)nullptr);
        LC_CHECK_LAUNCH("ctc_align_lse");
    }
#define LC_AL(PPL)                                                                                                   \
    do {                                                                                                             \
        if (phases & 2)                                                                                              \
            hipLaunchKernelGGL(align_sweep_kernel<PPL>, dim3(B), dim3(64), 0, s, logits, T, B, V, labels, label_offsets, \
                               seq_len, lse, bp, m.tg, endstate, score);                                             \
        if (phases & 4)                                                                                              \
            hipLaunchKernelGGL(align_trace_kernel<PPL>, dim3(B), dim3(64), 0, s, T, B, V, labels, label_offsets,     \
                               seq_len, bp, m.tg, endstate, ali, label_index);                                       \
    } while (0)
    switch (m.ppl) {
    case 1: LC_AL(1); break;
    case 2: LC_AL(2); break;
    case 4: LC_AL(4); break;
    case 8: LC_AL(8); break;
    case 16: LC_AL(16); break;
    default: LC_AL(32); break;
    }
#undef LC_AL
    LC_CHECK_LAUNCH("ctc_align");
    return LC_OK;
}
