// row_group.h — the two-launch frame criteria (xent.hip: one row per frame and a target; kd.hip, consistency.hip: two rows per
// frame), written once: reductions over a group of lanes that holds one frame, the grid-stride walk over the frames, a group's
// loads, argmaxes and stores of rows that fit registers, a wave's passes over a row of any width, the two kernels of a two-row
// CRITERION (what kd.hip and consistency.hip supply), the fixed-order fold of the per-frame terms and the host launcher with
// the V ladder.  The flag word's second bit is "the argmax is the target" for xent.hip and "the two argmaxes agree" for the
// other two.  DESIGN.md section 3.12.
#pragma once
#include "common.h"

// the flag word that goes to the workspace beside a frame's term
#define RG_SCORED 1
#define RG_AGREE 2
#define RG_BAD 4

#define RG_LOG2E 1.4426950408889634f
#define RG_LN2 0.6931471805599453f
#define RG_MAX_GRID 2048                 // blocks of four waves, as stream_grid in misc.hip
// A wide kernel over two rows re-reads both rows of a frame twice, and finds them in the Infinity Cache only while the rows of
// ALL waves in flight fit there: 2 rows x 4 V bytes x 4 waves per block.  Its grid is capped so that they take 128 MiB of the
// 256 (at least one block per CU): V = 5000 at 2048 blocks is 328 MB in flight and was measured at 1603 us per lc_kd_loss call,
// at 838 blocks 1256 us.
#define RG_WIDE_INFLIGHT_BYTES (128ll << 20)
#define RG_WIDE_MIN_GRID 256

namespace {

// ---- reductions over a group of G lanes (G = 16: one DPP row; G = 64: the wave); every lane of the group gets the result
#define RG_ROW_BUTTERFLY(OP, v, T, TOI, FROMI)                                                                          \
    v = OP(v, FROMI(__builtin_amdgcn_update_dpp(TOI(v), TOI(v), 0xB1, 0xf, 0xf, false)));  /* quad_perm [1,0,3,2] */   \
    v = OP(v, FROMI(__builtin_amdgcn_update_dpp(TOI(v), TOI(v), 0x4E, 0xf, 0xf, false)));  /* quad_perm [2,3,0,1] */   \
    v = OP(v, FROMI(__builtin_amdgcn_update_dpp(TOI(v), TOI(v), 0x141, 0xf, 0xf, false))); /* row_half_mirror */       \
    v = OP(v, FROMI(__builtin_amdgcn_update_dpp(TOI(v), TOI(v), 0x140, 0xf, 0xf, false)))  /* row_mirror */
__device__ __forceinline__ int rg_mini(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int rg_id(int a) { return a; }

template <int G> __device__ __forceinline__ float rg_max(float v)
{
    if (G == 64) return lc_wave_max(v);
    RG_ROW_BUTTERFLY(fmaxf, v, float, __float_as_int, __int_as_float);
    return v;
}
template <int G> __device__ __forceinline__ float rg_sum(float v)
{
    if (G == 64) return lc_wave_sum(v);
    RG_ROW_BUTTERFLY(lc_addf, v, float, __float_as_int, __int_as_float);
    return v;
}
template <int G> __device__ __forceinline__ int rg_min(int v)
{
    RG_ROW_BUTTERFLY(rg_mini, v, int, rg_id, rg_id);
    if (G == 64) {
        const int a = __builtin_amdgcn_readlane(v, 0), b = __builtin_amdgcn_readlane(v, 16);
        const int c = __builtin_amdgcn_readlane(v, 32), d = __builtin_amdgcn_readlane(v, 48);
        v = rg_mini(rg_mini(a, b), rg_mini(c, d));
    }
    return v;
}

// What a frame is: its utterance and its time step.  The waves walk the frames f = t * B + b with a grid stride; (t, b) are
// carried along by additions (one division pair per wave at the start, none per frame).
struct RgWalk {
    int t0, b0, st, sb;
    __device__ __forceinline__ RgWalk(int first, int stride, int B) : t0(first / B), b0(first % B), st(stride / B), sb(stride % B) {}
    __device__ __forceinline__ void next(int B)
    {
        t0 += st;
        b0 += sb;
        if (b0 >= B) { b0 -= B; ++t0; }
    }
};
// The walk of a kernel of four waves per block with FW frames per wave (group g of the wave takes the g-th of them): f(t, b,
// valid, bt) once per pass of the grid, bt the frame's place in the workspace (and in xent's targets), both [B,T].  Only the
// last wave's groups can be invalid (t >= T), and only with FW > 1.  <= 2048 * 16 frames per pass.
template <int FW, class F> __device__ __forceinline__ void rg_for_frames(int T, int B, F f)
{
    const int g = ((int)threadIdx.x & 63) / (64 / FW);
    const int stride = (int)gridDim.x * 4 * FW;
    const int first = ((int)blockIdx.x * 4 + ((int)threadIdx.x >> 6)) * FW;
    const long long TB = (long long)T * B;
    RgWalk w(first, stride, B);
    for (long long fb = first; fb < TB; fb += stride, w.next(B)) {
        int b = w.b0 + g, t = w.t0;
#pragma unroll
        for (int i = 0; i < FW - 1; ++i)             // g < FW: at most FW - 1 wraps (B = 1)
            if (b >= B) { b -= B; ++t; }
        f(t, b, FW == 1 || t < T, (size_t)b * T + t);
    }
}

// component k of a 16-byte access, k known where the loops are unrolled
__device__ __forceinline__ float rg_get(const float4 &q, int k) { return k == 0 ? q.x : k == 1 ? q.y : k == 2 ? q.z : q.w; }
__device__ __forceinline__ void rg_put(float4 &q, int k, float v)
{
    if (k == 0) q.x = v; else if (k == 1) q.y = v; else if (k == 2) q.z = v; else q.w = v;
}

// ---- rows that fit registers: lane l of a group of G holds NE elements of each row of its frame.  VEC (V % 4 == 0, every row
// on a 16-byte boundary): 16-byte accesses, register j is element 4 ((j / 4) G + l) + j % 4; otherwise dwords, element j G + l.
template <int G, int NE, bool VEC> struct RgGroup {
    static constexpr int NQ = NE / 4;                // 16-byte accesses per lane and row (VEC)
    const int l;
    __device__ __forceinline__ RgGroup() : l((int)threadIdx.x & (G - 1)) {}
    __device__ __forceinline__ int idx(int j) const { return VEC ? 4 * ((j >> 2) * G + l) + (j & 3) : j * G + l; }
    // NR rows at `row` from their bases xr, once: -inf beyond V and where `on` is false (nothing is read there)
    template <int NR> __device__ __forceinline__ void load(float (&x)[NR][NE], const float *const (&xr)[NR], size_t row, int V, bool on) const
    {
        const float *p[NR];                          // the lane's first element; the others are constants on
#pragma unroll
        for (int r = 0; r < NR; ++r) p[r] = xr[r] + row + (VEC ? 4 * l : l);
        if constexpr (VEC) {
#pragma unroll
            for (int jq = 0; jq < NQ; ++jq) {
                const int q = jq * G + l;
#pragma unroll
                for (int r = 0; r < NR; ++r) {
                    float4 v = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
                    if (on && 4 * q < V) v = *(const float4 *)(p[r] + 4 * jq * G);
                    x[r][4 * jq] = v.x; x[r][4 * jq + 1] = v.y; x[r][4 * jq + 2] = v.z; x[r][4 * jq + 3] = v.w;
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < NE; ++j) {
                const int e = j * G + l;
#pragma unroll
                for (int r = 0; r < NR; ++r) x[r][j] = (on && e < V) ? p[r][j * G] : -INFINITY;
            }
        }
    }
    // the maximum of each of NR rows and the lowest index that holds it (idx rises with j inside a lane)
    template <int NR> __device__ __forceinline__ void top(const float (&x)[NR][NE], float (&m)[NR], int (&amax)[NR]) const
    {
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            float v = x[r][0];
#pragma unroll
            for (int j = 1; j < NE; ++j) v = fmaxf(v, x[r][j]);
            m[r] = rg_max<G>(v);
        }
        int c[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) c[r] = 0x7fffffff;
#pragma unroll
        for (int j = NE - 1; j >= 0; --j) {
            const int e = idx(j);
#pragma unroll
            for (int r = 0; r < NR; ++r) c[r] = x[r][j] == m[r] ? e : c[r];
        }
#pragma unroll
        for (int r = 0; r < NR; ++r) amax[r] = rg_min<G>(c[r]);
    }
    // NG gradient rows of zeros at `row` from their bases g
    template <int NG> __device__ __forceinline__ void zero(float *const (&g)[NG], size_t row, int V) const
    {
        store(g, row, V, false, 0, [](int, float (&)[NG]) {});
    }
    // NG gradient rows: f(j, out) gives register j's element of each where the frame is good, a frame that is not gets zeros;
    // acc: added to what the rows hold (the caller leaves the rows of frames that are not good alone).  The 16-byte form builds
    // float4 values and adds to them as kd.hip's own loop did: which of a criterion's a * b - c * d the compiler fuses follows
    // from that shape, and tests/test_gpu_frame_loss_bits.py holds the bits.
    template <int NG, class F>
    __device__ __forceinline__ void store(float *const (&g)[NG], size_t row, int V, bool good, int acc, F f) const
    {
        float *p[NG];                                // the lane's first element; the others are constants on
#pragma unroll
        for (int i = 0; i < NG; ++i) p[i] = g[i] + row + (VEC ? 4 * l : l);
        if constexpr (VEC) {
#pragma unroll
            for (int jq = 0; jq < NQ; ++jq) {
                const int q = jq * G + l;
                if (4 * q >= V) continue;
                float4 v[NG];
#pragma unroll
                for (int i = 0; i < NG; ++i) v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (good) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        float out[NG];
                        f(4 * jq + k, out);
#pragma unroll
                        for (int i = 0; i < NG; ++i) rg_put(v[i], k, out[i]);
                    }
                    if (acc) {
#pragma unroll
                        for (int i = 0; i < NG; ++i) {
                            const float4 o = *(const float4 *)(p[i] + 4 * jq * G);
                            v[i].x += o.x; v[i].y += o.y; v[i].z += o.z; v[i].w += o.w;
                        }
                    }
                }
#pragma unroll
                for (int i = 0; i < NG; ++i) *(float4 *)(p[i] + 4 * jq * G) = v[i];
            }
        } else {
#pragma unroll
            for (int j = 0; j < NE; ++j) {
                const int e = j * G + l;
                if (e >= V) continue;
                float v[NG] = {};
                if (good) {
                    f(j, v);
                    if (acc) {
#pragma unroll
                        for (int i = 0; i < NG; ++i) v[i] += p[i][j * G];
                    }
                }
#pragma unroll
                for (int i = 0; i < NG; ++i) p[i][j * G] = v[i];
            }
        }
    }
};

// ---- one pass of a wave over a row of V elements.  VEC (16-byte aligned buffers, any V): the row starts `head` = 0 .. 3
// elements short of a 16-byte boundary; lanes 0 .. head - 1 take those as dwords, the body goes in 16-byte accesses, the last
// (V - head) % 4 elements as dwords again.  A lane's indices rise in the order it visits them.  f1(e): element e; f4(e):
// elements e .. e + 3, 16-byte aligned.
template <bool VEC, class F1, class F4>
__device__ __forceinline__ void rg_walk_row(int lane, int V, int head, F1 f1, F4 f4)
{
    if (!VEC) {
        for (int e = lane; e < V; e += 64) f1(e);
        return;
    }
    if (lane < head) f1(lane);
    const int nq = (V - head) >> 2;
    for (int q = lane; q < nq; q += 64) f4(head + 4 * q);
    const int rest = head + 4 * nq;
    if (lane < V - rest) f1(rest + lane);
}
// NG gradient rows of zeros
template <bool VEC, int NG> __device__ __forceinline__ void rg_wide_zero(int lane, int V, int head, float *const (&gr)[NG])
{
    rg_walk_row<VEC>(lane, V, head,
                     [&](int e) {
#pragma unroll
                         for (int i = 0; i < NG; ++i) gr[i][e] = 0.0f;
                     },
                     [&](int e) {
#pragma unroll
                         for (int i = 0; i < NG; ++i) *(float4 *)(gr[i] + e) = make_float4(0.f, 0.f, 0.f, 0.f);
                     });
}
// a pass over NR rows read together: f(e, x), x[r] element e of row r (f's to change)
template <bool VEC, int NR, class F>
__device__ __forceinline__ void rg_wide_pass(int lane, int V, int head, const float *const (&xr)[NR], F f)
{
    rg_walk_row<VEC>(lane, V, head,
                     [&](int e) {
                         float x[NR];
#pragma unroll
                         for (int r = 0; r < NR; ++r) x[r] = xr[r][e];
                         f(e, x);
                     },
                     [&](int e) {
                         float4 q[NR];
#pragma unroll
                         for (int r = 0; r < NR; ++r) q[r] = *(const float4 *)(xr[r] + e);
#pragma unroll
                         for (int k = 0; k < 4; ++k) {
                             float x[NR];
#pragma unroll
                             for (int r = 0; r < NR; ++r) x[r] = rg_get(q[r], k);
                             f(e + k, x);
                         }
                     });
}
// pass 1: the maximum of each row and the lowest index that holds it (a lane's indices rise, so strictly-greater keeps its first)
template <bool VEC, int NR>
__device__ __forceinline__ void rg_wide_top(int lane, int V, int head, const float *const (&xr)[NR], float (&m)[NR], int (&amax)[NR])
{
    float lm[NR];
    int c[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) { lm[r] = -INFINITY; c[r] = 0x7fffffff; }
    rg_wide_pass<VEC>(lane, V, head, xr, [&](int e, const float (&x)[NR]) {
#pragma unroll
        for (int r = 0; r < NR; ++r)
            if (x[r] > lm[r] || (c[r] == 0x7fffffff && x[r] == lm[r])) { lm[r] = x[r]; c[r] = e; }
    });
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        m[r] = lc_wave_max(lm[r]);
        amax[r] = rg_min<64>(lm[r] == m[r] ? c[r] : 0x7fffffff);
    }
}
// the last pass: f(e, x, out) makes element e of each of NG gradient rows from element e of each of NR rows; stored, or (acc)
// added to what the gradient rows hold; a frame that is not good reads nothing and stores zeros.  Without gradient rows (gr[0]
// null) f runs for what else it does.  Element by element, selects last, as kd.hip's own pass was: see RgGroup::store.
template <bool VEC, int NR, int NG, class F>
__device__ __forceinline__ void rg_wide_grad(int lane, int V, int head, const float *const (&xr)[NR], float *const (&gr)[NG],
                                             bool good, int acc, F f)
{
    auto g1 = [&](int e, float (&x)[NR], const float (&o)[NG], float (&out)[NG]) {
        f(e, x, out);
#pragma unroll
        for (int i = 0; i < NG; ++i) out[i] = !good ? 0.0f : acc ? out[i] + o[i] : out[i];
    };
    rg_walk_row<VEC>(lane, V, head,
                     [&](int e) {
                         float x[NR] = {}, o[NG] = {}, out[NG];
                         if (good) {
#pragma unroll
                             for (int r = 0; r < NR; ++r) x[r] = xr[r][e];
                             if (gr[0] && acc) {
#pragma unroll
                                 for (int i = 0; i < NG; ++i) o[i] = gr[i][e];
                             }
                         }
                         g1(e, x, o, out);
                         if (!gr[0]) return;
#pragma unroll
                         for (int i = 0; i < NG; ++i) gr[i][e] = out[i];
                     },
                     [&](int e) {
                         const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
                         float4 q[NR], o4[NG];
                         float v[NG][4];
#pragma unroll
                         for (int r = 0; r < NR; ++r) q[r] = zero4;
#pragma unroll
                         for (int i = 0; i < NG; ++i) o4[i] = zero4;
                         if (good) {
#pragma unroll
                             for (int r = 0; r < NR; ++r) q[r] = *(const float4 *)(xr[r] + e);
                             if (gr[0] && acc) {
#pragma unroll
                                 for (int i = 0; i < NG; ++i) o4[i] = *(const float4 *)(gr[i] + e);
                             }
                         }
#pragma unroll
                         for (int k = 0; k < 4; ++k) {
                             float x[NR], o[NG], out[NG];
#pragma unroll
                             for (int r = 0; r < NR; ++r) x[r] = rg_get(q[r], k);
#pragma unroll
                             for (int i = 0; i < NG; ++i) o[i] = rg_get(o4[i], k);
                             g1(e + k, x, o, out);
#pragma unroll
                             for (int i = 0; i < NG; ++i) v[i][k] = out[i];
                         }
                         if (!gr[0]) return;
#pragma unroll
                         for (int i = 0; i < NG; ++i) *(float4 *)(gr[i] + e) = make_float4(v[i][0], v[i][1], v[i][2], v[i][3]);
                     });
}

// ---- the fold: the body of a kernel of 256 threads, one workgroup per utterance (or pair) b = blockIdx.x.  terms [B,T]: a
// frame's term (float bits) and its flag word.  The terms are added in a FIXED order in double and rounded once.
__device__ __forceinline__ double rg_xor_d(double x, int mask)
{
    const int lo = __shfl_xor(__double2loint(x), mask, 64), hi = __shfl_xor(__double2hiint(x), mask, 64);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ void rg_fold(const int2 *__restrict__ terms, int T, float *__restrict__ loss, int *__restrict__ frames,
                                        int *__restrict__ agree)
{
    __shared__ double sacc[4];
    __shared__ int sn[4], sc[4], sbad[4];
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6;
    const int2 *row = terms + (size_t)b * T;
    double acc = 0.0;
    int n = 0, c = 0, bad = 0;
    for (int t = tid; t < T; t += 256) {             // thread i: frames i, i + 256, ... in sequence
        const int2 w = row[t];
        if (w.y & RG_SCORED) {
            acc += (double)__int_as_float(w.x);
            ++n;
            c += (w.y & RG_AGREE) ? 1 : 0;
        }
        bad |= w.y & RG_BAD;
    }
#pragma unroll
    for (int mask = 1; mask < 64; mask <<= 1) {      // both lanes of a pair add the same two operands: one result, fixed order
        acc += rg_xor_d(acc, mask);
        n += __shfl_xor(n, mask, 64);
        c += __shfl_xor(c, mask, 64);
        bad |= __shfl_xor(bad, mask, 64);
    }
    if ((tid & 63) == 0) { sacc[wave] = acc; sn[wave] = n; sc[wave] = c; sbad[wave] = bad; }
    __syncthreads();
    if (tid == 0) {
        const double total = (sacc[0] + sacc[1]) + (sacc[2] + sacc[3]);
        loss[b] = (sbad[0] | sbad[1] | sbad[2] | sbad[3]) ? __int_as_float(0x7fc00000) : (float)total;
        frames[b] = sn[0] + sn[1] + sn[2] + sn[3];
        agree[b] = sc[0] + sc[1] + sc[2] + sc[3];
    }
}
__global__ __launch_bounds__(256) void rg_fold_kernel(const int2 *__restrict__ terms, int T, float *__restrict__ loss,
                                                      int *__restrict__ frames, int *__restrict__ agree)
{
    rg_fold(terms, T, loss, frames, agree);
}

// ---- a two-row CRITERION: a struct passed to the two kernels below by value that says what differs between kd.hip and
// consistency.hip, and nothing else.
//   NG                        gradient rows per frame (1 or 2)
//   x[2], g[NG]               the bases of row 1, row 2 and the gradient row(s); g[0] null: no gradient
//   row(t, b, B, V)           the offset of frame (t, b)'s rows from those bases
//   head(row, V)              VEC wide kernel: how far the rows of that offset start short of a 16-byte boundary, 0 .. 3 elements
//   scored(t, b)              read only for frames inside [T, B]
//   Sums, open(m1, m2)        the frame's sums and coefficients, zeroed, with the two maxima
//   element(s, x1, x2, k)     first element loop: x1, x2 a register's elements of the two rows on entry and what the later steps
//                             need on exit, k a third register that is the criterion's to keep; the sums gain theirs
//   close<G>(s)               the sums over the group (rg_sum<G>, every lane) and the coefficients that follow from them
//   bad(s)                    the bad-row test, on the closed sums
//   TWO_LOOPS, second(s, x1, x2, k)   a second element loop after close() that the term needs (absent: neither)
//   term<G>(s)                the frame's term, every lane
//   grad_open(s, good)        the coefficients that only the gradient needs, where a gradient row is written
//   grad(s, x1, x2, out)      a register's gradient element(s)
// In the wide kernel a bad frame of a criterion with a second loop returns early (its term would come out of pass 3); one
// without goes through pass 3, reads nothing and stores zeros unless acc.  The per-lane order of every sum is j rising (rows in registers) or the order of rg_walk_row's visits (wide).
// At least five waves per SIMD: what <64, 16> had in kd.hip and consistency.hip (3 NE registers a lane and more); left to
// itself the scheduler gives consistency's 16-byte <64, 16> 106 VGPRs and four.
template <class Crit, int G, int NE, bool VEC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5))) void rg_rows_kernel(Crit cr, int T, int B, int V, int2 *__restrict__ terms, int acc)
{
    const RgGroup<G, NE, VEC> grp;
    rg_for_frames<64 / G>(T, B, [&](int t, int b, bool valid, size_t bt) {
        const bool scored = valid && cr.scored(t, b);
        const size_t row = cr.row(t, b, B, V);
        if (__builtin_amdgcn_ballot_w64(scored) == 0) {          // nothing to score in this wave: no row is read
            if (valid) {
                if (grp.l == 0) terms[bt] = make_int2(0, 0);
                if (cr.g[0] && !acc) grp.zero(cr.g, row, V);
            }
            return;
        }
        // both rows, once; -inf in groups that score nothing
        float x[2][NE], keep[NE], m[2];
        int amax[2];
        grp.load(x, cr.x, row, V, scored);
        grp.top(x, m, amax);
        auto s = cr.open(m[0], m[1]);
#pragma unroll
        for (int j = 0; j < NE; ++j) cr.element(s, x[0][j], x[1][j], keep[j]);
        cr.template close<G>(s);
        const bool bad = scored && cr.bad(s), good = scored && !bad;
        if constexpr (Crit::TWO_LOOPS) {
#pragma unroll
            for (int j = 0; j < NE; ++j) cr.second(s, x[0][j], x[1][j], keep[j]);
        }
        const float term = cr.template term<G>(s);
        if (valid && grp.l == 0)
            terms[bt] = make_int2(good ? __float_as_int(term) : 0,
                                  good ? (RG_SCORED | (amax[0] == amax[1] ? RG_AGREE : 0)) : (bad ? RG_BAD : 0));
        if (cr.g[0] && valid && (good || !acc)) {
            cr.grad_open(s, good);
            grp.store(cr.g, row, V, good, acc, [&](int j, float (&out)[Crit::NG]) { cr.grad(s, x[0][j], x[1][j], out); });
        }
    });
}

// Any row width: one frame per wave in three passes over the two rows (maxima + argmaxes, sums, second loop + gradient).
template <class Crit, bool VEC>
__global__ __launch_bounds__(256) void rg_wide_kernel(Crit cr, int T, int B, int V, int2 *__restrict__ terms, int acc)
{
    const int lane = threadIdx.x & 63;
    rg_for_frames<1>(T, B, [&](int t, int b, bool, size_t bt) {
        const size_t row = cr.row(t, b, B, V);
        const int head = VEC ? cr.head(row, V) : 0;
        const float *xr[2] = {cr.x[0] + row, cr.x[1] + row};
        float *gr[Crit::NG];
#pragma unroll
        for (int i = 0; i < Crit::NG; ++i) gr[i] = cr.g[i] ? cr.g[i] + row : nullptr;
        auto nothing = [&](int flags) {                                      // wave-uniform
            if (lane == 0) terms[bt] = make_int2(0, flags);
            if (gr[0] && !acc) rg_wide_zero<VEC>(lane, V, head, gr);
        };
        if (!cr.scored(t, b)) return nothing(0);
        float m[2];
        int amax[2];
        rg_wide_top<VEC>(lane, V, head, xr, m, amax);
        // pass 2: the sums, per lane in the order of its visits, then over the lanes
        auto s = cr.open(m[0], m[1]);
        rg_wide_pass<VEC>(lane, V, head, xr, [&](int, float (&x)[2]) {
            float keep;
            cr.element(s, x[0], x[1], keep);
        });
        cr.template close<64>(s);
        // a NaN slips past the maximum (comparisons), not past the sum.  The second loop has nothing to work on in a bad
        // frame; without one, a bad frame goes through pass 3 and stores zeros
        const bool good = !cr.bad(s);
        if (!good && Crit::TWO_LOOPS) return nothing(RG_BAD);
        // pass 3: the first loop again, into sums that are thrown away, then the second loop and the gradient row(s)
        if (Crit::TWO_LOOPS || (gr[0] && (good || !acc))) {
            cr.grad_open(s, good);
            rg_wide_grad<VEC>(lane, V, head, xr, gr, good, acc, [&](int, float (&x)[2], float (&out)[Crit::NG]) {
                auto away = s;
                float keep;
                cr.element(away, x[0], x[1], keep);
                if constexpr (Crit::TWO_LOOPS) cr.second(s, x[0], x[1], keep);
                cr.grad(s, x[0], x[1], out);
            });
        }
        const float term = cr.template term<64>(s);
        if (lane == 0)
            terms[bt] = make_int2(good ? __float_as_int(term) : 0, good ? (RG_SCORED | (amax[0] == amax[1] ? RG_AGREE : 0)) : RG_BAD);
    });
}

// ---- the host side, once.  The workspace: per frame its term (float) and a flag word.
inline size_t rg_workspace_bytes(int T, int B, int V)
{
    if (T <= 0 || B <= 0 || V < 2) return 0;
    return lc_align256((size_t)T * B * sizeof(int2));
}
// which kernel a V takes: G lanes a frame, NE registers a lane and row (0: the wide kernel)
template <int G_, int NE_, bool VEC_> struct RgShape {
    static constexpr int G = G_, NE = NE_;
    static constexpr bool VEC = VEC_;
};
// The two launches of a criterion call.  launch(RgShape, blocks) launches the frame kernel of that shape; vec / vec_wide: whether
// the rows-in-registers kernels / the wide kernel take 16-byte accesses; cap_wide: the wide kernel reads two rows a frame and
// its grid is capped for the Infinity Cache.
template <class L>
int rg_launch(const char *rows_tag, const char *fold_tag, int T, int B, int V, bool vec, bool vec_wide, bool cap_wide, int2 *terms,
              float *loss, int *frames, int *agree, hipStream_t s, L launch)
{
    long long cap = RG_MAX_GRID;
    if (cap_wide && V > 1024) {
        const long long fit = RG_WIDE_INFLIGHT_BYTES / (32ll * V);
        cap = fit < RG_WIDE_MIN_GRID ? RG_WIDE_MIN_GRID : fit < RG_MAX_GRID ? fit : RG_MAX_GRID;
    }
    auto go = [&](auto shape) {
        const long long per_block = 4 * (64 / decltype(shape)::G);
        long long nb = ((long long)T * B + per_block - 1) / per_block;
        if (nb > cap) nb = cap;
        launch(shape, (unsigned)nb);
    };
    auto either = [&](bool v, auto yes, auto no) { if (v) go(yes); else go(no); };
    if (V <= 64) either(vec, RgShape<16, 4, true>{}, RgShape<16, 4, false>{});
    else if (V <= 256) either(vec, RgShape<64, 4, true>{}, RgShape<64, 4, false>{});
    else if (V <= 512) either(vec, RgShape<64, 8, true>{}, RgShape<64, 8, false>{});
    else if (V <= 1024) either(vec, RgShape<64, 16, true>{}, RgShape<64, 16, false>{});
    else either(vec_wide, RgShape<64, 0, true>{}, RgShape<64, 0, false>{});
    LC_CHECK_LAUNCH(rows_tag);
    hipLaunchKernelGGL(rg_fold_kernel, dim3(B), dim3(256), 0, s, terms, T, loss, frames, agree);
    LC_CHECK_LAUNCH(fold_tag);
    return LC_OK;
}
// ... of a two-row criterion
template <class Crit>
int rg_launch_criterion(const char *rows_tag, const char *fold_tag, Crit cr, int T, int B, int V, bool vec, bool vec_wide,
                        int2 *terms, int acc, float *loss, int *frames, int *agree, hipStream_t s)
{
    return rg_launch(rows_tag, fold_tag, T, B, V, vec, vec_wide, true, terms, loss, frames, agree, s, [&](auto shape, unsigned nb) {
        using S = decltype(shape);
        if constexpr (S::NE == 0)
            hipLaunchKernelGGL((rg_wide_kernel<Crit, S::VEC>), dim3(nb), dim3(256), 0, s, cr, T, B, V, terms, acc);
        else
            hipLaunchKernelGGL((rg_rows_kernel<Crit, S::G, S::NE, S::VEC>), dim3(nb), dim3(256), 0, s, cr, T, B, V, terms, acc);
    });
}

}  // namespace
