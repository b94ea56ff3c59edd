// row_group.h — what the two-launch frame criteria share (xent.hip: one row per frame; kd.hip, consistency.hip: two rows per
// frame): reductions over a group of lanes that holds one frame, the grid-stride walk over the frames, a wave's pass over a row
// of any width, and the fixed-order fold of the per-frame terms.  The flag word's second bit is "the argmax is the target"
// for xent.hip and "the two argmaxes agree" for the other two.
#pragma once
#include "common.h"

// the flag word that goes to the workspace beside a frame's term
#define RG_SCORED 1
#define RG_AGREE 2
#define RG_BAD 4

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

}  // namespace
