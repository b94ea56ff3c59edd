// row_stream.h - the lanes-per-row skeleton of the memory-bound row passes, written once: LPR lanes (a power of two) walk one
// row of CV vectors, 256 / LPR rows per workgroup pass, workgroups take the row groups with a grid stride; V = float4 where
// every column count, pitch and base allows 16-byte accesses, V = float otherwise.  The passes that only move rows (misc.hip:
// packed frames, chunk.hip, time_reduce.hip) are one kernel over a row MAP; the passes that compute (row_conv.hip, specaug.hip,
// layer_norm.hip) keep their kernels and take the host side and the row loops from here.  What the skeleton guarantees: every
// output element is written exactly once, a dead source is never read, fills are +0, and there are no atomics and no LDS.
// DESIGN.md section 3.19.
#pragma once
#include "common.h"
#include <initializer_list>
#include <type_traits>

namespace {

constexpr int RS_MAX_GROUPS = 2048;      // workgroups per launch (8 per CU), the rest by grid stride

// ---- the host side
// Whether a pass may use 16-byte accesses: the column count and every pitch a multiple of 4 floats, every base 16-byte aligned
// (a null base passes: what is not there is not accessed).
inline bool rs_vec16(long long C, std::initializer_list<long long> pitches, std::initializer_list<const void *> bases)
{
    if (C % 4) return false;
    for (long long p : pitches) if (p % 4) return false;
    for (const void *b : bases) if ((uintptr_t)b & 15) return false;
    return true;
}

// Whether the byte ranges of an [rows_a, Ca] window at pitch lda and an [rows_b, Cb] window at pitch ldb intersect.
inline bool rs_overlap(const float *a, long long lda, long long rows_a, long long Ca, const float *b, long long ldb, long long rows_b,
                       long long Cb)
{
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + ((rows_a - 1) * lda + Ca) * sizeof(float);
    const uintptr_t b0 = (uintptr_t)b, b1 = b0 + ((rows_b - 1) * ldb + Cb) * sizeof(float);
    return !(a1 <= b0 || b1 <= a0);
}

// Lanes per row, the two rules.  Cover: the smallest power of two in lo .. hi that holds the row's CV vectors in one pass (hi
// where none does).
inline int rs_lanes_cover(int CV, int lo, int hi)
{
    int lpr = lo;
    while (lpr < hi && lpr < CV) lpr *= 2;
    return lpr;
}
// Fewest idle: the power of two in lo .. hi that leaves the fewest lanes idle over the row's passes (the widest such, at most 8
// passes per lane below hi) - 160 vectors take 32 lanes five times, not 256 lanes once with 96 of them idle.
inline int rs_lanes_fewest_idle(int CV, int lo, int hi)
{
    int lpr = hi;
    long long idle = -1;
    for (int l = hi; l >= lo; l /= 2) {
        const int passes = (CV + l - 1) / l;
        if (passes > 8 && l < hi) break;
        const long long w = (long long)passes * l - CV;
        if (idle < 0 || w < idle) { idle = w; lpr = l; }
    }
    return lpr;
}

// the workgroups of a launch over `items` items at `per_group` of them per workgroup pass
inline unsigned rs_grid(long long items, int per_group, int cap = RS_MAX_GROUPS)
{
    const long long groups = (items + per_group - 1) / per_group;
    return (unsigned)(groups < cap ? groups : cap);
}

// f(std::integral_constant<int, L>) for the power of two L = lpr in LO .. HI; any other value goes to HI.
template <int LO, int HI, class F> inline void rs_dispatch_lanes(int lpr, F &&f)
{
    if constexpr (LO < HI) {
        if (lpr == LO) f(std::integral_constant<int, LO>{});
        else rs_dispatch_lanes<2 * LO, HI>(lpr, f);
    } else {
        f(std::integral_constant<int, HI>{});
    }
}

// ---- the device side: a row of CV vectors under the LPR lanes that hold it
template <typename V, int LPR> __device__ __forceinline__ void zero_row(V *dst, int CV, int lane)
{
    for (int q = lane; q < CV; q += LPR) dst[q] = V{};
}
template <typename V, int LPR> __device__ __forceinline__ void copy_row(V *dst, const V *from, int CV, int lane)
{
    int q = lane;
    for (; q + 3 * LPR < CV; q += 4 * LPR) {                  // four loads in flight per lane before the first store
        const V v0 = from[q], v1 = from[q + LPR], v2 = from[q + 2 * LPR], v3 = from[q + 3 * LPR];
        dst[q] = v0; dst[q + LPR] = v1; dst[q + 2 * LPR] = v2; dst[q + 3 * LPR] = v3;
    }
    for (; q < CV; q += LPR) dst[q] = from[q];
}
__device__ __forceinline__ void rs_add(float &s, const float v) { s += v; }
__device__ __forceinline__ void rs_add(float4 &s, const float4 v) { s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w; }

// What a row map answers for output item i, in floats: the item's segment starts at out + dst and is the sum of n segments of x,
// the first at x + src, each next one `hop` further.  n = 0: the segment is +0 and x is not touched.
struct RsSpan {
    long long dst, src, hop;
    int n;
};
// The passes that only move rows.  Map: a small trivially-copyable struct with
//   static constexpr bool SUMS            whether n > 1 occurs (the sum loop is compiled only then)
//   template <int LPR> RsSpan locate(long long item, long long ldx, long long ldo) const
// n == 1 is copy_row; n > 1 adds the copies in ascending order, the first one initialising the sum (no 0 + ...).
template <typename V, int LPR, class Map>
__global__ __launch_bounds__(256) void map_rows_kernel(const float *__restrict__ x, long long ldx, long long nitems, int CV, Map m,
                                                       float *__restrict__ out, long long ldo)
{
    constexpr int RPB = 256 / LPR;
    const int lane = threadIdx.x % LPR, sub = threadIdx.x / LPR;
    const long long groups = (nitems + RPB - 1) / RPB;
    for (long long g = blockIdx.x; g < groups; g += gridDim.x) {
        const long long item = g * RPB + sub;
        if (item >= nitems) continue;
        const RsSpan sp = m.template locate<LPR>(item, ldx, ldo);
        V *dst = reinterpret_cast<V *>(out + sp.dst);
        if (sp.n == 0) {
            zero_row<V, LPR>(dst, CV, lane);
            continue;
        }
        if (!Map::SUMS || sp.n == 1) {
            copy_row<V, LPR>(dst, reinterpret_cast<const V *>(x + sp.src), CV, lane);
            continue;
        }
        if constexpr (Map::SUMS) {
            for (int q = lane; q < CV; q += LPR) {
                const float *p = x + sp.src;
                V s = reinterpret_cast<const V *>(p)[q];
                for (int k = 1; k < sp.n; ++k) {
                    p += sp.hop;
                    rs_add(s, reinterpret_cast<const V *>(p)[q]);
                }
                dst[q] = s;
            }
        }
    }
}

// Its launch: the 16-byte path where x, out and their pitches allow it, lanes per row by `lanes` (one of the two rules) in
// 4 .. 256, at most RS_MAX_GROUPS workgroups.
template <class Map>
void rs_launch_map(const float *x, long long ldx, float *out, long long ldo, long long nitems, int C, int (*lanes)(int, int, int),
                   const Map &m, hipStream_t s)
{
    auto go = [&](auto v, int CV) {
        using V = decltype(v);
        const int lpr = lanes(CV, 4, 256);
        const dim3 grid(rs_grid(nitems, 256 / lpr)), block(256);
        rs_dispatch_lanes<4, 256>(lpr, [&](auto L) {
            hipLaunchKernelGGL((map_rows_kernel<V, decltype(L)::value, Map>), grid, block, 0, s, x, ldx, nitems, CV, m, out, ldo);
        });
    };
    if (rs_vec16(C, {ldx, ldo}, {x, out})) go(float4{}, C / 4);
    else go(float{}, C);
}

}  // namespace
