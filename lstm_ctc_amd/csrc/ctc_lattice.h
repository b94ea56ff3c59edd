// ctc_lattice.h — the device helpers of the double-cell log2-domain CTC lattices (ctc_window.hip, ctc_delay.hip; DESIGN.md
// section 3.8): "log zero" is -inf itself, a cell is a double, the log-sum-exp of a cell's predecessors runs on the fp32
// exp2 / log2 pipes relative to their maximum.
#pragma once
#include "common.h"
#include <float.h>

__device__ __forceinline__ double cw_neg_inf() { return __longlong_as_double(0xfff0000000000000ull); }
// log2(2^a + 2^b [+ 2^c]); -inf operands are "log zero", all of them -inf gives -inf (see ctc_window.hip's header)
__device__ __forceinline__ double cw_lse2(double a, double b)
{
    const double m = fmax(fmax(a, b), -DBL_MAX);
    return m + (double)__builtin_amdgcn_logf(__builtin_amdgcn_exp2f((float)(a - m)) + __builtin_amdgcn_exp2f((float)(b - m)));
}
__device__ __forceinline__ double cw_lse3(double a, double b, double c)
{
    const double m = fmax(fmax(fmax(a, b), c), -DBL_MAX);
    return m + (double)__builtin_amdgcn_logf(__builtin_amdgcn_exp2f((float)(a - m)) + __builtin_amdgcn_exp2f((float)(b - m)) +
                                             __builtin_amdgcn_exp2f((float)(c - m)));
}
// lane i receives x of lane i-1, lane 0 receives -inf (two 32-bit DPP wave_shr:1 moves)
__device__ __forceinline__ double cw_shr1(double x)
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), 0x138, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp((int)0xfff00000, __double2hiint(x), 0x138, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double cw_readlane(double x, int lane)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(x), lane);
    return __hiloint2double(hi, lo);
}
