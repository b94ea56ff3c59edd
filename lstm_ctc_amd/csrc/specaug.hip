// specaug.hip — lc_spec_augment: SpecAugment time / frequency masking of the spliced, subsampled filterbank batch (Park et
// al., 2019; no reference counterpart).  One HBM-bound streaming kernel, no MFMA, no atomics: one read and one write of
// [T * B, D], the draws regenerated from a counter-based hash (lc_hash_u32) and never stored.
//
// A workgroup walks groups of RPP consecutive rows with a grid stride.  Per group, in this order:
//   1. every lane issues the loads of its UNR rows (they depend on no mask), so they fly over step 2;
//   2. 16 threads per row form the row's masks - one thread per mask: two hashes, and for a time mask the translation of its
//      raw-frame interval into the interval of SPLICED BLOCKS of this row that show a frame of it (block i shows
//      clamp(t*s + i - l, 0, n-1), monotone in i, so the blocks are a contiguous range).  With at most 32 blocks and 64 bins
//      (BITS; every recipe) the 16 intervals are OR-ed across the 16 lanes into ONE 16-byte LDS word per row: a bit per
//      block, a bit per bin.  Otherwise the 16 (start, width) pairs go to LDS as they are.  A row that nothing touches has an
//      all-zero word (no pair of non-zero width) and is a plain copy.  The threads of the rows with t == 0 also write the
//      utterance's plan;
//   3. one barrier (the table is double-buffered by pass parity), then each lane reads its rows' words - broadcast LDS reads,
//      all UNR issued before the first is used - tests its elements (two ANDs each; one unsigned compare per pair without
//      BITS) and stores.
// A lane's columns are the same in every row it handles, so their block and bin numbers (two integer divisions per element)
// are taken once per thread, outside the row loop (rows wider than the 256 lanes of a workgroup divide on the fly).
// Measured (profiles/specaug_probe.txt): the first version tested every element against the pairs, one dependent LDS read per
// pair - 2.0 x a device copy at [1000, 64, 360]; the one-word form is what the file records now.
#include "row_stream.h"
#include <math.h>

namespace {

constexpr uint32_t SPEC_STREAM = 0x53504543u;   // "SPEC"

struct SpecArgs {
    int tm, tw, tp, fm, fw, F;      // masks, width cap, percent cap; masks, width cap, bins per feature group
    int base, l, s, nb;             // base_dim, left context, max(subsample, 1), spliced blocks 1 + l + r
    float fill;
    uint32_t seed;
};

__device__ __forceinline__ long long spec_ranged(uint32_t v, long long m) { return (long long)(((uint64_t)v * (uint64_t)m) >> 32); }

// (start, width) of mask `slot` of utterance b, in raw frames (slots 0-7) or bins (slots 8-15); (0, 0) for an unused slot
__device__ inline void spec_draw(const SpecArgs &a, int b, long long n, int slot, long long &st, long long &wd)
{
    st = wd = 0;
    const uint64_t k0 = (uint64_t)b * 32;
    if (slot < 8) {
        if (slot >= a.tm) return;
        long long W = n * a.tp / 100;
        if (W > a.tw) W = a.tw;
        wd = spec_ranged(lc_hash_u32(a.seed, SPEC_STREAM, k0 + 2 * slot), W + 1);
        st = spec_ranged(lc_hash_u32(a.seed, SPEC_STREAM, k0 + 2 * slot + 1), n - wd + 1);
    } else {
        const int j = slot - 8;
        if (j >= a.fm) return;
        wd = spec_ranged(lc_hash_u32(a.seed, SPEC_STREAM, k0 + 16 + 2 * j), (long long)a.fw + 1);
        st = spec_ranged(lc_hash_u32(a.seed, SPEC_STREAM, k0 + 17 + 2 * j), (long long)a.F - wd + 1);
    }
}

template <typename V> struct SpecVec;
template <> struct SpecVec<float> {
    static constexpr int N = 1;
    static __device__ __forceinline__ float &at(float &v, int) { return v; }
};
template <> struct SpecVec<float4> {
    static constexpr int N = 4;
    static __device__ __forceinline__ float &at(float4 &v, int e) { return e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w; }
};

// V = float4: 16-byte accesses (D, both pitches multiples of 4, aligned bases); V = float: anything.  LPR lanes walk one row
// (the power of two that covers its CV vectors, 16 .. 256), RPB = 256 / LPR rows side by side, UNR of those per pass.
// BITS: 1 + l + r <= 32 and freq_bins <= 64.
// x and out may be the same buffer: no __restrict__ on them; a thread reads what it writes, and reads it first.
template <typename V, int LPR, bool BITS>
__global__ __launch_bounds__(256) void spec_augment_kernel(const float *x, long long ldx, long long nrows, int B, int CV,
                                                           const int *__restrict__ seq_len, SpecArgs a, float *out,
                                                           long long ldo, int *__restrict__ plan)
{
    constexpr int EPV = SpecVec<V>::N, RPB = 256 / LPR, UNR = 4, RPP = RPB * UNR;
    __shared__ uint4 word[2][RPP];                          // BITS: {block bits, bin bits 0-31, bin bits 32-63, 0}; else {any, ..}
    __shared__ int2 tab[BITS ? 1 : 2][BITS ? 1 : RPP][16];  // without BITS: the rows' (start, width) pairs
    const int tid = threadIdx.x, lane = tid % LPR, sub = tid / LPR;
    const bool one = CV <= LPR;                  // a lane holds one vector per row
    int blk[EPV], bin[EPV];
#pragma unroll
    for (int e = 0; e < EPV; ++e) {
        const int c = lane * EPV + e;
        blk[e] = c / a.base;
        bin[e] = (c - blk[e] * a.base) % a.F;
    }
    // an element against its row: BITS - w is the row's word; else - tb its pairs
    auto masked = [&](const uint4 &w, const int2 *tb, int bk, int bn) -> bool {
        if constexpr (BITS) {
            return ((w.x >> (bk & 31)) | ((bn < 32 ? w.y : w.z) >> (bn & 31))) & 1u;
        } else {
            bool m = false;
            for (int j = 0; j < a.tm; ++j) m |= (unsigned)(bk - tb[j].x) < (unsigned)tb[j].y;
            for (int j = 0; j < a.fm; ++j) m |= (unsigned)(bn - tb[8 + j].x) < (unsigned)tb[8 + j].y;
            return m;
        }
    };
    const long long groups = (nrows + RPP - 1) / RPP;
    int buf = 0;
    for (long long g = blockIdx.x; g < groups; g += gridDim.x, buf ^= 1) {
        const long long r0 = g * RPP;
        // 1. the pass's loads, in flight over the table
        V v[UNR];
        if (one && lane < CV) {
#pragma unroll
            for (int k = 0; k < UNR; ++k) {
                const long long r = r0 + k * RPB + sub;
                if (r < nrows) v[k] = reinterpret_cast<const V *>(x + r * ldx)[lane];
            }
        }
        // 2. the rows' masks: thread (row slot rs, mask slot) - 16 rows per sweep of the workgroup
        for (int first = 0; first < RPP; first += 16) {
            const int rs = first + (tid >> 4), slot = tid & 15;
            const long long r = r0 + rs;
            int st = 0, wd = 0;                  // this mask on this row: blocks (slots 0-7) or bins (8-15); width 0 = none
            if (rs < RPP && r < nrows) {
                const long long t = r / B;
                const int b = (int)(r - t * B);
                const int len = seq_len[b];
                const bool live = t < len, planned = plan != nullptr && t == 0;
                if (live || planned) {
                    const long long n = len > 0 ? (long long)len * a.s : 0;
                    long long dst, dwd;
                    spec_draw(a, b, n, slot, dst, dwd);
                    if (planned) {
                        plan[((long long)b * 16 + slot) * 2] = (int)dst;
                        plan[((long long)b * 16 + slot) * 2 + 1] = (int)dwd;
                    }
                    if (live && dwd > 0) {
                        if (slot < 8) {          // raw frames [dst, dst + dwd) -> blocks [ilo, ihi) of this row
                            const long long lb = t * a.s - a.l, e = dst + dwd;
                            long long ilo = dst <= 0 ? 0 : dst - lb, ihi = e >= n ? a.nb : e - lb;
                            if (ilo < 0) ilo = 0;
                            if (ihi > a.nb) ihi = a.nb;
                            if (ihi > ilo) { st = (int)ilo; wd = (int)(ihi - ilo); }
                        } else {
                            st = (int)dst;
                            wd = (int)dwd;
                        }
                    }
                }
            }
            if constexpr (BITS) {                // OR the 16 intervals of a row: 16 consecutive lanes
                const unsigned long long ones = wd >= 64 ? ~0ull : (1ull << wd) - 1ull, bits = ones << st;
                unsigned tb = slot < 8 ? (unsigned)bits : 0u;
                unsigned flo = slot < 8 ? 0u : (unsigned)bits, fhi = slot < 8 ? 0u : (unsigned)(bits >> 32);
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) {
                    tb |= __shfl_xor(tb, o, 16);
                    flo |= __shfl_xor(flo, o, 16);
                    fhi |= __shfl_xor(fhi, o, 16);
                }
                if (rs < RPP && slot == 0) word[buf][rs] = make_uint4(tb, flo, fhi, 0u);
            } else {
                const unsigned long long some = __ballot(wd > 0);
                if (rs < RPP) {
                    tab[buf][rs][slot] = make_int2(st, wd);
                    if (slot == 0) word[buf][rs] = make_uint4((unsigned)((some >> (tid & 48)) & 0xffffull), 0u, 0u, 0u);
                }
            }
        }
        __syncthreads();
        // 3. mask and store
        if (one) {
            if (lane < CV) {
                uint4 w[UNR];
#pragma unroll
                for (int k = 0; k < UNR; ++k) w[k] = word[buf][k * RPB + sub];
#pragma unroll
                for (int k = 0; k < UNR; ++k) {
                    const int rs = k * RPB + sub;
                    const long long r = r0 + rs;
                    if (r >= nrows) break;
                    V val = v[k];
                    if (w[k].x | w[k].y | w[k].z) {
#pragma unroll
                        for (int e = 0; e < EPV; ++e)
                            if (masked(w[k], tab[BITS ? 0 : buf][BITS ? 0 : rs], blk[e], bin[e])) SpecVec<V>::at(val, e) = a.fill;
                    }
                    reinterpret_cast<V *>(out + r * ldo)[lane] = val;
                }
            }
        } else {                                 // rows wider than the workgroup: LPR = 256, RPB = 1
            for (int k = 0; k < UNR; ++k) {
                const int rs = k * RPB + sub;
                const long long r = r0 + rs;
                if (r >= nrows) break;
                const uint4 w = word[buf][rs];
                const bool hit = (w.x | w.y | w.z) != 0;
                const V *src = reinterpret_cast<const V *>(x + r * ldx);
                V *dst = reinterpret_cast<V *>(out + r * ldo);
                for (int q = lane; q < CV; q += LPR) {
                    V val = src[q];
                    if (hit) {
#pragma unroll
                        for (int e = 0; e < EPV; ++e) {
                            const int c = q * EPV + e, bk = c / a.base, bn = (c - bk * a.base) % a.F;
                            if (masked(w, tab[BITS ? 0 : buf][BITS ? 0 : rs], bk, bn)) SpecVec<V>::at(val, e) = a.fill;
                        }
                    }
                    dst[q] = val;
                }
            }
        }
    }
}

template <typename V, bool BITS>
void launch_spec_augment(const float *x, int ldx, long long nrows, int B, int CV, const int *seq_len, const SpecArgs &a,
                         float *out, int ldo, int *plan, hipStream_t s)
{
    // lanes per row: the power of two that covers the row's vectors, 16 .. 256 (16 threads per row build its masks); 4 rows
    // per lane and pass
    const int lpr = rs_lanes_cover(CV, 16, 256);
    const dim3 grid(rs_grid(nrows, (256 / lpr) * 4)), block(256);
    rs_dispatch_lanes<16, 256>(lpr, [&](auto L) {
        hipLaunchKernelGGL((spec_augment_kernel<V, decltype(L)::value, BITS>), grid, block, 0, s, x, (long long)ldx, nrows, B, CV,
                           seq_len, a, out, (long long)ldo, plan);
    });
}

}  // namespace

extern "C" int lc_spec_augment(const float *x, int T, int B, int D, int ldx, const int *seq_len, const lc_spec_augment_t *cfg,
                               uint32_t seed, float *out, int ldo, int *plan, lc_stream_t stream)
{
    LC_CHECK_ARG(x && seq_len && cfg && out, "lc_spec_augment: null pointer");
    LC_CHECK_ARG(T > 0 && B > 0 && D > 0 && ldx >= D && ldo >= D, "lc_spec_augment: bad shape (T %d, B %d, D %d, ldx %d, ldo %d)",
                 T, B, D, ldx, ldo);
    LC_CHECK_ARG(cfg->time_masks >= 0 && cfg->time_masks <= 8 && cfg->freq_masks >= 0 && cfg->freq_masks <= 8,
                 "lc_spec_augment: mask counts must lie in 0..8 (time %d, freq %d)", cfg->time_masks, cfg->freq_masks);
    LC_CHECK_ARG(cfg->time_width >= 0 && cfg->freq_width >= 0, "lc_spec_augment: negative mask width");
    LC_CHECK_ARG(cfg->time_percent >= 0 && cfg->time_percent <= 100, "lc_spec_augment: time_percent %d outside 0..100",
                 cfg->time_percent);
    LC_CHECK_ARG(cfg->freq_bins > 0 && cfg->base_dim > 0 && cfg->base_dim % cfg->freq_bins == 0,
                 "lc_spec_augment: freq_bins %d must be positive and divide base_dim %d", cfg->freq_bins, cfg->base_dim);
    LC_CHECK_ARG(cfg->freq_width <= cfg->freq_bins, "lc_spec_augment: freq_width %d above freq_bins %d", cfg->freq_width,
                 cfg->freq_bins);
    LC_CHECK_ARG(cfg->left_context >= 0 && cfg->right_context >= 0 && cfg->subsample >= 0,
                 "lc_spec_augment: negative context or subsample");
    LC_CHECK_ARG((long long)cfg->base_dim * (1ll + cfg->left_context + cfg->right_context) == D,
                 "lc_spec_augment: D %d is not base_dim %d * (1 + %d + %d)", D, cfg->base_dim, cfg->left_context,
                 cfg->right_context);
    LC_CHECK_ARG(isfinite(cfg->fill), "lc_spec_augment: fill must be finite");
    SpecArgs a;
    a.tm = cfg->time_masks; a.tw = cfg->time_width; a.tp = cfg->time_percent;
    a.fm = cfg->freq_masks; a.fw = cfg->freq_width; a.F = cfg->freq_bins;
    a.base = cfg->base_dim; a.l = cfg->left_context; a.s = cfg->subsample > 1 ? cfg->subsample : 1;
    a.nb = 1 + cfg->left_context + cfg->right_context;
    a.fill = cfg->fill; a.seed = seed;
    const long long nrows = (long long)T * B;
    const bool vec = rs_vec16(D, {ldx, ldo}, {x, out});
    const bool bits = a.nb <= 32 && a.F <= 64;          // a row's masks fit one LDS word: a bit per block, a bit per bin
    hipStream_t s = (hipStream_t)stream;
    if (vec && bits) launch_spec_augment<float4, true>(x, ldx, nrows, B, D / 4, seq_len, a, out, ldo, plan, s);
    else if (vec) launch_spec_augment<float4, false>(x, ldx, nrows, B, D / 4, seq_len, a, out, ldo, plan, s);
    else if (bits) launch_spec_augment<float, true>(x, ldx, nrows, B, D, seq_len, a, out, ldo, plan, s);
    else launch_spec_augment<float, false>(x, ldx, nrows, B, D, seq_len, a, out, ldo, plan, s);
    LC_CHECK_LAUNCH("spec_augment");
    return LC_OK;
}
