// gemm_dispatch_dump.cpp - the host-side dispatch of csrc/gemm.hip, run without a device: every kernel launch is replaced
// by a recorder that prints the kernel expression, the grid and the argument block.  tests/test_gemm_dispatch_host.py
// builds this file (host only, together with error.cpp) against the tree's gemm.hip and compares the output with
// tests/golden/gemm_dispatch.txt, byte for byte.  With `--sweep SEED DRAWS` the same recorder runs over seeded random
// entries, shapes, alignments, workspaces, epilogues and options instead of the fixed list (compare two builds' outputs).
//
// No pointer is ever dereferenced: the operands are fixed fake addresses.  hipGetDevice is made to fail so that
// lc_num_cus() takes its 256-CU default on every machine, and the device is never opened.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

template <class... T> static void lc_record(const char *kernel, dim3 grid, dim3 block, const T &...args);
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, shmem, stream, ...) lc_record(#kernel, dim3(grid), dim3(block), __VA_ARGS__)
#define hipGetLastError() hipSuccess
#define hipGetDevice(p) hipErrorNoDevice

#include "gemm.hip"

static void print_epi(const EpiArgs &e)
{
    printf(" epi{keep=%.9g inv_keep=%.9g seed=%u stream0=%u P=%d c16=%p ldc16=%d row0=%d col0=%d skip_c=%d}", e.keep, e.inv_keep,
           e.seed, e.stream0, e.P, (void *)e.c16, e.ldc16, e.row0, e.col0, e.skip_c);
}
// (fields no kernel of the launch reads are left unset by some entries and not printed: the fp32 second pair - A2, B2, k1 - of
// an SGemmArgs' inner block, and the bf16 second pair outside the SEG2 form)
static void print_args(const GemmArgs &g, bool f32_operands)
{
    printf(" M=%d N=%d K=%d alpha=%.9g beta=%.9g A=%p lda=%d B=%p ldb=%d C=%p ldc=%d bias=%p vecA=%d vecB=%d kchunk=%d slab=%p"
           " slab_slice=%zu slab_ld=%d",
           g.M, g.N, g.K, g.alpha, g.beta, (const void *)g.A, g.lda, (const void *)g.B, g.ldb, (void *)g.C, g.ldc,
           (const void *)g.bias, g.vecA, g.vecB, g.kchunk, (void *)g.slab, g.slab_slice, g.slab_ld);
    if (f32_operands) printf(" A2=%p B2=%p k1=%d", (const void *)g.A2, (const void *)g.B2, g.k1);
    print_epi(g.epi);
}
static void print_launch(const GemmArgs &g) { print_args(g, true); }
static bool g_seg2;      // the launch under the recorder is gemm_bf16g_kernel's SEG2 form: the only reader of an SGemmArgs' second pair
static void print_launch(const SGemmArgs &s)
{
    print_args(s.g, false);
    printf(" sA=%p sB=%p", (const void *)s.A, (const void *)s.B);
    if (g_seg2) printf(" sA2=%p sB2=%p sk1=%d", (const void *)s.A2, (const void *)s.B2, s.k1);
}
static void print_reduce(const float *slab, int nslices, int M, int N, float alpha, float beta, float *C, int ldc, const float *bias)
{
    printf(" slab=%p nslices=%d M=%d N=%d alpha=%.9g beta=%.9g C=%p ldc=%d bias=%p", (const void *)slab, nslices, M, N, alpha, beta,
           (void *)C, ldc, (const void *)bias);
}
template <class... T> static void print_launch(const T &...args)
{
    if constexpr (sizeof...(T) == 9) print_reduce(args...);      // splitk_reduce_kernel; the cast kernels take 6 and 8
    else printf(" (not a product kernel)");
}

template <class... T> static void lc_record(const char *kernel, dim3 grid, dim3 block, const T &...args)
{
    printf("  launch %s grid=(%u,%u,%u) block=(%u,%u,%u)", kernel, grid.x, grid.y, grid.z, block.x, block.y, block.z);
    g_seg2 = strstr(kernel, "gemm_bf16g_kernel<false, false, false, true>") != nullptr;
    print_launch(args...);
    printf("\n");
}

// ---- one call ----------------------------------------------------------------------------------------------------------
enum Entry { F32, BF16, F32_NT2, BF16_NT, BF16_NT2, BF16_TN, BF16_NN, N_ENTRIES };
static const char *const ENTRY_NAME[] = {"lc_gemm_f32", "lc_gemm_bf16", "lc_gemm_f32_nt2", "lc_gemm_bf16_nt", "lc_gemm_bf16_nt2",
                                         "lc_gemm_bf16_tn", "lc_gemm_bf16_nn"};
static const char *const OPTIONS[] = {"gemm_f32_big", "gemm_bf16_big", "gemm_bf16_persist", "gemm_tail"};

// fake device addresses, 256-byte aligned and far apart
static const uintptr_t ADDR_A = 0x100000000000ull, ADDR_B = 0x200000000000ull, ADDR_C = 0x300000000000ull,
                       ADDR_BIAS = 0x400000000000ull, ADDR_WS = 0x500000000000ull, ADDR_A2 = 0x600000000000ull,
                       ADDR_B2 = 0x700000000000ull, ADDR_SHADOW = 0x800000000000ull;

struct Call {
    Entry entry = F32;
    int ta = 0, tb = 0, M = 0, N = 0, K = 0, K2 = 0;
    int lda = -1, ldb = -1, ldc = -1;                  // -1: the smallest valid one
    float alpha = 1.f, beta = 0.f;
    bool bias = false;
    int offA = 0, offB = 0;                            // bytes added to the operand addresses
    long long ws_bytes = -1;                           // -1: lc_gemm_workspace_bytes(M, N, K); -2: NULL; else this many bytes
    bool epi = false;                                  // arm lc_gemm_next_epilogue
    lc_gemm_epilogue_t e = {0.75f, 1234u, 7u, 320, (uint16_t *)ADDR_SHADOW, 0, 0};
    long opt[4] = {LC_OPTION_UNSET, LC_OPTION_UNSET, LC_OPTION_UNSET, LC_OPTION_UNSET};
};

static void run(const Call &c)
{
    const bool two = c.entry == F32_NT2 || c.entry == BF16_NT2;
    const bool kmajorA = c.entry == BF16_TN || ((c.entry == F32 || c.entry == BF16) && c.ta);
    const bool kmajorB = c.entry == BF16_TN || c.entry == BF16_NN || ((c.entry == F32 || c.entry == BF16) && !c.tb);
    const int kmax = two && c.K2 > c.K ? c.K2 : c.K;
    const int lda = c.lda >= 0 ? c.lda : (kmajorA ? c.M : kmax);
    const int ldb = c.ldb >= 0 ? c.ldb : (kmajorB ? c.N : kmax);
    const int ldc = c.ldc >= 0 ? c.ldc : c.N;
    const size_t ws_bytes = c.ws_bytes == -1 ? lc_gemm_workspace_bytes(c.M, c.N, c.K) : c.ws_bytes == -2 ? 0 : (size_t)c.ws_bytes;
    void *ws = c.ws_bytes == -2 ? nullptr : (void *)ADDR_WS;
    void *A = (void *)(ADDR_A + c.offA), *B = (void *)(ADDR_B + c.offB), *A2 = (void *)ADDR_A2, *B2 = (void *)ADDR_B2;
    float *C = (float *)ADDR_C;
    const float *bias = c.bias ? (const float *)ADDR_BIAS : nullptr;

    printf("%s(ta=%d tb=%d M=%d N=%d K=%d K2=%d alpha=%.9g A=%p lda=%d B=%p ldb=%d beta=%.9g C=%p ldc=%d bias=%p ws=%p"
           " ws_bytes=%zu)",
           ENTRY_NAME[c.entry], c.ta, c.tb, c.M, c.N, c.K, c.K2, c.alpha, A, lda, B, ldb, c.beta, (void *)C, ldc, (const void *)bias,
           ws, ws_bytes);
    for (int i = 0; i < 4; ++i) {
        lc_set_option(OPTIONS[i], c.opt[i]);
        if (c.opt[i] != LC_OPTION_UNSET) printf(" %s=%ld", OPTIONS[i], c.opt[i]);
    }
    lc_set_error("%s", "");
    if (c.epi) {
        lc_gemm_epilogue_t e = c.e;
        if (e.c_bf16 && e.ldc_bf16 == 0) e.ldc_bf16 = c.N + 8;
        printf(" epilogue{keep=%.9g seed=%u stream0=%u drop_width=%d c_bf16=%p ldc_bf16=%d shadow_only=%d}", e.keep, e.seed,
               e.stream0, e.drop_width, (void *)e.c_bf16, e.ldc_bf16, e.shadow_only);
        const int rc = lc_gemm_next_epilogue(&e);
        if (rc != LC_OK) printf(" (epilogue refused: %d \"%s\")", rc, lc_last_error());
    }
    printf("\n");
    int rc = 0;
    switch (c.entry) {
    case F32:
        rc = lc_gemm_f32(c.ta, c.tb, c.M, c.N, c.K, c.alpha, (const float *)A, lda, (const float *)B, ldb, c.beta, C, ldc, bias, ws,
                         ws_bytes, nullptr);
        break;
    case BF16:
        rc = lc_gemm_bf16(c.ta, c.tb, c.M, c.N, c.K, c.alpha, (const float *)A, lda, (const float *)B, ldb, c.beta, C, ldc, bias, ws,
                          ws_bytes, nullptr);
        break;
    case F32_NT2:
        rc = lc_gemm_f32_nt2(c.M, c.N, c.K, c.K2, c.alpha, (const float *)A, (const float *)A2, lda, (const float *)B,
                             (const float *)B2, ldb, c.beta, C, ldc, bias, nullptr);
        break;
    case BF16_NT:
        rc = lc_gemm_bf16_nt(c.M, c.N, c.K, c.alpha, (const uint16_t *)A, lda, (const uint16_t *)B, ldb, c.beta, C, ldc, bias, ws,
                             ws_bytes, nullptr);
        break;
    case BF16_NT2:
        rc = lc_gemm_bf16_nt2(c.M, c.N, c.K, c.K2, c.alpha, (const uint16_t *)A, (const uint16_t *)A2, lda, (const uint16_t *)B,
                              (const uint16_t *)B2, ldb, c.beta, C, ldc, bias, nullptr);
        break;
    case BF16_TN:
        rc = lc_gemm_bf16_tn(c.M, c.N, c.K, c.alpha, (const uint16_t *)A, lda, (const uint16_t *)B, ldb, c.beta, C, ldc, bias, ws,
                             ws_bytes, nullptr);
        break;
    case BF16_NN:
        rc = lc_gemm_bf16_nn(c.M, c.N, c.K, c.alpha, (const uint16_t *)A, lda, (const uint16_t *)B, ldb, c.beta, C, ldc, bias, ws,
                             ws_bytes, nullptr);
        break;
    default: break;
    }
    printf("  -> rc=%d error=\"%s\"\n", rc, lc_last_error());
    lc_gemm_next_epilogue(nullptr);
}

static Call call(Entry entry, int M, int N, int K, int ta = 0, int tb = 0)
{
    Call c;
    c.entry = entry; c.M = M; c.N = N; c.K = K; c.ta = ta; c.tb = tb;
    return c;
}
static size_t slab_bytes(int slices, int M, int N) { return (size_t)slices * M * N * sizeof(float); }

// ---- the fixed list ----------------------------------------------------------------------------------------------------
static void fixed_list()
{
    static const int shapes[][3] = {{5, 3, 7},          {257, 131, 70},      {128, 128, 16},     {300, 300, 64},
                                    {2100, 2100, 64},   {320, 320, 32000},   {1024, 1024, 64000}, {63936, 2048, 4096},
                                    {64000, 4100, 2048}, {1000, 1280, 40}};
    for (int bf16 = 0; bf16 < 2; ++bf16)                     // lc_gemm_f32: every shape; lc_gemm_bf16: the peeled and the split one
        for (int t = 0; t < 4; ++t)
            for (const auto &s : shapes) {
                if (bf16 && !(s[0] == 2100 || s[0] == 320 || s[0] == 1024)) continue;
                run(call(bf16 ? BF16 : F32, s[0], s[1], s[2], t >> 1, t & 1));
            }
    for (int t = 0; t < 4; ++t) {
        const int ta = t >> 1, tb = t & 1;
        Call c = call(F32, 2304, 2304, 64, ta, tb);            // an operand 4 bytes off alignment: no vector loads, no big kernel
        c.offA = 4; run(c);
        c.offA = 0; c.offB = 4; run(c);
        c = call(F32, 63936, 2100, 4096, ta, tb);             // ... of a strip only: the strips' own vec re-check
        c.lda = ta ? 63940 : 4096; c.ldb = tb ? 4096 : 2100;
        run(c);
        for (int big = 0; big < 2; ++big) {                   // the split of the big and of the small path, without its slab
            c = big ? call(F32, 1024, 1024, 64000, ta, tb) : call(F32, 320, 320, 32000, ta, tb);
            c.ws_bytes = -2; run(c);                                                   // NULL
            c.ws_bytes = 0; run(c);                                                    // a pointer, no bytes
            const int big_slices = pick_splitk_big(c.M, c.N, c.K, FGBK), small_slices = pick_splitk(c.M, c.N, c.K);
            c.ws_bytes = slab_bytes(big ? big_slices : small_slices, c.M, c.N) - 1; run(c);      // one byte too small
            c.ws_bytes += 1; run(c);
            if (big) { c.ws_bytes = slab_bytes(small_slices, c.M, c.N) - 1; run(c); }  // ... for the small path's count as well
        }
        for (const auto &s : shapes) {                        // beta and bias
            if (s[0] == 5 || s[0] == 128 || s[0] == 1000) continue;
            c = call(F32, s[0], s[1], s[2], ta, tb);
            c.alpha = 0.5f; c.beta = 1.f; c.bias = true;
            run(c);
        }
        for (int shadow = 0; shadow < 2; ++shadow) {          // an armed epilogue: no split; strips carry their block's origin
            static const int eshapes[][3] = {{320, 320, 32000}, {1024, 1024, 64000}, {2100, 2100, 64}, {63936, 2100, 4096},
                                             {64000, 4100, 2048}, {300, 300, 64}};
            for (const auto &s : eshapes) {
                c = call(F32, s[0], s[1], s[2], ta, tb);
                c.epi = true; c.bias = true;
                if (!shadow) c.e.c_bf16 = nullptr;
                else { c.e.keep = 1.f; c.e.shadow_only = 1; }
                run(c);
            }
        }
        static const int bshapes[][3] = {{2100, 2100, 64}, {1024, 1024, 64000}, {63936, 2048, 4096}, {64000, 4100, 2048}};
        for (const auto &s : bshapes) {                       // gemm_f32_big = 0
            c = call(F32, s[0], s[1], s[2], ta, tb);
            c.opt[0] = 0; run(c);
        }
        c = call(F32, 256, 512, 64, ta, tb);                  // gemm_f32_big = 2 takes the big kernel below half a chip
        run(c);
        c.opt[0] = 2; run(c);
        c = call(F32, 300, 600, 64, ta, tb); c.opt[0] = 2; run(c);
        static const int tshapes[][3] = {{64000, 4096, 2048}, {32000, 1280, 64}, {63936, 2048, 4096}};
        for (const auto &s : tshapes) {                       // gemm_tail = 1: whole rounds, the rest as a bottom strip
            c = call(F32, s[0], s[1], s[2], ta, tb);
            c.opt[3] = 1; run(c);
        }
        run(call(F32, 0, 128, 64, ta, tb));                   // empty, and the argument checks in their order
        run(call(F32, 128, 0, 64, ta, tb));
        run(call(F32, 128, 128, 0, ta, tb));
        c = call(F32, 128, 128, 64, ta, tb); c.lda = (ta ? 128 : 64) - 1; run(c);
        c = call(F32, 128, 128, 64, ta, tb); c.ldb = (tb ? 64 : 128) - 1; run(c);
        c = call(F32, 128, 128, 64, ta, tb); c.ldc = 127; run(c);
        c = call(F32, 128, -1, 64, ta, tb); run(c);
    }
    {
        Call c = call(BF16, 2100, 2100, 64, 0, 1);
        c.epi = true; run(c);
        c = call(BF16, 1024, 1024, 64000, 1, 0); c.ws_bytes = -2; run(c);
    }

    // lc_gemm_f32_nt2
    {
        Call c = call(F32_NT2, 64000, 2048, 1024); c.K2 = 1024; run(c);
        c.beta = 1.f; c.bias = true; run(c);
        c = call(F32_NT2, 63936, 2100, 1024); c.K2 = 512; c.lda = c.ldb = 1024; run(c);
        c.beta = 1.f; c.bias = true; run(c);
        c.epi = true; run(c);                                 // the strips: beta / bias first, the epilogue's block second
        c.e.c_bf16 = nullptr; run(c);
        c = call(F32_NT2, 300, 200, 64); c.K2 = 32; run(c);   // the two products in sequence
        c.epi = true; c.bias = true; run(c);
        c = call(F32_NT2, 64000, 2048, 1024); c.K2 = 1000; run(c);       // K2 % 32 != 0
        c = call(F32_NT2, 64000, 2048, 1024); c.K2 = 1024; c.offA = 4; run(c);
        c = call(F32_NT2, 64000, 2048, 1024); c.K2 = 1024; c.opt[0] = 0; run(c);
        c = call(F32_NT2, 512, 512, 64); c.K2 = 64; run(c);
        c.opt[0] = 2; run(c);
        c = call(F32_NT2, 512, 512, 64); c.K2 = 0; run(c);
        c = call(F32_NT2, 512, 512, 64); c.K2 = 64; c.lda = 32; run(c);
        c = call(F32_NT2, 0, 512, 64); c.K2 = 64; run(c);
    }

    // lc_gemm_bf16_nt
    {
        static const int shapes[][3] = {{64000, 4096, 2048}, {63936, 2048, 4096}, {1024, 1024, 64000}, {300, 200, 128},
                                        {257, 131, 72},      {64, 44, 2048},      {2100, 2100, 64},    {64000, 4100, 2048},
                                        {320, 320, 32000},   {63936, 2100, 4096}};
        for (const auto &s : shapes) run(call(BF16_NT, s[0], s[1], s[2]));
        Call c = call(BF16_NT, 1024, 1024, 64000);
        c.ws_bytes = -2; run(c);
        c.ws_bytes = slab_bytes(pick_splitk_big(c.M, c.N, c.K), c.M, c.N) - 1; run(c);
        c.ws_bytes = slab_bytes(pick_splitk(c.M, c.N, c.K), c.M, c.N) - 1; run(c);
        c = call(BF16_NT, 320, 320, 32000); c.ws_bytes = -2; run(c);
        for (const auto &s : shapes) {
            c = call(BF16_NT, s[0], s[1], s[2]);
            c.alpha = 2.f; c.beta = 1.f; c.bias = true; run(c);
            c.epi = true; run(c);
            c.opt[1] = 0; run(c);                             // gemm_bf16_big = 0
            c.epi = false; run(c);
        }
        c = call(BF16_NT, 64000, 4096, 2048); c.opt[2] = 1; run(c);      // gemm_bf16_persist = 1: 4000 tiles, K % 128 == 0
        c = call(BF16_NT, 64000, 4096, 2112); c.opt[2] = 1; run(c);      // ... K % 128 != 0: no walk
        c = call(BF16_NT, 1024, 1024, 64000); c.opt[2] = 1; run(c);      // ... split: no walk
        c = call(BF16_NT, 64000, 4096, 2048); c.opt[3] = 1; run(c);      // gemm_tail = 1
        c = call(BF16_NT, 63936, 2100, 4096); c.opt[3] = 1; run(c);
        c = call(BF16_NT, 256, 256, 60); run(c);                         // K not a multiple of 8
        c = call(BF16_NT, 256, 256, 64); c.offA = 8; run(c);
        c = call(BF16_NT, 256, 256, 64); c.lda = 56; run(c);
        c = call(BF16_NT, 0, 256, 64); run(c);
        c = call(BF16_NT, 256, 256, 0); run(c);
        c = call(BF16_NT, 300, 200, 0); run(c);
    }

    // lc_gemm_bf16_nt2
    {
        Call c = call(BF16_NT2, 64000, 2048, 1024); c.K2 = 1024; run(c);
        c.alpha = 2.f; c.beta = 1.f; c.bias = true; c.epi = true; run(c);
        c = call(BF16_NT2, 63936, 2100, 1024); c.K2 = 512; run(c);
        c.alpha = 2.f; c.beta = 1.f; c.bias = true; c.epi = true; run(c);      // strips in two launches: the hand-over
        c.e.keep = 1.f; c.e.shadow_only = 1; run(c);
        c = call(BF16_NT2, 300, 200, 128); c.K2 = 64; c.beta = 1.f; c.bias = true; c.epi = true; run(c);     // !big_ok
        c = call(BF16_NT2, 64000, 2048, 1024); c.K2 = 1000; run(c);
        c = call(BF16_NT2, 64000, 2048, 1024); c.K2 = 1024; c.opt[1] = 0; c.epi = true; run(c);
        c = call(BF16_NT2, 64000, 2048, 1024); c.K2 = 1024; c.opt[2] = 1; c.opt[3] = 1; run(c);
        c = call(BF16_NT2, 512, 512, 64); c.K2 = 0; run(c);
        c = call(BF16_NT2, 512, 512, 64); c.K2 = 60; run(c);
        c = call(BF16_NT2, 512, 512, 60); c.K2 = 64; run(c);
    }

    // lc_gemm_bf16_tn / _nn
    for (int nn = 0; nn < 2; ++nn) {
        const Entry e = nn ? BF16_NN : BF16_TN;
        run(call(e, 256, 256, 64));
        run(call(e, 256, 1024, 4100));                        // nn: K % 64 != 0
        run(call(e, 1024, 512, 8192));                        // split
        run(call(e, 4096, 2048, 64000));
        Call c = call(e, 1024, 512, 8192);
        c.ws_bytes = -2; run(c);
        c.ws_bytes = slab_bytes(pick_splitk_big(c.M, c.N, c.K), c.M, c.N) - 1; run(c);
        c = call(e, 1024, 512, 8192); c.alpha = 0.5f; c.beta = 1.f; c.bias = true; run(c);
        c.epi = true; run(c);                                 // an armed epilogue: no split
        c = call(e, 4096, 8192, 4096); c.opt[2] = 1; run(c);             // persist: 512 tiles, unsplit
        c = call(e, 4096, 8192, 4160); c.opt[2] = 1; run(c);             // ... an odd number of k tiles: no walk
        c = call(e, 1024, 512, 8192); c.opt[2] = 1; run(c);              // ... split: no walk
        run(call(e, 300, 256, 64));                           // M % 256 != 0
        run(call(e, 256, 0, 64));
        c = call(e, 256, 256, 64); c.lda = 60; run(c);
        c = call(e, 256, 256, 64); c.ldb = 260; run(c);
        c = call(e, 256, 256, 64); c.offB = 2; run(c);
        c = call(e, 256, 256, 1 << 22); c.ldb = 512; c.ws_bytes = -2; run(c);      // unsplit, 4 GB of B: operand too large
    }
}

// ---- the seeded sweep --------------------------------------------------------------------------------------------------
static uint64_t g_rng;
static uint32_t rnd()
{
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_rng >> 33);
}
static int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }
static int pick(const int *v, int n) { return v[rnd() % n]; }
static int rnd_extent(int max_tiles)        // biased towards multiples of 128 / 256, +- 1
{
    static const int small[] = {0, 1, 5, 44, 64, 100, 127, 131, 200, 300, 320};
    const int r = rnd() % 10;
    if (r == 0) return pick(small, 11);
    const int unit = (rnd() & 1) ? 128 : 256;
    const int tiles = (rnd() & 1) ? rnd_in(1, max_tiles) : rnd_in(1, 20);
    const int d = rnd() % 5;
    return unit * tiles + (d == 0 ? -1 : d == 1 ? 1 : d == 2 ? rnd_in(-130, 130) : 0);
}
static int rnd_depth()                      // around 4096, some tall, some tiny and odd
{
    static const int some[] = {0, 7, 16, 32, 40, 64, 70, 72, 96, 128, 1000, 1024, 2048, 4032, 4064, 4088, 4095, 4096, 4097, 4104, 4128,
                               4160, 8192, 12288, 32000, 64000, 64064};
    if (rnd() % 3) return pick(some, 27);
    return rnd_in(1, 160) * ((rnd() & 1) ? 64 : 8);
}
static void sweep(uint64_t seed, long draws)
{
    g_rng = seed;
    for (long i = 0; i < draws; ++i) {
        Call c;
        c.entry = (Entry)(rnd() % N_ENTRIES);
        c.ta = rnd() & 1; c.tb = rnd() & 1;
        const bool kmajor = c.entry == BF16_TN || c.entry == BF16_NN;
        c.M = kmajor && rnd() % 8 ? 256 * rnd_in(1, 24) : rnd_extent(250);
        c.N = kmajor && rnd() % 8 ? 256 * rnd_in(1, 24) : rnd_extent(17);
        // tidy (5 of 6): depths, paddings and offsets the bf16 entries accept (multiples of 8 elements, 16 bytes)
        const bool tidy = rnd() % 6 != 0;
        const int kunit = !tidy ? 1 : c.entry == BF16_NN ? 64 : 8;
        c.K = (rnd_depth() + kunit - 1) / kunit * kunit;
        c.K2 = (rnd_depth() + kunit - 1) / kunit * kunit;
        if (rnd() % 4 == 0) { c.alpha = 0.5f; c.beta = (rnd() & 1) ? 1.f : 0.25f; }
        c.bias = rnd() & 1;
        if (rnd() % 8 == 0) c.offA = tidy ? 16 : 4 << (rnd() % 3);
        if (rnd() % 8 == 0) c.offB = tidy ? 16 : 4 << (rnd() % 3);
        for (int *ld : {&c.lda, &c.ldb, &c.ldc}) {             // leading dimensions: the smallest, padded, or (rarely) too small
            const int r = rnd() % 8, pad[] = {8, 24, 64, 256, 1, 2, 4};
            if (r < 3) *ld = -1 - pick(pad, tidy ? 4 : 7);     // resolved below
            else if (r == 3 && rnd() % 8 == 0) *ld = -100;
        }
        {
            const bool two = c.entry == F32_NT2 || c.entry == BF16_NT2;
            const bool kmajorA = c.entry == BF16_TN || ((c.entry == F32 || c.entry == BF16) && c.ta);
            const bool kmajorB = kmajor || ((c.entry == F32 || c.entry == BF16) && !c.tb);
            const int kmax = two && c.K2 > c.K ? c.K2 : c.K;
            const int least[] = {kmajorA ? c.M : kmax, kmajorB ? c.N : kmax, c.N};
            int *lds[] = {&c.lda, &c.ldb, &c.ldc};
            for (int j = 0; j < 3; ++j) {
                if (*lds[j] == -100) *lds[j] = least[j] > 0 ? least[j] - 1 : 0;
                else if (*lds[j] < -1) *lds[j] = least[j] + (-1 - *lds[j]);
            }
        }
        switch (rnd() % 8) {                                   // workspace: what the library asks for, NULL, empty, a byte short
        case 0: c.ws_bytes = -2; break;
        case 1: c.ws_bytes = 0; break;
        case 2: c.ws_bytes = (long long)slab_bytes(pick_splitk(c.M, c.N, c.K), c.M, c.N) - 1; break;
        case 3: c.ws_bytes = (long long)slab_bytes(pick_splitk_big(c.M, c.N, c.K), c.M, c.N) - 1; break;
        case 4: c.ws_bytes = (long long)slab_bytes(pick_splitk_big(c.M, c.N, c.K, FGBK), c.M, c.N) - 1; break;
        default: break;
        }
        if (rnd() % 3 == 0) {
            c.epi = true;
            const int r = rnd() % 4;
            if (r == 0) c.e.c_bf16 = nullptr;
            else if (r == 1) c.e.keep = 1.f;
            else if (r == 2) { c.e.keep = 1.f; c.e.shadow_only = 1; }
            c.e.drop_width = (rnd() & 1) ? 320 : 1024;
        }
        if (rnd() % 4 == 0) c.opt[0] = rnd() % 3;
        if (rnd() % 6 == 0) c.opt[1] = rnd() % 2;
        if (rnd() % 4 == 0) c.opt[2] = rnd() % 2;
        if (rnd() % 3 == 0) c.opt[3] = rnd() % 2;
        run(c);
    }
}

int main(int argc, char **argv)
{
    if (argc == 4 && strcmp(argv[1], "--sweep") == 0) sweep(strtoull(argv[2], nullptr, 10), atol(argv[3]));
    else fixed_list();
    return 0;
}
