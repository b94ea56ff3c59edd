// lstm_dispatch_dump.cpp - the host-side dispatch of csrc/lstm.hip (everything from `al256` down), run without a device:
// every HIP call the dispatch makes is replaced by a function of this program, and the ones that carry information print a
// line.  tests/test_lstm_dispatch_host.py builds this file (host only, together with error.cpp) against the tree's lstm.hip,
// runs it once per set of fake-device answers and compares the output with tests/golden/lstm_dispatch.txt, byte for byte.
//
//   lstm_dispatch_dump ARCH CUS XCCS FLAT_PRIO CALLER_PRIO ATTR_FAILS MEMSET_FAILS [--full | --sweep SEED DRAWS | --plan]
//
// The seven answers are what the fake device reports (persist_device_ok() and dir_streams() cache per process, hence one
// process per answer set).  Without a mode the fixed list runs (`--full`: every record whole, none as a digest); `--sweep` runs seeded random draws instead (compare two
// builds' outputs); `--plan` reads `entry pass T B N ndir persistent` lines from stdin, makes each call silently and prints
// lc_debug_last_lstm_schedule() after it.
//
// A kernel is named by what it is: the program defines the registration functions the host object calls at start-up
// itself, keeps the (stub address -> mangled device name) map they deliver, and prints that name for a launch.  The HIP
// runtime is never entered and no pointer is ever dereferenced: the operands are fixed fake addresses.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>

// Everything a call prints is gathered into its record first.  A record is then printed whole or, for the parts of the fixed
// list that repeat the same launches with one input changed, as its first line (the entry and its arguments), the result
// and a 64-bit FNV-1a digest of the whole text: `--full` prints those whole too, to compare two builds line by line.
extern "C" int lc_debug_last_lstm_schedule(void);
static bool g_quiet, g_in_call, g_whole = true, g_always_whole;
static std::string g_record;
__attribute__((format(printf, 1, 2))) static void out(const char *fmt, ...)
{
    if (g_quiet) return;
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (g_in_call) g_record += buf;
    else fputs(buf, stdout);
}
// Joins what is printed next onto the record's last line if that line begins with `prefix` (runs of memsets, of repeated steps).
static bool join_last_line(const char *prefix)
{
    if (!g_in_call || g_quiet || g_record.size() < 2) return false;
    const size_t at = g_record.rfind('\n', g_record.size() - 2) + 1;
    if (g_record.compare(at, strlen(prefix), prefix) != 0) return false;
    g_record.pop_back();
    return true;
}
static void end_record(int rc)
{
    g_in_call = false;
    if (g_quiet) return;
    if (g_whole || g_always_whole) { fputs(g_record.c_str(), stdout); return; }
    unsigned long long h = 0xcbf29ce484222325ull;
    int lines = 0;
    for (unsigned char ch : g_record) { h = (h ^ ch) * 0x100000001b3ull; lines += ch == '\n'; }
    printf("%.*s -> rc=%d schedule=0x%x lines=%d record=%016llx\n", (int)g_record.find('\n'), g_record.c_str(), rc,
           (unsigned)lc_debug_last_lstm_schedule(), lines, h);
}

static const uintptr_t ADDR_SEQ = 0xc00000000000ull, ADDR_WS = 0xd00000000000ull, ADDR_STAMPS = 0xe00000000000ull,
                       ADDR_STREAM = 0xf00000000000ull;
// Fake addresses print as what they stand for: lane (bits 44 up), direction (bits 36 .. 43), byte offset; NULL as 0.
static const char *sym(const void *p)
{
    static const char *const lane[16] = {"?",  "zx", "R",  "wf",    "wi",    "wo",  "cs", "hs",
                                         "sh", "dh", "dpeep", "dbias", "seq", "ws",  "dbg", "s"};
    static char ring[32][40];
    static int next;
    if (!p) return "0";
    char *b = ring[next++ & 31];
    const unsigned long long a = (unsigned long long)(uintptr_t)p, off = a & 0xfffffffffull;
    if (off) snprintf(b, 40, "%s%llu+%llu", lane[(a >> 44) & 15], (a >> 36) & 0xff, off);
    else snprintf(b, 40, "%s%llu", lane[(a >> 44) & 15], (a >> 36) & 0xff);
    return b;
}

// ---- the fake device ---------------------------------------------------------------------------------------------------
static struct {
    const char *arch = "gfx950:sramecc+:xnack-";
    int cus = 256, xccs = 8, flat_prio = 0, caller_prio = 0, attr_fails = 0, memset_fails = 0;
} g_fake;

static struct { const void *stub; const char *name; } g_kernels[256];      // filled before main() by the module constructor
static int g_nkernels;
extern "C" void **__hipRegisterFatBinary(const void *)
{
    static void *handle;
    return &handle;
}
extern "C" void __hipUnregisterFatBinary(void **) {}
extern "C" void __hipRegisterFunction(void **, const void *stub, char *, const char *name, unsigned, void *, void *, void *, void *,
                                      int *)
{
    if (g_nkernels < 256) g_kernels[g_nkernels++] = {stub, name};
}
static const char *kernel_name(const void *stub)
{
    for (int i = 0; i < g_nkernels; ++i)
        if (g_kernels[i].stub == stub) return g_kernels[i].name;
    return "(unregistered)";
}
// ... without the anonymous namespace's prefix, which every kernel of lstm.hip carries
static const char *short_name(const void *stub)
{
    const char *n = kernel_name(stub);
    return strncmp(n, "_ZN12_GLOBAL__N_1", 17) == 0 ? n + 17 : n;
}

static hipError_t fake_get_device(int *dev) { *dev = 0; return hipSuccess; }
static hipError_t fake_properties(hipDeviceProp_t *p, int)
{
    memset(p, 0, sizeof(*p));
    strncpy(p->gcnArchName, g_fake.arch, sizeof(p->gcnArchName) - 1);
    p->multiProcessorCount = g_fake.cus;
    return hipSuccess;
}
static hipError_t fake_attribute(int *v, hipDeviceAttribute_t a, int)
{
    *v = a == hipDeviceAttributeNumberOfXccs ? g_fake.xccs : 0;
    return hipSuccess;
}
static hipError_t fake_func_attribute(const void *f, hipFuncAttribute a, int v)
{
    out("  func_attribute %s lds=%d%s\n", short_name(f), v, a == hipFuncAttributeMaxDynamicSharedMemorySize ? "" : " (?)");
    return g_fake.attr_fails ? hipErrorInvalidValue : hipSuccess;
}
static hipError_t fake_memset(void *p, int v, size_t n, hipStream_t s)
{
    if (join_last_line("  memset ")) out("; %s value=%d bytes=%zu stream=%s\n", sym(p), v, n, sym(s));
    else out("  memset %s value=%d bytes=%zu stream=%s\n", sym(p), v, n, sym(s));
    return g_fake.memset_fails ? hipErrorInvalidValue : hipSuccess;
}
static hipError_t fake_priority_range(int *lo, int *hi) { *lo = 0; *hi = g_fake.flat_prio ? 0 : -1; return hipSuccess; }
static hipError_t fake_stream_create(hipStream_t *s, unsigned flags, int prio)
{
    static uintptr_t next = 0xf01000000000ull;               // s1, s1+4096
    *s = (hipStream_t)next;
    next += 0x1000;
    out("  stream_create %s flags=%u priority=%d\n", sym(*s), flags, prio);
    return hipSuccess;
}
static hipError_t fake_stream_priority(hipStream_t, int *prio) { *prio = g_fake.caller_prio; return hipSuccess; }
static hipError_t fake_event_create(hipEvent_t *e, unsigned)
{
    static uintptr_t next = 0xf02000000000ull;               // s2, ...: the events
    *e = (hipEvent_t)next;
    next += 0x1000;
    return hipSuccess;
}
static hipError_t fake_event_record(hipEvent_t e, hipStream_t s) { out("  event_record %s stream=%s\n", sym(e), sym(s)); return hipSuccess; }
static hipError_t fake_stream_wait(hipStream_t s, hipEvent_t e, unsigned) { out("  stream_wait %s event=%s\n", sym(s), sym(e)); return hipSuccess; }

template <class... T> static void record_launch(const void *kernel, dim3 grid, dim3 block, size_t lds, hipStream_t s, const T &...args);
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, shmem, stream, ...) \
    record_launch((const void *)(kernel), dim3(grid), dim3(block), (size_t)(shmem), stream, __VA_ARGS__)
#undef hipGetDeviceProperties
#define hipGetDeviceProperties(p, dev) fake_properties(p, dev)
#define hipGetLastError() hipSuccess
#define hipGetDevice(p) fake_get_device(p)
#define hipDeviceGetAttribute(v, a, dev) fake_attribute(v, a, dev)
#define hipFuncSetAttribute(f, a, v) fake_func_attribute(f, a, v)
#define hipMemsetAsync(p, v, n, s) fake_memset(p, v, n, s)
#define hipDeviceGetStreamPriorityRange(lo, hi) fake_priority_range(lo, hi)
#define hipStreamCreateWithPriority(s, flags, prio) fake_stream_create(s, flags, prio)
#define hipStreamGetPriority(s, prio) fake_stream_priority(s, prio)
#define hipEventCreateWithFlags(e, flags) fake_event_create(e, flags)
#define hipEventRecord(e, s) fake_event_record(e, s)
#define hipStreamWaitEvent(s, e, flags) fake_stream_wait(s, e, flags)

#include "lstm.hip"

// gemm.hip and misc.hip are not linked: the two passes behind a recurrence are recorded here
extern "C" int lc_cast_bf16(const float *x, int rows, int C, int ldx, uint16_t *nat, int ldnat, uint16_t *tr, int ldtr, lc_stream_t stream)
{
    out("  lc_cast_bf16 x=%s rows=%d C=%d ldx=%d nat=%s ldnat=%d tr=%s ldtr=%d stream=%s\n", sym(x), rows, C, ldx, sym(nat),
        ldnat, sym(tr), ldtr, sym(stream));
    return LC_OK;
}
extern "C" int lc_split_bf16x3(const float *x, int rows, int cols, int ldx, uint16_t *o, int ldo, lc_stream_t stream)
{
    out("  lc_split_bf16x3 x=%s rows=%d cols=%d ldx=%d out=%s ldo=%d stream=%s\n", sym(x), rows, cols, ldx, sym(o), ldo,
        sym(stream));
    return LC_OK;
}

// ---- the argument blocks: every field the launched kernel reads (a field its entry leaves unset is not printed: the bf16
// shadow pointer of a direction outside the persistent kernels' blocks) ---------------------------------------------------
static std::string g_line;
__attribute__((format(printf, 1, 2))) static void put(const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_line += buf;
}
static void put_dir(const DirFwd &d, bool shadow)
{
    put(" {zx=%s R=%s w=%s,%s,%s cs=%s hs=%s hT=%s rev=%d", sym(d.zx), sym(d.R), sym(d.w_f), sym(d.w_i),
        sym(d.w_o), sym(d.cs), sym(d.hs), sym(d.hT), d.reverse);
    if (shadow) put(" hs16=%s", sym(d.hs16));
    put("}");
}
static void put_dir(const DirBwd &d, bool shadow)
{
    put(" {gates=%s RT=%s w=%s,%s,%s cs=%s dh=%s dc=%s dzT=%s rev=%d", sym(d.gates), sym(d.RT), sym(d.w_f),
        sym(d.w_i), sym(d.w_o), sym(d.cs), sym(d.dh), sym(d.dc), sym(d.dzT), d.reverse);
    if (shadow) put(" dz16=%s", sym(d.dz16));
    put("}");
}
template <class D> static void put_dirs(const D *d, bool shadow)
{
    const size_t at0 = g_line.size();
    put_dir(d[0], shadow);
    const size_t at1 = g_line.size();
    put_dir(d[1], shadow);          // one direction: the second block is a copy of the first
    if (g_line.compare(at0, at1 - at0, g_line, at1, std::string::npos) == 0) g_line.replace(at1, std::string::npos, " {same}");
}
static void put_geom(const PGeom &g)
{
    put(" g{T=%d B=%d N=%d ndir=%d gpd=%d rpg=%d upw=%d UP=%d nwg=%d}", g.T, g.B, g.N, g.ndir, g.gpd, g.rpg, g.upw, g.UP, g.nwg);
}
static int g_step = -1;        // the launch train's step index: printed behind the block, so that a train's launches compare equal
static void put_args(const FwdArgs &a)
{
    put_dirs(a.d, false);
    put(" seq=%s T=%d B=%d N=%d Bpad=%d row_base=%d fb=%.9g dbg=%s", sym(a.seq_len), a.T, a.B, a.N, a.Bpad, a.row_base,
        a.forget_bias, sym(a.dbg));
    g_step = a.step;
}
static void put_args(const BwdArgs &a)
{
    put_dirs(a.d, false);
    put(" seq=%s T=%d B=%d N=%d Bpad=%d row_base=%d", sym(a.seq_len), a.T, a.B, a.N, a.Bpad, a.row_base);
    g_step = a.step;
}
static void put_args(const PFwdArgs &a)
{
    put_dirs(a.d, true);
    put(" seq=%s", sym(a.seq_len));
    put_geom(a.g);
    put(" fb=%.9g spin=%u ctl=%s hT=%s dbg=%s", a.forget_bias, a.spin_limit, sym(a.ctl), sym(a.hT), sym(a.dbg));
}
static void put_args(const PBwdArgs &a)
{
    put_dirs(a.d, true);
    put(" seq=%s", sym(a.seq_len));
    put_geom(a.g);
    put(" spin=%u ctl=%s dzT=%s upg=%s,%s dbg=%s", a.spin_limit, sym(a.ctl), sym(a.dzT), sym(a.upg[0]), sym(a.upg[1]),
        sym(a.dbg));
}
static void put_args(const XFwdArgs &a)
{
    put_dirs(a.d, false);
    put(" seq=%s row_base=%d,%d T=%d B=%d fb=%.9g spin=%u ctl=%s hx=%s px=%s dbg=%s", sym(a.seq_len), a.row_base[0],
        a.row_base[1], a.T, a.B, a.forget_bias, a.spin_limit, sym(a.ctl), sym(a.hx), sym(a.px), sym(a.dbg));
}
static void put_args(const XBwdArgs &a)
{
    put_dirs(a.d, true);
    put(" seq=%s row_base=%d,%d T=%d B=%d spin=%u ctl=%s dzx=%s px=%s upg=%s,%s dbg=%s", sym(a.seq_len), a.row_base[0],
        a.row_base[1], a.T, a.B, a.spin_limit, sym(a.ctl), sym(a.dzx), sym(a.px), sym(a.upg[0]), sym(a.upg[1]),
        sym(a.dbg));
}
static void put_args(const PVerifyArgs &a)
{
    put(" ctl=%s nused=%d nwg=%d nout=%d out=%s,%s out16=%s,%s count=%zu count16=%zu", sym(a.ctl), a.nused, a.nwg, a.nout,
        sym(a.out[0]), sym(a.out[1]), sym(a.out16[0]), sym(a.out16[1]), a.count, a.count16);
}
// the plain argument lists of pack_k16 / pack_k32_bf16 / unit_param_grad / unit_param_fold
static void put_one(int v) { put(" %d", v); }
template <class P> static void put_one(P *v) { put(" %s", sym(v)); }
template <class... T> static void put_args(const T &...args) { (put_one(args), ...); }

static void put_dim(const char *what, dim3 d)
{
    if (d.z != 1) put(" %s=%u,%u,%u", what, d.x, d.y, d.z);
    else if (d.y != 1) put(" %s=%u,%u", what, d.x, d.y);
    else put(" %s=%u", what, d.x);
}
template <class... T> static void record_launch(const void *kernel, dim3 grid, dim3 block, size_t lds, hipStream_t s, const T &...args)
{
    static std::string last[2];                // per stream: the caller's, and any other
    std::string &mine = last[(uintptr_t)s != ADDR_STREAM];
    g_line.clear();
    g_step = -1;
    put("%s", short_name(kernel));
    put_dim("grid", grid);
    put_dim("block", block);
    put(" lds=%zu stream=%s", lds, sym(s));
    put_args(args...);
    // a launch train repeats one launch T times with nothing but the step index moving: the block is printed once
    char again[64];
    snprintf(again, sizeof(again), "  launch (as the last step launch on %s) step=", sym(s));
    if (g_step >= 0 && g_line == mine && join_last_line(again)) out(",%d\n", g_step);
    else if (g_step >= 0 && g_line == mine) out("%s%d\n", again, g_step);
    else if (g_step >= 0) out("  launch %s step=%d\n", g_line.c_str(), g_step);
    else out("  launch %s\n", g_line.c_str());
    if (g_step >= 0) mine = g_line;
    else last[0].clear(), last[1].clear();
}

// ---- one call ----------------------------------------------------------------------------------------------------------
enum Entry { F32, X3, BF16 };
static const char *const ENTRY_NAME[2][3] = {{"lc_lstm_fwd", "lc_lstm_fwd_x3", "lc_lstm_fwd_bf16"},
                                             {"lc_lstm_bwd", "lc_lstm_bwd_x3", "lc_lstm_bwd_bf16"}};
enum Tensor { ZX, RW, WF, WI, WO, CS, HS, SHADOW, DH, DPEEP, DBIAS };
// fake device addresses, 256-byte aligned and far apart: one 16 TB lane per tensor, 64 GB per direction
static void *addr(int tensor, int dir) { return (void *)(0x100000000000ull * (tensor + 1) + 0x001000000000ull * dir); }

struct Call {
    Entry entry = F32;
    bool bwd = false;
    int T = 5, B = 8, N = 64, ndir = 2;
    long persistent = LC_OPTION_UNSET, spin_limit = LC_OPTION_UNSET;
    bool stamps = false;
    bool peep[2] = {true, false};                      // as the edge tests' variant a: peepholes in direction 0 only
    bool dpeep[2] = {true, true}, dbias[2] = {true, true};
    bool shadow[2] = {true, true};                     // hs_bf16 / dz_bf16 (the plain fp32 entries ignore them)
    int shadow_only[2] = {0, 0};
    int reverse[2] = {0, 1};
    bool null_dirs = false, null_seq = false, null_ws = false;
    int null_inside = 0;                               // 1 .. 4: that required pointer of the last direction is NULL
    long long ws_delta = 0;                            // added to lc_lstm_*_workspace_bytes
};

static void run(const Call &c)
{
    lc_lstm_fwd_dir_t f[2];
    lc_lstm_bwd_dir_t b[2];
    memset(f, 0, sizeof(f));
    memset(b, 0, sizeof(b));
    const size_t ws_bytes = (c.bwd ? lc_lstm_bwd_workspace_bytes(c.B, c.N, c.ndir) : lc_lstm_fwd_workspace_bytes(c.B, c.N, c.ndir)) +
                            c.ws_delta;
    void *ws = c.null_ws ? nullptr : (void *)ADDR_WS;
    const int *seq = c.null_seq ? nullptr : (const int *)ADDR_SEQ;
    lc_stream_t stream = (lc_stream_t)ADDR_STREAM;
    g_record.clear();
    g_in_call = true;
    out("%s(ndir=%d T=%d B=%d N=%d ws_bytes=%zu%s%s%s)", ENTRY_NAME[c.bwd][c.entry], c.ndir, c.T, c.B, c.N, ws_bytes,
        c.null_seq ? " seq_len=0" : "", c.null_ws ? " ws=0" : "", c.null_dirs ? " dirs=0" : "");
    for (int d = 0; d < 2 && d < c.ndir; ++d) {
        const bool last = d == c.ndir - 1;
        float *wf = c.peep[d] ? (float *)addr(WF, d) : nullptr, *wi = c.peep[d] ? (float *)addr(WI, d) : nullptr,
              *wo = c.peep[d] ? (float *)addr(WO, d) : nullptr;
        uint16_t *sh = c.shadow[d] ? (uint16_t *)addr(SHADOW, d) : nullptr;
        f[d].zx = last && c.null_inside == 1 ? nullptr : (float *)addr(ZX, d);
        f[d].R = last && c.null_inside == 2 ? nullptr : (float *)addr(RW, d);
        f[d].cs = last && c.null_inside == 3 ? nullptr : (float *)addr(CS, d);
        f[d].hs = last && c.null_inside == 4 ? nullptr : (float *)addr(HS, d);
        f[d].w_f = wf; f[d].w_i = wi; f[d].w_o = wo;
        f[d].reverse = c.reverse[d]; f[d].hs_bf16 = sh; f[d].shadow_only = c.shadow_only[d];
        b[d].gates = f[d].zx; b[d].RT = f[d].R; b[d].cs = f[d].cs;
        b[d].dh = last && c.null_inside == 4 ? nullptr : (float *)addr(DH, d);
        b[d].w_f = wf; b[d].w_i = wi; b[d].w_o = wo;
        b[d].dpeep = c.dpeep[d] ? (float *)addr(DPEEP, d) : nullptr;
        b[d].dbias = c.dbias[d] ? (float *)addr(DBIAS, d) : nullptr;
        b[d].reverse = c.reverse[d]; b[d].dz_bf16 = sh; b[d].shadow_only = c.shadow_only[d];
        // operands sit at fixed addresses (see sym): the line says which of the optional ones are there, and which is missing
        static const char *const required[2][5] = {{"", " zx=0", " R=0", " cs=0", " hs=0"}, {"", " gates=0", " RT=0", " cs=0", " dh=0"}};
        if (c.null_dirs) continue;
        out(" dir%d{rev=%d%s%s%s%s%s", d, c.reverse[d], last ? required[c.bwd][c.null_inside] : "", c.peep[d] ? " w" : "",
            c.bwd && c.dpeep[d] ? " dpeep" : "", c.bwd && c.dbias[d] ? " dbias" : "", c.shadow[d] ? " shadow" : "");
        if (c.shadow_only[d]) out(" shadow_only=%d", c.shadow_only[d]);
        out("}");
    }
    lc_set_option("lstm_persistent", c.persistent);
    lc_set_option("lstm_spin_limit", c.spin_limit);
    if (c.persistent != LC_OPTION_UNSET) out(" lstm_persistent=%ld", c.persistent);
    if (c.spin_limit != LC_OPTION_UNSET) out(" lstm_spin_limit=%ld", c.spin_limit);
    if (c.stamps) out(" stamps");
    out("\n");
    lc_debug_set_lstm_stamps(c.stamps ? (unsigned long long *)ADDR_STAMPS : nullptr);
    lc_set_error("%s", "");
    const lc_lstm_fwd_dir_t *fd = c.null_dirs ? nullptr : f;
    const lc_lstm_bwd_dir_t *bd = c.null_dirs ? nullptr : b;
    int rc = 0;
    if (!c.bwd) {
        auto *fn = c.entry == F32 ? lc_lstm_fwd : c.entry == X3 ? lc_lstm_fwd_x3 : lc_lstm_fwd_bf16;
        rc = fn(fd, c.ndir, seq, c.T, c.B, c.N, 1.0f, ws, ws_bytes, stream);
    } else {
        auto *fn = c.entry == F32 ? lc_lstm_bwd : c.entry == X3 ? lc_lstm_bwd_x3 : lc_lstm_bwd_bf16;
        rc = fn(bd, c.ndir, seq, c.T, c.B, c.N, ws, ws_bytes, stream);
    }
    out("  -> rc=%d error=\"%s\" schedule=0x%x\n", rc, lc_last_error(), (unsigned)lc_debug_last_lstm_schedule());
    end_record(rc);
    lc_debug_set_lstm_stamps(nullptr);
}

static Call call(Entry entry, bool bwd, int T, int B, int N, int ndir, bool persistent = true)
{
    Call c;
    c.entry = entry; c.bwd = bwd; c.T = T; c.B = B; c.N = N; c.ndir = ndir;
    if (!persistent) c.persistent = 0;
    if (ndir == 1) c.reverse[0] = B % 2 == 0;
    return c;
}

// ---- the fixed list ----------------------------------------------------------------------------------------------------
struct Shape { Entry entry; int N, ndir, B, T; bool persistent; };
// ALL_CASES of tests/test_lstm_edges_host.py, in its order
static const Shape CASES[] = {
    {F32, 16, 1, 1, 4, true},     {F32, 48, 2, 5, 6, true},     {F32, 320, 2, 64, 5, true},    {F32, 512, 1, 128, 5, true},
    {F32, 512, 2, 65, 5, true},   {F32, 640, 2, 3, 4, true},    {F32, 768, 1, 64, 5, true},    {F32, 896, 1, 129, 5, true},
    {F32, 1024, 2, 65, 5, true},  {F32, 1024, 2, 33, 3, true},  {F32, 1040, 2, 64, 5, true},   {F32, 32, 2, 17, 1, true},
    {F32, 32, 2, 17, 2, true},    {F32, 32, 2, 17, 3, true},    {F32, 1024, 2, 100, 5, false}, {F32, 1024, 2, 32, 4, false},
    {X3, 64, 2, 3, 4, true},      {X3, 448, 2, 20, 5, true},    {X3, 512, 1, 128, 5, true},    {X3, 768, 2, 65, 5, true},
    {X3, 1024, 1, 40, 5, true},   {X3, 96, 2, 5, 5, true},      {X3, 640, 2, 3, 4, true},      {BF16, 32, 1, 1, 4, true},
    {BF16, 96, 2, 19, 5, true},   {BF16, 768, 2, 33, 5, true},  {BF16, 1024, 2, 64, 5, true},  {BF16, 1024, 1, 128, 5, true},
    {BF16, 64, 2, 40, 3, true},   {BF16, 1024, 2, 65, 5, true}};
// the shapes test_dispatch_edges_of_the_restated_rule names (entry, pass, T, B, N, ndir, persistent)
static const struct { Entry entry; bool bwd; int T, B, N, ndir; bool persistent; } EDGES[] = {
    {F32, false, 4, 64, 512, 2, true},  {F32, false, 4, 65, 512, 2, true},   {F32, true, 4, 128, 512, 1, true},
    {F32, true, 4, 129, 512, 1, true},  {F32, false, 3, 8, 512, 2, true},    {F32, false, 3, 8, 1024, 2, true},
    {F32, false, 4, 8, 528, 2, true},   {BF16, false, 4, 8, 528, 2, true},   {BF16, false, 4, 8, 544, 2, true},
    {F32, false, 4, 32, 1024, 2, false}, {F32, false, 4, 33, 1024, 2, false}, {X3, false, 4, 8, 896, 2, true},
    {X3, true, 4, 8, 1024, 2, true},    {F32, false, 4, 1 << 16, 1024, 2, true}};
// a representative of each schedule 1 .. 7 (on an MI355X; elsewhere they all ride the launch train)
static const Shape REPS[] = {{F32, 320, 2, 64, 5, true},  {BF16, 1024, 2, 64, 5, true}, {BF16, 512, 1, 8, 4, true},
                             {F32, 1024, 2, 33, 2, true}, {F32, 32, 2, 17, 2, true},    {F32, 896, 1, 129, 5, true},
                             {X3, 768, 2, 65, 5, true},   {X3, 448, 2, 20, 5, true}};

static bool fake_is_mi355x() { return strncmp(g_fake.arch, "gfx950", 6) == 0 && g_fake.cus == 256 && g_fake.xccs == 8; }

// The plain MI355X answers get the whole list.  Every other answer set gets what it can change: every schedule's
// representative, both passes (a device that is not an MI355X runs them all on the launch train, under the two failure
// sets each ends at its first failing call); the two stream-priority sets the two-stream forward alone.
static void fixed_list()
{
    const bool streams_only = g_fake.flat_prio || g_fake.caller_prio;
    const bool plain = fake_is_mi355x() && !streams_only && !g_fake.attr_fails && !g_fake.memset_fails;
    if (!plain) {
        for (const Shape &s : REPS)
            for (int bwd = 0; bwd < 2; ++bwd)
                if (!streams_only || (s.N == 1024 && s.T == 2 && !bwd)) {
                    g_whole = fake_is_mi355x() || s.N == 1024;       // (the launch train's records are whole in the plain set)
                    run(call(s.entry, bwd, s.T, s.B, s.N, s.ndir));
                }
        return;
    }
    for (const Shape &s : CASES)
        for (int bwd = 0; bwd < 2; ++bwd) run(call(s.entry, bwd, s.T, s.B, s.N, s.ndir, s.persistent));
    g_whole = false;          // from here on, apart from the x3 shadow's limit: a shape or one input of a call above changed, or a refusal
    for (const auto &e : EDGES) run(call(e.entry, e.bwd, e.T, e.B, e.N, e.ndir, e.persistent));
    for (const Shape &s : REPS)
        for (int bwd = 0; bwd < 2; ++bwd) {
            const Call base = call(s.entry, bwd, s.T, s.B, s.N, s.ndir);
            Call c = base;
            c.peep[0] = false; run(c);                                    // peepholes NULL everywhere, and present everywhere
            c.peep[0] = c.peep[1] = true; run(c);
            if (bwd) {                                                    // dpeep / dbias NULL per direction
                c = base; c.dpeep[0] = false; c.dbias[s.ndir - 1] = false; run(c);
                c = base; c.dpeep[0] = c.dpeep[1] = c.dbias[0] = c.dbias[1] = false; run(c);
            }
            c = base; c.shadow[0] = c.shadow[1] = false; run(c);          // no bf16 / x3 shadow
            c = base; c.shadow_only[0] = c.shadow_only[1] = 1; run(c);    // shadow_only: the bf16 kernels at N = 1024 take it
            if (s.entry == BF16 && s.N == 1024) {                         // ... when every direction sets it and has a shadow
                c.shadow_only[0] = 0; run(c);
                c = base; c.shadow_only[0] = c.shadow_only[1] = 1; c.shadow[1] = false; run(c);
            }
            c = base; c.spin_limit = 0; run(c);                           // (unset: the base call, above)
            c.spin_limit = -5; run(c);
            c = base; c.stamps = true; run(c);
        }
    {
        // lc_lstm_bwd_x3: the x3 shadow's byte offsets T * B * 12 N * 2 on either side of 0x7fffffff, at a width of each
        // split-operand schedule (one persistent launch each; on the launch train these would be T launches)
        static const int tb[][3] = {{1387, 63, 1024}, {43691, 2, 1024}, {1388, 63, 1024}, {1387, 126, 512}, {1388, 126, 512}};
        g_whole = true;
        for (const auto &x : tb) run(call(X3, true, x[0], x[1], x[2], 1));
        g_whole = false;
    }
    // every refusal: the schedule word behind it is the one before it
    for (int e = 0; e < 3; ++e)
        for (int bwd = 0; bwd < 2; ++bwd) {
            const Call base = call((Entry)e, bwd, 5, 8, 64, 2);
            run(base);
            Call c = base; c.null_dirs = true; run(c);
            c = base; c.null_seq = true; run(c);
            c = base; c.null_ws = true; run(c);
            for (int k = 1; k <= 4; ++k) { c = base; c.null_inside = k; run(c); }
            c = base; c.ndir = 3; run(c);
            c = base; c.ndir = 0; run(c);
            c = base; c.N = 72; run(c);                                   // N % 16 != 0
            c = base; c.N = 48; run(c);                                   // N % 32 != 0: the bf16 entries refuse
            c = base; c.T = 0; run(c);
            c = base; c.B = 0; run(c);
            c = base; c.ws_delta = -1; run(c);
            c = call((Entry)e, bwd, 5, 8, 1024, 1); c.ws_delta = -1; run(c);
            run(call((Entry)e, bwd, 2, 8, 64, 2));                        // ... and a call that is taken again
        }
    static const int GN[] = {16, 32, 48, 64, 320, 512, 528, 640, 768, 896, 1024, 1040}, GB[] = {1, 16, 17, 64, 65, 128, 129};
    for (int N : GN) {
        out("workspace_bytes(N=%d) fwd/bwd at B=1,16,17,64,65,128,129 x ndir=1,2:", N);
        for (int B : GB)
            for (int ndir = 1; ndir <= 2; ++ndir) out(" %zu/%zu", lc_lstm_fwd_workspace_bytes(B, N, ndir), lc_lstm_bwd_workspace_bytes(B, N, ndir));
        out("\n");
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
static void sweep(uint64_t seed, long draws)
{
    g_rng = seed;
    for (long i = 0; i < draws; ++i) {
        Call c;
        c.entry = (Entry)(rnd() % 3);
        c.bwd = rnd() & 1;
        c.T = rnd_in(1, 6);
        static const int rows[] = {1, 8, 16, 17, 32, 33, 64, 65, 128, 129};
        c.B = rnd() % 3 ? rnd_in(1, 200) : rows[rnd() % 10];
        static const int widths[] = {64, 320, 448, 512, 528, 544, 640, 768, 896, 1024, 1040};
        c.N = rnd() % 3 ? 16 * rnd_in(1, 66) : widths[rnd() % 11];
        c.ndir = 1 + (rnd() & 1);
        if (rnd() % 4 == 0) c.persistent = rnd() % 2;
        if (rnd() % 6 == 0) c.spin_limit = rnd() % 3 == 0 ? -1 : (long)(rnd() % 5000);
        c.stamps = rnd() % 8 == 0;
        for (int d = 0; d < 2; ++d) {
            c.peep[d] = rnd() & 1; c.dpeep[d] = rnd() % 4 != 0; c.dbias[d] = rnd() % 4 != 0;
            c.shadow[d] = rnd() % 4 != 0; c.shadow_only[d] = rnd() % 3 == 0; c.reverse[d] = rnd() & 1;
        }
        if (rnd() % 16 == 0) {
            switch (rnd() % 8) {
            case 0: c.null_dirs = true; break;
            case 1: c.null_seq = true; break;
            case 2: c.null_ws = true; break;
            case 3: c.null_inside = rnd_in(1, 4); break;
            case 4: c.ndir = rnd() & 1 ? 3 : 0; break;
            case 5: c.N += 8; break;
            case 6: if (rnd() & 1) c.T = 0; else c.B = 0; break;
            default: c.ws_delta = -1; break;
            }
        }
        run(c);
        if (rnd() % 64 == 0)
            out("workspace_bytes(B=%d N=%d ndir=%d) fwd=%zu bwd=%zu\n", c.B, c.N, c.ndir, lc_lstm_fwd_workspace_bytes(c.B, c.N, c.ndir),
                lc_lstm_bwd_workspace_bytes(c.B, c.N, c.ndir));
    }
}

// ---- the plan: schedule words for `entry pass T B N ndir persistent` lines ------------------------------------------------
static void plan()
{
    char entry[16], pass[16];
    int T, B, N, ndir, persistent;
    g_quiet = true;
    while (scanf("%15s %15s %d %d %d %d %d", entry, pass, &T, &B, &N, &ndir, &persistent) == 7) {
        const Entry e = strcmp(entry, "bf16") == 0 ? BF16 : strcmp(entry, "x3") == 0 ? X3 : F32;
        Call c = call(e, strcmp(pass, "bwd") == 0, T, B, N, ndir, persistent != 0);
        c.shadow[0] = c.shadow[1] = false;             // as the edge tests call: no shadow, so bit 18 stays clear
        run(c);
        printf("%s %s %d %d %d %d %d 0x%x %s\n", entry, pass, T, B, N, ndir, persistent, (unsigned)lc_debug_last_lstm_schedule(),
               lc_last_error());
    }
}

int main(int argc, char **argv)
{
    if (argc < 8) {
        fprintf(stderr, "usage: %s ARCH CUS XCCS FLAT_PRIO CALLER_PRIO ATTR_FAILS MEMSET_FAILS [--full | --sweep SEED DRAWS | --plan]\n", argv[0]);
        return 2;
    }
    g_fake.arch = argv[1];
    g_fake.cus = atoi(argv[2]); g_fake.xccs = atoi(argv[3]); g_fake.flat_prio = atoi(argv[4]); g_fake.caller_prio = atoi(argv[5]);
    g_fake.attr_fails = atoi(argv[6]); g_fake.memset_fails = atoi(argv[7]);
    if (argc == 11 && strcmp(argv[8], "--sweep") == 0) sweep(strtoull(argv[9], nullptr, 10), atol(argv[10]));
    else if (argc == 9 && strcmp(argv[8], "--plan") == 0) plan();
    else {
        g_always_whole = argc == 9 && strcmp(argv[8], "--full") == 0;
        fixed_list();
    }
    return 0;
}
