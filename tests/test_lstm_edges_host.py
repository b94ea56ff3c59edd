"""Host side of the lc_lstm_* edge tests: a float64 numpy reference of the two ops in the library's own layout, the case
tables, the length patterns, the problem generator and the dispatch restated from csrc/lstm.hip.
tests/test_gpu_lstm_edges.py imports all of them from here.  No GPU needed.

Reference (``ref_fwd`` / ``ref_bwd``): [T, B, *] tensors, gate-interleaved columns (column (n/8)*32 + g*8 + n%8 is gate g of
unit n; g = 0 i, 1 j, 2 f, 3 o), ``reverse`` by index order, a frame is live when t < seq_len[b], dead frames are 0 in every
output, peepholes optional.  The state a frame starts from is what the frame before it in processing order stored (zero when
that frame is dead or out of range): a dead frame is followed by a live one only in the reverse direction, where the state is
still zero, so this is dynamic_rnn's "carry the state through".  Both take an operand-rounding function (the bf16 entry
points round the two operands of the step product) and "forced" previous-step arrays (the kernel's own cs / hs, resp. dz), so
that a bf16 recurrence can be checked step by step without a rounding-boundary flip cascading.
``test_reference_agrees_with_the_c_oracle`` anchors both against oracle.lstmp_fwd / lstmp_bwd (kernel = [identity; R], bias 0,
no projection: the oracle's gates / cs / mp / dx are the op's gates / cs / hs / dz) at < 1e-12.

Dispatch, restated from lstm_plan / lstm_fwd_walk and the header (``expected``; test_lstm_dispatch_host.py holds it to the C
rule on the CPU), in this order:

    XCD-pair schedule (5; 6 = split-operand at N = 768 / 1024): fp32 and split-operand entries, N in {640, 768, 896, 1024},
        T >= 4, T * B * 4N * 4 < 2^32
    single-XCD schedule (1 fp32, 2 bf16, 7 = split-operand entry at N % 64 == 0): N <= 512 (bf16: N <= 1024, N % 32 == 0),
        T >= 4, ceil(B / (8 / ndir)) <= 16
    launch train otherwise, and always with persistent off.  Bpad = 16 (B <= 16), B rounded up to 32 (B <= 64) or to 64.
        forward: two streams (3, mt = 2) when not bf16, ndir = 2, Bpad = 64, N >= 1024; else (4) mt = 4 if Bpad >= 64 else
            Bpad / 16, halved (rounding up) while mt > 1 and (N / 8) * ceil(B / (16 mt)) * ndir < 200
        backward (4): mt = 2 if Bpad >= 32 and (N / 16) * ceil(B / 32) * ndir >= 200, else 1

Length patterns, deterministic in (B, T): ``mixed`` cycles T-1, 0, T, 1, T-2, T (unsorted, row 0 not the longest, zeros inside
a row group), ``short`` cycles T-2, 0, 1, T-3 clipped to [0, T-1] (no row reaches T: the reverse direction's first steps are
dead for every row; at T = 1 that leaves no live row at all), ``dead_group`` is mixed with rows 16..31 zero, ``all_zero``;
B = 1 gets [T] (mixed) and [T-2] (short).

Problems (``Problem``): zx 0.5 N(0,1), R 0.5 / sqrt(N) N(0,1), peepholes 0.2 N(0,1), dh 0.1 N(0,1), forget bias 1 - the scales
of test_persistent_recurrence_equals_launch_train.  Variant ``a``: peepholes in direction 0 (direction 1 of a bidirectional
call has all three NULL), dpeep / dbias start from 0.1 N(0,1), dead frames of zx / dh hold 1e30.  Variant ``b``: no peepholes
anywhere, dpeep passed anyway, dbias NULL in direction 0 of a bidirectional call (and in the one-directional cases listed in
NULL_DBIAS_1DIR), dead frames hold NaN."""
import functools
from collections import namedtuple

import numpy as np
import pytest

Case = namedtuple("Case", "entry N ndir B T persistent fwd bwd note")    # fwd / bwd: (schedule word bits 0-7, mt) expected
KINDS = {1: "persistent_f32", 2: "persistent_bf16", 3: "two_stream_train", 4: "launch_train", 5: "persistent_f32_xcd_pair",
         6: "persistent_x3_xcd_pair", 7: "persistent_x3"}
FORGET_BIAS = 1.0


def _c(entry, N, ndir, B, T, fwd, bwd, note="", persistent=True):
    return Case(entry, N, ndir, B, T, persistent, fwd, bwd, note)


# ------------------------------------------------------------------------------------------------ the case tables
F32_CASES = [
    _c("f32", 16, 1, 1, 4, (1, 0), (1, 0), "one column tile, one row"),
    _c("f32", 48, 2, 5, 6, (1, 0), (1, 0), "ragged K, an empty row group"),
    _c("f32", 320, 2, 64, 5, (1, 0), (1, 0), "16 rows per group"),
    _c("f32", 512, 1, 128, 5, (1, 0), (1, 0), "partial buffer full"),
    _c("f32", 512, 2, 65, 5, (4, 4), (4, 1), "falls to the train"),
    _c("f32", 640, 2, 3, 4, (5, 0), (5, 0), "pair, smallest launch"),
    _c("f32", 768, 1, 64, 5, (5, 0), (5, 0), "second slot idle"),
    _c("f32", 896, 1, 129, 5, (5, 0), (5, 0), "second launch with one row"),
    _c("f32", 1024, 2, 65, 5, (5, 0), (5, 0), "second block with one row"),
    _c("f32", 1024, 2, 33, 3, (3, 2), (4, 2), "two-stream, T < 4"),
    _c("f32", 1040, 2, 64, 5, (3, 2), (4, 2), "two-stream above every persistent width"),
    _c("f32", 32, 2, 17, 1, (4, 1), (4, 1), "train, T = 1"),
    _c("f32", 32, 2, 17, 2, (4, 1), (4, 1), "train, T = 2"),
    _c("f32", 32, 2, 17, 3, (4, 1), (4, 1), "train, T = 3"),
    _c("f32", 1024, 2, 100, 5, (4, 4), (4, 2), "persistent off", persistent=False),
    _c("f32", 1024, 2, 32, 4, (4, 2), (4, 1), "persistent off", persistent=False),
]
X3_CASES = [
    _c("x3", 64, 2, 3, 4, (7, 0), (7, 0), "smallest split-operand width"),
    _c("x3", 448, 2, 20, 5, (7, 0), (7, 0), ""),
    _c("x3", 512, 1, 128, 5, (7, 0), (7, 0), "partial buffer full"),
    _c("x3", 768, 2, 65, 5, (6, 0), (6, 0), "second block with one row"),
    _c("x3", 1024, 1, 40, 5, (6, 0), (6, 0), "second slot idle"),
    _c("x3", 96, 2, 5, 5, (1, 0), (1, 0), "falls through to schedule 1"),
    _c("x3", 640, 2, 3, 4, (5, 0), (5, 0), "falls through to schedule 5"),
]
BF16_CASES = [
    _c("bf16", 32, 1, 1, 4, (2, 0), (2, 0), "one block, one row"),
    _c("bf16", 96, 2, 19, 5, (2, 0), (2, 0), "ragged"),
    _c("bf16", 768, 2, 33, 5, (2, 0), (2, 0), ""),
    _c("bf16", 1024, 2, 64, 5, (2, 0), (2, 0), "full width, 16 rows per group"),
    _c("bf16", 1024, 1, 128, 5, (2, 0), (2, 0), "partial buffer full"),
    _c("bf16", 64, 2, 40, 3, (4, 1), (4, 1), "train"),
    _c("bf16", 1024, 2, 65, 5, (4, 4), (4, 2), "train"),
]
ALL_CASES = F32_CASES + X3_CASES + BF16_CASES
DEAD_GROUP_CASES = [c for c in ALL_CASES if (c.entry, c.N, c.ndir, c.B) in
                    (("f32", 320, 2, 64), ("f32", 1024, 2, 65), ("x3", 768, 2, 65), ("bf16", 1024, 2, 64))]
ALL_ZERO_CASES = [c for c in ALL_CASES if (c.entry, c.N, c.ndir, c.B) in
                  (("f32", 48, 2, 5), ("x3", 64, 2, 3), ("bf16", 96, 2, 19))]
NULL_DBIAS_1DIR = [("f32", 16), ("x3", 1024), ("bf16", 1024)]      # (entry, N) of one-directional cases, variant b


def case_id(c):
    return "%s-N%d-d%d-B%d-T%d%s" % (c.entry, c.N, c.ndir, c.B, c.T, "" if c.persistent else "-train")


# ------------------------------------------------------------------------------------------------ the restated dispatch
def bpad(B):
    return 16 if B <= 16 else (B + 31) // 32 * 32 if B <= 64 else (B + 63) // 64 * 64


def expected(entry, pass_, T, B, N, ndir, persistent=True):
    """What ops.last_lstm_schedule() must report after the call (module docstring)."""
    bf, x3, bwd = entry == "bf16", entry == "x3", pass_ == "bwd"
    cdiv = lambda a, b: -(-a // b)
    kind, mt = 0, 0
    if persistent and T >= 4:
        if not bf and N in (640, 768, 896, 1024) and T * B * 4 * N * 4 < 2 ** 32:
            kind = 6 if x3 and N in (768, 1024) else 5
        elif cdiv(B, 8 // ndir) <= 16 and (N <= 1024 and N % 32 == 0 if bf else N <= 512):
            kind = 2 if bf else 7 if x3 and N % 64 == 0 else 1
    if not kind:
        Bp = bpad(B)
        if bwd:
            kind, mt = 4, 2 if Bp >= 32 and (N // 16) * cdiv(B, 32) * ndir >= 200 else 1
        elif not bf and ndir == 2 and Bp == 64 and N >= 1024:
            kind, mt = 3, 2
        else:
            kind, mt = 4, 4 if Bp >= 64 else Bp // 16
            while mt > 1 and (N // 8) * cdiv(B, 16 * mt) * ndir < 200:
                mt = (mt + 1) // 2
    return dict(kind=KINDS[kind], mt=mt, bf16=bf and kind in (2, 4), backward=bwd, dz_shadow_in_kernel=False)


# ------------------------------------------------------------------------------------------------ length patterns
def lengths(pattern, B, T):
    def cyc(vals, hi):
        return np.array([min(max(vals[b % len(vals)], 0), hi) for b in range(B)], np.int32)
    if pattern == "all_zero":
        return np.zeros(B, np.int32)
    if B == 1:
        return np.array([T if pattern != "short" else max(T - 2, 0)], np.int32)
    if pattern == "short":
        return cyc([T - 2, 0, 1, T - 3], T - 1)
    seq = cyc([T - 1, 0, T, 1, T - 2, T], T)
    if pattern == "dead_group":
        seq[16:32] = 0
    else:
        assert pattern == "mixed", pattern
    return seq


# ------------------------------------------------------------------------------------------------ the reference
def gate_cols(N):
    """cols[g][n] = column of gate g of unit n in a gate-interleaved [., 4N] operand."""
    n = np.arange(N)
    return [(n // 8) * 32 + g * 8 + (n % 8) for g in range(4)]


def interleaved_to_tf(a, N):
    return a[..., np.concatenate(gate_cols(N))]


def _sig(v):
    return 1.0 / (1.0 + np.exp(-v))


def ref_fwd(zx, R, w, seq, forget_bias, reverse, rnd=None, forced=None):
    """zx [T,B,4N], R [N,4N], w = (w_f, w_i, w_o) or None -> gates, cs, hs (float64).  ``rnd``: rounding of the step product's
    two operands; ``forced`` = (cs, hs): every step starts from these arrays' previous frame instead of the reference's own."""
    T, B, G = zx.shape
    N = G // 4
    cols = gate_cols(N)
    q = (lambda v: rnd(v.astype(np.float32)).astype(np.float64)) if rnd else (lambda v: v)
    Rq = q(np.asarray(R, np.float64))
    wf, wi, wo = (np.zeros(N),) * 3 if w is None else (np.asarray(v, np.float64) for v in w)
    gates, cs, hs = np.zeros((T, B, G)), np.zeros((T, B, N)), np.zeros((T, B, N))
    pc, ph = (cs, hs) if forced is None else (np.asarray(forced[0], np.float64), np.asarray(forced[1], np.float64))
    zero = np.zeros((B, N))
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        tp = t + 1 if reverse else t - 1
        cp, hp = (pc[tp], ph[tp]) if 0 <= tp < T else (zero, zero)
        act = (t < np.asarray(seq))[:, None]
        z = np.where(act, np.where(act, zx[t], 0.0) + q(hp) @ Rq, 0.0)       # dead frames of zx may hold anything
        ia = _sig(z[:, cols[0]] + wi * cp)
        fa = _sig(z[:, cols[2]] + forget_bias + wf * cp)
        ja = np.tanh(z[:, cols[1]])
        cn = fa * cp + ia * ja
        oa = _sig(z[:, cols[3]] + wo * cn)
        for c, v in zip(cols, (ia, ja, fa, oa)):
            gates[t][:, c] = np.where(act, v, 0.0)
        cs[t] = np.where(act, cn, 0.0)
        hs[t] = np.where(act, oa * np.tanh(cn), 0.0)
    return gates, cs, hs


def param_sums(dz, cs, reverse):
    """dpeep [3,N] (w_f, w_i, w_o) and dbias [4N] as float64 sums over a given dz [T,B,4N]."""
    T, B, G = dz.shape
    cols = gate_cols(G // 4)
    dz, cs = np.asarray(dz, np.float64), np.asarray(cs, np.float64)
    cprev = np.zeros_like(cs)
    if reverse:
        cprev[:-1] = cs[1:]
    else:
        cprev[1:] = cs[:-1]
    dpeep = np.stack([(dz[:, :, cols[2]] * cprev).sum((0, 1)), (dz[:, :, cols[0]] * cprev).sum((0, 1)),
                      (dz[:, :, cols[3]] * cs).sum((0, 1))])
    return dpeep, dz.sum((0, 1))


def ref_bwd(gates, cs, R, w, seq, dh, reverse, rnd=None, forced=None):
    """gates [T,B,4N] activated, cs [T,B,N], dh [T,B,N] -> dz [T,B,4N], dpeep [3,N] (w_f, w_i, w_o), dbias [4N] (float64).
    ``forced`` = dz: every step's recurrent term comes from this array's previous step (the cell gradient stays the
    reference's own); dpeep / dbias are then sums over the reference's dz all the same."""
    T, B, G = gates.shape
    N = G // 4
    cols = gate_cols(N)
    q = (lambda v: rnd(v.astype(np.float32)).astype(np.float64)) if rnd else (lambda v: v)
    RTq = q(np.ascontiguousarray(np.asarray(R, np.float64).T))
    wf, wi, wo = (np.zeros(N),) * 3 if w is None else (np.asarray(v, np.float64) for v in w)
    g, cs = np.asarray(gates, np.float64), np.asarray(cs, np.float64)
    dz = np.zeros((T, B, G))
    pz = dz if forced is None else np.asarray(forced, np.float64)
    dc = np.zeros((B, N))
    order = list(range(T)) if reverse else list(range(T - 1, -1, -1))
    with np.errstate(over="ignore", invalid="ignore"):
        for s, t in enumerate(order):
            tp = t + 1 if reverse else t - 1
            cp = cs[tp] if 0 <= tp < T else np.zeros((B, N))
            act = (t < np.asarray(seq))[:, None]
            d = np.where(act, dh[t], 0.0)                                     # dead frames of dh may hold anything
            if s:
                d = d + q(pz[order[s - 1]]) @ RTq
            ia, ja, fa, oa = (g[t][:, c] for c in cols)
            cn = cs[t]
            tc = np.tanh(cn)
            do_pre = d * tc * oa * (1 - oa)
            dcn = dc + d * oa * (1 - tc * tc) + do_pre * wo
            di_pre = dcn * ja * ia * (1 - ia)
            dj_pre = dcn * ia * (1 - ja * ja)
            df_pre = dcn * cp * fa * (1 - fa)
            dc = np.where(act, dcn * fa + di_pre * wi + df_pre * wf, 0.0)
            for c, v in zip(cols, (di_pre, dj_pre, df_pre, do_pre)):
                dz[t][:, c] = np.where(act, v, 0.0)
    dpeep, dbias = param_sums(dz, cs, reverse)
    return dz, dpeep, dbias


# ------------------------------------------------------------------------------------------------ problems
VARIANTS = {"a": dict(pattern="mixed", garbage=1e30), "b": dict(pattern="short", garbage=float("nan"))}


class Problem:
    """One call's inputs as float32 numpy arrays (module docstring); ``dirs[d]``: zx, R, w (3 arrays or None), dh, dpeep0,
    dbias0 (the start of the accumulated outputs; dbias0 None = dbias is passed as NULL), reverse.  ``poisoned(name, d)``:
    that input with the variant's garbage in its dead frames; without, dead frames of zx / dh are +0."""

    def __init__(self, case, variant, pattern=None):
        self.case, self.variant = case, variant
        self.pattern = pattern or VARIANTS[variant]["pattern"]
        self.garbage = VARIANTS[variant]["garbage"]
        N, ndir, B, T = case.N, case.ndir, case.B, case.T
        self.seq = lengths(self.pattern, B, T)
        self.live = np.arange(T)[:, None] < self.seq[None, :]                 # [T, B]
        rng = np.random.default_rng([N, ndir, B, T, ord(variant), len(case.entry)])
        f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
        self.dirs = []
        for d in range(ndir):
            dd = dict(zx=f32(0.5 * rng.standard_normal((T, B, 4 * N))), R=f32(0.5 / np.sqrt(N) * rng.standard_normal((N, 4 * N))),
                      dh=f32(0.1 * rng.standard_normal((T, B, N))), reverse=int(d == 1 or (ndir == 1 and B % 2 == 0)))
            peep = [f32(0.2 * rng.standard_normal(N)) for _ in range(3)]
            dd["w"] = peep if variant == "a" and d == 0 else None
            dd["dpeep0"] = f32(0.1 * rng.standard_normal((3, N)))
            dd["dbias0"] = f32(0.1 * rng.standard_normal(4 * N))
            if variant == "b" and (d == 0 and ndir == 2 or ndir == 1 and (case.entry, N) in NULL_DBIAS_1DIR):
                dd["dbias0"] = None
            for k in ("zx", "dh"):
                dd[k][~self.live] = 0.0
            self.dirs.append(dd)

    def poisoned(self, name, d):
        a = self.dirs[d][name].copy()
        a[~self.live] = self.garbage
        return a


@functools.lru_cache(maxsize=None)
def reference(case, variant, pattern=None):
    """Free-running float64 reference of a problem: per direction dict(gates, cs, hs, dz, dpeep, dbias).  Computed once per
    (case, variant, pattern) and shared; callers must not write into it."""
    p = Problem(case, variant, pattern)
    out = []
    for dd in p.dirs:
        gates, cs, hs = ref_fwd(dd["zx"], dd["R"], dd["w"], p.seq, FORGET_BIAS, dd["reverse"])
        dz, dpeep, dbias = ref_bwd(gates, cs, dd["R"], dd["w"], p.seq, dd["dh"], dd["reverse"])
        out.append(dict(gates=gates, cs=cs, hs=hs, dz=dz, dpeep=dpeep, dbias=dbias))
    return out


# ------------------------------------------------------------------------------------------------ the host tests
@pytest.mark.parametrize("peep", [True, False], ids=["peepholes", "no_peepholes"])
@pytest.mark.parametrize("reverse", [0, 1], ids=["forward", "reverse"])
@pytest.mark.parametrize("N", [8, 16, 24])
def test_reference_agrees_with_the_c_oracle(oracle, N, reverse, peep):
    T, B = 6, 7
    rng = np.random.default_rng(100 * N + 2 * reverse + peep)
    seq = np.array([T - 1, 0, T, 1, T - 2, T, 3], np.int32)
    assert {0, 1, T - 1, T} <= set(seq.tolist())
    live = np.arange(T)[:, None] < seq[None, :]
    zx = 0.5 * rng.standard_normal((T, B, 4 * N))
    R = 0.5 / np.sqrt(N) * rng.standard_normal((N, 4 * N))
    dh = 0.1 * rng.standard_normal((T, B, N))
    w = [0.2 * rng.standard_normal(N) for _ in range(3)] if peep else None
    gates, cs, hs = ref_fwd(zx, R, w, seq, FORGET_BIAS, reverse)
    dz, dpeep, dbias = ref_bwd(gates, cs, R, w, seq, dh, reverse)
    for a in (gates, cs, hs, dz):
        assert not a[~live].any()
    assert np.abs(hs[live]).max() > 0.05 and np.abs(dz[live]).max() > 1e-3

    bt = lambda a: np.ascontiguousarray(np.swapaxes(a, 0, 1))               # [T,B,*] -> [B,T,*]
    rev = (lambda a: oracle.reverse_sequence(a, seq)) if reverse else (lambda a: a)
    kernel = np.vstack([np.eye(4 * N), interleaved_to_tf(R, N)])
    ow = (None, None, None) if w is None else w
    _, saved = oracle.lstmp_fwd(rev(bt(interleaved_to_tf(zx, N))), seq, kernel, np.zeros(4 * N), ow[0], ow[1], ow[2], None,
                                FORGET_BIAS)
    dx, grads = oracle.lstmp_bwd(saved, kernel, ow[0], ow[1], ow[2], None, rev(bt(dh)))
    worst = 0.0
    for mine, theirs in ((interleaved_to_tf(gates, N), saved["gates"]), (cs, saved["cs"]), (hs, saved["mp"]),
                         (interleaved_to_tf(dz, N), dx)):
        theirs = np.swapaxes(rev(theirs), 0, 1)
        worst = max(worst, np.abs(mine[live] - theirs[live]).max())
    worst = max(worst, np.abs(interleaved_to_tf(dbias, N) - grads["bias"]).max())
    if peep:
        for k, name in enumerate(("w_f_diag", "w_i_diag", "w_o_diag")):
            worst = max(worst, np.abs(dpeep[k] - grads[name]).max())
    assert worst < 1e-12, worst


def test_forced_steps_reproduce_the_free_run():
    """Forcing a run with its own outputs changes nothing, with and without operand rounding."""
    from oracle.oracle import bf16_round
    p = Problem(BF16_CASES[1], "a")
    dd = p.dirs[0]
    for rnd in (None, bf16_round):
        gates, cs, hs = ref_fwd(dd["zx"], dd["R"], dd["w"], p.seq, FORGET_BIAS, 1, rnd=rnd)
        again = ref_fwd(dd["zx"], dd["R"], dd["w"], p.seq, FORGET_BIAS, 1, rnd=rnd, forced=(cs, hs))
        assert all(np.array_equal(x, y) for x, y in zip((gates, cs, hs), again))
        dz, dpeep, dbias = ref_bwd(gates, cs, dd["R"], dd["w"], p.seq, dd["dh"], 1, rnd=rnd)
        again = ref_bwd(gates, cs, dd["R"], dd["w"], p.seq, dd["dh"], 1, rnd=rnd, forced=dz)
        assert all(np.array_equal(x, y) for x, y in zip((dz, dpeep, dbias), again))
    assert np.abs(ref_fwd(dd["zx"], dd["R"], dd["w"], p.seq, FORGET_BIAS, 1)[2] - hs).max() > 1e-6      # the rounding bites


def test_every_case_lands_on_the_schedule_it_names():
    words_f, words_b, mt_f, mt_b = set(), set(), set(), set()
    for c in ALL_CASES:
        assert c.T <= 6 and c.N % (32 if c.entry == "bf16" else 16) == 0, c
        ef = expected(c.entry, "fwd", c.T, c.B, c.N, c.ndir, c.persistent)
        eb = expected(c.entry, "bwd", c.T, c.B, c.N, c.ndir, c.persistent)
        assert (ef["kind"], ef["mt"]) == (KINDS[c.fwd[0]], c.fwd[1]), (c, ef)
        assert (eb["kind"], eb["mt"]) == (KINDS[c.bwd[0]], c.bwd[1]), (c, eb)
        assert eb["backward"] and not ef["backward"]
        assert ef["bf16"] == (c.entry == "bf16" and c.fwd[0] in (2, 4))
        words_f.add(c.fwd[0]); words_b.add(c.bwd[0])
        if c.fwd[0] in (3, 4):
            mt_f.add(c.fwd[1])
        if c.bwd[0] == 4:
            mt_b.add(c.bwd[1])
    assert words_f == {1, 2, 3, 4, 5, 6, 7} and words_b == {1, 2, 4, 5, 6, 7}        # 3 is a forward schedule only
    assert mt_f == {1, 2, 4} and mt_b == {1, 2}
    assert len(DEAD_GROUP_CASES) == 4 and len(ALL_ZERO_CASES) == 3
    assert {c.entry for c in ALL_ZERO_CASES} == {"f32", "x3", "bf16"}
    assert len({case_id(c) for c in ALL_CASES}) == len(ALL_CASES)


def test_dispatch_edges_of_the_restated_rule():
    kind = lambda *a, **k: expected(*a, **k)["kind"]
    assert kind("f32", "fwd", 4, 64, 512, 2) == "persistent_f32" and kind("f32", "fwd", 4, 65, 512, 2) == "launch_train"
    assert kind("f32", "bwd", 4, 128, 512, 1) == "persistent_f32" and kind("f32", "bwd", 4, 129, 512, 1) == "launch_train"
    assert kind("f32", "fwd", 3, 8, 512, 2) == "launch_train" and kind("f32", "fwd", 3, 8, 1024, 2) == "launch_train"
    assert kind("f32", "fwd", 4, 8, 528, 2) == "launch_train" and kind("bf16", "fwd", 4, 8, 528, 2) == "launch_train"
    assert kind("bf16", "fwd", 4, 8, 544, 2) == "persistent_bf16"
    assert kind("f32", "fwd", 4, 32, 1024, 2, persistent=False) == "launch_train"
    assert kind("f32", "fwd", 4, 33, 1024, 2, persistent=False) == "two_stream_train"
    assert kind("x3", "fwd", 4, 8, 896, 2) == "persistent_f32_xcd_pair" and kind("x3", "bwd", 4, 8, 1024, 2) == "persistent_x3_xcd_pair"
    assert kind("f32", "fwd", 4, 2 ** 16, 1024, 2) == "launch_train"                  # T * B * 4N * 4 = 2^32
    assert [bpad(b) for b in (1, 16, 17, 32, 33, 64, 65, 128, 129)] == [16, 16, 32, 32, 64, 64, 128, 128, 192]


def test_length_patterns_contain_what_they_claim():
    for c in ALL_CASES:
        B, T = c.B, c.T
        mixed, short = lengths("mixed", B, T), lengths("short", B, T)
        for s in (mixed, short):
            assert s.dtype == np.int32 and s.shape == (B,) and s.min() >= 0 and s.max() <= T
        assert short.max() < T
        if B == 1:
            assert mixed[0] == T and short[0] == T - 2
            continue
        assert 0 in mixed and 0 in short and mixed.max() == T and mixed[0] < T
        if T >= 2:
            assert short.max() >= 1
        if B >= 6 and T >= 4:
            assert {0, 1, T - 2, T - 1, T} <= set(mixed.tolist()) and {0, 1, T - 2, T - 3} <= set(short.tolist())
            assert list(mixed) != sorted(mixed) and list(mixed) != sorted(mixed, reverse=True)
        if B >= 17:
            assert 0 in mixed[:16] and 0 in mixed[1:15]                              # zeros inside a 16-row group
    for c in DEAD_GROUP_CASES:
        s = lengths("dead_group", c.B, c.T)
        assert c.B >= 64 and not s[16:32].any() and s[:16].any() and s[32:].max() == c.T
        if c.B > 64:
            assert s[64:].any()
    for c in ALL_ZERO_CASES:
        assert not lengths("all_zero", c.B, c.T).any()


def test_problems_are_what_the_variants_say():
    for c in ALL_CASES:
        a, b = Problem(c, "a"), Problem(c, "b")
        assert all(d["w"] is None for d in b.dirs) and a.dirs[0]["w"] is not None
        assert c.ndir == 1 or a.dirs[1]["w"] is None
        assert all(d["dbias0"] is not None for d in a.dirs) and b.dirs[-1]["dbias0"] is not None or \
            (c.ndir == 1 and (c.entry, c.N) in NULL_DBIAS_1DIR)
        assert c.ndir == 1 or b.dirs[0]["dbias0"] is None
        assert [d["reverse"] for d in a.dirs] == ([0, 1] if c.ndir == 2 else [int(c.B % 2 == 0)])
        if not a.live.all():
            assert (a.poisoned("zx", 0)[~a.live] == 1e30).all() and np.isnan(b.poisoned("dh", 0)[~b.live]).all()
        assert not a.dirs[0]["zx"][~a.live].any()
    assert {(c.entry, c.N) for c in ALL_CASES if c.ndir == 1 and Problem(c, "b").dirs[0]["dbias0"] is None} == set(NULL_DBIAS_1DIR)
    assert {Problem(c, "a").dirs[0]["reverse"] for c in ALL_CASES if c.ndir == 1} == {0, 1}
