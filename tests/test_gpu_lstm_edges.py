"""lc_lstm_fwd / lc_lstm_bwd and their split-operand and bf16 siblings at every schedule's length and pointer edges, against
the float64 reference of tests/test_lstm_edges_host.py (cases, length patterns, problems and the restated dispatch live there).

Every call goes through ``Harness``, which calls the C ABI itself and owns every buffer:

* every tensor lies between two 4 KB guard bands of a fixed byte, checked after each call;
* cs and hs are NaN before the forward call, so every element must be written;
* the forward workspace has exactly lc_lstm_fwd_workspace_bytes bytes and the backward one exactly
  lc_lstm_bwd_workspace_bytes; both are 0xFF bytes except the status word at LC_LSTM_STATUS_OFFSET, which is zeroed (all the
  header asks of a caller) and must still be 0 after each call;
* after each call ``ops.last_lstm_schedule()`` must be what ``expected`` restates for the shape.

Each case runs twice per variant, once with the variant's garbage (1e30 / NaN) in the dead frames of zx and dh and once with
+0 there: live outputs, dbias and dpeep must agree bit for bit (rows are independent in the step product and every mask is a
select), and gates, cs, hs, dz must be +0 on every dead frame.

Tolerances, all the project's own.  fp32 and split-operand entries, free-running against the reference: gates, cs, hs within
1e-4 max(1, max |ref|) (test_gpu_configs._check's bar); dz, and the increments of dbias and dpeep over their non-zero start,
through ``check_grad`` at GRAD_TOL (the start is 0.1 N(0,1), so the float32 rounding of start + gradient is 6e-8 of a value of
order 1, three orders below GRAD_TOL times the gradient's largest entry).  bf16 entry, teacher-forced from the kernel's own
previous cs / hs resp. dz with the same operand roundings: forward within 5e-5 max(1, |want|), dz per step within
3e-5 max(scale, 1) + 2e-6, dbias / dpeep against float64 sums over the kernel's own dz within 1e-4 max(1, max |want|) - the
bounds of test_gpu_configs' two teacher-forced tests, unchanged.  Every comparison puts error / allowed into MEASURED; the
last test prints the largest per (entry point, pass, schedule) and, with LC_MEASURED_DIR set, writes
lstm_edges_measured.txt there (kept as profiles/lstm_edges_measured.txt)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import GRAD_TOL, check_grad
from test_gpu_ops import ops  # noqa: F401  (fixture)
from test_lstm_edges_host import (ALL_CASES, ALL_ZERO_CASES, BF16_CASES, DEAD_GROUP_CASES, F32_CASES, FORGET_BIAS, X3_CASES,
                                  Case, Problem, case_id, expected, param_sums, ref_bwd, ref_fwd, reference)

pytestmark = pytest.mark.gpu
LC_EINVAL, LC_EWORKSPACE = -1, -3
GUARD, PATTERN = 4096, 0x5A
STATUS = 64                                   # LC_LSTM_STATUS_OFFSET
MEASURED = {}                                 # (entry, pass, schedule kind) -> largest error / allowed
FWD = {"f32": "lc_lstm_fwd", "x3": "lc_lstm_fwd_x3", "bf16": "lc_lstm_fwd_bf16"}
BWD = {"f32": "lc_lstm_bwd", "x3": "lc_lstm_bwd_x3", "bf16": "lc_lstm_bwd_bf16"}


# ----------------------------------------------------------------------------------------------- the harness
class _Buf:
    """A tensor between two guard bands.  ``stage`` (host array, optional) is what ``upload`` copies in on the current stream."""

    def __init__(self, shape, dtype=torch.float32, fill=None, stage=None):
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        self.raw = torch.full((2 * GUARD + n,), PATTERN, dtype=torch.uint8, device="cuda")
        self.t = self.raw[GUARD:GUARD + n].view(dtype).view(*shape)
        self.stage = None if stage is None else torch.from_numpy(np.ascontiguousarray(stage)).cuda()
        if fill is not None:
            self.t.fill_(fill)

    def upload(self):
        self.t.copy_(self.stage.view(self.t.shape), non_blocking=True)

    def intact(self):
        return bool((self.raw[:GUARD] == PATTERN).all()) and bool((self.raw[-GUARD:] == PATTERN).all())

    def ptr(self):
        return self.t.data_ptr()

    def host(self):
        return self.t.cpu().numpy().copy()


def _workspace(nbytes):
    b = _Buf((nbytes,), torch.uint8, fill=0xFF)
    b.t[STATUS:STATUS + 4] = 0
    return b


class Harness:
    """The buffers of one problem and the two calls on them.  The inputs of a call are copied in from staging tensors on the
    current stream right before it - behind ``spin_us`` microseconds of lc_debug_spin when set, so that a call that ran on
    another stream would read the NaN the buffers hold until then."""

    def __init__(self, problem, garbage=True, spin_us=0):
        from lstm_ctc_amd import _lib
        self.lib, self._lib = _lib.load(), _lib
        self.p, self.spin_us = problem, spin_us
        c = problem.case
        T, B, N, self.ndir = c.T, c.B, c.N, c.ndir
        nan = float("nan")
        self.seq = _Buf((B,), torch.int32, fill=-1, stage=problem.seq)
        self.d = []
        for i, dd in enumerate(problem.dirs):
            zx, dh = (problem.poisoned(k, i) if garbage else dd[k] for k in ("zx", "dh"))
            b = dict(zx=_Buf((T, B, 4 * N), fill=nan, stage=zx), R=_Buf((N, 4 * N), fill=nan, stage=dd["R"]),
                     RT=_Buf((4 * N, N), fill=nan, stage=dd["R"].T), dh=_Buf((T, B, N), fill=nan, stage=dh),
                     cs=_Buf((T, B, N), fill=nan), hs=_Buf((T, B, N), fill=nan),
                     w=None if dd["w"] is None else _Buf((3, N), fill=nan, stage=np.stack(dd["w"])),
                     dpeep=_Buf((3, N), stage=dd["dpeep0"]),
                     dbias=None if dd["dbias0"] is None else _Buf((4 * N,), stage=dd["dbias0"]))
            b["dpeep"].upload()
            if b["dbias"] is not None:
                b["dbias"].upload()
            self.d.append(b)
        self.ws_f = _workspace(self.lib.lc_lstm_fwd_workspace_bytes(B, N, self.ndir))
        self.ws_b = _workspace(self.lib.lc_lstm_bwd_workspace_bytes(B, N, self.ndir))
        torch.cuda.synchronize()

    def bufs(self):
        return [self.seq, self.ws_f, self.ws_b] + [v for b in self.d for v in b.values() if v is not None]

    def snapshot(self):
        torch.cuda.synchronize()
        return [b.raw.clone() for b in self.bufs()]

    def unchanged(self, snap):
        torch.cuda.synchronize()
        return all(torch.equal(b.raw, s) for b, s in zip(self.bufs(), snap))

    def _before(self, names, upload):
        if self.spin_us:
            from lstm_ctc_amd import ops
            ops.debug_spin(1, self.spin_us, 0)
        if upload:
            self.seq.upload()
            for b in self.d:
                for k in names:
                    if b[k] is not None:
                        b[k].upload()

    def _after(self, ws):
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:                           # a device error: start nothing more on this GPU
            pytest.exit("device error after an lc_lstm_* call of %s: %s" % (case_id(self.p.case), e), returncode=3)
        assert all(b.intact() for b in self.bufs()), "a guard band was written"
        return int(ws.t[STATUS:STATUS + 4].view(torch.int32).item())

    def _common(self, kw, ws):
        c = self.p.case
        a = dict(T=c.T, B=c.B, N=c.N, ndir=c.ndir, nbytes=ws.t.numel(), null_seq=False, null_ws=False, null_dir1=False)
        a.update(kw)
        return a

    def fwd(self, upload=True, **kw):
        """-> (return code, status word).  ``kw``: T, B, N, ndir, nbytes passed in place of the case's; null_seq / null_ws /
        null_dir1 pass NULL for seq_len / the workspace / dirs[1].zx."""
        a = self._common(kw, self.ws_f)
        arr = (self._lib.LstmFwdDir * 2)()
        for i, b in enumerate(self.d):
            arr[i].zx, arr[i].R, arr[i].cs, arr[i].hs = b["zx"].ptr(), b["R"].ptr(), b["cs"].ptr(), b["hs"].ptr()
            if b["w"] is not None:
                arr[i].w_f, arr[i].w_i, arr[i].w_o = (b["w"].t[k].data_ptr() for k in range(3))
            arr[i].reverse = self.p.dirs[i]["reverse"]
        if a["null_dir1"]:
            arr[1].zx = None
        self._before(("zx", "R", "w"), upload)
        rc = getattr(self.lib, FWD[self.p.case.entry])(
            ctypes.cast(arr, ctypes.c_void_p), a["ndir"], None if a["null_seq"] else self.seq.ptr(), a["T"], a["B"], a["N"],
            FORGET_BIAS, None if a["null_ws"] else self.ws_f.ptr(), a["nbytes"], torch.cuda.current_stream().cuda_stream)
        return rc, self._after(self.ws_f)

    def bwd(self, upload=True, **kw):
        """On the buffers the forward call left: gates -> dz in place.  ``kw`` as in fwd (null_dir1: dirs[1].gates)."""
        a = self._common(kw, self.ws_b)
        arr = (self._lib.LstmBwdDir * 2)()
        for i, b in enumerate(self.d):
            arr[i].gates, arr[i].RT, arr[i].cs, arr[i].dh = b["zx"].ptr(), b["RT"].ptr(), b["cs"].ptr(), b["dh"].ptr()
            if b["w"] is not None:
                arr[i].w_f, arr[i].w_i, arr[i].w_o = (b["w"].t[k].data_ptr() for k in range(3))
            arr[i].dpeep = b["dpeep"].ptr()
            arr[i].dbias = None if b["dbias"] is None else b["dbias"].ptr()
            arr[i].reverse = self.p.dirs[i]["reverse"]
        if a["null_dir1"]:
            arr[1].gates = None
        self._before(("RT", "dh"), upload)
        rc = getattr(self.lib, BWD[self.p.case.entry])(
            ctypes.cast(arr, ctypes.c_void_p), a["ndir"], None if a["null_seq"] else self.seq.ptr(), a["T"], a["B"], a["N"],
            None if a["null_ws"] else self.ws_b.ptr(), a["nbytes"], torch.cuda.current_stream().cuda_stream)
        return rc, self._after(self.ws_b)

    def outputs(self, names):
        return [{k: (None if b[k] is None else b[k].host()) for k in names} for b in self.d]


def run(ops, problem, garbage=True, spin_us=0):
    """Forward and backward call of one problem on buffers of its own -> per direction dict(gates, cs, hs, dz, dpeep, dbias)
    of float32 arrays (dbias None where it was passed as NULL) and the forward schedule kind."""
    c = problem.case
    h = Harness(problem, garbage, spin_us)
    if not c.persistent:
        ops.set_option("lstm_persistent", 0)
    try:
        rc, status = h.fwd()
        assert rc == 0, h.lib.lc_last_error()
        assert status == 0, "status word after the forward call"
        sf = ops.last_lstm_schedule()
        assert sf == expected(c.entry, "fwd", c.T, c.B, c.N, c.ndir, c.persistent), (case_id(c), sf)
        f = h.outputs(("zx", "cs", "hs"))
        rc, status = h.bwd()
        assert rc == 0, h.lib.lc_last_error()
        assert status == 0, "status word after the backward call"
        sb = ops.last_lstm_schedule()
        assert sb == expected(c.entry, "bwd", c.T, c.B, c.N, c.ndir, c.persistent), (case_id(c), sb)
        g = h.outputs(("zx", "dpeep", "dbias"))
    finally:
        if not c.persistent:
            ops.set_option("lstm_persistent", None)
    out = [dict(gates=a["zx"], cs=a["cs"], hs=a["hs"], dz=b["zx"], dpeep=b["dpeep"], dbias=b["dbias"]) for a, b in zip(f, g)]
    for d, o in enumerate(out):
        for k, v in o.items():
            assert v is None or np.isfinite(v).all(), (case_id(c), d, k, "NaN or Inf in an output")
        dead = ~problem.live
        for k in ("gates", "cs", "hs", "dz"):
            assert not o[k][dead].view(np.int32).any(), (case_id(c), d, k, "dead frames must be +0")
    return out, sf["kind"], sb["kind"]


def _bits_equal(a, b):
    return (a is None and b is None) or np.array_equal(a.view(np.int32), b.view(np.int32))


def _note(key, ratio):
    MEASURED[key] = max(MEASURED.get(key, 0.0), float(ratio))


def _increment(problem, d, got, name):
    return got[name].astype(np.float64) - problem.dirs[d][name + "0"].astype(np.float64)


def check_f32(tag, problem, out, kf, kb):
    """Free-running comparison with the float64 reference (fp32 and split-operand entries)."""
    e = problem.case.entry
    ref = reference(problem.case, problem.variant, problem.pattern)
    for d, (o, r) in enumerate(zip(out, ref)):
        for k in ("gates", "cs", "hs"):
            bar = 1e-4 * max(1.0, float(np.abs(r[k]).max()))
            err = float(np.abs(o[k] - r[k]).max())
            _note((e, "fwd", kf), err / bar)
            assert err <= bar, (tag, d, k, err, bar)
        grads = [("dz", o["dz"], r["dz"])]
        if o["dbias"] is not None:
            grads.append(("dbias", _increment(problem, d, o, "dbias"), r["dbias"]))
        if problem.dirs[d]["w"] is not None:
            grads.append(("dpeep", _increment(problem, d, o, "dpeep"), r["dpeep"]))
        for k, got, want in grads:
            _note((e, "bwd", kb), float(np.abs(got - want).max()) / (GRAD_TOL * max(float(np.abs(want).max()), 1e-3)))
            check_grad(got, want, tag, "dir%d/%s" % (d, k))


def check_bf16(tag, problem, out, kf, kb, rnd):
    """Teacher-forced comparison: every step from the kernel's own previous cs / hs (dz), operands rounded as the kernel's."""
    e, seq = problem.case.entry, problem.seq
    for d, (o, dd) in enumerate(zip(out, problem.dirs)):
        want = ref_fwd(dd["zx"], dd["R"], dd["w"], seq, FORGET_BIAS, dd["reverse"], rnd=rnd, forced=(o["cs"], o["hs"]))
        for k, w in zip(("gates", "cs", "hs"), want):
            err = float((np.abs(o[k] - w) / np.maximum(1.0, np.abs(w))).max())
            _note((e, "fwd", kf), err / 5e-5)
            assert err < 5e-5, (tag, d, k, err)
        dz = o["dz"].astype(np.float64)
        want, _, _ = ref_bwd(o["gates"], o["cs"], dd["R"], dd["w"], seq, dd["dh"], dd["reverse"], rnd=rnd, forced=dz)
        for t in range(problem.case.T):
            bound = 3e-5 * max(float(np.abs(want[t]).max()), 1.0) + 2e-6
            err = float(np.abs(dz[t] - want[t]).max())
            _note((e, "bwd", kb), err / bound)
            assert err < bound, (tag, d, "dz", t, err, bound)
        dpeep, dbias = param_sums(dz, o["cs"], dd["reverse"])
        sums = [("dbias", dbias)] if o["dbias"] is not None else []
        if dd["w"] is not None:
            sums.append(("dpeep", dpeep))
        for k, w in sums:
            bound = 1e-4 * max(1.0, float(np.abs(w).max()))
            err = float(np.abs(_increment(problem, d, o, k) - w).max())
            _note((e, "bwd", kb), err / bound)
            assert err < bound, (tag, d, k, err, bound)


def run_case(ops, oracle, case, variant, pattern=None):
    problem = Problem(case, variant, pattern)
    tag = "%s/%s/%s" % (case_id(case), variant, problem.pattern)
    out, kf, kb = run(ops, problem, garbage=True)
    clean, _, _ = run(ops, problem, garbage=False)
    for d, (o, z) in enumerate(zip(out, clean)):
        for k in o:
            assert _bits_equal(o[k], z[k]), (tag, d, k, "depends on what the dead frames of zx / dh hold")
        if problem.dirs[d]["w"] is None:                    # dpeep given with NULL peepholes: left alone
            assert _bits_equal(o["dpeep"], problem.dirs[d]["dpeep0"]), (tag, d, "dpeep written without peepholes")
    if case.entry == "bf16":
        check_bf16(tag, problem, out, kf, kb, oracle.bf16_round)
    else:
        check_f32(tag, problem, out, kf, kb)
    return problem, out


# ----------------------------------------------------------------------------------------------- the case tables
@pytest.mark.parametrize("variant", ["a", "b"])
@pytest.mark.parametrize("case", ALL_CASES, ids=case_id)
def test_table_case(ops, oracle, case, variant):
    run_case(ops, oracle, case, variant)


@pytest.mark.parametrize("case", DEAD_GROUP_CASES, ids=case_id)
def test_dead_row_group(ops, oracle, case):
    """Rows 16..31 all of length 0: a whole 16-row group (a quarter of a 64-row block) with nothing to do."""
    run_case(ops, oracle, case, "a", "dead_group")


@pytest.mark.parametrize("case", ALL_ZERO_CASES, ids=case_id)
def test_all_zero_lengths(ops, oracle, case):
    problem, out = run_case(ops, oracle, case, "a", "all_zero")
    for d, o in enumerate(out):
        for k in ("gates", "cs", "hs", "dz"):
            assert not o[k].view(np.int32).any(), (case_id(case), d, k)
        for k in ("dpeep", "dbias"):
            assert _bits_equal(o[k], problem.dirs[d][k + "0"]), (case_id(case), d, k)


# ----------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("entry", ["f32", "x3", "bf16"])
def test_refusals_launch_nothing(ops, oracle, entry):
    """Both passes of the entry point: a refused call returns its code, writes no byte of any buffer (outputs, workspace and
    status word included) and leaves lc_debug_last_lstm_schedule() as it was; a good call on the same buffers then passes."""
    case = Case(entry, 32, 2, 3, 4, True, None, None, "")
    problem = Problem(case, "a")
    h = Harness(problem)
    lib = h.lib
    bad = [dict(T=0), dict(B=0), dict(ndir=3), dict(N=24), dict(N=8), dict(null_seq=True), dict(null_dir1=True), dict(null_ws=True)]
    if entry == "bf16":
        bad.append(dict(N=48))
    for call, who, ws in ((h.fwd, FWD[entry], h.ws_f), (h.bwd, BWD[entry], h.ws_b)):
        if ws is h.ws_b:                                    # the backward refusals meet what a good forward call left
            rc, status = h.fwd()
            assert rc == 0 and status == 0, lib.lc_last_error()
        word = lib.lc_debug_last_lstm_schedule()
        snap = h.snapshot()
        for kw in bad:
            rc, status = call(upload=False, **kw)
            assert rc == LC_EINVAL and status == 0 and h.unchanged(snap), (who, kw, rc)
            assert lib.lc_debug_last_lstm_schedule() == word, (who, kw)
        rc, status = call(upload=False, nbytes=ws.t.numel() - 1)
        assert rc == LC_EWORKSPACE and status == 0 and h.unchanged(snap), (who, rc)
        assert lib.lc_last_error().decode().startswith(who + ": workspace too small"), lib.lc_last_error()
        assert lib.lc_debug_last_lstm_schedule() == word, who
    f = h.outputs(("zx", "cs", "hs"))
    rc, status = h.bwd()
    assert rc == 0 and status == 0, lib.lc_last_error()
    g = h.outputs(("zx", "dpeep", "dbias"))
    out = [dict(gates=a["zx"], cs=a["cs"], hs=a["hs"], dz=b["zx"], dpeep=b["dpeep"], dbias=b["dbias"]) for a, b in zip(f, g)]
    kf, kb = (expected(entry, p, 4, 3, 32, 2)["kind"] for p in ("fwd", "bwd"))
    assert ops.last_lstm_schedule()["kind"] == kb
    if entry == "bf16":
        check_bf16("after refusals", problem, out, kf, kb, oracle.bf16_round)
    else:
        check_f32("after refusals", problem, out, kf, kb)


# ----------------------------------------------------------------------------------------------- workspace and stream
def _through_ops(ops, problem):
    """The same problem through ops.lstm_fwd / ops.lstm_bwd and their cached per-stream workspace."""
    c = problem.case
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    kw = dict(bf16=c.entry == "bf16", x3=c.entry == "x3")
    seq = dev(problem.seq)
    fd, bd = [], []
    for i, dd in enumerate(problem.dirs):
        w = [None] * 3 if dd["w"] is None else [dev(v) for v in dd["w"]]
        fd.append(dict(zx=dev(problem.poisoned("zx", i)), R=dev(dd["R"]), w_f=w[0], w_i=w[1], w_o=w[2],
                       cs=torch.full((c.T, c.B, c.N), float("nan"), device="cuda"),
                       hs=torch.full((c.T, c.B, c.N), float("nan"), device="cuda"), reverse=dd["reverse"]))
    ops.lstm_fwd(fd, seq, c.T, c.B, c.N, FORGET_BIAS, **kw)
    assert ops.last_lstm_schedule() == expected(c.entry, "fwd", c.T, c.B, c.N, c.ndir)
    gates = [d["zx"].cpu().numpy().copy() for d in fd]
    for i, dd in enumerate(problem.dirs):
        bd.append(dict(gates=fd[i]["zx"], RT=dev(dd["R"].T), w_f=fd[i]["w_f"], w_i=fd[i]["w_i"], w_o=fd[i]["w_o"], cs=fd[i]["cs"],
                       dh=dev(problem.poisoned("dh", i)), dpeep=dev(dd["dpeep0"]),
                       dbias=None if dd["dbias0"] is None else dev(dd["dbias0"]), reverse=dd["reverse"]))
    ops.lstm_bwd(bd, seq, c.T, c.B, c.N, **kw)
    assert ops.last_lstm_schedule() == expected(c.entry, "bwd", c.T, c.B, c.N, c.ndir)
    torch.cuda.synchronize()
    host = lambda t: None if t is None else t.cpu().numpy()
    return [dict(gates=gates[i], cs=host(fd[i]["cs"]), hs=host(fd[i]["hs"]), dz=host(bd[i]["gates"]), dpeep=host(bd[i]["dpeep"]),
                 dbias=host(bd[i]["dbias"])) for i in range(c.ndir)]


def test_stale_workspace_is_ignored(ops, oracle):
    """ops.lstm_fwd / ops.lstm_bwd keep one workspace per stream.  A full-width bf16 call leaves its exchange buffers as
    0xFF "not arrived" sentinels and its tagged data behind; a small fp32 call and a small split-operand call right after it
    run on that, and must give, bit for bit, what ``run`` gives on a fresh 0xFF workspace of the exact size."""
    big = Problem(BF16_CASES[3], "a")
    assert (big.case.N, big.case.B) == (1024, 64)
    for small in (Problem(F32_CASES[1], "a"), Problem(X3_CASES[0], "a")):
        _through_ops(ops, big)
        got = _through_ops(ops, small)
        assert int(ops.lstm_status("cuda").item()) == 0
        fresh, kf, kb = run(ops, small)
        for d, (o, z) in enumerate(zip(got, fresh)):
            for k in o:
                assert _bits_equal(o[k], z[k]), (case_id(small.case), d, k)
        check_f32("stale workspace", small, got, kf, kb)


STREAM_CASES = [F32_CASES[1], F32_CASES[9], F32_CASES[12], F32_CASES[5]]      # kinds 1, 3, 4, 5


@pytest.mark.parametrize("case", STREAM_CASES, ids=case_id)
def test_runs_on_the_callers_stream(ops, oracle, case):
    """Forward and backward inside torch.cuda.stream(side), the inputs written by copies queued on ``side`` behind 3 ms of
    lc_debug_spin: a launch (or an internal memset) on any other stream would read the NaN the buffers hold until then.
    The two-stream forward runs a second time from a high-priority stream, where it must pick its low-priority sibling."""
    assert expected("f32", "fwd", case.T, case.B, case.N, case.ndir)["kind"] == \
        {48: "persistent_f32", 1024: "two_stream_train", 32: "launch_train", 640: "persistent_f32_xcd_pair"}[case.N]
    problem = Problem(case, "a")
    sides = [torch.cuda.Stream()] + ([torch.cuda.Stream(priority=-1)] if case.N == 1024 else [])
    for side in sides:
        with torch.cuda.stream(side):
            out, kf, kb = run(ops, problem, spin_us=3000)
        check_f32("side stream", problem, out, kf, kb)


# ----------------------------------------------------------------------------------------------- report
def test_zz_report_measured():
    lines = ["# lc_lstm_*, tests/test_gpu_lstm_edges.py: largest measured error / allowed, per entry point, pass and schedule",
             "# f32 / x3, free-running against float64: fwd 1e-4 max(1, max |ref|); bwd GRAD_TOL max(max |ref|, 1e-3)",
             "# bf16, teacher-forced: fwd 5e-5 max(1, |want|); bwd dz 3e-5 max(scale, 1) + 2e-6, dbias / dpeep 1e-4 max(1, max |want|)"]
    lines += ["%-5s %-4s %-24s %.4f" % (k + (v,)) for k, v in sorted(MEASURED.items())]
    print("\n" + "\n".join(lines))
    out = os.environ.get("LC_MEASURED_DIR")              # where to keep the table; unset: printed only
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "lstm_edges_measured.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
    assert MEASURED and all(v <= 1.0 for v in MEASURED.values())
