"""lc_ctc_loss_star (transcript-tolerant CTC: every lattice position may explain a frame by a penalised star, "some non-blank
class"; the loss, the expected number of star frames and the exact gradient) on the GPU, through every layer: kernel, ops,
CTCGraph, command lines.

Reference: ``star_ctc_ref`` of tests/test_ctc_star_host.py - float64 numpy, anchored there against brute-force enumeration of
all paths x own-or-star choices, central differences, the oracle's plain CTC and the concavity sandwich - evaluated on the
same fp32 logits.

Tolerances are the project's bar (tests/conftest.py GRAD_TOL = 1e-4), not new numbers: loss and star_frames within
GRAD_TOL max(|ref|, 1) of float64, a gradient through ``check_grad``, live gradient rows summing to 0 within V GRAD_TOL.
Every kernel call runs on guarded output buffers (a band of sentinels on either side, checked after the call), NaN-filled
outputs and a workspace of 0xFF bytes between guard bands.  The last test prints the largest measured / bar ratios and, with
LC_MEASURED_DIR set, writes them to ctc_star_measured.txt in that directory (kept as profiles/ctc_star_measured.txt).
Measured over this whole file on an MI355X: star_frames at 0.0077 of its bar (130 times inside it - it is a sum of products of
quantities that are each good to a few fp32 ulps, folded in double), the loss at 0.017, the gradient at 0.63 (one fp32 ulp of a
row whose largest element is 2e-3).  The star_frames bar is left where the project has it."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GRAD_TOL, check_grad
from test_ctc_star_host import DETECT_PENALTY, DETECT_TRANSCRIPTS, DETECT_V, detection_logits, star_ctc_ref
from test_ctc_window_host import OPEN, random_path
from test_gpu_ctc_delay import GEOMETRY, _b65, _guarded, _intact, _long_case, make_case
from test_gpu_ctc_window import SMOKE_CFG, Case, _dev, _smoke_batch, feasible_utts, make_labels, need_frames, windows_around

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = GRAD_TOL
INF = float("inf")
LC_EINVAL, LC_EWORKSPACE = -1, -3
MEASURED = {"loss": 0.0, "star": 0.0, "grad": 0.0, "n": 0}
bits = lambda a: a.view(np.int32)


# ----------------------------------------------------------------------------------------------- calling the kernel
def call(case, penalty, want_grad=True, windowed=None):
    """One lc_ctc_loss_star call -> (loss, star_frames, grad or None) on the host."""
    from lstm_ctc_amd import _lib
    lib = _lib.load()
    T, B, V = case.T, case.B, case.V
    windowed = case.windowed if windowed is None else windowed
    x, flat, offs, seq = (_dev(case.x, np.float32), _dev(case.flat if len(case.flat) else np.zeros(1), np.int32),
                          _dev(case.offs, np.int32), _dev(case.seq, np.int32))
    lo = _dev(case.lo if len(case.lo) else np.zeros(1), np.int32) if windowed else None
    hi = _dev(case.hi if len(case.hi) else np.zeros(1), np.int32) if windowed else None
    nbytes = lib.lc_ctc_star_workspace_bytes(T, B, V, case.maxlen)
    assert nbytes > 0
    wsbuf = torch.full((nbytes + 512,), 0xA5, dtype=torch.uint8, device="cuda")
    ws = wsbuf[256:256 + nbytes]
    ws.fill_(0xFF)
    nan = float("nan")
    lbuf, loss = _guarded((B,), nan)
    sbuf, star = _guarded((B,), nan)
    gbuf, grad = _guarded((T, B, V), nan) if want_grad else (None, None)
    p = lambda t: None if t is None else t.data_ptr()
    rc = lib.lc_ctc_loss_star(p(x), T, B, V, p(flat), p(offs), p(seq), case.maxlen, p(lo), p(hi), float(penalty[0]),
                              float(penalty[1]), p(loss), p(star), p(grad), p(ws), nbytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, lib.lc_last_error()
    assert _intact(lbuf) and _intact(sbuf) and (gbuf is None or _intact(gbuf)), "a guard band was written"
    assert bool((wsbuf[:256] == 0xA5).all()) and bool((wsbuf[256 + nbytes:] == 0xA5).all()), "the workspace's guards were written"
    host = lambda t: None if t is None else t.cpu().numpy().copy()
    return host(loss), host(star), host(grad)


def reference(case, b, penalty, windowed=None):
    Tb, labels, lo, hi = case.utts[b]
    windowed = case.windowed if windowed is None else windowed
    return star_ctc_ref(case.x[:Tb, b].astype(np.float64), labels, penalty[0], penalty[1], case.V - 1,
                        *((lo, hi) if windowed else (None, None)))


def check_against_reference(case, penalty, loss, star, grad, tag, utterances=None, windowed=None):
    """Loss, star_frames and gradient of every utterance: compared with the reference, or one of the convention cases, which
    are asserted exactly."""
    for b in (range(case.B) if utterances is None else utterances):
        Tb, labels = case.utts[b][0], np.asarray(case.utts[b][1])
        gb = None if grad is None else grad[:, b]
        if gb is not None:
            assert np.array_equal(bits(gb[Tb:]), np.zeros_like(gb[Tb:], np.int32)), (tag, b, "rows beyond seq_len")
        if Tb <= 0 or len(labels) > Tb:
            assert loss[b] == 0.0 and star[b] == 0.0 and (gb is None or not gb.any()), (tag, b, "skipped utterance")
            continue
        ref = reference(case, b, penalty, windowed)
        if not np.isfinite(ref["loss"]):
            assert loss[b] == np.inf and star[b] == 0.0, (tag, b, loss[b], star[b])
            if gb is not None:
                assert not np.isnan(gb).any()
                check_grad(gb[:Tb], ref["grad"], tag, "utt%d/softmax" % b)
            continue
        err = abs(float(loss[b]) - ref["loss"])
        serr = abs(float(star[b]) - ref["star_frames"])
        lbar, sbar = BAR * max(abs(ref["loss"]), 1.0), BAR * max(abs(ref["star_frames"]), 1.0)
        gerr = gbar = 0.0
        if gb is not None:
            gerr = float(np.abs(gb[:Tb] - ref["grad"]).max())
            gbar = BAR * max(float(np.abs(ref["grad"]).max()), 1e-3)
            MEASURED["grad"] = max(MEASURED["grad"], gerr / gbar)
        print("%s utt %d: T_b %d L %d  loss %.6f ref %.6f err %.2e (bar %.2e)  star_frames %.6f ref %.6f err %.2e (bar %.2e)  "
              "grad err %.2e (bar %.2e)" % (tag, b, Tb, len(labels), loss[b], ref["loss"], err, lbar, star[b],
                                            ref["star_frames"], serr, sbar, gerr, gbar))
        MEASURED["loss"] = max(MEASURED["loss"], err / lbar)
        MEASURED["star"] = max(MEASURED["star"], serr / sbar)
        MEASURED["n"] += 1
        assert star[b] >= 0.0, (tag, b, star[b])
        assert err <= lbar, (tag, b, loss[b], ref["loss"])
        assert serr <= sbar, (tag, b, star[b], ref["star_frames"])
        if gb is not None:
            assert not np.isnan(gb).any(), (tag, b)
            check_grad(gb[:Tb], ref["grad"], tag, "utt%d" % b)
            assert np.abs(gb[:Tb].sum(axis=1)).max() <= case.V * BAR, (tag, b, "live rows sum to 0")


# ----------------------------------------------------------------------------------------------- 1. geometry
@pytest.mark.parametrize("penalty", [(0.5, 1.5), (2.0, INF)])
@pytest.mark.parametrize("L,V", GEOMETRY)
def test_geometry_edges(L, V, penalty):
    """test_gpu_ctc_delay's geometry list (the positions-per-lane switches; V = 2: the star is the only label): ragged
    batches, T_b = frames needed + {0, 1, 3, 7}, plus an empty, a skipped and an infeasible utterance; half of the cases carry
    windows around a random path."""
    idx = GEOMETRY.index((L, V))
    windowed = (idx + (penalty[0] == 2.0)) % 2 == 1
    rng = np.random.RandomState(3000 * V + L + (7 if penalty[0] == 2.0 else 0))
    utts = feasible_utts(rng, V, L)                                              # the last one is empty (T_b = 0)
    utts.append((2, np.zeros(3, np.int64), np.zeros(3), np.full(3, OPEN)))      # skipped: more labels than frames
    if windowed and L:
        labels = make_labels(rng, V, L)
        Tb = need_frames(labels) + 3
        lo, hi = windows_around(rng, random_path(rng, labels, Tb), L)
        lo[L // 2], hi[L // 2] = 5, 4                                            # infeasible: a label without a frame
        utts.append((Tb, labels, lo, hi))
    else:
        utts.append((2, np.zeros(2, np.int64), np.zeros(2), np.full(2, OPEN)))  # infeasible: no frame for the blank between
    case = make_case(rng, V, utts, windowed)
    loss, star, grad = call(case, penalty)
    assert loss[-1] == np.inf and loss[-2] == 0.0 and loss[-3] == 0.0
    assert star[-1] == 0.0 and star[-2] == 0.0 and star[-3] == 0.0
    check_against_reference(case, penalty, loss, star, grad, "geom L%d V%d p%s%s" % (L, V, penalty, " win" if windowed else ""))


def test_one_frame_and_one_utterance():
    rng = np.random.RandomState(1)
    for V in (2, 44):
        for labels in ([], [0]):
            for windowed in (False, True):
                case = make_case(rng, V, [(1, np.array(labels, np.int64), np.zeros(len(labels)), np.zeros(len(labels)))], windowed)
                loss, star, grad = call(case, (0.7, 0.2))                         # T = 1, B = 1: one path, its cell still a mixture
                assert 0.0 < star[0] < 1.0
                check_against_reference(case, (0.7, 0.2), loss, star, grad, "T1B1 V%d L%d" % (V, len(labels)))


# ----------------------------------------------------------------------------------------------- 2. rows not a multiple of four
@pytest.mark.parametrize("windowed", [False, True])
def test_b65_ragged_and_unsorted(windowed):
    """B = 65: more utterances than one wave's lanes, T * B not a multiple of the four frames of a workgroup."""
    rng = np.random.RandomState(2)
    case = make_case(rng, 44, _b65(rng), windowed, T=23)
    assert (case.T * case.B) % 4
    loss, star, grad = call(case, (1.0, 2.0))
    check_against_reference(case, (1.0, 2.0), loss, star, grad, "B65")


# ----------------------------------------------------------------------------------------------- 3. one long case
def test_long_utterances_sandwich_and_monotonicity():
    """T = 1000: against the reference at p = 1, and the GPU's own values at p = 0.5, 1, 2, 4 against each other: for p0 < p1,
    loss(p0) + star_frames(p1) (p1 - p0) <= loss(p1) <= loss(p0) + star_frames(p0) (p1 - p0) (the loss is concave in p, its
    slope is star_frames), star_frames does not grow with p, and loss(p) <= the plain loss - each within the bars."""
    case = _long_case(1000, 44, 100, 4, False)
    ps = (0.5, 1.0, 2.0, 4.0)
    res = {p: call(case, (p, p), want_grad=(p == 1.0)) for p in ps}
    check_against_reference(case, (1.0, 1.0), *res[1.0], "T1000")
    plain = call(case, (INF, INF), want_grad=False)[0].astype(np.float64)
    tol = lambda v: BAR * np.maximum(np.abs(v), 1.0)
    for p0, p1 in zip(ps, ps[1:]):
        l0, s0, l1, s1 = (res[p0][0].astype(np.float64), res[p0][1].astype(np.float64), res[p1][0].astype(np.float64),
                          res[p1][1].astype(np.float64))
        assert np.isfinite(l0).all() and np.isfinite(l1).all() and (s0 > 0).all()
        lower, upper = l0 + s1 * (p1 - p0), l0 + s0 * (p1 - p0)
        assert (lower <= l1 + tol(l1) + tol(s1) * (p1 - p0)).all(), (p0, p1, lower, l1)
        assert (l1 <= upper + tol(upper) + tol(s0) * (p1 - p0)).all(), (p0, p1, l1, upper)
        assert (s1 <= s0 + tol(s0)).all() and (l1 <= plain + tol(plain)).all(), (p0, p1)
    assert (res[4.0][1] < res[0.5][1]).all() and (res[0.5][0] < plain).all()      # the penalty does bite


# ----------------------------------------------------------------------------------------------- 4. the siblings, bit for bit
@pytest.mark.parametrize("L,V", [(5, 8), (100, 8), (1023, 8)])
def test_infinite_penalties_are_the_siblings_bit_for_bit(L, V):
    """One sweep template and one gradient kernel under all entries: with both penalties +inf, loss and grad are
    lc_ctc_loss_windowed's with windows and lc_ctc_loss_delay's at lambda = 0 without, bit for bit, and star_frames is +0.
    Positions per lane 1, 4 and 32; a feasible utterance, one whose window excludes every frame (+inf, softmax rows) and one
    with a bad label (NaN, zero rows)."""
    from lstm_ctc_amd import ops
    rng = np.random.RandomState(6000 + 10 * L + V)
    utts = []
    for kind in ("fine", "no path", "bad label"):
        labels = make_labels(rng, V, L)
        Tb = need_frames(labels) + 3
        lo, hi = windows_around(rng, random_path(rng, labels, Tb), L)
        if kind == "no path":
            lo[L // 2], hi[L // 2] = Tb, -1
        if kind == "bad label":
            labels[L // 2] = V - 1
        utts.append((Tb, labels, lo, hi))
    case = make_case(rng, V, utts, True)
    dev = (_dev(case.x, np.float32), _dev(case.flat, np.int32), _dev(case.offs, np.int32), _dev(case.seq, np.int32))
    lo_d, hi_d = _dev(case.lo, np.int32), _dev(case.hi, np.int32)
    loss_w, grad_w = (t.cpu().numpy() for t in ops.ctc_loss_windowed(*dev, case.maxlen, lo_d, hi_d))
    loss_d, _, grad_d = ops.ctc_loss_delay(*dev, case.maxlen, 0.0, want_entry=False)
    loss_d, grad_d = loss_d.cpu().numpy(), grad_d.cpu().numpy()
    for windowed, want_loss, want_grad in ((True, loss_w, grad_w), (False, loss_d, grad_d)):
        loss, star, grad = call(case, (INF, INF), windowed=windowed)
        assert np.isfinite(loss[0]) and np.isnan(loss[2]) and (loss[1] == np.inf) == windowed
        assert np.array_equal(bits(loss), bits(want_loss)) and np.array_equal(bits(grad), bits(want_grad))
        assert np.array_equal(bits(star[:2]), np.zeros(2, np.int32)) and np.isnan(star[2])      # +0, and NaN for the bad label
        some = call(case, (1.0, 1.0), windowed=windowed)
        assert some[0][0] < loss[0] and some[1][0] > 0 and not np.array_equal(some[2][:, 0], grad[:, 0])


# ----------------------------------------------------------------------------------------------- 5. outputs and determinism
def test_optional_gradient_and_bit_identical_calls():
    rng = np.random.RandomState(6)
    V = 44
    utts = feasible_utts(rng, V, 70) + feasible_utts(rng, V, 9, slack=(0, 30))
    utts.append((50, make_labels(rng, V, 4), np.array([0, 9, 0, 0]), np.array([OPEN, 3, OPEN, OPEN])))      # no path
    utts.append((3, make_labels(rng, V, 9), np.zeros(9), np.full(9, OPEN)))                                    # skipped
    case = make_case(rng, V, utts, True)
    full = call(case, (0.5, 1.5))
    again = call(case, (0.5, 1.5))
    for a, b in zip(full, again):
        assert np.array_equal(bits(a), bits(b))                          # two calls are bit-identical
    no_grad = call(case, (0.5, 1.5), want_grad=False)
    assert no_grad[2] is None
    assert np.array_equal(bits(no_grad[0]), bits(full[0])) and np.array_equal(bits(no_grad[1]), bits(full[1]))
    check_against_reference(case, (0.5, 1.5), full[0], full[1], full[2], "coverage")
    check_against_reference(case, (0.5, 1.5), no_grad[0], no_grad[1], None, "coverage, no gradient")


# ----------------------------------------------------------------------------------------------- 6. the detection case
def test_detection_case_matches_the_reference():
    """tests/test_ctc_star_host.py's detection case, (T, B, V) = (18, 4, 8): the clean transcript and the three wrong ones
    side by side, seeds 0..19.  Every GPU value within the bars of its reference value; the >= 0.5 margin itself is asserted
    on the reference values in the host file (its seed-wise minimum of 0.706 leaves room for that there, not here)."""
    kinds = list(DETECT_TRANSCRIPTS)
    for seed in range(20):
        x = detection_logits(seed)
        T = x.shape[0]
        utts = [(T, np.array(DETECT_TRANSCRIPTS[k], np.int64), np.zeros(len(DETECT_TRANSCRIPTS[k])),
                 np.full(len(DETECT_TRANSCRIPTS[k]), OPEN)) for k in kinds]
        case = make_case(np.random.RandomState(seed), DETECT_V, utts, False, T=T)
        case.x[:] = x[:, None, :].astype(np.float32)
        assert (case.T, case.B, case.V) == (18, 4, 8)
        loss, star, grad = call(case, DETECT_PENALTY)
        check_against_reference(case, DETECT_PENALTY, loss, star, grad, "detect seed %d" % seed)


# ----------------------------------------------------------------------------------------------- 7. -inf logits
def test_frame_without_non_blank_mass_and_conventions():
    """At one live frame every non-blank logit is -inf: the frame has no star and no label, the paths pass it in a blank;
    the values are the reference's and no NaN appears.  Plus lc_ctc_loss's conventions, with and without a gradient."""
    rng = np.random.RandomState(5)
    V, T = 7, 12
    open3 = (np.zeros(3), np.full(3, OPEN))
    utts = [
        (T, np.array([1, 2, 3]), np.array([0, 3, 6]), np.array([4, 8, 11])),         # 0 fine
        (2, np.array([1, 2, 3])) + open3,                                            # 1 L > T_b: loss 0, star 0, gradient 0
        (T, np.array([1, 6, 3])) + open3,                                            # 2 the blank as a label: NaN, NaN, gradient 0
        (T, np.array([1, -1, 3])) + open3,                                           # 3 a negative label: NaN, NaN, gradient 0
        (T, np.array([1, 2, 3]), np.array([0, 5, 0]), np.array([11, 4, 11])),        # 4 an empty window: +inf, 0, softmax
        (T, np.array([1, 2, 3]), np.array([6, 0, 0]), np.array([11, 3, 11])),        # 5 windows force the wrong order
        (2, np.array([2, 2]), np.zeros(2), np.full(2, OPEN)),                        # 6 L fits, the blank between does not
        (T - 1, np.array([4, 4, 0]), np.array([0, 2, 0]), np.array([3, 9, OPEN])),   # 7 fine; frame 5 has no non-blank mass
        (0, np.array([1])) + (np.zeros(1), np.full(1, OPEN)),                        # 8 no frames
        (5, np.zeros(0, np.int64), np.zeros(0), np.zeros(0)),                        # 9 L = 0; frame 2 has no non-blank mass
        (3, np.array([0, 1, 2])) + open3,                                            # 10 T_b = L: one path, every cell a mixture
        (3, np.array([0, 1, 2])) + open3,                                            # 11 the same, frame 1 without non-blank mass
    ]
    for windowed in (True, False):
        case = make_case(rng, V, utts, windowed, T=T)
        case.x[5, 7, :V - 1] = -np.inf
        case.x[2, 9, :V - 1] = -np.inf
        case.x[1, 11, :V - 1] = -np.inf                                              # its label has no frame left: no path
        for penalty in ((0.5, 1.5), (INF, 1.0)):
            for want_grad in (True, False):
                loss, star, grad = call(case, penalty, want_grad=want_grad)
                assert np.isnan(loss[[2, 3]]).all() and np.isnan(star[[2, 3]]).all()
                assert loss[1] == 0.0 and loss[8] == 0.0 and star[1] == 0.0 and star[8] == 0.0
                infeasible = [4, 5, 6, 11] if windowed else [6, 11]
                assert (loss[infeasible] == np.inf).all() and (star[infeasible] == 0.0).all()
                rest = [b for b in range(12) if b not in (2, 3)]
                assert not np.isnan(loss[rest]).any() and not np.isnan(star[rest]).any()
                assert np.isfinite(loss[[0, 7, 9, 10]]).all() and (star[[0, 7, 9]] > 0).all()
                assert (star[10] > 0) == np.isfinite(penalty[0])                 # one path through label positions only
                if want_grad:
                    assert not grad[:, [1, 2, 3, 8]].any() and not np.isnan(grad).any()
                check_against_reference(case, penalty, loss, star, grad, "conventions", utterances=rest)


# ----------------------------------------------------------------------------------------------- 8. errors
def test_argument_checks_launch_nothing():
    from lstm_ctc_amd import _lib
    lib = _lib.load()
    rng = np.random.RandomState(7)
    V = 10
    case = Case(rng, V, feasible_utts(rng, V, 3, slack=(0, 2), empty=False))
    T, B = case.T, case.B
    nbytes = lib.lc_ctc_star_workspace_bytes(T, B, V, case.maxlen)
    nan = float("nan")
    lbuf, loss = _guarded((B,), nan)
    sbuf, star = _guarded((B,), nan)
    gbuf, grad = _guarded((T, B, V), nan)
    good = dict(x=_dev(case.x, np.float32), T=T, B=B, V=V, flat=_dev(case.flat, np.int32), offs=_dev(case.offs, np.int32),
                seq=_dev(case.seq, np.int32), maxlen=case.maxlen, lo=_dev(case.lo, np.int32), hi=_dev(case.hi, np.int32),
                pb=1.0, ps=2.0, loss=loss, star=star, grad=grad, ws=torch.zeros(nbytes, dtype=torch.uint8, device="cuda"), nbytes=nbytes)

    def raw(x, T, B, V, flat, offs, seq, maxlen, lo, hi, pb, ps, loss, star, grad, ws, nbytes):
        p = lambda t: None if t is None else t.data_ptr()
        rc = lib.lc_ctc_loss_star(p(x), T, B, V, p(flat), p(offs), p(seq), maxlen, p(lo), p(hi), pb, ps, p(loss), p(star),
                                  p(grad), p(ws), nbytes, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc

    untouched = lambda: (all(bool(torch.isnan(t).all()) for t in (loss, star, grad))
                         and _intact(lbuf) and _intact(sbuf) and _intact(gbuf))
    for kw in (dict(T=0), dict(T=-1), dict(B=0), dict(B=-2), dict(V=1), dict(V=0), dict(maxlen=-1), dict(maxlen=1024),
               dict(x=None), dict(flat=None), dict(offs=None), dict(seq=None), dict(lo=None), dict(hi=None),
               dict(loss=None), dict(star=None), dict(ws=None),
               dict(pb=-1.0), dict(pb=nan), dict(pb=-INF), dict(ps=-1.0), dict(ps=nan), dict(ps=-INF)):
        assert raw(**dict(good, **kw)) == LC_EINVAL, kw
        assert untouched(), kw
    for short in (0, nbytes - 1):
        assert raw(**dict(good, nbytes=short)) == LC_EWORKSPACE
        assert untouched()
    assert lib.lc_last_error().decode().startswith("lc_ctc_loss_star: workspace too small")
    assert raw(**dict(good, lo=None, hi=None, grad=None)) == 0                  # both windows NULL, no gradient
    assert not bool(torch.isnan(loss).any()) and not bool(torch.isnan(star).any()) and bool(torch.isnan(grad).all())
    assert raw(**dict(good, pb=INF, ps=0.0)) == 0                               # +inf and 0 are legal
    assert not bool(torch.isnan(grad).any()) and _intact(lbuf) and _intact(sbuf) and _intact(gbuf)


def test_ops_refuses_cpu_tensors_and_bad_arguments():
    from lstm_ctc_amd import _lib, ops
    rng = np.random.RandomState(9)
    case = Case(rng, 10, feasible_utts(rng, 10, 3, slack=(0, 2), empty=False))
    cpu = [torch.from_numpy(a) for a in (case.x, case.flat, case.offs, case.seq)]
    with pytest.raises(_lib.LibraryError, match="GPU tensors"):
        ops.ctc_loss_star(*cpu, case.maxlen, 1.0, 1.0)
    dev = [t.cuda() for t in cpu]
    with pytest.raises(ValueError, match="both or none"):
        ops.ctc_loss_star(*dev, case.maxlen, 1.0, 1.0, win_lo=_dev(case.lo, np.int32))
    for bad in ((float("nan"), 1.0), (1.0, -0.5), (-INF, 1.0), (True, 1.0)):
        with pytest.raises(ValueError, match="penalty"):
            ops.ctc_loss_star(*dev, case.maxlen, *bad)
    loss, star, grad = ops.ctc_loss_star(*dev, case.maxlen, 1.0, INF, want_grad=False)
    assert grad is None and bool(torch.isfinite(loss).all()) and bool((star >= 0).all())


# ----------------------------------------------------------------------------------------------- 9. the graph
PENALTY = (1.0, 2.0)


def _ops_on_logits(logits_btv, flat, offs, seq, penalty, lo=None, hi=None):
    """(sum of loss, float64 sum of star_frames, frames) of ops.ctc_loss_star on the step's own logits [B,T,V]."""
    from lstm_ctc_amd import ops
    d = lambda a: None if a is None else _dev(a, np.int32)
    loss, star, _ = ops.ctc_loss_star(_dev(np.ascontiguousarray(logits_btv.transpose(1, 0, 2)), np.float32), d(flat), d(offs),
                                      d(seq), int(np.diff(offs).max()), penalty[0], penalty[1], win_lo=d(lo), win_hi=d(hi),
                                      want_grad=False)
    loss, star = loss.cpu().numpy(), star.cpu().numpy()
    assert np.isfinite(loss).all()
    return float(loss.sum(dtype=np.float32)), float(star.astype(np.float64).sum()), int(np.sum(seq))


def _close(a, b):
    return abs(a - b) <= 1e-6 * max(abs(b), 1.0)


def test_graph_steps_with_star_penalty():
    from lstm_ctc_amd.nnet.graph import CTCGraph, flatten_labels
    batch = _smoke_batch()
    V = SMOKE_CFG["num_targets"]
    flat, offs, _ = flatten_labels(batch["nnet_target"])
    seq = batch["sequence_length"]
    graph = CTCGraph(None, SMOKE_CFG, learn_rate=1e-3, l2_decay_weight=0.0, seed=1, star_penalty=PENALTY)
    plain = CTCGraph(None, SMOKE_CFG, learn_rate=1e-3, l2_decay_weight=0.0, seed=1)
    before = graph.model.ps.flat.clone()
    ev = graph.step(batch, fetch_eval=True, fetch_logits=True, train=False)      # a train=False step: loss only
    assert torch.equal(before, graph.model.ps.flat) and "grad_norm" not in ev
    out = graph.step(batch, fetch_eval=True, fetch_logits=True)
    for res in (ev, out):
        total, stars, frames = _ops_on_logits(res["logits"], flat, offs, seq, PENALTY)
        assert _close(res["eval_loss"], total), (res["eval_loss"], total)
        assert _close(res["star_frames"], stars) and res["star_frame_count"] == frames and 0 < stars < frames
    for b in range(len(seq)):                                                    # and those are the reference's values
        ref = star_ctc_ref(out["logits"][b, :seq[b]].astype(np.float64), flat[offs[b]:offs[b + 1]], *PENALTY, V - 1)
        total -= ref["loss"]
        stars -= ref["star_frames"]
    assert abs(total) <= BAR * max(abs(out["eval_loss"]), 1.0) and abs(stars) <= BAR * max(out["star_frames"], 1.0)
    assert out["eval_loss"] < plain.step(batch, fetch_eval=True)["eval_loss"]    # never above plain CTC, same parameters
    assert not torch.equal(before, graph.model.ps.flat) and np.isfinite(out["grad_norm"]) and "decoded" in out
    out2 = graph.step(batch)
    assert graph.star_frame_count_total == 3 * frames
    assert abs(graph.star_frames_total - (ev["star_frames"] + out["star_frames"] + out2["star_frames"])) <= 1e-9 * graph.star_frames_total


def test_graph_without_star_penalty_is_untouched(monkeypatch):
    from lstm_ctc_amd import ops
    from lstm_ctc_amd.nnet.graph import create_graph_for_training_ctc
    calls = {"ctc_loss": 0, "ctc_loss_star": 0}
    for name in calls:
        def counted(*a, _name=name, _fn=getattr(ops, name), **kw):
            calls[_name] += 1
            return _fn(*a, **kw)
        monkeypatch.setattr(ops, name, counted)
    batch = _smoke_batch()
    outs = []
    for kw in (dict(), dict(star_penalty=None)):
        graph = create_graph_for_training_ctc(None, SMOKE_CFG, learn_rate=1e-2, seed=1, **kw)
        assert graph.star_penalty is None
        steps = [graph.step(batch, fetch_eval=True) for _ in range(2)]
        assert all("star_frames" not in s and "star_frame_count" not in s for s in steps)
        outs.append(([s["eval_loss"] for s in steps], [s["grad_norm"] for s in steps], graph.model.ps.flat.clone()))
        assert (graph.star_frames_total, graph.star_frame_count_total) == (0.0, 0)
    assert outs[0][0] == outs[1][0] and outs[0][1] == outs[1][1] and torch.equal(outs[0][2], outs[1][2])
    assert calls["ctc_loss"] >= 4 and calls["ctc_loss_star"] == 0
    off = create_graph_for_training_ctc(None, SMOKE_CFG, learn_rate=1e-2, seed=1, star_penalty=(INF, INF)).step(batch, fetch_eval=True)
    assert calls["ctc_loss_star"] == 1 and off["star_frames"] == 0.0             # both stars off: plain CTC's value
    assert abs(off["eval_loss"] - outs[0][0][0]) <= BAR * max(abs(outs[0][0][0]), 1.0)


def test_graph_star_penalty_composes_with_align_window():
    from lstm_ctc_amd import ops
    from lstm_ctc_amd.nnet.graph import create_graph_for_validation_ctc, flatten_labels
    batch = _smoke_batch()
    V, tau = SMOKE_CFG["num_targets"], 1
    graph = create_graph_for_validation_ctc(None, SMOKE_CFG, seed=1, align_window=tau, star_penalty=PENALTY)
    ali = graph.align(batch)
    with_report = graph.align(batch, star_penalty=PENALTY)
    for k in ("ali", "label_index", "score"):                                    # the alignment does not know about the report
        assert np.array_equal(ali[k].view(np.int32), with_report[k].view(np.int32)), k
    assert set(with_report) - set(ali) == {"ctc_loss", "star_loss", "star_frames"}
    out = graph.step(None, staged=graph.stage(dict(batch, frame_target=ali["ali"])), fetch_logits=True)      # the prefetch path
    flat, offs, _ = flatten_labels(batch["nnet_target"])
    seq = batch["sequence_length"]
    lo, hi, ok = ops.label_windows(ali["ali"], flat, offs, seq, tau, V - 1)
    assert ok.all() and (graph.windows_constrained, graph.windows_unconstrained) == (4, 0)
    total, stars, frames = _ops_on_logits(out["logits"], flat, offs, seq, PENALTY, lo, hi)
    open_total, open_stars, _ = _ops_on_logits(out["logits"], flat, offs, seq, PENALTY)
    assert total > open_total + 1e-3                                             # the windows reach the criterion
    assert _close(out["eval_loss"], total) and _close(out["star_frames"], stars) and out["star_frame_count"] == frames
    # align's report: ops.ctc_loss and ops.ctc_loss_star on the same logits, without windows
    plain, _ = ops.ctc_loss(_dev(np.ascontiguousarray(out["logits"].transpose(1, 0, 2)), np.float32), _dev(flat, np.int32),
                            _dev(offs, np.int32), _dev(seq, np.int32), int(np.diff(offs).max()), want_grad=False)
    assert np.array_equal(with_report["ctc_loss"], plain.cpu().numpy())
    assert _close(float(with_report["star_loss"].sum(dtype=np.float32)), open_total)
    assert _close(float(with_report["star_frames"].astype(np.float64).sum()), open_stars)
    assert (with_report["star_loss"] < with_report["ctc_loss"]).all() and with_report["star_loss"].shape == (4,)


def test_graph_star_penalty_composes_with_consistency_weight_and_dropout(monkeypatch):
    from lstm_ctc_amd import ops
    from lstm_ctc_amd.nnet.graph import create_graph_for_training_ctc
    cfg = dict(SMOKE_CFG, dropout_rate=0.8)
    seen = {}

    def spy(logits, labels, offsets, seq_len, *a, _fn=ops.ctc_loss_star, **kw):
        seen.update(flat=labels.cpu().numpy(), offs=offsets.cpu().numpy(), seq=seq_len.cpu().numpy())
        return _fn(logits, labels, offsets, seq_len, *a, **kw)
    monkeypatch.setattr(ops, "ctc_loss_star", spy)
    graph = create_graph_for_training_ctc(None, cfg, learn_rate=1e-2, optimizer="sgd", seed=11, consistency_weight=0.2,
                                          star_penalty=PENALTY)
    batch = _smoke_batch()
    out = graph.step(batch, fetch_eval=True, fetch_logits=True)
    monkeypatch.undo()
    B = len(batch["sequence_length"])
    assert out["logits"].shape[0] == 2 * B and (out["logits"][:B] != out["logits"][B:]).any()      # two views, both scored
    total, stars, frames = _ops_on_logits(out["logits"], seen["flat"], seen["offs"], seen["seq"], PENALTY)
    assert frames == 2 * int(batch["sequence_length"].sum())
    assert _close(out["eval_loss"], total) and _close(out["star_frames"], stars) and out["star_frame_count"] == frames
    assert out["cr_loss"] > 0 and _close(out["loss"], out["eval_loss"] + 0.2 * 0.5 * out["cr_loss"]) and np.isfinite(out["grad_norm"])


# ----------------------------------------------------------------------------------------------- 10. command lines
def _run(cli, *args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", cli)] + list(args), capture_output=True, timeout=300)
    return r.returncode, r.stderr.decode()


def _logged(err, name):
    lines = [l for l in err.split("\n") if l.startswith("INFO:tensorflow:%s = " % name)]
    assert len(lines) == 1, err
    return float(lines[0].split()[-1])


def _star_line(err):
    """(bypass, selfloop, share, frames) of the one 'star penalty' INFO line."""
    lines = [l for l in err.split("\n") if l.startswith("INFO:tensorflow:star penalty ")]
    assert len(lines) == 1, err
    m = re.fullmatch(r"INFO:tensorflow:star penalty bypass (\S+) selfloop (\S+): (\S+) of (\d+) frame\(s\) explained by the star", lines[0])
    assert m, lines[0]
    return float(m.group(1)), float(m.group(2)), float(m.group(3)), int(m.group(4))


def test_cli_train_validate_and_align_with_star_penalty(tmp_path):
    import lstm_ctc_amd.nnet as nnet
    rng = np.random.default_rng(7)
    D, V = 6, 9
    lines, frames, eligible = [], 0, []
    for i, T in enumerate([20, 24, 31, 40, 4]):
        path = str(tmp_path / ("utt%03d.tfrecords" % i))
        target = rng.integers(0, V - 1, size=int(rng.integers(1, 5)) if T > 4 else 3)      # the last one: 3 labels, 2 frames
        if T > 4:
            frames += T // 2                                                      # subsample = 2
            eligible.append(("utt%03d" % i, T // 2, len(target)))
        nnet.write_tfrecord(path, rng.normal(size=(T, D)).astype(np.float32), target)
        lines.append("utt%03d %d %d 1 %s" % (i, T, D, path))
    scp = tmp_path / "tfrecords.scp"
    scp.write_text("\n".join(lines[:4]) + "\n")
    scp_all = tmp_path / "all.scp"
    scp_all.write_text("\n".join(lines) + "\n")
    config = tmp_path / "nnet.config"
    config.write_text("nnet_type = lstm\ninput_dim = 6\nleft_context = 1\nright_context = 1\nsubsample = 2\nnum_layers = 2\n"
                      "num_neurons = 32\nnum_projects = 16\nnum_targets = 9\nuse_peepholes = true\ndropout_rate = 1.0\n")
    d = str(tmp_path)
    rc, err = _run("nnet-init.py", "--objective=ctc", "--batch-size", "2", str(scp), str(config), d + "/nnet.0")
    assert rc == 0, err
    rc, err = _run("nnet-train.py", "--objective=ctc", "--batch-size", "2", "--learn-rate=0.01", "--optimizer=adam", "--seed=1",
                   "--shuffle=false", "--star-penalty", "2,3", str(scp), str(config), d + "/nnet.0", d + "/nnet.1")
    assert rc == 0, err
    pb, ps, share, n = _star_line(err)
    assert (pb, ps) == (2.0, 3.0) and abs(n - frames) <= 4 and 0.0 < share < 1.0, err
    assert np.isfinite(_logged(err, "tr_loss")) and os.path.getsize(d + "/nnet.1") > 0
    val = ["--objective=ctc", "--batch-size", "2", str(scp), str(config), d + "/nnet.1"]
    rc, err = _run("nnet-validate.py", "--star-penalty", "2", *val)
    assert rc == 0, err
    pb, ps, share, n2 = _star_line(err)
    assert (pb, ps) == (2.0, 2.0) and n2 == n and 0.0 < share < 1.0 and np.isfinite(_logged(err, "cv_loss"))
    # nnet-align: the report beside a table that does not change
    ali = ["--batch-utts", "2", str(scp_all), str(config), d + "/nnet.1"]
    rc, err = _run("nnet-align.py", "--scores", d + "/scores.a", *ali, "ark:" + d + "/ali.a")
    assert rc == 0, err
    rc, err = _run("nnet-align.py", "--scores", d + "/scores.b", "--star-penalty", "2", "--star-report", d + "/report.txt", *ali,
                   "ark:" + d + "/ali.b")
    assert rc == 0, err
    for a, b in (("ali.a", "ali.b"), ("scores.a", "scores.b")):
        with open(os.path.join(d, a), "rb") as fa, open(os.path.join(d, b), "rb") as fb:
            assert fa.read() == fb.read() and fa.tell() > 0, a
    with open(d + "/report.txt") as f:
        report = f.read().splitlines()
    assert len(report) == len(eligible)                                          # not the utterance whose labels exceed its frames
    for line, (key, T, L) in zip(report, eligible):
        m = re.fullmatch(r"(\S+) (\d+) (\d+) (-?\d+\.\d{6}) (-?\d+\.\d{6}) (\d+\.\d{6})", line)
        assert m, line
        assert (m.group(1), int(m.group(3))) == (key, L) and abs(int(m.group(2)) - T) <= 1, line
        ctc, star_loss, stars = float(m.group(4)), float(m.group(5)), float(m.group(6))
        assert star_loss <= ctc + 1e-6 and 0.0 < stars < T, line


def test_zz_report_measured_error_over_bar():
    text = ("ctc_star: largest measured error / project bar (GRAD_TOL = %g) over %d utterances with a path: loss %.4f, "
            "star_frames %.4f, grad %.4f" % (BAR, MEASURED["n"], MEASURED["loss"], MEASURED["star"], MEASURED["grad"]))
    print("\n" + text)
    out = os.environ.get("LC_MEASURED_DIR")              # where to keep the line; unset: printed only
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "ctc_star_measured.txt"), "w") as f:
            f.write(text + "\n")
    assert MEASURED["loss"] <= 1.0 and MEASURED["star"] <= 1.0 and MEASURED["grad"] <= 1.0
