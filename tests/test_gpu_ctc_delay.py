"""lc_ctc_loss_delay (delay-penalised CTC and the expected label entry frame) on the GPU, through every layer: kernel, ops,
CTCGraph, command lines.

Reference: ``delay_ctc_ref`` of tests/test_ctc_delay_host.py - a float64 numpy alpha-beta recursion with the weight -lambda t
on the arcs that enter a label position at frame t, anchored there against brute-force enumeration of all paths.

Tolerances are the project's bars (tests/conftest.py GRAD_TOL = 1e-4), not new numbers: a loss and an entry_sum within
GRAD_TOL max(|ref|, 1) of float64, a gradient through ``check_grad``.  Every kernel call here runs on guarded output buffers
(a band of sentinels on either side, checked after the call), NaN-filled outputs and a workspace of 0xFF bytes.  The last test
prints the largest measured / bar ratios and, with LC_MEASURED_DIR set, writes them to ctc_delay_measured.txt in that directory
(kept as profiles/ctc_delay_measured.txt)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GRAD_TOL, check_grad
from test_ctc_delay_host import delay_ctc_ref
from test_ctc_window_host import OPEN, random_path
from test_gpu_ctc_window import SMOKE_CFG, Case, _dev, _smoke_batch, feasible_utts, make_labels, need_frames, windows_around

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = GRAD_TOL
LC_EINVAL, LC_EWORKSPACE = -1, -3
GUARD, SENTINEL = 64, 1234.5
MEASURED = {"loss": 0.0, "entry": 0.0, "grad": 0.0, "n": 0}


# ----------------------------------------------------------------------------------------------- calling the kernel
def _guarded(shape, fill):
    """(whole buffer, the view the kernel writes): GUARD sentinels on either side of ``fill``-filled elements."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENTINEL, device="cuda")
    buf[GUARD:GUARD + n] = fill
    return buf, buf[GUARD:GUARD + n].view(shape)


def _intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def call(case, lam, want_grad=True, want_entry=True, windowed=None):
    """One lc_ctc_loss_delay call -> (loss, entry_sum or None, grad or None) on the host."""
    from lstm_ctc_amd import _lib
    lib = _lib.load()
    T, B, V = case.T, case.B, case.V
    windowed = case.windowed if windowed is None else windowed
    x, flat, offs, seq = (_dev(case.x, np.float32), _dev(case.flat if len(case.flat) else np.zeros(1), np.int32),
                          _dev(case.offs, np.int32), _dev(case.seq, np.int32))
    lo = _dev(case.lo if len(case.lo) else np.zeros(1), np.int32) if windowed else None
    hi = _dev(case.hi if len(case.hi) else np.zeros(1), np.int32) if windowed else None
    nbytes = lib.lc_ctc_delay_workspace_bytes(T, B, V, case.maxlen)
    assert nbytes > 0
    wsbuf = torch.full((nbytes + 512,), 0xA5, dtype=torch.uint8, device="cuda")
    ws = wsbuf[256:256 + nbytes]
    ws.fill_(0xFF)
    nan = float("nan")
    lbuf, loss = _guarded((B,), nan)
    ebuf, entry = _guarded((B,), nan) if want_entry else (None, None)
    gbuf, grad = _guarded((T, B, V), nan) if want_grad else (None, None)
    p = lambda t: None if t is None else t.data_ptr()
    rc = lib.lc_ctc_loss_delay(p(x), T, B, V, p(flat), p(offs), p(seq), case.maxlen, p(lo), p(hi), float(lam), p(loss),
                               p(entry), p(grad), p(ws), nbytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, lib.lc_last_error()
    assert _intact(lbuf) and (ebuf is None or _intact(ebuf)) and (gbuf is None or _intact(gbuf)), "a guard band was written"
    assert bool((wsbuf[:256] == 0xA5).all()) and bool((wsbuf[256 + nbytes:] == 0xA5).all()), "the workspace's guards were written"
    host = lambda t: None if t is None else t.cpu().numpy().copy()
    return host(loss), host(entry), host(grad)


def reference(case, b, lam, windowed=None):
    Tb, labels, lo, hi = case.utts[b]
    windowed = case.windowed if windowed is None else windowed
    return delay_ctc_ref(case.x[:Tb, b].astype(np.float64), labels, lam, case.V - 1, *((lo, hi) if windowed else (None, None)))


def check_against_reference(case, lam, loss, entry, grad, tag, utterances=None, windowed=None):
    """Loss, entry_sum and gradient of every utterance, with the conventions of lc_ctc_loss."""
    for b in (range(case.B) if utterances is None else utterances):
        Tb, labels = case.utts[b][0], np.asarray(case.utts[b][1])
        gb = grad[:, b]
        assert np.array_equal(gb[Tb:].view(np.int32), np.zeros_like(gb[Tb:], np.int32)), (tag, b, "rows beyond seq_len")
        if Tb <= 0 or len(labels) > Tb:
            assert loss[b] == 0.0 and entry[b] == 0.0 and not gb.any(), (tag, b, "skipped utterance")
            continue
        ref = reference(case, b, lam, windowed)
        if not np.isfinite(ref["loss"]):
            assert loss[b] == np.inf and entry[b] == 0.0, (tag, b, loss[b], entry[b])
            assert not np.isnan(gb).any()
            check_grad(gb[:Tb], ref["grad"], tag, "utt%d/softmax" % b)
            continue
        err = abs(float(loss[b]) - ref["loss"])
        eerr = abs(float(entry[b]) - ref["entry_sum"])
        gerr = float(np.abs(gb[:Tb] - ref["grad"]).max())
        lbar, ebar = BAR * max(abs(ref["loss"]), 1.0), BAR * max(abs(ref["entry_sum"]), 1.0)
        gbar = BAR * max(float(np.abs(ref["grad"]).max()), 1e-3)
        print("%s utt %d: T_b %d L %d  loss %.6f ref %.6f err %.2e (bar %.2e)  entry_sum %.4f ref %.4f err %.2e (bar %.2e)  "
              "grad err %.2e (bar %.2e)" % (tag, b, Tb, len(labels), loss[b], ref["loss"], err, lbar, entry[b],
                                            ref["entry_sum"], eerr, ebar, gerr, gbar))
        MEASURED["loss"] = max(MEASURED["loss"], err / lbar)
        MEASURED["entry"] = max(MEASURED["entry"], eerr / ebar)
        MEASURED["grad"] = max(MEASURED["grad"], gerr / gbar)
        MEASURED["n"] += 1
        assert err <= lbar, (tag, b, loss[b], ref["loss"])
        assert eerr <= ebar, (tag, b, entry[b], ref["entry_sum"])
        check_grad(gb[:Tb], ref["grad"], tag, "utt%d" % b)
        assert np.abs(gb[:Tb].sum(axis=1)).max() <= case.V * BAR, (tag, b, "live rows sum to 0")


def make_case(rng, V, utts, windowed, T=None):
    case = Case(rng, V, utts, T=T)
    case.windowed = windowed
    return case


# ----------------------------------------------------------------------------------------------- geometry
# Positions per lane switch at S = 2L + 1 = 64, 128, 256, 512, 1024 (L = 31|32, 63|64, 127|128, 255|256, 511|512); frames
# fetched per chunk 8, 8, 8, 4, 2, 1.  Gradient and entry terms: four frames per workgroup, classes in strides of 64 lanes,
# blank positions in strides of 128, lattice positions in strides of 64; the class lists are built by 256 threads.
GEOMETRY = [(0, 2), (1, 44), (31, 44), (32, 44), (63, 129), (64, 44), (127, 44), (128, 1100), (255, 44), (256, 129), (511, 2),
            (512, 44), (1023, 44)]


@pytest.mark.parametrize("lam", [0.05, 1.0])
@pytest.mark.parametrize("L,V", GEOMETRY)
def test_geometry_edges(L, V, lam):
    """Ragged batches, T_b = frames needed + {0, 1, 3, 7}, plus an empty, a skipped and an infeasible utterance; half of
    the cases carry windows around a random path."""
    idx = GEOMETRY.index((L, V))
    windowed = (idx + (lam == 1.0)) % 2 == 1
    rng = np.random.RandomState(1000 * V + L + (7 if lam == 1.0 else 0))
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
    loss, entry, grad = call(case, lam)
    assert loss[-1] == np.inf and loss[-2] == 0.0 and loss[-3] == 0.0
    check_against_reference(case, lam, loss, entry, grad, "geom L%d V%d lam%g%s" % (L, V, lam, " win" if windowed else ""))


def test_one_frame_and_one_utterance():
    rng = np.random.RandomState(1)
    for V in (2, 44):
        for labels in ([], [0]):
            for windowed in (False, True):
                case = make_case(rng, V, [(1, np.array(labels, np.int64), np.zeros(len(labels)), np.zeros(len(labels)))], windowed)
                loss, entry, grad = call(case, 0.7)                               # T = 1, B = 1
                assert entry[0] == 0.0                                            # frame 0 carries no penalty
                check_against_reference(case, 0.7, loss, entry, grad, "T1B1 V%d L%d" % (V, len(labels)))


def _b65(rng, V=44):
    utts = []
    for b in range(65):
        L = int(rng.randint(0, 9))
        labels = make_labels(rng, V, L)
        Tb = 0 if b % 13 == 5 else max(need_frames(labels), 1) + int(rng.randint(0, 12))
        states = random_path(rng, labels, Tb) if Tb else None
        lo, hi = windows_around(rng, states, L) if Tb else (np.zeros(L), np.full(L, OPEN))
        utts.append((Tb, labels, lo, hi))
    return utts


@pytest.mark.parametrize("windowed", [False, True])
def test_b65_ragged_and_unsorted(windowed):
    """B = 65: more utterances than one wave's lanes, T * B not a multiple of the four frames of a workgroup."""
    rng = np.random.RandomState(2)
    case = make_case(rng, 44, _b65(rng), windowed, T=23)
    loss, entry, grad = call(case, 0.3)
    check_against_reference(case, 0.3, loss, entry, grad, "B65")


# ----------------------------------------------------------------------------------------------- lambda = 0 and the siblings
def test_lambda_zero_reproduces_ctc_loss_and_windowed_ctc():
    from lstm_ctc_amd import ops
    rng = np.random.RandomState(3)
    V = 44
    utts = []
    for L, extra in ((5, 0), (12, 9), (0, 4), (40, 30), (3, 60), (70, 11)):
        labels = make_labels(rng, V, L)
        Tb = need_frames(labels) + extra + (L == 0)
        lo, hi = windows_around(rng, random_path(rng, labels, Tb), L)
        utts.append((Tb, labels, lo, hi))
    case = make_case(rng, V, utts, False)
    dev = (_dev(case.x, np.float32), _dev(case.flat, np.int32), _dev(case.offs, np.int32), _dev(case.seq, np.int32))
    loss_c, grad_c = ops.ctc_loss(*dev, case.maxlen)
    loss_w, grad_w = ops.ctc_loss_windowed(*dev, case.maxlen, _dev(case.lo, np.int32), _dev(case.hi, np.int32))
    for windowed, want_loss, want_grad, name in ((False, loss_c, grad_c, "lc_ctc_loss"), (True, loss_w, grad_w, "windowed")):
        want_loss, want_grad = want_loss.cpu().numpy(), want_grad.cpu().numpy()
        loss, entry, grad = call(case, 0.0, windowed=windowed)
        assert np.isfinite(want_loss).all()
        assert (np.abs(loss - want_loss) <= BAR * np.maximum(np.abs(want_loss), 1.0)).all(), (name, loss, want_loss)
        for b in range(case.B):
            check_grad(grad[:utts[b][0], b], want_grad[:utts[b][0], b], "lambda 0 = " + name, "utt%d" % b)
        check_against_reference(case, 0.0, loss, entry, grad, "lambda 0 " + name, windowed=windowed)      # entry_sum too


@pytest.mark.parametrize("L,V", [(5, 8), (40, 8), (40, 129), (100, 8), (200, 8), (400, 8), (1023, 8)])
def test_lambda_zero_with_windows_is_windowed_ctc_bit_for_bit(L, V):
    """Both entries run one sweep template, so at lambda 0 (every arc weight is +0.0 or -0.0, and no cell is -0.0) they cannot
    differ in a bit: one label length per positions-per-lane class, a batch of a feasible utterance, one whose window
    excludes every frame (+inf, softmax rows) and one with a bad label (NaN, zero rows)."""
    from lstm_ctc_amd import _lib
    lib = _lib.load()
    rng = np.random.RandomState(4000 + 10 * L + V)
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
    loss, entry, grad = call(case, 0.0, want_entry=False)
    assert entry is None and np.isfinite(loss[0]) and loss[1] == np.inf and np.isnan(loss[2])
    T, B = case.T, case.B
    nbytes = lib.lc_ctc_window_workspace_bytes(T, B, V, case.maxlen)
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
    loss_w, grad_w = torch.full((B,), float("nan"), device="cuda"), torch.full((T, B, V), float("nan"), device="cuda")
    x, flat, offs, seq, lo, hi = (_dev(case.x, np.float32), _dev(case.flat, np.int32), _dev(case.offs, np.int32),
                                  _dev(case.seq, np.int32), _dev(case.lo, np.int32), _dev(case.hi, np.int32))
    p = lambda t: t.data_ptr()
    rc = lib.lc_ctc_loss_windowed(p(x), T, B, V, p(flat), p(offs), p(seq), case.maxlen, p(lo), p(hi), p(loss_w), p(grad_w),
                                  p(ws), nbytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, lib.lc_last_error()
    assert np.array_equal(loss.view(np.int32), loss_w.cpu().numpy().view(np.int32)), (loss, loss_w)
    assert np.array_equal(grad.view(np.int32), grad_w.cpu().numpy().view(np.int32))
    assert grad[:utts[1][0], 1].any() and not grad[:, 2].any()


# ----------------------------------------------------------------------------------------------- identities
def _long_case(T, V, L, B, windowed):
    rng = np.random.RandomState(T + V)
    utts = []
    for b in range(B):
        labels = make_labels(rng, V, L - b)
        lo, hi = windows_around(rng, random_path(rng, labels, T - 7 * b), L - b, width=20)
        utts.append((T - 7 * b, labels, lo, hi))
    return make_case(rng, V, utts, windowed, T=T)


@pytest.mark.parametrize("T,V,L,B,windowed", [(60, 8, 12, 3, False), (60, 8, 12, 3, True), (1000, 44, 100, 4, False)])
def test_sandwich_and_monotone_entry_sum(T, V, L, B, windowed):
    """loss(0) <= loss(lambda) <= loss(0) + lambda entry_sum(0) (the loss is concave in lambda, its slope is entry_sum), and
    entry_sum does not grow over lambda = 0, 0.05, 0.2, 1."""
    case = _long_case(T, V, L, B, windowed)
    lams = (0.0, 0.05, 0.2, 1.0)
    res = [call(case, lam, want_grad=False) for lam in lams]
    loss0, entry0 = res[0][0].astype(np.float64), res[0][1].astype(np.float64)
    assert np.isfinite(loss0).all() and (entry0 > 0).all()
    print("\nT=%d: entry_sum / L over lambda %s: %s" % (T, lams, [np.round(r[1] / np.diff(case.offs), 2) for r in res]))
    for lam, (loss, entry, _) in zip(lams[1:], res[1:]):
        loss = loss.astype(np.float64)
        upper = loss0 + lam * entry0
        assert (loss0 <= loss + BAR * np.maximum(np.abs(loss), 1.0)).all(), (lam, loss0, loss)
        assert (loss <= upper + BAR * np.maximum(np.abs(upper), 1.0)).all(), (lam, loss, upper)
    for (_, a, _), (_, b, _) in zip(res, res[1:]):
        assert (b <= a + BAR * np.maximum(np.abs(a), 1.0)).all(), (a, b)
    assert (res[-1][1] < res[0][1]).all()                               # and the penalty does pull the labels forward


def test_negative_lambda():
    rng = np.random.RandomState(8)
    case = make_case(rng, 44, feasible_utts(rng, 44, 40, slack=(0, 5, 30), empty=False), True)
    loss, entry, grad = call(case, -0.4)
    check_against_reference(case, -0.4, loss, entry, grad, "lambda -0.4")
    plain = call(case, 0.0)
    assert (loss < plain[0]).all()                                        # late entries are rewarded ...
    assert (entry >= plain[1] - BAR * np.maximum(np.abs(plain[1]), 1.0)).all()      # ... and become likelier (T_b = need: one path)


# ----------------------------------------------------------------------------------------------- outputs and determinism
def test_optional_outputs_and_bit_identical_calls():
    rng = np.random.RandomState(6)
    V = 44
    utts = feasible_utts(rng, V, 70) + feasible_utts(rng, V, 9, slack=(0, 30))
    utts.append((50, make_labels(rng, V, 4), np.array([0, 9, 0, 0]), np.array([OPEN, 3, OPEN, OPEN])))      # no path
    utts.append((3, make_labels(rng, V, 9), np.zeros(9), np.full(9, OPEN)))                                    # skipped
    case = make_case(rng, V, utts, True)
    bits = lambda a: a.view(np.int32)
    full = call(case, 0.2)
    again = call(case, 0.2)
    for a, b in zip(full, again):
        assert np.array_equal(bits(a), bits(b))                          # two calls are bit-identical, NaN payloads included
    loss_only = call(case, 0.2, want_grad=False, want_entry=False)
    no_entry = call(case, 0.2, want_entry=False)
    no_grad = call(case, 0.2, want_grad=False)
    for other in (loss_only, no_entry, no_grad):
        assert np.array_equal(bits(other[0]), bits(full[0]))             # the loss never depends on what else is asked for
    assert np.array_equal(bits(no_entry[2]), bits(full[2]))              # nor does the gradient
    # without a gradient the frame terms are summed position by position, with one class by class: the same sum in another
    # order, each in double
    assert (np.abs(no_grad[1] - full[1]) <= BAR * np.maximum(np.abs(full[1]), 1.0)).all(), (no_grad[1], full[1])
    check_against_reference(case, 0.2, full[0], full[1], full[2], "coverage")
    check_against_reference(case, 0.2, no_grad[0], no_grad[1], full[2], "coverage, entry without grad")


def test_conventions_of_ctc_loss():
    rng = np.random.RandomState(5)
    V, T = 7, 12
    open3 = (np.zeros(3), np.full(3, OPEN))
    utts = [
        (T, np.array([1, 2, 3]), np.array([0, 3, 6]), np.array([4, 8, 11])),         # 0 fine
        (2, np.array([1, 2, 3])) + open3,                                            # 1 L > T_b: loss 0, gradient 0
        (T, np.array([1, 6, 3])) + open3,                                            # 2 the blank as a label: NaN, gradient 0
        (T, np.array([1, -1, 3])) + open3,                                           # 3 a negative label: NaN, gradient 0
        (T, np.array([1, 2, 3]), np.array([0, 5, 0]), np.array([11, 4, 11])),        # 4 an empty window: +inf, softmax
        (T, np.array([1, 2, 3]), np.array([6, 0, 0]), np.array([11, 3, 11])),        # 5 windows force the wrong order
        (2, np.array([2, 2]), np.zeros(2), np.full(2, OPEN)),                        # 6 L fits, the blank between does not
        (T - 1, np.array([4, 4, 0]), np.array([0, 2, 0]), np.array([3, 9, OPEN])),   # 7 fine
        (0, np.array([1])) + (np.zeros(1), np.full(1, OPEN)),                        # 8 no frames
        (5, np.zeros(0, np.int64), np.zeros(0), np.zeros(0)),                        # 9 L = 0: the all-blank path
    ]
    for windowed in (True, False):
        case = make_case(rng, V, utts, windowed, T=T)
        for want_grad in (True, False):
            loss, entry, grad = call(case, 0.5, want_grad=want_grad)
            assert np.isnan(loss[[2, 3]]).all() and np.isnan(entry[[2, 3]]).all()
            assert loss[1] == 0.0 and loss[8] == 0.0 and entry[1] == 0.0 and entry[8] == 0.0
            infeasible = [4, 5, 6] if windowed else [6]
            assert (loss[infeasible] == np.inf).all() and (entry[infeasible] == 0.0).all()
            rest = [b for b in range(10) if b not in (2, 3)]
            assert not np.isnan(loss[rest]).any() and not np.isnan(entry[rest]).any()
            assert entry[9] == 0.0 and np.isfinite(loss[[0, 7, 9]]).all()
            if want_grad:
                assert not grad[:, [1, 2, 3, 8]].any() and not np.isnan(grad).any()
                check_against_reference(case, 0.5, loss, entry, grad, "conventions", utterances=rest)


def test_argument_checks_launch_nothing():
    from lstm_ctc_amd import _lib
    lib = _lib.load()
    rng = np.random.RandomState(7)
    V = 10
    case = Case(rng, V, feasible_utts(rng, V, 3, slack=(0, 2), empty=False))
    T, B = case.T, case.B
    nbytes = lib.lc_ctc_delay_workspace_bytes(T, B, V, case.maxlen)
    nan = float("nan")
    loss, entry, grad = torch.full((B,), nan, device="cuda"), torch.full((B,), nan, device="cuda"), torch.full((T, B, V), nan, device="cuda")
    good = dict(x=_dev(case.x, np.float32), T=T, B=B, V=V, flat=_dev(case.flat, np.int32), offs=_dev(case.offs, np.int32),
                seq=_dev(case.seq, np.int32), maxlen=case.maxlen, lo=_dev(case.lo, np.int32), hi=_dev(case.hi, np.int32),
                lam=0.1, loss=loss, entry=entry, grad=grad, ws=torch.zeros(nbytes, dtype=torch.uint8, device="cuda"), nbytes=nbytes)

    def raw(x, T, B, V, flat, offs, seq, maxlen, lo, hi, lam, loss, entry, grad, ws, nbytes):
        p = lambda t: None if t is None else t.data_ptr()
        rc = lib.lc_ctc_loss_delay(p(x), T, B, V, p(flat), p(offs), p(seq), maxlen, p(lo), p(hi), lam, p(loss), p(entry),
                                   p(grad), p(ws), nbytes, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc

    untouched = lambda: all(bool(torch.isnan(t).all()) for t in (loss, entry, grad))
    for kw in (dict(T=0), dict(T=-1), dict(B=0), dict(B=-2), dict(V=1), dict(V=0), dict(maxlen=-1), dict(maxlen=1024),
               dict(x=None), dict(flat=None), dict(offs=None), dict(seq=None), dict(lo=None), dict(hi=None),
               dict(loss=None), dict(ws=None), dict(lam=float("nan")), dict(lam=float("inf")), dict(lam=-float("inf"))):
        assert raw(**dict(good, **kw)) == LC_EINVAL, kw
        assert untouched(), kw
    for short in (0, nbytes - 1):
        assert raw(**dict(good, nbytes=short)) == LC_EWORKSPACE
        assert untouched()
    assert lib.lc_last_error().decode().startswith("lc_ctc_loss_delay: workspace too small")
    assert raw(**dict(good, lo=None, hi=None, entry=None, grad=None)) == 0      # both windows NULL, optional outputs NULL
    assert not bool(torch.isnan(loss).any()) and bool(torch.isnan(entry).all()) and bool(torch.isnan(grad).all())
    assert raw(**good) == 0
    assert not bool(torch.isnan(entry).any()) and not bool(torch.isnan(grad).any())


def test_ops_refuses_cpu_tensors_and_bad_arguments():
    from lstm_ctc_amd import _lib, ops
    rng = np.random.RandomState(9)
    case = Case(rng, 10, feasible_utts(rng, 10, 3, slack=(0, 2), empty=False))
    cpu = [torch.from_numpy(a) for a in (case.x, case.flat, case.offs, case.seq)]
    with pytest.raises(_lib.LibraryError, match="GPU tensors"):
        ops.ctc_loss_delay(*cpu, case.maxlen, 0.1)
    dev = [t.cuda() for t in cpu]
    with pytest.raises(ValueError, match="both or none"):
        ops.ctc_loss_delay(*dev, case.maxlen, 0.1, win_lo=_dev(case.lo, np.int32))
    with pytest.raises(ValueError, match="finite"):
        ops.ctc_loss_delay(*dev, case.maxlen, float("nan"))
    loss, entry, grad = ops.ctc_loss_delay(*dev, case.maxlen, 0.1, want_grad=False, want_entry=False)
    assert entry is None and grad is None and bool(torch.isfinite(loss).all())


# ----------------------------------------------------------------------------------------------- the graph
LAMBDA = 0.3


def _reference_on_logits(logits, batch, lam, V, lo=None, hi=None):
    from lstm_ctc_amd.nnet.graph import flatten_labels
    flat, offs, _ = flatten_labels(batch["nnet_target"])
    seq = batch["sequence_length"]
    total = entry = 0.0
    for b in range(len(seq)):
        win = (None, None) if lo is None else (lo[offs[b]:offs[b + 1]], hi[offs[b]:offs[b + 1]])
        ref = delay_ctc_ref(logits[b, :seq[b]].astype(np.float64), flat[offs[b]:offs[b + 1]], lam, V - 1, *win)
        total += ref["loss"]
        entry += ref["entry_sum"]
    return total, entry, len(flat)


def test_graph_training_step_with_delay_penalty():
    from lstm_ctc_amd.nnet.graph import CTCGraph
    batch = _smoke_batch()
    V = SMOKE_CFG["num_targets"]
    graph = CTCGraph(None, SMOKE_CFG, learn_rate=1e-3, l2_decay_weight=0.0, seed=1, delay_penalty=LAMBDA)
    before = graph.model.ps.flat.clone()
    out = graph.step(batch, fetch_eval=True, fetch_logits=True)
    total, entry, n = _reference_on_logits(out["logits"], batch, LAMBDA, V)
    assert abs(out["eval_loss"] - total) <= BAR * max(abs(total), 1.0), (out["eval_loss"], total)
    assert abs(out["entry_sum"] - entry) <= BAR * max(abs(entry), 1.0), (out["entry_sum"], entry)
    assert out["entry_labels"] == n == out["size"] and "decoded" in out
    plain, _, _ = _reference_on_logits(out["logits"], batch, 0.0, V)
    assert total > plain + 1e-3                                      # the penalty bites on this batch
    assert not torch.equal(before, graph.model.ps.flat) and np.isfinite(out["grad_norm"])
    out2 = graph.step(batch)
    assert graph.entry_labels_total == 2 * n
    assert abs(graph.entry_sum_total - (out["entry_sum"] + out2["entry_sum"])) <= 1e-9 * graph.entry_sum_total
    for bad in (dict(objective="xent", delay_penalty=0.1), dict(objective="kd", delay_penalty=0.1), dict(delay_penalty=-0.1),
                dict(delay_penalty=True), dict(delay_penalty=float("nan")), dict(delay_penalty=float("inf")),
                dict(delay_penalty="0.1")):
        with pytest.raises(ValueError, match="delay_penalty"):
            CTCGraph(None, SMOKE_CFG, seed=1, **bad)


def test_graph_without_delay_penalty_is_untouched(monkeypatch):
    """delay_penalty=None runs the old ops and never the new one (counted), and trains bit-identically to a graph built
    without the keyword."""
    from lstm_ctc_amd import ops
    from lstm_ctc_amd.nnet.graph import create_graph_for_training_ctc
    calls = {"ctc_loss": 0, "ctc_loss_windowed": 0, "ctc_loss_delay": 0}
    for name in calls:
        def counted(*a, _name=name, _fn=getattr(ops, name), **kw):
            calls[_name] += 1
            return _fn(*a, **kw)
        monkeypatch.setattr(ops, name, counted)
    batch = _smoke_batch()
    outs = []
    for kw in (dict(), dict(delay_penalty=None)):
        graph = create_graph_for_training_ctc(None, SMOKE_CFG, learn_rate=1e-2, seed=1, **kw)
        assert graph.delay_penalty is None
        steps = [graph.step(batch, fetch_eval=True) for _ in range(2)]
        assert all("entry_sum" not in s and "entry_labels" not in s for s in steps)
        outs.append(([s["eval_loss"] for s in steps], [s["grad_norm"] for s in steps], graph.model.ps.flat.clone()))
        assert (graph.entry_sum_total, graph.entry_labels_total) == (0.0, 0)
    assert outs[0][0] == outs[1][0] and outs[0][1] == outs[1][1] and torch.equal(outs[0][2], outs[1][2])
    plain_calls = calls["ctc_loss"]                                  # a step re-run on the launch train calls its op again
    assert plain_calls >= 4 and calls["ctc_loss_windowed"] == 0 and calls["ctc_loss_delay"] == 0
    graph = create_graph_for_training_ctc(None, SMOKE_CFG, learn_rate=1e-2, seed=1, align_window=1)
    graph.step(dict(batch, frame_target=graph.align(batch)["ali"]))
    assert calls["ctc_loss"] == plain_calls and calls["ctc_loss_windowed"] >= 1 and calls["ctc_loss_delay"] == 0
    # lambda = 0 is the new op, and plain CTC's value
    zero = create_graph_for_training_ctc(None, SMOKE_CFG, learn_rate=1e-2, seed=1, delay_penalty=0).step(batch)
    assert calls["ctc_loss_delay"] >= 1 and calls["ctc_loss"] == plain_calls
    assert abs(zero["eval_loss"] - outs[0][0][0]) <= BAR * max(abs(outs[0][0][0]), 1.0)


def test_graph_delay_penalty_composes_with_align_window():
    from lstm_ctc_amd import ops
    from lstm_ctc_amd.nnet.graph import create_graph_for_validation_ctc, flatten_labels
    batch = _smoke_batch()
    V, tau = SMOKE_CFG["num_targets"], 1
    graph = create_graph_for_validation_ctc(None, SMOKE_CFG, seed=1, align_window=tau, delay_penalty=LAMBDA)
    ali = graph.align(batch)["ali"]
    out = graph.step(None, staged=graph.stage(dict(batch, frame_target=ali)), fetch_logits=True)      # the prefetch path
    flat, offs, _ = flatten_labels(batch["nnet_target"])
    lo, hi, ok = ops.label_windows(ali, flat, offs, batch["sequence_length"], tau, V - 1)
    assert ok.all() and (graph.windows_constrained, graph.windows_unconstrained) == (4, 0)
    total, entry, n = _reference_on_logits(out["logits"], batch, LAMBDA, V, lo, hi)
    open_total, open_entry, _ = _reference_on_logits(out["logits"], batch, LAMBDA, V)
    assert total > open_total + 1e-3                                 # the windows bite as well
    assert abs(out["eval_loss"] - total) <= BAR * max(abs(total), 1.0), (out["eval_loss"], total)
    assert abs(out["entry_sum"] - entry) <= BAR * max(abs(entry), 1.0), (out["entry_sum"], entry)
    assert out["entry_labels"] == n


# ----------------------------------------------------------------------------------------------- command lines
def _run(cli, *args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", cli)] + list(args), capture_output=True, timeout=300)
    return r.returncode, r.stderr.decode()


def _logged(err, name):
    lines = [l for l in err.split("\n") if l.startswith("INFO:tensorflow:%s = " % name)]
    assert len(lines) == 1, err
    return float(lines[0].split()[-1])


def _entry_line(err):
    """(penalty, mean entry frame, labels) of the one 'delay penalty' INFO line."""
    import re
    lines = [l for l in err.split("\n") if l.startswith("INFO:tensorflow:delay penalty ")]
    assert len(lines) == 1, err
    m = re.fullmatch(r"INFO:tensorflow:delay penalty (\S+): mean label entry frame (\S+) over (\d+) label\(s\)", lines[0])
    assert m, lines[0]
    return float(m.group(1)), float(m.group(2)), int(m.group(3))


def test_cli_train_and_validate_with_delay_penalty(tmp_path):
    import lstm_ctc_amd.nnet as nnet
    rng = np.random.default_rng(7)
    D, V = 6, 9
    lines, labels = [], 0
    for i, T in enumerate([20, 24, 31, 40]):
        path = str(tmp_path / ("utt%03d.tfrecords" % i))
        target = rng.integers(0, V - 1, size=int(rng.integers(1, 5)))
        labels += len(target)
        nnet.write_tfrecord(path, rng.normal(size=(T, D)).astype(np.float32), target)
        lines.append("utt%03d %d %d 1 %s" % (i, T, D, path))
    scp = tmp_path / "tfrecords.scp"
    scp.write_text("\n".join(lines) + "\n")
    config = tmp_path / "nnet.config"
    config.write_text("nnet_type = lstm\ninput_dim = 6\nleft_context = 1\nright_context = 1\nsubsample = 2\nnum_layers = 2\n"
                      "num_neurons = 32\nnum_projects = 16\nnum_targets = 9\nuse_peepholes = true\ndropout_rate = 1.0\n")
    d = str(tmp_path)
    rc, err = _run("nnet-init.py", "--objective=ctc", "--batch-size", "2", str(scp), str(config), d + "/nnet.0")
    assert rc == 0, err
    rc, err = _run("nnet-train.py", "--objective=ctc", "--batch-size", "2", "--learn-rate=0.01", "--optimizer=adam", "--seed=1",
                   "--shuffle=false", "--delay-penalty", "0.05", str(scp), str(config), d + "/nnet.0", d + "/nnet.1")
    assert rc == 0, err
    penalty, mean, n = _entry_line(err)
    assert penalty == 0.05 and n == labels and 0.0 <= mean < 20.0, err        # 20 = the longest utterance after subsampling
    assert np.isfinite(_logged(err, "tr_loss")) and os.path.getsize(d + "/nnet.1") > 0
    val = ["--objective=ctc", "--batch-size", "2", str(scp), str(config), d + "/nnet.1"]
    rc, err = _run("nnet-validate.py", *val)
    assert rc == 0, err
    plain = _logged(err, "cv_loss")
    assert "delay penalty" not in err
    rc, err = _run("nnet-validate.py", "--delay-penalty", "0", *val)            # plain CTC plus the metric
    assert rc == 0, err
    assert abs(_logged(err, "cv_loss") - plain) <= 1e-4 * abs(plain), (err, plain)
    penalty0, mean0, n0 = _entry_line(err)
    assert penalty0 == 0.0 and n0 == labels and 0.0 <= mean0 < 20.0
    rc, err = _run("nnet-validate.py", "--delay-penalty", "0.5", *val)
    assert rc == 0, err
    assert _logged(err, "cv_loss") >= plain * (1 - 1e-4)
    assert _entry_line(err)[1] <= mean0 + 1e-3                                   # the tilted posterior enters no later


def test_zz_report_measured_error_over_bar():
    text = ("ctc_delay: largest measured error / project bar (GRAD_TOL = %g) over %d utterances with a path: loss %.4f, "
            "entry_sum %.4f, grad %.4f" % (BAR, MEASURED["n"], MEASURED["loss"], MEASURED["entry"], MEASURED["grad"]))
    print("\n" + text)
    out = os.environ.get("LC_MEASURED_DIR")              # where to keep the line; unset: printed only
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "ctc_delay_measured.txt"), "w") as f:
            f.write(text + "\n")
    assert MEASURED["loss"] <= 1.0 and MEASURED["entry"] <= 1.0 and MEASURED["grad"] <= 1.0
