"""lc_ctc_loss_windowed (alignment-windowed CTC) on the GPU, through every layer: kernel, ops, CTCGraph, command lines.

Reference: ``windowed_ctc_ref`` of tests/test_ctc_window_host.py - a float64 numpy alpha-beta recursion with the emission of
a label position set to -inf outside its window, anchored there against brute-force enumeration of all paths.

Tolerances.  The project's bar (tests/conftest.py GRAD_TOL = 1e-4): a loss within 1e-4 max(|loss|, 1) of float64, a gradient
through ``check_grad``.  Beside it the kernel's OWN error bound, derived from its arithmetic and not from what it was seen to
give (u = 2^-24; "log2 units" = error of a base-2 logarithm; first order in u):

* Per frame ONE fp32 log-sum-exp, the arithmetic of ctc_align.hip's: eps_lse(t) <= u (3 V + 8 + max|x_t|) nats (derivation:
  tests/test_gpu_align.py).
* Emission e2 = fl(fl(x - lse) * log2e): difference, constant, product: 3u |e2|, plus log2e eps_lse(t).
* A cell is a double: v = m + log2(sum_i 2^(a_i - m)), a' = v + e2.  The differences a_i - m are exact doubles rounded to
  fp32: u |a_i - m| each, which the exponential turns into a relative u ln2 |d| on a term of weight 2^-|d|: <= u / e per term,
  1.1u for three; the hardware exp2 (1 ulp): u; two fp32 additions: 2u; so the sum (in [1, 3]) is off by 4.1u relative = 5.9u
  log2 units; hardware log2 (1 ulp of a result below 1.585): 1.6u.  m + . and + e2 are DOUBLE additions: 2^-52 |a'| together.
  There is no re-centring.   delta(t, s) <= 8u + 2^-52 |alpha2(t, s)|, whatever the cell's magnitude.
* log-sum-exp is 1-Lipschitz and d log2 p / d (perturbation of cell (t, s)) is the occupancy gamma(t, s), sum_s gamma = 1:
      D = sum_t sum_s gamma(t, s) (u (8 + 3 |e2|) + 2^-52 |alpha2|) + log2e sum_t eps_lse(t)               (log2 units)
  and log2 p is off by D + 4u (the end cells' log-sum-exp).  The beta sweep is the same recursion: the same D with |beta2|.
      loss bound = ln2 (D_alpha + 4u) + u |loss|                                           (the one rounding to fp32).
* Gradient at (t, k): softmax 2^e2: eps_lse(t) + 3u.  Occupancy: the exponent alpha2 + beta2 - e2 - log2 p inherits the
  accumulated errors of alpha(t, s), beta(t, s) and log2 p.  Summed over the positions of one class these are expectations of
  the per-cell errors over the paths through that class at t - a sub-distribution of all surviving paths - hence <= D_alpha,
  D_beta and D_alpha + 4u.  The exponent is formed in double and rounded once to fp32: u |log2 gamma|, gamma-weighted <= 0.54u;
  its emission: 3u |e2| + log2e eps_lse; exp2: u; the sums (sequential + six reduction stages): (n + 6) u, n = largest number
  of positions of one class; the final subtraction: u.  With loc(t) = 0.54 + 3 sum_s gamma(t, s) |e2(t, s)|:
      grad bound = max_t [ ln2 (2 D_alpha + D_beta + 4u + u loc(t)) + 2 eps_lse(t) + (n + 11) u ].
  These bounds add errors LINEARLY over T frames (fp32 roundings are not correlated: measured errors grow like sqrt(T)), so at
  T ~ 1000 the gradient bound lies above the project's bar; both are asserted, each on its own, and the last test prints the
  largest measured / bound and measured / bar ratios.
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GRAD_TOL, check_grad
from test_ctc_window_host import OPEN, log_softmax64, random_path, windowed_ctc_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
BAR = GRAD_TOL                     # the project's bar for logits and loss
LOG2E = 1.0 / math.log(2.0)
LC_EINVAL, LC_EWORKSPACE = -1, -3
MEASURED = {"loss": 0.0, "grad": 0.0, "loss_bar": 0.0, "grad_bar": 0.0}


# ----------------------------------------------------------------------------------------------- the derived bound
def kernel_bound(ref, x, V):
    """(loss bound, gradient bound) of one utterance with a surviving path, from its float64 lattice."""
    g = ref["gamma"]
    w = g > 0
    z = lambda v: np.where(w, v, 0.0) * LOG2E
    a2, b2, e2 = np.abs(z(ref["alpha"])), np.abs(z(ref["beta"])), np.abs(z(ref["emis"]))
    eps_lse = U * (3 * V + 8 + np.abs(x).max(axis=1))
    d_alpha = float((g * (U * (8 + 3 * e2) + 2.0 ** -52 * a2)).sum() + LOG2E * eps_lse.sum())
    d_beta = float((g * (U * (8 + 3 * e2) + 2.0 ** -52 * b2)).sum() + LOG2E * eps_lse.sum())
    loss_bound = math.log(2.0) * (d_alpha + 4 * U) + U * abs(ref["loss"])
    loc = 0.54 + 3 * (g * e2).sum(axis=1)
    n = int(np.bincount(ref["ext"]).max())
    grad_bound = float((math.log(2.0) * (2 * d_alpha + d_beta + 4 * U + U * loc) + 2 * eps_lse + (n + 11) * U).max())
    return loss_bound, grad_bound


# ----------------------------------------------------------------------------------------------- cases
def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def need_frames(labels):
    return len(labels) + sum(1 for i in range(1, len(labels)) if labels[i] == labels[i - 1])


def make_labels(rng, V, L, repeat=0.3):
    labels = rng.randint(0, V - 1, L)
    for i in range(1, L):
        if rng.rand() < repeat:
            labels[i] = labels[i - 1]
    return labels


def windows_around(rng, states, L, open_share=0.3, width=5):
    """Windows that contain the path ``states``: widths 0 .. ``width`` on either side, a share of the labels unconstrained."""
    lo, hi = np.zeros(L, np.int64), np.full(L, OPEN, np.int64)
    for i in range(L):
        frames = np.flatnonzero(states == 2 * i + 1)
        if rng.rand() >= open_share:
            lo[i], hi[i] = frames[0] - rng.randint(0, width + 1), frames[-1] + rng.randint(0, width + 1)
        elif rng.rand() < 0.5:
            lo[i] = -rng.randint(0, 3)                     # unconstrained in other words than (0, INT32_MAX)
            hi[i] = len(states) - 1 + rng.randint(0, 3)
    return lo, hi


class Case:
    """A ragged batch: logits [T,B,V], per utterance (T_b, labels, lo, hi)."""

    def __init__(self, rng, V, utts, T=None, scale=2.0):
        self.V, self.B = V, len(utts)
        self.T = T or max(1, max(u[0] for u in utts))
        self.utts = utts
        self.x = (rng.randn(self.T, self.B, V) * scale).astype(np.float32)
        self.seq = np.array([u[0] for u in utts], np.int32)
        self.flat = np.concatenate([np.asarray(u[1], np.int64) for u in utts] + [np.zeros(0, np.int64)]).astype(np.int32)
        self.offs = np.concatenate(([0], np.cumsum([len(u[1]) for u in utts]))).astype(np.int32)
        self.lo = np.concatenate([np.asarray(u[2], np.int64) for u in utts] + [np.zeros(0, np.int64)]).astype(np.int32)
        self.hi = np.concatenate([np.asarray(u[3], np.int64) for u in utts] + [np.zeros(0, np.int64)]).astype(np.int32)
        self.maxlen = max(len(u[1]) for u in utts)

    def run(self, want_grad=True, lo=None, hi=None):
        from lstm_ctc_amd import ops
        loss, grad = ops.ctc_loss_windowed(_dev(self.x, np.float32), _dev(self.flat, np.int32), _dev(self.offs, np.int32),
                                           _dev(self.seq, np.int32), self.maxlen,
                                           _dev(self.lo if lo is None else lo, np.int32),
                                           _dev(self.hi if hi is None else hi, np.int32), want_grad=want_grad)
        torch.cuda.synchronize()
        return loss.cpu().numpy(), None if grad is None else grad.cpu().numpy()

    def reference(self, b, lo=None, hi=None):
        Tb, labels = self.utts[b][0], self.utts[b][1]
        lo = self.utts[b][2] if lo is None else lo
        hi = self.utts[b][3] if hi is None else hi
        return windowed_ctc_ref(self.x[:Tb, b].astype(np.float64), labels, lo, hi, self.V - 1)


def check_against_reference(case, loss, grad, tag, utterances=None, refs=None):
    """Loss and gradient of every utterance with the conventions of lc_ctc_loss; bar and derived bound both asserted."""
    assert not np.isnan(grad).any() or any(_bad(case, b) for b in range(case.B)), tag
    for b in (range(case.B) if utterances is None else utterances):
        Tb, labels = case.utts[b][0], np.asarray(case.utts[b][1])
        gb = grad[:, b]
        assert np.array_equal(gb[Tb:].view(np.int32), np.zeros_like(gb[Tb:], np.int32)), (tag, b, "rows beyond seq_len")
        if Tb <= 0 or len(labels) > Tb:
            assert loss[b] == 0.0 and not gb.any(), (tag, b, "skipped utterance")
            continue
        ref = refs[b] if refs is not None else case.reference(b)
        if not np.isfinite(ref["loss"]):
            assert loss[b] == np.inf, (tag, b, loss[b])
            assert not np.isnan(gb).any()
            check_grad(gb[:Tb], ref["grad"], tag, "utt%d/softmax" % b)
            continue
        lb, gbound = kernel_bound(ref, case.x[:Tb, b].astype(np.float64), case.V)
        err = abs(float(loss[b]) - ref["loss"])
        gerr = float(np.abs(gb[:Tb] - ref["grad"]).max())
        print("%s utt %d: T_b %d L %d  loss %.6f ref %.6f err %.2e (bound %.2e, bar %.2e)  grad err %.2e (bound %.2e)"
              % (tag, b, Tb, len(labels), loss[b], ref["loss"], err, lb, BAR * max(abs(ref["loss"]), 1.0), gerr, gbound))
        MEASURED["loss"] = max(MEASURED["loss"], err / lb)
        MEASURED["grad"] = max(MEASURED["grad"], gerr / gbound)
        MEASURED["loss_bar"] = max(MEASURED["loss_bar"], err / (BAR * max(abs(ref["loss"]), 1.0)))
        MEASURED["grad_bar"] = max(MEASURED["grad_bar"], gerr / (BAR * max(float(np.abs(ref["grad"]).max()), 1e-3)))
        assert err <= BAR * max(abs(ref["loss"]), 1.0), (tag, b, loss[b], ref["loss"])
        assert err <= lb, (tag, b, err, lb)
        check_grad(gb[:Tb], ref["grad"], tag, "utt%d" % b)
        assert gerr <= gbound, (tag, b, gerr, gbound)
        assert np.abs(gb[:Tb].sum(axis=1)).max() <= case.V * BAR, (tag, b, "live rows sum to 0")


def _bad(case, b):
    labels = np.asarray(case.utts[b][1])
    return bool(len(labels) and (labels.min() < 0 or labels.max() >= case.V - 1))


def feasible_utts(rng, V, L, slack=(0, 1, 3, 7), empty=True):
    """Utterances of L labels each with T_b = the minimum the labels need (repeats included) + slack, feasible windows that
    mix constrained and unconstrained labels; plus one of length 0."""
    utts = []
    for extra in slack:
        labels = make_labels(rng, V, L)
        Tb = max(need_frames(labels), 1) + extra
        states = random_path(rng, labels, Tb)
        lo, hi = windows_around(rng, states, L)
        utts.append((Tb, labels, lo, hi))
    if empty:
        utts.append((0, make_labels(rng, V, min(L, 3)), np.zeros(min(L, 3)), np.full(min(L, 3), OPEN)))
    return utts


# Sweep geometry: positions per lane switch at S = 2L + 1 = 64, 128, 256, 512, 1024 (L = 31|32, 63|64, 127|128, 255|256,
# 511|512); the row pitch is roundup(S, 64), so lanes beyond it skip their stores (L = 70, 300, 600); frames fetched per chunk
# 8, 8, 8, 4, 2, 1; re-centring every 8 frames.  Gradient: four frames per workgroup, classes in strides of 64 lanes, blank
# positions in strides of 128, the class lists are built by 256 threads (L, V above 256).
GEOMETRY = [(0, 2), (0, 44), (1, 2), (1, 44), (2, 129), (2, 1100), (31, 44), (32, 44), (63, 129), (64, 44), (70, 2),
            (127, 44), (128, 1100), (255, 44), (256, 129), (300, 44), (511, 2), (512, 44), (600, 129), (1023, 44)]


@pytest.mark.parametrize("L,V", GEOMETRY)
def test_geometry_edges(L, V):
    rng = np.random.RandomState(1000 * V + L)
    case = Case(rng, V, feasible_utts(rng, V, L))
    loss, grad = case.run()
    check_against_reference(case, loss, grad, "geom L%d V%d" % (L, V))


def test_one_frame_and_one_utterance():
    rng = np.random.RandomState(1)
    for V in (2, 44):
        for labels, lo, hi in (([], [], []), ([0], [0], [0]), ([0], [-3], [OPEN])):
            case = Case(rng, V, [(1, np.array(labels, np.int64), np.array(lo), np.array(hi))])     # T = 1, B = 1
            loss, grad = case.run()
            check_against_reference(case, loss, grad, "T1B1 V%d L%d" % (V, len(labels)))


def test_b65_ragged():
    """B = 65: more utterances than one wave's lanes, 2 * 65 sweep waves, T * B not a multiple of the gradient's four frames."""
    rng = np.random.RandomState(2)
    V = 44
    utts = []
    for b in range(65):
        L = int(rng.randint(0, 9))
        labels = make_labels(rng, V, L)
        Tb = 0 if b % 13 == 5 else max(need_frames(labels), 1) + int(rng.randint(0, 12))
        states = random_path(rng, labels, Tb) if Tb else None
        lo, hi = windows_around(rng, states, L) if Tb else (np.zeros(L), np.full(L, OPEN))
        utts.append((Tb, labels, lo, hi))
    case = Case(rng, V, utts, T=23)
    loss, grad = case.run()
    check_against_reference(case, loss, grad, "B65")


# ----------------------------------------------------------------------------------------------- unconstrained = lc_ctc_loss
@pytest.mark.parametrize("V", [44, 129])
def test_unconstrained_windows_reproduce_ctc_loss(V):
    """Both kernels against the float64 CTC value on the same inputs (each with float64, not with each other)."""
    from lstm_ctc_amd import ops
    rng = np.random.RandomState(V)
    utts = []
    for L, extra in ((5, 0), (12, 9), (0, 4), (40, 30), (3, 60)):
        labels = make_labels(rng, V, L)
        utts.append((need_frames(labels) + extra + (L == 0), labels, np.zeros(L), np.full(L, OPEN)))
    case = Case(rng, V, utts)
    refs = [case.reference(b) for b in range(case.B)]
    loss_w, grad_w = case.run()
    lo2 = np.concatenate([-np.arange(len(u[1])) for u in utts]).astype(np.int32)          # "lo <= 0, hi >= T - 1" as well
    hi2 = np.full(len(case.flat), case.T - 1, np.int32)
    loss_w2, grad_w2 = case.run(lo=lo2, hi=hi2)
    assert np.array_equal(loss_w, loss_w2) and np.array_equal(grad_w, grad_w2)
    loss_c, grad_c = ops.ctc_loss(_dev(case.x, np.float32), _dev(case.flat, np.int32), _dev(case.offs, np.int32),
                                  _dev(case.seq, np.int32), case.maxlen)
    loss_c, grad_c = loss_c.cpu().numpy(), grad_c.cpu().numpy()
    check_against_reference(case, loss_w, grad_w, "open V%d" % V, refs=refs)
    for b in range(case.B):
        Tb = utts[b][0]
        assert abs(loss_c[b] - refs[b]["loss"]) <= BAR * max(abs(refs[b]["loss"]), 1.0)
        check_grad(grad_c[:Tb, b], refs[b]["grad"], "lc_ctc_loss V%d" % V, "utt%d" % b)


# ----------------------------------------------------------------------------------------------- sandwich with lc_ctc_align
@pytest.mark.parametrize("T,V,L,B", [(60, 8, 12, 3), (1000, 44, 100, 4)])
def test_sandwich_with_the_alignment_kernel(T, V, L, B):
    """loss_unconstrained <= loss(tau = 3) <= loss(tau = 0) <= -score, windows from lc_ctc_align's path on the same logits."""
    from lstm_ctc_amd import ops
    rng = np.random.RandomState(T + V)
    utts = []
    for b in range(B):
        labels = make_labels(rng, V, L - b)
        utts.append((T - 7 * b, labels, np.zeros(L - b), np.full(L - b, OPEN)))
    case = Case(rng, V, utts, T=T)
    ali, lidx, score = ops.ctc_align(_dev(case.x, np.float32), _dev(case.flat, np.int32), _dev(case.offs, np.int32),
                                     _dev(case.seq, np.int32), case.maxlen)
    ali, score = ali.cpu().numpy(), score.cpu().numpy().astype(np.float64)
    assert np.isfinite(score).all()
    losses = [case.run()[0].astype(np.float64)]
    for tau in (3, 0):
        lo, hi, ok = ops.label_windows(ali, case.flat, case.offs, case.seq, tau, V - 1)
        assert ok.all()
        loss, grad = case.run(lo=lo, hi=hi)
        assert np.isfinite(loss).all()                             # finite whenever the score is
        losses.append(loss.astype(np.float64))
        if tau == 0:                                               # and right: against float64 on the tightest windows
            for b in range(B):
                o0, o1 = case.offs[b], case.offs[b + 1]
                case.utts[b] = (utts[b][0], utts[b][1], lo[o0:o1], hi[o0:o1])
            check_against_reference(case, loss, grad, "sandwich T%d tau0" % T)
    losses.append(-score)
    print("\nsandwich T=%d: unconstrained %s tau=3 %s tau=0 %s -score %s" % ((T,) + tuple(np.round(l, 3) for l in losses)))
    for lower, upper in zip(losses, losses[1:]):
        tol = BAR * np.maximum(np.abs(upper), 1.0)
        assert (lower <= upper + tol).all(), (lower, upper)
    assert (losses[0] < losses[2]).all()                           # and the windows do bite


# ----------------------------------------------------------------------------------------------- what the mask must do
def test_masked_classes_get_the_softmax():
    """Where no position of class k is inside its window at frame t, grad[t, b, k] is the softmax."""
    rng = np.random.RandomState(4)
    V, T = 6, 40
    labels = np.array([0, 1, 0, 2, 2, 3])
    states = random_path(rng, labels, T)
    lo = np.array([np.flatnonzero(states == 2 * i + 1)[0] - 1 for i in range(6)])
    hi = np.array([np.flatnonzero(states == 2 * i + 1)[-1] + 1 for i in range(6)])
    case = Case(rng, V, [(T, labels, lo, hi), (T - 5, labels, np.zeros(6), np.full(6, OPEN))], T=T)
    loss, grad = case.run()
    check_against_reference(case, loss, grad, "mask")
    soft = np.exp(log_softmax64(case.x[:, 0].astype(np.float64)))
    t = np.arange(T)[:, None]
    inside = (t >= lo[None, :]) & (t <= hi[None, :])                       # [T, L]
    masked = np.ones((T, V), bool)
    masked[:, V - 1] = False                                               # the blank is never masked
    for i, k in enumerate(labels):
        masked[:, k] &= ~inside[:, i]
    assert masked[:, :4].any(axis=0).all() and not masked.all()
    assert np.abs(grad[:, 0][masked] - soft[masked]).max() <= BAR * max(soft[masked].max(), 1e-3)
    assert (np.abs(grad[:, 0][~masked] - soft[~masked]).max() > 1e-3)      # elsewhere the occupancy is there


# ----------------------------------------------------------------------------------------------- conventions
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
        (T, np.array([1, 1, 3]), np.array([4, 5, 0]), np.array([4, 5, 11])),         # 6 no frame for the blank between 1 1
        (2, np.array([2, 2]), np.zeros(2), np.full(2, OPEN)),                        # 7 L fits, the blank between does not
        (T - 1, np.array([4, 4, 0]), np.array([0, 2, 0]), np.array([3, 9, OPEN])),   # 8 fine
        (0, np.array([1])) + (np.zeros(1), np.full(1, OPEN)),                        # 9 no frames
    ]
    case = Case(rng, V, utts, T=T)
    loss, grad = case.run()
    assert np.isnan(loss[[2, 3]]).all() and not grad[:, [2, 3]].any()
    assert loss[1] == 0.0 and loss[9] == 0.0 and not grad[:, [1, 9]].any()
    assert (loss[[4, 5, 6, 7]] == np.inf).all()
    assert not np.isnan(grad).any() and not np.isnan(loss[[0, 1, 4, 5, 6, 7, 8, 9]]).any()
    check_against_reference(case, loss, grad, "conventions", utterances=[0, 1, 4, 5, 6, 7, 8, 9])
    assert np.isfinite(loss[[0, 8]]).all()
    # the sweep meets a row in which every cell is dead half-way through, on a lattice wider than one lane group
    L = 40
    labels = make_labels(rng, 44, L, repeat=0.0)
    T2 = 100
    states = random_path(rng, labels, T2)
    lo, hi = windows_around(rng, states, L, open_share=0.0, width=0)
    blocked_lo, blocked_hi = lo.copy(), hi.copy()
    blocked_lo[L // 2], blocked_hi[L // 2] = 7, 3                              # no frame for one label in the middle
    case2 = Case(rng, 44, [(T2, labels, blocked_lo, blocked_hi), (T2, labels, lo, hi)], T=T2)
    loss2, grad2 = case2.run()
    assert loss2[0] == np.inf and np.isfinite(loss2[1]) and not np.isnan(grad2).any()
    check_against_reference(case2, loss2, grad2, "dead row")


# ----------------------------------------------------------------------------------------------- determinism and coverage
def _raw(lib, x, T, B, V, flat, offs, seq, maxlen, lo, hi, loss, grad, ws, nbytes):
    p = lambda t: None if t is None else t.data_ptr()
    rc = lib.lc_ctc_loss_windowed(p(x), T, B, V, p(flat), p(offs), p(seq), maxlen, p(lo), p(hi), p(loss), p(grad), p(ws),
                                  nbytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def test_every_element_is_written_and_calls_are_bit_identical():
    from lstm_ctc_amd import _lib
    lib = _lib.load()
    rng = np.random.RandomState(6)
    V = 44
    utts = feasible_utts(rng, V, 70) + feasible_utts(rng, V, 9, slack=(0, 30))
    utts.append((50, make_labels(rng, V, 4), np.array([0, 9, 0, 0]), np.array([OPEN, 3, OPEN, OPEN])))      # no path
    utts.append((3, make_labels(rng, V, 9), np.zeros(9), np.full(9, OPEN)))                                    # skipped
    case = Case(rng, V, utts)
    T, B = case.T, case.B
    dev = [_dev(case.x, np.float32), _dev(case.flat, np.int32), _dev(case.offs, np.int32), _dev(case.seq, np.int32),
           _dev(case.lo, np.int32), _dev(case.hi, np.int32)]
    nbytes = lib.lc_ctc_window_workspace_bytes(T, B, V, case.maxlen)
    outs = []
    for fill in (float("nan"), None):
        if fill is None:                                   # 0xFF bytes everywhere: NaNs with another payload, -1 integers
            ws = torch.full((nbytes,), 255, dtype=torch.uint8, device="cuda")
            loss = torch.full((B,), 255, dtype=torch.uint8, device="cuda").repeat_interleave(4).view(torch.float32)
            grad = torch.full((T * B * V * 4,), 255, dtype=torch.uint8, device="cuda").view(torch.float32).view(T, B, V)
        else:
            ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
            loss = torch.full((B,), fill, device="cuda")
            grad = torch.full((T, B, V), fill, device="cuda")
        assert _raw(lib, dev[0], T, B, V, dev[1], dev[2], dev[3], case.maxlen, dev[4], dev[5], loss, grad, ws, nbytes) == 0
        outs.append((loss.cpu().numpy().copy(), grad.cpu().numpy().copy()))
        loss_only = torch.full((B,), 7.0, device="cuda")
        assert _raw(lib, dev[0], T, B, V, dev[1], dev[2], dev[3], case.maxlen, dev[4], dev[5], loss_only, None, ws, nbytes) == 0
        assert np.array_equal(loss_only.cpu().numpy().view(np.int32), outs[-1][0].view(np.int32))              # grad = NULL
    assert np.array_equal(outs[0][0].view(np.int32), outs[1][0].view(np.int32))
    assert np.array_equal(outs[0][1].view(np.int32), outs[1][1].view(np.int32))
    check_against_reference(case, outs[0][0], outs[0][1], "coverage")


def test_argument_checks_launch_nothing():
    from lstm_ctc_amd import _lib
    lib = _lib.load()
    rng = np.random.RandomState(7)
    V = 10
    case = Case(rng, V, feasible_utts(rng, V, 3, slack=(0, 2), empty=False))
    T, B = case.T, case.B
    x, flat, offs, seq = (_dev(case.x, np.float32), _dev(case.flat, np.int32), _dev(case.offs, np.int32),
                          _dev(case.seq, np.int32))
    lo, hi = _dev(case.lo, np.int32), _dev(case.hi, np.int32)
    nbytes = lib.lc_ctc_window_workspace_bytes(T, B, V, case.maxlen)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    loss = torch.full((B,), float("nan"), device="cuda")
    grad = torch.full((T, B, V), float("nan"), device="cuda")
    untouched = lambda: bool(torch.isnan(loss).all()) and bool(torch.isnan(grad).all())
    good = dict(x=x, T=T, B=B, V=V, flat=flat, offs=offs, seq=seq, maxlen=case.maxlen, lo=lo, hi=hi, loss=loss, grad=grad,
                ws=ws, nbytes=nbytes)
    for kw in (dict(T=0), dict(T=-1), dict(B=0), dict(B=-2), dict(V=1), dict(V=0), dict(maxlen=-1), dict(maxlen=1024),
               dict(x=None), dict(flat=None), dict(offs=None), dict(seq=None), dict(lo=None), dict(hi=None),
               dict(loss=None), dict(ws=None)):
        assert _raw(lib, **dict(good, **kw)) == LC_EINVAL, kw
        assert untouched(), kw
    for short in (0, nbytes - 1):
        assert _raw(lib, **dict(good, nbytes=short)) == LC_EWORKSPACE
        assert untouched()
    assert lib.lc_last_error().decode().startswith("lc_ctc_loss_windowed: workspace too small")
    assert _raw(lib, **good) == 0
    assert not untouched()


# ----------------------------------------------------------------------------------------------- the graph
SMOKE_CFG = dict(nnet_type="blstm", input_dim=8, left_context=0, right_context=0, num_layers=2, num_neurons=32,
                 num_projects=16, num_targets=11, use_peepholes=True, dropout_rate=1.0)       # __graft_entry__.smoke's


def _smoke_batch():
    rng = np.random.default_rng(0)
    B, T = 4, 20
    seq = np.array([20, 17, 12, 9], np.int32)
    x = rng.normal(size=(B, T, 8)).astype(np.float32)
    target = np.full((B, 6), -1, np.int64)
    for b, n in enumerate((6, 5, 4, 3)):
        x[b, seq[b]:] = 0
        target[b, :n] = rng.integers(0, 10, size=n)
    return {"nnet_input": x, "sequence_length": seq, "nnet_target": target}


def test_graph_step_with_align_window(oracle):
    from lstm_ctc_amd import ops
    from lstm_ctc_amd.nnet.graph import CTCGraph, flatten_labels
    batch = _smoke_batch()
    V, tau = SMOKE_CFG["num_targets"], 2
    graph = CTCGraph(None, SMOKE_CFG, learn_rate=1e-3, l2_decay_weight=0.0, seed=1, align_window=tau)
    with pytest.raises(ValueError, match="frame_targets="):
        graph.step(batch)
    assert graph.global_step == 0
    ali = graph.align(batch)
    assert np.isfinite(ali["score"]).all()
    batch = dict(batch, frame_target=ali["ali"])
    p64 = {k: v.astype(np.float64) for k, v in graph.model.ps.export_tf().items()}
    out = graph.step(batch, fetch_eval=True)
    assert (graph.windows_constrained, graph.windows_unconstrained) == (4, 0)
    # float64: the oracle's forward, this file's windowed criterion on its logits, the oracle's backward
    flat, offs, _ = flatten_labels(batch["nnet_target"])
    seq = batch["sequence_length"]
    lo, hi, ok = ops.label_windows(ali["ali"], flat, offs, seq, tau, V - 1)
    assert ok.all() and (hi - lo >= 2 * tau).all()
    ref_logits, saved = oracle.forward(p64, SMOKE_CFG, batch["nnet_input"].astype(np.float64), seq)          # [B,T,V]
    dlogits = np.zeros_like(ref_logits)
    total = 0.0
    for b in range(4):
        ref = windowed_ctc_ref(ref_logits[b, :seq[b]], flat[offs[b]:offs[b + 1]], lo[offs[b]:offs[b + 1]],
                               hi[offs[b]:offs[b + 1]], V - 1)
        dlogits[b, :seq[b]] = ref["grad"]
        total += ref["loss"]
    plain, _, _ = oracle.ctc_loss(np.ascontiguousarray(ref_logits.transpose(1, 0, 2)), flat, offs, seq)
    assert total > float(np.sum(plain)) + 1e-3                      # the windows bite on this batch
    assert abs(out["eval_loss"] - total) <= BAR * max(abs(total), 1.0), (out["eval_loss"], total)
    ref_grads, _ = oracle.backward(p64, SMOKE_CFG, saved, dlogits)
    got = graph.model.ps.export_tf(grads=True)
    for k in ref_grads:
        check_grad(got[k], ref_grads[k], "graph align_window", k)
    assert "decoded" in out and out["size"] == len(flat)            # greedy eval is what it was


def test_graph_without_align_window_is_untouched_and_all_missing_rows_are_plain_ctc():
    from lstm_ctc_amd.nnet.graph import CTCGraph, create_graph_for_training_ctc
    batch = _smoke_batch()
    outs = []
    for kw in (dict(), dict(align_window=None)):
        graph = create_graph_for_training_ctc(None, SMOKE_CFG, learn_rate=1e-2, seed=1, **kw)
        assert graph.align_window is None
        steps = [graph.step(batch, fetch_eval=True) for _ in range(2)]
        outs.append(([s["eval_loss"] for s in steps], [s["grad_norm"] for s in steps], graph.model.ps.flat.clone()))
        assert (graph.windows_constrained, graph.windows_unconstrained) == (0, 0)
    assert outs[0][0] == outs[1][0] and outs[0][1] == outs[1][1] and torch.equal(outs[0][2], outs[1][2])
    # every row -1 (no entry / wrong length): plain CTC through the windowed kernel, every utterance counted unconstrained
    plain = CTCGraph(None, SMOKE_CFG, seed=1).step(batch)["eval_loss"]
    graph = CTCGraph(None, SMOKE_CFG, seed=1, align_window=0)
    missing = dict(batch, frame_target=np.full((4, 20), -1, np.int32))
    got = graph.step(None, staged=graph.stage(missing))["eval_loss"]            # through the prefetch path
    assert abs(got - plain) <= BAR * max(abs(plain), 1.0), (got, plain)
    assert (graph.windows_constrained, graph.windows_unconstrained) == (0, 4)
    for bad in (dict(objective="xent", align_window=1), dict(align_window=-1), dict(align_window=1.5)):
        with pytest.raises(ValueError, match="align_window"):
            CTCGraph(None, SMOKE_CFG, seed=1, **bad)


# ----------------------------------------------------------------------------------------------- command lines
def _run(cli, *args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", cli)] + list(args), capture_output=True, timeout=300)
    return r.returncode, r.stderr.decode()


def _logged(err, name):
    lines = [l for l in err.split("\n") if l.startswith("INFO:tensorflow:%s = " % name)]
    assert len(lines) == 1, err
    return float(lines[0].split()[-1])


def test_cli_align_then_windowed_train_and_validate(tmp_path):
    import lstm_ctc_amd.nnet as nnet
    rng = np.random.default_rng(7)
    D, V = 6, 9
    lines = []
    for i, T in enumerate([20, 24, 31, 40]):
        path = str(tmp_path / ("utt%03d.tfrecords" % i))
        nnet.write_tfrecord(path, rng.normal(size=(T, D)).astype(np.float32), rng.integers(0, V - 1, size=int(rng.integers(1, 5))))
        lines.append("utt%03d %d %d 1 %s" % (i, T, D, path))
    scp = tmp_path / "tfrecords.scp"
    scp.write_text("\n".join(lines) + "\n")
    config = tmp_path / "nnet.config"
    config.write_text("nnet_type = blstm\ninput_dim = 6\nleft_context = 1\nright_context = 1\nsubsample = 2\nnum_layers = 2\n"
                      "num_neurons = 32\nnum_projects = 16\nnum_targets = 9\nuse_peepholes = true\ndropout_rate = 1.0\n")
    d = str(tmp_path)
    for seed_dir in ("a", "b"):                        # two random models: nnet-init draws fresh weights on every run
        os.mkdir(os.path.join(d, seed_dir))
        rc, err = _run("nnet-init.py", "--objective=ctc", "--batch-size", "2", str(scp), str(config), d + "/%s/nnet.0" % seed_dir)
        assert rc == 0, err
        rc, err = _run("nnet-align.py", str(scp), str(config), d + "/%s/nnet.0" % seed_dir, "ark:" + d + "/%s/ali.ark" % seed_dir)
        assert rc == 0, err
    train = ["--objective=ctc", "--batch-size", "2", "--learn-rate=0.01", "--optimizer=adam", "--seed=1", "--shuffle=false"]
    rc, err = _run("nnet-train.py", *(train + ["--frame-targets", "ark:" + d + "/a/ali.ark", "--align-window", "1",
                                               str(scp), str(config), d + "/a/nnet.0", d + "/a/nnet.1"]))
    assert rc == 0, err
    assert ("INFO:tensorflow:label windows (+-1 frames): 4 utterance(s) constrained, 0 unconstrained (no entry, another "
            "length, or an alignment that does not spell the labels)") in err, err
    assert np.isfinite(_logged(err, "tr_loss")) and os.path.getsize(d + "/a/nnet.1") > 0
    # validation: windows wider than any utterance change nothing
    val = ["--objective=ctc", "--batch-size", "2", str(scp), str(config), d + "/a/nnet.1"]
    rc, err = _run("nnet-validate.py", *val)
    assert rc == 0, err
    plain = _logged(err, "cv_loss")
    assert "label windows" not in err
    rc, err = _run("nnet-validate.py", "--frame-targets", "ark:" + d + "/a/ali.ark", "--align-window", "100000", *val)
    assert rc == 0, err
    assert abs(_logged(err, "cv_loss") - plain) <= 1e-4 * abs(plain), (err, plain)
    assert "label windows (+-100000 frames): 4 utterance(s) constrained, 0 unconstrained" in err
    # another model's alignment with the tightest windows still runs; an utterance without an entry and one whose entry has
    # another length train on plain CTC and are counted, nothing is fatal
    from lstm_ctc_amd.kaldi_io import Int32VectorWriter, read_int32_vector_ark
    table = read_int32_vector_ark(d + "/b/ali.ark")
    w = Int32VectorWriter("ark,t:" + d + "/b/ali_partial.txt")
    for i, k in enumerate(sorted(table)):
        if i == 1:
            continue                                   # no entry
        w.Write(k, table[k][:-1] if i == 2 else table[k])
    w.Close()
    rc, err = _run("nnet-train.py", *(train + ["--frame-targets", "ark,t:" + d + "/b/ali_partial.txt", "--align-window", "0",
                                               str(scp), str(config), d + "/a/nnet.0", d + "/a/nnet.2"]))
    assert rc == 0, err
    assert "label windows (+-0 frames): 2 utterance(s) constrained, 2 unconstrained" in err, err
    assert "INFO:tensorflow:frame targets: 1 utterance(s) without an entry, 1 with an entry of another length" in err, err
    assert np.isfinite(_logged(err, "tr_loss")) and os.path.getsize(d + "/a/nnet.2") > 0


def test_zz_report_measured_error_over_bound():
    print("\nctc_window: largest measured error / derived bound: loss %.3f, grad %.3f; / project bar: loss %.4f, grad %.4f"
          % (MEASURED["loss"], MEASURED["grad"], MEASURED["loss_bar"], MEASURED["grad_bar"]))
    assert MEASURED["loss"] <= 1.0 and MEASURED["grad"] <= 1.0 and MEASURED["loss_bar"] <= 1.0 and MEASURED["grad_bar"] <= 1.0
