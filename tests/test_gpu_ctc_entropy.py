"""lc_ctc_loss_entropy (maximum-entropy CTC: the CTC loss, the entropy of the posterior over the feasible paths and the
gradient of loss - eta * entropy) on the GPU, through every layer: kernel, ops, CTCGraph, command lines.

Reference: ``entropy_ctc_ref`` of tests/test_ctc_entropy_host.py - float64 numpy, anchored there against brute-force
enumeration of all paths and central differences - evaluated on the same fp32 logits.

Tolerances are the project's bar (tests/conftest.py GRAD_TOL = 1e-4), not new numbers: a loss within GRAD_TOL max(|loss_ref|, 1)
of float64, a gradient through ``check_grad``, live gradient rows summing to 0 within V GRAD_TOL.  The entropy is log Z - Ebar,
two sums over the same fp32 emissions, so GRAD_TOL max(|loss_ref|, 1) is all that could be asked of it a priori; the tighter
GRAD_TOL max(|H_ref|, 1) was measured over this whole file at 0.0057 of that bar (profiles/ctc_entropy_measured.txt), far
inside the project's margin of 1 / 2.7, and is therefore what every case asserts.  Both ratios are still recorded.
Every kernel call runs on guarded output buffers (a band of sentinels on either side, checked after the call), NaN-filled
outputs and a workspace of 0xFF bytes between guard bands.  The last test prints
the largest measured / bar ratios and, with LC_MEASURED_DIR set, writes them to ctc_entropy_measured.txt in that directory
(kept as profiles/ctc_entropy_measured.txt)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GRAD_TOL, check_grad
from test_ctc_entropy_host import count_paths, entropy_ctc_ref
from test_ctc_window_host import OPEN, random_path
from test_gpu_ctc_delay import GEOMETRY, _b65, _guarded, _intact, _long_case, make_case
from test_gpu_ctc_window import SMOKE_CFG, Case, _dev, _smoke_batch, feasible_utts, make_labels, need_frames, windows_around

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = GRAD_TOL
LC_EINVAL, LC_EWORKSPACE = -1, -3
MEASURED = {"loss": 0.0, "entropy": 0.0, "entropy_tight": 0.0, "grad": 0.0, "n": 0}


# ----------------------------------------------------------------------------------------------- calling the kernel
def call(case, eta, want_grad=True, windowed=None):
    """One lc_ctc_loss_entropy call -> (loss, entropy, grad or None) on the host."""
    from lstm_ctc_amd import _lib
    lib = _lib.load()
    T, B, V = case.T, case.B, case.V
    windowed = case.windowed if windowed is None else windowed
    x, flat, offs, seq = (_dev(case.x, np.float32), _dev(case.flat if len(case.flat) else np.zeros(1), np.int32),
                          _dev(case.offs, np.int32), _dev(case.seq, np.int32))
    lo = _dev(case.lo if len(case.lo) else np.zeros(1), np.int32) if windowed else None
    hi = _dev(case.hi if len(case.hi) else np.zeros(1), np.int32) if windowed else None
    nbytes = lib.lc_ctc_entropy_workspace_bytes(T, B, V, case.maxlen)
    assert nbytes > 0
    wsbuf = torch.full((nbytes + 512,), 0xA5, dtype=torch.uint8, device="cuda")
    ws = wsbuf[256:256 + nbytes]
    ws.fill_(0xFF)
    nan = float("nan")
    lbuf, loss = _guarded((B,), nan)
    ebuf, entropy = _guarded((B,), nan)
    gbuf, grad = _guarded((T, B, V), nan) if want_grad else (None, None)
    p = lambda t: None if t is None else t.data_ptr()
    rc = lib.lc_ctc_loss_entropy(p(x), T, B, V, p(flat), p(offs), p(seq), case.maxlen, p(lo), p(hi), float(eta), p(loss),
                                 p(entropy), p(grad), p(ws), nbytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, lib.lc_last_error()
    assert _intact(lbuf) and _intact(ebuf) and (gbuf is None or _intact(gbuf)), "a guard band was written"
    assert bool((wsbuf[:256] == 0xA5).all()) and bool((wsbuf[256 + nbytes:] == 0xA5).all()), "the workspace's guards were written"
    host = lambda t: None if t is None else t.cpu().numpy().copy()
    return host(loss), host(entropy), host(grad)


def reference(case, b, eta, windowed=None):
    Tb, labels, lo, hi = case.utts[b]
    windowed = case.windowed if windowed is None else windowed
    return entropy_ctc_ref(case.x[:Tb, b].astype(np.float64), labels, eta, case.V - 1, *((lo, hi) if windowed else (None, None)))


def check_against_reference(case, eta, loss, entropy, grad, tag, utterances=None, windowed=None):
    """Loss, entropy and gradient of every utterance: compared with the reference, or one of the convention cases, which
    are asserted exactly."""
    for b in (range(case.B) if utterances is None else utterances):
        Tb, labels = case.utts[b][0], np.asarray(case.utts[b][1])
        gb = None if grad is None else grad[:, b]
        if gb is not None:
            assert np.array_equal(gb[Tb:].view(np.int32), np.zeros_like(gb[Tb:], np.int32)), (tag, b, "rows beyond seq_len")
        if Tb <= 0 or len(labels) > Tb:
            assert loss[b] == 0.0 and entropy[b] == 0.0 and (gb is None or not gb.any()), (tag, b, "skipped utterance")
            continue
        ref = reference(case, b, eta, windowed)
        if not np.isfinite(ref["loss"]):
            assert loss[b] == np.inf and entropy[b] == 0.0, (tag, b, loss[b], entropy[b])
            if gb is not None:
                assert not np.isnan(gb).any()
                check_grad(gb[:Tb], ref["grad"], tag, "utt%d/softmax" % b)
            continue
        err = abs(float(loss[b]) - ref["loss"])
        herr = abs(float(entropy[b]) - ref["entropy"])
        lbar, hbar = BAR * max(abs(ref["loss"]), 1.0), BAR * max(abs(ref["entropy"]), 1.0)
        gerr = gbar = 0.0
        if gb is not None:
            gerr = float(np.abs(gb[:Tb] - ref["grad"]).max())
            gbar = BAR * max(float(np.abs(ref["grad"]).max()), 1e-3)
            MEASURED["grad"] = max(MEASURED["grad"], gerr / gbar)
        print("%s utt %d: T_b %d L %d  loss %.6f ref %.6f err %.2e (bar %.2e)  entropy %.6f ref %.6f err %.2e (bar %.2e, tight "
              "%.2e)  grad err %.2e (bar %.2e)" % (tag, b, Tb, len(labels), loss[b], ref["loss"], err, lbar, entropy[b],
                                                   ref["entropy"], herr, lbar, hbar, gerr, gbar))
        MEASURED["loss"] = max(MEASURED["loss"], err / lbar)
        MEASURED["entropy"] = max(MEASURED["entropy"], herr / lbar)
        MEASURED["entropy_tight"] = max(MEASURED["entropy_tight"], herr / hbar)
        MEASURED["n"] += 1
        assert entropy[b] >= 0.0, (tag, b, entropy[b])
        assert err <= lbar, (tag, b, loss[b], ref["loss"])
        assert herr <= hbar, (tag, b, entropy[b], ref["entropy"])
        if gb is not None:
            check_grad(gb[:Tb], ref["grad"], tag, "utt%d" % b)
            assert np.abs(gb[:Tb].sum(axis=1)).max() <= case.V * BAR, (tag, b, "live rows sum to 0")


# ----------------------------------------------------------------------------------------------- geometry
@pytest.mark.parametrize("eta", [0.2, 1.0])
@pytest.mark.parametrize("L,V", GEOMETRY)
def test_geometry_edges(L, V, eta):
    """test_gpu_ctc_delay's geometry list (the positions-per-lane switches): ragged batches, T_b = frames needed +
    {0, 1, 3, 7}, plus an empty, a skipped and an infeasible utterance; half of the cases carry windows around a random path."""
    idx = GEOMETRY.index((L, V))
    windowed = (idx + (eta == 1.0)) % 2 == 1
    rng = np.random.RandomState(2000 * V + L + (7 if eta == 1.0 else 0))
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
    loss, entropy, grad = call(case, eta)
    assert loss[-1] == np.inf and loss[-2] == 0.0 and loss[-3] == 0.0
    assert entropy[-1] == 0.0 and entropy[-2] == 0.0 and entropy[-3] == 0.0
    check_against_reference(case, eta, loss, entropy, grad, "geom L%d V%d eta%g%s" % (L, V, eta, " win" if windowed else ""))


def test_one_frame_and_one_utterance():
    rng = np.random.RandomState(1)
    for V in (2, 44):
        for labels in ([], [0]):
            for windowed in (False, True):
                case = make_case(rng, V, [(1, np.array(labels, np.int64), np.zeros(len(labels)), np.zeros(len(labels)))], windowed)
                loss, entropy, grad = call(case, 0.7)                             # T = 1, B = 1: one path
                assert entropy[0] == 0.0 and not np.signbit(entropy[0])
                check_against_reference(case, 0.7, loss, entropy, grad, "T1B1 V%d L%d" % (V, len(labels)))


@pytest.mark.parametrize("windowed", [False, True])
def test_b65_ragged_and_unsorted(windowed):
    """B = 65: more utterances than one wave's lanes, T * B not a multiple of the four frames of a workgroup."""
    rng = np.random.RandomState(2)
    case = make_case(rng, 44, _b65(rng), windowed, T=23)
    loss, entropy, grad = call(case, 0.3)
    check_against_reference(case, 0.3, loss, entropy, grad, "B65")


def test_long_utterances():
    case = _long_case(1000, 44, 100, 4, False)
    loss, entropy, grad = call(case, 0.2)
    assert np.isfinite(loss).all() and (entropy > 1.0).all()
    check_against_reference(case, 0.2, loss, entropy, grad, "T1000")


# ----------------------------------------------------------------------------------------------- the siblings, bit for bit
@pytest.mark.parametrize("L,V", [(5, 8), (40, 8), (40, 129), (100, 8), (200, 8), (400, 8), (1023, 8)])
def test_bit_relations_to_windowed_and_delay(L, V):
    """One sweep template and one gradient kernel under all three entries: with windows the loss is lc_ctc_loss_windowed's,
    without windows lc_ctc_loss_delay's at lambda = 0, and at entropy_weight = 0 so is the gradient - bit for bit.  One label
    length per positions-per-lane class; a feasible utterance, one whose window excludes every frame (+inf, softmax rows) and
    one with a bad label (NaN, zero rows)."""
    from lstm_ctc_amd import ops
    rng = np.random.RandomState(5000 + 10 * L + V)
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
    bits = lambda a: a.view(np.int32)
    dev = (_dev(case.x, np.float32), _dev(case.flat, np.int32), _dev(case.offs, np.int32), _dev(case.seq, np.int32))
    lo_d, hi_d = _dev(case.lo, np.int32), _dev(case.hi, np.int32)
    loss_w, grad_w = (t.cpu().numpy() for t in ops.ctc_loss_windowed(*dev, case.maxlen, lo_d, hi_d))
    loss_d, _, grad_d = ops.ctc_loss_delay(*dev, case.maxlen, 0.0, want_entry=False)
    loss_d, grad_d = loss_d.cpu().numpy(), grad_d.cpu().numpy()
    for windowed, want_loss, want_grad in ((True, loss_w, grad_w), (False, loss_d, grad_d)):
        loss0, entropy0, grad0 = call(case, 0.0, windowed=windowed)
        loss1, entropy1, grad1 = call(case, 1.0, windowed=windowed)
        assert np.isfinite(loss0[0]) and np.isnan(loss0[2]) and (loss0[1] == np.inf) == windowed
        assert np.array_equal(bits(loss0), bits(want_loss)) and np.array_equal(bits(loss1), bits(want_loss))
        assert np.array_equal(bits(grad0), bits(want_grad))
        assert np.array_equal(bits(entropy0), bits(entropy1))                  # the entropy does not depend on its weight
        assert not np.array_equal(grad1[:, 0], grad0[:, 0]) and np.array_equal(bits(grad1[:, 2]), bits(grad0[:, 2]))
        assert not grad0[:, 2].any() and np.isnan(entropy0[2])


# ----------------------------------------------------------------------------------------------- outputs and determinism
def test_optional_gradient_and_bit_identical_calls():
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
        assert np.array_equal(bits(a), bits(b))                          # two calls are bit-identical
    no_grad = call(case, 0.2, want_grad=False)
    assert no_grad[2] is None
    assert np.array_equal(bits(no_grad[0]), bits(full[0])) and np.array_equal(bits(no_grad[1]), bits(full[1]))
    check_against_reference(case, 0.2, full[0], full[1], full[2], "coverage")
    check_against_reference(case, 0.2, no_grad[0], no_grad[1], None, "coverage, no gradient")


def test_conventions_of_ctc_loss():
    rng = np.random.RandomState(5)
    V, T = 7, 12
    open3 = (np.zeros(3), np.full(3, OPEN))
    utts = [
        (T, np.array([1, 2, 3]), np.array([0, 3, 6]), np.array([4, 8, 11])),         # 0 fine
        (2, np.array([1, 2, 3])) + open3,                                            # 1 L > T_b: loss 0, entropy 0, gradient 0
        (T, np.array([1, 6, 3])) + open3,                                            # 2 the blank as a label: NaN, NaN, gradient 0
        (T, np.array([1, -1, 3])) + open3,                                           # 3 a negative label: NaN, NaN, gradient 0
        (T, np.array([1, 2, 3]), np.array([0, 5, 0]), np.array([11, 4, 11])),        # 4 an empty window: +inf, 0, softmax
        (T, np.array([1, 2, 3]), np.array([6, 0, 0]), np.array([11, 3, 11])),        # 5 windows force the wrong order
        (2, np.array([2, 2]), np.zeros(2), np.full(2, OPEN)),                        # 6 L fits, the blank between does not
        (T - 1, np.array([4, 4, 0]), np.array([0, 2, 0]), np.array([3, 9, OPEN])),   # 7 fine
        (0, np.array([1])) + (np.zeros(1), np.full(1, OPEN)),                        # 8 no frames
        (5, np.zeros(0, np.int64), np.zeros(0), np.zeros(0)),                        # 9 L = 0: the all-blank path
        (3, np.array([0, 1, 2])) + open3,                                            # 10 T_b = L: one path
    ]
    for windowed in (True, False):
        case = make_case(rng, V, utts, windowed, T=T)
        for want_grad in (True, False):
            loss, entropy, grad = call(case, 0.5, want_grad=want_grad)
            assert np.isnan(loss[[2, 3]]).all() and np.isnan(entropy[[2, 3]]).all()
            assert loss[1] == 0.0 and loss[8] == 0.0 and entropy[1] == 0.0 and entropy[8] == 0.0
            infeasible = [4, 5, 6] if windowed else [6]
            assert (loss[infeasible] == np.inf).all() and (entropy[infeasible] == 0.0).all()
            rest = [b for b in range(11) if b not in (2, 3)]
            assert not np.isnan(loss[rest]).any() and not np.isnan(entropy[rest]).any()
            assert np.isfinite(loss[[0, 7, 9, 10]]).all()
            for b in (9, 10):                                                    # one path: +0 exactly
                assert entropy[b] == 0.0 and not np.signbit(entropy[b])
            if want_grad:
                assert not grad[:, [1, 2, 3, 8]].any() and not np.isnan(grad).any()
            check_against_reference(case, 0.5, loss, entropy, grad, "conventions", utterances=rest)


def test_argument_checks_launch_nothing():
    from lstm_ctc_amd import _lib
    lib = _lib.load()
    rng = np.random.RandomState(7)
    V = 10
    case = Case(rng, V, feasible_utts(rng, V, 3, slack=(0, 2), empty=False))
    T, B = case.T, case.B
    nbytes = lib.lc_ctc_entropy_workspace_bytes(T, B, V, case.maxlen)
    nan = float("nan")
    loss, entropy, grad = torch.full((B,), nan, device="cuda"), torch.full((B,), nan, device="cuda"), torch.full((T, B, V), nan, device="cuda")
    good = dict(x=_dev(case.x, np.float32), T=T, B=B, V=V, flat=_dev(case.flat, np.int32), offs=_dev(case.offs, np.int32),
                seq=_dev(case.seq, np.int32), maxlen=case.maxlen, lo=_dev(case.lo, np.int32), hi=_dev(case.hi, np.int32),
                eta=0.1, loss=loss, entropy=entropy, grad=grad, ws=torch.zeros(nbytes, dtype=torch.uint8, device="cuda"), nbytes=nbytes)

    def raw(x, T, B, V, flat, offs, seq, maxlen, lo, hi, eta, loss, entropy, grad, ws, nbytes):
        p = lambda t: None if t is None else t.data_ptr()
        rc = lib.lc_ctc_loss_entropy(p(x), T, B, V, p(flat), p(offs), p(seq), maxlen, p(lo), p(hi), eta, p(loss), p(entropy),
                                     p(grad), p(ws), nbytes, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc

    untouched = lambda: all(bool(torch.isnan(t).all()) for t in (loss, entropy, grad))
    for kw in (dict(T=0), dict(T=-1), dict(B=0), dict(B=-2), dict(V=1), dict(V=0), dict(maxlen=-1), dict(maxlen=1024),
               dict(x=None), dict(flat=None), dict(offs=None), dict(seq=None), dict(lo=None), dict(hi=None),
               dict(loss=None), dict(entropy=None), dict(ws=None), dict(eta=float("nan")), dict(eta=float("inf")),
               dict(eta=-float("inf"))):
        assert raw(**dict(good, **kw)) == LC_EINVAL, kw
        assert untouched(), kw
    for short in (0, nbytes - 1):
        assert raw(**dict(good, nbytes=short)) == LC_EWORKSPACE
        assert untouched()
    assert lib.lc_last_error().decode().startswith("lc_ctc_loss_entropy: workspace too small")
    assert raw(**dict(good, lo=None, hi=None, grad=None)) == 0                  # both windows NULL, no gradient
    assert not bool(torch.isnan(loss).any()) and not bool(torch.isnan(entropy).any()) and bool(torch.isnan(grad).all())
    assert raw(**dict(good, eta=-0.5)) == 0                                     # any finite weight
    assert not bool(torch.isnan(grad).any())


def test_ops_refuses_cpu_tensors_and_bad_arguments():
    from lstm_ctc_amd import _lib, ops
    rng = np.random.RandomState(9)
    case = Case(rng, 10, feasible_utts(rng, 10, 3, slack=(0, 2), empty=False))
    cpu = [torch.from_numpy(a) for a in (case.x, case.flat, case.offs, case.seq)]
    with pytest.raises(_lib.LibraryError, match="GPU tensors"):
        ops.ctc_loss_entropy(*cpu, case.maxlen, 0.1)
    dev = [t.cuda() for t in cpu]
    with pytest.raises(ValueError, match="both or none"):
        ops.ctc_loss_entropy(*dev, case.maxlen, 0.1, win_lo=_dev(case.lo, np.int32))
    with pytest.raises(ValueError, match="finite"):
        ops.ctc_loss_entropy(*dev, case.maxlen, float("nan"))
    loss, entropy, grad = ops.ctc_loss_entropy(*dev, case.maxlen, 0.1, want_grad=False)
    assert grad is None and bool(torch.isfinite(loss).all()) and bool((entropy >= 0).all())


def test_uniform_logits_give_the_log_of_the_path_count():
    """All-equal logits: H = ln N, N counted by the host test's integer dynamic programme.  The emission error cancels
    (every path has the same probability, whatever the fp32 log-softmax gives)."""
    rng = np.random.RandomState(10)
    T, L, V = 40, 10, 8
    utts = []
    for b in range(4):
        labels = rng.randint(0, V - 1, L - b)
        labels[4] = labels[3]                                                    # a repeated pair
        lo, hi = (np.arange(L - b) * 3, np.arange(L - b) * 3 + 12) if b % 2 else (np.zeros(L - b), np.full(L - b, OPEN))
        utts.append((T - 2 * b, labels, lo, hi))
    case = make_case(rng, V, utts, True, T=T)
    case.x[:] = -1.3
    loss, entropy, grad = call(case, 1.0)
    for b, (Tb, labels, lo, hi) in enumerate(utts):
        N = count_paths(Tb, labels, lo, hi)
        assert N > 1000
        assert abs(float(entropy[b]) - np.log(N)) <= BAR * np.log(N), (b, entropy[b], np.log(N))
        assert abs(float(loss[b]) - (Tb * np.log(V) - np.log(N))) <= BAR * float(loss[b])
    check_against_reference(case, 1.0, loss, entropy, grad, "uniform")


# ----------------------------------------------------------------------------------------------- the graph
ETA = 0.3


def _reference_on_logits(logits, batch, eta, V, lo=None, hi=None):
    """(sum of loss - eta H, sum of H, sum of the frames, d criterion / d logits [B,T,V]) of the float64 reference."""
    from lstm_ctc_amd.nnet.graph import flatten_labels
    flat, offs, _ = flatten_labels(batch["nnet_target"])
    seq = batch["sequence_length"]
    total = entropy = 0.0
    grad = np.zeros(logits.shape)
    for b in range(len(seq)):
        win = (None, None) if lo is None else (lo[offs[b]:offs[b + 1]], hi[offs[b]:offs[b + 1]])
        ref = entropy_ctc_ref(logits[b, :seq[b]].astype(np.float64), flat[offs[b]:offs[b + 1]], eta, V - 1, *win)
        total += ref["loss"] - eta * ref["entropy"]
        entropy += ref["entropy"]
        grad[b, :seq[b]] = ref["grad"]
    return total, entropy, int(np.sum(seq)), grad


def test_graph_training_step_with_entropy_weight(monkeypatch):
    from lstm_ctc_amd import ops
    from lstm_ctc_amd.nnet.graph import CTCGraph
    seen = {}

    def spy(*a, _fn=ops.ctc_loss_entropy, **kw):
        res = _fn(*a, **kw)
        seen["grad"] = res[2].clone()
        return res
    monkeypatch.setattr(ops, "ctc_loss_entropy", spy)
    batch = _smoke_batch()
    V = SMOKE_CFG["num_targets"]
    graph = CTCGraph(None, SMOKE_CFG, learn_rate=1e-3, l2_decay_weight=0.0, seed=1, entropy_weight=ETA)
    before = graph.model.ps.flat.clone()
    out = graph.step(batch, fetch_eval=True, fetch_logits=True)
    total, entropy, frames, grad = _reference_on_logits(out["logits"], batch, ETA, V)
    assert abs(out["eval_loss"] - total) <= BAR * max(abs(total), 1.0), (out["eval_loss"], total)
    assert abs(out["path_entropy"] - entropy) <= BAR * max(abs(entropy), 1.0), (out["path_entropy"], entropy)
    assert out["path_entropy_frames"] == frames and "decoded" in out and entropy > 1.0
    check_grad(seen["grad"].permute(1, 0, 2).cpu().numpy(), grad, "graph entropy_weight", "logits gradient")
    plain, _, _, _ = _reference_on_logits(out["logits"], batch, 0.0, V)
    assert total < plain - 1e-3                                      # the term bites on this batch
    assert not torch.equal(before, graph.model.ps.flat) and np.isfinite(out["grad_norm"])
    out2 = graph.step(batch)
    assert graph.path_entropy_frames_total == 2 * frames
    assert abs(graph.path_entropy_total - (out["path_entropy"] + out2["path_entropy"])) <= 1e-9 * graph.path_entropy_total


def test_graph_without_entropy_weight_is_untouched(monkeypatch):
    """entropy_weight=None runs the old ops and never the new one (counted), and trains bit-identically to a graph built
    without the keyword."""
    from lstm_ctc_amd import ops
    from lstm_ctc_amd.nnet.graph import create_graph_for_training_ctc
    calls = {"ctc_loss": 0, "ctc_loss_windowed": 0, "ctc_loss_delay": 0, "ctc_loss_entropy": 0}
    for name in calls:
        def counted(*a, _name=name, _fn=getattr(ops, name), **kw):
            calls[_name] += 1
            return _fn(*a, **kw)
        monkeypatch.setattr(ops, name, counted)
    batch = _smoke_batch()
    outs = []
    for kw in (dict(), dict(entropy_weight=None)):
        graph = create_graph_for_training_ctc(None, SMOKE_CFG, learn_rate=1e-2, seed=1, **kw)
        assert graph.entropy_weight is None
        steps = [graph.step(batch, fetch_eval=True) for _ in range(2)]
        assert all("path_entropy" not in s and "path_entropy_frames" not in s for s in steps)
        outs.append(([s["eval_loss"] for s in steps], [s["grad_norm"] for s in steps], graph.model.ps.flat.clone()))
        assert (graph.path_entropy_total, graph.path_entropy_frames_total) == (0.0, 0)
    assert outs[0][0] == outs[1][0] and outs[0][1] == outs[1][1] and torch.equal(outs[0][2], outs[1][2])
    plain_calls = calls["ctc_loss"]
    assert plain_calls >= 4 and calls["ctc_loss_entropy"] == 0 and calls["ctc_loss_windowed"] == 0
    create_graph_for_training_ctc(None, SMOKE_CFG, learn_rate=1e-2, seed=1, delay_penalty=0.1).step(batch)
    assert calls["ctc_loss_delay"] >= 1 and calls["ctc_loss_entropy"] == 0
    # eta = 0 is the new op, and plain CTC's value
    zero = create_graph_for_training_ctc(None, SMOKE_CFG, learn_rate=1e-2, seed=1, entropy_weight=0).step(batch)
    assert calls["ctc_loss_entropy"] >= 1 and calls["ctc_loss"] == plain_calls
    assert abs(zero["eval_loss"] - outs[0][0][0]) <= BAR * max(abs(outs[0][0][0]), 1.0) and zero["path_entropy"] > 0


def test_graph_entropy_weight_composes_with_align_window():
    from lstm_ctc_amd import ops
    from lstm_ctc_amd.nnet.graph import create_graph_for_validation_ctc, flatten_labels
    batch = _smoke_batch()
    V, tau = SMOKE_CFG["num_targets"], 1
    graph = create_graph_for_validation_ctc(None, SMOKE_CFG, seed=1, align_window=tau, entropy_weight=ETA)
    ali = graph.align(batch)["ali"]
    out = graph.step(None, staged=graph.stage(dict(batch, frame_target=ali)), fetch_logits=True)      # the prefetch path
    flat, offs, _ = flatten_labels(batch["nnet_target"])
    lo, hi, ok = ops.label_windows(ali, flat, offs, batch["sequence_length"], tau, V - 1)
    assert ok.all() and (graph.windows_constrained, graph.windows_unconstrained) == (4, 0)
    total, entropy, frames, _ = _reference_on_logits(out["logits"], batch, ETA, V, lo, hi)
    _, open_entropy, _, _ = _reference_on_logits(out["logits"], batch, ETA, V)
    assert abs(entropy - open_entropy) > 1e-3                        # the windows reach the entropy
    assert abs(out["eval_loss"] - total) <= BAR * max(abs(total), 1.0), (out["eval_loss"], total)
    assert abs(out["path_entropy"] - entropy) <= BAR * max(abs(entropy), 1.0), (out["path_entropy"], entropy)
    assert out["path_entropy_frames"] == frames


# ----------------------------------------------------------------------------------------------- command lines
def _run(cli, *args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", cli)] + list(args), capture_output=True, timeout=300)
    return r.returncode, r.stderr.decode()


def _logged(err, name):
    lines = [l for l in err.split("\n") if l.startswith("INFO:tensorflow:%s = " % name)]
    assert len(lines) == 1, err
    return float(lines[0].split()[-1])


def _entropy_line(err):
    """(weight, nats per frame, frames) of the one 'entropy weight' INFO line."""
    lines = [l for l in err.split("\n") if l.startswith("INFO:tensorflow:entropy weight ")]
    assert len(lines) == 1, err
    m = re.fullmatch(r"INFO:tensorflow:entropy weight (\S+): mean path entropy (\S+) nats per frame over (\d+) frame\(s\)", lines[0])
    assert m, lines[0]
    return float(m.group(1)), float(m.group(2)), int(m.group(3))


def test_cli_train_and_validate_with_entropy_weight(tmp_path):
    import lstm_ctc_amd.nnet as nnet
    rng = np.random.default_rng(7)
    D, V = 6, 9
    lines, frames = [], 0
    for i, T in enumerate([20, 24, 31, 40]):
        path = str(tmp_path / ("utt%03d.tfrecords" % i))
        target = rng.integers(0, V - 1, size=int(rng.integers(1, 5)))
        frames += T // 2                                                          # subsample = 2
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
                   "--shuffle=false", "--entropy-weight", "0.2", str(scp), str(config), d + "/nnet.0", d + "/nnet.1")
    assert rc == 0, err
    weight, nats, n = _entropy_line(err)
    assert weight == 0.2 and abs(n - frames) <= 4 and 0.0 < nats < np.log(V), err      # a frame holds at most ln V nats
    assert np.isfinite(_logged(err, "tr_loss")) and os.path.getsize(d + "/nnet.1") > 0
    val = ["--objective=ctc", "--batch-size", "2", str(scp), str(config), d + "/nnet.1"]
    rc, err = _run("nnet-validate.py", *val)
    assert rc == 0, err
    plain = _logged(err, "cv_loss")
    assert "entropy weight" not in err
    rc, err = _run("nnet-validate.py", "--entropy-weight", "0", *val)          # plain CTC plus the metric
    assert rc == 0, err
    assert abs(_logged(err, "cv_loss") - plain) <= 1e-4 * abs(plain), (err, plain)
    weight0, nats0, n0 = _entropy_line(err)
    assert weight0 == 0.0 and n0 == n and 0.0 < nats0 < np.log(V)
    rc, err = _run("nnet-validate.py", "--entropy-weight", "0.5", *val)
    assert rc == 0, err
    assert _logged(err, "cv_loss") < plain                                       # the criterion is loss - eta H, H > 0
    assert abs(_entropy_line(err)[1] - nats0) <= 1e-6 * nats0                    # and H itself does not depend on eta


def test_zz_report_measured_error_over_bar():
    text = ("ctc_entropy: largest measured error / project bar (GRAD_TOL = %g) over %d utterances with a path: loss %.4f, "
            "entropy %.4f (against the tighter bar GRAD_TOL max(|H_ref|, 1): %.4f), grad %.4f"
            % (BAR, MEASURED["n"], MEASURED["loss"], MEASURED["entropy"], MEASURED["entropy_tight"], MEASURED["grad"]))
    print("\n" + text)
    out = os.environ.get("LC_MEASURED_DIR")              # where to keep the line; unset: printed only
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "ctc_entropy_measured.txt"), "w") as f:
            f.write(text + "\n")
    assert MEASURED["loss"] <= 1.0 and MEASURED["entropy_tight"] <= 1.0 and MEASURED["grad"] <= 1.0
