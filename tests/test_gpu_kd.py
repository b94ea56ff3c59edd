"""lc_kd_loss (teacher-student distillation) on the GPU: the op, the graph's teacher term / kd objective and the command lines.

Reference: float64 numpy (``kd_ref``; torch float64 on the device for the one case too large for the host); for the model,
the oracle's forward / CTC / backward / l2_and_clip / apply_optimizer composed around that reference.

Tolerances - derived from the kernel's arithmetic, not from what it was seen to give (u = 2^-24, fp32 unit round-off).  Per
scored frame, s the teacher row, z the student row, the kernel forms (csrc/kd.hip)
    a_k = fl(s_k - max s), b_k = fl(z_k - max z), ep_k = exp2(fl(a_k c)), eq_k = exp2(fl(b_k c)), c = fl(log2e fl(1 / tau)),
    Sp = sum ep, Sq = sum eq, A = sum_{ep_k > 0} ep_k fl(a_k - b_k),  KL = A fl(1 / tau) rcp(Sp) + (log2 Sq - log2 Sp) ln2.
Write alpha_k = a_k / tau, beta_k = b_k / tau (the natural exponents), p = ep / Sp, q = eq / Sq.

* An exponential: the argument carries u (difference) + 3u (c: reciprocal, constant, product) + u (product) = 5u relative,
  which exp2 turns into a relative 5u |alpha_k|; the hardware exp2 adds 1 ulp.  ep_k |alpha_k| <= 1 / e, so a term of Sp is
  off by <= (5 / e) u + u ep_k <= 1.84u + u ep_k, V terms: (1.84 V + 1) u Sp (Sp >= 1).  The terms are added in fp32 in a
  fixed order, at most NADD(V) = ceil(V / 64) + 16 additions deep in every kernel variant (V <= 64: 4 + 4; V <= 1024:
  4 / 8 / 16 + 6; wider: <= V / 64 + 2 + 6):
      E_S(V) = 1.84 V + 1 + NADD(V)          relative error of Sp and of Sq, in units of u.
* L = (log2 Sq - log2 Sp) ln2: E_S u from each sum, 1 ulp of the hardware log2 each (u ln V), the subtraction (u ln V at
  most), the constant and the product (1.5u ln V): <= (2 E_S + 4.5 ln V) u.
* A / (tau Sp): a term ep_k fl(a_k - b_k) carries the exponential's (5 |alpha_k| + 1) u, the product's u, and the
  difference's 2u (|a_k| + |b_k|) (two rounded operands, one rounded result); the additions NADD u sum |term|; then fl(1 /
  tau), two products, the hardware reciprocal and Sp's own error: (4 + E_S) u relative.  With, from the reference,
      Aabs = sum_k p_k |alpha_k - beta_k|,   W = sum_k p_k (|alpha_k - beta_k| (5 |alpha_k| + 2) + 2 (|alpha_k| + |beta_k|)):
      <= u (W + (NADD + E_S + 4) Aabs).
* The frame's term adds the two parts (<= u (Aabs + |L|)); the fold adds an utterance's terms as doubles (2^-53 each -
  nothing at these sizes) and rounds the sum once (u |loss|):
      eps_frame = u (W + (NADD(V) + E_S(V) + 5) Aabs + 2 E_S(V) + 4.5 ln V + |L|)
      tol_loss[b] = sum over the scored frames of eps_frame + u |loss_b|.
* Gradient element grad_scale (eq_k / Sq - ep_k / Sp): each quotient carries the exponential's (5 |alpha_k| + 1) u, the sum's
  E_S u, the hardware reciprocal, the product with grad_scale and the product with the exponential (3u); p_k <= 1 and p_k
  |alpha_k| <= 1 / e; the difference rounds once (<= u):
      tol_grad = |grad_scale| u (2 (E_S(V) + 4 + 5 / e) + 1) <= |grad_scale| u (2 E_S(V) + 13)       absolute, per element;
  accumulating into G adds one rounding of the sum: + u |G + g|.
* Both are asserted TOGETHER with the project's bar (tests/conftest.py): 1e-4 max(|ref|, 1) for a loss, check_grad /
  GRAD_TOL for a gradient tensor.  frames and agree are integers and compared exactly; the inputs are drawn so that no row
  has two equal maxima (asserted on the reference) except in the tie test.
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import check_grad

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
BAR = 1e-4                         # tests/conftest.py: GRAD_TOL, the project's bar for logits and loss
LC_EINVAL, LC_EWORKSPACE = -1, -3
MEASURED = {"loss": 0.0, "grad": 0.0, "loss_bar": 0.0}     # largest measured error / bound (printed by the last test)


# ----------------------------------------------------------------------------------------------- reference and bounds
def nadd(V):
    return math.ceil(V / 64) + 16


def e_s(V):
    return 1.84 * V + 1 + nadd(V)


def tol_grad(V, scale):
    return abs(scale) * U * (2 * e_s(V) + 13)


def kd_ref(logits, teacher, seq, tlen, tau=1.0):
    """float64 reference.  logits, teacher [T,B,V], seq, tlen [B] -> dict(loss [B], frames, agree, grad [T,B,V] = q - p (not
    scaled), eps [B] = sum of eps_frame / u over the scored frames, scored [T,B] (bad rows excluded), bad [T,B])."""
    z, s = np.asarray(logits, np.float64), np.asarray(teacher, np.float64)
    T, B, V = z.shape
    live = (np.arange(T)[:, None] < np.asarray(seq)[None, :]) & (np.arange(T)[:, None] < np.asarray(tlen)[None, :])
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ms, mz = s.max(axis=-1, keepdims=True), z.max(axis=-1, keepdims=True)
        bad = live & ~(np.isfinite(ms[..., 0]) & ~np.isnan(s).any(axis=-1))
        scored = live & ~bad
        al, be = (s - ms) / tau, (z - mz) / tau
        ep, eq = np.exp(al), np.exp(be)
        sp, sq = ep.sum(axis=-1, keepdims=True), eq.sum(axis=-1, keepdims=True)
        p, q = ep / sp, eq / sq
        pos = p > 0
        d = np.where(pos, al - be, 0.0)
        lterm = (np.log(sq) - np.log(sp))[..., 0]
        kl = np.where(pos, p * d, 0.0).sum(axis=-1) + lterm
        aabs = np.where(pos, p * np.abs(d), 0.0).sum(axis=-1)
        w = np.where(pos, p * (np.abs(d) * (5 * np.abs(al) + 2) + 2 * (np.abs(al) + np.abs(be))), 0.0).sum(axis=-1)
        eps = w + (nadd(V) + e_s(V) + 5) * aabs + 2 * e_s(V) + 4.5 * math.log(V) + np.abs(lterm)
    kl = np.where(scored, kl, 0.0)
    eps = np.where(scored, eps, 0.0)
    grad = np.where(scored[..., None], q - p, 0.0)
    loss = kl.sum(axis=0)
    loss[bad.any(axis=0)] = np.nan
    keep = scored[..., None]
    same = np.where(keep, s, 0.0).argmax(axis=-1) == np.where(keep, z, 0.0).argmax(axis=-1)          # numpy: the first maximum
    return dict(loss=loss, frames=scored.sum(axis=0), agree=(scored & same).sum(axis=0), grad=grad, eps=eps.sum(axis=0),
                scored=scored, bad=bad)


def assert_unique_maxima(x):
    x = np.asarray(x)
    top2 = np.partition(x, -2, axis=-1)[..., -2:]
    assert (top2[..., 0] < top2[..., 1]).all(), "test input has a row with two equal maxima"


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def run_kd(logits, teacher, seq, tlen, tau=1.0, scale=1.0, want_grad=True, into=None):
    from lstm_ctc_amd import ops
    grad_in = None if into is None else _dev(into, np.float32)
    loss, frames, agree, grad = ops.kd_loss(_dev(logits, np.float32), _dev(teacher, np.float32), _dev(seq, np.int32),
                                            _dev(tlen, np.int32), temperature=tau, grad_scale=scale, grad=grad_in,
                                            want_grad=want_grad)
    torch.cuda.synchronize()
    return (loss.cpu().numpy(), frames.cpu().numpy(), agree.cpu().numpy(), None if grad is None else grad.cpu().numpy())


def check_loss(loss, ref, tag, extra=None):
    for b in range(len(loss)):
        r = ref["loss"][b]
        if not np.isfinite(r):
            assert (np.isnan(loss[b]) and np.isnan(r)) or loss[b] == r, (tag, b, loss[b], r)
            continue
        tol = U * (ref["eps"][b] + abs(r)) + (0.0 if extra is None else extra[b])
        bar = BAR * max(abs(r), 1.0)
        err = abs(float(loss[b]) - r)
        if tol > 0:
            MEASURED["loss"] = max(MEASURED["loss"], err / tol)
        MEASURED["loss_bar"] = max(MEASURED["loss_bar"], err / bar)
        assert err <= tol and err <= bar, (tag, b, err, tol, bar)


def check_against_ref(logits, teacher, seq, tlen, tau, scale, got, tag, into=None):
    loss, frames, agree, grad = got
    T, B, V = logits.shape
    ref = kd_ref(logits, teacher, seq, tlen, tau)
    assert np.array_equal(frames, ref["frames"]), (tag, frames, ref["frames"])
    assert np.array_equal(agree, ref["agree"]), (tag, agree, ref["agree"])
    check_loss(loss, ref, tag)
    if grad is not None:
        g = scale * ref["grad"]
        tol = np.full(g.shape, tol_grad(V, scale))
        if into is not None:
            g = g + np.asarray(into, np.float64)
            tol = tol + U * np.abs(g)
        assert np.isfinite(grad).all(), tag
        ratio = float((np.abs(grad - g) / tol).max())
        MEASURED["grad"] = max(MEASURED["grad"], ratio)
        assert ratio <= 1.0, (tag, ratio)
        check_grad(grad, g, tag, "dlogits")
        rest = ~ref["scored"]
        if into is None:
            assert not grad[rest].any() and not np.signbit(grad[rest]).any(), tag                    # exactly +0
        else:
            assert grad[rest].tobytes() == np.asarray(into, np.float32)[rest].tobytes(), tag         # left bit-exactly
    return ref


def make_case(rng, T, B, V, seq, scale=3.0, drop=None):
    """Student logits, teacher log-posteriors (their own random rows), lengths; ``drop``: the utterance (with frames) whose
    teacher_len is 0 - the first such utterance by default."""
    logits = (rng.standard_normal((T, B, V)) * scale).astype(np.float32)
    t = rng.standard_normal((T, B, V)) * scale
    teacher = (t - np.log(np.exp(t).sum(axis=-1, keepdims=True))).astype(np.float32)
    seq = np.asarray(seq, np.int32)
    tlen = seq.copy()
    if drop is None and B > 1:
        drop = int(np.flatnonzero(seq > 0)[0])
    if drop is not None:
        tlen[drop] = 0
    for b in range(B):
        if b != drop and seq[b] >= 4:
            tlen[b] = seq[b] - 1 if b % 2 else min(T, seq[b] + 1)       # shorter and longer than the utterance
    assert_unique_maxima(logits)
    assert_unique_maxima(teacher)
    return logits, teacher, seq, tlen


# ----------------------------------------------------------------------------------------------- 1. the op at the edges
EDGE_V = [2, 3, 16, 17, 44, 63, 64, 65, 128, 129, 255, 256, 257, 1024, 1025, 4099]
EDGE_SHAPES = [(5, 3, [5, 4, 1]), (5, 3, [0, 5, 4]), (1, 1, [1]), (37, 5, [37, 36, 1, 0, 20])]


@pytest.mark.parametrize("V", EDGE_V)
def test_op_matches_reference_at_lane_split_edges(V):
    rng = np.random.default_rng(2000 + V)
    for (T, B, seq), tau in zip(EDGE_SHAPES * 2, [1.0, 2.0, 0.5, 1.0, 0.5, 1.0, 2.0, 2.0]):
        logits, teacher, seq, tlen = make_case(rng, T, B, V, seq)
        if B > 1:
            assert ((tlen == 0) & (seq > 0)).sum() == 1
        scale = 0.5 * tau
        got = run_kd(logits, teacher, seq, tlen, tau, scale)
        ref = check_against_ref(logits, teacher, seq, tlen, tau, scale, got, ("edge", V, T, B, tau))
        assert ref["frames"].sum() > 0
        nograd = run_kd(logits, teacher, seq, tlen, tau, scale, want_grad=False)
        assert nograd[3] is None
        for a, b_ in zip(got[:3], nograd[:3]):                            # the same bits with and without a gradient
            assert a.tobytes() == b_.tobytes()


# ----------------------------------------------------------------------------------------------- raw calls
def raw_call(logits, teacher, seq, tlen, T, B, V, tau, scale, loss, frames, agree, grad, acc, ws, ws_bytes):
    from lstm_ctc_amd import _lib, ops
    lib = _lib.load()
    rc = lib.lc_kd_loss(ops._ptr(logits), ops._ptr(teacher), T, B, V, ops._ptr(seq), ops._ptr(tlen), tau, scale,
                        ops._ptr(loss), ops._ptr(frames), ops._ptr(agree), ops._ptr(grad), acc, ops._ptr(ws), ws_bytes,
                        ops._stream())
    torch.cuda.synchronize()
    return rc


def _prefilled(T, B, V):
    return (torch.full((B,), float("nan"), device="cuda"), torch.full((B,), -77, dtype=torch.int32, device="cuda"),
            torch.full((B,), -77, dtype=torch.int32, device="cuda"), torch.full((T, B, V), float("nan"), device="cuda"))


@pytest.mark.parametrize("V", [4, 44, 45, 300, 1030])
def test_accumulate_and_overwrite(V):
    from lstm_ctc_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(V)
    T, B, tau, scale = 9, 6, 2.0, 0.7
    logits, teacher, seq, tlen = make_case(rng, T, B, V, [9, 0, 5, 9, 3, 7], drop=3)
    ref = kd_ref(logits, teacher, seq, tlen, tau)
    assert ref["frames"][1] == ref["frames"][3] == 0 and ref["frames"].sum() > 0
    # accumulate: scored rows G + scale (q - p), every other row G to the bit - NaN rows among them: they are not read
    G = rng.standard_normal((T, B, V)).astype(np.float32)
    got = run_kd(logits, teacher, seq, tlen, tau, scale, into=G)
    check_against_ref(logits, teacher, seq, tlen, tau, scale, got, ("accumulate", V), into=G)
    Gn = G.copy()
    Gn[~ref["scored"]] = np.nan
    got_n = run_kd(logits, teacher, seq, tlen, tau, scale, into=Gn)
    assert np.isnan(got_n[3][~ref["scored"]]).all() and np.array_equal(got_n[3][ref["scored"]], got[3][ref["scored"]])
    assert got_n[0].tobytes() == got[0].tobytes()
    # overwrite on NaN-prefilled outputs and a dirty workspace: every element written, rows that are not scored exactly +0
    ld, td, sd, tl = _dev(logits, np.float32), _dev(teacher, np.float32), _dev(seq, np.int32), _dev(tlen, np.int32)
    nbytes = lib.lc_kd_workspace_bytes(T, B, V)
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
    for with_grad in (True, False):
        loss, frames, agree, grad = _prefilled(T, B, V)
        assert raw_call(ld, td, sd, tl, T, B, V, tau, scale, loss, frames, agree, grad if with_grad else None, 0, ws, nbytes) == 0
        l, f, c, g = loss.cpu().numpy(), frames.cpu().numpy(), agree.cpu().numpy(), grad.cpu().numpy()
        assert not np.isnan(l).any() and (f != -77).all() and (c != -77).all()
        for b in (1, 3):                                                  # no scored frame: loss 0 and counts 0
            assert l[b] == 0.0 and not np.signbit(l[b]) and f[b] == 0 and c[b] == 0
        if with_grad:
            assert not np.isnan(g).any()
            check_against_ref(logits, teacher, seq, tlen, tau, scale, (l, f, c, g), ("written", V))
        else:
            assert np.isnan(g).all()                                      # grad = NULL: not touched
            check_against_ref(logits, teacher, seq, tlen, tau, scale, (l, f, c, None), ("written-nograd", V))
            assert l.tobytes() == got[0].tobytes()                        # and the same bits as with a gradient


@pytest.mark.parametrize("T,B,V", [(50, 7, 44), (50, 7, 300), (20, 7, 4099)])
def test_two_calls_are_bit_identical(T, B, V):
    rng = np.random.default_rng(5)
    logits, teacher, seq, tlen = make_case(rng, T, B, V, rng.integers(0, T + 1, size=B))
    a, b_ = run_kd(logits, teacher, seq, tlen, 2.0, 1.5), run_kd(logits, teacher, seq, tlen, 2.0, 1.5)
    for x, y in zip(a, b_):
        assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("V", [44, 300, 1028, 1031])
def test_buffers_off_the_16_byte_boundary_take_the_unaligned_path(V):
    """All three buffers start 4 bytes behind a 16-byte boundary (views into larger buffers): within the tolerances of the
    reference, overwriting and accumulating."""
    from lstm_ctc_amd import ops
    rng = np.random.default_rng(V)
    T, B, tau, scale = 11, 3, 0.5, 0.25
    logits, teacher, seq, tlen = make_case(rng, T, B, V, [11, 10, 4], drop=2)

    def off(a):
        buf = torch.zeros(T * B * V + 1, device="cuda")
        view = buf[1:].view(T, B, V)
        view.copy_(_dev(a, np.float32))
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        return view

    G = rng.standard_normal((T, B, V)).astype(np.float32)
    for into in (None, G):
        for lg, tc in ((off(logits), off(teacher)), (off(logits), _dev(teacher, np.float32))):     # all, or one buffer only
            g_in = None if into is None else off(into)
            loss, frames, agree, grad = ops.kd_loss(lg, tc, _dev(seq, np.int32), _dev(tlen, np.int32), temperature=tau,
                                                    grad_scale=scale, grad=g_in)
            torch.cuda.synchronize()
            got = (loss.cpu().numpy(), frames.cpu().numpy(), agree.cpu().numpy(), grad.cpu().numpy())
            check_against_ref(logits, teacher, seq, tlen, tau, scale, got, ("unaligned", V), into=into)


# ----------------------------------------------------------------------------------------------- 4. anchors without kd_ref
@pytest.mark.parametrize("V", [7, 44, 300, 1100])
def test_anchor_teacher_equal_to_student(V):
    rng = np.random.default_rng(V)
    T, B = 8, 3
    logits, _, seq, _ = make_case(rng, T, B, V, [8, 5, 8])
    for tau in (1.0, 2.0):
        loss, frames, agree, grad = run_kd(logits, logits, seq, seq, tau, tau)
        assert np.array_equal(frames, seq) and np.array_equal(agree, frames)
        # eps_frame with W = Aabs = L = 0: the two sums' errors and the logarithms
        tol = frames * U * (2 * e_s(V) + 4.5 * math.log(V))
        assert (np.abs(loss) <= tol).all(), (loss, tol)
        assert np.abs(grad).max() <= tol_grad(V, tau)


@pytest.mark.parametrize("V", [7, 44, 300, 1100])
def test_anchor_one_hot_teacher_is_cross_entropy(V):
    """A teacher row of 0 at one class and -inf elsewhere at tau = 1 is the frame cross-entropy: loss, gradient and agree
    against ops.xent_loss on the same logits, within the sum of both derived bounds."""
    from lstm_ctc_amd import ops
    from test_gpu_xent import eps_lse, tol_grad as xent_tol_grad
    rng = np.random.default_rng(V)
    T, B = 8, 3
    logits, _, seq, _ = make_case(rng, T, B, V, [8, 5, 8])
    targets = rng.integers(0, V, size=(B, T)).astype(np.int32)
    teacher = np.full((T, B, V), -np.inf, np.float32)
    np.put_along_axis(teacher, targets.T[..., None].astype(np.int64), 0.0, axis=-1)
    loss, frames, agree, grad = run_kd(logits, teacher, seq, seq, 1.0, 1.0)
    xl, xf, xc, xg = ops.xent_loss(_dev(logits, np.float32), _dev(targets, np.int32), _dev(seq, np.int32))
    xl, xf, xc, xg = xl.cpu().numpy(), xf.cpu().numpy(), xc.cpu().numpy(), xg.cpu().numpy()
    assert np.array_equal(frames, xf) and np.array_equal(agree, xc)
    assert np.isfinite(grad).all() and np.isfinite(loss).all()
    # the bounds of either side from its own derivation; the terms' sizes from the kernels' own results (|term| = term >= 0)
    z = logits.astype(np.float64)
    maxabs = float(np.abs(logits).max())
    live = np.arange(T)[:, None] < seq[None, :]
    beta = np.take_along_axis(z, targets.T[..., None].astype(np.int64), axis=-1)[..., 0] - z.max(axis=-1)     # <= 0
    lse = np.log(np.exp(z - z.max(axis=-1, keepdims=True)).sum(axis=-1))
    aabs = np.abs(beta)
    eps_kd = (2 * aabs + 2 * aabs) + (nadd(V) + e_s(V) + 5) * aabs + 2 * e_s(V) + 4.5 * math.log(V) + lse       # W: alpha = 0
    for b in range(B):
        tol_kd = U * ((eps_kd[:, b] * live[:, b]).sum() + abs(float(loss[b])))
        tol_xe = frames[b] * eps_lse(V, maxabs) + 2 * U * abs(float(xl[b])) + U * abs(float(xl[b]))
        assert abs(float(loss[b]) - float(xl[b])) <= tol_kd + tol_xe, (b, loss[b], xl[b], tol_kd, tol_xe)
    assert np.abs(grad - xg).max() <= tol_grad(V, 1.0) + xent_tol_grad(V)


@pytest.mark.parametrize("V", [44, 1100])
def test_anchor_teacher_shift_is_immaterial(V):
    rng = np.random.default_rng(V)
    T, B = 8, 3
    logits, teacher, seq, tlen = make_case(rng, T, B, V, [8, 5, 8], drop=1)
    shift = rng.uniform(-20, 20, size=(T, B, 1)).astype(np.float32)
    a = run_kd(logits, teacher, seq, tlen, 2.0, 1.0)
    b_ = run_kd(logits, teacher + shift, seq, tlen, 2.0, 1.0)
    ref = kd_ref(logits, teacher, seq, tlen, 2.0)
    assert np.array_equal(a[1], b_[1]) and np.array_equal(a[2], b_[2])
    for b in range(B):                                                    # either call within its bound of the reference
        assert abs(float(a[0][b]) - float(b_[0][b])) <= 2 * U * (ref["eps"][b] + abs(ref["loss"][b])) + 1e-30
    assert np.abs(a[3] - b_[3]).max() <= 2 * tol_grad(V, 1.0)


# ----------------------------------------------------------------------------------------------- 5. special values
@pytest.mark.parametrize("V", [5, 44, 300, 1100])
def test_special_values(V):
    rng = np.random.default_rng(V)
    T, B, scale = 6, 4, 0.5
    logits, teacher, seq, tlen = make_case(rng, T, B, V, [6, 6, 6, 6], drop=3)
    tlen[:] = 6
    teacher[2, 0, 1] = -np.inf                        # probability 0 inside a finite row
    teacher[3, 0, :] = -np.inf
    teacher[3, 0, 2] = -1.5                           # a one-class row
    logits[3, 1, 2] = -np.inf                         # a student -inf ...
    teacher[3, 1, 2] = -0.25                          # ... under p_k > 0
    assert_unique_maxima(teacher)
    got = run_kd(logits, teacher, seq, tlen, 1.0, scale)
    loss, frames, agree, grad = got
    ref = check_against_ref(logits, teacher, seq, tlen, 1.0, scale, got, ("special", V))
    assert np.isfinite(loss[0]) and not np.isnan(grad).any()
    q = scale * np.exp(logits[2, 0].astype(np.float64) - np.log(np.exp(logits[2, 0].astype(np.float64)).sum()))
    assert abs(grad[2, 0, 1] - q[1]) <= tol_grad(V, scale)                # p = 0 there: the gradient is scale * q
    assert loss[1] == np.inf and np.isfinite(grad[3, 1]).all() and ref["loss"][1] == np.inf
    assert np.isfinite(loss[2]) and np.isfinite(loss[3])
    # bad teacher rows: NaN for that utterance only; the frame counts nowhere and its gradient row is zero / untouched
    logits, teacher, seq, tlen = make_case(rng, T, B, V, [6, 6, 5, 6], drop=3)
    tlen[:] = seq
    clean = run_kd(logits, teacher, seq, tlen, 2.0, scale)
    G = rng.standard_normal((T, B, V)).astype(np.float32)
    clean_acc = run_kd(logits, teacher, seq, tlen, 2.0, scale, into=G)
    for kind, b in (("all -inf", 1), ("nan", 2), ("+inf", 0), ("nan at the maximum", 1)):
        t2 = teacher.copy()
        if kind == "all -inf":
            t2[3, b, :] = -np.inf
        elif kind == "nan":
            t2[3, b, V - 1] = np.nan
        elif kind == "+inf":
            t2[3, b, V // 2] = np.inf
        else:
            t2[3, b, int(teacher[3, b].argmax())] = np.nan
        loss, frames, agree, grad = run_kd(logits, t2, seq, tlen, 2.0, scale)
        assert np.isnan(loss[b]) and frames[b] == clean[1][b] - 1, kind
        assert not grad[3, b].any(), kind
        for o in range(B):
            if o != b:                                # the neighbours are intact, to the bit
                assert loss[o] == clean[0][o] and frames[o] == clean[1][o] and agree[o] == clean[2][o], kind
                assert np.array_equal(grad[:, o], clean[3][:, o]), kind
        check_against_ref(logits, t2, seq, tlen, 2.0, scale, (loss, frames, agree, grad), ("bad row", V, kind))
        acc = run_kd(logits, t2, seq, tlen, 2.0, scale, into=G)
        assert acc[3][3, b].tobytes() == G[3, b].tobytes(), kind          # accumulate: the bad frame's row is left alone
        keep = np.ones((T, B), bool)
        keep[3, b] = False
        assert np.array_equal(acc[3][keep], clean_acc[3][keep]), kind
    # a bad row beyond either length is not scored: ignored
    t2 = teacher.copy()
    t2[5, 2, :] = np.nan
    again = run_kd(logits, t2, seq, tlen, 2.0, scale)
    for x, y in zip(again, clean):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("V", [6, 44, 300, 2000])
def test_argmax_tie_goes_to_the_lower_index(V):
    rng = np.random.default_rng(V)
    pairs = [(0, 1), (1, V - 1), (V // 2, V // 2 + 1), (2, min(V - 1, 70))]      # within a lane's span and across lanes
    T = len(pairs)
    seq = np.array([T, T, T, T], np.int32)
    logits = rng.standard_normal((T, 4, V)).astype(np.float32)
    teacher = rng.standard_normal((T, 4, V)).astype(np.float32)
    for t, (lo, hi) in enumerate(pairs):
        logits[t, 0, lo] = logits[t, 0, hi] = 9.5     # utterance 0: the student ties, the teacher peaks on the lower index
        teacher[t, 0, lo] = 9.5
        logits[t, 1, lo] = logits[t, 1, hi] = 9.5     # utterance 1: ... the teacher peaks on the higher one
        teacher[t, 1, hi] = 9.5
        teacher[t, 2, lo] = teacher[t, 2, hi] = 9.5   # utterances 2 and 3: the same with the teacher tying
        logits[t, 2, lo] = 9.5
        teacher[t, 3, lo] = teacher[t, 3, hi] = 9.5
        logits[t, 3, hi] = 9.5
    loss, frames, agree, _ = run_kd(logits, teacher, seq, seq)
    assert frames.tolist() == [T] * 4
    assert agree.tolist() == [T, 0, T, 0]
    ref = kd_ref(logits, teacher, seq, seq)
    assert np.array_equal(agree, ref["agree"])
    assert np.allclose(loss, ref["loss"], rtol=1e-5)


# ----------------------------------------------------------------------------------------------- 6. grid stride, indexing
@pytest.mark.parametrize("T,B,V", [(700, 48, 4), (130, 64, 68), (130, 64, 1028)])
def test_more_frames_than_one_pass_of_the_grid(T, B, V):
    """The launch is capped at 2048 blocks of four waves: 32768 frames per pass at four frames per wave (V <= 64), 8192 at
    one frame per wave.  These shapes need a second pass of the grid-stride loop, with the batch wrapping inside a wave."""
    assert T * B > (32768 if V <= 64 else 8192)
    rng = np.random.default_rng(V)
    seq = rng.integers(T // 2, T + 1, size=B)
    seq[-1] = T
    logits, teacher, seq, tlen = make_case(rng, T, B, V, seq, drop=5)
    tlen[-1] = T
    G = rng.standard_normal((T, B, V)).astype(np.float32)
    check_against_ref(logits, teacher, seq, tlen, 2.0, 1.0, run_kd(logits, teacher, seq, tlen, 2.0, 1.0), ("grid stride", V))
    check_against_ref(logits, teacher, seq, tlen, 2.0, 1.0, run_kd(logits, teacher, seq, tlen, 2.0, 1.0, into=G),
                      ("grid stride acc", V), into=G)


def test_elements_indexed_in_64_bits():
    """T * B * V just above 2^31: 64 sampled frames' gradient rows, every utterance's loss and the counts against torch
    float64 on the device."""
    from lstm_ctc_amd import ops
    T, B, V, tau, scale = 1024, 512, 4099, 2.0, 1.0
    assert T * B * V > 2 ** 31
    free, _ = torch.cuda.mem_get_info()
    if free < 40 * 2 ** 30:
        pytest.skip("needs 40 GB of free device memory")
    gen = torch.Generator(device="cuda").manual_seed(7)
    logits = torch.randn((T, B, V), device="cuda", generator=gen) * 3.0
    teacher = torch.randn((T, B, V), device="cuda", generator=gen) * 3.0
    seq = torch.randint(T // 2, T + 1, (B,), device="cuda", generator=gen, dtype=torch.int32)
    tlen = seq.clone()
    seq[-1] = seq[0] = tlen[-1] = tlen[0] = T
    tlen[7] = 0
    tlen[9] = tlen[9] - 3
    loss, frames, agree, grad = ops.kd_loss(logits, teacher, seq, tlen, temperature=tau, grad_scale=scale)
    torch.cuda.synchronize()
    scored = torch.arange(T, device="cuda")[:, None] < torch.minimum(seq, tlen)[None, :]
    ref_loss = torch.zeros(B, dtype=torch.float64, device="cuda")
    ref_eps = torch.zeros(B, dtype=torch.float64, device="cuda")
    ref_agree = torch.zeros(B, dtype=torch.int64, device="cuda")
    ar = torch.arange(V, device="cuda")
    for t0 in range(0, T, 16):
        z, s, sc = logits[t0:t0 + 16].double(), teacher[t0:t0 + 16].double(), scored[t0:t0 + 16]
        al, be = (s - s.max(-1, keepdim=True).values) / tau, (z - z.max(-1, keepdim=True).values) / tau
        lsp, lsq = torch.logsumexp(al, -1), torch.logsumexp(be, -1)
        p = torch.exp(al - lsp[..., None])
        d = al - be
        aabs = (p * d.abs()).sum(-1)
        w = (p * (d.abs() * (5 * al.abs() + 2) + 2 * (al.abs() + be.abs()))).sum(-1)
        lterm = lsq - lsp
        ref_loss += (((p * d).sum(-1) + lterm) * sc).sum(0)
        ref_eps += ((w + (nadd(V) + e_s(V) + 5) * aabs + 2 * e_s(V) + 4.5 * math.log(V) + lterm.abs()) * sc).sum(0)
        x, y = logits[t0:t0 + 16], teacher[t0:t0 + 16]
        fz = torch.where(x == x.max(-1, keepdim=True).values, ar, V).min(-1).values      # lowest index at the maximum
        fs = torch.where(y == y.max(-1, keepdim=True).values, ar, V).min(-1).values
        ref_agree += (sc & (fz == fs)).sum(0)
        del z, s, al, be, p, d, aabs, w, lterm, fz, fs
    assert torch.equal(frames.long(), scored.sum(0))
    assert torch.equal(agree.long(), ref_agree)
    tol = U * (ref_eps + ref_loss.abs())
    err = (loss.double() - ref_loss).abs()
    MEASURED["loss"] = max(MEASURED["loss"], float((err / tol.clamp(min=1e-300)).max()))
    MEASURED["loss_bar"] = max(MEASURED["loss_bar"], float((err / (BAR * ref_loss.abs().clamp(min=1.0))).max()))
    assert bool((err <= tol).all()) and bool((err <= BAR * ref_loss.abs().clamp(min=1.0)).all())
    # 64 frames, the last ones (the highest addresses) and some that are not scored included
    rng = np.random.default_rng(3)
    frames_s = [(T - 1, B - 1), (T - 1, 0), (T - 2, B - 1), (T - 1, B - 2), (0, 0), (5, 9), (3, 7), (T - 1, 7)]
    frames_s.append((T - 1, int(torch.argmin(seq))))
    while len(frames_s) < 64:
        frames_s.append((int(rng.integers(0, T)), int(rng.integers(0, B))))
    assert (T - 1) * B * V + (B - 1) * V > 2 ** 31
    worst = 0.0
    for t, b in frames_s:
        g = grad[t, b].double()
        if bool(scored[t, b]):
            r = scale * (torch.softmax(logits[t, b].double() / tau, dim=-1) - torch.softmax(teacher[t, b].double() / tau, dim=-1))
            e = float((g - r).abs().max())
            worst = max(worst, e)
            assert e <= tol_grad(V, scale) and e <= BAR * max(float(r.abs().max()), 1e-3), (t, b, e)
        else:
            assert not bool(g.any()), (t, b)
    MEASURED["grad"] = max(MEASURED["grad"], worst / tol_grad(V, scale))


# ----------------------------------------------------------------------------------------------- 7. argument checks
def test_argument_checks_leave_the_outputs_alone():
    from lstm_ctc_amd import _lib
    lib = _lib.load()
    T, B, V = 4, 3, 10
    rng = np.random.default_rng(0)
    logits, teacher, seq, tlen = make_case(rng, T, B, V, [4, 3, 2])
    ld, td, sd, tl = _dev(logits, np.float32), _dev(teacher, np.float32), _dev(seq, np.int32), _dev(tlen, np.int32)
    nbytes = lib.lc_kd_workspace_bytes(T, B, V)
    assert nbytes >= 8 * T * B
    assert lib.lc_kd_workspace_bytes(0, B, V) == 0 and lib.lc_kd_workspace_bytes(T, B, 1) == 0
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    loss, frames, agree, grad = _prefilled(T, B, V)

    def untouched():
        return (bool(torch.isnan(loss).all()) and bool((frames == -77).all()) and bool((agree == -77).all())
                and bool(torch.isnan(grad).all()))

    for kw in (dict(tau=0.0), dict(tau=float("nan")), dict(tau=-1.0), dict(tau=float("inf")), dict(teacher=None),
               dict(logits=None), dict(tlen=None), dict(seq=None), dict(loss=None), dict(frames=None), dict(agree=None),
               dict(ws=None), dict(T=0), dict(B=0), dict(V=1)):
        for acc in (0, 1):
            a = dict(logits=ld, teacher=td, seq=sd, tlen=tl, T=T, B=B, V=V, tau=1.0, scale=1.0, loss=loss, frames=frames,
                     agree=agree, grad=grad, acc=acc, ws=ws, ws_bytes=nbytes)
            a.update(kw)
            assert raw_call(**a) == LC_EINVAL, kw
            assert untouched(), kw
    for short in (0, nbytes - 1):
        assert raw_call(ld, td, sd, tl, T, B, V, 1.0, 1.0, loss, frames, agree, grad, 0, ws, short) == LC_EWORKSPACE
        assert untouched()
    assert lib.lc_last_error().decode().startswith("lc_kd_loss: workspace too small")
    assert raw_call(ld, td, sd, tl, T, B, V, 1.0, 1.0, loss, frames, agree, grad, 0, ws, nbytes) == 0
    assert not untouched()


# ----------------------------------------------------------------------------------------------- 8. the graph
MODEL_CFG = dict(nnet_type="blstm", input_dim=12, left_context=0, right_context=0, num_layers=2, num_neurons=32,
                 num_projects=16, num_targets=8, use_peepholes=True, dropout_rate=1.0)      # tests/test_gpu_xent.py's
MODELS = {"blstm": {}, "lstm": dict(nnet_type="lstm", num_projects=16)}
LAMBDA, TAU = 0.5, 2.0


def _model_batch(cfg, covered=True):
    """B = 5, T = 14: lengths 14, 9, 2, 5, 12 with 3, 2, 1, 0, 4 labels; the teacher does not cover utterance 1."""
    rng = np.random.default_rng(3)
    B, T, D, V = 5, 14, cfg["input_dim"], cfg["num_targets"]
    seq = np.array([14, 9, 2, 5, 12], np.int32)
    x = rng.normal(size=(B, T, D)).astype(np.float32)
    y = np.full((B, 4), -1, np.int64)
    for b, n in enumerate([3, 2, 1, 0, 4]):
        y[b, :n] = rng.integers(0, V - 1, size=n)
    tlen = seq.copy()
    tlen[1] = 0
    if not covered:
        tlen[:] = 0
    t = rng.standard_normal((T, B, V)) * 2.0
    teacher = (t - np.log(np.exp(t).sum(axis=-1, keepdims=True))).astype(np.float32)
    for b in range(B):
        x[b, seq[b]:] = 0
        teacher[tlen[b]:, b] = 0
    return {"nnet_input": x, "sequence_length": seq, "nnet_target": y, "target_length": (y >= 0).sum(axis=1).astype(np.int32),
            "teacher_scores": teacher, "teacher_length": tlen}


def _oracle_step(oracle, params, cfg, batch, state, optimizer, lr, objective):
    """One training step from the oracle's parts around kd_ref, in float64 around the float32 parameters."""
    from lstm_ctc_amd.nnet.graph import flatten_labels
    logits, saved = oracle.forward(params, cfg, batch["nnet_input"], batch["sequence_length"])      # [B,T,V]
    tbv = np.ascontiguousarray(np.asarray(logits).transpose(1, 0, 2))
    ref = kd_ref(tbv, batch["teacher_scores"], batch["sequence_length"], batch["teacher_length"], TAU)
    kd_sum = float(ref["loss"].sum())
    if objective == "kd":
        grad = TAU * ref["grad"]
        base = 0.0
        loss = TAU * TAU * kd_sum
    else:
        flat, offs, _ = flatten_labels(batch["nnet_target"])
        ctc, cgrad, _ = oracle.ctc_loss(tbv, flat, offs, batch["sequence_length"])
        grad = np.asarray(cgrad, np.float64) + LAMBDA * TAU * ref["grad"]
        base = float(np.asarray(ctc, np.float64).sum())
        loss = base + LAMBDA * TAU * TAU * kd_sum
    dlogits = np.ascontiguousarray(grad.transpose(1, 0, 2)).astype(np.asarray(logits).dtype)
    grads, _ = oracle.backward(params, cfg, saved, dlogits)
    clipped, norm = oracle.l2_and_clip(params, grads, 5.0, 1e-5)
    oracle.apply_optimizer(optimizer, params, clipped, state, lr)
    frames = int(ref["frames"].sum())
    return dict(frames=frames, agree=int(ref["agree"].sum()), kd=kd_sum, base=base, loss=loss, grad_norm=float(norm))


def _make_graph(objective, cfg, **kw):
    from lstm_ctc_amd.nnet import graph as G
    if objective == "kd":
        return G.create_graph_for_training_kd(None, cfg, teacher_temperature=TAU, **kw)
    return G.create_graph_for_training_ctc(None, cfg, teacher_weight=LAMBDA, teacher_temperature=TAU, **kw)


@pytest.mark.parametrize("optimizer", ["adam", "sgd"])
@pytest.mark.parametrize("model", sorted(MODELS))
@pytest.mark.parametrize("objective", ["kd", "ctc"])
def test_train_steps_vs_oracle_composition(oracle, objective, model, optimizer):
    cfg = dict(MODEL_CFG, **MODELS[model])
    batch = _model_batch(cfg)
    graph = _make_graph(objective, cfg, learn_rate=1e-2, clip_norm=5.0, optimizer=optimizer, seed=11)
    params = {k: v.copy() for k, v in graph.model.ps.export_tf().items()}
    state = {}
    for step in range(3):
        out = graph.step(batch, fetch_eval=True)
        ref = _oracle_step(oracle, params, cfg, batch, state, optimizer, 1e-2, objective)
        assert out["kd_frames"] == ref["frames"] == 14 + 2 + 5 + 12           # utterance 1 is not covered
        assert out["kd_agree"] == ref["agree"]
        assert abs(out["kd_loss"] - ref["kd"]) / ref["kd"] < 1e-4
        assert abs(out["loss"] - ref["loss"]) / ref["loss"] < 1e-4            # no regulariser in this configuration
        if objective == "kd":
            assert "decoded" not in out
            assert out["size"] == ref["frames"] and out["eval"] == float(ref["frames"] - ref["agree"])
            assert abs(out["eval_loss"] - ref["loss"]) / ref["loss"] < 1e-4
        else:
            assert out["size"] == 10 and "decoded" in out                     # the base criterion's: the labels
            assert abs(out["eval_loss"] - ref["base"]) / ref["base"] < 1e-4
        assert abs(out["grad_norm"] - ref["grad_norm"]) / ref["grad_norm"] < 2e-3
        got = graph.model.ps.export_tf()
        for k in params:
            assert np.abs(got[k] - params[k]).max() < 2e-4 * max(1.0, np.abs(params[k]).max()), (step, k)


@pytest.mark.parametrize("model", sorted(MODELS))
def test_teacher_weight_none_is_the_graph_without_the_keyword(model):
    from lstm_ctc_amd.nnet.graph import create_graph_for_training_ctc
    cfg = dict(MODEL_CFG, **MODELS[model])
    batch = _model_batch(cfg)
    plain_batch = {k: v for k, v in batch.items() if not k.startswith("teacher_")}
    kw = dict(learn_rate=1e-2, clip_norm=5.0, optimizer="adam", seed=11)
    a = create_graph_for_training_ctc(None, cfg, **kw)
    b_ = create_graph_for_training_ctc(None, cfg, teacher_weight=None, teacher_temperature=3.0, **kw)
    c = create_graph_for_training_ctc(None, cfg, teacher_weight=LAMBDA, teacher_temperature=TAU, **kw)
    assert torch.equal(a.model.ps.flat, c.model.ps.flat)
    # on the same parameters the weighted step's eval_loss is the unweighted step's, bit for bit
    oa, oc = a.step(plain_batch, fetch_eval=True), c.step(batch, fetch_eval=True)
    assert oa["eval_loss"] == oc["eval_loss"] and oa["eval"] == oc["eval"] and oa["size"] == oc["size"]
    assert "kd_loss" not in oa and oc["kd_loss"] > 0 and oc["loss"] == oc["eval_loss"] + LAMBDA * TAU * TAU * oc["kd_loss"]
    ob = b_.step(batch, fetch_eval=True)                                      # a batch that carries the keys is as good
    assert all(ob[k] == oa[k] for k in ("eval_loss", "loss", "eval", "size")) and "kd_loss" not in ob
    for _ in range(2):
        a.step(plain_batch)
        b_.step(batch)
    assert torch.equal(a.model.ps.flat, b_.model.ps.flat)
    assert not torch.equal(a.model.ps.flat, c.model.ps.flat)


@pytest.mark.parametrize("model", sorted(MODELS))
def test_six_adam_steps_reduce_the_kd_loss(model):
    cfg = dict(MODEL_CFG, **MODELS[model])
    batch = _model_batch(cfg)
    graph = _make_graph("kd", cfg, learn_rate=1e-2, clip_norm=5.0, optimizer="adam", seed=11)
    got = [graph.step(batch)["eval_loss"] for _ in range(6)]
    print("\nkd eval_loss (%s): %s" % (model, ["%.4f" % v for v in got]))
    assert got[-1] < got[0]


def test_validation_graph_without_a_covered_utterance_and_validation():
    from lstm_ctc_amd.nnet.graph import CTCGraph, create_graph_for_validation_kd, create_graph_for_training_kd
    cfg = dict(MODEL_CFG)
    graph = create_graph_for_validation_kd(None, cfg, seed=3, teacher_temperature=TAU)
    out = graph.step(_model_batch(cfg, covered=False), fetch_eval=True)
    assert out["size"] == 0 and out["eval_loss"] == 0.0 and out["loss"] == 0.0 and out["eval"] == 0.0
    staged = graph.stage(_model_batch(cfg))                                   # the prefetch path carries the scores along
    out2 = graph.step(None, staged=staged, fetch_eval=True)
    assert out2["size"] == 33 and 0 <= out2["eval"] <= 33 and out2["eval_loss"] > 0
    assert (graph.kd_frames_total, graph.kd_agree_total) == (33, out2["kd_agree"])
    # a training step on nothing still runs the optimizer (on the L2 term alone)
    tr = create_graph_for_training_kd(None, cfg, learn_rate=1e-2, optimizer="sgd", seed=11)
    before = tr.model.ps.flat.clone()
    assert tr.step(_model_batch(cfg, covered=False))["size"] == 0
    assert tr.opt_step == 1 and not torch.equal(before, tr.model.ps.flat)
    # validation of the keywords
    plain = {k: v for k, v in _model_batch(cfg).items() if not k.startswith("teacher_")}
    with pytest.raises(ValueError, match="teacher_scores"):
        graph.step(plain)
    for bad in (0.0, -1.0, float("nan"), float("inf"), "1", True):
        with pytest.raises(ValueError, match="teacher_weight"):
            CTCGraph(None, cfg, teacher_weight=bad)
    for bad in (0.0, -2.0, float("nan"), float("inf"), None):
        with pytest.raises(ValueError, match="teacher_temperature"):
            CTCGraph(None, cfg, teacher_weight=1.0, teacher_temperature=bad)
    with pytest.raises(ValueError, match="teacher_weight"):
        CTCGraph(None, cfg, objective="kd", teacher_weight=1.0)


def test_teacher_term_composes_with_align_window_and_xent():
    from lstm_ctc_amd.nnet.graph import create_graph_for_validation_ctc, create_graph_for_validation_xent
    cfg = dict(MODEL_CFG)
    batch = _model_batch(cfg)
    batch["frame_target"] = np.full((5, 14), -1, np.int32)                    # no usable alignment: plain CTC windows
    kd = create_graph_for_validation_ctc(None, cfg, seed=3, teacher_weight=LAMBDA, teacher_temperature=TAU).step(batch)
    win = create_graph_for_validation_ctc(None, cfg, seed=3, align_window=2, teacher_weight=LAMBDA,
                                          teacher_temperature=TAU).step(batch)
    assert win["kd_loss"] == kd["kd_loss"] and win["kd_frames"] == 33
    assert abs(win["eval_loss"] - kd["eval_loss"]) <= BAR * max(abs(kd["eval_loss"]), 1.0)
    rng = np.random.default_rng(0)
    batch["frame_target"] = rng.integers(0, 8, size=(5, 14)).astype(np.int32)
    xe = create_graph_for_validation_xent(None, cfg, seed=3, teacher_weight=LAMBDA, teacher_temperature=TAU).step(batch)
    assert xe["kd_loss"] == kd["kd_loss"] and xe["size"] == 14 + 9 + 2 + 5 + 12
    assert xe["loss"] == xe["eval_loss"] + LAMBDA * TAU * TAU * xe["kd_loss"]


# ----------------------------------------------------------------------------------------------- 9. command lines
def _run(cli, *args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", cli)] + list(args), capture_output=True, timeout=300)
    return r.returncode, r.stderr.decode()


def _logged(err, name):
    lines = [l for l in err.split("\n") if l.startswith("INFO:tensorflow:%s = " % name)]
    assert len(lines) == 1, err
    return float(lines[0].split()[-1])


def test_cli_chain_teacher_forward_student_train_validate(tmp_path):
    import lstm_ctc_amd.nnet as nnet
    from lstm_ctc_amd.kaldi_io import BaseFloatMatrixWriter, FloatMatrixTable
    rng = np.random.default_rng(7)
    D, V = 6, 9
    lines = []
    for i, T in enumerate([20, 24, 31, 40]):
        path = str(tmp_path / ("utt%03d.tfrecords" % i))
        nnet.write_tfrecord(path, rng.normal(size=(T, D)).astype(np.float32), rng.integers(0, V - 1, size=int(rng.integers(1, 5))))
        lines.append("utt%03d %d %d 1 %s" % (i, T, D, path))
    scp = tmp_path / "tfrecords.scp"
    scp.write_text("\n".join(lines) + "\n")
    body = ("input_dim = 6\nleft_context = 1\nright_context = 1\nsubsample = 2\nnum_layers = 2\nnum_neurons = 32\n"
            "num_projects = 16\nnum_targets = 9\nuse_peepholes = true\ndropout_rate = 1.0\n")
    teacher_cfg, student_cfg = tmp_path / "teacher.config", tmp_path / "student.config"
    teacher_cfg.write_text("nnet_type = blstm\n" + body)
    student_cfg.write_text("nnet_type = lstm\n" + body)
    d = str(tmp_path)
    rc, err = _run("nnet-init.py", "--objective=ctc", "--batch-size", "2", str(scp), str(teacher_cfg), d + "/teacher.0")
    assert rc == 0, err
    rc, err = _run("nnet-forward.py", "--apply-log=true", str(scp), str(teacher_cfg), d + "/teacher.0", "ark:" + d + "/post.ark")
    assert rc == 0, err
    table = FloatMatrixTable(d + "/post.ark")
    assert sorted(table.keys()) == ["utt%03d" % i for i in range(4)]
    assert [table.shape("utt%03d" % i) for i in range(4)] == [(10, 9), (12, 9), (15, 9), (20, 9)]      # frames after subsample = 2
    w = BaseFloatMatrixWriter("ark:" + d + "/post3.ark")                     # one utterance deleted on purpose
    for k in sorted(table.keys())[1:]:
        w.Write(k, table.get(k))
    w.Close()
    rc, err = _run("nnet-init.py", "--objective=ctc", "--batch-size", "2", str(scp), str(student_cfg), d + "/student.0")
    assert rc == 0, err
    train = ["--learn-rate=0.01", "--optimizer=adam", "--seed=1", "--shuffle=false", "--report-interval=1", "--batch-size", "2"]
    rc, err = _run("nnet-train.py", "--objective=ctc", "--teacher-scores", "ark:" + d + "/post3.ark", "--teacher-weight", "0.5",
                   *(train + [str(scp), str(student_cfg), d + "/student.0", d + "/student.1"]))
    assert rc == 0, err
    assert np.isfinite(_logged(err, "tr_loss"))
    assert ("INFO:tensorflow:teacher scores: 1 utterance(s) without an entry, 0 with an entry of another shape than [frames, "
            "targets], 0 with a row that is no distribution (none is scored); 47 frame(s) scored, the argmaxes agree on ") in err
    rc, err = _run("nnet-validate.py", "--objective=kd", "--teacher-scores", d + "/post3.ark", "--teacher-temperature", "2",
                   "--evaluate=true", "--batch-size", "2", str(scp), str(student_cfg), d + "/student.1")
    assert rc == 0, err
    assert np.isfinite(_logged(err, "cv_loss")) and 0.0 <= _logged(err, "cv_eval") <= 1.0
    assert "INFO:tensorflow:teacher scores: 1 utterance(s) without an entry" in err and "47 frame(s) scored" in err


def test_zz_report_measured_error_over_bound():
    print("\nkd: largest measured error / derived bound: loss %.3f, grad %.3f; loss error / project bar %.4f"
          % (MEASURED["loss"], MEASURED["grad"], MEASURED["loss_bar"]))
    assert MEASURED["loss"] <= 1.0 and MEASURED["grad"] <= 1.0 and MEASURED["loss_bar"] <= 1.0
