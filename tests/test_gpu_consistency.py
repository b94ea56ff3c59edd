"""lc_consistency_loss (consistency-regularised CTC) on the GPU: the op, the graph's consistency_weight and the command line.

Reference: float64 numpy (``cr_ref`` of tests/test_consistency_host.py); for the graph, the same graph WITHOUT the option run
on the explicitly doubled batch with the pair term's gradient added from ``cr_ref``.

Tolerances - derived from the kernel's arithmetic, not from what it was seen to give (u = 2^-24, fp32 unit round-off; first
order in u).  Per scored pair-frame, za and zb the two rows, the kernel forms (csrc/consistency.hip)
    a_k = fl(za_k - max za), b_k = fl(zb_k - max zb), ea_k = exp2(fl(a_k log2e)), eb_k = exp2(fl(b_k log2e)),
    Sa = sum ea, Sb = sum eb, d_k = fl(fl(ea_k rcp(Sa)) - fl(eb_k rcp(Sb))), L = fl((log2 Sa - log2 Sb) ln2),
    x_k = fl(fl(a_k - b_k) - L),  J = sum_{d_k != 0} fl(d_k x_k);   grad a = fl(grad_scale d_k), grad b = -grad a.
Write qa = ea / Sa, qb = eb / Sb, and x_k = log qa_k - log qb_k for the exact values.

* An exponential: the argument carries u (difference) + u (the constant) + u (product) = 3u relative, which exp2 turns into
  a relative 3u |a_k|; the hardware exp2 adds 1 ulp.  ea_k |a_k| <= 1 / e, so a term of Sa is off by <= (3 / e) u + u ea_k <=
  1.11u + u ea_k, V terms: (1.11 V + 1) u Sa (Sa >= 1).  The terms are added in fp32 in a fixed order, at most NADD(V) =
  ceil(V / 64) + 16 additions deep in every kernel variant (V <= 64: 4 + 4; V <= 1024: 4 / 8 / 16 + 6; wider: <= V / 64 + 2 +
  6):
      E_S(V) = 1.11 V + 1 + NADD(V)          relative error of Sa and of Sb, in units of u.
* A quotient qa_k: the exponential's (3 |a_k| + 1) u, the sum's E_S u, the hardware reciprocal and the product (2u): relative
  (3 |a_k| + E_S + 3) u.  The difference rounds once:
      delta_k = qa_k (3 |a_k| + E_S + 3) + qb_k (3 |b_k| + E_S + 3) + |d_k|        |error of d_k| <= u delta_k.
  With qa_k |a_k| <= 1 / e and qa_k <= 1 that is <= u (2 E_S + 9.3), and the product with grad_scale rounds once more:
      tol_grad = |grad_scale| u (2 E_S(V) + 11)       absolute, per element, for both rows;
  accumulating into G adds one rounding of the sum: + u |G + g|.
* L: E_S u from each sum, 1 ulp of the hardware log2 each (u ln V), the subtraction (u ln V at most), the constant and the
  product (1.5u ln V): <= Lambda u, Lambda = 2 E_S + 4.5 ln V.
* x_k: two rounded operands and the rounded difference a_k - b_k (u (|a_k| + |b_k| + |a_k - b_k|)), L's Lambda u, its own
  rounding (u |x_k|).
* J: a term d_k x_k carries |x_k| u delta_k + |d_k| u (|a_k| + |b_k| + |a_k - b_k| + Lambda + |x_k|) and the product's u |d_k
  x_k|; the additions NADD u sum |d_k x_k|.  The fold adds a pair's terms as doubles (2^-53 each - nothing at these sizes)
  and rounds the sum once (u |loss|):
      eps_frame = u sum_k (|x_k| delta_k + |d_k| (|a_k| + |b_k| + |a_k - b_k| + Lambda + |x_k|) + (1 + NADD) |d_k x_k|)
      tol_loss[b] = sum over the scored pair-frames of eps_frame + u |loss_b|.
  Two equal rows give d = 0 and J = 0 EXACTLY in the kernel (the same operations on the same bits; the two quotients are
  rounded before the difference), which the identity test asserts without a tolerance.
* All are asserted TOGETHER with the project's bar (tests/conftest.py): 1e-4 max(|ref|, 1) for a loss, check_grad / GRAD_TOL
  for a gradient tensor.  frames and agree are integers and compared exactly; the inputs are drawn so that no row has two
  equal maxima (asserted on the reference) except in the tie test.

The launch caps (csrc/consistency.hip): 2048 blocks of four waves - 32768 pair-frames per pass at four per wave (V <= 64),
8192 at one per wave; the grid-stride tests go past each.

Measured (MI355X, the last test's line): the largest error over its derived bound is 0.038 for a loss and 0.083 for a gradient
element; the largest loss error over the project's bar is 0.0020.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import check_grad
from test_consistency_host import cr_ref, e_s

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
BAR = 1e-4                         # tests/conftest.py: GRAD_TOL, the project's bar for logits and loss
LC_EINVAL, LC_EWORKSPACE = -1, -3
MEASURED = {"loss": 0.0, "grad": 0.0, "loss_bar": 0.0}     # largest measured error / bound (printed by the last test)


def tol_grad(V, scale):
    return abs(scale) * U * (2 * e_s(V) + 11)


def assert_unique_maxima(x):
    x = np.asarray(x)
    top2 = np.partition(x, -2, axis=-1)[..., -2:]
    assert (top2[..., 0] < top2[..., 1]).all(), "test input has a row with two equal maxima"


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def run_cr(logits, seq, scale=1.0, want_grad=True, into=None):
    from lstm_ctc_amd import ops
    grad_in = None if into is None else _dev(into, np.float32)
    loss, frames, agree, grad = ops.consistency_loss(_dev(logits, np.float32), _dev(seq, np.int32), grad_scale=scale,
                                                     grad=grad_in, want_grad=want_grad)
    torch.cuda.synchronize()
    return (loss.cpu().numpy(), frames.cpu().numpy(), agree.cpu().numpy(), None if grad is None else grad.cpu().numpy())


def check_loss(loss, ref, tag):
    for b in range(len(loss)):
        r = ref["loss"][b]
        if not np.isfinite(r):
            assert (np.isnan(loss[b]) and np.isnan(r)) or loss[b] == r, (tag, b, loss[b], r)
            continue
        tol = U * (ref["eps"][b] + abs(r))
        bar = BAR * max(abs(r), 1.0)
        err = abs(float(loss[b]) - r)
        print("loss", tag, b, "err %.3e tol %.3e bar %.3e" % (err, tol, bar))
        if tol > 0:
            MEASURED["loss"] = max(MEASURED["loss"], err / tol)
        MEASURED["loss_bar"] = max(MEASURED["loss_bar"], err / bar)
        assert err <= tol and err <= bar, (tag, b, err, tol, bar)


def check_against_ref(logits, seq, scale, got, tag, into=None, ref=None):
    loss, frames, agree, grad = got
    V = logits.shape[-1]
    ref = cr_ref(logits, seq) if ref is None else ref
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
        print("grad", tag, "err / tol %.3f" % ratio)
        MEASURED["grad"] = max(MEASURED["grad"], ratio)
        assert ratio <= 1.0, (tag, ratio)
        check_grad(grad, g, tag, "dlogits")
        rest = ~np.concatenate([ref["scored"]] * 2, axis=1)
        if into is None:
            assert not grad[rest].any() and not np.signbit(grad[rest]).any(), tag                    # exactly +0
        else:
            assert grad[rest].tobytes() == np.asarray(into, np.float32)[rest].tobytes(), tag         # left bit-exactly
    return ref


def make_case(rng, T, B, V, seq, scale=3.0):
    """[T,2B,V] logits, the two views their own random rows, and the pairs' lengths."""
    logits = (rng.standard_normal((T, 2 * B, V)) * scale).astype(np.float32)
    assert_unique_maxima(logits)
    return logits, np.asarray(seq, np.int32)


# ----------------------------------------------------------------------------------------------- 1. the op at the edges
EDGE_V = [2, 3, 16, 63, 64, 65, 256, 257, 512, 513, 1024, 1025, 1030, 4100]
EDGE_SHAPES = [(5, 3, [5, 0, 1]), (9, 3, [4, 9, 0]), (7, 1, [7]), (6, 1, [1])]


@pytest.mark.parametrize("V", EDGE_V)
def test_op_matches_reference_at_dispatch_edges(V):
    rng = np.random.default_rng(3000 + V)
    for (T, B, seq), scale in zip(EDGE_SHAPES, [1.0, 0.1, 0.5, 2.0]):
        logits, seq = make_case(rng, T, B, V, seq)
        got = run_cr(logits, seq, scale)
        ref = check_against_ref(logits, seq, scale, got, ("edge", V, T, B))
        assert ref["frames"].sum() > 0 and (B == 1 or (ref["frames"] == 0).any())
        assert np.array_equal(got[3][:, :B], -got[3][:, B:])             # the two rows are each other's negative, to the bit
        nograd = run_cr(logits, seq, scale, want_grad=False)
        assert nograd[3] is None
        for a, b_ in zip(got[:3], nograd[:3]):                            # the same bits with and without a gradient
            assert a.tobytes() == b_.tobytes()


# ----------------------------------------------------------------------------------------------- raw calls
def raw_call(logits, seq, T, B, V, scale, loss, frames, agree, grad, acc, ws, ws_bytes):
    from lstm_ctc_amd import _lib, ops
    lib = _lib.load()
    rc = lib.lc_consistency_loss(ops._ptr(logits), T, B, V, ops._ptr(seq), scale, ops._ptr(loss), ops._ptr(frames),
                                 ops._ptr(agree), ops._ptr(grad), acc, ops._ptr(ws), ws_bytes, ops._stream())
    torch.cuda.synchronize()
    return rc


GUARD = 64                                                                # floats / ints in front of and behind every buffer


class Guarded:
    """A buffer between two guard zones that must come back as they were."""

    def __init__(self, shape, dtype, fill):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
        self.guard = -12345 if dtype == torch.int32 else 777.25
        self.buf[:GUARD] = self.guard
        self.buf[GUARD + n:] = self.guard
        self.view = self.buf[GUARD:GUARD + n].view(*shape)
        assert self.view.data_ptr() % 16 == 0

    def intact(self):
        n = self.view.numel()
        return bool((self.buf[:GUARD] == self.guard).all()) and bool((self.buf[GUARD + n:] == self.guard).all())


@pytest.mark.parametrize("V", [4, 44, 45, 300, 1030, 1100])
def test_accumulate_and_overwrite_between_guards(V):
    from lstm_ctc_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(V)
    T, B, scale = 9, 5, 0.7
    logits, seq = make_case(rng, T, B, V, [9, 0, 5, 1, 7])
    ref = cr_ref(logits, seq)
    assert ref["frames"].tolist() == [9, 0, 5, 1, 7]
    scored2 = np.concatenate([ref["scored"]] * 2, axis=1)
    stored = run_cr(logits, seq, scale)
    # accumulate: scored rows G + g, g the stored call's row, within one rounding; every other row G to the bit - NaN rows
    # among them: they are not read
    G = rng.standard_normal((T, 2 * B, V)).astype(np.float32)
    got = run_cr(logits, seq, scale, into=G)
    check_against_ref(logits, seq, scale, got, ("accumulate", V), into=G)
    exact = G.astype(np.float64) + stored[3].astype(np.float64)
    assert (np.abs(got[3] - exact)[scored2] <= U * np.abs(exact)[scored2]).all()
    Gn = G.copy()
    Gn[~scored2] = np.nan
    got_n = run_cr(logits, seq, scale, into=Gn)
    assert np.isnan(got_n[3][~scored2]).all() and np.array_equal(got_n[3][scored2], got[3][scored2])
    assert got_n[0].tobytes() == got[0].tobytes() == stored[0].tobytes()
    # overwrite on NaN-prefilled outputs between guards and a 0xFF workspace: every element written, the guards intact
    nbytes = lib.lc_consistency_workspace_bytes(T, B, V)
    ld, sd = _dev(logits, np.float32), _dev(seq, np.int32)
    for with_grad in (True, False):
        loss, frames, agree = (Guarded((B,), torch.float32, float("nan")), Guarded((B,), torch.int32, -77),
                               Guarded((B,), torch.int32, -77))
        grad = Guarded((T, 2 * B, V), torch.float32, float("nan"))
        ws = Guarded((nbytes // 4,), torch.int32, -1)                     # 0xFF bytes
        assert raw_call(ld, sd, T, B, V, scale, loss.view, frames.view, agree.view, grad.view if with_grad else None, 0,
                        ws.view, nbytes) == 0
        assert all(x.intact() for x in (loss, frames, agree, grad, ws))
        l, f, c, g = (x.view.cpu().numpy() for x in (loss, frames, agree, grad))
        assert not np.isnan(l).any() and (f != -77).all() and (c != -77).all()
        assert l[1] == 0.0 and not np.signbit(l[1]) and f[1] == 0 and c[1] == 0      # no scored frame: loss +0, counts 0
        assert l.tobytes() == stored[0].tobytes() and np.array_equal(f, stored[1]) and np.array_equal(c, stored[2])
        if with_grad:
            assert g.tobytes() == stored[3].tobytes()
        else:
            assert np.isnan(g).all()                                      # grad = NULL: not touched
    # accumulate between guards
    grad = Guarded((T, 2 * B, V), torch.float32, 0.0)
    grad.view.copy_(_dev(G, np.float32))
    loss, frames, agree = Guarded((B,), torch.float32, 0.0), Guarded((B,), torch.int32, 0), Guarded((B,), torch.int32, 0)
    ws = Guarded((nbytes // 4,), torch.int32, -1)
    assert raw_call(ld, sd, T, B, V, scale, loss.view, frames.view, agree.view, grad.view, 1, ws.view, nbytes) == 0
    assert all(x.intact() for x in (loss, frames, agree, grad, ws))
    assert grad.view.cpu().numpy().tobytes() == got[3].tobytes()


@pytest.mark.parametrize("T,B,V", [(50, 7, 44), (50, 7, 300), (20, 7, 4100)])
def test_two_calls_are_bit_identical(T, B, V):
    rng = np.random.default_rng(5)
    logits, seq = make_case(rng, T, B, V, rng.integers(0, T + 1, size=B))
    a, b_ = run_cr(logits, seq, 1.5), run_cr(logits, seq, 1.5)
    for x, y in zip(a, b_):
        assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("V", [44, 300, 1028])
def test_buffers_off_the_16_byte_boundary_take_the_scalar_path(V):
    """logits, grad or both start 4 bytes behind a 16-byte boundary (views into larger buffers)."""
    from lstm_ctc_amd import ops
    rng = np.random.default_rng(V)
    T, B, scale = 11, 3, 0.25
    logits, seq = make_case(rng, T, B, V, [11, 10, 4])

    def off(a):
        buf = torch.zeros(a.size + 1, device="cuda")
        view = buf[1:].view(*a.shape)
        view.copy_(_dev(a, np.float32))
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        return view

    G = rng.standard_normal((T, 2 * B, V)).astype(np.float32)
    for lg, gr in ((off(logits), off(G)), (off(logits), _dev(G, np.float32)), (_dev(logits, np.float32), off(G))):
        loss, frames, agree, grad = ops.consistency_loss(lg, _dev(seq, np.int32), grad_scale=scale, grad=gr)
        torch.cuda.synchronize()
        got = (loss.cpu().numpy(), frames.cpu().numpy(), agree.cpu().numpy(), grad.cpu().numpy())
        check_against_ref(logits, seq, scale, got, ("unaligned", V), into=G)


# ----------------------------------------------------------------------------------------------- 2. identities
@pytest.mark.parametrize("V", [7, 44, 300, 1024, 1100, 1101])
def test_identical_halves_give_exactly_zero(V):
    rng = np.random.default_rng(V)
    T, B = 8, 3
    logits, seq = make_case(rng, T, B, V, [8, 5, 0])
    logits[:, B:] = logits[:, :B]
    loss, frames, agree, grad = run_cr(logits, seq, 0.37)
    assert np.array_equal(frames, seq) and np.array_equal(agree, frames)
    assert not loss.any() and not grad.any()
    G = rng.standard_normal((T, 2 * B, V)).astype(np.float32)
    acc = run_cr(logits, seq, 0.37, into=G)
    assert acc[3].tobytes() == G.tobytes()                                # G + 0


@pytest.mark.parametrize("V", [44, 1100])
def test_swapping_the_halves_swaps_the_gradient_rows(V):
    rng = np.random.default_rng(V)
    T, B = 8, 3
    logits, seq = make_case(rng, T, B, V, [8, 5, 8])
    a = run_cr(logits, seq, 1.0)
    b_ = run_cr(np.concatenate([logits[:, B:], logits[:, :B]], axis=1), seq, 1.0)
    ref = cr_ref(logits, seq)
    assert np.array_equal(a[1], b_[1]) and np.array_equal(a[2], b_[2])
    for b in range(B):                                                    # either call within its bound of the reference
        assert abs(float(a[0][b]) - float(b_[0][b])) <= 2 * U * (ref["eps"][b] + abs(ref["loss"][b]))
    assert np.abs(a[3][:, :B] - b_[3][:, B:]).max() <= 2 * tol_grad(V, 1.0)


# ----------------------------------------------------------------------------------------------- 3. special values
@pytest.mark.parametrize("V", [5, 44, 300, 1100])
def test_special_values(V):
    rng = np.random.default_rng(V)
    T, B, scale = 6, 4, 0.5
    logits, seq = make_case(rng, T, B, V, [6, 6, 6, 6])
    logits[2, 0, 1] = logits[2, 0 + B, 1] = -np.inf                       # probability 0 in both views: contributes 0
    logits[4, 0, 2] = -np.inf                                             # qb_k > 0 against za_k = -inf: +inf loss
    logits[3, 1 + B, 2] = -np.inf                                         # qa_k > 0 against zb_k = -inf: the same
    logits[3, 2, :] = -np.inf
    logits[3, 2, 2] = -1.5                                                # a one-class row
    assert_unique_maxima(logits)
    got = run_cr(logits, seq, scale)
    loss, frames, agree, grad = got
    ref = check_against_ref(logits, seq, scale, got, ("special", V))
    assert loss[0] == np.inf and loss[1] == np.inf and ref["loss"][1] == np.inf and np.isfinite(loss[3])
    assert np.isfinite(grad).all() and grad[2, 0, 1] == 0.0 and grad[2, B, 1] == 0.0
    qb = scale * np.exp(logits[4, B].astype(np.float64) - np.log(np.exp(logits[4, B].astype(np.float64)).sum()))
    assert abs(grad[4, 0, 2] + qb[2]) <= tol_grad(V, scale)               # qa = 0 there: row a gets -scale * qb
    # the class with -inf in both views alone leaves the pair finite, within the bound
    z = logits.copy()
    z[4, 0, 2] = 0.25
    assert_unique_maxima(z)
    got = run_cr(z, seq, scale)
    ref = check_against_ref(z, seq, scale, got, ("-inf in both views", V))
    assert np.isfinite(got[0][0]) and np.isfinite(ref["loss"][0]) and np.isfinite(ref["eps"][0])
    # bad rows in either view: NaN for that pair only; the pair-frame counts nowhere, its two gradient rows are zero / untouched
    logits, seq = make_case(rng, T, B, V, [6, 6, 5, 6])
    clean = run_cr(logits, seq, scale)
    G = rng.standard_normal((T, 2 * B, V)).astype(np.float32)
    clean_acc = run_cr(logits, seq, scale, into=G)
    for kind, b, view in (("all -inf", 1, 0), ("all -inf", 1, B), ("nan", 2, 0), ("nan", 2, B), ("+inf", 0, B),
                          ("nan at the maximum", 1, 0), ("nan at the maximum", 3, B)):
        z = logits.copy()
        if kind == "all -inf":
            z[3, b + view, :] = -np.inf
        elif kind == "nan":
            z[3, b + view, V - 1] = np.nan
        elif kind == "+inf":
            z[3, b + view, V // 2] = np.inf
        else:
            z[3, b + view, int(logits[3, b + view].argmax())] = np.nan
        loss, frames, agree, grad = run_cr(z, seq, scale)
        assert np.isnan(loss[b]) and frames[b] == clean[1][b] - 1, (kind, view)
        assert not grad[3, b].any() and not grad[3, b + B].any(), (kind, view)
        for o in range(B):
            if o != b:                                # the neighbours are intact, to the bit
                assert loss[o] == clean[0][o] and frames[o] == clean[1][o] and agree[o] == clean[2][o], kind
                assert np.array_equal(grad[:, o], clean[3][:, o]) and np.array_equal(grad[:, o + B], clean[3][:, o + B]), kind
        check_against_ref(z, seq, scale, (loss, frames, agree, grad), ("bad row", V, kind, view))
        acc = run_cr(z, seq, scale, into=G)
        assert acc[3][3, b].tobytes() == G[3, b].tobytes() and acc[3][3, b + B].tobytes() == G[3, b + B].tobytes(), kind
        keep = np.ones((T, 2 * B), bool)
        keep[3, b] = keep[3, b + B] = False
        assert np.array_equal(acc[3][keep], clean_acc[3][keep]), kind
    # a bad row beyond the pair's length is not scored: ignored
    z = logits.copy()
    z[5, 2, :] = np.nan
    z[5, 2 + B, :] = np.nan
    for x, y in zip(run_cr(z, seq, scale), clean):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("V", [6, 44, 300, 2000])
def test_argmax_tie_goes_to_the_lower_index(V):
    rng = np.random.default_rng(V)
    pairs = [(0, 1), (1, V - 1), (V // 2, V // 2 + 1), (2, min(V - 1, 70))]      # within a lane's span and across lanes
    T, B = len(pairs), 4
    seq = np.array([T] * B, np.int32)
    logits = rng.standard_normal((T, 2 * B, V)).astype(np.float32)
    for t, (lo, hi) in enumerate(pairs):
        logits[t, 0, lo] = logits[t, 0, hi] = 9.5     # pair 0: view a ties, view b peaks on the lower index
        logits[t, 0 + B, lo] = 9.5
        logits[t, 1, lo] = logits[t, 1, hi] = 9.5     # pair 1: ... view b peaks on the higher one
        logits[t, 1 + B, hi] = 9.5
        logits[t, 2 + B, lo] = logits[t, 2 + B, hi] = 9.5      # pairs 2 and 3: the same with view b tying
        logits[t, 2, lo] = 9.5
        logits[t, 3 + B, lo] = logits[t, 3 + B, hi] = 9.5
        logits[t, 3, hi] = 9.5
    loss, frames, agree, _ = run_cr(logits, seq)
    assert frames.tolist() == [T] * B
    assert agree.tolist() == [T, 0, T, 0]
    ref = cr_ref(logits, seq)
    assert np.array_equal(agree, ref["agree"])
    assert np.allclose(loss, ref["loss"], rtol=1e-5)


# ----------------------------------------------------------------------------------------------- 4. grid stride
@pytest.mark.parametrize("T,B,V", [(11000, 3, 4), (2750, 3, 65), (2750, 3, 300), (2750, 3, 1024), (2750, 3, 1028)])
def test_more_pair_frames_than_one_pass_of_the_grid(T, B, V):
    """Past the cap of every kernel variant (V <= 64: 32768 pair-frames per pass; one pair-frame per wave with 4, 8 and 16
    elements per lane - V = 65, 300, 1024 -: 8192; the wide kernel at V = 1028: 8192 too): a second pass of the grid-stride loop.  Pair 0 is scored to the end, so the frames
    of the second pass carry weight; pair 2 scores nothing."""
    assert T * B > (32768 if V <= 64 else 8192)
    rng = np.random.default_rng(V)
    logits, seq = make_case(rng, T, B, V, [T, T // 3, 0])
    G = rng.standard_normal((T, 2 * B, V)).astype(np.float32)
    ref = check_against_ref(logits, seq, 1.0, run_cr(logits, seq, 1.0), ("grid stride", V))
    check_against_ref(logits, seq, 1.0, run_cr(logits, seq, 1.0, into=G), ("grid stride acc", V), into=G, ref=ref)


# ----------------------------------------------------------------------------------------------- 5. argument checks
def _prefilled(T, B, V):
    return (torch.full((B,), float("nan"), device="cuda"), torch.full((B,), -77, dtype=torch.int32, device="cuda"),
            torch.full((B,), -77, dtype=torch.int32, device="cuda"), torch.full((T, 2 * B, V), float("nan"), device="cuda"))


def test_argument_checks_leave_the_outputs_alone():
    from lstm_ctc_amd import _lib
    lib = _lib.load()
    T, B, V = 4, 3, 10
    rng = np.random.default_rng(0)
    logits, seq = make_case(rng, T, B, V, [4, 3, 2])
    ld, sd = _dev(logits, np.float32), _dev(seq, np.int32)
    nbytes = lib.lc_consistency_workspace_bytes(T, B, V)
    assert nbytes >= 8 * T * B
    assert lib.lc_consistency_workspace_bytes(0, B, V) == 0 and lib.lc_consistency_workspace_bytes(T, B, 1) == 0
    ws = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device="cuda")
    loss, frames, agree, grad = _prefilled(T, B, V)

    def untouched():
        return (bool(torch.isnan(loss).all()) and bool((frames == -77).all()) and bool((agree == -77).all())
                and bool(torch.isnan(grad).all()) and bool((ws == 0x5A).all()))           # the workspace: nothing was launched

    for kw in (dict(scale=float("nan")), dict(scale=float("inf")), dict(scale=float("-inf")), dict(logits=None), dict(seq=None),
               dict(loss=None), dict(frames=None), dict(agree=None), dict(ws=None), dict(T=0), dict(B=0), dict(T=-1),
               dict(B=-2), dict(V=1)):
        for acc in (0, 1):
            a = dict(logits=ld, seq=sd, T=T, B=B, V=V, scale=1.0, loss=loss, frames=frames, agree=agree, grad=grad, acc=acc,
                     ws=ws, ws_bytes=nbytes)
            a.update(kw)
            assert raw_call(**a) == LC_EINVAL, kw
            assert untouched(), kw
    assert raw_call(ld, sd, T, B, V, 1.0, loss, frames, agree, None, 1, ws, nbytes) == LC_EINVAL      # accumulate into nothing
    assert untouched()
    for short in (0, nbytes - 1):
        assert raw_call(ld, sd, T, B, V, 1.0, loss, frames, agree, grad, 0, ws, short) == LC_EWORKSPACE
        assert untouched()
    assert lib.lc_last_error().decode().startswith("lc_consistency_loss: workspace too small")
    assert raw_call(ld, sd, T, B, V, 1.0, loss, frames, agree, grad, 0, ws, nbytes) == 0
    assert not untouched()
    from lstm_ctc_amd import ops
    with pytest.raises(ValueError, match="2B"):
        ops.consistency_loss(ld, _dev([4, 3], np.int32))
    with pytest.raises(ValueError, match="accumulate"):
        ops.consistency_loss(ld, sd, grad=torch.zeros(T, B, V, device="cuda"))


# ----------------------------------------------------------------------------------------------- 6. the graph
ALPHA = 0.2


def _cfg(layers, dropout):
    return dict(nnet_type="blstm", input_dim=12, left_context=0, right_context=0, num_layers=layers, num_neurons=32,
                num_projects=16, num_targets=12, use_peepholes=True, dropout_rate=dropout)


def _spec():
    from lstm_ctc_amd.nnet.augment import SpecAugment
    return SpecAugment(time_masks=2, time_width=4, time_percent=50, freq_masks=1, freq_width=3, freq_bins=12)


def _batch():
    """B = 3, T = 14: lengths 14, 9, 5 with 3, 2, 1 labels."""
    rng = np.random.default_rng(3)
    B, T, D, V = 3, 14, 12, 12
    seq = np.array([14, 9, 5], np.int32)
    x = rng.normal(size=(B, T, D)).astype(np.float32)
    y = np.full((B, 4), -1, np.int64)
    for b, n in enumerate([3, 2, 1]):
        y[b, :n] = rng.integers(0, V - 1, size=n)
        x[b, seq[b]:] = 0
    return {"nnet_input": x, "sequence_length": seq, "nnet_target": y}


def _graph(cfg, **kw):
    from lstm_ctc_amd.nnet.graph import create_graph_for_training_ctc
    return create_graph_for_training_ctc(None, cfg, learn_rate=1e-2, clip_norm=5.0, optimizer="sgd", seed=11,
                                         spec_augment=_spec(), **kw)


def _doubled(graph, batch, with_windows=False):
    """What ``graph._upload`` gives for ``batch``, doubled by hand on the device."""
    x, seq_d, seq, flat_d, offs_d, flat, offs, maxlen = graph._upload(batch)
    windows = None
    if with_windows:
        lo_d, hi_d, constrained = graph._upload_windows(batch, flat, offs, seq)
        assert constrained.all()
        windows = (torch.cat([lo_d, lo_d]), torch.cat([hi_d, hi_d]))
    offs2 = torch.cat([offs_d, offs_d[1:] + int(offs[-1])])
    return dict(x=torch.cat([x, x], dim=1), seq_d=torch.cat([seq_d, seq_d]), flat_d=torch.cat([flat_d, flat_d]), offs_d=offs2,
                maxlen=maxlen, size=2 * int(len(flat)), windows=windows)


@pytest.mark.parametrize("layers,dropout", [(1, 1.0), (2, 0.8)])
def test_training_step_is_the_doubled_batch_plus_the_pair_term(layers, dropout, monkeypatch):
    from lstm_ctc_amd import ops
    cfg = _cfg(layers, dropout)
    batch = _batch()
    seq = batch["sequence_length"]
    B, labels, frames = 3, 6, int(seq.sum())
    with_option, plain = _graph(cfg, consistency_weight=ALPHA), _graph(cfg)
    assert torch.equal(with_option.model.ps.flat, plain.model.ps.flat)
    # by hand: the graph without the option on the doubled batch, alpha * 0.5 * (qa - qb | qb - qa) added to the CTC gradient
    real, seen = ops.ctc_loss, {}

    def ctc_plus_pair_term(logits, *a, **k):
        loss, grad = real(logits, *a, **k)
        seen["ref"] = cr_ref(logits.cpu().numpy(), seq)
        grad += torch.from_numpy((ALPHA * 0.5 * seen["ref"]["grad"]).astype(np.float32)).cuda()
        return loss, grad

    d = _doubled(plain, batch)
    monkeypatch.setattr(ops, "ctc_loss", ctc_plus_pair_term)
    want = plain.step_device(d["x"], d["seq_d"], d["flat_d"], d["offs_d"], d["maxlen"], d["size"])
    monkeypatch.undo()
    ref = seen["ref"]
    assert ref["frames"].sum() == frames and ref["loss"].sum() > 0       # the two views differ
    # the option, through step_device on the caller's tensors
    x, seq_d, _, flat_d, offs_d, flat, offs, maxlen = with_option._upload(batch)
    keep = x.clone()
    out = with_option.step_device(x, seq_d, flat_d, offs_d, maxlen, int(len(flat)), fetch_eval=True, fetch_logits=True,
                                  flat_host=flat, offs_host=offs, seq_host=seq)
    assert torch.equal(x, keep)                                           # the caller's x is unchanged
    assert with_option.persist_fallbacks == 0 and plain.persist_fallbacks == 0
    assert out["size"] == 2 * labels == want["size"] and out["logits"].shape == (2 * B, 14, 12)
    assert abs(out["eval_loss"] - want["eval_loss"]) <= 1e-6 * max(1.0, abs(want["eval_loss"]))      # the same kernels, the same bits in
    assert out["cr_frames"] == frames and out["cr_agree"] == int(ref["agree"].sum())
    assert abs(out["cr_loss"] - ref["loss"].sum()) <= BAR * max(1.0, ref["loss"].sum())
    assert abs(out["loss"] - (out["eval_loss"] + ALPHA * 0.5 * out["cr_loss"])) <= 1e-6 * max(1.0, abs(out["loss"]))
    assert (with_option.cr_frames_total, with_option.cr_agree_total) == (out["cr_frames"], out["cr_agree"])
    assert with_option.cr_loss_total == out["cr_loss"]
    assert with_option.specaug_steps == 1 and with_option.specaug_frames == 2 * frames      # the shares count both views
    # eval: view a alone against the original labels
    tok, n = out["decoded"]
    assert tok.shape[0] == B and n.shape == (B,) and out["eval_size"] == labels       # eval / eval_size is the rate
    assert out["eval"] == float(ops.edit_distance_host(tok, n, flat, offs).sum())
    mine = cr_ref(out["logits"].transpose(1, 0, 2), seq)                  # the step's own logits: the doubled batch's
    assert abs(out["cr_loss"] - mine["loss"].sum()) <= BAR * max(1.0, mine["loss"].sum())
    assert abs(out["grad_norm"] - want["grad_norm"]) <= 2e-3 * want["grad_norm"]
    got, exp = with_option.model.ps.export_tf(), plain.model.ps.export_tf()
    for k in exp:                                                         # one SGD step: the existing step-level bar
        assert np.abs(got[k] - exp[k]).max() < 2e-4 * max(1.0, np.abs(exp[k]).max()), k
    bare = _graph(cfg)                                                    # the doubled batch alone is another step
    bare.step_device(d["x"], d["seq_d"], d["flat_d"], d["offs_d"], d["maxlen"], d["size"])
    assert not torch.equal(bare.model.ps.flat, with_option.model.ps.flat)
    # a second step through ``step``: the totals add up, the term is still there
    out2 = with_option.step(batch)
    assert out2["size"] == 2 * labels and out2["cr_frames"] == frames and out2["eval_size"] == labels
    assert np.array_equal(out2["sequence_length"], np.concatenate([seq, seq]))      # frames per second count both views
    assert with_option.cr_frames_total == 2 * frames and with_option.cr_agree_total == out["cr_agree"] + out2["cr_agree"]


def test_steps_that_do_not_train_are_the_graph_without_the_option():
    cfg = _cfg(2, 0.8)
    batch = _batch()
    with_option, plain = _graph(cfg, consistency_weight=ALPHA), _graph(cfg)
    a = plain.step(batch, fetch_eval=True, fetch_logits=True, train=False)
    b_ = with_option.step(batch, fetch_eval=True, fetch_logits=True, train=False)
    assert a["logits"].tobytes() == b_["logits"].tobytes() and a["logits"].shape[0] == 3
    assert all(a[k] == b_[k] for k in ("size", "eval_loss", "loss", "eval")) and "cr_loss" not in b_ and "eval_size" not in b_
    assert np.array_equal(b_["sequence_length"], batch["sequence_length"])
    assert with_option.cr_frames_total == 0 and torch.equal(with_option.model.ps.flat, plain.model.ps.flat)
    ali_a, ali_b = plain.align(batch), with_option.align(batch)
    assert np.array_equal(ali_a["ali"], ali_b["ali"]) and ali_b["ali"].shape == (3, 14)
    # and the option off is the step as it was: the same parameters after two training steps, to the bit
    fresh, off = _graph(cfg), _graph(cfg, consistency_weight=None)
    for _ in range(2):
        fresh.step(batch)
        off.step(batch)
    assert torch.equal(off.model.ps.flat, fresh.model.ps.flat)


def test_dropout_alone_gives_two_views_that_differ():
    """No spec_augment: the option is accepted on the strength of dropout, so the dropout hash must depend on the column -
    the two copies of an utterance get other masks, their posteriors differ and the term is not 0.  The graph's keep
    probability is the one the constructor's check computed from the config."""
    from lstm_ctc_amd.nnet.graph import create_graph_for_training_ctc
    from lstm_ctc_amd.nnet.model import config_keep
    cfg = _cfg(2, 0.8)
    graph = create_graph_for_training_ctc(None, cfg, learn_rate=1e-2, optimizer="sgd", seed=11, consistency_weight=ALPHA)
    assert graph.spec_augment is None and graph.model.keep == config_keep(cfg) == 0.8
    out = graph.step(_batch(), fetch_logits=True)
    logits = out["logits"]
    assert out["cr_frames"] == 28 and out["cr_loss"] > 0
    assert (logits[:3] != logits[3:]).any() and out["cr_loss"] == pytest.approx(
        cr_ref(logits.transpose(1, 0, 2), _batch()["sequence_length"])["loss"].sum(), rel=BAR)


def test_option_with_align_window_and_delay_penalty_doubles_the_windows():
    cfg = _cfg(1, 1.0)
    batch = _batch()
    kw = dict(align_window=2, delay_penalty=0.1)
    with_option, plain = _graph(cfg, consistency_weight=ALPHA, **kw), _graph(cfg, **kw)
    batch["frame_target"] = plain.align(batch)["ali"]                     # every utterance gets windows
    d = _doubled(plain, batch, with_windows=True)
    want = plain.step_device(d["x"], d["seq_d"], d["flat_d"], d["offs_d"], d["maxlen"], d["size"], windows=d["windows"])
    out = with_option.step(batch, fetch_eval=True)
    assert with_option.windows_constrained == 3
    assert out["size"] == want["size"] == 12 and out["entry_labels"] == want["entry_labels"] == 12
    assert abs(out["eval_loss"] - want["eval_loss"]) <= 1e-6 * max(1.0, abs(want["eval_loss"]))
    assert abs(out["entry_sum"] - want["entry_sum"]) <= 1e-6 * max(1.0, abs(want["entry_sum"]))
    assert out["cr_frames"] == 28 and np.isfinite(out["cr_loss"]) and out["cr_loss"] > 0 and np.isfinite(out["eval"])
    assert abs(out["loss"] - (out["eval_loss"] + ALPHA * 0.5 * out["cr_loss"])) <= 1e-6 * max(1.0, abs(out["loss"]))


def test_launch_train_retry_repeats_the_draws(monkeypatch):
    """As tests/test_gpu_spec_augment.py stages it: the first try reports a failed recurrence, the step is re-run with the
    counters put back and must double and draw again, and count once."""
    from lstm_ctc_amd import ops
    cfg = _cfg(1, 0.8)
    batch = _batch()
    straight, retried = _graph(cfg, consistency_weight=ALPHA), _graph(cfg, consistency_weight=ALPHA)
    with ops.force_launch_train():
        want = straight.step(batch)
    forward, calls = retried.model.forward, []

    def failing_once(x, *args, **kw):
        logits = forward(x, *args, **kw)
        calls.append((kw.get("drop_seed"), x.shape[1]))
        if len(calls) == 1:
            ops.lstm_status(retried.model.device).fill_(5)
        return logits

    monkeypatch.setattr(retried.model, "forward", failing_once)
    got = retried.step(batch)
    monkeypatch.undo()
    assert retried.persist_fallbacks == 1 and calls == [(straight.drop_seed, 6)] * 2
    assert retried.cr_frames_total == straight.cr_frames_total == 28 and retried.specaug_steps == 1
    assert all(got[k] == want[k] for k in ("size", "eval_loss", "loss", "cr_loss", "cr_frames", "cr_agree"))
    assert torch.equal(retried.model.ps.flat, straight.model.ps.flat)


def test_pack_frames_sees_an_ordinary_batch_of_2b():
    """The doubled lengths reach the model with the doubled input: with and without them on the host (the packed-frames map
    is built from them) the step is the same step."""
    cfg = _cfg(2, 0.8)
    batch = _batch()
    a, b_ = _graph(cfg, consistency_weight=ALPHA), _graph(cfg, consistency_weight=ALPHA)
    x, seq_d, seq, flat_d, offs_d, flat, offs, maxlen = a._upload(batch)
    oa = a.step_device(x, seq_d, flat_d, offs_d, maxlen, int(len(flat)), seq_host=seq)
    ob = b_.step_device(x, seq_d, flat_d, offs_d, maxlen, int(len(flat)))
    assert oa["cr_frames"] == ob["cr_frames"] == 28
    assert abs(oa["loss"] - ob["loss"]) <= BAR * max(1.0, abs(ob["loss"]))
    assert a.specaug_frames == 56 and b_.specaug_frames == 0


# ----------------------------------------------------------------------------------------------- 7. the command line
def _run(cli, *args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", cli)] + list(args), capture_output=True, timeout=300)
    return r.returncode, r.stderr.decode()


def test_cli_trains_with_consistency_weight_and_reports(tmp_path):
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
    config.write_text("nnet_type = lstm\ninput_dim = 6\nleft_context = 1\nright_context = 1\nsubsample = 2\nnum_layers = 2\n"
                      "num_neurons = 32\nnum_projects = 16\nnum_targets = 9\nuse_peepholes = true\ndropout_rate = 1.0\n")
    d = str(tmp_path)
    rc, err = _run("nnet-init.py", "--objective=ctc", "--batch-size", "2", str(scp), str(config), d + "/nnet.0")
    assert rc == 0, err
    rc, err = _run("nnet-train.py", "--objective=ctc", "--batch-size", "2", "--learn-rate=0.01", "--optimizer=adam", "--seed=1",
                   "--shuffle=false", "--report-interval=1", "--evaluate=true", "--spec-augment", "time=2x10,freq=1x2,bins=3,cap=50",
                   "--consistency-weight", "0.2", str(scp), str(config), d + "/nnet.0", d + "/nnet.1")
    assert rc == 0, err
    report = [l for l in err.split("\n") if l.startswith("INFO:tensorflow:consistency weight ")]
    assert len(report) == 1, err
    m = re.fullmatch(r"INFO:tensorflow:consistency weight 0\.2: mean symmetric KL (\S+) per frame over (\d+) frame\(s\) of a pair, "
                     r"the argmaxes agree on (\S+)%", report[0])
    assert m, report[0]
    # four utterances in two batches; 10, 12, 15 and 20 rows after subsample = 2
    assert int(m.group(2)) == 10 + 12 + 15 + 20 and float(m.group(1)) > 0 and 0.0 <= float(m.group(3)) <= 100.0
    losses = [float(l.split()[-1]) for l in err.split("\n") if l.startswith("INFO:tensorflow:tr_loss = ")]
    assert losses and np.isfinite(losses).all(), err
    rates = [float(l.split("eval = ")[1]) for l in err.split("\n") if ", eval = " in l]        # view a over view a's labels
    assert len(rates) == 2 and np.isfinite(rates).all() and min(rates) > 0, err
    assert os.path.getsize(d + "/nnet.1") > 0


def test_zz_report_measured_error_over_bound():
    print("\nconsistency: largest measured error / derived bound: loss %.3f, grad %.3f; loss error / project bar %.4f"
          % (MEASURED["loss"], MEASURED["grad"], MEASURED["loss_bar"]))
    assert MEASURED["loss"] <= 1.0 and MEASURED["grad"] <= 1.0 and MEASURED["loss_bar"] <= 1.0
