"""lc_ctc_loss at every dispatch and length edge, lc_ctc_greedy at its group widths and chunk edges, against the float64 oracle.

Cases, batches and the restated dispatch: tests/test_ctc_edges_host.py.  Every lc_ctc_loss call here goes through ``run``, which
calls the C ABI itself and owns every buffer:

* logits are rows [1, T + 1) of a [T + 2, B, V] tensor whose first and last rows are NaN, so a read one row out of range
  stays inside this allocation (and would show as NaN wherever its value is used);
* loss, grad and the workspace each lie between two 4 KB guard bands of a fixed byte, checked after the call;
* loss and grad are NaN before the call and the workspace, of exactly lc_ctc_workspace_bytes bytes, is 0xFF bytes: every
  element must be written, and nothing may depend on what the workspace held.

After every call ``ops.last_ctc_path()`` must be the case's expected kernel geometry.

Tolerances, all the project's own: loss within 1e-4 max(|ref|, 1) of float64 (tests/conftest.py's bar) and no further from it
than 4 x the float32 oracle + 1e-3 (test_ctc_vs_oracle's check); gradient through ``check_grad`` at GRAD_TOL per utterance for
batches of T <= 128 (test_unconstrained_windows_reproduce_ctc_loss holds lc_ctc_loss to it at T ~ 110), and for longer ones
test_ctc_vs_oracle's bound over the whole batch, max < 2e-3 max(1, T / 300) and mean < 2e-5 (the float32 oracle is itself
3.3e-3 from float64 at T = 1100, L = 500, so it is no yardstick for the gradient there).  The largest measured / allowed
ratios per kernel geometry are printed by the last test and, with LC_MEASURED_DIR set, written to ctc_edges_measured.txt in
that directory (kept as profiles/ctc_edges_measured.txt)."""
import os

import numpy as np
import pytest
import torch

from conftest import GRAD_TOL, check_grad
from test_ctc_edges_host import (BLOCK_MAPPING, THREE_KERNEL_LONG, THREE_KERNEL_WIDE, TWO_LAUNCH_FEW, TWO_LAUNCH_MANY,
                                 WIDE_ALPHABET, Batch, Case, case_id, reference)
from test_gpu_ops import ctc_frame_stats, ops  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
LC_EINVAL, LC_EWORKSPACE = -1, -3
GUARD, PATTERN = 4096, 0x5A
MEASURED = {}                       # kernel geometry -> [largest loss error / bar, largest gradient error / bound]


# ----------------------------------------------------------------------------------------------- the harness
def _guarded(nbytes):
    buf = torch.full((2 * GUARD + nbytes,), PATTERN, dtype=torch.uint8, device="cuda")
    return buf, buf[GUARD:GUARD + nbytes]


def _intact(buf):
    return bool((buf[:GUARD] == PATTERN).all()) and bool((buf[-GUARD:] == PATTERN).all())


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(batch, want_grad=True, **override):
    """One lc_ctc_loss call on buffers of its own (module docstring) -> (return code, loss [B], grad [T,B,V] or None).
    ``override``: T, B, V, maxlen, nbytes passed to the library in place of the batch's."""
    from lstm_ctc_amd import _lib
    lib = _lib.load()
    T, B, V = batch.T, batch.B, batch.V
    xfull = torch.full((T + 2, B, V), float("nan"), device="cuda")
    xfull[1:T + 1] = _dev(batch.x)
    flat = _dev(batch.flat if len(batch.flat) else np.zeros(1, np.int32))
    offs, seq = _dev(batch.offs), _dev(batch.seq)
    nbytes = lib.lc_ctc_workspace_bytes(T, B, V, batch.Lmax)
    lbuf, loss = _guarded(4 * B)
    loss = loss.view(torch.float32).fill_(float("nan"))
    gbuf, grad = _guarded(4 * T * B * V)
    grad = grad.view(torch.float32).view(T, B, V).fill_(float("nan"))
    wbuf, ws = _guarded(nbytes)
    ws.fill_(0xFF)
    a = dict(T=T, B=B, V=V, maxlen=batch.Lmax, nbytes=nbytes)
    a.update(override)
    rc = lib.lc_ctc_loss(xfull[1].data_ptr(), a["T"], a["B"], a["V"], flat.data_ptr(), offs.data_ptr(), seq.data_ptr(),
                         a["maxlen"], loss.data_ptr(), grad.data_ptr() if want_grad else None, ws.data_ptr(), a["nbytes"],
                         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert _intact(lbuf) and _intact(gbuf) and _intact(wbuf), "a guard band was written"
    if not want_grad:
        assert bool(torch.isnan(grad).all()), "grad = NULL, yet the buffer beside loss was written"
    return rc, loss.cpu().numpy().copy(), grad.cpu().numpy().copy() if want_grad else None


def check(tag, batch, loss, grad, ref, path):
    """Every utterance by the header's conventions, against the float64 oracle; ``grad`` may be None (loss-only call)."""
    l64, g64, _, l32, g32 = ref
    T, V = batch.T, batch.V
    assert not np.isnan(loss).any() and (grad is None or not np.isnan(grad).any()), tag
    m = MEASURED.setdefault("%s<%d,%d>" % (path["path"], path["ppl"], path["nw"]), [0.0, 0.0])
    for b, (Tb, labels, kind) in enumerate(batch.utts):
        gb = None if grad is None else grad[:, b]
        if gb is not None:
            assert np.array_equal(gb[Tb:].view(np.int32), np.zeros_like(gb[Tb:], np.int32)), (tag, b, "rows beyond seq_len")
        if kind in ("empty", "skipped"):
            assert loss[b] == 0.0 and (gb is None or not gb.any()), (tag, b, kind, loss[b])
            continue
        if kind == "infeasible":
            assert loss[b] == np.inf, (tag, b, loss[b])
            if gb is not None and T <= 128:
                check_grad(gb[:Tb], g64[:Tb, b], tag, "utt%d/softmax" % b)
            continue
        assert np.isfinite(loss[b]), (tag, b, loss[b])
        bar = GRAD_TOL * max(abs(l64[b]), 1.0)
        err = abs(float(loss[b]) - l64[b])
        m[0] = max(m[0], err / bar)
        assert err <= bar, (tag, b, Tb, len(labels), loss[b], l64[b])
        if gb is not None:
            assert np.abs(gb[:Tb].sum(axis=1)).max() <= V * GRAD_TOL, (tag, b, "live rows sum to 0")
            if T <= 128:
                den = max(float(np.abs(g64[:Tb, b]).max()), 1e-3)
                ratio = float(np.abs(gb[:Tb] - g64[:Tb, b]).max()) / (GRAD_TOL * den)
                if ratio > 0.5:
                    print("%s utt %d T_b %d L %d: grad err / bar %.3f (the float32 oracle's: %.3f)"
                          % (tag, b, Tb, len(labels), ratio, float(np.abs(g32[:Tb, b] - g64[:Tb, b]).max()) / (GRAD_TOL * den)))
                m[1] = max(m[1], ratio)
                check_grad(gb[:Tb], g64[:Tb, b], tag, "utt%d T_b %d L %d" % (b, Tb, len(labels)))
    if grad is not None and T > 128:
        bound = 2e-3 * max(1.0, T / 300)
        den = max(float(np.abs(g64).max()), 1e-3)
        diff = np.abs(grad - g64)
        print("%s: T %d  grad err max %.3e (bound %.3e) mean %.3e (bound 2e-5)" % (tag, T, diff.max(), bound, diff.mean()))
        m[1] = max(m[1], float(diff.max()) / bound)
        check_grad(grad, g64, tag, "batch", tol=bound / den)
        assert diff.mean() < 2e-5, (tag, diff.mean())
    fin = np.isfinite(l64)
    assert np.abs(loss[fin] - l64[fin]).max() <= 4 * np.abs(l32[fin] - l64[fin]).max() + 1e-3, tag


def run_case(ops, oracle, case, want_grad=True, lse2_option=None):
    batch = Batch(case)
    ref = reference(oracle, batch)
    rc, loss, grad = run(batch, want_grad)
    assert rc == 0, ops._lib.load().lc_last_error()
    path = ops.last_ctc_path()
    assert path == batch.expected(want_grad, lse2_option), (case, path)
    check(case_id(case), batch, loss, grad, ref, path)
    return batch, loss, grad


# ----------------------------------------------------------------------------------------------- the case table
@pytest.mark.parametrize("case", TWO_LAUNCH_FEW, ids=case_id)
def test_two_launch_few_utterances(ops, oracle, case, ctc_frame_stats):
    run_case(ops, oracle, case, lse2_option=1 if ctc_frame_stats == "in_phase_2" else None)


@pytest.mark.parametrize("case", BLOCK_MAPPING + TWO_LAUNCH_MANY + THREE_KERNEL_WIDE + THREE_KERNEL_LONG, ids=case_id)
def test_table_case(ops, oracle, case):
    batch, _, _ = run_case(ops, oracle, case)
    if case.B == 512:
        assert ops.last_ctc_path()["lse2"] and ops.get_option("ctc_lse2") is None      # by default, no option set


@pytest.mark.parametrize("want_grad", [True, False], ids=["grad", "loss_only"])
@pytest.mark.parametrize("case", WIDE_ALPHABET, ids=case_id)
def test_wide_alphabet(ops, oracle, case, want_grad):
    """V = 4100 is past the 64 KB of LDS ctc_grad_kernel may take without asking (16 V bytes); V = 10240 is the limit the
    header states with a gradient.  Both return the right values."""
    run_case(ops, oracle, case, want_grad=want_grad)


def test_refusals_launch_nothing(ops, oracle):
    batch = Batch(TWO_LAUNCH_FEW[3])                                        # (1, 44)
    untouched = lambda loss, grad: np.isnan(loss).all() and np.isnan(grad).all()
    for kw in (dict(maxlen=1024), dict(T=0), dict(B=0), dict(V=1)):
        rc, loss, grad = run(batch, **kw)
        assert rc == LC_EINVAL and untouched(loss, grad), kw
    nbytes = ops._lib.load().lc_ctc_workspace_bytes(batch.T, batch.B, batch.V, batch.Lmax)
    rc, loss, grad = run(batch, nbytes=nbytes - 1)
    assert rc == LC_EWORKSPACE and untouched(loss, grad)
    assert ops._lib.load().lc_last_error().decode().startswith("lc_ctc_loss: workspace too small")
    # one class past the header's limit with a gradient: refused before any launch; the loss alone has no such limit
    wide = Batch(Case(2, 10241, 3, 6, "three_kernel", 1, 1))
    rc, loss, grad = run(wide)
    assert rc == LC_EINVAL and untouched(loss, grad)
    rc, loss, _ = run(wide, want_grad=False)
    assert rc == 0
    check("V10241 loss only", wide, loss, None, reference(oracle, wide), ops.last_ctc_path())
    rc, loss, grad = run(batch)
    assert rc == 0 and not np.isnan(loss).any() and not np.isnan(grad).any()


def test_cached_workspace_state_is_ignored(ops, oracle):
    """ops.ctc_loss keeps one workspace per stream: (1, 2) right after (127, 128) runs on what the larger call left there, and
    must give, bit for bit, what it gives on a workspace of 0xFF bytes."""
    big, small = Batch(TWO_LAUNCH_FEW[-1]), Batch(TWO_LAUNCH_FEW[2])
    assert (big.Lmax, big.V, small.Lmax, small.V) == (127, 128, 1, 2)
    for b in (big, small):
        loss, grad = ops.ctc_loss(_dev(b.x), _dev(b.flat), _dev(b.offs), _dev(b.seq), b.Lmax)
        loss, grad = loss.cpu().numpy(), grad.cpu().numpy()
        assert ops.last_ctc_path() == b.expected()
    rc, hloss, hgrad = run(small)
    assert rc == 0
    assert np.array_equal(loss.view(np.int32), hloss.view(np.int32))
    assert np.array_equal(grad.view(np.int32), hgrad.view(np.int32))
    check("stale workspace", small, loss, grad, reference(oracle, small), ops.last_ctc_path())


# ----------------------------------------------------------------------------------------------- greedy decode
@pytest.mark.parametrize("i,V", list(enumerate([2, 16, 17, 32, 33, 64, 65, 200])))
def test_greedy_group_widths_and_chunk_edges(ops, oracle, i, V):
    """Both group widths of the row statistics (16 lanes for V <= 32, else 64) and its strided loop (V > 64); the collapse
    kernel walks T = 600 in chunks of 256 frames: a token that straddles 255|256 or 511|512 is emitted once, two different
    ones there are both kept (utterance 0 carries the one plant and utterance 1 the other, swapping with ``i``)."""
    rng = np.random.RandomState(V)
    T, B, blank = 600, 5, V - 1
    seq_len = np.array([600, 257, 256, 1, 0], np.int32)
    x = rng.randn(T, B, V).astype(np.float32)
    x[:, :, blank] += 2.0
    other = 1 if V >= 3 else blank                           # a one-symbol alphabet has no second token

    def plant(b, t, same):
        x[t - 1:t + 1, b, :] = -1.0
        x[t - 1, b, 0] = 9.0
        x[t, b, 0 if same else other] = 9.0

    for t in (256, 512):
        plant(0, t, i % 2 == 0)
    plant(1, 256, i % 2 == 1)
    x[:, 2, blank] = 50.0                                    # all blank, exactly one chunk long
    x[5:40, 0, :] = 0.25                                     # a whole row tied: class 0
    j, k = V // 3, (2 * V) // 3                              # two tied maxima (for V > 64 in different strides of the loop)
    x[50:60, 0, :] = -1.0
    x[50:60, 0, [j, k]] = 3.0
    x[60:70, 1, :] = np.float32(1.0)
    rt, rn, _ = oracle.ctc_greedy(x, seq_len)
    assert rn[2] == 0 and rn[4] == 0 and rn[0] > 20 and rn[3] <= 1
    tok, n = ops.ctc_greedy(_dev(x), _dev(seq_len))
    tok, n = tok.cpu().numpy(), n.cpu().numpy()
    assert np.array_equal(n, rn), (n, rn)
    for b in range(B):
        assert np.array_equal(tok[b, :n[b]], rt[b, :rn[b]]), b


# ----------------------------------------------------------------------------------------------- report
def test_zz_report_measured_ratios():
    lines = ["# lc_ctc_loss, tests/test_gpu_ctc_edges.py: largest measured error / allowed, per kernel geometry <PPL, NW>",
             "# loss: |loss - float64| / (1e-4 max(|float64|, 1));  grad: T <= 128: max error / (1e-4 max |grad_ref|) per",
             "# utterance, longer batches: max error / (2e-3 max(1, T / 300)) over the batch"]
    lines += ["%-22s loss %.4f  grad %.4f" % (k, v[0], v[1]) for k, v in sorted(MEASURED.items())]
    print("\n" + "\n".join(lines))
    out = os.environ.get("LC_MEASURED_DIR")              # where to keep the table; unset: printed only
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "ctc_edges_measured.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
    assert MEASURED and all(v[0] <= 1.0 and v[1] <= 1.0 for v in MEASURED.values())
