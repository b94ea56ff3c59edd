"""GPU tests of the row convolution (csrc/row_conv.hip: lc_row_conv_fwd / lc_row_conv_bwd; nnet.config key row_conv_frames;
DESIGN.md 3.16).

Ops level, through ops, against tests/row_conv_reference.py (float64, pinned to torch autograd by tests/test_row_conv_host.py).
Every output is a window of a larger NaN-filled buffer; the dead rows of x and dy hold NaN.  Tolerances are derived, not measured:
  y, dx  (tau + 2) * 2^-24 * sum_j |w_j * x_j| per element: at most tau + 1 products, rounded once each or fused, and tau adds;
  dw     (n + 1) * 2^-24 * sum |terms|, n that element's number of live terms: the worst case of ANY fp32 summation order.
Model level: a tiny nnet_type = lstm model (2 layers of 16, V = 5, T = 12, B = 3, lengths 12, 7, 2) against the plain model with
the same seed - the identity filter, a pure shift, a random filter, the lookahead bound, batch norm, three training steps."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import row_conv_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -24

# (T, B, C, tau, pitch pad): pad 0 = pitches C + 8 at a 16-byte aligned offset (vector path), else C + pad (scalar path)
CASES = [
    (9, 3, 64, 2, 0),
    (9, 3, 64, 0, 0),              # tau = 0
    (3, 2, 64, 8, 0),              # the window is longer than the batch
    (12, 4, 6, 3, 3),              # pitches C + 3: scalar path
    (7, 1, 1028, 2, 0),            # 257 vectors: more than the 64 lanes of a column group, a ragged last group
    (5, 300, 8, 1, 0),             # many narrow rows
    (40, 5, 16, 32, 0),            # tau at the cap
    # The launcher's constants (csrc/row_conv.hip): C = 4 is one vector, so 4 lanes per item and 64 items per workgroup pass;
    # an item is ROWCONV_SEG = 8 frames of one utterance, so T = 3 gives B items; csrc/row_stream.h's RS_MAX_GROUPS = 2048
    # workgroups take 2048 * 64 = 131072 items in one pass - 132000 need the grid stride.  The 396000 rows cap at ROWCONV_SLABS = 512 dw slabs
    # of ceil(396000 / 512) = 774 rows, the last one with 486.
    (3, 132000, 4, 2, 0),
]
IDS = ["T%d_B%d_C%d_tau%d_pad%d" % c for c in CASES]


def _window(rows, C, pad, fill=None):
    """(whole buffer, [rows, C] window of it): NaN everywhere, or the window filled with `fill` (a numpy [rows, C])."""
    ld, off = (C + 8, 4) if pad == 0 else (C + pad, 1)
    big = torch.full((rows + 4, ld), float("nan"), dtype=torch.float32, device="cuda")
    win = big[2:2 + rows, off:off + C]
    if fill is not None:
        win.copy_(torch.from_numpy(np.ascontiguousarray(fill)).cuda())
    return big, win


def _outside_untouched(big, rows, C, pad):
    off = 4 if pad == 0 else 1
    m = torch.ones_like(big, dtype=torch.bool)
    m[2:2 + rows, off:off + C] = False
    return bool(torch.isnan(big[m]).all())


def _dw_window(tau, C):
    big = torch.full(((tau + 1) * C + 16,), float("nan"), dtype=torch.float32, device="cuda")
    return big, big[8:8 + (tau + 1) * C].view(tau + 1, C)


def _dw_outside_untouched(big, tau, C):
    return bool(torch.isnan(big[:8]).all()) and bool(torch.isnan(big[8 + (tau + 1) * C:]).all())


def _length_sets(T, B, tau):
    """Lengths 0, 1, tau, tau + 1, T and one above T (it must clip), dealt over the B utterances; a batch smaller than the six
    kinds takes several rounds, so that every case sees every kind."""
    kinds = [T, 0, 1, tau, tau + 1, T + 5]
    rounds = -(-len(kinds) // B)
    return [np.array([kinds[(r * B + b) % len(kinds)] for b in range(B)], np.int32) for r in range(rounds)]


def _inputs(case, seq_len, seed):
    T, B, C, tau, pad = case
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(T, B, C)).astype(np.float32)
    dy = rng.normal(size=(T, B, C)).astype(np.float32)
    w = rng.normal(size=(tau + 1, C)).astype(np.float32)
    n = ref.lengths(seq_len, T)
    dead = np.arange(T)[:, None] >= n[None, :]                       # [T, B]
    x[dead] = np.nan                                                  # a dead frame must never be read
    dy[dead] = np.nan
    return x, dy, w, dead


def _run(case, x, dy, w, seq_len, want_dx=True, want_dw=True):
    """-> dict of the GPU results (numpy) and of the buffers around them."""
    from lstm_ctc_amd import ops
    T, B, C, tau, pad = case
    _, xw = _window(T * B, C, pad, x.reshape(T * B, C))
    _, dyw = _window(T * B, C, pad, dy.reshape(T * B, C))
    wd = torch.from_numpy(w).cuda()
    sl = torch.from_numpy(seq_len).cuda()
    ybig, y = _window(T * B, C, pad)
    ops.row_conv_fwd(xw, wd, sl, T, B, out=y)
    dxbig, dx = _window(T * B, C, pad) if want_dx else (None, None)
    dwbig, dw = _dw_window(tau, C) if want_dw else (None, None)
    got_dx, got_dw = ops.row_conv_bwd(xw, dyw, wd, sl, T, B, want_dx=want_dx, want_dw=want_dw, dx=dx, dw=dw)
    assert (got_dx is dx if want_dx else got_dx is None) and (got_dw is dw if want_dw else got_dw is None)
    return dict(y=y, dx=dx, dw=dw, ybig=ybig, dxbig=dxbig, dwbig=dwbig, xw=xw, dyw=dyw, wd=wd, sl=sl)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_row_conv_against_the_reference(case):
    from lstm_ctc_amd import ops
    T, B, C, tau, pad = case
    for rnd, seq_len in enumerate(_length_sets(T, B, tau)):
        x, dy, w, dead = _inputs(case, seq_len, T * 131 + B + rnd)
        r = _run(case, x, dy, w, seq_len)
        y, dx, dw = (r[k].cpu().numpy() for k in ("y", "dx", "dw"))
        assert not np.isnan(y).any() and not np.isnan(dx).any() and not np.isnan(dw).any()
        y, dx = y.reshape(T, B, C), dx.reshape(T, B, C)
        # dead rows are +0, everything outside the windows is as it was
        for a in (y, dx):
            assert not a[dead].any() and not np.signbit(a[dead]).any()
        assert _outside_untouched(r["ybig"], T * B, C, pad) and _outside_untouched(r["dxbig"], T * B, C, pad)
        assert _dw_outside_untouched(r["dwbig"], tau, C)
        # the three formulas within the derived bounds
        err_y = np.abs(y - ref.fwd(x, w, seq_len))
        err_dx = np.abs(dx - ref.dx(dy, w, seq_len))
        tol_y = (tau + 2) * U * ref.fwd(x, w, seq_len, abs_terms=True)
        tol_dx = (tau + 2) * U * ref.dx(dy, w, seq_len, abs_terms=True)
        n = ref.counts(tau, seq_len, T)
        err_dw = np.abs(dw - ref.dw(x, dy, tau, seq_len))
        tol_dw = (n[:, None] + 1) * U * ref.dw(x, dy, tau, seq_len, abs_terms=True)
        print("%s lengths %s: y %.2e of its bound, dx %.2e, dw %.2e"
              % (IDS[CASES.index(case)], seq_len[:6].tolist(), (err_y / np.maximum(tol_y, 1e-300)).max(),
                 (err_dx / np.maximum(tol_dx, 1e-300)).max(), (err_dw / np.maximum(tol_dw, 1e-300)).max()))
        assert (err_y <= tol_y).all() and (err_dx <= tol_dx).all() and (err_dw <= tol_dw).all()
        assert not dw[n == 0].any()                                   # a kernel row without a live pair is written too: 0
        # the same call gives the same bits (and contiguous outputs)
        y2 = ops.row_conv_fwd(r["xw"], r["wd"], r["sl"], T, B)
        dx2, dw2 = ops.row_conv_bwd(r["xw"], r["dyw"], r["wd"], r["sl"], T, B)
        assert torch.equal(y2, r["y"]) and torch.equal(dx2, r["dx"]) and torch.equal(dw2, r["dw"])
        # dx alone and dw alone are what the call with both gives
        only = _run(case, x, dy, w, seq_len, want_dw=False)
        assert torch.equal(only["dx"], r["dx"]) and _outside_untouched(only["dxbig"], T * B, C, pad)
        only = _run(case, x, dy, w, seq_len, want_dx=False)
        assert torch.equal(only["dw"], r["dw"]) and _dw_outside_untouched(only["dwbig"], tau, C)


@pytest.mark.parametrize("case", CASES[:7], ids=IDS[:7])
def test_one_hot_kernel_copies_shifted_rows_exactly(case):
    T, B, C, tau, pad = case
    seq_len = _length_sets(T, B, tau)[0]
    n = ref.lengths(seq_len, T)
    for j0 in sorted({0, tau // 2, tau}):
        x, dy, w, dead = _inputs(case, seq_len, 7 * T + j0)
        w[:] = 0
        w[j0] = 1
        r = _run(case, x, dy, w, seq_len, want_dw=False)
        want_y, want_dx = np.zeros_like(x), np.zeros_like(dy)
        for b in range(B):
            if n[b] > j0:
                want_y[:n[b] - j0, b] = x[j0:n[b], b]                 # y[t] = x[t + j0] while t + j0 is live
                want_dx[j0:n[b], b] = dy[:n[b] - j0, b]               # dx[t] = dy[t - j0] from t = j0 on
        assert np.array_equal(r["y"].cpu().numpy().reshape(T, B, C), want_y), j0
        assert np.array_equal(r["dx"].cpu().numpy().reshape(T, B, C), want_dx), j0


BAD_FWD = {   # overrides of (x, ldx, w, T, B, C, tau, seq_len, y, ldy); "=x": the pointer of x
    "T0": dict(T=0), "B0": dict(B=0), "C0": dict(C=0), "Tneg": dict(T=-1), "tauneg": dict(tau=-1), "tau33": dict(tau=33),
    "null_x": dict(x=None), "null_w": dict(w=None), "null_len": dict(seq_len=None), "null_y": dict(y=None),
    "ldx_small": dict(ldx=7), "ldy_small": dict(ldy=7), "y_is_x": dict(y="x"), "y_in_x": dict(y="x+"),
}
BAD_BWD = {   # overrides of (x, ldx, dy, lddy, w, T, B, C, tau, seq_len, dx, lddx, dw, ws, nbytes)
    "T0": dict(T=0), "B0": dict(B=0), "C0": dict(C=0), "tauneg": dict(tau=-1), "tau33": dict(tau=33),
    "null_dy": dict(dy=None), "null_w": dict(w=None), "null_len": dict(seq_len=None), "null_x": dict(x=None),
    "null_dx_dw": dict(dx=None, dw=None), "ldx_small": dict(ldx=7), "lddy_small": dict(lddy=7), "lddx_small": dict(lddx=7),
    "dx_is_dy": dict(dx="dy"), "dx_in_dy": dict(dx="dy+"),
    "ws_null": dict(ws=None, rc=-3), "ws_short": dict(nbytes=-1, rc=-3), "ws_zero": dict(nbytes=0, rc=-3),
}


def _error_call(which, bad):
    """Calls the library with one bad argument on real buffers -> (rc, outputs), the outputs NaN-filled before the call."""
    from lstm_ctc_amd import _lib
    lib = _lib.load()
    T, B, C, tau = 6, 2, 8, 2
    need = lib.lc_row_conv_workspace_bytes(T, B, C, tau)
    t = dict(x=torch.randn((64, C), device="cuda"), dy=torch.randn((64, C), device="cuda"),
             w=torch.randn((tau + 1, C), device="cuda"), seq_len=torch.tensor([6, 4], dtype=torch.int32, device="cuda"),
             ws=torch.zeros(need, dtype=torch.uint8, device="cuda"))
    outs = {k: torch.full((64, C), float("nan"), device="cuda") for k in ("y", "dx", "dw")}
    a = dict(ldx=C, lddy=C, ldy=C, lddx=C, T=T, B=B, C=C, tau=tau, nbytes=need, rc=-1)
    a.update({k: v.data_ptr() for k, v in list(t.items()) + list(outs.items())})
    for k, v in bad.items():
        if isinstance(v, str):                       # an alias: the named input itself, or one row into it
            v = t[v.rstrip("+")].data_ptr() + (4 * C if v.endswith("+") else 0)
        elif k == "nbytes" and v < 0:
            v = need + v
        a[k] = v
    p = lambda v: None if v is None else ctypes.c_void_p(v)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    if which == "fwd":
        rc = lib.lc_row_conv_fwd(p(a["x"]), a["ldx"], p(a["w"]), a["T"], a["B"], a["C"], a["tau"], p(a["seq_len"]), p(a["y"]),
                                 a["ldy"], stream)
    else:
        rc = lib.lc_row_conv_bwd(p(a["x"]), a["ldx"], p(a["dy"]), a["lddy"], p(a["w"]), a["T"], a["B"], a["C"], a["tau"],
                                 p(a["seq_len"]), p(a["dx"]), a["lddx"], p(a["dw"]), p(a["ws"]), a["nbytes"], stream)
    torch.cuda.synchronize()
    assert rc == a["rc"], (rc, a["rc"])
    assert lib.lc_last_error()
    return outs, t


@pytest.mark.parametrize("bad", sorted(BAD_FWD))
def test_fwd_errors_touch_nothing(bad):
    outs, t = _error_call("fwd", BAD_FWD[bad])
    assert all(bool(torch.isnan(o).all()) for o in outs.values())
    assert not bool(torch.isnan(t["x"]).any())


@pytest.mark.parametrize("bad", sorted(BAD_BWD))
def test_bwd_errors_touch_nothing(bad):
    outs, t = _error_call("bwd", BAD_BWD[bad])
    assert all(bool(torch.isnan(o).all()) for o in outs.values())
    assert not bool(torch.isnan(t["dy"]).any()) and not bool(t["ws"].any())


# ================================================================================================ the model
T_, B_, D_, V_ = 12, 3, 6, 5
LENS = np.array([12, 7, 2], np.int32)


def _cfg(**kw):
    cfg = dict(nnet_type="lstm", input_dim=D_, left_context=0, right_context=0, num_layers=2, num_neurons=16,
               num_targets=V_, dropout_rate=1.0)
    cfg.update(kw)
    return cfg


def _model(cfg, kernel=None, seed=3):
    """A model whose biases matter; the same seed and the same bias draws give a plain and a row-convolution model the same
    shared parameters."""
    from lstm_ctc_amd.nnet.model import Model
    model = Model(cfg, "cuda", seed=seed)
    rng = np.random.default_rng(17)
    params = model.ps.export_tf()
    for k in sorted(params):
        if "bias" in k or k == "Variable_1":
            params[k] = rng.normal(0, 0.2, size=params[k].shape).astype(np.float32)
    if kernel is not None:
        params["row_conv/kernel"] = np.asarray(kernel, np.float32)
    model.ps.load_tf(params)
    return model


def _one_hot(tau, j0, H=16):
    w = np.zeros((tau + 1, H), np.float32)
    w[j0] = 1
    return w


def _batch(T=T_, lens=LENS, seed=5):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(T, len(lens), D_)).astype(np.float32)
    dl = rng.normal(size=(T, len(lens), V_)).astype(np.float32)
    for b, n in enumerate(lens):
        x[n:, b] = 0
        dl[n:, b] = 0                                # no loss sends gradient into padded frames
    return x, dl


def _forward(model, x, lens=LENS):
    return model.forward(torch.from_numpy(x).cuda(), torch.from_numpy(np.asarray(lens, np.int32)).cuda())


def _run_model(model, x, dl, lens=LENS):
    """-> (logits [T, B, V], the top the head read [T, B, H], gradients by name), all on the GPU."""
    logits = _forward(model, x, lens).clone()
    top = model.saved["top"].clone().view(x.shape[0], len(lens), -1)
    model.backward(torch.from_numpy(dl).cuda())
    grads = {n: model.ps.g(n).clone() for n in model.ps.names()}
    return logits, top, grads


@pytest.fixture(scope="module")
def plain():
    """The plain model's run, computed once and left unchanged."""
    x, dl = _batch()
    model = _model(_cfg())
    logits, top, grads = _run_model(model, x, dl)
    return dict(model=model, x=x, dl=dl, logits=logits, top=top, grads=grads)


def _live(lens=LENS, T=T_):
    return torch.from_numpy(np.arange(T)[:, None] < np.asarray(lens)[None, :]).cuda()


def test_identity_kernel_is_the_plain_model(plain):
    conv = _model(_cfg(row_conv_frames=2))
    assert conv.lookahead_horizon() == 2 and plain["model"].lookahead_horizon() is None
    w = conv.ps.p("row_conv/kernel")
    assert torch.equal(w[0], torch.ones_like(w[0])) and not bool(w[1:].any())
    logits, top, grads = _run_model(conv, plain["x"], plain["dl"])
    live = _live()
    assert torch.equal(logits[live], plain["logits"][live])
    for name, g in plain["grads"].items():
        assert torch.equal(grads[name], g), name
    assert bool(torch.isfinite(grads["row_conv/kernel"]).all()) and bool(grads["row_conv/kernel"].any())


# (the bf16 recurrences take N % 32 == 0 only - include/lstm_ctc_hip.h, lc_lstm_fwd_bf16 -, so that one case runs 32 units)
@pytest.mark.parametrize("kw", [dict(), dict(compute_dtype="bf16", num_neurons=32), dict(compute_dtype="bf16x3"),
                                dict(nnet_type="cudnnlstm")], ids=["fp32", "bf16", "bf16x3", "cudnnlstm"])
def test_shift_kernel_forward(kw):
    x, _ = _batch()
    base = _forward(_model(_cfg(**kw)), x).clone()
    conv = _model(_cfg(row_conv_frames=3, **kw), kernel=_one_hot(3, 2, H=_cfg(**kw)["num_neurons"]))
    logits = _forward(conv, x)
    bias = conv.ps.p("Variable_1")
    for b, n in enumerate(LENS):
        assert torch.equal(logits[:max(n - 2, 0), b], base[2:n, b]), b            # logits[t] = plain logits[t + 2]
        for t in range(max(n - 2, 0), n):
            assert torch.equal(logits[t, b], bias), (t, b)                          # nothing live to read: the head's bias


def _head_bounds(top, dl):
    """fp64 head gradients from an fp32 top and dlogits, with the (n + 1) * 2^-24 * sum |terms| bounds; n = live frames."""
    t64, d64 = top.reshape(-1, top.shape[-1]).astype(np.float64), dl.reshape(-1, dl.shape[-1]).astype(np.float64)
    n = int(LENS.sum())
    return t64.T @ d64, (n + 1) * U * (np.abs(t64).T @ np.abs(d64)), d64.sum(0), (n + 1) * U * np.abs(d64).sum(0)


def test_shift_kernel_backward(plain):
    x, dl = plain["x"], plain["dl"]
    conv = _model(_cfg(row_conv_frames=3), kernel=_one_hot(3, 2))
    _, top, grads = _run_model(conv, x, dl)
    shifted = np.zeros_like(dl)
    for b, n in enumerate(LENS):
        shifted[2:n, b] = dl[:max(n - 2, 0), b]                  # dlogits'[t] = dlogits[t - 2]; 0 for t < 2 and in dead frames
    _, _, want = _run_model(plain["model"], x, shifted)
    below = [n for n in plain["model"].ps.names() if n not in ("Variable", "Variable_1")]
    assert below
    for name in below:                                           # the rows of the top gradient hold the same values
        assert torch.equal(grads[name], want[name]), name
    # the head sums the same terms over rows in another order: the derived bound, against float64 sums
    gW, tolW, gb, tolb = _head_bounds(top.cpu().numpy(), dl)
    errW = np.abs(grads["Variable"].cpu().numpy() - gW)
    errb = np.abs(grads["Variable_1"].cpu().numpy() - gb)
    print("head weight %.2e of its bound, head bias %.2e" % ((errW / tolW).max(), (errb / tolb).max()))
    assert (errW <= tolW).all() and (errb <= tolb).all()
    gW2, tolW2, _, _ = _head_bounds(plain["top"].cpu().numpy(), shifted)          # the plain model on dlogits': the same terms
    assert (np.abs(gW - gW2) <= 1e-12 * np.abs(gW2).max()).all() and (np.abs(tolW - tolW2) <= 1e-12 * tolW2.max()).all()


def test_random_kernel_against_the_reference(plain):
    from conftest import check_grad
    tau = 3
    w = np.random.default_rng(23).normal(0, 0.5, size=(tau + 1, 16)).astype(np.float32)
    conv = _model(_cfg(row_conv_frames=tau), kernel=w)
    logits, top, grads = _run_model(conv, plain["x"], plain["dl"])
    p = {k: v.astype(np.float64) for k, v in conv.ps.export_tf().items()}
    top64 = ref.fwd(plain["top"].cpu().numpy(), w, LENS)
    want = top64 @ p["Variable"] + p["Variable_1"]
    got = logits.cpu().numpy()
    scale = np.abs(want).max()
    # tests/test_gpu_model.py:74 - the bar of a head product of this size against float64
    assert np.abs(got - want).max() < 1e-4 * max(scale, 1.0), np.abs(got - want).max()
    dtop = plain["dl"].astype(np.float64) @ p["Variable"].T                       # the gradient of the convolved tensor
    want_dw = ref.dw(plain["top"].cpu().numpy(), dtop, tau, LENS)
    # tests/test_gpu_model.py:92 - check_grad: 1e-4 of the tensor's largest gradient
    check_grad(grads["row_conv/kernel"].cpu().numpy(), want_dw, "row_conv/random", "row_conv/kernel")


def test_lookahead_bound_is_tau_frames():
    tau, t0 = 3, 4
    w = np.random.default_rng(29).normal(0, 0.5, size=(tau + 1, 16)).astype(np.float32)
    conv = _model(_cfg(row_conv_frames=tau), kernel=w)
    assert conv.lookahead_horizon() == 3
    x, _ = _batch()
    base = _forward(conv, x).clone()
    far = x.copy()
    far[t0 + tau + 1:, 0] += 1.0                                 # frames above t0 + 3 of utterance 0
    got = _forward(conv, far).clone()
    assert torch.equal(got[:t0 + 1, 0], base[:t0 + 1, 0])
    assert not torch.equal(got[t0 + 1, 0], base[t0 + 1, 0])      # ... which the next frame does read
    assert torch.equal(got[:, 1:], base[:, 1:])
    near = x.copy()
    near[t0 + tau, 0] += 1.0                                     # frame t0 + 3 itself
    got = _forward(conv, near)
    assert not torch.equal(got[t0, 0], base[t0, 0])
    assert torch.equal(got[:t0, 0], base[:t0, 0])


def test_batch_norm_top_does_not_leak_padding():
    """Inference with moving averages: the batch-normalised top is non-zero in dead frames, and utterance 0's logits must not
    depend on how far the batch is padded or on what the padding holds."""
    tau = 2
    w = np.random.default_rng(31).normal(0, 0.5, size=(tau + 1, 16)).astype(np.float32)
    conv = _model(_cfg(row_conv_frames=tau, use_bn=True, is_training=False), kernel=w)
    rng = np.random.default_rng(37)
    for name in conv.ps.aux:
        a = conv.ps.aux[name]
        vals = rng.uniform(0.5, 1.5, size=a.shape) if name.endswith("variance") else rng.normal(0, 0.3, size=a.shape)
        a.copy_(torch.from_numpy(vals.astype(np.float32)).cuda())
    x, _ = _batch()
    short = _forward(conv, x).clone()
    assert bool(conv.saved["pre_conv"].view(T_, B_, -1)[LENS[1]:, 1].any())       # the premise: dead frames are not zero
    wide = rng.normal(size=(20, B_, D_)).astype(np.float32)                        # arbitrary input in every dead frame
    for b, n in enumerate(LENS):
        wide[:n, b] = x[:n, b]
    long = _forward(conv, wide)
    assert torch.equal(long[:T_, 0], short[:, 0])
    for b, n in enumerate(LENS):
        assert torch.equal(long[:n, b], short[:n, b]), b


def test_training_moves_the_kernel_and_checkpoints_round_trip(tmp_path):
    from lstm_ctc_amd.nnet.graph import create_graph_for_training_ctc, create_graph_for_validation_ctc
    cfg = _cfg(row_conv_frames=2)
    graph = create_graph_for_training_ctc(None, cfg, learn_rate=1e-2, clip_norm=5.0, optimizer="adam", seed=11)
    rng = np.random.default_rng(41)
    x, _ = _batch()
    labels = np.full((B_, 4), -1, np.int64)
    for b, n in enumerate((4, 3, 1)):
        labels[b, :n] = rng.integers(0, V_ - 1, size=n)
    batch = {"nnet_input": np.ascontiguousarray(x.transpose(1, 0, 2)), "sequence_length": LENS.copy(), "nnet_target": labels}
    for _ in range(3):
        out = graph.step(batch, fetch_eval=True)
        assert np.isfinite(out["eval_loss"]) and np.isfinite(out["loss"]) and np.isfinite(out["grad_norm"])
    w = graph.model.ps.p("row_conv/kernel")
    assert bool(torch.isfinite(w).all()) and bool(w[1:].any()) and not torch.equal(w[0], torch.ones_like(w[0]))
    logits = _forward(graph.model, x).clone()
    path = str(tmp_path / "nnet.3")
    graph.save(path)
    fresh = create_graph_for_validation_ctc(None, cfg, seed=99)
    fresh.restore(path)
    assert torch.equal(fresh.model.ps.flat, graph.model.ps.flat)
    assert torch.equal(_forward(fresh.model, x), logits)
    # a plain model's checkpoint in a row-convolution graph: the plain logits
    plain_graph = create_graph_for_validation_ctc(None, _cfg(), seed=7)
    plain_logits = _forward(plain_graph.model, x).clone()
    plain_path = str(tmp_path / "plain.0")
    plain_graph.save(plain_path)
    fresh.restore(plain_path)
    live = _live()
    assert torch.equal(_forward(fresh.model, x)[live], plain_logits[live])
