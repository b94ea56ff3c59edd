"""GPU tests of lc_layer_norm_fwd / lc_layer_norm_bwd through ops.layer_norm_fwd / ops.layer_norm_bwd, against
tests/layer_norm_reference.py: float64, evaluated on the same fp32 inputs.

The error bound (layer_norm_reference.bounds) is derived, not picked.  u = 2^-24 is fp32's unit roundoff; a sum of n fp32 terms
in ANY order errs by at most (n - 1) u sum|terms| (to first order), so nothing below depends on how the kernel walks a row.
Per live row, with S = mean_c |x|, rstd = 1 / sqrt(v + eps), xh = (x - m) rstd:
  m:     C - 1 additions and a division            |dm|    <= (C + 1) u S
  v:     the squares, their sum, the division and + eps: relative (C + 4) u; the error of m enters in second order only
         (sum_c (x - m) = 0), which is what makes the centred form robust - E[x^2] - m^2 errs by u m^2 in absolute terms
  rstd:  half of v's relative error, a square root and a division:     relative e_r = (C / 2 + 5) u
  xh:    |dxh|   <= (C + 1) u S rstd + |xh| (e_r + 2 u)
  y:     one fused multiply-add and the mask's product                 |dy|    <= f (|gamma| |dxh| + 2 u |y|), f the mask factor
  a = gamma g, g = f dy: two products                                  |da|    <= 2 u |a|
  s1 = mean a:      |ds1| <= (C + 1) u mean|a| + mean|da|
  s2 = mean a xh:   |ds2| <= (C + 2) u mean|a xh| + mean(|a| |dxh|) + mean(|da| |xh|)
  dx = rstd (a - s1 - xh s2):
         |ddx|   <= rstd (|da| + |ds1| + |xh| |ds2| + |s2| |dxh| + 3 u (|a| + |s1| + |xh s2|)) + |dx| (e_r + u)
  dgamma = sum over R live rows of g xh:  sum(|g| |dxh| + 2 u |g xh|) + R u sum|g xh|;   dbeta:  sum(u |g|) + R u sum|g|
all of it times a slack of 2 for the second-order terms.  The bound grows with S rstd, the row's offset in units of its spread:
that term is the rounding of the mean itself, which no fp32 kernel avoids.  Largest observed error / bound over the cases
below, measured on one MI355X: see DESIGN.md 3.18."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import layer_norm_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 7.25
GUARD = 64
WIDTHS = (1, 3, 4, 60, 256, 260, 2048, 2050, 8192)
LENGTHS = {"dense": (5, 2, 0), "pitched": (-3, 9, 4), "unaligned": (5, 2, 0)}


def _window(rows, C, layout, fill=None):
    """A [rows, C] fp32 view on the GPU inside a sentinel-filled buffer: pitch C (dense), C + 8 (pitched) or C + 5 from a base
    4 bytes off a 16-byte boundary (unaligned); with guard bands in front and behind.  -> (view, whole buffer)."""
    ld = {"dense": C, "pitched": C + 8, "unaligned": C + 5}[layout]
    off = GUARD + (1 if layout == "unaligned" else 0)
    flat = torch.full((off + rows * ld + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    view = flat.as_strided((rows, C), (ld, 1), off)
    assert (view.data_ptr() % 16 != 0) == (layout == "unaligned")
    if fill is not None:
        view.copy_(torch.from_numpy(np.ascontiguousarray(fill, dtype=np.float32).reshape(rows, C)))
    return view, flat


def _untouched_outside(view, flat):
    """Everything of the buffer that is not the [rows, C] window still holds the sentinel."""
    probe = flat.clone()
    probe.as_strided(view.shape, view.stride(), view.storage_offset()).fill_(SENTINEL)
    return bool((probe == SENTINEL).all())


def _data(seed, T, B, C, lens, nan_dead=True, offset=0.0):
    rng = np.random.default_rng(seed)
    x = (offset + rng.normal(0.5, 1.5, size=(T, B, C))).astype(np.float32)
    dy = rng.normal(size=(T, B, C)).astype(np.float32)
    gamma = rng.normal(1.0, 0.5, size=C).astype(np.float32)
    beta = rng.normal(size=C).astype(np.float32)
    if nan_dead:
        dead = ~ref.live_rows(lens, T)
        x[dead] = np.nan
        dy[dead] = np.nan
    return x, dy, gamma, beta


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check(tag, got, want, tol):
    err = np.abs(got.astype(np.float64) - want)
    ratio = float((err / tol).max())
    print("%s: max error %.3e, largest error / bound %.3f" % (tag, err.max(), ratio))
    assert np.isfinite(got).all() and ratio <= 1.0, (tag, ratio, float(err.max()))
    return ratio


def _run(T, B, C, lens, layout="dense", keep=1.0, dw=None, seed=0, data=None):
    """Both passes on one case, checked against the reference -> dict of the device results."""
    from lstm_ctc_amd import ops
    dw = C if dw is None else dw
    x, dy, gamma, beta = data if data is not None else _data(seed, T, B, C, lens)
    sl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    xv, _ = _window(T * B, C, layout, x)
    dyv, _ = _window(T * B, C, layout, dy)
    yv, ybuf = _window(T * B, C, layout)
    dxv, dxbuf = _window(T * B, C, layout)
    g, b = torch.from_numpy(gamma).cuda(), torch.from_numpy(beta).cuda()
    ops.layer_norm_fwd(xv, g, b, sl, T, B, keep, 11, 6, dw, out=yv)
    dx, dgamma, dbeta = ops.layer_norm_bwd(xv, dyv, g, sl, T, B, keep, 11, 6, dw, dx=dxv)
    torch.cuda.synchronize()
    assert dx is dxv and _untouched_outside(yv, ybuf) and _untouched_outside(dxv, dxbuf)
    m = ref.mask(11, 6, T, B, C, dw, keep)
    want_y = ref.fwd(x, gamma, beta, lens, m)
    want_dx, want_dg, want_db = ref.bwd(x, dy, gamma, lens, m)
    tol = ref.bounds(x, dy, gamma, beta, lens, m)
    tag = "C=%d %s keep=%g" % (C, layout, keep)
    y_h, dx_h = yv.cpu().numpy().reshape(T, B, C), dxv.cpu().numpy().reshape(T, B, C)
    _check(tag + " y", y_h, want_y, tol[0])
    _check(tag + " dx", dx_h, want_dx, tol[1])
    _check(tag + " dgamma", dgamma.cpu().numpy(), want_dg, tol[2])
    _check(tag + " dbeta", dbeta.cpu().numpy(), want_db, tol[3])
    dead = torch.from_numpy(~ref.live_rows(lens, T).reshape(-1)).cuda()
    assert int(_bits(yv[dead]).abs().sum()) == 0 and int(_bits(dxv[dead]).abs().sum()) == 0           # +0, bit for bit
    return dict(x=xv, dy=dyv, y=yv, dx=dxv, dgamma=dgamma, dbeta=dbeta, gamma=g, beta=b, sl=sl)


# ---------------------------------------------------------------------------------------------- 1. every width, pitch and path
@pytest.mark.parametrize("layout", sorted(LENGTHS))
@pytest.mark.parametrize("C", WIDTHS)
def test_both_passes_against_the_float64_reference(C, layout):
    """T = 5, B = 3; lengths {5, 2, 0} and {-3, 9, 4} (clamped to 0 and 5); dead rows of x and dy are NaN; pitches above C with
    guard bands that stay untouched; a base 4 bytes off a 16-byte boundary.  C: the scalar path (1, 3), one vector (4), a
    partial last pass of a 16-lane group (60), one full wave (256), 65 vectors (260), c4's width (2048), the scalar path at a
    large width (2050) and the cap (8192) - the last two with the backward's sums in LDS."""
    _run(5, 3, C, LENGTHS[layout], layout, seed=C)


def test_rows_beyond_one_pass_of_the_grid():
    """C = 8 takes 4 lanes a row, 64 rows per workgroup pass: more than LAYER_NORM_MAX_GROUPS * 64 rows reach the grid stride
    of the forward and give every workgroup of the backward more than one row group, hence the fold more than one partial
    per column."""
    from lstm_ctc_amd import ops
    B = 7
    T = ops.LAYER_NORM_MAX_GROUPS * ops.LAYER_NORM_MAX_ROWS_PER_GROUP // B + 10
    assert T * B > ops.LAYER_NORM_MAX_GROUPS * ops.LAYER_NORM_MAX_ROWS_PER_GROUP
    lens = (T, T - 1, T // 2, 3, 0, T + 5, T - 64)
    _run(T, B, 8, lens, "dense", seed=5)


# ---------------------------------------------------------------------------------------------- 2. properties
def test_dead_rows_are_never_read():
    from lstm_ctc_amd import ops
    T, B, C, lens = 5, 3, 60, (5, 2, 0)
    clean = _data(3, T, B, C, lens, nan_dead=False)
    dirty = tuple(a.copy() for a in clean)
    dead = ~ref.live_rows(lens, T)
    dirty[0][dead] = np.nan
    dirty[1][dead] = np.nan
    a, b = _run(T, B, C, lens, data=clean), _run(T, B, C, lens, data=dirty)
    for k in ("y", "dx", "dgamma", "dbeta"):
        assert torch.equal(_bits(a[k]), _bits(b[k])), k


def test_constant_rows_give_beta_and_finite_gradients():
    from lstm_ctc_amd import ops
    T, B, lens = 5, 3, (5, 2, 0)
    for C, value, exact in ((256, 1.5, True), (4, -3.0, True), (3, 0.1, False)):
        x, dy, gamma, beta = _data(4, T, B, C, lens)
        x[ref.live_rows(lens, T)] = value
        r = _run(T, B, C, lens, data=(x, dy, gamma, beta))                  # within the bound (rstd = 1 / sqrt(eps) here)
        live = torch.from_numpy(ref.live_rows(lens, T).reshape(-1)).cuda()
        if exact:                                                           # the mean of C equal powers-of-two multiples is exact
            assert torch.equal(r["y"][live], r["beta"].expand(int(live.sum()), C))
        assert bool(torch.isfinite(r["dx"]).all() and torch.isfinite(r["dgamma"]).all() and torch.isfinite(r["dbeta"]).all())


def test_a_far_offset_row_stays_within_the_bound_and_a_one_pass_variance_would_not():
    T, B, C, lens = 5, 3, 60, (5, 2, 0)
    rng = np.random.default_rng(6)
    x, dy, gamma, beta = _data(6, T, B, C, lens)
    live = ref.live_rows(lens, T)
    x[live] = (4096.0 + rng.uniform(-1, 1, size=(int(live.sum()), C))).astype(np.float32)
    _run(T, B, C, lens, data=(x, dy, gamma, beta))
    # the same rows through E[x^2] - m^2 in fp32 arithmetic: outside the bound (so the case tells the two forms apart)
    xs = x[live]
    m = xs.mean(axis=1, keepdims=True, dtype=np.float32)
    v1 = (xs * xs).mean(axis=1, keepdims=True, dtype=np.float32) - m * m
    with np.errstate(invalid="ignore", divide="ignore"):
        y1 = gamma * ((xs - m) / np.sqrt(v1 + np.float32(ref.EPS))) + beta
    tol = ref.bounds(x, dy, gamma, beta, lens)[0][live]
    err = np.abs(y1.astype(np.float64) - ref.fwd(x, gamma, beta, lens)[live])
    assert not np.all(np.nan_to_num(err, nan=np.inf) <= tol)


@pytest.mark.parametrize("C,dw", [(60, 60), (60, 30), (6, 6), (6, 3), (2048, 1024), (2050, 1025)])
def test_dropout_is_lc_dropout_scale_on_the_unmasked_output(C, dw):
    """keep < 1 over drop_width = C and C / 2 (two mask streams; 30 and 3 put a stream's edge inside a 16-byte vector):
    forward bit-identical to lc_dropout_scale applied to the keep = 1 output, window by window; backward against the
    reference with the same mask (inside _run)."""
    from lstm_ctc_amd import ops
    T, B, lens, keep = 5, 3, (5, 2, 0), 0.7
    data = _data(C + dw, T, B, C, lens, nan_dead=False)
    masked = _run(T, B, C, lens, keep=keep, dw=dw, data=data)
    plain = _run(T, B, C, lens, data=data)
    want = plain["y"].clone()
    for q in range(C // dw):
        ops.dropout_scale(want[:, q * dw:(q + 1) * dw], keep, 11, 6 + q)
    assert torch.equal(_bits(masked["y"]), _bits(want))
    assert not torch.equal(masked["y"], plain["y"])


@pytest.mark.parametrize("C", [60, 2048, 2050])
def test_determinism_aliasing_and_null_outputs(C):
    from lstm_ctc_amd import ops
    T, B, lens, keep = 5, 3, (5, 2, 0), 0.7
    r = _run(T, B, C, lens, keep=keep, dw=C // 2, seed=C)
    args = (r["x"], r["dy"], r["gamma"], r["sl"], T, B, keep, 11, 6, C // 2)
    dx2, dg2, db2 = ops.layer_norm_bwd(*args)
    for got, first in ((dx2, r["dx"]), (dg2, r["dgamma"]), (db2, r["dbeta"])):             # the same input, the same bits
        assert torch.equal(_bits(got), _bits(first))
    dx3, dg3, db3 = ops.layer_norm_bwd(*args, want_dparams=False)
    assert dg3 is None and db3 is None and torch.equal(_bits(dx3), _bits(r["dx"]))
    dx4, dg4, db4 = ops.layer_norm_bwd(*args, want_dx=False)
    assert dx4 is None and torch.equal(_bits(dg4), _bits(r["dgamma"])) and torch.equal(_bits(db4), _bits(r["dbeta"]))
    inplace = r["dy"].clone()
    inplace[torch.isnan(inplace)] = 0.0                                                   # (dead rows: any value)
    live_dy = inplace.clone()
    dx5, dg5, db5 = ops.layer_norm_bwd(r["x"], inplace, *args[2:], dx=inplace)
    assert dx5 is inplace and torch.equal(_bits(inplace), _bits(r["dx"])) and not torch.equal(inplace, live_dy)
    assert torch.equal(_bits(dg5), _bits(r["dgamma"])) and torch.equal(_bits(db5), _bits(r["dbeta"]))


# ---------------------------------------------------------------------------------------------- 3. refusals
def test_bad_arguments_return_einval_and_touch_nothing():
    from lstm_ctc_amd import _lib, ops
    lib = _lib.load()
    T, B, C = 5, 3, 8
    rows = T * B
    mk = lambda n: torch.full((n,), SENTINEL, dtype=torch.float32, device="cuda")
    big = 2 * 8196 * rows
    x, dy, y, dx = mk(big), mk(big), mk(big), mk(big)
    gamma, beta, dgamma, dbeta = mk(8196), mk(8196), mk(8196), mk(8196)
    sl = torch.tensor((5, 2, 0), dtype=torch.int32, device="cuda")
    nbytes = lib.lc_layer_norm_workspace_bytes(T, B, C)
    ws = torch.zeros(max(lib.lc_layer_norm_workspace_bytes(T, B, 8192), 256), dtype=torch.uint8, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    off = lambda t, n: ctypes.c_void_p(t.data_ptr() + 4 * n)

    def fwd(C=C, ldx=None, ldy=None, dw=None, y_=None):
        return lib.lc_layer_norm_fwd(p(x), C if ldx is None else ldx, p(gamma), p(beta), T, B, C, 1e-5, p(sl), 0.7, 1, 0,
                                     C if dw is None else dw, p(y) if y_ is None else y_, C if ldy is None else ldy, None)

    def bwd(C=C, ldx=None, lddy=None, lddx=None, dw=None, dx_=None, dg=True, db=True, wb=nbytes):
        ld = lambda v: C if v is None else v
        return lib.lc_layer_norm_bwd(p(x), ld(ldx), p(dy), ld(lddy), p(gamma), T, B, C, 1e-5, p(sl), 0.7, 1, 0, ld(dw),
                                     p(dx) if dx_ is None else dx_, ld(lddx), p(dgamma) if dg else None,
                                     p(dbeta) if db else None, p(ws), wb, None)

    calls = [lambda: fwd(C=8196), lambda: fwd(ldx=C - 1), lambda: fwd(ldy=C - 1), lambda: fwd(dw=3), lambda: fwd(y_=off(x, 4)),
             lambda: bwd(C=8196, wb=ws.numel()), lambda: bwd(ldx=C - 1), lambda: bwd(lddy=C - 1), lambda: bwd(lddx=C - 1),
             lambda: bwd(dw=3), lambda: bwd(dx_=off(dy, 4)), lambda: bwd(dx_=off(x, C * (rows - 1))), lambda: bwd(wb=nbytes - 1),
             lambda: bwd(dg=False), lambda: bwd(db=False)]
    for i, call in enumerate(calls):
        assert call() == -1, i                                                          # LC_EINVAL
        assert b"lc_layer_norm" in lib.lc_last_error()
    torch.cuda.synchronize()
    for t in (x, dy, y, dx, gamma, beta, dgamma, dbeta):
        assert bool((t == SENTINEL).all())
    assert int(ws.sum()) == 0
    # ... and the same buffers with good arguments run
    assert fwd() == 0 and bwd() == 0
    torch.cuda.synchronize()
    assert not bool((y[:rows * C] == SENTINEL).all()) and not bool((dgamma[:C] == SENTINEL).all())
