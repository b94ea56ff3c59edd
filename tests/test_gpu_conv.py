"""GPU tests of lc_conv_fwd / lc_conv_bwd through ops.conv_fwd / ops.conv_bwd, against
tests/conv_reference.py: float64, evaluated on the same fp32 inputs.  The backward test hands the kernel's own fp32 y to the
kernel and to the reference, so the ReLU mask is the same set on both sides.

The error bounds (conv_reference.bounds) are derived in that module's docstring from u = 2^-24 and the reduction lengths; they
hold for any order of the sums.  Largest observed error / bound over the cases below, measured on one MI355X: DESIGN.md 3.20."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import conv_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 7.25
GUARD = 64
BINS = (1, 2, 5, 8, 40, 41)
CINS = (1, 3, 8, 32)
COUTS = (8, 32, 64)
WINDOWS = ("dense", "pitched", "unaligned")
# (T, lengths): 0, 1, T and above T among them; B of 1 to 5, so that rows t - 1 and t + 1 of another utterance are adjacent
BATCHES = ((1, (1,)), (1, (1, 0, 4)), (2, (2, 1, 0, 5)), (7, (7, 1, 0, 9, 4)), (7, (3, 7)), (2, (-1, 2, 2)))


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


def _data(seed, T, B, F, Cin, Cout, lens, nan_dead=True):
    rng = np.random.default_rng(seed)
    Fo = ref.out_bins(F)
    x = rng.normal(0.2, 1.0, size=(T, B, Cin * F)).astype(np.float32)
    dy = rng.normal(size=(T, B, Fo * Cout)).astype(np.float32)
    w = (rng.normal(size=(3, 3, Cin, Cout)) / np.sqrt(3.0 * Cin)).astype(np.float32)
    bias = rng.normal(0.0, 0.5, size=Cout).astype(np.float32)
    if nan_dead:
        dead = ~ref.live_rows(lens, T)
        x[dead] = np.nan
        dy[dead] = np.nan
    return x, dy, w, bias


def _bits(t):
    return t.contiguous().view(torch.int32)


RATIOS = {}


def _check(tag, kind, got, want, tol):
    err = np.abs(got.astype(np.float64) - want)
    ratio = float((err / tol).max())
    RATIOS[kind] = max(RATIOS.get(kind, 0.0), ratio)
    print("%s %s: max error %.3e, largest error / bound %.3f (largest so far %.3f)" % (tag, kind, err.max(), ratio, RATIOS[kind]))
    assert np.isfinite(got).all() and ratio <= 1.0, (tag, kind, ratio, float(err.max()))


def _run(T, lens, F, Cin, Cout, gm, layout="dense", seed=0, data=None):
    """Both passes on one case, checked against the reference -> dict of the device results."""
    from lstm_ctc_amd import ops
    B, Fo = len(lens), ref.out_bins(F)
    x, dy, w, bias = data if data is not None else _data(seed, T, B, F, Cin, Cout, lens)
    sl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    xv, _ = _window(T * B, Cin * F, layout, x)
    dyv, _ = _window(T * B, Fo * Cout, layout, dy)
    yv, ybuf = _window(T * B, Fo * Cout, layout)
    dxv, dxbuf = _window(T * B, Cin * F, layout)
    wd, bd = torch.from_numpy(w).cuda(), torch.from_numpy(bias).cuda()
    tag = "T=%d B=%d F=%d Cin=%d Cout=%d gm=%d %s" % (T, B, F, Cin, Cout, gm, layout)
    out = ops.conv_fwd(xv, wd, bd, sl, T, B, F, gm, out=yv)
    torch.cuda.synchronize()
    assert out is yv and _untouched_outside(yv, ybuf)
    dead = torch.from_numpy(~ref.live_rows(lens, T).reshape(-1)).cuda()
    assert int(_bits(yv[dead]).abs().sum()) == 0                                             # +0, bit for bit
    y_h = yv.cpu().numpy().reshape(T, B, Fo * Cout)
    # the kernel's own y, its dead rows poisoned, goes to the backward pass and to the reference
    y_poison = y_h.copy()
    y_poison[~ref.live_rows(lens, T)] = np.nan
    yv.copy_(torch.from_numpy(y_poison.reshape(T * B, -1)))
    tol = ref.bounds(x, y_poison, dy, w, bias, lens, F, gm)
    _check(tag, "y", y_h, ref.fwd(x, w, bias, lens, F, gm), tol[0])
    dx, dw, db = ops.conv_bwd(xv, yv, dyv, wd, sl, T, B, F, gm, dx=dxv)
    torch.cuda.synchronize()
    assert dx is dxv and _untouched_outside(dxv, dxbuf)
    assert int(_bits(dxv[dead]).abs().sum()) == 0
    want_dx, want_dw, want_db = ref.bwd(x, y_poison, dy, w, lens, F, gm)
    _check(tag, "dx", dxv.cpu().numpy().reshape(T, B, Cin * F), want_dx, tol[1])
    _check(tag, "dw", dw.cpu().numpy(), want_dw, tol[2])
    _check(tag, "dbias", db.cpu().numpy(), want_db, tol[3])
    return dict(x=xv, y=yv, dy=dyv, dx=dxv, dw=dw, dbias=db, w=wd, bias=bd, sl=sl)


# ---------------------------------------------------------------------------------------------- 1. every shape, pitch and path
@pytest.mark.parametrize("Cout", COUTS)
@pytest.mark.parametrize("Cin", CINS)
@pytest.mark.parametrize("F", BINS)
def test_both_passes_against_the_float64_reference(F, Cin, Cout):
    """Every (F, Cin, Cout) in both input layouts; the batch (T, lengths) and the window (dense, pitched, unaligned) rotate
    through the cases so that each appears with every F, Cin and Cout.  F: one bin (only the centre and one side tap), 2, odd
    (5, 41: the last output bin has no right neighbour), 8, and 40 / 41, which take more than one tile of bins at Cout = 64;
    Cin: below one vector (1, 3), one chunk of the reduction (8), four (32); Cout: 2, 8 and 16 threads per position."""
    k = BINS.index(F) + 2 * CINS.index(Cin) + 3 * COUTS.index(Cout)
    for gm in (False, True):
        T, lens = BATCHES[(k + 3 * gm) % len(BATCHES)]
        _run(T, lens, F, Cin, Cout, gm, WINDOWS[(k + gm) % 3], seed=k)


@pytest.mark.parametrize("layout", WINDOWS)
@pytest.mark.parametrize("gm", (False, True))
@pytest.mark.parametrize("batch", range(len(BATCHES)))
def test_every_batch_in_every_window(batch, gm, layout):
    T, lens = BATCHES[batch]
    _run(T, lens, 5, 3, 8, gm, layout, seed=batch)
    _run(T, lens, 8, 8, 32, gm, layout, seed=batch)


@pytest.mark.parametrize("gm", (False, True))
def test_eight_utterances_side_by_side_in_a_tile(gm):
    """Cout = 8 leaves 64 positions to a tile and F = 16 has 8 output bins: 8 utterances lie side by side in one tile of the
    forward pass and of the input gradient (Cin = 3: one thread per position) - the most a tile takes and its largest LDS
    footprint; B = 11 adds a second, partial group of utterances, T = 9 a second segment of frames."""
    _run(9, (9, 1, 0, 12, 4, 8, 9, 2, 5, 0, 7), 16, 3, 8, gm, "pitched", seed=4)


def test_more_tiles_than_one_pass_of_the_grid():
    """Cout = 64 puts 16 positions in a tile, so the 17 output bins of F = 33 take two tiles: T = 12, B = 400 are
    2 x 400 x 2 = 1600 tiles of the forward pass and 3 x 400 = 1200 of the input gradient (Cin = 32: 8 threads per position,
    one utterance's 17 positions a tile) - both beyond CONV_MAX_GROUPS, so workgroups walk a second tile - and 2 x 400 x 2
    tiles of the weight gradient, 7 to each of the CONV_DW_GROUPS / 4 workgroups of a chunk of input channels."""
    from lstm_ctc_amd import ops
    T, B = 12, 400
    assert -(-T // ops.CONV_FWD_FRAMES) * B * 2 > ops.CONV_MAX_GROUPS and -(-T // ops.CONV_DX_FRAMES) * B > ops.CONV_MAX_GROUPS
    assert -(-T // ops.CONV_DW_FRAMES) * B * 2 > ops.CONV_DW_GROUPS // 4
    rng = np.random.default_rng(1)
    lens = tuple(int(v) for v in rng.integers(0, T + 3, size=B))
    _run(T, lens, 33, 32, 64, False, "dense", seed=2)


# ---------------------------------------------------------------------------------------------- 2. properties
def test_dead_rows_are_never_read():
    T, lens, F, Cin, Cout = 7, (7, 1, 0, 9, 4), 5, 3, 8
    clean = _data(3, T, len(lens), F, Cin, Cout, lens, nan_dead=False)
    dirty = tuple(a.copy() for a in clean)
    dead = ~ref.live_rows(lens, T)
    dirty[0][dead] = np.nan
    dirty[1][dead] = np.nan
    for gm in (False, True):
        a, b = _run(T, lens, F, Cin, Cout, gm, data=clean), _run(T, lens, F, Cin, Cout, gm, data=dirty)
        live = torch.from_numpy(~dead.reshape(-1)).cuda()
        assert torch.equal(_bits(a["y"][live]), _bits(b["y"][live]))
        for k in ("dx", "dw", "dbias"):
            assert torch.equal(_bits(a[k]), _bits(b[k])), k


def test_utterances_do_not_leak_into_each_other():
    """Each utterance of a batch alone (B = 1) gives the bits it gives inside the batch."""
    from lstm_ctc_amd import ops
    T, lens, F, Cin, Cout = 7, (7, 1, 0, 9, 4), 8, 3, 8
    x, dy, w, bias = _data(5, T, len(lens), F, Cin, Cout, lens)
    r = _run(T, lens, F, Cin, Cout, False, data=(x, dy, w, bias))
    B = len(lens)
    for b in range(B):
        sl = torch.tensor(lens[b:b + 1], dtype=torch.int32, device="cuda")
        xb = torch.from_numpy(np.ascontiguousarray(x[:, b])).cuda()
        yb = ops.conv_fwd(xb, r["w"], r["bias"], sl, T, 1, F)
        want = r["y"].reshape(T, B, -1)[:, b]
        live = torch.arange(T, device="cuda") < min(max(lens[b], 0), T)
        assert torch.equal(_bits(yb[live]), _bits(want[live]))
        dxb, _, _ = ops.conv_bwd(xb, yb, torch.from_numpy(np.ascontiguousarray(dy[:, b])).cuda(), r["w"], sl, T, 1, F,
                                 want_dparams=False)
        assert torch.equal(_bits(dxb), _bits(r["dx"].reshape(T, B, -1)[:, b]))


@pytest.mark.parametrize("gm", (False, True))
def test_the_centre_tap_on_the_diagonal_copies_relu_of_the_even_bins(gm):
    from lstm_ctc_amd import ops
    T, lens, F, C = 7, (7, 1, 0, 9, 4), 9, 8
    B, Fo = len(lens), ref.out_bins(F)
    x, _, _, _ = _data(7, T, B, F, C, C, lens)
    w = np.zeros((3, 3, C, C), np.float32)
    w[1, 1] = np.eye(C, dtype=np.float32)
    sl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    y = ops.conv_fwd(torch.from_numpy(x.reshape(T * B, -1)).cuda(), torch.from_numpy(w).cuda(), torch.zeros(C, device="cuda"), sl,
                     T, B, F, gm)
    live = ref.live_rows(lens, T)
    even = ref.to_bins(x, F, gm)[:, :, 0::2, :]                                            # [T, B, Fo, C]
    want = np.where(live[:, :, None, None], np.maximum(even, 0), 0).astype(np.float32).reshape(T * B, Fo * C)
    assert np.array_equal(y.cpu().numpy(), want)


@pytest.mark.parametrize("F,Cin,Cout,gm", [(5, 3, 8, True), (40, 32, 32, False), (41, 8, 64, False)])
def test_determinism_and_null_outputs(F, Cin, Cout, gm):
    from lstm_ctc_amd import ops
    T, lens = 7, (7, 1, 0, 9, 4)
    B = len(lens)
    r = _run(T, lens, F, Cin, Cout, gm, seed=F)
    y2 = ops.conv_fwd(r["x"], r["w"], r["bias"], r["sl"], T, B, F, gm)
    live = torch.from_numpy(ref.live_rows(lens, T).reshape(-1)).cuda()
    assert torch.equal(_bits(y2[live]), _bits(r["y"][live]))                                # (r["y"]: dead rows poisoned since)
    args = (r["x"], r["y"], r["dy"], r["w"], r["sl"], T, B, F, gm)
    dx2, dw2, db2 = ops.conv_bwd(*args)
    for got, first in ((dx2, r["dx"]), (dw2, r["dw"]), (db2, r["dbias"])):                  # the same input, the same bits
        assert torch.equal(_bits(got), _bits(first))
    dx3, dw3, db3 = ops.conv_bwd(*args, want_dparams=False)
    assert dw3 is None and db3 is None and torch.equal(_bits(dx3), _bits(r["dx"]))
    dx4, dw4, db4 = ops.conv_bwd(*args, want_dx=False)
    assert dx4 is None and torch.equal(_bits(dw4), _bits(r["dw"])) and torch.equal(_bits(db4), _bits(r["dbias"]))


# ---------------------------------------------------------------------------------------------- 3. refusals
def test_bad_arguments_and_a_short_workspace_return_their_codes_and_touch_nothing():
    from lstm_ctc_amd import _lib
    lib = _lib.load()
    T, B, F, Cin, Cout = 5, 3, 5, 3, 8
    rows, Fo = T * B, 3
    Cx, Cy = Cin * F, Fo * Cout
    mk = lambda n: torch.full((n,), SENTINEL, dtype=torch.float32, device="cuda")
    big = 4096 * rows
    x, y, dy, dx = mk(big), mk(big), mk(big), mk(big)
    w, bias, dw, dbias = mk(9 * 64 * 72), mk(128), mk(9 * 64 * 72), mk(128)
    sl = torch.tensor((5, 2, 0), dtype=torch.int32, device="cuda")
    nbytes = lib.lc_conv_workspace_bytes(T, B, F, Cin, Cout)
    assert nbytes > 0 and lib.lc_conv_workspace_bytes(T, B, F, Cin, 12) == 0 and lib.lc_conv_workspace_bytes(T, B, 513, Cin, Cout) == 0
    ws = torch.zeros(max(lib.lc_conv_workspace_bytes(T, B, 512, 64, 64), 256), dtype=torch.uint8, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    off = lambda t, n: ctypes.c_void_p(t.data_ptr() + 4 * n)

    def fwd(T=T, B=B, F=F, Cin=Cin, Cout=Cout, ldx=Cx, ldy=Cy, x_=None, w_=None, b_=None, sl_=None, y_=None):
        g = lambda v, t: p(t) if v is None else v
        return lib.lc_conv_fwd(g(x_, x), ldx, 1, g(w_, w), g(b_, bias), T, B, F, Cin, Cout, g(sl_, sl), g(y_, y), ldy, None)

    def bwd(T=T, B=B, F=F, Cin=Cin, Cout=Cout, ldx=Cx, ldy=Cy, lddy=Cy, lddx=Cx, dx_=None, dw_=None, db_=None, y_=None, wb=nbytes):
        g = lambda v, t: p(t) if v is None else (None if v is False else v)
        return lib.lc_conv_bwd(p(x), ldx, 1, g(y_, y), ldy, p(dy), lddy, p(w), T, B, F, Cin, Cout, p(sl), g(dx_, dx), lddx,
                               g(dw_, dw), g(db_, dbias), p(ws), wb, None)

    null = ctypes.c_void_p(0)
    einval = [lambda: fwd(T=0), lambda: fwd(B=0), lambda: fwd(F=0), lambda: fwd(Cin=0), lambda: fwd(Cout=0), lambda: fwd(F=513, ldx=4096, ldy=4096),
              lambda: fwd(Cin=65, ldx=4096), lambda: fwd(Cout=72, ldy=4096), lambda: fwd(Cout=12, ldy=4096), lambda: fwd(ldx=Cx - 1),
              lambda: fwd(ldy=Cy - 1), lambda: fwd(x_=null), lambda: fwd(w_=null), lambda: fwd(b_=null), lambda: fwd(sl_=null),
              lambda: fwd(y_=null), lambda: fwd(y_=off(x, 4)), lambda: fwd(y_=off(w, 8)),
              lambda: bwd(T=-1), lambda: bwd(Cout=12, ldy=4096, lddy=4096), lambda: bwd(Cin=65, ldx=4096, lddx=4096, wb=ws.numel()),
              lambda: bwd(ldx=Cx - 1), lambda: bwd(ldy=Cy - 1), lambda: bwd(lddy=Cy - 1), lambda: bwd(lddx=Cx - 1), lambda: bwd(y_=null),
              lambda: bwd(dw_=False), lambda: bwd(db_=False), lambda: bwd(dx_=False, dw_=False, db_=False),
              lambda: bwd(dx_=off(x, Cx * (rows - 1))), lambda: bwd(dx_=off(dy, 4)), lambda: bwd(dx_=off(y, 4)),
              lambda: bwd(dw_=off(w, 4)), lambda: bwd(db_=off(dw, 4))]
    for i, call in enumerate(einval):
        assert call() == -1, i                                                          # LC_EINVAL
        assert b"lc_conv" in lib.lc_last_error()
    assert bwd(wb=nbytes - 1) == -3 and b"lc_conv_bwd" in lib.lc_last_error()           # LC_EWORKSPACE
    assert bwd(dx_=False, wb=0) == -3
    torch.cuda.synchronize()
    for t in (x, y, dy, dx, w, bias, dw, dbias):
        assert bool((t == SENTINEL).all())
    assert int(ws.sum()) == 0
    # ... and the same buffers with good arguments run (dx alone needs no workspace)
    assert fwd() == 0 and bwd() == 0 and bwd(dw_=False, db_=False, wb=0) == 0
    torch.cuda.synchronize()
    assert not bool((y[:rows * Cy] == SENTINEL).all()) and not bool((dw[:9 * Cin * Cout] == SENTINEL).all())
