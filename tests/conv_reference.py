"""float64 restatement of one layer of the convolutional front-end (include/lstm_ctc_hip.h, lc_conv_fwd / lc_conv_bwd;
DESIGN.md 3.20), for tests/test_conv_host.py and the GPU tests.  A helper, not a test.

x, dx: [T, B, Cin * F] (column ci * F + f with ``group_major``, else f * Cin + ci); y, dy: [T, B, Fo * Cout] (column
fo * Cout + co), Fo = ceil(F / 2); w: [3, 3, Cin, Cout] (time tap, bin tap, in, out); bias: [Cout]; seq_len: [B].
len_b = clamp(seq_len[b], 0, T), live(t, b) = t < len_b.  Kernel 3 x 3, time stride 1, frequency stride 2, zero padding 1, bias
and ReLU.  Dead rows never reach a result: they are selected away, not multiplied by zero, so NaN there changes nothing.

``bounds`` turns the same quantities into the error bounds the GPU tests assert.  The derivation: u = 2^-24 is fp32's unit
roundoff, and a sum of n fp32 terms in ANY order errs by at most (n - 1) u sum|terms| to first order, each product adding one
more u of its own.  So
  y:      n = 9 Cin products and the bias; ReLU is 1-Lipschitz:     |dy|  <= (9 Cin + 2) u (|bias| + sum |w| |xz|)
  dx:     at most 3 time taps x 2 bin taps x Cout products:          |ddx| <= (6 Cout + 2) u sum |w| |g|
  dw:     one product per live position (R = live frames x Fo):      |ddw| <= (R + 2) u sum |g| |xz|
  dbias:  one term per live position:                                |ddb| <= (R + 1) u sum |g|
all of it times a slack of 2 for the second-order terms (as tests/test_gpu_layer_norm.py).  Nothing depends on how the kernel
walks its sums, and nothing was fitted to what it returns."""
import numpy as np
import torch

U = 2.0 ** -24          # fp32 unit roundoff


def out_bins(F):
    return (F + 1) // 2


def lengths(seq_len, T):
    return np.clip(np.asarray(seq_len, np.int64), 0, T)


def live_rows(seq_len, T):
    """[T, B] bool."""
    return np.arange(T)[:, None] < lengths(seq_len, T)[None, :]


def to_bins(x, F, group_major):
    """[T, B, Cin * F] in either layout -> [T, B, F, Cin]."""
    T, B, D = x.shape
    Cin = D // F
    assert Cin * F == D
    return x.reshape(T, B, Cin, F).transpose(0, 1, 3, 2) if group_major else x.reshape(T, B, F, Cin)


def from_bins(x4, group_major):
    T, B, F, Cin = x4.shape
    return (x4.transpose(0, 1, 3, 2) if group_major else x4).reshape(T, B, Cin * F)


def _padded(x, F, group_major, live):
    """xz with one zero frame and one zero bin in front and behind (two bins behind where F is even is never needed):
    [T + 2, B, F + 2, Cin]."""
    x4 = np.where(live[:, :, None, None], to_bins(x, F, group_major), 0.0)          # dead rows: selected away
    return np.pad(x4, ((1, 1), (0, 0), (1, 1), (0, 0)))


def _taps(T, Fo):
    """(i, j, frame slice, bin slice) of the padded input under output (t, fo): frame t + i - 1, bin 2 fo + j - 1."""
    for i in range(3):
        for j in range(3):
            yield i, j, slice(i, i + T), slice(j, j + 2 * Fo - 1, 2)


def pre_activation(x, w, bias, seq_len, F, group_major=False):
    x, w, bias = (np.asarray(a, np.float64) for a in (x, w, bias))
    T, B, _ = x.shape
    Fo = out_bins(F)
    xp = _padded(x, F, group_major, live_rows(seq_len, T))
    pre = np.zeros((T, B, Fo, w.shape[3])) + bias
    for i, j, ts, fs in _taps(T, Fo):
        pre += xp[ts, :, fs, :] @ w[i, j]
    return pre


def fwd(x, w, bias, seq_len, F, group_major=False):
    """y = relu(bias + conv(xz, w)) in live rows, 0 in dead ones -> [T, B, Fo * Cout]."""
    T, B, _ = np.shape(x)
    live = live_rows(seq_len, T)
    pre = pre_activation(x, w, bias, seq_len, F, group_major)
    y = np.where(live[:, :, None, None], np.maximum(pre, 0.0), 0.0)
    return y.reshape(T, B, -1)


def gate(y, dy, seq_len):
    """g = dy where the row is live and y > 0, else 0 (selected, so NaN in dead rows of y and dy changes nothing)."""
    y, dy = np.asarray(y, np.float64), np.asarray(dy, np.float64)
    live = live_rows(seq_len, y.shape[0])
    with np.errstate(invalid="ignore"):
        return np.where(live[:, :, None] & (y > 0), dy, 0.0)


def bwd(x, y, dy, w, seq_len, F, group_major=False):
    """(dx [T, B, Cin * F] in x's layout, dw [3, 3, Cin, Cout], dbias [Cout]) from the SAME y the caller hands the kernel."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    T, B, _ = x.shape
    Fo, Cin, Cout = out_bins(F), w.shape[2], w.shape[3]
    live = live_rows(seq_len, T)
    g = gate(y, dy, seq_len).reshape(T, B, Fo, Cout)
    xp = _padded(x, F, group_major, live)
    dxp = np.zeros_like(xp)
    dw = np.zeros_like(w)
    for i, j, ts, fs in _taps(T, Fo):
        dw[i, j] = np.einsum("tbfc,tbfo->co", xp[ts, :, fs, :], g)
        dxp[ts, :, fs, :] += g @ w[i, j].T
    dx = np.where(live[:, :, None, None], dxp[1:T + 1, :, 1:F + 1, :], 0.0)
    return from_bins(dx, group_major), dw, g.sum(axis=(0, 1, 2))


def torch_conv(x, lens, w, bias, group_major=False):
    """The same forward on a float64 tensor [T, B, Cin * F], differentiable, through torch's own conv2d: for the float64 model
    compositions and for pinning ``fwd`` / ``bwd`` to torch.  F is the row width over w's Cin."""
    T, B, D = x.shape
    Cin, Cout = w.shape[2], w.shape[3]
    F = D // Cin
    live = (torch.arange(T)[:, None] < torch.as_tensor(np.asarray(lens)).clamp(0, T)[None, :])[:, :, None]
    xs = torch.where(live, x, torch.zeros_like(x))
    img = xs.reshape(T, B, Cin, F).permute(1, 2, 0, 3) if group_major else xs.reshape(T, B, F, Cin).permute(1, 3, 0, 2)
    out = torch.nn.functional.conv2d(img, w.permute(3, 2, 0, 1), bias, stride=(1, 2), padding=1)      # [B, Cout, T, Fo]
    out = torch.relu(out).permute(2, 0, 3, 1).reshape(T, B, -1)
    return torch.where(live, out, torch.zeros_like(out))


def bounds(x, y, dy, w, bias, seq_len, F, group_major=False, slack=2.0):
    """(tol_y, tol_dx, tol_dw, tol_dbias): elementwise bounds on |fp32 result - float64 reference| for ANY order of the sums
    (the module docstring derives them)."""
    x, w, bias = (np.asarray(a, np.float64) for a in (x, w, bias))
    T, B, _ = x.shape
    Fo, Cin, Cout = out_bins(F), w.shape[2], w.shape[3]
    live = live_rows(seq_len, T)
    xa = np.abs(_padded(x, F, group_major, live))
    ga = np.abs(gate(y, dy, seq_len)).reshape(T, B, Fo, Cout)
    wa = np.abs(w)
    mag_y = np.zeros((T, B, Fo, Cout)) + np.abs(bias)
    mag_dxp = np.zeros_like(xa)
    mag_dw = np.zeros_like(w)
    for i, j, ts, fs in _taps(T, Fo):
        mag_y += xa[ts, :, fs, :] @ wa[i, j]
        mag_dxp[ts, :, fs, :] += ga @ wa[i, j].T
        mag_dw[i, j] = np.einsum("tbfc,tbfo->co", xa[ts, :, fs, :], ga)
    R = int(live.sum()) * Fo
    tol_y = np.where(live[:, :, None, None], (9 * Cin + 2) * U * mag_y, 0.0).reshape(T, B, -1)
    tol_dx = from_bins(np.where(live[:, :, None, None], (6 * Cout + 2) * U * mag_dxp[1:T + 1, :, 1:F + 1, :], 0.0), group_major)
    tol_dw = (R + 2) * U * mag_dw
    tol_db = (R + 1) * U * ga.sum(axis=(0, 1, 2))
    tiny = 1e-30
    return tuple(slack * t + tiny for t in (tol_y, tol_dx, tol_dw, tol_db))
