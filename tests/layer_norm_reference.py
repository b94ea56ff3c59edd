"""float64 restatement of layer normalisation between the LSTM layers (include/lstm_ctc_hip.h, lc_layer_norm_fwd /
lc_layer_norm_bwd), for tests/test_layer_norm_host.py and the GPU tests.  A helper, not a test.

x, dy: [T, B, C]; gamma, beta: [C]; seq_len: [B].  len_b = clamp(seq_len[b], 0, T), live(t, b) = t < len_b.  Dead rows never
reach a result: they are selected away, not multiplied by zero, so NaN there changes nothing.  ``mask`` is the DropoutWrapper
factor per element ([T, B, C], from oracle.torch_f64.dropout_mask) or None for keep = 1.

``bounds`` turns the same quantities into the error bounds the GPU tests assert - derived there, evaluated here."""
import numpy as np
import torch

from oracle.torch_f64 import dropout_mask

EPS = 1e-5
U = 2.0 ** -24          # fp32 unit roundoff


def lengths(seq_len, T):
    return np.clip(np.asarray(seq_len, np.int64), 0, T)


def live_rows(seq_len, T):
    """[T, B] bool."""
    return np.arange(T)[:, None] < lengths(seq_len, T)[None, :]


def mask(seed, stream0, T, B, C, drop_width, keep):
    """[T, B, C] float64: column c takes stream stream0 + c // drop_width at index (t * B + b) * drop_width + c % drop_width -
    the concatenation of the [T, B, drop_width] masks of C // drop_width consecutive streams.  None for keep >= 1."""
    if keep >= 1.0:
        return None
    assert C % drop_width == 0
    return torch.cat([dropout_mask(seed, stream0 + q, T, B, drop_width, keep, "cpu") for q in range(C // drop_width)],
                     dim=2).numpy()


def _stats(x, live):
    xs = np.where(live[:, :, None], x, 0.0)                 # dead rows: selected away
    m = xs.mean(axis=2, keepdims=True)
    v = ((xs - m) ** 2).mean(axis=2, keepdims=True)
    rstd = 1.0 / np.sqrt(v + EPS)
    return xs, m, rstd, (xs - m) * rstd


def fwd(x, gamma, beta, seq_len, mask=None):
    """y = mask * (gamma * (x - m) / sqrt(v + eps) + beta) in live rows, 0 in dead ones; m, v over the C columns (v biased)."""
    x, gamma, beta = (np.asarray(a, np.float64) for a in (x, gamma, beta))
    live = live_rows(seq_len, x.shape[0])
    _, _, _, xh = _stats(x, live)
    y = gamma * xh + beta
    if mask is not None:
        y = y * mask
    return np.where(live[:, :, None], y, 0.0)


def bwd(x, dy, gamma, seq_len, mask=None):
    """(dx, dgamma, dbeta): with g = mask * dy, a = gamma * g: dx = rstd * (a - mean(a) - xh * mean(a * xh)) in live rows, 0 in
    dead ones; dgamma = sum over live rows of g * xh; dbeta = sum over live rows of g."""
    x, dy, gamma = (np.asarray(a, np.float64) for a in (x, dy, gamma))
    live = live_rows(seq_len, x.shape[0])
    _, _, rstd, xh = _stats(x, live)
    g = np.where(live[:, :, None], dy, 0.0)
    if mask is not None:
        g = g * mask
    a = gamma * g
    dx = rstd * (a - a.mean(axis=2, keepdims=True) - xh * (a * xh).mean(axis=2, keepdims=True))
    dx = np.where(live[:, :, None], dx, 0.0)
    return dx, (g * xh).sum(axis=(0, 1)), g.sum(axis=(0, 1))         # (xh and g are 0 in dead rows)


def torch_layer_norm(y, seq_len, gamma, beta, mask=None):
    """The same forward on a float64 tensor [T, B, C], differentiable, for the float64 model compositions."""
    T = y.shape[0]
    live = (torch.arange(T)[:, None] < torch.as_tensor(np.asarray(seq_len)).clamp(0, T)[None, :])[:, :, None]
    ys = torch.where(live, y, torch.zeros_like(y))
    m = ys.mean(dim=2, keepdim=True)
    v = ((ys - m) ** 2).mean(dim=2, keepdim=True)
    out = gamma * (ys - m) / torch.sqrt(v + EPS) + beta
    if mask is not None:
        out = out * torch.as_tensor(mask)
    return torch.where(live, out, torch.zeros_like(out))


def bounds(x, dy, gamma, beta, seq_len, mask=None, slack=2.0):
    """(tol_y, tol_dx, tol_dgamma, tol_dbeta): elementwise bounds on |fp32 result - float64 reference| for ANY order of the
    sums, from u = 2^-24, the reduction lengths and the magnitudes (derivation: tests/test_gpu_layer_norm.py's docstring).
    ``slack`` covers the second-order terms the derivation drops."""
    x, dy, gamma, beta = (np.asarray(a, np.float64) for a in (x, dy, gamma, beta))
    T, B, C = x.shape
    live = live_rows(seq_len, T)
    xs, m, rstd, xh = _stats(x, live)
    S = np.abs(xs).mean(axis=2, keepdims=True)
    f = np.ones_like(x) if mask is None else mask
    e_rstd = (C / 2.0 + 5) * U                                        # relative
    e_xh = (C + 1) * U * S * rstd + np.abs(xh) * (e_rstd + 2 * U)
    y = gamma * xh + beta
    tol_y = f * (np.abs(gamma) * e_xh + 2 * U * np.abs(y))
    g = np.where(live[:, :, None], dy, 0.0) * f
    a = gamma * g
    s1, s2 = a.mean(axis=2, keepdims=True), (a * xh).mean(axis=2, keepdims=True)
    e_a = 2 * U * np.abs(a)                                           # the mask's product and gamma's
    e_s1 = (C + 1) * U * np.abs(a).mean(axis=2, keepdims=True) + e_a.mean(axis=2, keepdims=True)
    e_s2 = ((C + 2) * U * np.abs(a * xh).mean(axis=2, keepdims=True) + (np.abs(a) * e_xh).mean(axis=2, keepdims=True)
            + (e_a * np.abs(xh)).mean(axis=2, keepdims=True))
    dx = rstd * (a - s1 - xh * s2)
    tol_dx = (rstd * (e_a + e_s1 + np.abs(xh) * e_s2 + np.abs(s2) * e_xh + 3 * U * (np.abs(a) + np.abs(s1) + np.abs(xh * s2)))
              + np.abs(dx) * (e_rstd + U))
    R = max(int(live.sum()), 1)
    tol_dgamma = (np.abs(g) * e_xh + 2 * U * np.abs(g * xh)).sum(axis=(0, 1)) + R * U * np.abs(g * xh).sum(axis=(0, 1))
    tol_dbeta = (U * np.abs(g)).sum(axis=(0, 1)) + R * U * np.abs(g).sum(axis=(0, 1))
    tiny = 1e-30
    return tuple(slack * t + tiny for t in (np.where(live[:, :, None], tol_y, 0.0), np.where(live[:, :, None], tol_dx, 0.0),
                                            tol_dgamma, tol_dbeta))
