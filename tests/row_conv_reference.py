"""float64 restatement of the row convolution's three formulas (include/lstm_ctc_hip.h, lc_row_conv_fwd / lc_row_conv_bwd), for
tests/test_row_conv_host.py and tests/test_gpu_row_conv.py.  A helper, not a test.

x, dy: [T, B, C]; w: [tau + 1, C]; seq_len: [B].  len_b = clamp(seq_len[b], 0, T), live(t, b) = t < len_b.  Dead frames never
reach a result: NaN there is masked away, not multiplied by zero.  ``abs_terms=True`` returns the sum of the terms' magnitudes
instead (for the derived tolerances), ``counts`` the number of live terms per dw element.  Loops run over t and j only; every
statement is the formula for all utterances at once."""
import numpy as np


def lengths(seq_len, T):
    return np.clip(np.asarray(seq_len, np.int64), 0, T)


def _masked(mask, term, abs_terms):
    term = np.where(mask[:, None], term, 0.0)
    return np.abs(term) if abs_terms else term


def fwd(x, w, seq_len, abs_terms=False):
    """y[t, b, c] = sum over j = 0 .. tau with live(t + j, b) of w[j, c] * x[t + j, b, c] if live(t, b), else 0."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    T, B, C = x.shape
    n = lengths(seq_len, T)
    y = np.zeros((T, B, C))
    for t in range(T):
        for j in range(min(w.shape[0], T - t)):
            y[t] += _masked(t + j < n, w[j] * x[t + j], abs_terms)          # live(t + j) implies live(t)
    return y


def dx(dy, w, seq_len, abs_terms=False):
    """dx[t, b, c] = sum over j = 0 .. min(tau, t) of w[j, c] * dy[t - j, b, c] if live(t, b), else 0."""
    dy, w = np.asarray(dy, np.float64), np.asarray(w, np.float64)
    T, B, C = dy.shape
    n = lengths(seq_len, T)
    out = np.zeros((T, B, C))
    for t in range(T):
        for j in range(min(w.shape[0], t + 1)):
            out[t] += _masked(t < n, w[j] * dy[t - j], abs_terms)
    return out


def dw(x, dy, tau, seq_len, abs_terms=False):
    """dw[j, c] = sum over b and over t with live(t + j, b) of dy[t, b, c] * x[t + j, b, c]."""
    x, dy = np.asarray(x, np.float64), np.asarray(dy, np.float64)
    T, B, C = x.shape
    n = lengths(seq_len, T)
    out = np.zeros((tau + 1, C))
    for j in range(min(tau + 1, T)):
        for t in range(T - j):
            out[j] += _masked(t + j < n, dy[t] * x[t + j], abs_terms).sum(axis=0)
    return out


def counts(tau, seq_len, T):
    """[tau + 1]: the number of live terms of dw[j, :]."""
    return np.array([sum(max(int(n) - j, 0) for n in lengths(seq_len, T)) for j in range(tau + 1)], np.int64)
