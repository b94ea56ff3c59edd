"""Restatement of the pyramidal BiLSTM - TEST INFRASTRUCTURE, not product code.

``np_time_reduce_fwd`` / ``np_time_reduce_bwd``: the statement of lc_time_reduce_fwd / lc_time_reduce_bwd in
include/lstm_ctc_hip.h as loops over (t, b).  ``pyramid_forward`` / ``pyramid_gradients``: the model in float64 on the CPU,
built from oracle/torch_f64.py's ``lstmp_forward``, ``reverse_sequence`` and ``dropout_mask`` the way ``blstm_forward`` is:
in front of each reduced layer, r consecutive frames of the layer below side by side (dead frames and the cut-short last
group zero), and from there on ceil(T / r) frames with lengths ceil(len / r); a layer's dropout masks hash the index at its own
frame count.  Gradients by autograd of sum(logits * dlogits).  tests/test_time_reduce_host.py pins this file to
``blstm_forward`` (key off) and to itself one utterance at a time (key on)."""
import numpy as np
import torch

from oracle.torch_f64 import dropout_mask, lstmp_forward, reverse_sequence


def cdiv(a, b):
    return -(-a // b)


def np_time_reduce_fwd(x, seq_len, r):
    """x [T, B, C] -> y [ceil(T / r), B, r * C]: y[to, b, j * C + c] = x[r * to + j, b, c] if r * to + j < len_b, else +0,
    len_b = clamp(seq_len[b], 0, T).  Dead frames of x are never read."""
    T, B, C = x.shape
    y = np.zeros((cdiv(T, r), B, r * C), x.dtype)
    for b in range(B):
        for t in range(min(max(int(seq_len[b]), 0), T)):
            y[t // r, b, (t % r) * C:(t % r + 1) * C] = x[t, b]
    return y


def np_time_reduce_bwd(dy, seq_len, r, T):
    """dy [ceil(T / r), B, r * C] -> dx [T, B, C]: dx[t, b, c] = dy[t // r, b, (t % r) * C + c] if t < len_b, else +0."""
    To, B, rC = dy.shape
    assert To == cdiv(T, r) and rC % r == 0
    C = rC // r
    dx = np.zeros((T, B, C), dy.dtype)
    for b in range(B):
        for t in range(min(max(int(seq_len[b]), 0), T)):
            dx[t, b] = dy[t // r, b, (t % r) * C:(t % r + 1) * C]
    return dx


def output_lengths(seq_len, layers, r):
    out = np.asarray(seq_len).astype(np.int64)
    for _ in layers:
        out = (out + r - 1) // r
    return out


def torch_time_reduce(x, sl, r):
    """The same re-lay on a float64 tensor, differentiable: [T, B, C] -> [ceil(T / r), B, r * C]."""
    T, B, C = x.shape
    To = cdiv(T, r)
    live = torch.arange(T)[:, None] < sl[None, :]
    x = torch.where(live[:, :, None], x, torch.zeros_like(x))
    if To * r > T:
        x = torch.cat([x, torch.zeros((To * r - T, B, C), dtype=x.dtype)], dim=0)
    return x.reshape(To, r, B, C).permute(0, 2, 1, 3).reshape(To, B, r * C)


def pyramid_forward(params, cfg, x_tbd, seq_len, layers, r, drop_seed=0):
    """Logits [T_L, B, V] float64 (CPU) of the plain-head BiLSTM of ``cfg`` whose layers ``layers`` read a reduced input."""
    assert not cfg.get("num_experts"), "plain head only"
    dtype, device = torch.float64, "cpu"

    def g(k):
        v = params.get(k)
        if v is None or torch.is_tensor(v):
            return v
        return torch.as_tensor(np.asarray(v, np.float64), device=device)

    x = torch.as_tensor(x_tbd).to(device=device, dtype=dtype)
    sl = torch.as_tensor(np.asarray(seq_len)).to(device=device, dtype=torch.int64)
    keep = 1.0 if not cfg.get("is_training", True) else float(cfg.get("dropout_rate", 1.0))
    T, B, D = x.shape
    finput = x
    for i in range(cfg["num_layers"]):
        if i in layers:
            finput = torch_time_reduce(finput, sl.clamp(0, T), r)
            sl = (sl.clamp(0, T) + r - 1) // r
            T = cdiv(T, r)
        halves = []
        for d, prefix in enumerate(("fd%d/frnn%d" % (i, i), "bd%d/brnn%d" % (i, i))):
            inp = finput if d == 0 else reverse_sequence(finput, sl)
            o = lstmp_forward(inp, sl, g(prefix + "/kernel"), g(prefix + "/bias"), g(prefix + "/w_f_diag"),
                              g(prefix + "/w_i_diag"), g(prefix + "/w_o_diag"), g(prefix + "/projection/kernel"), 5.0)
            if d == 1:
                o = reverse_sequence(o, sl)
            mask = dropout_mask(drop_seed, 2 * i + d, T, B, o.shape[2], keep, device, dtype)     # at this layer's own T
            halves.append(o if mask is None else o * mask)
        cat = torch.cat(halves, dim=2)
        finput = finput + cat if (i == 0 and D == cat.shape[2]) else cat
    return (finput.reshape(T * B, -1) @ g("Variable") + g("Variable_1")).reshape(T, B, -1)


def pyramid_gradients(params, cfg, x_tbd, seq_len, dlogits_tbv, layers, r, drop_seed=0):
    """(logits float64 [T_L, B, V], {TF variable name: numpy float64 gradient of sum(logits * dlogits)})."""
    leaves = {k: torch.as_tensor(np.asarray(v, np.float64)).requires_grad_(True) for k, v in params.items() if v is not None}
    logits = pyramid_forward(leaves, cfg, x_tbd, seq_len, layers, r, drop_seed=drop_seed)
    (logits * torch.as_tensor(dlogits_tbv).to(torch.float64)).sum().backward()
    return logits.detach(), {k: v.grad.detach().numpy() for k, v in leaves.items() if v.grad is not None}
