"""float64 restatement of the latency-controlled BiLSTM - TEST INFRASTRUCTURE, not product code.

Built from oracle/torch_f64.py's ``lstmp_forward`` and ``reverse_sequence`` on the CPU: the forward direction over the whole
utterance as ``blstm_forward`` runs it; the backward direction, per chunk c, over the window of frames
[c * Nc, c * Nc + Tc), Tc = min(Nc + Nr, T), with the lengths clamp(seq_len - c * Nc, 0, Tc): reverse_sequence -> dynamic_rnn
from a zero state -> reverse_sequence, of which only the first Nc frames are kept.  Gradients by autograd of
sum(logits * dlogits), as ``blstm_gradients`` takes them.  tests/test_lc_blstm_reference.py pins this file to
``blstm_forward`` where the two must agree (every window reaching the end of its utterance)."""
import numpy as np
import torch

from oracle.torch_f64 import dropout_mask, lstmp_forward, reverse_sequence


def lc_blstm_forward(params, cfg, x_tbd, seq_len, chunk, lookahead, drop_seed=0):
    """Logits [T, B, V] float64 (CPU) of the plain-head BiLSTM of ``cfg`` with its backward directions chunked."""
    assert not cfg.get("num_experts"), "plain head only"
    dtype, device = torch.float64, "cpu"

    def g(k):
        v = params.get(k)
        if v is None or torch.is_tensor(v):
            return v
        return torch.as_tensor(np.asarray(v, np.float64), device=device)

    x = torch.as_tensor(x_tbd).to(device=device, dtype=dtype)
    sl = torch.as_tensor(seq_len).to(device=device, dtype=torch.int64)
    keep = 1.0 if not cfg.get("is_training", True) else float(cfg.get("dropout_rate", 1.0))
    T, B, D = x.shape
    nC, Tc = -(-T // chunk), min(chunk + lookahead, T)
    finput = x
    for i in range(cfg["num_layers"]):
        halves = []
        for d, prefix in enumerate(("fd%d/frnn%d" % (i, i), "bd%d/brnn%d" % (i, i))):
            cell = (g(prefix + "/kernel"), g(prefix + "/bias"), g(prefix + "/w_f_diag"), g(prefix + "/w_i_diag"),
                    g(prefix + "/w_o_diag"), g(prefix + "/projection/kernel"), 5.0)
            if d == 0:
                o = lstmp_forward(finput, sl, *cell)
            else:
                kept = []
                for c in range(nC):
                    window = finput[c * chunk:min(c * chunk + Tc, T)]
                    lens = (sl - c * chunk).clamp(0, Tc)
                    oc = reverse_sequence(lstmp_forward(reverse_sequence(window, lens), lens, *cell), lens)
                    kept.append(oc[:chunk])                  # the lookahead frames' outputs are thrown away
                o = torch.cat(kept, dim=0)
                assert o.shape[0] == T
            mask = dropout_mask(drop_seed, 2 * i + d, T, B, o.shape[2], keep, device, dtype)     # hashes the padded index
            halves.append(o if mask is None else o * mask)
        cat = torch.cat(halves, dim=2)
        finput = finput + cat if (i == 0 and D == cat.shape[2]) else cat
    return (finput.reshape(T * B, -1) @ g("Variable") + g("Variable_1")).reshape(T, B, -1)


def lc_blstm_gradients(params, cfg, x_tbd, seq_len, dlogits_tbv, chunk, lookahead, drop_seed=0):
    """(logits float64 [T, B, V], {TF variable name: numpy float64 gradient of sum(logits * dlogits)})."""
    leaves = {k: torch.as_tensor(np.asarray(v, np.float64)).requires_grad_(True) for k, v in params.items() if v is not None}
    logits = lc_blstm_forward(leaves, cfg, x_tbd, seq_len, chunk, lookahead, drop_seed=drop_seed)
    (logits * torch.as_tensor(dlogits_tbv).to(torch.float64)).sum().backward()
    return logits.detach(), {k: v.grad.detach().numpy() for k, v in leaves.items() if v.grad is not None}


def horizon(num_layers, Nc, Nr, c, T):
    """H_L(c), clipped to T: the logits of chunk c read no input frame at or beyond it."""
    H = min((c + 1) * Nc + Nr, T)
    for _ in range(num_layers - 1):
        H = min(((H - 1) // Nc + 1) * Nc + Nr, T)
    return H
