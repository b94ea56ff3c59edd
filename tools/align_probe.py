"""lc_ctc_align alone: HIP-event time per call at three shapes, split into its three launches (per-frame log-sum-exp, forward
sweep, backtrace; lc_debug_ctc_align_phases runs them one by one on a workspace a full call has filled), with lc_ctc_loss
(grad = NULL: same lattice, same chain length) timed in the same process as the yardstick.  Also the largest measured error
of the score against float64 next to the bound tests/test_gpu_align.py derives.
Usage: python tools/align_probe.py [output file, default profiles/align_probe.txt]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from lstm_ctc_amd import _lib, ops

T, V = 1000, 44
SHAPES = [(64, 100), (512, 100), (64, 600)]            # (B, L)
WARM, REPS, ROUNDS = 5, 40, 5


def timed(fn):
    """Median over ROUNDS of the mean time of REPS back-to-back calls, in microseconds."""
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / REPS * 1e3)
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def score_error(logits, labels, L, ali, score):
    """max_b |score - float64 sum of log-softmax along the returned path| / bound (the tests' tol_b, without tol_c)."""
    x = logits.double().cpu().numpy()                                             # [T,B,V]
    lp = x - (x.max(-1, keepdims=True) + np.log(np.exp(x - x.max(-1, keepdims=True)).sum(-1, keepdims=True)))
    a = ali.cpu().numpy().astype(np.int64)                                        # [B,T]
    path = np.take_along_axis(lp, a.T[:, :, None], axis=2)[:, :, 0].sum(axis=0)   # [B]
    s = score.cpu().numpy().astype(np.float64)
    u = 2.0 ** -24
    bound = T * u * (3 * V + 8 + float(np.abs(x).max())) + 2 * u * np.abs(s)
    err = np.abs(s - path)
    b = int(np.argmax(err / bound))
    return err[b], bound[b], abs(s[b])


def main():
    lib = _lib.load()
    lines = ["# tools/align_probe.py on %s: T = %d, V = %d, %d x %d calls per figure (median [min .. max] of the rounds), us"
             % (torch.cuda.get_device_name(0), T, V, ROUNDS, REPS)]
    for B, L in SHAPES:
        g = torch.Generator().manual_seed(5)
        logits = (2 * torch.randn((T, B, V), generator=g)).cuda()
        labels = torch.randint(0, V - 1, (B * L,), generator=g, dtype=torch.int32).cuda()
        offs = (torch.arange(B + 1, dtype=torch.int64) * L).to(torch.int32).cuda()
        seq = torch.full((B,), T, dtype=torch.int32).cuda()
        res = {}
        lib.lc_debug_ctc_align_phases(7)
        ali, idx, score = ops.ctc_align(logits, labels, offs, seq, L)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(score).all())
        res["align"] = timed(lambda: ops.ctc_align(logits, labels, offs, seq, L))
        for name, mask in (("lse", 1), ("sweep", 2), ("trace", 4)):
            lib.lc_debug_ctc_align_phases(mask)
            res[name] = timed(lambda: ops.ctc_align(logits, labels, offs, seq, L))
        lib.lc_debug_ctc_align_phases(7)
        ali2, idx2, score2 = ops.ctc_align(logits, labels, offs, seq, L)
        assert torch.equal(ali, ali2) and torch.equal(idx, idx2) and torch.equal(score, score2)
        res["loss"] = timed(lambda: ops.ctc_loss(logits, labels, offs, seq, L, want_grad=False))
        err, bound, mag = score_error(logits, labels, L, ali, score)
        f = lambda k: "%.1f [%.1f .. %.1f]" % res[k]
        lines.append("B=%d T=%d V=%d L=%d: lc_ctc_align %s = lse %s + sweep %s + backtrace %s (each launch alone);  "
                     "lc_ctc_loss(grad=NULL) %s" % (B, T, V, L, f("align"), f("lse"), f("sweep"), f("trace"), f("loss")))
        lines.append("    score vs float64 along the returned path: largest error %.3e at |score| = %.1f, derived bound %.3e, "
                     "project bar %.3e" % (err, mag, bound, 1e-4 * max(mag, 1.0)))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(root, "profiles", "align_probe.txt")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
