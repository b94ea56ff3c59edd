"""lc_ctc_loss_delay alone: HIP-event time per call at tools/ctc_window_probe.py's three shapes, with and without entry_sum,
with and without a gradient, unconstrained (NULL windows); lc_ctc_loss_windowed on the same inputs (open windows), timed in
the same process, is the yardstick.  No gate: the figures and ratios go to the output file (DESIGN.md section 3.10 quotes them).
Usage: python tools/ctc_delay_probe.py [output file, default profiles/ctc_delay_probe.txt]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from lstm_ctc_amd import ops

T, V, LAMBDA = 1000, 44, 0.05
SHAPES = [(64, 100), (512, 100), (64, 600)]            # (B, L)
WARM, REPS, ROUNDS = 3, 20, 5


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


def main():
    lines = ["# tools/ctc_delay_probe.py on %s: T = %d, V = %d, delay_penalty = %g, %d x %d calls per figure (median [min .. max] "
             "of the rounds), us; (x ...) = over lc_ctc_loss_windowed with open windows on the same inputs, with / without a "
             "gradient alike" % (torch.cuda.get_device_name(0), T, V, LAMBDA, ROUNDS, REPS)]
    for B, L in SHAPES:
        g = torch.Generator().manual_seed(5)
        logits = (2 * torch.randn((T, B, V), generator=g)).cuda()
        labels = torch.randint(0, V - 1, (B * L,), generator=g, dtype=torch.int32).cuda()
        offs = (torch.arange(B + 1, dtype=torch.int64) * L).to(torch.int32).cuda()
        seq = torch.full((B,), T, dtype=torch.int32).cuda()
        open_lo = torch.zeros_like(labels)
        open_hi = torch.full_like(labels, ops.WINDOW_OPEN)
        delay = lambda grad, entry, lam=LAMBDA: ops.ctc_loss_delay(logits, labels, offs, seq, L, lam, want_grad=grad,
                                                                   want_entry=entry)
        variants = {"win_grad": lambda: ops.ctc_loss_windowed(logits, labels, offs, seq, L, open_lo, open_hi),
                    "win_loss": lambda: ops.ctc_loss_windowed(logits, labels, offs, seq, L, open_lo, open_hi, want_grad=False),
                    "grad_entry": lambda: delay(True, True), "grad": lambda: delay(True, False),
                    "entry": lambda: delay(False, True), "loss": lambda: delay(False, False)}
        zero = delay(False, True, 0.0)
        pen = delay(False, True)
        win = variants["win_loss"]()[0].double()
        rel = float(((zero[0].double() - win).abs().max() / win.abs().max()).item())
        res = {k: timed(fn) for k, fn in variants.items()}
        f = lambda k: "%.1f [%.1f .. %.1f]" % res[k]
        r = lambda k, y: res[k][0] / res[y][0]
        lines.append("B=%d T=%d V=%d L=%d: lc_ctc_loss_windowed with a gradient %s, loss only %s" % (B, T, V, L, f("win_grad"),
                                                                                                   f("win_loss")))
        lines.append("    lc_ctc_loss_delay with a gradient: with entry_sum %s (x %.2f), without %s (x %.2f)"
                     % (f("grad_entry"), r("grad_entry", "win_grad"), f("grad"), r("grad", "win_grad")))
        lines.append("    lc_ctc_loss_delay without a gradient: with entry_sum %s (x %.2f: both sweeps and the entry pass), "
                     "without %s (x %.2f)" % (f("entry"), r("entry", "win_loss"), f("loss"), r("loss", "win_loss")))
        lines.append("    mean loss: windowed %.3f, delay_penalty 0 %.3f (largest difference %.1e of the loss), %g %.3f; mean label "
                     "entry frame: delay_penalty 0 %.2f, %g %.2f"
                     % (win.mean().item(), zero[0].double().mean().item(), rel, LAMBDA, pen[0].double().mean().item(),
                        zero[1].double().sum().item() / (B * L), LAMBDA, pen[1].double().sum().item() / (B * L)))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(root, "profiles", "ctc_delay_probe.txt")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
