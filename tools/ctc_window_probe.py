"""lc_ctc_loss_windowed alone: HIP-event time per call WITH a gradient at tools/align_probe.py's three shapes, unconstrained and
with windows of tau = 10 frames around lc_ctc_align's path on the same logits, with lc_ctc_loss (with a gradient) timed in the
same process as the yardstick.  No gate: the figures and ratios go to the output file (DESIGN.md section 3.8 quotes them).
Usage: python tools/ctc_window_probe.py [output file, default profiles/ctc_window_probe.txt] [--once]
--once: three calls per variant and no timing - the run to put under a kernel trace for the per-launch split."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from lstm_ctc_amd import ops

T, V, TAU = 1000, 44, 10
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
    argv = [a for a in sys.argv[1:] if a != "--once"]
    once = "--once" in sys.argv[1:]
    lines = ["# tools/ctc_window_probe.py on %s: T = %d, V = %d, with a gradient, %d x %d calls per figure (median [min .. max] "
             "of the rounds), us" % (torch.cuda.get_device_name(0), T, V, ROUNDS, REPS)]
    for B, L in SHAPES:
        g = torch.Generator().manual_seed(5)
        logits = (2 * torch.randn((T, B, V), generator=g)).cuda()
        labels = torch.randint(0, V - 1, (B * L,), generator=g, dtype=torch.int32).cuda()
        offs = (torch.arange(B + 1, dtype=torch.int64) * L).to(torch.int32).cuda()
        seq = torch.full((B,), T, dtype=torch.int32).cuda()
        ali, _, score = ops.ctc_align(logits, labels, offs, seq, L)
        assert bool(torch.isfinite(score).all())
        lo, hi, ok = ops.label_windows(ali.cpu().numpy(), labels.cpu().numpy(), offs.cpu().numpy(), seq.cpu().numpy(), TAU,
                                       V - 1)
        assert ok.all()
        lo, hi = torch.from_numpy(lo).cuda(), torch.from_numpy(hi).cuda()
        open_lo = torch.zeros_like(lo)
        open_hi = torch.full_like(hi, ops.WINDOW_OPEN)
        variants = {"ctc": lambda: ops.ctc_loss(logits, labels, offs, seq, L),
                    "open": lambda: ops.ctc_loss_windowed(logits, labels, offs, seq, L, open_lo, open_hi),
                    "tau": lambda: ops.ctc_loss_windowed(logits, labels, offs, seq, L, lo, hi)}
        loss = {k: fn()[0].double().cpu().numpy() for k, fn in variants.items()}
        assert np.isfinite(loss["tau"]).all() and (loss["open"] <= loss["tau"] + 1e-4 * loss["tau"]).all()
        rel = float(np.abs(loss["open"] - loss["ctc"]).max() / np.abs(loss["ctc"]).max())
        if once:
            for fn in variants.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            continue
        res = {k: timed(fn) for k, fn in variants.items()}
        f = lambda k: "%.1f [%.1f .. %.1f]" % res[k]
        lines.append("B=%d T=%d V=%d L=%d: lc_ctc_loss %s;  lc_ctc_loss_windowed unconstrained %s (x %.2f), tau = %d around "
                     "lc_ctc_align's path %s (x %.2f)" % (B, T, V, L, f("ctc"), f("open"), res["open"][0] / res["ctc"][0], TAU,
                                                          f("tau"), res["tau"][0] / res["ctc"][0]))
        lines.append("    mean loss: lc_ctc_loss %.3f, unconstrained %.3f (largest difference %.1e of the loss), tau = %d %.3f"
                     % (loss["ctc"].mean(), loss["open"].mean(), rel, TAU, loss["tau"].mean()))
    if once:
        return
    text = "\n".join(lines) + "\n"
    print(text, end="")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = argv[0] if argv else os.path.join(root, "profiles", "ctc_window_probe.txt")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
