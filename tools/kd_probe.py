"""lc_kd_loss alone: HIP-event time per call - overwrite, accumulate and grad = NULL - by raw library calls on preallocated
buffers, with lc_xent_loss (with a gradient) and lc_label_smoothing (with a gradient) timed in the same process as the
yardsticks.  No gate: the figures and the ratios to lc_xent_loss go to the output file (DESIGN.md section 3.9 quotes them);
by bytes the ratios at V = 5000 should be 1.5 (overwrite: 12 V against 8 V per frame) and 2 (accumulate: 16 V).
Usage: python tools/kd_probe.py [output file, default profiles/kd_probe.txt] [--once]
--once: three calls per variant and no timing - the run to put under a kernel trace for the per-launch split."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from lstm_ctc_amd import _lib, ops

T, B = 1000, 64
SHAPES = [(44, 200), (5000, 20), (4999, 20)]           # (V, calls per round)
WARM, ROUNDS = 3, 7
TAU = 2.0
HBM = 8e12


def timed(fn, reps):
    """Median [min .. max] over ROUNDS of the mean time of `reps` back-to-back calls, in microseconds."""
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / reps * 1e3)
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def main():
    argv = [a for a in sys.argv[1:] if a != "--once"]
    once = "--once" in sys.argv[1:]
    lib = _lib.load()
    p, st = ops._ptr, ops._stream
    lines = ["# tools/kd_probe.py on %s: %d rounds per figure, median [min .. max] of the rounds' mean time per call, us;"
             % (torch.cuda.get_device_name(0), ROUNDS),
             "# GB/s = the bytes the call has to move (kd: (12 V + 16) per frame overwriting, (16 V + 16) accumulating, (8 V + 16) "
             "without a gradient; xent: 8 V + 20; label smoothing: 12 V) / median time; % = of 8 TB/s; x = time / lc_xent_loss's"]
    for V, reps in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(5)
        logits = torch.randn((T, B, V), device="cuda", generator=g) * 3.0
        teacher = torch.log_softmax(torch.randn((T, B, V), device="cuda", generator=g) * 3.0, dim=-1)
        targets = torch.randint(0, V, (B, T), device="cuda", generator=g, dtype=torch.int32)
        seq = torch.full((B,), T, dtype=torch.int32, device="cuda")
        loss = torch.empty(B, device="cuda")
        n1, n2 = torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
        grad = torch.zeros((T, B, V), device="cuda")
        acc = torch.zeros(1, dtype=torch.float64, device="cuda")
        kd_bytes, xe_bytes = lib.lc_kd_workspace_bytes(T, B, V), lib.lc_xent_workspace_bytes(T, B, V)
        ws = torch.empty(max(kd_bytes, xe_bytes), dtype=torch.uint8, device="cuda")

        def kd(gr, accumulate):
            _lib.check(lib.lc_kd_loss(p(logits), p(teacher), T, B, V, p(seq), p(seq), TAU, TAU, p(loss), p(n1), p(n2), p(gr),
                                      accumulate, p(ws), kd_bytes, st()), "lc_kd_loss")

        def xent():
            _lib.check(lib.lc_xent_loss(p(logits), T, B, V, p(targets), p(seq), p(loss), p(n1), p(n2), p(grad), p(ws), xe_bytes,
                                        st()), "lc_xent_loss")

        def smoothing():
            _lib.check(lib.lc_label_smoothing(p(logits), T * B, V, None, 0.1, p(acc), p(grad), st()), "lc_label_smoothing")

        frames = T * B
        variants = [("lc_xent_loss with gradient", xent, frames * (8 * V + 20)),
                    ("lc_label_smoothing + gradient", smoothing, frames * 12 * V),
                    ("lc_kd_loss overwrite", lambda: kd(grad, 0), frames * (12 * V + 16)),
                    ("lc_kd_loss accumulate", lambda: kd(grad, 1), frames * (16 * V + 16)),
                    ("lc_kd_loss grad = NULL", lambda: kd(None, 0), frames * (8 * V + 16))]
        if once:
            for _, fn, _ in variants:
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            continue
        lines.append("T=%d B=%d V=%d (%.1f MB of logits, %d calls per round):" % (T, B, V, T * B * V * 4 / 1e6, reps))
        base = None
        for name, fn, nbytes in variants:
            med, lo, hi = timed(fn, reps)
            base = med if base is None else base
            lines.append("    %-30s %.1f [%.1f .. %.1f] us, %.0f GB/s (%.0f%%), x %.2f"
                         % (name, med, lo, hi, nbytes / med / 1e3, 100 * nbytes / (med * 1e-6) / HBM, med / base))
    if once:
        return
    text = "\n".join(lines) + "\n"
    print(text, end="")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = argv[0] if argv else os.path.join(root, "profiles", "kd_probe.txt")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
