"""lc_xent_loss alone: HIP-event time per call (both launches: the frame kernel and the per-utterance fold) with and without a
gradient, the bytes it has to move over that time against the 8 TB/s of HBM, and lc_label_smoothing with a gradient at the
same shapes in the same process as the yardstick (it reads the logits and read-modify-writes the gradient: 12 V bytes per
frame against 8 V + 4).  Raw library calls on preallocated buffers, so the host's share is two launches per call.
Usage: python tools/xent_probe.py [output file, default profiles/xent_probe.txt]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from lstm_ctc_amd import _lib, ops

SHAPES = [(1000, 64, 44, 200), (1000, 64, 5000, 20), (1000, 64, 4999, 20)]      # (T, B, V, calls per round)
WARM, ROUNDS = 5, 7
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
    lib = _lib.load()
    p, s = ops._ptr, ops._stream
    lines = ["# tools/xent_probe.py on %s: %d rounds per figure, median [min .. max] of the rounds' mean time per call, us;"
             % (torch.cuda.get_device_name(0), ROUNDS),
             "# GB/s = the bytes the call has to move (xent: (8 V + 4 + 16) per frame with a gradient, (4 V + 4 + 16) without; "
             "label smoothing: 12 V per frame) / median time; %% = of 8 TB/s"]
    for T, B, V, reps in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(5)
        logits = torch.randn((T, B, V), device="cuda", generator=g) * 2
        targets = torch.randint(0, V, (B, T), device="cuda", generator=g, dtype=torch.int32)
        seq = torch.full((B,), T, dtype=torch.int32, device="cuda")
        loss = torch.empty(B, device="cuda")
        frames = torch.empty(B, dtype=torch.int32, device="cuda")
        correct = torch.empty(B, dtype=torch.int32, device="cuda")
        grad = torch.empty_like(logits)
        nbytes = lib.lc_xent_workspace_bytes(T, B, V)
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        acc = torch.zeros(1, dtype=torch.float64, device="cuda")

        def xent(gr):
            _lib.check(lib.lc_xent_loss(p(logits), T, B, V, p(targets), p(seq), p(loss), p(frames), p(correct), p(gr), p(ws),
                                        nbytes, s()), "lc_xent_loss")

        def smooth():
            _lib.check(lib.lc_label_smoothing(p(logits), T * B, V, None, 0.1, p(acc), p(grad), s()), "lc_label_smoothing")

        xent(grad)
        torch.cuda.synchronize()
        ref = -torch.log_softmax(logits[:, 0].double(), -1).gather(-1, targets[0].long()[:, None]).sum()
        assert abs(float(loss[0]) - float(ref)) < 1e-4 * float(ref) and int(frames[0]) == T
        res = {"grad": timed(lambda: xent(grad), reps), "nograd": timed(lambda: xent(None), reps), "smooth": timed(smooth, reps)}
        byt = {"grad": T * B * (8 * V + 20), "nograd": T * B * (4 * V + 20), "smooth": T * B * 12 * V}
        f = lambda k: "%.1f [%.1f .. %.1f] us, %.0f GB/s (%.0f%%)" % (res[k] + (byt[k] / res[k][0] / 1e3,
                                                                      100 * byt[k] / (res[k][0] * 1e-6) / HBM))
        lines.append("T=%d B=%d V=%d (%.1f MB of logits, %d calls per round):" % (T, B, V, T * B * V * 4 / 1e6, reps))
        lines.append("    lc_xent_loss with gradient    %s" % f("grad"))
        lines.append("    lc_xent_loss grad = NULL      %s" % f("nograd"))
        lines.append("    lc_label_smoothing + gradient %s" % f("smooth"))
        del logits, grad
    text = "\n".join(lines) + "\n"
    print(text, end="")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(root, "profiles", "xent_probe.txt")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
