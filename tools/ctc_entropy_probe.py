"""lc_ctc_loss_entropy alone: HIP-event time per call at B = 64, T = 1000, L = 100, V = 44, with and without a gradient,
unconstrained (NULL windows); lc_ctc_loss_windowed on the same inputs (open windows), alternating with it in the same process,
is the yardstick.  No gate: the figures and ratios go to the output file (DESIGN.md section 3.14 quotes them).
Usage: python tools/ctc_entropy_probe.py [output file, default profiles/ctc_entropy_probe.txt]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from lstm_ctc_amd import _lib, ops

T, V, B, L, ETA = 1000, 44, 64, 100, 0.2
WARM, REPS, ROUNDS = 3, 20, 5


def one_round(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS * 1e3


def main():
    g = torch.Generator().manual_seed(5)
    logits = (2 * torch.randn((T, B, V), generator=g)).cuda()
    labels = torch.randint(0, V - 1, (B * L,), generator=g, dtype=torch.int32).cuda()
    offs = (torch.arange(B + 1, dtype=torch.int64) * L).to(torch.int32).cuda()
    seq = torch.full((B,), T, dtype=torch.int32).cuda()
    open_lo = torch.zeros_like(labels)
    open_hi = torch.full_like(labels, ops.WINDOW_OPEN)
    variants = {"win_grad": lambda: ops.ctc_loss_windowed(logits, labels, offs, seq, L, open_lo, open_hi),
                "ent_grad": lambda: ops.ctc_loss_entropy(logits, labels, offs, seq, L, ETA),
                "win_loss": lambda: ops.ctc_loss_windowed(logits, labels, offs, seq, L, open_lo, open_hi, want_grad=False),
                "ent_loss": lambda: ops.ctc_loss_entropy(logits, labels, offs, seq, L, ETA, want_grad=False)}
    for fn in variants.values():
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in variants}
    for _ in range(ROUNDS):                                # the entries alternate within every round
        for k, fn in variants.items():
            rounds[k].append(one_round(fn))
    res = {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in rounds.items()}
    f = lambda k: "%.1f [%.1f .. %.1f]" % res[k]
    loss_w = variants["win_loss"]()[0]
    loss_e, entropy, _ = variants["ent_loss"]()
    lib = _lib.load()
    ws_w, ws_e = lib.lc_ctc_window_workspace_bytes(T, B, V, L), lib.lc_ctc_entropy_workspace_bytes(T, B, V, L)
    lines = ["# tools/ctc_entropy_probe.py on %s: B = %d, T = %d, L = %d, V = %d, entropy_weight = %g, NULL windows; %d x %d calls "
             "per figure, the entries alternating (median [min .. max] of the rounds), us; (x ...) = over lc_ctc_loss_windowed "
             "with open windows on the same inputs" % (torch.cuda.get_device_name(0), B, T, L, V, ETA, ROUNDS, REPS),
             "with a gradient: lc_ctc_loss_windowed %s, lc_ctc_loss_entropy %s (x %.2f)"
             % (f("win_grad"), f("ent_grad"), res["ent_grad"][0] / res["win_grad"][0]),
             "without a gradient (forward sweep only): lc_ctc_loss_windowed %s, lc_ctc_loss_entropy %s (x %.2f)"
             % (f("win_loss"), f("ent_loss"), res["ent_loss"][0] / res["win_loss"][0]),
             "workspace: windowed %.1f MiB, entropy %.1f MiB (x %.2f)" % (ws_w / 2 ** 20, ws_e / 2 ** 20, ws_e / ws_w),
             "loss bit-identical to lc_ctc_loss_windowed: %s; mean loss %.3f, mean path entropy %.3f nats = %.4f per frame"
             % (bool(torch.equal(loss_w, loss_e)), loss_e.double().mean().item(), entropy.double().mean().item(),
                entropy.double().sum().item() / (B * T))]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(root, "profiles", "ctc_entropy_probe.txt")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
