"""lc_ctc_loss_star alone: HIP-event time per call at B = 64, T = 1000, L = 100, V = 44, with and without a gradient,
unconstrained (NULL windows); lc_ctc_loss_delay at penalty 0 on the same inputs, alternating with it in the same process, is
the yardstick (with a gradient: with entry_sum, so that both entries run both sweeps, a gradient pass and a fold; without:
delay's forward sweep alone next to the star's two sweeps and frame pass, which star_frames needs).  No gate: the figures and
ratios go to the output file (DESIGN.md section 3.15 quotes them).
Usage: python tools/ctc_star_probe.py [output file, default profiles/ctc_star_probe.txt]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from lstm_ctc_amd import _lib, ops

T, V, B, L, PENALTY = 1000, 44, 64, 100, (2.0, 2.0)
WARM, REPS, ROUNDS = 3, 20, 5
INF = float("inf")


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
    variants = {"delay_grad": lambda: ops.ctc_loss_delay(logits, labels, offs, seq, L, 0.0),
                "star_grad": lambda: ops.ctc_loss_star(logits, labels, offs, seq, L, *PENALTY),
                "delay_loss": lambda: ops.ctc_loss_delay(logits, labels, offs, seq, L, 0.0, want_grad=False, want_entry=False),
                "delay_entry": lambda: ops.ctc_loss_delay(logits, labels, offs, seq, L, 0.0, want_grad=False),
                "star_loss": lambda: ops.ctc_loss_star(logits, labels, offs, seq, L, *PENALTY, want_grad=False)}
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
    loss_d, _, grad_d = variants["delay_grad"]()
    loss_i, star_i, grad_i = ops.ctc_loss_star(logits, labels, offs, seq, L, INF, INF)
    loss_s, star_s, _ = variants["star_loss"]()
    lib = _lib.load()
    ws_d, ws_s = lib.lc_ctc_delay_workspace_bytes(T, B, V, L), lib.lc_ctc_star_workspace_bytes(T, B, V, L)
    lines = ["# tools/ctc_star_probe.py on %s: B = %d, T = %d, L = %d, V = %d, penalties %g / %g, NULL windows; %d x %d calls per "
             "figure, the entries alternating (median [min .. max] of the rounds), us; (x ...) = over lc_ctc_loss_delay at penalty "
             "0 on the same inputs" % (torch.cuda.get_device_name(0), B, T, L, V, PENALTY[0], PENALTY[1], ROUNDS, REPS),
             "with a gradient: lc_ctc_loss_delay (with entry_sum) %s, lc_ctc_loss_star %s (x %.2f)"
             % (f("delay_grad"), f("star_grad"), res["star_grad"][0] / res["delay_grad"][0]),
             "without a gradient: lc_ctc_loss_delay, forward sweep only %s, with entry_sum (both sweeps, frame pass, fold) %s; "
             "lc_ctc_loss_star (both sweeps, class lists, frame pass, fold) %s (x %.2f / x %.2f)"
             % (f("delay_loss"), f("delay_entry"), f("star_loss"), res["star_loss"][0] / res["delay_loss"][0],
                res["star_loss"][0] / res["delay_entry"][0]),
             "workspace: delay %.1f MiB, star %.1f MiB (+ %d bytes = T * B floats)" % (ws_d / 2 ** 20, ws_s / 2 ** 20, ws_s - ws_d),
             "penalties (inf, inf): loss bit-identical to lc_ctc_loss_delay(0): %s, grad bit-identical: %s, star_frames all +0: %s"
             % (bool(torch.equal(loss_d, loss_i)), bool(torch.equal(grad_d, grad_i)),
                bool((star_i.view(torch.int32) == 0).all())),
             "mean loss: plain %.3f, star %.3f; mean star_frames %.3f = %.4f of the frames"
             % (loss_d.double().mean().item(), loss_s.double().mean().item(), star_s.double().mean().item(),
                star_s.double().sum().item() / (B * T))]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(root, "profiles", "ctc_star_probe.txt")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
