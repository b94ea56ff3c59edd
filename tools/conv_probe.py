"""Convolutional front-end probe (run on the GPU box).  First the three passes of lc_conv_fwd / lc_conv_bwd - forward, input
gradient alone, weight gradient alone - per layer of a two-layer front-end with 32 channels over 40 bins at c4's (T = 1000,
B = 64) and c2's (T = 1000, B = 32) batch shapes, with 1 and 3 input channels, each against (a) a torch device-to-device copy of
the bytes the pass must move (read plus written, each tensor once) and (b) its FLOPs at the fp32 MFMA peak, timed in the same
run: warm, five rounds of twenty calls, the median round and the spread of the rounds.  Then the full train step of bench.py's c2
and c4 workloads without and with conv_layers = 2 (conv_channels = 32, conv_bins = 40: one input channel, the benchmark's 40-d
input): one graph per setting in one process, the settings alternating - ten timed steps each after a warm-up of both, three
alternations - so that a difference is read against the run-to-run spread of the same box; and the event brackets of one step's
conv passes next to their FLOP floor.  Prints text; `python tools/conv_probe.py > profiles/conv_probe.txt`.

    python tools/conv_probe.py [passes] [c2] [c4]        (default: all three)"""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from lstm_ctc_amd import ops  # noqa: E402
from lstm_ctc_amd.nnet.graph import create_graph_for_training_ctc  # noqa: E402

PEAK = bench.PEAK_F32_MFMA_TFLOPS * 1e12
CONV_KEYS = dict(conv_layers=2, conv_channels=32, conv_bins=40)


def timed(fn, iters=20, rounds=5):
    """(median, spread) in seconds per call over ``rounds`` rounds of ``iters`` calls, after a warm-up."""
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            fn()
        e.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(e) / iters * 1e-3)
    out.sort()
    return out[len(out) // 2], out[-1] - out[0]


def copy_of(nbytes):
    """A device copy that moves ``nbytes`` in all (half read, half written) -> (median, spread)."""
    n = max(int(nbytes) // 8, 1)
    src, dst = torch.randn(n, device="cuda"), torch.empty(n, device="cuda")
    return timed(lambda: dst.copy_(src))


def pass_probe(name, Cin0, Cc=32, F0=40):
    w = bench.WORKLOADS[name]
    T, B = w["T"], w["B"]
    rows = T * B
    seq = torch.full((B,), T, dtype=torch.int32, device="cuda")
    total = 0.0
    F, Cin = F0, Cin0
    for k in range(2):
        Fo = ops.conv_out_bins(F)
        gm = k == 0
        x = torch.randn((rows, Cin * F), device="cuda")
        wt = torch.randn((3, 3, Cin, Cc), device="cuda") / (9 * Cin) ** 0.5
        bias = torch.zeros(Cc, device="cuda")
        y = ops.conv_fwd(x, wt, bias, seq, T, B, F, gm)
        dy = torch.randn_like(y)
        dx, dw, db = torch.empty_like(x), torch.empty_like(wt), torch.empty_like(bias)
        nx, ny = 4.0 * rows * Cin * F, 4.0 * rows * Fo * Cc
        flops = 2.0 * 9 * Cin * Cc * Fo * rows
        floor = flops / PEAK
        for what, fn, nbytes in (
                ("forward", lambda: ops.conv_fwd(x, wt, bias, seq, T, B, F, gm, out=y), nx + ny),
                ("input gradient", lambda: ops.conv_bwd(x, y, dy, wt, seq, T, B, F, gm, want_dparams=False, dx=dx), 2 * ny + nx),
                ("weight gradient", lambda: ops.conv_bwd(x, y, dy, wt, seq, T, B, F, gm, want_dx=False, dw=dw, dbias=db), 2 * ny + nx)):
            t, s = timed(fn)
            tc, sc = copy_of(nbytes)
            if not (k == 0 and what == "input gradient"):          # (the first layer's dx is never asked for in a step)
                total += t
            print("%s rows %d, layer %d: %d ch x %d bins -> %d ch x %d bins, %-15s: %8.1f us (spread %.1f) = %.2f of a copy of its "
                  "%.1f MB (%.1f us, spread %.1f) = %.1f of its %.3f GFLOP at %.1f TFLOP/s (%.1f us): %.2f TFLOP/s"
                  % (name, rows, k, Cin, F, Cc, Fo, what, t * 1e6, s * 1e6, t / tc, nbytes / 1e6, tc * 1e6, sc * 1e6, t / floor,
                     flops / 1e9, PEAK / 1e12, floor * 1e6, flops / t / 1e12), flush=True)
        F, Cin = Fo, Cc
    print("%s, %d input channel(s): the five conv passes of one train step (no dx for layer 0) take %.3f ms"
          % (name, Cin0, total * 1e3), flush=True)


def step_probe(name, steps=10, rounds=3):
    w = bench.WORKLOADS[name]
    T, B = w["T"], w["B"]
    settings = (False, True)
    label = {False: "plain", True: "conv_layers = 2"}
    graphs = {s: create_graph_for_training_ctc(None, dict(w["cfg"], **(CONV_KEYS if s else {})), learn_rate=4e-4,
                                               clip_norm=5.0, optimizer="adam", device="cuda", seed=123) for s in settings}
    x, seq, labels, offs = bench.synth_batch(w, 0, "cuda")
    size, maxlen = int(labels.numel()), w["L"]

    def run(s, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            graphs[s].step_device(x, seq, labels, offs, maxlen, size, fetch_eval=False)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n

    for s in settings:
        run(s, 3)                                         # warm-up of every path
    ms = {s: [] for s in settings}
    for _ in range(rounds):
        for s in settings:
            ms[s].append(run(s, steps) * 1e3)
    mean = {s: sum(v) / len(v) for s, v in ms.items()}
    spread = {s: max(v) - min(v) for s, v in ms.items()}
    for s in settings:
        assert graphs[s].persist_fallbacks == 0
        print("%s T=%d B=%d keep=%.2f, %-16s: %s ms/step (mean %.2f, spread %.2f) -> %.1f k frames/s" % (
            name, T, B, graphs[s].model.keep, label[s], " ".join("%.2f" % t for t in ms[s]), mean[s], spread[s],
            T * B / mean[s]), flush=True)
    d = mean[True] - mean[False]
    verdict = "beyond both spreads" if abs(d) > spread[True] + spread[False] else "WITHIN the runs' spreads"
    print("%s: conv_layers = 2 is %.2f ms/step %s than plain (%.1f %%), %s (layer 0 reads %d columns instead of %d)" % (
        name, abs(d), "SLOWER" if d > 0 else "faster", 100.0 * d / mean[False], verdict, graphs[True].model.ps.D0,
        graphs[True].model.ps.D), flush=True)
    model = graphs[True].model
    overlap, model.overlap_wgrad = model.overlap_wgrad, False      # a bracket then holds one kernel's time
    run(True, 1)
    ops.PROFILE = []
    run(True, 1)
    prof, ops.PROFILE = ops.PROFILE, None
    model.overlap_wgrad = overlap
    conv = [(wk, st.elapsed_time(e)) for k, wk, st, e in prof if k == "conv"]
    floor = sum(wk for wk, _ in conv) / PEAK * 1e3
    took = sum(t for _, t in conv)
    print("   conv_layers = 2, one step's conv passes (forward 0, forward 1, backward 1, backward 0): %s ms | %.3f ms of the step's "
          "%.2f = %.1f times their %.3f ms FLOP floor at %.1f TFLOP/s"
          % (" ".join("%.3f" % t for _, t in conv), took, mean[True], took / floor, floor, PEAK / 1e12), flush=True)


if __name__ == "__main__":
    what = sys.argv[1:] or ["passes", "c2", "c4"]
    if "passes" in what:
        for name in ("c4", "c2"):
            for Cin0 in (1, 3):
                pass_probe(name, Cin0)
    for name in ("c2", "c4"):
        if name in what:
            step_probe(name)
