"""Layer-normalisation probe (run on the GPU box).  First the two passes, lc_layer_norm_fwd / lc_layer_norm_bwd, on c4's
[64000, 2048] and c2's [32000, 640] layer outputs with keep = 1 and keep = 0.9 (the recipes' dropout_rate), each against a
torch device-to-device copy of the bytes the pass moves (8 per element forward: x read, y written; 12 backward: x and dy read, dx written), timed in the same
run: warm, five rounds of twenty calls, the median round and the spread of the rounds.  Then the full train step of bench.py's
c2 and c4 workloads without and with layer_norm = true: one graph per setting in one process, the settings alternating - ten
timed steps each after a warm-up of both, three alternations - so that a difference is read against the run-to-run spread of
the same box; and per setting the event brackets of one step's normalisation passes.  Prints text;
`python tools/layer_norm_probe.py > profiles/layer_norm_probe.txt`.

    python tools/layer_norm_probe.py [passes] [c2] [c4]        (default: all three)"""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from lstm_ctc_amd import ops  # noqa: E402
from lstm_ctc_amd.nnet.graph import create_graph_for_training_ctc  # noqa: E402


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


def pass_probe(name):
    w = bench.WORKLOADS[name]
    T, B, P = w["T"], w["B"], w["cfg"]["num_projects"]
    C = 2 * P
    x = torch.randn((T * B, C), device="cuda")
    dy = torch.randn((T * B, C), device="cuda")
    y, dx = torch.empty_like(x), torch.empty_like(x)
    # the backward's yardstick: 12 bytes per element of [T * B, C] = a copy of one and a half such matrices
    src3, dst3 = torch.randn((T * B * 3 // 2, C), device="cuda"), torch.empty((T * B * 3 // 2, C), device="cuda")
    gamma, beta = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
    dgamma, dbeta = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    for what, seq in (("full lengths", torch.full((B,), T, dtype=torch.int32, device="cuda")),
                      ("lengths 0.6 T .. T", torch.linspace(0.6 * T, T, B).to(torch.int32).cuda())):
        t8, s8 = timed(lambda: y.copy_(x))
        t12, s12 = timed(lambda: dst3.copy_(src3))
        for keep in (1.0, 0.9):
            tf, sf = timed(lambda: ops.layer_norm_fwd(x, gamma, beta, seq, T, B, keep, 1, 0, P, out=y))
            tb, sb = timed(lambda: ops.layer_norm_bwd(x, dy, gamma, seq, T, B, keep, 1, 0, P, dx=dx, dgamma=dgamma, dbeta=dbeta))
            print("%s layer output [%d, %d] f32, %s, keep = %.1f: lc_layer_norm_fwd %.1f us (spread %.1f) = %.2f of the 8-byte "
                  "copy's %.1f us (spread %.1f), %.0f GB/s | lc_layer_norm_bwd %.1f us (spread %.1f) = %.2f of the 12-byte copy's "
                  "%.1f us (spread %.1f), %.0f GB/s"
                  % (name, T * B, C, what, keep, tf * 1e6, sf * 1e6, tf / t8, t8 * 1e6, s8 * 1e6, 8.0 * T * B * C / tf / 1e9,
                     tb * 1e6, sb * 1e6, tb / t12, t12 * 1e6, s12 * 1e6, 12.0 * T * B * C / tb / 1e9), flush=True)


def step_probe(name, steps=10, rounds=3):
    w = bench.WORKLOADS[name]
    T, B = w["T"], w["B"]
    settings = (False, True)
    label = {False: "plain", True: "layer_norm = true"}
    graphs = {s: create_graph_for_training_ctc(None, dict(w["cfg"], **({"layer_norm": True} if s else {})), learn_rate=4e-4,
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
        print("%s T=%d B=%d keep=%.2f, %-18s: %s ms/step (mean %.2f, spread %.2f) -> %.1f k frames/s" % (
            name, T, B, graphs[s].model.keep, label[s], " ".join("%.2f" % t for t in ms[s]), mean[s], spread[s],
            T * B / mean[s]), flush=True)
    d = mean[True] - mean[False]
    verdict = "beyond both spreads" if abs(d) > spread[True] + spread[False] else "WITHIN the runs' spreads"
    print("%s: layer_norm = true is %.2f ms/step %s than plain (%.1f %%), %s" % (
        name, abs(d), "SLOWER" if d > 0 else "faster", 100.0 * d / mean[False], verdict), flush=True)
    model = graphs[True].model
    overlap, model.overlap_wgrad = model.overlap_wgrad, False      # a bracket then holds one kernel's time
    run(True, 1)
    ops.PROFILE = []
    run(True, 1)
    prof, ops.PROFILE = ops.PROFILE, None
    model.overlap_wgrad = overlap
    fwd = [st.elapsed_time(e) for k, wk, st, e in prof if k == "layer_norm" and wk == 8.0 * T * B * model.ps.H]
    bwd = [st.elapsed_time(e) for k, wk, st, e in prof if k == "layer_norm" and wk == 12.0 * T * B * model.ps.H]
    print("   layer_norm = true, one step's normalisation passes: forward %s ms | backward %s ms | %.3f ms of the step's %.2f"
          % (" ".join("%.3f" % t for t in fwd), " ".join("%.3f" % t for t in bwd), sum(fwd) + sum(bwd), mean[True]), flush=True)


if __name__ == "__main__":
    what = sys.argv[1:] or ["passes", "c2", "c4"]
    if "passes" in what:
        for name in ("c4", "c2"):
            pass_probe(name)
    for name in ("c2", "c4"):
        if name in what:
            step_probe(name)
