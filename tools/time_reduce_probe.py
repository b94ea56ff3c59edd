"""Pyramidal BiLSTM probe (run on the GPU box).  First the two layout passes, lc_time_reduce_fwd / lc_time_reduce_bwd with
r = 2, on c4's [64000, 2048] and c2's [32000, 640] layer outputs, as GB/s read plus written against a torch device-to-device
copy of the same bytes timed in the same run.  Then the full train step of bench.py's c4 and c2 workloads, plain and with
time_reduce_layers = 2 (c4 also 1,3): one graph per setting in one process, the settings alternating - ten timed steps each
after a warm-up of all, three alternations - so that a difference is read against the run-to-run spread of the same box; and
per setting the event brackets of one step's recurrences, layer by layer.  Prints text;
`python tools/time_reduce_probe.py > profiles/time_reduce_probe.txt`.

    python tools/time_reduce_probe.py [passes] [c2] [c4]        (default: all three)"""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from lstm_ctc_amd import ops  # noqa: E402
from lstm_ctc_amd.nnet.graph import create_graph_for_training_ctc  # noqa: E402

SETTINGS = {"c4": ("0", "2", "1,3"), "c2": ("0", "2")}


def name_of(s):
    return "plain" if s == "0" else "time_reduce_layers = %s" % s


def timed(fn, iters=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e-3


def pass_probe(name, r=2):
    w = bench.WORKLOADS[name]
    T, B, C = w["T"], w["B"], 2 * w["cfg"]["num_projects"]
    To = ops.time_reduce_frames(T, r)
    x = torch.randn((T * B, C), device="cuda")
    y = torch.empty((To * B, r * C), device="cuda")
    dx = torch.empty_like(x)
    nbytes = 8.0 * T * B * C
    for what, seq in (("full lengths", torch.full((B,), T, dtype=torch.int32, device="cuda")),
                      ("lengths 0.6 T .. T", torch.linspace(0.6 * T, T, B).to(torch.int32).cuda())):
        # the yardstick moves the same bytes: a [T * B, C] matrix read and written
        t_copy = timed(lambda: dx.copy_(x))
        t_fwd = timed(lambda: ops.time_reduce_fwd(x, seq, T, B, r, out=y))
        t_bwd = timed(lambda: ops.time_reduce_bwd(y, seq, T, B, r, out=dx))
        copy, fwd, bwd = (nbytes / t / 1e9 for t in (t_copy, t_fwd, t_bwd))
        print("%s layer output [%d, %d] f32, r = %d, %s: torch copy %.0f GB/s | lc_time_reduce_fwd %.0f GB/s = %.2f of the copy | "
              "lc_time_reduce_bwd %.0f GB/s = %.2f of the copy   (read + written, %.1f / %.1f / %.1f us)"
              % (name, T * B, C, r, what, copy, fwd, fwd / copy, bwd, bwd / copy, t_copy * 1e6, t_fwd * 1e6, t_bwd * 1e6), flush=True)


def step_probe(name, steps=10, rounds=3):
    w = bench.WORKLOADS[name]
    T, B, L = w["T"], w["B"], w["cfg"]["num_layers"]
    settings = SETTINGS[name]
    graphs = {s: create_graph_for_training_ctc(None, dict(w["cfg"], time_reduce_layers=s if "," in s else int(s)), learn_rate=4e-4,
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
        print("%s T=%d B=%d, %-26s: %s ms/step (mean %.2f, spread %.2f) -> %.1f k input frames/s, logits [%d, %d, V]" % (
            name, T, B, name_of(s), " ".join("%.2f" % t for t in ms[s]), mean[s], spread[s], T * B / mean[s],
            graphs[s].model.output_frames(T), B), flush=True)
    for s in settings[1:]:
        d = mean[s] - mean[settings[0]]
        verdict = ("beyond both spreads" if abs(d) > spread[s] + spread[settings[0]] else "WITHIN the runs' spreads")
        print("%s: %s is %.2f ms/step %s than plain (%.1f %%), %s" % (
            name, name_of(s), abs(d), "SLOWER" if d > 0 else "faster", 100.0 * d / mean[settings[0]], verdict), flush=True)
    for s in settings:
        model = graphs[s].model
        overlap, model.overlap_wgrad = model.overlap_wgrad, False      # a bracket then holds one kernel's time
        run(s, 1)
        ops.PROFILE = []
        run(s, 1)
        prof, ops.PROFILE = ops.PROFILE, None
        model.overlap_wgrad = overlap
        fwd = [st.elapsed_time(e) for k, _, st, e in prof if k == "lstm_fwd"]
        bwd = [st.elapsed_time(e) for k, _, st, e in prof if k == "lstm_bwd"][::-1]      # the BPTT visits the layers top down
        lay = [st.elapsed_time(e) for k, _, st, e in prof if k == "time_reduce"]
        gemm = sum(st.elapsed_time(e) for k, _, st, e in prof if k.startswith("gemm"))
        assert len(fwd) == L and len(bwd) == L
        print("   %-26s per layer, both directions in one call: forward pass %s ms | BPTT %s ms | recurrences %.1f ms, products "
              "%.1f ms, time-reduce passes %s ms" % (name_of(s), " ".join("%.2f" % t for t in fwd), " ".join("%.2f" % t for t in bwd),
                                                   sum(fwd) + sum(bwd), gemm, " ".join("%.3f" % t for t in lay) or "-"), flush=True)


if __name__ == "__main__":
    what = sys.argv[1:] or ["passes", "c2", "c4"]
    if "passes" in what:
        for name in ("c4", "c2"):
            pass_probe(name)
    for name in ("c2", "c4"):
        if name in what:
            step_probe(name)
