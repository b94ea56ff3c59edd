"""Row-convolution probe (run on the GPU box): lc_row_conv_fwd and lc_row_conv_bwd (dx alone, dw alone, both) at c1's top
shape (T = 1000, B = 32, C = 256) and at a 1024-wide one (T = 1000, B = 64), for tau = 2, 8 and 32, each as a multiple of
lc_chunk_gather with one chunk - a plain copy of the same bytes, the in-project yardstick of a streaming pass - timed in the
same process.  Then the full train step of bench.py's c1 workload with the key off and with row_conv_frames = 4, the two
alternating - ten timed steps each, three alternations - so that the difference is read against the box's own spread.
Writes profiles/row_conv_probe.txt (or the path given) and prints the same text.

    python tools/row_conv_probe.py [out.txt]"""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from lstm_ctc_amd import ops  # noqa: E402
from lstm_ctc_amd.nnet.graph import create_graph_for_training_ctc  # noqa: E402

SHAPES = ((1000, 32, 256), (1000, 64, 1024))
TAUS = (2, 8, 32)
LINES = []


def say(line):
    LINES.append(line)
    print(line, flush=True)


def timed(fn, iters=20):
    """Mean microseconds of fn() over `iters` back-to-back calls between two events, after three warm-up calls."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3


def kernel_probe(T, B, C):
    rows = T * B
    x, dy = torch.randn((rows, C), device="cuda"), torch.randn((rows, C), device="cuda")
    y, dx = torch.empty_like(x), torch.empty_like(x)
    seq = torch.full((B,), T, dtype=torch.int32, device="cuda")
    copy = timed(lambda: ops.chunk_gather(x, T, B, T, 0, out=y))
    gb = 8.0 * rows * C / 1e9
    say("T=%d B=%d C=%d: lc_chunk_gather, one chunk (a copy of %.0f MB): %.1f us = %.0f GB/s read + written"
        % (T, B, C, 4.0 * rows * C / 1e6, copy, gb / (copy * 1e-6)))
    for tau in TAUS:
        w = torch.randn((tau + 1, C), device="cuda")
        dw = torch.empty_like(w)
        t_f = timed(lambda: ops.row_conv_fwd(x, w, seq, T, B, out=y))
        t_dx = timed(lambda: ops.row_conv_bwd(x, dy, w, seq, T, B, want_dw=False, dx=dx))
        t_dw = timed(lambda: ops.row_conv_bwd(x, dy, w, seq, T, B, want_dx=False, dw=dw))
        t_b = timed(lambda: ops.row_conv_bwd(x, dy, w, seq, T, B, dx=dx, dw=dw))
        say("   tau=%2d: fwd %.1f us (%.2f x copy, %.0f GB/s of x + y) | bwd dx %.1f us (%.2f x) | dw %.1f us (%.2f x) | dx + dw in "
            "one call %.1f us (%.2f x)" % (tau, t_f, t_f / copy, gb / (t_f * 1e-6), t_dx, t_dx / copy, t_dw, t_dw / copy, t_b,
                                          t_b / copy))


def step_probe(tau=4, steps=10, rounds=3):
    w = bench.WORKLOADS["c1"]
    graphs = {}
    for key in (0, tau):
        cfg = dict(w["cfg"], **({"row_conv_frames": key} if key else {}))
        graphs[key] = create_graph_for_training_ctc(None, cfg, learn_rate=4e-4, clip_norm=5.0, optimizer="adam", device="cuda",
                                                    seed=123)
    x, seq, labels, offs = bench.synth_batch(w, 0, "cuda")
    size, maxlen = int(labels.numel()), w["L"]

    def run(key, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            graphs[key].step_device(x, seq, labels, offs, maxlen, size, fetch_eval=False)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n

    for key in graphs:
        run(key, 3)
    ms = {key: [] for key in graphs}
    for _ in range(rounds):
        for key in graphs:
            ms[key].append(run(key, steps) * 1e3)
    mean = {key: sum(v) / len(v) for key, v in ms.items()}
    for key, v in ms.items():
        say("c1 T=%d B=%d, %-20s: %s ms/step (mean %.3f, spread %.3f)" % (
            w["T"], w["B"], "row_conv_frames = %d" % key if key else "key off", " ".join("%.3f" % t for t in v), mean[key],
            max(v) - min(v)))
    d = mean[tau] - mean[0]
    say("c1: row_conv_frames = %d costs %+.3f ms/step (%+.1f %%)" % (tau, d, 100.0 * d / mean[0]))


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "row_conv_probe.txt")
    say("# tools/row_conv_probe.py on %s" % torch.cuda.get_device_name(0))
    for shape in SHAPES:
        kernel_probe(*shape)
    step_probe()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(LINES) + "\n")
