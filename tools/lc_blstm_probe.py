"""Latency-controlled BiLSTM probe (run on the GPU box): the full train step of bench.py's c2 and c4 workloads with the keys
absent and with (chunk_frames, lookahead_frames) = (40, 20) and (100, 40), the three settings alternating in the same process -
ten timed steps each after a warm-up of all, three alternations - so that a difference is read against the run-to-run spread
of the same box.  Then, per setting, event brackets of one step (side-stream overlap off, so that a bracket holds one kernel's
time): per layer the recurrences and the layout passes (lc_chunk_gather / lc_chunk_fold), and the layout passes' rate against a
torch device-to-device copy of a [T*B, 4N] matrix timed in the same run.  Prints text;
`python tools/lc_blstm_probe.py > profiles/lc_blstm_probe.txt`.

    python tools/lc_blstm_probe.py [c2] [c4]        (default: both)"""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from lstm_ctc_amd import ops  # noqa: E402
from lstm_ctc_amd.nnet.graph import create_graph_for_training_ctc  # noqa: E402

SETTINGS = ((0, 0), (40, 20), (100, 40))


def name_of(s):
    return "plain" if not s[0] else "Nc=%d Nr=%d" % s


def copy_rate(rows, C, iters=20):
    """GB/s (read + written) of a torch device-to-device copy of a [rows, C] float32 matrix."""
    a = torch.randn((rows, C), device="cuda")
    b = torch.empty_like(a)
    for _ in range(3):
        b.copy_(a)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        b.copy_(a)
    e.record()
    torch.cuda.synchronize()
    return 8.0 * rows * C / (s.elapsed_time(e) / iters * 1e-3) / 1e9


def step_probe(name, steps=10, rounds=3):
    w = bench.WORKLOADS[name]
    cfg = w["cfg"]
    T, B, N, L = w["T"], w["B"], cfg["num_neurons"], cfg["num_layers"]
    graph = create_graph_for_training_ctc(None, cfg, learn_rate=4e-4, clip_norm=5.0, optimizer="adam", device="cuda", seed=123)
    x, seq, labels, offs = bench.synth_batch(w, 0, "cuda")
    size, maxlen = int(labels.numel()), w["L"]

    def run(setting, n):
        graph.model.chunk, graph.model.lookahead = setting
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            graph.step_device(x, seq, labels, offs, maxlen, size, fetch_eval=False)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n

    for s in SETTINGS:
        run(s, 3)                                         # warm-up of every path
    ms = {s: [] for s in SETTINGS}
    for _ in range(rounds):
        for s in SETTINGS:
            ms[s].append(run(s, steps) * 1e3)
    assert graph.persist_fallbacks == 0
    mean = {s: sum(v) / len(v) for s, v in ms.items()}
    for s in SETTINGS:
        v = ms[s]
        print("%s T=%d B=%d, %-14s: %s ms/step (mean %.2f, spread %.2f) -> %.1f k frames/s" % (
            name, T, B, name_of(s), " ".join("%.2f" % t for t in v), mean[s], max(v) - min(v), T * B / mean[s]), flush=True)
    for s in SETTINGS[1:]:
        d = mean[s] - mean[SETTINGS[0]]
        nC, Tc, Bc = ops.chunk_shape(T, B, *s)
        print("%s: %s (%d chunk rows of %d frames) is %.2f ms/step %s than plain (%.1f %%)" % (
            name, name_of(s), Bc, Tc, abs(d), "SLOWER" if d > 0 else "faster", 100.0 * d / mean[SETTINGS[0]]), flush=True)
    rate = copy_rate(T * B, 4 * N)
    print("%s: torch device-to-device copy of [%d, %d] f32: %.0f GB/s (read + written)" % (name, T * B, 4 * N, rate), flush=True)
    overlap, graph.model.overlap_wgrad = graph.model.overlap_wgrad, False
    for s in SETTINGS:
        run(s, 1)
        ops.PROFILE = []
        run(s, 1)
        prof, ops.PROFILE = ops.PROFILE, None
        fwd = [st.elapsed_time(e) for k, _, st, e in prof if k == "lstm_fwd"]
        bwd = [st.elapsed_time(e) for k, _, st, e in prof if k == "lstm_bwd"]
        lay = [(st.elapsed_time(e), work) for k, work, st, e in prof if k == "chunk"]
        if not s[0]:
            assert len(fwd) == L and len(bwd) == L and not lay
            print("   %-14s per layer, both directions in one call: forward pass %s ms | BPTT %s ms" % (
                name_of(s), " ".join("%.2f" % t for t in fwd), " ".join("%.2f" % t for t in bwd)), flush=True)
            continue
        assert len(fwd) == 2 * L and len(bwd) == 2 * L and len(lay) == 4 * L
        bwd = bwd[::-1]                                   # the BPTT visits the layers top down
        lay_b = lay[2 * L:][::-1]                         # (gather dh, fold dz) per layer, top down
        for i in range(L):
            passes = [lay[2 * i], lay[2 * i + 1], lay_b[2 * i + 1], lay_b[2 * i]]      # gather zx, fold hs, gather dh, fold dz
            t_lay, bytes_lay = sum(p[0] for p in passes), sum(p[1] for p in passes)
            gbs = bytes_lay / (t_lay * 1e-3) / 1e9
            print("   %-14s layer %d: forward direction %.2f + %.2f ms (forward pass + BPTT) | backward direction, chunked %.2f + "
                  "%.2f ms | layout passes %.3f ms (gather zx %.3f, fold hs %.3f, gather dh %.3f, fold dz %.3f): %.0f GB/s = %.2f "
                  "of the copy's rate" % (name_of(s), i, fwd[2 * i], bwd[2 * i + 1], fwd[2 * i + 1], bwd[2 * i], t_lay,
                                          passes[0][0], passes[1][0], passes[2][0], passes[3][0], gbs, gbs / rate), flush=True)
    graph.model.overlap_wgrad = overlap
    graph.model.chunk, graph.model.lookahead = SETTINGS[0]


if __name__ == "__main__":
    what = sys.argv[1:] or ["c2", "c4"]
    for name in ("c2", "c4"):
        if name in what:
            step_probe(name)
