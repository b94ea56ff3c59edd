"""Packed-frames probe (run on the GPU box): lc_pack_rows / lc_unpack_rows alone at c4's shapes with bench.py's ragged
lengths (GB/s from the bytes the shapes say), then one c4 and one c2 ragged train step with pack_frames alternating off / on
in the same process - ten timed steps each after warm-up of both, three alternations - so that the difference is read against
the run-to-run spread of the same box.  Prints text; `python tools/pack_probe.py > profiles/<name>.txt`.

    python tools/pack_probe.py [kernels] [c4] [c2]        (default: all three)"""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from lstm_ctc_amd import ops  # noqa: E402
from lstm_ctc_amd.nnet.frames import FrameMap  # noqa: E402
from lstm_ctc_amd.nnet.graph import create_graph_for_training_ctc  # noqa: E402


def timeit(fn, warmup=3, iters=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e-3


def kernel_probe():
    w = bench.WORKLOADS["c4"]
    _, seq, _, _, _ = bench.synth_batch_ragged(w, 0, "cuda")
    T, B = w["T"], w["B"]
    fm = FrameMap(seq.cpu().numpy(), T, B)
    rows_d, inv_d = fm.device("cuda")
    print("c4 ragged lengths: T*B = %d, M = %d live (%.1f %% dead), Mp = %d" % (T * B, fm.M, 100.0 * (1 - fm.M / (T * B)), fm.Mp))
    for C in (2048, 4096):
        x = torch.randn((T * B, C), device="cuda")
        p = torch.empty((fm.Mp, C), device="cuda")
        u = torch.empty((T * B, C), device="cuda")
        tp = timeit(lambda: ops.pack_rows(x, rows_d, out=p))
        tu = timeit(lambda: ops.unpack_rows(p, inv_d, out=u))
        tc = timeit(lambda: u.copy_(x))
        bp, bu = 4.0 * C * (fm.M + fm.Mp), 4.0 * C * (fm.M + T * B)
        print("C = %4d: pack_rows %.3f ms %.0f GB/s | unpack_rows %.3f ms %.0f GB/s | plain device copy of [T*B, C] %.3f ms %.0f GB/s"
              % (C, tp * 1e3, bp / tp / 1e9, tu * 1e3, bu / tu / 1e9, tc * 1e3, 8.0 * C * T * B / tc / 1e9), flush=True)


def step_probe(name, steps=10, rounds=3):
    w = bench.WORKLOADS[name]
    graph = create_graph_for_training_ctc(None, w["cfg"], learn_rate=4e-4, clip_norm=5.0, optimizer="adam", device="cuda", seed=123)
    x, seq, labels, offs, maxlen = bench.synth_batch_ragged(w, 0, "cuda")
    size = int(labels.numel())
    frames = int(seq.sum().item())

    def run(pack, n):
        graph.model.pack_frames = pack
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            graph.step_device(x, seq, labels, offs, maxlen, size, fetch_eval=False)
        torch.cuda.synchronize()
        assert graph.model.packed is pack
        return (time.perf_counter() - t0) / n

    for pack in (False, True):
        run(pack, 3)                                      # warm-up of both paths
    ms = {False: [], True: []}
    for _ in range(rounds):
        for pack in (False, True):
            ms[pack].append(run(pack, steps) * 1e3)
    assert graph.persist_fallbacks == 0
    for pack in (False, True):
        v = ms[pack]
        print("%s ragged, pack_frames %-3s: %s ms/step (mean %.2f, spread %.2f) -> %.1f k frames/s" % (
            name, "on" if pack else "off", " ".join("%.2f" % t for t in v), sum(v) / len(v), max(v) - min(v),
            frames / (sum(v) / len(v))), flush=True)
    d = sum(ms[False]) / rounds - sum(ms[True]) / rounds
    print("%s ragged: packed is %.2f ms/step %s than padded (%.1f %%)" % (name, abs(d), "faster" if d > 0 else "SLOWER",
                                                                         100.0 * d / (sum(ms[False]) / rounds)))
    # where the time goes: event brackets of one step each (side-stream overlap off, so that a bracket holds one kernel's time)
    overlap, graph.model.overlap_wgrad = graph.model.overlap_wgrad, False
    for pack in (False, True):
        run(pack, 1)
        ops.PROFILE = []
        run(pack, 1)
        prof, ops.PROFILE = ops.PROFILE, None
        agg = {}
        rows_all, fm = w["T"] * w["B"], graph.model.frame_map(seq, w["T"], w["B"])
        for kind, work, s, e in prof:
            key = kind
            if kind == "pack":            # work = 8 n C: which of the four passes, by its shape
                n = rows_all if (work / 8) % rows_all == 0 else fm.Mp
                wide = work / 8 / n == 4 * w["cfg"]["num_neurons"]
                key = ("unpack " + ("zx" if wide else "dX")) if n == rows_all else ("pack " + ("dz" if wide else "X"))
            a = agg.setdefault(key, [0.0, 0])
            a[0] += s.elapsed_time(e)
            a[1] += 1
        print("   pack_frames %-3s, per step:" % ("on" if pack else "off"),
              "; ".join("%s %.2f ms / %d" % (k, v[0], v[1]) for k, v in sorted(agg.items()) if k != "ctc"), flush=True)
    graph.model.overlap_wgrad = overlap


if __name__ == "__main__":
    what = sys.argv[1:] or ["kernels", "c4", "c2"]
    if "kernels" in what:
        kernel_probe()
    for name in ("c4", "c2"):
        if name in what:
            step_probe(name)
