"""lc_consistency_loss against the only way to get its term without it: HIP-event time per call, by raw library calls on
preallocated buffers, of
  1. lc_consistency_loss accumulating into a [T,2B,V] gradient (2 rows read, 2 gradient rows read-modify-written per frame of
     a pair: 6 row passes),
  2. two accumulating lc_kd_loss calls at temperature 1 on contiguous copies of the two halves, each half once as the student
     with the other as its teacher (8 row passes; the copies themselves are made outside the timed window),
  3. a device-to-device copy that moves the bytes of 1. (3 rows read and 3 written per frame of a pair: a buffer of 3 rows
     per pair-frame copied to another),
at [T = 1000, 2B = 128] and V = 44 and 1024, the variants alternating inside every round.  Then one c4-shaped training step
(bench.py's workload) with consistency_weight at B = 32 against the plain step at B = 64 - equal 2B, so the difference is what
the pair term and the doubling cost on top of the doubled batch.  No gate: the figures go to the output file (DESIGN.md
section 3.12 quotes them).
Usage: python tools/consistency_probe.py [output file, default profiles/consistency_probe.txt] [--no-step]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from lstm_ctc_amd import _lib, ops

T, PAIRS = 1000, 64
SHAPES = [(44, 200), (1024, 40)]                       # (V, calls per round)
WARM, ROUNDS = 3, 9
HBM = 8e12
STEP_WARM, STEP_ROUNDS, STEPS_PER_ROUND = 3, 5, 4
ALPHA = 0.2


def timed(variants, reps):
    """{name: (median, min, max)} over ROUNDS of the mean time of `reps` back-to-back calls, in microseconds; every round
    times every variant once, in turn, so that a drift of the machine meets all of them alike."""
    for _, fn in variants:
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    out = {name: [] for name, _ in variants}
    for _ in range(ROUNDS):
        for name, fn in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out[name].append(e0.elapsed_time(e1) / reps * 1e3)
    return {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in out.items()}, out


def op_lines(lib):
    p, st = ops._ptr, ops._stream
    lines = []
    for V, reps in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(5)
        logits = torch.randn((T, 2 * PAIRS, V), device="cuda", generator=g) * 3.0
        half_a, half_b = logits[:, :PAIRS].contiguous(), logits[:, PAIRS:].contiguous()
        seq = torch.full((PAIRS,), T, dtype=torch.int32, device="cuda")
        loss = torch.empty(PAIRS, device="cuda")
        n1, n2 = torch.empty(PAIRS, dtype=torch.int32, device="cuda"), torch.empty(PAIRS, dtype=torch.int32, device="cuda")
        grad = torch.zeros((T, 2 * PAIRS, V), device="cuda")
        grad_a, grad_b = torch.zeros((T, PAIRS, V), device="cuda"), torch.zeros((T, PAIRS, V), device="cuda")
        src, dst = torch.zeros(3 * T * PAIRS * V, device="cuda"), torch.empty(3 * T * PAIRS * V, device="cuda")      # 12 V bytes a side
        cr_bytes, kd_bytes = lib.lc_consistency_workspace_bytes(T, PAIRS, V), lib.lc_kd_workspace_bytes(T, PAIRS, V)
        ws = torch.empty(max(cr_bytes, kd_bytes), dtype=torch.uint8, device="cuda")

        def fused():
            _lib.check(lib.lc_consistency_loss(p(logits), T, PAIRS, V, p(seq), 0.1, p(loss), p(n1), p(n2), p(grad), 1, p(ws),
                                               cr_bytes, st()), "lc_consistency_loss")

        def two_kd():
            for student, teacher, gr in ((half_a, half_b, grad_a), (half_b, half_a, grad_b)):
                _lib.check(lib.lc_kd_loss(p(student), p(teacher), T, PAIRS, V, p(seq), p(seq), 1.0, 0.1, p(loss), p(n1), p(n2),
                                          p(gr), 1, p(ws), kd_bytes, st()), "lc_kd_loss")

        variants = [("lc_consistency_loss accumulate", fused), ("2 x lc_kd_loss accumulate", two_kd),
                    ("copy, 3 rows in and 3 out", lambda: dst.copy_(src))]
        res, raw = timed(variants, reps)
        frames = T * PAIRS
        moved = {"lc_consistency_loss accumulate": frames * (24 * V + 8), "2 x lc_kd_loss accumulate": frames * (32 * V + 32),
                 "copy, 3 rows in and 3 out": frames * 24 * V}
        lines.append("T=%d 2B=%d V=%d (%.1f MB of logits, %d calls per round):" % (T, 2 * PAIRS, V, T * 2 * PAIRS * V * 4 / 1e6, reps))
        base = res["lc_consistency_loss accumulate"][0]
        for name, _ in variants:
            med, lo, hi = res[name]
            lines.append("    %-32s %.1f [%.1f .. %.1f] us, %.0f GB/s (%.0f%%), x %.2f"
                         % (name, med, lo, hi, moved[name] / med / 1e3, 100 * moved[name] / (med * 1e-6) / HBM, med / base))
        ratio = np.asarray(raw["2 x lc_kd_loss accumulate"]) / np.asarray(raw["lc_consistency_loss accumulate"])
        lines.append("    two kd calls / fused, round by round: median %.2f [%.2f .. %.2f]"
                     % (float(np.median(ratio)), float(ratio.min()), float(ratio.max())))
    return lines


def step_lines():
    import bench
    from lstm_ctc_amd.nnet.graph import create_graph_for_training_ctc
    w = bench.WORKLOADS["c4"]
    runs = []
    for name, B, kw in (("consistency_weight=%g at B=32 (64 columns)" % ALPHA, 32, dict(consistency_weight=ALPHA)),
                        ("plain step at B=64", 64, {})):
        graph = create_graph_for_training_ctc(None, w["cfg"], learn_rate=1e-4, seed=777, **kw)
        x, seq, labels, offs = bench.synth_batch(dict(w, B=B), 0, graph.model.device)
        runs.append((name, graph, lambda graph=graph, a=(x, seq, labels, offs, w["L"], B * w["L"]): graph.step_device(*a)))
    for _, _, step in runs:
        for _ in range(STEP_WARM):
            step()
    ms = {name: [] for name, _, _ in runs}
    for _ in range(STEP_ROUNDS):
        for name, _, step in runs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(STEPS_PER_ROUND):
                step()                                  # ends in the step's device-to-host copy: a synchronise
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / STEPS_PER_ROUND * 1e3)
    lines = ["%s, T=%d: one training step, host clock around %d steps, %d rounds alternating:"
             % (w["desc"].split(":")[0], w["T"], STEPS_PER_ROUND, STEP_ROUNDS)]
    for name, graph, _ in runs:
        v = ms[name]
        lines.append("    %-42s %.1f [%.1f .. %.1f] ms, persist_fallbacks %d"
                     % (name, float(np.median(v)), min(v), max(v), graph.persist_fallbacks))
    names = [name for name, _, _ in runs]
    ratio = np.asarray(ms[names[0]]) / np.asarray(ms[names[1]])
    lines.append("    with the option / plain, round by round: median %.3f [%.3f .. %.3f]"
                 % (float(np.median(ratio)), float(ratio.min()), float(ratio.max())))
    return lines


def main():
    argv = [a for a in sys.argv[1:] if not a.startswith("--")]
    lib = _lib.load()
    lines = ["# tools/consistency_probe.py on %s: %d rounds per figure, median [min .. max] of the rounds' mean time per call, us;"
             % (torch.cuda.get_device_name(0), ROUNDS),
             "# GB/s = the bytes the call has to move per frame of a pair (fused: 24 V + 8; two kd calls: 32 V + 32; copy: 24 V) "
             "/ median time; % = of 8 TB/s; x = time / lc_consistency_loss's"]
    lines += op_lines(lib)
    if "--no-step" not in sys.argv[1:]:
        lines += step_lines()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    out = argv[0] if argv else os.path.join(ROOT, "profiles", "consistency_probe.txt")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
