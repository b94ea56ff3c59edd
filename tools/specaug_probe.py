"""lc_spec_augment alone: HIP-event time per call of the pass at the recipes' shapes, beside a torch device-to-device copy of
the same tensor in the same process - the yardstick: the pass moves the same bytes (one read and one write of [T, B, D]).  No
gate: both figures and their ratio go to the output file (DESIGN.md section 3.11 quotes them).
Variants: the recipe's settings (time=2x40 capped at 20 percent, freq=2x15 of 40 bins) on full-length and on ragged utterances,
the same with the plan written, and no masks at all (every row takes the plain-copy branch).
Usage: python tools/specaug_probe.py [output file, default profiles/specaug_probe.txt]"""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from lstm_ctc_amd import _lib, ops
from lstm_ctc_amd.nnet.augment import SpecAugment

# (T, B, base_dim, left, right, subsample, calls per round)
SHAPES = [(1000, 64, 40, 0, 0, 1, 400), (1000, 64, 120, 1, 1, 3, 100), (334, 256, 120, 1, 1, 3, 100)]
WARM, ROUNDS = 3, 7
RECIPE = SpecAugment(time_masks=2, time_width=40, time_percent=20, freq_masks=2, freq_width=15, freq_bins=40)
NONE = SpecAugment(freq_bins=40)


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
    p, st = ops._ptr, ops._stream
    lines = ["# tools/specaug_probe.py on %s: %d rounds per figure, median [min .. max] of the rounds' mean time per call, us;"
             % (torch.cuda.get_device_name(0), ROUNDS),
             "# GB/s = 8 bytes per element (one read, one write) / median time; x = time / the torch copy's (out.copy_(x), same "
             "tensors, same process)"]
    for T, B, base, left, right, sub, reps in SHAPES:
        D = base * (1 + left + right)
        g = torch.Generator(device="cuda").manual_seed(5)
        x = torch.randn((T, B, D), device="cuda", generator=g)
        out = torch.empty_like(x)
        full = torch.full((B,), T, dtype=torch.int32, device="cuda")
        ragged = torch.randint(T // 2, T + 1, (B,), device="cuda", generator=g, dtype=torch.int32)
        plan = torch.empty((B, 16, 2), dtype=torch.int32, device="cuda")
        seed = [0]

        def aug(spec, seq, plan_d=None):
            cfg = _lib.SpecAugmentConfig(spec.time_masks, spec.time_width, spec.time_percent, spec.freq_masks, spec.freq_width,
                                         spec.freq_bins, base, left, right, sub, spec.fill)
            seed[0] += 1                                   # new masks every call, as in training
            _lib.check(lib.lc_spec_augment(p(x), T, B, D, D, p(seq), ctypes.byref(cfg), seed[0], p(out), D, p(plan_d), st()),
                       "lc_spec_augment")

        variants = [("torch copy", lambda: out.copy_(x)),
                    ("lc_spec_augment recipe, full lengths", lambda: aug(RECIPE, full)),
                    ("lc_spec_augment recipe, ragged", lambda: aug(RECIPE, ragged)),
                    ("lc_spec_augment recipe + plan", lambda: aug(RECIPE, full, plan)),
                    ("lc_spec_augment no masks", lambda: aug(NONE, full))]
        nbytes = 8.0 * T * B * D
        lines.append("T=%d B=%d D=%d (base %d, contexts %d/%d, subsample %d; %.1f MB, %d calls per round):"
                     % (T, B, D, base, left, right, sub, T * B * D * 4 / 1e6, reps))
        ref = None
        for name, fn in variants:
            med, lo, hi = timed(fn, reps)
            ref = med if ref is None else ref
            lines.append("    %-38s %.1f [%.1f .. %.1f] us, %.0f GB/s, x %.2f" % (name, med, lo, hi, nbytes / med / 1e3, med / ref))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    argv = sys.argv[1:]
    path = argv[0] if argv else os.path.join(root, "profiles", "specaug_probe.txt")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
