#!/usr/bin/env python3
"""Generates tests/golden/frame_loss_bits.json: the SHA-256 of the raw bytes of every output of lc_xent_loss, lc_kd_loss and
lc_consistency_loss on a fixed set of cases.  tests/test_gpu_frame_loss_bits.py rebuilds the cases through cases() /
run_case() below and asserts the same hashes: the three frame criteria are bit-reproducible, and a change that does not mean
to alter their arithmetic (a refactor, a compiler flag) must leave every bit where it is.  A change that DOES mean to alter it
regenerates the file (`python tests/golden/make_frame_loss_bits.py`, on the GPU) and says so.

Every input comes from numpy.random.default_rng(seed) on the host, as integers scaled by a power of two (exact in float32, no
transcendental on the way): nothing is drawn on the GPU and nothing depends on a host libm.  The calls are raw library calls,
so that every buffer of a case can sit off the 16-byte boundary.

Cases (the smallest shapes at which each dispatch path can go wrong):
  ladder   V in LADDER at T = 9, B = 3 (27 frames: with four frames per wave a group wraps from one t to the next inside a
           wave and the last wave holds an invalid group), lengths [9, 5, 0] and [3, 2, 0] (whole waves unscored)
  b1       B = 1, T = 7 at V = 44 and 300: one direct row per wave, the FW - 1 wraps
  off      every float buffer a view from element 1 of a larger allocation, V = 44 and 1028
  grid     more frames than one pass of the grid, overwrite only
Half of the cases carry special rows: a single -inf teacher element, an all -inf teacher row on a scored frame (bad), a +inf in
one view (bad), two pair-frames with identical halves, a target V on a live frame (bad).
Per case: xent with and without a gradient; kd at (temperature, grad_scale) = (1, 1) and (2, 0.3), consistency at grad_scale 1
and 0.3, each overwriting, and at the second setting without a gradient and accumulating into an rng-filled tensor."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "frame_loss_bits.json")
LADDER = [4, 44, 45, 64, 65, 256, 257, 512, 516, 1024, 1028, 1101]
GRID = [(11000, 3, 4), (2750, 3, 65), (2750, 3, 1028)]


def cases():
    """[(case id, spec)]; a spec is all a case is made from."""
    out = []

    def add(kind, T, B, V, lens, tlens, special, off=False, modes=True):
        cid = "%s-T%d-B%d-V%d-len%s%s" % (kind, T, B, V, "_".join(map(str, lens)), "-special" if special else "")
        out.append((cid, dict(seed=len(out) + 1, T=T, B=B, V=V, lens=lens, tlens=tlens, special=special, off=off, modes=modes)))

    for i, V in enumerate(LADDER):
        for k, lens in enumerate(([9, 5, 0], [3, 2, 0])):
            add("ladder", 9, 3, V, lens, [7, 9, 4], (i + k) % 2 == 1)
    for V in (44, 300):
        for special in (False, True):
            add("b1", 7, 1, V, [5], [4], special)
    add("off", 9, 3, 44, [9, 5, 0], [7, 9, 4], False, off=True)
    add("off", 9, 3, 1028, [9, 5, 0], [7, 9, 4], True, off=True)
    for T, B, V in GRID:
        add("grid", T, B, V, [T, T // 3, 0], [T - 3, T, T // 2], False, modes=False)
    return out


def _floats(rng, shape):
    """Multiples of 1/4096 in [-8, 8): exact in float32."""
    return (rng.integers(-32768, 32768, size=shape).astype(np.float32) / np.float32(4096.0)).astype(np.float32)


def inputs(spec):
    """The host arrays of a case, drawn in a fixed order."""
    rng = np.random.default_rng(spec["seed"])
    T, B, V = spec["T"], spec["B"], spec["V"]
    d = dict(logits=_floats(rng, (T, B, V)), teacher=_floats(rng, (T, B, V)), pair=_floats(rng, (T, 2 * B, V)),
             into=_floats(rng, (T, B, V)), into_pair=_floats(rng, (T, 2 * B, V)),
             targets=rng.integers(0, V, size=(B, T)).astype(np.int32),
             lens=np.array(spec["lens"], np.int32), tlens=np.array(spec["tlens"], np.int32))
    d["targets"][:, 3::4] = -1                           # ignored
    d["targets"][0, 0] = V - 1                           # the blank
    if spec["special"]:                                  # all on frames that every set of lengths scores
        b1 = min(1, B - 1)
        d["targets"][0, 1] = V                           # bad target on a live frame
        d["teacher"][1, 0, V // 2] = -np.inf             # probability 0
        d["teacher"][0, b1, :] = -np.inf                 # bad teacher row
        d["pair"][1, B + b1, V - 1] = np.inf             # bad row in view b
        d["pair"][0, B, :] = d["pair"][0, 0, :]          # identical halves
        d["pair"][2, B, :] = d["pair"][2, 0, :]
    return d


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def run_case(spec):
    """{run: {output: sha256}} of a case on cuda:0."""
    import torch
    from lstm_ctc_amd import _lib, ops
    lib = _lib.load()
    p, st = ops._ptr, ops._stream
    T, B, V = spec["T"], spec["B"], spec["V"]
    h = inputs(spec)

    def dev(a):
        a = torch.from_numpy(a)
        if not spec["off"] or not a.is_floating_point():
            return a.cuda()
        buf = torch.zeros(a.numel() + 1, device="cuda")
        view = buf[1:].view(a.shape)
        view.copy_(a)
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        return view

    logits, teacher, pair = dev(h["logits"]), dev(h["teacher"]), dev(h["pair"])
    targets, lens, tlens = dev(h["targets"]), dev(h["lens"]), dev(h["tlens"])
    nbytes = max(lib.lc_xent_workspace_bytes(T, B, V), lib.lc_kd_workspace_bytes(T, B, V),
                 lib.lc_consistency_workspace_bytes(T, B, V))
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
    out = {}

    def run(name, call, grad):
        """grad: None, "nan" + a shape (overwrite: prefilled with NaN) or a host array to accumulate into."""
        loss = torch.full((B,), float("nan"), device="cuda")
        n1 = torch.full((B,), -77, dtype=torch.int32, device="cuda")
        n2 = torch.full((B,), -77, dtype=torch.int32, device="cuda")
        acc = isinstance(grad, np.ndarray)
        g = None if grad is None else dev(grad) if acc else dev(np.full(grad, np.nan, np.float32))
        call(loss, n1, n2, g, 1 if acc else 0)
        torch.cuda.synchronize()
        out[name] = dict(loss=_sha(loss), frames=_sha(n1), agree=_sha(n2))
        if g is not None:
            out[name]["grad"] = _sha(g)

    def xent(loss, n1, n2, g, acc):
        _lib.check(lib.lc_xent_loss(p(logits), T, B, V, p(targets), p(lens), p(loss), p(n1), p(n2), p(g), p(ws), nbytes, st()),
                   "lc_xent_loss")

    def kd(tau, scale):
        return lambda loss, n1, n2, g, acc: _lib.check(
            lib.lc_kd_loss(p(logits), p(teacher), T, B, V, p(lens), p(tlens), tau, scale, p(loss), p(n1), p(n2), p(g), acc,
                           p(ws), nbytes, st()), "lc_kd_loss")

    def cr(scale):
        return lambda loss, n1, n2, g, acc: _lib.check(
            lib.lc_consistency_loss(p(pair), T, B, V, p(lens), scale, p(loss), p(n1), p(n2), p(g), acc, p(ws), nbytes, st()),
            "lc_consistency_loss")

    run("xent", xent, (T, B, V))
    run("kd-tau1-scale1", kd(1.0, 1.0), (T, B, V))
    run("kd-tau2-scale0.3", kd(2.0, 0.3), (T, B, V))
    run("cr-scale1", cr(1.0), (T, 2 * B, V))
    run("cr-scale0.3", cr(0.3), (T, 2 * B, V))
    if spec["modes"]:
        run("xent-nograd", xent, None)
        run("kd-tau2-scale0.3-nograd", kd(2.0, 0.3), None)
        run("kd-tau2-scale0.3-acc", kd(2.0, 0.3), h["into"])
        run("cr-scale0.3-nograd", cr(0.3), None)
        run("cr-scale0.3-acc", cr(0.3), h["into_pair"])
    return out


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    path = sys.argv[1] if len(sys.argv) > 1 else OUT
    table = {cid: run_case(spec) for cid, spec in cases()}
    with open(path, "w") as fh:
        json.dump(table, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print("wrote %d cases to %s" % (len(table), path))


if __name__ == "__main__":
    main()
