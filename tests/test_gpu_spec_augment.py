"""lc_spec_augment on the GPU against its numpy definition (nnet.augment.apply_host / mask_plan), bit for bit, at every launch
geometry and buffer edge; every LC_EINVAL with outputs untouched; and the graph option: a training step reads the masked input,
out of place, seeded by the step's dropout seed."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from lstm_ctc_amd.nnet import augment  # noqa: E402
from lstm_ctc_amd.nnet.augment import SpecAugment, apply_host, mask_plan  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GUARD = 64                    # floats in front of and behind every buffer
SENTINEL = 777.25             # what guards and the columns beyond D hold


def _spec(time=(0, 0), freq=(0, 0), bins=4, cap=100, fill=0.0):
    return SpecAugment(time_masks=time[0], time_width=time[1], time_percent=cap, freq_masks=freq[0], freq_width=freq[1],
                       freq_bins=bins, fill=fill)


# name: T, B, base_dim, l, r, subsample, spec, seq_len (None: ragged, drawn), x pitch - D, out pitch - D, base offset in floats,
#       what the host mirror must show before the GPU is asked (m = an element masked, p = a row with some blocks time-masked
#       and others not, e = a time mask holds raw frame 0 or n - 1), seed (None: the first that shows all of it)
CASES = {
    # the two plans of tests/test_spec_augment_host.py; seed 777 happens to touch no utterance's first or last frame, so the
    # same shape runs again with a seed that does
    "plan_777":       (9, 5, 16, 1, 1, 3, _spec((2, 6), (2, 3), 8, cap=40), [9, 7, 4, 1, 0], 0, 0, 0, "mp", 777),
    "plan_777_edge":  (9, 5, 16, 1, 1, 3, _spec((2, 6), (2, 3), 8, cap=40, fill=-3.5), [9, 7, 4, 1, 0], 0, 0, 0, "mpe", None),
    "plan_5":         (12, 3, 4, 2, 2, 1, _spec((2, 4), (1, 2), 4), [12, 5, 2], 0, 0, 0, "mpe", 5),
    # scalar path: D no multiple of 4; a base 4 bytes off a 16-byte boundary; pitches that are no multiples of 4
    "scalar_d18":     (7, 3, 6, 1, 1, 2, _spec((2, 5), (2, 2), 3, fill=2.0), None, 0, 0, 0, "mpe", None),
    "misaligned":     (7, 3, 8, 1, 1, 3, _spec((2, 9), (2, 3), 4), None, 0, 0, 1, "mpe", None),
    "scalar_pitch":   (7, 3, 8, 1, 1, 3, _spec((2, 9), (2, 3), 4, fill=-1.0), None, 1, 3, 0, "mpe", None),
    # 16-byte path under pitches larger than D
    "vector_pitch":   (7, 3, 8, 1, 1, 3, _spec((2, 9), (2, 3), 4), None, 4, 8, 0, "mpe", None),
    # the narrowest and the recipes' row: one vector per row (16 lanes a row), 90 vectors (128 lanes a row)
    "d4":             (6, 5, 4, 0, 0, 1, _spec((2, 3), (1, 2), 2, fill=1.5), None, 0, 0, 0, "m", None),
    "d360":           (6, 3, 120, 1, 1, 3, _spec((2, 10), (2, 15), 40, cap=60), None, 0, 0, 0, "mpe", None),
    # the other lane counts: 24 scalars (32 lanes), 60 vectors (64), 150 vectors (256, one vector per lane)
    "d240":           (5, 3, 80, 1, 1, 3, _spec((2, 10), (2, 15), 40), None, 0, 0, 0, "mpe", None),
    "d600":           (5, 2, 200, 1, 1, 3, _spec((2, 10), (2, 15), 40), None, 0, 0, 0, "mpe", None),
    # rows wider than a workgroup (a lane walks several vectors and divides on the fly): 258 vectors; 270 scalars in 15 blocks
    "d1032":          (4, 2, 344, 1, 1, 2, _spec((2, 6), (2, 5), 8, fill=4.0), None, 0, 0, 0, "mpe", None),
    "d270_15blocks":  (9, 2, 18, 7, 7, 1, _spec((3, 4), (2, 3), 6), None, 0, 0, 0, "mpe", None),
    # more than 64 bins, or more than 32 blocks: the rows' masks stay (start, width) pairs instead of one bit word
    "bins80":         (6, 3, 80, 1, 1, 3, _spec((2, 9), (2, 70), 80, fill=3.0), None, 0, 0, 0, "mpe", None),
    "blocks33":       (40, 2, 2, 16, 16, 1, _spec((3, 12), (1, 1), 2), None, 0, 0, 0, "mpe", None),
    "d1032_bins86":   (4, 2, 344, 1, 1, 2, _spec((2, 6), (2, 60), 86), None, 0, 0, 0, "mpe", None),
    "b1":             (9, 1, 8, 1, 1, 3, _spec((2, 9), (2, 3), 4), [9], 0, 0, 0, "mpe", None),
    "t1":             (1, 4, 8, 1, 1, 3, _spec((2, 3), (2, 3), 4), [1, 1, 0, 1], 0, 0, 0, "mpe", None),
    # nothing live: a copy, and the plan's frequency rows are still drawn
    "all_empty":      (4, 3, 8, 1, 1, 3, _spec((2, 9), (2, 3), 4), [0, 0, 0], 0, 0, 0, "", 11),
    # zero masks of either kind, and of both (a pure copy)
    "no_time_masks":  (7, 3, 8, 1, 1, 3, _spec((0, 9), (2, 3), 4), None, 0, 0, 0, "m", None),
    "no_freq_masks":  (7, 3, 8, 1, 1, 3, _spec((2, 9), (0, 3), 4), None, 0, 0, 0, "mpe", None),
    "no_masks":       (7, 3, 8, 1, 1, 3, _spec((0, 9), (0, 3), 4), None, 0, 0, 0, "", 11),
    "zero_widths":    (7, 3, 8, 1, 1, 3, _spec((2, 0), (2, 0), 4), None, 0, 0, 0, "", 11),
    # a frequency mask may take every bin: "F" below asks for an utterance whose rows are masked whole
    "freq_all_bins":  (5, 3, 8, 1, 1, 3, _spec((0, 0), (1, 4), 4, fill=-2.0), None, 0, 0, 0, "mF", None),
    # more row groups than the launch's 2048 workgroups (64 rows a group at this width): the grid stride runs twice
    "grid_stride":    (2100, 64, 4, 0, 0, 1, _spec((2, 300), (1, 2), 4, cap=30, fill=0.5), None, 0, 0, 0, "m", None),
}


def _seq(name, T, B, given):
    if given is not None:
        return np.asarray(given, np.int32)
    rng = np.random.default_rng(len(name))
    seq = rng.integers(0, T + 1, size=B).astype(np.int32)
    seq[0] = T
    return seq


def _shows(plan, seq, spec, base, l, r, s, x, want):
    """Whether the host mirror shows everything ``want`` asks for."""
    T, B, D = x.shape
    ss, nb = max(s, 1), 1 + l + r
    ref = apply_host(x, seq, plan, spec, base, l, r, s)
    changed = ref.view(np.uint32) != x.view(np.uint32)
    if "m" in want and not changed.any():
        return False
    if "p" in want:
        onlytime = apply_host(x, seq, plan, _spec((spec.time_masks, spec.time_width), (0, 0), spec.freq_bins,
                                                  spec.time_percent, 1e30), base, l, r, s)
        blocks = (onlytime == np.float32(1e30)).reshape(T, B, nb, base).all(axis=3)
        if not (blocks.any(axis=2) & ~blocks.all(axis=2)).any():
            return False
    if "e" in want:
        n = seq.astype(np.int64) * ss
        t0, w = plan[:, :8, 0].astype(np.int64), plan[:, :8, 1].astype(np.int64)
        live = (n > 0)[:, None] & (w > 0)
        if not (live & ((t0 == 0) | (t0 + w == n[:, None]))).any():
            return False
    if "F" in want:
        full = (plan[:, 8, 1] == spec.freq_bins) & (seq > 0)
        if not full.any() or not all(changed[:seq[b], b].all() for b in np.nonzero(full)[0]):
            return False
    return True


def _buffer(T, B, D, pad, offset):
    """A guarded device buffer and its [T, B, D] view (rows at pitch D + pad, the first ``offset`` floats behind the guard)."""
    ld = D + pad
    flat = torch.full((GUARD + offset + T * B * ld + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    return flat, flat.as_strided((T, B, D), (B * ld, ld, 1), GUARD + offset)


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_matches_the_host_mirror_bit_for_bit(name):
    from lstm_ctc_amd import ops
    T, B, base, l, r, s, spec, seq, pad_x, pad_o, offset, want, seed = CASES[name]
    D = base * (1 + l + r)
    seq = _seq(name, T, B, seq)
    rng = np.random.default_rng(1)
    x = rng.standard_normal((T, B, D)).astype(np.float32)
    x[T - 1, B - 1, D - 1] = np.nan                                   # must come through bit for bit wherever it is copied
    x.view(np.uint32)[0, 0, 0] = 0x7fc12345                           # a NaN with a payload
    if seed is None:
        seed = next((k for k in range(2000) if _shows(mask_plan(k, seq, spec, s), seq, spec, base, l, r, s, x, want)), None)
        assert seed is not None, "no seed below 2000 makes this case test what it is for"
    plan = mask_plan(seed, seq, spec, s)
    assert _shows(plan, seq, spec, base, l, r, s, x, want)
    if name == "plan_777":
        assert plan[0, :2].tolist() == [[16, 4], [4, 1]] and plan[4, 8:10].tolist() == [[3, 0], [4, 0]]
    if name == "grid_stride":
        assert (T * B + 63) // 64 > 2048
    ref = apply_host(x, seq, plan, spec, base, l, r, s)
    layout = (base, l, r, s)
    seq_d = torch.from_numpy(seq).cuda()

    x_flat, x_view = _buffer(T, B, D, pad_x, offset)
    x_view.copy_(torch.from_numpy(x))
    x_before = _bits(x_flat).copy()
    want_flat, want_view = _buffer(T, B, D, pad_o, offset)            # the whole output buffer as it must look afterwards
    want_view.copy_(torch.from_numpy(ref))
    want_bits = _bits(want_flat)

    results = []
    for call in range(2):                                              # two calls: identical bits
        o_flat, o_view = _buffer(T, B, D, pad_o, offset)
        o_view.fill_(float("nan"))
        plan_d = torch.full((B + 2, 16, 2), -7, dtype=torch.int32, device="cuda")
        got, got_plan = ops.spec_augment(x_view, seq_d, spec, layout, seed, out=o_view, plan=plan_d[1:B + 1])
        torch.cuda.synchronize()
        assert got.data_ptr() == o_view.data_ptr()
        assert np.array_equal(_bits(o_flat), want_bits), name         # D columns = the mirror; pitch columns and guards untouched
        p = plan_d.cpu().numpy()
        assert np.array_equal(p[1:B + 1], plan) and (p[0] == -7).all() and (p[B + 1] == -7).all()
        assert np.array_equal(_bits(x_flat), x_before)                # out of place: the input is only read
        results.append(_bits(o_flat))
    assert np.array_equal(results[0], results[1])
    # without a plan buffer, into a tensor of its own
    alone = ops.spec_augment(x_view, seq_d, spec, layout, seed)
    assert alone.is_contiguous() and np.array_equal(_bits(alone), ref.view(np.uint32))
    # in place equals out of place (the x buffer has the x pitch: compare the views, then the rest of the buffer)
    same = ops.spec_augment(x_view, seq_d, spec, layout, seed, out=x_view)
    torch.cuda.synchronize()
    assert same.data_ptr() == x_view.data_ptr() and np.array_equal(_bits(x_view), ref.view(np.uint32))
    x_view.copy_(torch.from_numpy(x))
    assert np.array_equal(_bits(x_flat), x_before)                    # so nothing outside the view had been written


def test_seed_and_utterance_slot_select_the_draw():
    """The same utterance length in another batch slot, and the same slot under another seed, draw other masks; the low 32 bits
    of the seed are what counts."""
    from lstm_ctc_amd import ops
    spec = _spec((4, 30), (4, 10), 20)
    seq = np.full(6, 40, np.int32)
    x = torch.randn(40, 6, 40, device="cuda")
    seq_d = torch.from_numpy(seq).cuda()
    plans = {}
    for seed in (1, 2, 1 + 2 ** 32):
        _, p = ops.spec_augment(x, seq_d, spec, (40, 0, 0, 0), seed, plan=True)
        plans[seed] = p.cpu().numpy()
        assert np.array_equal(plans[seed], mask_plan(seed, seq, spec, 0))
    assert not np.array_equal(plans[1], plans[2]) and np.array_equal(plans[1], plans[1 + 2 ** 32])
    assert len({plans[1][b].tobytes() for b in range(6)}) == 6


# ----------------------------------------------------------------------------------------------- LC_EINVAL
def test_every_bad_argument_is_refused_with_outputs_untouched():
    from lstm_ctc_amd import _lib
    lib = _lib.load()
    T, B, D = 3, 2, 24
    x = torch.randn(T, B, D, device="cuda")
    out = torch.full((T, B, D), float("nan"), device="cuda")
    plan = torch.full((B, 16, 2), -7, dtype=torch.int32, device="cuda")
    seq = torch.tensor([3, 2], dtype=torch.int32, device="cuda")
    ok = dict(time_masks=2, time_width=5, time_percent=50, freq_masks=2, freq_width=3, freq_bins=4, base_dim=8,
              left_context=1, right_context=1, subsample=3, fill=0.0)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(cfg=None, T=T, B=B, D=D, ldx=D, ldo=D, xp=x.data_ptr(), sp=seq.data_ptr(), op=out.data_ptr(), null_cfg=False):
        c = _lib.SpecAugmentConfig(**dict(ok, **(cfg or {})))
        return lib.lc_spec_augment(xp, T, B, D, ldx, sp, None if null_cfg else ctypes.byref(c), 1, op, ldo, plan.data_ptr(),
                                   stream)

    bad_shapes = (dict(T=0), dict(B=0), dict(D=0), dict(T=-1), dict(B=-2), dict(D=-24), dict(xp=None), dict(sp=None),
                  dict(op=None), dict(null_cfg=True), dict(ldx=D - 1), dict(ldo=D - 1), dict(D=16, ldx=16, ldo=16),
                  dict(D=32, ldx=32, ldo=32))
    bad_cfgs = (dict(time_masks=9), dict(time_masks=-1), dict(freq_masks=9), dict(freq_masks=-1), dict(time_width=-1),
                dict(freq_width=-1), dict(time_percent=101), dict(time_percent=-1), dict(freq_bins=0), dict(freq_bins=-4),
                dict(freq_bins=3), dict(freq_width=5), dict(left_context=-1, right_context=3),
                dict(right_context=-1, left_context=3), dict(subsample=-1), dict(fill=float("nan")), dict(fill=float("inf")),
                dict(fill=float("-inf")), dict(base_dim=12), dict(left_context=2))
    for kw in bad_shapes:
        assert call(**kw) == -1, kw
        assert b"lc_spec_augment" in lib.lc_last_error()
    for cfg in bad_cfgs:
        assert call(cfg=cfg) == -1, cfg
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and (plan == -7).all()
    # and the same buffers are fine for a good call: subsample 0 (none) and freq_width == freq_bins are legal
    assert call(cfg=dict(subsample=0, freq_width=4)) == 0
    torch.cuda.synchronize()
    assert not torch.isnan(out).any() and (plan != -7).all()


# ----------------------------------------------------------------------------------------------- the graph option
SMOKE = dict(nnet_type="blstm", input_dim=8, left_context=0, right_context=0, num_layers=2, num_neurons=32,
             num_projects=16, num_targets=11, use_peepholes=True, dropout_rate=1.0)          # __graft_entry__.smoke's
LAYOUTS = {"smoke": {}, "spliced": dict(left_context=1, right_context=1, subsample=3)}
GRAPH_SPEC = _spec((2, 8), (2, 3), 4, cap=50)


def _batch(cfg):
    rng = np.random.default_rng(0)
    B, T = 4, 20
    D = cfg["input_dim"] * (1 + cfg["left_context"] + cfg["right_context"])
    seq = np.array([20, 17, 12, 9], np.int32)
    x = rng.normal(size=(B, T, D)).astype(np.float32)
    labels = np.full((B, 6), -1, np.int64)
    for b, n in enumerate((6, 5, 4, 3)):
        x[b, seq[b]:] = 0
        labels[b, :n] = rng.integers(0, 10, size=n)
    return {"nnet_input": x, "sequence_length": seq, "nnet_target": labels}


def _next_seed(graph):
    return (graph.drop_seed * 1664525 + 1013904223) & 0x7FFFFFFF


def _masked_input(graph, batch, cfg, seed):
    """(x [T,B,D], the same under the masks the step seeded ``seed`` draws) on the host."""
    x = np.ascontiguousarray(batch["nnet_input"].transpose(1, 0, 2))
    lay = augment.layout_of(cfg)
    plan = mask_plan(seed, batch["sequence_length"], GRAPH_SPEC, lay.subsample)
    xa = apply_host(x, batch["sequence_length"], plan, GRAPH_SPEC, *lay)
    assert (xa != x).any()
    return x, xa, plan


def _forward(graph, x_tbd, seq, seed):
    from lstm_ctc_amd import ops
    ops.lstm_status(graph.model.device).zero_()
    logits = graph.model.forward(torch.from_numpy(x_tbd).cuda(), torch.from_numpy(seq).cuda(), drop_seed=seed, seq_len_host=seq)
    return logits.permute(1, 0, 2).cpu().numpy()


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_training_step_reads_the_masked_input(layout):
    from lstm_ctc_amd.nnet.graph import create_graph_for_training_ctc
    cfg = dict(SMOKE, **LAYOUTS[layout])
    batch = _batch(cfg)
    seq = batch["sequence_length"]
    graph = create_graph_for_training_ctc(None, cfg, learn_rate=1e-2, seed=3, spec_augment=GRAPH_SPEC)
    seed = _next_seed(graph)
    x, xa, plan = _masked_input(graph, batch, cfg, seed)
    want, plain = _forward(graph, xa, seq, seed), _forward(graph, x, seq, seed)
    assert not np.array_equal(want, plain)
    out = graph.step(batch, fetch_logits=True)
    assert graph.drop_seed == seed and np.array_equal(out["logits"], want)
    assert graph.specaug_steps == 1
    shares = augment.masked_shares(plan, seq, GRAPH_SPEC, cfg.get("subsample"))
    assert (graph.specaug_frames_masked, graph.specaug_frames, graph.specaug_bins_masked, graph.specaug_bins) == shares
    assert shares[0] > 0 and shares[1] == int(seq.sum()) * max(cfg.get("subsample") or 0, 1)
    # a train=False step of the same graph reads the input as it is, and counts nowhere
    seed = _next_seed(graph)
    plain = _forward(graph, x, seq, seed)
    out = graph.step(batch, fetch_logits=True, train=False)
    assert np.array_equal(out["logits"], plain) and graph.specaug_steps == 1 and graph.specaug_frames == shares[1]


def test_step_device_leaves_the_callers_tensor_alone():
    from lstm_ctc_amd.nnet.graph import create_graph_for_training_ctc
    cfg = dict(SMOKE, **LAYOUTS["spliced"])
    batch = _batch(cfg)
    graph = create_graph_for_training_ctc(None, cfg, learn_rate=1e-2, seed=3, spec_augment=GRAPH_SPEC)
    x, seq_d, seq, flat_d, offs_d, flat, offs, maxlen = graph._upload(batch)
    keep = x.clone()
    losses = []
    for step in range(3):                                              # the same tensor step after step, as bench.py does
        seed = _next_seed(graph)
        want = _forward(graph, _masked_input(graph, batch, cfg, seed)[1], seq, seed)
        out = graph.step_device(x, seq_d, flat_d, offs_d, maxlen, int(len(flat)), fetch_logits=True)
        assert np.array_equal(out["logits"], want), step
        assert torch.equal(x, keep)
        losses.append(out["eval_loss"])
    assert len(set(losses)) == 3                                       # new masks (and parameters) every step
    assert graph.specaug_steps == 3 and graph.specaug_frames == 0      # no seq_host: the shares count nowhere


def test_validation_graph_ignores_the_option():
    from lstm_ctc_amd.nnet.graph import CTCGraph, create_graph_for_validation_ctc
    cfg = dict(SMOKE, **LAYOUTS["spliced"])
    batch = _batch(cfg)
    seq = batch["sequence_length"]
    with pytest.raises(TypeError):
        create_graph_for_validation_ctc(None, cfg, seed=3, spec_augment=GRAPH_SPEC)
    graph = CTCGraph(None, cfg, seed=3, spec_augment=GRAPH_SPEC)      # no learn_rate: a validation graph
    x = np.ascontiguousarray(batch["nnet_input"].transpose(1, 0, 2))
    plain = _forward(graph, x, seq, _next_seed(graph))
    out = graph.step(batch, fetch_logits=True)
    assert np.array_equal(out["logits"], plain) and graph.specaug_steps == 0
    ref = create_graph_for_validation_ctc(None, cfg, seed=3).step(batch, fetch_logits=True)
    assert np.array_equal(out["logits"], ref["logits"]) and out["eval_loss"] == ref["eval_loss"]


def test_same_seed_agrees_and_ranks_differ(monkeypatch):
    from lstm_ctc_amd.nnet import dp
    from lstm_ctc_amd.nnet.graph import create_graph_for_training_ctc
    cfg = dict(SMOKE, **LAYOUTS["spliced"])
    batch = _batch(cfg)
    make = lambda: create_graph_for_training_ctc(None, cfg, learn_rate=1e-2, seed=3, spec_augment=GRAPH_SPEC)
    a, b = make(), make()
    for step in range(2):
        oa, ob = a.step(batch, fetch_logits=True), b.step(batch, fetch_logits=True)
        assert np.array_equal(oa["logits"], ob["logits"]) and oa["eval_loss"] == ob["eval_loss"]
    # two ranks of one job: the same parameters, other masks (the group is only asked for its size and this rank)
    ranks = []
    for rank in (0, 1):
        monkeypatch.setattr(dp, "world_size", lambda pg: 2)
        monkeypatch.setattr(dp, "rank", lambda pg, rank=rank: rank)
        graph = make()
        monkeypatch.undo()
        graph.world = 1                                                # step alone: nothing to reduce with
        ranks.append(graph)
    assert ranks[0].drop_seed != ranks[1].drop_seed
    p0, p1 = ranks[0].model.ps.export_tf(), ranks[1].model.ps.export_tf()
    assert all(np.array_equal(p0[k], p1[k]) for k in p0)              # the replicas start identical
    plans = [mask_plan(_next_seed(g), batch["sequence_length"], GRAPH_SPEC, 3) for g in ranks]
    assert not np.array_equal(plans[0], plans[1])
    for g, plan in zip(ranks, plans):
        seed = _next_seed(g)
        x = np.ascontiguousarray(batch["nnet_input"].transpose(1, 0, 2))
        want = _forward(g, apply_host(x, batch["sequence_length"], plan, GRAPH_SPEC, 8, 1, 1, 3), batch["sequence_length"], seed)
        assert np.array_equal(g.step(batch, fetch_logits=True)["logits"], want)


def test_launch_train_retry_repeats_the_draw(monkeypatch):
    """A step whose first try reports a failed recurrence is re-run under ``ops.force_launch_train`` with the counters put
    back: it must draw the masks again, not the next ones.  The failure is staged - the status word is set behind a forward
    that ran fine - so the optimizer skips the first try's update exactly as it does after a real one."""
    from lstm_ctc_amd import ops
    from lstm_ctc_amd.nnet.graph import create_graph_for_training_ctc
    cfg = dict(SMOKE, **LAYOUTS["spliced"])
    batch = _batch(cfg)
    make = lambda: create_graph_for_training_ctc(None, cfg, learn_rate=1e-2, seed=3, spec_augment=GRAPH_SPEC)
    straight, retried = make(), make()
    with ops.force_launch_train():                                     # the schedule the retry will run on
        want = straight.step(batch, fetch_logits=True)
    forward, calls = retried.model.forward, []

    def failing_once(*args, **kw):
        logits = forward(*args, **kw)
        calls.append(kw.get("drop_seed"))
        if len(calls) == 1:
            ops.lstm_status(retried.model.device).fill_(5)
        return logits

    monkeypatch.setattr(retried.model, "forward", failing_once)
    got = retried.step(batch, fetch_logits=True)
    monkeypatch.undo()
    assert retried.persist_fallbacks == 1 and len(calls) == 2 and calls[0] == calls[1] == straight.drop_seed
    assert retried.drop_seed == straight.drop_seed and retried.global_step == straight.global_step == 1
    assert retried.specaug_steps == 1 and retried.specaug_frames == straight.specaug_frames
    assert np.array_equal(got["logits"], want["logits"]) and got["eval_loss"] == want["eval_loss"]
    pa, pb = straight.model.ps.export_tf(), retried.model.ps.export_tf()
    for k in pa:                                                       # one update, the same one
        assert np.array_equal(pa[k], pb[k]), k


# ----------------------------------------------------------------------------------------------- the command line
def _run(cli, *args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", cli)] + list(args), capture_output=True, timeout=300)
    return r.returncode, r.stderr.decode()


def _logged(err, name):
    lines = [l for l in err.split("\n") if l.startswith("INFO:tensorflow:%s = " % name)]
    assert len(lines) == 1, err
    return float(lines[0].split()[-1])


def test_cli_trains_with_spec_augment_and_reports(tmp_path):
    import lstm_ctc_amd.nnet as nnet
    rng = np.random.default_rng(7)
    D, V = 6, 9
    lines = []
    for i, T in enumerate([20, 24, 31, 40]):
        path = str(tmp_path / ("utt%03d.tfrecords" % i))
        nnet.write_tfrecord(path, rng.normal(size=(T, D)).astype(np.float32), rng.integers(0, V - 1, size=int(rng.integers(1, 5))))
        lines.append("utt%03d %d %d 1 %s" % (i, T, D, path))
    scp = tmp_path / "tfrecords.scp"
    scp.write_text("\n".join(lines) + "\n")
    config = tmp_path / "nnet.config"
    config.write_text("nnet_type = lstm\ninput_dim = 6\nleft_context = 1\nright_context = 1\nsubsample = 2\nnum_layers = 2\n"
                      "num_neurons = 32\nnum_projects = 16\nnum_targets = 9\nuse_peepholes = true\ndropout_rate = 1.0\n")
    d = str(tmp_path)
    rc, err = _run("nnet-init.py", "--objective=ctc", "--batch-size", "2", str(scp), str(config), d + "/nnet.0")
    assert rc == 0, err
    train = ["--objective=ctc", "--batch-size", "2", "--learn-rate=0.01", "--optimizer=adam", "--seed=1", "--shuffle=false"]
    tail = [str(scp), str(config), d + "/nnet.0"]
    rc, err = _run("nnet-train.py", *train, "--spec-augment", "time=2x10,freq=1x2,bins=3,cap=50", *tail, d + "/nnet.1")
    assert rc == 0, err
    report = [l for l in err.split("\n") if l.startswith("INFO:tensorflow:spec augment ")]
    assert len(report) == 1, err
    m = re.fullmatch(r"INFO:tensorflow:spec augment time=2x10,freq=1x2,bins=3,cap=50,fill=0\.0: (\d+) step\(s\) augmented; (\S+)% of "
                     r"(\d+) live raw frame\(s\) under a time mask, (\S+)% of the bins under a frequency mask", report[0])
    assert m, report[0]
    # four utterances in two batches; 10, 12, 15 and 20 rows of two raw frames each
    assert int(m.group(1)) == 2 and int(m.group(3)) == 2 * (10 + 12 + 15 + 20)
    assert 0.0 < float(m.group(2)) <= 2 * 10 * 4 * 100.0 / 114 and 0.0 <= float(m.group(4)) <= 100.0 * 2 / 3
    augmented = _logged(err, "tr_loss")
    assert np.isfinite(augmented) and os.path.getsize(d + "/nnet.1") > 0
    rc, err = _run("nnet-train.py", *train, *tail, d + "/nnet.2")                 # the same run without the flag
    assert rc == 0, err
    assert "spec augment" not in err and _logged(err, "tr_loss") != augmented
