"""Which stream the work runs on, and what orders it against other streams - the axis the arithmetic tests are blind on: on
the default stream a launch or memset on the wrong stream is serialised anyway and gives the right answer.

Part A, ``test_entry_runs_on_the_callers_stream``: every row of tests/stream_cases.py (every C entry point with an
``lc_stream_t``, at the smallest shape that takes its multi-launch path) runs once on the default stream - the reference; its
arithmetic is pinned elsewhere - and once on ONE side stream that 3 ms of lc_debug_spin hold: until the spin ends every float
input, in/out tensor and ``out=`` tensor holds NaN; behind the spin the side stream copies the float inputs in, fills the
``out=`` tensors with a sentinel and 0xFF into the side stream's cached workspaces (the recurrences' excepted: its control
block belongs to the caller), and then the op is called.  A launch or memset on any other stream runs during the spin: it
reads NaN, and what it writes is overwritten.  Integer inputs hold their final values from the start, so nothing here can
turn a stream bug into an out-of-bounds access.  Every returned tensor, in/out tensor and whole ``out=`` buffer (windows
included: what lies outside a window must still hold the sentinel) must equal the default-stream result bit for bit.
``test_harness_reports_a_misplaced_call`` misplaces two cheap rows itself and must see a mismatch.

Part B, ``test_overlapped_backward_under_forced_skew``: ``Model.backward`` with ``overlap_wgrad`` runs layer i's weight-gradient
products on ``model._side`` under the BPTT of layer i - 1.  Per configuration the same ``dlogits`` go through backward three
ways, every gradient compared bit for bit: serial (``overlap_wgrad`` off), side late (a spin of ten serial backwards, 0.1 .. 2 s,
queued on ``_side`` in front of backward: all side work starts after main has run to its final ``wait_stream`` - main
rewriting, freeing or re-allocating what the side stream has yet to read would show) and main late (5 ms of spin on main
behind every ``_side.wait_event``: the side stream runs ahead after every fork - reading what main produces after the fork
would show).  ``fuse_dx`` is off in all three so that all three issue the same products.  FALLBACK names the
configurations whose serial run differs for a reason that is not ordering; there the skewed runs are compared bit for bit
with the unskewed overlapped run, and all of them with the serial run within conftest.GRAD_TOL.
``test_staged_upload_under_a_held_main_stream``: ``graph.stage`` beside a held main stream.

The last test prints, per part B configuration, the serial backward's wall time and the spin chosen from it, and writes
them to LC_MEASURED_DIR/stream_discipline_measured.txt when that is set."""
import os
import time

import numpy as np
import pytest
import torch

import stream_cases
from conftest import GRAD_TOL
from test_gpu_ops import ops  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
SENTINEL = -7.25
MEASURED = {}                 # part B: case id -> (serial backward seconds, spin microseconds, comparison)
_SIDE = []


def side_stream():
    """ONE side stream for the whole module (a process has 4 hardware queues, and the recurrences use a stream of their own)."""
    if not _SIDE:
        _SIDE.append(torch.cuda.Stream())
    return _SIDE[0]


# ----------------------------------------------------------------------------------------------- part A: the harness
def _bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


def _tensors(ret):
    if ret is None:
        return []
    if torch.is_tensor(ret):
        return [ret]
    return [r for r in ret if torch.is_tensor(r)]


def _results(case, t, ret):
    """[(label, tensor)] of everything a call leaves: what it returned, its in/out tensors and its whole out= buffers."""
    ret = _tensors(case.post(ret) if case.post is not None else ret)
    return ([("returned[%d]" % i, r) for i, r in enumerate(ret)] + [("in/out " + k, t[k]) for k in case.io] +
            [("out= " + k, t[k]) for k in sorted(case.out)])


def _fill_value(dtype, value):
    return value if dtype.is_floating_point else int(value) if value == value else -1


def reference_run(ops, case):
    """The row on the default stream -> (the float inputs as the call met them, the integer inputs, its results)."""
    t = {k: torch.as_tensor(v).cuda() for k, v in case.inp.items()}
    ints = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in case.ints.items()}
    if case.prep is not None:
        t.update(case.prep(ops, t))
    floats = {k: v.clone() for k, v in t.items()}
    t.update(ints)
    for k, (shape, dtype) in case.out.items():
        t[k] = torch.full(shape, _fill_value(dtype, SENTINEL), dtype=dtype, device="cuda")
    ret = case.call(ops, t)
    torch.cuda.synchronize()
    return floats, ints, [(label, v.clone()) for label, v in _results(case, t, ret)]


def _poison_workspaces(ops, stream):
    for (name, _, handle), buf in list(ops._workspaces.items()):
        if handle == stream.cuda_stream and name != "lstm":
            buf.fill_(0xFF)


def held_run(ops, case, floats, ints, misplace=False):
    """The row on the held side stream (module docstring) -> its results.  ``misplace``: the call itself is wrapped in the
    default stream - what a launch that ignored its ``stream`` argument would look like."""
    side = side_stream()
    nan = float("nan")
    with torch.cuda.stream(side):
        t = {k: torch.full_like(v, nan) for k, v in floats.items()}
        t.update({k: v.clone() for k, v in ints.items()})
        for k, (shape, dtype) in case.out.items():
            t[k] = torch.full(shape, _fill_value(dtype, nan), dtype=dtype, device="cuda")
        torch.cuda.synchronize()
        ops.debug_spin(1, 3000, 0)
        for k, v in floats.items():
            t[k].copy_(v, non_blocking=True)
        for k, (shape, dtype) in case.out.items():
            t[k].fill_(_fill_value(dtype, SENTINEL))
        _poison_workspaces(ops, side)
        if misplace:
            with torch.cuda.stream(torch.cuda.default_stream()):
                ret = case.call(ops, t)
        else:
            ret = case.call(ops, t)
    side.synchronize()
    torch.cuda.synchronize()
    return _results(case, t, ret)


def mismatches(want, got):
    bad = [] if len(want) == len(got) else ["%d results against %d" % (len(got), len(want))]
    for (label, w), (_, g) in zip(want, got):
        if w.shape != g.shape or w.dtype != g.dtype:
            bad.append("%s: %s %s against %s %s" % (label, tuple(g.shape), g.dtype, tuple(w.shape), w.dtype))
        elif not torch.equal(_bits(w), _bits(g)):
            n = int((_bits(w) != _bits(g)).sum())
            bad.append("%s: %d of %d bytes differ" % (label, n, _bits(w).numel()))
    return bad


def _row(name):
    return next(r for r in stream_cases.ROWS if r.name == name)


def _seed(name):
    return sum(ord(c) * (i + 1) for i, c in enumerate(name))


@pytest.mark.parametrize("row", stream_cases.ROWS, ids=lambda r: r.name)
def test_entry_runs_on_the_callers_stream(ops, row, monkeypatch):
    for k, v in row.env.items():
        monkeypatch.setenv(k, v)
    case = row.make(np.random.default_rng(_seed(row.name)))
    floats, ints, want = reference_run(ops, case)
    assert want, "the row compares nothing"
    for label, w in want:
        if w.dtype.is_floating_point and label.startswith(("returned", "in/out")):
            assert not torch.isnan(w.float()).any(), (row.name, label, "NaN in the default-stream result")
    # the same call gives the same bits (every entry here sums in a fixed order): what makes the comparison meaningful
    _, _, again = reference_run(ops, case)
    assert not mismatches(want, again), (row.name, "not reproducible on the default stream", mismatches(want, again))
    got = held_run(ops, case, floats, ints)
    bad = mismatches(want, got)
    assert not bad, (row.name, row.entries, bad)


@pytest.mark.parametrize("name", ["transpose", "colsum_plain"])
def test_harness_reports_a_misplaced_call(ops, name):
    """The harness against a call the test misplaces itself: it runs on the default stream during the spin, reads the NaN the
    inputs still hold, and the harness must say so (a harness that compared nothing would pass every row)."""
    row = _row(name)
    case = row.make(np.random.default_rng(_seed(name)))
    floats, ints, want = reference_run(ops, case)
    assert not mismatches(want, held_run(ops, case, floats, ints))
    assert mismatches(want, held_run(ops, case, floats, ints, misplace=True)), name


# ----------------------------------------------------------------------------------------------- part B: the overlapped backward
T_, B_, D_, V_ = 12, 5, 10, 9
LENGTHS = np.array([12, 7, 0, 9, 3], np.int32)


def _cfg(nnet_type="blstm", **kw):
    """tests/test_gpu_model.py's dict (tests/test_gpu_row_conv.py's for the unidirectional models), three layers."""
    cfg = dict(nnet_type=nnet_type, input_dim=D_, left_context=0, right_context=0, num_layers=3, num_neurons=32,
               num_projects=16, num_targets=V_, use_peepholes=True, dropout_rate=1.0)
    if nnet_type != "blstm":
        del cfg["num_projects"], cfg["use_peepholes"]
    cfg.update(kw)
    return cfg


# id -> (config, environment, model.X3_FORCE, lengths)
CONFIGS = {
    "blstm": (_cfg(), {}, False, LENGTHS),
    "blstm_dropout_residual": (_cfg(dropout_rate=0.8, input_dim=32), {}, False, LENGTHS),
    "moe": (_cfg(num_experts=3, moe_temp=3.0), {}, False, LENGTHS),
    "layer_norm_dropout": (_cfg(layer_norm=True, dropout_rate=0.8), {}, False, LENGTHS),
    "time_reduce": (_cfg(time_reduce_layers=1), {}, False, LENGTHS),
    "lc_blstm": (_cfg(chunk_frames=4, lookahead_frames=2), {}, False, LENGTHS),
    "conv": (_cfg(conv_layers=2, conv_channels=8, conv_bins=5), {}, False, LENGTHS),
    "pack_frames": (_cfg(pack_frames=True), {}, False, np.sort(LENGTHS)),
    "lstm_row_conv": (_cfg("lstm", row_conv_frames=2), {}, False, LENGTHS),
    "lstm_bn": (_cfg("lstm", use_bn=True), {}, False, LENGTHS),
    "bf16x3": (_cfg(compute_dtype="bf16x3"), {}, False, LENGTHS),
    "bf16x3_dropout": (_cfg(compute_dtype="bf16x3", dropout_rate=0.8), {}, False, LENGTHS),
    "bf16x3_side_f32": (_cfg(compute_dtype="bf16x3"), {"LC_X3_SIDE_WGRAD": "f32"}, False, LENGTHS),
    "bf16x3_dropout_side_f32": (_cfg(compute_dtype="bf16x3", dropout_rate=0.8), {"LC_X3_SIDE_WGRAD": "f32"}, False, LENGTHS),
    # at N = 32 no product is large enough for the split-operand kernels by the model's own rule: the same four with every
    # eligible product forced onto them, so that both streams really fill and read the x3 shadow cache
    "bf16x3_forced": (_cfg(compute_dtype="bf16x3"), {}, True, LENGTHS),
    "bf16x3_forced_dropout": (_cfg(compute_dtype="bf16x3", dropout_rate=0.8), {}, True, LENGTHS),
    "bf16x3_forced_side_f32": (_cfg(compute_dtype="bf16x3"), {"LC_X3_SIDE_WGRAD": "f32"}, True, LENGTHS),
    "bf16x3_forced_dropout_side_f32": (_cfg(compute_dtype="bf16x3", dropout_rate=0.8), {"LC_X3_SIDE_WGRAD": "f32"}, True,
                                       LENGTHS),
}
# Configurations whose serial run differs from the overlapped one for a reason that is not ordering.
FALLBACK = {
    "bf16x3_forced_side_f32":
        "LC_X3_SIDE_WGRAD=f32 moves the weight gradients of layers > 0 to the fp32 kernels only where they are overlapped",
    "bf16x3_forced_dropout_side_f32":
        "LC_X3_SIDE_WGRAD=f32 moves the weight gradients of layers > 0 to the fp32 kernels only where they are overlapped",
}


def _inputs(cfg, lengths):
    rng = np.random.default_rng(5)
    x = rng.normal(size=(T_, B_, cfg["input_dim"])).astype(np.float32)
    for b, n in enumerate(lengths):
        x[n:, b] = 0
    return torch.from_numpy(x).cuda(), torch.from_numpy(np.ascontiguousarray(lengths)).cuda(), rng


def _backward(model, x, seq, dl, before=None):
    """forward + backward (left enqueued) -> the logits; ``before(model)`` runs between the two, behind a synchronisation."""
    logits = model.forward(x, seq, drop_seed=7).clone()
    torch.cuda.synchronize()
    if before is not None:
        before(model)
    model.backward(dl)
    model.returned_at = time.perf_counter()             # the host's clock when backward came back, nothing awaited yet
    return logits


@pytest.mark.parametrize("persistent", ["default", "0"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_overlapped_backward_under_forced_skew(ops, name, persistent, monkeypatch):
    from lstm_ctc_amd.nnet import model as model_mod
    cfg, env, force, lengths = CONFIGS[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if persistent == "0":
        monkeypatch.setenv("LC_LSTM_PERSISTENT", "0")
    monkeypatch.setattr(model_mod, "X3_FORCE", force)
    model = model_mod.Model(cfg, "cuda", seed=3)
    assert model.overlap_wgrad, name
    assert model.x3_side_f32 == (env.get("LC_X3_SIDE_WGRAD") == "f32")
    model.fuse_dx = False
    model._side = side_stream()
    x, seq, rng = _inputs(cfg, lengths)
    main = torch.cuda.current_stream()

    model.overlap_wgrad = False                                       # serial: the reference (first run: warm-up)
    logits = model.forward(x, seq, drop_seed=7).clone()
    dl = torch.from_numpy(rng.normal(size=tuple(logits.shape)).astype(np.float32)).cuda()
    model.backward(dl)
    torch.cuda.synchronize()
    model.forward(x, seq, drop_seed=7)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.backward(dl)
    torch.cuda.synchronize()
    serial_s = time.perf_counter() - t0
    serial = model.ps.grad.clone()
    assert torch.isfinite(serial).all() and float(serial.abs().max()) > 0
    spin_us = int(min(max(10 * serial_s * 1e6, 100e3), 2e6))

    model.overlap_wgrad = True
    plain = None
    if name in FALLBACK:                                              # the unskewed overlapped run
        assert torch.equal(_bits(_backward(model, x, seq, dl)), _bits(logits))
        torch.cuda.synchronize()
        plain = model.ps.grad.clone()

    held = {}

    def hold_side(m):                                                 # side late
        with torch.cuda.stream(m._side):
            ops.debug_spin(1, spin_us, 0)
        held["t0"] = time.perf_counter()
    again = _backward(model, x, seq, dl, before=hold_side)
    enqueued_s = model.returned_at - held["t0"]
    torch.cuda.synchronize()
    assert torch.equal(_bits(again), _bits(logits))
    side_late = model.ps.grad.clone()
    assert model._side is side_stream()
    # the host was back before the spin was half over: the side stream really ran everything behind main
    assert enqueued_s < spin_us * 1e-6 / 2, (name, enqueued_s, spin_us)

    forks = []
    original = torch.cuda.Stream.wait_event

    def wait_event_then_hold_main(self, event):                       # main late
        original(self, event)
        if self is model._side:
            forks.append(1)
            ops.debug_spin(1, 5000, 0)
    with monkeypatch.context() as m:
        m.setattr(torch.cuda.Stream, "wait_event", wait_event_then_hold_main)
        assert torch.cuda.current_stream() == main
        assert torch.equal(_bits(_backward(model, x, seq, dl)), _bits(logits))
    torch.cuda.synchronize()
    main_late = model.ps.grad.clone()
    assert len(forks) == cfg["num_layers"] - 1, forks

    MEASURED[(name, persistent)] = (serial_s, spin_us, "fallback" if name in FALLBACK else "serial")
    if name in FALLBACK:
        assert torch.equal(_bits(side_late), _bits(plain)), (name, "side late differs from the unskewed overlapped run")
        assert torch.equal(_bits(main_late), _bits(plain)), (name, "main late differs from the unskewed overlapped run")
        den = max(float(serial.abs().max()), 1e-3)
        for tag, g in (("overlapped", plain), ("side late", side_late), ("main late", main_late)):
            assert float((g - serial).abs().max()) < GRAD_TOL * den, (name, tag)
    else:
        for tag, g in (("side late", side_late), ("main late", main_late)):
            assert torch.equal(_bits(g), _bits(serial)), (
                name, tag, "%d of %d gradient elements differ" % (int((g.view(torch.int32) != serial.view(torch.int32)).sum()),
                                                                  g.numel()), float((g - serial).abs().max()))


# ----------------------------------------------------------------------------------------------- the staged upload
def _batches():
    rng = np.random.default_rng(9)
    out = []
    for k in range(2):
        seq = np.array([12, 7, 9, 3, 10], np.int32)[::1 if k == 0 else -1].copy()
        x = rng.normal(size=(B_, T_, D_)).astype(np.float32)
        y = np.full((B_, 3), -1, np.int64)
        for b in range(B_):
            x[b, seq[b]:] = 0
            n = int(min(3, seq[b] // 3))
            y[b, :n] = rng.integers(0, V_ - 1, size=n)
        out.append({"nnet_input": x, "sequence_length": seq, "nnet_target": y})
    return out


def _same(a, b):
    assert set(a) == set(b), (sorted(a), sorted(b))
    for k in a:
        if k == "decoded":                                  # (tokens [B,T], their number [B]): a row's tail is unspecified
            (ta, na), (tb, nb) = a[k], b[k]
            assert np.array_equal(na, nb), k
            assert all(np.array_equal(ta[i, :n], tb[i, :n]) for i, n in enumerate(na)), k
        else:
            assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


def test_staged_upload_under_a_held_main_stream(ops):
    """Two train steps, the second batch staged on the copy stream while 20 ms of spin hold the main stream: losses, tokens
    and parameters equal, bit for bit, those of a graph of the same seed that ran both steps unstaged - in the order a
    caller that has just run step k stages k + 1, and in the order ``stage``'s own documentation names (k + 1 staged before
    step k is enqueued, so that the copy runs beside the held step)."""
    from lstm_ctc_amd.nnet.graph import create_graph_for_training_ctc
    cfg = _cfg(num_layers=2, dropout_rate=0.8)
    b0, b1 = _batches()

    def graph():
        return create_graph_for_training_ctc(None, cfg, learn_rate=1e-2, optimizer="adam", seed=3)
    g = graph()
    want = [g.step(b0), g.step(b1)]
    torch.cuda.synchronize()
    params = g.model.ps.flat.clone()
    assert np.isfinite(want[1]["eval_loss"])

    g = graph()
    ops.debug_spin(1, 20000, 0)
    first = g.step(b0)
    staged = g.stage(b1)
    got = [first, g.step(None, staged=staged)]
    torch.cuda.synchronize()
    for a, b in zip(want, got):
        _same(a, b)
    assert torch.equal(_bits(g.model.ps.flat), _bits(params))

    g = graph()
    ops.debug_spin(1, 20000, 0)
    staged = g.stage(b1)
    got = [g.step(b0), g.step(None, staged=staged)]
    torch.cuda.synchronize()
    for a, b in zip(want, got):
        _same(a, b)
    assert torch.equal(_bits(g.model.ps.flat), _bits(params))


# ----------------------------------------------------------------------------------------------- report
def test_zz_report_measured():
    lines = ["# tests/test_gpu_stream_discipline.py, part B: per configuration and LC_LSTM_PERSISTENT, the wall time of one",
             "# synchronised serial backward, the spin queued on the side stream (10 x, 0.1 .. 2 s), and what the skewed runs were",
             "# compared with bit for bit (serial, or - fallback - the unskewed overlapped run, all within GRAD_TOL of serial)"]
    lines += ["%-32s persistent=%-7s serial %7.2f ms  spin %7.1f ms  %s" % (k[0], k[1], v[0] * 1e3, v[1] / 1e3, v[2])
              for k, v in sorted(MEASURED.items())]
    lines += ["# fallback %s: %s" % kv for kv in sorted(FALLBACK.items())]
    print("\n" + "\n".join(lines))
    out = os.environ.get("LC_MEASURED_DIR")              # where to keep the table; unset: printed only
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "stream_discipline_measured.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
    assert MEASURED
