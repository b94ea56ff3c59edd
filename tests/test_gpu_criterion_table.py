"""The wiring of the CTC criterion's option table (nnet.graph.CRITERION_OPTIONS) to the ops, on the GPU: three training steps
of ``CTCGraph.step_device`` under each form of the criterion - plain, windowed, delay-penalised, maximum-entropy,
transcript-tolerant - and after every step ``eval_loss`` and the option's own output must be, bit for bit, what the
``ops.ctc_loss*`` wrapper gives on the step's own logits, reduced as the graph documents: ``eval_loss`` the float32 sum of the
criterion per utterance (``loss - eta * H`` under entropy_weight), the option's output the float64 sum of its [B] vector over
the utterances with a finite, non-skipped loss, its count their labels (delay) or frames (entropy, star).  No stored
number: the kernels are checked against their references elsewhere (test_gpu_ctc_window / _delay / _entropy / _star)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CFG = dict(nnet_type="blstm", input_dim=8, left_context=0, right_context=0, num_layers=1, num_neurons=32, num_projects=16,
           num_targets=12, use_peepholes=True, dropout_rate=1.0)
T, B, V = 24, 3, 12
INF = float("inf")
SETTINGS = {"plain": {}, "window": {"align_window": 2}, "delay": {"delay_penalty": 0.05}, "entropy": {"entropy_weight": 0.2},
            "star": {"star_penalty": (2, INF)}}
# setting -> (the ops wrapper, its output key, the count's key, what is counted, the graph's two totals)
WIRING = {"delay": ("ctc_loss_delay", "entry_sum", "entry_labels", "labels", ("entry_sum_total", "entry_labels_total")),
          "entropy": ("ctc_loss_entropy", "path_entropy", "path_entropy_frames", "frames",
                      ("path_entropy_total", "path_entropy_frames_total")),
          "star": ("ctc_loss_star", "star_frames", "star_frame_count", "frames", ("star_frames_total", "star_frame_count_total"))}
ALL_TOTALS = [t for w in WIRING.values() for t in w[4]]


def batch():
    """Label lengths 0, 2 and 5; an alignment that spells them (label i on frames 3 i + 1, 3 i + 2, blanks between)."""
    rng = np.random.RandomState(20)
    x = rng.normal(size=(T, B, CFG["input_dim"])).astype(np.float32)
    seq = np.array([24, 20, 17], np.int32)
    labels = [np.zeros(0, np.int32), np.array([3, 3], np.int32), np.array([0, 7, 7, 10, 1], np.int32)]
    flat = np.concatenate(labels).astype(np.int32)
    offs = np.concatenate([[0], np.cumsum([len(l) for l in labels])]).astype(np.int32)
    frame_target = np.full((B, T), V - 1, np.int32)
    for b, l in enumerate(labels):
        for i, sym in enumerate(l):
            frame_target[b, 3 * i + 1:3 * i + 3] = sym
        frame_target[b, seq[b]:] = -1
    return x, seq, flat, offs, frame_target


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_three_steps_are_the_ops_on_the_steps_logits_bit_for_bit(setting):
    from lstm_ctc_amd import ops
    from lstm_ctc_amd.nnet.graph import CTCGraph
    x, seq, flat, offs, frame_target = batch()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    x_d, seq_d, flat_d, offs_d = dev(x), dev(seq), dev(flat), dev(offs)
    maxlen = int(np.diff(offs).max())
    windows = None
    if setting == "window":
        lo, hi, constrained = ops.label_windows(frame_target, flat, offs, seq, 2, V - 1)
        assert constrained.all() and (hi - lo == 5).all()
        windows = (dev(lo), dev(hi))
    graph = CTCGraph(None, CFG, learn_rate=1e-2, optimizer="sgd", seed=5, **SETTINGS[setting])
    for keyword in ("delay_penalty", "entropy_weight", "star_penalty"):
        assert getattr(graph, keyword) == SETTINGS[setting].get(keyword)
    sums = {t: 0 for t in ALL_TOTALS}
    for step in range(3):
        out = graph.step_device(x_d, seq_d, flat_d, offs_d, maxlen, len(flat), fetch_logits=True, windows=windows)
        logits = dev(out["logits"].transpose(1, 0, 2))                       # [T,B,V]: the step's own, bit for bit
        head = (logits, flat_d, offs_d, seq_d, maxlen)
        if setting == "plain":
            loss, extra = ops.ctc_loss(*head, want_grad=False)[0], None
        elif setting == "window":
            loss, extra = ops.ctc_loss_windowed(*head, *windows, want_grad=False)[0], None
        else:
            value = getattr(graph, next(iter(SETTINGS[setting])))
            loss, extra, _ = getattr(ops, WIRING[setting][0])(*head, *(value if isinstance(value, tuple) else (value,)),
                                                              want_grad=False)
        assert bool(torch.isfinite(loss).all())
        criterion = loss - 0.2 * extra if setting == "entropy" else loss
        eval_loss = criterion.sum().to(torch.float64).item()                 # the float32 sum, widened exactly
        print("%s step %d: eval_loss %s graph %s" % (setting, step, eval_loss.hex(), float(out["eval_loss"]).hex()))
        assert out["eval_loss"] == eval_loss and out["size"] == len(flat) and np.isfinite(out["grad_norm"])
        keys = [k for w in WIRING.values() for k in w[1:3]]
        if extra is None:
            assert not any(k in out for k in keys)
            continue
        _, key, count_key, counts, totals = WIRING[setting]
        assert [k for k in keys if k in out] == [key, count_key]
        # every utterance here has a finite loss, frames, and no more labels than frames: all three are selected
        extra_sum = float(extra.cpu().numpy().astype(np.float64).sum())      # three float32 values: exact in float64
        count = int(np.diff(offs).sum()) if counts == "labels" else int(seq.sum())
        print("%s step %d: %s %s graph %s, %s %d" % (setting, step, key, extra_sum.hex(), float(out[key]).hex(), count_key, count))
        assert out[key] == extra_sum and type(out[key]) is float
        assert out[count_key] == count and type(out[count_key]) is int
        sums[totals[0]] += out[key]
        sums[totals[1]] += out[count_key]
    assert {t: getattr(graph, t) for t in ALL_TOTALS} == sums                # the sums over the steps; 0 for the other options
    assert graph.global_step == 3
