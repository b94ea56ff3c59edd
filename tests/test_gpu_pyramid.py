"""GPU tests of the pyramidal BiLSTM (nnet.config keys time_reduce_layers / time_reduce_factor), model, graph and
command lines.

Sizes and tolerances are tests/test_gpu_lc_blstm.py's - N = 32, P = 16, D = 10, V = 9, peepholes, non-zero biases - with 3
layers; logits within 1e-4 of the logit scale, gradients through conftest.check_grad.  The reference is
tests/time_reduce_reference.py (float64, pinned to oracle/torch_f64.py by tests/test_time_reduce_host.py)."""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from time_reduce_reference import cdiv, output_lengths, pyramid_gradients  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(**kw):
    cfg = dict(nnet_type="blstm", input_dim=10, left_context=0, right_context=0, num_layers=3,
               num_neurons=32, num_projects=16, num_targets=9, use_peepholes=True, dropout_rate=1.0)
    cfg.update(kw)
    return cfg


def _inputs(rng, D, B, T, seq_len):
    x = rng.normal(size=(B, T, D)).astype(np.float32)
    for b in range(B):
        x[b, seq_len[b]:] = 0
    return x


def _model(cfg, rng, seed=3):
    from lstm_ctc_amd.nnet.model import Model
    model = Model(cfg, "cuda", seed=seed)
    params = model.ps.export_tf()
    for k in params:                                            # non-zero biases so they matter
        if "bias" in k or k == "Variable_1":
            params[k] = rng.normal(0, 0.2, size=params[k].shape).astype(np.float32)
    model.ps.load_tf(params)
    return model, {k: v.astype(np.float64) for k, v in params.items()}


def _tm(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a.transpose(1, 0, 2)).astype(dtype)).cuda()


def _dlogits(rng, shape, out_len):
    dl = rng.normal(size=shape)                                 # batch-major [B, T_L, V]
    for b in range(shape[0]):
        dl[b, out_len[b]:] = 0                                  # zero beyond the OUTPUT lengths
    return dl


def _check_logits(got, ref):
    scale = np.abs(ref).max()
    err = np.abs(got - ref)
    print("logits: max error %.3e, scale %.3e" % (err.max(), scale))
    assert err.max() < 1e-4 * max(scale, 1.0), err.max()
    assert np.all(err <= 1e-4 * np.maximum(np.abs(ref), 0.1 * max(scale, 1.0)))


# ---------------------------------------------------------------------------------------------- 1. against the float64 model
RAGGED = [11, 8, 6, 4, 1]
CASES = {   # name -> (layers, r, B, T, lengths or None, config overrides, launch train)
    "l1_r2": ((1,), 2, 5, 11, RAGGED, {}, False),
    "l1_r2_dropout": ((1,), 2, 5, 11, RAGGED, dict(dropout_rate=0.8), False),
    "l1_r2_dropout_launch_train": ((1,), 2, 5, 11, RAGGED, dict(dropout_rate=0.8), True),
    "l1_r2_launch_train": ((1,), 2, 5, 11, RAGGED, {}, True),
    "l12_r2": ((1, 2), 2, 5, 11, RAGGED, {}, False),
    "l2_r3": ((2,), 3, 5, 11, RAGGED, {}, False),
    "l1_r2_b70": ((1,), 2, 70, 6, None, {}, False),             # past the 64- and 128-row schedule limits
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_model_against_the_float64_restatement(case):
    from conftest import check_grad
    from lstm_ctc_amd import ops
    layers, r, B, T, lens, extra, train = CASES[case]
    cfg = _cfg(time_reduce_layers=",".join(map(str, layers)), time_reduce_factor=r, **extra)
    rng = np.random.default_rng(sorted(CASES).index(case) + 90)
    if lens is None:
        lens = np.sort(rng.integers(1, T + 1, size=B))[::-1].copy()
        lens[0], lens[-1] = T, 1
    seq_len = np.asarray(lens, np.int32)
    x = _inputs(rng, cfg["input_dim"], B, T, seq_len)
    model, p64 = _model(cfg, rng)
    R = r ** len(layers)
    assert model.time_factor == R and model.output_frames(T) == cdiv(T, R)
    out_len = output_lengths(seq_len, layers, r)
    assert np.array_equal(model.output_lengths(seq_len), out_len) and np.array_equal(out_len, -(-seq_len.astype(np.int64) // R))
    TL = cdiv(T, R)
    dl = _dlogits(rng, (B, TL, cfg["num_targets"]), out_len)
    ref_logits, ref_grads = pyramid_gradients(p64, cfg, x.transpose(1, 0, 2).astype(np.float64), seq_len,
                                              dl.transpose(1, 0, 2), layers, r, drop_seed=7)
    sl = torch.from_numpy(seq_len).cuda()
    with (ops.force_launch_train() if train else contextlib.nullcontext()):
        logits = model.forward(_tm(x), sl, drop_seed=7)
        assert tuple(logits.shape) == (TL, B, cfg["num_targets"])
        assert torch.equal(model.output_lengths(sl).cpu(), torch.from_numpy(out_len.astype(np.int32)))
        got = logits.cpu().numpy()
        enc = model.encoder()
        model.backward(_tm(dl))
        if train:
            assert ops.last_lstm_schedule()["kind"] in ("launch_train", "two_stream_train")
    assert tuple(enc.shape)[0] == B and bool(torch.isfinite(enc).all())
    _check_logits(got, ref_logits.numpy())
    grads = model.ps.export_tf(grads=True)
    assert set(grads) == set(ref_grads), set(grads) ^ set(ref_grads)
    for k in sorted(ref_grads):
        check_grad(grads[k], ref_grads[k], "pyramid/" + case, k)


# ---------------------------------------------------------------------------------------------- 2. off is the plain model; refusals
def test_key_absent_0_and_0_with_a_factor_are_the_plain_model_to_the_bit():
    from lstm_ctc_amd import ops
    from lstm_ctc_amd.nnet.model import Model
    rng = np.random.default_rng(70)
    B, T = 5, 11
    cfg = _cfg(dropout_rate=0.8)
    seq_len = np.array(RAGGED, np.int32)
    x = _inputs(rng, cfg["input_dim"], B, T, seq_len)
    dl = _tm(_dlogits(rng, (B, T, cfg["num_targets"]), seq_len))
    xt, sl = _tm(x), torch.from_numpy(seq_len).cuda()
    res = []
    for extra in ({}, dict(time_reduce_layers=0), dict(time_reduce_layers=0, time_reduce_factor=3)):
        m = Model(dict(cfg, **extra), "cuda", seed=3)
        assert m.time_factor == 1 and m.time_reduce == () and m.output_frames(T) == T and m.output_lengths(sl) is sl
        logits = m.forward(xt, sl, drop_seed=7).clone()
        fwd = ops.last_lstm_schedule()
        m.backward(dl)
        res.append((logits, m.ps.grad.clone(), m.ps.flat.clone(), dict(m.ps.offsets), fwd, ops.last_lstm_schedule()))
    for got in res[1:]:
        assert torch.equal(got[0], res[0][0]) and torch.equal(got[1], res[0][1]) and torch.equal(got[2], res[0][2])
        assert got[3] == res[0][3] and got[4] == res[0][4] and got[5] == res[0][5]
    # ... and the key changes the model: other logits' shape, a wider kernel
    m = Model(dict(cfg, time_reduce_layers=1), "cuda", seed=3)
    assert tuple(m.forward(xt, sl, drop_seed=7).shape) == (6, B, 9)
    assert m.ps.shapes["fd1/frnn1/kernel"] == (2 * 32 + 16, 128)


@pytest.mark.parametrize("bad", [dict(compute_dtype="bf16"), dict(compute_dtype="bf16x3"), dict(nnet_type="lstm"),
                                 dict(chunk_frames=4)], ids=["bf16", "bf16x3", "lstm", "chunk"])
def test_key_is_refused_where_it_cannot_run(bad):
    from lstm_ctc_amd.nnet.model import Model
    with pytest.raises(ValueError, match="time_reduce_layers"):
        Model(_cfg(time_reduce_layers=1, **bad), "cuda", seed=3)
    Model(_cfg(time_reduce_layers=0, **bad), "cuda", seed=3)                         # 0: the key is off


def test_pack_frames_with_the_key_runs_padded():
    from lstm_ctc_amd.nnet.model import Model
    m = Model(_cfg(time_reduce_layers=1, pack_frames=True), "cuda", seed=3)
    assert m.pack_frames is False
    rng = np.random.default_rng(71)
    seq_len = np.array(RAGGED, np.int32)
    x = _inputs(rng, 10, 5, 11, seq_len)
    m.forward(_tm(x), torch.from_numpy(seq_len).cuda())
    assert m.packed is False


# ---------------------------------------------------------------------------------------------- 3. graph
def _batch(B=5, T=22, D=10, V=9, seed=3):
    """Lengths 22, 17, 12, 9 and 5 with 1 to 3 labels (the last utterance: 1): the ceil(len / 2) = 11, 9, 6, 5, 3 and the
    ceil(len / 4) = 6, 5, 3, 3, 2 output frames hold them with their repeats, so every loss is finite."""
    rng = np.random.default_rng(seed)
    seq = np.array([22, 17, 12, 9, 5], np.int32)[:B]
    x = rng.normal(size=(B, T, D)).astype(np.float32)
    y = np.full((B, 4), -1, np.int64)
    for b in range(B):
        n = 1 if b >= 2 else int(rng.integers(1, 4))
        y[b, :n] = rng.integers(0, V - 1, size=n)
        x[b, seq[b]:] = 0
    return {"nnet_input": x, "sequence_length": seq, "nnet_target": y}


def test_train_step_scores_and_decodes_under_the_output_lengths(oracle):
    from lstm_ctc_amd.nnet.graph import create_graph_for_training_ctc
    cfg = _cfg(time_reduce_layers=1)
    graph = create_graph_for_training_ctc(None, cfg, learn_rate=1e-2, clip_norm=5.0, optimizer="sgd", seed=11)
    assert "output_length" in graph
    batch = _batch()
    seq = batch["sequence_length"]
    before = graph.model.ps.flat.clone()
    out = graph.step(batch, fetch_eval=True, fetch_logits=True)
    out_len = (seq + 1) // 2
    assert np.array_equal(out["sequence_length"], seq) and np.array_equal(out["output_length"], out_len)
    logits = out["logits"]                                       # [B, T_L, V]
    assert logits.shape == (5, 11, 9)
    tbv = np.ascontiguousarray(logits.transpose(1, 0, 2)).astype(np.float64)
    flat, offs = oracle.flatten_labels(batch["nnet_target"])
    ref_loss, _, _ = oracle.ctc_loss(tbv, flat, offs, out_len.astype(np.int32), want_grad=False)
    assert np.isfinite(ref_loss).all()
    assert abs(out["eval_loss"] - ref_loss.sum()) / ref_loss.sum() < 1e-4
    # ... which the input lengths would not give (they read frames the logits do not have; here: another number)
    tok, n = out["decoded"]
    rt, rn, _ = oracle.ctc_greedy(tbv.astype(np.float32), out_len.astype(np.int32))
    assert np.array_equal(n, rn)
    for b in range(len(n)):
        assert np.array_equal(tok[b, :n[b]], rt[b, :n[b]])
    assert not torch.equal(before, graph.model.ps.flat) and np.isfinite(out["grad_norm"])
    # labels + repeats against the output frames, from the host's copies
    want_short = sum(int(len(flat[offs[b]:offs[b + 1]]) + int((np.diff(flat[offs[b]:offs[b + 1]]) == 0).sum()) > out_len[b])
                     for b in range(5))
    assert graph.time_reduce_short == want_short
    plain = create_graph_for_training_ctc(None, _cfg(), learn_rate=1e-2, optimizer="sgd", seed=11)
    assert "output_length" not in plain.step(batch) and "output_length" not in plain


def test_consistency_and_spec_augment_count_the_output_frames():
    from lstm_ctc_amd.nnet.augment import SpecAugment
    from lstm_ctc_amd.nnet.graph import create_graph_for_training_ctc
    spec = SpecAugment(time_masks=2, time_width=4, time_percent=50, freq_masks=1, freq_width=3, freq_bins=10)
    graph = create_graph_for_training_ctc(None, _cfg(time_reduce_layers="1,2"), learn_rate=1e-2, optimizer="sgd", seed=11,
                                          spec_augment=spec, consistency_weight=0.2)
    batch = _batch()
    out = graph.step(batch, fetch_logits=True)
    out_len = -(-batch["sequence_length"] // 4)
    assert out["cr_frames"] == int(out_len.sum()) and out["cr_loss"] > 0 and np.isfinite(out["loss"])
    assert out["logits"].shape == (10, 6, 9)
    assert np.array_equal(out["output_length"], np.concatenate([out_len, out_len]))
    assert np.array_equal(out["sequence_length"], np.concatenate([batch["sequence_length"]] * 2))


@pytest.mark.parametrize("criterion", [dict(delay_penalty=0.05), dict(entropy_weight=0.1), dict(star_penalty=(2.0, 1.0)),
                                       dict()], ids=["delay", "entropy", "star", "label_smoothing"])
def test_criterion_options_run_with_the_key(criterion):
    from lstm_ctc_amd.nnet.graph import create_graph_for_training_ctc
    cfg = _cfg(time_reduce_layers=1, **({} if criterion else dict(uniform_label_sm=0.1)))
    graph = create_graph_for_training_ctc(None, cfg, learn_rate=1e-2, optimizer="sgd", seed=11, **criterion)
    out = graph.step(_batch())
    assert np.isfinite(out["loss"]) and np.isfinite(out["grad_norm"])


def test_table_options_and_alignment_are_refused_at_construction():
    from lstm_ctc_amd.nnet import graph as G
    cfg = _cfg(time_reduce_layers=1)
    for make in (lambda: G.create_graph_for_training_ctc(None, cfg, learn_rate=1e-2, align_window=2),
                 lambda: G.create_graph_for_validation_ctc(None, cfg, align_window=0),
                 lambda: G.create_graph_for_training_ctc(None, cfg, learn_rate=1e-2, teacher_weight=0.5),
                 lambda: G.create_graph_for_training_xent(None, cfg, learn_rate=1e-2),
                 lambda: G.create_graph_for_validation_xent(None, cfg),
                 lambda: G.create_graph_for_training_kd(None, cfg, learn_rate=1e-2),
                 lambda: G.create_graph_for_validation_kd(None, cfg),
                 lambda: G.create_graph_for_alignment(None, cfg)):
        with pytest.raises(ValueError, match="time_reduce_layers"):
            make()
    graph = G.create_graph_for_validation_ctc(None, cfg)
    with pytest.raises(ValueError, match="time_reduce_layers"):
        graph.align(_batch())


# ---------------------------------------------------------------------------------------------- 4. command lines
def _run(cli, *args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", cli)] + list(args), capture_output=True, timeout=600)
    return r.returncode, r.stderr.decode()


def test_cli_trains_validates_and_forwards_with_and_without_the_key(tmp_path):
    from lstm_ctc_amd.kaldi_io import read_float_matrix_ark
    from lstm_ctc_amd.nnet import write_tfrecord
    rng = np.random.default_rng(8)
    D, V = 6, 9
    lines, frames = [], {}
    for i in range(8):
        T = int(rng.integers(24, 41))
        path = str(tmp_path / ("utt%03d.tfrecords" % i))
        write_tfrecord(path, rng.normal(size=(T, D)).astype(np.float32), rng.integers(0, V - 1, size=int(rng.integers(1, 5))))
        lines.append("utt%03d %d %d 1 %s" % (i, T, D, path))
        frames["utt%03d" % i] = T
    scp = tmp_path / "tfrecords.scp"
    scp.write_text("\n".join(sorted(lines)) + "\n")
    text = ("nnet_type = blstm\ninput_dim = 6\nleft_context = 0\nright_context = 0\nnum_layers = 3\n"
            "num_neurons = 32\nnum_projects = 16\nnum_targets = 9\nuse_peepholes = true\ndropout_rate = 0.9\n")
    plain, pyramid = tmp_path / "plain.config", tmp_path / "pyramid.config"
    plain.write_text(text)
    pyramid.write_text(text + "time_reduce_layers = 1\n")
    d = str(tmp_path)
    nets = {}
    for name, config in (("plain", plain), ("pyramid", pyramid)):
        nets[name] = d + "/%s.0" % name
        rc, err = _run("nnet-init.py", "--objective=ctc", "--batch-size", "3", str(scp), str(config), nets[name])
        assert rc == 0, err
        assert len([l for l in err.split("\n") if "pyramidal BiLSTM" in l]) == (1 if name == "pyramid" else 0), err
    rc, err = _run("nnet-train.py", "--objective=ctc", "--learn-rate=0.01", "--optimizer=adam", "--seed=1", "--shuffle=false",
                   "--batch-size", "3", "--report-interval=1", str(scp), str(pyramid), nets["pyramid"], d + "/pyramid.1")
    assert rc == 0, err
    assert any(l.startswith("INFO:tensorflow:step = 3, ") for l in err.split("\n")), err          # 8 utterances by 3: 3 steps
    tr = [l for l in err.split("\n") if l.startswith("INFO:tensorflow:tr_loss")]
    assert len(tr) == 1 and np.isfinite(float(tr[0].split()[-1]))
    info = [l for l in err.split("\n") if "pyramidal BiLSTM" in l]
    assert len(info) == 1 and "time_reduce_layers = 1, time_reduce_factor = 2: R = 2" in info[0], err
    assert "once per 2 model frames (2 raw frames)" in info[0], info
    assert len([l for l in err.split("\n") if "time reduction by 2: 0 utterance(s)" in l]) == 1, err
    rc, err = _run("nnet-validate.py", "--objective=ctc", "--batch-size", "3", str(scp), str(pyramid), d + "/pyramid.1")
    assert rc == 0, err
    cv = [l for l in err.split("\n") if l.startswith("INFO:tensorflow:cv_loss")]
    assert len(cv) == 1 and np.isfinite(float(cv[0].split()[-1])), err
    # a plain checkpoint does not fit the pyramid
    rc, err = _run("nnet-validate.py", "--objective=ctc", "--batch-size", "3", str(scp), str(pyramid), nets["plain"])
    assert rc != 0 and "fd1/frnn1/kernel" in err, err
    for name, config, net in (("plain", plain, nets["plain"]), ("pyramid", pyramid, d + "/pyramid.1")):
        ark = d + "/%s.ark" % name
        rc, err = _run("nnet-forward.py", "--apply-log=true", "--batch-utts", "3", str(scp), str(config), net, "ark:" + ark)
        assert rc == 0, err
        assert len([l for l in err.split("\n") if "pyramidal BiLSTM" in l]) == (1 if name == "pyramid" else 0)
        post = read_float_matrix_ark(ark)
        assert sorted(post) == sorted(frames)
        for k, T in frames.items():
            assert post[k].shape == ((T + 1) // 2 if name == "pyramid" else T, V), (name, k, post[k].shape, T)
            assert np.isfinite(post[k]).all()
    # a table at the input's frame rate is refused by name
    targets = tmp_path / "ali.txt"
    targets.write_text("".join("%s %s\n" % (k, " ".join(["0"] * T)) for k, T in sorted(frames.items())))
    rc, err = _run("nnet-train.py", "--objective=ctc", "--frame-targets", "ark,t:" + str(targets), "--align-window", "2",
                   "--learn-rate=0.01", "--batch-size", "3", str(scp), str(pyramid), nets["pyramid"], d + "/never")
    assert rc != 0 and "time_reduce_layers" in err and not os.path.exists(d + "/never"), err
