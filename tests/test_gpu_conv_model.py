"""GPU tests of the convolutional front-end (nnet.config keys conv_layers / conv_channels / conv_bins): model and
command lines.

The float64 model is tests/conv_reference.py's ``torch_conv`` (pinned to torch's conv2d by tests/test_conv_host.py) in front of
the float64 composition of tests/test_gpu_layer_norm_model.py (oracle/torch_f64.py's pieces), differentiated by autograd.
Tolerances are that file's: logits within 1e-4 of the logit scale, gradients through conftest.check_grad."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import conv_reference as ref  # noqa: E402
from test_gpu_layer_norm_model import _check_logits, f64_forward as f64_stack  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

T_, D_, V_ = 12, 12, 5
LENS = np.array([12, 9, 5, 1], np.int32)            # ragged, one utterance of one frame


def _cfg(nnet_type="blstm", **kw):
    cfg = dict(nnet_type=nnet_type, input_dim=D_, left_context=0, right_context=0, num_layers=2, num_neurons=16,
               num_projects=8, num_targets=V_, use_peepholes=True, dropout_rate=1.0, conv_layers=1, conv_channels=8, conv_bins=4)
    if nnet_type != "blstm":
        del cfg["num_projects"]
    cfg.update(kw)
    return {k: v for k, v in cfg.items() if v is not None}


def _model(cfg, seed=3):
    """Biases that matter (the front-end's among them), gains and offsets away from 1 and 0."""
    from lstm_ctc_amd.nnet.model import Model
    model = Model(cfg, "cuda", seed=seed)
    rng = np.random.default_rng(17)
    params = model.ps.export_tf()
    for k in sorted(params):
        if "bias" in k or k == "Variable_1" or k.endswith("/beta"):
            params[k] = rng.normal(0, 0.2, size=params[k].shape).astype(np.float32)
        elif k.endswith("/gamma"):
            params[k] = rng.normal(1.0, 0.2, size=params[k].shape).astype(np.float32)
        elif k == "row_conv/kernel":                                       # (the identity at initialisation)
            params[k] = (params[k] + rng.normal(0, 0.2, size=params[k].shape)).astype(np.float32)
    model.ps.load_tf(params)
    return model, {k: v.astype(np.float64) for k, v in params.items()}


def _batch(T=T_, lens=LENS, seed=5, out_lens=None, T_out=None):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(T, len(lens), D_)).astype(np.float32)
    T_out, out_lens = T_out or T, lens if out_lens is None else out_lens
    dl = rng.normal(size=(T_out, len(lens), V_)).astype(np.float32)
    for b in range(len(lens)):
        x[lens[b]:, b] = 0
        dl[out_lens[b]:, b] = 0                                  # no loss sends gradient into padded frames
    return x, dl


def _run(model, x, dl, lens=LENS, drop_seed=7):
    logits = model.forward(torch.from_numpy(x).cuda(), torch.from_numpy(np.asarray(lens, np.int32)).cuda(),
                           drop_seed=drop_seed).clone()
    front = [c["y"] for c in model.saved["conv"]]
    model.backward(torch.from_numpy(dl).cuda())
    return logits.cpu().numpy(), model.ps.export_tf(grads=True), front


def f64_forward(params, cfg, x_tbd, seq_len, drop_seed=0):
    """The front-end in float64 (the first layer reads the loader's channel-major columns, the others the layer below's
    bin-major ones), then the stack of tests/test_gpu_layer_norm_model.py on its output: that composition takes its layer-0
    width, and with it the reference's residual rule, from the tensor it is handed."""
    from lstm_ctc_amd.nnet.model import conv_config
    h = torch.as_tensor(x_tbd).to(torch.float64)
    for k in range(len(conv_config(cfg))):
        h = ref.torch_conv(h, seq_len, params["conv%d/kernel" % k], params["conv%d/bias" % k], group_major=k == 0)
    if not cfg.get("row_conv_frames"):
        return f64_stack(params, cfg, h, seq_len, drop_seed)
    # row convolution between the top layer and the head: that composition has none, so it is asked for the top layer's output
    # (an identity head) and the filter and the head follow here
    w, b = params["Variable"], params["Variable_1"]
    eye = dict(params, Variable=torch.eye(w.shape[0], dtype=torch.float64), Variable_1=torch.zeros(w.shape[0], dtype=torch.float64))
    top = _torch_row_conv(f64_stack(eye, cfg, h, seq_len, drop_seed), seq_len, params["row_conv/kernel"])
    T, B, _ = top.shape
    return (top.reshape(T * B, -1) @ w + b).reshape(T, B, -1)


def _torch_row_conv(x, lens, w):
    """y[t, b] = sum_j w[j] * x[t + j, b] over the live frames t + j, 0 in dead frames (tests/row_conv_reference.py's fwd)."""
    T = x.shape[0]
    live = (torch.arange(T)[:, None] < torch.as_tensor(np.asarray(lens)).clamp(0, T)[None, :])[:, :, None]
    xs = torch.where(live, x, torch.zeros_like(x))
    out = sum(w[j] * torch.cat([xs[j:], torch.zeros_like(xs[:j])], dim=0) for j in range(w.shape[0]))
    return torch.where(live, out, torch.zeros_like(out))


def f64_gradients(params, cfg, x_tbd, seq_len, dlogits_tbv, drop_seed=0):
    leaves = {k: torch.as_tensor(np.asarray(v, np.float64)).requires_grad_(True) for k, v in params.items()}
    logits = f64_forward(leaves, cfg, x_tbd, seq_len, drop_seed)
    (logits * torch.as_tensor(dlogits_tbv).to(torch.float64)).sum().backward()
    return logits.detach().numpy(), {k: v.grad.numpy() for k, v in leaves.items() if v.grad is not None}


# ---------------------------------------------------------------------------------------------- 1. against the float64 model
CASES = {
    "blstm_residual": _cfg(),                                                   # 2 bins x 8 channels = 2P: layer 0 adds the front-end
    "blstm_residual_dropout": _cfg(dropout_rate=0.8),                           # ... and takes the gradient in front of its mask
    "blstm_residual_one_layer": _cfg(num_layers=1, dropout_rate=0.8),           # (dY straight from the head)
    "blstm_two_layers": _cfg(conv_layers=2, dropout_rate=0.8),                  # bins 4 -> 2 -> 1: layer 0 reads 8 columns
    "blstm_bins6": _cfg(conv_bins=6, dropout_rate=0.8),                         # 2 input channels, bins 6 -> 3: 24 columns
    "blstm_bins6_two_layers_noproj": _cfg(conv_bins=6, conv_layers=2, num_projects=None),     # 6 -> 3 -> 2 (odd in the middle)
    "blstm_one_channel": _cfg(conv_bins=12, conv_layers=3),                     # 12 -> 6 -> 3 -> 2, one input channel
    "lstm_residual0": _cfg("lstm", dropout_rate=0.8),                           # 16 columns = P: the residual on layer 0
    "lstm_two_layers_proj": _cfg("lstm", conv_layers=2, num_projects=6),
    "cudnnlstm": _cfg("cudnnlstm", conv_bins=6, conv_layers=2),
    "layer_norm": _cfg(layer_norm=True, dropout_rate=0.8),
    "time_reduce": _cfg(num_layers=3, time_reduce_layers=1, conv_layers=2, dropout_rate=0.8),
    "chunked": _cfg(chunk_frames=4, lookahead_frames=2, conv_layers=2),
    "row_conv": _cfg("lstm", row_conv_frames=2, conv_bins=6),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_model_against_the_float64_composition(case):
    from conftest import check_grad
    cfg = CASES[case]
    model, p64 = _model(cfg)
    n = cfg["conv_layers"]
    assert len(model.conv) == n and model.ps.D == D_ and model.ps.D0 == model.conv[-1][3] * 8
    T_out = model.output_frames(T_)
    out_lens = np.asarray(model.output_lengths(LENS))
    x, dl = _batch(out_lens=out_lens, T_out=T_out)
    want, want_grads = f64_gradients(p64, cfg, x, LENS, dl, drop_seed=7)
    got, grads, front = _run(model, x, dl)
    _check_logits(got, want, case)
    assert set(grads) == set(want_grads), set(grads) ^ set(want_grads)
    assert {"conv%d/%s" % (k, s) for k in range(n) for s in ("kernel", "bias")} <= set(grads)
    for k in sorted(want_grads):
        check_grad(grads[k], want_grads[k], "conv/" + case, k)
    # the padding of every front-end layer's output is +0, bit for bit, and its live rows are not all zero
    dead = torch.from_numpy(~ref.live_rows(LENS, T_).reshape(-1)).cuda()
    for y in front:
        assert int(y[dead].contiguous().view(torch.int32).abs().sum()) == 0 and bool(y[~dead].any())


@pytest.mark.parametrize("nnet_type", ["blstm", "lstm"])
def test_results_do_not_depend_on_the_padded_frames_of_x(nnet_type):
    model, _ = _model(_cfg(nnet_type, conv_layers=2, dropout_rate=0.8))
    x, dl = _batch()
    dirty = x.copy()
    rng = np.random.default_rng(1)
    for b in range(len(LENS)):
        dirty[LENS[b]:, b] = rng.normal(0, 1e3, size=dirty[LENS[b]:, b].shape)
    dirty[LENS[2]:, 2] = np.nan
    a, b = _run(model, x, dl), _run(model, dirty, dl)
    assert np.array_equal(a[0], b[0])
    for k in a[1]:
        assert np.array_equal(a[1][k], b[1][k]), k


@pytest.mark.parametrize("nnet_type", ["blstm", "lstm", "cudnnlstm"])
def test_keys_absent_and_zero_are_the_plain_model_to_the_bit(nnet_type):
    from lstm_ctc_amd.nnet.model import Model
    base = {k: v for k, v in _cfg(nnet_type, dropout_rate=0.8).items() if not k.startswith("conv_")}
    x, dl = _batch()
    res = []
    for extra in ({}, dict(conv_layers=0), dict(conv_layers=0, conv_channels=8, conv_bins=5)):      # (0: the others are not read)
        m = Model(dict(base, **extra), "cuda", seed=3)
        assert not m.conv and m.ps.D0 == m.ps.D and not any(n.startswith("conv") for n in m.ps.names())
        logits = m.forward(torch.from_numpy(x).cuda(), torch.from_numpy(LENS).cuda(), drop_seed=7).clone()
        assert m.saved["conv"] == []
        m.backward(torch.from_numpy(dl).cuda())
        res.append((logits, m.ps.grad.clone(), m.ps.flat.clone(), dict(m.ps.offsets), m.ps.n_decay))
    for other in res[1:]:
        assert all(torch.equal(a, b) for a, b in zip(res[0][:3], other[:3])) and res[0][3:] == other[3:]
    # ... and the keys change the model
    m = Model(dict(base, conv_layers=1, conv_channels=8, conv_bins=4), "cuda", seed=3)
    out = m.forward(torch.from_numpy(x).cuda(), torch.from_numpy(LENS).cuda(), drop_seed=7)
    assert out.shape == res[0][0].shape and not torch.equal(out, res[0][0])


def test_training_moves_the_front_end_and_checkpoints_round_trip(tmp_path):
    from lstm_ctc_amd.nnet.graph import create_graph_for_training_ctc, create_graph_for_validation_ctc
    cfg = _cfg(conv_layers=2, dropout_rate=0.8)
    graph = create_graph_for_training_ctc(None, cfg, learn_rate=1e-2, clip_norm=5.0, optimizer="sgd", l2_decay_weight=0.1, seed=11)
    ps = graph.model.ps
    rng = np.random.default_rng(41)
    x, _ = _batch()
    labels = np.full((len(LENS), 4), -1, np.int64)
    for b, n in enumerate((4, 3, 2, 1)):
        labels[b, :n] = rng.integers(0, V_ - 1, size=n)
    batch = {"nnet_input": np.ascontiguousarray(x.transpose(1, 0, 2)), "sequence_length": LENS.copy(), "nnet_target": labels}
    start = ps.flat.clone()
    for _ in range(2):
        out = graph.step(batch, fetch_eval=True)
        assert np.isfinite(out["eval_loss"]) and np.isfinite(out["loss"]) and np.isfinite(out["grad_norm"])
    for k in range(2):
        for s in ("kernel", "bias"):
            o, n = ps.offsets["conv%d/%s" % (k, s)], ps.p("conv%d/%s" % (k, s)).numel()
            assert bool(torch.isfinite(ps.flat[o:o + n]).all()) and not torch.equal(ps.flat[o:o + n], start[o:o + n])
    # the kernels are decayed, the biases are not: an update with a zero gradient and l2 = 0.1
    before = ps.flat.clone()
    ps.grad.zero_()
    graph._apply_gradients()
    torch.cuda.synchronize()
    assert torch.equal(ps.flat[ps.n_decay:], before[ps.n_decay:]) and ps.offsets["conv0/bias"] >= ps.n_decay
    o = ps.offsets["conv1/kernel"]
    assert o < ps.n_decay and not torch.equal(ps.flat[o:o + 64], before[o:o + 64])
    path = str(tmp_path / "nnet.2")
    graph.save(path)
    fresh = create_graph_for_validation_ctc(None, dict(cfg, is_training=False), seed=99)
    fresh.restore(path)
    assert torch.equal(fresh.model.ps.flat, ps.flat)
    # the two refusals, through the checkpoint files
    plain_cfg = {k: v for k, v in cfg.items() if not k.startswith("conv_")}
    plain = create_graph_for_validation_ctc(None, dict(plain_cfg, is_training=False), seed=7)
    with pytest.raises(KeyError, match="conv0/kernel"):
        plain.restore(path)
    plain_path = str(tmp_path / "plain.0")
    plain.save(plain_path)
    with pytest.raises(KeyError, match="conv0/kernel"):
        fresh.restore(plain_path)


# ---------------------------------------------------------------------------------------------- 2. command lines
def _cli(cli, *args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", cli)] + list(args), capture_output=True, timeout=300)
    return r.returncode, r.stderr.decode()


def test_the_five_command_lines_run_a_conv_model_and_log_it(tmp_path):
    """nnet-init, -train, -validate, -forward and -align on a tiny latency-controlled conv model, each in a fresh child process:
    the info line, the chunk line with the front-end's two future frames in it, finite losses, one row per input frame."""
    from lstm_ctc_amd.kaldi_io import read_float_matrix_ark, read_int32_vector_ark
    from lstm_ctc_amd.nnet import write_tfrecord
    from lstm_ctc_amd.nnet.model import chunk_horizon
    rng = np.random.default_rng(8)
    D, V = 12, 9
    lines, frames = [], {}
    for i in range(6):
        T = int(rng.integers(24, 41))
        path = str(tmp_path / ("utt%03d.tfrecords" % i))
        write_tfrecord(path, rng.normal(size=(T, D)).astype(np.float32), rng.integers(0, V - 1, size=int(rng.integers(1, 5))))
        lines.append("utt%03d %d %d 1 %s" % (i, T, D, path))
        frames["utt%03d" % i] = T
    scp = tmp_path / "tfrecords.scp"
    scp.write_text("\n".join(sorted(lines)) + "\n")
    config = tmp_path / "conv.config"
    config.write_text("nnet_type = blstm\ninput_dim = 12\nleft_context = 0\nright_context = 0\nnum_layers = 2\nnum_neurons = 32\n"
                      "num_projects = 16\nnum_targets = 9\nuse_peepholes = true\ndropout_rate = 0.9\nchunk_frames = 8\n"
                      "lookahead_frames = 4\nconv_layers = 2\nconv_channels = 8\nconv_bins = 4\n")
    d = str(tmp_path)
    ahead = chunk_horizon(2, 8, 4) - 8 + 2
    want_info = ("convolutional front-end: conv_layers = 2, conv_channels = 8, conv_bins = 4: 3 input channels, bins 4 -> 2 -> 1, "
                 "layer 0 reads 8 columns; %d parameters added; every logit reads 2 more frames on each side"
                 % (9 * 3 * 8 + 8 + 9 * 8 * 8 + 8))
    want_chunk = "a chunk's logits read %d model frames (%d raw frames) past its end" % (ahead, ahead)

    def logged(err):
        info = [l for l in err.split("\n") if "convolutional front-end" in l]
        assert len(info) == 1 and info[0].endswith(want_info), err
        assert len([l for l in err.split("\n") if l.endswith(want_chunk)]) == 1, err

    rc, err = _cli("nnet-init.py", "--objective=ctc", "--batch-size", "3", str(scp), str(config), d + "/nnet.0")
    assert rc == 0, err
    assert len([l for l in err.split("\n") if "convolutional front-end" in l]) == 1, err
    # (training with SpecAugment - its masks run on x, in front of the convolution - and the consistency term on its two views)
    rc, err = _cli("nnet-train.py", "--objective=ctc", "--learn-rate=0.01", "--optimizer=adam", "--seed=1", "--shuffle=false",
                   "--batch-size", "3", "--report-interval=1", "--spec-augment", "time=2x10,freq=1x2,bins=4,cap=50",
                   "--consistency-weight", "0.2", str(scp), str(config), d + "/nnet.0", d + "/nnet.1")
    assert rc == 0, err
    logged(err)
    tr = [float(l.split()[-1]) for l in err.split("\n") if l.startswith("INFO:tensorflow:tr_loss = ")]
    assert tr and np.isfinite(tr).all(), err
    assert len([l for l in err.split("\n") if l.startswith("INFO:tensorflow:consistency weight 0.2: ")]) == 1, err
    rc, err = _cli("nnet-validate.py", "--objective=ctc", "--batch-size", "3", str(scp), str(config), d + "/nnet.1")
    assert rc == 0, err
    logged(err)
    cv = [l for l in err.split("\n") if l.startswith("INFO:tensorflow:cv_loss")]
    assert len(cv) == 1 and np.isfinite(float(cv[0].split()[-1])), err
    rc, err = _cli("nnet-forward.py", "--apply-log=true", "--batch-utts", "3", str(scp), str(config), d + "/nnet.1", "ark:" + d + "/post.ark")
    assert rc == 0, err
    logged(err)
    post = read_float_matrix_ark(d + "/post.ark")
    assert sorted(post) == sorted(frames)
    for k, T in frames.items():
        assert post[k].shape == (T, V) and np.isfinite(post[k]).all()
    rc, err = _cli("nnet-align.py", str(scp), str(config), d + "/nnet.1", "ark:" + d + "/ali.ark")
    assert rc == 0, err
    logged(err)
    ali = read_int32_vector_ark(d + "/ali.ark")
    assert ali and all(len(v) == frames[k] for k, v in ali.items())
