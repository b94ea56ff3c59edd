"""GPU tests of layer normalisation between the LSTM layers (nnet.config key layer_norm): model, graph and
command lines.

The float64 model is composed here from oracle/torch_f64.py's ``lstmp_forward``, ``reverse_sequence`` and ``dropout_mask`` and
tests/layer_norm_reference.py's ``torch_layer_norm`` (pinned to torch by tests/test_layer_norm_host.py), and differentiated by
autograd.  Tolerances are those of the other float64 model comparisons (tests/test_gpu_pyramid.py, tests/test_gpu_lc_blstm.py):
logits within 1e-4 of the logit scale, gradients through conftest.check_grad; packed against padded within two of those, as
tests/test_gpu_packed.py argues; bf16 against fp32 at tests/test_gpu_model.py's bf16 bound (3e-2 / 6e-2)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import layer_norm_reference as ref  # noqa: E402
from time_reduce_reference import cdiv, torch_time_reduce  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

T_, D_, V_ = 12, 6, 5
LENS = np.array([12, 9, 5, 1], np.int32)            # ragged, one short utterance
CUDNN_CELL = "rnn/multi_rnn_cell/cell_%d/cudnn_compatible_lstm_cell"


def _cfg(nnet_type="blstm", **kw):
    cfg = dict(nnet_type=nnet_type, input_dim=D_, left_context=0, right_context=0, num_layers=2, num_neurons=16,
               num_projects=8, num_targets=V_, use_peepholes=True, dropout_rate=1.0, layer_norm=True)
    if nnet_type != "blstm":
        del cfg["num_projects"]
    cfg.update(kw)
    return {k: v for k, v in cfg.items() if v is not None}


def _model(cfg, seed=3):
    """Biases that matter, gains and offsets away from 1 and 0."""
    from lstm_ctc_amd.nnet.model import Model
    model = Model(cfg, "cuda", seed=seed)
    rng = np.random.default_rng(17)
    params = model.ps.export_tf()
    for k in sorted(params):
        if "bias" in k or k == "Variable_1" or k.endswith("/beta"):
            params[k] = rng.normal(0, 0.2, size=params[k].shape).astype(np.float32)
        elif k.endswith("/gamma"):
            params[k] = rng.normal(1.0, 0.2, size=params[k].shape).astype(np.float32)
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
    saved = model.saved
    # every layer's normalised output as its reader takes it (a reduced layer: r frames side by side, at its own frame rate),
    # with the reader's frame count and lengths; the head reads at the top layer's
    readers = saved["layers"][1:] + saved["layers"][-1:]
    normed = [L["inp"] for L in saved["layers"][1:]] + [saved["top"]]
    shapes = [(L["T"], L["seq_len"].cpu().numpy()) for L in readers]
    model.backward(torch.from_numpy(dl).cuda())
    return logits.cpu().numpy(), model.ps.export_tf(grads=True), normed, shapes


def f64_forward(params, cfg, x_tbd, seq_len, drop_seed=0):
    """Logits [T_L, B, V] float64 of the plain-head model of ``cfg``: blstm (with time_reduce_layers or chunk_frames), lstm or
    cudnnlstm, with dropout(LN(Y_i)) as every layer's output when cfg['layer_norm']."""
    from lstm_ctc_amd.nnet.model import chunk_config, time_reduce_config
    from oracle.torch_f64 import dropout_mask, lstmp_forward, reverse_sequence
    g = lambda k: params.get(k)
    kind = cfg["nnet_type"]
    x = torch.as_tensor(x_tbd).to(torch.float64)
    sl = torch.as_tensor(np.asarray(seq_len)).to(torch.int64)
    keep = 1.0 if kind == "cudnnlstm" or not cfg.get("is_training", True) else float(cfg.get("dropout_rate", 1.0))
    layers, r = time_reduce_config(cfg)
    chunk, lookahead = chunk_config(cfg)
    ln = bool(cfg.get("layer_norm"))
    T, B, D = x.shape
    finput = x
    for i in range(cfg["num_layers"]):
        if i in layers:
            finput = torch_time_reduce(finput, sl.clamp(0, T), r)
            sl, T = (sl.clamp(0, T) + r - 1) // r, cdiv(T, r)
        if kind == "blstm":
            halves = []
            for d, prefix in enumerate(("fd%d/frnn%d" % (i, i), "bd%d/brnn%d" % (i, i))):
                cell = (g(prefix + "/kernel"), g(prefix + "/bias"), g(prefix + "/w_f_diag"), g(prefix + "/w_i_diag"),
                        g(prefix + "/w_o_diag"), g(prefix + "/projection/kernel"), 5.0)
                if d == 0:
                    o = lstmp_forward(finput, sl, *cell)
                elif chunk:
                    Tc, kept = min(chunk + lookahead, T), []
                    for c in range(cdiv(T, chunk)):
                        lens_c = (sl - c * chunk).clamp(0, Tc)
                        window = finput[c * chunk:min(c * chunk + Tc, T)]
                        kept.append(reverse_sequence(lstmp_forward(reverse_sequence(window, lens_c), lens_c, *cell), lens_c)[:chunk])
                    o = torch.cat(kept, dim=0)
                else:
                    o = reverse_sequence(lstmp_forward(reverse_sequence(finput, sl), sl, *cell), sl)
                if not ln:
                    mask = dropout_mask(drop_seed, 2 * i + d, T, B, o.shape[2], keep, "cpu")
                    o = o if mask is None else o * mask
                halves.append(o)
            y = torch.cat(halves, dim=2)
            y = finput + y if (i == 0 and D == y.shape[2]) else y
            width = y.shape[2] // 2
        else:
            prefix = (CUDNN_CELL % i) if kind == "cudnnlstm" else "drnn%d/lstm_cell" % i
            y = lstmp_forward(finput, sl, g(prefix + "/kernel"), g(prefix + "/bias"), g(prefix + "/w_f_diag"),
                              g(prefix + "/w_i_diag"), g(prefix + "/w_o_diag"), g(prefix + "/projection/kernel"),
                              0.0 if kind == "cudnnlstm" else 1.0)
            if kind == "lstm" and not (i == 0 and D != y.shape[2]):
                y = y + finput
            width = y.shape[2]
            if not ln and keep < 1.0:
                y = y * dropout_mask(drop_seed, 2 * i, T, B, width, keep, "cpu")
        if ln:
            y = ref.torch_layer_norm(y, sl, g("ln%d/gamma" % i), g("ln%d/beta" % i),
                                     ref.mask(drop_seed, 2 * i, T, B, y.shape[2], width, keep))
        finput = y
    return (finput.reshape(T * B, -1) @ g("Variable") + g("Variable_1")).reshape(T, B, -1)


def f64_gradients(params, cfg, x_tbd, seq_len, dlogits_tbv, drop_seed=0):
    leaves = {k: torch.as_tensor(np.asarray(v, np.float64)).requires_grad_(True) for k, v in params.items()}
    logits = f64_forward(leaves, cfg, x_tbd, seq_len, drop_seed)
    (logits * torch.as_tensor(dlogits_tbv).to(torch.float64)).sum().backward()
    return logits.detach().numpy(), {k: v.grad.numpy() for k, v in leaves.items() if v.grad is not None}


def _check_logits(got, want, tag, rel=1e-4, per_logit=True):
    """Within ``rel`` of the logit scale; fp32: and per logit, for those of at least a tenth of the scale (the bf16 bound of
    tests/test_gpu_model.py is the first alone)."""
    scale = max(float(np.abs(want).max()), 1.0)
    err = np.abs(got - want)
    print("%s: logits max error %.3e, scale %.3e" % (tag, err.max(), scale))
    assert err.max() < rel * scale, (tag, err.max())
    if per_logit:
        assert np.all(err <= rel * np.maximum(np.abs(want), 0.1 * scale))


def _check_padding_is_zero(normed, shapes, B):
    """The padding of every layer's normalised output is +0, bit for bit."""
    for t, (T, lens) in zip(normed, shapes):
        dead = torch.from_numpy(~ref.live_rows(lens, T).reshape(-1)).cuda()
        assert t.shape[0] == T * B and int(t[dead].contiguous().view(torch.int32).abs().sum()) == 0
        assert bool(t[~dead].any())


# ---------------------------------------------------------------------------------------------- 1. against the float64 model
CASES = {
    "blstm_proj": _cfg(),
    "blstm_proj_dropout": _cfg(dropout_rate=0.8),
    "blstm_noproj": _cfg(num_projects=None),
    "blstm_noproj_dropout": _cfg(num_projects=None, dropout_rate=0.8),
    "blstm_residual": _cfg(num_projects=3, dropout_rate=0.8),            # D == 2P: layer 0 adds its input before the norm
    "lstm": _cfg("lstm"),
    "lstm_proj_dropout": _cfg("lstm", num_projects=8, dropout_rate=0.8),
    "lstm_residual0_dropout": _cfg("lstm", num_projects=6, dropout_rate=0.8),   # D == P: the residual on layer 0 too
    "cudnnlstm": _cfg("cudnnlstm"),
    "chunked": _cfg(chunk_frames=4, lookahead_frames=2, dropout_rate=0.8),
    "time_reduce": _cfg(num_layers=3, time_reduce_layers=1, dropout_rate=0.8),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_model_against_the_float64_composition(case):
    from conftest import check_grad
    cfg = CASES[case]
    model, p64 = _model(cfg)
    assert model.layer_norm and model.ps.layer_norm
    T_out = model.output_frames(T_)
    out_lens = np.asarray(model.output_lengths(LENS))
    x, dl = _batch(out_lens=out_lens, T_out=T_out)
    want, want_grads = f64_gradients(p64, cfg, x, LENS, dl, drop_seed=7)
    got, grads, normed, shapes = _run(model, x, dl)
    _check_logits(got, want, case)
    assert set(grads) == set(want_grads), set(grads) ^ set(want_grads)
    assert {"ln0/gamma", "ln0/beta", "ln1/gamma", "ln1/beta"} <= set(grads)
    for k in sorted(want_grads):
        check_grad(grads[k], want_grads[k], "layer_norm/" + case, k)
    _check_padding_is_zero(normed, shapes, len(LENS))


def test_bf16_against_fp32():
    """compute_dtype = bf16 on 32 units: the normalised output is fp32 and the next product casts its own shadow."""
    res = {}
    for cd in ("fp32", "bf16"):
        cfg = _cfg(num_neurons=32, num_projects=16, dropout_rate=0.8, compute_dtype=cd)
        model, _ = _model(cfg)
        assert model.bf16 == (cd == "bf16")
        x, dl = _batch()
        res[cd] = _run(model, x, dl)
    _check_logits(res["bf16"][0], res["fp32"][0].astype(np.float64), "bf16", rel=3e-2, per_logit=False)
    for k in sorted(res["fp32"][1]):
        a, b = res["bf16"][1][k], res["fp32"][1][k]
        assert np.abs(a - b).max() < 6e-2 * max(float(np.abs(b).max()), 1e-3), k
    _check_padding_is_zero(res["bf16"][2], res["bf16"][3], len(LENS))


@pytest.mark.parametrize("nnet_type", ["blstm", "lstm", "cudnnlstm"])
def test_key_absent_and_false_are_the_plain_model_to_the_bit(nnet_type):
    from lstm_ctc_amd.nnet.model import Model
    base = _cfg(nnet_type, dropout_rate=0.8)
    del base["layer_norm"]
    x, dl = _batch()
    res = []
    for extra in ({}, dict(layer_norm=False)):
        m = Model(dict(base, **extra), "cuda", seed=3)
        assert not m.layer_norm and not any(n.startswith("ln") for n in m.ps.names())
        logits = m.forward(torch.from_numpy(x).cuda(), torch.from_numpy(LENS).cuda(), drop_seed=7).clone()
        m.backward(torch.from_numpy(dl).cuda())
        res.append((logits, m.ps.grad.clone(), m.ps.flat.clone(), dict(m.ps.offsets), m.ps.n_decay))
    assert all(torch.equal(a, b) for a, b in zip(res[0][:3], res[1][:3])) and res[0][3:] == res[1][3:]
    # ... and the key changes the model
    m = Model(dict(base, layer_norm=True), "cuda", seed=3)
    assert torch.equal(m.ps.flat[:m.ps.n_decay], res[0][2][:res[0][4]])                   # the same seed, the same tensors
    assert not torch.equal(m.forward(torch.from_numpy(x).cuda(), torch.from_numpy(LENS).cuda(), drop_seed=7), res[0][0])


def test_pack_frames_equals_the_padded_run():
    from conftest import GRAD_TOL
    res = {}
    for pack in (False, True):
        model, _ = _model(_cfg(dropout_rate=0.8, pack_frames=pack))
        x, dl = _batch()
        res[pack] = _run(model, x, dl)
        assert model.packed is pack
    assert np.abs(res[True][0] - res[False][0]).max() < 2e-4 * max(np.abs(res[False][0]).max(), 1.0)
    for k in sorted(res[False][1]):
        a, b = res[True][1][k], res[False][1][k]
        assert np.abs(a - b).max() < 2 * GRAD_TOL * max(float(np.abs(b).max()), 1e-3), k
    _check_padding_is_zero(res[True][2], res[True][3], len(LENS))


# ---------------------------------------------------------------------------------------------- 2. graph
def _graph_batch():
    rng = np.random.default_rng(41)
    x, _ = _batch()
    labels = np.full((len(LENS), 4), -1, np.int64)
    for b, n in enumerate((4, 3, 2, 1)):
        labels[b, :n] = rng.integers(0, V_ - 1, size=n)
    return {"nnet_input": np.ascontiguousarray(x.transpose(1, 0, 2)), "sequence_length": LENS.copy(), "nnet_target": labels}, x


def test_training_moves_the_gains_leaves_them_undecayed_and_checkpoints_round_trip(tmp_path):
    from lstm_ctc_amd.nnet.graph import create_graph_for_training_ctc, create_graph_for_validation_ctc
    cfg = _cfg(dropout_rate=0.8)
    graph = create_graph_for_training_ctc(None, cfg, learn_rate=1e-2, clip_norm=5.0, optimizer="sgd", l2_decay_weight=0.1, seed=11)
    ps = graph.model.ps
    batch, x = _graph_batch()
    for _ in range(2):
        out = graph.step(batch, fetch_eval=True)
        assert np.isfinite(out["eval_loss"]) and np.isfinite(out["loss"]) and np.isfinite(out["grad_norm"])
    for i in range(2):
        gamma, beta = ps.p("ln%d/gamma" % i), ps.p("ln%d/beta" % i)
        assert bool(torch.isfinite(gamma).all()) and not torch.equal(gamma, torch.ones_like(gamma)) and bool(beta.any())
    # no decay on them: an update with a zero gradient and l2 = 0.1 shrinks every decayed tensor and leaves gamma (set back to
    # exactly 1) and beta as they are
    ps.p("ln0/gamma").fill_(1.0)
    before = ps.flat.clone()
    ps.grad.zero_()
    graph._apply_gradients()
    torch.cuda.synchronize()
    assert torch.equal(ps.p("ln0/gamma"), torch.ones_like(ps.p("ln0/gamma")))
    assert torch.equal(ps.flat[ps.n_decay:], before[ps.n_decay:])
    kernel = ps.offsets["fd0/frnn0/kernel"]
    assert not torch.equal(ps.flat[kernel:kernel + 64], before[kernel:kernel + 64])
    fwd = lambda m: m.forward(torch.from_numpy(x).cuda(), torch.from_numpy(LENS).cuda())
    path = str(tmp_path / "nnet.2")
    graph.save(path)
    fresh = create_graph_for_validation_ctc(None, dict(cfg, is_training=False), seed=99)      # (as the tools build it)
    fresh.restore(path)
    assert torch.equal(fresh.model.ps.flat, ps.flat)
    graph.model.is_training, graph.model.keep = False, 1.0                                   # (as CTCGraph's own eval pass does)
    assert torch.equal(fwd(fresh.model), fwd(graph.model))
    # the two refusals, through the checkpoint files
    plain_cfg = dict(cfg)
    del plain_cfg["layer_norm"]
    plain = create_graph_for_validation_ctc(None, dict(plain_cfg, is_training=False), seed=7)
    with pytest.raises(KeyError, match="ln0/gamma"):
        plain.restore(path)
    plain_path = str(tmp_path / "plain.0")
    plain.save(plain_path)
    with pytest.raises(KeyError, match="ln0/gamma"):
        fresh.restore(plain_path)


# ---------------------------------------------------------------------------------------------- 3. command lines
def _cli(cli, *args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", cli)] + list(args), capture_output=True, timeout=600)
    return r.returncode, r.stderr.decode()


def test_cli_trains_and_forwards_with_the_key_and_refuses_a_plain_checkpoint(tmp_path):
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
    plain, normed = tmp_path / "plain.config", tmp_path / "ln.config"
    plain.write_text(text)
    normed.write_text(text + "layer_norm = true\n")
    d = str(tmp_path)
    nets = {}
    for name, config in (("plain", plain), ("ln", normed)):
        nets[name] = d + "/%s.0" % name
        rc, err = _cli("nnet-init.py", "--objective=ctc", "--batch-size", "3", str(scp), str(config), nets[name])
        assert rc == 0, err
        assert len([l for l in err.split("\n") if "layer normalisation" in l]) == (1 if name == "ln" else 0), err
    rc, err = _cli("nnet-train.py", "--objective=ctc", "--learn-rate=0.01", "--optimizer=adam", "--seed=1", "--shuffle=false",
                   "--batch-size", "3", "--report-interval=1", str(scp), str(normed), nets["ln"], d + "/ln.1")
    assert rc == 0, err
    tr = [l for l in err.split("\n") if l.startswith("INFO:tensorflow:tr_loss")]
    assert len(tr) == 1 and np.isfinite(float(tr[0].split()[-1]))
    info = [l for l in err.split("\n") if "layer normalisation" in l]
    assert len(info) == 1 and "layer_norm = true" in info[0] and "layers 0..2" in info[0] and "eps = 1e-05" in info[0], err
    ark = d + "/ln.ark"
    rc, err = _cli("nnet-forward.py", "--apply-log=true", "--batch-utts", "3", str(scp), str(normed), d + "/ln.1", "ark:" + ark)
    assert rc == 0, err
    assert len([l for l in err.split("\n") if "layer normalisation" in l]) == 1
    post = read_float_matrix_ark(ark)
    assert sorted(post) == sorted(frames)
    for k, T in frames.items():
        assert post[k].shape == (T, V) and np.isfinite(post[k]).all()
    # a plain checkpoint is refused by name, in both tools (the other way round: the graph test above)
    rc, err = _cli("nnet-forward.py", "--apply-log=true", "--batch-utts", "3", str(scp), str(normed), nets["plain"], "ark:" + d + "/no.ark")
    assert rc != 0 and "ln0/gamma" in err, err
    rc, err = _cli("nnet-train.py", "--objective=ctc", "--learn-rate=0.01", "--batch-size", "3", str(scp), str(normed),
                   nets["plain"], d + "/never")
    assert rc != 0 and "ln0/gamma" in err and not os.path.exists(d + "/never"), err
