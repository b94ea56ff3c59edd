"""GPU tests of the latency-controlled BiLSTM (nnet.config keys chunk_frames / lookahead_frames), model level.

Sizes and tolerances are tests/test_gpu_model.py's: 2 layers, N = 32, P = 16, D = 10, V = 9, peepholes, non-zero biases; logits
within 1e-4 of the logit scale, gradients through conftest.check_grad.

1. lookahead >= T - chunk: every window reaches the end of its utterance, the mode equals the plain model up to summation order
   - the fp64 C oracle of the plain model is the reference (holds the gradient fold and the chunk-layout dR, no new yardstick);
2. true truncation against tests/lc_blstm_reference.py (float64, pinned to oracle/torch_f64.py by tests/test_lc_blstm_host.py);
3. causality, bit for bit: chunk c's logits do not move when input frames >= H_L(c) change, and do when frame H_L(c) - 1 does;
4. refusals, and chunk_frames = 0 being the plain model to the bit;
5. nnet-train / nnet-forward end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from lc_blstm_reference import horizon, lc_blstm_gradients  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(**kw):
    cfg = dict(nnet_type="blstm", input_dim=10, left_context=0, right_context=0, num_layers=2,
               num_neurons=32, num_projects=16, num_targets=9, use_peepholes=True, dropout_rate=1.0)
    cfg.update(kw)
    return cfg


def _data(rng, cfg, B, T):
    """tests/test_gpu_model.py's lengths: T first, 1 last, the rest between T // 2 and T."""
    D = cfg["input_dim"]
    seq_len = np.sort(rng.integers(max(1, T // 2), T + 1, size=B))[::-1].astype(np.int32).copy()
    seq_len[0] = T
    if B > 2:
        seq_len[-1] = 1
    return _inputs(rng, D, B, T, seq_len), seq_len


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


def _dlogits(rng, shape, seq_len):
    dl = rng.normal(size=shape)                                 # batch-major [B,T,V]
    for b in range(shape[0]):
        dl[b, seq_len[b]:] = 0                                  # no loss sends gradient into padded frames
    return dl


def _check_logits(got, ref):
    scale = np.abs(ref).max()
    err = np.abs(got - ref)
    print("logits: max error %.3e, scale %.3e" % (err.max(), scale))
    assert err.max() < 1e-4 * max(scale, 1.0), err.max()
    assert np.all(err <= 1e-4 * np.maximum(np.abs(ref), 0.1 * max(scale, 1.0)))


# ---------------------------------------------------------------------------------------------- 1. full context = plain model
FULL = {   # name -> (B, T, Nc, Nr, config overrides, launch train)
    "b5": (5, 11, 4, 11, {}, False),
    "b70": (70, 6, 2, 6, {}, False),                             # Bc = 210: past the 64- and 128-row schedule limits
    "launch_train": (5, 11, 4, 11, {}, True),
    "dropout": (5, 11, 4, 11, dict(dropout_rate=0.8), False),
    "pack_frames": (5, 11, 4, 11, dict(pack_frames=True), False),
}


@pytest.mark.parametrize("case", sorted(FULL))
def test_full_lookahead_equals_the_plain_oracle(oracle, case):
    import contextlib
    from conftest import check_grad
    from lstm_ctc_amd import ops
    B, T, Nc, Nr, extra, train = FULL[case]
    plain = _cfg(**{k: v for k, v in extra.items() if k != "pack_frames"})
    cfg = dict(plain, chunk_frames=Nc, lookahead_frames=Nr, **{k: v for k, v in extra.items() if k == "pack_frames"})
    rng = np.random.default_rng(sorted(FULL).index(case) + 40)
    x, seq_len = _data(rng, cfg, B, T)
    model, p64 = _model(cfg, rng)
    assert (model.chunk, model.lookahead) == (Nc, Nr)
    ref_logits, saved = oracle.forward(p64, plain, x.astype(np.float64), seq_len, drop_seed=7)
    dl = _dlogits(rng, ref_logits.shape, seq_len)
    ref_grads, _ = oracle.backward(p64, plain, saved, dl)
    with (ops.force_launch_train() if train else contextlib.nullcontext()):
        logits = model.forward(_tm(x), torch.from_numpy(seq_len).cuda(), drop_seed=7)
        got = logits.cpu().numpy().transpose(1, 0, 2)
        model.backward(_tm(dl))
        if train:
            assert ops.last_lstm_schedule()["kind"] in ("launch_train", "two_stream_train")
    if "pack_frames" in extra:
        assert model.packed is True
    _check_logits(got, ref_logits)
    grads = model.ps.export_tf(grads=True)
    assert set(grads) == set(ref_grads), set(grads) ^ set(ref_grads)
    for k in sorted(ref_grads):
        check_grad(grads[k], ref_grads[k], "lc_blstm_full/" + case, k)


# ---------------------------------------------------------------------------------------------- 2. true truncation
@pytest.mark.parametrize("drop", [1.0, 0.8], ids=["nodrop", "dropout"])
def test_truncated_lookahead_against_the_float64_restatement(drop):
    """Nc = 4, Nr = 2 at T = 11; lengths 11 (ragged last chunk), 8 (a multiple of Nc), 6, 4 (exactly Nc) and 1 (chunks of
    length 0)."""
    from conftest import check_grad
    B, T, Nc, Nr = 5, 11, 4, 2
    cfg = _cfg(chunk_frames=Nc, lookahead_frames=Nr, dropout_rate=drop)
    rng = np.random.default_rng(50)
    seq_len = np.array([11, 8, 6, 4, 1], np.int32)
    x = _inputs(rng, cfg["input_dim"], B, T, seq_len)
    model, p64 = _model(cfg, rng)
    dl = _dlogits(rng, (B, T, cfg["num_targets"]), seq_len)
    ref_logits, ref_grads = lc_blstm_gradients(p64, cfg, x.transpose(1, 0, 2).astype(np.float64), seq_len,
                                               dl.transpose(1, 0, 2), Nc, Nr, drop_seed=7)
    ref_logits = ref_logits.numpy()
    sl = torch.from_numpy(seq_len).cuda()
    got = model.forward(_tm(x), sl, drop_seed=7).cpu().numpy()
    model.backward(_tm(dl))
    _check_logits(got, ref_logits)
    grads = model.ps.export_tf(grads=True)
    assert set(grads) == set(ref_grads), set(grads) ^ set(ref_grads)
    for k in sorted(ref_grads):
        check_grad(grads[k], ref_grads[k], "lc_blstm_truncated/%g" % drop, k)
    # ... and it is not the plain model: the same parameters without the keys give other logits
    from lstm_ctc_amd.nnet.model import Model
    plain = Model(_cfg(dropout_rate=drop), "cuda", seed=3)
    plain.ps.flat.copy_(model.ps.flat)
    other = plain.forward(_tm(x), sl, drop_seed=7).cpu().numpy()
    assert np.abs(other - got).max() > 1e-3 * max(np.abs(got).max(), 1.0)


# ---------------------------------------------------------------------------------------------- 3. causality
def test_logits_of_a_chunk_stop_reading_at_the_horizon():
    L, Nc, Nr, T, B = 2, 4, 2, 23, 3
    cfg = _cfg(chunk_frames=Nc, lookahead_frames=Nr, is_training=False)
    rng = np.random.default_rng(60)
    model, _ = _model(cfg, rng)
    assert model.lookahead_horizon() == 6
    assert horizon(1, Nc, Nr, 0, T) == 6 and horizon(L, Nc, Nr, 0, T) == 10 and horizon(L, Nc, Nr, 2, T) == 18
    sl = torch.full((B,), T, dtype=torch.int32, device="cuda")
    x = rng.normal(size=(T, B, cfg["input_dim"])).astype(np.float32)
    base = model.forward(torch.from_numpy(x).cuda(), sl).clone()
    for c in (0, 2):
        H = horizon(L, Nc, Nr, c, T)
        assert H - (c + 1) * Nc == model.lookahead_horizon()
        y = x.copy()
        y[H:] = rng.normal(size=y[H:].shape)                    # everything at or beyond the horizon: not read
        got = model.forward(torch.from_numpy(y).cuda(), sl)
        assert torch.equal(got[c * Nc:(c + 1) * Nc], base[c * Nc:(c + 1) * Nc]), c
        assert not torch.equal(got[T - 1], base[T - 1])
        y = x.copy()
        y[H - 1] = rng.normal(size=y[H - 1].shape)              # the last frame inside it: read - the bound is tight
        got = model.forward(torch.from_numpy(y).cuda(), sl)
        assert not torch.equal(got[c * Nc:(c + 1) * Nc], base[c * Nc:(c + 1) * Nc]), c


# ---------------------------------------------------------------------------------------------- 4. refusals, chunk_frames = 0
@pytest.mark.parametrize("bad", [dict(compute_dtype="bf16"), dict(compute_dtype="bf16x3"), dict(nnet_type="lstm")],
                         ids=["bf16", "bf16x3", "lstm"])
def test_keys_are_refused_where_they_cannot_run(bad):
    from lstm_ctc_amd.nnet.model import Model
    with pytest.raises(ValueError, match="chunk_frames"):
        Model(_cfg(chunk_frames=4, lookahead_frames=2, **bad), "cuda", seed=3)
    Model(_cfg(chunk_frames=0, lookahead_frames=2, **bad), "cuda", seed=3)          # chunk_frames = 0: the keys are off


def test_encoder_is_refused_and_chunk_frames_0_is_the_plain_model():
    from lstm_ctc_amd import ops
    from lstm_ctc_amd.nnet.model import Model
    rng = np.random.default_rng(70)
    B, T = 5, 11
    cfg = _cfg(dropout_rate=0.8)
    x, seq_len = _data(rng, cfg, B, T)
    dl = _tm(_dlogits(rng, (B, T, cfg["num_targets"]), seq_len))
    xt, sl = _tm(x), torch.from_numpy(seq_len).cuda()
    res = []
    for extra in ({}, dict(chunk_frames=0), dict(chunk_frames=0, lookahead_frames=3)):
        m = Model(dict(cfg, **extra), "cuda", seed=3)
        assert m.chunk == 0 and m.lookahead_horizon() is None
        logits = m.forward(xt, sl, drop_seed=7).clone()
        fwd = ops.last_lstm_schedule()
        enc = m.encoder()
        m.backward(dl)
        res.append((logits, m.ps.grad.clone(), enc, fwd, ops.last_lstm_schedule()))
    for r in res[1:]:
        assert torch.equal(r[0], res[0][0]) and torch.equal(r[1], res[0][1]) and torch.equal(r[2], res[0][2])
        assert r[3] == res[0][3] and r[4] == res[0][4]
    m = Model(dict(cfg, chunk_frames=4, lookahead_frames=2), "cuda", seed=3)
    assert torch.equal(m.ps.flat, Model(cfg, "cuda", seed=3).ps.flat)                # same parameters, same layout
    m.forward(xt, sl, drop_seed=7)
    with pytest.raises(NotImplementedError, match="chunk_frames"):
        m.encoder()
    m.backward(dl)


# ---------------------------------------------------------------------------------------------- 5. command lines
def _run(cli, *args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", cli)] + list(args), capture_output=True, timeout=600)
    return r.returncode, r.stderr.decode()


def test_cli_trains_chunked_and_forwards_with_and_without_the_keys(tmp_path):
    from lstm_ctc_amd.kaldi_io import read_float_matrix_ark
    from lstm_ctc_amd.nnet import write_tfrecord
    rng = np.random.default_rng(8)
    D, V = 6, 9
    lines = []
    for i in range(8):
        T = int(rng.integers(24, 41))
        path = str(tmp_path / ("utt%03d.tfrecords" % i))
        write_tfrecord(path, rng.normal(size=(T, D)).astype(np.float32), rng.integers(0, V - 1, size=int(rng.integers(1, 5))))
        lines.append((T, "utt%03d %d %d 1 %s" % (i, T, D, path)))
    scp = tmp_path / "tfrecords.scp"
    scp.write_text("\n".join(l[1] for l in sorted(lines)) + "\n")
    text = ("nnet_type = blstm\ninput_dim = 6\nleft_context = 1\nright_context = 1\nsubsample = 2\nnum_layers = 2\n"
            "num_neurons = 32\nnum_projects = 16\nnum_targets = 9\nuse_peepholes = true\ndropout_rate = 0.9\n")
    plain, chunked = tmp_path / "plain.config", tmp_path / "chunked.config"
    plain.write_text(text)
    chunked.write_text(text + "chunk_frames = 8\nlookahead_frames = 4\n")
    d = str(tmp_path)
    rc, err = _run("nnet-init.py", "--objective=ctc", "--batch-size", "3", str(scp), str(plain), d + "/nnet.0")
    assert rc == 0, err
    rc, err = _run("nnet-train.py", "--objective=ctc", "--delay-penalty", "0.01", "--learn-rate=0.01", "--optimizer=adam",
                   "--seed=1", "--shuffle=false", "--batch-size", "3", "--report-interval=1", str(scp), str(chunked),
                   d + "/nnet.0", d + "/nnet.1")
    assert rc == 0, err
    assert any(l.startswith("INFO:tensorflow:step = 3, ") for l in err.split("\n")), err          # 8 utterances by 3: 3 steps
    tr = [l for l in err.split("\n") if l.startswith("INFO:tensorflow:tr_loss")]
    assert len(tr) == 1 and np.isfinite(float(tr[0].split()[-1]))
    info = [l for l in err.split("\n") if "latency-controlled" in l]
    # H_2(0) = ((8 + 4 - 1) // 8 + 1) * 8 + 4 = 20: 12 model frames past the chunk, 12 * 2 + 1 raw frames
    assert len(info) == 1 and "chunk_frames = 8, lookahead_frames = 4, 2 layers" in info[0], err
    assert "12 model frames (25 raw frames)" in info[0], info
    assert os.path.exists(d + "/nnet.1")
    post = {}
    for name, config in (("plain", plain), ("chunked", chunked)):
        ark = d + "/%s.ark" % name
        rc, err = _run("nnet-forward.py", "--apply-log=true", "--batch-utts", "3", str(scp), str(config), d + "/nnet.1",
                       "ark:" + ark)
        assert rc == 0, err
        assert len([l for l in err.split("\n") if "latency-controlled" in l]) == (1 if name == "chunked" else 0)
        post[name] = read_float_matrix_ark(ark)
    assert sorted(post["plain"]) == sorted(post["chunked"]) == ["utt%03d" % i for i in range(8)]
    diff = 0.0
    for k in post["plain"]:
        assert post["plain"][k].shape == post["chunked"][k].shape
        assert np.isfinite(post["plain"][k]).all() and np.isfinite(post["chunked"][k]).all()
        diff = max(diff, float(np.abs(post["plain"][k] - post["chunked"][k]).max()))
    assert diff > 1e-3, diff                                     # the same checkpoint, another model
