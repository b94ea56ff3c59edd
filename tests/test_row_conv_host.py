"""Host tests of the row convolution: the float64 reference the GPU tests use against torch autograd, the
config key's rules, the parameter's place in the store and in checkpoints, the INFO line's arithmetic, and the library's entry
points and their argument checks.  None needs a GPU."""
import ctypes
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import row_conv_reference as ref  # noqa: E402


def _cfg(**kw):
    cfg = dict(nnet_type="lstm", input_dim=10, left_context=0, right_context=0, num_layers=2, num_neurons=16,
               num_targets=5, dropout_rate=1.0)
    cfg.update(kw)
    return cfg


# ---------------------------------------------------------------------------------------------- the reference itself
def _torch_row_conv(x, w, seq_len):
    """A masked unfold-and-sum: x [T, B, C] (requires grad), w [tau + 1, C] -> y, dead frames masked on both sides."""
    T, B, C = x.shape
    live = (torch.arange(T).reshape(T, 1) < seq_len.clamp(0, T).reshape(1, B)).reshape(T, B, 1)
    xm = torch.where(live, x, torch.zeros_like(x))                       # a dead frame contributes nothing, whatever it holds
    pad = torch.cat([xm, torch.zeros((w.shape[0] - 1, B, C), dtype=x.dtype)], dim=0)
    win = pad.unfold(0, w.shape[0], 1)                                  # [T, B, C, tau + 1]: win[t, b, c, j] = x[t + j, b, c]
    y = (win * w.t().reshape(1, 1, C, -1)).sum(dim=3)
    return torch.where(live, y, torch.zeros_like(y))


@pytest.mark.parametrize("T,B,C,tau,lens", [
    (9, 6, 5, 2, [9, 0, 1, 2, 3, 14]),             # 0, 1, tau, tau + 1, T and one above T (clips)
    (7, 3, 4, 0, [7, 3, 0]),
    (3, 4, 3, 8, [3, 2, 1, 0]),                    # every length below tau + 1
    (12, 2, 2, 32, [12, 5]),
])
def test_reference_equals_torch_autograd(T, B, C, tau, lens):
    rng = np.random.default_rng(T * 7 + tau)
    x, dy, w = rng.normal(size=(T, B, C)), rng.normal(size=(T, B, C)), rng.normal(size=(tau + 1, C))
    n = ref.lengths(lens, T)
    xn, dyn = x.copy(), dy.copy()
    for b in range(B):                             # the reference never reads a dead frame
        xn[n[b]:, b] = np.nan
        dyn[n[b]:, b] = np.nan
    xt = torch.tensor(x, requires_grad=True)
    wt = torch.tensor(w, requires_grad=True)
    y = _torch_row_conv(xt, wt, torch.tensor(lens))
    live = (np.arange(T)[:, None] < n[None, :])[:, :, None]
    (y * torch.tensor(np.where(live, dy, 0.0))).sum().backward()
    got_y, got_dx, got_dw = ref.fwd(xn, w, lens), ref.dx(dyn, w, lens), ref.dw(xn, dyn, tau, lens)
    assert not np.isnan(got_y).any() and not np.isnan(got_dx).any() and not np.isnan(got_dw).any()
    assert np.abs(got_y - y.detach().numpy()).max() < 1e-12
    assert np.abs(got_dx - xt.grad.numpy()).max() < 1e-12
    assert np.abs(got_dw - wt.grad.numpy()).max() < 1e-12
    assert not got_y[~np.broadcast_to(live, got_y.shape)].any() and not got_dx[~np.broadcast_to(live, got_dx.shape)].any()
    # the bounds' ingredients: magnitudes dominate the sums, counts are the numbers of live pairs
    assert (ref.fwd(xn, w, lens, abs_terms=True) >= np.abs(got_y)).all()
    assert (ref.dw(xn, dyn, tau, lens, abs_terms=True) >= np.abs(got_dw) - 1e-12).all()
    assert ref.counts(tau, lens, T).tolist() == [int(sum(max(k - j, 0) for k in n)) for j in range(tau + 1)]


# ---------------------------------------------------------------------------------------------- the config key
def test_row_conv_config_accepts_and_refuses():
    from lstm_ctc_amd.nnet.model import row_conv_config
    assert row_conv_config(_cfg()) == 0 and row_conv_config(_cfg(row_conv_frames=0)) == 0
    assert row_conv_config(_cfg(row_conv_frames=None)) == 0
    assert row_conv_config(_cfg(nnet_type="blstm")) == 0 and row_conv_config(_cfg(nnet_type="blstm", row_conv_frames=0)) == 0
    for v in (1, 4, 32, np.int32(3), np.int64(32)):
        for nt in ("lstm", "cudnnlstm"):
            got = row_conv_config(_cfg(nnet_type=nt, row_conv_frames=v))
            assert got == int(v) and type(got) is int
    for cd in ("fp32", "bf16", "bf16x3"):
        assert row_conv_config(_cfg(row_conv_frames=2, compute_dtype=cd)) == 2
    assert row_conv_config(_cfg(row_conv_frames=2, use_bn=True, pack_frames=True)) == 2
    for v in (True, False, -1, 33, 1000, 2.0, 1.5, "4", [4]):
        with pytest.raises(ValueError, match="row_conv_frames"):
            row_conv_config(_cfg(row_conv_frames=v))
    with pytest.raises(ValueError, match="blstm"):
        row_conv_config(_cfg(nnet_type="blstm", row_conv_frames=4))
    cfg = _cfg(row_conv_frames=4)
    del cfg["nnet_type"]                           # the default nnet_type is blstm
    with pytest.raises(ValueError, match="blstm"):
        row_conv_config(cfg)


# ---------------------------------------------------------------------------------------------- the parameter
def _store(cfg, seed=3):
    from lstm_ctc_amd.nnet.model import ParamStore
    ps = ParamStore(cfg, torch.device("cpu"))
    ps.init_random(seed)
    return ps


@pytest.mark.parametrize("kw", [dict(), dict(use_bn=True), dict(nnet_type="cudnnlstm"), dict(num_projects=8)],
                         ids=["lstm", "bn", "cudnn", "proj"])
def test_param_store_places_and_initialises_the_kernel(kw):
    tau = 3
    plain, conv = _store(_cfg(**kw)), _store(_cfg(row_conv_frames=tau, **kw))
    H = conv.H
    assert conv.row_conv == tau and plain.row_conv == 0
    assert "row_conv/kernel" not in plain.names()
    assert conv.shapes["row_conv/kernel"] == (tau + 1, H) and conv.kinds["row_conv/kernel"] == "row_conv"
    assert conv.offsets["row_conv/kernel"] % 4 == 0                     # floats: 16-byte aligned
    names = conv.names()
    k = names.index("row_conv/kernel")
    assert names[k + 1] == "Variable"                                   # behind the layers' and batch-norm tensors
    assert [n for n in names if n != "row_conv/kernel"] == plain.names()
    assert all(conv.offsets[n] == plain.offsets[n] for n in names[:k])  # nothing below it moved
    assert conv.offsets["row_conv/kernel"] < conv.n_decay               # L2-decayed: no "bias" in the name
    w = conv.p("row_conv/kernel").numpy()
    assert np.array_equal(w[0], np.ones(H, np.float32)) and not w[1:].any()
    for n in plain.names():                                             # nothing drawn for it: same seed, same model
        assert torch.equal(conv.p(n), plain.p(n)), n
    assert conv.num_params() == plain.num_params() + (tau + 1) * H


def test_checkpoint_round_trip_and_plain_checkpoint():
    from lstm_ctc_amd.nnet import tflog
    conv = _store(_cfg(row_conv_frames=2), seed=5)
    rng = np.random.default_rng(0)
    conv.p("row_conv/kernel").copy_(torch.from_numpy(rng.normal(size=(3, conv.H)).astype(np.float32)))
    saved = conv.export_tf()
    assert saved["row_conv/kernel"].shape == (3, conv.H)
    assert np.array_equal(saved["row_conv/kernel"], conv.p("row_conv/kernel").numpy())       # TF layout = internal layout
    other = _store(_cfg(row_conv_frames=2), seed=6)
    other.load_tf(saved)
    assert torch.equal(other.flat, conv.flat)
    # a plain model's checkpoint: everything it has, and the identity for the filter, with one INFO line
    plain = _store(_cfg(), seed=9)
    lines = []
    orig = tflog.info
    tflog.info = lambda msg, *a: lines.append(msg % a if a else msg)
    try:
        other.load_tf(plain.export_tf())
    finally:
        tflog.info = orig
    assert len(lines) == 1 and "row_conv/kernel" in lines[0] and "identity" in lines[0], lines
    w = other.p("row_conv/kernel").numpy()
    assert np.array_equal(w[0], np.ones(conv.H, np.float32)) and not w[1:].any()
    for n in plain.names():
        assert torch.equal(other.p(n), plain.p(n)), n
    # anything else missing is still an error, with or without the filter; a wrong shape too
    lacking = plain.export_tf()
    del lacking["Variable_1"]
    with pytest.raises(KeyError, match="Variable_1"):
        other.load_tf(lacking)
    lacking = dict(saved)
    del lacking["Variable"]
    with pytest.raises(KeyError, match="Variable"):
        other.load_tf(lacking)
    wrong = dict(saved)
    wrong["row_conv/kernel"] = np.zeros((4, conv.H), np.float32)
    with pytest.raises(ValueError, match="row_conv/kernel"):
        other.load_tf(wrong)
    with pytest.raises(KeyError):                  # a plain model does not take the identity route
        lacking = plain.export_tf()
        del lacking["Variable"]
        plain.load_tf(lacking)


# ---------------------------------------------------------------------------------------------- the INFO line
def test_info_line_counts_raw_frames(capsys):
    from lstm_ctc_amd.nnet.model import row_conv_horizon_raw, row_conv_info_line
    cfg = _cfg(row_conv_frames=4, subsample=3, right_context=1, left_context=2)
    assert row_conv_horizon_raw(cfg) == (4, 4 * 3 + 1)
    assert row_conv_horizon_raw(_cfg(row_conv_frames=5)) == (5, 5)                # no subsample key: factor 1
    assert row_conv_horizon_raw(_cfg(row_conv_frames=5, subsample=0, right_context=2)) == (5, 7)
    assert row_conv_info_line(_cfg()) is None and row_conv_info_line(_cfg(row_conv_frames=0)) is None
    assert row_conv_info_line(cfg) == ("row convolution: row_conv_frames = 4: logits read 4 model frames (13 raw frames) past "
                                       "their own")
    spec = importlib.util.spec_from_file_location("_common_for_row_conv_test", os.path.join(ROOT, "bin", "_common.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.report_row_conv(_cfg())
    assert "row convolution" not in capsys.readouterr().err
    mod.report_row_conv(cfg)
    lines = [l for l in capsys.readouterr().err.splitlines() if "row convolution" in l]
    assert len(lines) == 1 and lines[0].startswith("INFO:tensorflow:"), lines
    assert "row_conv_frames = 4" in lines[0] and "4 model frames" in lines[0] and "13 raw frames" in lines[0]
    with pytest.raises(SystemExit):
        mod.report_row_conv(_cfg(row_conv_frames=4, nnet_type="blstm"))
    assert "FATAL:tensorflow:" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        mod.report_row_conv(_cfg(row_conv_frames=33))
    assert "FATAL:tensorflow:" in capsys.readouterr().err
    for tool in ("nnet-train.py", "nnet-validate.py", "nnet-forward.py", "nnet-align.py"):
        assert "report_row_conv(nnet_config)" in open(os.path.join(ROOT, "bin", tool)).read(), tool


# ---------------------------------------------------------------------------------------------- the library
def test_library_exports_the_entry_points_and_refuses_bad_arguments():
    """The header's three symbols are in the built library and in the binding; LC_EINVAL and LC_EWORKSPACE come before any
    launch, so every rejection can be seen without a GPU (the pointers are never dereferenced)."""
    import __graft_entry__ as g
    g.build()
    from lstm_ctc_amd import _lib
    header = " ".join(open(os.path.join(ROOT, "include", "lstm_ctc_hip.h")).read().split())
    assert "size_t lc_row_conv_workspace_bytes(int T, int B, int C, int tau);" in header
    assert ("int lc_row_conv_fwd(const float *x, int ldx, const float *w, int T, int B, int C, int tau, const int *seq_len, "
            "float *y, int ldy, lc_stream_t stream);") in header
    assert ("int lc_row_conv_bwd(const float *x, int ldx, const float *dy, int lddy, const float *w, int T, int B, int C, "
            "int tau, const int *seq_len, float *dx") in header
    assert "no reference counterpart" in header.split("row convolution")[1][:400]
    assert [len(_lib.SIGNATURES[n][1]) for n in ("lc_row_conv_workspace_bytes", "lc_row_conv_fwd", "lc_row_conv_bwd")] == [4, 11, 16]
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(raw, n) for n in ("lc_row_conv_workspace_bytes", "lc_row_conv_fwd", "lc_row_conv_bwd"))
    lib = _lib.load()
    assert lib.lc_version() >= 12
    T, B, C, tau = 6, 2, 8, 2
    need = lib.lc_row_conv_workspace_bytes(T, B, C, tau)
    assert need >= (tau + 1) * C * 4 and need % 256 == 0
    assert lib.lc_row_conv_workspace_bytes(1000, 64, 1024, 32) >= 33 * 1024 * 4
    for bad in ((0, B, C, tau), (T, 0, C, tau), (T, B, 0, tau), (T, B, C, -1), (T, B, C, 33)):
        assert lib.lc_row_conv_workspace_bytes(*bad) == 0, bad
    # far apart, 16-byte aligned made-up addresses
    X, Y, W, L, DY, DX, DW, WS = (0x100000 * k for k in range(1, 9))

    def fwd(x=X, ldx=C, w=W, T=T, B=B, C=C, tau=tau, seq_len=L, y=Y, ldy=C):
        return lib.lc_row_conv_fwd(x, ldx, w, T, B, C, tau, seq_len, y, ldy, None)

    def bwd(x=X, ldx=C, dy=DY, lddy=C, w=W, T=T, B=B, C=C, tau=tau, seq_len=L, dx=DX, lddx=C, dw=DW, ws=WS, nbytes=need):
        return lib.lc_row_conv_bwd(x, ldx, dy, lddy, w, T, B, C, tau, seq_len, dx, lddx, dw, ws, nbytes, None)

    for kw in (dict(T=0), dict(B=0), dict(C=0), dict(T=-3), dict(tau=-1), dict(tau=33), dict(x=None), dict(w=None),
               dict(seq_len=None), dict(y=None), dict(ldx=7), dict(ldy=7), dict(y=X), dict(y=X + 4 * C), dict(y=X - 4 * C),
               dict(ldx=2 * C, ldy=2 * C, y=X + 4 * (C - 1))):
        assert fwd(**kw) == -1, kw
        assert b"lc_row_conv_fwd" in lib.lc_last_error()
    for kw in (dict(T=0), dict(B=0), dict(C=0), dict(tau=-1), dict(tau=33), dict(dy=None), dict(w=None), dict(seq_len=None),
               dict(x=None), dict(dx=None, dw=None), dict(ldx=7), dict(lddy=7), dict(lddx=7), dict(dx=DY),
               dict(dx=DY + 4 * C * (T * B - 1)), dict(lddy=2 * C, lddx=2 * C, dx=DY + 4 * (C + 1))):
        assert bwd(**kw) == -1, kw
        assert b"lc_row_conv_bwd" in lib.lc_last_error()
    for kw in (dict(ws=None), dict(nbytes=need - 1), dict(nbytes=0), dict(dx=None, nbytes=need - 1)):
        assert bwd(**kw) == -3, kw                 # LC_EWORKSPACE
        assert b"workspace" in lib.lc_last_error()
