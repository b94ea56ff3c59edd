"""Host tests of layer normalisation between the LSTM layers (nnet.config key layer_norm): the float64
reference against torch, the config rule, the parameter layout, checkpoints, and the library's entry points.  No GPU."""
import ctypes
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import layer_norm_reference as ref  # noqa: E402

TYPES = ("blstm", "lstm", "cudnnlstm")


def _cfg(nnet_type="blstm", **kw):
    cfg = dict(nnet_type=nnet_type, input_dim=10, left_context=0, right_context=0, num_layers=3, num_neurons=32,
               num_projects=16, num_targets=9, use_peepholes=True, dropout_rate=1.0)
    if nnet_type == "cudnnlstm":
        del cfg["num_projects"]
    cfg.update(kw)
    return cfg


def _width(nnet_type):
    return {"blstm": 32, "lstm": 16, "cudnnlstm": 32}[nnet_type]


# ---------------------------------------------------------------------------------------------- the reference is pinned
def _case(seed, T=6, B=4, C=7, lens=(6, 3, 0, 9)):
    rng = np.random.default_rng(seed)
    return (rng.normal(1.0, 2.0, size=(T, B, C)), rng.normal(size=(T, B, C)), rng.normal(1.0, 0.5, size=C), rng.normal(size=C),
            np.array(lens, np.int64))


@pytest.mark.parametrize("keep", [1.0, 0.7])
def test_reference_forward_is_torch_layer_norm_on_the_live_rows(keep):
    x, _, gamma, beta, lens = _case(1)
    T, B, C = x.shape
    m = ref.mask(5, 2, T, B, C, C, keep)
    y = ref.fwd(x, gamma, beta, lens, m)
    want = torch.nn.functional.layer_norm(torch.as_tensor(x), (C,), torch.as_tensor(gamma), torch.as_tensor(beta), ref.EPS).numpy()
    if m is not None:
        assert set(np.unique(m)) == {0.0, float(np.float32(1) / np.float32(keep))}
        want = want * m
    live = ref.live_rows(lens, T)
    assert live.sum() == 6 + 3 + 0 + 6                                   # 9 is clamped to T
    assert np.abs(y - want)[live].max() < 1e-13
    assert np.array_equal(y[~live], np.zeros_like(y[~live])) and not np.signbit(y[~live]).any()
    xn = x.copy()
    xn[~live] = np.nan                                                   # dead rows are never read
    assert np.array_equal(ref.fwd(xn, gamma, beta, lens, m), y)
    again = ref.torch_layer_norm(torch.as_tensor(xn), lens, torch.as_tensor(gamma), torch.as_tensor(beta), m).numpy()
    assert np.abs(again - y).max() < 1e-13 and np.array_equal(again[~live], y[~live])


@pytest.mark.parametrize("keep", [1.0, 0.7])
def test_reference_backward_is_autograd(keep):
    x, dy, gamma, beta, lens = _case(2)
    T, B, C = x.shape
    m = ref.mask(5, 2, T, B, C, C, keep)
    live = ref.live_rows(lens, T)
    xt, gt, bt = (torch.as_tensor(a).clone().requires_grad_(True) for a in (x, gamma, beta))
    out = torch.nn.functional.layer_norm(xt, (C,), gt, bt, ref.EPS)
    if m is not None:
        out = out * torch.as_tensor(m)
    (out * torch.as_tensor(np.where(live[:, :, None], dy, 0.0))).sum().backward()            # live rows only
    dyn = dy.copy()
    dyn[~live] = np.nan
    dx, dgamma, dbeta = ref.bwd(x, dyn, gamma, lens, m)
    assert np.abs(dx - xt.grad.numpy())[live].max() < 1e-12 and np.array_equal(dx[~live], np.zeros_like(dx[~live]))
    assert np.abs(dgamma - gt.grad.numpy()).max() < 1e-12 and np.abs(dbeta - bt.grad.numpy()).max() < 1e-12
    # ... and of the differentiable restatement the model compositions use
    xt, gt, bt = (torch.as_tensor(a).clone().requires_grad_(True) for a in (x, gamma, beta))
    (ref.torch_layer_norm(xt, lens, gt, bt, m) * torch.as_tensor(dy)).sum().backward()
    assert np.abs(dx - xt.grad.numpy()).max() < 1e-12 and np.abs(dgamma - gt.grad.numpy()).max() < 1e-12
    assert np.abs(dbeta - bt.grad.numpy()).max() < 1e-12


def test_reference_mask_is_one_stream_per_drop_width_columns():
    from oracle.torch_f64 import dropout_mask
    T, B, C = 3, 2, 8
    m = ref.mask(9, 4, T, B, C, 4, 0.6)
    for q in range(2):
        assert np.array_equal(m[:, :, 4 * q:4 * q + 4], dropout_mask(9, 4 + q, T, B, 4, 0.6, "cpu").numpy())
    assert ref.mask(9, 4, T, B, C, 4, 1.0) is None


def test_bounds_are_positive_and_grow_with_the_offset():
    x, dy, gamma, beta, lens = _case(3)
    near = ref.bounds(x, dy, gamma, beta, lens)
    far = ref.bounds(x + 4096.0, dy, gamma, beta, lens)
    live = ref.live_rows(lens, x.shape[0])
    for a, b in zip(near, far):
        assert (a > 0).all() and (b >= a).all()
    assert far[0][live].min() > 10 * near[0][live].max() and near[0][live].max() < 1e-4


# ---------------------------------------------------------------------------------------------- config
def test_config_rules():
    from lstm_ctc_amd.nnet.model import layer_norm_config
    for t in TYPES:
        assert layer_norm_config(_cfg(t)) is False and layer_norm_config(_cfg(t, layer_norm=False)) is False
        assert layer_norm_config(_cfg(t, layer_norm=True)) is True
        assert layer_norm_config(_cfg(t, layer_norm=False, use_bn=True)) is False              # off: nothing to refuse
    for bad in (1, 0, "true", "yes", 1.0, [True]):
        with pytest.raises(ValueError, match="layer_norm"):
            layer_norm_config(_cfg(layer_norm=bad))
    for t in TYPES:
        with pytest.raises(ValueError, match="use_bn"):
            layer_norm_config(_cfg(t, layer_norm=True, use_bn=True))


def test_config_as_parse_config_delivers_it(tmp_path):
    from lstm_ctc_amd.nnet.config import parse_config
    from lstm_ctc_amd.nnet.model import layer_norm_config
    p = tmp_path / "nnet.config"
    p.write_text("nnet_type = lstm\nnum_layers = 2\nlayer_norm = true\n")
    assert layer_norm_config(parse_config(str(p))) is True
    p.write_text("nnet_type = lstm\nnum_layers = 2\nlayer_norm = False\n")
    assert layer_norm_config(parse_config(str(p))) is False
    p.write_text("nnet_type = lstm\nnum_layers = 2\nlayer_norm = 1\n")
    with pytest.raises(ValueError, match="layer_norm"):
        layer_norm_config(parse_config(str(p)))
    p.write_text("nnet_type = lstm\nnum_layers = 2\nlayer_norm = true\nuse_bn = true\n")
    with pytest.raises(ValueError, match="use_bn"):
        layer_norm_config(parse_config(str(p)))


def test_info_line_and_report(capsys):
    from lstm_ctc_amd import ops
    from lstm_ctc_amd.nnet.model import layer_norm_info_line
    assert ops.LN_EPS == 1e-5 == ref.EPS
    assert layer_norm_info_line(_cfg()) is None and layer_norm_info_line(_cfg(layer_norm=False)) is None
    line = layer_norm_info_line(_cfg(num_layers=5, layer_norm=True))
    assert line.startswith("layer normalisation: layer_norm = true") and "layers 0..4" in line and "eps = 1e-05" in line
    spec = importlib.util.spec_from_file_location("_common_under_test", os.path.join(ROOT, "bin", "_common.py"))
    common = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(common)
    common.report_layer_norm(_cfg())
    assert "layer normalisation" not in capsys.readouterr().err
    common.report_layer_norm(_cfg("lstm", layer_norm=True))
    assert capsys.readouterr().err.count("layer normalisation: layer_norm = true") == 1
    with pytest.raises(SystemExit) as exc:
        common.report_layer_norm(_cfg("lstm", layer_norm=True, use_bn=True))
    assert exc.value.code == 1 and "use_bn" in capsys.readouterr().err
    for cli in ("nnet-train.py", "nnet-validate.py", "nnet-forward.py", "nnet-align.py"):
        assert "report_layer_norm(nnet_config)" in open(os.path.join(ROOT, "bin", cli)).read(), cli


# ---------------------------------------------------------------------------------------------- parameters
@pytest.mark.parametrize("nnet_type", TYPES)
def test_param_store_layout(nnet_type):
    from lstm_ctc_amd.nnet.model import Model, ParamStore
    plain = ParamStore(_cfg(nnet_type), "cpu")
    for off in (dict(layer_norm=False),):
        ps = ParamStore(_cfg(nnet_type, **off), "cpu")
        assert ps.names() == plain.names() and ps.offsets == plain.offsets and ps.n_decay == plain.n_decay and ps.n == plain.n
        assert ps.layer_norm is False
    ln = ParamStore(_cfg(nnet_type, layer_norm=True), "cpu")
    H = _width(nnet_type)
    new = [n for n in ln.names() if n not in plain.names()]
    assert new == [n for i in range(3) for n in ("ln%d/gamma" % i, "ln%d/beta" % i)]
    assert ln.H == H and all(ln.shapes[n] == (H,) for n in new)
    assert [ln.kinds[n] for n in new] == ["ln_gamma", "ln_beta"] * 3
    # the decayed block is the plain model's, tensor for tensor; the new ones lie behind it, behind the biases
    assert ln.n_decay == plain.n_decay
    for n in plain.names():
        assert ln.offsets[n] == plain.offsets[n], n
    assert all(ln.offsets[n] >= ln.n_decay for n in new)
    assert min(ln.offsets[n] for n in new) >= max(plain.offsets[n] for n in plain.names() if "bias" in n)
    assert ln.n == plain.n + 6 * H and ln.num_params() == plain.num_params() + 6 * H
    # no layer's gradient range (the data-parallel buckets) contains them, and the ranges are the plain model's
    shell = Model.__new__(Model)
    for ps in (plain, ln):
        shell.ps = ps
        ranges = [Model.layer_grad_range(shell, i) for i in range(3)]
        if ps is plain:
            want = ranges
        assert ranges == want
        for lo, hi in ranges:
            assert hi <= ps.n_decay
            assert not any(lo <= ln.offsets[n] < hi for n in new)


@pytest.mark.parametrize("nnet_type", TYPES)
def test_same_seed_gives_the_plain_models_other_tensors(nnet_type):
    """What nnet-init writes: gamma ones, beta zeros, nothing drawn for them."""
    from lstm_ctc_amd.nnet.model import ParamStore
    plain, ln = ParamStore(_cfg(nnet_type), "cpu"), ParamStore(_cfg(nnet_type, layer_norm=True), "cpu")
    plain.init_random(4)
    ln.init_random(4)
    a, b = plain.export_tf(), ln.export_tf()
    assert set(b) - set(a) == {"ln%d/%s" % (i, w) for i in range(3) for w in ("gamma", "beta")}
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    for i in range(3):
        assert np.array_equal(b["ln%d/gamma" % i], np.ones(_width(nnet_type), np.float32))
        assert np.array_equal(b["ln%d/beta" % i], np.zeros(_width(nnet_type), np.float32))
    assert torch.equal(plain.flat[:plain.n_decay], ln.flat[:ln.n_decay])


def test_load_tf_refuses_both_ways_and_round_trips():
    from lstm_ctc_amd.nnet.model import ParamStore
    plain, ln = ParamStore(_cfg(), "cpu"), ParamStore(_cfg(layer_norm=True), "cpu")
    plain.init_random(4)
    ln.init_random(5)
    with pytest.raises(KeyError, match="ln0/gamma.*layer_norm = true"):
        ln.load_tf(plain.export_tf())
    with pytest.raises(KeyError, match="ln0/gamma.*layer_norm"):
        plain.load_tf(ln.export_tf())
    ck = ln.export_tf()
    rng = np.random.default_rng(0)
    for i in range(3):
        ck["ln%d/gamma" % i] = rng.normal(1, 0.1, size=32).astype(np.float32)
        ck["ln%d/beta" % i] = rng.normal(0, 0.1, size=32).astype(np.float32)
    again = ParamStore(_cfg(layer_norm=True), "cpu")
    again.load_tf(ck)
    back = again.export_tf()
    assert set(back) == set(ck) and all(np.array_equal(back[k], ck[k]) for k in ck)
    bad = dict(ck)
    bad["ln1/beta"] = np.zeros(16, np.float32)
    with pytest.raises(ValueError, match="ln1/beta"):
        again.load_tf(bad)


# ---------------------------------------------------------------------------------------------- the library
def test_library_exports_the_entry_points_and_refuses_bad_arguments():
    """The header's three symbols are in the built library and in the binding, lc_version() says 14; LC_EINVAL comes before
    any launch, so every rejection can be seen without a GPU (the pointers are never dereferenced)."""
    import __graft_entry__ as g
    g.build()
    from lstm_ctc_amd import _lib
    header = " ".join(open(os.path.join(ROOT, "include", "lstm_ctc_hip.h")).read().split())
    assert "size_t lc_layer_norm_workspace_bytes(int T, int B, int C);" in header
    assert ("int lc_layer_norm_fwd(const float *x, int ldx, const float *gamma, const float *beta, int T, int B, int C, float "
            "eps, const int *seq_len, float keep, uint32_t seed, uint32_t stream0, int drop_width, float *y, int ldy, "
            "lc_stream_t stream);") in header
    assert ("int lc_layer_norm_bwd(const float *x, int ldx, const float *dy, int lddy, const float *gamma, int T, int B, int C, "
            "float eps, const int *seq_len, float keep, uint32_t seed, uint32_t stream0, int drop_width, float *dx /* or NULL "
            "*/, int lddx, float *dgamma, float *dbeta /* both or neither; overwritten */, void *workspace, size_t "
            "workspace_bytes, lc_stream_t stream);") in header
    names = ("lc_layer_norm_workspace_bytes", "lc_layer_norm_fwd", "lc_layer_norm_bwd")
    assert [len(_lib.SIGNATURES[n][1]) for n in names] == [3, 16, 21]
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(raw, n) for n in names)
    lib = _lib.load()
    assert lib.lc_version() >= 14
    T, B, C = 5, 3, 8
    X, Y, DY, DX, G, Bt, L, DG, DB, W = (0x100000 * k for k in range(1, 11))      # far apart, 16-byte aligned made-up addresses
    ws = lib.lc_layer_norm_workspace_bytes(T, B, C)
    assert ws >= 2 * C * 4 and ws % 256 == 0
    assert lib.lc_layer_norm_workspace_bytes(T, B, 8192) > 0
    for bad in ((0, B, C), (T, 0, C), (T, B, 0), (T, B, 8196), (T, B, -1)):
        assert lib.lc_layer_norm_workspace_bytes(*bad) == 0

    def fwd(x=X, ldx=C, gamma=G, beta=Bt, T=T, B=B, C=C, eps=1e-5, seq_len=L, keep=1.0, dw=C, y=Y, ldy=C):
        return lib.lc_layer_norm_fwd(x, ldx, gamma, beta, T, B, C, eps, seq_len, keep, 1, 0, dw, y, ldy, None)

    def bwd(x=X, ldx=C, dy=DY, lddy=C, gamma=G, T=T, B=B, C=C, eps=1e-5, seq_len=L, keep=1.0, dw=C, dx=DX, lddx=C, dgamma=DG,
            dbeta=DB, w=W, wb=ws):
        return lib.lc_layer_norm_bwd(x, ldx, dy, lddy, gamma, T, B, C, eps, seq_len, keep, 1, 0, dw, dx, lddx, dgamma, dbeta, w,
                                     wb, None)

    nbytes = 4 * T * B * C
    for kw in (dict(T=0), dict(B=0), dict(C=0), dict(T=-1), dict(C=8196, ldx=8196, ldy=8196, dw=8196), dict(x=None),
               dict(gamma=None), dict(beta=None), dict(seq_len=None), dict(y=None), dict(ldx=C - 1), dict(ldy=C - 1),
               dict(eps=0.0), dict(keep=0.0), dict(keep=1.5), dict(dw=0), dict(dw=3), dict(dw=16), dict(keep=0.5, dw=5),
               dict(y=X), dict(y=X + nbytes - 4), dict(y=X - nbytes + 4)):
        assert fwd(**kw) == -1, kw
        assert b"lc_layer_norm_fwd" in lib.lc_last_error()
    for kw in (dict(T=0), dict(B=0), dict(C=0), dict(C=8196, ldx=8196, lddy=8196, lddx=8196, dw=8196), dict(x=None),
               dict(dy=None), dict(gamma=None), dict(seq_len=None), dict(ldx=C - 1), dict(lddy=C - 1), dict(lddx=C - 1),
               dict(eps=-1.0), dict(keep=0.0), dict(dw=3), dict(dgamma=None), dict(dbeta=None),
               dict(dx=None, dgamma=None, dbeta=None), dict(wb=ws - 1), dict(w=None), dict(dx=X), dict(dx=X + nbytes - 4),
               dict(dx=DY + 4 * C), dict(dx=DY - 4), dict(dx=DY, lddx=C + 4), dict(dx=DY, lddy=C + 4)):
        assert bwd(**kw) == -1, kw
        assert b"lc_layer_norm_bwd" in lib.lc_last_error()
