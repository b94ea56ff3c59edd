"""Host-side tests of the convolutional front-end (lc_conv_fwd / lc_conv_bwd, nnet.config keys conv_layers / conv_channels /
conv_bins): the float64 reference pinned to torch, the config rules and every refusal text, the parameter
layout, the checkpoint refusals and the library's argument checks.  No GPU."""
import ctypes
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import conv_reference as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES = ("blstm", "lstm", "cudnnlstm")


def _cfg(nnet_type="blstm", **kw):
    cfg = dict(nnet_type=nnet_type, input_dim=120, left_context=0, right_context=0, num_layers=3, num_neurons=32,
               num_projects=16, num_targets=9, use_peepholes=True, dropout_rate=1.0)
    if nnet_type != "blstm":
        del cfg["num_projects"]
    cfg.update(kw)
    return {k: v for k, v in cfg.items() if v is not None}


CONV = dict(conv_layers=2, conv_channels=16, conv_bins=40)


# ---------------------------------------------------------------------------------------------- the reference
def _case(seed, T, lens, F, Cin, Cout, nan_dead):
    rng = np.random.default_rng(seed)
    B, Fo = len(lens), ref.out_bins(F)
    x = rng.normal(size=(T, B, Cin * F))
    dy = rng.normal(size=(T, B, Fo * Cout))
    w = rng.normal(size=(3, 3, Cin, Cout))
    bias = rng.normal(size=Cout)
    xn, dyn = x.copy(), dy.copy()
    if nan_dead:
        dead = ~ref.live_rows(lens, T)
        xn[dead] = np.nan
        dyn[dead] = np.nan
    return x, dy, w, bias, xn, dyn


@pytest.mark.parametrize("nan_dead", (False, True))
@pytest.mark.parametrize("gm", (False, True))
@pytest.mark.parametrize("F", (1, 2, 5, 8, 41))
def test_reference_forward_is_conv2d_and_relu_on_the_live_rows(F, gm, nan_dead):
    """Per utterance, on its own live frames only: torch's conv2d(padding=1, stride=(1, 2)) + relu in float64."""
    T, lens, Cin, Cout = 7, (7, 1, 0, 9, 4), 3, 8
    x, _, w, bias, xn, _ = _case(F, T, lens, F, Cin, Cout, nan_dead)
    y = ref.fwd(xn, w, bias, lens, F, gm).reshape(T, len(lens), ref.out_bins(F), Cout)
    for b, n in enumerate(np.clip(lens, 0, T)):
        assert not y[n:, b].any()
        if n == 0:
            continue
        img = torch.from_numpy(ref.to_bins(x, F, gm)[:n, b]).permute(2, 0, 1)[None]               # [1, Cin, n, F]
        want = torch.relu(torch.nn.functional.conv2d(img, torch.from_numpy(w).permute(3, 2, 0, 1), torch.from_numpy(bias),
                                                     stride=(1, 2), padding=1))[0].permute(1, 2, 0).numpy()
        assert np.abs(y[:n, b] - want).max() < 1e-12
    assert np.abs(ref.torch_conv(torch.from_numpy(x), lens, torch.from_numpy(w), torch.from_numpy(bias), gm).numpy()
                  - y.reshape(T, len(lens), -1)).max() < 1e-12


@pytest.mark.parametrize("gm", (False, True))
@pytest.mark.parametrize("F", (1, 2, 5, 8, 41))
def test_reference_backward_is_autograd(F, gm):
    T, lens, Cin, Cout = 7, (7, 1, 0, 9, 4), 3, 8
    x, dy, w, bias, xn, dyn = _case(10 + F, T, lens, F, Cin, Cout, True)
    leaves = [torch.from_numpy(a).requires_grad_(True) for a in (x, w, bias)]
    y = ref.torch_conv(leaves[0], lens, leaves[1], leaves[2], gm)
    live = ref.live_rows(lens, T)
    (y * torch.from_numpy(np.where(live[:, :, None], dy, 0.0))).sum().backward()
    y_np = y.detach().numpy().copy()
    y_np[~live] = np.nan                                                                    # dead rows of y: never read either
    dx, dw, db = ref.bwd(xn, y_np, dyn, w, lens, F, gm)
    for got, leaf in ((dx, leaves[0]), (dw, leaves[1]), (db, leaves[2])):
        assert np.isfinite(got).all() and np.abs(got - leaf.grad.numpy()).max() < 1e-12
    assert not dx[~live].any()
    tol = ref.bounds(xn, y_np, dyn, w, bias, lens, F, gm)
    assert [t.shape for t in tol] == [y_np.shape, x.shape, w.shape, bias.shape] and all(np.isfinite(t).all() for t in tol)
    assert tol[0][~live].max() < 1e-29 and tol[0][live].min() > 1e-9 and tol[2].max() < 1e-2      # (dead rows: exactly +0)


def test_layouts_are_two_views_of_the_same_image():
    rng = np.random.default_rng(0)
    x4 = rng.normal(size=(3, 2, 5, 4))
    for gm in (False, True):
        assert np.array_equal(ref.to_bins(ref.from_bins(x4, gm), 5, gm), x4)
    assert ref.from_bins(x4, True)[1, 1, 2 * 5 + 3] == x4[1, 1, 3, 2] == ref.from_bins(x4, False)[1, 1, 3 * 4 + 2]


# ---------------------------------------------------------------------------------------------- config
def test_config_rules():
    from lstm_ctc_amd.nnet.model import conv_config
    for t in TYPES:
        assert conv_config(_cfg(t)) == () and conv_config(_cfg(t, conv_layers=0)) == ()
        # off: the other keys are not read and nothing is refused
        assert conv_config(_cfg(t, conv_layers=0, conv_channels=7, conv_bins=7, left_context=2, use_bn=True)) == ()
        assert conv_config(_cfg(t, **CONV)) == ((3, 16, 40, 20), (16, 16, 20, 10))
    assert conv_config(_cfg(conv_layers=1)) == ((1, 32, 120, 60),)                          # defaults: 32 channels, one input channel
    assert conv_config(_cfg(conv_layers=3, conv_bins=5, input_dim=15)) == ((3, 32, 5, 3), (32, 32, 3, 2), (32, 32, 2, 1))
    for key, bad in (("conv_layers", 4), ("conv_layers", -1), ("conv_layers", True), ("conv_layers", "2"), ("conv_layers", 1.0),
                     ("conv_channels", 4), ("conv_channels", 12), ("conv_channels", 72), ("conv_channels", 0), ("conv_channels", 16.0),
                     ("conv_bins", 0), ("conv_bins", 7), ("conv_bins", 240), ("conv_bins", "40")):
        with pytest.raises(ValueError, match=key):
            conv_config(_cfg(**dict(CONV, **{key: bad})))
    with pytest.raises(ValueError, match="conv_bins = 1 leaves input_dim / conv_bins = 120 input channels, more than 64"):
        conv_config(_cfg(conv_layers=1, conv_bins=1))
    with pytest.raises(ValueError, match="conv_bins must be in 1..512"):
        conv_config(_cfg(conv_layers=1, input_dim=600))
    with pytest.raises(ValueError, match="input_dim"):
        conv_config(dict(conv_layers=1))


def test_every_refusal_names_its_key():
    from lstm_ctc_amd.nnet.model import Model, conv_config
    for kw, text in ((dict(left_context=2), "conv_layers does not combine with left_context / right_context \\(2, 0\\)"),
                     (dict(right_context=1), "conv_layers does not combine with left_context / right_context \\(0, 1\\)"),
                     (dict(nnet_type="lstm", use_bn=True), "conv_layers does not combine with use_bn"),
                     (dict(pack_frames=True), "conv_layers does not combine with pack_frames = true"),
                     (dict(compute_dtype="bf16"), "conv_layers is built for compute_dtype = fp32 only, got compute_dtype = bf16"),
                     (dict(compute_dtype="bf16x3"), "conv_layers is built for compute_dtype = fp32 only, got compute_dtype = bf16x3")):
        with pytest.raises(ValueError, match=text):
            conv_config(_cfg(**dict(CONV, **kw)))
        with pytest.raises(ValueError, match="conv_layers"):                                # before a model is built
            Model(_cfg(**dict(CONV, **kw)), "cpu", seed=0)
    assert conv_config(_cfg(pack_frames=False, compute_dtype="fp32", **CONV))


def test_config_as_parse_config_delivers_it(tmp_path):
    from lstm_ctc_amd.nnet.config import parse_config
    from lstm_ctc_amd.nnet.model import conv_config
    p = tmp_path / "nnet.config"
    p.write_text("nnet_type = blstm\ninput_dim = 120\nnum_layers = 2\nconv_layers = 2\nconv_channels = 16\nconv_bins = 40\n")
    assert conv_config(parse_config(str(p))) == ((3, 16, 40, 20), (16, 16, 20, 10))
    p.write_text("nnet_type = blstm\ninput_dim = 120\nnum_layers = 2\nconv_layers = 2\nleft_context = 1\n")
    with pytest.raises(ValueError, match="left_context"):
        conv_config(parse_config(str(p)))
    p.write_text("nnet_type = blstm\ninput_dim = 120\nnum_layers = 2\nconv_layers = true\n")
    with pytest.raises(ValueError, match="conv_layers"):
        conv_config(parse_config(str(p)))


def test_info_line_lookahead_lines_and_report(capsys):
    from lstm_ctc_amd.nnet.model import (chunk_horizon, chunk_horizon_raw, chunk_info_line, conv_info_line, row_conv_horizon_raw,
                                         row_conv_info_line)
    assert conv_info_line(_cfg()) is None and conv_info_line(_cfg(conv_layers=0)) is None
    assert conv_info_line(_cfg(**CONV)) == (
        "convolutional front-end: conv_layers = 2, conv_channels = 16, conv_bins = 40: 3 input channels, bins 40 -> 20 -> 10, layer 0 "
        "reads 160 columns; %d parameters added; every logit reads 2 more frames on each side" % (9 * 3 * 16 + 16 + 9 * 16 * 16 + 16))
    # every logit reads n more future frames: the chunk keys' line and the row convolution's say so
    chunked = _cfg(chunk_frames=8, lookahead_frames=4, subsample=3)
    h = chunk_horizon(3, 8, 4) - 8
    assert chunk_horizon_raw(chunked) == (h, 3 * h) and chunk_horizon_raw(dict(chunked, **CONV)) == (h + 2, 3 * (h + 2))
    assert "read %d model frames (%d raw frames) past its end" % (h + 2, 3 * (h + 2)) in chunk_info_line(dict(chunked, **CONV))
    assert "read %d model frames (%d raw frames) past its end" % (h, 3 * h) in chunk_info_line(chunked)
    rc = _cfg("lstm", row_conv_frames=4, subsample=3)
    assert row_conv_horizon_raw(rc) == (4, 12) and row_conv_horizon_raw(dict(rc, **CONV)) == (6, 18)
    assert row_conv_info_line(dict(rc, **CONV)).endswith("row_conv_frames = 4: logits read 6 model frames (18 raw frames) past their own")
    assert row_conv_info_line(rc).endswith("row_conv_frames = 4: logits read 4 model frames (12 raw frames) past their own")
    spec = importlib.util.spec_from_file_location("_common_under_test", os.path.join(ROOT, "bin", "_common.py"))
    common = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(common)
    common.report_conv(_cfg())
    assert "convolutional front-end" not in capsys.readouterr().err
    common.report_conv(_cfg("lstm", **CONV))
    assert capsys.readouterr().err.count("convolutional front-end: conv_layers = 2") == 1
    with pytest.raises(SystemExit) as exc:
        common.report_conv(_cfg(left_context=1, **CONV))
    assert exc.value.code == 1 and "left_context" in capsys.readouterr().err
    for cli in ("nnet-train.py", "nnet-validate.py", "nnet-forward.py", "nnet-align.py"):
        assert "report_conv(nnet_config)" in open(os.path.join(ROOT, "bin", cli)).read(), cli


# ---------------------------------------------------------------------------------------------- parameters
@pytest.mark.parametrize("nnet_type", TYPES)
def test_param_store_layout(nnet_type):
    from lstm_ctc_amd.nnet.model import Model, ParamStore
    plain = ParamStore(_cfg(nnet_type), "cpu")
    off = ParamStore(_cfg(nnet_type, conv_layers=0), "cpu")
    assert off.names() == plain.names() and off.offsets == plain.offsets and off.n_decay == plain.n_decay and off.n == plain.n
    assert off.conv == () and off.D0 == off.D == 120
    cv = ParamStore(_cfg(nnet_type, **CONV), "cpu")
    assert cv.D == 120 and cv.D0 == 160
    new = [n for n in cv.names() if n not in plain.names()]
    assert new == ["conv0/kernel", "conv1/kernel", "conv0/bias", "conv1/bias"]
    assert [cv.shapes[n] for n in new] == [(3, 3, 3, 16), (3, 3, 16, 16), (16,), (16,)]
    assert [cv.kinds[n] for n in new] == ["conv_kernel", "conv_kernel", "conv_bias", "conv_bias"]
    # layer 0's kernels are as tall as the front-end's output (plus the recurrent part), every other shape is the plain model's
    first = [n for n in plain.names() if n.endswith("/kernel") and ("0/" in n or "cell_0/" in n) and "projection" not in n]
    assert first
    for n in plain.names():
        if n in first:
            assert cv.shapes[n] == (160 + cv.Pout, 4 * 32) and plain.shapes[n] == (120 + cv.Pout, 4 * 32), n
        else:
            assert cv.shapes[n] == plain.shapes[n], n
    # decay split: the kernels are decayed, the biases are not; both lie behind the LSTM layers' tensors of their block
    names = cv.names()
    assert cv.offsets["conv0/kernel"] < cv.offsets["conv1/kernel"] < cv.n_decay <= cv.offsets["conv0/bias"] < cv.offsets["conv1/bias"]
    lstm_decayed = [n for n in names if cv.kinds[n] in ("lstm_kernel", "peephole", "proj")]
    lstm_biases = [n for n in names if cv.kinds[n] == "lstm_bias"]
    assert cv.offsets["conv0/kernel"] > max(cv.offsets[n] for n in lstm_decayed)
    assert cv.offsets["conv0/bias"] > max(cv.offsets[n] for n in lstm_biases)
    assert cv.offsets["Variable"] > cv.offsets["conv1/kernel"]
    assert all(cv.offsets[n] % 4 == 0 for n in names)
    added = 9 * 3 * 16 + 9 * 16 * 16 + 32
    grown = sum(40 * 4 * 32 for _ in first)
    assert cv.num_params() == plain.num_params() + added + grown
    # no layer's gradient range (the data-parallel buckets) contains them
    shell = Model.__new__(Model)
    shell.ps = cv
    ranges = [Model.layer_grad_range(shell, i) for i in range(3)]
    for lo, hi in ranges:
        assert hi <= cv.n_decay and not any(lo <= cv.offsets[n] < hi for n in new)
    assert ranges[-1][1] == cv.offsets["conv0/kernel"]


def test_initialiser_is_seeded_glorot_uniform_with_zero_biases():
    from lstm_ctc_amd.nnet.model import ParamStore
    a, b, c = (ParamStore(_cfg(**CONV), "cpu") for _ in range(3))
    a.init_random(4)
    b.init_random(4)
    c.init_random(5)
    pa, pb, pc = a.export_tf(), b.export_tf(), c.export_tf()
    for k, (cin, cout) in enumerate(((3, 16), (16, 16))):
        w = pa["conv%d/kernel" % k]
        lim = np.sqrt(6.0 / (9 * cin + 9 * cout))
        assert w.shape == (3, 3, cin, cout) and np.abs(w).max() <= lim and np.abs(w).max() > 0.8 * lim and abs(w.mean()) < 0.2 * lim
        assert np.array_equal(w, pb["conv%d/kernel" % k]) and not np.array_equal(w, pc["conv%d/kernel" % k])
        assert np.array_equal(pa["conv%d/bias" % k], np.zeros(cout, np.float32))


def test_load_tf_refuses_both_ways_and_round_trips():
    from lstm_ctc_amd.nnet.model import ParamStore
    plain, cv = ParamStore(_cfg(), "cpu"), ParamStore(_cfg(**CONV), "cpu")
    plain.init_random(4)
    cv.init_random(5)
    with pytest.raises(KeyError, match="checkpoint has no conv0/kernel, conv1/kernel: a model with conv_layers = 2"):
        cv.load_tf(plain.export_tf())
    with pytest.raises(KeyError, match="checkpoint has conv0/kernel: it was written by a model with conv_layers set"):
        plain.load_tf(cv.export_tf())
    ck = cv.export_tf()
    rng = np.random.default_rng(0)
    ck["conv1/bias"] = rng.normal(size=16).astype(np.float32)
    again = ParamStore(_cfg(**CONV), "cpu")
    again.load_tf(ck)
    back = again.export_tf()
    assert set(back) == set(ck) and all(np.array_equal(back[k], ck[k]) for k in ck)
    bad = dict(ck)
    bad["conv0/kernel"] = np.zeros((3, 3, 1, 16), np.float32)
    with pytest.raises(ValueError, match="conv0/kernel"):
        again.load_tf(bad)


# ---------------------------------------------------------------------------------------------- the library
def test_library_exports_the_entry_points_and_refuses_bad_arguments():
    """The header's three symbols are in the built library and in the binding, lc_version() says 15; LC_EINVAL and
    LC_EWORKSPACE come before any launch, so every rejection can be seen without a GPU (the pointers are never dereferenced)."""
    import __graft_entry__ as g
    g.build()
    from lstm_ctc_amd import _lib
    header = " ".join(open(os.path.join(ROOT, "include", "lstm_ctc_hip.h")).read().split())
    assert "size_t lc_conv_workspace_bytes(int T, int B, int F, int Cin, int Cout);" in header
    assert ("int lc_conv_fwd(const float *x, int ldx, int x_group_major, const float *w, const float *bias, int T, int B, int F, "
            "int Cin, int Cout, const int *seq_len, float *y, int ldy, lc_stream_t stream);") in header
    assert ("int lc_conv_bwd(const float *x, int ldx, int x_group_major, const float *y, int ldy, const float *dy, int lddy, "
            "const float *w, int T, int B, int F, int Cin, int Cout, const int *seq_len, float *dx /* or NULL */, int lddx, "
            "float *dw, float *dbias /* both or neither; overwritten */, void *workspace, size_t workspace_bytes, lc_stream_t "
            "stream);") in header
    names = ("lc_conv_workspace_bytes", "lc_conv_fwd", "lc_conv_bwd")
    assert [len(_lib.SIGNATURES[n][1]) for n in names] == [5, 14, 21]
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(raw, n) for n in names)
    lib = _lib.load()
    assert lib.lc_version() >= 15
    T, B, F, Cin, Cout = 5, 3, 5, 3, 8
    Cx, Cy = Cin * F, 3 * Cout
    X, Y, DY, DX, W, Bs, L, DW, DB, WS = (0x100000 * k for k in range(1, 11))      # far apart, 16-byte aligned made-up addresses
    ws = lib.lc_conv_workspace_bytes(T, B, F, Cin, Cout)
    assert ws >= (9 * Cin * Cout + Cout) * 4 and ws % 256 == 0
    assert lib.lc_conv_workspace_bytes(1000, 64, 512, 64, 64) > 0
    for bad in ((0, B, F, Cin, Cout), (T, 0, F, Cin, Cout), (T, B, 0, Cin, Cout), (T, B, F, 0, Cout), (T, B, F, Cin, 0),
                (T, B, 513, Cin, Cout), (T, B, F, 65, Cout), (T, B, F, Cin, 72), (T, B, F, Cin, 12), (T, B, F, Cin, 4), (-1, B, F, Cin, Cout)):
        assert lib.lc_conv_workspace_bytes(*bad) == 0

    def fwd(x=X, ldx=Cx, gm=1, w=W, bias=Bs, T=T, B=B, F=F, Cin=Cin, Cout=Cout, seq_len=L, y=Y, ldy=Cy):
        return lib.lc_conv_fwd(x, ldx, gm, w, bias, T, B, F, Cin, Cout, seq_len, y, ldy, None)

    def bwd(x=X, ldx=Cx, gm=1, y=Y, ldy=Cy, dy=DY, lddy=Cy, w=W, T=T, B=B, F=F, Cin=Cin, Cout=Cout, seq_len=L, dx=DX, lddx=Cx,
            dw=DW, dbias=DB, wsp=WS, wb=ws):
        return lib.lc_conv_bwd(x, ldx, gm, y, ldy, dy, lddy, w, T, B, F, Cin, Cout, seq_len, dx, lddx, dw, dbias, wsp, wb, None)

    wide = dict(ldx=1 << 16, ldy=1 << 16)
    ybytes = 4 * T * B * Cy
    for kw in (dict(T=0), dict(B=0), dict(F=0), dict(Cin=0), dict(Cout=0), dict(T=-1), dict(F=513, **wide), dict(Cin=65, **wide),
               dict(Cout=72, **wide), dict(Cout=12, **wide), dict(Cout=4, **wide), dict(x=None), dict(w=None), dict(bias=None),
               dict(seq_len=None), dict(y=None), dict(ldx=Cx - 1), dict(ldy=Cy - 1), dict(y=X), dict(y=X - ybytes + 4),
               dict(y=W), dict(y=W + 4 * 9 * Cin * Cout - 4), dict(y=Bs + 4)):
        assert fwd(**kw) == -1, kw
        assert b"lc_conv_fwd" in lib.lc_last_error()
    wideb = dict(ldx=1 << 16, ldy=1 << 16, lddy=1 << 16, lddx=1 << 16)
    for kw in (dict(T=0), dict(B=0), dict(F=0), dict(Cin=0), dict(Cout=0), dict(F=513, **wideb), dict(Cin=65, **wideb),
               dict(Cout=72, **wideb), dict(Cout=12, **wideb), dict(y=None), dict(dy=None), dict(w=None), dict(seq_len=None),
               dict(x=None), dict(ldx=Cx - 1), dict(ldy=Cy - 1), dict(lddy=Cy - 1), dict(lddx=Cx - 1), dict(dw=None), dict(dbias=None),
               dict(dx=None, dw=None, dbias=None), dict(dx=X), dict(dx=X + 4 * T * B * Cx - 4), dict(dx=Y), dict(dx=DY + 4), dict(dx=W),
               dict(dw=W), dict(dw=X + 8), dict(dbias=DY), dict(dbias=DW + 16), dict(dw=DX), dict(dw=DB)):
        assert bwd(**kw) == -1, kw
        assert b"lc_conv_bwd" in lib.lc_last_error()
    for kw in (dict(wb=ws - 1), dict(wsp=None), dict(wb=0, dx=None)):
        assert bwd(**kw) == -3, kw                                                          # LC_EWORKSPACE
        assert b"lc_conv_bwd" in lib.lc_last_error()
