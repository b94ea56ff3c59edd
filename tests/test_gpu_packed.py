"""GPU tests of pack_frames: the input products of a ragged batch on live rows only (lc_pack_rows / lc_unpack_rows,
nnet/frames.py, Model.pack_frames).

1. the two kernels against torch indexing, exactly;
2. the packed model against the fp64 oracle at the yardsticks of test_gpu_model.py / test_gpu_configs.py (their helpers,
   imported, not restated), with which products ran on how many rows read from ops.PROFILE;
3. packed against padded on the same model and batch;
4. garbage in the dead frames of the input cannot reach anything;
5. the cases that must stay on the padded path;
6. a train loop over two alternating batches against the oracle's train steps.

Every model batch here has FIXED lengths with at least 20 % dead frames (asserted), in three orders: descending (the other GPU
tests' order), ascending (bench.py's) and unsorted (what a data-parallel rank may get)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ batches
def _lengths(B, T, order, shortest=None):
    """B lengths from T down to about 0.35 T in equal steps (so about a third of the frames are dead), in the given order."""
    lo = max(1, int(round(0.35 * T))) if shortest is None else shortest
    seq = np.round(np.linspace(T, lo, B)).astype(np.int32) if B > 1 else np.array([T], np.int32)
    seq[0] = T
    if order == "ascending":
        seq = seq[::-1].copy()
    elif order == "unsorted":
        seq = seq[np.random.default_rng(B * 1000 + T).permutation(B)].copy()
    else:
        assert order == "descending"
    assert 1.0 - seq.sum() / float(T * B) >= 0.2 or B == 1, seq           # the padded share that makes the case mean something
    return seq


def _inputs(rng, seq, T, D):
    B = len(seq)
    x = rng.normal(size=(B, T, D)).astype(np.float32)
    for b in range(B):
        x[b, seq[b]:] = 0
    return x


def _labels(rng, seq, T, V):
    """Dense labels every utterance can align (at most half its frames), with adjacent repeats: test_gpu_configs._batch's."""
    B = len(seq)
    labels = np.full((B, max(1, T // 2)), -1, np.int64)
    for b in range(B):
        n = int(rng.integers(1, max(2, seq[b] // 2 + 1)))
        labels[b, :n] = rng.integers(0, V - 1, size=n)
        if n >= 2 and b % 3 == 0:
            labels[b, 1] = labels[b, 0]
    return labels


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _tm(a):
    """batch-major [B,T,*] host array -> time-major device tensor"""
    return _dev(np.ascontiguousarray(a.transpose(1, 0, 2)).astype(np.float32))


def _profiled(fn):
    """Runs fn() with ops.PROFILE on; returns (result, records)."""
    from lstm_ctc_amd import ops
    ops.PROFILE = []
    try:
        res = fn()
        torch.cuda.synchronize()
        return res, list(ops.PROFILE)
    finally:
        ops.PROFILE = None


# ------------------------------------------------------------------------------------------------ 1. the kernels
def _ref_gather(x, index):
    """out[r] = x[index[r]] where index[r] >= 0 else +0.0 (host, torch indexing)."""
    out = torch.zeros((index.shape[0], x.shape[1]), dtype=torch.float32)
    ok = index >= 0
    out[ok] = x[index[ok].long()]
    return out


def _is_plus_zero(t):
    return bool((t.contiguous().view(torch.int32) == 0).all())


@pytest.mark.parametrize("C", [40, 44, 120, 2048, 4096])
@pytest.mark.parametrize("lengths", ["unsorted_zero", "ascending", "descending"])
def test_pack_unpack_rows_exact(C, lengths):
    from lstm_ctc_amd import ops
    from lstm_ctc_amd.nnet.frames import FrameMap
    T, B = 23, 14
    if lengths == "unsorted_zero":
        seq = np.array([9, 23, 0, 17, 4, 23, 11, 1, 0, 20, 7, 15, 2, 19], np.int32)       # two empty utterances
    else:
        seq = _lengths(B, T, lengths)
    fm = FrameMap(seq, T, B)
    assert 0 < fm.M < T * B and fm.Mp > fm.M
    rows_d, inv_d = fm.device("cuda")
    rows_h, inv_h = torch.from_numpy(fm.rows), torch.from_numpy(fm.inverse)
    g = torch.Generator().manual_seed(C)
    x = torch.randn((T * B, C), generator=g)
    x[3, 1] = float("nan")                        # a NaN in a live row travels as a bit pattern
    x[5, 0] = -0.0
    xd = x.cuda()
    # pack: NaN-poisoned output, every row written once, tail rows exactly +0.0
    out = torch.full((fm.Mp, C), float("nan"), device="cuda")
    res = ops.pack_rows(xd, rows_d, out=out)
    assert res is out
    want = _ref_gather(x, rows_h)
    got = out.cpu()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert _is_plus_zero(got[fm.M:])
    # unpack: dead rows exactly +0.0, live rows the packed ones
    back = torch.full((T * B, C), float("nan"), device="cuda")
    ops.unpack_rows(out, inv_d, out=back)
    back_h = back.cpu()
    assert torch.equal(back_h.view(torch.int32), _ref_gather(got, inv_h).view(torch.int32))
    dead = inv_h < 0
    assert _is_plus_zero(back_h[dead])
    x0 = x.clone()
    x0[dead] = 0.0
    assert torch.equal(back_h.view(torch.int32), x0.view(torch.int32))           # unpack(pack(x)) == x, dead rows zeroed
    # allocating form
    assert torch.equal(ops.pack_rows(xd, rows_d).cpu().view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("C,off,width", [(40, 0, 64), (44, 4, 52), (120, 8, 256), (2048, 2048, 4096), (44, 3, 50), (41, 0, 41),
                                         (4096, 4, 4104)])
def test_pack_unpack_rows_column_windows(C, off, width):
    """Row pitches: source and destination are column windows of wider buffers (16-byte aligned or not); nothing outside the
    destination window is touched."""
    from lstm_ctc_amd import ops
    from lstm_ctc_amd.nnet.frames import FrameMap
    T, B = 9, 7
    seq = np.array([9, 2, 6, 0, 9, 4, 1], np.int32)
    fm = FrameMap(seq, T, B)
    rows_d, inv_d = fm.device("cuda")
    g = torch.Generator().manual_seed(C + off)
    wide = torch.randn((T * B, width), generator=g)
    src = wide.cuda()[:, off:off + C]
    dst_wide = torch.full((fm.Mp, width), 7.0, device="cuda")
    ops.pack_rows(src, rows_d, out=dst_wide[:, off:off + C])
    want = torch.full((fm.Mp, width), 7.0)
    want[:, off:off + C] = _ref_gather(wide[:, off:off + C], torch.from_numpy(fm.rows))
    assert torch.equal(dst_wide.cpu(), want)
    back_wide = torch.full((T * B, width), -3.0, device="cuda")
    ops.unpack_rows(dst_wide[:, off:off + C], inv_d, out=back_wide[:, off:off + C])
    want_b = torch.full((T * B, width), -3.0)
    want_b[:, off:off + C] = _ref_gather(want[:, off:off + C], torch.from_numpy(fm.inverse))
    assert torch.equal(back_wide.cpu(), want_b)


def test_pack_rows_many_rows_grid_stride():
    """More row groups than workgroups (the grid-stride walk), at a c4 width."""
    from lstm_ctc_amd import ops
    from lstm_ctc_amd.nnet.frames import FrameMap
    T, B, C = 150, 64, 2048
    seq = _lengths(B, T, "ascending")
    fm = FrameMap(seq, T, B)
    assert fm.Mp > 4096
    rows_d, inv_d = fm.device("cuda")
    x = torch.randn((T * B, C), generator=torch.Generator().manual_seed(1))
    p = ops.pack_rows(x.cuda(), rows_d)
    assert torch.equal(p.cpu(), _ref_gather(x, torch.from_numpy(fm.rows)))
    u = ops.unpack_rows(p, inv_d)
    x[torch.from_numpy(fm.inverse) < 0] = 0
    assert torch.equal(u.cpu(), x)


def test_pack_rows_records_its_kind_and_rejects_bad_arguments():
    from lstm_ctc_amd import _lib, ops
    x = torch.randn(6, 8, device="cuda")
    idx = torch.tensor([0, 5, -1, 2], dtype=torch.int32, device="cuda")
    _, prof = _profiled(lambda: (ops.pack_rows(x, idx), ops.unpack_rows(x, idx)))
    assert [k for k, _, _, _ in prof] == ["pack", "pack"] and prof[0][1] == 8.0 * 4 * 8
    with pytest.raises(_lib.LibraryError):
        ops.pack_rows(x.cpu(), idx)
    lib = _lib.load()
    assert lib.lc_pack_rows(None, 8, idx.data_ptr(), 4, 8, x.data_ptr(), 8, None) != 0
    assert lib.lc_unpack_rows(x.data_ptr(), 4, idx.data_ptr(), 4, 8, x.data_ptr(), 8, None) != 0        # pitch < C
    assert lib.lc_version() >= 2


# ------------------------------------------------------------------------------------------------ 2. against the oracle
PACKED_VARIANTS = {
    # variant of test_gpu_model.VARIANTS: order of the lengths
    "blstm": "ascending",
    "blstm_residual": "unsorted",
    "blstm_dropout_moe": "descending",
    "blstm_3layer_b70": "unsorted",
    "lstm": "descending",
    "lstm_bn_dropout": "ascending",
    "cudnnlstm": "unsorted",
}


def _variant_cfg(variant, **kw):
    from test_gpu_model import VARIANTS, _cfg
    cfg = _cfg(**VARIANTS[variant])
    cfg.update(kw)
    return {k: v for k, v in cfg.items() if v is not None}


def _variant_setup(variant, rng, pack=True, **kw):
    """Model + batch of test_gpu_model.test_model_forward_backward_vs_oracle, with fixed ragged lengths."""
    from lstm_ctc_amd.nnet.model import Model
    cfg = _variant_cfg(variant, **kw)
    B, T = (70, 6) if variant.endswith("b70") else (5, 11)
    seq = _lengths(B, T, PACKED_VARIANTS.get(variant, "descending"), shortest=1)
    x = _inputs(rng, seq, T, cfg["input_dim"])
    model = Model(dict(cfg, pack_frames=pack), "cuda", seed=3)
    params = model.ps.export_tf()
    for k in params:                                            # non-zero biases so they matter
        if "bias" in k or k in ("Variable_1", "Variable_3") or k.endswith("/beta") or k.endswith("/moving_mean"):
            params[k] = rng.normal(0, 0.2, size=params[k].shape).astype(np.float32)
        if k.endswith("/gamma") or k.endswith("/moving_variance"):
            params[k] = rng.uniform(0.5, 1.5, size=params[k].shape).astype(np.float32)
    model.ps.load_tf(params)
    dl = rng.normal(size=(B, T, cfg["num_targets"]))            # arbitrary upstream gradient, batch-major
    for b in range(B):
        dl[b, seq[b]:] = 0                                      # CTC never sends gradient into padded frames
    return cfg, model, params, x, seq, dl


def _forward_backward(model, x, seq, dl, drop_seed=7):
    """-> (logits [B,T,V] host, gradients in TF layout, profile records)"""
    xt, sl, dlt = _tm(x), _dev(seq), _tm(dl)

    def run():
        logits = model.forward(xt, sl, drop_seed=drop_seed)
        packed = model.packed
        got = logits.cpu().numpy().transpose(1, 0, 2)
        model.backward(dlt)
        return got, packed

    (got, packed), prof = _profiled(run)
    return got, model.ps.export_tf(grads=True), prof, packed


@pytest.mark.parametrize("variant", sorted(PACKED_VARIANTS))
def test_packed_model_forward_backward_vs_oracle(oracle, variant):
    from conftest import check_grad
    rng = np.random.default_rng(sum(map(ord, variant)))
    cfg, model, params, x, seq, dl = _variant_setup(variant, rng)
    assert model.pack_frames
    p64 = {k: v.astype(np.float64) for k, v in params.items()}
    ref_logits, saved = oracle.forward(p64, cfg, x.astype(np.float64), seq, drop_seed=7)
    xt, sl = _tm(x), _dev(seq)

    def fwd():
        return model.forward(xt, sl, drop_seed=7)

    logits, prof_f = _profiled(fwd)
    assert model.packed is True
    assert "pack" in {k for k, _, _, _ in prof_f}
    got = logits.cpu().numpy().transpose(1, 0, 2)
    scale = np.abs(ref_logits).max()
    e = np.abs(got - ref_logits)
    assert e.max() < 1e-4 * max(scale, 1.0), e.max()
    assert np.all(e <= 1e-4 * np.maximum(np.abs(ref_logits), 0.1 * max(scale, 1.0)))
    if cfg["nnet_type"] == "blstm":
        np.testing.assert_allclose(model.encoder().cpu().numpy(), saved["encoder"], atol=1e-4)
    for L in model.saved["layers"]:                              # the padded buffers are still the saved ones
        assert L["inp"].shape[0] == x.shape[0] * x.shape[1] and L["inp_packed"].shape[0] % 256 == 0
    ref_grads, _ = oracle.backward(p64, cfg, saved, dl)
    _, prof_b = _profiled(lambda: model.backward(_tm(dl)))
    assert "pack" in {k for k, _, _, _ in prof_b}
    grads = model.ps.export_tf(grads=True)
    assert set(grads) == set(ref_grads), set(grads) ^ set(ref_grads)
    for k in sorted(ref_grads):
        check_grad(grads[k], ref_grads[k], "packed/" + str(variant), k)


PACKED_CONFIG_CASES = {
    # case of test_gpu_configs.FP32_CASES: order of the lengths
    "c2_3x320_persistent": "ascending",            # N <= 512: weight gradients on the side stream (overlap_wgrad)
    "c4_1024_b64_t40": "unsorted",
    "c4_5x1024_b64_t8": "ascending",               # five layers: the two-segment dX product on packed rows
    "c4_1024_b100_t6": "descending",
    "c4_1024_b33_t5_launch_train": "unsorted",     # LC_LSTM_PERSISTENT=0
}


@pytest.mark.parametrize("case", sorted(PACKED_CONFIG_CASES))
def test_packed_configs_vs_oracle(oracle, case, monkeypatch):
    """test_gpu_configs.test_fp32_configs_vs_oracle's check (logits, loss, CTC gradient, tokens, every gradient; schedule
    asserted) at the benchmark widths, with pack_frames on."""
    import test_gpu_configs as tc
    from lstm_ctc_amd.nnet.model import Model
    cfg, B, T, want_f, want_b, env = tc.FP32_CASES[case]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(sum(map(ord, case)))
    seq = _lengths(B, T, PACKED_CONFIG_CASES[case], shortest=max(2, T // 3))
    x = _inputs(rng, seq, T, cfg["input_dim"])
    labels = _labels(rng, seq, T, cfg["num_targets"])
    model = Model(dict(cfg, pack_frames=True), "cuda", seed=17)
    params = tc._randomise_biases(model, rng)
    got = tc._run_model(model, cfg, x, seq, labels)
    assert model.packed is True and "pack" in got["kinds"], got["kinds"]
    assert (got["sched_f"]["kind"], got["sched_f"]["mt"] if want_f[1] else 0) == want_f, got["sched_f"]
    assert (got["sched_b"]["kind"], got["sched_b"]["mt"] if want_b[1] else 0) == want_b, got["sched_b"]
    assert model.overlap_wgrad == (cfg["num_neurons"] <= 512)
    ref, ref_grads = tc._oracle_reference(oracle, params, cfg, x, seq, labels)
    _check = tc._check
    _check(got, ref["logits"], ref["loss_per_utt"], ref["dlogits"], ref["tokens"], ref["token_len"], ref_grads,
           tag="packed/" + case, elementwise=True)


def _expected_gemm_work(cfg, T, B, Mp):
    """Sum of 2 M N K over every fp32 product of one forward + backward of a BiLSTM-P stack with an affine head and no
    dropout: Mp rows for zx, dKx and dX, T * B for everything else that has a row dimension."""
    D, N, P, V, L = cfg["input_dim"], cfg["num_neurons"], cfg["num_projects"], cfg["num_targets"], cfg["num_layers"]
    rows = T * B
    w = 0.0
    for i in range(L):
        I = D if i == 0 else 2 * P
        for _ in range(2):
            w += 2.0 * Mp * 4 * N * I                  # zx = X Kx                       (packed)
            w += 2.0 * N * 4 * N * P                   # R = proj Kh                     (weights only)
            w += 2.0 * rows * P * N                    # projection m = m' proj
            w += 2.0 * rows * N * P                    # dh = dY_half proj^T
            w += 2.0 * I * 4 * N * Mp                  # dKx = X^T dZ                    (packed)
            w += 2.0 * N * 4 * N * (rows - B)          # dR = M'_prev^T dZ
            w += 2.0 * P * 4 * N * N                   # dKh = proj^T dR                 (weights only)
            w += 2.0 * N * P * rows                    # dproj = M'^T dY_half
            w += 2.0 * N * P * 4 * N                   # dproj += dR Kh^T                (weights only)
            if i > 0:
                w += 2.0 * Mp * I * 4 * N              # dX = dZ Kx^T                    (packed)
    w += 2.0 * rows * V * 2 * P                        # logits
    w += 2.0 * rows * 2 * P * V                        # dY = dlogits W^T
    w += 2.0 * 2 * P * V * rows                        # dW = Y^T dlogits
    return w


@pytest.mark.parametrize("layers", [1, 2])
def test_packed_products_run_on_Mp_rows(layers):
    """ops.PROFILE records 2 M N K per product: with pack_frames the zx, dKx and dX products must account for Mp rows and
    every other product for T * B - and without it every product for T * B."""
    from lstm_ctc_amd.nnet.frames import FrameMap
    from lstm_ctc_amd.nnet.model import Model
    cfg = _variant_cfg("blstm", num_layers=layers, input_dim=12)
    T, B = 40, 16                                     # T * B = 640 rows, M = 432 of them live -> Mp = 512
    seq = _lengths(B, T, "ascending")
    fm = FrameMap(seq, T, B)
    assert fm.Mp < T * B and fm.Mp != fm.M
    rng = np.random.default_rng(layers)
    x = _inputs(rng, seq, T, cfg["input_dim"])
    dl = rng.normal(size=(B, T, cfg["num_targets"]))
    for pack, m_rows in ((True, fm.Mp), (False, T * B)):
        model = Model(dict(cfg, pack_frames=pack), "cuda", seed=3)
        _, _, prof, packed = _forward_backward(model, x, seq, dl)
        assert packed is pack
        work = sum(w for k, w, _, _ in prof if k == "gemm")
        assert work == _expected_gemm_work(cfg, T, B, m_rows), (pack, work, _expected_gemm_work(cfg, T, B, m_rows))
        n_pack = sum(1 for k, _, _, _ in prof if k == "pack")
        # per layer: pack X, unpack zx x 2, pack dz x 2, and from the second layer up unpack dX
        assert n_pack == (5 * layers + (layers - 1) if pack else 0), n_pack


# ------------------------------------------------------------------------------------------------ 3. packed against padded
@pytest.mark.parametrize("variant", ["blstm", "blstm_dropout_moe", "blstm_3layer_b70", "lstm_bn_dropout"])
def test_packed_against_padded(variant):
    """Same parameters, same batch: each run is within one oracle tolerance of the oracle, so they are within two of each
    other (not bit-identical: the GEMM kernel choice depends on the row count, and the kernels sum K in different orders)."""
    from conftest import GRAD_TOL
    res = {}
    for pack in (True, False):
        rng = np.random.default_rng(sum(map(ord, variant)))
        cfg, model, params, x, seq, dl = _variant_setup(variant, rng, pack=pack)
        res[pack] = _forward_backward(model, x, seq, dl)
        assert res[pack][3] is pack
    (l1, g1, _, _), (l0, g0, _, _) = res[True], res[False]
    assert np.abs(l1 - l0).max() < 2e-4 * max(np.abs(l0).max(), 1.0)
    assert set(g1) == set(g0)
    for k in sorted(g0):
        assert np.abs(g1[k] - g0[k]).max() < 2 * GRAD_TOL * max(float(np.abs(g0[k]).max()), 1e-3), k


# ------------------------------------------------------------------------------------------------ 4. dead frames
@pytest.mark.parametrize("garbage", [1e30, float("nan")])
def test_dead_frame_garbage_cannot_leak(garbage):
    """The packed products never read a dead row of the input: 1e30 or NaN there changes no bit of the live logits or of any
    gradient.  (The padded path cannot offer this: it multiplies those rows.)"""
    rng = np.random.default_rng(5)
    cfg, model, params, x, seq, dl = _variant_setup("blstm", rng)
    B, T = x.shape[:2]
    xg = x.copy()
    for b in range(B):
        xg[b, seq[b]:] = garbage
    assert not np.array_equal(np.nan_to_num(xg, nan=1.0), x)
    clean = _forward_backward(model, x, seq, dl)
    dirty = _forward_backward(model, xg, seq, dl)
    assert clean[3] is True and dirty[3] is True
    assert np.isfinite(dirty[0]).all()
    for b in range(B):
        assert np.array_equal(clean[0][b, :seq[b]].view(np.int32), dirty[0][b, :seq[b]].view(np.int32)), b
    for k in sorted(clean[1]):
        assert np.array_equal(clean[1][k].view(np.int32), dirty[1][k].view(np.int32)), k
        assert np.isfinite(dirty[1][k]).all(), k
    assert max(float(np.abs(v).max()) for v in clean[1].values()) > 0


# ------------------------------------------------------------------------------------------------ 5. fallbacks
@pytest.mark.parametrize("dtype", ["bf16", "bf16x3"])
def test_bf16_modes_stay_padded(dtype):
    res = {}
    for pack in (True, False):
        rng = np.random.default_rng(9)
        cfg, model, params, x, seq, dl = _variant_setup("blstm", rng, pack=pack, compute_dtype=dtype)
        assert model.pack_frames is False
        res[pack] = _forward_backward(model, x, seq, dl)
        assert res[pack][3] is False and model.packed is False
        assert "pack" not in {k for k, _, _, _ in res[pack][2]}
    assert np.array_equal(res[True][0].view(np.int32), res[False][0].view(np.int32))
    for k in res[False][1]:
        assert np.array_equal(res[True][1][k].view(np.int32), res[False][1][k].view(np.int32)), k


def test_full_batch_stays_padded():
    from lstm_ctc_amd.nnet.model import Model
    cfg = _variant_cfg("blstm")
    B, T = 5, 11
    rng = np.random.default_rng(2)
    seq = np.full(B, T, np.int32)
    x = _inputs(rng, seq, T, cfg["input_dim"])
    dl = rng.normal(size=(B, T, cfg["num_targets"]))
    res = {}
    for pack in (True, False):
        model = Model(dict(cfg, pack_frames=pack), "cuda", seed=3)
        assert model.pack_frames is pack
        res[pack] = _forward_backward(model, x, seq, dl)
        assert res[pack][3] is False
        assert "pack" not in {k for k, _, _, _ in res[pack][2]}
    assert np.array_equal(res[True][0].view(np.int32), res[False][0].view(np.int32))
    for k in res[False][1]:
        assert np.array_equal(res[True][1][k].view(np.int32), res[False][1][k].view(np.int32)), k


def test_environment_overrides_the_config_key(monkeypatch):
    from lstm_ctc_amd.nnet.model import Model
    rng = np.random.default_rng(4)
    cfg = _variant_cfg("blstm")
    seq = _lengths(5, 11, "descending")
    x = _inputs(rng, seq, 11, cfg["input_dim"])
    assert Model(cfg, "cuda", seed=3).pack_frames is False                    # the default
    for env, key, want in (("0", True, False), ("1", False, True), ("1", True, True), ("0", False, False)):
        monkeypatch.setenv("LC_PACK_FRAMES", env)
        model = Model(dict(cfg, pack_frames=key), "cuda", seed=3)
        assert model.pack_frames is want
        model.forward(_tm(x), _dev(seq))
        assert model.packed is want
    monkeypatch.delenv("LC_PACK_FRAMES")
    assert Model(dict(cfg, pack_frames=True), "cuda", seed=3).pack_frames is True


def test_frame_map_cache_keys():
    """One device tensor re-used step after step: one map, no copy; another tensor, other lengths in the same tensor, or host
    lengths handed over: the map of THAT batch."""
    from lstm_ctc_amd.nnet.model import Model
    rng = np.random.default_rng(4)
    cfg = _variant_cfg("blstm", pack_frames=True)
    T, B = 11, 5
    seq = _lengths(B, T, "descending")
    xt = _tm(_inputs(rng, seq, T, cfg["input_dim"]))
    model = Model(cfg, "cuda", seed=3)
    sl = _dev(seq)
    model.forward(xt, sl)
    fm = model.frame_map(sl, T, B)
    model.forward(xt, sl)
    assert model.frame_map(sl, T, B) is fm and fm.M == int(seq.sum())
    other = _dev(seq[::-1].copy())
    fm2 = model.frame_map(other, T, B)
    assert fm2 is not fm and np.array_equal(fm2.seq_len, seq[::-1])
    sl.copy_(other)                                                  # same address, new contents: _version moved
    fm3 = model.frame_map(sl, T, B)
    assert np.array_equal(fm3.seq_len, seq[::-1])
    fm4 = model.frame_map(sl, T, B, seq_len_host=seq)                # host lengths win and are compared by value
    assert np.array_equal(fm4.seq_len, seq)
    assert model.frame_map(sl, T, B, seq_len_host=seq.copy()) is fm4
    assert model.frame_map(sl, T, B, seq_len_host=seq[::-1].copy()) is not fm4


# ------------------------------------------------------------------------------------------------ 6. train loop
TRAIN_BATCH_SEED = 4        # see test_packed_train_steps_vs_oracle


def _train_batches(seed):
    rng = np.random.default_rng(seed)
    B, T, D, V = 5, 14, 12, 8
    batches = []
    for order in ("descending", "unsorted"):
        seq = _lengths(B, T, order, shortest=4)
        labels = np.full((B, 6), -1, np.int64)
        for b in range(B):
            n = int(rng.integers(1, min(6, seq[b] // 2) + 1))
            labels[b, :n] = rng.integers(0, V - 1, size=n)
        batches.append({"nnet_input": _inputs(rng, seq, T, D), "sequence_length": seq, "nnet_target": labels})
    return batches


TRAIN_CFG = dict(nnet_type="blstm", input_dim=12, left_context=0, right_context=0, num_layers=2, num_neurons=32,
                 num_projects=16, num_targets=8, use_peepholes=True, dropout_rate=0.9)


def test_packed_train_steps_vs_oracle(oracle):
    """Three CTCGraph.step calls, adam, dropout 0.9, on two alternating ragged host batches of the same shape (A, B, A): a
    frame map left over from the other batch would drop live frames and keep dead ones, and the step would leave the oracle's
    trajectory.  Tolerances of test_gpu_train.py::test_train_steps_vs_oracle.

    The batch draw (TRAIN_BATCH_SEED; the lengths are fixed, the seed draws frames and labels): the parameter comparison after an
    Adam step divides every gradient element by its own magnitude, so an element whose gradient lies at the fp32 rounding
    level of its tensor moves by an lr-sized step that follows the rounding, in any implementation.  Seed 3, the first one
    tried, has such an element: bd0/brnn0/kernel[11, 30] has a first-step gradient of 4.9e-6 against its tensor's largest of
    2.8, the kernels return 5.35e-6 (an error of 1.5e-7 of the largest entry, GRAD_TOL being 1e-4) and Adam turns that into
    a parameter difference of 2.02e-4 against the bound of 2e-4 - with pack_frames off as well as on, the same digits.
    Measured over seeds 3 .. 10, packed = padded to four digits in every one: 2.0e-4, 5.3e-6, 1.6e-5, 1.1e-5, 5.6e-5, 2.5e-5,
    1.8e-5, 1.1e-3.  The draw says nothing about packing; seed 4 is the next one."""
    from lstm_ctc_amd.nnet.graph import create_graph_for_training_ctc
    cfg = TRAIN_CFG
    batches = _train_batches(TRAIN_BATCH_SEED)
    assert not np.array_equal(batches[0]["sequence_length"], batches[1]["sequence_length"])
    graph = create_graph_for_training_ctc(None, dict(cfg, pack_frames=True), learn_rate=1e-2, clip_norm=5.0,
                                          optimizer="adam", seed=11)
    assert graph.model.pack_frames and graph.model.keep == 0.9
    params = {k: v.copy() for k, v in graph.model.ps.export_tf().items()}
    state = {}
    maps = []
    for step, batch in enumerate((batches[0], batches[1], batches[0])):
        out = graph.step(batch, fetch_eval=True)
        assert graph.model.packed is True
        maps.append(graph.model._frame_map[2])
        assert np.array_equal(maps[-1].seq_len, batch["sequence_length"])
        ref = oracle.train_step(params, cfg, batch["nnet_input"], batch["sequence_length"], batch["nnet_target"],
                                state, optimizer="adam", lr=1e-2, clip_norm=5.0, l2=1e-5, drop_seed=graph.drop_seed)
        assert out["size"] == ref["size"]
        assert abs(out["eval_loss"] - ref["eval_loss"]) / ref["eval_loss"] < 1e-4
        assert abs(out["loss"] - ref["loss"]) / abs(ref["loss"]) < 1e-4
        assert out["eval"] == ref["eval"]
        tok, n = out["decoded"]
        assert np.array_equal(n, ref["token_len"])
        for b in range(len(n)):
            assert np.array_equal(tok[b, :n[b]], ref["tokens"][b, :n[b]])
        assert abs(out["grad_norm"] - ref["grad_norm"]) / ref["grad_norm"] < 2e-3
        got = graph.model.ps.export_tf()
        for k in params:
            assert np.abs(got[k] - params[k]).max() < 2e-4 * max(1.0, np.abs(params[k]).max()), (step, k)
    assert graph.persist_fallbacks == 0
    assert maps[0] is not maps[1] and maps[1] is not maps[2]
