"""Host tests of the latency-controlled BiLSTM: the float64 reference the GPU tests use is pinned to
oracle/torch_f64.py where the two must agree, the config keys' rules, the horizon arithmetic and its INFO line, the chunk
lengths, and the library's entry points and their argument checks.  None needs a GPU."""
import ctypes
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from lc_blstm_reference import horizon, lc_blstm_forward, lc_blstm_gradients  # noqa: E402


def _cfg(**kw):
    cfg = dict(nnet_type="blstm", input_dim=10, left_context=0, right_context=0, num_layers=2, num_neurons=32,
               num_projects=16, num_targets=9, use_peepholes=True, dropout_rate=1.0)
    cfg.update(kw)
    return cfg


def _params(cfg, rng):
    from lstm_ctc_amd.nnet.model import ParamStore
    ps = ParamStore(cfg, torch.device("cpu"))
    ps.init_random(3)
    params = ps.export_tf()
    for k in params:
        if "bias" in k or k == "Variable_1":
            params[k] = rng.normal(0, 0.2, size=params[k].shape).astype(np.float32)
    return {k: v.astype(np.float64) for k, v in params.items()}


# ---------------------------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("Nc,Nr,drop", [(4, 7, 1.0), (4, 11, 0.8), (3, 40, 1.0), (16, 0, 1.0)])
def test_reference_equals_the_plain_model_when_every_window_reaches_the_end(Nc, Nr, drop):
    """Nr >= T - Nc: each chunk's window runs to the end of its utterance, so the chunked backward direction sees what the
    plain one sees.  float64 on both sides; the only difference is where the dead steps sit: 1e-12."""
    from oracle import torch_f64
    T, B = 11, 5
    assert Nr >= T - Nc
    cfg = _cfg(dropout_rate=drop)
    rng = np.random.default_rng(5)
    params = _params(cfg, rng)
    seq_len = np.array([11, 8, 6, 4, 1], np.int64)
    x = rng.normal(size=(T, B, cfg["input_dim"]))
    for b in range(B):
        x[seq_len[b]:, b] = 0
    dl = rng.normal(size=(T, B, cfg["num_targets"]))
    for b in range(B):
        dl[seq_len[b]:, b] = 0
    ref_logits, ref_grads = torch_f64.blstm_gradients(params, cfg, x, seq_len, dl, drop_seed=7, device="cpu")
    logits, grads = lc_blstm_gradients(params, cfg, x, seq_len, dl, Nc, Nr, drop_seed=7)
    assert float((logits - ref_logits).abs().max()) < 1e-12
    assert set(grads) == set(ref_grads)
    for k in ref_grads:
        assert np.abs(grads[k] - ref_grads[k]).max() < 1e-12 * max(np.abs(ref_grads[k]).max(), 1.0), k


def test_reference_truncates_and_obeys_the_horizon():
    """With a short lookahead the reference differs from the plain model, and chunk c's logits ignore frames >= H_L(c)."""
    from oracle import torch_f64
    T, B, Nc, Nr = 23, 2, 4, 2
    cfg = _cfg()
    rng = np.random.default_rng(6)
    params = _params(cfg, rng)
    seq_len = np.array([T, T], np.int64)
    x = rng.normal(size=(T, B, cfg["input_dim"]))
    a = lc_blstm_forward(params, cfg, x, seq_len, Nc, Nr)
    assert float((a - torch_f64.blstm_forward(params, cfg, x, seq_len, device="cpu")).abs().max()) > 1e-6
    for c in (0, 2):
        H = horizon(2, Nc, Nr, c, T)
        y = x.copy()
        y[H:] = rng.normal(size=y[H:].shape)
        assert torch.equal(lc_blstm_forward(params, cfg, y, seq_len, Nc, Nr)[c * Nc:(c + 1) * Nc], a[c * Nc:(c + 1) * Nc])
        y = x.copy()
        y[H - 1] = rng.normal(size=y[H - 1].shape)
        assert not torch.equal(lc_blstm_forward(params, cfg, y, seq_len, Nc, Nr)[c * Nc:(c + 1) * Nc], a[c * Nc:(c + 1) * Nc])


# ---------------------------------------------------------------------------------------------- keys, horizon, INFO line
def test_chunk_config_rules():
    from lstm_ctc_amd.nnet.model import chunk_config
    assert chunk_config(_cfg()) == (0, 0)
    assert chunk_config(_cfg(chunk_frames=0, lookahead_frames=5)) == (0, 0)
    assert chunk_config(_cfg(chunk_frames=0, nnet_type="lstm", compute_dtype="bf16")) == (0, 0)
    assert chunk_config(_cfg(chunk_frames=8)) == (8, 0)
    assert chunk_config(_cfg(chunk_frames=8, lookahead_frames=4, compute_dtype="fp32")) == (8, 4)
    for bad in (dict(chunk_frames=-1), dict(chunk_frames=2.5), dict(chunk_frames=True), dict(chunk_frames="x")):
        with pytest.raises(ValueError, match="chunk_frames"):
            chunk_config(_cfg(**bad))
    with pytest.raises(ValueError, match="lookahead_frames"):
        chunk_config(_cfg(chunk_frames=4, lookahead_frames=-2))
    for nt in ("lstm", "cudnnlstm"):
        with pytest.raises(ValueError, match="chunk_frames"):
            chunk_config(_cfg(chunk_frames=4, nnet_type=nt))
    for cd in ("bf16", "bfloat16", "bf16x3"):
        with pytest.raises(ValueError, match="chunk_frames"):
            chunk_config(_cfg(chunk_frames=4, compute_dtype=cd))


def test_horizon_arithmetic():
    from lstm_ctc_amd.nnet.model import chunk_horizon
    assert chunk_horizon(1, 4, 2) == 6 and chunk_horizon(2, 4, 2) == 10 and chunk_horizon(3, 4, 2) == 14
    assert chunk_horizon(2, 4, 2, c=2) == 18 and chunk_horizon(2, 4, 2, c=2, T=23) == 18
    assert chunk_horizon(2, 4, 2, c=5, T=23) == 23
    assert chunk_horizon(5, 40, 20) == 5 * 40 + 20 and chunk_horizon(5, 100, 40) == 5 * 100 + 40    # Nr <= Nc: a chunk per layer
    assert chunk_horizon(3, 8, 0) == 8                                    # no lookahead: nothing past the chunk, at any depth
    for L in (1, 2, 3):
        for Nc, Nr in ((4, 2), (1, 0), (3, 7), (8, 8)):
            for c in (0, 1, 3):
                for T in (9, 23, 100):
                    assert chunk_horizon(L, Nc, Nr, c=c, T=T) == horizon(L, Nc, Nr, c, T)


def test_info_line_counts_raw_frames(capsys):
    from lstm_ctc_amd.nnet.model import chunk_horizon_raw, chunk_info_line
    cfg = _cfg(chunk_frames=4, lookahead_frames=2, subsample=3, right_context=2, left_context=1)
    assert chunk_horizon_raw(cfg) == (6, 6 * 3 + 2)
    assert chunk_horizon_raw(_cfg(chunk_frames=8, lookahead_frames=4)) == (12, 12)           # no subsample key: factor 1
    assert chunk_horizon_raw(_cfg(chunk_frames=8, lookahead_frames=4, subsample=0, num_layers=1)) == (4, 4)
    assert chunk_info_line(_cfg()) is None and chunk_info_line(_cfg(chunk_frames=0)) is None
    spec = importlib.util.spec_from_file_location("_common_for_lc_blstm_test", os.path.join(ROOT, "bin", "_common.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.report_chunking(_cfg())
    assert "latency" not in capsys.readouterr().err
    mod.report_chunking(cfg)
    lines = [l for l in capsys.readouterr().err.splitlines() if "latency-controlled" in l]
    assert len(lines) == 1 and lines[0].startswith("INFO:tensorflow:"), lines
    for word in ("chunk_frames = 4", "lookahead_frames = 2", "2 layers", "6 model frames", "20 raw frames"):
        assert word in lines[0], (word, lines[0])
    with pytest.raises(SystemExit):
        mod.report_chunking(_cfg(chunk_frames=4, nnet_type="lstm"))
    assert "FATAL:tensorflow:" in capsys.readouterr().err


def test_chunk_lengths_agree_with_a_loop():
    from lstm_ctc_amd import ops
    for T, Nc, Nr, lens in ((11, 4, 2, [11, 8, 6, 4, 1]), (11, 4, 9, [11, 0, 3]), (12, 4, 0, [12, 4]), (5, 16, 3, [5, 2]),
                            (1, 1, 0, [1, 0])):
        nC, Tc, Bc = ops.chunk_shape(T, len(lens), Nc, Nr)
        assert (nC, Tc, Bc) == (-(-T // Nc), min(Nc + Nr, T), -(-T // Nc) * len(lens))
        got = ops.chunk_lengths(torch.tensor(lens, dtype=torch.int32), T, Nc, Nr)
        want = [min(max(n - c * Nc, 0), Tc) for c in range(nC) for n in lens]
        assert got.dtype == torch.int32 and got.is_contiguous() and got.tolist() == want
    for bad in ((0, 2, 4, 0), (4, 0, 4, 0), (4, 2, 0, 0), (4, 2, 4, -1)):
        with pytest.raises(ValueError):
            ops.chunk_shape(*bad)


# ---------------------------------------------------------------------------------------------- the library
def test_library_exports_the_entry_points_and_refuses_bad_arguments():
    """The header's two symbols are in the built library and in the binding; LC_EINVAL comes before any launch, so every
    rejection can be seen without a GPU (the pointers are never dereferenced)."""
    import __graft_entry__ as g
    g.build()
    from lstm_ctc_amd import _lib
    header = open(os.path.join(ROOT, "include", "lstm_ctc_hip.h")).read()
    assert "int lc_chunk_gather(const float *x, int ldx, int T, int B, int C, int chunk, int lookahead, int zero_lookahead" in header
    assert "int lc_chunk_fold(const float *xc, int ldc, int T, int B, int C, int chunk, int lookahead, int sum_copies" in header
    assert len(_lib.SIGNATURES["lc_chunk_gather"][1]) == 11 and len(_lib.SIGNATURES["lc_chunk_fold"][1]) == 12
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "lc_chunk_gather") and hasattr(raw, "lc_chunk_fold")
    lib = _lib.load()
    assert lib.lc_version() >= 9

    def call(fold, x=4096, ldx=8, T=6, B=2, C=8, chunk=2, lookahead=1, out=4096, ldo=8):
        if fold:
            return lib.lc_chunk_fold(x, ldx, T, B, C, chunk, lookahead, 1, None, out, ldo, None)
        return lib.lc_chunk_gather(x, ldx, T, B, C, chunk, lookahead, 0, out, ldo, None)

    for fold in (0, 1):
        for kw in (dict(T=0), dict(B=0), dict(C=0), dict(T=-3), dict(chunk=0), dict(chunk=-1), dict(lookahead=-1), dict(x=None),
                   dict(out=None), dict(ldx=7), dict(ldo=7)):
            assert call(fold, **kw) == -1, (fold, kw)
            assert (b"lc_chunk_fold" if fold else b"lc_chunk_gather") in lib.lc_last_error()
