"""Host tests of the pyramidal BiLSTM (nnet.config keys time_reduce_layers / time_reduce_factor): the config
rules and refusals, the length arithmetic, the INFO line, the parameter store, the numpy statement of the two passes (adjoint
of each other), the float64 reference the GPU tests use, and the library's entry points and their argument checks.  None needs
a GPU."""
import ctypes
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import time_reduce_reference as ref  # noqa: E402


def _cfg(**kw):
    cfg = dict(nnet_type="blstm", input_dim=10, left_context=0, right_context=0, num_layers=3, num_neurons=32,
               num_projects=16, num_targets=9, use_peepholes=True, dropout_rate=1.0)
    cfg.update(kw)
    return cfg


# ---------------------------------------------------------------------------------------------- config
def test_config_rules():
    from lstm_ctc_amd.nnet.model import time_reduce_config
    assert time_reduce_config(_cfg()) == ((), 2)
    assert time_reduce_config(_cfg(time_reduce_layers=0)) == ((), 2)
    assert time_reduce_config(_cfg(time_reduce_layers=0, time_reduce_factor=3)) == ((), 2)     # the factor is not read
    assert time_reduce_config(_cfg(time_reduce_layers=0, time_reduce_factor=99)) == ((), 2)
    assert time_reduce_config(_cfg(time_reduce_layers=1)) == ((1,), 2)
    assert time_reduce_config(_cfg(time_reduce_layers=2, time_reduce_factor=3)) == ((2,), 3)
    assert time_reduce_config(_cfg(time_reduce_layers="1,2", time_reduce_factor=4)) == ((1, 2), 4)
    assert time_reduce_config(_cfg(time_reduce_layers="2")) == ((2,), 2)
    assert time_reduce_config(_cfg(num_layers=5, time_reduce_layers="1,3")) == ((1, 3), 2)
    for bad in (3, -1, "0", "0,1", "2,1", "1,1", "1,3", "1,,2", "a", "", 1.5, True, "1;2"):
        with pytest.raises(ValueError, match="time_reduce_layers"):
            time_reduce_config(_cfg(time_reduce_layers=bad))
    for bad in (1, 5, 0, -2, 2.0, "2", True):
        with pytest.raises(ValueError, match="time_reduce_factor"):
            time_reduce_config(_cfg(time_reduce_layers=1, time_reduce_factor=bad))


def test_config_as_parse_config_delivers_it(tmp_path):
    from lstm_ctc_amd.nnet.config import parse_config
    from lstm_ctc_amd.nnet.model import time_reduce_config
    for text, want in (("time_reduce_layers = 2\n", ((2,), 2)), ("time_reduce_layers = 1,2\ntime_reduce_factor = 3\n", ((1, 2), 3)),
                       ("time_reduce_layers = 0\n", ((), 2)), ("", ((), 2))):
        fn = tmp_path / "nnet.config"
        fn.write_text("num_layers = 3\nnnet_type = blstm\n" + text)
        assert time_reduce_config(parse_config(str(fn))) == want


@pytest.mark.parametrize("extra", [dict(nnet_type="lstm"), dict(nnet_type="cudnnlstm", num_projects=None),
                                   dict(compute_dtype="bf16"), dict(compute_dtype="bf16x3"), dict(chunk_frames=4),
                                   dict(chunk_frames=4, lookahead_frames=2)])
def test_what_cannot_run_it_is_refused(extra):
    from lstm_ctc_amd.nnet.model import ParamStore, time_reduce_config
    with pytest.raises(ValueError, match="time_reduce_layers"):
        time_reduce_config(_cfg(time_reduce_layers=1, **extra))
    with pytest.raises(ValueError, match="time_reduce_layers"):
        ParamStore(_cfg(time_reduce_layers=1, **extra), "cpu")
    time_reduce_config(_cfg(time_reduce_layers=0, **{k: v for k, v in extra.items() if k != "num_projects"}))    # off: nothing to refuse


# ---------------------------------------------------------------------------------------------- lengths
def test_length_arithmetic_agrees_with_a_loop():
    from lstm_ctc_amd import ops
    from lstm_ctc_amd.nnet.model import Model  # noqa: F401  (importable without a GPU)
    for r in (2, 3, 4):
        n = np.arange(0, 200, dtype=np.int32)
        want = np.array([len(range(0, int(v), r)) for v in n], np.int32)          # groups of r frames, the last one cut short
        got = ops.time_reduce_lengths(n, r)
        assert got.dtype == np.int32 and np.array_equal(got, want)
        on_torch = ops.time_reduce_lengths(torch.from_numpy(n), r)
        assert on_torch.dtype == torch.int32 and np.array_equal(on_torch.numpy(), want)
        twice = ops.time_reduce_lengths(got, r)
        assert np.array_equal(twice, -(-n.astype(np.int64) // (r * r)))            # ceil(ceil(n / r) / r) == ceil(n / r^2)
        assert all(ops.time_reduce_frames(int(v), r) == int(w) for v, w in zip(n, want))
    with pytest.raises(ValueError):
        ops.time_reduce_lengths(np.arange(3), 0)


def test_output_lengths_of_a_model_shaped_object():
    """Model.output_frames / output_lengths need no device: call them unbound on a stand-in."""
    from types import SimpleNamespace
    from lstm_ctc_amd.nnet.model import Model
    m = SimpleNamespace(time_reduce=(1, 2), time_reduce_factor=2)
    assert Model.output_frames(m, 11) == 3 and Model.output_frames(m, 1) == 1 and Model.output_frames(m, 8) == 2
    assert Model.output_lengths(m, np.array([11, 8, 6, 4, 1, 0], np.int32)).tolist() == [3, 2, 2, 1, 1, 0]
    got = Model.output_lengths(m, torch.tensor([11, 8, 6, 4, 1, 0], dtype=torch.int32))
    assert torch.is_tensor(got) and got.dtype == torch.int32 and got.tolist() == [3, 2, 2, 1, 1, 0]
    off = SimpleNamespace(time_reduce=(), time_reduce_factor=2)
    seq = np.array([5, 3], np.int32)
    assert Model.output_lengths(off, seq) is seq and Model.output_frames(off, 7) == 7


def test_info_line():
    from lstm_ctc_amd.nnet.model import time_reduce_info_line
    assert time_reduce_info_line(_cfg()) is None and time_reduce_info_line(_cfg(time_reduce_layers=0)) is None
    line = time_reduce_info_line(_cfg(num_layers=5, time_reduce_layers="1,3", subsample=2))
    assert line == ("pyramidal BiLSTM: time_reduce_layers = 1,3, time_reduce_factor = 2: R = 4, the logits come once per 4 model "
                    "frames (8 raw frames)")
    line = time_reduce_info_line(_cfg(time_reduce_layers=2, time_reduce_factor=3))
    assert "time_reduce_layers = 2, time_reduce_factor = 3: R = 3" in line and "(3 raw frames)" in line


def test_report_time_reduce_prints_one_line_and_refuses_tables(capsys):
    from types import SimpleNamespace
    spec = importlib.util.spec_from_file_location("_common_under_test", os.path.join(ROOT, "bin", "_common.py"))
    common = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(common)
    common.report_time_reduce(_cfg())                                   # off: silent
    assert "pyramidal" not in capsys.readouterr().err
    plain = SimpleNamespace(frame_targets=None, align_window=None, teacher_scores=None, objective="ctc")
    common.report_time_reduce(_cfg(time_reduce_layers=1, subsample=2), plain)
    err = capsys.readouterr().err
    assert err.count("pyramidal BiLSTM") == 1 and "(4 raw frames)" in err
    for bad in (dict(frame_targets="ark:x"), dict(align_window=3, frame_targets="ark:x"), dict(teacher_scores="ark:x"),
                dict(objective="xent"), dict(objective="kd")):
        with pytest.raises(SystemExit) as exc:
            common.report_time_reduce(_cfg(time_reduce_layers=1), SimpleNamespace(**dict(vars(plain), **bad)))
        assert exc.value.code == 1 and "time_reduce_layers" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        common.report_time_reduce(_cfg(time_reduce_layers=1), aligning=True)
    with pytest.raises(SystemExit):
        common.report_time_reduce(_cfg(time_reduce_layers=1, nnet_type="lstm"))


def test_short_utterances_are_counted_from_the_host_labels():
    """labels + adjacent repeats > output length; each utterance once under a doubled (consistency) batch; 0 without host
    copies."""
    from types import SimpleNamespace
    from lstm_ctc_amd import ops
    from lstm_ctc_amd.nnet.graph import CTCGraph
    out_len = lambda s: ops.time_reduce_lengths(s, 2)      # noqa: E731
    flat = np.array([1, 1, 1,  2, 3,  4, 4,  5], np.int32)             # needs 5, 2, 3, 1 frames
    offs = np.array([0, 3, 5, 7, 8], np.int32)
    seq = np.array([9, 3, 4, 0], np.int32)                             # 5, 2, 2, 0 output frames: the last two are short
    b = SimpleNamespace(flat=flat, offs=offs, seq=seq, pairs=None)
    assert CTCGraph._time_reduce_short(b, out_len) == 2
    assert CTCGraph._time_reduce_short(SimpleNamespace(**dict(vars(b), seq=seq + 2)), out_len) == 0
    doubled = SimpleNamespace(flat=np.concatenate([flat, flat]), offs=np.concatenate([offs, offs[1:] + 8]),
                              seq=np.concatenate([seq, seq]), pairs=torch.from_numpy(seq))
    assert CTCGraph._time_reduce_short(doubled, out_len) == 2
    assert CTCGraph._time_reduce_short(SimpleNamespace(flat=None, offs=None, seq=seq, pairs=None), out_len) == 0


# ---------------------------------------------------------------------------------------------- parameters
def test_param_store_widens_the_reduced_layers_only():
    from lstm_ctc_amd.nnet.model import ParamStore
    plain = ParamStore(_cfg(), "cpu")
    pyr = ParamStore(_cfg(time_reduce_layers="1,2", time_reduce_factor=3), "cpu")
    one = ParamStore(_cfg(time_reduce_layers=2), "cpu")
    assert pyr.names() == plain.names() == one.names()
    P, N = 16, 32
    for pre in ("fd%d/frnn%d", "bd%d/brnn%d"):
        assert pyr.shapes[pre % (0, 0) + "/kernel"] == plain.shapes[pre % (0, 0) + "/kernel"] == (10 + P, 4 * N)
        assert plain.shapes[pre % (1, 1) + "/kernel"] == (2 * P + P, 4 * N)
        assert pyr.shapes[pre % (1, 1) + "/kernel"] == pyr.shapes[pre % (2, 2) + "/kernel"] == (3 * 2 * P + P, 4 * N)
        assert one.shapes[pre % (1, 1) + "/kernel"] == (2 * P + P, 4 * N)
        assert one.shapes[pre % (2, 2) + "/kernel"] == (2 * 2 * P + P, 4 * N)
    for name in plain.names():
        if not name.endswith("/kernel") or name.startswith(("fd0", "bd0")):
            assert pyr.shapes[name] == plain.shapes[name], name
    # off, in all three spellings: the plain layout to the offset
    for off in (_cfg(time_reduce_layers=0), _cfg(time_reduce_layers=0, time_reduce_factor=4)):
        ps = ParamStore(off, "cpu")
        assert ps.offsets == plain.offsets and ps.shapes == plain.shapes and ps.n == plain.n and ps.n_decay == plain.n_decay


def test_a_plain_checkpoint_does_not_fit_and_load_tf_says_which_variable():
    from lstm_ctc_amd.nnet.model import ParamStore
    plain = ParamStore(_cfg(), "cpu")
    plain.init_random(1)
    pyr = ParamStore(_cfg(time_reduce_layers=2), "cpu")
    before = pyr.flat.clone()
    with pytest.raises(ValueError) as exc:
        pyr.load_tf(plain.export_tf())
    msg = str(exc.value)
    assert "fd2/frnn2/kernel" in msg and "(48, 128)" in msg and "(80, 128)" in msg and "time_reduce_layers" in msg
    assert pyr.flat.shape == before.shape
    pyr.init_random(2)
    again = ParamStore(_cfg(time_reduce_layers=2), "cpu")
    again.load_tf(pyr.export_tf())                                       # its own checkpoint fits
    assert torch.equal(again.flat, pyr.flat)


# ---------------------------------------------------------------------------------------------- the statement of the passes
LENS = lambda T, r: [0, 1, r - 1, r, r + 1, T - 1, T, T + 3]      # noqa: E731


@pytest.mark.parametrize("T,C,r", [(7, 5, 2), (10, 3, 3), (9, 2, 4), (1, 3, 2), (3, 2, 4), (8, 1, 2)])
def test_bwd_is_the_adjoint_of_fwd(T, C, r):
    """<fwd(x), dy> == <x, bwd(dy)> exactly, on integer-valued float64 data with the dead frames zeroed."""
    rng = np.random.default_rng(T * 10 + r)
    lens = LENS(T, r)
    B = len(lens)
    To = ref.cdiv(T, r)
    x = rng.integers(-9, 10, size=(T, B, C)).astype(np.float64)
    dy = rng.integers(-9, 10, size=(To, B, r * C)).astype(np.float64)
    for b in range(B):
        x[min(max(lens[b], 0), T):, b] = 0
    y, dx = ref.np_time_reduce_fwd(x, lens, r), ref.np_time_reduce_bwd(dy, lens, r, T)
    assert y.shape == (To, B, r * C) and dx.shape == (T, B, C)
    assert float((y * dy).sum()) == float((x * dx).sum())
    # bwd(fwd(x)) is x on live frames, +0 elsewhere; and the torch form the reference model uses says the same
    assert np.array_equal(ref.np_time_reduce_bwd(y, lens, r, T), x)
    assert np.array_equal(ref.torch_time_reduce(torch.from_numpy(x), torch.tensor(lens).clamp(0, T), r).numpy(), y)
    # dead frames are never read
    xn = x.copy()
    for b in range(B):
        xn[min(max(lens[b], 0), T):, b] = np.nan
    assert np.array_equal(ref.np_time_reduce_fwd(xn, lens, r), y)


# ---------------------------------------------------------------------------------------------- the reference is pinned
def _params(cfg, seed):
    from lstm_ctc_amd.nnet.model import ParamStore
    ps = ParamStore(cfg, "cpu")
    ps.init_random(seed)
    params = ps.export_tf()
    rng = np.random.default_rng(seed)
    for k in params:
        if "bias" in k or k == "Variable_1":
            params[k] = rng.normal(0, 0.2, size=params[k].shape).astype(np.float32)
    return {k: v.astype(np.float64) for k, v in params.items()}


def test_reference_with_the_key_off_is_blstm_forward():
    from oracle.torch_f64 import blstm_forward
    cfg = _cfg(dropout_rate=0.8)
    p = _params(cfg, 5)
    rng = np.random.default_rng(6)
    seq = np.array([11, 8, 6, 4, 1], np.int32)
    x = rng.normal(size=(11, 5, 10))
    for b in range(5):
        x[seq[b]:, b] = 0
    want = blstm_forward(p, cfg, x, seq, drop_seed=7, device="cpu")
    got = ref.pyramid_forward(p, cfg, x, seq, (), 2, drop_seed=7)
    assert torch.equal(got, want)


@pytest.mark.parametrize("layers,r", [((1,), 2), ((1, 2), 2), ((2,), 3), ((1,), 4)])
def test_reference_gives_each_utterance_what_it_gets_alone(layers, r):
    """B = 1, T = len_b alone against the ragged batch, to 1e-12: the masking, the cut-short last group and the per-layer
    lengths."""
    cfg = _cfg(time_reduce_layers=",".join(map(str, layers)), time_reduce_factor=r)
    p = _params(cfg, 8)
    rng = np.random.default_rng(9)
    seq = np.array([11, 8, 6, 4, 1], np.int32)
    T, B = 11, 5
    x = rng.normal(size=(T, B, 10))
    for b in range(B):
        x[seq[b]:, b] = 0
    batch = ref.pyramid_forward(p, cfg, x, seq, layers, r).numpy()
    out_len = ref.output_lengths(seq, layers, r)
    assert batch.shape[0] == ref.output_lengths([T], layers, r)[0]
    for b in range(B):
        alone = ref.pyramid_forward(p, cfg, x[:seq[b], b:b + 1], seq[b:b + 1], layers, r).numpy()
        assert alone.shape[0] == out_len[b]
        assert np.abs(alone[:, 0] - batch[:out_len[b], b]).max() < 1e-12, b
    # and it is another model than the plain one run on every R-th frame
    assert batch.shape != (T, B, 9)


# ---------------------------------------------------------------------------------------------- the library
def test_library_exports_the_entry_points_and_refuses_bad_arguments():
    """The header's two symbols are in the built library and in the binding; LC_EINVAL comes before any launch, so every
    rejection can be seen without a GPU (the pointers are never dereferenced)."""
    import __graft_entry__ as g
    g.build()
    from lstm_ctc_amd import _lib
    header = " ".join(open(os.path.join(ROOT, "include", "lstm_ctc_hip.h")).read().split())
    assert ("int lc_time_reduce_fwd(const float *x, int ldx, int T, int B, int C, int r, const int *seq_len, float *y, int ldy, "
            "lc_stream_t stream);") in header
    assert ("int lc_time_reduce_bwd(const float *dy, int lddy, int T, int B, int C, int r, const int *seq_len, float *dx, "
            "int lddx, lc_stream_t stream);") in header
    assert "no reference counterpart" in header.split("time reduction")[1][:400]
    assert [len(_lib.SIGNATURES[n][1]) for n in ("lc_time_reduce_fwd", "lc_time_reduce_bwd")] == [10, 10]
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(raw, n) for n in ("lc_time_reduce_fwd", "lc_time_reduce_bwd"))
    lib = _lib.load()
    assert lib.lc_version() >= 13
    T, B, C, r = 7, 2, 8, 2
    To = 4
    # far apart, 16-byte aligned made-up addresses
    X, Y, L = 0x100000, 0x200000, 0x300000

    def fwd(x=X, ldx=C, T=T, B=B, C=C, r=r, seq_len=L, y=Y, ldy=r * C):
        return lib.lc_time_reduce_fwd(x, ldx, T, B, C, r, seq_len, y, ldy, None)

    def bwd(dy=Y, lddy=r * C, T=T, B=B, C=C, r=r, seq_len=L, dx=X, lddx=C):
        return lib.lc_time_reduce_bwd(dy, lddy, T, B, C, r, seq_len, dx, lddx, None)

    x_bytes, y_bytes = 4 * T * B * C, 4 * To * B * r * C
    for kw in (dict(T=0), dict(B=0), dict(C=0), dict(T=-3), dict(B=-1), dict(C=-1), dict(r=1), dict(r=0), dict(r=5), dict(r=-2),
               dict(x=None), dict(seq_len=None), dict(y=None), dict(ldx=C - 1), dict(ldy=r * C - 1), dict(ldy=C),
               dict(y=X), dict(y=X + x_bytes - 4), dict(y=X - y_bytes + 4)):
        assert fwd(**kw) == -1, kw
        assert b"lc_time_reduce_fwd" in lib.lc_last_error()
    for kw in (dict(T=0), dict(B=0), dict(C=0), dict(r=1), dict(r=5), dict(dy=None), dict(seq_len=None), dict(dx=None),
               dict(lddx=C - 1), dict(lddy=r * C - 1), dict(dx=Y), dict(dx=Y + y_bytes - 4), dict(dx=Y - x_bytes + 4)):
        assert bwd(**kw) == -1, kw
        assert b"lc_time_reduce_bwd" in lib.lc_last_error()
