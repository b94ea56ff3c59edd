"""Host side of SpecAugment: the draws (known answers and properties), the numpy reference of the pass, the command-line form,
the --spec-augment flag of nnet-train, the graph keyword's validation and the library entry.  No GPU needed."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from lstm_ctc_amd.nnet import augment  # noqa: E402
from lstm_ctc_amd.nnet.augment import SpecAugment, apply_host, mask_plan, parse_spec  # noqa: E402


# ----------------------------------------------------------------------------------------------- the draws
def test_hash_known_answers():
    h = lambda seed, k: int(augment.hash_u32(seed, augment.STREAM, k))
    assert augment.STREAM == 0x53504543
    assert h(777, 0) == 0xa6e4d3b9 and h(777, 33) == 0x6007bfd4 and h(0, 2 ** 32 + 5) == 0x7a3bf685
    got = augment.hash_u32(777, augment.STREAM, np.array([[0, 33], [33, 0]]))                  # any shape, uint32 out
    assert got.dtype == np.uint32 and got.tolist() == [[0xa6e4d3b9, 0x6007bfd4], [0x6007bfd4, 0xa6e4d3b9]]


def test_mask_plan_known_answers():
    spec = SpecAugment(time_masks=2, time_width=6, time_percent=40, freq_masks=2, freq_width=3, freq_bins=8)
    plan = mask_plan(777, [9, 7, 4, 1, 0], spec, 3)
    assert plan.dtype == np.int32 and plan.shape == (5, 16, 2)
    assert plan[:, :2].tolist() == [[[16, 4], [4, 1]], [[6, 4], [16, 0]], [[8, 0], [4, 1]], [[0, 0], [1, 0]], [[0, 0], [0, 0]]]
    assert plan[:, 8:10].tolist() == [[[3, 1], [3, 2]], [[5, 1], [7, 0]], [[5, 2], [8, 0]], [[4, 2], [4, 2]], [[3, 0], [4, 0]]]
    assert not plan[:, 2:8].any() and not plan[:, 10:].any()                                  # unused rows are (0, 0)
    spec = SpecAugment(time_masks=2, time_width=4, time_percent=100, freq_masks=1, freq_width=2, freq_bins=4)
    for subsample in (1, 0, None):                                                            # 0 / None: no subsampling
        plan = mask_plan(5, [12, 5, 2], spec, subsample)
        assert plan[:, :2].tolist() == [[[1, 2], [1, 4]], [[0, 0], [2, 0]], [[0, 2], [0, 0]]]
        assert plan[:, 8].tolist() == [[0, 2], [3, 1], [0, 0]]
        assert not plan[:, 2:8].any() and not plan[:, 9:].any()


def test_mask_plan_properties_over_seeds():
    rng = np.random.default_rng(0)
    seq = np.array([0, 1, 2, 3, 17, 100, 1, 0, 999], np.int32)
    for seed in range(300):
        tm, fm = int(rng.integers(0, 9)), int(rng.integers(0, 9))
        F = int(rng.integers(1, 41))
        spec = SpecAugment(time_masks=tm, time_width=int(rng.integers(0, 50)), time_percent=int(rng.integers(0, 101)),
                           freq_masks=fm, freq_width=int(rng.integers(0, F + 1)), freq_bins=F)
        s = int(rng.integers(0, 4))
        plan = mask_plan(seed * 7919 + 1, seq, spec, s).astype(np.int64)
        n = seq.astype(np.int64) * max(s, 1)
        t0, tw, f0, fw = plan[:, :8, 0], plan[:, :8, 1], plan[:, 8:, 0], plan[:, 8:, 1]
        assert (t0 >= 0).all() and (tw >= 0).all() and (t0 + tw <= n[:, None]).all()            # inside [0, n)
        assert (tw <= spec.time_width).all() and (tw <= (n * spec.time_percent // 100)[:, None]).all()   # both caps
        assert (f0 >= 0).all() and (fw >= 0).all() and (f0 + fw <= F).all() and (fw <= spec.freq_width).all()
        assert not plan[:, tm:8].any() and not plan[:, 8 + fm:].any()
        assert not plan[seq == 0, :8].any()                                                   # nothing to mask in no frames
        # a pure function of (seed, b): another batch composition draws the same masks for the same slot
        assert np.array_equal(mask_plan(seed * 7919 + 1, seq[:4], spec, s), plan[:4])
    # the draws do reach both ends of their ranges
    spec = SpecAugment(time_masks=8, time_width=3, freq_masks=8, freq_width=2, freq_bins=3)
    plans = np.stack([mask_plan(seed, [4], spec, 1)[0] for seed in range(300)])
    assert set(plans[:, :8, 1].ravel()) == {0, 1, 2, 3} and set(plans[:, 8:, 1].ravel()) == {0, 1, 2}
    assert plans[:, :8].sum(axis=2).max() == 4 and plans[:, 8:].sum(axis=2).max() == 3


# ----------------------------------------------------------------------------------------------- the pass
def _plan(time=(), freq=(), B=1):
    plan = np.zeros((B, 16, 2), np.int32)
    for b in range(B):
        for j, m in enumerate(time):
            plan[b, j] = m
        for j, m in enumerate(freq):
            plan[b, 8 + j] = m
    return plan


def _spliced(T_raw, base_dim, l, r, s):
    """The loader's matrix for raw frames whose every element holds its frame number * 1000 + its column."""
    from lstm_ctc_amd.nnet.tfrecord import splice, subsample
    raw = (np.arange(T_raw)[:, None] * 1000 + np.arange(base_dim)[None, :]).astype(np.float32)
    x = splice(raw, l, r)
    return subsample(x, s) if s > 1 else x


def test_apply_host_rows_show_disjoint_frames_under_the_recipe_layout():
    """l = r = 1, s = 3: row t shows raw frames 3t-1 .. 3t+1 (clamped at the edges), each raw frame in exactly one place."""
    l = r = 1
    s, base = 3, 4
    x = _spliced(12, base, l, r, s)[:, None, :]                                 # [4, 1, 12]
    spec = SpecAugment(time_masks=1, time_width=12, freq_bins=4, fill=-7.0)
    # frame 11 is the one no row shows: row 3 ends at 3 * 3 + 1 = 10
    assert np.array_equal(apply_host(x, [4], _plan(time=[(11, 1)]), spec, base, l, r, s), x)
    for frame in range(11):
        out = apply_host(x, [4], _plan(time=[(frame, 1)]), spec, base, l, r, s)
        hit = out != x
        shown = (x // 1000).astype(int)
        assert np.array_equal(hit, shown == frame) and (out[hit] == -7.0).all()
        # frame 0 is also what the first row's left context shows (the edge copy)
        assert hit.sum() == base * (2 if frame == 0 else 1)
        assert np.count_nonzero(hit.any(axis=2)) == 1                           # one row only


def test_apply_host_removes_a_frame_from_every_row_that_shows_it():
    """l = r = 2, s = 1: raw frame 5 of 10 is shown by rows 3 .. 7, in blocks 4 .. 0."""
    l = r = 2
    base = 3
    x = _spliced(10, base, l, r, 1)[:, None, :]                                 # [10, 1, 15]
    spec = SpecAugment(time_masks=1, time_width=10, freq_bins=3, fill=0.5)
    out = apply_host(x, [10], _plan(time=[(5, 1)]), spec, base, l, r, 1)
    shown = (x // 1000).astype(int)
    assert np.array_equal(out != x, shown == 5) and not (out // 1000 == 5).any()
    rows = np.nonzero((out != x).any(axis=2)[:, 0])[0]
    assert rows.tolist() == [3, 4, 5, 6, 7]
    for t in rows:
        block = 5 - t + l
        assert np.array_equal(np.nonzero(out[t, 0] == 0.5)[0], np.arange(block * base, (block + 1) * base))
    # the edge copies go with their frame: frame 0 also fills the left context of rows 0 and 1, frame 9 the right of 8, 9
    spec = SpecAugment(time_masks=2, time_width=10, freq_bins=3, fill=0.5)
    out = apply_host(x, [10], _plan(time=[(0, 1), (9, 1)]), spec, base, l, r, 1)
    assert np.array_equal(out != x, (shown == 0) | (shown == 9))
    assert (out[0, 0, :3 * base] == 0.5).all() and (out[9, 0, 2 * base:] == 0.5).all()


def test_apply_host_masks_a_bin_in_every_group_and_block():
    l, r, s, F, base = 1, 1, 1, 4, 12                                           # three feature groups of four bins
    rng = np.random.default_rng(1)
    x = rng.standard_normal((5, 2, base * 3)).astype(np.float32)
    spec = SpecAugment(freq_masks=2, freq_width=4, freq_bins=F, fill=9.0)
    out = apply_host(x, [5, 5], _plan(freq=[(1, 2), (2, 1)], B=2), spec, base, l, r, s)
    cols = np.arange(base * 3)
    want = np.isin((cols % base) % F, [1, 2])
    assert want.sum() == 2 * 3 * 3
    assert np.array_equal(out != x, np.broadcast_to(want, x.shape)) and (out[..., want] == 9.0).all()
    with pytest.raises(ValueError):
        apply_host(x, [5, 5], _plan(B=2), SpecAugment(freq_bins=5), base, l, r, s)          # 5 does not divide 12
    with pytest.raises(ValueError):
        apply_host(x, [5, 5], _plan(B=2), spec, base, l, 0, s)                               # D is not base * (1 + l + r)


def test_apply_host_leaves_padding_rows_alone():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((6, 3, 8)).astype(np.float32)
    x[5, 0, 3] = np.nan
    spec = SpecAugment(time_masks=1, time_width=99, freq_masks=1, freq_width=8, freq_bins=8, fill=1.0)
    seq = [4, 0, 6]
    keep = x.copy()
    out = apply_host(x, seq, _plan(time=[(0, 99)], freq=[(0, 8)], B=3), spec, 8, 0, 0, 2)
    assert np.array_equal(x.view(np.uint32), keep.view(np.uint32))              # the input is not written
    for b, n in enumerate(seq):
        assert (out[:n, b] == 1.0).all()
        assert np.array_equal(out[n:, b].view(np.uint32), x[n:, b].view(np.uint32))           # bit for bit, the NaN too
    # nothing drawn, nothing changed
    none = apply_host(x, seq, mask_plan(3, seq, SpecAugment(freq_bins=8), 2), SpecAugment(freq_bins=8), 8, 0, 0, 2)
    assert np.array_equal(none.view(np.uint32), x.view(np.uint32))


# ----------------------------------------------------------------------------------------------- settings and their text
def test_parse_spec_round_trips():
    spec = parse_spec("time=2x40,freq=2x15,bins=40,cap=20")
    assert spec == SpecAugment(time_masks=2, time_width=40, time_percent=20, freq_masks=2, freq_width=15, freq_bins=40, fill=0.0)
    assert (spec.time_masks, spec.time_width, spec.time_percent, spec.freq_masks, spec.freq_width, spec.freq_bins,
            spec.fill) == (2, 40, 20, 2, 15, 40, 0.0)
    assert parse_spec("time=2x40,freq=2x15,bins=40").time_percent == 100
    assert parse_spec(" bins = 40 , fill = -1.5 ,freq=1x0") == SpecAugment(freq_masks=1, freq_width=0, freq_bins=40, fill=-1.5)
    for text in ("time=2x40,freq=2x15,bins=40,cap=20", "bins=8", "time=8x0,freq=0x8,bins=8,cap=0,fill=1e-3",
                 "fill=0.1,bins=3,freq=1x3"):
        spec = parse_spec(text)
        assert parse_spec(str(spec)) == spec and hash(parse_spec(str(spec))) == hash(spec)
    assert parse_spec("bins=3,fill=0.1").fill == float(np.float32(0.1))                      # what the kernel will write
    with pytest.raises(AttributeError):
        spec.fill = 2.0
    with pytest.raises(AttributeError):
        del spec.fill


@pytest.mark.parametrize("text", [
    "", " ", "time=2x40", "time=2x40,freq=2x15", "bins=40,bins=40", "bins=40,warp=5", "bins", "bins=", "=40", "bins=40,",
    "time=2,bins=40", "time=2x,bins=40", "time=x4,bins=40", "time=2x4x6,bins=40", "time=-1x4,bins=40", "time=2x-4,bins=40",
    "time=2.5x4,bins=40", "time=9x4,bins=40", "freq=9x4,bins=40", "freq=1x41,bins=40", "bins=0", "bins=-8", "bins=4.0",
    "bins=40,cap=101", "bins=40,cap=-1", "bins=40,cap=5.5", "bins=40,fill=nan", "bins=40,fill=inf", "bins=40,fill=-inf",
    "bins=40,fill=1e39", "bins=40,fill=zero", "time=2x40;freq=2x15;bins=40", "time=99999999999x1,bins=40"])
def test_parse_spec_rejects(text):
    with pytest.raises(ValueError):
        parse_spec(text)


def test_spec_augment_validates():
    ok = dict(time_masks=2, time_width=40, time_percent=20, freq_masks=2, freq_width=15, freq_bins=40, fill=0.0)
    SpecAugment(**ok)
    for bad in (dict(time_masks=9), dict(time_masks=-1), dict(freq_masks=9), dict(freq_masks=-1), dict(time_width=-1),
                dict(freq_width=-1), dict(freq_width=41), dict(time_percent=101), dict(time_percent=-1), dict(freq_bins=0),
                dict(freq_bins=None), dict(fill=float("nan")), dict(fill=float("inf")), dict(fill=1e39), dict(fill="0"),
                dict(time_masks=2.0), dict(time_masks=True), dict(time_width=2 ** 31), dict(fill=None)):
        with pytest.raises(ValueError):
            SpecAugment(**dict(ok, **bad))
    with pytest.raises(ValueError):
        SpecAugment(time_masks=1, time_width=3)                                  # freq_bins is required
    SpecAugment(**ok).check_layout(120)
    with pytest.raises(ValueError):
        SpecAugment(**ok).check_layout(100)
    assert augment.layout_of(dict(input_dim=120, left_context=1, right_context=1, subsample=3)) == (120, 1, 1, 3)
    assert augment.layout_of(dict(input_dim=40, left_context=None)) == (40, 0, 0, 0)


def test_masked_shares_count_overlaps_once():
    spec = SpecAugment(time_masks=2, time_width=9, freq_masks=2, freq_width=4, freq_bins=4)
    plan = _plan(time=[(2, 4), (4, 4)], freq=[(0, 2), (1, 1)], B=2)
    plan[1] = 0
    assert augment.masked_shares(plan, [5, 3], spec, 2) == (6, 16, 2, 8)


# ----------------------------------------------------------------------------------------------- the command line
def _run(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "nnet-train.py")] + list(args), capture_output=True,
                       timeout=120)
    return r.returncode, r.stderr.decode(), r.stdout.decode()


def _fatal(err):
    return [line for line in err.splitlines() if line.startswith("FATAL:tensorflow:")]


def _argv(tmp_path, config="nnet.config"):
    scp = tmp_path / "t.scp"
    scp.write_text("utt0 5 3 0 %s\n" % (tmp_path / "utt0.tfrecords"))
    return [str(scp), str(config), "nnet.in", "nnet.out"]


@pytest.mark.parametrize("value", ["time=2x40", "time=2,bins=40", "bins=40,warp=5", "freq=1x41,bins=40", "bins=40,cap=101",
                                   "bins=40,fill=nan", "time=9x4,bins=40"])
def test_cli_malformed_spec_augment_is_fatal_before_the_device(value, tmp_path):
    rc, err, _ = _run("--objective", "ctc", "--spec-augment", value, *_argv(tmp_path))
    fatal = _fatal(err)
    assert rc == 1 and len(fatal) == 1, err
    assert "--spec-augment" in fatal[0] and "no GPU" not in fatal[0] and "Traceback" not in err, err


def test_cli_bins_must_divide_the_configs_input_dim(tmp_path):
    config = tmp_path / "nnet.config"
    config.write_text("nnet_type = blstm\ninput_dim = 120\nleft_context = 1\nright_context = 1\nsubsample = 3\n")
    rc, err, _ = _run("--objective", "ctc", "--spec-augment", "time=2x40,freq=2x15,bins=50", *_argv(tmp_path, config))
    fatal = _fatal(err)
    assert rc == 1 and len(fatal) == 1 and "--spec-augment" in fatal[0] and "120" in fatal[0] and "no GPU" not in fatal[0], err


def test_cli_help_lists_the_flag_for_nnet_train_only():
    rc, _, out = _run("--help")
    assert rc == 0 and "--spec-augment" in out and "bins=F" in out
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "nnet-validate.py"), "--help"], capture_output=True,
                       timeout=120)
    assert r.returncode == 0 and "--spec-augment" not in r.stdout.decode()


def test_spec_augment_keywords_and_report_line(tmp_path, capsys):
    import importlib.util
    mod_spec = importlib.util.spec_from_file_location("_common_for_specaug_test", os.path.join(ROOT, "bin", "_common.py"))
    mod = importlib.util.module_from_spec(mod_spec)
    mod_spec.loader.exec_module(mod)
    assert mod.FLAGS["--spec-augment"]["default"] is None
    cli = mod.build_cli(("nnet_config",), ("--spec-augment",))
    assert mod.spec_augment_keywords(cli.parse_args(["missing.config"])) == {}
    kw = mod.spec_augment_keywords(cli.parse_args(["missing.config", "--spec-augment", "time=2x40,freq=2x15,bins=40,cap=20"]))
    assert kw == {"spec_augment": parse_spec("time=2x40,freq=2x15,bins=40,cap=20")}

    class Graph:
        spec_augment = kw["spec_augment"]
        specaug_steps, specaug_frames_masked, specaug_frames, specaug_bins_masked, specaug_bins = 7, 250, 1000, 30, 120
    mod.report_spec_augment(Graph())
    line = [l for l in capsys.readouterr().err.splitlines() if "spec augment" in l]
    assert len(line) == 1 and line[0].startswith("INFO:tensorflow:"), line
    assert "time=2x40,freq=2x15,bins=40,cap=20" in line[0] and "7 step(s)" in line[0]
    assert "25.00% of 1000 live raw frame(s)" in line[0] and "25.00% of the bins" in line[0]


# ----------------------------------------------------------------------------------------------- graph and library
def test_training_factories_take_the_keyword_and_validation_ones_do_not():
    import inspect
    import lstm_ctc_amd.nnet as nnet
    from lstm_ctc_amd.nnet import graph
    for name in ("create_graph_for_training_ctc", "create_graph_for_training_xent", "create_graph_for_training_kd"):
        assert inspect.signature(getattr(nnet, name)).parameters["spec_augment"].default is None
    for name in ("create_graph_for_validation_ctc", "create_graph_for_validation_xent", "create_graph_for_validation_kd",
                 "create_graph_for_alignment", "create_graph_for_inference"):
        assert "spec_augment" not in inspect.signature(getattr(nnet, name)).parameters
    assert inspect.signature(graph.CTCGraph.__init__).parameters["spec_augment"].default is None
    # refused before anything touches a device
    cfg = dict(nnet_type="blstm", input_dim=12, left_context=1, right_context=1, subsample=3)
    with pytest.raises(ValueError, match="freq_bins"):
        graph.CTCGraph(None, cfg, learn_rate=0.1, spec_augment=SpecAugment(freq_masks=1, freq_width=2, freq_bins=5))
    with pytest.raises(ValueError, match="SpecAugment"):
        graph.CTCGraph(None, cfg, learn_rate=0.1, spec_augment="time=2x40,bins=4")


def test_signatures_declare_the_entry_and_the_struct_matches_the_header():
    import ctypes
    import re
    from lstm_ctc_amd import _lib
    assert len(_lib.SIGNATURES["lc_spec_augment"][1]) == 12
    header = open(os.path.join(ROOT, "include", "lstm_ctc_hip.h")).read()
    assert "int lc_spec_augment(const float *x, int T, int B, int D, int ldx, const int *seq_len, const lc_spec_augment_t *cfg" in header
    body = re.search(r"typedef struct lc_spec_augment \{(.*?)\} lc_spec_augment_t;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.split(None, 1)[1].split(",")]
    assert names == [n for n, _ in _lib.SpecAugmentConfig._fields_]
    assert ctypes.sizeof(_lib.SpecAugmentConfig) == 44
    assert "lc_hash_u32" in open(os.path.join(ROOT, "lstm_ctc_amd", "csrc", "common.h")).read()


def test_library_version_is_at_least_7():
    from lstm_ctc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    assert _lib.load().lc_version() >= 7


def test_entry_refuses_bad_arguments_without_a_device():
    """LC_EINVAL comes before any launch, so every rejection can be seen on a box without a GPU (the pointers are never
    dereferenced: the call returns at its argument checks)."""
    import ctypes
    import __graft_entry__ as g
    g.build()
    from lstm_ctc_amd import _lib
    lib = _lib.load()
    ok = dict(time_masks=2, time_width=5, time_percent=50, freq_masks=2, freq_width=3, freq_bins=4, base_dim=8,
              left_context=1, right_context=1, subsample=3, fill=0.0)

    def call(cfg=None, T=3, B=2, D=24, ldx=24, ldo=24, x=4096, seq=4096, out=4096, null_cfg=False):
        c = _lib.SpecAugmentConfig(**dict(ok, **(cfg or {})))
        return lib.lc_spec_augment(x, T, B, D, ldx, seq, None if null_cfg else ctypes.byref(c), 1, out, ldo, None, None)

    for kw in (dict(T=0), dict(B=0), dict(D=0), dict(T=-1), dict(x=None), dict(seq=None), dict(out=None), dict(null_cfg=True),
               dict(ldx=23), dict(ldo=23), dict(D=16, ldx=16, ldo=16), dict(D=32, ldx=32, ldo=32)):
        assert call(**kw) == -1, kw
        assert b"lc_spec_augment" in lib.lc_last_error()
    for cfg in (dict(time_masks=9), dict(time_masks=-1), dict(freq_masks=9), dict(freq_masks=-1), dict(time_width=-1),
                dict(freq_width=-1), dict(time_percent=101), dict(time_percent=-1), dict(freq_bins=0), dict(freq_bins=-4),
                dict(freq_bins=3), dict(freq_width=5), dict(left_context=-1, right_context=3), dict(right_context=-1, left_context=3),
                dict(subsample=-1), dict(fill=float("nan")), dict(fill=float("inf")), dict(fill=float("-inf")),
                dict(base_dim=12), dict(left_context=2)):
        assert call(cfg=cfg) == -1, cfg
