"""Consistency-regularised CTC on the host: the float64 reference of lc_consistency_loss (``cr_ref``, which
tests/test_gpu_consistency.py imports) and its identities, the stop-gradient claim by finite differences, the doubled-batch
builder of the graph, the option's validation, the command line's fatal paths and the library's declarations.  No GPU."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------------------------- reference and bounds
def nadd(V):
    """fp32 additions a sum over a row goes through at most, in every kernel variant (tests/test_gpu_kd.py: NADD)."""
    return math.ceil(V / 64) + 16


def e_s(V):
    """Relative error of a sum of exponentials in units of u (derivation: tests/test_gpu_consistency.py)."""
    return 1.11 * V + 1 + nadd(V)


def cr_ref(logits, seq):
    """float64 reference.  logits [T,2B,V] (column b: view a of pair b, column b + B: view b), seq [B] -> dict(loss [B], frames,
    agree, grad [T,2B,V] = (qa - qb | qb - qa) (not scaled), eps [B] = the loss bound of tests/test_gpu_consistency.py in
    units of u, summed over the scored pair-frames, scored [T,B] (bad pair-frames excluded), bad [T,B])."""
    z = np.asarray(logits, np.float64)
    T, B2, V = z.shape
    B = B2 // 2
    assert B2 == 2 * B and len(seq) == B
    za, zb = z[:, :B], z[:, B:]
    live = np.arange(T)[:, None] < np.asarray(seq)[None, :]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ma, mb = za.max(axis=-1, keepdims=True), zb.max(axis=-1, keepdims=True)
        ok = lambda x, m: np.isfinite(m[..., 0]) & ~np.isnan(x).any(axis=-1)
        bad = live & ~(ok(za, ma) & ok(zb, mb))
        scored = live & ~bad
        a, b = za - ma, zb - mb
        ea, eb = np.exp(a), np.exp(b)
        sa, sb = ea.sum(axis=-1, keepdims=True), eb.sum(axis=-1, keepdims=True)
        qa, qb = ea / sa, eb / sb
        d = qa - qb
        some = (qa > 0) | (qb > 0)                                        # probability 0 in both views: no term
        x = np.where(some, (a - b) - (np.log(sa) - np.log(sb)), 0.0)      # log qa - log qb
        j = np.where(some, d * x, 0.0).sum(axis=-1)
        # the bound's parts (0 * inf = 0 where a probability is 0)
        mag = lambda q, v: np.where(q > 0, q * np.abs(v), 0.0)
        delta = mag(qa, 3 * a) + mag(qb, 3 * b) + (qa + qb) * (e_s(V) + 3) + np.abs(d)
        lam = 2 * e_s(V) + 4.5 * math.log(V)
        ab = np.where(some & np.isfinite(a) & np.isfinite(b), np.abs(a) + np.abs(b) + np.abs(a - b), 0.0)
        eps = (np.abs(x) * delta + np.abs(d) * (ab + lam + np.abs(x)) + (1 + nadd(V)) * np.abs(d * x))
        eps = np.where(some, eps, 0.0).sum(axis=-1)
    j = np.where(scored, j, 0.0)
    eps = np.where(scored, eps, 0.0)
    g = np.where(scored[..., None], d, 0.0)
    loss = j.sum(axis=0)
    loss[bad.any(axis=0)] = np.nan
    keep = scored[..., None]
    same = np.where(keep, za, 0.0).argmax(axis=-1) == np.where(keep, zb, 0.0).argmax(axis=-1)        # numpy: the first maximum
    return dict(loss=loss, frames=scored.sum(axis=0), agree=(scored & same).sum(axis=0), grad=np.concatenate([g, -g], axis=1),
                eps=eps.sum(axis=0), scored=scored, bad=bad)


def _case(seed=0, T=7, B=3, V=11):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((T, 2 * B, V)) * 2.0, np.array([T, 0, 4][:B], np.int32)


def _swap(x, B):
    return np.concatenate([x[:, B:], x[:, :B]], axis=1)


# ----------------------------------------------------------------------------------------------- identities of the reference
def test_reference_is_the_symmetric_kl_written_out():
    logits, seq = _case()
    ref = cr_ref(logits, seq)
    T, B = 7, 3
    want = np.zeros(B)
    for b in range(B):
        for t in range(seq[b]):
            za, zb = logits[t, b], logits[t, b + B]
            la, lb = za - np.log(np.exp(za).sum()), zb - np.log(np.exp(zb).sum())
            want[b] += (np.exp(lb) * (lb - la)).sum() + (np.exp(la) * (la - lb)).sum()       # KL(qb || qa) + KL(qa || qb)
    assert np.allclose(ref["loss"], want, rtol=1e-12, atol=1e-14)
    assert ref["frames"].tolist() == [7, 0, 4] and ref["loss"][1] == 0.0
    assert (ref["agree"] <= ref["frames"]).all()
    assert not ref["grad"][~np.concatenate([ref["scored"]] * 2, axis=1)].any()


def test_reference_is_non_negative_zero_for_equal_rows_and_symmetric():
    logits, seq = _case(1)
    B = 3
    ref = cr_ref(logits, seq)
    per_frame = cr_ref(logits.reshape(1, -1, logits.shape[-1])[:, :2 * 21], np.ones(21, np.int32))     # any pairing: J >= 0
    assert (per_frame["loss"] >= 0).all() and (ref["loss"] >= 0).all() and ref["loss"][0] > 0
    same = np.concatenate([logits[:, :B], logits[:, :B]], axis=1)
    eq = cr_ref(same, seq)
    assert not eq["loss"].any() and not eq["grad"].any() and np.array_equal(eq["agree"], eq["frames"])
    assert not eq["eps"].any()                                           # and so is the bound: the kernel's 0 is exact
    sw = cr_ref(_swap(logits, B), seq)
    assert np.array_equal(sw["loss"], ref["loss"]) and np.array_equal(sw["agree"], ref["agree"])
    assert np.array_equal(_swap(sw["grad"], B), ref["grad"])             # the halves swap with the views ...
    assert np.array_equal(ref["grad"][:, :B], -ref["grad"][:, B:])       # ... and grad_a = -grad_b
    assert np.array_equal(_swap(ref["grad"], B), -ref["grad"])


def test_reference_non_finite_rows():
    logits, seq = _case(2)
    B = 3
    clean = cr_ref(logits, seq)
    for view in (0, B):
        for kind in ("all -inf", "nan", "+inf"):
            z = logits.copy()
            if kind == "all -inf":
                z[2, 2 + view, :] = -np.inf
            else:
                z[2, 2 + view, 5] = np.nan if kind == "nan" else np.inf
            ref = cr_ref(z, seq)
            assert np.isnan(ref["loss"][2]) and ref["loss"][0] == clean["loss"][0]
            assert ref["frames"][2] == clean["frames"][2] - 1 and ref["bad"][2, 2] and ref["bad"].sum() == 1
            assert not ref["grad"][2, 2].any() and not ref["grad"][2, 2 + B].any()
    z = logits.copy()
    z[1, 0, 3] = z[1, B, 3] = -np.inf                                     # probability 0 in both views: contributes 0
    ref = cr_ref(z, seq)
    assert np.isfinite(ref["loss"][0]) and np.isfinite(ref["eps"][0]) and ref["grad"][1, 0, 3] == 0.0
    z[1, 0, 4] = -np.inf                                                  # qb > 0 against za = -inf
    ref = cr_ref(z, seq)
    assert ref["loss"][0] == np.inf and np.isfinite(ref["grad"]).all()


@pytest.mark.parametrize("seed", [0, 1])
def test_stop_gradient_rows_are_the_derivatives_with_the_other_view_held(seed):
    """d/dza KL(qb || softmax(za)) = qa - qb with qb constant, d/dzb KL(qa || softmax(zb)) = qb - qa with qa constant: central
    differences.  And the pair is NOT the derivative of J, which also moves the target."""
    rng = np.random.default_rng(seed)
    V = 9
    za, zb = rng.standard_normal(V) * 2.0, rng.standard_normal(V) * 2.0
    lsm = lambda z: z - np.log(np.exp(z).sum())
    kl = lambda p_log, q_log: (np.exp(p_log) * (p_log - q_log)).sum()
    ref = cr_ref(np.stack([za, zb])[None], np.array([1], np.int32))
    ga, gb = ref["grad"][0, 0], ref["grad"][0, 1]
    h = 1e-6
    fd_a, fd_b, fd_j = np.zeros(V), np.zeros(V), np.zeros(V)
    for k in range(V):
        e = np.zeros(V)
        e[k] = h
        fd_a[k] = (kl(lsm(zb), lsm(za + e)) - kl(lsm(zb), lsm(za - e))) / (2 * h)
        fd_b[k] = (kl(lsm(za), lsm(zb + e)) - kl(lsm(za), lsm(zb - e))) / (2 * h)
        jp = kl(lsm(zb), lsm(za + e)) + kl(lsm(za + e), lsm(zb))
        jm = kl(lsm(zb), lsm(za - e)) + kl(lsm(za - e), lsm(zb))
        fd_j[k] = (jp - jm) / (2 * h)
    assert np.abs(fd_a - ga).max() < 1e-8 and np.abs(fd_b - gb).max() < 1e-8
    assert np.abs(fd_j - ga).max() > 1e-3                                 # the full derivative of J is another vector


# ----------------------------------------------------------------------------------------------- the doubled batch
def test_double_batch_known_answers():
    from lstm_ctc_amd.nnet.graph import double_batch
    seq = np.array([5, 3, 4], np.int32)
    flat = np.array([7, 1, 2, 9, 9, 4], np.int32)                         # 2, 0 and 4 labels
    offs = np.array([0, 2, 2, 6], np.int32)
    lo, hi = np.array([0, 1, 0, 1, 2, 3], np.int32), np.array([2, 4, 0, 1, 2, 3], np.int32)
    s2, f2, o2, l2, h2 = double_batch(seq, flat, offs, lo, hi)
    assert s2.tolist() == [5, 3, 4, 5, 3, 4] and s2.dtype == np.int32
    assert f2.tolist() == [7, 1, 2, 9, 9, 4, 7, 1, 2, 9, 9, 4] and f2.dtype == np.int32
    assert o2.tolist() == [0, 2, 2, 6, 8, 8, 12] and o2.dtype == np.int32
    assert l2.tolist() == lo.tolist() * 2 and h2.tolist() == hi.tolist() * 2
    for b in range(3):                                                    # utterance b + B spells what utterance b spells
        assert f2[o2[b]:o2[b + 1]].tolist() == f2[o2[b + 3]:o2[b + 4]].tolist() == flat[offs[b]:offs[b + 1]].tolist()
    assert seq.tolist() == [5, 3, 4] and offs.tolist() == [0, 2, 2, 6]    # the inputs are not written
    # without windows, without labels at all, and with only the label arrays
    s2, f2, o2, l2, h2 = double_batch(seq[:1], flat[:0], np.array([0, 0], np.int32))
    assert s2.tolist() == [5, 5] and f2.tolist() == [] and o2.tolist() == [0, 0, 0] and l2 is None and h2 is None
    s2, f2, o2, _, _ = double_batch(None, flat, offs)
    assert s2 is None and o2.tolist() == [0, 2, 2, 6, 8, 8, 12] and len(f2) == 12


def test_double_batch_takes_tensors():
    import torch
    from lstm_ctc_amd.nnet.graph import double_batch
    t = lambda *v: torch.tensor(v, dtype=torch.int32)
    s2, f2, o2, l2, h2 = double_batch(t(2, 6), t(3, 3, 1), t(0, 1, 3), t(0, 0, 2), t(1, 3, 5))
    assert s2.tolist() == [2, 6, 2, 6] and f2.tolist() == [3, 3, 1, 3, 3, 1] and o2.tolist() == [0, 1, 3, 4, 6]
    assert l2.tolist() == [0, 0, 2, 0, 0, 2] and h2.tolist() == [1, 3, 5, 1, 3, 5]
    assert all(x.dtype == torch.int32 for x in (s2, f2, o2, l2, h2))


# ----------------------------------------------------------------------------------------------- the option
CFG = dict(nnet_type="blstm", input_dim=12, left_context=0, right_context=0, num_layers=1, num_neurons=32, num_projects=16,
           num_targets=12, use_peepholes=True, dropout_rate=0.8)


def test_factory_takes_the_keyword():
    import inspect
    import lstm_ctc_amd.nnet as nnet
    from lstm_ctc_amd.nnet import graph
    assert inspect.signature(nnet.create_graph_for_training_ctc).parameters["consistency_weight"].default is None
    assert inspect.signature(graph.CTCGraph.__init__).parameters["consistency_weight"].default is None
    for name in ("create_graph_for_validation_ctc", "create_graph_for_training_xent", "create_graph_for_training_kd"):
        assert "consistency_weight" not in inspect.signature(getattr(nnet, name)).parameters


def test_option_is_validated_before_anything_touches_a_device():
    from lstm_ctc_amd.nnet import graph
    from lstm_ctc_amd.nnet.augment import SpecAugment
    for bad in (0.0, -0.5, float("nan"), float("inf"), "0.2", True):
        with pytest.raises(ValueError, match="consistency_weight must be"):
            graph.CTCGraph(None, CFG, learn_rate=0.1, consistency_weight=bad)
    for objective in ("xent", "kd"):
        with pytest.raises(ValueError, match="objective"):
            graph.CTCGraph(None, CFG, learn_rate=0.1, objective=objective, consistency_weight=0.2)
    with pytest.raises(ValueError, match="teacher_weight"):
        graph.CTCGraph(None, CFG, learn_rate=0.1, teacher_weight=0.5, consistency_weight=0.2)
    spec = SpecAugment(time_masks=1, time_width=3, freq_masks=1, freq_width=2, freq_bins=12)
    for cfg in (dict(CFG, dropout_rate=1.0), dict(CFG, dropout_rate=None), dict(CFG, is_training=False),
                dict(CFG, nnet_type="cudnnlstm")):
        assert graph.config_keep(cfg) == 1.0
        with pytest.raises(ValueError, match="two views"):
            graph.CTCGraph(None, cfg, learn_rate=0.1, consistency_weight=0.2)
        with pytest.raises(ValueError, match="teacher_weight"):          # with spec_augment the views differ: the next check speaks
            graph.CTCGraph(None, cfg, learn_rate=0.1, spec_augment=spec, teacher_weight=1.0, consistency_weight=0.2)
    assert graph.config_keep(CFG) == 0.8 and graph.config_keep(dict(CFG, nnet_type="lstm")) == 0.8


# ----------------------------------------------------------------------------------------------- the command line
def _run(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "nnet-train.py")] + list(args), capture_output=True,
                       timeout=120)
    return r.returncode, r.stderr.decode(), r.stdout.decode()


def _fatal(err):
    return [line for line in err.splitlines() if line.startswith("FATAL:tensorflow:")]


def _argv(tmp_path, dropout="0.8"):
    scp = tmp_path / "t.scp"
    scp.write_text("utt0 5 3 0 %s\n" % (tmp_path / "utt0.tfrecords"))
    config = tmp_path / "nnet.config"
    config.write_text("nnet_type = blstm\ninput_dim = 40\nleft_context = 0\nright_context = 0\ndropout_rate = %s\n" % dropout)
    return [str(scp), str(config), "nnet.in", "nnet.out"]


SPEC = ["--spec-augment", "time=1x4,freq=1x5,bins=40"]


@pytest.mark.parametrize("flags,word", [
    (["--objective", "ctc", "--consistency-weight", "0"] + SPEC, "> 0"),
    (["--objective", "ctc", "--consistency-weight", "-0.2"] + SPEC, "> 0"),
    (["--objective", "ctc", "--consistency-weight", "nan"] + SPEC, "> 0"),
    (["--objective", "ctc", "--consistency-weight", "inf"] + SPEC, "> 0"),
    (["--objective", "xent", "--consistency-weight", "0.2"] + SPEC, "--objective ctc"),
    (["--objective", "kd", "--consistency-weight", "0.2"] + SPEC, "--objective ctc"),
    (["--objective", "ctc", "--consistency-weight", "0.2", "--teacher-scores", "ark:none.ark"] + SPEC, "--teacher-scores"),
])
def test_cli_fatal_paths_come_before_the_device(flags, word, tmp_path):
    rc, err, _ = _run(*flags, *_argv(tmp_path))
    fatal = _fatal(err)
    assert rc == 1 and len(fatal) == 1, err
    assert "--consistency-weight" in fatal[0] and word in fatal[0], err
    assert "no GPU" not in fatal[0] and "Traceback" not in err, err


def test_cli_needs_spec_augment_or_dropout(tmp_path):
    rc, err, _ = _run("--objective", "ctc", "--consistency-weight", "0.2", *_argv(tmp_path, dropout="1.0"))
    fatal = _fatal(err)
    assert rc == 1 and len(fatal) == 1 and "--consistency-weight" in fatal[0] and "--spec-augment" in fatal[0], err
    assert "no GPU" not in fatal[0] and "Traceback" not in err, err


def test_cli_dropout_rate_that_is_no_number_is_fatal_not_a_traceback(tmp_path):
    rc, err, _ = _run("--objective", "ctc", "--consistency-weight", "0.2", *_argv(tmp_path, dropout="often"))
    fatal = _fatal(err)
    assert rc == 1 and len(fatal) == 1 and "--consistency-weight" in fatal[0] and "dropout_rate" in fatal[0], err
    assert "no GPU" not in fatal[0] and "Traceback" not in err, err


def test_cli_help_lists_the_flag_for_nnet_train_only():
    rc, _, out = _run("--help")
    assert rc == 0 and "--consistency-weight" in out
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "nnet-validate.py"), "--help"], capture_output=True,
                       timeout=120)
    assert r.returncode == 0 and "--consistency-weight" not in r.stdout.decode()


def test_keywords_and_report_line(capsys):
    import importlib.util
    mod_spec = importlib.util.spec_from_file_location("_common_for_consistency_test", os.path.join(ROOT, "bin", "_common.py"))
    mod = importlib.util.module_from_spec(mod_spec)
    mod_spec.loader.exec_module(mod)
    assert mod.FLAGS["--consistency-weight"]["default"] is None
    cli = mod.build_cli(("nnet_config",), ("--objective", "--consistency-weight", "--teacher-scores"))
    assert mod.consistency_keywords(cli.parse_args(["missing.config", "--objective", "ctc"]), {}) == {}
    args = cli.parse_args(["missing.config", "--objective", "ctc", "--consistency-weight", "0.2"])
    assert mod.consistency_keywords(args, {"spec_augment": object()}) == {"consistency_weight": 0.2}
    assert mod.consistency_keywords(args, {}) == {"consistency_weight": 0.2}      # an unreadable config is reported elsewhere

    class Graph:
        consistency_weight, cr_loss_total, cr_frames_total, cr_agree_total = 0.2, 50.0, 1000, 875
    mod.report_consistency(Graph())
    line = [l for l in capsys.readouterr().err.splitlines() if "consistency weight" in l]
    assert len(line) == 1 and line[0].startswith("INFO:tensorflow:consistency weight 0.2: "), line
    assert "mean symmetric KL 0.050000 per frame over 1000 frame(s)" in line[0] and "agree on 87.50%" in line[0]


# ----------------------------------------------------------------------------------------------- the run loop
class _FakeGraph:
    """What nnet.train asks of a graph: key access, no process group, a device to reduce on (never used without a group)."""
    pg = None

    class model:
        device = "cpu"

    def __init__(self, keys):
        self.keys = keys

    def __contains__(self, key):
        return key in self.keys

    def __getitem__(self, key):
        if key not in self.keys:
            raise KeyError(key)
        return key


class _FakeSession:
    def __init__(self, steps):
        self.steps = list(steps)

    def run(self, nodes):
        from lstm_ctc_amd.nnet.graph import OutOfRangeError
        if not self.steps:
            raise OutOfRangeError()
        res = self.steps.pop(0)
        return {k: res.get(v) for k, v in nodes.items()}


def _eval_lines(err):
    return [float(l.split("eval = ")[1]) for l in err.splitlines() if ", eval = " in l]


def test_train_loop_logs_the_error_rate_of_view_a_not_half_of_it(capsys):
    """A doubled step reports ``size`` = the labels of both views and ``eval`` = the edit distance of view a alone: the logged
    ``eval`` is eval / eval_size, label-weighted over the steps, and the loss stays per label of both views."""
    from lstm_ctc_amd.nnet import funcs
    keys = ["size", "train", "summary", "loss", "eval_loss", "sequence_length", "eval", "eval_size"]
    steps = [dict(size=20, eval_size=10, eval_loss=40.0, loss=41.0, eval=5.0, sequence_length=None),
             dict(size=60, eval_size=30, eval_loss=60.0, loss=61.0, eval=3.0, sequence_length=None)]
    funcs.train(_FakeSession(steps), _FakeGraph(keys), evaluate=True, report_interval=1)
    err = capsys.readouterr().err
    got = _eval_lines(err)
    assert got == [pytest.approx(0.5, abs=1e-6), pytest.approx(8.0 / 40.0, abs=1e-6)], err
    assert "tr_loss = %f" % (100.0 / 80.0) in err
    # a graph without the key (every graph without the option) is normalised by size, as it always was
    plain = [dict(s, eval_size=None) for s in steps]
    funcs.train(_FakeSession(plain), _FakeGraph(keys[:-1]), evaluate=True, report_interval=1)
    assert _eval_lines(capsys.readouterr().err) == [pytest.approx(0.25, abs=1e-6), pytest.approx(8.0 / 80.0, abs=1e-6)]


def test_running_mean_without_eval_size_is_the_arithmetic_it_was():
    from lstm_ctc_amd.nnet.funcs import _Running
    run, loss, acc, processed = _Running(True), 0.0, 0.0, 0
    for size, eval_loss, batch_eval in ((7, 30.5, 3.0), (0, 0.0, 0.0), (13, 11.25, 9.0)):
        run.update(size, eval_loss, batch_eval)
        if size > 0:
            processed += size
            loss += (eval_loss / size - loss) * size / processed
            acc += (batch_eval / size - acc) * size / processed
    assert (run.loss, run.acc, run.processed, run.step) == (loss, acc, processed, 3)


def test_model_and_constructor_share_one_keep_rule():
    import inspect
    from lstm_ctc_amd.nnet import graph, model
    assert graph.config_keep is model.config_keep
    assert "config_keep(self.cfg)" in inspect.getsource(model.Model.__init__)


# ----------------------------------------------------------------------------------------------- the library
def test_signatures_declare_both_entries_as_the_header_does():
    from lstm_ctc_amd import _lib
    assert len(_lib.SIGNATURES["lc_consistency_workspace_bytes"][1]) == 3
    assert len(_lib.SIGNATURES["lc_consistency_loss"][1]) == 14
    header = " ".join(open(os.path.join(ROOT, "include", "lstm_ctc_hip.h")).read().split())
    assert "size_t lc_consistency_workspace_bytes(int T, int B, int V);" in header
    assert ("int lc_consistency_loss(const float *logits, int T, int B, int V, const int *seq_len, float grad_scale, float *loss, "
            "int *frames, int *agree, float *grad, int accumulate, void *workspace, size_t workspace_bytes, lc_stream_t stream);"
            ) in header
    assert "STOP-GRADIENT" in header and "NOT the derivative" in header


def test_library_version_is_at_least_8_and_the_entry_refuses_bad_arguments_without_a_device():
    """LC_EINVAL / LC_EWORKSPACE come before any launch, so every rejection can be seen on a box without a GPU (the pointers
    are never dereferenced: the call returns at its argument checks)."""
    import __graft_entry__ as g
    g.build()
    from lstm_ctc_amd import _lib
    lib = _lib.load()
    assert lib.lc_version() >= 8
    assert lib.lc_consistency_workspace_bytes(7, 3, 12) >= 8 * 7 * 3
    for shape in ((0, 3, 12), (7, 0, 12), (7, 3, 1), (-1, 3, 12)):
        assert lib.lc_consistency_workspace_bytes(*shape) == 0
    need = lib.lc_consistency_workspace_bytes(7, 3, 12)

    def call(T=7, B=3, V=12, logits=4096, seq=4096, scale=1.0, loss=4096, frames=4096, agree=4096, grad=4096, acc=0, ws=4096,
             nbytes=need):
        return lib.lc_consistency_loss(logits, T, B, V, seq, scale, loss, frames, agree, grad, acc, ws, nbytes, None)

    for kw in (dict(T=0), dict(B=0), dict(T=-3), dict(B=-1), dict(V=1), dict(V=0), dict(scale=float("nan")),
               dict(scale=float("inf")), dict(scale=float("-inf")), dict(logits=None), dict(seq=None), dict(loss=None),
               dict(frames=None), dict(agree=None), dict(ws=None), dict(grad=None, acc=1)):
        assert call(**kw) == -1, kw
        assert lib.lc_last_error().startswith(b"lc_consistency_loss: "), kw
    for short in (0, need - 1):
        assert call(nbytes=short) == -3
    assert lib.lc_last_error().startswith(b"lc_consistency_loss: workspace too small")
