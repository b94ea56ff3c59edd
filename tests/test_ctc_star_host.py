"""Host side of transcript-tolerant CTC (lc_ctc_loss_star): the float64 reference the GPU tests compare against (anchored
here against brute-force enumeration over all paths x own-or-star choices per frame, against central differences, against
the oracle's plain CTC and against the concavity sandwich, before a GPU is involved), the detection case, the
--star-penalty / --star-report flags' FATAL paths, the graph keyword and the workspace query.  No GPU needed.

The criterion: with q = softmax(x[t]), Qnb = sum_{k < V-1} q_k, qstar = Qnb / (V - 1) and the weights
wb = exp(-bypass_penalty), ws = exp(-selfloop_penalty), the emission of lattice position s at frame t is
    e'(t, s) = q_y + wb qstar at a label position of class y,   q_blank + ws qstar at a blank position,
Z = sum over lc_ctc_loss_windowed's feasible paths of prod_t e'(t, s_t), loss = -log Z (it may be negative),
    star_frames = sum_t M(t),  M(t) = sum_s occupancy(t, s) sigma(t, s),  sigma = w qstar / e',
    grad[t, k] = q_k - rho_k occ_k - [k < V-1] (q_k / Qnb) M(t),  rho = q_class / e'.
tests/test_gpu_ctc_star.py imports ``star_ctc_ref`` and the detection case from here."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

from test_ctc_window_host import OPEN, _lse, _shl, _shr, log_softmax64, random_path, windowed_ctc_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


# ----------------------------------------------------------------------------------------------- reference
def star_ctc_ref(x, labels, pb, ps, blank, lo=None, hi=None):
    """x [T,V] logits of the LIVE frames (T >= 1), labels [L], pb / ps = bypass / self-loop penalty (>= 0 or +inf), optional
    windows lo / hi [L] -> dict: ``loss`` = -log Z (+inf without a surviving path), ``star_frames`` (0 then), ``grad`` [T,V]
    (the softmax then), ``gamma`` [T,S] occupancies, ``m`` [T] the star's share per frame.  float64, log domain throughout:
    nothing underflows at T = 1000."""
    lp = log_softmax64(x)
    T, V = lp.shape
    assert blank == V - 1
    labels = np.asarray(labels, np.int64).reshape(-1)
    L = len(labels)
    S = 2 * L + 1
    ext = np.full(S, blank, np.int64)
    ext[1::2] = labels
    with np.errstate(invalid="ignore", divide="ignore"):
        top = np.maximum(lp[:, :blank].max(axis=1), -1e300)
        lnb = top + np.log(np.exp(lp[:, :blank] - top[:, None]).sum(axis=1))        # log Qnb, its own log-sum-exp
    pen = np.where(np.arange(S) % 2 == 1, float(pb), float(ps))
    own = lp[:, ext]
    star = (lnb - np.log(V - 1))[:, None] - pen[None, :]                             # -inf for a penalty of +inf
    emis = np.logaddexp(own, star)
    if L and lo is not None:
        t = np.arange(T)[:, None]
        inside = (t >= np.asarray(lo, np.int64)[None, :]) & (t <= np.asarray(hi, np.int64)[None, :])
        emis[:, 1::2] = np.where(inside, emis[:, 1::2], -np.inf)
    skip_in = np.zeros(S, bool)
    skip_in[3::2] = ext[3::2] != ext[1:-2:2]
    skip_out = np.zeros(S, bool)
    skip_out[1:-2:2] = skip_in[3::2]
    ninf = -np.inf
    alpha, beta = np.full((T, S), ninf), np.full((T, S), ninf)
    a = np.full(S, ninf)
    a[0] = 0.0
    for t in range(T):
        a = _lse(a, _shr(a, 1), np.where(skip_in, _shr(a, 2), ninf)) + emis[t]
        alpha[t] = a
    b = np.full(S, ninf)
    b[S - 1] = 0.0
    for t in range(T - 1, -1, -1):
        b = _lse(b, _shl(b, 1), np.where(skip_out, _shl(b, 2), ninf)) + emis[t]
        beta[t] = b
    ll = alpha[T - 1, S - 1] if S < 2 else float(_lse(alpha[T - 1, S - 1], alpha[T - 1, S - 2]))
    soft = np.exp(lp)
    out = {"ext": ext, "emis": emis, "loglik": ll}
    if not np.isfinite(ll):
        out.update(loss=np.inf, star_frames=0.0, grad=soft, gamma=np.zeros((T, S)), m=np.zeros(T))
        return out
    live = np.isfinite(alpha) & np.isfinite(beta) & np.isfinite(emis)
    with np.errstate(invalid="ignore"):
        gamma = np.where(live, np.exp(np.where(live, alpha + beta - emis - ll, 0.0)), 0.0)
        rho = np.where(live & np.isfinite(own), np.exp(np.where(live, own - emis, 0.0)), 0.0)
        sigma = np.where(live & np.isfinite(star), np.exp(np.where(live, star - emis, 0.0)), 0.0)
    m = (gamma * sigma).sum(axis=1)
    occ = np.zeros((T, V))
    np.add.at(occ, (np.arange(T)[:, None], ext[None, :]), gamma * rho)
    grad = soft - occ
    has = m > 0                                                                      # m > 0 needs Qnb > 0
    with np.errstate(invalid="ignore"):
        share = np.where(has[:, None], np.exp(np.where(has[:, None], lp[:, :blank] - lnb[:, None], 0.0)), 0.0)
    grad[:, :blank] -= share * m[:, None]
    out.update(loss=-ll, star_frames=float(m.sum()), grad=grad, gamma=gamma, m=m)
    return out


def brute_force_star(x, labels, pb, ps, blank, lo=None, hi=None):
    """(-log Z, star_frames) by enumeration of every lattice path and, per frame, the choice between the position's own
    class and the star; (inf, 0) without a feasible path.  Probabilities, not logs: T <= 5."""
    q = np.exp(log_softmax64(x))
    T, V = q.shape
    labels = list(labels)
    L = len(labels)
    S = 2 * L + 1
    qstar = q[:, :blank].sum(axis=1) / (V - 1)
    wb, ws = np.exp(-pb), np.exp(-ps)
    total = stars = 0.0
    for path in itertools.product(range(S), repeat=T):
        if path[0] > 1 or path[-1] < S - 2:
            continue
        ok = True
        for t in range(1, T):
            d = path[t] - path[t - 1]
            if d == 2:
                s = path[t]
                ok = s % 2 == 1 and labels[s // 2] != labels[s // 2 - 1]
            elif d not in (0, 1):
                ok = False
            if not ok:
                break
        if ok and lo is not None:
            ok = all(s % 2 == 0 or lo[s // 2] <= t <= hi[s // 2] for t, s in enumerate(path))
        if not ok:
            continue
        for choice in itertools.product((0, 1), repeat=T):                           # 1 = the frame is the star's
            p = 1.0
            for t, s in enumerate(path):
                if choice[t]:
                    p *= (wb if s % 2 else ws) * qstar[t]
                else:
                    p *= q[t, labels[s // 2] if s % 2 else blank]
            total += p
            stars += p * sum(choice)
    if total == 0.0:
        return np.inf, 0.0
    return -np.log(total), stars / total


# ----------------------------------------------------------------------------------------------- the reference is right
BRUTE_CASES = [(4, 3, [0, 1]), (5, 4, [1, 1]), (5, 3, [0]), (4, 5, []), (5, 4, [2, 0])]
BRUTE_PENALTIES = [(0.5, 1.5), (0.0, 0.0), (3.0, INF), (INF, 2.0)]


@pytest.mark.parametrize("pb,ps", BRUTE_PENALTIES)
def test_reference_matches_enumeration_of_paths_and_star_choices(pb, ps):
    rng = np.random.RandomState(41)
    for T, V, labels in BRUTE_CASES:
        x = rng.randn(T, V) * 1.5
        ref = star_ctc_ref(x, labels, pb, ps, V - 1)
        loss, stars = brute_force_star(x, labels, pb, ps, V - 1)
        assert np.isfinite(loss)
        assert abs(ref["loss"] - loss) < 1e-12, (T, V, labels, ref["loss"], loss)
        assert abs(ref["star_frames"] - stars) < 1e-12, (T, V, labels, ref["star_frames"], stars)
        assert np.abs(ref["gamma"].sum(axis=1) - 1.0).max() < 1e-12
        assert np.abs(ref["grad"].sum(axis=1)).max() < 1e-12                       # live rows sum to 0
    # windows: the same enumeration inside them
    x = rng.randn(5, 4) * 1.5
    lo, hi = np.array([0, 2]), np.array([2, 4])
    ref = star_ctc_ref(x, [2, 0], pb, ps, 3, lo, hi)
    loss, stars = brute_force_star(x, [2, 0], pb, ps, 3, lo, hi)
    assert abs(ref["loss"] - loss) < 1e-12 and abs(ref["star_frames"] - stars) < 1e-12
    assert loss > brute_force_star(x, [2, 0], pb, ps, 3)[0]


@pytest.mark.parametrize("pb,ps", BRUTE_PENALTIES + [(2.0, 2.0)])
@pytest.mark.parametrize("windows", [False, True])
def test_reference_gradient_is_the_derivative_of_its_loss(pb, ps, windows):
    """Central differences at h = 1e-6: truncation of the order h^2 = 1e-12, rounding of the order 1e-16 |loss| / h = 1e-9
    for a loss of some nats; the bar is 1e-8."""
    rng = np.random.RandomState(42)
    T, V, labels = 9, 5, np.array([1, 1, 0, 3])
    x = rng.randn(T, V) * 1.5
    states = random_path(rng, labels, T)
    lo = np.array([np.flatnonzero(states == 2 * i + 1)[0] for i in range(len(labels))]) - 2
    hi = np.array([np.flatnonzero(states == 2 * i + 1)[-1] for i in range(len(labels))]) + 2
    win = (lo, hi) if windows else (None, None)
    ref = star_ctc_ref(x, labels, pb, ps, V - 1, *win)
    assert np.isfinite(ref["loss"])
    h = 1e-6
    num = np.zeros_like(x)
    for t in range(T):
        for k in range(V):
            xp, xm = x.copy(), x.copy()
            xp[t, k] += h
            xm[t, k] -= h
            num[t, k] = (star_ctc_ref(xp, labels, pb, ps, V - 1, *win)["loss"]
                         - star_ctc_ref(xm, labels, pb, ps, V - 1, *win)["loss"]) / (2 * h)
    assert np.abs(num - ref["grad"]).max() < 1e-8, np.abs(num - ref["grad"]).max()
    if np.isfinite(pb) and np.isfinite(ps) and min(pb, ps) >= h:                     # star_frames = d loss / d p, both moving
        d = (star_ctc_ref(x, labels, pb + h, ps + h, V - 1, *win)["loss"]
             - star_ctc_ref(x, labels, pb - h, ps - h, V - 1, *win)["loss"]) / (2 * h)
        assert abs(d - ref["star_frames"]) < 1e-8, (d, ref["star_frames"])


def test_infinite_penalties_are_plain_ctc(oracle):
    rng = np.random.RandomState(43)
    T, B, V = 14, 3, 6
    x = rng.randn(T, B, V) * 2
    labels = [np.array([1, 1, 0, 3, 2]), np.array([], np.int64), np.array([4, 0])]
    seq = np.array([14, 5, 9], np.int32)
    flat = np.concatenate(labels).astype(np.int32)
    offs = np.concatenate(([0], np.cumsum([len(l) for l in labels]))).astype(np.int32)
    loss, grad, bad = oracle.ctc_loss(np.ascontiguousarray(x), flat, offs, seq)
    assert bad == 0
    for b in range(B):
        ref = star_ctc_ref(x[:seq[b], b], labels[b], INF, INF, V - 1)
        assert abs(ref["loss"] - loss[b]) < 1e-10 * max(abs(loss[b]), 1.0), (b, ref["loss"], loss[b])
        assert np.abs(ref["grad"] - grad[:seq[b], b]).max() < 1e-10
        assert ref["star_frames"] == 0.0 and not ref["m"].any()
        L = len(labels[b])
        want = windowed_ctc_ref(x[:seq[b], b], labels[b], np.zeros(L), np.full(L, OPEN), V - 1)
        assert abs(ref["loss"] - want["loss"]) < 1e-12 and np.abs(ref["grad"] - want["grad"]).max() < 1e-14


def test_sandwich_and_never_above_plain_ctc():
    """loss is concave in a penalty p that moves both stars: for p0 < p1,
    loss(p0) + star_frames(p1) (p1 - p0) <= loss(p1) <= loss(p0) + star_frames(p0) (p1 - p0), and loss(p) <= plain CTC."""
    rng = np.random.RandomState(44)
    for case in range(200):
        T = int(rng.randint(1, 12))
        V = int(rng.randint(2, 7))
        L = int(rng.randint(0, min(T, 4) + 1))
        labels = rng.randint(0, V - 1, L)
        if random_path(rng, labels, T) is None:
            continue
        x = rng.randn(T, V) * rng.choice([0.5, 2.0, 5.0])
        p0 = float(rng.uniform(0, 3))
        p1 = p0 + float(rng.uniform(0.01, 3))
        r0, r1 = star_ctc_ref(x, labels, p0, p0, V - 1), star_ctc_ref(x, labels, p1, p1, V - 1)
        plain = star_ctc_ref(x, labels, INF, INF, V - 1)["loss"]
        eps = 1e-11 * max(abs(r1["loss"]), 1.0)
        assert r0["loss"] + r1["star_frames"] * (p1 - p0) <= r1["loss"] + eps, case
        assert r1["loss"] <= r0["loss"] + r0["star_frames"] * (p1 - p0) + eps, case
        assert r0["loss"] <= r1["loss"] + eps and r1["loss"] <= plain + eps, case
        assert 0.0 <= r1["star_frames"] <= r0["star_frames"] + 1e-11 <= T + 2e-11, case


def test_long_utterance_does_not_underflow():
    rng = np.random.RandomState(45)
    T, V, L = 1000, 44, 100
    ref = star_ctc_ref(rng.randn(T, V) * 2, rng.randint(0, V - 1, L), 1.0, 1.0, V - 1)
    assert np.isfinite(ref["loss"]) and 0 < ref["star_frames"] < T and np.isfinite(ref["grad"]).all()
    assert np.abs(ref["grad"].sum(axis=1)).max() < 1e-9


# ----------------------------------------------------------------------------------------------- the detection case
DETECT_V, DETECT_TRUE, DETECT_PENALTY = 8, [0, 3, 5, 2, 6, 1], (2.0, 2.0)
DETECT_TRANSCRIPTS = {"clean": [0, 3, 5, 2, 6, 1], "substitution": [0, 3, 4, 2, 6, 1], "deletion": [0, 3, 2, 6, 1],
                      "insertion": [0, 3, 5, 4, 2, 6, 1]}


def detection_logits(seed):
    """T = 18: every true label on two frames, then a blank frame; N(0, 0.3^2) noise plus 6 on the path's class."""
    rng = np.random.RandomState(seed)
    path = []
    for k in DETECT_TRUE:
        path += [k, k, DETECT_V - 1]
    x = rng.randn(len(path), DETECT_V) * 0.3
    x[np.arange(len(path)), path] += 6.0
    return x


def test_detection_of_a_wrong_transcript():
    """One substitution, one deletion or one insertion in the transcript raises star_frames by at least 0.5 over the clean
    transcript, on every one of 20 seeds."""
    smallest = np.inf
    for seed in range(20):
        x = detection_logits(seed)
        got = {k: star_ctc_ref(x, t, *DETECT_PENALTY, DETECT_V - 1)["star_frames"] for k, t in DETECT_TRANSCRIPTS.items()}
        for kind in ("substitution", "deletion", "insertion"):
            smallest = min(smallest, got[kind] - got["clean"])
            assert got[kind] - got["clean"] >= 0.5, (seed, kind, got)
    print("smallest margin over 20 seeds: %.3f" % smallest)


# ----------------------------------------------------------------------------------------------- command line
def _run(cli, *args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", cli)] + list(args), capture_output=True, timeout=120)
    return r.returncode, r.stderr.decode()


def _common():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_common_for_star_test", os.path.join(ROOT, "bin", "_common.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("cli", ("nnet-train.py", "nnet-validate.py"))
def test_cli_star_penalty_fatal_paths_before_the_device(cli, tmp_path):
    """--star-penalty malformed, negative, NaN, with another objective than ctc, with --delay-penalty or --entropy-weight: one
    FATAL line naming the flag and exit 1, decided on the host - the same on a box with and without a GPU."""
    scp = tmp_path / "t.scp"
    scp.write_text("utt0 5 3 1 %s\n" % (tmp_path / "utt0.tfrecords"))
    argv = [str(scp), "nnet.config", "nnet.in"] + (["nnet.out"] if cli == "nnet-train.py" else [])
    for flags in (["--objective", "ctc", "--star-penalty=-1"], ["--objective", "ctc", "--star-penalty", "nan"],
                  ["--objective", "ctc", "--star-penalty=2,-inf"], ["--objective", "ctc", "--star-penalty", "1,2,3"],
                  ["--objective", "ctc", "--star-penalty", "two"], ["--objective", "ctc", "--star-penalty", ""],
                  ["--objective", "xent", "--star-penalty", "2"], ["--star-penalty", "2"],      # xent is the default objective
                  ["--objective", "ctc", "--star-penalty", "2", "--delay-penalty", "0.05"],
                  ["--objective", "ctc", "--star-penalty", "2,3", "--entropy-weight", "0.1"]):
        rc, err = _run(cli, *(flags + argv))
        fatal = [l for l in err.splitlines() if l.startswith("FATAL:tensorflow:")]
        assert rc == 1 and len(fatal) == 1, (flags, err)
        assert "--star-penalty" in fatal[0] and "no GPU" not in fatal[0], (flags, err)


def test_cli_align_star_flags_go_together(tmp_path):
    scp = tmp_path / "t.scp"
    scp.write_text("utt0 5 3 1 %s\n" % (tmp_path / "utt0.tfrecords"))
    argv = [str(scp), "nnet.config", "nnet.in", "ark:" + str(tmp_path / "ali.ark")]
    for flags in (["--star-penalty", "2"], ["--star-report", str(tmp_path / "r.txt")],
                  ["--star-penalty", "-2", "--star-report", str(tmp_path / "r.txt")],
                  ["--star-penalty", "x", "--star-report", str(tmp_path / "r.txt")]):
        rc, err = _run("nnet-align.py", *(flags + argv))
        fatal = [l for l in err.splitlines() if l.startswith("FATAL:tensorflow:")]
        assert rc == 1 and len(fatal) == 1, (flags, err)
        assert "--star-" in fatal[0] and "no GPU" not in fatal[0], (flags, err)
    assert not (tmp_path / "r.txt").exists()


def test_cli_help_names_the_flags_and_nnet_init_has_none():
    for cli, has in (("nnet-train.py", True), ("nnet-validate.py", True), ("nnet-align.py", True), ("nnet-init.py", False)):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", cli), "--help"], capture_output=True, timeout=120)
        assert r.returncode == 0 and (b"--star-penalty" in r.stdout) == has, cli
        assert (b"--star-report star-report" in r.stdout) == (cli == "nnet-align.py"), cli      # the option itself, with its metavar


def test_star_keywords_and_report_line():
    mod = _common()
    parser = mod.build_cli(("tfrecords_scp",), ("--objective", "--delay-penalty", "--entropy-weight", "--star-penalty"))
    assert mod.FLAGS["--star-penalty"]["default"] is None
    assert mod.star_keywords(parser.parse_args(["x.scp", "--objective", "ctc"])) == {}
    assert mod.star_keywords(parser.parse_args(["x.scp"])) == {}                                    # no flag: any objective
    assert mod.star_keywords(parser.parse_args(["x.scp", "--objective", "ctc", "--star-penalty", "2"])) == {"star_penalty": (2.0, 2.0)}
    assert mod.star_keywords(parser.parse_args(["x.scp", "--objective", "ctc", "--star-penalty", "0.5,3"])) == {"star_penalty": (0.5, 3.0)}
    assert mod.star_keywords(parser.parse_args(["x.scp", "--objective", "ctc", "--star-penalty", "inf,0"])) == {"star_penalty": (INF, 0.0)}
    assert mod.parse_star_penalty("1e-1, 2") == (0.1, 2.0)
    for bad in ("", "1,2,3", "-1", "nan", "1,-inf", "a", "1,"):
        with pytest.raises(ValueError):
            mod.parse_star_penalty(bad)
    line = mod.star_report_line("utt-1", 37, 5, 12.5, 3.25, 0.1234567)
    assert line == "utt-1 37 5 12.500000 3.250000 0.123457\n"
    assert mod.star_report_line("u", 3, 0, 0.0, -0.5, 1.0) == "u 3 0 0.000000 -0.500000 1.000000\n"      # the loss may be negative


# ----------------------------------------------------------------------------------------------- library
SMOKE_CFG = dict(nnet_type="blstm", input_dim=8, left_context=0, right_context=0, num_layers=2, num_neurons=32,
                 num_projects=16, num_targets=11, use_peepholes=True, dropout_rate=1.0)


def test_graph_keyword_is_validated_before_a_model_is_built():
    import inspect
    from lstm_ctc_amd.nnet import graph
    for bad in (dict(objective="xent", star_penalty=(2, 2)), dict(objective="kd", star_penalty=(2, 2)), dict(star_penalty=(-1, 2)),
                dict(star_penalty=(2, float("nan"))), dict(star_penalty=(2, -INF)), dict(star_penalty=2.0), dict(star_penalty=(2,)),
                dict(star_penalty=(1, 2, 3)), dict(star_penalty=("2", 2)), dict(star_penalty=(True, 2)),
                dict(star_penalty=(2, 2), delay_penalty=0.05), dict(star_penalty=(2, 2), entropy_weight=0.1)):
        with pytest.raises(ValueError, match="star_penalty"):
            graph.CTCGraph(None, SMOKE_CFG, seed=1, device="cpu", **bad)
    for factory in (graph.create_graph_for_training_ctc, graph.create_graph_for_validation_ctc):
        # the factories forward the criterion options to CTCGraph, where the keyword and its default live
        assert "criterion" in inspect.signature(factory).parameters
        assert inspect.signature(graph.CTCGraph.__init__).parameters["star_penalty"].default is None
        extra = {"learn_rate": 1e-3} if "training" in factory.__name__ else {}
        with pytest.raises(ValueError, match="star_penalty"):
            factory(None, SMOKE_CFG, **dict(extra, star_penalty=(-1.0, 0)))
        with pytest.raises(ValueError, match="delay_penalty"):
            factory(None, SMOKE_CFG, **dict(extra, star_penalty=(2, 2), delay_penalty=0.1))
        with pytest.raises(ValueError, match="entropy_weight"):
            factory(None, SMOKE_CFG, **dict(extra, star_penalty=(2, 2), entropy_weight=0.1))
    assert "star_penalty" in inspect.signature(graph.CTCGraph.align).parameters


def test_workspace_query_and_version():
    import __graft_entry__ as g
    g.build()
    from lstm_ctc_amd import _lib
    lib = _lib.load()
    assert lib.lc_version() >= 11
    q, qd = lib.lc_ctc_star_workspace_bytes, lib.lc_ctc_delay_workspace_bytes
    for shape in ((10, 2, 5, 3), (1000, 64, 44, 100), (10, 2, 5, 0), (1, 1, 2, 1023), (23, 65, 44, 70)):
        T, B = shape[:2]
        assert q(*shape) >= qd(*shape) + 4 * T * B > 0, shape
        assert q(*shape) <= qd(*shape) + 4 * T * B + 256, shape                     # the delay entry's plus T * B floats
    assert q(20, 2, 5, 3) > q(10, 2, 5, 3) and q(10, 2, 5, 40) > q(10, 2, 5, 3)
    for bad in ((0, 2, 5, 3), (10, 0, 5, 3), (10, 2, 1, 3), (10, 2, 5, -1), (10, 2, 5, 1024), (-1, 2, 5, 3)):
        assert q(*bad) == 0, bad
    assert hasattr(lib, "lc_ctc_loss_star")
