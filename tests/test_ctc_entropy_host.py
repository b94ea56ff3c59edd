"""Host side of maximum-entropy CTC: the float64 reference the GPU tests compare against (anchored here against brute-force
enumeration of all V^T paths and against central differences, before a GPU is involved), the identities the criterion obeys,
the --entropy-weight flag's FATAL paths, the graph keyword and the workspace query.  No GPU needed.

The criterion: over the feasible paths pi of an utterance (lc_ctc_loss_windowed's conventions), with
log p(pi) = sum_t log_softmax(x[t])[pi_t], Z = sum_pi p(pi) and Ebar = sum_pi (p(pi) / Z) log p(pi),
    loss = -log Z,   entropy = H = log Z - Ebar >= 0,   criterion = loss - eta H,
    grad[t, k] = softmax[t, k] - sum_{s: class(s) = k} gamma(t, s) (1 + eta (Ebar - c(t, s))),
c(t, s) the mean of log p(pi) over the posterior restricted to the paths through (t, s).  The reference
(``entropy_ctc_ref``) takes alpha, beta and gamma from ``windowed_ctc_ref`` and carries the expectation semiring's second
component beside them: m_alpha(t, s) = emis(t, s) + the mean of m_alpha(t - 1, .) over the cell's predecessors under the
weights exp(alpha(t - 1, .)), m_beta alike on the way back, c = m_alpha + m_beta - emis.
tests/test_gpu_ctc_entropy.py imports it from here."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

from test_ctc_window_host import OPEN, _shl, _shr, log_softmax64, random_path, windowed_ctc_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------------------------- reference
def _mean_sweep(lat, emis, allow2, backward):
    """m[t, s] = emis[t, s] + the mean of m over the cell's predecessors in the sweep's direction, weighted by exp(lat) of
    the predecessors; 0 in a dead cell.  ``lat`` is alpha (forward: predecessors s, s-1, s-2 of the row before) or beta
    (backward: s, s+1, s+2 of the row after), ``allow2`` says whether the cell may be reached from two positions away."""
    T, S = lat.shape
    shift = _shl if backward else _shr
    zshift = (lambda a, n: np.concatenate((a, np.zeros(n)))[n:]) if backward else (lambda a, n: np.concatenate((np.zeros(n), a))[:len(a)])
    a = np.full(S, -np.inf)
    a[S - 1 if backward else 0] = 0.0                    # behind the last / before the first frame
    m = np.zeros(S)
    out = np.zeros((T, S))
    for t in (range(T - 1, -1, -1) if backward else range(T)):
        terms = np.stack([a, shift(a, 1), np.where(allow2, shift(a, 2), -np.inf)])
        means = np.stack([m, zshift(m, 1), zshift(m, 2)])
        top = np.maximum(terms.max(axis=0), -1e300)
        w = np.exp(terms - top)                          # 0 for a dead predecessor
        den = w.sum(axis=0)
        mean = (w * means).sum(axis=0) / np.where(den > 0, den, 1.0)
        live = np.isfinite(lat[t])
        m = np.where(live, np.where(live, emis[t], 0.0) + mean, 0.0)
        a = lat[t]
        out[t] = m
    return out


def entropy_ctc_ref(x, labels, eta, blank, lo=None, hi=None):
    """x [T,V] logits of the LIVE frames (T >= 1), labels [L], eta = entropy weight, optional windows lo / hi [L] -> dict:
    ``loss`` = -log Z (+inf without a surviving path), ``entropy`` = H in nats (0 then), ``grad`` [T,V] of loss - eta H (the
    softmax then), ``gamma`` [T,S] occupancies, and ``ebar``, ``c`` [T,S] (0 in cells no path passes), ``alpha``, ``beta``,
    ``emis``, ``ext`` as ``windowed_ctc_ref`` gives them."""
    labels = np.asarray(labels, np.int64).reshape(-1)
    L = len(labels)
    if lo is None:
        lo, hi = np.zeros(L, np.int64), np.full(L, OPEN, np.int64)
    out = windowed_ctc_ref(x, labels, lo, hi, blank)
    T, V = np.asarray(x).shape
    S = 2 * L + 1
    if not np.isfinite(out["loss"]):
        out.update(entropy=0.0, ebar=0.0, c=np.zeros((T, S)))
        return out
    ext, emis, alpha, beta, gamma, ll = out["ext"], out["emis"], out["alpha"], out["beta"], out["gamma"], out["loglik"]
    skip_in = np.zeros(S, bool)
    skip_in[3::2] = ext[3::2] != ext[1:-2:2]
    skip_out = np.zeros(S, bool)
    skip_out[1:-2:2] = skip_in[3::2]
    ma = _mean_sweep(alpha, emis, skip_in, False)
    mb = _mean_sweep(beta, emis, skip_out, True)
    ends = [S - 1] + ([S - 2] if S >= 2 else [])
    wend = np.array([np.exp(alpha[T - 1, s] - ll) for s in ends])
    ebar = float((wend * ma[T - 1, ends]).sum())
    through = gamma > 0
    c = np.where(through, ma + mb - np.where(through, emis, 0.0), 0.0)
    tilt = gamma * (1.0 + eta * np.where(through, ebar - c, 0.0))
    occ = np.zeros((T, V))
    np.add.at(occ, (np.arange(T)[:, None], ext[None, :]), tilt)
    out.update(entropy=float(ll - ebar), ebar=ebar, c=c, grad=np.exp(log_softmax64(x)) - occ)
    return out


def criterion(x, labels, eta, blank, lo=None, hi=None):
    ref = entropy_ctc_ref(x, labels, eta, blank, lo, hi)
    return ref["loss"] - eta * ref["entropy"]


def feasible_paths(T, V, labels, blank, lo=None, hi=None):
    """Every path of V^T that collapses to ``labels`` with every label's run inside its window."""
    paths = []
    for path in itertools.product(range(V), repeat=T):
        runs = []                                        # (symbol, first, last) of the maximal non-blank runs
        for t, k in enumerate(path):
            if k == blank:
                continue
            if runs and runs[-1][0] == k and runs[-1][2] == t - 1:
                runs[-1][2] = t
            else:
                runs.append([k, t, t])
        if [r[0] for r in runs] != list(labels):
            continue
        if lo is not None and any(r[1] < lo[i] or r[2] > hi[i] for i, r in enumerate(runs)):
            continue
        paths.append(path)
    return paths


def brute_force_entropy(x, labels, blank, lo=None, hi=None):
    """(-log Z, H) by enumeration; (inf, 0) without a feasible path."""
    lp = log_softmax64(x)
    T, V = lp.shape
    logs = np.array([lp[np.arange(T), p].sum() for p in feasible_paths(T, V, labels, blank, lo, hi)])
    if not len(logs):
        return np.inf, 0.0
    top = logs.max()
    logz = top + np.log(np.exp(logs - top).sum())
    post = np.exp(logs - logz)
    return -logz, float(-(post * (logs - logz)).sum())


def count_paths(T, labels, lo=None, hi=None):
    """The number of feasible paths, by an integer dynamic programme over the same lattice (Python ints: no overflow)."""
    labels = list(labels)
    L = len(labels)
    S = 2 * L + 1
    n = [0] * S
    before = [1] + [0] * (S - 1)                         # "before frame 0": reaches positions 0 and 1
    for t in range(T):
        for s in range(S):
            v = before[s] + (before[s - 1] if s >= 1 else 0)
            if s >= 3 and s % 2 == 1 and labels[s // 2] != labels[s // 2 - 1]:
                v += before[s - 2]
            if s % 2 == 1 and lo is not None and not (lo[s // 2] <= t <= hi[s // 2]):
                v = 0
            n[s] = v
        before, n = n, [0] * S
    return before[S - 1] + (before[S - 2] if S >= 2 else 0)


# ----------------------------------------------------------------------------------------------- the reference is right
HAND_CASES = [                                           # (T, V, labels, lo, hi)
    (5, 3, [1, 1], None, None),                          # a repeated label: the blank between is forced
    (6, 3, [0, 0, 1], None, None),
    (4, 4, [], None, None),                              # L = 0: the all-blank path
    (3, 4, [2, 0, 1], None, None),                       # T = L: one path
    (7, 3, [0, 1], None, None),
    (2, 3, [1, 1], None, None),                          # L fits the frames, the blank between the equal labels does not
    (1, 2, [0], None, None),                             # T = 1
    (6, 4, [1, 2, 1], [0, 1, 3], [2, 4, 5]),             # windows
    (6, 3, [0, 1], [2, 0], [5, 1]),                      # windows no monotone path satisfies
]


def test_reference_matches_enumeration_of_all_paths():
    rng = np.random.RandomState(31)
    finite = []
    cases = list(HAND_CASES)
    for case in range(24):                               # random cases, windows around a random path, sometimes disturbed
        T = int(rng.randint(1, 8))
        V = int(rng.randint(2, 5))
        if V ** T > 5000:
            T = 6
        L = int(rng.randint(0, min(T, 3) + 1))
        labels = rng.randint(0, V - 1, L)
        lo = hi = None
        states = random_path(rng, labels, T)
        if case % 2 and L and states is not None:
            lo = np.array([np.flatnonzero(states == 2 * i + 1)[0] for i in range(L)]) - rng.randint(0, 2, L)
            hi = np.array([np.flatnonzero(states == 2 * i + 1)[-1] for i in range(L)]) + rng.randint(0, 2, L)
            if case % 3 == 1:
                lo = lo + rng.randint(-1, 3, L)
                hi = hi - rng.randint(0, 3, L)
        cases.append((T, V, list(labels), lo, hi))
    for i, (T, V, labels, lo, hi) in enumerate(cases):
        x = rng.randn(T, V) * 1.5
        ref = entropy_ctc_ref(x, labels, 0.5, V - 1, lo, hi)
        loss, H = brute_force_entropy(x, labels, V - 1, lo, hi)
        if not np.isfinite(loss):
            assert ref["loss"] == np.inf and ref["entropy"] == 0.0 and not ref["gamma"].any(), i
            assert np.array_equal(ref["grad"], np.exp(log_softmax64(x))), i
            finite.append(False)
            continue
        finite.append(True)
        assert abs(ref["loss"] - loss) < 1e-12, (i, ref["loss"], loss)
        assert abs(ref["entropy"] - H) < 1e-12, (i, ref["entropy"], H)
        assert ref["entropy"] >= -1e-13, i
        # Ebar is also the expected sum of the emissions along a path: an independent route to the same number
        through = ref["gamma"] > 0
        assert abs(ref["ebar"] - (ref["gamma"] * np.where(through, ref["emis"], 0.0)).sum()) < 1e-12, i
    assert finite[:9] == [True, True, True, True, True, False, True, True, False]
    assert sum(finite) >= 15 and finite.count(False) >= 3, finite


def _windowed_case(seed, T=9, V=4, labels=(1, 1, 0, 2)):
    rng = np.random.RandomState(seed)
    labels = np.array(labels)
    x = rng.randn(T, V) * 1.5
    states = random_path(rng, labels, T)
    lo = np.array([np.flatnonzero(states == 2 * i + 1)[0] for i in range(len(labels))]) - 2
    hi = np.array([np.flatnonzero(states == 2 * i + 1)[-1] for i in range(len(labels))]) + 2
    return x, labels, lo, hi


@pytest.mark.parametrize("windows", [False, True])
@pytest.mark.parametrize("eta", [0.2, 1.0])
def test_reference_gradient_is_the_derivative_of_the_criterion(eta, windows):
    """Central differences of loss - eta H at h = 1e-6: the truncation error is of the order h^2 = 1e-12, the rounding error
    of the order 1e-16 |criterion| / h = 1e-9 for a criterion of some tens of nats; 1e-7 leaves two orders of magnitude."""
    x, labels, lo, hi = _windowed_case(2)
    win = (lo, hi) if windows else (None, None)
    ref = entropy_ctc_ref(x, labels, eta, 3, *win)
    assert np.isfinite(ref["loss"]) and ref["entropy"] > 0.1
    h = 1e-6
    num = np.zeros_like(x)
    for t in range(x.shape[0]):
        for k in range(x.shape[1]):
            xp, xm = x.copy(), x.copy()
            xp[t, k] += h
            xm[t, k] -= h
            num[t, k] = (criterion(xp, labels, eta, 3, *win) - criterion(xm, labels, eta, 3, *win)) / (2 * h)
    assert np.abs(num - ref["grad"]).max() < 1e-7, np.abs(num - ref["grad"]).max()
    plain = entropy_ctc_ref(x, labels, 0.0, 3, *win)["grad"]
    assert np.abs(ref["grad"] - plain).max() > 1e-3                  # and the entropy term is not a rounding error


def test_uniform_logits_give_the_log_of_the_path_count():
    """All-equal logits: every feasible path has the same probability, H = ln N."""
    rng = np.random.RandomState(33)
    for T, V, labels, lo, hi in [c for c in HAND_CASES if c[0] <= 6] + [(6, 3, [0, 0], None, None), (7, 2, [0, 0, 0], None, None)]:
        N = count_paths(T, labels, lo, hi)
        assert N == len(feasible_paths(T, V, labels, V - 1, lo, hi)), (T, V, labels)
        ref = entropy_ctc_ref(np.full((T, V), 0.7), labels, 0.3, V - 1, lo, hi)
        if N == 0:
            assert ref["loss"] == np.inf and ref["entropy"] == 0.0
        else:
            assert abs(ref["entropy"] - np.log(N)) < 1e-12, (T, V, labels, N)
            assert abs(ref["loss"] - (T * np.log(V) - np.log(N))) < 1e-12
    T, V, L = 40, 8, 10
    labels = rng.randint(0, V - 1, L)
    labels[4] = labels[3]                                            # a repeated pair
    N = count_paths(T, labels)
    assert N > 10 ** 9
    ref = entropy_ctc_ref(np.full((T, V), -1.3), labels, 1.0, V - 1)
    assert abs(ref["entropy"] - np.log(N)) < 1e-10 * np.log(N), (ref["entropy"], np.log(N))
    lo, hi = np.arange(L) * 3, np.arange(L) * 3 + 12
    Nw = count_paths(T, labels, lo, hi)
    assert 1 < Nw < N
    assert abs(entropy_ctc_ref(np.full((T, V), -1.3), labels, 1.0, V - 1, lo, hi)["entropy"] - np.log(Nw)) < 1e-10 * np.log(Nw)


def test_edge_values_and_eta_zero_is_windowed_ctc():
    rng = np.random.RandomState(34)
    for T, V, labels in ((5, 4, [0, 1, 2, 0, 1]), (3, 3, []), (1, 2, [0]), (4, 5, [3, 1, 0, 2])):      # T = L without repeats, L = 0
        ref = entropy_ctc_ref(rng.randn(T, V) * 2, labels, 0.7, V - 1)
        assert np.isfinite(ref["loss"]) and abs(ref["entropy"]) < 1e-12, (T, labels, ref["entropy"])
        plain = entropy_ctc_ref(rng.randn(T, V) * 2, labels, 0.0, V - 1)
        assert abs(plain["entropy"]) < 1e-12
    x, labels, lo, hi = _windowed_case(4, T=14, V=5, labels=(1, 1, 0, 3, 2))
    L = len(labels)
    for win, wref in (((None, None), (np.zeros(L), np.full(L, OPEN))), ((lo, hi), (lo, hi))):
        got = entropy_ctc_ref(x, labels, 0.0, 4, *win)
        want = windowed_ctc_ref(x, labels, wref[0], wref[1], 4)
        assert got["loss"] == want["loss"] and got["entropy"] > 0
        assert np.abs(got["grad"] - want["grad"]).max() < 1e-15
        some = entropy_ctc_ref(x, labels, 0.4, 4, *win)
        assert some["loss"] == want["loss"] and some["entropy"] == got["entropy"]      # neither depends on eta


@pytest.mark.parametrize("windows", [False, True])
def test_rows_sum_to_zero(windows):
    x, labels, lo, hi = _windowed_case(5, T=14, V=5, labels=(1, 1, 0, 3, 2))
    for eta in (0.0, 0.2, 1.0, 3.0):
        ref = entropy_ctc_ref(x, labels, eta, 4, *((lo, hi) if windows else (None, None)))
        assert np.isfinite(ref["loss"])
        assert np.abs(ref["gamma"].sum(axis=1) - 1.0).max() < 1e-11
        tilt = (ref["gamma"] * np.where(ref["gamma"] > 0, ref["ebar"] - ref["c"], 0.0)).sum(axis=1)
        assert np.abs(tilt).max() < 1e-10, eta                               # sum_s gamma (Ebar - c) = 0 on every frame
        assert np.abs(ref["grad"].sum(axis=1)).max() < 1e-10, eta            # so live gradient rows still sum to 0


# ----------------------------------------------------------------------------------------------- command line
def _run(cli, *args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", cli)] + list(args), capture_output=True, timeout=120)
    return r.returncode, r.stderr.decode()


@pytest.mark.parametrize("cli", ("nnet-train.py", "nnet-validate.py"))
def test_cli_entropy_weight_fatal_paths_before_the_device(cli, tmp_path):
    """--entropy-weight negative, not finite, with another objective than ctc or with --delay-penalty: one FATAL line naming
    the flag and exit 1, decided on the host - the same on a box with and without a GPU."""
    scp = tmp_path / "t.scp"
    scp.write_text("utt0 5 3 1 %s\n" % (tmp_path / "utt0.tfrecords"))
    argv = [str(scp), "nnet.config", "nnet.in"] + (["nnet.out"] if cli == "nnet-train.py" else [])
    for flags in (["--objective", "ctc", "--entropy-weight=-0.1"], ["--objective", "ctc", "--entropy-weight", "nan"],
                  ["--objective", "ctc", "--entropy-weight", "inf"], ["--objective", "xent", "--entropy-weight", "0.1"],
                  ["--objective", "kd", "--entropy-weight", "0.1"], ["--entropy-weight", "0"],      # xent is the default objective
                  ["--objective", "ctc", "--entropy-weight", "0.1", "--delay-penalty", "0.05"],
                  ["--objective", "ctc", "--entropy-weight", "0", "--delay-penalty", "0"]):
        rc, err = _run(cli, *(flags + argv))
        fatal = [l for l in err.splitlines() if l.startswith("FATAL:tensorflow:")]
        assert rc == 1 and len(fatal) == 1, (flags, err)
        assert "--entropy-weight" in fatal[0] and "no GPU" not in fatal[0], (flags, err)


def test_cli_help_names_the_flag_and_nnet_init_has_none():
    for cli, has in (("nnet-train.py", True), ("nnet-validate.py", True), ("nnet-init.py", False)):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", cli), "--help"], capture_output=True, timeout=120)
        assert r.returncode == 0 and (b"--entropy-weight" in r.stdout) == has, cli


def test_entropy_keywords():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_common_for_entropy_test", os.path.join(ROOT, "bin", "_common.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    parser = mod.build_cli(("tfrecords_scp",), ("--objective", "--delay-penalty", "--entropy-weight"))
    assert mod.FLAGS["--entropy-weight"]["default"] is None
    assert mod.entropy_keywords(parser.parse_args(["x.scp", "--objective", "ctc"])) == {}
    assert mod.entropy_keywords(parser.parse_args(["x.scp"])) == {}                                 # no flag: any objective
    assert mod.entropy_keywords(parser.parse_args(["x.scp", "--objective", "ctc", "--delay-penalty", "0.1"])) == {}
    assert mod.entropy_keywords(parser.parse_args(["x.scp", "--objective", "ctc", "--entropy-weight", "0"])) == {"entropy_weight": 0.0}
    assert mod.entropy_keywords(parser.parse_args(["x.scp", "--objective", "ctc", "--entropy-weight", "0.2"])) == {"entropy_weight": 0.2}


# ----------------------------------------------------------------------------------------------- library
SMOKE_CFG = dict(nnet_type="blstm", input_dim=8, left_context=0, right_context=0, num_layers=2, num_neurons=32,
                 num_projects=16, num_targets=11, use_peepholes=True, dropout_rate=1.0)


def test_graph_keyword_is_validated_before_a_model_is_built():
    import inspect
    from lstm_ctc_amd.nnet import graph
    for bad in (dict(objective="xent", entropy_weight=0.1), dict(objective="kd", entropy_weight=0.1), dict(entropy_weight=-0.1),
                dict(entropy_weight=True), dict(entropy_weight=float("nan")), dict(entropy_weight=float("inf")),
                dict(entropy_weight="0.1"), dict(entropy_weight=0.1, delay_penalty=0.05), dict(entropy_weight=0, delay_penalty=0)):
        with pytest.raises(ValueError, match="entropy_weight"):
            graph.CTCGraph(None, SMOKE_CFG, seed=1, device="cpu", **bad)
    for factory in (graph.create_graph_for_training_ctc, graph.create_graph_for_validation_ctc):
        # the factories forward the criterion options to CTCGraph, where the keyword and its default live
        assert "criterion" in inspect.signature(factory).parameters
        assert inspect.signature(graph.CTCGraph.__init__).parameters["entropy_weight"].default is None
        with pytest.raises(ValueError, match="entropy_weight"):
            factory(None, SMOKE_CFG, **dict({"learn_rate": 1e-3} if "training" in factory.__name__ else {}, entropy_weight=-1.0))
        with pytest.raises(ValueError, match="delay_penalty"):
            factory(None, SMOKE_CFG, **dict({"learn_rate": 1e-3} if "training" in factory.__name__ else {}, entropy_weight=0.2,
                                            delay_penalty=0.1))


def test_workspace_query_and_version():
    import __graft_entry__ as g
    g.build()
    from lstm_ctc_amd import _lib
    lib = _lib.load()
    assert lib.lc_version() >= 10
    q, qw = lib.lc_ctc_entropy_workspace_bytes, lib.lc_ctc_window_workspace_bytes
    small, big = q(10, 2, 5, 3), q(1000, 64, 44, 100)
    assert small > qw(10, 2, 5, 3) > 0
    assert big >= 4 * 1000 * 64 * 256 * 8                            # both lattices and both lattices of means
    assert big >= qw(1000, 64, 44, 100) + 2 * 1000 * 64 * 256 * 8
    assert q(10, 2, 5, 0) > qw(10, 2, 5, 0) and q(1, 1, 2, 1023) > qw(1, 1, 2, 1023)
    assert q(20, 2, 5, 3) > small and q(10, 2, 5, 40) > small
    for bad in ((0, 2, 5, 3), (10, 0, 5, 3), (10, 2, 1, 3), (10, 2, 5, -1), (10, 2, 5, 1024), (-1, 2, 5, 3)):
        assert q(*bad) == 0, bad
    assert hasattr(lib, "lc_ctc_loss_entropy")
