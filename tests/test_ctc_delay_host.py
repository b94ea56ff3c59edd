"""Host side of delay-penalised CTC: the float64 reference the GPU tests compare against (anchored here against brute-force
enumeration of all V^T paths, before a GPU is involved), the identities the criterion obeys, the --delay-penalty flag's FATAL
paths and the workspace query.  No GPU needed.

The criterion: with e_j(path) the first frame of label j's run and E(path) = sum_j e_j(path),
    loss = -log sum_path p(path | x) exp(-lambda E(path)),
    grad = softmax - occupancy under q(path) ~ p(path | x) exp(-lambda E(path)),
    entry_sum = E_q[E] = sum_t sum_s gamma(t, s) (L - (s + 1) // 2)            (labels not yet entered at position s).
The reference (``delay_ctc_ref``) is ``windowed_ctc_ref``'s alpha-beta recursion with the weight -lambda t on every arc that
ENTERS a label position (odd s, from s-1 or s-2) at frame t; "stay" arcs and arcs into blanks carry none.  The beta recursion
walks the same arcs backwards: the arc s -> s' taken between frames t and t + 1 carries -lambda (t + 1) when s' is odd.
tests/test_gpu_ctc_delay.py imports it from here."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

from test_ctc_window_host import OPEN, _lse, _shl, _shr, log_softmax64, path_symbols, random_path, windowed_ctc_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------------------------- reference
def delay_ctc_ref(x, labels, lam, blank, lo=None, hi=None):
    """x [T,V] logits of the LIVE frames (T >= 1), labels [L], lam = delay penalty, optional windows lo / hi [L] -> dict:
    ``loss`` (+inf without a surviving path), ``grad`` [T,V] (the softmax then), ``entry_sum`` (0 then), and the lattice in
    natural logs: ``alpha`` and ``beta`` [T,S] (both INCLUDE the frame's emission and the weights of the arcs behind /
    ahead of them), ``emis`` [T,S] (masked), ``gamma`` [T,S] occupancies, ``ext`` [S]."""
    lp = log_softmax64(x)
    T, V = lp.shape
    labels = np.asarray(labels, np.int64).reshape(-1)
    L = len(labels)
    S = 2 * L + 1
    lam = float(lam)
    ext = np.full(S, blank, np.int64)
    ext[1::2] = labels
    emis = lp[:, ext].copy()
    if L and lo is not None:
        t = np.arange(T)[:, None]
        inside = (t >= np.asarray(lo, np.int64)[None, :]) & (t <= np.asarray(hi, np.int64)[None, :])
        emis[:, 1::2] = np.where(inside, emis[:, 1::2], -np.inf)
    odd = (np.arange(S) % 2 == 1).astype(np.float64)
    even_src = 1.0 - odd                                  # 1 where s + 1 is a label position (beyond S - 1 the arc is -inf)
    skip_in = np.zeros(S, bool)                           # may s be entered from s - 2
    skip_in[3::2] = ext[3::2] != ext[1:-2:2]
    skip_out = np.zeros(S, bool)                          # may s move on to s + 2
    skip_out[1:-2:2] = skip_in[3::2]
    ninf = -np.inf
    alpha = np.full((T, S), ninf)
    a = np.full(S, ninf)
    a[0] = 0.0                                            # "before frame 0": frame 0 reaches positions 0 and 1
    for t in range(T):
        w = -lam * t                                      # on the arcs into the label positions of frame t
        a = _lse(a, _shr(a, 1) + w * odd, np.where(skip_in, _shr(a, 2) + w, ninf)) + emis[t]
        alpha[t] = a
    beta = np.full((T, S), ninf)
    b = np.full(S, ninf)
    b[S - 1] = 0.0                                        # "behind the last frame": it is reached from S-1 and S-2
    for t in range(T - 1, -1, -1):
        w = -lam * (t + 1)                                # on the arcs into the label positions of frame t + 1
        b = _lse(b, _shl(b, 1) + w * even_src, np.where(skip_out, _shl(b, 2) + w, ninf)) + emis[t]
        beta[t] = b
    ll = alpha[T - 1, S - 1] if S < 2 else float(_lse(alpha[T - 1, S - 1], alpha[T - 1, S - 2]))
    soft = np.exp(lp)
    out = {"alpha": alpha, "beta": beta, "emis": emis, "ext": ext, "loglik": ll}
    if not np.isfinite(ll):
        out.update(loss=np.inf, grad=soft, gamma=np.zeros((T, S)), entry_sum=0.0)
        return out
    live = np.isfinite(alpha) & np.isfinite(beta) & np.isfinite(emis)
    with np.errstate(invalid="ignore"):
        gamma = np.where(live, np.exp(np.where(live, alpha + beta - emis - ll, 0.0)), 0.0)
    occ = np.zeros((T, V))
    np.add.at(occ, (np.arange(T)[:, None], ext[None, :]), gamma)
    notyet = L - (np.arange(S) + 1) // 2
    out.update(loss=-ll, grad=soft - occ, gamma=gamma, entry_sum=float((gamma * notyet[None, :]).sum()))
    return out


def brute_force_delay(x, labels, lam, blank, lo=None, hi=None):
    """(sum of p(path) exp(-lam E(path)), class occupancy [T,V] and sum of E(path), both under those weights) over the paths
    that collapse to ``labels`` with every label inside its window, by enumeration of all V^T paths."""
    p = np.exp(log_softmax64(x))
    T, V = p.shape
    total, occ, esum = 0.0, np.zeros((T, V)), 0.0
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
        E = sum(r[1] for r in runs)
        w = float(np.prod(p[np.arange(T), path])) * np.exp(-lam * E)
        total += w
        occ[np.arange(T), path] += w
        esum += w * E
    return total, occ, esum


# ----------------------------------------------------------------------------------------------- the reference is right
HAND_CASES = [                                           # (T, V, labels, lambda, lo, hi)
    (5, 3, [1, 1], 0.7, None, None),                     # a repeated label: the blank between is forced
    (6, 3, [0, 0, 1], 0.3, None, None),
    (4, 4, [], 0.5, None, None),                         # L = 0: the all-blank path, E = 0
    (5, 4, [2, 0], -0.6, None, None),                    # lambda < 0 rewards late entries
    (5, 3, [0, 1], 0.0, None, None),                     # lambda = 0: plain CTC
    (2, 3, [1, 1], 0.4, None, None),                     # L fits the frames, the blank between the equal labels does not
    (1, 2, [0], 2.0, None, None),                        # T = 1
    (6, 4, [1, 2, 1], 1.5, [0, 1, 3], [2, 4, 5]),        # windows
    (6, 3, [0, 1], 0.9, [2, 0], [5, 1]),                 # windows no monotone path satisfies
]


def _check_against_enumeration(T, V, labels, lam, lo, hi, x, tag):
    blank = V - 1
    ref = delay_ctc_ref(x, labels, lam, blank, lo, hi)
    total, occ, esum = brute_force_delay(x, labels, lam, blank, lo, hi)
    soft = np.exp(log_softmax64(x))
    if total == 0.0:
        assert ref["loss"] == np.inf and ref["entry_sum"] == 0.0 and np.array_equal(ref["grad"], soft), tag
        return False
    assert abs(ref["loss"] + np.log(total)) < 1e-10, (tag, ref["loss"], -np.log(total))
    assert np.abs(ref["grad"] - (soft - occ / total)).max() < 1e-10, tag
    assert abs(ref["entry_sum"] - esum / total) < 1e-10, (tag, ref["entry_sum"], esum / total)
    assert np.abs(ref["gamma"].sum(axis=1) - 1.0).max() < 1e-12, tag
    return True


def test_reference_matches_enumeration_of_all_paths():
    rng = np.random.RandomState(21)
    finite = []
    for i, (T, V, labels, lam, lo, hi) in enumerate(HAND_CASES):
        finite.append(_check_against_enumeration(T, V, labels, lam, lo, hi, rng.randn(T, V) * 1.5, "hand %d" % i))
    assert finite == [True, True, True, True, True, False, True, True, False]
    kinds = {"finite": 0, "inf": 0}
    for case in range(30):                               # random cases, windows around a random path, sometimes disturbed
        T = int(rng.randint(1, 7))
        V = int(rng.randint(2, 5))
        L = int(rng.randint(0, min(T, 3) + 1))
        labels = rng.randint(0, V - 1, L)
        lam = float(rng.choice([0.0, 0.05, 1.0, 3.0, -0.5]))
        lo = hi = None
        states = random_path(rng, labels, T)
        if case % 2 and L and states is not None:
            lo = np.array([np.flatnonzero(states == 2 * i + 1)[0] for i in range(L)]) - rng.randint(0, 2, L)
            hi = np.array([np.flatnonzero(states == 2 * i + 1)[-1] for i in range(L)]) + rng.randint(0, 2, L)
            if case % 3 == 1:
                lo = lo + rng.randint(-1, 3, L)
                hi = hi - rng.randint(0, 3, L)
        ok = _check_against_enumeration(T, V, list(labels), lam, lo, hi, rng.randn(T, V) * 1.5, "random %d" % case)
        kinds["finite" if ok else "inf"] += 1
    assert kinds["finite"] >= 10 and kinds["inf"] >= 2, kinds


def _windowed_case(seed, T=14, V=5, labels=(1, 1, 0, 3, 2)):
    rng = np.random.RandomState(seed)
    labels = np.array(labels)
    x = rng.randn(T, V) * 1.5
    states = random_path(rng, labels, T)
    lo = np.array([np.flatnonzero(states == 2 * i + 1)[0] for i in range(len(labels))]) - 2
    hi = np.array([np.flatnonzero(states == 2 * i + 1)[-1] for i in range(len(labels))]) + 2
    return x, labels, lo, hi


@pytest.mark.parametrize("windows", [False, True])
def test_gamma_rows_sum_to_one(windows):
    """Every path passes exactly one position per frame: sum_s gamma(t, s) = 1.  This is what fails when the backward sweep
    puts an arc's weight on the wrong row (the weight belongs to the arc's target frame in the forward orientation)."""
    x, labels, lo, hi = _windowed_case(1)
    for lam in (0.0, 0.05, 1.0, 4.0, -0.8):
        ref = delay_ctc_ref(x, labels, lam, 4, *((lo, hi) if windows else (None, None)))
        assert np.isfinite(ref["loss"])
        assert np.abs(ref["gamma"].sum(axis=1) - 1.0).max() < 1e-11, lam
        assert np.abs(ref["grad"].sum(axis=1)).max() < 1e-11, lam


def test_reference_gradient_is_the_derivative_of_its_loss():
    x, labels, lo, hi = _windowed_case(2, T=9, V=4, labels=(1, 1, 0, 2))
    lam, h = 0.6, 1e-5
    ref = delay_ctc_ref(x, labels, lam, 3, lo, hi)
    assert np.isfinite(ref["loss"])
    num = np.zeros_like(x)
    for t in range(x.shape[0]):
        for k in range(x.shape[1]):
            xp, xm = x.copy(), x.copy()
            xp[t, k] += h
            xm[t, k] -= h
            num[t, k] = (delay_ctc_ref(xp, labels, lam, 3, lo, hi)["loss"] - delay_ctc_ref(xm, labels, lam, 3, lo, hi)["loss"]) / (2 * h)
    assert np.abs(num - ref["grad"]).max() < 1e-6


@pytest.mark.parametrize("windows", [False, True])
def test_entry_sum_is_the_derivative_of_the_loss_in_lambda(windows):
    x, labels, lo, hi = _windowed_case(3)
    win = (lo, hi) if windows else (None, None)
    h = 1e-5
    for lam in (0.0, 0.05, 1.0, -0.4):
        num = (delay_ctc_ref(x, labels, lam + h, 4, *win)["loss"] - delay_ctc_ref(x, labels, lam - h, 4, *win)["loss"]) / (2 * h)
        got = delay_ctc_ref(x, labels, lam, 4, *win)["entry_sum"]
        assert abs(num - got) < 1e-6 * max(abs(got), 1.0), (lam, num, got)


def test_lambda_zero_is_windowed_ctc():
    x, labels, lo, hi = _windowed_case(4)
    L = len(labels)
    for win, wref in (((None, None), (np.zeros(L), np.full(L, OPEN))), ((lo, hi), (lo, hi))):
        got = delay_ctc_ref(x, labels, 0.0, 4, *win)
        want = windowed_ctc_ref(x, labels, wref[0], wref[1], 4)
        assert abs(got["loss"] - want["loss"]) < 1e-12
        for k in ("grad", "gamma", "alpha", "beta"):
            assert np.allclose(got[k], want[k], rtol=0, atol=1e-12), k


def test_sandwich_and_monotone_entry_sum():
    """loss(0) <= loss(lambda) <= loss(0) + lambda entry_sum(0) (the loss is concave in lambda with slope entry_sum), and
    entry_sum does not grow with lambda."""
    x, labels, lo, hi = _windowed_case(5, T=30)
    for win in ((None, None), (lo, hi)):
        refs = [delay_ctc_ref(x, labels, lam, 4, *win) for lam in (0.0, 0.05, 0.2, 1.0)]
        entries = [r["entry_sum"] for r in refs]
        assert all(a >= b - 1e-10 for a, b in zip(entries, entries[1:])), entries
        assert entries[0] > entries[-1] + 1e-3                    # and the penalty does pull the labels forward
        for lam, r in zip((0.05, 0.2, 1.0), refs[1:]):
            assert refs[0]["loss"] - 1e-10 <= r["loss"] <= refs[0]["loss"] + lam * entries[0] + 1e-10


# ----------------------------------------------------------------------------------------------- command line
def _run(cli, *args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", cli)] + list(args), capture_output=True, timeout=120)
    return r.returncode, r.stderr.decode()


@pytest.mark.parametrize("cli", ("nnet-train.py", "nnet-validate.py"))
def test_cli_delay_penalty_fatal_paths_before_the_device(cli, tmp_path):
    """--delay-penalty negative, not finite, or with another objective than ctc: one FATAL line naming the flag and exit 1,
    decided on the host - the same on a box with and without a GPU."""
    scp = tmp_path / "t.scp"
    scp.write_text("utt0 5 3 1 %s\n" % (tmp_path / "utt0.tfrecords"))
    argv = [str(scp), "nnet.config", "nnet.in"] + (["nnet.out"] if cli == "nnet-train.py" else [])
    for flags in (["--objective", "ctc", "--delay-penalty=-0.1"], ["--objective", "ctc", "--delay-penalty", "nan"],
                  ["--objective", "ctc", "--delay-penalty", "inf"], ["--objective", "xent", "--delay-penalty", "0.1"],
                  ["--objective", "kd", "--delay-penalty", "0.1"], ["--delay-penalty", "0"]):      # xent is the default objective
        rc, err = _run(cli, *(flags + argv))
        fatal = [l for l in err.splitlines() if l.startswith("FATAL:tensorflow:")]
        assert rc == 1 and len(fatal) == 1, (flags, err)
        assert "--delay-penalty" in fatal[0] and "no GPU" not in fatal[0], (flags, err)


def test_cli_help_names_the_flag_and_nnet_init_has_none():
    for cli, has in (("nnet-train.py", True), ("nnet-validate.py", True), ("nnet-init.py", False)):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", cli), "--help"], capture_output=True, timeout=120)
        assert r.returncode == 0 and (b"--delay-penalty" in r.stdout) == has, cli


def test_delay_keywords():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_common_for_delay_test", os.path.join(ROOT, "bin", "_common.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    parser = mod.build_cli(("tfrecords_scp",), ("--objective", "--delay-penalty"))
    assert mod.FLAGS["--delay-penalty"]["default"] is None
    assert mod.delay_keywords(parser.parse_args(["x.scp", "--objective", "ctc"])) == {}
    assert mod.delay_keywords(parser.parse_args(["x.scp"])) == {}                                   # no flag: any objective
    assert mod.delay_keywords(parser.parse_args(["x.scp", "--objective", "ctc", "--delay-penalty", "0"])) == {"delay_penalty": 0.0}
    assert mod.delay_keywords(parser.parse_args(["x.scp", "--objective", "ctc", "--delay-penalty", "0.05"])) == {"delay_penalty": 0.05}


# ----------------------------------------------------------------------------------------------- library
def test_workspace_query_and_version():
    import __graft_entry__ as g
    g.build()
    from lstm_ctc_amd import _lib
    lib = _lib.load()
    assert lib.lc_version() >= 6
    q = lib.lc_ctc_delay_workspace_bytes
    small, big = q(10, 2, 5, 3), q(1000, 64, 44, 100)
    assert small > 0 and big >= 2 * 1000 * 64 * 256 * 8 + 1000 * 64 * 8     # both lattices and a double per frame
    assert big >= lib.lc_ctc_window_workspace_bytes(1000, 64, 44, 100) + 1000 * 64 * 8
    assert q(10, 2, 5, 0) > 0 and q(1, 1, 2, 1023) > 0
    assert q(20, 2, 5, 3) > small and q(10, 2, 5, 40) > small
    for bad in ((0, 2, 5, 3), (10, 0, 5, 3), (10, 2, 1, 3), (10, 2, 5, -1), (10, 2, 5, 1024), (-1, 2, 5, 3)):
        assert q(*bad) == 0, bad
