"""Host side of alignment-windowed CTC: the float64 reference the GPU tests compare against (anchored here against brute-force
enumeration of all V^T paths, before a GPU is involved), ``ops.label_windows``, the --align-window flag's FATAL paths and the
workspace query.  No GPU needed.

The reference (``windowed_ctc_ref``) is the alpha-beta recursion over the extended label sequence (blank, l_0, blank, ...,
blank; S = 2L + 1) with the library's ctc_merge_repeated transitions, the emission of position 2i + 1 at frame t set to -inf
outside [lo_i, hi_i]; loss = -logsumexp of the two end cells; occupancy = exp(alpha + beta - emission - loglik) summed per
class; gradient = softmax - occupancy.  tests/test_gpu_ctc_window.py imports it from here."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPEN = np.iinfo(np.int32).max


# ----------------------------------------------------------------------------------------------- reference
def log_softmax64(x):
    x = np.asarray(x, np.float64)
    m = x.max(axis=-1, keepdims=True)
    return x - (m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True)))


def _lse(*terms):
    with np.errstate(invalid="ignore"):
        out = terms[0]
        for v in terms[1:]:
            out = np.logaddexp(out, v)
    return out


def _shr(a, n):
    """a shifted towards higher positions by n, -inf shifted in."""
    return np.concatenate((np.full(n, -np.inf), a))[:len(a)]


def _shl(a, n):
    return np.concatenate((a, np.full(n, -np.inf)))[n:]


def windowed_ctc_ref(x, labels, lo, hi, blank):
    """x [T,V] logits of the LIVE frames (T >= 1), labels [L], lo / hi [L] -> dict: ``loss`` (+inf without a surviving path),
    ``grad`` [T,V] (the softmax then), and the lattice in natural logs: ``alpha`` and ``beta`` [T,S] (both INCLUDE the
    frame's emission), ``emis`` [T,S] (masked), ``gamma`` [T,S] occupancies, ``ext`` [S]."""
    lp = log_softmax64(x)
    T, V = lp.shape
    labels = np.asarray(labels, np.int64).reshape(-1)
    L = len(labels)
    S = 2 * L + 1
    ext = np.full(S, blank, np.int64)
    ext[1::2] = labels
    emis = lp[:, ext].copy()
    if L:
        t = np.arange(T)[:, None]
        inside = (t >= np.asarray(lo, np.int64)[None, :]) & (t <= np.asarray(hi, np.int64)[None, :])
        emis[:, 1::2] = np.where(inside, emis[:, 1::2], -np.inf)
    skip_in = np.zeros(S, bool)                           # may s be entered from s - 2
    skip_in[3::2] = ext[3::2] != ext[1:-2:2]
    skip_out = np.zeros(S, bool)                          # may s move on to s + 2
    skip_out[1:-2:2] = skip_in[3::2]
    ninf = -np.inf
    alpha = np.full((T, S), ninf)
    a = np.full(S, ninf)
    a[0] = 0.0                                            # "before frame 0": frame 0 reaches positions 0 and 1
    for t in range(T):
        a = _lse(a, _shr(a, 1), np.where(skip_in, _shr(a, 2), ninf)) + emis[t]
        alpha[t] = a
    beta = np.full((T, S), ninf)
    b = np.full(S, ninf)
    b[S - 1] = 0.0                                        # "behind the last frame": it is reached from S-1 and S-2
    for t in range(T - 1, -1, -1):
        b = _lse(b, _shl(b, 1), np.where(skip_out, _shl(b, 2), ninf)) + emis[t]
        beta[t] = b
    ll = alpha[T - 1, S - 1] if S < 2 else float(_lse(alpha[T - 1, S - 1], alpha[T - 1, S - 2]))
    soft = np.exp(lp)
    out = {"alpha": alpha, "beta": beta, "emis": emis, "ext": ext, "loglik": ll}
    if not np.isfinite(ll):
        out.update(loss=np.inf, grad=soft, gamma=np.zeros((T, S)))
        return out
    live = np.isfinite(alpha) & np.isfinite(beta) & np.isfinite(emis)
    with np.errstate(invalid="ignore"):
        gamma = np.where(live, np.exp(np.where(live, alpha + beta - emis - ll, 0.0)), 0.0)
    occ = np.zeros((T, V))
    np.add.at(occ, (np.arange(T)[:, None], ext[None, :]), gamma)
    out.update(loss=-ll, grad=soft - occ, gamma=gamma)
    return out


def viterbi_ref(x, labels, blank):
    """Best path's log-probability and its lattice position per frame (float64; ties: stay, s-1, s-2; S-1 at the end)."""
    lp = log_softmax64(x)
    T = lp.shape[0]
    labels = np.asarray(labels, np.int64)
    S = 2 * len(labels) + 1
    ext = np.full(S, blank, np.int64)
    ext[1::2] = labels
    skip_in = np.zeros(S, bool)
    skip_in[3::2] = ext[3::2] != ext[1:-2:2]
    a = np.full(S, -np.inf)
    a[0] = 0.0
    bp = np.zeros((T, S), np.int64)
    for t in range(T):
        best, code = a.copy(), np.zeros(S, np.int64)
        p1, p2 = _shr(a, 1), np.where(skip_in, _shr(a, 2), -np.inf)
        m = p1 > best
        best[m], code[m] = p1[m], 1
        m = p2 > best
        best[m], code[m] = p2[m], 2
        a, bp[t] = best + lp[t, ext], code
    end = S - 1 if S < 2 or a[S - 1] >= a[S - 2] else S - 2
    if not np.isfinite(a[end]):
        return -np.inf, None
    states = np.zeros(T, np.int64)
    s = end
    for t in range(T - 1, -1, -1):
        states[t] = s
        s -= bp[t, s] if t > 0 else 0
    return float(a[end]), states


def random_path(rng, labels, T):
    """A random valid CTC path: lattice position per frame, or None when the labels do not fit T frames."""
    labels = list(labels)
    L = len(labels)
    need = L + sum(1 for i in range(1, L) if labels[i] == labels[i - 1])
    if need > T:
        return None
    # the units the path must contain, in order: label positions and the blanks between equal neighbours
    units = []
    for i in range(L):
        if i and labels[i] == labels[i - 1]:
            units.append(2 * i)
        units.append(2 * i + 1)
    # optional blanks: 0, 2, .., 2L except the forced ones; a random subset of them, as far as the frames allow
    forced = set(units)
    optional = [s for s in range(0, 2 * L + 1, 2) if s not in forced and rng.rand() < 0.5]
    if len(optional) > T - len(units):
        optional = list(rng.permutation(optional)[:T - len(units)])
    chosen = sorted(units + [int(s) for s in optional]) or [0]
    extra = rng.multinomial(T - len(chosen), np.ones(len(chosen)) / len(chosen)) if chosen else []
    return np.repeat(np.asarray(chosen, np.int64), 1 + np.asarray(extra, np.int64))


def path_symbols(states, labels, blank):
    """Symbol per frame of a path given as lattice positions: what lc_ctc_align writes as ``ali``."""
    states = np.asarray(states, np.int64)
    out = np.full(len(states), blank, np.int32)
    odd = states % 2 == 1
    out[odd] = np.asarray(labels, np.int64)[states[odd] // 2]
    return out


def brute_force(x, labels, lo, hi, blank):
    """Total probability of the paths that collapse to ``labels`` with every label inside its window, and the occupancy
    [T,V] of the classes under those paths, by enumeration of all V^T paths."""
    p = np.exp(log_softmax64(x))
    T, V = p.shape
    total, occ = 0.0, np.zeros((T, V))
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
        if any(r[1] < lo[i] or r[2] > hi[i] for i, r in enumerate(runs)):
            continue
        w = float(np.prod(p[np.arange(T), path]))
        total += w
        occ[np.arange(T), path] += w
    return total, occ


# ----------------------------------------------------------------------------------------------- the reference is right
def test_reference_matches_enumeration_of_all_paths():
    """30 random cases (T <= 6, V = 3): windows from ``ops.label_windows`` around a random valid path, widened or shifted at
    random so that feasible, tight and infeasible ones all occur."""
    from lstm_ctc_amd import ops
    rng = np.random.RandomState(11)
    V, blank = 3, 2
    kinds = {"finite": 0, "inf": 0}
    for case in range(30):
        T = int(rng.randint(1, 7))
        L = int(rng.randint(0, min(T, 3) + 1))
        labels = rng.randint(0, V - 1, L)
        x = rng.randn(T, V) * 1.5
        states = random_path(rng, labels, T)
        if states is not None:
            row = path_symbols(states, labels, blank)[None, :]
            lo, hi, ok = ops.label_windows(row, labels.astype(np.int32), np.array([0, L], np.int32), np.array([T], np.int32),
                                           int(rng.randint(0, 3)), blank)
            assert ok[0]
            lo, hi = lo.astype(np.int64), hi.astype(np.int64)
        else:
            lo, hi = np.zeros(L, np.int64), np.full(L, T - 1, np.int64)
        if case % 3 == 1 and L:                          # disturb: shifts and empty windows
            lo = lo + rng.randint(-1, 3, L)
            hi = np.minimum(hi, T + 1) - rng.randint(0, 3, L)
        ref = windowed_ctc_ref(x, labels, lo, hi, blank)
        total, occ = brute_force(x, labels, lo, hi, blank)
        if total == 0.0:
            kinds["inf"] += 1
            assert ref["loss"] == np.inf and np.array_equal(ref["grad"], np.exp(log_softmax64(x)))
            continue
        kinds["finite"] += 1
        assert abs(ref["loss"] + np.log(total)) < 1e-10, (case, ref["loss"], -np.log(total))
        want = np.exp(log_softmax64(x)) - occ / total
        assert np.abs(ref["grad"] - want).max() < 1e-10, case
        assert np.abs(ref["grad"].sum(axis=1)).max() < 1e-12
    assert kinds["finite"] >= 10 and kinds["inf"] >= 2, kinds


def test_reference_gradient_is_the_derivative_of_its_loss():
    from lstm_ctc_amd import ops
    rng = np.random.RandomState(5)
    T, V, blank = 9, 4, 3
    labels = np.array([1, 1, 0, 2])
    x = rng.randn(T, V)
    states = random_path(rng, labels, T)
    lo, hi, ok = ops.label_windows(path_symbols(states, labels, blank)[None, :], labels.astype(np.int32),
                                   np.array([0, 4], np.int32), np.array([T], np.int32), 1, blank)
    assert ok[0]
    ref = windowed_ctc_ref(x, labels, lo, hi, blank)
    assert np.isfinite(ref["loss"])
    h = 1e-5
    num = np.zeros_like(x)
    for t in range(T):
        for k in range(V):
            xp, xm = x.copy(), x.copy()
            xp[t, k] += h
            xm[t, k] -= h
            num[t, k] = (windowed_ctc_ref(xp, labels, lo, hi, blank)["loss"]
                         - windowed_ctc_ref(xm, labels, lo, hi, blank)["loss"]) / (2 * h)
    assert np.abs(num - ref["grad"]).max() < 1e-6


def test_reference_tightening_windows_never_lowers_the_loss():
    """T = 60, V = 8, L = 12, windows around the Viterbi path: unconstrained <= tau 10 <= 3 <= 1 <= 0 <= -score."""
    from lstm_ctc_amd import ops
    rng = np.random.RandomState(3)
    T, V, L, blank = 60, 8, 12, 7
    x = rng.randn(T, V) * 2.0
    labels = rng.randint(0, V - 1, L)
    score, states = viterbi_ref(x, labels, blank)
    row = path_symbols(states, labels, blank)[None, :]
    offs, seq = np.array([0, L], np.int32), np.array([T], np.int32)
    chain = [windowed_ctc_ref(x, labels, np.zeros(L), np.full(L, T), blank)["loss"]]
    for tau in (10, 3, 1, 0):
        lo, hi, ok = ops.label_windows(row, labels.astype(np.int32), offs, seq, tau, blank)
        assert ok[0]
        chain.append(windowed_ctc_ref(x, labels, lo, hi, blank)["loss"])
    chain.append(-score)
    assert all(np.isfinite(chain)) and all(a <= b + 1e-9 for a, b in zip(chain, chain[1:])), chain
    assert chain[0] < chain[-2] < chain[-1]


# ----------------------------------------------------------------------------------------------- ops.label_windows
def test_label_windows_on_hand_made_rows():
    from lstm_ctc_amd import ops
    blank = 9
    rows = np.array([
        [9, 3, 3, 9, 3, 5, 5, 9, -1, -1],       # labels 3 3 5 (equal neighbours, separated by a blank), 8 frames
        [9, 9, 9, 9, -1, -1, -1, -1, -1, -1],   # L = 0, all blank: qualifies
        [9, 1, -1, 2, 9, 9, 9, 9, 9, 9],        # a -1 inside the row
        [1, 9, 2, 9, 9, 9, 9, 9, 9, 9],         # spells 1 2, the labels are 1 4
        [7, 7, 9, 9, 9, 9, 9, 9, 9, 8],         # windows pushed past both ends
        [-1] * 10,                              # what the pipeline hands out for a missing entry
        [4, 4, 4, 4, 4, 4, 4, 4, 4, 4],         # one run for two equal labels: does not spell them
    ], np.int32)
    seq = np.array([8, 4, 10, 10, 10, 10, 10], np.int32)
    labels = [[3, 3, 5], [], [1, 2], [1, 4], [7, 8], [2], [4, 4]]
    flat = np.array([l for ls in labels for l in ls], np.int32)
    offs = np.concatenate(([0], np.cumsum([len(ls) for ls in labels]))).astype(np.int32)
    lo, hi, ok = ops.label_windows(rows, flat, offs, seq, 2, blank)
    assert lo.dtype == np.int32 and hi.dtype == np.int32 and ok.dtype == bool
    assert ok.tolist() == [True, True, False, False, True, False, False]
    assert lo[0:3].tolist() == [-1, 2, 3] and hi[0:3].tolist() == [4, 6, 8]
    for a, b in ((3, 5), (5, 7), (9, 10), (10, 12)):                       # unconstrained: lo = 0, hi = INT32_MAX
        assert lo[a:b].tolist() == [0] * (b - a) and hi[a:b].tolist() == [OPEN] * (b - a)
    assert lo[7:9].tolist() == [-2, 7] and hi[7:9].tolist() == [3, 11]
    # tau = 0: exactly the runs; a huge tau saturates instead of wrapping
    lo0, hi0, _ = ops.label_windows(rows, flat, offs, seq, 0, blank)
    assert lo0[0:3].tolist() == [1, 4, 5] and hi0[0:3].tolist() == [2, 4, 6]
    lob, hib, okb = ops.label_windows(rows, flat, offs, seq, OPEN, blank)
    assert okb.tolist() == ok.tolist() and (lob[0:3] < 0).all() and hib[0:3].tolist() == [OPEN] * 3
    # frames beyond seq_len are not looked at: the same rows with garbage behind the utterances
    rows2 = rows.copy()
    rows2[0, 8:], rows2[1, 4:] = 5, 3
    lo2, hi2, ok2 = ops.label_windows(rows2, flat, offs, seq, 2, blank)
    assert np.array_equal(lo2, lo) and np.array_equal(hi2, hi) and np.array_equal(ok2, ok)


def test_label_windows_never_raises_for_content():
    from lstm_ctc_amd import ops
    rng = np.random.RandomState(0)
    for _ in range(50):
        B, T = int(rng.randint(1, 4)), int(rng.randint(1, 8))
        rows = rng.randint(-3, 6, (B, T)).astype(np.int32)
        lens = rng.randint(0, 4, B)
        flat = rng.randint(-2, 7, int(lens.sum())).astype(np.int32)
        offs = np.concatenate(([0], np.cumsum(lens))).astype(np.int32)
        seq = rng.randint(-1, T + 3, B).astype(np.int32)
        lo, hi, ok = ops.label_windows(rows, flat, offs, seq, int(rng.randint(0, 4)), 4)
        assert lo.shape == hi.shape == flat.shape and ok.shape == (B,)


# ----------------------------------------------------------------------------------------------- command line
def _run(cli, *args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", cli)] + list(args), capture_output=True, timeout=120)
    return r.returncode, r.stderr.decode()


def _argv(cli, tmp_path):
    scp = tmp_path / "t.scp"
    scp.write_text("utt0 5 3 1 %s\n" % (tmp_path / "utt0.tfrecords"))
    table = tmp_path / "ali.txt"
    table.write_text("utt0 4 0 4 1 4 \n")
    return str(table), [str(scp), "nnet.config", "nnet.in"] + (["nnet.out"] if cli == "nnet-train.py" else [])


@pytest.mark.parametrize("cli", ("nnet-train.py", "nnet-validate.py"))
def test_cli_align_window_fatal_paths_before_the_device(cli, tmp_path):
    """--align-window without a table, negative, or with --objective xent: one FATAL line naming the flag and exit 1, decided
    on the host - the same on a box with and without a GPU."""
    table, argv = _argv(cli, tmp_path)
    for flags in (["--objective", "ctc", "--align-window", "2"],
                  ["--objective", "ctc", "--align-window", "-1", "--frame-targets", "ark,t:" + table],
                  ["--objective", "xent", "--align-window", "2", "--frame-targets", "ark,t:" + table],
                  ["--align-window", "2", "--frame-targets", "ark,t:" + table]):          # xent is the default objective
        rc, err = _run(cli, *(flags + argv))
        fatal = [l for l in err.splitlines() if l.startswith("FATAL:tensorflow:")]
        assert rc == 1 and len(fatal) == 1, (flags, err)
        assert "--align-window" in fatal[0] and "no GPU" not in fatal[0], (flags, err)


def test_cli_help_names_the_flag_and_nnet_init_has_none():
    for cli, has in (("nnet-train.py", True), ("nnet-validate.py", True), ("nnet-init.py", False)):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", cli), "--help"], capture_output=True, timeout=120)
        assert r.returncode == 0 and (b"--align-window" in r.stdout) == has, cli


def test_read_frame_targets_reads_the_table_for_windowed_ctc(tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location("_common_for_window_test", os.path.join(ROOT, "bin", "_common.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    table, argv = _argv("nnet-validate.py", tmp_path)
    parser = mod.build_cli(("tfrecords_scp",), ("--objective", "--frame-targets", "--align-window"))
    args = parser.parse_args([argv[0], "--objective", "ctc", "--frame-targets", "ark,t:" + table, "--align-window", "0"])
    got = mod.read_frame_targets(args)
    assert list(got) == ["utt0"] and got["utt0"].tolist() == [4, 0, 4, 1, 4]
    # plain ctc still reads nothing, with or without a table
    assert mod.read_frame_targets(parser.parse_args([argv[0], "--objective", "ctc"])) is None
    assert mod.read_frame_targets(parser.parse_args([argv[0], "--objective", "ctc", "--frame-targets", "ark,t:" + table])) is None


# ----------------------------------------------------------------------------------------------- library
def test_workspace_query():
    import __graft_entry__ as g
    g.build()
    from lstm_ctc_amd import _lib
    lib = _lib.load()
    assert lib.lc_version() >= 4
    q = lib.lc_ctc_window_workspace_bytes
    small, big = q(10, 2, 5, 3), q(1000, 64, 44, 100)
    assert small > 0 and big >= 2 * 1000 * 64 * 256 * 8          # both lattices: T * B * roundup(2L + 1, 64) doubles each
    assert q(10, 2, 5, 0) > 0 and q(1, 1, 2, 1023) > 0
    assert q(20, 2, 5, 3) > small and q(10, 2, 5, 40) > small
    for bad in ((0, 2, 5, 3), (10, 0, 5, 3), (10, 2, 1, 3), (10, 2, 5, -1), (10, 2, 5, 1024), (-1, 2, 5, 3)):
        assert q(*bad) == 0, bad
