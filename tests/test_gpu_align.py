"""lc_ctc_align (CTC forced alignment, best path through the 2L+1 lattice) on the GPU.

Reference: a float64 numpy Viterbi over the extended label sequence with the library's transition rules and tie rule
(stay over s-1 over s-2 at a cell, S-1 over S-2 at the end); brute-force enumeration of all V^T paths for the tiny cases.

Tolerances - derived from the kernel's arithmetic, not from what it was seen to give (u = 2^-24, fp32 unit round-off):

* Per frame the kernel takes ONE fp32 log-sum-exp: m = max_k x_k (exact); p_k = exp2(fl(fl(x_k - m) * log2e)) on the
  hardware exp (1 ulp); the argument carries <= 3u |a_k| (difference, constant, product), which the exponential turns into
  a relative 3u ln2 |a_k|, and p_k |a_k| <= 1 / (e ln2), so a term is off by <= 1.11u + 2u p_k; the V terms are summed in
  fp32 in a fixed order: <= (V - 1) u S.  With S >= 1 the sum's relative error is <= (2.2 V + 2) u.  ln S = log2(S) * ln2:
  hardware log2 (1 ulp), constant, product: <= 4u ln V more.  lse = fl(m + ln S): <= u (max|x| + ln V).  Together
      eps_lse <= u (2.2 V + 2 + 5 ln V + max|x|) <= u (3 V + 8 + max|x|)                       (5 ln V <= 0.8 V + 6, V >= 2).
* A cell's emission is (double) x - (double) lse: EXACT in double.  The T_b additions along a path are double additions
  (2^-53 each); there is no re-centring.  So the kernel's lattice values are the float64 sums of x - lse32 up to
  T_b 2^-53 |score|, and its decisions are exact comparisons of those.
* (c) optimality: the error of lse32 is one number per FRAME, the same for every class, and every path visits every frame
  once - it shifts all paths alike and cannot change their order.  What is left are the double roundings in the kernel and
  in this file's reference (the log-softmax and T_b additions each): tol_c = T_b 2^-50 (|optimum| + max|x| + ln V + 1).
* (b) score consistency: score - (float64 sum along the returned path) = sum_t (lse64 - lse32) + the final rounding of the
  score to fp32: tol_b = T_b eps_lse + 2u |score| + tol_c.
* Both must fit the project's bar 1e-4 max(|score|, 1) (tests/conftest.py GRAD_TOL): asserted for every utterance checked.
  (With fp32 additions along the path the bound would carry T_b u |score| and pass the bar near T = 840 - hence doubles.)
"""
import itertools
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
BAR = 1e-4                        # tests/conftest.py: GRAD_TOL, the project's bar for logits and loss
LC_EINVAL, LC_EWORKSPACE = -1, -3
MEASURED = {"b": 0.0, "c": 0.0}   # largest measured error / bound over the session (printed by the last test)


# ----------------------------------------------------------------------------------------------- reference
def log_softmax64(x):
    x = np.asarray(x, np.float64)
    m = x.max(axis=-1, keepdims=True)
    return x - (m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True)))


def viterbi_ref(lp, labels, blank):
    """lp [T,V] float64 log-softmax, labels list -> (score, states [T]) or (-inf, None).  Tie rule: stay, s-1, s-2; S-1."""
    T = lp.shape[0]
    L = len(labels)
    S = 2 * L + 1
    ext = np.full(S, blank, np.int64)
    ext[1::2] = labels
    allow2 = np.zeros(S, bool)
    allow2[3::2] = ext[3::2] != ext[1:-2:2]
    if T == 0:
        return 0.0, np.zeros(0, np.int64)
    a = np.full(S, -np.inf)
    a[0] = 0.0                                           # "before frame 0": frame 0 reaches positions 0 and 1
    bp = np.zeros((T, S), np.int8)
    for t in range(T):
        p1 = np.concatenate(([-np.inf], a))[:S]
        p2 = np.concatenate(([-np.inf, -np.inf], a))[:S]
        p2[~allow2] = -np.inf
        best, code = a.copy(), np.zeros(S, np.int8)
        m = p1 > best
        best[m], code[m] = p1[m], 1
        m = p2 > best
        best[m], code[m] = p2[m], 2
        a = best + lp[t, ext]
        bp[t] = code
    end, score = S - 1, a[S - 1]
    if S >= 2 and a[S - 2] > score:
        end, score = S - 2, a[S - 2]
    if not np.isfinite(score):
        return -np.inf, None
    states = np.zeros(T, np.int64)
    s = end
    for t in range(T - 1, -1, -1):
        states[t] = s
        if t:
            s -= int(bp[t, s])
    return float(score), states


def states_to_symbols(states, labels, blank):
    lab = np.asarray(list(labels) + [blank], np.int64)
    return np.where(states % 2 == 1, lab[np.minimum(states // 2, len(labels))], blank)


def collapse(sym, blank):
    out, prev = [], None
    for s in sym:
        if s != prev and s != blank:
            out.append(int(s))
        prev = s
    return out


def min_frames(labels):
    return len(labels) + sum(1 for i in range(1, len(labels)) if labels[i] == labels[i - 1])


# ----------------------------------------------------------------------------------------------- running the kernel
def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _flat(labels):
    offs = np.zeros(len(labels) + 1, np.int32)
    offs[1:] = np.cumsum([len(l) for l in labels])
    flat = np.asarray([v for l in labels for v in l], np.int32)
    return flat, offs


def run_align(logits, labels, seq, max_len=None, want_label_index=True):
    from lstm_ctc_amd import ops
    flat, offs = _flat(labels)
    L = max([len(l) for l in labels] + [0]) if max_len is None else max_len
    ali, idx, score = ops.ctc_align(_dev(logits, np.float32), _dev(flat, np.int32), _dev(offs, np.int32),
                                    _dev(seq, np.int32), L, want_label_index=want_label_index)
    return ali.cpu().numpy(), None if idx is None else idx.cpu().numpy(), score.cpu().numpy()


def raw_align(logits_d, flat_d, offs_d, seq_d, L, ali, idx, score, ws, nbytes):
    from lstm_ctc_amd import _lib, ops
    T, B, V = logits_d.shape
    return _lib.load().lc_ctc_align(ops._ptr(logits_d), T, B, V, ops._ptr(flat_d), ops._ptr(offs_d), ops._ptr(seq_d), L,
                                    ops._ptr(ali), ops._ptr(idx), ops._ptr(score), ops._ptr(ws), nbytes, ops._stream())


def check_properties(logits, labels, seq, ali, idx, score, optimum=None):
    """(a) validity, (b) score consistency, (c) optimality of every utterance; returns the reference scores."""
    T, B, V = logits.shape
    blank = V - 1
    xmax = float(np.abs(logits).max()) if logits.size else 0.0
    refs = []
    for b in range(B):
        Tb = min(int(seq[b]), T)
        lab = list(labels[b])
        lp = log_softmax64(logits[:Tb, b])
        opt = viterbi_ref(lp, lab, blank)[0] if optimum is None else optimum[b]
        refs.append(opt)
        assert (ali[b, Tb:] == -1).all() and (idx is None or (idx[b, Tb:] == -1).all()), b
        if Tb == 0:
            assert score[b] == 0.0, (b, score[b])
            continue
        if not np.isfinite(opt):                                   # no path: -inf and all -1
            assert score[b] == -np.inf, (b, score[b])
            assert (ali[b] == -1).all() and (idx is None or (idx[b] == -1).all()), b
            continue
        a = ali[b, :Tb]
        assert ((a >= 0) & (a < V)).all(), b
        assert collapse(a, blank) == lab, (b, collapse(a, blank), lab)                       # (a)
        if idx is not None:
            i = idx[b, :Tb]
            assert ((i == -1) == (a == blank)).all(), b
            nz = i[i >= 0]
            assert (np.diff(nz) >= 0).all() and (np.diff(nz) <= 1).all(), b
            assert len(nz) == 0 and not lab or (nz[0] == 0 and nz[-1] == len(lab) - 1), b
            assert (np.asarray(lab + [blank])[i] == a).all(), b
        path = float(lp[np.arange(Tb), a].sum())
        tol_c = Tb * 2.0 ** -50 * (abs(opt) + xmax + math.log(V) + 1)
        tol_b = Tb * U * (3 * V + 8 + xmax) + 2 * U * abs(float(score[b])) + tol_c
        bar = BAR * max(abs(opt), 1.0)
        assert tol_b <= bar, (b, tol_b, bar)                       # the derived bound fits the project's bar
        err_b, err_c = abs(float(score[b]) - path), abs(path - opt)
        MEASURED["b"] = max(MEASURED["b"], err_b / tol_b)
        MEASURED["c"] = max(MEASURED["c"], err_c / tol_c)
        print("align b=%d T=%d L=%d V=%d: |score-path|=%.3e (bound %.3e)  |path-opt|=%.3e (bound %.3e)  bar %.3e"
              % (b, Tb, len(lab), V, err_b, tol_b, err_c, tol_c, bar))
        assert err_b <= tol_b, (b, score[b], path, tol_b)                                   # (b)
        assert err_c <= tol_c, (b, path, opt, tol_c)                                        # (c)
    return refs


def random_labels(rng, L, V):
    return [int(v) for v in rng.integers(0, V - 1, size=L)]


# ----------------------------------------------------------------------------------------------- exhaustive tiny cases
ALL_SEQS = [list(s) for n in range(4) for s in itertools.product((0, 1), repeat=n)]      # 15 label sequences


@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 6, 7])
def test_exhaustive_against_enumeration(T):
    V, blank = 3, 2
    rng = np.random.default_rng(100 + T)
    B = len(ALL_SEQS)
    logits = rng.normal(0, 2, size=(T, B, V)).astype(np.float32)
    paths = np.array(list(itertools.product(range(V), repeat=T)), np.int64)                # [V^T, T]
    keys = [tuple(collapse(p, blank)) for p in paths]
    best = []
    for b, lab in enumerate(ALL_SEQS):
        lp = log_softmax64(logits[:, b])
        sums = lp[np.arange(T)[None, :], paths].sum(axis=1)
        mine = [s for s, k in zip(sums, keys) if k == tuple(lab)]
        best.append(max(mine) if mine else -np.inf)
        assert (not mine) == (min_frames(lab) > T)
    ali, idx, score = run_align(logits, ALL_SEQS, np.full(B, T, np.int32))
    check_properties(logits, ALL_SEQS, np.full(B, T), ali, idx, score, optimum=best)
    for b in range(B):                                  # -inf / all -1 exactly when the enumeration finds no path
        assert (score[b] == -np.inf) == (not np.isfinite(best[b])) == bool((ali[b] == -1).all())


# ----------------------------------------------------------------------------------------------- exact-path cases
def random_valid_path(rng, labels, T, blank):
    """A uniformly drawn run-length assignment over a random choice of optional blanks -> states [T]."""
    L = len(labels)
    while True:
        keep = [True] * (2 * L + 1)
        for s in range(0, 2 * L + 1, 2):
            mandatory = 0 < s < 2 * L and labels[s // 2 - 1] == labels[s // 2]
            keep[s] = mandatory or rng.random() < 0.5
        if L == 0:
            keep[0] = True
        states = [s for s in range(2 * L + 1) if keep[s]]
        if len(states) <= T:
            break
    cuts = np.sort(rng.choice(np.arange(1, T), size=len(states) - 1, replace=False)) if len(states) > 1 else []
    runs = np.diff(np.concatenate(([0], cuts, [T]))).astype(int)
    return np.repeat(states, runs)


@pytest.mark.parametrize("V,L,T,B", [(5, 6, 20, 3), (44, 100, 300, 2), (5, 40, 130, 1)])
def test_planted_alignment_is_returned_exactly(V, L, T, B):
    rng = np.random.default_rng(V * 1000 + L)
    blank = V - 1
    labels = [random_labels(rng, L - b, V) for b in range(B)]
    seq = np.asarray([T - 3 * b for b in range(B)], np.int32)
    logits = np.zeros((T, B, V), np.float32)
    want = np.full((B, T), -1, np.int64)
    for b in range(B):
        st = random_valid_path(rng, labels[b], int(seq[b]), blank)
        want[b, :seq[b]] = states_to_symbols(st, labels[b], blank)
        logits[np.arange(seq[b]), b, want[b, :seq[b]]] = 8.0
    ali, idx, score = run_align(logits, labels, seq)
    assert np.array_equal(ali, want)
    assert all(collapse(ali[b, :seq[b]], blank) == labels[b] for b in range(B))


@pytest.mark.parametrize("labels,T", [([[1, 1, 0, 2], [0], [2, 2, 2], []], 11),
                                      ([[i % 3 for i in range(40)], [1] * 20 + [0] * 10], 75)])
def test_exact_ties_follow_the_tie_rule(labels, T):
    V, blank = 5, 4
    B = len(labels)
    rng = np.random.default_rng(T)
    logits = np.repeat(rng.normal(0, 2, size=(T, B, 1)).astype(np.float32), V, axis=2)     # rows constant over the classes
    seq = np.asarray([T - (b % 2) for b in range(B)], np.int32)
    ali, idx, score = run_align(logits, labels, seq)
    for b in range(B):
        Tb = int(seq[b])
        ref_score, st = viterbi_ref(log_softmax64(logits[:Tb, b]), labels[b], blank)
        assert st is not None
        assert np.array_equal(ali[b, :Tb], states_to_symbols(st, labels[b], blank)), b
        assert np.array_equal(idx[b, :Tb], np.where(st % 2 == 1, st // 2, -1)), b
        assert (ali[b, Tb:] == -1).all() and (idx[b, Tb:] == -1).all()


# ----------------------------------------------------------------------------------------------- geometry edges
# S = 2L+1 against 64 lanes x {1, 2, 4, 8, 16, 32} positions per lane: the lane count changes nowhere (one wave), the
# positions per lane change at S = 64, 128, 256, 512, 1024, i.e. between L = 31|32, 63|64, 127|128, 255|256, 511|512;
# backpointer words: 16 frames per word at one position per lane down to 2 words per frame at 32.  Nothing depends on B.
EDGE_L = [0, 1, 31, 32, 63, 64, 127, 128, 255, 256, 511, 512, 1023]
EDGE_V = [2, 5, 44, 129, 300]
GEOMETRY = [(L, 1, EDGE_V[i % 5]) for i, L in enumerate(EDGE_L)] + [(L, 3, EDGE_V[(i + 2) % 5]) for i, L in enumerate(EDGE_L)]


@pytest.mark.parametrize("L,B,V", GEOMETRY)
def test_geometry_edges(L, B, V):
    rng = np.random.default_rng(L * 7 + B * 3 + V)
    labels = [random_labels(rng, L if b == 0 else max(L - b, 0), V) for b in range(B)]      # utterance 0 has the full L
    need = [max(min_frames(l), 1) for l in labels]
    seq = np.asarray([need[b] + (2, 0, 1)[b % 3] for b in range(B)], np.int32)             # just above what L needs
    T = int(seq.max()) + 1
    logits = rng.normal(0, 2, size=(T, B, V)).astype(np.float32)
    ali, idx, score = run_align(logits, labels, seq, max_len=L)
    refs = check_properties(logits, labels, seq, ali, idx, score)
    assert all(np.isfinite(r) for r in refs)


def test_label_length_limit():
    """L = 1023 is accepted (test_geometry_edges runs it); one past is LC_EINVAL naming the limit, with nothing launched."""
    from lstm_ctc_amd import _lib
    lib = _lib.load()
    T, B, V = 4, 1, 3
    logits = torch.zeros(T, B, V, device="cuda")
    flat, offs, seq = _dev([0], np.int32), _dev([0, 1], np.int32), _dev([T], np.int32)
    ali = torch.full((B, T), 77, dtype=torch.int32, device="cuda")
    score = torch.full((B,), 77.0, device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    assert lib.lc_ctc_align_workspace_bytes(T, B, V, 1023) > 0
    rc = raw_align(logits, flat, offs, seq, 1024, ali, None, score, ws, ws.numel())
    assert rc == LC_EINVAL
    assert b"1023" in lib.lc_last_error()
    torch.cuda.synchronize()
    assert (ali == 77).all() and (score == 77.0).all()
    assert raw_align(logits, flat, offs, seq, -1, ali, None, score, ws, ws.numel()) == LC_EINVAL
    assert raw_align(logits[:, :, :1].contiguous(), flat, offs, seq, 1, ali, None, score, ws, ws.numel()) == LC_EINVAL


# ----------------------------------------------------------------------------------------------- length edges in one batch
def test_length_edges_within_one_batch():
    V, blank, T = 7, 6, 14
    A = [0, 1, 2, 3, 4, 5]                       # no repeats: L = 6
    R = [3, 3, 1, 1, 1, 0]                       # r = 3 adjacent repeats: needs L + r = 9 frames
    labels = [A, [2], A, A, A, R, R, A, R]
    seq = np.asarray([T, 1, 0, len(A), len(A) - 1, len(R) + 3, len(R) + 2, 1, T], np.int32)
    rng = np.random.default_rng(8)
    logits = rng.normal(0, 2, size=(T, len(labels), V)).astype(np.float32)
    ali, idx, score = run_align(logits, labels, seq)
    refs = check_properties(logits, labels, seq, ali, idx, score)
    assert [bool(np.isfinite(r)) for r in refs] == [True, True, True, True, False, True, False, False, True]
    assert score[2] == 0.0 and (ali[2] == -1).all()
    assert ali[1, 0] == 2 and idx[1, 0] == 0                                      # one frame, one label
    assert ali[3, :6].tolist() == A and idx[3, :6].tolist() == list(range(6))     # only the blank-free path exists
    assert ali[5, :9].tolist() == [3, blank, 3, 1, blank, 1, blank, 1, 0]         # just feasible: one blank per repeat
    assert idx[5, :9].tolist() == [0, -1, 1, 2, -1, 3, -1, 4, 5]
    for b in (4, 6, 7):
        assert score[b] == -np.inf and (ali[b] == -1).all() and (idx[b] == -1).all()


# ----------------------------------------------------------------------------------------------- other checks
def _medium_case(seed=21, T=90, B=4, V=44, L=30):
    rng = np.random.default_rng(seed)
    labels = [random_labels(rng, L - 3 * b, V) for b in range(B)]
    seq = np.asarray([T - 5 * b for b in range(B)], np.int32)
    logits = rng.normal(0, 2, size=(T, B, V)).astype(np.float32)
    return logits, labels, seq


def test_two_calls_are_bit_identical_and_label_index_is_optional():
    logits, labels, seq = _medium_case()
    a1, i1, s1 = run_align(logits, labels, seq)
    a2, i2, s2 = run_align(logits, labels, seq)
    assert np.array_equal(a1, a2) and np.array_equal(i1, i2) and s1.tobytes() == s2.tobytes()
    a3, i3, s3 = run_align(logits, labels, seq, want_label_index=False)           # label_index = NULL
    assert i3 is None and np.array_equal(a1, a3) and s1.tobytes() == s3.tobytes()
    check_properties(logits, labels, seq, a1, i1, s1)


def test_outputs_fully_overwritten_and_workspace_checked():
    from lstm_ctc_amd import _lib
    lib = _lib.load()
    logits, labels, seq = _medium_case(seed=22)
    labels[2] = list(range(40)) * 3                      # 120 labels in 80 frames: no path for this one
    seq[3] = 0
    T, B, V = logits.shape
    flat, offs = _flat(labels)
    L = max(len(l) for l in labels)
    ld, fd, od, sd = _dev(logits, np.float32), _dev(flat, np.int32), _dev(offs, np.int32), _dev(seq, np.int32)
    nbytes = lib.lc_ctc_align_workspace_bytes(T, B, V, L)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    outs = []
    for sentinel in (0x5a5a5a5a, -12345):
        ali = torch.full((B, T), sentinel, dtype=torch.int32, device="cuda")
        idx = torch.full((B, T), sentinel, dtype=torch.int32, device="cuda")
        score = torch.full((B,), float("nan"), device="cuda")
        assert raw_align(ld, fd, od, sd, L, ali, idx, score, ws, nbytes) == 0
        outs.append((ali.cpu().numpy(), idx.cpu().numpy(), score.cpu().numpy()))
        assert not (outs[-1][0] == sentinel).any() and not (outs[-1][1] == sentinel).any()
        assert not np.isnan(outs[-1][2]).any()
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    assert outs[0][2].tobytes() == outs[1][2].tobytes()
    check_properties(logits, labels, seq, *outs[0])
    ali = torch.full((B, T), 77, dtype=torch.int32, device="cuda")
    score = torch.full((B,), 77.0, device="cuda")
    assert raw_align(ld, fd, od, sd, L, ali, None, score, ws, nbytes - 1) == LC_EWORKSPACE
    assert b"workspace" in lib.lc_last_error()
    torch.cuda.synchronize()
    assert (ali == 77).all() and (score == 77.0).all()


def test_runs_on_the_callers_stream():
    logits, labels, seq = _medium_case(seed=23)
    want = run_align(logits, labels, seq)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = run_align(logits, labels, seq)
    side.synchronize()
    assert np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1]) and want[2].tobytes() == got[2].tobytes()


# ----------------------------------------------------------------------------------------------- graph and CLI
TINY = dict(nnet_type="blstm", input_dim=8, left_context=0, right_context=0, num_layers=2, num_neurons=16,
            num_projects=16, num_targets=6, use_peepholes=True, dropout_rate=1.0)


def test_graph_align_equals_ops_on_a_separate_forward():
    from lstm_ctc_amd import ops
    from lstm_ctc_amd.nnet.graph import create_graph_for_alignment, flatten_labels
    rng = np.random.default_rng(31)
    B, T, D, V = 3, 20, 8, 6
    seq = np.asarray([20, 13, 17], np.int32)
    x = rng.normal(size=(B, T, D)).astype(np.float32)
    y = np.full((B, 5), -1, np.int64)
    for b, n in enumerate((5, 2, 4)):
        x[b, seq[b]:] = 0
        y[b, :n] = rng.integers(0, V - 1, size=n)
    batch = {"nnet_input": x, "sequence_length": seq, "nnet_target": y}
    graph = create_graph_for_alignment(None, TINY)
    before = graph.model.ps.flat.clone()
    counters = (graph.global_step, graph.drop_seed, graph.opt_step)
    got = graph.align(batch)
    assert (graph.global_step, graph.drop_seed, graph.opt_step) == counters
    assert torch.equal(before, graph.model.ps.flat)
    assert set(got) == {"ali", "label_index", "score", "sequence_length"}
    assert all(isinstance(got[k], np.ndarray) for k in got)
    logits = graph.step(batch, fetch_eval=False, fetch_logits=True, train=False)["logits"]          # [B,T,V]
    assert torch.equal(before, graph.model.ps.flat)
    flat, offs, maxlen = flatten_labels(y)
    tbv = torch.from_numpy(np.ascontiguousarray(logits.transpose(1, 0, 2))).cuda()
    ali, idx, score = ops.ctc_align(tbv, _dev(flat, np.int32), _dev(offs, np.int32), _dev(seq, np.int32), maxlen)
    assert np.array_equal(got["ali"], ali.cpu().numpy())
    assert np.array_equal(got["label_index"], idx.cpu().numpy())
    assert got["score"].tobytes() == score.cpu().numpy().tobytes()
    assert np.array_equal(got["sequence_length"], seq)
    for b in range(B):
        assert collapse(got["ali"][b, :seq[b]], V - 1) == [int(v) for v in y[b] if v >= 0]
    bad = dict(batch, nnet_target=np.where(y == y[0, 0], V - 1, y))                                # the blank is not a label
    with pytest.raises(ValueError):
        graph.align(bad)


def test_cli_nnet_align(tmp_path):
    from lstm_ctc_amd.kaldi_io import read_int32_vector_ark
    from lstm_ctc_amd.nnet import write_tfrecord
    from lstm_ctc_amd.nnet.graph import create_graph_for_validation_ctc
    rng = np.random.default_rng(41)
    D, V = 8, 6
    utts = [("good%d" % i, int(rng.integers(12, 25)), random_labels(rng, int(rng.integers(1, 5)), V)) for i in range(5)]
    utts.insert(2, ("nolabels", 9, []))
    utts.insert(4, ("toolong", 3, [0, 1, 2, 3, 4]))
    scp = tmp_path / "tfrecords.scp"
    with open(scp, "w") as f:
        for key, T, lab in utts:
            path = str(tmp_path / (key + ".tfrecords"))
            write_tfrecord(path, rng.normal(size=(T, D)).astype(np.float32), lab)
            f.write("%s %d %d 1 %s\n" % (key, T, D, path))
    config = tmp_path / "nnet.config"
    config.write_text("".join("%s = %s\n" % (k, str(v).lower() if isinstance(v, bool) else v) for k, v in TINY.items()))
    model = str(tmp_path / "nnet.0")
    create_graph_for_validation_ctc(None, TINY, seed=5).save(model)

    def run(tag, *extra):
        ark = str(tmp_path / (tag + ".ark"))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "nnet-align.py"), str(scp), str(config), model,
                            "ark:" + ark] + list(extra), capture_output=True, timeout=300)
        return r.returncode, r.stderr.decode(), ark

    seg, sco = str(tmp_path / "segments.txt"), str(tmp_path / "scores.txt")
    rc, err, ark = run("a", "--segments", seg, "--scores", sco, "--batch-utts", "4", "--report-interval", "2")
    assert rc == 0, err
    good = [(k, T, lab) for k, T, lab in utts if k.startswith("good")]
    back = read_int32_vector_ark(ark)
    assert list(back) == [k for k, _, _ in good]                                 # scp order, the two bad ones skipped
    for key, T, lab in good:
        assert len(back[key]) == T and collapse(back[key], V - 1) == lab, key
    warnings = [l for l in err.split("\n") if "WARNING" in l]
    assert len(warnings) == 2 and "nolabels" in warnings[0] and "toolong" in warnings[1], err
    assert "INFO:tensorflow:processed = 2" in err and "INFO:tensorflow:done" in err and "2 skipped" in err
    segs = [l.split() for l in open(seg).read().splitlines()]
    for key, T, lab in good:
        mine = [(int(l[1]), int(l[2]), int(l[3])) for l in segs if l[0] == key]
        assert [m[0] for m in mine] == lab, key
        for label, start, n in mine:
            assert n >= 1 and (back[key][start:start + n] == label).all()
    scores = dict(l.split() for l in open(sco).read().splitlines())
    assert list(scores) == [k for k, _, _ in good] and all(float(v) < 0 for v in scores.values())
    rc, err, ark1 = run("b", "--batch-utts", "1")
    assert rc == 0, err
    assert open(ark, "rb").read() == open(ark1, "rb").read()


def test_zz_report_largest_measured_error():
    """Not a check of its own: prints the largest measured error / derived bound the property checks of this session saw."""
    print("align: largest measured |score - path| / tol_b = %.3e, |path - optimum| / tol_c = %.3e"
          % (MEASURED["b"], MEASURED["c"]))
    assert MEASURED["b"] <= 1.0 and MEASURED["c"] <= 1.0
