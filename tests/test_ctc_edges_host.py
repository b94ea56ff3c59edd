"""Host side of the lc_ctc_loss / lc_ctc_greedy edge tests: the case table, the batch generator and what keeps a case from
passing vacuously.  tests/test_gpu_ctc_edges.py imports all three from here.  No GPU needed.

Which kernels lc_ctc_loss runs, restated from csrc/ctc.hip (``mm_supported``, ``mm_geometry``, the LC_MMK / LC_SCAN chains).
With S = 2 * max_label_len + 1 lattice positions:

    nw  = 1 if S <= 64 else 2 if S <= 128 else 4            scan waves per direction            (ctc_nw)
    ppl = 1 if S <= 256 else 2 if S <= 512 else 4 if S <= 1024 else 8     positions per lane    (ctc_ppl)
    two launches of ctc_mm_kernel<ppl, nw, kg>  when  V <= 128 and T * B * V * 4 < 0xfffffff0 and S <= 1024
                                                      and (S <= 256 or B > 128);
        B > 128 and S <= 256 -> ppl, nw = 4, 1;    kg = 3 if V <= 48 else 5 if V <= 80 else 8;
        lse2 = a gradient is asked for and (option "ctc_lse2" if set, else B >= 512)
    otherwise three kernels: ctc_row_stats_kernel<g> (g = 16 if V <= 32 else 64), ctc_scan_kernel<ppl, nw>, ctc_grad_kernel.

``expected_path`` is that text as code; ``test_table_agrees_with_the_restated_dispatch`` holds the table's <ppl, nw> column to
it here, and the GPU run holds it to the library through ``ops.last_ctc_path()``.

Batches (``Batch``; one generator, seeded per case; ``need(labels)`` = L + adjacent repeats, the frames a label
sequence takes).  In priority order, cut or filled to the case's B, then put in a seeded random order (unsorted lengths):

* four utterances of exactly Lmax labels, T_b = need + 0, 1, 8, 17.  The first carries a repeated pair across every cut
  between scan waves - label indices c/2 - 1, c/2 for the lattice positions c = 64 ppl, 2 * 64 ppl, 3 * 64 ppl - so no skip
  transition crosses the hand-off; the second has distinct labels there (where the alphabet has two: V >= 3), so one does;
* planted: seq_len = 0; L = T_b + 1 (skipped; needs Lmax >= 1, since max_label_len is Lmax); T_b = L with a repeated pair
  (infeasible: +inf, gradient = softmax; needs Lmax >= 2);
* short tier (Lmax <= 127): one utterance per T_b in EDGE_T - both halves T_b / 2 and T_b - T_b / 2 of the meet-in-the-middle
  split land on 7|8|9 (the ring of 8, the re-centring every 8), 15|16|17 (the pipeline iteration) and 31|32|33 - the label
  count cycling over 0, 1, T_b // 3 and "as many as fit", capped at Lmax;
  long tier (Lmax >= 128): six short ones, T_b in 1, 2, 9, 16, 17, 33 with L in 0, 1;
* many-utterance cases: short-tier utterances of at most 8 labels from further seeds.

T is the largest T_b + 3 unless the case fixes it (then the list of T_b is cut to what fits).  Labels repeat their predecessor
with probability 0.3.  Logits are 1.5 * N(0, 1) with the blank 2 higher - blank-heavy like a CTC model's, and what gives a
one-symbol alphabet (V = 2, where almost every frame sequence spells the labels) a gradient worth comparing.  Then frame 0 of
every utterance is clipped to [-1, 1]: the gradient of a one-frame utterance is softmax - onehot, and 1 - softmax[target] >=
1 - 1 / (1 + e^-2) = 0.12 keeps "max |grad_ref| > 0.1" below from hanging on the seed."""
from collections import namedtuple

import numpy as np
import pytest

EDGE_T = [1, 2, 3, 7, 8, 9] + list(range(14, 20)) + list(range(30, 36)) + list(range(62, 68)) + [72]
LONG_SHORT_T = [1, 2, 9, 16, 17, 33]
SCALE, BLANK_BIAS = 1.5, 2.0

Case = namedtuple("Case", "Lmax V B T path ppl nw")


def _rows(path, ppl, nw, shapes):
    return [Case(*(tuple(s) + (None,) * (4 - len(s)) + (path, ppl, nw))) for s in shapes]


# (Lmax, V[, B[, T]]) -> expected <ppl, nw>; B, T None: whatever the generator's tiers give (B <= 40)
TWO_LAUNCH_FEW = (_rows("two_launch", 1, 1, [(0, 2), (0, 128), (1, 2), (1, 44), (31, 48), (31, 49)]) +
                  _rows("two_launch", 1, 2, [(32, 17), (32, 80), (63, 81), (63, 128)]) +
                  _rows("two_launch", 1, 4, [(64, 44), (64, 128), (127, 2), (127, 48), (127, 80), (127, 128)]))
BLOCK_MAPPING = _rows("two_launch", 1, 1, [(5, 9, B, 24) for B in (1, 7, 8, 9, 16, 17)])
TWO_LAUNCH_MANY = (_rows("two_launch", 4, 1, [(127, 44, 129), (5, 9, 512, 24)]) +
                   _rows("two_launch", 2, 4, [(128, 20, 129), (255, 81, 129)]) +
                   _rows("two_launch", 4, 4, [(256, 12, 129), (511, 48, 129)]))
THREE_KERNEL_WIDE = (_rows("three_kernel", 1, 1, [(31, 129)]) + _rows("three_kernel", 1, 2, [(32, 200)]) +
                     _rows("three_kernel", 1, 4, [(64, 129), (127, 300)]))
THREE_KERNEL_LONG = (_rows("three_kernel", 2, 4, [(128, 32), (255, 129)]) +
                     _rows("three_kernel", 4, 4, [(256, 33), (511, 20)]) +
                     _rows("three_kernel", 8, 4, [(512, 20), (1023, 20), (512, 12, 129)]))
WIDE_ALPHABET = _rows("three_kernel", 1, 1, [(2, 4100, 3, 6), (2, 10240, 3, 6)])      # 10240: the header's limit with a gradient
ALL_CASES = TWO_LAUNCH_FEW + BLOCK_MAPPING + TWO_LAUNCH_MANY + THREE_KERNEL_WIDE + THREE_KERNEL_LONG + WIDE_ALPHABET


def case_id(c):
    return "L%d-V%d" % (c.Lmax, c.V) + ("-B%d" % c.B if c.B else "") + ("-T%d" % c.T if c.T else "")


def expected_path(Lmax, V, B, T, grad=True, lse2_option=None):
    """The module docstring's restatement of the dispatch: the dict ``ops.last_ctc_path()`` must return."""
    S = 2 * Lmax + 1
    nw = 1 if S <= 64 else 2 if S <= 128 else 4
    ppl = 1 if S <= 256 else 2 if S <= 512 else 4 if S <= 1024 else 8
    if V <= 128 and T * B * V * 4 < 0xfffffff0 and S <= 1024 and (S <= 256 or B > 128):
        if B > 128 and S <= 256:
            ppl, nw = 4, 1
        lse2 = bool(grad and (lse2_option if lse2_option is not None else B >= 512))
        return dict(path="two_launch", ppl=ppl, nw=nw, kg=3 if V <= 48 else 5 if V <= 80 else 8, lse2=lse2, g=0)
    return dict(path="three_kernel", ppl=ppl, nw=nw, kg=0, lse2=False, g=16 if V <= 32 else 64)


# ----------------------------------------------------------------------------------------------- generator
def need(labels):
    return len(labels) + sum(1 for i in range(1, len(labels)) if labels[i] == labels[i - 1])


def draw_labels(rng, V, L):
    labels = rng.randint(0, V - 1, L).astype(np.int64)
    for i in range(1, L):
        if rng.rand() < 0.3:
            labels[i] = labels[i - 1]
    return labels


def _as_many_as_fit(rng, V, Tb, cap):
    labels = draw_labels(rng, V, min(cap, Tb))
    while need(labels) > Tb:
        labels = labels[:-1]
    return labels


def _edge_utts(rng, V, Ts, cap):
    utts = []
    for i, Tb in enumerate(Ts):
        L = (0, 1, Tb // 3, None)[i % 4]
        labels = _as_many_as_fit(rng, V, Tb, cap) if L is None else _as_many_as_fit(rng, V, Tb, min(L, cap))
        utts.append((Tb, labels, "live"))
    return utts


class Batch:
    """x [T,B,V] float32, seq [B], flat labels + offs [B+1], utts[b] = (T_b, labels, kind): kind in live, empty (seq_len 0),
    skipped (L > T_b), infeasible."""

    def __init__(self, case, seed=None):
        Lmax, V = case.Lmax, case.V
        self.case, self.V, self.Lmax = case, V, Lmax
        seed = ((Lmax * 131 + V) * 1009 + (case.B or 0)) if seed is None else seed
        rng = np.random.RandomState(seed)
        cuts = [c // 2 for c in (64 * case.ppl * k for k in (1, 2, 3)) if c // 2 < Lmax]
        utts = []
        for i, extra in enumerate((0, 1, 8, 17)):
            labels = draw_labels(rng, V, Lmax)
            for j in cuts:
                if i == 0:
                    labels[j] = labels[j - 1]
                elif i == 1 and V >= 3 and labels[j] == labels[j - 1]:
                    labels[j] = (labels[j - 1] + 1) % (V - 1)
            Tb = max(need(labels), 1) + extra
            utts.append((min(Tb, case.T) if case.T else Tb, labels, "live"))
        assert all(need(u[1]) <= u[0] for u in utts)
        utts.append((0, draw_labels(rng, V, min(Lmax, 2)), "empty"))
        if Lmax >= 1:
            L = min(Lmax, 4)
            utts.append((L - 1, draw_labels(rng, V, L), "skipped"))
        if Lmax >= 2:
            labels = draw_labels(rng, V, min(Lmax, 3))
            labels[1] = labels[0]
            utts.append((len(labels), labels, "infeasible"))
        Tmax = case.T if case.T else 1 << 30
        if Lmax <= 127:
            utts += _edge_utts(rng, V, [t for t in EDGE_T if t <= Tmax], Lmax)
        else:
            utts += [(Tb, draw_labels(rng, V, i % 2), "live") for i, Tb in enumerate(LONG_SHORT_T)]
        r = 0
        while case.B and len(utts) < case.B:                       # many utterances: short ones from further seeds
            r += 1
            utts += _edge_utts(np.random.RandomState((seed * 1000 + r) % 2 ** 32), V, [t for t in EDGE_T if t <= Tmax], min(Lmax, 8))
        utts = utts[:case.B] if case.B else utts
        self.utts = [utts[i] for i in rng.permutation(len(utts))]
        self.B = len(self.utts)
        self.T = case.T if case.T else max(u[0] for u in self.utts) + 3
        self.seq = np.array([u[0] for u in self.utts], np.int32)
        self.flat = np.concatenate([u[1] for u in self.utts] + [np.zeros(0, np.int64)]).astype(np.int32)
        self.offs = np.concatenate(([0], np.cumsum([len(u[1]) for u in self.utts]))).astype(np.int32)
        assert max(len(u[1]) for u in self.utts) == Lmax and self.seq.max() <= self.T
        x = rng.randn(self.T, self.B, V) * SCALE
        x[:, :, V - 1] += BLANK_BIAS
        x[0] = np.clip(x[0], -1.0, 1.0)
        self.x = x.astype(np.float32)

    def kinds(self, kind):
        return [b for b, u in enumerate(self.utts) if u[2] == kind]

    def expected(self, grad=True, lse2_option=None):
        return expected_path(self.Lmax, self.V, self.B, self.T, grad, lse2_option)


_REFS = {}


def reference(oracle, batch):
    """float64 (loss, grad, bad) and the float32 oracle's (loss, grad), computed once per case and shared, never modified."""
    key = batch.case
    if key not in _REFS:
        l64, g64, bad = oracle.ctc_loss(batch.x.astype(np.float64), batch.flat, batch.offs, batch.seq)
        l32, g32, _ = oracle.ctc_loss(batch.x, batch.flat, batch.offs, batch.seq)
        for a in (l64, g64, l32, g32):
            a.setflags(write=False)
        _REFS[key] = (l64, g64, bad, l32, g32)
    return _REFS[key]


# ----------------------------------------------------------------------------------------------- tests
def test_table_agrees_with_the_restated_dispatch():
    assert len(set(ALL_CASES)) == len(ALL_CASES) == 16 + 6 + 6 + 4 + 7 + 2
    for c in ALL_CASES:
        b = Batch(c)
        e = b.expected()
        assert (e["path"], e["ppl"], e["nw"]) == (c.path, c.ppl, c.nw), (c, e)
        assert b.B == (c.B or b.B) and b.T == (c.T or b.T) and b.B <= (c.B or 40)
    # every instantiation family of the dispatch is reached: (path, ppl, nw, kg or g)
    seen = {(e["path"], e["ppl"], e["nw"], e["kg"] or e["g"]) for e in (Batch(c).expected() for c in ALL_CASES)}
    for geo in ((1, 1), (1, 2), (1, 4)):                                   # few utterances: every geometry x every KG
        for kg in (3, 5, 8):
            assert ("two_launch",) + geo + (kg,) in seen, (geo, kg)
    for geo in ((4, 1), (2, 4), (4, 4)):                                   # many utterances: every geometry
        assert any(("two_launch",) + geo + (kg,) in seen for kg in (3, 5, 8)), geo
    for geo in ((1, 1), (1, 2), (1, 4), (2, 4), (4, 4), (8, 4)):           # all six legacy scans; both row-statistics widths
        assert any(("three_kernel",) + geo + (g,) in seen for g in (16, 64)), geo
    assert {s[3] for s in seen if s[0] == "three_kernel"} == {16, 64}
    assert Batch(TWO_LAUNCH_MANY[1]).expected()["lse2"] and not Batch(TWO_LAUNCH_MANY[0]).expected()["lse2"]
    assert not Batch(TWO_LAUNCH_MANY[1]).expected(grad=False)["lse2"] and Batch(TWO_LAUNCH_FEW[0]).expected(lse2_option=1)["lse2"]


@pytest.mark.parametrize("case", ALL_CASES, ids=case_id)
def test_no_case_passes_vacuously(oracle, case):
    b = Batch(case)
    # the edges the case is there for
    live = [u for u in b.utts if u[2] == "live"]
    assert sum(1 for u in live if len(u[1]) == case.Lmax) >= min(4, b.B)
    if b.B >= 7:
        assert len(b.kinds("empty")) == 1 and len(b.kinds("skipped")) == (case.Lmax >= 1)
        assert len(b.kinds("infeasible")) == (case.Lmax >= 2)
    if b.B >= 20:
        assert {u[0] for u in live} >= set(LONG_SHORT_T if case.Lmax >= 128 else [t for t in EDGE_T if t <= b.T])
    assert list(b.seq) != sorted(b.seq) or b.B == 1
    loss, grad, bad, _, _ = reference(oracle, b)
    assert bad == len(b.kinds("infeasible"))
    for k in b.kinds("infeasible"):
        assert loss[k] == np.inf and len(b.utts[k][1]) <= b.utts[k][0]
    for k in b.kinds("empty") + b.kinds("skipped"):
        assert loss[k] == 0.0 and not grad[:, k].any()
        assert b.seq[k] <= 0 or len(b.utts[k][1]) > b.seq[k]
    for k in b.kinds("live"):
        assert np.isfinite(loss[k]) and loss[k] > 0.0, (k, b.utts[k])
        assert np.abs(grad[:, k]).max() > 0.1, (k, b.utts[k][0], len(b.utts[k][1]))
    assert not np.isnan(grad).any()


def test_cut_plants_cross_every_hand_off_both_ways():
    for c in ALL_CASES:
        b = Batch(c)
        cuts = [k * 64 * c.ppl // 2 for k in (1, 2, 3) if k * 64 * c.ppl // 2 < c.Lmax]
        if (c.nw > 1) and c.Lmax >= 64:
            assert cuts, c
        full = [u[1] for u in sorted((u for u in b.utts if u[2] == "live" and len(u[1]) == c.Lmax), key=lambda u: u[0])]
        rep = [all(l[j] == l[j - 1] for j in cuts) for l in full]
        dis = [all(l[j] != l[j - 1] for j in cuts) for l in full]
        if cuts and b.B >= 4:
            assert any(rep) and (any(dis) or c.V < 3), c


def test_oracle_closed_forms_at_the_new_edges(oracle):
    rng = np.random.RandomState(11)
    for V in (2, 7, 200):
        x = rng.randn(9, 3, V) * 1.5
        lsm = x - np.log(np.exp(x).sum(axis=2, keepdims=True))
        label = int(rng.randint(0, V - 1))
        flat, offs = np.array([label], np.int32), np.array([0, 0, 1, 1], np.int32)          # L = 0, 1, 0
        loss, grad, bad = oracle.ctc_loss(x, flat, offs, np.array([1, 1, 9], np.int32))
        assert bad == 0
        assert abs(loss[0] + lsm[0, 0, V - 1]) < 1e-12                      # T_b = 1, L = 0: -log softmax[blank]
        assert abs(loss[1] + lsm[0, 1, label]) < 1e-12                      # T_b = 1, L = 1: -log softmax[label]
        assert abs(loss[2] + lsm[:, 2, V - 1].sum()) < 1e-11                # L = 0: -sum_t log softmax[blank]
        onehot = np.zeros(V)
        onehot[label] = 1.0
        assert np.abs(grad[0, 1] - (np.exp(lsm[0, 1]) - onehot)).max() < 1e-12 and not grad[1:, :2].any()
