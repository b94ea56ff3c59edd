"""lc_xent_loss (frame-level softmax cross-entropy) on the GPU: the op, the graph's xent objective and the command lines.

Reference: float64 numpy log-softmax (torch float64 on the device for the one case too large for the host); for the model,
the oracle's forward / backward / l2_and_clip / apply_optimizer composed around that reference.

Tolerances - derived from the kernel's arithmetic, not from what it was seen to give (u = 2^-24, fp32 unit round-off):

* Per scored frame the kernel takes ONE fp32 log-sum-exp: m = max_k x_k (exact); p_k = exp2(fl(fl(x_k - m) * log2e)) on the
  hardware exp (1 ulp); the argument carries <= 3u |a_k| (difference, constant, product), which the exponential turns into a
  relative 3u ln2 |a_k|, and p_k |a_k| <= 1 / (e ln2), so a term is off by <= 1.11u + 2u p_k: V terms, <= (1.11 V + 2) u S
  with S = sum_k p_k >= 1.  The terms are added in fp32 in a fixed order - a lane adds its own elements in sequence, then a
  tree over the lanes of the frame's group: at most NADD(V) = ceil(V / 64) + 16 additions deep in every kernel variant
  (V <= 64: 4 + 4; V <= 1024: 4 / 8 / 16 + 6; wider: <= V / 64 + 6 + 6), <= NADD u S.  ln S = log2(S) * ln2: hardware log2
  (1 ulp), constant, product: <= 4u ln V.  lse = fl(m + ln S): <= u (max|x| + ln V).  Together
      eps_lse(V) = u (1.11 V + 2 + NADD(V) + 5 ln V + max|x|).
* The frame's term is fl(lse - x_target): ONE fp32 subtraction, <= u |term| more.
* The fold adds an utterance's terms as doubles (2^-53 each - nothing at these sizes) and rounds the sum once: u |loss|.
      tol_loss[b] = n_b eps_lse + 2u sum_t |term_t| + u |loss_b|            (n_b = scored frames of utterance b)
* Gradient element: p_k / S with p_k as above (relative 3u ln2 |a_k| + u), S (relative (1.11 V + 2 + NADD) u), the hardware
  reciprocal (1 ulp), the product and the subtraction of the one-hot (u each); p_k / S <= 1 and |a_k| p_k <= 1 / (e ln2):
      tol_grad = u (1.11 V + NADD(V) + 14)                                   absolute, per element.
* Both are asserted TOGETHER with the project's bar (tests/conftest.py): 1e-4 max(|ref|, 1) for a loss, check_grad /
  GRAD_TOL for a gradient tensor.  frames and correct are integers and compared exactly; the inputs are drawn so that no row
  has two equal maxima (asserted on the reference), so an argmax mismatch cannot hide behind a tie.
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import check_grad

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
BAR = 1e-4                         # tests/conftest.py: GRAD_TOL, the project's bar for logits and loss
LC_EINVAL, LC_EWORKSPACE = -1, -3
MEASURED = {"loss": 0.0, "grad": 0.0, "loss_bar": 0.0}     # largest measured error / bound (printed by the last test)


# ----------------------------------------------------------------------------------------------- reference and bounds
def nadd(V):
    return math.ceil(V / 64) + 16


def eps_lse(V, maxabs):
    return U * (1.11 * V + 2 + nadd(V) + 5 * math.log(V) + maxabs)


def tol_grad(V):
    return U * (1.11 * V + nadd(V) + 14)


def xent_ref(logits, targets, seq):
    """float64 reference.  logits [T,B,V], targets [B,T], seq [B] -> dict(loss [B], frames, correct, grad [T,B,V],
    sumabs [B] = sum of |term| over the scored frames, scored [T,B])."""
    x = np.asarray(logits, np.float64)
    T, B, V = x.shape
    tg = np.asarray(targets, np.int64).T                                  # [T,B]
    live = np.arange(T)[:, None] < np.asarray(seq)[None, :]
    scored = live & (tg >= 0) & (tg < V)
    bad = live & ((tg < -1) | (tg >= V))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = x.max(axis=-1, keepdims=True)
        lse = m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True))
        lsm = x - lse
        p = np.exp(lsm)
    safe = np.where(scored, tg, 0)
    term = -np.take_along_axis(lsm, safe[..., None], axis=-1)[..., 0]
    term = np.where(scored, term, 0.0)
    onehot = np.zeros_like(x)
    np.put_along_axis(onehot, safe[..., None], 1.0, axis=-1)
    grad = np.where(scored[..., None], p - onehot, 0.0)
    loss = term.sum(axis=0)
    loss[bad.any(axis=0)] = np.nan
    amax = x.argmax(axis=-1)                                              # numpy: the first among equal maxima
    return dict(loss=loss, frames=scored.sum(axis=0), correct=(scored & (amax == tg)).sum(axis=0), grad=grad,
                sumabs=np.abs(term).sum(axis=0), scored=scored)


def assert_unique_maxima(logits):
    x = np.asarray(logits)
    top2 = np.partition(x, -2, axis=-1)[..., -2:]
    assert (top2[..., 0] < top2[..., 1]).all(), "test input has a row with two equal maxima"


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def run_xent(logits, targets, seq, want_grad=True):
    from lstm_ctc_amd import ops
    loss, frames, correct, grad = ops.xent_loss(_dev(logits, np.float32), _dev(targets, np.int32), _dev(seq, np.int32),
                                                want_grad=want_grad)
    torch.cuda.synchronize()
    return (loss.cpu().numpy(), frames.cpu().numpy(), correct.cpu().numpy(), grad.cpu().numpy() if want_grad else None)


def check_against_ref(logits, targets, seq, got, tag):
    loss, frames, correct, grad = got
    T, B, V = logits.shape
    ref = xent_ref(logits, targets, seq)
    assert np.array_equal(frames, ref["frames"]), (tag, frames, ref["frames"])
    assert np.array_equal(correct, ref["correct"]), (tag, correct, ref["correct"])
    maxabs = float(np.abs(logits[np.isfinite(logits)]).max()) if np.isfinite(logits).any() else 0.0
    for b in range(B):
        r = ref["loss"][b]
        if not np.isfinite(r):
            assert (np.isnan(loss[b]) and np.isnan(r)) or loss[b] == r, (tag, b, loss[b], r)
            continue
        tol = ref["frames"][b] * eps_lse(V, maxabs) + 2 * U * ref["sumabs"][b] + U * abs(r)
        bar = BAR * max(abs(r), 1.0)
        err = abs(float(loss[b]) - r)
        if tol > 0:
            MEASURED["loss"] = max(MEASURED["loss"], err / tol)
        MEASURED["loss_bar"] = max(MEASURED["loss_bar"], err / bar)
        assert err <= tol and err <= bar, (tag, b, err, tol, bar)
    if grad is not None:
        g = ref["grad"]
        fin = np.isfinite(g)
        assert np.array_equal(np.isfinite(grad), fin), tag
        err = float(np.abs(np.where(fin, grad - g, 0.0)).max())
        MEASURED["grad"] = max(MEASURED["grad"], err / tol_grad(V))
        assert err <= tol_grad(V), (tag, err, tol_grad(V))
        check_grad(np.where(fin, grad, 0.0), np.where(fin, g, 0.0), tag, "dlogits")
        assert not grad[~ref["scored"]].any() and not np.signbit(grad[~ref["scored"]]).any(), tag     # exactly +0
    return ref


def make_case(rng, T, B, V, seq, scale=3.0):
    logits = (rng.standard_normal((T, B, V)) * scale).astype(np.float32)
    targets = rng.integers(0, V, size=(B, T)).astype(np.int32)            # live values beyond seq_len too: to be ignored
    seq = np.asarray(seq, np.int32)
    for b in range(B):
        n = int(seq[b])
        if n >= 1:
            targets[b, 0] = V - 1 if b % 2 == 0 else 0                    # the blank and class 0 as targets
        if n >= 3:
            targets[b, 1] = -1                                            # "ignore" inside the live frames
            targets[b, 2] = 0 if b % 2 == 0 else V - 1
    assert_unique_maxima(logits)
    return logits, targets, seq


# ----------------------------------------------------------------------------------------------- 1. the op at the edges
EDGE_V = [2, 3, 16, 17, 44, 63, 64, 65, 128, 129, 255, 256, 257, 1024, 1025, 4099]
EDGE_SHAPES = [(5, 3, [5, 4, 1]), (5, 3, [0, 5, 4]), (1, 1, [1]), (37, 5, [37, 36, 1, 0, 20])]


@pytest.mark.parametrize("V", EDGE_V)
def test_op_matches_reference_at_lane_split_edges(V):
    rng = np.random.default_rng(1000 + V)
    for T, B, seq in EDGE_SHAPES:
        logits, targets, seq = make_case(rng, T, B, V, seq)
        got = run_xent(logits, targets, seq)
        ref = check_against_ref(logits, targets, seq, got, ("edge", V, T, B))
        assert ref["frames"].sum() > 0
        nograd = run_xent(logits, targets, seq, want_grad=False)
        assert nograd[3] is None
        for a, b_ in zip(got[:3], nograd[:3]):                            # the same bits with and without a gradient
            assert np.array_equal(a, b_, equal_nan=True)


# ----------------------------------------------------------------------------------------------- raw calls
def raw_call(logits, targets, seq, T, B, V, loss, frames, correct, grad, ws, ws_bytes):
    from lstm_ctc_amd import _lib, ops
    lib = _lib.load()
    rc = lib.lc_xent_loss(ops._ptr(logits), T, B, V, ops._ptr(targets), ops._ptr(seq), ops._ptr(loss), ops._ptr(frames),
                          ops._ptr(correct), ops._ptr(grad), ops._ptr(ws), ws_bytes, ops._stream())
    torch.cuda.synchronize()
    return rc


def _prefilled(T, B, V):
    return (torch.full((B,), float("nan"), device="cuda"), torch.full((B,), -77, dtype=torch.int32, device="cuda"),
            torch.full((B,), -77, dtype=torch.int32, device="cuda"), torch.full((T, B, V), float("nan"), device="cuda"))


@pytest.mark.parametrize("V", [4, 44, 45, 300, 1030])
def test_every_output_element_is_written(V):
    from lstm_ctc_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(V)
    T, B = 9, 6
    logits, targets, seq = make_case(rng, T, B, V, [9, 0, 5, 9, 3, 7])
    targets[3, :] = -1                                                    # live frames, nothing scored
    targets[4, :3] = -1
    ref = xent_ref(logits, targets, seq)
    assert ref["frames"][1] == ref["frames"][3] == ref["frames"][4] == 0
    ld, td, sd = _dev(logits, np.float32), _dev(targets, np.int32), _dev(seq, np.int32)
    nbytes = lib.lc_xent_workspace_bytes(T, B, V)
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")    # a dirty workspace: all-ones words
    for with_grad in (True, False):
        loss, frames, correct, grad = _prefilled(T, B, V)
        assert raw_call(ld, td, sd, T, B, V, loss, frames, correct, grad if with_grad else None, ws, nbytes) == 0
        l, f, c, g = loss.cpu().numpy(), frames.cpu().numpy(), correct.cpu().numpy(), grad.cpu().numpy()
        assert not np.isnan(l).any() and (f != -77).all() and (c != -77).all()
        for b in (1, 3, 4):                                               # no scored frame: loss 0 and counts 0
            assert l[b] == 0.0 and not np.signbit(l[b]) and f[b] == 0 and c[b] == 0
        if with_grad:
            assert not np.isnan(g).any()
            check_against_ref(logits, targets, seq, (l, f, c, g), ("written", V))
        else:
            assert np.isnan(g).all()                                      # grad = NULL: not touched
            check_against_ref(logits, targets, seq, (l, f, c, None), ("written-nograd", V))


@pytest.mark.parametrize("T,B,V", [(50, 7, 44), (50, 7, 300), (20, 7, 4099)])
def test_two_calls_are_bit_identical(T, B, V):
    rng = np.random.default_rng(5)
    logits, targets, seq = make_case(rng, T, B, V, rng.integers(0, T + 1, size=B))
    a, b_ = run_xent(logits, targets, seq), run_xent(logits, targets, seq)
    for x, y in zip(a, b_):
        assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("V", [44, 300, 1028, 1031])
def test_buffers_off_the_16_byte_boundary_take_the_dword_path(V):
    """Logits that start 4 bytes behind a 16-byte boundary (a view into a larger buffer): the same results, to the bit, as
    from an aligned copy wherever the aligned call takes dwords too, and within the tolerances everywhere."""
    from lstm_ctc_amd import ops
    rng = np.random.default_rng(V)
    T, B = 11, 3
    logits, targets, seq = make_case(rng, T, B, V, [11, 10, 4])
    buf = torch.zeros(T * B * V + 1, device="cuda")
    view = buf[1:].view(T, B, V)
    view.copy_(_dev(logits, np.float32))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    loss, frames, correct, grad = ops.xent_loss(view, _dev(targets, np.int32), _dev(seq, np.int32))
    torch.cuda.synchronize()
    got = (loss.cpu().numpy(), frames.cpu().numpy(), correct.cpu().numpy(), grad.cpu().numpy())
    check_against_ref(logits, targets, seq, got, ("unaligned", V))


@pytest.mark.parametrize("V", [6, 44, 300, 2000])
def test_argmax_tie_goes_to_the_lower_index(V):
    rng = np.random.default_rng(V)
    pairs = [(0, 1), (1, V - 1), (V // 2, V // 2 + 1), (2, min(V - 1, 70))]      # within a lane's span and across lanes
    T, B = len(pairs), 2
    logits = rng.standard_normal((T, B, V)).astype(np.float32)
    targets = np.zeros((B, T), np.int32)
    for t, (lo, hi) in enumerate(pairs):
        logits[t, :, lo] = logits[t, :, hi] = 9.5
        targets[0, t], targets[1, t] = lo, hi
    loss, frames, correct, _ = run_xent(logits, targets, np.array([T, T], np.int32))
    assert frames.tolist() == [T, T]
    assert correct.tolist() == [T, 0]                 # the lower index is the argmax: targets on the higher one are wrong
    ref = xent_ref(logits, targets, [T, T])
    assert np.array_equal(correct, ref["correct"])
    assert np.allclose(loss, ref["loss"], rtol=1e-5)


@pytest.mark.parametrize("V", [5, 44, 300, 1100])
def test_special_values(V):
    rng = np.random.default_rng(V)
    T, B = 6, 4
    logits, targets, seq = make_case(rng, T, B, V, [6, 6, 6, 6])
    logits[2, 0, 1] = -np.inf                         # a -inf class that is not the target
    targets[0, 2] = 3
    logits[3, 1, 2] = -np.inf                         # a -inf target
    targets[1, 3] = 2
    logits[4, 2, :] = -np.inf                         # a row of -inf
    got = run_xent(logits, targets, seq)
    loss, frames, correct, grad = got
    assert np.isfinite(loss[0]) and grad[2, 0, 1] == 0.0 and not np.signbit(grad[2, 0, 1])
    assert loss[1] == np.inf
    assert np.isnan(loss[2])
    assert np.isfinite(loss[3])
    check_against_ref(logits, targets, seq, got, ("special", V))
    # a target outside [-1, V): NaN for that utterance only, its frame is a zero row and counts nowhere
    logits, targets, seq = make_case(rng, T, B, V, [6, 6, 5, 6])
    clean = run_xent(logits, targets, seq)
    for bad_value, b in ((V, 1), (-2, 2)):
        t2 = targets.copy()
        t2[b, 3] = bad_value
        loss, frames, correct, grad = run_xent(logits, t2, seq)
        assert np.isnan(loss[b]) and frames[b] == clean[1][b] - 1
        assert not grad[3, b].any()
        for o in range(B):
            if o != b:                                # the neighbours are intact, to the bit
                assert loss[o] == clean[0][o] and frames[o] == clean[1][o] and correct[o] == clean[2][o]
                assert np.array_equal(grad[:, o], clean[3][:, o])
        check_against_ref(logits, t2, seq, (loss, frames, correct, grad), ("bad target", V, bad_value))
    # a bad target beyond seq_len is not live: ignored
    t2 = targets.copy()
    t2[2, 5] = V + 7
    again = run_xent(logits, t2, seq)
    for x, y in zip(again, clean):
        assert np.array_equal(x, y)


def test_bad_frame_target_through_the_graph_raises():
    from lstm_ctc_amd.nnet.graph import create_graph_for_validation_xent
    cfg = dict(MODEL_CFG)
    graph = create_graph_for_validation_xent(None, cfg, seed=3)
    batch = _model_batch(cfg)
    assert graph.step(batch, fetch_eval=True)["size"] > 0
    for bad in (cfg["num_targets"], -2):
        b2 = dict(batch, frame_target=batch["frame_target"].copy())
        b2["frame_target"][0, 2] = bad
        with pytest.raises(ValueError, match=r"\[-1, %d\)" % cfg["num_targets"]):
            graph.step(b2)
    b2 = dict(batch, frame_target=batch["frame_target"].copy())
    b2["frame_target"][2, 5] = 99                      # beyond that utterance's length (1): not live, no error
    graph.step(b2)
    with pytest.raises(ValueError, match="unsupported objective"):
        from lstm_ctc_amd.nnet.graph import CTCGraph
        CTCGraph(None, cfg, objective="mmi")


@pytest.mark.parametrize("T,B,V", [(700, 48, 4), (130, 64, 68), (130, 64, 1028)])
def test_more_frames_than_one_pass_of_the_grid(T, B, V):
    """The launch is capped at 2048 blocks of four waves: 32768 frames per pass at four frames per wave (V <= 64), 8192 at
    one frame per wave.  These shapes need a second pass of the grid-stride loop, with the batch wrapping inside a wave."""
    assert T * B > (32768 if V <= 64 else 8192)
    rng = np.random.default_rng(V)
    seq = rng.integers(T // 2, T + 1, size=B)
    seq[-1] = T
    logits, targets, seq = make_case(rng, T, B, V, seq)
    check_against_ref(logits, targets, seq, run_xent(logits, targets, seq), ("grid stride", V))


def test_elements_indexed_in_64_bits():
    """T * B * V just above 2^31: 64 sampled frames' gradient rows, every utterance's loss and the counts against torch
    float64 on the device."""
    from lstm_ctc_amd import ops
    T, B, V = 1024, 512, 4099
    assert T * B * V > 2 ** 31
    free, _ = torch.cuda.mem_get_info()
    if free < 24 * 2 ** 30:
        pytest.skip("needs 24 GB of free device memory")
    gen = torch.Generator(device="cuda").manual_seed(7)
    logits = torch.randn((T, B, V), device="cuda", generator=gen) * 3.0
    targets = torch.randint(0, V, (B, T), device="cuda", generator=gen, dtype=torch.int32)
    targets[:, 5] = -1
    seq = torch.randint(T // 2, T + 1, (B,), device="cuda", generator=gen, dtype=torch.int32)
    seq[-1] = T
    seq[0] = T
    loss, frames, correct, grad = ops.xent_loss(logits, targets, seq, want_grad=True)
    torch.cuda.synchronize()
    tg = targets.t().long()                                               # [T,B]
    scored = (torch.arange(T, device="cuda")[:, None] < seq[None, :]) & (tg >= 0)
    ref_loss = torch.zeros(B, dtype=torch.float64, device="cuda")
    ref_abs = torch.zeros(B, dtype=torch.float64, device="cuda")
    ref_correct = torch.zeros(B, dtype=torch.int64, device="cuda")
    ar = torch.arange(V, device="cuda")
    for t0 in range(0, T, 32):
        x = logits[t0:t0 + 32]
        sc, tgc = scored[t0:t0 + 32], tg[t0:t0 + 32].clamp(min=0)
        lsm = torch.log_softmax(x.double(), dim=-1)
        term = -lsm.gather(-1, tgc[..., None])[..., 0] * sc
        ref_loss += term.sum(0)
        ref_abs += term.abs().sum(0)
        first = torch.where(x == x.max(-1, keepdim=True).values, ar, V).min(-1).values      # lowest index at the maximum
        ref_correct += (sc & (first == tgc)).sum(0)
        del lsm, term, first
    assert torch.equal(frames.long(), scored.sum(0))
    assert torch.equal(correct.long(), ref_correct)
    maxabs = float(logits.abs().max())
    n = scored.sum(0).double()
    tol = n * eps_lse(V, maxabs) + 2 * U * ref_abs + U * ref_loss.abs()
    err = (loss.double() - ref_loss).abs()
    MEASURED["loss"] = max(MEASURED["loss"], float((err / tol).max()))
    MEASURED["loss_bar"] = max(MEASURED["loss_bar"], float((err / (BAR * ref_loss.abs().clamp(min=1.0))).max()))
    assert bool((err <= tol).all()) and bool((err <= BAR * ref_loss.abs().clamp(min=1.0)).all())
    # 64 frames, the last ones (the highest addresses) and one beyond its utterance's length included
    rng = np.random.default_rng(3)
    frames_s = [(T - 1, B - 1), (T - 1, 0), (T - 2, B - 1), (T - 1, B - 2), (0, 0), (5, 9)]
    short = int(torch.argmin(seq))
    frames_s.append((T - 1, short))
    while len(frames_s) < 64:
        frames_s.append((int(rng.integers(0, T)), int(rng.integers(0, B))))
    assert (T - 1) * B * V + (B - 1) * V > 2 ** 31
    worst = 0.0
    for t, b in frames_s:
        g = grad[t, b].double()
        if bool(scored[t, b]):
            r = torch.softmax(logits[t, b].double(), dim=-1)
            r[int(tg[t, b])] -= 1.0
            e = float((g - r).abs().max())
            worst = max(worst, e)
            assert e <= tol_grad(V) and e <= BAR * max(float(r.abs().max()), 1e-3), (t, b, e)
        else:
            assert not bool(g.any()), (t, b)
    MEASURED["grad"] = max(MEASURED["grad"], worst / tol_grad(V))


def test_argument_checks_leave_the_outputs_alone():
    from lstm_ctc_amd import _lib
    lib = _lib.load()
    T, B, V = 4, 3, 10
    rng = np.random.default_rng(0)
    logits, targets, seq = make_case(rng, T, B, V, [4, 3, 2])
    ld, td, sd = _dev(logits, np.float32), _dev(targets, np.int32), _dev(seq, np.int32)
    nbytes = lib.lc_xent_workspace_bytes(T, B, V)
    assert nbytes >= 8 * T * B
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    outs = _prefilled(T, B, V)
    loss, frames, correct, grad = outs

    def untouched():
        return (bool(torch.isnan(loss).all()) and bool((frames == -77).all()) and bool((correct == -77).all())
                and bool(torch.isnan(grad).all()))

    for kw in (dict(T=0), dict(T=-1), dict(B=0), dict(V=1), dict(V=0), dict(logits=None), dict(targets=None),
               dict(seq=None), dict(loss=None), dict(frames=None), dict(correct=None), dict(ws=None)):
        a = dict(logits=ld, targets=td, seq=sd, T=T, B=B, V=V, loss=loss, frames=frames, correct=correct, grad=grad, ws=ws,
                 ws_bytes=nbytes)
        a.update(kw)
        assert raw_call(**a) == LC_EINVAL, kw
        assert untouched(), kw
    for short in (0, nbytes - 1):
        assert raw_call(ld, td, sd, T, B, V, loss, frames, correct, grad, ws, short) == LC_EWORKSPACE
        assert untouched()
    assert lib.lc_last_error().decode().startswith("lc_xent_loss: workspace too small")
    assert raw_call(ld, td, sd, T, B, V, loss, frames, correct, grad, ws, nbytes) == 0
    assert not untouched()


# ----------------------------------------------------------------------------------------------- the graph
MODEL_CFG = dict(nnet_type="blstm", input_dim=12, left_context=0, right_context=0, num_layers=2, num_neurons=32,
                 num_projects=16, num_targets=8, use_peepholes=True, dropout_rate=1.0)      # test_train_steps_vs_oracle's
MODELS = {"blstm": {}, "lstm": dict(nnet_type="lstm", num_projects=16)}


def _model_batch(cfg):
    """B = 5, T = 14: lengths 14, 9, 1, 0, 12; utterance 1 has no target at all; a blank and an "ignore" among the targets."""
    rng = np.random.default_rng(3)
    B, T, D, V = 5, 14, cfg["input_dim"], cfg["num_targets"]
    seq = np.array([14, 9, 1, 0, 12], np.int32)
    x = rng.normal(size=(B, T, D)).astype(np.float32)
    ft = np.full((B, T), -1, np.int32)
    for b in range(B):
        x[b, seq[b]:] = 0
        ft[b, :seq[b]] = rng.integers(0, V, size=seq[b])
    ft[1, :] = -1
    ft[0, 3] = V - 1
    ft[0, 5] = -1
    ft[2, 0] = V - 1
    return {"nnet_input": x, "sequence_length": seq, "nnet_target": np.full((B, 0), -1, np.int64), "frame_target": ft}


def _oracle_step(oracle, params, cfg, batch, state, optimizer, lr):
    """One training step of the xent objective from the oracle's parts, in float64 around the float32 parameters."""
    logits, saved = oracle.forward(params, cfg, batch["nnet_input"], batch["sequence_length"])      # [B,T,V]
    tbv = np.ascontiguousarray(np.asarray(logits).transpose(1, 0, 2))
    ref = xent_ref(tbv, batch["frame_target"], batch["sequence_length"])
    dlogits = np.ascontiguousarray(ref["grad"].transpose(1, 0, 2)).astype(np.asarray(logits).dtype)
    grads, _ = oracle.backward(params, cfg, saved, dlogits)
    clipped, norm = oracle.l2_and_clip(params, grads, 5.0, 1e-5)
    oracle.apply_optimizer(optimizer, params, clipped, state, lr)
    size = int(ref["frames"].sum())
    return dict(size=size, eval_loss=float(ref["loss"].sum()), eval=float(size - int(ref["correct"].sum())),
                grad_norm=float(norm))


@pytest.mark.parametrize("optimizer", ["adam", "sgd", "momentum"])
@pytest.mark.parametrize("model", sorted(MODELS))
def test_train_steps_vs_oracle_composition(oracle, model, optimizer):
    from lstm_ctc_amd.nnet.graph import create_graph_for_training_xent
    cfg = dict(MODEL_CFG, **MODELS[model])
    batch = _model_batch(cfg)
    graph = create_graph_for_training_xent(None, cfg, learn_rate=1e-2, clip_norm=5.0, optimizer=optimizer, seed=11)
    params = {k: v.copy() for k, v in graph.model.ps.export_tf().items()}
    state = {}
    for step in range(3):
        out = graph.step(batch, fetch_eval=True)
        ref = _oracle_step(oracle, params, cfg, batch, state, optimizer, 1e-2)
        assert "decoded" not in out
        assert out["size"] == ref["size"] == 14 + 1 + 12 - 1                  # utterance 1 and one "ignore" are not scored
        assert abs(out["eval_loss"] - ref["eval_loss"]) / ref["eval_loss"] < 1e-4
        assert abs(out["loss"] - ref["eval_loss"]) / ref["eval_loss"] < 1e-4  # no regulariser in this configuration
        assert out["eval"] == ref["eval"]
        assert abs(out["grad_norm"] - ref["grad_norm"]) / ref["grad_norm"] < 2e-3
        got = graph.model.ps.export_tf()
        for k in params:
            assert np.abs(got[k] - params[k]).max() < 2e-4 * max(1.0, np.abs(params[k]).max()), (step, k)


@pytest.mark.parametrize("model", sorted(MODELS))
def test_six_adam_steps_learn_the_frame_targets(oracle, model):
    """The float64 oracle alone goes 2.03 -> 1.39 (blstm) and 2.07 -> 1.30 (lstm) on this batch, monotonically (checked
    on the CPU; asserted again here)."""
    from lstm_ctc_amd.nnet.graph import create_graph_for_training_xent
    cfg = dict(MODEL_CFG, **MODELS[model])
    batch = _model_batch(cfg)
    graph = create_graph_for_training_xent(None, cfg, learn_rate=1e-2, clip_norm=5.0, optimizer="adam", seed=11)
    params = {k: v.copy() for k, v in graph.model.ps.export_tf().items()}
    state, got, want = {}, [], []
    for step in range(6):
        out = graph.step(batch)
        ref = _oracle_step(oracle, params, cfg, batch, state, "adam", 1e-2)
        got.append(out["eval_loss"] / out["size"])
        want.append(ref["eval_loss"] / ref["size"])
        assert abs(got[-1] - want[-1]) <= BAR * max(abs(want[-1]), 1.0), (step, got, want)
    print("\nmean frame loss (%s): gpu %s oracle %s" % (model, ["%.4f" % v for v in got], ["%.4f" % v for v in want]))
    assert got[-1] < got[0]
    assert all(b_ < a for a, b_ in zip(want, want[1:]))


def test_validation_graph_and_empty_batch():
    """A batch without a scored frame: size 0, loss 0 - and a training step still runs the optimizer (on the L2 term alone)."""
    from lstm_ctc_amd.nnet.graph import create_graph_for_training_xent
    cfg = dict(MODEL_CFG)
    batch = _model_batch(cfg)
    batch["frame_target"][:] = -1
    graph = create_graph_for_training_xent(None, cfg, learn_rate=1e-2, optimizer="sgd", seed=11)
    before = graph.model.ps.flat.clone()
    out = graph.step(batch, fetch_eval=True)
    assert out["size"] == 0 and out["eval_loss"] == 0.0 and out["eval"] == 0.0
    assert graph.opt_step == 1 and not torch.equal(before, graph.model.ps.flat)
    staged = graph.stage(_model_batch(cfg))                                  # the prefetch path carries the targets along
    out2 = graph.step(None, staged=staged, fetch_eval=True, train=False)
    assert out2["size"] == 26 and 0 <= out2["eval"] <= 26 and np.isfinite(out2["eval_loss"])


# ----------------------------------------------------------------------------------------------- command lines
def _run(cli, *args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", cli)] + list(args), capture_output=True, timeout=300)
    return r.returncode, r.stderr.decode()


def _logged(err, name):
    lines = [l for l in err.split("\n") if l.startswith("INFO:tensorflow:%s = " % name)]
    assert len(lines) == 1, err
    return float(lines[0].split()[-1])


def test_cli_chain_ctc_init_align_xent_train_validate(tmp_path):
    import lstm_ctc_amd.nnet as nnet
    from lstm_ctc_amd.kaldi_io import Int32VectorWriter, read_int32_vector_ark
    rng = np.random.default_rng(7)
    D, V = 6, 9
    lines = []
    for i, T in enumerate([20, 24, 31, 40]):
        path = str(tmp_path / ("utt%03d.tfrecords" % i))
        nnet.write_tfrecord(path, rng.normal(size=(T, D)).astype(np.float32), rng.integers(0, V - 1, size=int(rng.integers(1, 5))))
        lines.append("utt%03d %d %d 1 %s" % (i, T, D, path))
    scp = tmp_path / "tfrecords.scp"
    scp.write_text("\n".join(lines) + "\n")
    config = tmp_path / "nnet.config"
    config.write_text("nnet_type = blstm\ninput_dim = 6\nleft_context = 1\nright_context = 1\nsubsample = 2\nnum_layers = 2\n"
                      "num_neurons = 32\nnum_projects = 16\nnum_targets = 9\nuse_peepholes = true\ndropout_rate = 1.0\n")
    d = str(tmp_path)
    rc, err = _run("nnet-init.py", "--objective=ctc", "--batch-size", "2", str(scp), str(config), d + "/nnet.0")
    assert rc == 0, err
    rc, err = _run("nnet-align.py", str(scp), str(config), d + "/nnet.0", "ark:" + d + "/ali.ark")
    assert rc == 0, err
    table = read_int32_vector_ark(d + "/ali.ark")
    assert sorted(table) == ["utt%03d" % i for i in range(4)]
    assert [len(table["utt%03d" % i]) for i in range(4)] == [10, 12, 15, 20]           # frames after subsample = 2
    common = ["--objective=xent", "--frame-targets", "ark:" + d + "/ali.ark", "--batch-size", "2"]
    train = ["--learn-rate=0.01", "--optimizer=adam", "--seed=1", "--shuffle=false", "--report-interval=1"]
    rc, err = _run("nnet-train.py", *(common + train + [str(scp), str(config), d + "/nnet.0", d + "/nnet.1"]))
    assert rc == 0, err
    tr_loss = _logged(err, "tr_loss")
    assert np.isfinite(tr_loss)
    assert "INFO:tensorflow:frame targets: 0 utterance(s) without an entry, 0 with an entry of another length" in err
    assert "INFO:tensorflow:step = 1, batch_size = 22, loss = " in err                 # size = scored frames of the batch
    # the same batches through CTCGraph.step in this process
    cfg = nnet.parse_config(str(config))
    cfg["is_training"] = True
    _, ds, dim = nnet.dataset_from_tfrecords(tfrecords_scp=str(scp), left_context=1, right_context=1, subsample=2)
    _, pipe = nnet.create_pipeline_sequence_batch(dataset=ds, input_dim=dim, batch_size=2, frame_targets=table)
    graph = nnet.create_graph_for_training_xent(pipeline=pipe, nnet_config=cfg, learn_rate=0.01, optimizer="adam", seed=1)
    graph.restore(d + "/nnet.0")
    mean, seen = 0.0, 0
    for batch in pipe:
        out = graph.step(batch)
        seen += out["size"]
        mean += (out["eval_loss"] / out["size"] - mean) * out["size"] / seen
    assert seen == 57
    assert abs(mean - tr_loss) <= BAR * max(abs(mean), 1.0) + 1e-6, (mean, tr_loss)
    # validation: mean loss per frame and the frame error rate
    rc, err = _run("nnet-validate.py", *(common + ["--evaluate=true", str(scp), str(config), d + "/nnet.1"]))
    assert rc == 0, err
    assert np.isfinite(_logged(err, "cv_loss")) and 0.0 <= _logged(err, "cv_eval") <= 1.0
    # a table that lacks one utterance still trains, and says so
    w = Int32VectorWriter("ark,t:" + d + "/ali3.txt")
    for k in sorted(table)[1:]:
        w.Write(k, table[k])
    w.Close()
    rc, err = _run("nnet-train.py", "--objective=xent", "--frame-targets", "ark,t:" + d + "/ali3.txt", "--batch-size", "2",
                   *(train + [str(scp), str(config), d + "/nnet.0", d + "/nnet.2"]))
    assert rc == 0, err
    assert np.isfinite(_logged(err, "tr_loss"))
    assert "INFO:tensorflow:frame targets: 1 utterance(s) without an entry, 0 with an entry of another length" in err
    assert "INFO:tensorflow:step = 1, batch_size = 12, loss = " in err


def test_zz_report_measured_error_over_bound():
    print("\nxent: largest measured error / derived bound: loss %.3f, grad %.3f; loss error / project bar %.4f"
          % (MEASURED["loss"], MEASURED["grad"], MEASURED["loss_bar"]))
    assert MEASURED["loss"] <= 1.0 and MEASURED["grad"] <= 1.0 and MEASURED["loss_bar"] <= 1.0
