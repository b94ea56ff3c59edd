"""GPU parity tests of the streaming kernels of bn.hip and misc.hip PAST their launch caps: every kernel below walks its
data with a grid stride, and the other op-level tests stop at sizes where each lane makes one trip through that loop.  Here
each case takes the smallest shape that crosses the cap written in the code (and asserts that it does), runs on column
windows of wider buffers (row pitch > extent), and compares with a plain reference of the same operation.

Reductions are checked EXACTLY: their inputs are drawn from {+-1, +-3, +-5, +-7}, so every partial sum is an integer below
2^24 and fp32 (and double) arithmetic makes no rounding at all - the comparison is bit equality whatever the summation
order, and because every entry is odd and non-zero, one dropped or doubled element changes every sum it belongs to.
Where rounding is unavoidable the bound is derived in the test from the shape and the number format, or is one of the
suite's existing constants on the same input distribution; none was taken from what the kernels return."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# the launch caps, as written in lstm_ctc_amd/csrc/misc.hip and bn.hip (each case asserts that its shape exceeds them)
VEC_DROPOUT_QUADS = 16384 * 256        # dropout_scale_vec_kernel: 16384 blocks x 256 threads, one column quad each
SCALAR_DROPOUT_ELEMS = 2048 * 256      # dropout_scale_kernel: stream_grid(.., 256) caps at 2048 blocks
SLABS, SLAB_ROWS = 128, 4 * 64         # colsum / bn_moments / bn_bwd: <= 128 row slabs of 4 row phases, cdiv(rows, 256) of them
STREAM_ELEMS = 4096 * 256              # bn_apply / bn_bwd_apply / length_mask: stream_blocks caps at 4096 blocks
WAVE_ROWS = 2048 * 4                   # posteriors / label smoothing / MoE: 2048 blocks x 4 waves, one row per wave
OPT_BLOCKS, OPT_PER_BLOCK = 1024, 256 * 8      # optimizer: cdiv(n, 2048) blocks, capped at 1024; norm_finish folds on 256 threads
U = 2.0 ** -24                         # unit roundoff of fp32


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from lstm_ctc_amd import ops as o, _lib
    _lib.load()
    return o


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def odd_ints(rng, shape):
    """Entries from {+-1, +-3, +-5, +-7} as float32."""
    return (rng.integers(0, 4, size=shape) * 2 + 1).astype(np.float32) * rng.choice(np.float32([-1, 1]), size=shape)


def assert_exact_sums(*cols):
    """The property that makes an integer case exact: every column's sum of magnitudes stays below 2^24."""
    for a in cols:
        assert float(np.abs(a.astype(np.float64)).sum(axis=0).max()) < 2 ** 24


def slabs_of(rows):
    return min(SLABS, -(-rows // SLAB_ROWS))


def tree_depth(rows):
    """Additions on the longest path of the documented column-sum tree: a thread's serial run over its rows (cdiv(rows,
    4 * slabs) of them), two levels over the four row phases, one serial fold over the slabs."""
    ny = slabs_of(rows)
    return -(-rows // (4 * ny)) + 2 + ny


# ================================================================================================ 1. vector dropout, wrapped
KEEP, SEED, STREAM = 0.8, 31, 4


@pytest.fixture(scope="module")
def dropout_case(oracle):
    """(rows, P) -> inputs and the oracle mask of that shape, made once, left unchanged and released with the module: x
    normal, xd / yd dyadic (multiples of 1/8 and integers)."""
    cache = {}

    def get(rows, P):
        if (rows, P) not in cache:
            rng = np.random.default_rng(rows + P)
            x = rng.normal(size=(rows, 2 * P)).astype(np.float32)
            xd = (rng.integers(-64, 65, size=(rows, 2 * P)) / 8.0).astype(np.float32)
            yd = odd_ints(rng, (rows, P))
            m = oracle.dropout_mask(SEED, STREAM, (rows, 1, P), KEEP).reshape(rows, P)
            assert set(np.unique(m).tolist()) == {0.0, 1.25}          # 1 / 0.8f rounds to 1.25 exactly
            cache[(rows, P)] = (x, xd, yd, m)
        return cache[(rows, P)]

    yield get
    cache.clear()


@pytest.mark.parametrize("form", ["in_place", "accumulate", "shadow"])
@pytest.mark.parametrize("rows,P,carry", [(53000, 320, True), (16500, 1024, False)])
def test_vector_dropout_wrapped(ops, oracle, dropout_case, rows, P, carry, form):
    """dropout_scale_vec_kernel<false/true> beyond its 16384-block grid: the lanes of the first blocks make a second trip,
    advancing (row, column quad) by the precomputed (dr, dc) with a carry.  The carry branch is taken only when the grid
    stride is no multiple of P / 4: at P = 320 (c2's width) it is, at P = 1024 (c4's) it never is - both arms are pinned.
    Bit equality with x * oracle mask on a column window of a [rows, 2P] buffer.  The accumulating form uses dyadic inputs
    (x multiples of 1/8, y integers, factor 1.25): x * f + y is then exact, so the comparison does not depend on whether the
    compiler contracts the multiply and the add into one fma."""
    quads, stride = rows * (P // 4), VEC_DROPOUT_QUADS
    assert quads > VEC_DROPOUT_QUADS                                     # the walk wraps
    assert (stride % (P // 4) != 0) == carry                            # ... with / without the carry branch
    if carry:
        second = np.arange(quads - stride) % (P // 4) + stride % (P // 4) >= P // 4         # lanes whose second trip carries
        assert second.any() and not second.all()
    xh, xd, yd, m = dropout_case(rows, P)
    if form == "accumulate":
        x, y = dev(xd), dev(yd)
        ops.dropout_scale(x[:, P:], KEEP, SEED, STREAM, out=y, accumulate=True)
        assert np.array_equal(host(y), yd + xd[:, P:] * m)
        assert np.array_equal(host(x), xd)                               # the source is only read
        return
    x = dev(xh)
    want = xh[:, P:] * m
    if form == "in_place":
        ops.dropout_scale(x[:, P:], KEEP, SEED, STREAM)
    else:
        sh = torch.zeros((rows, 2 * P), dtype=torch.bfloat16, device="cuda")
        ops.dropout_scale(x[:, P:], KEEP, SEED, STREAM, shadow=sh[:, P:])
    got = host(x)
    assert np.array_equal(bits(got[:, P:]), bits(want))
    assert np.array_equal(bits(got[:, :P]), bits(xh[:, :P]))             # the other half of the buffer is untouched
    if form == "shadow":
        assert np.array_equal(host(sh[:, P:].float()), oracle.bf16_round(want))
        assert not host(sh[:, :P].float()).any()
        nat, _ = ops.cast_bf16(x[:, P:].contiguous(), nat=True, tr=False)
        assert torch.equal(nat, sh[:, P:].contiguous())


# ================================================================================================ 2. scalar dropout, wrapped
@pytest.mark.parametrize("accumulate", [False, True])
def test_scalar_dropout_wrapped(ops, oracle, accumulate):
    """dropout_scale_kernel (P no multiple of 4) beyond its 2048-block grid, source and destination windows of buffers with
    different pitches.  Exact; the accumulating form on dyadic inputs, as above."""
    rows, P = 4100, 129
    assert P % 4 != 0 and rows * P > SCALAR_DROPOUT_ELEMS
    rng = np.random.default_rng(129)
    m = oracle.dropout_mask(7, 9, (rows, 1, P), KEEP).reshape(rows, P)
    if accumulate:
        xh = (rng.integers(-64, 65, size=(rows, 140)) / 8.0).astype(np.float32)
        yh = odd_ints(rng, (rows, 151))
    else:
        xh = rng.normal(size=(rows, 140)).astype(np.float32)
        yh = rng.normal(size=(rows, 151)).astype(np.float32)
    x, y = dev(xh), dev(yh)
    ops.dropout_scale(x[:, 3:3 + P], KEEP, 7, 9, out=y[:, 5:5 + P], accumulate=accumulate)
    want = yh.copy()
    want[:, 5:5 + P] = yh[:, 5:5 + P] + xh[:, 3:3 + P] * m if accumulate else xh[:, 3:3 + P] * m
    assert np.array_equal(bits(host(y)), bits(want))                     # the window exactly, the rest untouched
    assert np.array_equal(bits(host(x)), bits(xh))


# ================================================================================================ 3. colsum
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("rows", [255, 256, 257, 33000])
def test_colsum_exact(ops, rows, accumulate):
    """colsum_partial / colsum_fold on integer input: 1 slab, 1 slab, 2 slabs, and the 128-slab cap with 64 - 65 rows per
    thread; N = 70 is two column groups, the second ragged; the input is a column window (ldx > N).  Bit equality with the
    int64 sum."""
    N = 70
    assert slabs_of(rows) == {255: 1, 256: 1, 257: 2, 33000: SLABS}[rows]
    if rows == 33000:
        assert -(-rows // SLAB_ROWS) > SLABS and rows % (4 * SLABS) != 0           # capped, and threads differ in their trip count
    rng = np.random.default_rng(rows)
    xh = odd_ints(rng, (rows, 100))
    o0 = odd_ints(rng, N)
    assert_exact_sums(np.concatenate([xh[:, 13:13 + N], o0[None]]))
    out = dev(o0)
    got = ops.colsum(dev(xh)[:, 13:13 + N], out=out, accumulate=accumulate)
    want = xh[:, 13:13 + N].astype(np.int64).sum(axis=0) + (o0.astype(np.int64) if accumulate else 0)
    assert got is out and np.array_equal(host(got).astype(np.float64), want.astype(np.float64))


def test_colsum_normal_within_the_tree_bound(ops):
    """Random normal input at the slab cap: |sum - float64 sum| <= d * 2^-24 * sum |x| per column, d the depth of the
    documented summation tree, computed from the shape."""
    rows, N = 33000, 70
    rng = np.random.default_rng(5)
    xh = rng.normal(size=(rows, 100)).astype(np.float32)
    got = host(ops.colsum(dev(xh)[:, 13:13 + N])).astype(np.float64)
    w = xh[:, 13:13 + N].astype(np.float64)
    d = tree_depth(rows)
    assert d == 65 + 2 + 128
    err, bound = np.abs(got - w.sum(axis=0)), d * U * np.abs(w).sum(axis=0)
    print("colsum: largest error / bound", float((err / bound).max()))
    assert (err <= bound).all()


# ================================================================================================ 4. / 5. batch normalisation
ROWS, C = 33000, 70
XW, YW = (17, 100), (11, 90)          # (first column, buffer width) of the windows the activations live in
NAME = "bn"


def _window(a, w, rng):
    """a [rows, C] as the window w of a wider buffer filled with other numbers; -> (host buffer, device window, device buffer)."""
    buf = rng.normal(size=(a.shape[0], w[1])).astype(np.float32)
    buf[:, w[0]:w[0] + a.shape[1]] = a
    d = dev(buf)
    return buf, d[:, w[0]:w[0] + a.shape[1]], d


def _untouched_outside(buf_host, buf_dev, w, ncol):
    got = host(buf_dev)
    return (np.array_equal(bits(got[:, :w[0]]), bits(buf_host[:, :w[0]])) and
            np.array_equal(bits(got[:, w[0] + ncol:]), bits(buf_host[:, w[0] + ncol:])))


def emulate_moments(x, handover=np.float64):
    """The arithmetic bn.hip's header documents, in numpy: float32 partials per (slab, row phase) - thread (k, s) adds rows
    4k + s, 4k + s + 4 * slabs, ... in order - then `handover` (double in the kernel) for the sums over the four phases, the
    slabs in index order, and mean / variance.  -> (mean, var) in float32."""
    rows, ncol = x.shape
    ny = slabs_of(rows)
    trips = -(-rows // (4 * ny))
    xp = np.zeros((trips * 4 * ny, ncol), np.float32)                    # + 0 is exact: pad the last trip
    xp[:rows] = x
    xp = xp.reshape(trips, 4 * ny, ncol)
    s0, s1 = np.zeros((4 * ny, ncol), np.float32), np.zeros((4 * ny, ncol), np.float32)
    for t in range(trips):
        s0 += xp[t]
        s1 += xp[t] * xp[t]
    tot = []
    for s in (s0, s1):
        p = s.reshape(ny, 4, ncol).astype(handover)
        part = ((p[:, 0] + p[:, 1]) + p[:, 2]) + p[:, 3]
        a = np.zeros(ncol, handover)
        for k in range(ny):
            a = a + part[k]
        tot.append(a)
    m = tot[0] / handover(rows)
    v = tot[1] / handover(rows) - m * m
    return m.astype(np.float32), np.maximum(v, 0).astype(np.float32)


def plain_fp32_moments(x):
    """One pass in float32 from end to end: running sums of x and x^2 down the rows, var = E[x^2] - mean^2."""
    n = np.float32(x.shape[0])
    m = np.cumsum(x, axis=0, dtype=np.float32)[-1] / n
    return m, np.cumsum(x * x, axis=0, dtype=np.float32)[-1] / n - m * m


@pytest.fixture(scope="module")
def bn_case(oracle):
    """One BN problem at the slab cap, made once: normal x, integer dy, random gamma / beta / moving statistics, and the
    float64 oracle's forward and backward for training and inference."""
    assert -(-ROWS // SLAB_ROWS) > SLABS and ROWS * C > STREAM_ELEMS and XW[1] > C and YW[1] > C
    rng = np.random.default_rng(70)
    c = dict(x=rng.normal(size=(ROWS, C)).astype(np.float32), dy=odd_ints(rng, (ROWS, C)))
    c["params"] = {NAME + "/gamma": rng.uniform(0.5, 2.0, C).astype(np.float32),
                   NAME + "/beta": rng.normal(size=C).astype(np.float32),
                   NAME + "/moving_mean": rng.normal(0, 0.3, C).astype(np.float32),
                   NAME + "/moving_variance": rng.uniform(0.5, 2.0, C).astype(np.float32)}
    p64 = {k: v.astype(np.float64) for k, v in c["params"].items()}
    for training in (True, False):
        y, sv = oracle.bn_forward(c["x"].astype(np.float64), p64, NAME, training)
        c[training] = dict(y=y, sv=sv, bwd=oracle.bn_backward(sv, p64, NAME, c["dy"].astype(np.float64)))
    return c


def _bn_forward_on_windows(ops, xh, params, training, seed=1):
    rng = np.random.default_rng(seed)
    xbuf, xw, xd = _window(xh, XW, rng)
    ybuf, yw, yd = _window(np.zeros_like(xh), YW, rng)
    p = {k[len(NAME) + 1:]: dev(v) for k, v in params.items()}
    y, mean, var = ops.bn_forward(xw, p["gamma"], p["beta"], training, p["moving_mean"], p["moving_variance"], out=yw)
    assert y is yw
    assert _untouched_outside(ybuf, yd, YW, C) and np.array_equal(bits(host(xd)), bits(xbuf))
    return host(yw), host(mean), host(var)


def _unit_params():
    return {NAME + "/gamma": np.ones(C, np.float32), NAME + "/beta": np.zeros(C, np.float32),
            NAME + "/moving_mean": np.zeros(C, np.float32), NAME + "/moving_variance": np.ones(C, np.float32)}


def test_bn_moments_exact_on_integers(ops):
    """bn_moments_partial / bn_fold / bn_moments_finish at the 128-slab cap on integer input: both column sums are exact in
    every format, so mean and var may differ from the float64 evaluation of sum / rows and sum2 / rows - mean^2 only in the
    final cast to float32: one ulp."""
    assert -(-ROWS // SLAB_ROWS) > SLABS and slabs_of(ROWS) == SLABS and ROWS * C > STREAM_ELEMS
    rng = np.random.default_rng(4)
    xh = odd_ints(rng, (ROWS, C))
    assert_exact_sums(xh, xh * xh)
    _, mean, var = _bn_forward_on_windows(ops, xh, _unit_params(), True)
    x64 = xh.astype(np.float64)
    m = x64.sum(axis=0) / ROWS
    v = (x64 * x64).sum(axis=0) / ROWS - m * m
    for got, ref in ((mean, m), (var, v)):
        r32 = ref.astype(np.float32)
        assert (np.abs(got.astype(np.float64) - r32.astype(np.float64)) <= np.spacing(np.abs(r32))).all()


def test_bn_variance_of_offset_input_needs_the_double_handover(ops, oracle):
    """x = N(10, 1): var = E[x^2] - mean^2 cancels two numbers near 101 to one near 1.  Reference: oracle.bn_forward in
    float64; measure: largest relative error of var over the columns; bound: 10 x the error that the numpy emulation of the
    header's documented arithmetic (float32 partials per slab and row phase, double from there on) makes on the same input.
    A plain float32 one-pass evaluation must miss that bound - so would a kernel that hands over in float.
    The same tree with a float32 hand-over misses it too.
    Measured (default_rng(0), 33000 x 70): emulation 3.0e-6, plain float32 one-pass 1.8e-3, float32 hand-over 9.6e-5, the
    kernels 3.0e-6 (their partials may contract v * v + s into one fma; the emulation rounds the product first)."""
    assert -(-ROWS // SLAB_ROWS) > SLABS and slabs_of(ROWS) == SLABS and ROWS * C > STREAM_ELEMS
    rng = np.random.default_rng(0)
    xh = (10.0 + rng.normal(size=(ROWS, C))).astype(np.float32)
    _, sv = oracle.bn_forward(xh.astype(np.float64), {k: v.astype(np.float64) for k, v in _unit_params().items()}, NAME, True)
    rel = lambda v: float((np.abs(v.astype(np.float64) - sv["var"]) / sv["var"]).max())
    e_emul, e_plain = rel(emulate_moments(xh)[1]), rel(plain_fp32_moments(xh)[1])
    _, mean, var = _bn_forward_on_windows(ops, xh, _unit_params(), True)
    e_gpu = rel(var)
    print("bn var relative error: emulation %.3g, plain fp32 %.3g, kernels %.3g" % (e_emul, e_plain, e_gpu))
    e_float = rel(emulate_moments(xh, np.float32)[1])
    print("bn var relative error: float32 hand-over %.3g" % e_float)
    assert e_plain > 10 * e_emul and e_float > 10 * e_emul
    assert e_gpu <= 10 * e_emul
    # the mean: the float32 part of the tree (a thread's rows, then the four phases) and the final cast
    bound = ((tree_depth(ROWS) - slabs_of(ROWS)) * U * np.abs(xh.astype(np.float64)).sum(axis=0) / ROWS
             + np.spacing(np.abs(sv["mean"]).astype(np.float32)))
    assert (np.abs(mean.astype(np.float64) - sv["mean"]) <= bound).all()


@pytest.mark.parametrize("training", [True, False])
def test_bn_apply_wrapped_vs_oracle(ops, bn_case, training):
    """bn_apply beyond its 4096-block grid (2.31 M elements), input and output windows of different pitches; inference uses
    the moving statistics.  y within 1e-5 * max|y| of oracle.bn_forward in float64 on N(0, 1) input with random gamma and
    beta: the margin over one rsqrtf and two float32 multiplies (a few 2^-24 of |y|).  Measured worst error:
    7.1e-8 * max|y| (training), 8.7e-8 * max|y| (inference)."""
    y, mean, var = _bn_forward_on_windows(ops, bn_case["x"], bn_case["params"], training)
    ref = bn_case[training]
    err = float(np.abs(y - ref["y"]).max() / np.abs(ref["y"]).max())
    print("bn y error / max|y| (training=%s): %.3g" % (training, err))
    assert err <= 1e-5


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("training", [True, False])
def test_bn_backward_wrapped_vs_oracle(ops, bn_case, training, in_place):
    """bn_bwd_partial / bn_fold / bn_bwd_apply at the slab cap and beyond the 4096-block grid, x / dy / dx windows of
    different pitches, dx separate and in place over dy.  dbeta: exact (integer dy).  dgamma: within the summation bound of
    the column-sum tree applied to |dy * xhat| (float64 oracle).  dx: within 1e-5 * max|dx| of oracle.bn_backward.
    Measured worst dx error: 1.4e-7 * max|dx| (training), 5.6e-8 * max|dx| (inference); dgamma: 3e-4 of its bound."""
    rng = np.random.default_rng(2)
    xh, dyh, params = bn_case["x"], bn_case["dy"], bn_case["params"]
    assert_exact_sums(dyh)
    ref = bn_case[training]
    dx_ref, dgamma_ref, dbeta_ref = ref["bwd"]
    xbuf, xw, xd = _window(xh, XW, rng)
    dybuf, dyw, dyd = _window(dyh, (5, 96), rng)
    if training:                                                          # the statistics the forward pass returns
        _, mean, var = ops.bn_forward(xw, dev(params[NAME + "/gamma"]), dev(params[NAME + "/beta"]), True, None, None)
    else:
        mean, var = dev(params[NAME + "/moving_mean"]), dev(params[NAME + "/moving_variance"])
    dgamma, dbeta = torch.full((C,), np.nan, device="cuda"), torch.full((C,), np.nan, device="cuda")
    if in_place:
        dxbuf, dxw, dxd, w = dybuf, dyw, dyd, (5, 96)
    else:
        dxbuf, dxw, dxd = _window(np.zeros_like(xh), YW, rng)
        w = YW
    dx = ops.bn_backward(xw, dyw, mean, var, dev(params[NAME + "/gamma"]), training, dgamma, dbeta, dx=dxw)
    assert dx is dxw
    assert np.array_equal(host(dbeta).astype(np.float64), dbeta_ref)
    bound = tree_depth(ROWS) * U * np.abs(dyh.astype(np.float64) * ref["sv"]["xhat"]).sum(axis=0)
    eg = np.abs(host(dgamma) - dgamma_ref)
    err = float(np.abs(host(dxw) - dx_ref).max() / np.abs(dx_ref).max())
    print("bn backward (training=%s): dx error / max|dx| %.3g, dgamma error / bound %.3g" % (training, err, float((eg / bound).max())))
    assert (eg <= bound).all()
    assert err <= 1e-5
    assert _untouched_outside(dxbuf, dxd, w, C) and np.array_equal(bits(host(xd)), bits(xbuf))
    if not in_place:
        assert np.array_equal(bits(host(dyd)), bits(dybuf))


def test_bn_update_moving_exact(ops, oracle):
    """assign_moving_average is one float32 expression, v - (v - batch) * float32(1 - momentum): the same bits as
    oracle.bn_update_moving."""
    rng = np.random.default_rng(3)
    n = 1000                                                             # four blocks, the last ragged
    mm, mv = rng.normal(size=n).astype(np.float32), rng.uniform(0.5, 2, n).astype(np.float32)
    mean, var = rng.normal(size=n).astype(np.float32), rng.uniform(0.5, 2, n).astype(np.float32)
    params = {NAME + "/moving_mean": mm.copy(), NAME + "/moving_variance": mv.copy()}
    oracle.bn_update_moving(params, dict(bn={NAME: dict(mean=mean, var=var)}))
    dmm, dmv = dev(mm), dev(mv)
    ops.bn_update_moving(dmm, dmv, dev(mean), dev(var))
    assert np.array_equal(bits(host(dmm)), bits(params[NAME + "/moving_mean"]))
    assert np.array_equal(bits(host(dmv)), bits(params[NAME + "/moving_variance"]))


# ================================================================================================ 6. length mask
def test_length_mask_wrapped_on_a_window(ops):
    """length_mask_kernel beyond its 4096-block grid on a column window: rows of live frames keep their bits, rows beyond
    an utterance's length (filled with NaN and 1e30) become exactly +0.0, nothing outside the window changes."""
    T, B, Cm, ld, c0 = 50, 33, 640, 1024, 200
    assert T * B * Cm > STREAM_ELEMS
    rng = np.random.default_rng(6)
    seq = rng.integers(1, T, size=B).astype(np.int32)
    seq[[4, 20]], seq[[0, 31]] = 0, T                                    # unsorted, with empty and full utterances
    assert not (np.diff(seq) <= 0).all() and not (np.diff(seq) >= 0).all()
    dead = (np.arange(T)[:, None] >= seq[None, :]).reshape(T * B)
    buf = rng.normal(size=(T * B, ld)).astype(np.float32)
    buf[dead, ::2], buf[dead, 1::2] = np.nan, 1e30                       # also outside the window: it must stay
    assert dead.any() and not dead.all()
    x = dev(buf)
    out = ops.length_mask_(x[:, c0:c0 + Cm], dev(seq), T, B)
    got = bits(host(x))
    want = bits(buf).copy()
    want[dead, c0:c0 + Cm] = 0                                           # the bits of +0.0
    assert out.data_ptr() == x[:, c0:c0 + Cm].data_ptr() and np.array_equal(got, want)


# ================================================================================================ 7. posteriors, label smoothing
WIDE = [(8300, 44), (70, 64), (70, 65), (70, 72), (70, 200)]


@pytest.mark.parametrize("rows,V", WIDE)
def test_posteriors_wrapped_rows_and_wide_alphabets(ops, rows, V):
    """posteriors_kernel beyond 2048 blocks x 4 rows, and its V > 64 lane loops: all four apply_softmax / apply_log
    combinations, with and without the prior, against float64; atol 1e-5 on the input distribution of
    test_posteriors_and_colsum_transpose."""
    assert rows > WAVE_ROWS or V >= 64
    rng = np.random.default_rng(19 + V)
    x = rng.normal(size=(rows, V)).astype(np.float32)
    prior = rng.normal(size=V).astype(np.float32)
    z = 0.7 * x.astype(np.float64)
    lsm = z - z.max(1, keepdims=True) - np.log(np.exp(z - z.max(1, keepdims=True)).sum(1, keepdims=True))
    xd, pd = dev(x), dev(prior)
    for softmax in (True, False):
        for log in (True, False):
            for pr in (None, prior):
                got = host(ops.posteriors(xd, 0.7, softmax, log, pd if pr is not None else None))
                ref = (lsm if log else np.exp(lsm)) if softmax else x.astype(np.float64)
                ref = ref - (pr.astype(np.float64) if pr is not None else 0.0)
                np.testing.assert_allclose(got, ref, rtol=0, atol=1e-5, err_msg=str((softmax, log, pr is not None)))


@pytest.mark.parametrize("with_prior", [True, False])
@pytest.mark.parametrize("rows,V", WIDE)
def test_label_smoothing_wrapped_rows_and_wide_alphabets(ops, oracle, rows, V, with_prior):
    """label_smooth_kernel beyond 2048 blocks x 4 rows, and its V > 64 lane loops, with a class prior (one -1e10 entry) and
    uniform, with the gradient accumulated into dlogits and with dlogits = None; inputs and tolerances of
    test_label_smoothing_kernel_prior_vs_oracle (loss 1e-5 relative, gradient 1e-4 * max(1, max|g|))."""
    assert rows > WAVE_ROWS or V >= 64
    rng = np.random.default_rng(2 + V)
    logits = rng.normal(0, 2.0, size=(rows, V)).astype(np.float32)
    logq = np.log(rng.dirichlet(np.ones(V))).astype(np.float32)
    logq[3] = -1e10
    base = rng.normal(size=(rows, V)).astype(np.float32)
    cfg = dict(prior_label_sm=0.3) if with_prior else dict(uniform_label_sm=0.3)
    rl, rg = oracle.label_smoothing(logits.astype(np.float64)[None], cfg, logq.astype(np.float64) if with_prior else None)
    ld, qd = dev(logits), dev(logq) if with_prior else None
    d = dev(base)
    acc = ops.label_smoothing(ld, 0.3, qd, d)
    assert abs(float(acc.item()) - rl) / abs(rl) < 1e-5
    got = host(d) - base
    assert np.abs(got - rg[0]).max() < 1e-4 * max(1.0, np.abs(rg).max())
    acc = ops.label_smoothing(ld, 0.3, qd, None)                         # the value alone
    assert abs(float(acc.item()) - rl) / abs(rl) < 1e-5


# ================================================================================================ 8. MoE combine
@pytest.mark.parametrize("keep", [1.0, 0.8])
@pytest.mark.parametrize("R,E,V,H", [(8300, 3, 5, 8), (9, 65, 130, 8)])
def test_moe_combine_wrapped_rows_and_wide_experts(ops, oracle, R, E, V, H, keep):
    """moe_fwd / moe_bwd beyond 2048 blocks x 4 rows, and their E > 64 and V > 64 lane loops, against oracle.moe_fwd /
    moe_bwd exactly as test_moe_combine does, with its tolerances; the gate probabilities of every row sum to 1."""
    assert R > WAVE_ROWS or (E > 64 and V > 64)
    rng = np.random.default_rng(13 + R)
    h = rng.normal(size=(R, H)).astype(np.float32)
    Wp, bp = rng.normal(0, .3, (H, E)).astype(np.float32), rng.normal(0, .1, E).astype(np.float32)
    W, b = rng.normal(0, .3, (H, E * V)).astype(np.float32), rng.normal(0, .1, E * V).astype(np.float32)
    dy = rng.normal(size=(R, V)).astype(np.float32)
    dpi = oracle.dropout_mask(3, 1000, (R, 1, E), keep).reshape(R, E) if keep < 1 else None
    dz = oracle.dropout_mask(3, 1001, (R, 1, E * V), keep).reshape(R, E * V) if keep < 1 else None
    y_ref, sv = oracle.moe_fwd(h.astype(np.float64), Wp, bp, W, b, 10.0, dpi, dz)
    dh_ref, g_ref = oracle.moe_bwd(sv, Wp.astype(np.float64), W.astype(np.float64), 10.0, dy.astype(np.float64))
    a = ops.gemm(dev(h), dev(Wp), bias=dev(bp))
    q = ops.gemm(dev(h), dev(W), bias=dev(b))
    logits, pi = ops.moe_combine_fwd(a, q, E, V, 10.0, keep, 3)
    np.testing.assert_allclose(host(logits), y_ref, atol=2e-4)
    assert np.abs(host(pi).astype(np.float64).sum(axis=1) - 1.0).max() <= 1e-6
    da = ops.moe_combine_bwd(pi, q, dev(dy), E, V, 10.0, keep, 3)
    dh = ops.gemm(da, dev(Wp), tb=True)
    ops.gemm(q, dev(W), tb=True, out=dh, beta=1.0)
    np.testing.assert_allclose(host(dh), dh_ref, atol=2e-3, rtol=1e-3)
    np.testing.assert_allclose(host(ops.gemm(dev(h), da, ta=True)), g_ref["Wp"], atol=2e-3, rtol=1e-3)
    np.testing.assert_allclose(host(ops.colsum(q)), g_ref["b"], atol=2e-3, rtol=1e-3)


# ================================================================================================ 9. optimizer
def _opt_inputs(n):
    rng = np.random.default_rng(17)
    p0 = rng.normal(size=n).astype(np.float32)
    g0 = (rng.normal(size=n) * 3).astype(np.float32)
    g0[n - 100] = 1000.0            # one large element in the last 256 (its partial is folded in norm_finish's first trip)
    g0[SPIKE] = 1000.0              # and one in a partial that norm_finish reaches only on a later trip (asserted in the test)
    return p0, g0


SPIKE = 400000


def _partial_index(i, vec):
    """The block of l2_sumsq_kernel (= index of the partial) that takes element i: a grid stride of 1024 x 256 threads over
    the elements, or over their quads on the 16-byte path."""
    return ((i // 4 if vec else i) % (OPT_BLOCKS * 256)) // 256


@pytest.mark.parametrize("n_decay", [2000000, 2000001])       # the second: element-wise L2 pass although n % 4 == 0
@pytest.mark.parametrize("n", [2101252, 2101251])             # 16-byte and element-wise paths
@pytest.mark.parametrize("opt", ["sgd", "momentum", "adam"])
def test_optimizer_past_the_block_cap(ops, oracle, opt, n, n_decay):
    """l2_sumsq / norm_finish / update beyond the 1024-block cap: every lane loops, and norm_finish folds 1024 partials on
    256 threads in four trips.  Two steps against oracle.l2_and_clip / apply_optimizer: parameters to the suite's atol 2e-6,
    the norm to 1e-6 relative, the gradient buffer after the L2 pass to 1e-7 * max|g| - and, since that is 1e-4 here, also
    element by element to the two roundings that g + l2 * theta can differ by between a fused and a separate multiply-add."""
    blocks = -(-n // OPT_PER_BLOCK)
    assert blocks > OPT_BLOCKS and OPT_BLOCKS > 256 and n_decay < n
    assert (n % 4 == 0) == (n == 2101252) and (n_decay % 4 == 0) == (n_decay == 2000000)
    p0, g0 = _opt_inputs(n)
    assert float(g0[n - 100]) ** 2 > 0.01 * float(np.square(g0, dtype=np.float64).sum())          # element n - 100: in the last 256
    assert _partial_index(SPIKE, n % 4 == 0 and n_decay % 4 == 0) >= 256 and g0[SPIKE] == 1000.0  # a partial of a later trip
    params = {"w": p0[:n_decay].copy(), "x/bias": p0[n_decay:].copy()}
    grads = {"w": g0[:n_decay].copy(), "x/bias": g0[n_decay:].copy()}
    P, G = dev(p0), dev(g0)
    state = torch.zeros(2 * n, device="cuda")
    norm = torch.zeros(2, device="cuda")
    ost = {}
    for step in (1, 2):
        before = host(P)
        ops.optimizer_step(P, G, n_decay, 1e-5, 5.0, opt, 1e-2, step, state, norm)
        cl, nrm = oracle.l2_and_clip(params, grads, 5.0, 1e-5)
        l2p = np.zeros(n, np.float32)
        l2p[:n_decay] = before[:n_decay] * np.float32(1e-5)
        g_ref = g0 + l2p                                                 # what l2_and_clip adds before it rescales
        g_got = host(G)
        assert np.abs(g_got - g_ref).max() <= 1e-7 * np.abs(g_ref).max()
        assert (np.abs(g_got - g_ref) <= 2 * np.spacing(np.abs(g_ref) + np.abs(l2p))).all()
        assert np.array_equal(bits(g_got[n_decay:]), bits(g0[n_decay:]))
        oracle.apply_optimizer(opt, params, cl, ost, 1e-2)
        assert abs(norm[0].item() - nrm) / nrm < 1e-6
        ref = np.concatenate([params["w"], params["x/bias"]])
        np.testing.assert_allclose(host(P), ref, atol=2e-6)
        G.copy_(dev(g0))


@pytest.mark.parametrize("opt", ["momentum", "adam"])
def test_optimizer_guard(ops, opt):
    """update_kernel's guard: a non-zero device word leaves parameters and both slots bit-unchanged (the norm is still
    reported); a zero word gives the same bits as no guard at all."""
    n, n_decay = 2101252, 2000000
    assert -(-n // OPT_PER_BLOCK) > OPT_BLOCKS                           # every lane of update_kernel loops
    p0, g0 = _opt_inputs(n)
    rng = np.random.default_rng(1)
    s0 = np.abs(rng.normal(size=2 * n)).astype(np.float32)

    def run(guard):
        P, G, S = dev(p0), dev(g0), dev(s0)
        norm = torch.zeros(2, device="cuda")
        g = None if guard is None else torch.tensor([guard], dtype=torch.int32, device="cuda")
        ops.optimizer_step(P, G, n_decay, 1e-5, 5.0, opt, 1e-2, 3, S, norm, guard=g)
        return bits(host(P)), bits(host(S)), bits(host(norm))

    free, zero, held = run(None), run(0), run(1)
    assert np.array_equal(held[0], bits(p0)) and np.array_equal(held[1], bits(s0))
    assert np.array_equal(held[2], free[2]) and held[2][0] != 0
    assert not np.array_equal(free[0], bits(p0))                         # the free run did move the parameters
    for a, b in zip(free, zero):
        assert np.array_equal(a, b)


# ================================================================================================ 10. transpose
@pytest.mark.parametrize("rows,cols", [(1000, 1030), (33, 4096)])
def test_transpose_ragged_tiles(ops, rows, cols):
    """transpose_kernel on several 32 x 32 tiles in both directions with ragged edge tiles: exactly x.T."""
    assert (rows % 32 or cols % 32) and rows > 32 and cols > 32
    x = np.random.default_rng(rows).normal(size=(rows, cols)).astype(np.float32)
    got = ops.transpose(dev(x))
    assert got.shape == (cols, rows) and np.array_equal(bits(host(got)), bits(x.T))
