"""The bf16 / bf16x3 product router and its shadow cache on the device, at the shapes where each route begins.

(a) Every row of ROUTES (tests/test_bf16_routes_host.py, the one table of `Model._mm`'s decision) through a real Model: the
    route taken is the one the host file pins, the result agrees with the float64 product of the operands as the kernel
    rounds them, nothing is written outside an `out` window, and the padded route's pad columns and pad product are zero.
(b) Whole training steps with every shadow getter wrapped: a shadow handed to a product, or registered by the kernel that
    wrote it, is bit for bit the round-to-nearest-even bf16 (the exact three-term split) of its fp32 source AS IT IS AT THAT
    MOMENT - a stale cache hit or a wrong window costs one bf16 ulp and fails here.
(c) Every product of those steps, caught at the funnel all product wrappers pass through (ops._product), against float64 on
    the operands as passed - at the views, strides, `beta` and `out` windows the model really uses.

Bounds are the project's own (test_gpu_ops.py): bf16 kernels |alpha| * 2e-6 * K * 4 + 1e-5 absolute; x3 and fp32 kernels
error over the sum of magnitudes below 3e-7 * max(1, sqrt(K) / 4).  The steps' operands are not N(0, 1) (gradients are
small), so (c) holds the bf16 kernels to a second, scale-free bound as well: their operands are exact, a product of two
bf16 values is exact in float32, and K + 3 float32 roundings (the sum in any order, alpha, beta * C, bias) cannot leave
more than (K + 3) * 2^-24 of the sum of magnitudes - whatever the order.

Every test prints its figures (largest error / bound per route or kernel, wall time) before it asserts; the last test
prints the table of them and, with LC_MEASURED_DIR set, writes it to bf16_route_tests.txt in that directory (kept as
profiles/bf16_route_tests.txt).
"""
import collections
import os
import time
import zlib

import numpy as np
import pytest
import torch

from test_bf16_routes_host import (ALPHA, ROUTES, SENTINEL, Spy, call_mm, check_route, error_ratio, is_big, operands,
                                   reference, unsplit_x3)

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
MEASURED = {}                       # route -> [largest error / bound over its ROUTES rows, rows]
WALL = {}                           # test -> seconds, the device drained


@pytest.fixture(autouse=True)
def _wall(request):
    t0 = time.perf_counter()
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    WALL[request.node.name] = time.perf_counter() - t0


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from lstm_ctc_amd import ops as o, _lib
    _lib.load()
    return o


# ------------------------------------------------------------------------------------------ (a) every ROUTES row
_TINY = dict(nnet_type="blstm", input_dim=8, left_context=0, right_context=0, num_layers=1, num_neurons=32, num_projects=16,
             num_targets=11, use_peepholes=True, dropout_rate=1.0)
_MODELS = {}


def _tiny_model(mode):
    from lstm_ctc_amd.nnet.model import Model
    if mode not in _MODELS:
        _MODELS[mode] = Model(dict(_TINY, compute_dtype=mode), "cuda", seed=1)
    return _MODELS[mode]


def _device_ratio(row, t, got):
    """error_ratio for the rows a CPU would take minutes over (the x3 / fp32 bound): float64 on the device."""
    assert row["mode"] != "bf16"
    A, B = t["A"].double(), t["B"].double()
    opA, opB = (A.t() if row["ta"] else A), (B.t() if row["tb"] else B)
    ref, mag = ALPHA * (opA @ opB), ALPHA * (opA.abs() @ opB.abs())
    if t["C0"] is not None:
        ref, mag = ref + t["beta"] * t["C0"].double(), mag + abs(t["beta"]) * t["C0"].double().abs()
    if t["bias"] is not None:
        ref, mag = ref + t["bias"].double(), mag + t["bias"].double().abs()
    lim = 3e-7 * max(1.0, np.sqrt(row["K"]) / 4) * mag
    assert bool((lim > 0).all())
    return float(((got.double() - ref).abs() / lim).max())


@pytest.mark.parametrize("row", ROUTES, ids=[r["id"] for r in ROUTES])
def test_route_on_the_device(ops, row, monkeypatch):
    from lstm_ctc_amd.nnet import model as model_mod
    t0 = time.perf_counter()
    monkeypatch.setattr(model_mod, "X3_FORCE", bool(row.get("force")))
    model = _tiny_model(row["mode"])
    assert (model.bf16, model.x3) == (row["mode"] == "bf16", row["mode"] == "bf16x3")
    monkeypatch.setattr(model, "use_shadows", model.bf16 and row.get("shadows", True))
    model._shadows.clear()
    spy = Spy(monkeypatch, real=True)
    t = operands(row, "cuda")
    got = call_mm(model, row, t)
    torch.cuda.synchronize()
    model._shadows.clear()
    c = check_route(row, t, spy)
    assert tuple(got.shape) == (row["M"], row["N"]) and got.dtype == torch.float32
    if t["out"] is not None:
        assert got is t["out"]
    else:
        assert got.is_contiguous()
    if is_big(row):
        ratio = _device_ratio(row, t, got)
    else:
        ref, mag = reference(row, t)
        ratio = error_ratio(row, got.cpu().numpy(), ref, mag)
    print("route %-8s %-30s error / bound %.4f  wall %.2f s" % (row["route"], row["id"], ratio, time.perf_counter() - t0))
    m = MEASURED.setdefault(row["route"], [0.0, 0])
    m[0], m[1] = max(m[0], ratio), m[1] + 1
    assert ratio < 1.0, (row["id"], ratio)
    if t["parent"] is not None:
        keep = torch.ones_like(t["parent"], dtype=torch.bool)
        (keep[8:8 + row["M"]] if row["out"] == "rows" else keep[:, 256:256 + row["N"]]).fill_(False)
        assert bool((t["parent"][keep] == SENTINEL).all()), "written outside the window"
    if row["route"] == "pad_tn":
        # the whole padded product against the reference of the zero-padded operand: what the pad columns meet is 0 exactly
        full = c["result"]
        if row["forms"][0] == "pad256":
            assert full.shape == (256, row["N"]) and torch.equal(full[:row["M"]], got) and not bool(full[row["M"]:].any())
        else:
            assert full.shape == (row["M"], 256) and torch.equal(full[:, :row["N"]], got) and not bool(full[:, row["N"]:].any())
    if t["shadow"] is not None:
        assert torch.equal(t["shadow"], got.to(BF16)), "the epilogue's shadow is the rounding of C"


# ------------------------------------------------------------------------------------------ (b), (c) whole steps
def _cfg(**kw):
    cfg = dict(nnet_type="blstm", input_dim=40, left_context=0, right_context=0, num_layers=2, num_neurons=256,
               num_projects=256, num_targets=44, use_peepholes=True, dropout_rate=1.0, compute_dtype="bf16")
    cfg.update(kw)
    return cfg


def _ragged(T, B, seed):
    seq = np.random.default_rng(seed).integers(T // 2, T + 1, size=B).astype(np.int32)
    seq[0] = T
    return seq


def _live(T, B, total):
    """B lengths <= T, the first one T, that add up to ``total`` live rows."""
    seq = np.full(B, T - 8, np.int32)
    seq[0] = T
    i = 1
    while seq.sum() != total:
        step = int(np.clip(total - seq.sum(), -(T // 2), 8))
        seq[i] += step
        i += 1
    assert seq.max() <= T and seq.min() >= T // 4 and seq.sum() == total
    return seq


_BIG_KERNELS = {"lc_gemm_bf16_tn", "lc_gemm_bf16_nn", "lc_gemm_bf16_nt2", "lc_gemm_bf16_nt"}
# name -> cfg, T, B, lengths, the getter kinds the step must use, the kernels it must run, X3_FORCE
CASES = {
    # 4096 rows: the smallest step on which the K >= 4096 padded route (input layer's dKx, head's weight gradient), the
    # K-major kernels on natural shadows (dKx of layer 1, dR, dproj, the forward products) and the two-segment dX all run
    "blstm_4096": dict(cfg=_cfg(), T=64, B=64, seq=_ragged(64, 64, 1), kinds={"nat", "tr", "pad256", "adopt"},
                       kernels=_BIG_KERNELS, pad=True),
    # a 300-wide head: neither narrow nor whole tiles - its weight gradient takes transposed shadows of 4096 rows
    "blstm_4096_wide_head": dict(cfg=_cfg(num_targets=300), T=64, B=64, seq=_ragged(64, 64, 2),
                                 kinds={"nat", "tr", "pad256", "adopt"}, kernels=_BIG_KERNELS, pad=True),
    # pack_frames with 4097 live rows (odd) and with 17 * 256: the bf16 modes have no packed operand form and run these on
    # the 72 * 64 padded rows (asserted) - the cases stand for the day they get one
    "blstm_packed_4097_live": dict(cfg=_cfg(pack_frames=True), T=72, B=64, seq=_live(72, 64, 4097),
                                   kinds={"nat", "tr", "pad256", "adopt"}, kernels=_BIG_KERNELS, pad=True),
    "blstm_packed_4352_live": dict(cfg=_cfg(pack_frames=True), T=72, B=64, seq=_live(72, 64, 4352),
                                   kinds={"nat", "tr", "pad256", "adopt"}, kernels=_BIG_KERNELS, pad=True),
    # 512 rows: the other model kinds' plumbing (two heads and accumulating dY; batch norm's in-place passes; the residual
    # sum into a layer output whose shadow must not have been taken before it)
    "blstm_moe_512": dict(cfg=_cfg(num_experts=4, moe_temp=10.0), T=8, B=64, seq=_ragged(8, 64, 3),
                          kinds={"nat", "tr", "adopt"}, kernels={"lc_gemm_bf16_nt", "lc_gemm_bf16_nn", "lc_gemm_bf16_tn"}),
    "lstm_bn_512": dict(cfg=_cfg(nnet_type="lstm", use_bn=True), T=8, B=64, seq=_ragged(8, 64, 4),
                        kinds={"nat", "tr", "adopt"}, kernels={"lc_gemm_bf16_nt", "lc_gemm_bf16_nn", "lc_gemm_bf16_tn"}),
    "blstm_residual_512": dict(cfg=_cfg(input_dim=512), T=8, B=64, seq=_ragged(8, 64, 5),
                               kinds={"nat", "tr", "adopt"}, kernels={"lc_gemm_bf16_nt", "lc_gemm_bf16_nn", "lc_gemm_bf16_tn"}),
    # dropout: the masks ride in the products' epilogues together with the shadows ((b) only: (c) has no mask emulation)
    "blstm_4096_dropout": dict(cfg=_cfg(dropout_rate=0.9), T=64, B=64, seq=_ragged(64, 64, 6),
                               kinds={"nat", "tr", "pad256", "adopt"}, kernels=None, pad=True),
    # bf16x3 with every product forced onto the split-operand kernels
    "x3_4096_forced": dict(cfg=_cfg(compute_dtype="bf16x3"), T=64, B=64, seq=_ragged(64, 64, 7), kinds={"x3"},
                           kernels={"lc_gemm_bf16x3_nt", "lc_gemm_bf16x3_tn"}, force=True),
}
PRODUCT_CASES = [c for c in sorted(CASES) if CASES[c]["kernels"] is not None]

_BF16_KERNELS = {"lc_gemm_bf16", "lc_gemm_bf16_nt", "lc_gemm_bf16_nt2", "lc_gemm_bf16_tn", "lc_gemm_bf16_nn"}
_F32_KERNELS = {"lc_gemm_f32", "lc_gemm_f32_nt2", "lc_gemm_bf16x3_nt", "lc_gemm_bf16x3_tn"}


def _x3_mismatches(src, s):
    """Elements at which the x3 shadow ``s`` is not the exact split of the fp32 matrix ``src`` - the statement of
    test_gpu_ops.py::test_split_bf16x3_is_exact: [row][k / 16][term][16], hi the RNE bf16 of x, mid of what hi left,
    hi + mid + lo == x exactly, pad columns zero; below 1e-30 the low terms flush and the sum is within 2^-125."""
    rows, K = src.shape
    Kp = (K + 15) // 16 * 16
    if tuple(s.shape) != (rows, 3 * Kp) or s.dtype != BF16:
        return -1
    v = s.reshape(rows, Kp // 16, 3, 16).float()
    hi, mid, lo = (v[:, :, i, :].reshape(rows, Kp) for i in range(3))
    bad = int((hi[:, K:] != 0).sum() + (mid[:, K:] != 0).sum() + (lo[:, K:] != 0).sum())
    hi, mid, lo = hi[:, :K], mid[:, :K], lo[:, :K]
    hi_ref = src.to(BF16).float()
    mid_ref = (src - hi_ref).to(BF16).float()
    diff = (hi.double() + mid.double() + lo.double() - src.double()).abs()
    normal = (src.abs() > 1e-30) | (src == 0)
    wrong = (hi != hi_ref) | (normal & ((mid != mid_ref) | (diff != 0))) | (~normal & (diff >= 2.0 ** -125))
    return bad + int(wrong.sum())


class _Watch:
    """The wrappers of one step: counts per getter kind, products recorded and checked, failures as text."""

    def __init__(self, ops, mp, products):
        from lstm_ctc_amd.nnet.model import Model
        self.ops = ops
        self.counts, self.failures = collections.Counter(), []
        self.recorded = self.checked = self.nt2_funnel = self.ep_shadows = 0
        self.kernels = collections.Counter()
        self.worst = {}                       # kernel -> [error / bound, error / ((K + 3) 2^-24 magnitudes) or None]
        self.pad_ids, self.tn_pad, self.tn_nat = set(), 0, 0
        watch = self
        o_shadow, o_shadow3, o_pad, o_adopt = Model._shadow, Model._shadow3, Model._shadow_pad256, Model._adopt_shadow

        def _shadow(self, t, tr):
            s = o_shadow(self, t, tr)
            rows, C = t.shape
            if tr:
                ok = (tuple(s.shape) == (C, (rows + 7) // 8 * 8) and torch.equal(s[:, :rows], t.t().to(BF16))
                      and not bool(s[:, rows:].any()))
            else:
                ok = s.shape == t.shape and torch.equal(s, t.to(BF16))
            watch.note("tr" if tr else "nat", ok, t, s)
            return s

        def _shadow3(self, t, tr=False):
            s = o_shadow3(self, t, tr)
            n = _x3_mismatches(t.t().contiguous() if tr else t, s)
            watch.note("x3", n == 0, t, s, "%d elements, tr=%s" % (n, tr))
            return s

        def _shadow_pad256(self, t):
            s = o_pad(self, t)
            C = t.shape[1]
            ok = (tuple(s.shape) == (t.shape[0], 256) and torch.equal(s[:, :C], t.to(BF16)) and not bool(s[:, C:].any()))
            watch.note("pad256", ok, t, s)
            watch.pad_ids.add(id(s))
            return s

        def _adopt_shadow(self, t, shadow):
            ok = shadow.dtype == BF16 and shadow.shape == t.shape and torch.equal(shadow, t.to(BF16))
            watch.note("adopt", ok, t, shadow)
            return o_adopt(self, t, shadow)

        for name, fn in (("_shadow", _shadow), ("_shadow3", _shadow3), ("_shadow_pad256", _shadow_pad256),
                         ("_adopt_shadow", _adopt_shadow)):
            mp.setattr(Model, name, fn)
        if products:
            o_product, o_nt2 = ops._product, ops._product_nt2

            def _product_nt2(*a, **kw):
                watch.nt2_funnel += 1
                return o_nt2(*a, **kw)

            def _product(name, kind, head, M, N, Ks, A, B, out, alpha, beta, bias, epilogue=None, **kw):
                watch.recorded += 1
                watch.kernels[name] += 1
                A0, B0 = tuple(a.clone() for a in A), tuple(b.clone() for b in B)
                out0 = out.clone() if out is not None and beta != 0.0 else None
                bias0 = bias.clone() if bias is not None else None
                if name == "lc_gemm_bf16_tn":
                    padded = any(id(x) in watch.pad_ids for x in A + B)
                    watch.tn_pad, watch.tn_nat = watch.tn_pad + padded, watch.tn_nat + (not padded)
                res = o_product(name, kind, head, M, N, Ks, A, B, out, alpha, beta, bias, epilogue, **kw)
                watch.check_product(name, head, M, N, Ks, A0, B0, out0, alpha, beta, bias0, epilogue, res)
                return res

            mp.setattr(ops, "_product", _product)
            mp.setattr(ops, "_product_nt2", _product_nt2)

    def note(self, kind, ok, t, s, what=""):
        self.counts[kind] += 1
        if not ok and len(self.failures) < 20:
            if kind in ("nat", "adopt") and s.shape == t.shape:
                what = "%d elements differ" % int((s != t.to(BF16)).sum())
            self.failures.append("%s shadow #%d of %s stride %s is not the rounding of its source (%s)"
                                 % (kind, self.counts[kind], tuple(t.shape), t.stride(), what))

    def check_product(self, name, head, M, N, Ks, A, B, out0, alpha, beta, bias, epilogue, res):
        K = sum(Ks)
        f64 = lambda x: x.double()
        if name in ("lc_gemm_f32", "lc_gemm_bf16"):
            rnd = (lambda x: x.to(BF16).double()) if name == "lc_gemm_bf16" else f64
            a, b = rnd(A[0]), rnd(B[0])
            pairs = [(a.t() if head[0] else a, b.t() if head[1] else b)]
        elif name in ("lc_gemm_bf16_nt", "lc_gemm_bf16_nt2", "lc_gemm_f32_nt2"):
            pairs = [(f64(a[:, :k]), f64(b[:, :k]).t()) for a, b, k in zip(A, B, Ks)]
        elif name == "lc_gemm_bf16_tn":
            pairs = [(f64(A[0]).t(), f64(B[0]))]
        elif name == "lc_gemm_bf16_nn":
            pairs = [(f64(A[0]), f64(B[0]))]
        elif name == "lc_gemm_bf16x3_nt":
            pairs = [(unsplit_x3(A[0], K), unsplit_x3(B[0], K).t())]
        elif name == "lc_gemm_bf16x3_tn":
            pairs = [(unsplit_x3(A[0], M).t(), unsplit_x3(B[0], N))]
        else:
            self.failures.append("a product nobody knows: %s" % name)
            return
        if any(p.shape != (M, k) or q.shape != (k, N) for (p, q), k in zip(pairs, Ks)) or tuple(res.shape) != (M, N):
            self.failures.append("%s: operand shapes do not give [%d, %d] over K = %s" % (name, M, N, Ks))
            return
        ref = alpha * sum(p @ q for p, q in pairs)
        mag = abs(alpha) * sum(p.abs() @ q.abs() for p, q in pairs)
        if out0 is not None:
            ref, mag = ref + beta * out0.double(), mag + abs(beta) * out0.double().abs()
        if bias is not None:
            ref, mag = ref + bias.double(), mag + bias.double().abs()
        err = (res.double() - ref).abs()

        def over(lim):                       # largest err / lim; an error where the limit is zero counts as infinite
            return float(torch.where(lim > 0, err / lim.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0)).max())

        grade = over(3e-7 * max(1.0, np.sqrt(K) / 4) * mag)
        if name in _BF16_KERNELS:
            ratio, second = float(err.max()) / (abs(alpha) * 2e-6 * K * 4 + 1e-5), over((K + 3) * 2.0 ** -24 * mag)
            ok = ratio < 1.0 and second <= 1.0
        else:
            assert name in _F32_KERNELS
            ratio, second = grade, None
            ok = ratio < 1.0
        w = self.worst.setdefault(name, [0.0, 0.0, 0.0])
        w[0], w[1], w[2] = max(w[0], ratio), max(w[1], second or 0.0), max(w[2], grade)
        if not ok and len(self.failures) < 20:
            self.failures.append("%s product #%d [%d, %d] K = %s alpha %g beta %g: error / bound %.3g (%s)"
                                 % (name, self.recorded, M, N, Ks, alpha, beta, ratio, second))
        if epilogue is not None:
            if epilogue.keep != 1.0 or epilogue.shadow_only:
                self.failures.append("%s: an epilogue that changes C in a step without dropout" % name)
            elif epilogue.shadow is not None:
                self.ep_shadows += 1
                if not torch.equal(epilogue.shadow, res.to(BF16)):
                    self.failures.append("%s product #%d: the epilogue's shadow is not the rounding of C" % (name, self.recorded))
        self.checked += 1


_RUNS = {}


def _run(ops, name):
    """One training step (forward, lc_ctc_loss, backward) of a case under the wrappers; run once, shared by (b) and (c)."""
    if name in _RUNS:
        return _RUNS[name]
    from lstm_ctc_amd.nnet import model as model_mod
    from lstm_ctc_amd.nnet.model import Model
    case = CASES[name]
    cfg, T, B = case["cfg"], case["T"], case["B"]
    t0 = time.perf_counter()
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("LC_C5_SHADOW_ONLY", "0")          # every fp32 source exists (=1: test_gpu_round6.py, bit identity)
        mp.delenv("LC_PACK_FRAMES", raising=False)
        mp.setattr(model_mod, "X3_FORCE", bool(case.get("force")))
        model = Model(cfg, "cuda", seed=3)
        assert not model.shadow_only and not model.pack_frames
        assert model.keep == cfg["dropout_rate"]
        g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
        x = torch.randn(T, B, cfg["input_dim"], generator=g).cuda()
        seq = torch.from_numpy(case["seq"]).cuda()
        L = 6 if T >= 16 else 2
        labels = torch.randint(0, cfg["num_targets"] - 1, (B * L,), generator=g, dtype=torch.int32).cuda()
        offs = (torch.arange(B + 1) * L).to(torch.int32).cuda()
        watch = _Watch(ops, mp, products=case["kernels"] is not None)
        logits = model.forward(x, seq, drop_seed=7)
        assert not model.packed
        loss, grad = ops.ctc_loss(logits, labels, offs, seq, L)
        model.backward(grad)
        torch.cuda.synchronize()
        assert int(ops.lstm_status("cuda").item()) == 0
        assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(model.ps.grad).all()) and float(model.ps.grad.abs().max()) > 0
    watch.wall = time.perf_counter() - t0
    _RUNS[name] = watch
    return watch


@pytest.mark.parametrize("case", sorted(CASES))
def test_shadows_are_fresh(ops, case):
    """(b): each getter kind the case uses fired, and every shadow it handed out or registered was exact."""
    w = _run(ops, case)
    print("shadows %-24s %s  step under the wrappers %.2f s" % (case, dict(w.counts), w.wall))
    assert not [f for f in w.failures if " shadow #" in f], w.failures
    assert {k for k, n in w.counts.items() if n > 0} == CASES[case]["kinds"], dict(w.counts)
    assert sum(w.counts.values()) > 0


def test_the_wrappers_see_a_stale_or_misplaced_shadow(ops):
    """(b) can fail: a source changed by one part in 64 after its cast (two bf16 ulps: a stale cache hit), the shadow of the
    neighbouring column window adopted, a value left in a pad column, a low term of a split dropped - each is reported;
    the same calls on untouched tensors are not."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(_tiny_model("bf16"), "use_shadows", True)
        for mode in ("bf16", "bf16x3"):
            _tiny_model(mode)._shadows.clear()
        w = _Watch(ops, mp, products=True)
        m, m3 = _tiny_model("bf16"), _tiny_model("bf16x3")
        g = torch.Generator().manual_seed(5)
        buf = torch.randn(4096, 80, generator=g).cuda()
        W = torch.randn(4096, 256, generator=g).cuda()
        x = buf[:, :40]
        m._mm(x, W, ta=True)                                   # padded shadow of x, natural of W
        m._mm(x, W[:, :136], ta=True)                          # transposed ones
        m._adopt_shadow(buf[:, 40:], buf[:, 40:].to(BF16))
        m._mm(buf[:, 40:], W[:, :136], ta=True)
        s3 = m3._shadow3(W)
        assert not w.failures and w.checked == w.recorded == 3
        assert {k: n for k, n in w.counts.items()} == {"pad256": 1, "nat": 1, "tr": 4, "adopt": 1, "x3": 1}
        x.mul_(1.0 + 2.0 ** -6)
        m._mm(x, W, ta=True)                                   # stale padded shadow (W's is still right)
        assert len(w.failures) == 1 and w.failures[0].startswith("pad256 shadow #2")
        m._mm(x, W[:, :136], ta=True)                          # stale transposed shadow
        assert len(w.failures) == 2 and w.failures[1].startswith("tr shadow #5")
        m._adopt_shadow(buf[:, :40], buf[:, 40:].to(BF16))     # the other half's shadow
        assert len(w.failures) == 3 and w.failures[2].startswith("adopt shadow #2")
        m._shadows.clear()
        m._shadow_pad256(x)[7, 200] = 1.0
        m._shadow_pad256(x)                                    # the cached buffer again, with a value in a pad column
        assert len(w.failures) == 4 and w.failures[3].startswith("pad256 shadow #4")
        s3.view(4096, 16, 3, 16)[:, :, 2, :] = 0               # hi + mid alone: a 16-bit split
        m3._shadow3(W)
        assert len(w.failures) == 5 and w.failures[4].startswith("x3 shadow #2")
        assert w.checked == w.recorded == 5                    # the products themselves were right on what they were given
        m._shadows.clear()
        m3._shadows.clear()


@pytest.mark.parametrize("case", PRODUCT_CASES)
def test_every_product_of_the_step(ops, case):
    """(c): every product call of the step was checked, on the kernels the case is there for."""
    w = _run(ops, case)
    for k in sorted(w.worst):
        print("products %-24s %-18s x %-3d error / bound %.4f  / (K+3) 2^-24 magnitudes %.4f  / fp32 grade %.4f"
              % (case, k, w.kernels[k], *w.worst[k]))
    print("products %-24s checked %d of %d, %d epilogue shadows, tn on padded / natural operands %d / %d"
          % (case, w.checked, w.recorded, w.ep_shadows, w.tn_pad, w.tn_nat))
    assert w.recorded > 0 and w.checked == w.recorded, (w.checked, w.recorded)
    assert not w.failures, w.failures
    assert set(w.kernels) >= CASES[case]["kernels"], dict(w.kernels)
    assert set(w.kernels) <= _BF16_KERNELS | _F32_KERNELS
    assert w.nt2_funnel == w.kernels["lc_gemm_bf16_nt2"] + w.kernels["lc_gemm_f32_nt2"]
    if CASES[case].get("pad"):
        # layer 0's two dKx and the head's weight gradient (a 300-wide head: the layer's alone) on the padded shadows;
        # layer 1's dKx, dR and dproj on the natural ones
        assert w.tn_pad >= 2 and w.tn_nat >= 6, (w.tn_pad, w.tn_nat)
        assert w.ep_shadows > 0


# ----------------------------------------------------------------------------------------------- report
def test_zz_report_measured_ratios():
    from test_bf16_routes_host import ROUTE_FN
    lines = ["# Model._mm's routes and the steps around them, tests/test_gpu_bf16_routes.py: largest measured error / bound",
             "# bound: bf16 routes and kernels |alpha| * 2e-6 * K * 4 + 1e-5; x3 and fp32 ones error / sum of magnitudes over",
             "# 3e-7 max(1, sqrt(K) / 4).  second: bf16 kernels in a step, error over (K + 3) 2^-24 sums of magnitudes",
             "# (a) per route, over its ROUTES rows"]
    lines += ["route %-7s rows %2d  error / bound %.4f" % (k, v[1], v[0]) for k, v in sorted(MEASURED.items())]
    lines.append("# (b) per step, shadows checked bit for bit per getter kind; (c) products checked / recorded, per kernel")
    for case in sorted(_RUNS):
        w = _RUNS[case]
        lines.append("step %-24s shadows %s" % (case, " ".join("%s %d" % kv for kv in sorted(w.counts.items()))))
        if CASES[case]["kernels"] is not None:
            lines.append("step %-24s products %d / %d, epilogue shadows %d" % (case, w.checked, w.recorded, w.ep_shadows))
            lines += ["step %-24s %-18s x %-3d error / bound %.4f  second %.4f" % (case, k, w.kernels[k], *w.worst[k][:2])
                      for k in sorted(w.worst)]
    lines.append("# wall time per test, seconds (a step is run by the first test that needs it); the file: %.1f"
                 % sum(WALL.values()))
    lines += ["wall %-70s %.3f" % kv for kv in sorted(WALL.items())]
    print("\n" + "\n".join(lines))
    out = os.environ.get("LC_MEASURED_DIR")              # where to keep the table; unset: printed only
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "bf16_route_tests.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
    assert MEASURED and set(MEASURED) <= set(ROUTE_FN) and all(v[0] < 1.0 for v in MEASURED.values())
    assert _RUNS and all(sum(w.counts.values()) > 0 for w in _RUNS.values())
