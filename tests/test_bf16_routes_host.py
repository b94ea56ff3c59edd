"""The product router of the bf16 / bf16x3 modes (`Model._mm`, lstm_ctc_amd/nnet/model.py), pinned without a GPU.

`_mm` decides from shapes, strides, `beta`, `bias`, `epilogue` and `K >= 4096` which of eight kernels a product with an
activation operand runs on, and in which form (natural / transposed / zero-padded 256-column bf16 shadow, x3 shadow, fp32
as it lies) each operand reaches it.  ROUTES below is the one table of that decision, in the order `_mm` tests its
conditions, at the smallest shapes at which each route is still (or just no longer) taken; tests/test_gpu_bf16_routes.py
imports it and runs every row on the device.

Here a bare `Model` (object.__new__, the four attributes `_mm` reads) is driven through the table with the ops entry points
replaced by CPU stand-ins (`Spy`) that record the call and compute what the kernel would: each row asserts the product
function called, the operand forms it received, the arguments handed through, and - the plumbing around the kernels: the
valid block of a padded product, `out` windows - the value against float64.  The last tests prove that the bounds the two
files assert can fail: a dropped k index, two swapped operand rows and a non-zero pad column each exceed them.
"""
import zlib

import numpy as np
import pytest
import torch

from lstm_ctc_amd import ops
from lstm_ctc_amd.nnet import model as model_mod
from lstm_ctc_amd.nnet.model import Model
from oracle.oracle import bf16_round

ALPHA = 0.5
SENTINEL = 12345.0
BIG = 2e9             # M * N * K above which a row is not computed on the CPU (the two stand-alone x3 products)


def _row(id, mode, route, forms, M, N, K, ta=False, tb=False, **kw):
    """mode: compute_dtype of the model; route: see ROUTE_FN; forms: the form of (A, B) at the product - nat / tr / pad256
    (bf16 shadows), x3 / x3tr (x3 shadow of the matrix / of its transpose), f32 (the fp32 view as passed).
    A is stored [K, M] where ta, B [N, K] where tb.  Options: a_win / b_win = (extra columns of the parent buffer, column
    offset of the window in it); out = "rows" (contiguous row window of a taller buffer) / "cols" (strided column window of a
    wider one); beta; bias; ep (an epilogue that writes the bf16 shadow of C); x3_ok; force (model.X3_FORCE); shadows."""
    return dict(id=id, mode=mode, route=route, forms=forms, M=M, N=N, K=K, ta=ta, tb=tb, **kw)


# route -> (ops function, its bf16 flag where the function is ops.gemm)
ROUTE_FN = {"x3_nt": ("gemm_bf16x3_nt", None), "x3_tn": ("gemm_bf16x3_tn", None), "f32": ("gemm", False),
            "tn": ("gemm_bf16_tn", None), "pad_tn": ("gemm_bf16_tn", None), "nn": ("gemm_bf16_nn", None),
            "nt": ("gemm_bf16_nt", None), "conv": ("gemm", True)}

ROUTES = [
    # ---- bf16x3, X3_FORCE off: the two split-operand kernels where they pay (_x3_pays), the fp32 kernels elsewhere
    _row("x3_nt_8192x1024x1216", "bf16x3", "x3_nt", ("x3", "x3tr"), 8192, 1024, 1216),
    _row("x3_nt_8192x1024x1216_tb", "bf16x3", "x3_nt", ("x3", "x3"), 8192, 1024, 1216, tb=True),
    _row("x3_nt_k1152_too_small", "bf16x3", "f32", ("f32", "f32"), 8192, 1024, 1152),                 # 2MNK < 2e10
    _row("x3_tn_4096x2048x4096", "bf16x3", "x3_tn", ("x3", "x3"), 2048, 4096, 4096, ta=True),
    _row("x3_tn_k4088_too_short", "bf16x3", "f32", ("f32", "f32"), 2048, 4096, 4088, ta=True),       # < 256 tiles: K >= 4096
    _row("x3_tn_not_ok", "bf16x3", "f32", ("f32", "f32"), 2048, 4096, 4096, ta=True, x3_ok=False),
    _row("x3_tn_epilogue", "bf16x3", "f32", ("f32", "f32"), 2048, 4096, 4096, ta=True, ep=True),
    # (X3_FORCE on, as the parity tests run the mode: the same two routes at shapes a CPU multiplies in no time)
    _row("x3_nt_forced_300x200x100", "bf16x3", "x3_nt", ("x3", "x3tr"), 300, 200, 100, force=True, bias=True),
    _row("x3_nt_forced_tb_window", "bf16x3", "x3_nt", ("x3", "x3"), 300, 200, 100, tb=True, force=True, a_win=(100, 100),
         beta=1.0),
    _row("x3_tn_forced_1000x300x520", "bf16x3", "x3_tn", ("x3", "x3"), 300, 520, 1000, ta=True, force=True, out="rows"),
    # ---- fp32 mode: any shape -> ops.gemm
    _row("f32_nn", "fp32", "f32", ("f32", "f32"), 256, 256, 64, bias=True),
    _row("f32_ta_narrow", "fp32", "f32", ("f32", "f32"), 40, 512, 4096, ta=True, out="rows"),
    _row("f32_tb", "fp32", "f32", ("f32", "f32"), 130, 70, 33, tb=True, beta=1.0, out="cols"),
    # ---- bf16, ta: X^T dZ.  Whole 256-tiles on both sides and 16-byte rows -> the K-major kernel on the natural shadows
    _row("ta_tn_520x256x512", "bf16", "tn", ("nat", "nat"), 256, 512, 520, ta=True),
    _row("ta_tn_strided_windows", "bf16", "tn", ("nat", "nat"), 256, 512, 520, ta=True, a_win=(256, 256), b_win=(8, 8),
         beta=1.0, bias=True, out="rows"),
    _row("ta_nt_n264", "bf16", "nt", ("tr", "tr"), 256, 264, 520, ta=True),                           # 256 < N, N % 256 != 0
    _row("ta_conv_k4100_n264", "bf16", "conv", ("f32", "f32"), 256, 264, 4100, ta=True),              # ... and K % 8 != 0
    _row("ta_window_stride_260", "bf16", "nt", ("tr", "tr"), 256, 512, 520, ta=True, a_win=(4, 4)),   # stride(0) % 8 != 0
    # ---- bf16, ta, ONE narrow side and K >= 4096: the K-major kernel on a zero-padded 256-column shadow
    _row("pad_40x512", "bf16", "pad_tn", ("pad256", "nat"), 40, 512, 4096, ta=True),
    _row("pad_512x44", "bf16", "pad_tn", ("nat", "pad256"), 512, 44, 4096, ta=True),
    _row("pad_255x256", "bf16", "pad_tn", ("pad256", "nat"), 255, 256, 4096, ta=True),
    _row("pad_1x256", "bf16", "pad_tn", ("pad256", "nat"), 1, 256, 4096, ta=True),
    _row("pad_k4100", "bf16", "pad_tn", ("pad256", "nat"), 40, 512, 4100, ta=True),                   # K % 8 != 0
    _row("pad_k4097_odd_wide_window", "bf16", "pad_tn", ("nat", "pad256"), 256, 44, 4097, ta=True, a_win=(256, 256)),
    _row("pad_k4088_too_short", "bf16", "nt", ("tr", "tr"), 40, 512, 4088, ta=True),
    _row("pad_k4095_too_short", "bf16", "conv", ("f32", "f32"), 40, 512, 4095, ta=True),
    _row("pad_both_narrow", "bf16", "nt", ("tr", "tr"), 40, 44, 4096, ta=True),
    _row("pad_not_with_beta", "bf16", "nt", ("tr", "tr"), 40, 512, 4096, ta=True, beta=1.0, out="rows"),
    _row("pad_not_with_bias", "bf16", "nt", ("tr", "tr"), 40, 512, 4096, ta=True, bias=True),
    _row("pad_not_with_epilogue", "bf16", "nt", ("tr", "tr"), 40, 512, 4096, ta=True, ep=True),
    _row("pad_out_row_window", "bf16", "pad_tn", ("pad256", "nat"), 40, 512, 4096, ta=True, out="rows"),
    _row("pad_out_strided", "bf16", "pad_tn", ("nat", "pad256"), 512, 44, 4096, ta=True, out="cols"),
    # ---- bf16, neither transposed: X . W.  Whole 256-tiles, K in 64s -> activation and weight in their natural layouts
    _row("nn_256x256x64", "bf16", "nn", ("nat", "nat"), 256, 256, 64),
    _row("nn_windows_out_half", "bf16", "nn", ("nat", "nat"), 256, 256, 64, a_win=(64, 64), b_win=(256, 256), out="cols",
         bias=True, ep=True),
    _row("nn_k72", "bf16", "nt", ("nat", "tr"), 256, 256, 72),
    _row("nn_m264", "bf16", "nt", ("nat", "tr"), 264, 256, 64),
    _row("nn_n264", "bf16", "nt", ("nat", "tr"), 256, 264, 64),
    _row("nn_window_stride_68", "bf16", "nt", ("nat", "tr"), 256, 256, 64, a_win=(4, 4)),             # stride(0) % 8 != 0
    _row("nn_k60", "bf16", "conv", ("f32", "f32"), 256, 256, 60),
    _row("nn_k8", "bf16", "nt", ("nat", "tr"), 256, 256, 8),
    _row("nn_k7", "bf16", "conv", ("f32", "f32"), 256, 256, 7),
    # ---- bf16, what is left with K in 8s -> the NT kernel (k contiguous in both shadows), else the converting loader
    _row("tb_half_window", "bf16", "nt", ("nat", "nat"), 512, 256, 256, tb=True, a_win=(256, 256)),   # dh = dY[:, half] . proj^T
    _row("tb_head_k44", "bf16", "conv", ("f32", "f32"), 512, 512, 44, tb=True, ep=True),              # dY = dlogits . W^T
    _row("shadows_off", "bf16", "conv", ("f32", "f32"), 256, 256, 64, shadows=False),
]


def is_big(row):
    return float(row["M"]) * row["N"] * row["K"] > BIG


def operands(row, device="cpu"):
    """The tensors of one ROUTES row (the same values on every device): N(0, 1), non-symmetric; views as the row says."""
    g = torch.Generator().manual_seed(zlib.crc32(row["id"].encode()))
    M, N, K = row["M"], row["N"], row["K"]

    def window(shape, win):
        pad, off = win
        buf = torch.randn(shape[0], shape[1] + pad, generator=g).to(device)
        return buf[:, off:off + shape[1]]

    A = window((K, M) if row["ta"] else (M, K), row.get("a_win", (0, 0)))
    B = window((N, K) if row["tb"] else (K, N), row.get("b_win", (0, 0)))
    C0 = torch.randn(M, N, generator=g).to(device)
    bias = torch.randn(N, generator=g).to(device) if row.get("bias") else None
    beta = float(row.get("beta", 0.0))
    parent = out = None
    if row.get("out") == "rows":
        parent = torch.full((M + 16, N), SENTINEL, device=device)
        out = parent[8:8 + M]
    elif row.get("out") == "cols":
        parent = torch.full((M, N + 264), SENTINEL, device=device)
        out = parent[:, 256:256 + N]
    elif beta != 0.0:
        out = torch.empty(M, N, device=device)
    if out is not None and beta != 0.0:
        out.copy_(C0)
    shadow = torch.zeros(M, N, dtype=torch.bfloat16, device=device) if row.get("ep") else None
    ep = ops.Epilogue(1.0, 0, 0, 1, shadow) if row.get("ep") else None
    return dict(A=A, B=B, C0=C0 if beta != 0.0 else None, bias=bias, beta=beta, out=out, parent=parent, ep=ep, shadow=shadow)


def rounded(row, t):
    """A float32 host array as the row's route rounds it on load: to bf16 in bf16 mode, not at all in the other two."""
    a = np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32)
    return (bf16_round(a) if row["mode"] == "bf16" else a).astype(np.float64)


def reference(row, t, A=None, B=None):
    """(float64 result, its sum of magnitudes) of the row's product on the operands as the kernel rounds them."""
    A = rounded(row, t["A"]) if A is None else A
    B = rounded(row, t["B"]) if B is None else B
    opA, opB = (A.T if row["ta"] else A), (B.T if row["tb"] else B)
    ref, mag = ALPHA * (opA @ opB), ALPHA * (np.abs(opA) @ np.abs(opB))
    if t["C0"] is not None:
        c0 = t["C0"].cpu().numpy().astype(np.float64)
        ref, mag = ref + t["beta"] * c0, mag + abs(t["beta"]) * np.abs(c0)
    if t["bias"] is not None:
        b = t["bias"].cpu().numpy().astype(np.float64)
        ref, mag = ref + b, mag + np.abs(b)
    return ref, mag


def error_ratio(row, got, ref, mag):
    """Largest error over its bound (< 1 passes).  The project's own bounds: bf16 routes |alpha| * 2e-6 * K * 4 + 1e-5
    absolute (test_gpu_ops.py::test_gemm_bf16_tn_on_natural_shadows); x3 and fp32 routes the error over the sum of magnitudes
    below 3e-7 * max(1, sqrt(K) / 4) (test_gemm_bf16x3_is_fp32_grade)."""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    if row["mode"] == "bf16":
        return float(err.max() / (abs(ALPHA) * 2e-6 * row["K"] * 4 + 1e-5))
    lim = 3e-7 * max(1.0, np.sqrt(row["K"]) / 4) * mag
    return float(np.where(lim > 0, err / np.where(lim > 0, lim, 1.0), np.where(err > 0, np.inf, 0.0)).max())


def split_x3(x):
    """lc_split_bf16x3 restated: [rows, K] f32 -> [rows, 3 * roundup(K, 16)] bf16, laid out [row][k / 16][term][16]."""
    rows, K = x.shape
    Kp = (K + 15) // 16 * 16
    xp = torch.zeros(rows, Kp, dtype=torch.float32, device=x.device)
    xp[:, :K] = x
    hi = xp.to(torch.bfloat16)
    r1 = xp - hi.float()
    mid = r1.to(torch.bfloat16)
    lo = (r1 - mid.float()).to(torch.bfloat16)
    return torch.stack([p.view(rows, Kp // 16, 16) for p in (hi, mid, lo)], dim=2).reshape(rows, 3 * Kp)


def unsplit_x3(s, cols):
    """The float64 sum of the three terms of the first ``cols`` columns of an x3 shadow (or of a row window of one)."""
    rows = s.shape[0]
    return s.reshape(rows, -1, 3, 16).double().sum(dim=2).reshape(rows, -1)[:, :cols]


class Spy:
    """Puts recorders in front of the ops entry points `_mm` uses.  real = False: CPU stand-ins that compute what the kernels
    would (compute = False: zeros of the right shape); real = True: the recorders call through.  Every shadow a cast / split
    returns is tagged with its form and the fp32 tensor it was made from; a product call records the forms it received."""
    PRODUCTS = ("gemm", "gemm_bf16_nt", "gemm_bf16_tn", "gemm_bf16_nn", "gemm_bf16x3_nt", "gemm_bf16x3_tn")
    CASTS = ("cast_bf16", "split_bf16x3", "transpose")

    def __init__(self, monkeypatch, real=False, compute=True):
        self.real, self.compute = real, compute
        self.calls, self.casts, self._forms, self._keep = [], [], {}, []
        self.orig = {n: getattr(ops, n) for n in self.PRODUCTS + self.CASTS}
        for n in self.PRODUCTS + self.CASTS:
            monkeypatch.setattr(ops, n, getattr(self, "_" + n))

    # ---- forms
    def tag(self, t, form, src):
        self._forms[id(t)] = (form, src)
        self._keep.append(t)                     # (alive: its id cannot be handed to another tensor)
        return t

    def form(self, t):
        return self._forms.get(id(t), ("f32", t))

    # ---- casts
    def _cast_bf16(self, x, nat=True, tr=False, out_nat=None):
        self.casts.append("cast_bf16")
        if self.real:
            n, t = self.orig["cast_bf16"](x, nat=nat, tr=tr, out_nat=out_nat)
        else:
            n = t = None
            rows, C = x.shape
            if out_nat is not None:
                out_nat[:, :C] = x.to(torch.bfloat16)
                n = out_nat
            elif nat:
                n = x.to(torch.bfloat16)
            if tr:
                t = torch.zeros((C, (rows + 7) // 8 * 8), dtype=torch.bfloat16)
                t[:, :rows] = x.t().to(torch.bfloat16)
        if n is not None:
            self.tag(n, "pad256" if out_nat is not None else "nat", x)
        if t is not None:
            self.tag(t, "tr", x)
        return n, t

    def _transpose(self, x):
        self.casts.append("transpose")
        return self.tag(self.orig["transpose"](x) if self.real else x.t().contiguous(), "T", x)

    def _split_bf16x3(self, x):
        self.casts.append("split_bf16x3")
        form, src = self.form(x)
        return self.tag(self.orig["split_bf16x3"](x) if self.real else split_x3(x), "x3tr" if form == "T" else "x3", src)

    # ---- products
    def _finish(self, name, A, B, P, shape, out, alpha, beta, bias, epilogue, **extra):
        """P: a function giving the float64 product of the operands as handed over (CPU stand-in only)."""
        rec = dict(name=name, forms=(self.form(A)[0], self.form(B)[0]), srcs=(self.form(A)[1], self.form(B)[1]), A=A, B=B,
                   out=out, alpha=alpha, beta=beta, bias=bias, epilogue=epilogue, **extra)
        self.calls.append(rec)
        if self.real:
            kw = {k: v for k, v in extra.items() if k in ("ta", "tb", "bf16", "K")}
            pos = [extra[k] for k in ("K3", "M3", "N3") if k in extra]
            if name != "gemm_bf16x3_tn":
                kw["epilogue"] = epilogue
            rec["result"] = self.orig[name](A, B, *pos, out=out, alpha=alpha, beta=beta, bias=bias, **kw)
            return rec["result"]
        if self.compute:
            res = alpha * P()
            if beta != 0.0:
                res = res + beta * out.double()
            if bias is not None:
                res = res + bias.double()
            res = res.float()
        else:
            res = torch.zeros(shape)
        assert tuple(res.shape) == tuple(shape)
        if epilogue is not None and epilogue.shadow is not None:
            epilogue.shadow.copy_(res.to(torch.bfloat16))
        if out is None:
            out = res
        else:
            out.copy_(res)
        rec["result"] = out
        return out

    def _gemm(self, A, B, ta=False, tb=False, out=None, alpha=1.0, beta=0.0, bias=None, bf16=False, epilogue=None):
        M, K = (A.shape[1], A.shape[0]) if ta else tuple(A.shape)
        N = B.shape[0] if tb else B.shape[1]
        rnd = (lambda t: t.to(torch.bfloat16).double()) if bf16 else (lambda t: t.double())
        return self._finish("gemm", A, B, lambda: (rnd(A).t() if ta else rnd(A)) @ (rnd(B).t() if tb else rnd(B)), (M, N), out,
                            alpha, beta, bias, epilogue, ta=ta, tb=tb, bf16=bf16)

    def _gemm_bf16_nt(self, A, B, out=None, alpha=1.0, beta=0.0, bias=None, K=None, epilogue=None):
        assert A.dtype == B.dtype == torch.bfloat16
        k = A.shape[1] if K is None else K
        return self._finish("gemm_bf16_nt", A, B, lambda: A[:, :k].double() @ B[:, :k].double().t(), (A.shape[0], B.shape[0]),
                            out, alpha, beta, bias, epilogue, K=K)

    def _gemm_bf16_tn(self, A, B, out=None, alpha=1.0, beta=0.0, bias=None, epilogue=None):
        assert A.dtype == B.dtype == torch.bfloat16 and A.shape[0] == B.shape[0]
        return self._finish("gemm_bf16_tn", A, B, lambda: A.double().t() @ B.double(), (A.shape[1], B.shape[1]), out, alpha, beta,
                            bias, epilogue)

    def _gemm_bf16_nn(self, A, B, out=None, alpha=1.0, beta=0.0, bias=None, epilogue=None):
        assert A.dtype == B.dtype == torch.bfloat16 and A.shape[1] == B.shape[0]
        return self._finish("gemm_bf16_nn", A, B, lambda: A.double() @ B.double(), (A.shape[0], B.shape[1]), out, alpha, beta, bias,
                            epilogue)

    def _gemm_bf16x3_nt(self, A3, B3, K, out=None, alpha=1.0, beta=0.0, bias=None, epilogue=None):
        assert A3.dtype == B3.dtype == torch.bfloat16
        return self._finish("gemm_bf16x3_nt", A3, B3, lambda: unsplit_x3(A3, K) @ unsplit_x3(B3, K).t(),
                            (A3.shape[0], B3.shape[0]), out, alpha, beta, bias, epilogue, K3=K)

    def _gemm_bf16x3_tn(self, A3, B3, M, N, out=None, alpha=1.0, beta=0.0, bias=None):
        assert A3.dtype == B3.dtype == torch.bfloat16 and A3.shape[0] == B3.shape[0]
        return self._finish("gemm_bf16x3_tn", A3, B3, lambda: unsplit_x3(A3, M).t() @ unsplit_x3(B3, N), (M, N), out, alpha, beta,
                            bias, None, M3=M, N3=N)


def bare_model(row):
    """A Model with nothing but what `_mm` reads."""
    m = object.__new__(Model)
    m.bf16, m.x3 = row["mode"] == "bf16", row["mode"] == "bf16x3"
    m.use_shadows = m.bf16 and row.get("shadows", True)
    m._shadows = {}
    return m


def call_mm(model, row, t):
    return model._mm(t["A"], t["B"], ta=row["ta"], tb=row["tb"], out=t["out"], alpha=ALPHA, beta=t["beta"], bias=t["bias"],
                     epilogue=t["ep"], x3_ok=row.get("x3_ok", True))


def check_route(row, t, spy):
    """What both files assert of the calls a row made: ONE product, on the function and the operand forms the table names,
    each shadow made from the very view `_mm` was given, and every argument handed through."""
    assert len(spy.calls) == 1, [c["name"] for c in spy.calls]
    c = spy.calls[0]
    fn, bf16 = ROUTE_FN[row["route"]]
    assert c["name"] == fn, (row["id"], c["name"], c["forms"])
    assert c["forms"] == tuple(row["forms"]), (row["id"], c["forms"])
    assert c["srcs"][0] is t["A"] and c["srcs"][1] is t["B"], row["id"]
    assert c["alpha"] == ALPHA
    if fn == "gemm":
        assert (c["bf16"], c["ta"], c["tb"]) == (bf16, row["ta"], row["tb"])
    if fn == "gemm_bf16_nt":
        assert c["K"] == row["K"]
    if fn == "gemm_bf16x3_nt":
        assert c["K3"] == row["K"]
    if fn == "gemm_bf16x3_tn":
        assert (c["M3"], c["N3"]) == (row["M"], row["N"])
    if row["route"] == "pad_tn":
        # the kernel writes a fresh [256, N] / [M, 256] product; `_mm` copies the valid block out
        assert c["out"] is None and c["beta"] == 0.0 and c["bias"] is None and c["epilogue"] is None
        pad, src = (c["A"], t["A"]) if row["forms"][0] == "pad256" else (c["B"], t["B"])
        assert pad.shape == (row["K"], 256) and pad.dtype == torch.bfloat16
        assert not bool(pad[:, src.shape[1]:].any()), "pad columns of the 256-column shadow must be zero"
        assert torch.equal(pad[:, :src.shape[1]], src.to(torch.bfloat16))
    else:
        assert c["out"] is t["out"] and c["beta"] == t["beta"] and c["bias"] is t["bias"] and c["epilogue"] is t["ep"]
    return c


@pytest.mark.parametrize("row", ROUTES, ids=[r["id"] for r in ROUTES])
def test_route(row, monkeypatch):
    monkeypatch.setattr(model_mod, "X3_FORCE", bool(row.get("force")))
    spy = Spy(monkeypatch, compute=not is_big(row))
    t = operands(row)
    got = call_mm(bare_model(row), row, t)
    check_route(row, t, spy)
    assert tuple(got.shape) == (row["M"], row["N"]) and got.dtype == torch.float32
    if t["out"] is not None:
        assert got is t["out"]
    else:
        assert got.is_contiguous()
    if t["parent"] is not None:
        keep = torch.ones_like(t["parent"], dtype=torch.bool)
        (keep[8:8 + row["M"]] if row["out"] == "rows" else keep[:, 256:256 + row["N"]]).fill_(False)
        assert bool((t["parent"][keep] == SENTINEL).all()), "written outside the window"
    if not is_big(row):
        ref, mag = reference(row, t)
        assert error_ratio(row, got.numpy(), ref, mag) < 1.0, row["id"]
        if t["shadow"] is not None:
            assert torch.equal(t["shadow"], got.to(torch.bfloat16))


def test_table_holds_the_rows_it_must():
    """The shapes the routes begin and end at: a row that leaves the table takes its threshold out of both files."""
    have = {(r["mode"], r["ta"], r["tb"], r["M"], r["N"], r["K"], r["route"]) for r in ROUTES}
    for want in [("bf16", True, False, 256, 512, 520, "tn"), ("bf16", True, False, 256, 264, 520, "nt"),
                 ("bf16", True, False, 256, 264, 4100, "conv"),
                 ("bf16", True, False, 40, 512, 4096, "pad_tn"), ("bf16", True, False, 512, 44, 4096, "pad_tn"),
                 ("bf16", True, False, 255, 256, 4096, "pad_tn"), ("bf16", True, False, 1, 256, 4096, "pad_tn"),
                 ("bf16", True, False, 40, 512, 4100, "pad_tn"), ("bf16", True, False, 40, 512, 4088, "nt"),
                 ("bf16", True, False, 40, 512, 4095, "conv"), ("bf16", True, False, 40, 44, 4096, "nt"),
                 ("bf16", False, False, 256, 256, 64, "nn"), ("bf16", False, False, 256, 256, 72, "nt"),
                 ("bf16", False, False, 264, 256, 64, "nt"), ("bf16", False, False, 256, 264, 64, "nt"),
                 ("bf16", False, False, 256, 256, 60, "conv"), ("bf16", False, False, 256, 256, 8, "nt"),
                 ("bf16", False, False, 256, 256, 7, "conv"),
                 ("bf16x3", False, False, 8192, 1024, 1216, "x3_nt"), ("bf16x3", False, True, 8192, 1024, 1216, "x3_nt"),
                 ("bf16x3", False, False, 8192, 1024, 1152, "f32"), ("bf16x3", True, False, 2048, 4096, 4096, "x3_tn"),
                 ("bf16x3", True, False, 2048, 4096, 4088, "f32")]:
        assert want in have, want
    by_id = {r["id"]: r for r in ROUTES}
    assert len(by_id) == len(ROUTES)
    assert by_id["ta_window_stride_260"]["route"] != "tn" and (256 + 4) % 8 != 0
    for rid in ("pad_not_with_beta", "pad_not_with_bias", "pad_not_with_epilogue"):
        assert "pad256" not in by_id[rid]["forms"] and (by_id[rid]["M"], by_id[rid]["N"], by_id[rid]["K"]) == (40, 512, 4096)
    assert by_id["pad_out_row_window"]["out"] == "rows" and by_id["pad_out_strided"]["out"] == "cols"
    assert not by_id["x3_tn_not_ok"]["x3_ok"] and by_id["x3_tn_epilogue"]["ep"]
    assert not any(r.get("force") for r in ROUTES if is_big(r))
    assert {r["route"] for r in ROUTES} == set(ROUTE_FN) and any(r["mode"] == "fp32" for r in ROUTES)


def test_shadow_cache_is_keyed_on_the_view(monkeypatch):
    """One cast per (address, shape, row stride, orientation) and step: a second product on the same view re-uses the shadow,
    a narrower window at the same address, another orientation or the padded form do not."""
    spy = Spy(monkeypatch, compute=False)
    m = bare_model(dict(mode="bf16"))
    buf, W = torch.randn(4096, 520), torch.randn(4096, 512)
    m._mm(buf[:, :512], W, ta=True)
    assert spy.casts == ["cast_bf16"] * 2
    m._mm(buf[:, :512], W, ta=True)
    assert len(spy.casts) == 2 and spy.calls[1]["A"] is spy.calls[0]["A"] and spy.calls[1]["B"] is spy.calls[0]["B"]
    m._mm(buf[:, :256], W, ta=True)                                      # same address, other shape
    assert len(spy.casts) == 3 and spy.calls[2]["A"] is not spy.calls[0]["A"] and spy.calls[2]["B"] is spy.calls[0]["B"]
    m._mm(buf[:, :40], W, ta=True)                                       # ... and the padded form of a third
    assert len(spy.casts) == 4 and spy.calls[3]["forms"] == ("pad256", "nat") and spy.calls[3]["A"].shape == (4096, 256)
    m._mm(buf[:, :40], W[:, :264], ta=True)                              # NT: transposed shadows of both, cast anew
    assert len(spy.casts) == 6 and spy.calls[4]["forms"] == ("tr", "tr")
    assert torch.equal(spy.calls[4]["A"], buf[:, :40].t().to(torch.bfloat16))
    m._adopt_shadow(buf[:, :512], torch.zeros(4096, 512, dtype=torch.bfloat16))
    m._mm(buf[:, :512], W, ta=True)                                      # an adopted shadow takes the cast one's place
    assert len(spy.casts) == 6 and not bool(spy.calls[5]["A"].any())


# ------------------------------------------------------------------------------ the bounds can fail (one row per route)
PROOF = ["x3_nt_forced_300x200x100", "x3_tn_forced_1000x300x520", "f32_tb", "ta_tn_520x256x512", "pad_40x512", "pad_512x44",
         "nn_256x256x64", "ta_nt_n264", "ta_conv_k4100_n264"]


@pytest.mark.parametrize("rid", PROOF)
def test_the_bound_of_a_row_can_fail(rid):
    """A reference with one k index dropped, or with two rows of one stored operand swapped, is further from the true
    reference than the row's bound allows - a kernel that does either cannot pass -, while the plain float32 product of the
    same operands stays inside it."""
    row = {r["id"]: r for r in ROUTES}[rid]
    t = operands(row)
    A, B = rounded(row, t["A"]), rounded(row, t["B"])
    ref, mag = reference(row, t, A, B)
    a32, b32 = A.astype(np.float32), B.astype(np.float32)
    f32 = np.float32(ALPHA) * ((a32.T if row["ta"] else a32) @ (b32.T if row["tb"] else b32))
    if t["C0"] is not None:
        f32 = f32 + np.float32(t["beta"]) * t["C0"].numpy()
    if t["bias"] is not None:
        f32 = f32 + t["bias"].numpy()
    assert f32.dtype == np.float32 and error_ratio(row, f32, ref, mag) < 1.0
    k = row["K"] // 3
    Ad, Bd = np.delete(A, k, axis=0 if row["ta"] else 1), np.delete(B, k, axis=1 if row["tb"] else 0)
    dropped, _ = reference(row, t, Ad, Bd)
    assert error_ratio(row, dropped, ref, mag) > 1.0
    for which in (0, 1):
        X = [A.copy(), B.copy()]
        X[which][[1, 2]] = X[which][[2, 1]]
        swapped, _ = reference(row, t, X[0], X[1])
        assert error_ratio(row, swapped, ref, mag) > 1.0, which
    assert set(r["route"] for r in ROUTES if r["id"] in PROOF) == set(ROUTE_FN)


@pytest.mark.parametrize("rid", ["pad_40x512", "pad_512x44"])
def test_a_nonzero_pad_column_fails(rid):
    """The padded route's kernel multiplies all 256 columns of the padded shadow; its whole [256, N] / [M, 256] product is
    compared with the reference of the zero-padded operand (the GPU file does).  One 1.0 in a pad column puts a sum of the
    other operand's entries where a zero belongs."""
    row = {r["id"]: r for r in ROUTES}[rid]
    t = operands(row)
    side = 0 if row["forms"][0] == "pad256" else 1
    X = [rounded(row, t["A"]), rounded(row, t["B"])]
    C = X[side].shape[1]
    X[side] = np.concatenate([X[side], np.zeros((row["K"], 256 - C))], axis=1)
    ref, mag = reference(row, t, X[0], X[1])
    valid, _ = reference(row, t)
    assert np.array_equal(ref[:C] if side == 0 else ref[:, :C], valid) and not (ref[C:] if side == 0 else ref[:, C:]).any()
    X[side][5, C] = 1.0
    bad, _ = reference(row, t, X[0], X[1])
    assert error_ratio(row, bad, ref, mag) > 1.0
    assert np.array_equal(bad[:C] if side == 0 else bad[:, :C], valid)      # the valid block alone would not have seen it
