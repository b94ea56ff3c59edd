"""The table of tests/test_gpu_stream_discipline.py, part A: one row per call shape of every C entry point of
include/lstm_ctc_hip.h that takes an ``lc_stream_t``, at the smallest shape that still takes the entry's multi-launch path.
Imports without a GPU (tests/test_stream_table_host.py reads ``ROWS`` and ``COVERED_ELSEWHERE`` on the host): nothing here
touches a device until a row's ``call`` runs.

A row is ``Row(name, entries, env, make)``: the C entries it exercises, environment variables the test sets around it
(``monkeypatch.setenv``), and ``make(rng)`` -> ``Case``:

    inp    {name: float32 numpy array or CPU torch tensor}  float inputs and in/out tensors, at their FINAL values
    ints   {name: integer numpy array}                      lengths, labels, offsets, row maps, windows, frame targets, guards
    out    {name: (shape, torch dtype)}                      tensors the call receives as ``out=`` (the harness owns their fill)
    io     names in ``inp`` that the call also writes (accumulators, in-place forms): compared after the call
    prep   None or f(ops, t) -> {name: tensor}               derived float inputs made on the default stream (x3 shadows)
    call   f(ops, t) -> a tensor, a tuple of tensors or None the op(s), through lstm_ctc_amd.ops, on the tensors ``t[name]``
    post   None or f(ret) -> ret                             normalises returned tensors whose tail is unspecified

Integer inputs never go through NaN: the harness gives them their final values before anything is launched, so a launch
that ran early could read garbage VALUES and never a garbage INDEX."""
import re
from collections import namedtuple

import numpy as np

Row = namedtuple("Row", "name entries env make")
Case = namedtuple("Case", "inp ints out io prep call post")
ROWS = []

# Entries whose stream discipline another test holds: entry -> "file::test" (the host test greps the file for the name).
COVERED_ELSEWHERE = {
    "lc_lstm_fwd": "tests/test_gpu_lstm_edges.py::test_runs_on_the_callers_stream",
    "lc_lstm_bwd": "tests/test_gpu_lstm_edges.py::test_runs_on_the_callers_stream",
    "lc_ctc_align": "tests/test_gpu_align.py::test_runs_on_the_callers_stream",
    # the spin is the harness's own tool: a misplaced call is only reported when the spin really holds the side stream
    "lc_debug_spin": "tests/test_gpu_stream_discipline.py::test_harness_reports_a_misplaced_call",
}


def stream_entries(header_text):
    """Every prototype of the header with an ``lc_stream_t`` parameter, in order of appearance."""
    text = re.sub(r"/\*.*?\*/", " ", header_text, flags=re.S)
    names = []
    for m in re.finditer(r"\b(?:int|void|size_t)\s+(lc_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        if re.search(r"\blc_stream_t\b", m.group(2)):
            names.append(m.group(1))
    return names


def row(name, entries, env=None):
    def deco(make):
        ROWS.append(Row(name, tuple(entries), dict(env or {}), make))
        return make
    return deco


def case(inp, call, ints=None, out=None, io=(), prep=None, post=None):
    return Case(dict(inp), dict(ints or {}), dict(out or {}), tuple(io), prep, call, post)


def _f(rng, *shape, scale=1.0):
    return (rng.normal(size=shape) * scale).astype(np.float32)


def _bf16(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16)


def _torch():
    import torch
    return torch


BIG = {"LC_GEMM_F32_BIG": "2"}


# ------------------------------------------------------------------------------------------------ lc_gemm_f32 / lc_gemm_bf16
def _gemm_row(name, entry, M, N, K, env=None, bf16=False, full=False, epilogue=False):
    @row(name, [entry], env)
    def make(rng):
        inp = dict(A=_f(rng, M, K), B=_f(rng, K, N))
        out = {}
        io = ()
        if full:
            inp.update(C=_f(rng, M, N), bias=_f(rng, N))
            io = ("C",)
        else:
            out["C"] = ((M, N), _torch().float32)
        if epilogue:
            out["C16"] = ((M, N), _torch().bfloat16)

        def call(ops, t):
            ep = ops.Epilogue(0.7, 5, 2, N // 2, t["C16"]) if epilogue else None
            if full:
                ops.gemm(t["A"], t["B"], out=t["C"], alpha=0.5, beta=2.0, bias=t["bias"], bf16=bf16)
            else:
                ops.gemm(t["A"], t["B"], out=t["C"], bf16=bf16, epilogue=ep)
        return case(inp, call, out=out, io=io)


_gemm_row("gemm_f32_split_k", "lc_gemm_f32", 200, 300, 8192)
_gemm_row("gemm_f32_big_split_k", "lc_gemm_f32", 256, 256, 8192, env=BIG)
_gemm_row("gemm_f32_big_strips", "lc_gemm_f32", 300, 520, 64, env=BIG)
_gemm_row("gemm_f32_alpha_beta_bias", "lc_gemm_f32", 257, 131, 70, full=True)
_gemm_row("gemm_f32_epilogue", "lc_gemm_f32", 96, 64, 40, epilogue=True)
_gemm_row("gemm_bf16_split_k", "lc_gemm_bf16", 200, 300, 8192, bf16=True)
_gemm_row("gemm_bf16_alpha_beta_bias", "lc_gemm_bf16", 257, 131, 70, bf16=True, full=True)


def _nt2_row(name, entry, M, N, K1, K2, env=None, bf16=False):
    """Both pairs as column windows of one [., K1 + K2] buffer each: the entry wants one row stride per side."""
    @row(name, [entry], env)
    def make(rng):
        A, B = _f(rng, M, K1 + K2), _f(rng, N, K1 + K2)
        inp = dict(A=_bf16(A) if bf16 else A, B=_bf16(B) if bf16 else B, C=_f(rng, M, N), bias=_f(rng, N))

        def call(ops, t):
            a, b = t["A"], t["B"]
            fn = ops.gemm_bf16_nt2 if bf16 else ops.gemm_nt2
            fn(a[:, :K1], b[:, :K1], a[:, K1:], b[:, K1:], out=t["C"], alpha=0.5, beta=2.0, bias=t["bias"])
        return case(inp, call, io=("C",))


_nt2_row("gemm_f32_nt2_big_and_strips", "lc_gemm_f32_nt2", 600, 300, 128, 128, env=BIG)
_nt2_row("gemm_f32_nt2_sequence", "lc_gemm_f32_nt2", 100, 64, 64, 32)
_nt2_row("gemm_bf16_nt2_whole_tiles", "lc_gemm_bf16_nt2", 256, 256, 64, 64, bf16=True)
_nt2_row("gemm_bf16_nt2_ragged", "lc_gemm_bf16_nt2", 257, 131, 72, 40, bf16=True)


# ------------------------------------------------------------------------------------------------ bf16 shadows
for _nat, _tr in ((True, False), (False, True), (True, True)):
    def _cast(nat=_nat, tr=_tr):
        @row("cast_bf16_%s" % ("both" if nat and tr else "nat" if nat else "tr"), ["lc_cast_bf16"])
        def make(rng):
            def call(ops, t):
                return ops.cast_bf16(t["x"], nat=nat, tr=tr)
            return case(dict(x=_f(rng, 37, 52)), call)
    _cast()


def _shadow_product(name, entry, form, M, N, K):
    """form: "nt" A [M,K] B [N,K]; "tn" A [K,M] B [K,N]; "nn" A [M,K] B [K,N] - bf16, last stride 1."""
    @row(name, [entry])
    def make(rng):
        sa = (K, M) if form == "tn" else (M, K)
        sb = (N, K) if form == "nt" else (K, N)
        inp = dict(A=_bf16(_f(rng, *sa)), B=_bf16(_f(rng, *sb)), C=_f(rng, M, N), bias=_f(rng, N))

        def call(ops, t):
            fn = {"nt": ops.gemm_bf16_nt, "tn": ops.gemm_bf16_tn, "nn": ops.gemm_bf16_nn}[form]
            fn(t["A"], t["B"], out=t["C"], alpha=0.5, beta=2.0, bias=t["bias"])
        return case(inp, call, io=("C",))


_shadow_product("gemm_bf16_nt_ragged", "lc_gemm_bf16_nt", "nt", 257, 131, 72)
_shadow_product("gemm_bf16_nt_whole_tiles", "lc_gemm_bf16_nt", "nt", 256, 384, 192)
_shadow_product("gemm_bf16_nt_split_k", "lc_gemm_bf16_nt", "nt", 768, 256, 4160)
_shadow_product("gemm_bf16_tn_ragged_k", "lc_gemm_bf16_tn", "tn", 256, 512, 200)
_shadow_product("gemm_bf16_tn_split_k", "lc_gemm_bf16_tn", "tn", 768, 256, 4160)
_shadow_product("gemm_bf16_nn_whole_tiles", "lc_gemm_bf16_nn", "nn", 256, 256, 64)
_shadow_product("gemm_bf16_nn_split_k", "lc_gemm_bf16_nn", "nn", 768, 256, 4160)


@row("split_bf16x3", ["lc_split_bf16x3"])
def _split(rng):
    return case(dict(x=_f(rng, 37, 52)), lambda ops, t: ops.split_bf16x3(t["x"]))


def _x3_product(name, entry, form, M, N, K):
    """The x3 shadows are made by lc_split_bf16x3 on the default stream first (``prep``): they are the row's float inputs."""
    @row(name, [entry])
    def make(rng):
        host = dict(A=_f(rng, *((K, M) if form == "tn" else (M, K))), B=_f(rng, *((K, N) if form == "tn" else (N, K))))

        def prep(ops, t):
            torch = _torch()
            return {"A3": ops.split_bf16x3(torch.from_numpy(host["A"]).cuda()),
                    "B3": ops.split_bf16x3(torch.from_numpy(host["B"]).cuda())}

        def call(ops, t):
            if form == "nt":
                ops.gemm_bf16x3_nt(t["A3"], t["B3"], K, out=t["C"], alpha=0.5, beta=2.0, bias=t["bias"])
            else:
                ops.gemm_bf16x3_tn(t["A3"], t["B3"], M, N, out=t["C"], alpha=0.5, beta=2.0, bias=t["bias"])
        return case(dict(C=_f(rng, M, N), bias=_f(rng, N)), call, io=("C",), prep=prep)


_x3_product("gemm_bf16x3_nt_ragged", "lc_gemm_bf16x3_nt", "nt", 300, 130, 40)
_x3_product("gemm_bf16x3_nt_whole_tiles", "lc_gemm_bf16x3_nt", "nt", 256, 256, 64)
_x3_product("gemm_bf16x3_tn_split_k", "lc_gemm_bf16x3_tn", "tn", 40, 512, 5000)
_x3_product("gemm_bf16x3_tn_one_slice", "lc_gemm_bf16x3_tn", "tn", 33, 17, 100)


# ------------------------------------------------------------------------------------------------ recurrences
def _lengths(B, T):
    return np.array([[T - 1, 0, T, 1, T - 2, T][b % 6] for b in range(B)], np.int32).clip(0, T)


def _lstm_row(name, entry, N, ndir, B, T, kind):
    """Forward and backward call of one problem (tests/test_lstm_edges_host.py's scales); ``kind``: the schedule both calls
    must report - the dispatch for these shapes is stated in tests/test_lstm_edges_host.py's tables."""
    bf16, x3 = entry == "bf16", entry == "x3"

    @row(name, ["lc_lstm_fwd_%s" % entry, "lc_lstm_bwd_%s" % entry])
    def make(rng):
        torch = _torch()
        inp, out, io = {}, {}, []
        for d in range(ndir):
            R = _f(rng, N, 4 * N, scale=0.5 / np.sqrt(N))
            inp.update({"zx%d" % d: _f(rng, T, B, 4 * N, scale=0.5), "R%d" % d: R, "RT%d" % d: np.ascontiguousarray(R.T),
                        "dh%d" % d: _f(rng, T, B, N, scale=0.1), "dpeep%d" % d: _f(rng, 3, N, scale=0.1),
                        "dbias%d" % d: _f(rng, 4 * N, scale=0.1)})
            if d == 0:
                inp["w0"] = _f(rng, 3, N, scale=0.2)
            io += ["zx%d" % d, "dpeep%d" % d, "dbias%d" % d]
            out.update({"cs%d" % d: ((T, B, N), torch.float32), "hs%d" % d: ((T, B, N), torch.float32)})
            if bf16:
                out.update({"hs16_%d" % d: ((T, B, N), torch.bfloat16), "dz16_%d" % d: ((T, B, 4 * N), torch.bfloat16)})
            if x3:
                out["dzx3_%d" % d] = ((T * B, 12 * N), torch.bfloat16)

        def call(ops, t):
            fw, bw = [], []
            for d in range(ndir):
                w = t["w0"] if d == 0 else None
                peep = dict(w_f=w[0], w_i=w[1], w_o=w[2]) if w is not None else {}
                fw.append(dict(zx=t["zx%d" % d], R=t["R%d" % d], cs=t["cs%d" % d], hs=t["hs%d" % d], reverse=d,
                               hs_bf16=t.get("hs16_%d" % d), **peep))
                bw.append(dict(gates=t["zx%d" % d], RT=t["RT%d" % d], cs=t["cs%d" % d], dh=t["dh%d" % d],
                               dpeep=t["dpeep%d" % d], dbias=t["dbias%d" % d], reverse=d, dz_bf16=t.get("dz16_%d" % d),
                               dz_x3=t.get("dzx3_%d" % d), **peep))
            ops.lstm_fwd(fw, t["seq"], T, B, N, 1.0, bf16=bf16, x3=x3)
            assert ops.last_lstm_schedule()["kind"] == kind, ops.last_lstm_schedule()
            ops.lstm_bwd(bw, t["seq"], T, B, N, bf16=bf16, x3=x3)
            assert ops.last_lstm_schedule()["kind"] == kind, ops.last_lstm_schedule()
        return case(inp, call, ints=dict(seq=_lengths(B, T)), out=out, io=io)


_lstm_row("lstm_bf16_persistent", "bf16", 96, 2, 19, 5, "persistent_bf16")
_lstm_row("lstm_bf16_launch_train", "bf16", 64, 2, 40, 3, "launch_train")
_lstm_row("lstm_x3_persistent", "x3", 64, 2, 3, 4, "persistent_x3")
_lstm_row("lstm_x3_launch_train", "x3", 64, 2, 17, 3, "launch_train")


# ------------------------------------------------------------------------------------------------ misc.hip
def _dropout_row(name, entry, P, accumulate, shadow=False):
    @row(name, [entry])
    def make(rng):
        rows = 45
        inp = dict(x=_f(rng, rows, 2 * P))
        out, io = {}, ["x"]
        if accumulate:
            inp["y"] = _f(rng, rows, P)
            io.append("y")
        if shadow:
            out["y16"] = ((rows, 2 * P), _torch().bfloat16)

        def call(ops, t):
            ops.dropout_scale(t["x"][:, P:], 0.9, 77, 3, out=t["y"] if accumulate else None, accumulate=accumulate,
                              shadow=t["y16"][:, P:] if shadow else None)
        return case(inp, call, out=out, io=io)


_dropout_row("dropout_scale_scalar", "lc_dropout_scale", 10, False)
_dropout_row("dropout_scale_vector", "lc_dropout_scale", 12, False)
_dropout_row("dropout_scale_accumulate", "lc_dropout_scale", 64, True)
_dropout_row("dropout_scale_bf16", "lc_dropout_scale_bf16", 12, False, shadow=True)
_dropout_row("dropout_scale_bf16_accumulate", "lc_dropout_scale_bf16", 64, True, shadow=True)


@row("colsum_plain", ["lc_colsum"])
def _colsum_plain(rng):
    return case(dict(x=_f(rng, 257, 70)), lambda ops, t: ops.colsum(t["x"], out=t["s"]),
                out=dict(s=((70,), _torch().float32)))


@row("colsum_accumulate", ["lc_colsum"])
def _colsum_acc(rng):
    return case(dict(x=_f(rng, 257, 70), s=_f(rng, 70)), lambda ops, t: ops.colsum(t["x"], out=t["s"], accumulate=True),
                io=("s",))


@row("transpose", ["lc_transpose"])
def _transpose(rng):
    return case(dict(x=_f(rng, 37, 44)), lambda ops, t: ops.transpose(t["x"]))


@row("moe_combine", ["lc_moe_combine_fwd", "lc_moe_combine_bwd"])
def _moe(rng):
    R, E, V = 30, 3, 11

    def call(ops, t):
        logits, pi = ops.moe_combine_fwd(t["a"], t["q"], E, V, 10.0, 0.8, 3)
        return logits, pi, ops.moe_combine_bwd(pi, t["q"], t["dl"], E, V, 10.0, 0.8, 3)
    return case(dict(a=_f(rng, R, E), q=_f(rng, R, E * V), dl=_f(rng, R, V)), call, io=("q",))


for _opt in ("sgd", "momentum", "adam"):
    def _optim(opt=_opt):
        @row("optimizer_step_%s" % opt, ["lc_optimizer_step"])
        def make(rng):
            n, n_decay = 10007, 9000          # clip (|g| = 3 sqrt(n) > 5) and L2 on: all three kernels have work

            def call(ops, t):
                ops.optimizer_step(t["p"], t["g"], n_decay, 1e-5, 5.0, opt, 1e-2, 2, t["state"], t["norm"], guard=t["guard"])
            return case(dict(p=_f(rng, n), g=_f(rng, n, scale=3.0), state=np.abs(_f(rng, 2 * n, scale=0.1))), call,
                        ints=dict(guard=np.zeros(1, np.int32)), out=dict(norm=((2,), _torch().float32)),
                        io=("p", "g", "state"))
    _optim()


def _smoothing_row(name, prior):
    @row(name, ["lc_label_smoothing"])
    def make(rng):
        # 7 rows = 2 workgroups: the loss is two double addends onto a zero, the same sum in either order (more workgroups
        # would make the atomic sum order-dependent and a bit-for-bit comparison meaningless)
        rows, V = 7, 44
        inp = dict(x=_f(rng, rows, V), d=_f(rng, rows, V))
        if prior:
            q = np.abs(_f(rng, V)) + 0.1
            inp["logq"] = np.log(q / q.sum()).astype(np.float32)
        return case(inp, lambda ops, t: ops.label_smoothing(t["x"], 0.05, log_q=t.get("logq"), dlogits=t["d"]), io=("d",))


_smoothing_row("label_smoothing_uniform", False)
_smoothing_row("label_smoothing_prior", True)


@row("posteriors", ["lc_posteriors"])
def _posteriors(rng):
    return case(dict(x=_f(rng, 37, 44), prior=_f(rng, 44)), lambda ops, t: ops.posteriors(t["x"], 0.7, True, True, t["prior"]))


@row("length_mask", ["lc_length_mask"])
def _length_mask(rng):
    T, B, C = 9, 5, 20

    def call(ops, t):
        ops.length_mask_(t["x"][:, :C], t["seq"], T, B)
    return case(dict(x=_f(rng, T * B, C + 4)), call, ints=dict(seq=_lengths(B, T)), io=("x",))


@row("pack_unpack_rows", ["lc_pack_rows", "lc_unpack_rows"])
def _pack(rng):
    T, B, C = 9, 5, 20
    seq = _lengths(B, T)
    live = (np.arange(T)[:, None] < seq[None, :]).reshape(-1)
    rows = np.flatnonzero(live).astype(np.int32)
    rows = np.concatenate([rows, np.full(3, -1, np.int32)])               # pad rows of the packed matrix: no source
    inverse = np.full(T * B, -1, np.int32)
    inverse[rows[:-3]] = np.arange(len(rows) - 3, dtype=np.int32)
    f32 = _torch().float32

    def call(ops, t):
        ops.pack_rows(t["x"][:, :C], t["rows"], out=t["p"][:, 4:])
        ops.unpack_rows(t["p"][:, 4:], t["inverse"], out=t["u"][:, :C])
    return case(dict(x=_f(rng, T * B, C + 4)), call, ints=dict(rows=rows, inverse=inverse),
                out=dict(p=((len(rows), C + 4), f32), u=((T * B, C + 8), f32)))


# ------------------------------------------------------------------------------------------------ bn.hip
@row("batch_norm", ["lc_bn_moments", "lc_bn_apply", "lc_bn_bwd", "lc_bn_update_moving"])
def _bn(rng):
    rows, C = 300, 40
    f32 = _torch().float32

    def call(ops, t):
        y, mean, var = ops.bn_forward(t["x"], t["gamma"], t["beta"], True, t["mm"], t["mv"], out=t["y"])
        ops.bn_backward(t["x"], t["dy"], mean, var, t["gamma"], True, t["dgamma"], t["dbeta"], dx=t["dx"])
        ops.bn_update_moving(t["mm"], t["mv"], mean, var)
        return mean, var
    return case(dict(x=_f(rng, rows, C), gamma=_f(rng, C), beta=_f(rng, C), dy=_f(rng, rows, C), mm=_f(rng, C),
                     mv=np.abs(_f(rng, C)) + 0.5), call, io=("mm", "mv"),
                out=dict(y=((rows, C), f32), dx=((rows, C), f32), dgamma=((C,), f32), dbeta=((C,), f32)))


# ------------------------------------------------------------------------------------------------ row passes
@row("chunk_gather_fold", ["lc_chunk_gather", "lc_chunk_fold"])
def _chunk(rng):
    T, B, C, chunk, look = 11, 3, 20, 4, 2
    nC, Tc = -(-T // chunk), min(chunk + look, T)
    f32 = _torch().float32

    def call(ops, t):
        ops.chunk_gather(t["x"][:, :C], T, B, chunk, look, zero_lookahead=True, out=t["g"][:, 4:])
        ops.chunk_fold(t["g"][:, 4:], T, B, chunk, look, sum_copies=True, seq_len=t["seq"], out=t["f"][:, :C])
        ops.chunk_fold(t["xc"], T, B, chunk, look, sum_copies=False, out=t["h"])
    return case(dict(x=_f(rng, T * B, C + 4), xc=_f(rng, Tc * nC * B, C)), call, ints=dict(seq=_lengths(B, T)),
                out=dict(g=((Tc * nC * B, C + 4), f32), f=((T * B, C + 8), f32), h=((T * B, C), f32)))


@row("row_conv", ["lc_row_conv_fwd", "lc_row_conv_bwd"])
def _row_conv(rng):
    T, B, C, tau = 40, 9, 36, 2                   # 360 rows: the filter gradient sums more than one slab and folds them
    f32 = _torch().float32

    def call(ops, t):
        ops.row_conv_fwd(t["x"][:, :C], t["w"], t["seq"], T, B, out=t["y"][:, 4:])
        ops.row_conv_bwd(t["x"][:, :C], t["dy"], t["w"], t["seq"], T, B, dx=t["dx"][:, :C], dw=t["dw"])
    return case(dict(x=_f(rng, T * B, C + 4), w=_f(rng, tau + 1, C), dy=_f(rng, T * B, C)), call,
                ints=dict(seq=_lengths(B, T)),
                out=dict(y=((T * B, C + 4), f32), dx=((T * B, C + 8), f32), dw=((tau + 1, C), f32)))


@row("time_reduce", ["lc_time_reduce_fwd", "lc_time_reduce_bwd"])
def _time_reduce(rng):
    T, B, C, r = 11, 3, 20, 2
    To = -(-T // r)
    f32 = _torch().float32

    def call(ops, t):
        ops.time_reduce_fwd(t["x"][:, :C], t["seq"], T, B, r, out=t["y"][:, 4:])
        ops.time_reduce_bwd(t["dy"], t["seq"], T, B, r, out=t["dx"][:, :C])
    return case(dict(x=_f(rng, T * B, C + 4), dy=_f(rng, To * B, r * C)), call, ints=dict(seq=_lengths(B, T)),
                out=dict(y=((To * B, r * C + 4), f32), dx=((T * B, C + 8), f32)))


def _layer_norm_row(C):
    @row("layer_norm_C%d" % C, ["lc_layer_norm_fwd", "lc_layer_norm_bwd"])
    def make(rng):
        T, B = 30, 7
        f32 = _torch().float32

        def call(ops, t):
            kw = dict(keep=0.8, seed=11, stream0=4, drop_width=C // 2)
            ops.layer_norm_fwd(t["x"], t["gamma"], t["beta"], t["seq"], T, B, out=t["y"], **kw)
            ops.layer_norm_bwd(t["x"], t["dy"], t["gamma"], t["seq"], T, B, dx=t["dx"], dgamma=t["dgamma"], dbeta=t["dbeta"], **kw)
        return case(dict(x=_f(rng, T * B, C), gamma=_f(rng, C), beta=_f(rng, C), dy=_f(rng, T * B, C)), call,
                    ints=dict(seq=_lengths(B, T)),
                    out=dict(y=((T * B, C), f32), dx=((T * B, C), f32), dgamma=((C,), f32), dbeta=((C,), f32)))


_layer_norm_row(60)            # sums in registers
_layer_norm_row(2050)          # sums through LDS


def _conv_row(F, Cin, Cout, group_major):
    @row("conv_F%d_Cin%d_Cout%d" % (F, Cin, Cout), ["lc_conv_fwd", "lc_conv_bwd"])
    def make(rng):
        T, B = 10, 3
        Fo = (F + 1) // 2
        f32 = _torch().float32

        def call(ops, t):
            ops.conv_fwd(t["x"], t["w"], t["bias"], t["seq"], T, B, F, group_major=group_major, out=t["y"])
            ops.conv_bwd(t["x"], t["y"], t["dy"], t["w"], t["seq"], T, B, F, group_major=group_major, dx=t["dx"],
                         dw=t["dw"], dbias=t["dbias"])
        return case(dict(x=_f(rng, T * B, Cin * F), w=_f(rng, 3, 3, Cin, Cout, scale=0.3), bias=_f(rng, Cout),
                         dy=_f(rng, T * B, Fo * Cout)), call, ints=dict(seq=_lengths(B, T)),
                    out=dict(y=((T * B, Fo * Cout), f32), dx=((T * B, Cin * F), f32), dw=((3, 3, Cin, Cout), f32),
                             dbias=((Cout,), f32)))


_conv_row(5, 3, 8, True)
_conv_row(41, 8, 64, False)


@row("spec_augment", ["lc_spec_augment"])
def _spec_augment(rng):
    T, B, D = 14, 3, 12

    def call(ops, t):
        from lstm_ctc_amd.nnet.augment import SpecAugment
        spec = SpecAugment(time_masks=2, time_width=4, time_percent=50, freq_masks=1, freq_width=3, freq_bins=D)
        return ops.spec_augment(t["x"], t["seq"], spec, (D, 0, 0, 0), 5, out=t["y"], plan=True)[1]
    return case(dict(x=_f(rng, T, B, D)), call, ints=dict(seq=np.array([14, 9, 0], np.int32)),
                out=dict(y=((T, B, D), _torch().float32)))


# ------------------------------------------------------------------------------------------------ losses
def _ctc_batch(rng, T, B, V, Lmax):
    """Ragged lengths with a 0; utterance 0 is full length with Lmax labels; every label sequence fits its frames (repeats
    included: 2 L + 1 <= its frames).  Returns float logits and the integer inputs."""
    seq = _lengths(B, T)
    seq[0] = T
    lab, offs = [], [0]
    for b in range(B):
        L = Lmax if b == 0 else int(min(Lmax, max(0, (seq[b] - 1) // 2)))
        assert 2 * L + 1 <= max(int(seq[b]), 1)
        lab += list(rng.integers(0, V - 1, size=L))
        offs.append(len(lab))
    ints = dict(labels=np.asarray(lab, np.int32), offsets=np.asarray(offs, np.int32), seq=seq)
    return _f(rng, T, B, V), ints


def _ctc_loss_row(name, T, B, V, Lmax, path, lse2=None):
    @row(name, ["lc_ctc_loss"])
    def make(rng):
        logits, ints = _ctc_batch(rng, T, B, V, Lmax)

        def call(ops, t):
            if lse2 is not None:
                ops.set_option("ctc_lse2", lse2)
            try:
                ret = ops.ctc_loss(t["logits"], t["labels"], t["offsets"], t["seq"], Lmax)
            finally:
                if lse2 is not None:
                    ops.set_option("ctc_lse2", None)
            got = ops.last_ctc_path()
            assert (got["path"], got["lse2"], got["g"]) == path, got
            return ret
        return case(dict(logits=logits), call, ints=ints)


# shapes by tests/test_ctc_edges_host.py's restated dispatch: V <= 128 and S <= 256 -> two launches; V > 128 or S > 256 with
# B <= 128 -> three kernels, the row statistics 16 lanes wide for V <= 32 and 64 above
_ctc_loss_row("ctc_loss_two_launch", 24, 5, 9, 5, ("two_launch", False, 0))
_ctc_loss_row("ctc_loss_two_launch_lse2", 24, 5, 9, 5, ("two_launch", True, 0), lse2=1)
_ctc_loss_row("ctc_loss_three_kernel_wide", 12, 3, 129, 4, ("three_kernel", False, 64))
_ctc_loss_row("ctc_loss_three_kernel_long", 280, 2, 20, 128, ("three_kernel", False, 16))


@row("ctc_greedy", ["lc_ctc_greedy"])
def _greedy(rng):
    logits, ints = _ctc_batch(rng, 24, 5, 9, 5)

    def post(ret):
        torch = _torch()
        tokens, n = ret                                     # row b holds out_len[b] tokens: the rest is unspecified
        keep = torch.arange(tokens.shape[1], device=tokens.device)[None, :] < n[:, None]
        return torch.where(keep, tokens, torch.zeros_like(tokens)), n
    return case(dict(logits=logits), lambda ops, t: ops.ctc_greedy(t["logits"], t["seq"]), ints=dict(seq=ints["seq"]), post=post)


def _windows(ints, T):
    """Per label a window of half the utterance around the label's even share of it: constrains, and leaves paths."""
    lo, hi = [], []
    for b in range(len(ints["seq"])):
        n, L = int(ints["seq"][b]), int(ints["offsets"][b + 1] - ints["offsets"][b])
        for j in range(L):
            c = (j + 0.5) * n / L
            lo.append(int(c - n / 2))
            hi.append(int(c + n / 2))
    return dict(ints, win_lo=np.asarray(lo, np.int32), win_hi=np.asarray(hi, np.int32))


def _lattice_row(name, entry, fn, scalars, windows, grad):
    @row(name, [entry])
    def make(rng):
        T, B, V, Lmax = 24, 5, 9, 5
        logits, ints = _ctc_batch(rng, T, B, V, Lmax)
        if windows:
            ints = _windows(ints, T)

        def call(ops, t):
            kw = dict(win_lo=t["win_lo"], win_hi=t["win_hi"]) if windows else {}
            return getattr(ops, fn)(t["logits"], t["labels"], t["offsets"], t["seq"], Lmax, *scalars, want_grad=grad, **kw)
        return case(dict(logits=logits), call, ints=ints)


_lattice_row("ctc_loss_windowed", "lc_ctc_loss_windowed", "ctc_loss_windowed", (), True, True)
_lattice_row("ctc_loss_delay", "lc_ctc_loss_delay", "ctc_loss_delay", (0.05,), False, True)
_lattice_row("ctc_loss_delay_windows_no_grad", "lc_ctc_loss_delay", "ctc_loss_delay", (0.05,), True, False)
_lattice_row("ctc_loss_entropy", "lc_ctc_loss_entropy", "ctc_loss_entropy", (0.2,), False, True)
_lattice_row("ctc_loss_entropy_windows_no_grad", "lc_ctc_loss_entropy", "ctc_loss_entropy", (0.2,), True, False)
_lattice_row("ctc_loss_star", "lc_ctc_loss_star", "ctc_loss_star", (2.0, 3.0), False, True)
_lattice_row("ctc_loss_star_windows_no_grad", "lc_ctc_loss_star", "ctc_loss_star", (2.0, 3.0), True, False)


def _frame_loss_row(name, entry, V, accumulate):
    """V = 9: four frames per wave; V = 1100: rows are re-read.  accumulate: the ``grad=`` form of kd / consistency."""
    @row(name, [entry])
    def make(rng):
        T, B = 13, 4
        seq = _lengths(B, T)
        inp, ints, io = {}, dict(seq=seq), ()
        if entry == "lc_consistency_loss":
            inp["logits"] = _f(rng, T, 2 * B, V)
        else:
            inp["logits"] = _f(rng, T, B, V)
        if entry == "lc_xent_loss":
            ints["targets"] = rng.integers(-1, V, size=(B, T)).astype(np.int32)
        if entry == "lc_kd_loss":
            inp["teacher"] = _f(rng, T, B, V)
            ints["teacher_len"] = np.minimum(seq + 1, T).astype(np.int32)
        if accumulate:
            inp["grad"] = _f(rng, *inp["logits"].shape)
            io = ("grad",)

        def call(ops, t):
            if entry == "lc_xent_loss":
                return ops.xent_loss(t["logits"], t["targets"], t["seq"])
            if entry == "lc_kd_loss":
                return ops.kd_loss(t["logits"], t["teacher"], t["seq"], t["teacher_len"], temperature=2.0, grad_scale=0.5,
                                   grad=t.get("grad"))[:3 if accumulate else 4]
            return ops.consistency_loss(t["logits"], t["seq"], grad_scale=0.5, grad=t.get("grad"))[:3 if accumulate else 4]
        return case(inp, call, ints=ints, io=io)


_frame_loss_row("xent_loss_narrow", "lc_xent_loss", 9, False)
_frame_loss_row("xent_loss_wide", "lc_xent_loss", 1100, False)
_frame_loss_row("kd_loss", "lc_kd_loss", 9, False)
_frame_loss_row("kd_loss_accumulate", "lc_kd_loss", 1100, True)
_frame_loss_row("consistency_loss", "lc_consistency_loss", 9, False)
_frame_loss_row("consistency_loss_accumulate", "lc_consistency_loss", 1100, True)


def covered_entries():
    return {e for r in ROWS for e in r.entries}
