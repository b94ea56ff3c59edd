"""GPU tests of the chunk layout passes (csrc/chunk.hip: lc_chunk_gather / lc_chunk_fold) through ops, against numpy index
arithmetic restating include/lstm_ctc_hip.h.

Every output is a window of a larger NaN-filled buffer: the window must be written completely, nothing outside it may be
touched.  All comparisons are exact: the passes copy, or add float32 terms in a fixed order (the numpy sum takes them in the
same ascending chunk order, the first term initialising it)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (T, B, C, Nc, Nr, pitch pad): pad 0 = pitches C + 8 at a 16-byte aligned offset (vector path), else C + pad (scalar path)
CASES = [
    (11, 3, 64, 4, 2, 0),
    (11, 3, 64, 4, 0, 0),
    (11, 3, 64, 4, 9, 0),          # three copies per frame
    (11, 1, 64, 16, 3, 0),         # one chunk, Tc = T
    (12, 3, 64, 4, 2, 0),          # T a multiple of Nc
    (7, 2, 6, 3, 1, 3),            # pitches C + 3: scalar path
    (5, 300, 8, 2, 1, 0),          # Bc = 900 rows
    (11, 4, 64, 4, 9, 0),          # B = 4: the four kinds of length side by side (seq_len tests)
    # every path of csrc/row_stream.h's map_rows_kernel through the chunk maps
    (5, 2, 4100, 2, 1, 0),         # 1025 float4 per row on 256 lanes: the four-in-flight copy loop and its remainder
    (5, 2, 1030, 2, 1, 3),         # the same through the scalar path
    (4, 33000, 8, 2, 1, 0),        # 198000 gathered / 132000 folded rows at 4 lanes: RS_MAX_GROUPS * 64 = 131072 rows per sweep
]
IDS = ["T%d_B%d_C%d_Nc%d_Nr%d_pad%d" % c for c in CASES]


def _shape(T, B, Nc, Nr):
    nC = -(-T // Nc)
    return nC, min(Nc + Nr, T), nC * B


def _window(rows, C, pad, fill=None):
    """(whole buffer, [rows, C] window of it): NaN everywhere, or the window filled with `fill` (a numpy [rows, C])."""
    ld, off = (C + 8, 4) if pad == 0 else (C + pad, 1)
    big = torch.full((rows + 4, ld), float("nan"), dtype=torch.float32, device="cuda")
    win = big[2:2 + rows, off:off + C]
    if fill is not None:
        win.copy_(torch.from_numpy(np.ascontiguousarray(fill)).cuda())
    return big, win


def _outside_untouched(big, rows, C, pad):
    off = 4 if pad == 0 else 1
    m = torch.ones_like(big, dtype=torch.bool)
    m[2:2 + rows, off:off + C] = False
    return bool(torch.isnan(big[m]).all())


def np_gather(x, Nc, Nr, zero_lookahead):
    T, B, C = x.shape
    nC, Tc, Bc = _shape(T, B, Nc, Nr)
    out = np.zeros((Tc, Bc, C), np.float32)
    for c in range(nC):
        for tau in range(Tc):
            t = c * Nc + tau
            if t < T and (not zero_lookahead or tau < Nc):
                out[tau, c * B:(c + 1) * B] = x[t]
    return out


def np_lengths(seq_len, T, Nc, Nr):
    nC, Tc, _ = _shape(T, len(seq_len), Nc, Nr)
    return np.array([min(max(int(seq_len[b]) - c * Nc, 0), Tc) for c in range(nC) for b in range(len(seq_len))], np.int32)


def np_fold(xc, T, B, Nc, Nr, sum_copies, seq_len=None):
    nC, Tc, Bc = _shape(T, B, Nc, Nr)
    C = xc.shape[2]
    out = np.zeros((T, B, C), np.float32)
    lens = None if seq_len is None else np_lengths(seq_len, T, Nc, Nr)
    for t in range(T):
        for b in range(B):
            if seq_len is not None and t >= seq_len[b]:
                continue
            chunks = [c for c in range(nC) if c * Nc <= t < c * Nc + Tc] if sum_copies else [t // Nc]
            acc = None
            for c in chunks:                       # ascending; the first term initialises the sum
                if lens is not None and t - c * Nc >= lens[c * B + b]:
                    continue
                v = xc[t - c * Nc, c * B + b]
                acc = v.copy() if acc is None else (acc + v).astype(np.float32)
            if acc is not None:
                out[t, b] = acc
    return out


def _lengths_for(T, B, Nc):
    kinds = [T, (T // Nc) * Nc if T >= Nc else T, 1, 0]            # T, a multiple of Nc, 1, 0
    return np.array([kinds[b % 4] for b in range(B)], np.int32)


@pytest.mark.parametrize("zero_lookahead", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_chunk_gather(case, zero_lookahead):
    from lstm_ctc_amd import ops
    T, B, C, Nc, Nr, pad = case
    rng = np.random.default_rng(T * 131 + B)
    x = rng.normal(size=(T, B, C)).astype(np.float32)
    x[0, 0, 0] = -0.0
    _, xw = _window(T * B, C, pad, x.reshape(T * B, C))
    nC, Tc, Bc = _shape(T, B, Nc, Nr)
    assert ops.chunk_shape(T, B, Nc, Nr) == (nC, Tc, Bc)
    big, out = _window(Tc * Bc, C, pad)
    ops.chunk_gather(xw, T, B, Nc, Nr, zero_lookahead=bool(zero_lookahead), out=out)
    ref = np_gather(x, Nc, Nr, zero_lookahead).reshape(Tc * Bc, C)
    got = out.cpu().numpy()
    assert np.array_equal(got, ref)
    assert np.array_equal(np.signbit(got), np.signbit(ref))          # copies keep -0, fills are +0
    assert _outside_untouched(big, Tc * Bc, C, pad)
    again = torch.empty((Tc * Bc, C), dtype=torch.float32, device="cuda")
    ops.chunk_gather(xw, T, B, Nc, Nr, zero_lookahead=bool(zero_lookahead), out=again)
    assert torch.equal(again, out)                                   # same call, same bits (and a contiguous out)


@pytest.mark.parametrize("with_len", [False, True], ids=["nolen", "len"])
@pytest.mark.parametrize("sum_copies", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_chunk_fold(case, sum_copies, with_len):
    from lstm_ctc_amd import ops
    T, B, C, Nc, Nr, pad = case
    rng = np.random.default_rng(T * 17 + B + 5 * sum_copies)
    nC, Tc, Bc = _shape(T, B, Nc, Nr)
    xc = rng.normal(size=(Tc, Bc, C)).astype(np.float32)
    seq_len = None
    if with_len:
        seq_len = _lengths_for(T, B, Nc)
        lens = np_lengths(seq_len, T, Nc, Nr)
        got_lens = ops.chunk_lengths(torch.from_numpy(seq_len).cuda(), T, Nc, Nr)
        assert got_lens.dtype == torch.int32 and np.array_equal(got_lens.cpu().numpy(), lens)
        for r in range(Bc):
            xc[lens[r]:, r] = np.nan               # what a recurrence left in dead frames must not matter
    _, xw = _window(Tc * Bc, C, pad, xc.reshape(Tc * Bc, C))
    big, out = _window(T * B, C, pad)
    sl = None if seq_len is None else torch.from_numpy(seq_len).cuda()
    ops.chunk_fold(xw, T, B, Nc, Nr, sum_copies=bool(sum_copies), seq_len=sl, out=out)
    ref = np_fold(xc, T, B, Nc, Nr, sum_copies, seq_len).reshape(T * B, C)
    got = out.cpu().numpy()
    assert not np.isnan(got).any()
    assert np.array_equal(got, ref)
    if with_len:
        dead = (np.arange(T)[:, None] >= seq_len[None, :]).reshape(T * B)
        assert dead.any() or B == 1
        assert not got[dead].any() and not np.signbit(got[dead]).any()          # +0 rows beyond seq_len
    assert _outside_untouched(big, T * B, C, pad)
    again = torch.empty((T * B, C), dtype=torch.float32, device="cuda")
    ops.chunk_fold(xw, T, B, Nc, Nr, sum_copies=bool(sum_copies), seq_len=sl, out=again)
    assert torch.equal(again, out)


def test_gather_then_fold_is_identity_and_counts_copies():
    """fold(gather(x)) = x bit for bit; the summed fold of gathered ones counts the chunk windows that hold each frame."""
    from lstm_ctc_amd import ops
    T, B, C, Nc, Nr = 11, 3, 64, 4, 9
    x = torch.randn((T * B, C), device="cuda")
    assert torch.equal(ops.chunk_fold(ops.chunk_gather(x, T, B, Nc, Nr), T, B, Nc, Nr), x)
    ones = torch.ones((T * B, C), device="cuda")
    n = ops.chunk_fold(ops.chunk_gather(ones, T, B, Nc, Nr), T, B, Nc, Nr, sum_copies=True).view(T, B, C)
    nC, Tc, _ = _shape(T, B, Nc, Nr)
    for t in range(T):
        assert float(n[t, 0, 0]) == sum(1 for c in range(nC) if c * Nc <= t < c * Nc + Tc)


BAD = {   # name -> overrides of (x, ldx, T, B, C, chunk, lookahead, out, ldo)
    "T0": dict(T=0), "B0": dict(B=0), "C0": dict(C=0), "Tneg": dict(T=-1), "chunk0": dict(chunk=0), "chunkneg": dict(chunk=-2),
    "lookaheadneg": dict(lookahead=-1), "null_x": dict(x=None), "null_out": dict(out=None), "ldx_small": dict(ldx=7),
    "ldo_small": dict(ldo=7),
}


@pytest.mark.parametrize("fold", [0, 1], ids=["gather", "fold"])
@pytest.mark.parametrize("bad", sorted(BAD))
def test_chunk_einval_touches_nothing(bad, fold):
    from lstm_ctc_amd import _lib
    lib = _lib.load()
    T, B, C, Nc, Nr = 6, 2, 8, 2, 1
    x = torch.randn((64, C), device="cuda")
    out = torch.full((64, C), float("nan"), device="cuda")
    a = dict(x=x.data_ptr(), ldx=C, T=T, B=B, C=C, chunk=Nc, lookahead=Nr, out=out.data_ptr(), ldo=C)
    a.update(BAD[bad])
    p = lambda v: None if v is None else ctypes.c_void_p(v)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    if fold:
        rc = lib.lc_chunk_fold(p(a["x"]), a["ldx"], a["T"], a["B"], a["C"], a["chunk"], a["lookahead"], 1, None, p(a["out"]),
                               a["ldo"], stream)
    else:
        rc = lib.lc_chunk_gather(p(a["x"]), a["ldx"], a["T"], a["B"], a["C"], a["chunk"], a["lookahead"], 0, p(a["out"]),
                                 a["ldo"], stream)
    torch.cuda.synchronize()
    assert rc == -1                                  # LC_EINVAL
    assert lib.lc_last_error()
    assert bool(torch.isnan(out).all())
