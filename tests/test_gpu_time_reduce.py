"""GPU tests of lc_time_reduce_fwd / lc_time_reduce_bwd through ops.time_reduce_fwd / _bwd: bit equality with
the numpy statement in tests/time_reduce_reference.py, with sentinels around the output window (rows before and after it, pad
columns beside it) and NaN in every dead source row and every pad column of the source."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import time_reduce_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -77.25
GRID_CAP = 2048                      # csrc/row_stream.h: RS_MAX_GROUPS workgroups, the rest by grid stride
SEGMENTS_PER_WORKGROUP_AT_C4 = 64    # 256 threads / 4 lanes per segment, the narrowest row
ONE_SWEEP = GRID_CAP * SEGMENTS_PER_WORKGROUP_AT_C4      # 131072 segments: more than this and workgroups take a second stride


def _lens(T, r, B):
    """0, 1, r - 1, r, r + 1, T - 1, T and one value above T, then whatever fills B."""
    base = [0, 1, r - 1, r, r + 1, T - 1, T, T + 3]
    rng = np.random.default_rng(T + B)
    more = rng.integers(0, T + 2, size=max(B - len(base), 0)).tolist()
    return np.array((base + more)[:B] if B >= len(base) else base, np.int32)


def _window(rows, C, pitch, offset, fill, guard=3):
    """A [rows, C] window at row pitch ``pitch`` whose base lies ``offset`` floats into a 16-byte aligned buffer, ``guard``
    rows of the buffer before and after it; every element of the buffer is ``fill``."""
    buf = torch.full(((rows + 2 * guard) * pitch + 8,), fill, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    start = guard * pitch + offset
    view = buf[start:start + rows * pitch].view(rows, pitch)[:, :C]
    return buf, view


def _outside_untouched(buf, view, fill):
    """Everything of ``buf`` that is not in ``view`` still holds ``fill``."""
    probe = buf.clone()
    rows, C = view.shape
    start = (view.data_ptr() - buf.data_ptr()) // 4
    probe[start:start + rows * view.stride(0)].view(rows, view.stride(0))[:, :C] = fill
    return bool((probe == fill).all())


def _run(T, B, C, r, lens, x_off=0, x_pad=0, y_off=0, y_pad=0):
    from lstm_ctc_amd import ops
    rng = np.random.default_rng(T * 1000 + B * 10 + C + r)
    To = ref.cdiv(T, r)
    n = np.clip(lens, 0, T)
    sl = torch.from_numpy(lens).cuda()
    live = np.arange(T)[:, None] < n[None, :]
    # ---- fwd: NaN in dead rows and pad columns of x, sentinels around y
    x = rng.normal(size=(T, B, C)).astype(np.float32)
    xbuf, xv = _window(T * B, C, C + x_pad, x_off, float("nan"))
    xn = np.where(live[:, :, None], x, np.nan).astype(np.float32)
    xv.copy_(torch.from_numpy(xn.reshape(T * B, C)).cuda())
    ybuf, yv = _window(To * B, r * C, r * C + y_pad, y_off, SENTINEL)
    out = ops.time_reduce_fwd(xv, sl, T, B, r, out=yv)
    assert out is yv
    want = ref.np_time_reduce_fwd(xn, lens, r)
    got = yv.cpu().numpy().reshape(To, B, r * C)
    assert not np.isnan(got).any()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert _outside_untouched(ybuf, yv, SENTINEL)
    # ---- bwd: NaN in the parts of dy whose frame is dead and in its pad columns, sentinels around dx
    dy = rng.normal(size=(To, B, r * C)).astype(np.float32)
    part_live = (np.arange(To * r)[:, None] < n[None, :]).reshape(To, r, B).transpose(0, 2, 1)          # [To, B, r]
    dyn = np.where(np.repeat(part_live, C, axis=2), dy, np.nan).astype(np.float32)
    dybuf, dyv = _window(To * B, r * C, r * C + y_pad, y_off, float("nan"))
    dyv.copy_(torch.from_numpy(dyn.reshape(To * B, r * C)).cuda())
    dxbuf, dxv = _window(T * B, C, C + x_pad, x_off, SENTINEL)
    ops.time_reduce_bwd(dyv, sl, T, B, r, out=dxv)
    want_dx = ref.np_time_reduce_bwd(dyn, lens, r, T)
    got_dx = dxv.cpu().numpy().reshape(T, B, C)
    assert not np.isnan(got_dx).any()
    assert np.array_equal(got_dx.view(np.uint32), want_dx.view(np.uint32))
    assert _outside_untouched(dxbuf, dxv, SENTINEL)
    # ---- fwd then bwd: the identity on live frames, +0 elsewhere
    back = ops.time_reduce_bwd(yv, sl, T, B, r).cpu().numpy().reshape(T, B, C)
    assert np.array_equal(back.view(np.uint32), np.where(live[:, :, None], x, np.float32(0)).astype(np.float32).view(np.uint32))


SHAPES = {   # name -> (T, B, C, r)
    "scalar_odd_T": (7, 8, 5, 2),
    "vec16": (8, 8, 8, 2),
    "r3": (10, 8, 12, 3),
    "r4": (9, 8, 4, 4),
    "T_below_r_2": (1, 8, 4, 2),
    "T_below_r_4": (3, 8, 4, 4),
    "C1": (7, 8, 1, 2),
    "C1028": (5, 8, 1028, 2),           # 257 vectors: more than a workgroup's 256 lanes (64 lanes by the fewest-idle rule)
    "C4100": (3, 8, 4100, 2),           # 1025 vectors: 256 lanes, five passes - the four-in-flight copy loop and its remainder
    "B3": (7, 3, 5, 2),                 # the issue's shapes at their own B: the lengths are cut to the first B of the list
    "B4": (8, 4, 8, 2),
    "B2": (10, 2, 12, 3),
    "B5": (9, 5, 4, 4),
}


@pytest.mark.parametrize("case", sorted(SHAPES))
def test_passes_equal_the_numpy_statement_bit_for_bit(case):
    T, B, C, r = SHAPES[case]
    lens = _lens(T, r, max(B, 8))
    if B < 8:                           # narrow batches: walk the eight lengths in windows of B
        for lo in range(0, 8, B):
            sub = np.resize(lens[lo:lo + B], B).astype(np.int32)
            _run(T, B, C, r, sub)
    else:
        _run(T, B, C, r, lens)


@pytest.mark.parametrize("case", ["base_off_by_one_float", "pitch_C_plus_1", "both_sides_padded_vec"])
def test_unaligned_bases_and_odd_pitches_take_the_scalar_path_and_stay_exact(case):
    T, B, C, r = 9, 8, 8, 2
    lens = _lens(T, r, B)
    if case == "base_off_by_one_float":
        _run(T, B, C, r, lens, x_off=1)
        _run(T, B, C, r, lens, y_off=1)
    elif case == "pitch_C_plus_1":
        _run(T, B, C, r, lens, x_pad=1)
        _run(T, B, C, r, lens, y_pad=1)
    else:                               # pitches that stay multiples of 4: the 16-byte path through column windows
        _run(T, B, C, r, lens, x_pad=4, y_pad=8)


def test_more_segments_than_one_sweep_of_the_grid():
    """(4, 70000, 4, 2): 280000 segments of one float4 each against GRID_CAP * 64 = 131072 per sweep - the grid stride runs."""
    T, B, C, r = 4, 70000, 4, 2
    assert T * B > ONE_SWEEP and ref.cdiv(T, r) * B * r > ONE_SWEEP
    _run(T, B, C, r, _lens(T, r, B))


def test_bad_arguments_leave_the_outputs_alone():
    from lstm_ctc_amd import _lib
    lib = _lib.load()
    T, B, C, r = 7, 3, 8, 2
    To = 4
    x = torch.full((T * B, C), SENTINEL, device="cuda")
    y = torch.full((To * B, r * C), SENTINEL, device="cuda")
    sl = torch.tensor([7, 3, 0], dtype=torch.int32, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731

    def fwd(x_=P(x), ldx=C, T=T, B=B, C=C, r=r, s=P(sl), y_=P(y), ldy=r * C):
        return lib.lc_time_reduce_fwd(x_, ldx, T, B, C, r, s, y_, ldy, None)

    def bwd(dy=P(y), lddy=r * C, T=T, B=B, C=C, r=r, s=P(sl), dx=P(x), lddx=C):
        return lib.lc_time_reduce_bwd(dy, lddy, T, B, C, r, s, dx, lddx, None)

    inside_x = ctypes.c_void_p(x.data_ptr() + 16)
    for kw in (dict(T=0), dict(B=0), dict(C=0), dict(r=1), dict(r=5), dict(x_=None), dict(s=None), dict(y_=None), dict(ldx=C - 1),
               dict(ldy=r * C - 1), dict(y_=P(x)), dict(y_=inside_x)):
        assert fwd(**kw) == -1, kw
    for kw in (dict(T=0), dict(B=0), dict(C=0), dict(r=1), dict(r=5), dict(dy=None), dict(s=None), dict(dx=None), dict(lddx=C - 1),
               dict(lddy=r * C - 1), dict(dx=P(y)), dict(dy=inside_x)):
        assert bwd(**kw) == -1, kw
    torch.cuda.synchronize()
    assert bool((x == SENTINEL).all()) and bool((y == SENTINEL).all())
    with pytest.raises(ValueError):
        from lstm_ctc_amd import ops
        ops.time_reduce_fwd(x, sl, T, B, 5)
