"""nnet.frames.FrameMap (host arithmetic, no GPU): the packed <-> padded row maps of a ragged batch against a brute-force
loop, for every order of lengths the callers produce."""
import numpy as np
import pytest


def _brute(seq_len, T, B):
    """packed row -> padded row, time-major over the live (t, b)."""
    out = []
    for t in range(T):
        for b in range(B):
            if t < min(int(seq_len[b]), T):
                out.append(t * B + b)
    return out


CASES = {
    "ascending": ([3, 5, 5, 8, 9], 9),
    "descending": ([9, 8, 5, 5, 3], 9),
    "unsorted": ([4, 9, 1, 7, 7, 2], 9),
    "zero_length": ([6, 0, 4, 0, 6], 6),
    "above_T": ([12, 3, 7], 7),                      # clipped to T
    "all_full": ([5, 5, 5, 5], 5),
    "b1": ([4], 6),
    "b1_full": ([6], 6),
    "more_than_a_tile": (list(range(1, 41)), 40),    # M = 820: four tiles, a tail of 204
    "nothing_live": ([0, 0, 0], 4),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_frame_map_against_brute_force(case):
    from lstm_ctc_amd.nnet.frames import FrameMap
    seq_len, T = CASES[case]
    B = len(seq_len)
    fm = FrameMap(np.asarray(seq_len, np.int32), T, B)
    want = _brute(seq_len, T, B)
    assert fm.M == len(want) == sum(min(n, T) for n in seq_len)
    assert fm.Mp % 256 == 0 and fm.M <= fm.Mp < fm.M + 256
    assert fm.rows.dtype == np.int32 and fm.rows.shape == (fm.Mp,)
    assert fm.inverse.dtype == np.int32 and fm.inverse.shape == (T * B,)
    assert fm.rows[:fm.M].tolist() == want
    assert np.all(fm.rows[fm.M:] == -1)
    # inverse to each other on live frames, -1 elsewhere
    live = np.zeros(T * B, bool)
    live[want] = True
    assert np.all(fm.inverse[~live] == -1)
    assert np.array_equal(fm.inverse[fm.rows[:fm.M]], np.arange(fm.M))
    assert np.array_equal(fm.rows[fm.inverse[live]], np.flatnonzero(live))
    assert fm.full == (fm.M == T * B) == (case in ("all_full", "b1_full"))
    # time-major: a step's live rows are ONE contiguous run of the packed matrix, b strictly increasing inside it
    at = 0
    for t in range(T):
        lo, hi = fm.step_run(t)
        assert lo == at and hi - lo == sum(1 for n in seq_len if t < min(n, T))
        run = fm.rows[lo:hi]
        assert np.all(run // B == t)
        assert np.all(np.diff(run) > 0)
        at = hi
    assert at == fm.M


def test_frame_map_accepts_any_integer_lengths_and_checks_B():
    from lstm_ctc_amd.nnet.frames import FrameMap
    a = FrameMap(np.asarray([3, 1, 2], np.int64), 3, 3)
    b = FrameMap([3, 1, 2], 3, 3)
    assert np.array_equal(a.rows, b.rows) and np.array_equal(a.inverse, b.inverse)
    assert a.rows[:a.M].tolist() == [0, 1, 2, 3, 5, 6]
    with pytest.raises(ValueError):
        FrameMap([3, 1], 3, 3)
    c = FrameMap([-2, 2], 2, 2)                        # a negative length is an empty utterance
    assert c.M == 2 and c.rows[:2].tolist() == [1, 3]


def test_library_version_and_pack_symbols_declared():
    """The two packed-frame exports are in the header and in the ctypes table (the .so side is
    test_host.py::test_library_loads_and_exports_every_declared_symbol), and the ABI version says so."""
    import os
    from lstm_ctc_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "lstm_ctc_hip.h")).read()
    for name in ("lc_pack_rows", "lc_unpack_rows"):
        assert name in _lib.SIGNATURES and ("int %s(" % name) in header
    if os.path.exists(_lib.LIB_PATH):
        assert _lib.load().lc_version() >= 2
