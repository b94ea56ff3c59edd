"""The output BITS of lc_xent_loss, lc_kd_loss and lc_consistency_loss, pinned: tests/golden/frame_loss_bits.json holds the
SHA-256 of every output (loss, frames, agree / correct and the whole gradient tensor) of the cases that
tests/golden/make_frame_loss_bits.py builds - every step of the V ladder in both access widths, one row per wave, lengths that
leave whole waves unscored, special rows, overwrite / accumulate / no gradient, buffers off the 16-byte boundary and more
frames than one pass of the grid.  The file was generated on the library BEFORE the three criteria moved onto one skeleton
(csrc/row_group.h); the kernels are bit-reproducible, so equality is the whole assertion.  A change that means to alter the
arithmetic regenerates the file and says so."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from make_frame_loss_bits import OUT, cases, run_case  # noqa: E402

CASES = cases()
with open(OUT) as _fh:
    EXPECTED = json.load(_fh)


def test_the_fixture_holds_exactly_the_generator_s_cases():
    assert sorted(EXPECTED) == sorted(cid for cid, _ in CASES)


@pytest.mark.gpu
@pytest.mark.parametrize("cid,spec", CASES, ids=[cid for cid, _ in CASES])
def test_every_output_bit_is_where_it_was(cid, spec):
    got = run_case(spec)
    want = EXPECTED[cid]
    assert sorted(got) == sorted(want)
    wrong = [(run, k) for run in sorted(want) for k in sorted(want[run]) if got[run].get(k) != want[run][k]]
    assert not wrong, "%s: outputs whose bits moved: %s" % (cid, wrong)
