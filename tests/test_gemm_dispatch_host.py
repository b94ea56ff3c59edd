"""The host-side dispatch of csrc/gemm.hip, checked without a GPU (hipcc compiles the host half alone).

tests/gemm_dispatch_dump.cpp includes gemm.hip with the launch macro replaced by a recorder and calls every lc_gemm_* entry
over a fixed list of shapes, alignments, workspaces, epilogues and options: each record holds the entry's arguments, every
launch's kernel expression, grid, block and argument block, the split-K reduction's arguments, and the return code with
lc_last_error().  tests/golden/gemm_dispatch.txt is that output from the gemm.hip in front of the refactor that gave the
dispatch one K-split plan, one strip peel and one reduction launch; the dispatch may be reshaped freely as long as every
product still launches the same kernels with the same arguments - byte for byte.  A change that is MEANT to alter a launch
regenerates the golden file (run the program this test builds) and says so."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "lstm_ctc_amd", "csrc")


def test_every_product_launches_what_the_golden_record_says(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    exe = tmp_path / "gemm_dispatch_dump"
    subprocess.run([HIPCC, "--cuda-host-only", "-x", "hip", "-std=c++17", "-O1", "-I", CSRC,
                    os.path.join(ROOT, "tests", "gemm_dispatch_dump.cpp"), os.path.join(CSRC, "error.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=600)
    got = subprocess.run([str(exe)], check=True, capture_output=True, timeout=120).stdout
    want = open(os.path.join(ROOT, "tests", "golden", "gemm_dispatch.txt"), "rb").read()
    if got != want:
        g, w = got.split(b"\n"), want.split(b"\n")
        first = next((i for i, (a, b) in enumerate(zip(g, w)) if a != b), min(len(g), len(w)))
        entry = next((w[i] for i in range(min(first, len(w) - 1), -1, -1) if w[i].startswith(b"lc_")), b"")
        pytest.fail("record differs from tests/golden/gemm_dispatch.txt at line %d (%d lines against %d)\n  in:   %s\n  want: %s\n"
                    "  got:  %s" % (first + 1, len(g), len(w), entry.decode(), (w[first] if first < len(w) else b"<end>").decode(),
                                    (g[first] if first < len(g) else b"<end>").decode()))
    assert got.count(b"\nlc_") > 300 and got.count(b"launch splitk_reduce_kernel") > 40      # the list ran, splits included
