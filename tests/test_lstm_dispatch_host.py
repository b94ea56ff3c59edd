"""The host-side dispatch of csrc/lstm.hip (from `al256` to the end of the file), checked without a GPU.

tests/lstm_dispatch_dump.cpp includes lstm.hip with every HIP call of the dispatch replaced by a recorder and calls the six
lc_lstm_* entries and the two workspace-size functions over a fixed list: every Case of test_lstm_edges_host.py in both passes,
the shapes of its dispatch-edge test, the pointer / option variants of one representative per schedule, the x3 shadow on either
side of its 32-bit limit, every refusal, and a grid of workspace sizes.  A record holds the entry's arguments, every memset,
LDS attribute, stream / event call and launch in order (a kernel by its mangled device name, with grid, block, LDS bytes, stream
and every field of its argument block), the return code, lc_last_error() and lc_debug_last_lstm_schedule() behind the call.
The cases, the x3 limit and the failure paths are in the file whole; the calls that repeat those launches with a shape or one
input changed (edges, variants, refusals) as the entry line, the result and a 64-bit digest of the whole record.  When a digest
differs, run the program this test builds with `--full` behind the answers on both trees and compare the two outputs.

persist_device_ok() and dir_streams() cache per process, so the program takes the fake device's answers on its command line
and runs once per answer set (ANSWER_SETS).  tests/golden/lstm_dispatch.txt is the output from the lstm.hip in front of the
refactor that put one schedule plan under the six entries; the dispatch may be reshaped freely as long as every call still
makes the same HIP calls with the same arguments - byte for byte.  A change that is MEANT to alter a launch regenerates the
golden file (``python tests/test_lstm_dispatch_host.py > tests/golden/lstm_dispatch.txt``) and says so."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "lstm_ctc_amd", "csrc")
MI355X = ["gfx950:sramecc+:xnack-", "256", "8"]
# name, then: arch string, CUs, XCCs, stream priority range degenerate, caller stream's priority, hipFuncSetAttribute fails,
# hipMemsetAsync fails
ANSWER_SETS = [("mi355x", MI355X + ["0", "0", "0", "0"]),
               ("not_an_mi355x", ["gfx942:sramecc+:xnack-", "304", "8", "0", "0", "0", "0"]),
               ("no_second_stream", MI355X + ["1", "0", "0", "0"]),
               ("caller_stream_at_high_priority", MI355X + ["0", "-1", "0", "0"]),
               ("func_attribute_fails", MI355X + ["0", "0", "1", "0"]),
               ("memset_fails", MI355X + ["0", "0", "0", "1"])]


def build(exe):
    """(error.cpp as plain C++: a second HIP translation unit would ask the linker for a device image of its own)"""
    subprocess.run([HIPCC, "--cuda-host-only", "-std=c++17", "-O1", "-I", CSRC, "-x", "hip",
                    os.path.join(ROOT, "tests", "lstm_dispatch_dump.cpp"), "-x", "c++", os.path.join(CSRC, "error.cpp"),
                    "-o", str(exe)], check=True, capture_output=True, timeout=600)


def record(exe):
    got = b""
    for name, answers in ANSWER_SETS:
        got += ("== %s: %s\n" % (name, " ".join(answers))).encode()
        got += subprocess.run([str(exe)] + answers, check=True, capture_output=True, timeout=120).stdout
    return got


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    exe = tmp_path_factory.mktemp("lstm_dispatch") / "lstm_dispatch_dump"
    build(exe)
    return exe


def test_every_call_does_what_the_golden_record_says(dump):
    got = record(dump)
    want = open(os.path.join(ROOT, "tests", "golden", "lstm_dispatch.txt"), "rb").read()
    if got != want:
        g, w = got.split(b"\n"), want.split(b"\n")
        first = next((i for i, (a, b) in enumerate(zip(g, w)) if a != b), min(len(g), len(w)))
        entry = next((w[i] for i in range(min(first, len(w) - 1), -1, -1) if w[i].startswith((b"lc_", b"=="))), b"")
        pytest.fail("record differs from tests/golden/lstm_dispatch.txt at line %d (%d lines against %d)\n  in:   %s\n  want: %s\n"
                    "  got:  %s" % (first + 1, len(g), len(w), entry.decode(), (w[first] if first < len(w) else b"<end>").decode(),
                                    (g[first] if first < len(g) else b"<end>").decode()))
    assert got.count(b"\nlc_lstm_") > 350 and got.count(b"\n  launch ") > 250 and got.count(b" record=") > 200
    assert got.count(b"\nworkspace_bytes(") == 12 and got.count(b"/") == 12 * 15
    for word in (b"0x1\n", b"0x10002\n", b"0x203\n", b"0x104\n", b"0x5\n", b"0x6\n", b"0x7\n", b"0x60006\n", b"0x60007\n"):
        assert b"schedule=" + word in got, word          # the whole records reach every schedule, and the in-kernel x3 shadow


def test_the_restated_rule_is_the_library_s_plan(dump):
    """``expected`` of test_lstm_edges_host.py (the dispatch restated in Python, which the GPU edge tests hold the library to)
    against the schedule word the library's own plan gives on an MI355X, without a GPU: every Case in both passes, and a grid
    around each boundary that module's docstring names - T = 3 / 4, B at 8 / ndir * 16 and one more, N = 512 / 528 / 544,
    the four XCD-pair widths and their neighbours, T * B * 4N * 4 at 2^32 and one frame less, Bpad 32 / 64 / 128, and the
    launch train's `< 200` workgroup thresholds (reached with lstm_persistent off)."""
    from lstm_ctc_amd.ops import decode_lstm_schedule
    from test_lstm_edges_host import ALL_CASES, expected
    shapes = [(c.entry, p, c.T, c.B, c.N, c.ndir, int(c.persistent)) for c in ALL_CASES for p in ("fwd", "bwd")]
    widths = [512, 528, 544] + [n + d for n in (640, 768, 896, 1024) for d in (-16, 0, 16)] + [784, 800, 816, 1584, 1600, 1616]
    for entry in ("f32", "x3", "bf16"):
        for p in ("fwd", "bwd"):
            shapes += [(entry, p, T, B, N, ndir, on) for N in widths if entry != "bf16" or N % 32 == 0 for T in (3, 4)
                       for B in (16, 17, 32, 33, 64, 65, 128, 129) for ndir in (1, 2) for on in (1, 0)]
            shapes += [(entry, p, T, B, 1024, ndir, 1) for T, B in ((4, 2 ** 16), (7, 37449)) for ndir in (1, 2)]
    lines = "".join("%s %s %d %d %d %d %d\n" % s for s in shapes)
    got = subprocess.run([str(dump)] + ANSWER_SETS[0][1] + ["--plan"], input=lines.encode(), check=True, capture_output=True,
                         timeout=120).stdout.decode().splitlines()
    assert len(got) == len(shapes) > 6000
    kinds = set()
    for s, line in zip(shapes, got):
        f = line.split()
        assert tuple(f[:2]) == s[:2] and tuple(map(int, f[2:7])) == s[2:] and len(f) == 8, line      # (no error text follows)
        want = expected(s[0], s[1], s[2], s[3], s[4], s[5], bool(s[6]))
        assert decode_lstm_schedule(int(f[7], 16)) == want, (s, f[7], want)
        kinds.add((want["kind"], want["mt"], want["backward"]))
    assert len({k for k, _, _ in kinds}) == 7 and {m for k, m, _ in kinds if k == "launch_train"} == {1, 2, 4}


if __name__ == "__main__":       # regenerate: python tests/test_lstm_dispatch_host.py > tests/golden/lstm_dispatch.txt
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        build(os.path.join(tmp, "lstm_dispatch_dump"))
        sys.stdout.buffer.write(record(os.path.join(tmp, "lstm_dispatch_dump")))
