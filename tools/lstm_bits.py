"""Bit record of the lc_lstm_* entries: every Case of tests/test_lstm_edges_host.py (variant a: mixed lengths, peepholes in
direction 0, 1e30 in the dead frames), forward then backward through the case's own entry, one SHA-256 per output tensor -
gates, cs, hs, dz, dpeep, dbias, and the shadows the entry can write (hs_bf16 / dz_bf16 of the bf16 entries, the x3 shadow of
dz of lc_lstm_bwd_x3) -, a line per direction with the first 16 hex digits of each and a last line with the SHA-256 over all of
them at full length.  Two builds of the library compute the same bits when their outputs are identical:

    python tools/lstm_bits.py > a.txt;  python tools/lstm_bits.py --lib other/liblstm_ctc_hip.so > b.txt;  cmp a.txt b.txt

Needs a GPU.  Every case has T <= 6; the whole list takes a few seconds."""
import argparse
import ctypes
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from lstm_ctc_amd import _lib  # noqa: E402
from test_lstm_edges_host import ALL_CASES, FORGET_BIAS, Problem, case_id  # noqa: E402

FWD = {"f32": "lc_lstm_fwd", "x3": "lc_lstm_fwd_x3", "bf16": "lc_lstm_fwd_bf16"}
BWD = {"f32": "lc_lstm_bwd", "x3": "lc_lstm_bwd_x3", "bf16": "lc_lstm_bwd_bf16"}


ALL = hashlib.sha256()


def sha(t):
    h = hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()
    ALL.update(h.encode())
    return h


def run_case(lib, c):
    p = Problem(c, "a")
    T, B, N = c.T, c.B, c.N
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    nan = lambda *shape: torch.full(shape, float("nan"), device="cuda")
    seq = dev(p.seq)
    stream = torch.cuda.current_stream().cuda_stream
    bufs, f, b = [], (_lib.LstmFwdDir * 2)(), (_lib.LstmBwdDir * 2)()
    for i, dd in enumerate(p.dirs):
        d = dict(zx=dev(p.poisoned("zx", i)), R=dev(dd["R"]), RT=dev(dd["R"].T), dh=dev(p.poisoned("dh", i)), cs=nan(T, B, N),
                 hs=nan(T, B, N), w=None if dd["w"] is None else dev(np.stack(dd["w"])), dpeep=dev(dd["dpeep0"]),
                 dbias=dev(dd["dbias0"]))
        if c.entry == "bf16":
            d["hs_bf16"] = torch.full((T, B, N), -1, dtype=torch.int16, device="cuda")
        if c.entry != "f32":                       # bf16: [T, B, 4N] bf16 copy of dz; x3: its three-term split, [T * B, 12 N]
            d["dz_bf16"] = torch.full((T * B, (12 if c.entry == "x3" else 4) * N), -1, dtype=torch.int16, device="cuda")
        f[i].zx, f[i].R, f[i].cs, f[i].hs = (d[k].data_ptr() for k in ("zx", "R", "cs", "hs"))
        b[i].gates, b[i].RT, b[i].cs, b[i].dh = (d[k].data_ptr() for k in ("zx", "RT", "cs", "dh"))
        if d["w"] is not None:
            f[i].w_f, f[i].w_i, f[i].w_o = (d["w"][k].data_ptr() for k in range(3))
            b[i].w_f, b[i].w_i, b[i].w_o = f[i].w_f, f[i].w_i, f[i].w_o
        b[i].dpeep, b[i].dbias = d["dpeep"].data_ptr(), d["dbias"].data_ptr()
        f[i].reverse = b[i].reverse = dd["reverse"]
        f[i].hs_bf16 = d["hs_bf16"].data_ptr() if "hs_bf16" in d else None
        b[i].dz_bf16 = d["dz_bf16"].data_ptr() if "dz_bf16" in d else None
        bufs.append(d)
    ws_f = torch.zeros(lib.lc_lstm_fwd_workspace_bytes(B, N, c.ndir), dtype=torch.uint8, device="cuda")
    ws_b = torch.zeros(lib.lc_lstm_bwd_workspace_bytes(B, N, c.ndir), dtype=torch.uint8, device="cuda")
    lib.lc_set_option(b"lstm_persistent", _lib.OPTION_UNSET if c.persistent else 0)
    try:
        _lib.check(getattr(lib, FWD[c.entry])(ctypes.cast(f, ctypes.c_void_p), c.ndir, seq.data_ptr(), T, B, N, FORGET_BIAS,
                                              ws_f.data_ptr(), ws_f.numel(), stream), FWD[c.entry])
        word_f = lib.lc_debug_last_lstm_schedule()
        torch.cuda.synchronize()
        out = [dict(gates=sha(d["zx"]), cs=sha(d["cs"]), hs=sha(d["hs"])) for d in bufs]
        _lib.check(getattr(lib, BWD[c.entry])(ctypes.cast(b, ctypes.c_void_p), c.ndir, seq.data_ptr(), T, B, N, ws_b.data_ptr(),
                                              ws_b.numel(), stream), BWD[c.entry])
        word_b = lib.lc_debug_last_lstm_schedule()
        torch.cuda.synchronize()
    finally:
        lib.lc_set_option(b"lstm_persistent", _lib.OPTION_UNSET)
    status = [int(w[_lib.LSTM_STATUS_OFFSET:_lib.LSTM_STATUS_OFFSET + 4].view(torch.int32).item()) for w in (ws_f, ws_b)]
    print("%s schedule fwd=0x%x bwd=0x%x status=%d,%d" % (case_id(c), word_f, word_b, status[0], status[1]))
    for i, d in enumerate(bufs):
        out[i].update(dz=sha(d["zx"]), dpeep=sha(d["dpeep"]), dbias=sha(d["dbias"]))
        out[i].update({k: sha(d[k]) for k in ("hs_bf16", "dz_bf16") if k in d})
        print("  dir%d %s" % (i, " ".join("%s=%s" % (k, v[:16]) for k, v in out[i].items())))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", help="another build of liblstm_ctc_hip.so to load instead of the tree's")
    args = ap.parse_args()
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    lib = _lib.load()
    for c in ALL_CASES:
        run_case(lib, c)
    print("sha256 over every tensor's sha256: %s" % ALL.hexdigest())


if __name__ == "__main__":
    main()
