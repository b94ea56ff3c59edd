"""Tensor-level wrappers over the C ABI (include/lstm_ctc_hip.h).

PyTorch is used here for device memory and streams only: every function takes CUDA(ROCm) float32 /
int32 tensors, passes raw ``data_ptr()``s plus the current HIP stream to ``liblstm_ctc_hip.so``, and
returns tensors.  No arithmetic happens in torch on the product path, and nothing falls back to the
CPU: a missing library or a CPU tensor raises.
"""
import ctypes
import threading

import numpy as np
import torch

from . import _lib

_workspaces = {}

# Optional live profiling (bench.py): when PROFILE is a list, every GEMM / CTC call is bracketed by HIP
# events on the launch stream and (kind, work, start_event, end_event) is appended; work = flops or bytes.
PROFILE = None


def _prof_begin():
    if PROFILE is None:
        return None
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


def _prof_end(kind, work, start):
    if start is not None:
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        PROFILE.append((kind, work, start, e))


def _require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise _lib.LibraryError("lstm_ctc_amd ops need GPU tensors (got a CPU tensor); there is no CPU path")


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def workspace(name, nbytes, device):
    """A cached, grow-only scratch buffer (the library never allocates)."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:                    # "cuda" and "cuda:0" are the same buffer
        device = torch.device("cuda", torch.cuda.current_device())
    key = (name, str(device), torch.cuda.current_stream(device).cuda_stream)      # one scratch buffer per stream
    buf = _workspaces.get(key)
    if buf is None or buf.numel() < nbytes:
        new = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        if name == "lstm":
            # the first 256 bytes are the control block with the sticky status word (lstm_ctc_hip.h): it survives growth
            if buf is None:
                new[:256].zero_()
            else:
                new[:256].copy_(buf[:256])
        buf = new
        _workspaces[key] = buf
    return buf


def lstm_status(device):
    """int32 view [1] of the sticky status word of this stream's LSTM workspace (LC_LSTM_STATUS_OFFSET): non-zero after
    a persistent-recurrence launch could not complete (its outputs are NaN).  Zero it at the start of a step, read it
    at the step's sync point; get the view AFTER the step's last lstm call (the workspace may have grown)."""
    buf = workspace("lstm", 256, device)
    o = _lib.LSTM_STATUS_OFFSET
    return buf[o:o + 4].view(torch.int32)


def debug_spin(blocks, microseconds, lds_bytes=96 * 1024):
    """Development hook (lc_debug_spin): `blocks` idle workgroups, each holding `lds_bytes` of LDS, resident for `microseconds`
    on the CURRENT stream - a foreign kernel for the co-residency tests (96 KB: no persistent recurrence fits beside one)."""
    _lib.check(_lib.load().lc_debug_spin(int(blocks), int(microseconds), int(lds_bytes), _stream()), "lc_debug_spin")


def set_option(name, value=None):
    """Per-thread override of a library development switch (lc_set_option; None clears it)."""
    _lib.check(_lib.load().lc_set_option(name.encode(), _lib.OPTION_UNSET if value is None else int(value)),
               "lc_set_option")


def get_option(name):
    """Effective value of a switch (override, else its LC_* environment variable), or None for the library default."""
    v = ctypes.c_long(0)
    _lib.check(_lib.load().lc_get_option(name.encode(), ctypes.byref(v)), "lc_get_option")
    return None if v.value == _lib.OPTION_UNSET else int(v.value)


_tls = threading.local()


class force_launch_train:
    """Context: every lstm_fwd / lstm_bwd issued by THIS thread inside runs the per-step launch train - the checked
    fallback of the persistent schedules.  A per-thread library override (lc_set_option "lstm_persistent"), not an
    environment mutation: loader threads that read os.environ are never raced."""

    def __enter__(self):
        self._outer = getattr(_tls, "launch_train_depth", 0)
        _tls.launch_train_depth = self._outer + 1
        set_option("lstm_persistent", 0)

    def __exit__(self, *exc):
        _tls.launch_train_depth = self._outer
        if self._outer == 0:
            set_option("lstm_persistent", None)


def decode_lstm_schedule(v):
    """The schedule word of lc_debug_last_lstm_schedule() as dict(kind, mt, bf16, backward, dz_shadow_in_kernel)."""
    kinds = {0: "none", 1: "persistent_f32", 2: "persistent_bf16", 3: "two_stream_train", 4: "launch_train",
             5: "persistent_f32_xcd_pair", 6: "persistent_x3_xcd_pair", 7: "persistent_x3"}
    return dict(kind=kinds.get(v & 0xff, "?"), mt=(v >> 8) & 0xff, bf16=bool(v >> 16 & 1), backward=bool(v >> 17 & 1),
                dz_shadow_in_kernel=bool(v >> 18 & 1))


def last_lstm_schedule():
    """Decoded lc_debug_last_lstm_schedule() of this thread's last accepted lc_lstm_* call."""
    return decode_lstm_schedule(_lib.load().lc_debug_last_lstm_schedule())


def last_ctc_path():
    """Decoded lc_debug_last_ctc_path(): dict(path, ppl, nw, kg, lse2, g) of this thread's last successful ctc_loss."""
    v = _lib.load().lc_debug_last_ctc_path()
    paths = {0: "none", 1: "two_launch", 2: "three_kernel"}
    return dict(path=paths.get(v & 0xf, "?"), ppl=(v >> 4) & 0x3f, nw=(v >> 10) & 0xf, kg=(v >> 14) & 0xf,
                lse2=bool(v >> 18 & 1), g=(v >> 19) & 0x7f)


def _f32c(t):
    assert t.dtype == torch.float32, t.dtype
    return t if t.is_contiguous() else t.contiguous()


def _ld(t):
    """Leading dimension of a 2-D view whose last stride is 1: its row stride - which torch leaves arbitrary on a single row,
    so there at least the row's width."""
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


def _rowmajor2d(t):
    assert t.dim() == 2 and t.dtype == torch.float32
    if t.stride(1) != 1:
        t = t.contiguous()
    return t, _ld(t)


# ------------------------------------------------------------------------------------------ GEMM
class Epilogue:
    """Fused finish of ONE product (lc_gemm_next_epilogue): the dropout mask of stream ``stream0 + col // width`` applied
    to the output, and / or its bf16 shadow ``shadow`` ([M,N] bf16 view, last stride 1) written in the same pass."""

    def __init__(self, keep=1.0, seed=0, stream0=0, width=1, shadow=None, shadow_only=False):
        self.keep, self.seed, self.stream0, self.width, self.shadow = float(keep), int(seed), int(stream0), int(width), shadow
        self.shadow_only = bool(shadow_only) and shadow is not None      # the fp32 output is left untouched (nobody reads it)


def _arm(lib, epilogue, out):
    """Arms the calling thread's next lc_gemm_* call; call it RIGHT before that call (nothing between may fail)."""
    if epilogue is None:
        return
    sh = epilogue.shadow
    if sh is not None:
        _require_cuda(sh)
        assert sh.dtype == torch.bfloat16 and sh.shape == out.shape and sh.stride(1) == 1
    e = _lib.GemmEpilogue(epilogue.keep, epilogue.seed & 0xFFFFFFFF, epilogue.stream0, epilogue.width,
                          _ptr(sh), _ld(sh) if sh is not None else 0,
                          int(getattr(epilogue, "shadow_only", False)))
    _lib.check(lib.lc_gemm_next_epilogue(ctypes.byref(e)), "lc_gemm_next_epilogue")


def _product(name, kind, head, M, N, Ks, A, B, out, alpha, beta, bias, epilogue=None, dtype=torch.bfloat16, pool=None,
             nbytes=0):
    """out[M,N] = alpha * (what lc_<name> makes of A and B) + beta*out (+ bias): the one path under every product wrapper.
    A, B: tuples of 2-D `dtype` views with last stride 1 (dtype None: the caller has normalised them, _rowmajor2d) - one operand
    each, or the two of an nt2 product, which share their row stride.  The entry's arguments are head, M, N, Ks, alpha, A.., lda, B.., ldb, beta, out, ldc, bias, then the workspace
    if it takes one (pool: its name here; "gemm" is sized by lc_gemm_workspace_bytes, any other by nbytes), then the stream.
    sum(Ks) is the reduction depth of the FLOP count under the profiling kind."""
    lib = _lib.load()
    _require_cuda(*A, *B, out, bias)
    for t in A + B if dtype is not None else ():
        assert t.dim() == 2 and t.dtype == dtype and t.stride(1) == 1, (t.dtype, tuple(t.shape), t.stride())
    if out is None:
        assert beta == 0.0
        out = torch.empty((M, N), dtype=torch.float32, device=A[0].device)
    assert out.shape == (M, N) and out.stride(1) == 1 and out.dtype == torch.float32
    args = [*head, M, N, *Ks, alpha, *map(_ptr, A), _ld(A[0]), *map(_ptr, B), _ld(B[0]), beta, _ptr(out), _ld(out), _ptr(bias)]
    if pool is not None:
        if pool == "gemm":
            nbytes = lib.lc_gemm_workspace_bytes(M, N, sum(Ks))
        ws = workspace(pool, nbytes, A[0].device) if nbytes else None
        args += [_ptr(ws), nbytes]
    ev = _prof_begin()
    _arm(lib, epilogue, out)
    _lib.check(getattr(lib, name)(*args, _stream()), name)
    _prof_end(kind, 2.0 * M * N * sum(Ks), ev)
    return out


def gemm(A, B, ta=False, tb=False, out=None, alpha=1.0, beta=0.0, bias=None, bf16=False, epilogue=None):
    """out[M,N] = alpha * op(A) @ op(B) + beta*out (+ bias).  A/B/out are 2-D row-major views whose
    last stride is 1 (row stride free, so column slices of wider buffers are fine).
    bf16=True: operands rounded to bf16 on load, fp32 accumulate (lc_gemm_bf16; config c5)."""
    _require_cuda(A, B, out, bias)
    A, B = _rowmajor2d(A)[0], _rowmajor2d(B)[0]
    M, K = (A.shape[1], A.shape[0]) if ta else (A.shape[0], A.shape[1])
    K2, N = (B.shape[1], B.shape[0]) if tb else (B.shape[0], B.shape[1])
    assert K == K2, (A.shape, B.shape, ta, tb)
    name, kind = ("lc_gemm_bf16", "gemm_bf16") if bf16 else ("lc_gemm_f32", "gemm")
    return _product(name, kind, (int(ta), int(tb)), M, N, (K,), (A,), (B,), out, alpha, beta, bias, epilogue, dtype=None,
                    pool="gemm")


def transpose(x):
    lib = _lib.load()
    _require_cuda(x)
    x = _f32c(x)
    rows, cols = x.shape
    out = torch.empty((cols, rows), dtype=torch.float32, device=x.device)
    _lib.check(lib.lc_transpose(_ptr(x), rows, cols, _ptr(out), _stream()), "lc_transpose")
    return out


def colsum(x, out=None, accumulate=False):
    lib = _lib.load()
    _require_cuda(x, out)
    x, ldx = _rowmajor2d(x)
    rows, N = x.shape
    if out is None:
        out = torch.empty(N, dtype=torch.float32, device=x.device)
        accumulate = False
    nbytes = lib.lc_colsum_workspace_bytes(N)
    ws = workspace("colsum", nbytes, x.device)
    _lib.check(lib.lc_colsum(_ptr(x), rows, N, ldx, _ptr(out), int(accumulate), _ptr(ws), nbytes, _stream()),
               "lc_colsum")
    return out


def dropout_scale(x, keep, seed, stream_id, out=None, accumulate=False, shadow=None):
    """out (+)= x * Bernoulli(keep)/keep with the counter-based mask; x, out: 2-D [rows,P] views.  shadow: optional bf16
    [rows,P] view that receives the rounded result in the same pass (lc_dropout_scale_bf16)."""
    lib = _lib.load()
    _require_cuda(x, out, shadow)
    assert x.dim() == 2 and x.stride(1) == 1
    if out is None:
        out = x
    rows, P = x.shape
    if shadow is not None:
        assert shadow.dtype == torch.bfloat16 and shadow.shape == x.shape and shadow.stride(1) == 1
        ev = _prof_begin()
        _lib.check(lib.lc_dropout_scale_bf16(_ptr(x), rows, P, x.stride(0), float(keep), int(seed) & 0xFFFFFFFF,
                                             int(stream_id), _ptr(out), out.stride(0), int(accumulate), _ptr(shadow),
                                             shadow.stride(0), _stream()), "lc_dropout_scale_bf16")
        _prof_end("cast_bf16", float(rows) * P * 10, ev)       # bytes moved: 4 read + 4 + 2 written
        return out
    _lib.check(lib.lc_dropout_scale(_ptr(x), rows, P, x.stride(0), float(keep), int(seed) & 0xFFFFFFFF,
                                    int(stream_id), _ptr(out), out.stride(0), int(accumulate), _stream()),
               "lc_dropout_scale")
    return out


# ------------------------------------------------------------------------------------------ CTC
# The lattice entries of include/lstm_ctc_hip.h, by the wrapper that calls them: (C entry, its workspace query, workspace
# name, windows - None: the entry takes none, "required", "optional" - and whether a [B] output follows ``loss``).
_LATTICE = {
    "ctc_loss": ("lc_ctc_loss", "lc_ctc_workspace_bytes", "ctc", None, False),
    "ctc_loss_windowed": ("lc_ctc_loss_windowed", "lc_ctc_window_workspace_bytes", "ctc_window", "required", False),
    "ctc_loss_delay": ("lc_ctc_loss_delay", "lc_ctc_delay_workspace_bytes", "ctc_delay", "optional", True),
    "ctc_loss_entropy": ("lc_ctc_loss_entropy", "lc_ctc_entropy_workspace_bytes", "ctc_entropy", "optional", True),
    "ctc_loss_star": ("lc_ctc_loss_star", "lc_ctc_star_workspace_bytes", "ctc_star", "optional", True),
}


def _ctc_lattice_call(who, logits, labels, offsets, seq_len, max_label_len, win_lo=None, win_hi=None, scalars=(),
                      want_grad=True, want_extra=True):
    """The one body under the five CTC wrappers: ``who`` names the wrapper (its row of _LATTICE, and the errors' prefix),
    ``scalars`` are the floats the entry takes between win_hi and loss.  Returns (loss[B], extra[B] or None, grad[T,B,V] or
    None); extra is None as well for an entry that has none."""
    entry, query, pool, windows, has_extra = _LATTICE[who]
    lib = _lib.load()
    _require_cuda(logits, labels, offsets, seq_len, win_lo, win_hi)
    logits = _f32c(logits)
    T, B, V = logits.shape
    assert labels.dtype == torch.int32 and offsets.dtype == torch.int32 and seq_len.dtype == torch.int32
    if windows == "optional" and (win_lo is None) != (win_hi is None):
        raise ValueError("%s: win_lo and win_hi go together (both or none)" % who)
    if windows == "required" or win_lo is not None:
        assert win_lo.dtype == torch.int32 and win_hi.dtype == torch.int32
        if win_lo.numel() != labels.numel() or win_hi.numel() != labels.numel():
            raise ValueError("%s: win_lo / win_hi must be parallel to labels (%d, %d, %d elements)"
                             % (who, win_lo.numel(), win_hi.numel(), labels.numel()))
        win_lo, win_hi = win_lo.contiguous(), win_hi.contiguous()
    loss = torch.empty(B, dtype=torch.float32, device=logits.device)
    extra = torch.empty(B, dtype=torch.float32, device=logits.device) if has_extra and want_extra else None
    grad = torch.empty_like(logits) if want_grad else None
    nbytes = getattr(lib, query)(T, B, V, int(max_label_len))
    ws = workspace(pool, nbytes, logits.device)
    if labels.numel() == 0:                                                  # an empty vector has no address to pass
        labels = torch.zeros(1, dtype=torch.int32, device=logits.device)
        if win_lo is not None:
            win_lo = torch.zeros(1, dtype=torch.int32, device=logits.device)
            win_hi = torch.zeros(1, dtype=torch.int32, device=logits.device)
    args = [_ptr(logits), T, B, V, _ptr(labels), _ptr(offsets), _ptr(seq_len), int(max_label_len)]
    if windows is not None:
        args += [_ptr(win_lo), _ptr(win_hi)]
    args += [float(s) for s in scalars] + [_ptr(loss)] + ([_ptr(extra)] if has_extra else []) + [_ptr(grad), _ptr(ws), nbytes]
    ev = _prof_begin()
    _lib.check(getattr(lib, entry)(*args, _stream()), entry)
    _prof_end("ctc", (T, B, V), ev)
    return loss, extra, grad


def ctc_loss(logits, labels, offsets, seq_len, max_label_len, want_grad=True):
    """logits [T,B,V] f32; labels flat int32; offsets [B+1] int32; seq_len [B] int32 (all on device).
    Returns (loss[B], grad[T,B,V] or None)."""
    loss, _, grad = _ctc_lattice_call("ctc_loss", logits, labels, offsets, seq_len, max_label_len, want_grad=want_grad)
    return loss, grad


def ctc_loss_windowed(logits, labels, offsets, seq_len, max_label_len, win_lo, win_hi, want_grad=True):
    """Alignment-windowed CTC - no reference counterpart.  Arguments as for :func:`ctc_loss`, plus win_lo / win_hi: int32
    on the device, parallel to the flat labels; label j may sit on frame t only when win_lo[j] <= t <= win_hi[j] (values
    outside the utterance clip; see :func:`label_windows`).  Returns (loss[B], grad[T,B,V] or None) over the surviving paths;
    +inf and a softmax gradient where no path survives."""
    loss, _, grad = _ctc_lattice_call("ctc_loss_windowed", logits, labels, offsets, seq_len, max_label_len, win_lo, win_hi,
                                      want_grad=want_grad)
    return loss, grad


def ctc_loss_delay(logits, labels, offsets, seq_len, max_label_len, delay_penalty, win_lo=None, win_hi=None, want_grad=True,
                   want_entry=True):
    """Delay-penalised CTC - no reference counterpart.  Arguments as for :func:`ctc_loss`, plus delay_penalty (lambda, any
    finite float: a path is weighted by exp(-lambda * sum of the frames at which its labels are entered)) and, optionally,
    the windows of :func:`ctc_loss_windowed` (both or none).  Returns (loss[B], entry_sum[B] or None, grad[T,B,V] or None):
    entry_sum is the expected sum of the label entry frames under the penalised path posterior, = d loss / d lambda."""
    if isinstance(delay_penalty, bool) or not np.isfinite(delay_penalty):
        raise ValueError("ctc_loss_delay: delay_penalty must be a finite float, got %r" % (delay_penalty,))
    return _ctc_lattice_call("ctc_loss_delay", logits, labels, offsets, seq_len, max_label_len, win_lo, win_hi,
                             (delay_penalty,), want_grad, want_entry)


def ctc_loss_entropy(logits, labels, offsets, seq_len, max_label_len, entropy_weight, win_lo=None, win_hi=None, want_grad=True):
    """Maximum-entropy CTC (Liu et al. 2018) - no reference counterpart.  Arguments as for :func:`ctc_loss`, plus
    entropy_weight (eta, any finite float) and, optionally, the windows of :func:`ctc_loss_windowed` (both or none).
    Returns (loss[B], entropy[B], grad[T,B,V] or None): loss is plain (windowed) CTC's, entropy the entropy in nats of the
    posterior over the feasible paths, grad the exact gradient of ``loss - entropy_weight * entropy``."""
    if isinstance(entropy_weight, bool) or not np.isfinite(entropy_weight):
        raise ValueError("ctc_loss_entropy: entropy_weight must be a finite float, got %r" % (entropy_weight,))
    return _ctc_lattice_call("ctc_loss_entropy", logits, labels, offsets, seq_len, max_label_len, win_lo, win_hi,
                             (entropy_weight,), want_grad)


def ctc_loss_star(logits, labels, offsets, seq_len, max_label_len, bypass_penalty, selfloop_penalty, win_lo=None, win_hi=None,
                  want_grad=True):
    """Transcript-tolerant CTC (after OTC / STC) - no reference counterpart.  Arguments as for :func:`ctc_loss`, plus the two
    penalties (each a float >= 0 or +inf, which switches that star off) and, optionally, the windows of
    :func:`ctc_loss_windowed` (both or none).  Returns (loss[B], star_frames[B], grad[T,B,V] or None): loss is -log of the path
    sum over the lattice whose cells may explain a frame by the penalised star (it may be negative), star_frames the expected
    number of frames the star explains under the path posterior, grad the exact gradient of loss."""
    for name, p in (("bypass_penalty", bypass_penalty), ("selfloop_penalty", selfloop_penalty)):
        if isinstance(p, bool) or not p >= 0:                                   # NaN fails the comparison
            raise ValueError("ctc_loss_star: %s must be a float >= 0 or +inf, got %r" % (name, p))
    return _ctc_lattice_call("ctc_loss_star", logits, labels, offsets, seq_len, max_label_len, win_lo, win_hi,
                             (bypass_penalty, selfloop_penalty), want_grad)


WINDOW_OPEN = np.iinfo(np.int32).max


def label_windows(frame_target, flat, offsets, seq_len, tau, blank):
    """HOST function on numpy arrays: the windows :func:`ctc_loss_windowed` takes, from a frame-level alignment.
    frame_target [B,T] int32 is one symbol per frame as :func:`ctc_align` writes it (``blank`` on blank frames, -1 = no
    entry); flat / offsets are the flattened labels, seq_len [B] the frame counts.  Returns (win_lo, win_hi, constrained):
    two int32 vectors parallel to ``flat`` and a bool per utterance.

    For utterance b, take the maximal runs of equal non-blank symbols in frame_target[b, :seq_len[b]].  If the row holds no
    -1 and the runs' symbols spell the utterance's labels exactly (a valid CTC path separates equal neighbours by a blank,
    so runs and labels correspond one to one; no labels and an all-blank row qualify), label i gets
    [first frame of run i - tau, last frame of run i + tau].  Otherwise - an all -1 row, which is what the pipeline hands
    out for a missing or wrong-length entry, or any row that does not spell the labels - the utterance stays unconstrained
    (lo = 0, hi = INT32_MAX) and constrained[b] is False.  Never raises for content."""
    frame_target = np.asarray(frame_target)
    flat = np.asarray(flat).reshape(-1)
    offsets = np.asarray(offsets).reshape(-1)
    B = len(offsets) - 1
    tau = int(tau)
    lo = np.zeros(flat.shape[0], np.int32)
    hi = np.full(flat.shape[0], WINDOW_OPEN, np.int32)
    constrained = np.zeros(B, bool)
    T = frame_target.shape[1] if frame_target.ndim == 2 else 0
    for b in range(B):
        o0, o1 = int(offsets[b]), int(offsets[b + 1])
        n = min(max(int(seq_len[b]), 0), T)
        if frame_target.ndim != 2 or b >= frame_target.shape[0] or o1 < o0:
            continue
        row = frame_target[b, :n].astype(np.int64)
        if row.size and row.min() < 0:
            continue
        # run starts: a non-blank frame whose predecessor holds another symbol
        nb = row != blank
        start = nb.copy()
        start[1:] &= row[1:] != row[:-1]
        end = nb.copy()
        end[:-1] &= row[1:] != row[:-1]
        first, last = np.flatnonzero(start), np.flatnonzero(end)
        if len(first) != o1 - o0 or not np.array_equal(row[first], flat[o0:o1].astype(np.int64)):
            continue
        lo[o0:o1] = np.maximum(first - tau, np.iinfo(np.int32).min)
        hi[o0:o1] = np.minimum(last + tau, WINDOW_OPEN)
        constrained[b] = True
    return lo, hi, constrained


def ctc_align(logits, labels, offsets, seq_len, max_label_len, want_label_index=True):
    """Best-path (Viterbi) forced alignment - no reference counterpart.  Arguments as for :func:`ctc_loss`.
    Returns (ali [B,T] int32, label_index [B,T] int32 or None, score [B] f32) on the device: the symbol per frame
    (blank = V-1), the index into the utterance's labels (-1 on blank frames) and the best path's log-probability;
    -1 / -inf where an utterance has no path, -1 beyond seq_len."""
    lib = _lib.load()
    _require_cuda(logits, labels, offsets, seq_len)
    logits = _f32c(logits)
    T, B, V = logits.shape
    assert labels.dtype == torch.int32 and offsets.dtype == torch.int32 and seq_len.dtype == torch.int32
    ali = torch.empty((B, T), dtype=torch.int32, device=logits.device)
    lidx = torch.empty((B, T), dtype=torch.int32, device=logits.device) if want_label_index else None
    score = torch.empty(B, dtype=torch.float32, device=logits.device)
    nbytes = lib.lc_ctc_align_workspace_bytes(T, B, V, int(max_label_len))
    ws = workspace("ctc_align", nbytes, logits.device)
    if labels.numel() == 0:
        labels = torch.zeros(1, dtype=torch.int32, device=logits.device)
    _lib.check(lib.lc_ctc_align(_ptr(logits), T, B, V, _ptr(labels), _ptr(offsets), _ptr(seq_len), int(max_label_len),
                                _ptr(ali), _ptr(lidx), _ptr(score), _ptr(ws), nbytes, _stream()), "lc_ctc_align")
    return ali, lidx, score


def _frame_outputs(B, dev):
    """The [B] outputs of a frame loss: (loss f32, frames i32, a second count i32), uninitialised."""
    return (torch.empty(B, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.int32, device=dev),
            torch.empty(B, dtype=torch.int32, device=dev))


def _grad_to_fill(who, shape, logits, grad, want_grad):
    """(grad, accumulate) of kd_loss / consistency_loss: a given ``grad`` - contiguous float32 of the logits' shape, ``shape``
    in the error's words - is accumulated into (1); else (0) a new one is overwritten, or None without ``want_grad``."""
    if grad is not None:
        if grad.dtype != torch.float32 or grad.shape != logits.shape or not grad.is_contiguous():
            raise ValueError("%s: grad must be a contiguous float32 %s tensor to accumulate into" % (who, shape))
        return grad, 1
    return (torch.empty_like(logits) if want_grad else None), 0


def xent_loss(logits, targets, seq_len, want_grad=True):
    """Frame-level softmax cross-entropy - no reference counterpart.  logits [T,B,V] f32; targets [B,T] int32, one symbol
    per frame as :func:`ctc_align` writes them (the blank V-1 is a legal target, -1 = ignore); seq_len [B] int32.
    Returns (loss [B] f32, frames [B] int32, correct [B] int32, grad [T,B,V] or None) on the device: the summed
    -log_softmax[target] of the scored frames (t < seq_len[b], 0 <= target < V), their number, how many of them the
    argmax gets right, and d sum(loss) / d logits (zero rows on frames that are not scored)."""
    lib = _lib.load()
    _require_cuda(logits, targets, seq_len)
    logits = _f32c(logits)
    T, B, V = logits.shape
    assert targets.dtype == torch.int32 and seq_len.dtype == torch.int32
    if tuple(targets.shape) != (B, T) or seq_len.numel() != B:
        raise ValueError("xent_loss: targets must be [B, T] = [%d, %d] and seq_len [B] (got %s, %s)"
                         % (B, T, tuple(targets.shape), tuple(seq_len.shape)))
    targets = targets.contiguous()
    dev = logits.device
    loss, frames, correct = _frame_outputs(B, dev)
    grad = torch.empty_like(logits) if want_grad else None
    nbytes = lib.lc_xent_workspace_bytes(T, B, V)
    ws = workspace("xent", nbytes, dev)
    ev = _prof_begin()
    _lib.check(lib.lc_xent_loss(_ptr(logits), T, B, V, _ptr(targets), _ptr(seq_len), _ptr(loss), _ptr(frames),
                                _ptr(correct), _ptr(grad), _ptr(ws), nbytes, _stream()), "lc_xent_loss")
    _prof_end("xent", (T, B, V), ev)
    return loss, frames, correct, grad


def kd_loss(logits, teacher, seq_len, teacher_len, temperature=1.0, grad_scale=1.0, grad=None, want_grad=True):
    """Teacher-student distillation - no reference counterpart.  logits, teacher [T,B,V] f32 (teacher in the log domain;
    -inf = probability 0); seq_len, teacher_len [B] int32.  A frame is scored when t < min(seq_len[b], teacher_len[b]).
    Returns (loss [B] f32, frames [B] int32, agree [B] int32, grad) on the device: the summed KL(softmax(teacher / tau) ||
    softmax(logits / tau)) of the scored frames (not scaled), their number, how many of them have the two argmaxes
    coincide, and grad_scale * (q - p).  ``grad=None`` allocates a tensor and overwrites it (zero rows on frames that are
    not scored); a given tensor is accumulated into (rows that are not scored stay untouched); ``want_grad=False`` with
    ``grad=None`` computes no gradient and returns None."""
    lib = _lib.load()
    _require_cuda(logits, teacher, seq_len, teacher_len, grad)
    logits = _f32c(logits)
    teacher = _f32c(teacher)
    T, B, V = logits.shape
    assert seq_len.dtype == torch.int32 and teacher_len.dtype == torch.int32
    if tuple(teacher.shape) != (T, B, V) or seq_len.numel() != B or teacher_len.numel() != B:
        raise ValueError("kd_loss: teacher must be [T, B, V] = [%d, %d, %d], seq_len and teacher_len [B] (got %s, %s, %s)"
                         % (T, B, V, tuple(teacher.shape), tuple(seq_len.shape), tuple(teacher_len.shape)))
    grad, accumulate = _grad_to_fill("kd_loss", "[T, B, V]", logits, grad, want_grad)
    dev = logits.device
    loss, frames, agree = _frame_outputs(B, dev)
    nbytes = lib.lc_kd_workspace_bytes(T, B, V)
    ws = workspace("kd", nbytes, dev)
    ev = _prof_begin()
    _lib.check(lib.lc_kd_loss(_ptr(logits), _ptr(teacher), T, B, V, _ptr(seq_len.contiguous()), _ptr(teacher_len.contiguous()),
                              float(temperature), float(grad_scale), _ptr(loss), _ptr(frames), _ptr(agree), _ptr(grad),
                              accumulate, _ptr(ws), nbytes, _stream()), "lc_kd_loss")
    _prof_end("kd", (T, B, V), ev)
    return loss, frames, agree, grad


def consistency_loss(logits, seq_len, grad_scale=1.0, grad=None, want_grad=True):
    """Consistency-regularised CTC's pair term - no reference counterpart.  logits [T,2B,V] f32: column b is view a of pair b,
    column b + B its view b; seq_len [B] int32, one length per PAIR.  A pair-frame is scored when t < seq_len[b].  Returns
    (loss [B] f32, frames [B] int32, agree [B] int32, grad) on the device: the summed J = KL(qb || qa) + KL(qa || qb) of the
    scored pair-frames (not scaled), their number, how many of them have the two argmaxes coincide, and the STOP-GRADIENT
    rows grad_scale * (qa - qb) / grad_scale * (qb - qa) (each view a constant target for the other: not the derivative of
    J).  ``grad=None`` allocates a [T,2B,V] tensor and overwrites it (zero rows on pair-frames that are not scored); a given
    tensor is accumulated into (rows that are not scored stay untouched); ``want_grad=False`` with ``grad=None`` computes no
    gradient and returns None."""
    lib = _lib.load()
    _require_cuda(logits, seq_len, grad)
    logits = _f32c(logits)
    T, B2, V = logits.shape
    assert seq_len.dtype == torch.int32
    B = seq_len.numel()
    if B2 != 2 * B or B == 0:
        raise ValueError("consistency_loss: logits must be [T, 2B, V] for seq_len [B] (got %s, %s)"
                         % (tuple(logits.shape), tuple(seq_len.shape)))
    grad, accumulate = _grad_to_fill("consistency_loss", "[T, 2B, V]", logits, grad, want_grad)
    dev = logits.device
    loss, frames, agree = _frame_outputs(B, dev)
    nbytes = lib.lc_consistency_workspace_bytes(T, B, V)
    ws = workspace("consistency", nbytes, dev)
    ev = _prof_begin()
    _lib.check(lib.lc_consistency_loss(_ptr(logits), T, B, V, _ptr(seq_len.contiguous()), float(grad_scale), _ptr(loss),
                                       _ptr(frames), _ptr(agree), _ptr(grad), accumulate, _ptr(ws), nbytes,
                                       _stream()), "lc_consistency_loss")
    _prof_end("consistency", (T, B, V), ev)
    return loss, frames, agree, grad


def alignment_segments(ali, label_index, seq_len):
    """HOST function on numpy arrays: ali / label_index [B,T] and seq_len [B] as :func:`ctc_align` returns them ->
    per utterance a list of (label, start_frame, num_frames) runs of non-blank frames.  A run ends where label_index
    changes, so two equal labels in a row stay two segments."""
    ali, label_index = np.asarray(ali), np.asarray(label_index)
    out = []
    for b in range(ali.shape[0]):
        n = min(int(seq_len[b]), ali.shape[1])
        segs, start = [], None
        for t in range(n + 1):
            cur = int(label_index[b, t]) if t < n else -1
            if start is not None and cur != int(label_index[b, start]):
                segs.append((int(ali[b, start]), start, t - start))
                start = None
            if start is None and cur >= 0:
                start = t
        out.append(segs)
    return out


def ctc_greedy(logits, seq_len):
    """Returns (tokens [B,T] int32, out_len [B] int32) on device."""
    lib = _lib.load()
    _require_cuda(logits, seq_len)
    logits = _f32c(logits)
    T, B, V = logits.shape
    tokens = torch.empty((B, T), dtype=torch.int32, device=logits.device)
    out_len = torch.empty(B, dtype=torch.int32, device=logits.device)
    ws = workspace("greedy", 4 * T * B, logits.device)
    _lib.check(lib.lc_ctc_greedy(_ptr(logits), T, B, V, _ptr(seq_len), _ptr(tokens), _ptr(out_len), _ptr(ws),
                                 _stream()), "lc_ctc_greedy")
    return tokens, out_len


def edit_distance_host(tokens, token_len, truth_flat, truth_offsets):
    """Host-side Levenshtein per utterance (numpy int32 in, numpy int32 out)."""
    lib = _lib.load()
    tokens = np.ascontiguousarray(tokens, np.int32)
    token_len = np.ascontiguousarray(token_len, np.int32)
    truth_flat = np.ascontiguousarray(truth_flat, np.int32)
    truth_offsets = np.ascontiguousarray(truth_offsets, np.int32)
    B = tokens.shape[0]
    dist = np.zeros(B, np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    _lib.check(lib.lc_edit_distance_host(p(tokens), tokens.shape[1], p(token_len), p(truth_flat), p(truth_offsets),
                                         B, p(dist)), "lc_edit_distance_host")
    return dist


# ------------------------------------------------------------------------------------------ LSTM
def lstm_fwd(dirs, seq_len, T, B, N, forget_bias, bf16=False, x3=False):
    """dirs: list (1 or 2) of dict(zx, R, w_f, w_i, w_o, cs, hs, reverse).  Runs the recurrence in place.
    bf16=True: the step GEMM's operands (m'_{t-1}, R) are rounded to bf16 (lc_lstm_fwd_bf16; config c5).
    x3=True: the step product as fp32-on-bf16x3 - both operands split exactly into three bf16 terms, six term products in
    fp32 (lc_lstm_fwd_x3; fp32-grade results) - where a split-operand kernel exists for the shape, fp32 kernels elsewhere."""
    assert not (bf16 and x3)
    lib = _lib.load()
    arr = (_lib.LstmFwdDir * len(dirs))()
    for i, d in enumerate(dirs):
        _require_cuda(d["zx"], d["R"], d["cs"], d["hs"])
        arr[i].zx, arr[i].R = d["zx"].data_ptr(), d["R"].data_ptr()
        arr[i].w_f = d["w_f"].data_ptr() if d.get("w_f") is not None else None
        arr[i].w_i = d["w_i"].data_ptr() if d.get("w_i") is not None else None
        arr[i].w_o = d["w_o"].data_ptr() if d.get("w_o") is not None else None
        arr[i].cs, arr[i].hs = d["cs"].data_ptr(), d["hs"].data_ptr()
        arr[i].reverse = int(d["reverse"])
        h16 = d.get("hs_bf16") if bf16 else None          # optional fused bf16 copy of hs (bf16 entry point only)
        if h16 is not None:
            _require_cuda(h16)
            assert h16.dtype == torch.bfloat16 and h16.is_contiguous() and h16.numel() == d["hs"].numel()
        arr[i].hs_bf16 = h16.data_ptr() if h16 is not None else None
        arr[i].shadow_only = int(bool(d.get("shadow_only")) and h16 is not None)      # fp32 hs unspecified afterwards
    # one workspace for both passes (it carries the sticky status word): sized for the larger (backward) one at once
    nbytes = max(lib.lc_lstm_fwd_workspace_bytes(B, N, len(dirs)), lib.lc_lstm_bwd_workspace_bytes(B, N, len(dirs)))
    ws = workspace("lstm", nbytes, dirs[0]["zx"].device)
    ev = _prof_begin()
    fn, who = ((lib.lc_lstm_fwd_bf16, "lc_lstm_fwd_bf16") if bf16 else
               (lib.lc_lstm_fwd_x3, "lc_lstm_fwd_x3") if x3 else (lib.lc_lstm_fwd, "lc_lstm_fwd"))
    _lib.check(fn(ctypes.cast(arr, ctypes.c_void_p), len(dirs), _ptr(seq_len), T, B, N,
                  float(forget_bias), _ptr(ws), nbytes, _stream()), who)
    _prof_end("lstm_fwd", 2.0 * len(dirs) * T * B * N * 4 * N, ev)


def lstm_bwd(dirs, seq_len, T, B, N, bf16=False, x3=False):
    """dirs: list of dict(gates, RT, w_f, w_i, w_o, cs, dh, dpeep, dbias, reverse).  gates -> dz in place;
    dpeep [3,N] and dbias [4N] are accumulated into (+=).
    bf16=True: the step GEMM's operands (dz_{t'}, R^T) are rounded to bf16 (lc_lstm_bwd_bf16).
    x3=True: split-operand step product (lc_lstm_bwd_x3), as in lstm_fwd."""
    assert not (bf16 and x3)
    lib = _lib.load()
    arr = (_lib.LstmBwdDir * len(dirs))()
    for i, d in enumerate(dirs):
        _require_cuda(d["gates"], d["RT"], d["cs"], d["dh"])
        arr[i].gates, arr[i].RT = d["gates"].data_ptr(), d["RT"].data_ptr()
        arr[i].w_f = d["w_f"].data_ptr() if d.get("w_f") is not None else None
        arr[i].w_i = d["w_i"].data_ptr() if d.get("w_i") is not None else None
        arr[i].w_o = d["w_o"].data_ptr() if d.get("w_o") is not None else None
        arr[i].cs, arr[i].dh = d["cs"].data_ptr(), d["dh"].data_ptr()
        arr[i].dpeep = d["dpeep"].data_ptr() if d.get("dpeep") is not None else None
        arr[i].dbias = d["dbias"].data_ptr() if d.get("dbias") is not None else None
        arr[i].reverse = int(d["reverse"])
        z16 = d.get("dz_bf16") if bf16 else None          # optional fused bf16 copy of dz (bf16 entry point only)
        if z16 is not None:
            _require_cuda(z16)
            assert z16.dtype == torch.bfloat16 and z16.is_contiguous() and z16.numel() == d["gates"].numel()
        if x3 and d.get("dz_x3") is not None:             # split-operand entry point: the x3 shadow of dz ([rows, 12 N])
            z16 = d["dz_x3"]
            _require_cuda(z16)
            assert z16.dtype == torch.bfloat16 and z16.is_contiguous() and z16.numel() == 3 * d["gates"].numel()
        arr[i].dz_bf16 = z16.data_ptr() if z16 is not None else None
        arr[i].shadow_only = int(bool(d.get("shadow_only")) and bf16 and z16 is not None)      # fp32 dz unspecified afterwards
    nbytes = max(lib.lc_lstm_fwd_workspace_bytes(B, N, len(dirs)), lib.lc_lstm_bwd_workspace_bytes(B, N, len(dirs)))
    ws = workspace("lstm", nbytes, dirs[0]["gates"].device)
    ev = _prof_begin()
    fn, who = ((lib.lc_lstm_bwd_bf16, "lc_lstm_bwd_bf16") if bf16 else
               (lib.lc_lstm_bwd_x3, "lc_lstm_bwd_x3") if x3 else (lib.lc_lstm_bwd, "lc_lstm_bwd"))
    _lib.check(fn(ctypes.cast(arr, ctypes.c_void_p), len(dirs), _ptr(seq_len), T, B, N, _ptr(ws),
                  nbytes, _stream()), who)
    _prof_end("lstm_bwd", 2.0 * len(dirs) * T * B * N * 4 * N, ev)


# ------------------------------------------------------------------------------------------ MoE head
def moe_combine_fwd(a, q, E, V, tau, keep, seed):
    lib = _lib.load()
    _require_cuda(a, q)
    R = a.shape[0]
    logits = torch.empty((R, V), dtype=torch.float32, device=a.device)
    pi = torch.empty((R, E), dtype=torch.float32, device=a.device)
    _lib.check(lib.lc_moe_combine_fwd(_ptr(a), _ptr(q), R, E, V, float(tau), float(keep), int(seed) & 0xFFFFFFFF,
                                      _ptr(logits), _ptr(pi), _stream()), "lc_moe_combine_fwd")
    return logits, pi


def moe_combine_bwd(pi, q, dlogits, E, V, tau, keep, seed):
    lib = _lib.load()
    _require_cuda(pi, q, dlogits)
    R = pi.shape[0]
    da = torch.empty((R, E), dtype=torch.float32, device=pi.device)
    _lib.check(lib.lc_moe_combine_bwd(_ptr(pi), _ptr(q), _ptr(_f32c(dlogits)), R, E, V, float(tau), float(keep),
                                      int(seed) & 0xFFFFFFFF, _ptr(da), _stream()), "lc_moe_combine_bwd")
    return da


# ------------------------------------------------------------------------------------------ optimizer
OPTIMIZERS = {"sgd": 0, "momentum": 1, "adam": 2}


def optimizer_step(params, grads, n_decay, l2, clip_norm, optimizer, lr, step, state, norm_out, guard=None):
    """guard: optional device int32 tensor; the update is skipped on the device when it is non-zero (lstm_status)."""
    lib = _lib.load()
    _require_cuda(params, grads, state, norm_out, guard)
    n = params.numel()
    nbytes = lib.lc_optimizer_workspace_bytes(n)
    ws = workspace("optim", nbytes, params.device)
    _lib.check(lib.lc_optimizer_step(_ptr(params), _ptr(grads), n, int(n_decay), float(l2), float(clip_norm),
                                     OPTIMIZERS[optimizer], float(lr), int(step), _ptr(state), _ptr(norm_out),
                                     _ptr(guard), _ptr(ws), nbytes, _stream()), "lc_optimizer_step")


def label_smoothing(logits, weight, log_q=None, dlogits=None):
    """Returns the device double scalar w*sum p(log p - log q) over all rows; accumulates the gradient into dlogits."""
    lib = _lib.load()
    _require_cuda(logits, log_q, dlogits)
    logits = _f32c(logits)
    rows, V = logits.shape
    acc = torch.zeros(1, dtype=torch.float64, device=logits.device)
    _lib.check(lib.lc_label_smoothing(_ptr(logits), rows, V, _ptr(log_q), float(weight), _ptr(acc), _ptr(dlogits),
                                      _stream()), "lc_label_smoothing")
    return acc


def posteriors(logits, smooth=1.0, apply_softmax=True, apply_log=True, log_prior=None):
    lib = _lib.load()
    _require_cuda(logits, log_prior)
    logits = _f32c(logits)
    rows, V = logits.shape
    out = torch.empty_like(logits)
    _lib.check(lib.lc_posteriors(_ptr(logits), rows, V, float(smooth), int(apply_softmax), int(apply_log),
                                 _ptr(log_prior), _ptr(out), _stream()), "lc_posteriors")
    return out


# ------------------------------------------------------------------------------------------ batch normalisation
BN_EPS, BN_MOMENTUM = 1e-3, 0.99          # tf.layers.batch_normalization defaults (nnet/lstm.py:273,290)


def bn_forward(x, gamma, beta, training, moving_mean, moving_var, out=None):
    """tf.layers.batch_normalization on x [rows, C] (nnet/lstm.py:271-294).  training: batch moments over all rows
    (returned for the backward and the moving-average update); else the moving averages.  -> (y, mean, var)."""
    lib = _lib.load()
    _require_cuda(x, gamma, beta, moving_mean, moving_var)
    x, ldx = _rowmajor2d(x)
    rows, C = x.shape
    if out is None:
        out = torch.empty((rows, C), dtype=torch.float32, device=x.device)
    if training:
        mean = torch.empty(C, dtype=torch.float32, device=x.device)
        var = torch.empty(C, dtype=torch.float32, device=x.device)
        nbytes = lib.lc_bn_workspace_bytes(C)
        ws = workspace("bn", nbytes, x.device)
        _lib.check(lib.lc_bn_moments(_ptr(x), rows, C, ldx, _ptr(mean), _ptr(var), _ptr(ws), nbytes, _stream()),
                   "lc_bn_moments")
    else:
        mean, var = moving_mean, moving_var
    _lib.check(lib.lc_bn_apply(_ptr(x), rows, C, ldx, _ptr(mean), _ptr(var), _ptr(gamma), _ptr(beta), BN_EPS,
                               _ptr(out), out.stride(0), _stream()), "lc_bn_apply")
    return out, mean, var


def bn_backward(x, dy, mean, var, gamma, training, dgamma, dbeta, dx=None):
    """Gradient of bn_forward; dgamma / dbeta are overwritten; dx may be dy (in place)."""
    lib = _lib.load()
    _require_cuda(x, dy, mean, var, gamma, dgamma, dbeta)
    x, ldx = _rowmajor2d(x)
    dy, lddy = _rowmajor2d(dy)
    rows, C = x.shape
    if dx is None:
        dx = torch.empty((rows, C), dtype=torch.float32, device=x.device)
    nbytes = lib.lc_bn_workspace_bytes(C)
    ws = workspace("bn", nbytes, x.device)
    _lib.check(lib.lc_bn_bwd(_ptr(x), _ptr(dy), rows, C, ldx, lddy, _ptr(mean), _ptr(var), _ptr(gamma), BN_EPS,
                             int(bool(training)), _ptr(dx), dx.stride(0), _ptr(dgamma), _ptr(dbeta), _ptr(ws), nbytes,
                             _stream()), "lc_bn_bwd")
    return dx


def bn_update_moving(moving_mean, moving_var, mean, var):
    lib = _lib.load()
    _require_cuda(moving_mean, moving_var, mean, var)
    _lib.check(lib.lc_bn_update_moving(_ptr(moving_mean), _ptr(moving_var), _ptr(mean), _ptr(var),
                                       moving_mean.numel(), BN_MOMENTUM, _stream()), "lc_bn_update_moving")


def length_mask_(x, seq_len, T, B):
    """Zero the rows of the time-major x [T*B, C] that lie beyond each utterance's length (in place)."""
    lib = _lib.load()
    _require_cuda(x, seq_len)
    assert x.dim() == 2 and x.stride(1) == 1 and x.shape[0] == T * B
    _lib.check(lib.lc_length_mask(_ptr(x), T, B, x.shape[1], x.stride(0), _ptr(seq_len), _stream()), "lc_length_mask")
    return x


# ------------------------------------------------------------------------------------------ packed frames
def _gather_rows(fn, x, index, out):
    lib = _lib.load()
    _require_cuda(x, index, out)
    _check_rows(x)
    assert index.dim() == 1 and index.dtype == torch.int32 and index.is_contiguous()
    n, C = index.shape[0], x.shape[1]
    if out is None:
        out = torch.empty((n, C), dtype=torch.float32, device=x.device)
    _check_rows(out, n, C)
    ev = _prof_begin()
    _lib.check(getattr(lib, fn)(_ptr(x), _rows_pitch(x, C), _ptr(index), n, C, _ptr(out), _rows_pitch(out, C), _stream()), fn)
    _prof_end("pack", 8.0 * n * C, ev)           # bytes moved when every row has a source: 4 read + 4 written
    return out


def pack_rows(x, rows, out=None):
    """out[r, :] = x[rows[r], :] where rows[r] >= 0, else +0: the live frames of the time-major x [T*B, C] (a 2-D view, last
    stride 1) as a dense [Mp, C] matrix.  rows: device int32 [Mp], nnet.frames.FrameMap.rows - every entry < x.shape[0]."""
    return _gather_rows("lc_pack_rows", x, rows, out)


def unpack_rows(x, inverse, out=None):
    """out[q, :] = x[inverse[q], :] where inverse[q] >= 0, else +0: the packed x [Mp, C] back on the T*B padded rows, dead
    rows zero.  inverse: device int32 [T*B], FrameMap.inverse - every entry < x.shape[0]."""
    return _gather_rows("lc_unpack_rows", x, inverse, out)


# ------------------------------------------------------------------------------------------ chunked batch (LC-BLSTM)
def chunk_shape(T, B, chunk, lookahead):
    """(nC, Tc, Bc) of the chunked layout of a [T, B] batch: nC = ceil(T / chunk) chunks of Tc = min(chunk + lookahead, T)
    frames, Bc = nC * B rows (chunk row c * B + b)."""
    T, B, chunk, lookahead = int(T), int(B), int(chunk), int(lookahead)
    if T <= 0 or B <= 0 or chunk <= 0 or lookahead < 0:
        raise ValueError("chunk_shape: need T, B, chunk >= 1 and lookahead >= 0, got %r" % ((T, B, chunk, lookahead),))
    nC = -(-T // chunk)
    return nC, min(chunk + lookahead, T), nC * B


def chunk_lengths(seq_len, T, chunk, lookahead):
    """Lengths of the chunk rows, [nC * B] int32 on seq_len's device: row c * B + b has clamp(seq_len[b] - c * chunk, 0, Tc)
    frames.  Plain torch, no kernel of ours and no synchronisation."""
    nC, Tc, _ = chunk_shape(T, seq_len.numel(), chunk, lookahead)
    start = torch.arange(nC, dtype=torch.int32, device=seq_len.device) * int(chunk)
    return (seq_len.to(torch.int32).reshape(1, -1) - start.reshape(-1, 1)).clamp_(0, Tc).reshape(-1).contiguous()


def _rows_pitch(t, C):
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), C)


def _check_rows(m, rows=None, C=None):
    """What every row pass asks of a matrix: a 2-D fp32 view, last stride 1, of this shape (None: any)."""
    assert m.dim() == 2 and m.dtype == torch.float32 and m.stride(1) == 1 and (rows is None or m.shape[0] == rows) \
        and (C is None or m.shape[1] == C), (tuple(m.shape), m.stride(), (rows, C))


def _check_lengths(seq_len, B):
    """... and of the lengths: int32, contiguous, one per utterance."""
    assert seq_len.dtype == torch.int32 and seq_len.is_contiguous() and seq_len.numel() == B


def chunk_gather(x, T, B, chunk, lookahead, zero_lookahead=False, out=None):
    """Padded -> chunked (lc_chunk_gather): x [T*B, C] time-major f32 (a 2-D view, last stride 1) -> out [Tc*Bc, C],
    out[tau * Bc + c * B + b] = x[(c * chunk + tau) * B + b] where that frame exists (and, with zero_lookahead, tau < chunk),
    +0 elsewhere.  Every element of out is written."""
    lib = _lib.load()
    _require_cuda(x, out)
    _, Tc, Bc = chunk_shape(T, B, chunk, lookahead)
    _check_rows(x, T * B)
    C = x.shape[1]
    if out is None:
        out = torch.empty((Tc * Bc, C), dtype=torch.float32, device=x.device)
    _check_rows(out, Tc * Bc, C)
    ev = _prof_begin()
    _lib.check(lib.lc_chunk_gather(_ptr(x), _rows_pitch(x, C), T, B, C, int(chunk), int(lookahead), int(bool(zero_lookahead)),
                                   _ptr(out), _rows_pitch(out, C), _stream()), "lc_chunk_gather")
    _prof_end("chunk", 8.0 * Tc * Bc * C, ev)
    return out


def chunk_fold(xc, T, B, chunk, lookahead, sum_copies=False, seq_len=None, out=None):
    """Chunked -> padded (lc_chunk_fold): xc [Tc*Bc, C] -> out [T*B, C].  sum_copies=False: each frame's copy from its own
    chunk, bit for bit; True: the fp32 sum of every chunk copy of the frame, in ascending chunk order.  seq_len ([B] int32,
    optional): dead copies are skipped and rows beyond each length are +0."""
    lib = _lib.load()
    _require_cuda(xc, seq_len, out)
    _, Tc, Bc = chunk_shape(T, B, chunk, lookahead)
    _check_rows(xc, Tc * Bc)
    C = xc.shape[1]
    if seq_len is not None:
        _check_lengths(seq_len, B)
    if out is None:
        out = torch.empty((T * B, C), dtype=torch.float32, device=xc.device)
    _check_rows(out, T * B, C)
    ev = _prof_begin()
    _lib.check(lib.lc_chunk_fold(_ptr(xc), _rows_pitch(xc, C), T, B, C, int(chunk), int(lookahead), int(bool(sum_copies)),
                                 _ptr(seq_len), _ptr(out), _rows_pitch(out, C), _stream()), "lc_chunk_fold")
    _prof_end("chunk", 4.0 * C * (T * B + (Tc * Bc if sum_copies else T * B)), ev)
    return out


# ------------------------------------------------------------------------------------------ row convolution
ROW_CONV_MAX_TAU = 32       # the library's design cap (include/lstm_ctc_hip.h)


def _row_conv_args(w, seq_len, T, B, *mats):
    assert w.dim() == 2 and w.dtype == torch.float32 and w.is_contiguous(), (w.shape, w.stride())
    tau, C = w.shape[0] - 1, w.shape[1]
    _check_lengths(seq_len, B)
    for m in mats:
        _check_rows(m, T * B, C)
    return tau, C


def row_conv_fwd(x2d, w, seq_len, T, B, out=None):
    """Row convolution (lc_row_conv_fwd): x2d [T*B, C] time-major f32 (a 2-D view, last stride 1), w [tau+1, C] dense, seq_len
    [B] int32 -> out [T*B, C], out[t, b] = sum_j w[j] * x[t + j, b] over the live frames t + j of utterance b, +0 in dead rows.
    Every element of out is written; dead rows of x are never read."""
    lib = _lib.load()
    _require_cuda(x2d, w, seq_len, out)
    tau, C = _row_conv_args(w, seq_len, T, B, x2d)
    if out is None:
        out = torch.empty((T * B, C), dtype=torch.float32, device=x2d.device)
    _row_conv_args(w, seq_len, T, B, out)
    ev = _prof_begin()
    _lib.check(lib.lc_row_conv_fwd(_ptr(x2d), _rows_pitch(x2d, C), _ptr(w), T, B, C, tau, _ptr(seq_len), _ptr(out),
                                   _rows_pitch(out, C), _stream()), "lc_row_conv_fwd")
    _prof_end("row_conv", 8.0 * T * B * C, ev)         # HBM bytes: x read once (the re-reads are L2's), y written
    return out


def row_conv_bwd(x2d, dy2d, w, seq_len, T, B, want_dx=True, want_dw=True, dx=None, dw=None):
    """Gradients of row_conv_fwd (lc_row_conv_bwd) -> (dx [T*B, C] or None, dw [tau+1, C] or None): dx[t, b] = sum_j w[j] *
    dy[t - j, b] in live rows, +0 in dead ones; dw[j] = sum over the live pairs of dy[t, b] * x[t + j, b], overwritten.
    ``dx`` / ``dw``: optional destinations (dw dense).  The dw workspace is owned here."""
    lib = _lib.load()
    _require_cuda(x2d, dy2d, w, seq_len, dx, dw)
    if not (want_dx or want_dw):
        raise ValueError("row_conv_bwd: want_dx and want_dw are both false")
    tau, C = _row_conv_args(w, seq_len, T, B, dy2d, *([x2d] if want_dw else []))
    if want_dx:
        if dx is None:
            dx = torch.empty((T * B, C), dtype=torch.float32, device=dy2d.device)
        _row_conv_args(w, seq_len, T, B, dx)
    else:
        dx = None
    ws, nbytes = None, 0
    if want_dw:
        if dw is None:
            dw = torch.empty((tau + 1, C), dtype=torch.float32, device=dy2d.device)
        assert dw.dtype == torch.float32 and tuple(dw.shape) == (tau + 1, C) and dw.is_contiguous()
        nbytes = lib.lc_row_conv_workspace_bytes(T, B, C, tau)
        ws = workspace("row_conv", nbytes, dy2d.device)
    else:
        dw = None
    xa = x2d if want_dw else None
    ev = _prof_begin()
    _lib.check(lib.lc_row_conv_bwd(_ptr(xa), _rows_pitch(xa, C) if xa is not None else C, _ptr(dy2d), _rows_pitch(dy2d, C),
                                   _ptr(w), T, B, C, tau, _ptr(seq_len), _ptr(dx), _rows_pitch(dx, C) if dx is not None else C,
                                   _ptr(dw), _ptr(ws), nbytes, _stream()), "lc_row_conv_bwd")
    _prof_end("row_conv", 4.0 * T * B * C * (2 * bool(want_dx) + 2 * bool(want_dw)), ev)
    return dx, dw


# ------------------------------------------------------------------------------------------ time reduction (pyramidal BiLSTM)
TIME_REDUCE_MIN_FACTOR, TIME_REDUCE_MAX_FACTOR = 2, 4       # the library's range of r (include/lstm_ctc_hip.h)


def time_reduce_frames(T, r):
    """ceil(T / r): the frames (or, for a length, the live frames) left after joining r consecutive ones."""
    return -(-int(T) // int(r))


def time_reduce_lengths(seq_len, r):
    """ceil(seq_len / r), elementwise: the lengths behind a reduction by r.  A device tensor stays on its device (integer
    ops, no kernel of ours and no synchronisation) and comes back int32 and contiguous; anything else comes back as a numpy
    int32 array."""
    r = int(r)
    if r < 1:
        raise ValueError("time_reduce_lengths: need r >= 1, got %r" % (r,))
    if isinstance(seq_len, torch.Tensor):
        return torch.div(seq_len.to(torch.int32) + (r - 1), r, rounding_mode="floor").to(torch.int32).contiguous()
    a = np.asarray(seq_len)
    return ((a.astype(np.int64) + (r - 1)) // r).astype(np.int32)


def _time_reduce_args(seq_len, T, B, C, r, narrow, wide):
    if not (TIME_REDUCE_MIN_FACTOR <= int(r) <= TIME_REDUCE_MAX_FACTOR):
        raise ValueError("time reduction: r must be in %d..%d, got %r" % (TIME_REDUCE_MIN_FACTOR, TIME_REDUCE_MAX_FACTOR, r))
    To = time_reduce_frames(T, r)
    _check_lengths(seq_len, B)
    _check_rows(narrow, T * B, C)
    _check_rows(wide, To * B, r * C)
    return To


def time_reduce_fwd(x2d, seq_len, T, B, r, out=None):
    """Time reduction (lc_time_reduce_fwd): x2d [T*B, C] time-major f32 (a 2-D view, last stride 1), seq_len [B] int32 -> out
    [ceil(T / r) * B, r * C], out[to, b, j * C + c] = x[r * to + j, b, c] where frame r * to + j of utterance b is live, +0
    elsewhere.  Every element of out is written; dead frames of x are never read."""
    lib = _lib.load()
    _require_cuda(x2d, seq_len, out)
    T, B, r = int(T), int(B), int(r)
    assert x2d.dim() == 2
    C = x2d.shape[1]
    if out is None:
        out = torch.empty((time_reduce_frames(T, r) * B, r * C), dtype=torch.float32, device=x2d.device)
    _time_reduce_args(seq_len, T, B, C, r, x2d, out)
    ev = _prof_begin()
    _lib.check(lib.lc_time_reduce_fwd(_ptr(x2d), _rows_pitch(x2d, C), T, B, C, r, _ptr(seq_len), _ptr(out),
                                      _rows_pitch(out, r * C), _stream()), "lc_time_reduce_fwd")
    _prof_end("time_reduce", 8.0 * T * B * C, ev)
    return out


def time_reduce_bwd(dy2d, seq_len, T, B, r, out=None):
    """The adjoint of time_reduce_fwd (lc_time_reduce_bwd): dy2d [ceil(T / r) * B, r * C] -> out [T*B, C], out[t, b, c] =
    dy[t // r, b, (t % r) * C + c] in live frames, +0 in dead ones.  Every element of out is written."""
    lib = _lib.load()
    _require_cuda(dy2d, seq_len, out)
    T, B, r = int(T), int(B), int(r)
    assert dy2d.dim() == 2 and r >= 1 and dy2d.shape[1] % r == 0, (tuple(dy2d.shape), r)
    C = dy2d.shape[1] // r
    if out is None:
        out = torch.empty((T * B, C), dtype=torch.float32, device=dy2d.device)
    _time_reduce_args(seq_len, T, B, C, r, out, dy2d)
    ev = _prof_begin()
    _lib.check(lib.lc_time_reduce_bwd(_ptr(dy2d), _rows_pitch(dy2d, r * C), T, B, C, r, _ptr(seq_len), _ptr(out),
                                      _rows_pitch(out, C), _stream()), "lc_time_reduce_bwd")
    _prof_end("time_reduce", 8.0 * T * B * C, ev)
    return out


# ------------------------------------------------------------------------------------------ layer normalisation
LN_EPS = 1e-5               # one constant, like BN_EPS
LAYER_NORM_MAX_C = 8192     # the library's cap: a row lives in one wave's registers (include/lstm_ctc_hip.h)
# csrc/layer_norm.hip's launch constants (LN_MAX_GROUPS, its cap for row_stream.h's rs_grid; 256 threads over rows of at least 4
# lanes): more rows than their product
# and every lane choice's launch walks its rows in more than one pass, and the backward leaves more than one partial per column
LAYER_NORM_MAX_GROUPS, LAYER_NORM_MAX_ROWS_PER_GROUP = 1024, 64


def _layer_norm_args(C, seq_len, T, B, keep, drop_width, vecs, *mats):
    _check_lengths(seq_len, B)
    for v in vecs:
        assert v.dim() == 1 and v.dtype == torch.float32 and v.is_contiguous() and v.numel() == C, (tuple(v.shape), C)
    for m in mats:
        _check_rows(m, T * B, C)
    if not 1 <= C <= LAYER_NORM_MAX_C:
        raise ValueError("layer normalisation: C must be in 1..%d, got %d" % (LAYER_NORM_MAX_C, C))
    if not 0.0 < keep <= 1.0:
        raise ValueError("layer normalisation: keep must be in (0, 1], got %r" % (keep,))
    if drop_width < 1 or C % drop_width:
        raise ValueError("layer normalisation: drop_width %r does not divide C = %d" % (drop_width, C))


def layer_norm_fwd(x2d, gamma, beta, seq_len, T, B, keep=1.0, seed=0, stream0=0, drop_width=None, out=None):
    """Layer normalisation with the dropout mask behind it (lc_layer_norm_fwd): x2d [T*B, C] time-major f32 (a 2-D view, last
    stride 1), gamma / beta [C], seq_len [B] int32 -> out [T*B, C] = mask * (gamma * (x - m) / sqrt(v + LN_EPS) + beta) in live
    rows (m, v: mean and biased variance over the C columns), +0 in dead ones.  keep < 1: column c takes the DropoutWrapper
    factor of stream ``stream0 + c // drop_width`` at index ``row * drop_width + c % drop_width`` (drop_width defaults to C).
    Every element of out is written; dead rows of x are never read."""
    lib = _lib.load()
    _require_cuda(x2d, gamma, beta, seq_len, out)
    T, B = int(T), int(B)
    assert x2d.dim() == 2
    C = x2d.shape[1]
    drop_width = C if drop_width is None else int(drop_width)
    if out is None:
        out = torch.empty((T * B, C), dtype=torch.float32, device=x2d.device)
    _layer_norm_args(C, seq_len, T, B, keep, drop_width, (gamma, beta), x2d, out)
    ev = _prof_begin()
    _lib.check(lib.lc_layer_norm_fwd(_ptr(x2d), _rows_pitch(x2d, C), _ptr(gamma), _ptr(beta), T, B, C, LN_EPS, _ptr(seq_len),
                                     float(keep), int(seed) & 0xFFFFFFFF, int(stream0), drop_width, _ptr(out),
                                     _rows_pitch(out, C), _stream()), "lc_layer_norm_fwd")
    _prof_end("layer_norm", 8.0 * T * B * C, ev)         # HBM bytes: x read, y written
    return out


def layer_norm_bwd(x2d, dy2d, gamma, seq_len, T, B, keep=1.0, seed=0, stream0=0, drop_width=None, want_dx=True,
                   want_dparams=True, dx=None, dgamma=None, dbeta=None):
    """Gradients of layer_norm_fwd (lc_layer_norm_bwd) -> (dx [T*B, C] or None, dgamma [C] or None, dbeta [C] or None), from the
    layer's input x2d alone (mean and variance are recomputed) and the same mask arguments: with g = mask * dy and xh the
    normalised x, dx = rstd * (gamma g - mean(gamma g) - xh * mean(gamma g xh)) in live rows and +0 in dead ones, dgamma = sum
    over live rows of g * xh, dbeta = sum over live rows of g, both overwritten.  ``dx``: optional destination, dy2d itself for
    the in-place form.  The workspace of the parameter gradients is owned here."""
    lib = _lib.load()
    _require_cuda(x2d, dy2d, gamma, seq_len, dx, dgamma, dbeta)
    if not (want_dx or want_dparams):
        raise ValueError("layer_norm_bwd: want_dx and want_dparams are both false")
    T, B = int(T), int(B)
    assert x2d.dim() == 2
    C = x2d.shape[1]
    drop_width = C if drop_width is None else int(drop_width)
    _layer_norm_args(C, seq_len, T, B, keep, drop_width, (gamma,), x2d, dy2d)
    if want_dx:
        if dx is None:
            dx = torch.empty((T * B, C), dtype=torch.float32, device=dy2d.device)
        _layer_norm_args(C, seq_len, T, B, keep, drop_width, (), dx)
    else:
        dx = None
    ws, nbytes = None, 0
    if want_dparams:
        dgamma = torch.empty(C, dtype=torch.float32, device=dy2d.device) if dgamma is None else dgamma
        dbeta = torch.empty(C, dtype=torch.float32, device=dy2d.device) if dbeta is None else dbeta
        _layer_norm_args(C, seq_len, T, B, keep, drop_width, (dgamma, dbeta))
        nbytes = lib.lc_layer_norm_workspace_bytes(T, B, C)
        ws = workspace("layer_norm", nbytes, dy2d.device)
    else:
        dgamma = dbeta = None
    ev = _prof_begin()
    _lib.check(lib.lc_layer_norm_bwd(_ptr(x2d), _rows_pitch(x2d, C), _ptr(dy2d), _rows_pitch(dy2d, C), _ptr(gamma), T, B, C,
                                     LN_EPS, _ptr(seq_len), float(keep), int(seed) & 0xFFFFFFFF, int(stream0), drop_width,
                                     _ptr(dx), _rows_pitch(dx, C) if dx is not None else C, _ptr(dgamma), _ptr(dbeta), _ptr(ws),
                                     nbytes, _stream()), "lc_layer_norm_bwd")
    _prof_end("layer_norm", 12.0 * T * B * C, ev)        # HBM bytes: x and dy read, dx written
    return dx, dgamma, dbeta


# ------------------------------------------------------------------------------------------ convolutional front-end
CONV_MAX_CHANNELS, CONV_MAX_BINS = 64, 512      # the library's design caps (include/lstm_ctc_hip.h)
# csrc/conv.hip's launch constants: the forward pass and the input gradient launch at most CONV_MAX_GROUPS workgroups, each on a
# tile of CONV_FWD_FRAMES / CONV_DX_FRAMES frames of at most CONV_MAX_POS (utterance, bin) positions - more tiles than that and
# a workgroup walks several; the weight gradient's CONV_DW_GROUPS workgroups split into ceil(Cin / 8) chunks of input channels
# times the partials per weight, each walking tiles of CONV_DW_FRAMES frames x 16 output bins of one utterance
CONV_MAX_GROUPS, CONV_FWD_FRAMES, CONV_DX_FRAMES, CONV_MAX_POS, CONV_DW_GROUPS, CONV_DW_FRAMES = 1024, 8, 4, 64, 1024, 8


def conv_out_bins(F):
    """Bins a conv layer writes for F input bins: ceil(F / 2) (kernel 3, stride 2, padding 1)."""
    return (int(F) + 1) // 2


def _conv_args(w, seq_len, T, B, F):
    assert w.dim() == 4 and tuple(w.shape[:2]) == (3, 3) and w.dtype == torch.float32 and w.is_contiguous(), (w.shape, w.stride())
    Cin, Cout = int(w.shape[2]), int(w.shape[3])
    _check_lengths(seq_len, B)
    if not (1 <= Cin <= CONV_MAX_CHANNELS and 8 <= Cout <= CONV_MAX_CHANNELS and Cout % 8 == 0 and 1 <= F <= CONV_MAX_BINS):
        raise ValueError("conv: need Cin in 1..%d, Cout a multiple of 8 in 8..%d and F in 1..%d, got Cin %d, Cout %d, F %d"
                         % (CONV_MAX_CHANNELS, CONV_MAX_CHANNELS, CONV_MAX_BINS, Cin, Cout, F))
    return Cin, Cout, conv_out_bins(F)


def conv_fwd(x2d, w, bias, seq_len, T, B, F, group_major=False, out=None):
    """One layer of the convolutional front-end (lc_conv_fwd): x2d [T*B, Cin*F] time-major f32 (a 2-D view, last stride 1;
    column ci * F + f with ``group_major``, else f * Cin + ci), w [3, 3, Cin, Cout] dense, bias [Cout], seq_len [B] int32 ->
    out [T*B, ceil(F/2) * Cout] (column fo * Cout + co) = relu(conv2d(x, w, padding 1, stride (1, 2)) + bias) in live rows, +0
    in dead ones.  Every element of out is written; dead rows of x are never read."""
    lib = _lib.load()
    _require_cuda(x2d, w, bias, seq_len, out)
    T, B, F = int(T), int(B), int(F)
    Cin, Cout, Fo = _conv_args(w, seq_len, T, B, F)
    _check_rows(x2d, T * B, Cin * F)
    assert bias.dtype == torch.float32 and tuple(bias.shape) == (Cout,) and bias.is_contiguous()
    if out is None:
        out = torch.empty((T * B, Fo * Cout), dtype=torch.float32, device=x2d.device)
    _check_rows(out, T * B, Fo * Cout)
    ev = _prof_begin()
    _lib.check(lib.lc_conv_fwd(_ptr(x2d), _rows_pitch(x2d, Cin * F), int(bool(group_major)), _ptr(w), _ptr(bias), T, B, F, Cin,
                               Cout, _ptr(seq_len), _ptr(out), _rows_pitch(out, Fo * Cout), _stream()), "lc_conv_fwd")
    _prof_end("conv", 2.0 * 9 * Cin * Cout * Fo * T * B, ev)            # FLOPs
    return out


def conv_bwd(x2d, y2d, dy2d, w, seq_len, T, B, F, group_major=False, want_dx=True, want_dparams=True, dx=None, dw=None,
             dbias=None):
    """Gradients of conv_fwd (lc_conv_bwd) -> (dx [T*B, Cin*F] or None, dw [3, 3, Cin, Cout] or None, dbias [Cout] or None), with
    g = dy2d where y2d > 0 (y2d: what conv_fwd wrote): dx the transposed convolution of g in live rows and +0 in dead ones, in
    x2d's layout; dw = sum over the live positions of g * x, dbias = sum of g, both overwritten.  The workspace of the parameter
    gradients is owned here."""
    lib = _lib.load()
    _require_cuda(x2d, y2d, dy2d, w, seq_len, dx, dw, dbias)
    if not (want_dx or want_dparams):
        raise ValueError("conv_bwd: want_dx and want_dparams are both false")
    T, B, F = int(T), int(B), int(F)
    Cin, Cout, Fo = _conv_args(w, seq_len, T, B, F)
    _check_rows(y2d, T * B, Fo * Cout)
    _check_rows(dy2d, T * B, Fo * Cout)
    if want_dx:
        if dx is None:
            dx = torch.empty((T * B, Cin * F), dtype=torch.float32, device=dy2d.device)
        _check_rows(dx, T * B, Cin * F)
    else:
        dx = None
    ws, nbytes, xa = None, 0, None
    if want_dparams:
        xa = x2d
        _check_rows(x2d, T * B, Cin * F)
        dw = torch.empty((3, 3, Cin, Cout), dtype=torch.float32, device=dy2d.device) if dw is None else dw
        dbias = torch.empty(Cout, dtype=torch.float32, device=dy2d.device) if dbias is None else dbias
        assert dw.dtype == torch.float32 and tuple(dw.shape) == (3, 3, Cin, Cout) and dw.is_contiguous()
        assert dbias.dtype == torch.float32 and tuple(dbias.shape) == (Cout,) and dbias.is_contiguous()
        nbytes = lib.lc_conv_workspace_bytes(T, B, F, Cin, Cout)
        ws = workspace("conv", nbytes, dy2d.device)
    else:
        dw = dbias = None
    ev = _prof_begin()
    _lib.check(lib.lc_conv_bwd(_ptr(xa), _rows_pitch(xa, Cin * F) if xa is not None else Cin * F, int(bool(group_major)),
                               _ptr(y2d), _rows_pitch(y2d, Fo * Cout), _ptr(dy2d), _rows_pitch(dy2d, Fo * Cout), _ptr(w), T, B, F,
                               Cin, Cout, _ptr(seq_len), _ptr(dx), _rows_pitch(dx, Cin * F) if dx is not None else Cin * F,
                               _ptr(dw), _ptr(dbias), _ptr(ws), nbytes, _stream()), "lc_conv_bwd")
    _prof_end("conv", 2.0 * 9 * Cin * Cout * Fo * T * B * (bool(want_dx) + bool(want_dparams)), ev)
    return dx, dw, dbias


# ------------------------------------------------------------------------------------------ SpecAugment
def _tbd_pitch(t, T, B, D):
    """Row pitch of a time-major [T, B, D] tensor whose T * B rows lie at one pitch (a column window of a wider buffer is
    fine)."""
    assert t.dtype == torch.float32 and t.dim() == 3 and tuple(t.shape) == (T, B, D), (t.dtype, tuple(t.shape))
    assert D == 1 or t.stride(2) == 1, t.stride()
    ld = t.stride(1) if B > 1 else (t.stride(0) if T > 1 else D)
    assert ld >= D and (B == 1 or T == 1 or t.stride(0) == B * ld), t.stride()
    return ld


def spec_augment(x, seq_len, spec, layout, seed, out=None, plan=None):
    """SpecAugment on the device (lc_spec_augment): x [T,B,D] time-major f32 (rows at one pitch), seq_len [B] i32, ``spec`` a
    ``nnet.augment.SpecAugment``, ``layout`` = (base_dim, left_context, right_context, subsample) of the loader
    (``nnet.augment.layout_of(nnet_config)``), ``seed`` the 32-bit seed of the draws.  Returns ``out`` (a new tensor unless
    given; ``out=x`` masks in place): ``spec.fill`` where a time mask holds the element's raw frame or a frequency mask its
    bin, x bit for bit elsewhere.  ``plan=True`` (or an int32 [B,16,2] tensor) also returns the (start, width) table of the
    draws: ``(out, plan)``.  ``nnet.augment.apply_host`` / ``mask_plan`` are the same in numpy."""
    lib = _lib.load()
    _require_cuda(x, seq_len, out, plan if torch.is_tensor(plan) else None)
    T, B, D = x.shape
    assert seq_len.dtype == torch.int32 and seq_len.is_contiguous() and seq_len.numel() == B
    base_dim, left, right, subsample = (int(v or 0) for v in layout)
    if out is None:
        out = torch.empty((T, B, D), dtype=torch.float32, device=x.device)
    if plan is True:
        plan = torch.empty((B, 16, 2), dtype=torch.int32, device=x.device)
    elif plan is False:
        plan = None
    if plan is not None:
        assert plan.dtype == torch.int32 and tuple(plan.shape) == (B, 16, 2) and plan.is_contiguous()
    cfg = _lib.SpecAugmentConfig(spec.time_masks, spec.time_width, spec.time_percent, spec.freq_masks, spec.freq_width,
                                 spec.freq_bins, base_dim, left, right, subsample, spec.fill)
    ev = _prof_begin()
    _lib.check(lib.lc_spec_augment(_ptr(x), T, B, D, _tbd_pitch(x, T, B, D), _ptr(seq_len), ctypes.byref(cfg),
                                   int(seed) & 0xFFFFFFFF, _ptr(out), _tbd_pitch(out, T, B, D), _ptr(plan), _stream()),
               "lc_spec_augment")
    _prof_end("specaug", 8.0 * T * B * D, ev)
    return out if plan is None else (out, plan)


# ------------------------------------------------------------------------------------------ bf16 shadow operands (c5)
def cast_bf16(x, nat=True, tr=False, out_nat=None):
    """bf16 copies of the float32 matrix x [rows, C]: (nat [rows, C] or None, tr [C, rows8] or None), rows8 = rows
    rounded up to a multiple of 8 (the transposed copy's row pitch; its pad columns are zero).  out_nat: an existing
    bf16 [rows, >= C] tensor (last stride 1) to receive the natural copy in its first C columns (the rest is left alone:
    a zero-padded operand of a 256-wide tile)."""
    lib = _lib.load()
    _require_cuda(x, out_nat)
    x, ldx = _rowmajor2d(x)
    rows, C = x.shape
    ldn = C
    if out_nat is not None:
        assert (out_nat.dtype == torch.bfloat16 and out_nat.dim() == 2 and out_nat.shape[0] == rows and out_nat.shape[1] >= C
                and out_nat.stride(1) == 1)
        nat = True
        ldn = out_nat.stride(0) if rows > 1 else max(out_nat.stride(0), C)
    n = out_nat if out_nat is not None else (torch.empty((rows, C), dtype=torch.bfloat16, device=x.device) if nat else None)
    t = None
    if tr:
        rows8 = (rows + 7) // 8 * 8
        t = (torch.zeros if rows8 != rows else torch.empty)((C, rows8), dtype=torch.bfloat16, device=x.device)
    ev = _prof_begin()
    _lib.check(lib.lc_cast_bf16(_ptr(x), rows, C, ldx, _ptr(n), ldn, _ptr(t), t.shape[1] if t is not None else 0,
                                _stream()), "lc_cast_bf16")
    _prof_end("cast_bf16", float(rows) * C * (4 + 2 * (int(nat) + int(tr))), ev)      # bytes moved
    return n, t


def gemm_bf16_nt(A, B, out=None, alpha=1.0, beta=0.0, bias=None, K=None, epilogue=None):
    """out[M,N] = alpha * A[M,K] @ B[N,K]^T + beta*out (+ bias) on bf16 shadow operands (k contiguous in both).
    K defaults to A.shape[1] (pass the true K when the operands carry zero pad columns)."""
    K = A.shape[1] if K is None else K
    assert B.shape[1] >= K and A.shape[1] >= K
    return _product("lc_gemm_bf16_nt", "gemm_bf16", (), A.shape[0], B.shape[0], (K,), (A,), (B,), out, alpha, beta, bias, epilogue,
                    pool="gemm")


def _product_nt2(name, kind, dtype, A1, B1, A2, B2, out, alpha, beta, bias, epilogue):
    M, N, K1, K2 = A1.shape[0], B1.shape[0], A1.shape[1], A2.shape[1]
    assert A2.shape[0] == M and B2.shape[0] == N and B1.shape[1] == K1 and B2.shape[1] == K2
    assert A1.stride(0) == A2.stride(0) and B1.stride(0) == B2.stride(0) and M > 1 and N > 1
    return _product(name, kind, (), M, N, (K1, K2), (A1, A2), (B1, B2), out, alpha, beta, bias, epilogue, dtype=dtype)


def gemm_nt2(A1, B1, A2, B2, out=None, alpha=1.0, beta=0.0, bias=None, epilogue=None):
    """out[M,N] = alpha * (A1 @ B1^T + A2 @ B2^T) + beta*out (+ bias) in one pass over out, float32 (lc_gemm_f32_nt2): A [M,K],
    B [N,K] row-major views with last stride 1, both pairs with the same row strides - the dX of a bidirectional layer."""
    return _product_nt2("lc_gemm_f32_nt2", "gemm", torch.float32, A1, B1, A2, B2, out, alpha, beta, bias, epilogue)


def gemm_bf16_nt2(A1, B1, A2, B2, out=None, alpha=1.0, beta=0.0, bias=None, epilogue=None):
    """out[M,N] = alpha * (A1 @ B1^T + A2 @ B2^T) + beta*out (+ bias) in one pass over out (lc_gemm_bf16_nt2): bf16 shadow
    operands, k contiguous, both pairs with the same row strides - the dX of a bidirectional layer."""
    return _product_nt2("lc_gemm_bf16_nt2", "gemm_bf16", torch.bfloat16, A1, B1, A2, B2, out, alpha, beta, bias, epilogue)


def gemm_bf16_tn(A, B, out=None, alpha=1.0, beta=0.0, bias=None, epilogue=None):
    """out[M,N] = alpha * A^T @ B + beta*out (+ bias) on bf16 operands that are both K-MAJOR: A [K,M], B [K,N] (row
    windows of natural-layout shadows are fine: only the last stride must be 1).  M, N multiples of 256."""
    K, M = A.shape
    assert B.shape[0] == K
    return _product("lc_gemm_bf16_tn", "gemm_bf16", (), M, B.shape[1], (K,), (A,), (B,), out, alpha, beta, bias, epilogue, pool="gemm")


def gemm_bf16_nn(A, B, out=None, alpha=1.0, beta=0.0, bias=None, epilogue=None):
    """out[M,N] = alpha * A @ B + beta*out (+ bias) on bf16 operands in their NATURAL layouts: A [M,K] (k contiguous), B [K,N]
    (K-major).  M, N multiples of 256, K of 64."""
    M, K = A.shape
    assert B.shape[0] == K
    return _product("lc_gemm_bf16_nn", "gemm_bf16", (), M, B.shape[1], (K,), (A,), (B,), out, alpha, beta, bias, epilogue, pool="gemm")


# ------------------------------------------------------------------------------------------ fp32 products as bf16 x 3
def split_bf16x3(x):
    """x [rows, K] f32 (last stride 1) -> its x3 shadow [rows, 3 * roundup(K, 16)] bf16 (lc_split_bf16x3)."""
    lib = _lib.load()
    _require_cuda(x)
    assert x.dim() == 2 and x.dtype == torch.float32 and x.stride(1) == 1
    rows, K = x.shape
    ldo = 3 * ((K + 15) // 16 * 16)
    out = torch.empty((rows, ldo), dtype=torch.bfloat16, device=x.device)
    ldx = x.stride(0) if rows > 1 else max(x.stride(0), K)
    ev = _prof_begin()
    _lib.check(lib.lc_split_bf16x3(_ptr(x), rows, K, ldx, _ptr(out), ldo, _stream()), "lc_split_bf16x3")
    _prof_end("cast_bf16", float(rows) * K * 10, ev)
    return out


def gemm_bf16x3_nt(A3, B3, K, out=None, alpha=1.0, beta=0.0, bias=None, epilogue=None):
    """out[M,N] = alpha * A @ B^T + beta*out (+ bias) from the x3 shadows of A [M,K] and B [N,K]: fp32-grade result on the
    bf16 matrix cores (six bf16 term products per element product)."""
    return _product("lc_gemm_bf16x3_nt", "gemm_x3", (), A3.shape[0], B3.shape[0], (K,), (A3,), (B3,), out, alpha, beta, bias, epilogue)


def gemm_bf16x3_tn(A3, B3, M, N, out=None, alpha=1.0, beta=0.0, bias=None):
    """out[M,N] = alpha * A^T @ B + beta*out (+ bias) from the x3 shadows of A [K,M] and B [K,N] (both K-major; row windows
    of larger shadows are fine): the weight gradients, fp32-grade, on the bf16 matrix cores."""
    K = A3.shape[0]
    assert B3.shape[0] == K and A3.shape[1] >= 3 * ((M + 15) // 16 * 16) and B3.shape[1] >= 3 * ((N + 15) // 16 * 16)
    # K slices: CU fill, and the 2 GB descriptor reach
    nbytes = _lib.load().lc_gemm_bf16x3_tn_workspace_bytes_ld(M, N, K, _ld(A3), _ld(B3))
    return _product("lc_gemm_bf16x3_tn", "gemm_x3", (), M, N, (K,), (A3,), (B3,), out, alpha, beta, bias, pool="gemm_x3",
                    nbytes=nbytes)
