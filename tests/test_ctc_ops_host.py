"""The argument lists the five CTC wrappers of lstm_ctc_amd/ops.py hand to the C entries, on the host: a recording stand-in
takes the native library's place, CPU tensors the device's, and every call is compared, slot by slot, with the entry's
prototype as include/lstm_ctc_hip.h declares it (the slot lists below are written from the header, not from ops.py).  A wrong
order or count here would be a fault on the GPU, not a failed assertion.  No GPU."""
import numpy as np
import pytest
import torch

from lstm_ctc_amd import ops

T, B, V, MAXLEN = 3, 2, 4, 2
NBYTES = 4096
HEAD = ("logits", "T", "B", "V", "labels", "label_offsets", "seq_len", "max_label_len")
TAIL = ("grad", "workspace", "workspace_bytes", "stream")
# include/lstm_ctc_hip.h: entry -> (its workspace query, the slots between max_label_len and grad)
PROTOTYPES = {
    "lc_ctc_loss": ("lc_ctc_workspace_bytes", ("loss",)),
    "lc_ctc_loss_windowed": ("lc_ctc_window_workspace_bytes", ("win_lo", "win_hi", "loss")),
    "lc_ctc_loss_delay": ("lc_ctc_delay_workspace_bytes", ("win_lo", "win_hi", "delay_penalty", "loss", "entry_sum")),
    "lc_ctc_loss_entropy": ("lc_ctc_entropy_workspace_bytes", ("win_lo", "win_hi", "entropy_weight", "loss", "entropy")),
    "lc_ctc_loss_star": ("lc_ctc_star_workspace_bytes", ("win_lo", "win_hi", "bypass_penalty", "selfloop_penalty", "loss",
                                                         "star_frames")),
}
POINTERS = {"logits", "labels", "label_offsets", "seq_len", "win_lo", "win_hi", "loss", "entry_sum", "entropy", "star_frames",
            "grad", "workspace"}
STREAM = object()


class Recorder:
    """Stands in for the loaded library: every ``lc_*`` attribute is a function that writes its call down; a workspace query
    answers NBYTES, an entry 0."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("lc_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, args))
            return NBYTES if name.endswith("_workspace_bytes") else 0
        return fn


@pytest.fixture
def lib(monkeypatch):
    rec = Recorder()
    rec.workspaces = []

    def workspace(name, nbytes, device):
        rec.workspaces.append((name, nbytes))
        rec.ws = torch.empty(nbytes, dtype=torch.uint8)
        return rec.ws
    monkeypatch.setattr(ops._lib, "load", lambda: rec)
    monkeypatch.setattr(ops, "_require_cuda", lambda *tensors: None)
    monkeypatch.setattr(ops, "_stream", lambda: STREAM)
    monkeypatch.setattr(ops, "_ptr", lambda t: t)                # a pointer slot records the tensor itself, NULL is None
    monkeypatch.setattr(ops, "workspace", workspace)
    return rec


def batch(empty=False):
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    logits = torch.arange(T * B * V, dtype=torch.float32).reshape(T, B, V)
    if empty:
        return dict(logits=logits, labels=i32(), offsets=i32(0, 0, 0), seq_len=i32(3, 2), maxlen=0, lo=i32(), hi=i32())
    return dict(logits=logits, labels=i32(1, 2, 1), offsets=i32(0, 1, 3), seq_len=i32(3, 2), maxlen=MAXLEN, lo=i32(0, 0, 1),
                hi=i32(2, 1, 2))                                 # labels [[1], [2, 1]]


def check_call(lib, entry, b, scalars, windows, want_grad, extra, tag, returned):
    """The one query and the one entry call that ``lib`` recorded, against ``entry``'s prototype."""
    query, middle = PROTOTYPES[entry]
    slots = HEAD + middle + TAIL
    assert [name for name, _ in lib.calls] == [query, entry]
    assert lib.calls[0][1] == (T, B, V, b["maxlen"]) and lib.workspaces == [(tag, NBYTES)]
    args = lib.calls[1][1]
    assert len(args) == len(slots)
    got = dict(zip(slots, args))
    plain = tuple(got[s] for s in slots if s not in POINTERS and s != "stream")
    want_plain = (T, B, V, b["maxlen"]) + tuple(scalars) + (NBYTES,)
    assert plain == want_plain and [type(v) for v in plain] == [type(v) for v in want_plain]
    assert got["stream"] is STREAM
    null = {s for s in slots if s in POINTERS and got[s] is None}
    want_null = set() if want_grad else {"grad"}
    if "win_lo" in slots and not windows:
        want_null |= {"win_lo", "win_hi"}
    name_of_extra = middle[-1] if middle[-1] != "loss" else None
    if name_of_extra and not extra:
        want_null.add(name_of_extra)
    assert null == want_null
    same = lambda a, t: a.data_ptr() == t.data_ptr() and a.shape == t.shape and a.dtype == t.dtype
    assert same(got["logits"], b["logits"]) and same(got["label_offsets"], b["offsets"]) and same(got["seq_len"], b["seq_len"])
    assert got["workspace"] is lib.ws
    given = [("labels", b["labels"])] + ([("win_lo", b["lo"]), ("win_hi", b["hi"])] if windows else [])
    for slot, t in given:
        if t.numel():
            assert same(got[slot], t), slot
        else:                                                    # an empty vector has no address: a one-element stand-in
            assert got[slot].dtype == torch.int32 and got[slot].numel() == 1 and got[slot].is_contiguous(), slot
    outputs = [got["loss"]] + ([got[name_of_extra]] if name_of_extra and extra else [])
    for t in outputs:
        assert t.dtype == torch.float32 and tuple(t.shape) == (B,)
    if want_grad:
        assert got["grad"].dtype == torch.float32 and tuple(got["grad"].shape) == (T, B, V) and got["grad"].is_contiguous()
    # what the wrapper returns are the buffers the entry wrote: loss first, the gradient (or None) last
    assert returned[0] is got["loss"] and returned[-1] is got["grad"]
    if name_of_extra:
        assert len(returned) == 3 and returned[1] is got[name_of_extra]
    else:
        assert len(returned) == 2


CASES = [  # wrapper, entry, workspace tag, positional scalars, the scalars as the entry gets them
    ("ctc_loss", "lc_ctc_loss", "ctc", (), ()),
    ("ctc_loss_windowed", "lc_ctc_loss_windowed", "ctc_window", (), ()),
    ("ctc_loss_delay", "lc_ctc_loss_delay", "ctc_delay", (0.05,), (0.05,)),
    ("ctc_loss_entropy", "lc_ctc_loss_entropy", "ctc_entropy", (0.2,), (0.2,)),
    ("ctc_loss_star", "lc_ctc_loss_star", "ctc_star", (2, float("inf")), (2.0, float("inf"))),
]


LEGAL = {"ctc_loss": (False,), "ctc_loss_windowed": (True,)}      # windows: never / always; the other three: with and without
CALLS = [c + (w,) for c in CASES for w in LEGAL.get(c[0], (False, True))]


@pytest.mark.parametrize("empty", [False, True], ids=["labels", "no-labels"])
@pytest.mark.parametrize("want_grad", [True, False], ids=["grad", "no-grad"])
@pytest.mark.parametrize("wrapper,entry,tag,scalars,c_scalars,windows", CALLS,
                         ids=["%s-%s" % (c[0], "windows" if c[5] else "open") for c in CALLS])
def test_wrapper_passes_the_prototypes_arguments(lib, wrapper, entry, tag, scalars, c_scalars, windows, want_grad, empty):
    b = batch(empty)
    head = (b["logits"], b["labels"], b["offsets"], b["seq_len"], b["maxlen"]) + scalars
    entries = (True, False) if wrapper == "ctc_loss_delay" else (True,)
    for want_entry in entries:
        del lib.calls[:], lib.workspaces[:]
        kw = dict(want_grad=want_grad)
        if wrapper == "ctc_loss_delay":
            kw["want_entry"] = want_entry
        if wrapper == "ctc_loss_windowed":
            returned = ops.ctc_loss_windowed(*head, b["lo"], b["hi"], **kw)
        elif windows:
            returned = getattr(ops, wrapper)(*head, win_lo=b["lo"], win_hi=b["hi"], **kw)
        else:
            returned = getattr(ops, wrapper)(*head, **kw)
        check_call(lib, entry, b, c_scalars, windows, want_grad, want_entry, tag, returned)


def test_wrappers_refuse_before_the_library_is_called(lib):
    b = batch()
    head = (b["logits"], b["labels"], b["offsets"], b["seq_len"], b["maxlen"])
    texts = {
        "ctc_loss_delay": ((float("nan"),), "ctc_loss_delay: delay_penalty must be a finite float, got nan"),
        "ctc_loss_entropy": ((float("inf"),), "ctc_loss_entropy: entropy_weight must be a finite float, got inf"),
        "ctc_loss_star": ((1.0, -0.5), "ctc_loss_star: selfloop_penalty must be a float >= 0 or +inf, got -0.5"),
    }
    for wrapper, (bad, text) in texts.items():
        good = (0.5,) * len(bad)
        with pytest.raises(ValueError) as e:
            getattr(ops, wrapper)(*head, *bad)
        assert str(e.value) == text
        with pytest.raises(ValueError) as e:
            getattr(ops, wrapper)(*head, *good, win_lo=b["lo"])
        assert str(e.value) == "%s: win_lo and win_hi go together (both or none)" % wrapper
        with pytest.raises(ValueError) as e:
            getattr(ops, wrapper)(*head, *good, win_lo=b["lo"][:2], win_hi=b["hi"])
        assert str(e.value) == "%s: win_lo / win_hi must be parallel to labels (2, 3, 3 elements)" % wrapper
    with pytest.raises(ValueError) as e:
        ops.ctc_loss_windowed(*head, b["lo"], b["hi"][:1])
    assert str(e.value) == "ctc_loss_windowed: win_lo / win_hi must be parallel to labels (3, 1, 3 elements)"
    assert not any(name.startswith("lc_ctc_loss") for name, _ in lib.calls)
    np.testing.assert_array_equal(b["labels"].numpy(), [1, 2, 1])
