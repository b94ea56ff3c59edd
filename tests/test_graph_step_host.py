"""The host-side pieces of the graph's step (lstm_ctc_amd/nnet/graph.py): the launch-train retry of ``_FallbackLatch.run``
on scripted status words, the named one-copy scalar collector ``_HostScalars`` on CPU tensors, and the number check of the
constructor's options, message by message.  No GPU."""
import contextlib

import numpy as np
import pytest
import torch

from lstm_ctc_amd.nnet import graph

CFG = dict(nnet_type="blstm", input_dim=12, left_context=0, right_context=0, num_layers=1, num_neurons=32, num_projects=16,
           num_targets=12, use_peepholes=True, dropout_rate=0.8)


# ------------------------------------------------------------------------------------------------------- _FallbackLatch.run
class Script:
    """``fn`` of ``_FallbackLatch.run``: returns ("r<call number>", next scripted status) and writes down, per call, whether it
    ran inside ``ops.force_launch_train()``."""

    def __init__(self, monkeypatch, statuses):
        self.statuses, self.events, self.forced, self.calls = list(statuses), [], False, 0
        monkeypatch.setattr(graph.ops, "force_launch_train", self._force)
        monkeypatch.setattr("lstm_ctc_amd.nnet.tflog.info", lambda text: self.events.append(("log", text)))

    @contextlib.contextmanager
    def _force(self):
        self.forced = True
        try:
            with contextlib.nullcontext():
                yield
        finally:
            self.forced = False

    def __call__(self):
        self.events.append("forced" if self.forced else "try")
        self.calls += 1
        return "r%d" % self.calls, self.statuses.pop(0)

    def before_retry(self):
        self.events.append("before_retry")

    def kinds(self):
        return [e if isinstance(e, str) else e[0] for e in self.events]


def test_a_success_leaves_the_counts_alone(monkeypatch):
    fn, latch = Script(monkeypatch, [0, 0]), graph._FallbackLatch()
    assert latch.run(fn, before_retry=fn.before_retry) == "r1" and latch.run(fn) == "r2"
    assert fn.kinds() == ["try", "try"]
    assert (latch.total, latch.consecutive, latch.latched) == (0, 0, False)


def test_a_single_failure_retries_once_after_before_retry(monkeypatch):
    fn, latch = Script(monkeypatch, [5, 0]), graph._FallbackLatch()
    assert latch.run(fn, before_retry=fn.before_retry) == "r2"              # the retry's result, not the failed try's
    assert fn.kinds() == ["try", "log", "before_retry", "forced"]
    assert (latch.total, latch.consecutive, latch.latched) == (1, 1, False)
    assert fn.events[1][1] == ("persistent LSTM launch did not complete (status 5, fallback #1); re-running the step with "
                               "the per-step launch train")
    fn.statuses = [7, 0]
    del fn.events[:]
    assert graph._FallbackLatch().run(fn) == "r4" and fn.kinds() == ["try", "log", "forced"]      # before_retry is optional


def test_two_failures_in_a_row_latch_and_the_next_call_is_forced_at_once(monkeypatch):
    fn, latch = Script(monkeypatch, [3, 0, 3, 0, 0, 0]), graph._FallbackLatch()
    assert graph._FallbackLatch.LATCH_AFTER == 2
    latch.run(fn, before_retry=fn.before_retry)
    assert not latch.latched
    latch.run(fn, before_retry=fn.before_retry)
    assert latch.latched and (latch.total, latch.consecutive) == (2, 2)
    assert fn.events[-3][1] == ("persistent LSTM launch did not complete (status 3, fallback #2); re-running the step with "
                                "the per-step launch train - and staying on it for the rest of this run (2 failures in a row)")
    del fn.events[:]
    assert latch.run(fn, before_retry=fn.before_retry) == "r5" and latch.run(fn) == "r6"
    assert fn.kinds() == ["forced", "forced"]                                # no first try, no log, no before_retry
    assert latch.latched and latch.total == 2


def test_a_success_between_two_failures_does_not_latch(monkeypatch):
    fn, latch = Script(monkeypatch, [3, 0, 0, 3, 0, 0]), graph._FallbackLatch()
    for _ in range(3):
        latch.run(fn, before_retry=fn.before_retry)
    assert (latch.total, latch.consecutive, latch.latched) == (2, 1, False)
    assert latch.run(fn) == "r6" and fn.kinds()[-1] == "try" and latch.consecutive == 0


def test_a_failing_retry_raises_with_the_callers_text(monkeypatch):
    fn, latch = Script(monkeypatch, [3, 4]), graph._FallbackLatch()
    with pytest.raises(RuntimeError) as e:
        latch.run(fn, before_retry=fn.before_retry)
    assert str(e.value) == "LSTM recurrence failed on the launch train as well (status 4)"      # step_device, align
    fn.statuses = [3, 4]
    with pytest.raises(RuntimeError) as e:
        latch.run(fn, error="LSTM recurrence failed on the launch train as well")               # forward_batch
    assert str(e.value) == "LSTM recurrence failed on the launch train as well" and latch.latched
    fn.statuses = [9, 9]
    step_device = dict(latched_error="LSTM recurrence failed on the launch train (status {status})")
    with pytest.raises(RuntimeError) as e:
        latch.run(fn, **step_device)                                                            # latched: its own text
    assert str(e.value) == "LSTM recurrence failed on the launch train (status 9)"
    with pytest.raises(RuntimeError) as e:
        latch.run(fn)                                                                           # align, latched
    assert str(e.value) == "LSTM recurrence failed on the launch train as well (status 9)"
    assert not fn.forced                                                     # the override ended with every raise


def test_graphs_report_the_latchs_count():
    class G(graph.CTCGraph):
        def __init__(self):
            self._fallback = graph._FallbackLatch()
    g = G()
    g._fallback.total = 3
    assert g.persist_fallbacks == 3 and graph.InferenceGraph.persist_fallbacks.fget(g) == 3


# ------------------------------------------------------------------------------------------------------------ _HostScalars
BIG = 2 ** 24 + 1                  # not a float32
F32 = np.float32(1.0) / np.float32(3.0)
SOURCES = {                        # name -> (device tensor as a step adds it, the exact Python value)
    "eval_loss": (torch.tensor([F32, F32], dtype=torch.float32).sum(), float(np.float32(F32 + F32))),
    "status": (torch.tensor([0], dtype=torch.int32), 0.0),
    "reg": (torch.tensor(F32, dtype=torch.float32), float(F32)),
    "grad_norm": (torch.tensor([F32, 7.0], dtype=torch.float32)[:1], float(F32)),
    "kd_loss": (torch.tensor([0.1, 0.2], dtype=torch.float32).to(torch.float64).sum(),
                float(np.float32(0.1)) + float(np.float32(0.2))),
    "kd_frames": (torch.tensor([BIG, 2], dtype=torch.int32).to(torch.float64).sum(), float(BIG + 2)),
    "entry_labels": (torch.tensor([BIG, 4], dtype=torch.int64).sum(), float(BIG + 4)),
    "count": (torch.tensor(BIG, dtype=torch.int32), float(BIG)),
}
SUBSETS = [("eval_loss", "status"), ("eval_loss", "status", "reg", "grad_norm"), ("status", "kd_loss", "kd_frames", "count"),
           ("count", "entry_labels", "eval_loss", "status", "grad_norm", "kd_frames"), tuple(reversed(list(SOURCES)))]


@pytest.mark.parametrize("names", SUBSETS, ids=lambda names: "+".join(names))
def test_scalars_come_back_by_name_exactly_in_one_copy(names, monkeypatch):
    cats, cat = [], torch.cat
    monkeypatch.setattr(torch, "cat", lambda parts, *a, **kw: cats.append(len(parts)) or cat(parts, *a, **kw))
    word = graph._HostScalars()
    for name in names:
        word.add(name, SOURCES[name][0])
    assert cats == []                                                        # collecting moves nothing
    host = word.fetch()
    assert cats == [len(names)]                                              # one word, one copy
    assert list(host) == list(names)
    for name in names:
        assert type(host[name]) is float and host[name] == SOURCES[name][1], name
    assert int(host.get("count", BIG)) == BIG


def test_a_name_is_collected_once():
    word = graph._HostScalars()
    word.add("status", torch.zeros(1, dtype=torch.int32))
    with pytest.raises(KeyError):
        word.add("status", torch.zeros(1, dtype=torch.int32))


# ------------------------------------------------------------------------------------------------------- the number check
# the messages of the parent's five inline checks, copied from its source
MESSAGES = {"teacher_weight": "teacher_weight must be a finite float > 0 or None, got %r",
            "teacher_temperature": "teacher_temperature must be finite and > 0, got %r",
            "delay_penalty": "delay_penalty must be a finite float >= 0 or None, got %r",
            "consistency_weight": "consistency_weight must be a finite float > 0 or None, got %r",
            "align_window": "align_window must be an int >= 0 (frames) or None, got %r"}
ACCEPTS_ZERO = ("delay_penalty", "align_window")
VALUES = [True, "1", float("nan"), float("inf"), 0, -1]


@pytest.mark.parametrize("option", list(MESSAGES))
@pytest.mark.parametrize("value", VALUES, ids=repr)
def test_number_check_messages_are_the_parents(option, value):
    options, speaks = {option: value}, (option, value)
    if option in ACCEPTS_ZERO and value == 0:                                # 0 passes: a LATER check speaks, no device yet
        options["consistency_weight"] = True
        speaks = ("consistency_weight", True)
    with pytest.raises(ValueError) as e:
        graph.CTCGraph(None, CFG, learn_rate=0.1, **options)
    assert str(e.value) == MESSAGES[speaks[0]] % (speaks[1],)


def test_number_check_order_and_results():
    make = lambda **kw: graph.CTCGraph(None, CFG, learn_rate=0.1, **kw)
    order = ["teacher_weight", "teacher_temperature", "align_window", "delay_penalty", "consistency_weight"]
    for i, first in enumerate(order):                                        # of several bad options the earliest check wins
        with pytest.raises(ValueError) as e:
            make(**{name: -1 for name in order[i:]})
        assert str(e.value) == MESSAGES[first] % (-1,)
    check = graph._checked_number
    for got, want in ((check("w", np.float32(0.5), 0, True, ""), 0.5), (check("w", 2, 0, True, ""), 2.0),
                      (check("p", 0, 0, False, ""), 0.0), (check("n", np.int64(3), 0, False, "", integer=True), 3)):
        assert got == want and type(got) is type(want)
    with pytest.raises(ValueError, match=r"^n must be an int, got 2\.0$"):
        check("n", 2.0, 0, False, "an int", integer=True)
