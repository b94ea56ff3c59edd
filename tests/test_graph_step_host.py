"""The host-side pieces of the graph's step (lstm_ctc_amd/nnet/graph.py): the launch-train retry of ``_FallbackLatch.run``
on scripted status words, the named one-copy scalar collector ``_HostScalars`` on CPU tensors, and the number check of the
constructor's options, message by message; the table of exclusive CTC criterion options (CRITERION_OPTIONS here,
CRITERION_FLAGS in bin/_common.py): every refusal in the parent's words, the merged selection sums, the factories' pass-through.
No GPU."""
import argparse
import contextlib
import importlib.util
import os

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
# the messages of the parent's inline checks, copied from its source
MESSAGES = {"teacher_weight": "teacher_weight must be a finite float > 0 or None, got %r",
            "teacher_temperature": "teacher_temperature must be finite and > 0, got %r",
            "delay_penalty": "delay_penalty must be a finite float >= 0 or None, got %r",
            "entropy_weight": "entropy_weight must be a finite float >= 0 or None, got %r",
            "star_penalty": "star_penalty must be a pair (bypass_penalty, selfloop_penalty) of floats >= 0 or +inf, or None, got %r",
            "consistency_weight": "consistency_weight must be a finite float > 0 or None, got %r",
            "align_window": "align_window must be an int >= 0 (frames) or None, got %r"}
NEEDS_CTC = {"delay_penalty": "delay_penalty tilts the CTC criterion: it needs objective=\"ctc\", not \"%s\"",
             "entropy_weight": "entropy_weight regularises the CTC criterion: it needs objective=\"ctc\", not \"%s\"",
             "star_penalty": "star_penalty relaxes the CTC criterion: it needs objective=\"ctc\", not \"%s\""}
ACCEPTS_ZERO = ("delay_penalty", "entropy_weight", "align_window")
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
    order = ["teacher_weight", "teacher_temperature", "align_window", "delay_penalty", "entropy_weight", "star_penalty",
             "consistency_weight"]
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


# ------------------------------------------------------------------------------------------ the exclusive criterion options
INF = float("inf")
GOOD = {"delay_penalty": 0.05, "entropy_weight": 0.2, "star_penalty": (2, INF)}
# the parent's three pairwise refusals, copied from its source: the LATER option speaks and names the earlier one
EXCLUSIONS = {
    frozenset(("delay_penalty", "entropy_weight")):
        "entropy_weight does not combine with delay_penalty (the entropy of the tilted path posterior is not built)",
    frozenset(("delay_penalty", "star_penalty")):
        "star_penalty does not combine with delay_penalty (the star under the delay tilt is not built)",
    frozenset(("entropy_weight", "star_penalty")):
        "star_penalty does not combine with entropy_weight (the star under the entropy term is not built)",
}


@pytest.mark.parametrize("first,second", [(a, b) for a in GOOD for b in GOOD if a != b])
def test_two_criterion_options_are_refused_in_the_parents_words(first, second):
    with pytest.raises(ValueError) as e:
        graph.CTCGraph(None, CFG, learn_rate=0.1, objective="ctc", **{first: GOOD[first], second: GOOD[second]})
    assert str(e.value) == EXCLUSIONS[frozenset((first, second))]


def test_criterion_option_checks_in_the_parents_order():
    make = lambda **kw: graph.CTCGraph(None, CFG, learn_rate=0.1, **kw)
    with pytest.raises(ValueError) as e:                                     # all three: the first refusal the parent reached
        make(objective="ctc", **GOOD)
    assert str(e.value) == EXCLUSIONS[frozenset(("delay_penalty", "entropy_weight"))]
    for option, text in NEEDS_CTC.items():
        for objective in ("xent", "kd"):
            with pytest.raises(ValueError) as e:                             # the objective before the number, per option
                make(objective=objective, **{option: -1})
            assert str(e.value) == text % objective
    with pytest.raises(ValueError) as e:                                     # the number before the exclusion
        make(delay_penalty=0.05, entropy_weight=-1)
    assert str(e.value) == MESSAGES["entropy_weight"] % (-1,)
    with pytest.raises(ValueError) as e:                                     # an earlier option's number before a later one's objective
        make(objective="xent", star_penalty=(2, 2), entropy_weight=0.1)
    assert str(e.value) == NEEDS_CTC["entropy_weight"] % "xent"
    assert [o.keyword for o in graph.CRITERION_OPTIONS.values()] == list(GOOD) == list(graph.CRITERION_OPTIONS)


TOTALS = ("entry_sum_total", "entry_labels_total", "path_entropy_total", "path_entropy_frames_total", "star_frames_total",
          "star_frame_count_total")


@pytest.mark.parametrize("option", [None] + list(GOOD))
def test_option_values_and_totals_are_graph_attributes(option):
    g = graph.CTCGraph(None, CFG, learn_rate=0.1, device="cpu", seed=1, **({option: GOOD[option]} if option else {}))
    want = {"delay_penalty": 0.05, "entropy_weight": 0.2, "star_penalty": (2.0, INF)}
    for name in GOOD:
        got = getattr(g, name)
        assert got == (want[name] if name == option else None) and type(got) is (type(want[name]) if name == option else type(None))
    assert [getattr(g, t) for t in TOTALS] == [0.0, 0, 0.0, 0, 0.0, 0]
    assert [type(getattr(g, t)) for t in TOTALS] == [float, int] * 3


def test_selected_sums_of_labels_and_of_frames():
    """Four utterances - finite; +inf loss; no frames; more labels than frames - and only the first is counted."""
    loss = np.array([1.5, np.inf, 0.0, 0.0], np.float32)
    extra = np.array([0.3, 7.0, 11.0, 13.0], np.float32)
    seq = np.array([5, 4, 0, 2], np.int32)
    offs = np.array([0, 2, 3, 4, 7], np.int32)
    labels = np.diff(offs).astype(np.int64)
    ok = np.isfinite(loss) & (seq > 0) & (labels <= seq)
    assert ok.tolist() == [True, False, False, False]
    t = torch.from_numpy
    for count in (labels, seq):
        got = graph.CTCGraph._selected_sums(t(loss), t(extra), t(labels), t(seq), t(count))
        assert [x.dtype for x in got] == [torch.float64, torch.int64] and all(x.dim() == 0 for x in got)
        assert got[0].item() == extra.astype(np.float64)[ok].sum() and got[1].item() == int(count.astype(np.int64)[ok].sum())
    two = np.array([1.5, np.inf, 0.0, 2.5], np.float32), np.array([5, 4, 0, 3], np.int32)      # the last one now fits
    got = graph.CTCGraph._selected_sums(t(two[0]), t(extra), t(labels), t(two[1]), t(two[1]))
    assert got[0].item() == float(np.float64(extra[0]) + np.float64(extra[3])) and got[1].item() == 8


def test_factories_pass_options_through():
    cpu = dict(device="cpu", seed=1)
    g = graph.create_graph_for_validation_ctc(None, CFG, align_window=3, star_penalty=(2, 3), **cpu)
    assert (g.objective, g.training, g.align_window, g.star_penalty) == ("ctc", False, 3, (2.0, 3.0))
    g = graph.create_graph_for_training_ctc(None, CFG, 0.1, delay_penalty=0.05, consistency_weight=0.2, teacher_temperature=2, **cpu)
    assert (g.objective, g.learn_rate, g.delay_penalty, g.consistency_weight, g.teacher_temperature) == ("ctc", 0.1, 0.05, 0.2, 2.0)
    assert (g.clip_norm, g.optimizer, g.l2) == (5.0, "sgd", 1e-5)
    assert graph.create_graph_for_training_ctc(None, CFG, 0.1, entropy_weight=0, **cpu).entropy_weight == 0.0
    g = graph.create_graph_for_validation_xent(None, CFG, teacher_weight=0.5, **cpu)
    assert (g.objective, g.training, g.teacher_weight) == ("xent", False, 0.5)
    g = graph.create_graph_for_training_xent(None, CFG, 0.1, 4.0, "adam", teacher_weight=0.5, teacher_temperature=3, **cpu)
    assert (g.objective, g.clip_norm, g.optimizer, g.teacher_weight, g.teacher_temperature) == ("xent", 4.0, "adam", 0.5, 3.0)
    g = graph.create_graph_for_validation_kd(None, CFG, teacher_temperature=2, **cpu)
    assert (g.objective, g.training, g.teacher_temperature, g.needs_teacher) == ("kd", False, 2.0, True)
    g = graph.create_graph_for_training_kd(None, CFG, 0.1, teacher_temperature=2, **cpu)
    assert (g.objective, g.learn_rate, g.teacher_temperature) == ("kd", 0.1, 2.0)
    with pytest.raises(ValueError) as e:                                     # the graph's own refusals come through
        graph.create_graph_for_training_ctc(None, CFG, 0.1, star_penalty=(2, 2), entropy_weight=0.1)
    assert str(e.value) == EXCLUSIONS[frozenset(("entropy_weight", "star_penalty"))]
    training = ("create_graph_for_training_ctc", "create_graph_for_training_xent", "create_graph_for_training_kd")
    for name in training + ("create_graph_for_validation_ctc", "create_graph_for_validation_xent", "create_graph_for_validation_kd"):
        with pytest.raises(TypeError, match="no_such_option"):               # a keyword CTCGraph does not know
            getattr(graph, name)(None, CFG, *((0.1,) if name in training else ()), no_such_option=1)
    for name, kw in (("create_graph_for_validation_ctc", dict(spec_augment=None)),       # as at the parent: CTCGraph knows these,
                     ("create_graph_for_validation_ctc", dict(consistency_weight=0.2)),  # the factory does not take them
                     ("create_graph_for_validation_xent", dict(star_penalty=(2, 2))),
                     ("create_graph_for_training_kd", dict(learn_rate=0.1, delay_penalty=0.05))):
        with pytest.raises(TypeError, match=next(iter(k for k in kw if k != "learn_rate"))):
            getattr(graph, name)(None, CFG, **kw)


# ------------------------------------------------------------------------------------------ the same table on the command line
def _common():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("_common_for_graph_step_test", os.path.join(root, "bin", "_common.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _one_at_a_time(mod, args):
    """The parent's three calls, in its order."""
    return dict(**mod.delay_keywords(args), **mod.entropy_keywords(args), **mod.star_keywords(args))


# (objective, --delay-penalty, --entropy-weight, --star-penalty) -> the parent's FATAL line, copied from its source
FATAL = [
    (("ctc", -1.0, -1.0, "-1"), "--delay-penalty must be a finite number >= 0, got -1.0"),
    (("ctc", INF, None, None), "--delay-penalty must be a finite number >= 0, got inf"),
    (("xent", 0.05, 0.1, "2"), "--delay-penalty tilts the CTC criterion: it needs --objective ctc, not \"xent\""),
    (("xent", None, float("nan"), "x"), "--entropy-weight must be a finite number >= 0, got nan"),
    (("kd", None, 0.1, "x"), "--entropy-weight regularises the CTC criterion: it needs --objective ctc, not \"kd\""),
    (("ctc", 0.05, 0.1, "2"),
     "--entropy-weight does not combine with --delay-penalty (the entropy of the tilted path posterior is not built)"),
    (("ctc", None, None, "-1"), "--star-penalty must be B[,S] with penalties >= 0 or inf, got '-1' (a penalty must be >= 0 or inf)"),
    (("ctc", None, None, "1,2,3"), "--star-penalty must be B[,S] with penalties >= 0 or inf, got '1,2,3' (expected B or B,S)"),
    (("ctc", None, None, "two"),
     "--star-penalty must be B[,S] with penalties >= 0 or inf, got 'two' (could not convert string to float: 'two')"),
    (("xent", None, None, "2"), "--star-penalty relaxes the CTC criterion: it needs --objective ctc, not \"xent\""),
    (("ctc", 0.0, None, "2"), "--star-penalty does not combine with --delay-penalty (the star under that term is not built)"),
    (("ctc", None, 0.0, "2,3"), "--star-penalty does not combine with --entropy-weight (the star under that term is not built)"),
]


@pytest.mark.parametrize("flags,text", FATAL, ids=[repr(f[0]) for f in FATAL])
def test_criterion_keywords_fatal_lines_are_the_parents(flags, text, capsys):
    mod = _common()
    args = argparse.Namespace(objective=flags[0], delay_penalty=flags[1], entropy_weight=flags[2], star_penalty=flags[3])
    for keywords in (mod.criterion_keywords, lambda a: _one_at_a_time(mod, a)):
        with pytest.raises(SystemExit) as e:
            keywords(args)
        assert e.value.code == 1 and capsys.readouterr().err == "FATAL:tensorflow:" + text + "\n"


def test_criterion_keywords_and_reports(capsys):
    mod = _common()
    ns = lambda **kw: argparse.Namespace(**dict(dict(objective="ctc", delay_penalty=None, entropy_weight=None, star_penalty=None), **kw))
    assert mod.criterion_keywords(ns()) == {} and mod.criterion_keywords(argparse.Namespace(objective="xent")) == {}      # nnet-init
    for kw, want in ((dict(delay_penalty=0.0), {"delay_penalty": 0.0}), (dict(entropy_weight=0.2), {"entropy_weight": 0.2}),
                     (dict(star_penalty="inf,0"), {"star_penalty": (INF, 0.0)}), (dict(star_penalty="2"), {"star_penalty": (2.0, 2.0)})):
        assert mod.criterion_keywords(ns(**kw)) == want == _one_at_a_time(mod, ns(**kw))
    assert mod.star_report_keywords(ns(star_penalty="1,2", star_report="r.txt")) == {"star_penalty": (1.0, 2.0)}
    with pytest.raises(SystemExit):
        mod.star_report_keywords(ns(star_penalty="-2", star_report="r.txt"))
    assert capsys.readouterr().err == ("FATAL:tensorflow:--star-penalty must be B[,S] with penalties >= 0 or inf, got '-2' "
                                       "(a penalty must be >= 0 or inf)\n")
    off = dict(delay_penalty=None, entropy_weight=None, star_penalty=None, entry_sum_total=0.0, entry_labels_total=0,
               path_entropy_total=0.0, path_entropy_frames_total=0, star_frames_total=0.0, star_frame_count_total=0)
    lines = {      # the parent's three report formats, copied from its source
        "delay_penalty": (dict(delay_penalty=0.05, entry_sum_total=25.0, entry_labels_total=4), mod.report_delay_penalty,
                          "delay penalty 0.05: mean label entry frame 6.250 over 4 label(s)"),
        "entropy_weight": (dict(entropy_weight=0.2, path_entropy_total=3.0, path_entropy_frames_total=8), mod.report_entropy_weight,
                           "entropy weight 0.2: mean path entropy 0.375000 nats per frame over 8 frame(s)"),
        "star_penalty": (dict(star_penalty=(2.0, INF), star_frames_total=1.5, star_frame_count_total=0), mod.report_star_penalty,
                         "star penalty bypass 2 selfloop inf: 1.500000 of 0 frame(s) explained by the star"),
    }
    mod.report_criterion(argparse.Namespace(**off))
    assert capsys.readouterr().err == ""                                     # no option, no line
    for attrs, old_name, line in lines.values():
        g = argparse.Namespace(**dict(off, **attrs))
        for report in (mod.report_criterion, old_name):
            report(g)
            assert capsys.readouterr().err == "INFO:tensorflow:" + line + "\n"
