"""Train / validation / inference "graphs" — host-side mirror of mobvoi/lstm_ctc ``nnet/graph.py``.

The reference builds TF graphs whose nodes ``sess.run`` evaluates; here a graph is a small object that
owns the model and executes one batch per :meth:`Session.run`, returning the same keys the reference's
graph dict exposes (``size, eval_loss, loss, eval, sequence_length, logits, nnet_output, filename`` …),
so ``nnet.train`` / ``nnet.validate`` (funcs.py) read exactly like the reference's loops.

* validation graph .. ``create_graph_for_validation_ctc``  nnet/graph.py:51-162
* training graph .... ``create_graph_for_training_ctc``    nnet/graph.py:165-209
* inference graph ... ``create_graph_for_inference``       nnet/graph.py:212-241
* data parallelism .. NEW (no reference counterpart): one process per GPU, the flat fp32
  gradient buffer is summed with ONE RCCL all-reduce before the clip, so N ranks x B utterances
  reproduce a single batch of N*B (the clip at graph.py:190 acts on the total gradient of a SUM loss).
"""
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import torch

from .. import ops
from . import dp
from .model import Model, config_keep, time_reduce_config


class OutOfRangeError(Exception):
    """End of the input pipeline (tf.errors.OutOfRangeError in the reference's run loops)."""


def flatten_labels(dense):
    """Dense [B,Lmax] int64 labels padded with -1 -> (flat int32, offsets[B+1], max_len): the
    tf.where / gather_nd / SparseTensor conversion of nnet/graph.py:76-104."""
    dense = np.asarray(dense)
    keep = dense != -1
    lens = keep.sum(axis=1).astype(np.int64)
    flat = dense[keep].astype(np.int32)            # row-major order == tf.where order
    offs = np.zeros(len(lens) + 1, np.int32)
    np.cumsum(lens, out=offs[1:])
    return flat, offs, int(lens.max()) if len(lens) else 0


def double_batch(seq, flat, offs, win_lo=None, win_hi=None):
    """consistency_weight: the batch with every utterance twice, utterance b again in place b + B - numpy arrays or tensors
    alike.  (seq [2B], flat, offsets [2B+1], win_lo, win_hi): lengths, labels and label windows repeated, the second copy's
    offsets shifted by the first copy's label count ``offs[-1]``; an argument that is None stays None.  The first halves ARE
    the original batch."""
    cat = torch.cat if torch.is_tensor(offs) else np.concatenate
    twice = lambda a: None if a is None else cat([a, a])
    return twice(seq), twice(flat), cat([offs, offs[1:] + offs[-1]]), twice(win_lo), twice(win_hi)


def _label_smoothing_setup(nnet_config, device):
    """(weight, log q or None) of the KL regulariser, bilstm.py:255-269: uniform wins over prior (the elif there)."""
    u, pw = nnet_config.get("uniform_label_sm"), nnet_config.get("prior_label_sm")
    if u is not None and u > 0:
        return float(u), None
    if pw is not None and pw > 0 and nnet_config.get("prior_label_path") is not None:
        from .class_prior import get_class_prior
        return float(pw), torch.from_numpy(get_class_prior(nnet_config["prior_label_path"])).to(device)
    return 0.0, None


def _create_logits(nnet_type):
    def create_logits(nnet_input, sequence_length, nnet_config, model=None):
        """``create_logits(nnet_input[B,T,D] f32, sequence_length[B] i32, nnet_config) -> (logits[B,T,V], encoder,
        reg_loss)`` - the callable ``get_create_logits`` hands to the graph builders (nnet/graph.py:24-34,63-67;
        bodies nnet/bilstm.py:25-273, nnet/lstm.py:125-368).  Inputs are GPU tensors (or numpy arrays, uploaded);
        the stack is built from ``nnet_config`` (seed = its ``seed`` key) unless an existing ``model`` is passed;
        the Model that ran is left on ``create_logits.model`` (its ParamStore holds the TF-named variables).
        ``logits`` is a [B,T,V] view of the time-major result; ``encoder`` is the final-state concat for blstm
        (bilstm.py:206-208) and None for lstm; ``reg_loss`` is the list of (device scalar, weight) pairs of
        bilstm.py:255-269 (empty for lstm and when both smoothing weights are 0)."""
        cfg = dict(nnet_config, nnet_type=nnet_type)
        if model is None:
            dev = nnet_input.device if torch.is_tensor(nnet_input) else torch.device("cuda")
            model = Model(cfg, dev, seed=cfg.get("seed"))
        dev = model.device
        x = torch.as_tensor(np.asarray(nnet_input) if not torch.is_tensor(nnet_input) else nnet_input)
        x = x.to(dev, torch.float32).permute(1, 0, 2).contiguous()                 # time-major [T,B,D]
        seq = torch.as_tensor(np.asarray(sequence_length) if not torch.is_tensor(sequence_length)
                              else sequence_length).to(dev, torch.int32)
        ops.lstm_status(dev).zero_()
        tbv = model.forward(x, seq)
        if int(ops.lstm_status(dev).item()) != 0:      # a persistent recurrence could not complete: NaN outputs
            with ops.force_launch_train():
                ops.lstm_status(dev).zero_()
                tbv = model.forward(x, seq)
            if int(ops.lstm_status(dev).item()) != 0:
                raise RuntimeError("LSTM recurrence failed on the launch train as well")
        reg_loss = []
        encoder = None
        if nnet_type == "blstm":
            # (latency-controlled mode: one backward final state per chunk - there is no encoder tensor, model.encoder raises)
            encoder = None if model.chunk else model.encoder()
            w, logq = _label_smoothing_setup(cfg, dev)
            if w > 0:
                T_, B_, V_ = tbv.shape
                reg_loss.append((ops.label_smoothing(tbv.view(T_ * B_, V_), w, logq, None), w))
        create_logits.model = model
        return tbv.permute(1, 0, 2), encoder, reg_loss
    create_logits.model = None
    create_logits.__name__ = "create_logits_" + nnet_type
    return create_logits


create_logits_blstm = _create_logits("blstm")
create_logits_lstm = _create_logits("lstm")
# nnet/lstm.py:26-122, by intent like 'lstm': as shipped it returns the bare logits tensor where graph.py:63 unpacks a triple;
# here it returns (logits, None, []) - a stack of plain LSTM cells (no peepholes / projection / dropout, forget bias 0) and an
# affine head with sigma = 1 / sqrt(num_neurons)
create_logits_cudnnlstm = _create_logits("cudnnlstm")


def get_create_logits(string):
    """nnet/graph.py:24-34: 'blstm' | 'cudnnlstm' | 'lstm' -> the function, anything else -> None."""
    return {"blstm": create_logits_blstm, "cudnnlstm": create_logits_cudnnlstm,
            "lstm": create_logits_lstm}.get(string) if string else None


def get_optimizer(string):
    """nnet/graph.py:37-48 — the three optimizers the reference knows."""
    return string if string in ("adam", "sgd", "momentum") else None


class _FallbackLatch:
    """Bookkeeping of persistent-recurrence failures.  A failed launch costs its bounded waits (seconds) plus a second
    run of the step, so a cause that does not go away - a shared GPU, a resident collective, anything that keeps 256
    workgroups from being co-resident - must not be paid on every step: after LATCH_AFTER consecutive failures the
    graph stays on the launch train for the rest of the run.  Every failure is logged."""
    LATCH_AFTER = 2
    AS_WELL = "LSTM recurrence failed on the launch train as well (status {status})"

    def __init__(self):
        self.consecutive, self.latched, self.total = 0, False, 0

    def run(self, fn, before_retry=None, error=AS_WELL, latched_error=None):
        """``fn() -> (result, status)``, status the LSTM status word behind it: the result of the first try when it is 0 -
        else, after ``before_retry()`` (the caller puts back what the failed try advanced), of a second one under
        ``ops.force_launch_train()``.  Latched, the only try is the forced one.  RuntimeError(``error``, or
        ``latched_error`` for a latched graph; ``{status}`` is filled in) when the launch train fails too."""
        latched = self.latched
        if not latched:
            result, status = fn()
            if status == 0:
                self.consecutive = 0
                return result
            self.failed(status)
            if before_retry is not None:
                before_retry()
        with ops.force_launch_train():
            result, status = fn()
        if status != 0:
            raise RuntimeError((latched_error if latched and latched_error else error).format(status=status))
        return result

    def failed(self, status):
        from . import tflog
        self.total += 1
        self.consecutive += 1
        self.latched = self.consecutive >= self.LATCH_AFTER
        tflog.info("persistent LSTM launch did not complete (status %d, fallback #%d); re-running the step with the "
                   "per-step launch train%s" % (status, self.total, (" - and staying on it for the rest of this run (%d "
                                                                     "failures in a row)" % self.consecutive)
                                                if self.latched else ""))


class _HostScalars:
    """The device scalars a step wants on the host, by name.  ``add`` collects one-element tensors of any dtype (float32 and
    int32 widen to float64 exactly), ``fetch`` moves all of them in ONE device-to-host copy - the step's single sync - and
    returns {name: Python float}."""

    def __init__(self):
        self.names, self.parts = [], []

    def add(self, name, t):
        if name in self.names:
            raise KeyError("host scalar %r collected twice" % name)
        self.names.append(name)
        self.parts.append(t.to(torch.float64).reshape(1))

    def fetch(self):
        return dict(zip(self.names, torch.cat(self.parts).cpu().tolist()))


def _checked_star_penalty(value):
    """``star_penalty`` as a pair of floats (bypass, self-loop), each a number - never a bool - that is >= 0 or +inf; else
    ValueError naming the keyword."""
    must_be = "a pair (bypass_penalty, selfloop_penalty) of floats >= 0 or +inf, or None"
    if not isinstance(value, (tuple, list)) or len(value) != 2:
        raise ValueError("star_penalty must be %s, got %r" % (must_be, value))
    for p in value:
        if isinstance(p, bool) or not isinstance(p, (int, float, np.integer, np.floating)) or not p >= 0:
            raise ValueError("star_penalty must be %s, got %r" % (must_be, value))
    return float(value[0]), float(value[1])


def _checked_number(name, value, lower, strict, must_be, integer=False):
    """``value`` as a float (``integer``: an int) when it is a finite number - never a bool - that is > ``lower`` (``strict``)
    or >= it; else ValueError("<name> must be <must_be>, got <value>")."""
    kinds = (int, np.integer) if integer else (int, float, np.integer, np.floating)
    if (isinstance(value, bool) or not isinstance(value, kinds) or not (integer or np.isfinite(value))
            or (not value > lower if strict else value < lower)):
        raise ValueError("%s must be %s, got %r" % (name, must_be, value))
    return int(value) if integer else float(value)


def _needs_ctc(keyword, verb, objective):
    if objective != "ctc":
        raise ValueError("%s %s the CTC criterion: it needs objective=\"ctc\", not \"%s\"" % (keyword, verb, objective))


class _CriterionOption(namedtuple("_CriterionOption", "keyword check verb under excuse op as_args keys counts totals minus_extra",
                                  defaults=(False,))):
    """One row of CRITERION_OPTIONS: an alternative form of the CTC criterion, of which a graph takes at most one.
    ``check(value)`` -> the value the graph keeps, or ValueError; ``verb`` fills "<keyword> <verb> the CTC criterion"; ``excuse``
    stands in parentheses when the option meets an EARLIER row (whose ``under`` fills its %(under)s); ``op`` names the
    ``ops`` function - looked up per call - that takes ``as_args(value)`` after max_label_len and returns (loss[B], extra[B],
    grad); ``keys`` are the two output keys, the sum of extra and the sum of ``counts`` ("labels" or "frames") over the
    utterances with a finite, non-skipped loss; ``totals`` the attributes that sum them over the steps; ``minus_extra``:
    eval_loss is (loss - value * extra).sum() instead of loss.sum()."""

    def call(self, value, logits, flat_d, offs_d, seq_d, maxlen, **kw):
        return getattr(ops, self.op)(logits, flat_d, offs_d, seq_d, maxlen, *self.as_args(value), **kw)


def _nonnegative(keyword):
    return lambda value: _checked_number(keyword, value, 0, False, "a finite float >= 0 or None")


# Adding an exclusive CTC criterion option: one row here (in the order the constructor checks them), its ``ops`` wrapper, its
# keyword in CTCGraph.__init__ - and its row in bin/_common.py CRITERION_FLAGS.
CRITERION_OPTIONS = {option.keyword: option for option in (
    _CriterionOption("delay_penalty", _nonnegative("delay_penalty"), "tilts", "delay tilt", None,
                     "ctc_loss_delay", lambda v: (v,), ("entry_sum", "entry_labels"), "labels",
                     ("entry_sum_total", "entry_labels_total")),
    _CriterionOption("entropy_weight", _nonnegative("entropy_weight"), "regularises", "entropy term",
                     "the entropy of the tilted path posterior is not built",
                     "ctc_loss_entropy", lambda v: (v,), ("path_entropy", "path_entropy_frames"), "frames",
                     ("path_entropy_total", "path_entropy_frames_total"), minus_extra=True),
    _CriterionOption("star_penalty", _checked_star_penalty, "relaxes", "star",
                     "the star under the %(under)s is not built",
                     "ctc_loss_star", tuple, ("star_frames", "star_frame_count"), "frames",
                     ("star_frames_total", "star_frame_count_total")),
)}


class CTCGraph:
    """Validation (and, with ``learn_rate``, training) graph over a batch pipeline.

    ``objective="ctc"`` is the reference's criterion.  ``objective="xent"`` (new, no reference counterpart) is the frame-level
    softmax cross-entropy against ``batch["frame_target"]`` [B,T] int32 (one symbol per frame as ``align`` writes them, the
    blank included; -1 = ignore): ``size`` is then the number of scored frames, ``eval_loss`` their summed -log p(target),
    ``eval`` the number of them the argmax gets wrong - so the run loops log the mean loss per frame and the frame error
    rate - and ``nnet_target`` is not read.

    ``align_window=N`` (new, ``objective="ctc"`` only; an int >= 0) is alignment-windowed CTC: the criterion is summed only
    over the paths that keep every label within N frames of the run ``batch["frame_target"]`` gives it
    (``ops.label_windows`` on the host, ``ops.ctc_loss_windowed`` where the step calls ``ops.ctc_loss``); an utterance whose
    row is all -1 or does not spell its labels trains on plain CTC.  ``windows_constrained`` / ``windows_unconstrained``
    count the utterances of either kind.  ``None`` is the unwindowed step, untouched.

    ``teacher_weight=lambda`` (new, ``objective`` "ctc" or "xent"; a finite float > 0) adds teacher-student distillation to the
    criterion: ``lambda * tau^2 * sum KL(softmax(teacher / tau) || softmax(logits / tau))`` over the frames that
    ``batch["teacher_scores"]`` [T,B,V] / ``batch["teacher_length"]`` [B] cover, tau = ``teacher_temperature``
    (``ops.kd_loss`` accumulating into the base criterion's gradient).  ``loss`` gains the term; ``eval_loss``, ``eval`` and
    ``size`` stay the base criterion's; the output gains ``kd_loss`` (the plain sum of KL), ``kd_frames`` and ``kd_agree``.
    ``objective="kd"`` is the term alone (lambda = 1): ``size`` is the number of scored frames, ``eval_loss`` = tau^2 * sum
    KL, ``eval`` the frames whose two argmaxes disagree, and ``nnet_target`` is not read.  ``kd_frames_total`` /
    ``kd_agree_total`` sum over the steps.  ``None`` is the step without the term, untouched.

    ``delay_penalty=lambda`` (new, ``objective="ctc"`` only; a finite float >= 0) is delay-penalised CTC: a path is weighted
    by ``exp(-lambda * sum of the frames at which its labels are entered)`` (``ops.ctc_loss_delay`` where the step calls
    ``ops.ctc_loss`` / ``ops.ctc_loss_windowed``; with ``align_window`` the windows go to it).  ``eval_loss`` / ``loss`` are the
    penalised criterion; the output gains ``entry_sum`` (the expected sum of the label entry frames under the criterion's
    path posterior) and ``entry_labels`` (the labels of the utterances with a finite, non-skipped loss), so that
    ``entry_sum / entry_labels`` is the mean frame at which a label is entered; ``entry_sum_total`` / ``entry_labels_total``
    sum over the steps.  0 is plain CTC plus the metric.  ``None`` is the step without it, untouched.

    ``entropy_weight=eta`` (new, ``objective="ctc"`` only; a finite float >= 0) is maximum-entropy CTC (Liu et al. 2018):
    the criterion is ``loss - eta * H``, H the entropy in nats of the posterior over the utterance's feasible paths
    (``ops.ctc_loss_entropy`` where the step calls ``ops.ctc_loss`` / ``ops.ctc_loss_windowed``; with ``align_window`` the
    windows go to it and H is the entropy over the paths inside them).  ``eval_loss`` / ``loss`` are that criterion; the output
    gains ``path_entropy`` (the float64 sum of H over the utterances with a finite, non-skipped loss) and
    ``path_entropy_frames`` (the sum of their sequence lengths), so that ``path_entropy / path_entropy_frames`` is the entropy
    in nats per utterance-frame; ``path_entropy_total`` / ``path_entropy_frames_total`` sum over the steps (each rank its
    own).  0 is plain CTC plus the metric.  It does not combine with ``delay_penalty`` (the entropy of the tilted posterior
    is not built).  ``None`` is the step without it, untouched.

    ``star_penalty=(pb, ps)`` (new, ``objective="ctc"`` only; each a float >= 0 or +inf) is transcript-tolerant CTC (after
    OTC / STC): every lattice position may explain a frame by a penalised star, "some non-blank class", instead of by its own
    class - a label position at ``exp(-pb)`` (the label is bypassed: a substituted or inserted label), a blank position at
    ``exp(-ps)`` (the blank absorbs speech: a deleted label) - so that wrong transcripts neither blow the loss up nor push
    correctly recognised frames towards the wrong label (``ops.ctc_loss_star`` where the step calls ``ops.ctc_loss`` /
    ``ops.ctc_loss_windowed``; with ``align_window`` the windows go to it).  ``eval_loss`` / ``loss`` are that criterion (it
    may be negative); the output gains ``star_frames`` (the float64 sum over the utterances with a finite, non-skipped loss of
    the expected number of frames the star explains) and ``star_frame_count`` (the sum of their sequence lengths);
    ``star_frames_total`` / ``star_frame_count_total`` sum over the steps (each rank its own).  It combines with neither
    ``delay_penalty`` nor ``entropy_weight``.  ``None`` is the step without it, untouched.

    ``spec_augment=SpecAugment(...)`` (new, training graphs, every objective; ``nnet.augment``) masks the input of every
    TRAINING step on the device: the model reads ``ops.spec_augment(x, ...)``, written OUT OF PLACE - the caller's ``x`` is
    never changed, so ``step_device`` callers may pass the same tensor step after step.  The draws are seeded with the step's
    ``drop_seed``: ranks and epochs differ, and a step re-run on the launch train repeats them.  The layout is
    ``left_context`` / ``right_context`` / ``subsample`` / ``input_dim`` of ``nnet_config``.  ``train=False`` steps and
    ``align`` never augment.  ``specaug_steps`` counts the augmented steps; ``specaug_frames_masked`` / ``specaug_frames`` and
    ``specaug_bins_masked`` / ``specaug_bins`` sum the masked and the live raw frames and bins over the steps whose sequence
    lengths were on the host (``step``; ``step_device`` with ``seq_host``).  ``None`` is the step without it, untouched.

    ``consistency_weight=alpha`` (new, ``objective="ctc"`` training graphs; a finite float > 0) is consistency-regularised
    CTC (CR-CTC, Yao et al. 2024).  Every TRAINING step runs on the batch with each utterance twice (``double_batch``:
    utterance b again in column b + B; spec-augment masks and dropout are hashes of the column, so the two copies are two
    independent views), takes the criterion (plain, windowed or delay-penalised) and the label-smoothing term on all 2B
    columns, and adds ``alpha * 0.5 * sum J``, J = KL(qb || qa) + KL(qa || qb) per frame of a pair, through
    ``ops.consistency_loss(logits, seq, grad_scale=0.5 * alpha, grad=grad)`` in its STOP-GRADIENT form (each view a fixed
    target for the other).  NORMALISATION: the project's loss is a SUM over utterances, so the step is exactly "a batch of 2B
    utterances plus alpha * 0.5 * J" - the CTC part is not halved; pick batch size and learning rate accordingly.  ``size``
    counts the labels of both views, ``eval_loss`` is the criterion summed over both, ``loss`` gains the term, ``eval`` (when
    fetched) is the edit distance of view a alone against the original labels, and ``eval_size`` comes with it: the number
    of those labels, half of ``size`` - the error RATE is ``eval / eval_size`` (the run loops divide by it), never ``eval /
    size``; ``sequence_length`` holds the lengths of both views, so that frames per second count what the device processed;
    the output gains ``cr_loss`` (the plain sum
    of J), ``cr_frames`` and ``cr_agree`` (frames of a pair scored / with equal argmaxes), in the step's one copy;
    ``cr_loss_total`` / ``cr_frames_total`` / ``cr_agree_total`` sum over the steps; the spec-augment shares count both
    views.  It needs two views that differ - ``spec_augment`` or dropout - and does not combine with ``teacher_weight``.
    ``train=False`` steps and ``align`` never double.  ``None`` is the step without it, untouched."""

    def __init__(self, pipeline, nnet_config, learn_rate=None, clip_norm=5.0, optimizer="sgd",
                 l2_decay_weight=1e-5, device="cuda", seed=None, process_group=None, objective="ctc", align_window=None,
                 teacher_weight=None, teacher_temperature=1.0, delay_penalty=None, spec_augment=None,
                 consistency_weight=None, entropy_weight=None, star_penalty=None):
        nnet_type = nnet_config.get("nnet_type")
        if get_create_logits(nnet_type) is None:
            raise ValueError("unsupported nnet_type: %s" % nnet_type)
        if objective not in ("ctc", "xent", "kd"):
            raise ValueError("unsupported objective: %s" % objective)
        self.objective = objective
        if teacher_weight is not None:
            if objective == "kd":
                raise ValueError("objective=\"kd\" is the distillation term alone (weight 1): it takes no teacher_weight")
            teacher_weight = _checked_number("teacher_weight", teacher_weight, 0, True, "a finite float > 0 or None")
        self.teacher_weight = teacher_weight
        self.teacher_temperature = _checked_number("teacher_temperature", teacher_temperature, 0, True, "finite and > 0")
        self.needs_teacher = objective == "kd" or teacher_weight is not None
        self.kd_frames_total = self.kd_agree_total = 0
        if align_window is not None:
            _needs_ctc("align_window", "constrains", objective)
            align_window = _checked_number("align_window", align_window, 0, False, "an int >= 0 (frames) or None",
                                           integer=True)
        self.align_window = align_window
        self.windows_constrained = self.windows_unconstrained = 0
        given = dict(delay_penalty=delay_penalty, entropy_weight=entropy_weight, star_penalty=star_penalty)
        self._criterion_option = None                    # at most one row of CRITERION_OPTIONS
        for option in CRITERION_OPTIONS.values():
            value = given[option.keyword]
            if value is not None:
                _needs_ctc(option.keyword, option.verb, objective)
                value = option.check(value)
                earlier = self._criterion_option
                if earlier is not None:
                    raise ValueError("%s does not combine with %s (%s)"
                                     % (option.keyword, earlier.keyword, option.excuse % {"under": earlier.under}))
                self._criterion_option = option
            setattr(self, option.keyword, value)
            setattr(self, option.totals[0], 0.0)
            setattr(self, option.totals[1], 0)
        self.spec_layout = None
        if spec_augment is not None:
            from . import augment
            if not isinstance(spec_augment, augment.SpecAugment):
                raise ValueError("spec_augment must be an nnet.augment.SpecAugment or None, got %r" % (spec_augment,))
            self.spec_layout = augment.layout_of(nnet_config)
            spec_augment.check_layout(self.spec_layout.base_dim)           # ValueError: freq_bins must divide input_dim
        self.spec_augment = spec_augment
        self.specaug_steps = 0
        if consistency_weight is not None:
            _needs_ctc("consistency_weight", "pairs two views under", objective)
            consistency_weight = _checked_number("consistency_weight", consistency_weight, 0, True,
                                                 "a finite float > 0 or None")
            if teacher_weight is not None:
                raise ValueError("consistency_weight does not combine with teacher_weight (a doubled teacher tensor is not built)")
            if spec_augment is None and config_keep(nnet_config) >= 1.0:
                raise ValueError("consistency_weight needs two views that differ: spec_augment or dropout (the model has "
                                 "neither, the term would be 0)")
        self.consistency_weight = consistency_weight
        self.cr_loss_total, self.cr_frames_total, self.cr_agree_total = 0.0, 0, 0
        self.specaug_frames_masked = self.specaug_frames = self.specaug_bins_masked = self.specaug_bins = 0
        self.pipeline = pipeline
        # pyramidal BiLSTM (time_reduce_layers): the logits come at 1 / R of the input's frame rate, so whatever brings a
        # table at the input's rate is refused - frame targets, alignment windows, teacher scores - before anything is built
        if time_reduce_config(nnet_config)[0]:
            tabled = [name for name, on in (("objective = %s" % objective, objective != "ctc"),
                                            ("align_window", align_window is not None),
                                            ("teacher_weight", teacher_weight is not None)) if on]
            if tabled:
                raise ValueError("time_reduce_layers does not combine with %s: its table is at the input's frame rate, the "
                                 "logits are not (re-timed tables are not built)" % ", ".join(tabled))
        self.model = Model(nnet_config, device, seed=seed)
        self.time_reduce_short = 0       # utterances whose labels (+ adjacent repeats) no longer fit the output frames
        self.training = learn_rate is not None
        self.learn_rate = learn_rate
        self.clip_norm = clip_norm
        self.l2 = l2_decay_weight
        self.optimizer = optimizer
        if self.training and get_optimizer(optimizer) is None:
            raise ValueError("unsupported optimizer: %s" % optimizer)
        self.pg = process_group
        self.world = dp.world_size(process_group)
        self.global_step = 0
        self.opt_step = 0          # Adam's t: restarts with the process, like the reference (nnet-train.py:83)
        dev = self.model.device
        n = self.model.ps.n
        slots = {"sgd": 0, "momentum": 1, "adam": 2}.get(optimizer, 0) if self.training else 0
        self.opt_state = torch.zeros(max(slots * n, 1), dtype=torch.float32, device=dev)
        self.norm_out = torch.zeros(2, dtype=torch.float32, device=dev)
        # Dropout stream: every rank draws its own masks (rank r's utterance b must not share rank 0's noise), while
        # the INIT seed above stays common to all ranks so that the replicas start identical.
        self.rank = dp.rank(process_group)
        self.drop_seed = 0 if seed is None else int(seed)
        if self.world > 1:
            self.drop_seed = (self.drop_seed * 0x9E3779B1 + (self.rank + 1) * 0x85EBCA6B) & 0x7FFFFFFF
        self._fallback = _FallbackLatch()
        # per-layer gradient buckets, all-reduced beside the lower layers' weight-gradient GEMMs (dp.GradientBuckets);
        # LC_DP_BUCKETS=0: one all-reduce of the whole flat gradient after the backward
        import os
        self.dp_buckets = os.environ.get("LC_DP_BUCKETS", "1") != "0"
        self._force_buckets = os.environ.get("LC_DP_BUCKETS") == "2"      # also with a single rank (the RCCL test)
        self._buckets = None
        # label-smoothing regulariser (bilstm.py:255-269; blstm only): uniform wins over prior, like the elif there
        self.sm_weight, self.sm_logq = 0.0, None
        if nnet_type == "blstm":
            self.sm_weight, self.sm_logq = _label_smoothing_setup(nnet_config, dev)
        self.keys = ["nnet_input", "sequence_length", "logits", "raw_target", "nnet_target", "size", "eval_loss",
                     "loss", "eval", "global_step", "summary"] + (["lrate", "train"] if self.training else [])
        if self.model.time_factor > 1:
            self.keys.append("output_length")            # ceil(sequence_length / R): the lengths of the logits
        if self.consistency_weight is not None:
            self.keys.append("eval_size")               # what ``eval`` is to be divided by: ``size`` counts both views

    # the reference's graph is a dict; give the same key access
    def __contains__(self, key):
        return key in self.keys

    def __getitem__(self, key):
        if key not in self.keys:
            raise KeyError(key)
        return key

    @property
    def persist_fallbacks(self):
        """Steps re-run on the launch train after a persistent launch failed."""
        return self._fallback.total

    # -------------------------------------------------------------------------------------------------
    def _upload(self, batch):
        dev = self.model.device
        a = batch["nnet_input"]
        if (isinstance(a, np.ndarray) and a.dtype == np.float32 and a.ndim == 3
                and a.transpose(1, 0, 2).flags.c_contiguous):
            # the batching pipeline's buffer: time-major (page-locked) memory seen through a [B,T,D] view - one DMA
            x = torch.from_numpy(a.transpose(1, 0, 2)).to(dev, non_blocking=True)
        else:
            x = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
            x = x.to(dev, non_blocking=True).permute(1, 0, 2).contiguous()       # [B,T,D] -> time-major [T,B,D]
        seq = np.ascontiguousarray(batch["sequence_length"], dtype=np.int32)
        flat, offs, maxlen = flatten_labels(batch["nnet_target"])
        d = lambda a: torch.from_numpy(a).to(dev, non_blocking=True)
        return x, d(seq), seq, d(flat), d(offs), flat, offs, maxlen

    def _upload_frame_target(self, batch):
        """objective = xent: (device [B,T] int32, the same on the host) of ``batch["frame_target"]``.  A pure copy."""
        ft = np.ascontiguousarray(batch["frame_target"], dtype=np.int32)
        return torch.from_numpy(ft).to(self.model.device, non_blocking=True), ft

    def _upload_teacher(self, batch):
        """teacher_weight / objective = kd: (teacher [T,B,V] f32, teacher_length [B] i32) on the device, (None, None) when the
        batch carries none (``step`` raises for that).  Pure copies."""
        ts = batch.get("teacher_scores")
        if ts is None or batch.get("teacher_length") is None:
            return None, None
        dev = self.model.device
        ts = np.ascontiguousarray(ts, dtype=np.float32)
        tl = np.ascontiguousarray(batch["teacher_length"], dtype=np.int32)
        return torch.from_numpy(ts).to(dev, non_blocking=True), torch.from_numpy(tl).to(dev, non_blocking=True)

    def _upload_windows(self, batch, flat, offs, seq):
        """align_window: (win_lo, win_hi on the device, constrained [B] on the host) from ``batch["frame_target"]``; (None,
        None, None) when the batch carries none (``step`` raises for that).  A pure function of the batch plus copies:
        ``ops.label_windows`` never raises for content."""
        ft = batch.get("frame_target")
        if ft is None:
            return None, None, None
        lo, hi, constrained = ops.label_windows(np.asarray(ft), flat, offs, seq, self.align_window, self.model.ps.V - 1)
        d = lambda a: torch.from_numpy(a).to(self.model.device, non_blocking=True)
        return d(lo), d(hi), constrained

    def _raise_together(self, bad, mine, theirs):
        """Under data parallelism every rank must leave the step together (a rank that raised alone would strand the others
        in the gradient collectives), so the verdict is summed over the group first."""
        if self.pg is not None and self.world > 1:
            flag = torch.tensor([int(bad)], dtype=torch.int32, device=self.model.device)
            dp.allreduce_sum_(flag, self.pg)
            bad_anywhere = int(flag.item()) != 0
        else:
            bad_anywhere = bad
        if bad_anywhere:
            raise ValueError(mine() if bad else theirs)

    def _validate_frame_targets(self, ft, seq):
        """objective = xent: a live frame's target must lie in [-1, V) (-1 = ignore; the blank V - 1 is a legal target).  Like
        _validate_labels: for the batch being CONSUMED, one verdict for all ranks.  (The kernel alone would turn such a target
        into a NaN loss.)"""
        V = self.model.ps.V
        live = ft[np.arange(ft.shape[1])[None, :] < np.asarray(seq)[:, None]] if ft.size else ft.reshape(-1)
        bad = bool(live.size and (int(live.min()) < -1 or int(live.max()) >= V))
        self._raise_together(bad, lambda: "frame_target holds a symbol outside [-1, %d): min %d, max %d (num_targets = %d)"
                             % (V, int(live.min()), int(live.max()), V),
                             "another rank's frame_target holds a symbol outside [-1, %d)" % V)

    def _validate_labels(self, flat):
        """tf.nn.ctc_loss raises InvalidArgument for labels outside [0, num_classes - 1) (the blank, V - 1, is not a label).
        Done in ``step`` for the batch being CONSUMED - not while batch k + 1 is staged, which would raise before step k has
        trained and been reported, and would run a collective on the copy stream.  Under data parallelism every rank must
        leave the step together (a rank that raised alone would strand the others in the gradient collectives), so the verdict
        is summed over the group first."""
        V = self.model.ps.V
        bad = bool(flat.size and (int(flat.min()) < 0 or int(flat.max()) >= V - 1))
        self._raise_together(bad, lambda: "nnet_target holds a label outside [0, %d): min %d, max %d (num_targets = %d, "
                             "blank = %d)" % (V - 1, int(flat.min()), int(flat.max()), V, V - 1),
                             "another rank's nnet_target holds a label outside [0, %d)" % (V - 1))

    def _upload_all(self, batch):
        """What ``step`` consumes of ``batch``, by name: the eight values of ``_upload`` plus ``frame_target`` (device, host;
        objective = xent), ``windows`` (lo, hi on the device, constrained on the host; align_window) and ``teacher`` (scores,
        length on the device) - each None when the graph does not use it or the batch carries none (``step`` raises for
        that).  Copies and ``ops.label_windows``: nothing here raises for the batch's CONTENT."""
        x, seq_d, seq, flat_d, offs_d, flat, offs, maxlen = self._upload(batch)
        up = SimpleNamespace(x=x, seq_d=seq_d, seq=seq, flat_d=flat_d, offs_d=offs_d, flat=flat, offs=offs, maxlen=maxlen,
                             frame_target=None, windows=None, teacher=None)
        if self.objective == "xent":
            up.frame_target = self._upload_frame_target(batch)
        elif self.align_window is not None:
            windows = self._upload_windows(batch, flat, offs, seq)
            up.windows = None if windows[0] is None else windows
        if self.needs_teacher:
            teacher = self._upload_teacher(batch)
            up.teacher = None if teacher[0] is None else teacher
        return up

    def stage(self, batch):
        """Uploads ``batch`` on a side stream NOW, to be consumed by a later ``step(None, staged=...)``: called for batch
        k + 1 before step k is enqueued, the copy runs under step k's kernels instead of in front of step k + 1's.  Pure
        copies: nothing here can raise for batch k + 1's CONTENT or touch the process group (see _validate_labels)."""
        dev = self.model.device
        if getattr(self, "_h2d_stream", None) is None:
            self._h2d_stream = torch.cuda.Stream(dev)
        with torch.cuda.stream(self._h2d_stream):
            up = self._upload_all(batch)
            ev = torch.cuda.Event()
            ev.record()
        return up, ev

    def step(self, batch, fetch_eval=True, fetch_logits=False, train=None, staged=None):
        """One sess.run of the graph on one batch (dict of numpy arrays in the pipeline contract of
        nnet/pipeline.py:35-61; or ``staged``, the result of an earlier ``stage(batch)``).  Returns a dict of host
        values."""
        if staged is not None:
            up, ev = staged
            cur = torch.cuda.current_stream(self.model.device)
            cur.wait_event(ev)
            for field in vars(up).values():
                for t in field if isinstance(field, tuple) else (field,):
                    if torch.is_tensor(t):
                        t.record_stream(cur)      # allocated on the copy stream, consumed on this one
        else:
            up = self._upload_all(batch)
        if self.needs_teacher and up.teacher is None:
            raise ValueError("teacher_weight / objective = kd needs teacher_scores and teacher_length in the batch "
                             "(create_pipeline_sequence_batch(..., teacher_scores=...))")
        frame_target = windows = None
        if self.objective == "xent":                  # reads no nnet_target: has_label = 0 corpora are fine
            frame_target, ft_host = up.frame_target
            self._validate_frame_targets(ft_host, up.seq)
        elif self.objective == "ctc":                 # (kd reads neither)
            self._validate_labels(up.flat)
            if self.align_window is not None:
                if up.windows is None:
                    raise ValueError("align_window needs frame_target in the batch "
                                     "(create_pipeline_sequence_batch(..., frame_targets=...))")
                lo_d, hi_d, constrained = up.windows
                windows = (lo_d, hi_d)
                self.windows_constrained += int(constrained.sum())
                self.windows_unconstrained += int(len(constrained) - constrained.sum())
        out = self.step_device(up.x, up.seq_d, up.flat_d, up.offs_d, up.maxlen, int(len(up.flat)), fetch_eval=fetch_eval,
                               fetch_logits=fetch_logits, train=train, flat_host=up.flat, offs_host=up.offs, seq_host=up.seq,
                               frame_target=frame_target, windows=windows, teacher=up.teacher)
        out["sequence_length"] = np.concatenate([up.seq, up.seq]) if "cr_loss" in out else up.seq   # what the device processed
        if self.model.time_factor > 1:                    # the lengths of the logits, of ``decoded`` and of every loss term
            out["output_length"] = self.model.output_lengths(out["sequence_length"])
        return out

    def step_device(self, x, seq_d, flat_d, offs_d, maxlen, size, fetch_eval=False, fetch_logits=False, train=None,
                    flat_host=None, offs_host=None, seq_host=None, frame_target=None, windows=None, teacher=None):
        """The same step on tensors already resident in HBM: x [T,B,D] time-major f32, seq_d [B] i32,
        labels flat i32 + offsets [B+1] i32.  seq_host: seq_d's values on the host, when the caller has them (pack_frames
        then builds a new batch's frame map without a device-to-host copy).  frame_target: [B,T] i32 on the device, the
        targets of objective = xent (labels / offsets / size are then not used).  windows: (win_lo, win_hi) int32 on the device,
        parallel to the labels - required when the graph was built with align_window.  teacher: (scores [T,B,V] f32 in the
        log domain, teacher_length [B] i32) on the device - required with teacher_weight and under objective = kd.

        A persistent-recurrence launch that cannot complete (lstm_ctc_hip.h: bounded waits, sticky status word) leaves
        NaN outputs and makes the optimizer skip its update on the device; the word is read at the step's one sync
        point and the step is then re-run, in this process, with the per-step launch train."""
        train = self.training if train is None else train
        if self.align_window is not None and windows is None:
            raise ValueError("align_window needs the label windows (step: frame_target in the batch, frame_targets= of the "
                             "pipeline; step_device: windows=)")
        if self.needs_teacher and (teacher is None or teacher[0] is None):
            raise ValueError("teacher_weight / objective = kd needs the teacher scores (step: teacher_scores in the batch, "
                             "teacher_scores= of the pipeline; step_device: teacher=)")
        b = SimpleNamespace(x=x, seq_d=seq_d, flat_d=flat_d, offs_d=offs_d, maxlen=maxlen, size=size, flat=flat_host,
                            offs=offs_host, seq=seq_host, frame_target=frame_target, windows=windows, teacher=teacher,
                            pairs=None)
        counters = (self.global_step, self.drop_seed, self.opt_step)

        def restore():
            self.global_step, self.drop_seed, self.opt_step = counters

        return self._fallback.run(lambda: self._step_once(b, fetch_eval=fetch_eval, fetch_logits=fetch_logits, train=train),
                                  before_retry=restore,       # (latched: co-residency is structurally unavailable)
                                  latched_error="LSTM recurrence failed on the launch train (status {status})")

    def _step_once(self, b, fetch_eval, fetch_logits, train):
        """One try of the step on ``b``, the arguments of ``step_device`` by name (``flat`` / ``offs`` / ``seq``: the host's
        copies or None): (outputs, 0), or (None, status) when a recurrence failed.  ``b`` is not changed - the retry reads it
        again."""
        ops.lstm_status(self.model.device).zero_()
        self.global_step += 1
        self.drop_seed = (self.drop_seed * 1664525 + 1013904223) & 0x7FFFFFFF
        if train and self.consistency_weight is not None:    # every utterance twice; out of place: the caller keeps its x
            x = torch.cat([b.x, b.x], dim=1)
            lo_d, hi_d = b.windows if b.windows is not None else (None, None)
            seq_d, flat_d, offs_d, lo_d, hi_d = double_batch(b.seq_d, b.flat_d, b.offs_d, lo_d, hi_d)
            flat, offs = b.flat, b.offs
            if offs is not None:
                _, flat, offs, _, _ = double_batch(None, flat, np.asarray(offs))
            b = SimpleNamespace(**dict(vars(b), x=x, seq_d=seq_d, flat_d=flat_d, offs_d=offs_d, flat=flat, offs=offs,
                                       seq=None if b.seq is None else np.concatenate([b.seq, b.seq]), size=2 * b.size,
                                       windows=None if b.windows is None else (lo_d, hi_d),
                                       pairs=b.seq_d))           # pairs: the [B] lengths; everything else is the 2B batch
        x, specaug_counts = b.x, None
        if train and self.spec_augment is not None:          # out of place: the caller keeps its x
            x = ops.spec_augment(x, b.seq_d, self.spec_augment, self.spec_layout, self.drop_seed)
            if b.seq is not None:
                from . import augment
                sub = self.spec_layout.subsample
                specaug_counts = augment.masked_shares(augment.mask_plan(self.drop_seed, b.seq, self.spec_augment, sub),
                                                       b.seq, self.spec_augment, sub)
        logits = self.model.forward(x, b.seq_d, drop_seed=self.drop_seed, seq_len_host=b.seq)      # [T,B,V]
        short = 0
        if self.model.time_factor > 1:
            # pyramidal BiLSTM: the logits are [ceil(T / R), B, V].  EVERYTHING that reads them from here on - criterion,
            # greedy decode, consistency term, the criterion options' sums - gets the OUTPUT lengths, on the device and on the
            # host: a loss kernel walking input lengths over these logits would read past the buffer
            out_len = self.model.output_lengths
            short = self._time_reduce_short(b, out_len)
            T_out = logits.shape[0]
            b = SimpleNamespace(**dict(vars(b), seq_d=out_len(b.seq_d).clamp_(max=T_out),
                                       seq=None if b.seq is None else np.minimum(out_len(b.seq), T_out),
                                       pairs=None if b.pairs is None else out_len(b.pairs).clamp_(max=T_out)))
            assert logits.shape[0] == self.model.output_frames(x.shape[0]), (tuple(logits.shape), tuple(x.shape))
        out, status = self._finish_step(logits, b, fetch_eval=fetch_eval, fetch_logits=fetch_logits, train=train)
        if status == 0:
            self.time_reduce_short += short
        if status == 0 and train and self.spec_augment is not None:          # a failed step is re-run: count it once
            self.specaug_steps += 1
            if specaug_counts is not None:
                self.specaug_frames_masked += specaug_counts[0]
                self.specaug_frames += specaug_counts[1]
                self.specaug_bins_masked += specaug_counts[2]
                self.specaug_bins += specaug_counts[3]
        return out, status

    @staticmethod
    def _time_reduce_short(b, out_len):
        """How many utterances of the step no longer fit the logits of a pyramidal model: labels + adjacent repeats (each
        needs a blank between) > output length.  From the host's labels and lengths (0 when the step has none: step_device
        without them); under consistency_weight each utterance counts once.  The criteria handle these themselves - loss 0
        when skipped, +inf without a path."""
        if b.flat is None or b.offs is None or b.seq is None:
            return 0
        flat, offs, frames = np.asarray(b.flat), np.asarray(b.offs), out_len(b.seq)
        n = len(frames) if b.pairs is None else int(b.pairs.numel())
        short = 0
        for u in range(n):
            lab = flat[offs[u]:offs[u + 1]]
            short += int(len(lab) + int((lab[1:] == lab[:-1]).sum()) > int(frames[u]))
        return short

    KD_KEYS = ("kd_loss", "kd_frames", "kd_agree")          # the teacher term's outputs (objective = kd: the criterion's)
    CR_KEYS = ("cr_loss", "cr_frames", "cr_agree")           # the consistency term's

    # A criterion calls its ``ops.*`` loss on the logits and returns (grad, scalars, outputs): the gradient buffer that the
    # shared terms accumulate into (None when not training); ``scalars()`` -> the (name, device scalar) pairs it wants on the
    # host, reduced at the step's one copy; ``outputs(host, out, fetch_eval)`` writing size, eval_loss, eval and its own keys
    # into ``out`` from the fetched {name: float} - and adding to its ``*_total`` counters, so only for a step that completed.
    def _ctc_criterion(self, logits, b, train):
        option = self._criterion_option
        lo_d, hi_d = b.windows if self.align_window is not None else (None, None)
        extra_b = None
        if option is not None:
            value = getattr(self, option.keyword)
            loss_b, extra_b, grad = option.call(value, logits, b.flat_d, b.offs_d, b.seq_d, b.maxlen, win_lo=lo_d, win_hi=hi_d,
                                                want_grad=train)
        elif self.align_window is not None:
            loss_b, grad = ops.ctc_loss_windowed(logits, b.flat_d, b.offs_d, b.seq_d, b.maxlen, lo_d, hi_d, want_grad=train)
        else:
            loss_b, grad = ops.ctc_loss(logits, b.flat_d, b.offs_d, b.seq_d, b.maxlen, want_grad=train)

        def scalars():
            if option is None:
                return [("eval_loss", loss_b.sum())]                             # graph.py:116 reduce_sum, in float32
            total = (loss_b - value * extra_b if option.minus_extra else loss_b).sum()
            labels_b = (b.offs_d[1:] - b.offs_d[:-1]).to(torch.int64)
            sums = self._selected_sums(loss_b, extra_b, labels_b, b.seq_d, labels_b if option.counts == "labels" else b.seq_d)
            return [("eval_loss", total)] + list(zip(option.keys, sums))

        def outputs(host, out, fetch_eval):                  # (``eval`` needs the greedy decode: the tail's)
            out["size"], out["eval_loss"] = b.size, host["eval_loss"]
            if option is not None:
                for key, total, kind in zip(option.keys, option.totals, (float, int)):
                    out[key] = kind(host[key])
                    setattr(self, total, getattr(self, total) + out[key])
        return grad, scalars, outputs

    def _xent_criterion(self, logits, b, train):
        """``size`` the scored frames, ``eval`` those the argmax gets wrong.  A batch without a scored frame (size 0) still
        runs the optimizer step - on a zero loss gradient - so that ranks stay in lockstep (kd alike)."""
        if b.frame_target is None:
            raise ValueError("objective = xent needs frame_target (create_pipeline_sequence_batch(..., frame_targets=...))")
        loss_b, frames, correct, grad = ops.xent_loss(logits, b.frame_target, b.seq_d, want_grad=train)

        def outputs(host, out, fetch_eval):
            out["size"], out["eval_loss"] = int(host["frames"]), host["eval_loss"]
            if fetch_eval:
                out["eval"] = float(out["size"] - int(host["correct"]))
        return grad, lambda: zip(("eval_loss", "frames", "correct"), self._f64_sums((loss_b, frames, correct))), outputs

    def _kd_criterion(self, logits, b, train):
        """The distillation term alone (lambda = 1): ``size`` the scored frames, ``eval`` those whose two argmaxes disagree."""
        tau = self.teacher_temperature
        loss_b, frames, agree, grad = ops.kd_loss(logits, b.teacher[0], b.seq_d, b.teacher[1], temperature=tau, grad_scale=tau,
                                                  want_grad=train)

        def outputs(host, out, fetch_eval):
            out["eval_loss"] = self._kd_outputs(out, host)
            out["size"] = out["kd_frames"]
            if fetch_eval:
                out["eval"] = float(out["kd_frames"] - out["kd_agree"])
        return grad, lambda: zip(self.KD_KEYS, self._f64_sums((loss_b, frames, agree))), outputs

    @staticmethod
    def _f64_sums(tensors):
        return [t.to(torch.float64).sum() for t in tensors]

    @staticmethod
    def _selected_sums(loss_b, extra_b, labels_b, seq_d, count_b):
        """A criterion option's two scalars: [float64 sum of extra_b, int64 sum of count_b] over the utterances with a finite,
        non-skipped loss (frames, and no more labels - labels_b, int64 - than frames).  count_b: labels_b for delay_penalty,
        seq_d for entropy_weight and star_penalty."""
        ok = torch.isfinite(loss_b) & (seq_d > 0) & (labels_b <= seq_d)
        zero = torch.zeros((), dtype=torch.float64, device=loss_b.device)
        count_b = count_b.to(torch.int64)
        return [torch.where(ok, extra_b.to(torch.float64), zero).sum(), torch.where(ok, count_b, torch.zeros_like(count_b)).sum()]

    def _kd_outputs(self, out, host):
        """Writes kd_loss / kd_frames / kd_agree into ``out`` and returns what the term adds to ``loss``."""
        tau = self.teacher_temperature
        out["kd_loss"], out["kd_frames"], out["kd_agree"] = host["kd_loss"], int(host["kd_frames"]), int(host["kd_agree"])
        self.kd_frames_total += out["kd_frames"]
        self.kd_agree_total += out["kd_agree"]
        return (1.0 if self.teacher_weight is None else self.teacher_weight) * tau * tau * out["kd_loss"]

    def _new_buckets(self):
        """The backward's per-layer gradient buckets (None: one all-reduce after it); ``_apply_gradients`` finishes them."""
        self._buckets = (dp.GradientBuckets(self.model.ps.grad, self.pg)
                         if self.pg is not None and self.dp_buckets and (self.world > 1 or self._force_buckets) else None)
        return self._buckets

    def _finish_step(self, logits, b, fetch_eval, fetch_logits, train):
        """What follows the forward in ``_step_once``, for every objective: criterion, the terms that share its gradient
        buffer - in this order, the bits depend on it - backward, optimizer, the step's ONE device-to-host copy."""
        criterion = {"ctc": self._ctc_criterion, "xent": self._xent_criterion, "kd": self._kd_criterion}[self.objective]
        grad, scalars, outputs = criterion(logits, b, train)
        T_, B_, V_ = logits.shape
        reg = kd = cr = tokens = None
        if self.sm_weight > 0:                                                   # graph.py:120-133: loss += reg
            reg = ops.label_smoothing(logits.view(T_ * B_, V_), self.sm_weight, self.sm_logq,
                                      grad.view(T_ * B_, V_) if train else None)
        if self.teacher_weight is not None:       # lambda * tau * (q - p) into the criterion's gradient (train=False: loss only)
            tau = self.teacher_temperature
            kd = ops.kd_loss(logits, b.teacher[0], b.seq_d, b.teacher[1], temperature=tau,
                             grad_scale=self.teacher_weight * tau, grad=grad if train else None, want_grad=False)[:3]
        if b.pairs is not None:                                                  # (teacher_weight is excluded)
            cr = ops.consistency_loss(logits, b.pairs, grad_scale=0.5 * self.consistency_weight, grad=grad)[:3]
        if fetch_eval and self.objective == "ctc":
            tokens, out_len = ops.ctc_greedy(logits, b.seq_d)
        bn_saved = None
        if train:
            bn_saved = dict(self.model.saved.get("bn") or {})
            self.model.backward(grad, buckets=self._new_buckets())
            self._apply_gradients()
        # everything the host wants, in ONE device->host copy: the step's single sync, like the reference's sess.run
        word = _HostScalars()
        for name, t in scalars():
            word.add(name, t)
        word.add("status", ops.lstm_status(self.model.device))
        if reg is not None:
            word.add("reg", reg)
        if train:
            word.add("grad_norm", self.norm_out[:1])
        for keys, term in ((self.KD_KEYS, kd), (self.CR_KEYS, cr)):
            for name, t in zip(keys, self._f64_sums(term or ())):
                word.add(name, t)
        host = word.fetch()
        status = int(host["status"])
        if status != 0:
            return None, status
        if train and bn_saved:
            self.model.update_moving_averages(bn_saved)   # batch-norm UPDATE_OPS (graph.py:194-196); only with use_bn
        out = {}
        outputs(host, out, fetch_eval)
        out["loss"] = out["eval_loss"] + host.get("reg", 0.0)
        if cr is not None:
            out["cr_loss"], out["cr_frames"], out["cr_agree"] = host["cr_loss"], int(host["cr_frames"]), int(host["cr_agree"])
            self.cr_loss_total += out["cr_loss"]
            self.cr_frames_total += out["cr_frames"]
            self.cr_agree_total += out["cr_agree"]
            out["loss"] += self.consistency_weight * 0.5 * out["cr_loss"]
        elif kd is not None:
            out["loss"] += self._kd_outputs(out, host)
        if tokens is not None:
            tok, n = tokens.cpu().numpy(), out_len.cpu().numpy()
            flat, offs = b.flat, b.offs
            if flat is None:
                flat, offs = b.flat_d.cpu().numpy(), b.offs_d.cpu().numpy()
            if b.pairs is not None:                        # view a against the original labels: the first halves
                B_ = b.pairs.numel()
                tok, n, offs = tok[:B_], n[:B_], offs[:B_ + 1]
                flat = flat[:offs[-1]]
                out["eval_size"] = b.size // 2             # the labels ``eval`` was counted against
            out["eval"] = float(ops.edit_distance_host(tok, n, flat, offs).sum())   # graph.py:143-150
            out["decoded"] = (tok, n)
        if fetch_logits:
            out["logits"] = logits.permute(1, 0, 2).cpu().numpy()                # reference layout [B,T,V]
        if train:
            out["grad_norm"] = host["grad_norm"]
        return out, 0

    # ------------------------------------------------------------------------------------------------- forced alignment
    def align(self, batch, star_penalty=None):
        """Best-path (Viterbi) CTC alignment of one batch in the pipeline contract - no reference counterpart.  One forward
        in inference mode (no dropout, batch-norm on its moving averages), then ``ops.ctc_align`` on the logits.  Returns
        host arrays: ``ali`` [B,T] int32 (symbol per frame, blank = V-1; -1 beyond an utterance's length and when its labels
        do not fit its frames), ``label_index`` [B,T] int32, ``score`` [B] float32 (-inf without a path) and
        ``sequence_length``.  Never trains: parameters, ``global_step`` and the dropout stream are left as they were.
        ``star_penalty=(pb, ps)`` (new) adds ``ctc_loss``, ``star_loss`` and ``star_frames``, each [B] float32: ``ops.ctc_loss``
        and ``ops.ctc_loss_star`` on the same logits, no gradient - what a per-utterance transcript report is written from;
        ``ali``, ``label_index`` and ``score`` are what they are without it."""
        star = CRITERION_OPTIONS["star_penalty"]
        if self.model.time_factor > 1:
            raise ValueError("time_reduce_layers does not combine with alignment: an alignment names a symbol per input frame, "
                             "the logits come once per %d of them" % self.model.time_factor)
        if star_penalty is not None:
            star_penalty = star.check(star_penalty)
        x, seq_d, seq, flat_d, offs_d, flat, offs, maxlen = self._upload(batch)
        self._validate_labels(flat)
        model, dev = self.model, self.model.device
        mode = (model.is_training, model.keep)
        model.is_training, model.keep = False, 1.0
        try:
            def run():
                ops.lstm_status(dev).zero_()
                logits = model.forward(x, seq_d, seq_len_host=seq)
                res = ops.ctc_align(logits, flat_d, offs_d, seq_d, maxlen)
                if star_penalty is not None:
                    plain, _ = ops.ctc_loss(logits, flat_d, offs_d, seq_d, maxlen, want_grad=False)
                    star_loss, star_frames, _ = star.call(star_penalty, logits, flat_d, offs_d, seq_d, maxlen, want_grad=False)
                    res = tuple(res) + (plain, star_loss, star_frames)
                return res, int(ops.lstm_status(dev).item())

            res = self._fallback.run(run)
        finally:
            model.is_training, model.keep = mode
        names = ("ali", "label_index", "score", "ctc_loss", "star_loss", "star_frames")
        out = {k: v.cpu().numpy() for k, v in zip(names, res)}
        out["sequence_length"] = seq
        return out

    def _apply_gradients(self):
        """L2 + clip_by_global_norm + optimizer.apply_gradients (graph.py:183-200), after the DP all-reduce.  The
        update is guarded by the LSTM status word: a step whose recurrence failed leaves parameters and slots alone.
        (Under DP every rank must skip together: the status words are summed with the gradient's collective.)"""
        ps = self.model.ps
        guard = ops.lstm_status(ps.flat.device)
        if self.pg is not None and self.world > 1:
            dp.allreduce_sum_(guard, self.pg)
        if getattr(self, "_buckets", None) is not None:
            self.last_bucket_ranges = len(self._buckets.done)      # per-layer ranges that went out during the backward
            self._buckets.finish()               # the layers' buckets went out during the backward; this is the rest
            self._buckets = None
        else:
            dp.allreduce_sum_(ps.grad, self.pg)
        self.opt_step += 1
        ops.optimizer_step(ps.flat, ps.grad, ps.n_decay, self.l2, self.clip_norm, self.optimizer, self.learn_rate,
                           self.opt_step, self.opt_state, self.norm_out, guard=guard)

    # ------------------------------------------------------------------------------------------------- checkpoints
    def save(self, path):
        save_params(self.model.ps, path)

    def restore(self, path):
        load_params(self.model.ps, path)


class InferenceGraph:
    """create_graph_for_inference — nnet/graph.py:212-241: one utterance per run, softmax(smooth*logits)."""

    def __init__(self, pipeline, nnet_config, smooth_factor=1.0, device="cuda"):
        cfg = dict(nnet_config)
        self.pipeline = pipeline
        self.model = Model(cfg, device)
        self.smooth = smooth_factor
        self._fallback = _FallbackLatch()
        self.keys = ["filename", "nnet_input", "sequence_length", "logits", "nnet_output"]

    persist_fallbacks = property(lambda self: self._fallback.total, doc=CTCGraph.persist_fallbacks.__doc__)

    def __getitem__(self, key):
        if key not in self.keys:
            raise KeyError(key)
        return key

    def forward_batch(self, feats_list):
        """feats_list: list of [T_i, D] float32 arrays -> list of (logits[T_i,V]) on the host, computed as ONE
        padded batch (result-identical to the reference's B=1 runs because padding is masked; SURVEY §8f NEXT-3)."""
        dev = self.model.device
        B = len(feats_list)
        T = max(f.shape[0] for f in feats_list)
        D = feats_list[0].shape[1]
        x = np.zeros((T, B, D), np.float32)
        for b, f in enumerate(feats_list):
            x[:f.shape[0], b] = f
        seq = np.asarray([f.shape[0] for f in feats_list], np.int32)
        xd, sd = torch.from_numpy(x).to(dev), torch.from_numpy(seq).to(dev)
        def run():
            ops.lstm_status(dev).zero_()
            out = self.model.forward(xd, sd)
            return out, int(ops.lstm_status(dev).item())

        # (pyramidal BiLSTM: the logits are [ceil(T / R), B, V] and the second value their lengths, ceil(T_i / R))
        return (self._fallback.run(run, error="LSTM recurrence failed on the launch train as well"),
                self.model.output_lengths(seq))

    def restore(self, path):
        load_params(self.model.ps, path)


def save_params(ps, path):
    """Single-file checkpoint at exactly ``path`` (the scripts pass an opaque prefix, scripts/train.sh:164,230):
    safetensors with the TF variable names and TF layouts (tf.trainable_variables only — no optimizer slots,
    like saver = tf.train.Saver(tf.trainable_variables()), bin/nnet-train.py:83)."""
    from safetensors.numpy import save_file
    tensors = {k: np.ascontiguousarray(v) for k, v in ps.export_tf().items()}
    save_file(tensors, path)


def load_params(ps, path):
    """``path`` is either this repository's single-file checkpoint (safetensors, TF variable names and layouts) or the
    PREFIX of a TensorFlow Saver checkpoint (``<path>.index`` + ``<path>.data-*``: what the reference's nnet-train.py
    wrote, bin/nnet-train.py:83,97) - a model trained there is continued or decoded here without TensorFlow."""
    import os
    from . import tf_checkpoint
    if not os.path.isfile(path) and tf_checkpoint.is_bundle(path):
        from . import tflog
        tflog.info("WARNING: reading a TensorFlow tensor-bundle checkpoint (%s.index / .data-*) without TensorFlow: this "
                   "reader is written from the format's definition and has only been tested against this repository's own "
                   "writer and hand-built streams, never against a file TensorFlow wrote - compare a validation loss with "
                   "the reference before relying on it" % path)
        ps.load_tf(tf_checkpoint.read_bundle(path))
        return
    from safetensors.numpy import load_file
    ps.load_tf(load_file(path))


# ----------------------------------------------------------------------------------------------------- reference-named factories
def _criterion_only(options):
    """A CTC factory's ``**criterion``: the keywords of CRITERION_OPTIONS pass to CTCGraph, anything else is the TypeError of a
    keyword the factory does not take (a validation graph takes no spec_augment, say)."""
    for name in options:
        if name not in CRITERION_OPTIONS:
            raise TypeError("got an unexpected keyword argument %r" % name)
    return options


def create_graph_for_validation_ctc(pipeline, nnet_config, device="cuda", seed=None, align_window=None,
                                    teacher_weight=None, teacher_temperature=1.0, **criterion):
    return CTCGraph(pipeline, nnet_config, device=device, seed=seed, align_window=align_window,
                    teacher_weight=teacher_weight, teacher_temperature=teacher_temperature, **_criterion_only(criterion))


def create_graph_for_training_ctc(pipeline, nnet_config, learn_rate, clip_norm=5.0, optimizer="sgd",
                                  l2_decay_weight=1e-5, device="cuda", seed=None, process_group=None, align_window=None,
                                  teacher_weight=None, teacher_temperature=1.0, spec_augment=None, consistency_weight=None,
                                  **criterion):
    return CTCGraph(pipeline, nnet_config, learn_rate=learn_rate, clip_norm=clip_norm, optimizer=optimizer,
                    l2_decay_weight=l2_decay_weight, device=device, seed=seed, process_group=process_group,
                    align_window=align_window, teacher_weight=teacher_weight, teacher_temperature=teacher_temperature,
                    spec_augment=spec_augment, consistency_weight=consistency_weight, **_criterion_only(criterion))


def create_graph_for_validation_xent(pipeline, nnet_config, device="cuda", seed=None, teacher_weight=None,
                                     teacher_temperature=1.0):
    """Frame cross-entropy against the pipeline's ``frame_target`` (new, no reference counterpart)."""
    return CTCGraph(pipeline, nnet_config, device=device, seed=seed, objective="xent", teacher_weight=teacher_weight,
                    teacher_temperature=teacher_temperature)


def create_graph_for_training_xent(pipeline, nnet_config, learn_rate, clip_norm=5.0, optimizer="sgd",
                                   l2_decay_weight=1e-5, device="cuda", seed=None, process_group=None, teacher_weight=None,
                                   teacher_temperature=1.0, spec_augment=None):
    return CTCGraph(pipeline, nnet_config, learn_rate=learn_rate, clip_norm=clip_norm, optimizer=optimizer,
                    l2_decay_weight=l2_decay_weight, device=device, seed=seed, process_group=process_group,
                    objective="xent", teacher_weight=teacher_weight, teacher_temperature=teacher_temperature,
                    spec_augment=spec_augment)


def create_graph_for_validation_kd(pipeline, nnet_config, device="cuda", seed=None, teacher_temperature=1.0):
    """Distillation alone against the pipeline's ``teacher_scores`` (new, no reference counterpart)."""
    return CTCGraph(pipeline, nnet_config, device=device, seed=seed, objective="kd",
                    teacher_temperature=teacher_temperature)


def create_graph_for_training_kd(pipeline, nnet_config, learn_rate, clip_norm=5.0, optimizer="sgd",
                                 l2_decay_weight=1e-5, device="cuda", seed=None, process_group=None, teacher_temperature=1.0,
                                 spec_augment=None):
    return CTCGraph(pipeline, nnet_config, learn_rate=learn_rate, clip_norm=clip_norm, optimizer=optimizer,
                    l2_decay_weight=l2_decay_weight, device=device, seed=seed, process_group=process_group,
                    objective="kd", teacher_temperature=teacher_temperature, spec_augment=spec_augment)


def create_graph_for_alignment(pipeline, nnet_config, device="cuda"):
    """A CTCGraph that is only asked to ``align`` (new, no reference counterpart): no optimizer, no dropout."""
    if time_reduce_config(nnet_config)[0]:
        raise ValueError("time_reduce_layers does not combine with alignment: an alignment names a symbol per input frame, "
                         "the logits come once per R of them")
    return CTCGraph(pipeline, dict(nnet_config, is_training=False), device=device)


def create_graph_for_inference(pipeline, nnet_config, smooth_factor=1.0, device="cuda"):
    return InferenceGraph(pipeline, nnet_config, smooth_factor=smooth_factor, device=device)


class Session:
    """Stands in for tf.Session in the run loops: ``run(nodes)`` executes the graph on the next batch of
    its pipeline and returns {key: value} for the requested keys; raises OutOfRangeError at end of data."""

    def __init__(self, graph):
        self.graph = graph
        self._it = None
        self._ahead = None           # the NEXT batch, already on its way to the device

    def _stage_next(self):
        try:
            batch = next(self._it)
        except StopIteration:
            return None
        return self.graph.stage(batch) if hasattr(self.graph, "stage") else (batch,)

    def run(self, nodes):
        if self._it is None:
            self._it = iter(self.graph.pipeline)
            self._ahead = self._stage_next()
        cur = self._ahead
        if cur is None:
            raise OutOfRangeError()
        self._ahead = self._stage_next()        # batch k + 1 starts its upload before step k is enqueued
        want = set(nodes.values()) if isinstance(nodes, dict) else set(nodes)
        kw = dict(fetch_eval=("eval" in want), fetch_logits=("logits" in want), train=("train" in want))
        res = self.graph.step(cur[0], **kw) if len(cur) == 1 else self.graph.step(None, staged=cur, **kw)
        res["train"] = None
        res["summary"] = None
        if isinstance(nodes, dict):
            return {k: res.get(v) for k, v in nodes.items()}
        return [res.get(v) for v in nodes]
