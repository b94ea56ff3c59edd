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
import numpy as np
import torch

from .. import ops
from . import dp
from .model import Model, config_keep


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

    def __init__(self):
        self.consecutive, self.latched = 0, False

    def good(self):
        self.consecutive = 0

    def failed(self, status, total):
        from . import tflog
        self.consecutive += 1
        self.latched = self.consecutive >= self.LATCH_AFTER
        tflog.info("persistent LSTM launch did not complete (status %d, fallback #%d); re-running the step with the "
                   "per-step launch train%s" % (status, total, (" - and staying on it for the rest of this run (%d "
                                                                "failures in a row)" % self.consecutive)
                                                if self.latched else ""))


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
                 consistency_weight=None):
        nnet_type = nnet_config.get("nnet_type")
        if get_create_logits(nnet_type) is None:
            raise ValueError("unsupported nnet_type: %s" % nnet_type)
        if objective not in ("ctc", "xent", "kd"):
            raise ValueError("unsupported objective: %s" % objective)
        self.objective = objective
        if teacher_weight is not None:
            if objective == "kd":
                raise ValueError("objective=\"kd\" is the distillation term alone (weight 1): it takes no teacher_weight")
            if (isinstance(teacher_weight, bool) or not isinstance(teacher_weight, (int, float, np.integer, np.floating))
                    or not np.isfinite(teacher_weight) or not teacher_weight > 0):
                raise ValueError("teacher_weight must be a finite float > 0 or None, got %r" % (teacher_weight,))
            teacher_weight = float(teacher_weight)
        if (isinstance(teacher_temperature, bool) or not isinstance(teacher_temperature, (int, float, np.integer, np.floating))
                or not np.isfinite(teacher_temperature) or not teacher_temperature > 0):
            raise ValueError("teacher_temperature must be finite and > 0, got %r" % (teacher_temperature,))
        self.teacher_weight = teacher_weight
        self.teacher_temperature = float(teacher_temperature)
        self.needs_teacher = objective == "kd" or teacher_weight is not None
        self.kd_frames_total = self.kd_agree_total = 0
        if align_window is not None:
            if objective != "ctc":
                raise ValueError("align_window constrains the CTC criterion: it needs objective=\"ctc\", not \"%s\"" % objective)
            if isinstance(align_window, bool) or not isinstance(align_window, (int, np.integer)) or align_window < 0:
                raise ValueError("align_window must be an int >= 0 (frames) or None, got %r" % (align_window,))
            align_window = int(align_window)
        self.align_window = align_window
        self.windows_constrained = self.windows_unconstrained = 0
        if delay_penalty is not None:
            if objective != "ctc":
                raise ValueError("delay_penalty tilts the CTC criterion: it needs objective=\"ctc\", not \"%s\"" % objective)
            if (isinstance(delay_penalty, bool) or not isinstance(delay_penalty, (int, float, np.integer, np.floating))
                    or not np.isfinite(delay_penalty) or delay_penalty < 0):
                raise ValueError("delay_penalty must be a finite float >= 0 or None, got %r" % (delay_penalty,))
            delay_penalty = float(delay_penalty)
        self.delay_penalty = delay_penalty
        self.entry_sum_total, self.entry_labels_total = 0.0, 0
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
            if objective != "ctc":
                raise ValueError("consistency_weight pairs two views under the CTC criterion: it needs objective=\"ctc\", "
                                 "not \"%s\"" % objective)
            if (isinstance(consistency_weight, bool)
                    or not isinstance(consistency_weight, (int, float, np.integer, np.floating))
                    or not np.isfinite(consistency_weight) or not consistency_weight > 0):
                raise ValueError("consistency_weight must be a finite float > 0 or None, got %r" % (consistency_weight,))
            if teacher_weight is not None:
                raise ValueError("consistency_weight does not combine with teacher_weight (a doubled teacher tensor is not built)")
            if spec_augment is None and config_keep(nnet_config) >= 1.0:
                raise ValueError("consistency_weight needs two views that differ: spec_augment or dropout (the model has "
                                 "neither, the term would be 0)")
            consistency_weight = float(consistency_weight)
        self.consistency_weight = consistency_weight
        self.cr_loss_total, self.cr_frames_total, self.cr_agree_total = 0.0, 0, 0
        self.specaug_frames_masked = self.specaug_frames = self.specaug_bins_masked = self.specaug_bins = 0
        self.pipeline = pipeline
        self.model = Model(nnet_config, device, seed=seed)
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
        self.persist_fallbacks = 0     # steps re-run on the launch train after a persistent launch failed
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
        if self.consistency_weight is not None:
            self.keys.append("eval_size")                # what ``eval`` is to be divided by: ``size`` counts both views

    # the reference's graph is a dict; give the same key access
    def __contains__(self, key):
        return key in self.keys

    def __getitem__(self, key):
        if key not in self.keys:
            raise KeyError(key)
        return key

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

    def stage(self, batch):
        """Uploads ``batch`` on a side stream NOW, to be consumed by a later ``step(None, staged=...)``: called for batch
        k + 1 before step k is enqueued, the copy runs under step k's kernels instead of in front of step k + 1's.  Pure
        copies: nothing here can raise for batch k + 1's CONTENT or touch the process group (see _validate_labels)."""
        dev = self.model.device
        if getattr(self, "_h2d_stream", None) is None:
            self._h2d_stream = torch.cuda.Stream(dev)
        with torch.cuda.stream(self._h2d_stream):
            up = self._upload(batch)
            if self.objective == "xent":
                up = up + self._upload_frame_target(batch)
            elif self.align_window is not None:
                up = up + self._upload_windows(batch, up[5], up[6], up[2])
            if self.needs_teacher:
                up = up + self._upload_teacher(batch)
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
            for t in up:
                if torch.is_tensor(t):
                    t.record_stream(cur)          # allocated on the copy stream, consumed on this one
        else:
            up = self._upload(batch)
            if self.objective == "xent":
                up = up + self._upload_frame_target(batch)
            elif self.align_window is not None:
                up = up + self._upload_windows(batch, up[5], up[6], up[2])
            if self.needs_teacher:
                up = up + self._upload_teacher(batch)
        teacher = None
        if self.needs_teacher:
            up, teacher = up[:-2], up[-2:]
            if teacher[0] is None:
                raise ValueError("teacher_weight / objective = kd needs teacher_scores and teacher_length in the batch "
                                 "(create_pipeline_sequence_batch(..., teacher_scores=...))")
        x, seq_d, seq, flat_d, offs_d, flat, offs, maxlen = up[:8]
        ft_d = windows = None
        if self.objective == "xent":                  # reads no nnet_target: has_label = 0 corpora are fine
            ft_d, ft = up[8:]
            self._validate_frame_targets(ft, seq)
        elif self.objective == "kd":                  # neither
            pass
        else:
            self._validate_labels(flat)
            if self.align_window is not None:
                lo_d, hi_d, constrained = up[8:]
                if lo_d is None:
                    raise ValueError("align_window needs frame_target in the batch "
                                     "(create_pipeline_sequence_batch(..., frame_targets=...))")
                windows = (lo_d, hi_d)
                self.windows_constrained += int(constrained.sum())
                self.windows_unconstrained += int(len(constrained) - constrained.sum())
        out = self.step_device(x, seq_d, flat_d, offs_d, maxlen, int(len(flat)), fetch_eval=fetch_eval,
                               fetch_logits=fetch_logits, train=train, flat_host=flat, offs_host=offs, seq_host=seq,
                               frame_target=ft_d, windows=windows, teacher=teacher)
        out["sequence_length"] = np.concatenate([seq, seq]) if "cr_loss" in out else seq      # what the device processed
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
        counters = (self.global_step, self.drop_seed, self.opt_step)
        if self.align_window is not None and windows is None:
            raise ValueError("align_window needs the label windows (step: frame_target in the batch, frame_targets= of the "
                             "pipeline; step_device: windows=)")
        if self.needs_teacher and (teacher is None or teacher[0] is None):
            raise ValueError("teacher_weight / objective = kd needs the teacher scores (step: teacher_scores in the batch, "
                             "teacher_scores= of the pipeline; step_device: teacher=)")
        args = (x, seq_d, flat_d, offs_d, maxlen, size, fetch_eval, fetch_logits, train, flat_host, offs_host, seq_host,
                frame_target, windows, teacher)
        if self._fallback.latched:                     # co-residency is structurally unavailable: stay on the train
            with ops.force_launch_train():
                out, status = self._step_once(*args)
            if status != 0:
                raise RuntimeError("LSTM recurrence failed on the launch train (status %d)" % status)
            return out
        out, status = self._step_once(*args)
        if status == 0:
            self._fallback.good()
            return out
        self.global_step, self.drop_seed, self.opt_step = counters
        self.persist_fallbacks += 1
        self._fallback.failed(status, self.persist_fallbacks)
        with ops.force_launch_train():
            out, status = self._step_once(*args)
        if status != 0:
            raise RuntimeError("LSTM recurrence failed on the launch train as well (status %d)" % status)
        return out

    def _step_once(self, x, seq_d, flat_d, offs_d, maxlen, size, fetch_eval, fetch_logits, train, flat_host, offs_host,
                   seq_host=None, frame_target=None, windows=None, teacher=None):
        dev = self.model.device
        ops.lstm_status(dev).zero_()
        self.global_step += 1
        self.drop_seed = (self.drop_seed * 1664525 + 1013904223) & 0x7FFFFFFF
        pairs = None
        if train and self.consistency_weight is not None:    # every utterance twice; out of place: the caller keeps its x
            pairs = seq_d
            x = torch.cat([x, x], dim=1)
            lo_d, hi_d = windows if windows is not None else (None, None)
            seq_d, flat_d, offs_d, lo_d, hi_d = double_batch(seq_d, flat_d, offs_d, lo_d, hi_d)
            windows = (lo_d, hi_d) if windows is not None else None
            if seq_host is not None:
                seq_host = np.concatenate([seq_host, seq_host])
            if offs_host is not None:
                _, flat_host, offs_host, _, _ = double_batch(None, flat_host, np.asarray(offs_host))
            size = 2 * size
        specaug_counts = None
        if train and self.spec_augment is not None:          # out of place: the caller keeps its x
            x = ops.spec_augment(x, seq_d, self.spec_augment, self.spec_layout, self.drop_seed)
            if seq_host is not None:
                from . import augment
                sub = self.spec_layout.subsample
                specaug_counts = augment.masked_shares(augment.mask_plan(self.drop_seed, seq_host, self.spec_augment, sub),
                                                       seq_host, self.spec_augment, sub)
        logits = self.model.forward(x, seq_d, drop_seed=self.drop_seed, seq_len_host=seq_host)      # [T,B,V]
        out, status = self._finish_step(logits, seq_d, flat_d, offs_d, maxlen, size, fetch_eval, fetch_logits, train, flat_host,
                                        offs_host, frame_target, windows, teacher, pairs)
        if status == 0 and train and self.spec_augment is not None:          # a failed step is re-run: count it once
            self.specaug_steps += 1
            if specaug_counts is not None:
                self.specaug_frames_masked += specaug_counts[0]
                self.specaug_frames += specaug_counts[1]
                self.specaug_bins_masked += specaug_counts[2]
                self.specaug_bins += specaug_counts[3]
        return out, status

    def _finish_step(self, logits, seq_d, flat_d, offs_d, maxlen, size, fetch_eval, fetch_logits, train, flat_host, offs_host,
                     frame_target, windows, teacher, pairs=None):
        """What follows the forward in ``_step_once``: criterion, backward, optimizer, the step's one sync.  ``pairs``: the [B]
        lengths of a batch that ``_step_once`` doubled for consistency_weight (everything else is then the 2B batch)."""
        dev = self.model.device
        if self.objective == "xent":
            return self._finish_xent(logits, seq_d, frame_target, fetch_eval, fetch_logits, train, teacher)
        if self.objective == "kd":
            return self._finish_kd(logits, seq_d, teacher, fetch_eval, fetch_logits, train)
        entry_b = None
        if self.delay_penalty is not None:
            lo_d, hi_d = windows if self.align_window is not None else (None, None)
            loss_b, entry_b, grad = ops.ctc_loss_delay(logits, flat_d, offs_d, seq_d, maxlen, self.delay_penalty, win_lo=lo_d,
                                                       win_hi=hi_d, want_grad=train)
        elif self.align_window is not None:
            loss_b, grad = ops.ctc_loss_windowed(logits, flat_d, offs_d, seq_d, maxlen, windows[0], windows[1],
                                                 want_grad=train)
        else:
            loss_b, grad = ops.ctc_loss(logits, flat_d, offs_d, seq_d, maxlen, want_grad=train)
        out = {"size": size}
        tokens = out_len = None
        reg = None
        if self.sm_weight > 0:                                                   # graph.py:120-133: loss += reg
            T_, B_, V_ = logits.shape
            reg = ops.label_smoothing(logits.view(T_ * B_, V_), self.sm_weight, self.sm_logq,
                                      grad.view(T_ * B_, V_) if train else None)
        kd = self._teacher_term(logits, seq_d, teacher, grad, train)
        if pairs is not None:                              # teacher_weight is excluded: the two share kd's place in the word
            kd = ops.consistency_loss(logits, pairs, grad_scale=0.5 * self.consistency_weight, grad=grad)[:3]
        if fetch_eval:
            tokens, out_len = ops.ctc_greedy(logits, seq_d)
        bn_saved = None
        if train:
            bn_saved = dict(self.model.saved.get("bn") or {})
            self._buckets = (dp.GradientBuckets(self.model.ps.grad, self.pg)
                             if self.pg is not None and self.dp_buckets and (self.world > 1 or self._force_buckets) else None)
            self.model.backward(grad, buckets=self._buckets)
            self._apply_gradients()
        # one device->host sync per step, like the reference's sess.run
        if kd is None and entry_b is None:
            eval_loss = float(loss_b.sum().item())                               # graph.py:116 reduce_sum
        else:                                             # the same float32 sum, with the options' scalars in its copy
            word = torch.cat([loss_b.sum().to(torch.float64).view(1)] + (self._kd_scalars(kd) if kd is not None else []) +
                             (self._entry_scalars(loss_b, entry_b, offs_d, seq_d) if entry_b is not None else [])
                             ).cpu().numpy()
            eval_loss = float(word[0])
        status = int(ops.lstm_status(dev).item())
        if status != 0:
            return None, status
        if train and bn_saved:
            self.model.update_moving_averages(bn_saved)   # batch-norm UPDATE_OPS (graph.py:194-196); only with use_bn
        out["eval_loss"] = eval_loss
        out["loss"] = eval_loss + (float(reg.item()) if reg is not None else 0.0)
        if pairs is not None:
            out["cr_loss"], out["cr_frames"], out["cr_agree"] = float(word[1]), int(word[2]), int(word[3])
            self.cr_loss_total += out["cr_loss"]
            self.cr_frames_total += out["cr_frames"]
            self.cr_agree_total += out["cr_agree"]
            out["loss"] += self.consistency_weight * 0.5 * out["cr_loss"]
        elif kd is not None:
            out["loss"] += self._kd_outputs(out, word[1:4])
        if entry_b is not None:
            out["entry_sum"], out["entry_labels"] = float(word[-2]), int(word[-1])
            self.entry_sum_total += out["entry_sum"]
            self.entry_labels_total += out["entry_labels"]
        if fetch_eval:
            tok, n = tokens.cpu().numpy(), out_len.cpu().numpy()
            if flat_host is None:
                flat_host, offs_host = flat_d.cpu().numpy(), offs_d.cpu().numpy()
            if pairs is not None:                          # view a against the original labels: the first halves
                B_ = pairs.numel()
                tok, n, offs_host = tok[:B_], n[:B_], offs_host[:B_ + 1]
                flat_host = flat_host[:offs_host[-1]]
                out["eval_size"] = size // 2               # the labels ``eval`` was counted against
            out["eval"] = float(ops.edit_distance_host(tok, n, flat_host, offs_host).sum())   # graph.py:143-150
            out["decoded"] = (tok, n)
        if fetch_logits:
            out["logits"] = logits.permute(1, 0, 2).cpu().numpy()                # reference layout [B,T,V]
        if train:
            out["grad_norm"] = float(self.norm_out[0].item())
        return out, 0

    def _teacher_term(self, logits, seq_d, teacher, grad, train):
        """teacher_weight on a base criterion: ``ops.kd_loss`` adding lambda * tau * (q - p) to the criterion's gradient
        (loss only when not training).  None without the option."""
        if self.teacher_weight is None:
            return None
        tau = self.teacher_temperature
        return ops.kd_loss(logits, teacher[0], seq_d, teacher[1], temperature=tau, grad_scale=self.teacher_weight * tau,
                           grad=grad if train else None, want_grad=False)[:3]

    @staticmethod
    def _entry_scalars(loss_b, entry_b, offs_d, seq_d):
        """delay_penalty: [sum of entry_sum, number of labels] over the utterances with a finite, non-skipped loss."""
        n = (offs_d[1:] - offs_d[:-1]).to(torch.int64)
        ok = torch.isfinite(loss_b) & (seq_d > 0) & (n <= seq_d)
        zero = torch.zeros((), dtype=torch.float64, device=loss_b.device)
        return [torch.where(ok, entry_b.to(torch.float64), zero).sum().view(1),
                torch.where(ok, n, torch.zeros_like(n)).sum().to(torch.float64).view(1)]

    @staticmethod
    def _kd_scalars(kd):
        return [t.to(torch.float64).sum().view(1) for t in kd]

    def _kd_outputs(self, out, word):
        """Writes kd_loss / kd_frames / kd_agree into ``out`` and returns what the term adds to ``loss``."""
        tau = self.teacher_temperature
        out["kd_loss"], out["kd_frames"], out["kd_agree"] = float(word[0]), int(word[1]), int(word[2])
        self.kd_frames_total += out["kd_frames"]
        self.kd_agree_total += out["kd_agree"]
        return (1.0 if self.teacher_weight is None else self.teacher_weight) * tau * tau * out["kd_loss"]

    def _finish_kd(self, logits, seq_d, teacher, fetch_eval, fetch_logits, train):
        """The rest of a step under objective = kd: ``ops.kd_loss`` in the place of ``ops.ctc_loss`` (lambda = 1);
        regulariser, backward, L2, clip, optimizer and status word as in the CTC step.  A batch without a scored frame (size
        0) still runs the optimizer step - on a zero loss gradient - so that ranks stay in lockstep."""
        dev = self.model.device
        tau = self.teacher_temperature
        loss_b, frames, agree, grad = ops.kd_loss(logits, teacher[0], seq_d, teacher[1], temperature=tau, grad_scale=tau,
                                                  want_grad=train)
        reg = None
        if self.sm_weight > 0:
            T_, B_, V_ = logits.shape
            reg = ops.label_smoothing(logits.view(T_ * B_, V_), self.sm_weight, self.sm_logq,
                                      grad.view(T_ * B_, V_) if train else None)
        bn_saved = None
        if train:
            bn_saved = dict(self.model.saved.get("bn") or {})
            self._buckets = (dp.GradientBuckets(self.model.ps.grad, self.pg)
                             if self.pg is not None and self.dp_buckets and (self.world > 1 or self._force_buckets) else None)
            self.model.backward(grad, buckets=self._buckets)
            self._apply_gradients()
        # everything the host wants, in ONE device->host copy: the step's single sync
        zero = torch.zeros(1, dtype=torch.float64, device=dev)
        word = torch.cat(self._kd_scalars((loss_b, frames, agree, ops.lstm_status(dev))) +
                         [reg.to(torch.float64).view(1) if reg is not None else zero,
                          self.norm_out[:1].to(torch.float64) if train else zero]).cpu().numpy()
        status = int(word[3])
        if status != 0:
            return None, status
        if train and bn_saved:
            self.model.update_moving_averages(bn_saved)
        out = {}
        out["eval_loss"] = self._kd_outputs(out, word[:3])
        out["size"] = out["kd_frames"]
        out["loss"] = out["eval_loss"] + float(word[4])
        if fetch_eval:
            out["eval"] = float(out["kd_frames"] - out["kd_agree"])      # frames whose two argmaxes disagree
        if fetch_logits:
            out["logits"] = logits.permute(1, 0, 2).cpu().numpy()
        if train:
            out["grad_norm"] = float(word[5])
        return out, 0

    def _finish_xent(self, logits, seq_d, frame_target, fetch_eval, fetch_logits, train, teacher=None):
        """The rest of a step under objective = xent: ``ops.xent_loss`` in the place of ``ops.ctc_loss``; regulariser,
        backward, L2, clip, optimizer and status word as in the CTC step.  A batch without a scored frame (size 0) still
        runs the optimizer step - on a zero loss gradient - so that ranks stay in lockstep."""
        if frame_target is None:
            raise ValueError("objective = xent needs frame_target (create_pipeline_sequence_batch(..., frame_targets=...))")
        dev = self.model.device
        loss_b, frames, correct, grad = ops.xent_loss(logits, frame_target, seq_d, want_grad=train)
        reg = None
        if self.sm_weight > 0:
            T_, B_, V_ = logits.shape
            reg = ops.label_smoothing(logits.view(T_ * B_, V_), self.sm_weight, self.sm_logq,
                                      grad.view(T_ * B_, V_) if train else None)
        kd = self._teacher_term(logits, seq_d, teacher, grad, train)
        bn_saved = None
        if train:
            bn_saved = dict(self.model.saved.get("bn") or {})
            self._buckets = (dp.GradientBuckets(self.model.ps.grad, self.pg)
                             if self.pg is not None and self.dp_buckets and (self.world > 1 or self._force_buckets) else None)
            self.model.backward(grad, buckets=self._buckets)
            self._apply_gradients()
        # everything the host wants, in ONE device->host copy: the step's single sync
        f64 = lambda t: t.to(torch.float64).sum().view(1)
        zero = torch.zeros(1, dtype=torch.float64, device=dev)
        word = torch.cat([f64(loss_b), f64(frames), f64(correct), f64(ops.lstm_status(dev)),
                          reg.to(torch.float64).view(1) if reg is not None else zero,
                          self.norm_out[:1].to(torch.float64) if train else zero] +
                         (self._kd_scalars(kd) if kd is not None else [])).cpu().numpy()
        status = int(word[3])
        if status != 0:
            return None, status
        if train and bn_saved:
            self.model.update_moving_averages(bn_saved)
        n_frames = int(word[1])
        out = {"size": n_frames, "eval_loss": float(word[0]), "loss": float(word[0]) + float(word[4])}
        if kd is not None:
            out["loss"] += self._kd_outputs(out, word[6:9])
        if fetch_eval:
            out["eval"] = float(n_frames - int(word[2]))          # frames the argmax gets wrong
        if fetch_logits:
            out["logits"] = logits.permute(1, 0, 2).cpu().numpy()
        if train:
            out["grad_norm"] = float(word[5])
        return out, 0

    # ------------------------------------------------------------------------------------------------- forced alignment
    def align(self, batch):
        """Best-path (Viterbi) CTC alignment of one batch in the pipeline contract - no reference counterpart.  One forward
        in inference mode (no dropout, batch-norm on its moving averages), then ``ops.ctc_align`` on the logits.  Returns
        host arrays: ``ali`` [B,T] int32 (symbol per frame, blank = V-1; -1 beyond an utterance's length and when its labels
        do not fit its frames), ``label_index`` [B,T] int32, ``score`` [B] float32 (-inf without a path) and
        ``sequence_length``.  Never trains: parameters, ``global_step`` and the dropout stream are left as they were."""
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
                return res, int(ops.lstm_status(dev).item())

            if self._fallback.latched:
                with ops.force_launch_train():
                    res, status = run()
            else:
                res, status = run()
                if status == 0:
                    self._fallback.good()
                else:                                      # a persistent launch could not complete: launch train
                    self.persist_fallbacks += 1
                    self._fallback.failed(status, self.persist_fallbacks)
                    with ops.force_launch_train():
                        res, status = run()
            if status != 0:
                raise RuntimeError("LSTM recurrence failed on the launch train as well (status %d)" % status)
        finally:
            model.is_training, model.keep = mode
        ali, lidx, score = res
        return {"ali": ali.cpu().numpy(), "label_index": lidx.cpu().numpy(), "score": score.cpu().numpy(),
                "sequence_length": seq}

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
        self.persist_fallbacks = 0
        self._fallback = _FallbackLatch()
        self.keys = ["filename", "nnet_input", "sequence_length", "logits", "nnet_output"]

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

        if self._fallback.latched:
            with ops.force_launch_train():
                logits, status = run()
        else:
            logits, status = run()
            if status == 0:
                self._fallback.good()
            else:                                          # a persistent launch could not complete: launch train
                self.persist_fallbacks += 1
                self._fallback.failed(status, self.persist_fallbacks)
                with ops.force_launch_train():
                    logits, status = run()
        if status != 0:
            raise RuntimeError("LSTM recurrence failed on the launch train as well")
        return logits, seq

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
def create_graph_for_validation_ctc(pipeline, nnet_config, device="cuda", seed=None, align_window=None,
                                    teacher_weight=None, teacher_temperature=1.0, delay_penalty=None):
    return CTCGraph(pipeline, nnet_config, device=device, seed=seed, align_window=align_window,
                    teacher_weight=teacher_weight, teacher_temperature=teacher_temperature, delay_penalty=delay_penalty)


def create_graph_for_training_ctc(pipeline, nnet_config, learn_rate, clip_norm=5.0, optimizer="sgd",
                                  l2_decay_weight=1e-5, device="cuda", seed=None, process_group=None, align_window=None,
                                  teacher_weight=None, teacher_temperature=1.0, delay_penalty=None, spec_augment=None,
                                  consistency_weight=None):
    return CTCGraph(pipeline, nnet_config, learn_rate=learn_rate, clip_norm=clip_norm, optimizer=optimizer,
                    l2_decay_weight=l2_decay_weight, device=device, seed=seed, process_group=process_group,
                    align_window=align_window, teacher_weight=teacher_weight, teacher_temperature=teacher_temperature,
                    delay_penalty=delay_penalty, spec_augment=spec_augment, consistency_weight=consistency_weight)


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
