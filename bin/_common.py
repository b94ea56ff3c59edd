"""Shared plumbing of the bin/nnet-*.py command lines (flag parsing quirks, device / process-group setup)."""
import argparse
import collections
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def str2bool(v):
    """yes/true/t/y/1 and no/false/f/n/0, as every reference CLI does (bin/nnet-train.py:103-109)."""
    if v.lower() in ('yes', 'true', 't', 'y', '1'):
        return True
    if v.lower() in ('no', 'false', 'f', 'n', '0'):
        return False
    raise argparse.ArgumentTypeError('Boolean value expected.')


def setup_device():
    """One process per GPU.  Returns (device, process_group or None, rank, world_size)."""
    import torch
    if not torch.cuda.is_available():
        sys.stderr.write("FATAL:tensorflow:no GPU visible - lstm_ctc_amd has no CPU path\n")
        sys.exit(1)
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # tests only (tests/test_gpu_round6.py): LC_DP_TEST_SHARED_GPU=1 puts every rank on GPU 0 with gloo as the collective
    # backend (RCCL refuses two ranks on one device), so that an 8-rank launch can be rehearsed on a one-GPU box
    shared = world > 1 and os.environ.get("LC_DP_TEST_SHARED_GPU") == "1"
    if shared:
        local = 0
    elif torch.cuda.device_count() <= local:
        sys.stderr.write("FATAL:tensorflow:rank %d needs GPU %d but %d GPU(s) are visible (one process per GPU)\n"
                         % (rank, local, torch.cuda.device_count()))
        sys.exit(1)
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    pg = None
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if shared:
            torch.distributed.init_process_group("gloo")
        else:
            torch.distributed.init_process_group("nccl", device_id=device)      # nccl == RCCL on ROCm
        pg = torch.distributed.group.WORLD
    return device, pg, rank, world


def _fatal(msg):
    sys.stderr.write("FATAL:tensorflow:" + msg + "\n")
    sys.exit(1)


def read_frame_targets(args):
    """--objective xent, or --objective ctc with --align-window: {utterance key: int32 vector} of --frame-targets, or the FATAL
    line and exit 1 when the flag is missing or the table unreadable - which it also is when it names no utterance of
    <tfrecords.scp> - and when --align-window is negative or meets another objective than ctc.  None for every other
    command line.  Host work only: runs BEFORE the device is set up, so a bad command line fails without touching a GPU."""
    window = getattr(args, 'align_window', None)
    if window is not None:
        if args.objective != 'ctc':
            _fatal('--align-window constrains the CTC criterion: it needs --objective ctc, not "%s"' % args.objective)
        if window < 0:
            _fatal('--align-window must be a number of frames >= 0, got %d' % window)
        if not args.frame_targets:
            _fatal('--align-window needs --frame-targets <rspecifier> (the table nnet-align writes)')
    elif args.objective != 'xent':
        return None
    spec = args.frame_targets
    if not spec:
        _fatal('--objective xent needs --frame-targets <rspecifier> (the table nnet-align writes)')
    opts, sep, path = spec.partition(':')
    if not sep:
        opts, path = 'ark', spec
    opts = [o.strip() for o in opts.split(',')]
    if 'ark' not in opts or not path:
        _fatal('--frame-targets: unsupported rspecifier (need ark:FILE, ark,t:FILE or a path): %s' % spec)
    from lstm_ctc_amd.kaldi_io import read_int32_vector_ark
    try:
        table = read_int32_vector_ark(path, text='t' in opts)
    except Exception as exc:                          # missing file, truncated or foreign content
        _fatal('--frame-targets: cannot read "%s": %s: %s' % (path, type(exc).__name__, exc))
    try:
        keys = [os.path.splitext(os.path.basename(line.split()[4]))[0] for line in open(args.tfrecords_scp) if line.split()]
    except (OSError, IndexError) as exc:
        _fatal('cannot read "%s": %s' % (args.tfrecords_scp, exc))
    if not any(k in table for k in keys):
        _fatal('--frame-targets: "%s" (%d entries) names no utterance of "%s"' % (path, len(table), args.tfrecords_scp))
    return table


def read_teacher_scores(args):
    """--teacher-scores: the lazily read table (kaldi_io.FloatMatrixTable) of the teacher's per-frame scores, or None without
    the flag.  The FATAL line and exit 1 for --objective kd without the flag, a weight or temperature that is not a
    positive finite number, an unsupported rspecifier, an unreadable table and a table that names no utterance of
    <tfrecords.scp>.  Host work only: runs BEFORE the device is set up."""
    spec = getattr(args, 'teacher_scores', None)
    if args.objective == 'kd' and not spec:
        _fatal('--objective kd needs --teacher-scores <rspecifier> (the table nnet-forward --apply-log writes)')
    import math
    for flag, value in (('--teacher-weight', getattr(args, 'teacher_weight', 1.0)),
                        ('--teacher-temperature', getattr(args, 'teacher_temperature', 1.0))):
        if not (math.isfinite(value) and value > 0):
            _fatal('%s must be a finite number > 0, got %r' % (flag, value))
    if not spec:
        return None
    if args.teacher_domain not in ('log', 'prob'):
        _fatal('--teacher-domain must be "log" or "prob", got "%s"' % args.teacher_domain)
    opts, sep, path = spec.partition(':')
    if not sep:
        opts, path = 'ark', spec
    opts = [o.strip() for o in opts.split(',')]
    if 'ark' not in opts or not path:
        _fatal('--teacher-scores: unsupported rspecifier (need ark:FILE, ark,t:FILE or a path): %s' % spec)
    from lstm_ctc_amd.kaldi_io import FloatMatrixTable
    try:
        table = FloatMatrixTable(path, text='t' in opts)
    except Exception as exc:                          # missing file, truncated or foreign content
        _fatal('--teacher-scores: cannot read "%s": %s: %s' % (path, type(exc).__name__, exc))
    try:
        keys = [os.path.splitext(os.path.basename(line.split()[4]))[0] for line in open(args.tfrecords_scp) if line.split()]
    except (OSError, IndexError) as exc:
        _fatal('cannot read "%s": %s' % (args.tfrecords_scp, exc))
    if not any(k in table for k in keys):
        _fatal('--teacher-scores: "%s" (%d entries) names no utterance of "%s"' % (path, len(table), args.tfrecords_scp))
    return table


def teacher_keywords(args, table, nnet_config):
    """(pipeline keywords, graph keywords) of the teacher flags; both empty without --teacher-scores."""
    if table is None:
        return {}, {}
    graph = {'teacher_temperature': args.teacher_temperature}
    if args.objective != 'kd':
        graph['teacher_weight'] = args.teacher_weight
    return ({'teacher_scores': table, 'teacher_domain': args.teacher_domain, 'num_targets': nnet_config.get('num_targets')},
            graph)


def report_teacher_scores(pipeline, graph):
    """One INFO line at the end of a pass with --teacher-scores: the utterances the table did not cover and how the student
    compares on the frames it did."""
    from lstm_ctc_amd.nnet import tflog
    n, a = graph.kd_frames_total, graph.kd_agree_total
    tflog.info('teacher scores: %d utterance(s) without an entry, %d with an entry of another shape than [frames, targets], '
               '%d with a row that is no distribution (none is scored); %d frame(s) scored, the argmaxes agree on %.2f%%'
               % (pipeline.teacher_missing, pipeline.teacher_mismatched, pipeline.teacher_bad, n, 100.0 * a / max(n, 1)))


def report_frame_targets(pipeline):
    """One INFO line at the end of a pass under --objective xent: the utterances that trained on nothing."""
    from lstm_ctc_amd.nnet import tflog
    tflog.info('frame targets: %d utterance(s) without an entry, %d with an entry of another length than their frames '
               '(neither is scored)' % (pipeline.targets_missing, pipeline.targets_mismatched))


def report_label_windows(graph):
    """One INFO line at the end of a pass under --align-window: how many utterances the windows reached."""
    from lstm_ctc_amd.nnet import tflog
    tflog.info('label windows (+-%d frames): %d utterance(s) constrained, %d unconstrained (no entry, another length, or an '
               'alignment that does not spell the labels)'
               % (graph.align_window, graph.windows_constrained, graph.windows_unconstrained))


def _finite_nonnegative(value):
    import math
    if not (math.isfinite(value) and value >= 0):
        raise ValueError
    return value


def parse_star_penalty(text):
    """'B[,S]' -> (bypass_penalty, selfloop_penalty); one value sets both, 'inf' is accepted.  ValueError for anything else,
    for NaN and for a negative value."""
    parts = [p.strip() for p in text.split(',')]
    if len(parts) not in (1, 2):
        raise ValueError('expected B or B,S')
    values = tuple(float(p) for p in parts)              # '' and words raise here
    if not all(v >= 0 for v in values):                  # NaN fails the comparison
        raise ValueError('a penalty must be >= 0 or inf')
    return values * 2 if len(values) == 1 else values


# The exclusive forms of the CTC criterion, by flag and in the order they are checked (nnet.graph.CRITERION_OPTIONS has the same
# rows for the graph): parse (the flag's value -> the graph keyword's, or ValueError), "<flag> must be <must_be>", "<flag> <verb>
# the CTC criterion", the earlier flags it refuses and the excuse in parentheses, the INFO line at the end of a pass, and the two
# graph attributes that line reads after the graph's value(s): their quotient, then the second.
_Flag = collections.namedtuple('_Flag', 'parse must_be verb refuses excuse line totals')
CRITERION_FLAGS = {
    '--delay-penalty': _Flag(_finite_nonnegative, 'a finite number >= 0', 'tilts', (), None,
                             'delay penalty %g: mean label entry frame %.3f over %d label(s)',
                             ('entry_sum_total', 'entry_labels_total')),
    '--entropy-weight': _Flag(_finite_nonnegative, 'a finite number >= 0', 'regularises', ('--delay-penalty',),
                              'the entropy of the tilted path posterior is not built',
                              'entropy weight %g: mean path entropy %.6f nats per frame over %d frame(s)',
                              ('path_entropy_total', 'path_entropy_frames_total')),
    '--star-penalty': _Flag(parse_star_penalty, 'B[,S] with penalties >= 0 or inf', 'relaxes', ('--delay-penalty', '--entropy-weight'),
                            'the star under that term is not built',
                            'star penalty bypass %g selfloop %g: %.6f of %d frame(s) explained by the star',
                            ('star_frames_total', 'star_frame_count_total')),
}
_attribute = lambda flag: flag.lstrip('-').replace('-', '_')


def _parsed(flag, value):
    try:
        return CRITERION_FLAGS[flag].parse(value)
    except ValueError as e:
        _fatal('%s must be %s, got %r%s' % (flag, CRITERION_FLAGS[flag].must_be, value, ' (%s)' % e if str(e) else ''))


def criterion_keywords(args, flags=tuple(CRITERION_FLAGS)):
    """--delay-penalty, --entropy-weight, --star-penalty: the graph keywords of those given, empty without (nnet-init has
    none).  Per flag, in the table's order, the FATAL line and exit 1 when parse refuses the value, when it meets another
    objective than ctc, and when it comes with a flag it refuses.  Host work only: runs BEFORE the device is set up."""
    keywords = {}
    for flag in flags:
        row, value = CRITERION_FLAGS[flag], getattr(args, _attribute(flag), None)
        if value is None:
            continue
        keywords[_attribute(flag)] = _parsed(flag, value)
        if args.objective != 'ctc':
            _fatal('%s %s the CTC criterion: it needs --objective ctc, not "%s"' % (flag, row.verb, args.objective))
        for other in row.refuses:
            if getattr(args, _attribute(other), None) is not None:
                _fatal('%s does not combine with %s (%s)' % (flag, other, row.excuse))
    return keywords


def report_criterion(graph, flags=tuple(CRITERION_FLAGS)):
    """One INFO line at the end of a pass under the flag of CRITERION_FLAGS that is set: what the criterion's own path
    posterior says - the mean frame at which a label is entered, the path entropy in nats per utterance-frame, the share of
    the frames the star explains."""
    from lstm_ctc_amd.nnet import tflog
    for flag in flags:
        row, value = CRITERION_FLAGS[flag], getattr(graph, _attribute(flag), None)
        if value is not None:
            total, n = (getattr(graph, name) for name in row.totals)
            tflog.info(row.line % ((value if isinstance(value, tuple) else (value,)) + (total / max(n, 1), n)))


# the table's rows one at a time, under their earlier names
delay_keywords = lambda args: criterion_keywords(args, ('--delay-penalty',))
entropy_keywords = lambda args: criterion_keywords(args, ('--entropy-weight',))
star_keywords = lambda args: criterion_keywords(args, ('--star-penalty',))
report_delay_penalty = lambda graph: report_criterion(graph, ('--delay-penalty',))
report_entropy_weight = lambda graph: report_criterion(graph, ('--entropy-weight',))
report_star_penalty = lambda graph: report_criterion(graph, ('--star-penalty',))


def star_report_keywords(args):
    """nnet-align's --star-penalty / --star-report: the keyword of ``CTCGraph.align``, empty without the flags.  The FATAL line
    and exit 1 for either flag without the other and for a bad penalty, before the device is touched."""
    text, report = getattr(args, 'star_penalty', None), getattr(args, 'star_report', None)
    if text is None and report is None:
        return {}
    if text is None or report is None:
        _fatal('--star-penalty and --star-report go together: the report is what the penalty is for')
    return {'star_penalty': _parsed('--star-penalty', text)}


def star_report_line(key, frames, labels, ctc_loss, star_loss, star_frames):
    """One line of nnet-align's --star-report: key frames labels ctc_loss star_loss star_frames."""
    return '%s %d %d %.6f %.6f %.6f\n' % (key, frames, labels, ctc_loss, star_loss, star_frames)


def spec_augment_keywords(args):
    """--spec-augment: the graph keyword, empty without the flag.  The FATAL line and exit 1 for a value that
    nnet.augment.parse_spec refuses, and for bins that do not divide the input_dim of a readable <nnet-config>.  Host work
    only: runs BEFORE the device is set up."""
    text = getattr(args, 'spec_augment', None)
    if text is None:
        return {}
    from lstm_ctc_amd.nnet import augment
    try:
        spec = augment.parse_spec(text)
    except ValueError as exc:                         # "spec-augment: ..." or "SpecAugment: ..."
        _fatal('--%s' % exc if str(exc).startswith('spec-augment') else '--spec-augment: %s' % exc)
    try:
        from lstm_ctc_amd.nnet.config import parse_config
        input_dim = parse_config(args.nnet_config).get('input_dim')
    except (OSError, AttributeError):                 # an unreadable config is reported where it is read for the model
        input_dim = None
    if isinstance(input_dim, int):
        try:
            spec.check_layout(input_dim)
        except ValueError as exc:
            _fatal('--spec-augment: %s' % exc)
    return {'spec_augment': spec}


def report_spec_augment(graph):
    """One INFO line at the end of a pass under --spec-augment: the settings, the steps augmented and how much of the input the
    masks covered (nnet.augment.mask_plan on the sequence lengths the steps had on the host)."""
    from lstm_ctc_amd.nnet import tflog
    tflog.info('spec augment %s: %d step(s) augmented; %.2f%% of %d live raw frame(s) under a time mask, %.2f%% of the bins '
               'under a frequency mask'
               % (graph.spec_augment, graph.specaug_steps, 100.0 * graph.specaug_frames_masked / max(graph.specaug_frames, 1),
                  graph.specaug_frames, 100.0 * graph.specaug_bins_masked / max(graph.specaug_bins, 1)))


def consistency_keywords(args, augmented):
    """--consistency-weight: the graph keyword, empty without the flag.  ``augmented``: what spec_augment_keywords returned.
    The FATAL line and exit 1 for a value that is not finite and > 0, another objective than ctc, --teacher-scores, and two
    views that cannot differ (no --spec-augment while a readable <nnet-config> has no dropout).  Host work only: runs BEFORE
    the device is set up."""
    weight = getattr(args, 'consistency_weight', None)
    if weight is None:
        return {}
    import math
    if not (math.isfinite(weight) and weight > 0):
        _fatal('--consistency-weight must be a finite number > 0, got %r' % weight)
    if args.objective != 'ctc':
        _fatal('--consistency-weight pairs two views under the CTC criterion: it needs --objective ctc, not "%s"' % args.objective)
    if getattr(args, 'teacher_scores', None):
        _fatal('--consistency-weight does not combine with --teacher-scores')
    if not augmented:
        try:
            from lstm_ctc_amd.nnet.config import parse_config
            from lstm_ctc_amd.nnet.graph import config_keep
            keep = config_keep(dict(parse_config(args.nnet_config), is_training=True))
        except (OSError, AttributeError):             # an unreadable config is reported where it is read for the model
            keep = None
        except (TypeError, ValueError) as exc:        # a dropout_rate that is no number
            _fatal('--consistency-weight: cannot read dropout_rate of "%s": %s' % (args.nnet_config, exc))
        if keep is not None and keep >= 1.0:
            _fatal('--consistency-weight needs two views that differ: pass --spec-augment, or train a model with dropout '
                   '("%s" has none)' % args.nnet_config)
    return {'consistency_weight': weight}


def report_consistency(graph):
    """One INFO line at the end of a pass under --consistency-weight: how far apart the two views' posteriors were."""
    from lstm_ctc_amd.nnet import tflog
    n = graph.cr_frames_total
    tflog.info('consistency weight %g: mean symmetric KL %.6f per frame over %d frame(s) of a pair, the argmaxes agree on %.2f%%'
               % (graph.consistency_weight, graph.cr_loss_total / max(n, 1), n, 100.0 * graph.cr_agree_total / max(n, 1)))


def report_chunking(nnet_config):
    """One INFO line when <nnet-config> sets chunk_frames (the latency-controlled BiLSTM): Nc, Nr, the layers
    and how far past a chunk's end its logits read, in model frames and in raw frames (x subsample, + right_context).  A
    config that sets the keys for a model that cannot run them: the FATAL line and exit 1, before a model is built."""
    from lstm_ctc_amd.nnet.model import chunk_info_line
    try:
        line = chunk_info_line(nnet_config)
    except ValueError as exc:
        _fatal(str(exc))
    if line:
        from lstm_ctc_amd.nnet import tflog
        tflog.info(line)


def report_row_conv(nnet_config):
    """One INFO line when <nnet-config> sets row_conv_frames (the uni-LSTM's row convolution): tau and how far
    past their own frame the logits read, in model frames and in raw frames (x subsample, + right_context).  A config the
    model refuses: the FATAL line and exit 1, before a model is built."""
    from lstm_ctc_amd.nnet.model import row_conv_info_line
    try:
        line = row_conv_info_line(nnet_config)
    except ValueError as exc:
        _fatal(str(exc))
    if line:
        from lstm_ctc_amd.nnet import tflog
        tflog.info(line)


def report_layer_norm(nnet_config):
    """One INFO line when <nnet-config> sets layer_norm (layer normalisation of every layer's output): which
    layers are normalised, and eps.  A config the model refuses: the FATAL line and exit 1, before a model is built."""
    from lstm_ctc_amd.nnet.model import layer_norm_info_line
    try:
        line = layer_norm_info_line(nnet_config)
    except ValueError as exc:
        _fatal(str(exc))
    if line:
        from lstm_ctc_amd.nnet import tflog
        tflog.info(line)


def report_conv(nnet_config):
    """One INFO line when <nnet-config> sets conv_layers (the convolutional front-end): layers, channels, bins
    per layer, the width layer 0 reads and the parameters added.  A config the model refuses (a spliced input, use_bn,
    pack_frames, a compute_dtype other than fp32, bad values): the FATAL line and exit 1, before a model is built."""
    from lstm_ctc_amd.nnet.model import conv_info_line
    try:
        line = conv_info_line(nnet_config)
    except ValueError as exc:
        _fatal(str(exc))
    if line:
        from lstm_ctc_amd.nnet import tflog
        tflog.info(line)


def report_time_reduce(nnet_config, args=None, aligning=False):
    """One INFO line when <nnet-config> sets time_reduce_layers (the pyramidal BiLSTM): the layers, r, R and how
    many model and raw frames one frame of the logits stands for.  A config the model refuses, or (``args``) a command line
    that brings a table at the input's frame rate - --frame-targets / --align-window, --teacher-scores, --objective xent|kd -:
    the FATAL line and exit 1, before a model is built."""
    from lstm_ctc_amd.nnet.model import time_reduce_info_line
    try:
        line = time_reduce_info_line(nnet_config)
    except ValueError as exc:
        _fatal(str(exc))
    if not line:
        return
    tabled = [flag for flag, on in (('--frame-targets', getattr(args, 'frame_targets', None)),
                                    ('--align-window', getattr(args, 'align_window', None) is not None),
                                    ('--teacher-scores', getattr(args, 'teacher_scores', None)),
                                    ('--objective %s' % getattr(args, 'objective', 'ctc'),
                                     getattr(args, 'objective', 'ctc') not in (None, 'ctc'))) if on]
    if aligning:
        _fatal('time_reduce_layers does not combine with alignment: an alignment names a symbol per input frame, the logits '
               'come once per several of them')
    if tabled:
        _fatal('time_reduce_layers does not combine with %s: its table is at the input\'s frame rate, the logits are not '
               '(re-timed tables are not built)' % ', '.join(tabled))
    from lstm_ctc_amd.nnet import tflog
    tflog.info(line)


def report_time_reduce_short(graph):
    """One INFO line at the end of a pass of a pyramidal model: the utterances whose labels, with a blank between adjacent
    repeats, needed more frames than the logits had left (the criterion skips them or finds no path)."""
    if getattr(graph.model, 'time_factor', 1) > 1:
        from lstm_ctc_amd.nnet import tflog
        tflog.info('time reduction by %d: %d utterance(s) whose labels and adjacent repeats no longer fit their output frames'
                   % (graph.model.time_factor, graph.time_reduce_short))


def quiet_unless_rank0(rank):
    """Only rank 0 emits the machine-parsed log lines (scripts/train.sh greps one tr_loss / cv_loss line)."""
    if rank != 0:
        from lstm_ctc_amd.nnet import tflog
        tflog.info = lambda *a, **k: None


# ---- the command-line contract ---------------------------------------------------------------------------------------
# Flag names, types and defaults are what scripts/train*.sh and scripts/decode_*.sh pass (bin/nnet-train.py:113-151,
# nnet-validate.py:108-129, nnet-init.py:107-128, nnet-forward.py:129-151 of the reference) and must not move; the texts
# describe what the flag does HERE.
POSITIONAL = {
    'tfrecords_scp': ('<tfrecords.scp>', 'list of utterances: "<key> <rows> <cols> <has_label> <file.tfrecords>" per line'),
    'nnet_config': ('<nnet-config>', '"key = value" model description (nnet.parse_config)'),
    'nnet_in': ('<nnet-in>', 'checkpoint to start from (safetensors at exactly this path)'),
    'nnet_out': ('<nnet-out>', 'checkpoint to write (safetensors at exactly this path)'),
    'nnet_output': ('<nnet-output-wspecifier>', 'Kaldi table wspecifier (ark:... / ark,t:... / ark,scp:...) for the outputs'),
    'alignment': ('<alignment-wspecifier>', 'Kaldi int32-vector table wspecifier for the per-frame symbols (new: nnet-align)'),
}
FLAGS = {
    '--objective': dict(type=str, default='xent', help='training criterion: "ctc" (the recipes pass it), or "xent" = frame-level '
                        'softmax cross-entropy against --frame-targets (new); the loss is then per frame and eval the frame error rate; '
                        'or "kd" = distillation from --teacher-scores alone (new): loss per frame, eval the argmax disagreement rate'),
    '--teacher-scores': dict(type=str, default=None, help='Kaldi float-matrix table rspecifier (ark:FILE, ark,t:FILE or a path) with the '
                             'teacher\'s per-frame scores [frames, targets], as nnet-forward --apply-log writes them (new); adds '
                             'weight * T^2 * KL(teacher || student) to --objective ctc / xent, required by --objective kd'),
    '--teacher-domain': dict(type=str, default='log', help='"log": the table holds log-posteriors or logits; "prob": probabilities (new)'),
    '--teacher-weight': dict(type=float, default=1.0, help='weight of the distillation term beside --objective ctc / xent (new)'),
    '--teacher-temperature': dict(type=float, default=1.0, help='temperature T both distributions are softened with (new)'),
    '--frame-targets': dict(type=str, default=None, help='Kaldi int32-vector table rspecifier (ark:FILE, ark,t:FILE or a path) with one '
                            'symbol per frame and utterance, as nnet-align writes it; required by --objective xent (new)'),
    '--align-window': dict(type=int, default=None, help='with --objective ctc and --frame-targets: sum the CTC criterion only over '
                           'paths that keep every label within this many frames of where the alignment table puts it (new); '
                           'utterances the table does not cover train on plain CTC'),
    '--delay-penalty': dict(type=float, default=None, help='with --objective ctc: weight every path by exp(-penalty * sum of the '
                            'frames at which its labels are entered), so that the model learns to emit earlier (new); needs no '
                            'table, composes with --align-window; 0 is plain CTC and reports the mean label entry frame'),
    '--entropy-weight': dict(type=float, default=None, help='with --objective ctc: maximum-entropy CTC (new): subtract weight * '
                             'the entropy of the posterior over the feasible paths from the CTC loss, so that the model does not '
                             'collapse onto a few spiky alignments; needs no table, composes with --align-window, not with '
                             '--delay-penalty; 0 is plain CTC and reports the mean path entropy in nats per frame'),
    '--star-penalty': dict(type=str, default=None, help='B[,S]: transcript-tolerant CTC (new): every lattice position may explain '
                           'a frame by a star, "some non-blank class", instead of its own class - a label position at penalty B (a '
                           'substituted or inserted label), a blank position at penalty S (a deleted label; one value sets both, inf '
                           'switches one off); with --objective ctc in nnet-train / nnet-validate it is the criterion, composes with '
                           '--align-window, not with --delay-penalty / --entropy-weight, and reports the share of frames the star '
                           'explains; in nnet-align it goes with --star-report'),
    '--star-report': dict(type=str, default=None, help='with --star-penalty (new: nnet-align): write text lines "key frames labels '
                          'ctc_loss star_loss star_frames" here, one per utterance with labels that fit its frames - a large '
                          'star_frames marks a suspect transcript'),
    '--spec-augment': dict(type=str, default=None, help='SpecAugment on the device, training steps only (new): '
                           'time=NxW,freq=NxW,bins=F[,cap=P][,fill=V] = N time masks of at most W raw frames (and at most P percent '
                           'of the utterance, default 100), N frequency masks of at most W of the F bins of a feature group '
                           '(statics, deltas, ...; F divides input_dim), masked elements set to V (default 0); e.g. '
                           'time=2x40,freq=2x15,bins=40,cap=20'),
    '--consistency-weight': dict(type=float, default=None, help='with --objective ctc: consistency-regularised CTC (new): every '
                                 'training step runs each utterance twice, under two draws of --spec-augment and dropout, and adds '
                                 'weight * 0.5 * the symmetric KL between the two views\' frame posteriors to the CTC criterion of both '
                                 '(a step then costs a batch of twice --batch-size); needs --spec-augment or a model with dropout'),
    '--optimizer': dict(type=str, default='sgd', help='sgd | momentum (0.9) | adam, constant learning rate'),
    '--evaluate': dict(type=str2bool, default='false', help='also report an error rate: greedy decoding and the token error rate (ctc), the frame error rate (xent)'),
    '--learn-rate': dict(type=float, default=0.0001, help='step size of the optimizer'),
    '--batch-size': dict(type=int, default=256, help='utterances per step (per GPU under torchrun)'),
    '--batch-threads': dict(type=int, default=8, help='batches assembled concurrently by the loader (capped at 4)'),
    '--seed': dict(type=int, default=777, help='seed of the file-list shuffle, the dropout stream and (nnet-train) the graph'),
    '--num-parallel-calls': dict(type=int, default=32, help='loader threads decoding TFRecords (native code, GIL released)'),
    '--report-interval': dict(type=int, default=100, help='log a progress line every this many steps / utterances'),
    '--shuffle': dict(type=str2bool, default='true', help='permute the utterance list (seeded) before batching'),
    '--clip-norm': dict(type=float, default=5.0, help='global-norm bound applied to the summed gradient'),
    '--apply-softmax': dict(type=str2bool, default='true', help='write softmax(smooth * logits) instead of logits'),
    '--apply-log': dict(type=str2bool, default='true', help='write log-posteriors (implies --apply-softmax)'),
    '--class-prior': dict(type=str, default=None, help='label.counts file; its log-prior is subtracted from the log-posteriors'),
    '--smooth-factor': dict(type=float, default=1.0, help='temperature multiplied into the logits before the softmax'),
    '--batch-utts': dict(type=int, default=16, help='utterances per padded GPU batch (new; results do not depend on it)'),
    '--segments': dict(type=str, default=None, help='also write text lines "key label start_frame num_frames" here (new: nnet-align)'),
    '--scores': dict(type=str, default=None, help='also write text lines "key best_path_log_prob" here (new: nnet-align)'),
}


def build_cli(positional, flags):
    parser = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    for name in positional:
        metavar, text = POSITIONAL[name]
        parser.add_argument(name, metavar=metavar, type=str, help=text)
    for flag in flags:
        parser.add_argument(flag, metavar=flag.lstrip('-'), **FLAGS[flag])
    return parser
