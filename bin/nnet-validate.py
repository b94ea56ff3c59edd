#!/usr/bin/env python3
"""CV pass of a saved model: logs ``cv_loss`` / ``cv_eval``.  Mirrors mobvoi/lstm_ctc bin/nnet-validate.py
(main 26-92, flags 108-129)."""
import sys

from _common import (build_cli, setup_device, quiet_unless_rank0, read_frame_targets, report_frame_targets,
                     report_label_windows, read_teacher_scores, teacher_keywords, report_teacher_scores, criterion_keywords,
                     report_criterion, report_chunking, report_row_conv, report_layer_norm, report_conv, report_time_reduce,
                     report_time_reduce_short)


def run(args, init_only):
    try:
        criterion = criterion_keywords(args)              # --delay-penalty / --entropy-weight / --star-penalty; fatal before the device
        frame_targets = read_frame_targets(args)          # xent, or ctc with --align-window; fatal before the device is touched
        teacher = read_teacher_scores(args)               # --teacher-scores / --objective kd; likewise
        device, pg, rank, world = setup_device()
        import lstm_ctc_amd.nnet as nnet
        from lstm_ctc_amd.nnet import tflog
        quiet_unless_rank0(rank)
        nnet_config = nnet.parse_config(args.nnet_config)
        nnet_config['is_training'] = False
        report_chunking(nnet_config)                      # chunk_frames / lookahead_frames: one INFO line
        report_row_conv(nnet_config)                      # row_conv_frames: one INFO line
        report_layer_norm(nnet_config)                    # layer_norm: one INFO line
        report_conv(nnet_config)                          # conv_layers: one INFO line
        report_time_reduce(nnet_config, args)             # time_reduce_layers: one INFO line; fatal with a frame-rate table
        nnet_type = nnet_config.get('nnet_type')
        filename, tfrecord, input_dim = nnet.dataset_from_tfrecords(
            tfrecords_scp=args.tfrecords_scp, left_context=nnet_config.get('left_context'),
            right_context=nnet_config.get('right_context'), subsample=nnet_config.get('subsample'), shuffle=False)
        if args.objective not in ('ctc', 'xent', 'kd'):
            tflog.fatal('unsupported objective: %s' % args.objective)
            sys.exit(1)
        if nnet_type not in ('blstm', 'cudnnlstm', 'lstm'):
            tflog.fatal('unsupported nnet_type: %s' % nnet_type)
            sys.exit(1)
        teacher_pipe, teacher_graph = teacher_keywords(args, teacher, nnet_config)
        _, pipeline = nnet.create_pipeline_sequence_batch(dataset=tfrecord, input_dim=input_dim,
                                                          batch_size=args.batch_size, batch_threads=args.batch_threads,
                                                          rank=rank, world_size=world, frame_targets=frame_targets,
                                                          **teacher_pipe)
        # nnet-init sets no graph seed (bin/nnet-init.py:27-31): fresh random weights on every run
        create_graph = {'xent': nnet.create_graph_for_validation_xent, 'kd': nnet.create_graph_for_validation_kd}.get(
            args.objective, nnet.create_graph_for_validation_ctc)
        align_window = getattr(args, 'align_window', None)      # nnet-init has no such flag
        windowed = {'align_window': align_window} if align_window is not None else {}
        graph = create_graph(pipeline=pipeline, nnet_config=nnet_config, device=device, seed=None if init_only else 123,
                             **windowed, **teacher_graph, **criterion)
        if init_only and pg is not None:                   # every rank must score the same random model
            from lstm_ctc_amd.nnet import dp
            dp.broadcast_(graph.model.ps.flat, pg, src=0)
        graph.pg, graph.world = pg, world
        if not init_only:
            graph.restore(args.nnet_in)
        sess = nnet.Session(graph)
        nnet.validate(sess=sess, graph=graph, evaluate=args.evaluate, report_interval=args.report_interval)
        if frame_targets is not None:
            report_frame_targets(pipeline)
        if teacher is not None:
            report_teacher_scores(pipeline, graph)
        if align_window is not None:
            report_label_windows(graph)
        report_criterion(graph)
        report_time_reduce_short(graph)
        if init_only and rank == 0:
            tflog.info('saving nnet to "%s"' % args.nnet_out)
            graph.save(args.nnet_out)
    except KeyboardInterrupt:
        from lstm_ctc_amd.nnet import tflog
        tflog.fatal('interrupted by user')
        sys.exit(1)


def build_parser(init_only):
    return build_cli(('tfrecords_scp', 'nnet_config', 'nnet_out' if init_only else 'nnet_in'),
                     ('--objective', '--evaluate', '--batch-size', '--batch-threads', '--report-interval',
                      '--frame-targets') + (() if init_only else (
                          '--align-window', '--delay-penalty', '--entropy-weight', '--star-penalty', '--teacher-scores',
                          '--teacher-domain', '--teacher-weight', '--teacher-temperature')))


if __name__ == '__main__':
    args = build_parser(False).parse_args()
    sys.stderr.write('INFO:tensorflow:' + ' '.join(sys.argv) + '\n')
    run(args, init_only=False)
