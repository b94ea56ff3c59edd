#!/usr/bin/env python3
"""CTC forced alignment: per utterance the best-path (Viterbi) symbol of every frame -> Kaldi int32-vector table.
New here (the reference has no counterpart: TF 1.8 offers no such op); built like bin/nnet-forward.py: utterances go
through the GPU in padded batches of consecutive files, the outputs do not depend on the batch size and are written in
scp order.  An utterance without labels, or whose labels do not fit its frames, is skipped with a WARNING."""
import os
import sys

from _common import build_cli, setup_device, report_chunking, report_row_conv, report_layer_norm, report_conv, report_time_reduce, star_report_keywords, star_report_line


def main(args):
    import numpy as np
    tolerant = star_report_keywords(args)                 # --star-penalty / --star-report; fatal before the device is touched
    device, _, _, _ = setup_device()
    import lstm_ctc_amd.nnet as nnet
    from lstm_ctc_amd import ops
    from lstm_ctc_amd.kaldi_io import Int32VectorWriter
    from lstm_ctc_amd.nnet import tflog
    writer = Int32VectorWriter(args.alignment)
    segments = open(args.segments, "w") if args.segments else None
    scores = open(args.scores, "w") if args.scores else None
    report = open(args.star_report, "w") if tolerant else None
    nnet_config = nnet.parse_config(args.nnet_config)
    nnet_config['is_training'] = False
    report_chunking(nnet_config)                          # chunk_frames / lookahead_frames: one INFO line
    report_row_conv(nnet_config)                          # row_conv_frames: one INFO line
    report_layer_norm(nnet_config)                        # layer_norm: one INFO line
    report_conv(nnet_config)                              # conv_layers: one INFO line
    report_time_reduce(nnet_config, aligning=True)        # time_reduce_layers: fatal, alignments are per input frame
    filename, tfrecord, _ = nnet.dataset_from_tfrecords(
        tfrecords_scp=args.tfrecords_scp, left_context=nnet_config.get('left_context'),
        right_context=nnet_config.get('right_context'), subsample=nnet_config.get('subsample'), shuffle=False)
    _, pipeline = nnet.create_pipeline_sequential(filename=filename, tfrecord=tfrecord, with_target=True)
    graph = nnet.create_graph_for_alignment(pipeline=pipeline, nnet_config=nnet_config, device=device)
    graph.restore(args.nnet_in)
    from lstm_ctc_amd.nnet.funcs import StepWatchdog
    dog = StepWatchdog(tag="align batch").start()       # a hung runtime call ends the process with status 1 (LC_STEP_TIMEOUT)
    try:
        processed = skipped = 0
        pending = []

        def flush():
            nonlocal processed, skipped
            if not pending:
                return
            B = len(pending)
            T = max(p["nnet_input"].shape[0] for p in pending)
            L = max(len(p["nnet_target"]) for p in pending)
            x = np.zeros((B, T, pending[0]["nnet_input"].shape[1]), np.float32)
            y = np.full((B, L), -1, np.int64)
            for b, p in enumerate(pending):
                x[b, :p["nnet_input"].shape[0]] = p["nnet_input"]
                y[b, :len(p["nnet_target"])] = p["nnet_target"]
            seq = np.asarray([p["nnet_input"].shape[0] for p in pending], np.int32)
            out = graph.align({"nnet_input": x, "nnet_target": y, "sequence_length": seq}, **tolerant)
            segs = ops.alignment_segments(out["ali"], out["label_index"], seq) if segments else None
            dog.kick()                 # the device part of the batch is done ...
            dog.pause()                # ... and back-pressure from whoever reads the table is not a hang
            for b, p in enumerate(pending):
                key, _ = os.path.splitext(os.path.basename(p["filename"]))
                processed += 1
                if report and 0 < len(p["nnet_target"]) <= seq[b]:
                    report.write(star_report_line(key, seq[b], len(p["nnet_target"]), float(out["ctc_loss"][b]),
                                                  float(out["star_loss"][b]), float(out["star_frames"][b])))
                if len(p["nnet_target"]) == 0:
                    tflog.info('WARNING: %s has no labels, skipped' % key)
                    skipped += 1
                elif not np.isfinite(out["score"][b]):
                    tflog.info('WARNING: %s has no alignment (%d labels do not fit %d frames), skipped'
                               % (key, len(p["nnet_target"]), seq[b]))
                    skipped += 1
                else:
                    writer.Write(key, out["ali"][b, :seq[b]])
                    if segments:
                        for label, start, n in segs[b]:
                            segments.write("%s %d %d %d\n" % (key, label, start, n))
                    if scores:
                        scores.write("%s %.6f\n" % (key, float(out["score"][b])))
                if args.report_interval and processed % args.report_interval == 0:
                    tflog.info('processed = %d' % processed)
            pending.clear()
            dog.resume()

        for item in pipeline:
            pending.append(item)
            if len(pending) >= args.batch_utts:
                flush()
        flush()
        tflog.info('done, %d utterances aligned, %d skipped' % (processed - skipped, skipped))
    except KeyboardInterrupt:
        tflog.fatal('interrupted by user')
        sys.exit(1)
    finally:
        dog.stop()
    writer.Close()
    for f in (segments, scores, report):
        if f is not None:
            f.close()


if __name__ == '__main__':
    args = build_cli(('tfrecords_scp', 'nnet_config', 'nnet_in', 'alignment'),
                     ('--batch-utts', '--report-interval', '--segments', '--scores', '--star-penalty', '--star-report')).parse_args()
    sys.stderr.write('INFO:tensorflow:' + ' '.join(sys.argv) + '\n')
    main(args)
