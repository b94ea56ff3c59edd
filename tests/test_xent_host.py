"""Host side of the frame cross-entropy objective: frame targets in the batching pipeline, the --frame-targets flag of the
three training CLIs and the library version.  No GPU needed."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLIS = ("nnet-train.py", "nnet-validate.py", "nnet-init.py")


class _FakeDataset:
    """Any dataset with ``load`` (no ``open_batch``): the pipeline pads its utterance dicts in ``_collate``."""
    has_label = False

    def __init__(self, frames, dim):
        self.files = ["/corpus/part%d/utt%d.tfrecords" % (i % 2, i) for i in range(len(frames))]
        self.frames = dict(zip(self.files, frames))
        self.dim = dim

    def __len__(self):
        return len(self.files)

    def load(self, path):
        T = self.frames[path]
        return {"nnet_input": np.full((T, self.dim), float(T), np.float32), "sequence_length": np.int32(T)}


def test_pipeline_collates_frame_targets():
    import lstm_ctc_amd.nnet as nnet
    from lstm_ctc_amd.nnet.pipeline import SequenceBatchPipeline
    assert SequenceBatchPipeline.utterance_key("/a/b.c/utt7.tfrecords") == "utt7"       # basename without extension
    assert SequenceBatchPipeline.utterance_key("utt8") == "utt8"
    ds = _FakeDataset([5, 3, 4, 6, 2], 3)
    table = {"utt0": np.array([4, 0, 1, 4, 4], np.int32),      # fits (the blank 4 is a target like any other)
             "utt1": np.array([2, 2, 2, 2], np.int32),         # 4 entries for 3 frames: mismatch
             # utt2: no entry
             "utt3": np.array([1, -1, 3, 3, 0, 4], np.int64),  # fits, holds an "ignore"
             "utt4": np.array([0, 1], np.int32),
             "stranger": np.array([1], np.int32)}
    _, pipe = nnet.create_pipeline_sequence_batch(dataset=ds, input_dim=3, batch_size=3, frame_targets=table)
    batches = list(pipe)
    assert [b["frame_target"].shape for b in batches] == [(3, 5), (2, 6)]
    for b in batches:
        assert b["frame_target"].dtype == np.int32
        assert b["frame_target"].shape == b["nnet_input"].shape[:2]
    assert batches[0]["frame_target"].tolist() == [[4, 0, 1, 4, 4], [-1] * 5, [-1] * 5]
    assert batches[1]["frame_target"].tolist() == [[1, -1, 3, 3, 0, 4], [0, 1, -1, -1, -1, -1]]
    assert (pipe.targets_missing, pipe.targets_mismatched) == (1, 1)
    # the other keys are what they were
    assert batches[0]["sequence_length"].tolist() == [5, 3, 4] and batches[0]["nnet_target"].shape == (3, 0)


def test_pipeline_without_frame_targets_is_unchanged():
    import lstm_ctc_amd.nnet as nnet
    ds = _FakeDataset([2, 3], 2)
    _, pipe = nnet.create_pipeline_sequence_batch(dataset=ds, input_dim=2, batch_size=2)
    (batch,) = list(pipe)
    assert set(batch) == {"nnet_input", "nnet_target", "sequence_length", "target_length"}


def test_native_and_generic_paths_agree_on_frame_targets(tmp_path):
    """The native ``_assemble`` path (TFRecordDataset.open_batch) against ``_collate``, with
    subsampling: an entry must have the frame count AFTER splice and subsample."""
    import __graft_entry__ as g
    g.build()
    import lstm_ctc_amd.nnet as nnet
    rng = np.random.RandomState(2)
    scp = str(tmp_path / "t.scp")
    with open(scp, "w") as f:
        for i, T in enumerate([7, 4, 9]):
            path = str(tmp_path / ("u%d.tfrecords" % i))
            nnet.write_tfrecord(path, rng.randn(T, 3).astype(np.float32), None)
            f.write("u%d %d 3 0 %s\n" % (i, T, path))
    table = {"u0": np.arange(3, dtype=np.int32), "u1": np.arange(4, dtype=np.int32), "u2": np.arange(4, dtype=np.int32)}
    _, ds, dim = nnet.dataset_from_tfrecords(tfrecords_scp=scp, left_context=1, right_context=1, subsample=2)
    _, pipe = nnet.create_pipeline_sequence_batch(dataset=ds, input_dim=dim, batch_size=3, frame_targets=table)
    (native,) = list(pipe)
    assert native["sequence_length"].tolist() == [3, 2, 4]
    assert native["frame_target"].tolist() == [[0, 1, 2, -1], [-1] * 4, [0, 1, 2, 3]]
    assert (pipe.targets_missing, pipe.targets_mismatched) == (0, 1)

    class Generic:                                   # the same dataset without open_batch
        files, has_label, load, __len__ = ds.files, False, ds.load, lambda self: len(ds.files)
    _, pipe2 = nnet.create_pipeline_sequence_batch(dataset=Generic(), input_dim=dim, batch_size=3, frame_targets=table)
    (generic,) = list(pipe2)
    assert np.array_equal(generic["frame_target"], native["frame_target"])
    assert np.array_equal(generic["nnet_input"], native["nnet_input"])


def _run(cli, *args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", cli)] + list(args), capture_output=True, timeout=120)
    return r.returncode, r.stderr.decode()


def _argv(cli, tmp_path):
    scp = tmp_path / "t.scp"
    scp.write_text("utt0 5 3 0 %s\n" % (tmp_path / "utt0.tfrecords"))
    return [str(scp), "nnet.config", "nnet.in"] + (["nnet.out"] if cli == "nnet-train.py" else [])


@pytest.mark.parametrize("cli", CLIS)
def test_cli_xent_without_frame_targets_is_fatal_before_the_device(cli, tmp_path):
    """--objective xent (the default!) without --frame-targets: the FATAL line about the flag, exit 1 - decided on the host,
    so the same on a box with and without a GPU."""
    for objective in (["--objective", "xent"], []):
        rc, err = _run(cli, *(objective + _argv(cli, tmp_path)))
        fatal = [l for l in err.splitlines() if l.startswith("FATAL:tensorflow:")]
        assert rc == 1 and len(fatal) == 1, err
        assert "--frame-targets" in fatal[0] and "no GPU" not in fatal[0], err


@pytest.mark.parametrize("cli", CLIS)
def test_cli_xent_unreadable_frame_targets_are_fatal(cli, tmp_path):
    argv = _argv(cli, tmp_path)
    foreign = tmp_path / "foreign.txt"
    foreign.write_text("someone_else 1 2 3 \n")
    garbage = tmp_path / "garbage.ark"
    garbage.write_bytes(b"utt0 not a kaldi table")
    for spec, word in (("ark:" + str(tmp_path / "missing.ark"), "cannot read"),
                       ("ark:" + str(garbage), "cannot read"),
                       ("scp:" + str(foreign), "unsupported rspecifier"),
                       ("ark,t:" + str(foreign), "names no utterance")):       # readable, but matches nothing of the scp
        rc, err = _run(cli, "--objective", "xent", "--frame-targets", spec, *argv)
        fatal = [l for l in err.splitlines() if l.startswith("FATAL:tensorflow:")]
        assert rc == 1 and len(fatal) == 1 and word in fatal[0], (spec, err)


def test_read_frame_targets_accepts_the_three_rspecifier_forms(tmp_path):
    import importlib.util
    from lstm_ctc_amd.kaldi_io import Int32VectorWriter
    spec = importlib.util.spec_from_file_location("_common_for_xent_test", os.path.join(ROOT, "bin", "_common.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    scp = tmp_path / "t.scp"
    scp.write_text("a 5 3 0 /x/utt0.tfrecords\n\nb 4 3 0 /x/utt1.tfrecords\n")
    for wspec, rspecs in (("ark:%s", ("ark:%s", "%s")), ("ark,t:%s", ("ark,t:%s",))):
        path = str(tmp_path / "ali")
        w = Int32VectorWriter(wspec % path)
        w.Write("utt1", [3, 3, 0, 1])
        w.Close()
        for rspec in rspecs:
            parser = mod.build_cli(("tfrecords_scp",), ("--objective", "--frame-targets"))
            table = mod.read_frame_targets(parser.parse_args([str(scp), "--frame-targets", rspec % path]))
            assert list(table) == ["utt1"] and table["utt1"].tolist() == [3, 3, 0, 1]
    # every other objective reads nothing (and "ctc" keeps ignoring the flag's absence)
    assert mod.read_frame_targets(mod.build_cli(("tfrecords_scp",), ("--objective", "--frame-targets")).parse_args(
        [str(scp), "--objective", "ctc"])) is None


@pytest.mark.parametrize("cli", CLIS)
def test_cli_help_lists_frame_targets(cli):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", cli), "--help"], capture_output=True, timeout=120)
    text = r.stdout.decode()
    assert r.returncode == 0 and "--frame-targets" in text and "xent" in text


def test_graph_factories_are_exported():
    import lstm_ctc_amd.nnet as nnet
    assert "create_graph_for_training_xent" in nnet.__all__ and "create_graph_for_validation_xent" in nnet.__all__


def test_library_version_is_at_least_3():
    from lstm_ctc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    lib = _lib.load()
    assert lib.lc_version() >= 3
    assert lib.lc_xent_workspace_bytes(10, 3, 44) >= 10 * 3 * 8
    assert lib.lc_xent_workspace_bytes(0, 3, 44) == 0 and lib.lc_xent_workspace_bytes(10, 3, 1) == 0
