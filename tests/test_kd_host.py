"""Host side of teacher-student distillation: the lazy float-matrix table, teacher scores in the batching pipeline, the
--teacher-* flags of the training CLIs, the factories and the library version.  No GPU needed."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLIS = ("nnet-train.py", "nnet-validate.py")
FLAGS = ("--teacher-scores", "--teacher-domain", "--teacher-weight", "--teacher-temperature")


# ----------------------------------------------------------------------------------------------- FloatMatrixTable
def _write_ark(path, mats, text=False):
    from lstm_ctc_amd.kaldi_io import BaseFloatMatrixWriter
    w = BaseFloatMatrixWriter(("ark,t:" if text else "ark:") + str(path))
    for k, m in mats.items():
        w.Write(k, m)
    w.Close()


def _mats(rng):
    return {"utt0": rng.standard_normal((5, 3)).astype(np.float32),
            "empty": np.zeros((0, 3), np.float32),
            "a_much_longer_utterance_key_than_sixteen_bytes": rng.standard_normal((2, 3)).astype(np.float32),
            "u": rng.standard_normal((40, 3)).astype(np.float32)}


def test_float_matrix_table_binary_matches_the_eager_reader(tmp_path):
    from lstm_ctc_amd.kaldi_io import FloatMatrixTable, read_float_matrix_ark
    mats = _mats(np.random.default_rng(0))
    path = tmp_path / "m.ark"
    _write_ark(path, mats)
    eager = read_float_matrix_ark(str(path))
    table = FloatMatrixTable(str(path))
    assert len(table) == 4 and list(table.keys()) == list(mats) == list(eager)
    assert "utt0" in table and "stranger" not in table and table.get("stranger") is None
    for k, m in eager.items():
        assert table.shape(k) == m.shape
        got = table.get(k)
        assert got.dtype == np.float32 and got.shape == m.shape and np.array_equal(got, m) and np.array_equal(table[k], m)
        got[...] = 7                                   # the caller's own copy
        assert np.array_equal(table.get(k), m)
    assert table.get("empty").shape == (0, 3)
    with pytest.raises(KeyError):
        table["stranger"]
    # three threads reading concurrently: no shared file position
    errors = []

    def reader(seed):
        order = np.random.default_rng(seed).permutation(200) % 4
        for i in order:
            k = list(mats)[i]
            if not np.array_equal(table.get(k), mats[k]):
                errors.append(k)

    threads = [threading.Thread(target=reader, args=(s,)) for s in range(3)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors


def test_float_matrix_table_reads_no_body_while_indexing(tmp_path):
    """An ark cut off right behind its last header: the index is complete (so no body was needed for it), the earlier
    matrices read, the missing one raises when it is asked for."""
    from lstm_ctc_amd.kaldi_io import FloatMatrixTable
    mats = _mats(np.random.default_rng(1))
    path = tmp_path / "m.ark"
    _write_ark(path, mats)
    data = path.read_bytes()
    path.write_bytes(data[:len(data) - 40 * 3 * 4])
    table = FloatMatrixTable(str(path))
    assert list(table.keys()) == list(mats) and table.shape("u") == (40, 3)
    assert np.array_equal(table.get("utt0"), mats["utt0"])
    with pytest.raises(OSError):
        table.get("u")
    for garbage in (b"utt0 not a kaldi table", b"nokeyatall", b"k \0BFM \x04\x01\x00"):
        bad = tmp_path / "bad.ark"
        bad.write_bytes(garbage)
        with pytest.raises(ValueError):
            FloatMatrixTable(str(bad))
    with pytest.raises(OSError):
        FloatMatrixTable(str(tmp_path / "missing.ark"))


def test_float_matrix_table_text(tmp_path):
    from lstm_ctc_amd.kaldi_io import FloatMatrixTable
    mats = _mats(np.random.default_rng(2))
    path = tmp_path / "m.txt"
    _write_ark(path, mats, text=True)
    table = FloatMatrixTable(str(path), text=True)
    assert len(table) == 4 and list(table.keys()) == list(mats)
    for k, m in mats.items():
        assert table.shape(k)[0] == m.shape[0] and k in table
        if m.size:
            assert np.abs(table.get(k) - m).max() <= 5e-7          # "%f": six decimals
    assert table.get("empty").size == 0 and table.get("stranger") is None


# ----------------------------------------------------------------------------------------------- the pipeline
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


def _teacher_table(rng, V=4):
    post = lambda n: rng.standard_normal((n, V)).astype(np.float32)
    table = {"utt0": post(5),                          # fits
             "utt1": post(4),                          # 4 rows for 3 frames: mismatch
             # utt2: no entry
             "utt3": post(6),                          # fits, holds a -inf (probability 0: fine)
             "utt4": post(2)[:, :3],                   # another column count: mismatch
             "utt5": post(3),                          # a row of -inf: bad
             "utt6": post(3),                          # a NaN: bad
             "utt7": post(3),                          # a +inf: bad
             "stranger": post(1)}
    table["utt3"][2, 1] = -np.inf
    table["utt5"][1, :] = -np.inf
    table["utt6"][0, 2] = np.nan
    table["utt7"][2, 0] = np.inf
    return table


def test_pipeline_collates_teacher_scores():
    import lstm_ctc_amd.nnet as nnet
    ds = _FakeDataset([5, 3, 4, 6, 2, 3, 3, 3], 3)
    table = _teacher_table(np.random.default_rng(0))
    _, pipe = nnet.create_pipeline_sequence_batch(dataset=ds, input_dim=3, batch_size=4, teacher_scores=table, num_targets=4)
    batches = list(pipe)
    assert [b["teacher_scores"].shape for b in batches] == [(6, 4, 4), (3, 4, 4)]
    for b in batches:
        ts = b["teacher_scores"]
        assert ts.dtype == np.float32 and ts.flags.c_contiguous                       # [T, B, V], time-major
        assert ts.shape[:2] == b["nnet_input"].shape[:2][::-1]
        assert b["teacher_length"].dtype == np.int32
    assert batches[0]["teacher_length"].tolist() == [5, 0, 0, 6] and batches[1]["teacher_length"].tolist() == [0, 0, 0, 0]
    ts = batches[0]["teacher_scores"]
    assert np.array_equal(ts[:5, 0], table["utt0"]) and not ts[5:, 0].any()            # zeros in the padding
    assert np.array_equal(ts[:, 3], table["utt3"]) and ts[2, 3, 1] == -np.inf
    assert not ts[:, 1].any() and not ts[:, 2].any() and not batches[1]["teacher_scores"].any()
    assert (pipe.teacher_missing, pipe.teacher_mismatched, pipe.teacher_bad) == (1, 2, 3)
    # the other keys are what they were
    assert batches[0]["sequence_length"].tolist() == [5, 3, 4, 6] and batches[0]["nnet_target"].shape == (4, 0)
    # num_targets defaults to the first entry's column count
    _, pipe2 = nnet.create_pipeline_sequence_batch(dataset=ds, input_dim=3, batch_size=4, teacher_scores=table)
    assert np.array_equal(next(iter(pipe2))["teacher_scores"], ts)
    with pytest.raises(ValueError, match="teacher_domain"):
        nnet.create_pipeline_sequence_batch(dataset=ds, input_dim=3, batch_size=4, teacher_scores=table, teacher_domain="odds")


def test_pipeline_prob_domain_takes_the_log():
    import lstm_ctc_amd.nnet as nnet
    ds = _FakeDataset([2, 2, 2, 2], 3)
    table = {"utt0": np.array([[0.5, 0.5, 0.0], [0.1, 0.2, 0.7]], np.float32),         # a zero becomes -inf
             "utt1": np.array([[0.5, 0.6, -0.1], [0.1, 0.2, 0.7]], np.float32),        # a negative entry: bad
             "utt2": np.array([[0.0, 0.0, 0.0], [0.1, 0.2, 0.7]], np.float32),         # a row of zeros: bad
             "utt3": np.array([[0.5, np.nan, 0.5], [0.1, 0.2, 0.7]], np.float32)}      # a NaN: bad
    _, pipe = nnet.create_pipeline_sequence_batch(dataset=ds, input_dim=3, batch_size=4, teacher_scores=table,
                                                  teacher_domain="prob", num_targets=3)
    (batch,) = list(pipe)
    assert batch["teacher_length"].tolist() == [2, 0, 0, 0]
    with np.errstate(divide="ignore"):
        assert np.array_equal(batch["teacher_scores"][:, 0], np.log(table["utt0"]))
    assert batch["teacher_scores"][0, 0, 2] == -np.inf and not batch["teacher_scores"][:, 1:].any()
    assert (pipe.teacher_missing, pipe.teacher_mismatched, pipe.teacher_bad) == (0, 0, 3)


def test_pipeline_without_teacher_scores_is_unchanged():
    import lstm_ctc_amd.nnet as nnet
    ds = _FakeDataset([2, 3], 2)
    _, pipe = nnet.create_pipeline_sequence_batch(dataset=ds, input_dim=2, batch_size=2)
    (batch,) = list(pipe)
    assert set(batch) == {"nnet_input", "nnet_target", "sequence_length", "target_length"}


def test_native_and_generic_paths_agree_on_teacher_scores(tmp_path):
    """The native ``_assemble`` path (TFRecordDataset.open_batch) against ``_collate``, with subsampling - an entry must have
    the frame count AFTER splice and subsample - and the table read lazily from an ark."""
    import __graft_entry__ as g
    g.build()
    import lstm_ctc_amd.nnet as nnet
    from lstm_ctc_amd.kaldi_io import FloatMatrixTable
    rng = np.random.RandomState(2)
    scp = str(tmp_path / "t.scp")
    with open(scp, "w") as f:
        for i, T in enumerate([7, 4, 9]):
            path = str(tmp_path / ("u%d.tfrecords" % i))
            nnet.write_tfrecord(path, rng.randn(T, 3).astype(np.float32), None)
            f.write("u%d %d 3 0 %s\n" % (i, T, path))
    mats = {"u0": rng.randn(3, 5).astype(np.float32), "u1": rng.randn(4, 5).astype(np.float32),
            "u2": rng.randn(4, 5).astype(np.float32)}
    _write_ark(tmp_path / "post.ark", mats)
    table = FloatMatrixTable(str(tmp_path / "post.ark"))
    _, ds, dim = nnet.dataset_from_tfrecords(tfrecords_scp=scp, left_context=1, right_context=1, subsample=2)
    _, pipe = nnet.create_pipeline_sequence_batch(dataset=ds, input_dim=dim, batch_size=3, teacher_scores=table, num_targets=5)
    (native,) = list(pipe)
    assert native["sequence_length"].tolist() == [3, 2, 4]
    assert native["teacher_length"].tolist() == [3, 0, 4]
    assert native["teacher_scores"].shape == (4, 3, 5)
    assert np.array_equal(native["teacher_scores"][:3, 0], mats["u0"]) and np.array_equal(native["teacher_scores"][:, 2], mats["u2"])
    assert (pipe.teacher_missing, pipe.teacher_mismatched, pipe.teacher_bad) == (0, 1, 0)

    class Generic:                                   # the same dataset without open_batch
        files, has_label, load, __len__ = ds.files, False, ds.load, lambda self: len(ds.files)
    _, pipe2 = nnet.create_pipeline_sequence_batch(dataset=Generic(), input_dim=dim, batch_size=3, teacher_scores=table,
                                                   num_targets=5)
    (generic,) = list(pipe2)
    assert np.array_equal(generic["teacher_scores"], native["teacher_scores"])
    assert np.array_equal(generic["teacher_length"], native["teacher_length"])
    assert np.array_equal(generic["nnet_input"], native["nnet_input"])


# ----------------------------------------------------------------------------------------------- command lines
def _run(cli, *args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", cli)] + list(args), capture_output=True, timeout=120)
    return r.returncode, r.stderr.decode()


def _argv(cli, tmp_path):
    scp = tmp_path / "t.scp"
    scp.write_text("utt0 5 3 0 %s\n" % (tmp_path / "utt0.tfrecords"))
    return [str(scp), "nnet.config", "nnet.in"] + (["nnet.out"] if cli == "nnet-train.py" else [])


def _fatal(err):
    return [l for l in err.splitlines() if l.startswith("FATAL:tensorflow:")]


@pytest.mark.parametrize("cli", CLIS + ("nnet-init.py",))
def test_cli_kd_without_teacher_scores_is_fatal_before_the_device(cli, tmp_path):
    rc, err = _run(cli, "--objective", "kd", *_argv(cli, tmp_path))
    fatal = _fatal(err)
    assert rc == 1 and len(fatal) == 1, err
    assert "--teacher-scores" in fatal[0] and "no GPU" not in fatal[0], err


@pytest.mark.parametrize("cli", CLIS)
def test_cli_unreadable_teacher_scores_are_fatal(cli, tmp_path):
    argv = _argv(cli, tmp_path)
    _write_ark(tmp_path / "foreign.ark", {"someone_else": np.zeros((2, 3), np.float32)})
    _write_ark(tmp_path / "foreign.txt", {"someone_else": np.zeros((2, 3), np.float32)}, text=True)
    garbage = tmp_path / "garbage.ark"
    garbage.write_bytes(b"utt0 not a kaldi table")
    for objective in ("kd", "ctc"):
        for spec, word in (("ark:" + str(tmp_path / "missing.ark"), "cannot read"),
                           ("ark:" + str(garbage), "cannot read"),
                           ("scp:" + str(garbage), "unsupported rspecifier"),
                           (str(tmp_path / "foreign.ark"), "names no utterance"),      # readable, but matches nothing of the scp
                           ("ark,t:" + str(tmp_path / "foreign.txt"), "names no utterance")):
            rc, err = _run(cli, "--objective", objective, "--teacher-scores", spec, *argv)
            fatal = _fatal(err)
            assert rc == 1 and len(fatal) == 1 and word in fatal[0] and "no GPU" not in fatal[0], (spec, err)


@pytest.mark.parametrize("cli", CLIS)
def test_cli_weight_and_temperature_must_be_positive(cli, tmp_path):
    argv = _argv(cli, tmp_path)
    _write_ark(tmp_path / "post.ark", {"utt0": np.zeros((5, 3), np.float32)})
    for flag in ("--teacher-weight", "--teacher-temperature"):
        for value in ("0", "-1.5", "nan", "inf"):
            rc, err = _run(cli, "--objective", "ctc", "--teacher-scores", "ark:" + str(tmp_path / "post.ark"), flag, value, *argv)
            fatal = _fatal(err)
            assert rc == 1 and len(fatal) == 1 and flag in fatal[0] and "no GPU" not in fatal[0], (flag, value, err)
    rc, err = _run(cli, "--objective", "ctc", "--teacher-scores", "ark:" + str(tmp_path / "post.ark"), "--teacher-domain", "odds", *argv)
    assert rc == 1 and "--teacher-domain" in _fatal(err)[0], err


@pytest.mark.parametrize("cli", CLIS)
def test_cli_help_lists_the_teacher_flags(cli):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", cli), "--help"], capture_output=True, timeout=120)
    text = r.stdout.decode()
    assert r.returncode == 0 and "kd" in text
    for flag in FLAGS:
        assert flag in text, flag


def test_read_teacher_scores_returns_the_lazy_table(tmp_path):
    import importlib.util
    from lstm_ctc_amd.kaldi_io import FloatMatrixTable
    spec = importlib.util.spec_from_file_location("_common_for_kd_test", os.path.join(ROOT, "bin", "_common.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    scp = tmp_path / "t.scp"
    scp.write_text("a 5 3 0 /x/utt0.tfrecords\n\nb 4 3 0 /x/utt1.tfrecords\n")
    m = np.arange(12, dtype=np.float32).reshape(4, 3)
    flags = ("--objective",) + FLAGS
    for text, rspecs in ((False, ("ark:%s", "%s")), (True, ("ark,t:%s",))):
        path = str(tmp_path / "post")
        _write_ark(path, {"utt1": m}, text=text)
        for rspec in rspecs:
            args = mod.build_cli(("tfrecords_scp",), flags).parse_args([str(scp), "--objective", "ctc", "--teacher-scores", rspec % path,
                                                                        "--teacher-weight", "0.5", "--teacher-temperature", "2"])
            table = mod.read_teacher_scores(args)
            assert isinstance(table, FloatMatrixTable) and list(table.keys()) == ["utt1"] and np.array_equal(table.get("utt1"), m)
            pipe_kw, graph_kw = mod.teacher_keywords(args, table, {"num_targets": 3})
            assert pipe_kw == {"teacher_scores": table, "teacher_domain": "log", "num_targets": 3}
            assert graph_kw == {"teacher_weight": 0.5, "teacher_temperature": 2.0}
    _write_ark(path, {"utt1": m})
    args = mod.build_cli(("tfrecords_scp",), flags).parse_args([str(scp), "--objective", "kd", "--teacher-scores", path])
    assert mod.teacher_keywords(args, mod.read_teacher_scores(args), {"num_targets": 3})[1] == {"teacher_temperature": 1.0}
    # without the flag nothing is read and nothing is passed on
    args = mod.build_cli(("tfrecords_scp",), flags).parse_args([str(scp), "--objective", "ctc"])
    assert mod.read_teacher_scores(args) is None and mod.teacher_keywords(args, None, {}) == ({}, {})


# ----------------------------------------------------------------------------------------------- exports and the library
def test_graph_factories_are_exported():
    import lstm_ctc_amd.nnet as nnet
    assert "create_graph_for_training_kd" in nnet.__all__ and "create_graph_for_validation_kd" in nnet.__all__
    assert callable(nnet.create_graph_for_training_kd) and callable(nnet.create_graph_for_validation_kd)


def test_signatures_declare_the_kd_entries():
    from lstm_ctc_amd import _lib
    assert len(_lib.SIGNATURES["lc_kd_workspace_bytes"][1]) == 3
    assert len(_lib.SIGNATURES["lc_kd_loss"][1]) == 17
    header = open(os.path.join(ROOT, "include", "lstm_ctc_hip.h")).read()
    assert "int lc_kd_loss(" in header and "size_t lc_kd_workspace_bytes(int T, int B, int V);" in header


def test_library_version_is_at_least_5():
    from lstm_ctc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    lib = _lib.load()
    assert lib.lc_version() >= 5
    assert lib.lc_kd_workspace_bytes(10, 3, 44) >= 10 * 3 * 8
    assert lib.lc_kd_workspace_bytes(0, 3, 44) == 0 and lib.lc_kd_workspace_bytes(10, 3, 1) == 0
