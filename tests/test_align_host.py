"""Host side of the forced-alignment feature: the int32-vector table writer, alignment_segments and the sequential
pipeline's with_target flag.  No GPU needed."""
import os
import struct

import numpy as np
import pytest


def test_int32_vector_binary_round_trip_and_exact_bytes(tmp_path):
    from lstm_ctc_amd.kaldi_io import Int32VectorWriter, read_int32_vector_ark
    path = str(tmp_path / "a.ark")
    w = Int32VectorWriter("ark:" + path)
    vecs = [("utt1", [3, 0, 258, -1]), ("empty", []), ("u3", list(range(70000, 70005)))]
    for k, v in vecs:
        assert w.Write(k, np.asarray(v, np.int64))
    w.Close()
    data = open(path, "rb").read()
    # key, space, \0B, size byte 4, int32 count, count little-endian int32 values
    first = b"utt1 " + b"\x00B" + b"\x04" + b"\x04\x00\x00\x00" + \
            b"\x03\x00\x00\x00" + b"\x00\x00\x00\x00" + b"\x02\x01\x00\x00" + b"\xff\xff\xff\xff"
    assert data.startswith(first)
    empty = b"empty \x00B\x04" + struct.pack("<i", 0)
    assert data[len(first):len(first) + len(empty)] == empty
    back = read_int32_vector_ark(path)
    assert list(back) == [k for k, _ in vecs]
    for k, v in vecs:
        assert back[k].dtype == np.int32 and back[k].tolist() == v


def test_int32_vector_text_round_trip(tmp_path):
    from lstm_ctc_amd.kaldi_io import Int32VectorWriter, read_int32_vector_ark
    path = str(tmp_path / "a.txt")
    w = Int32VectorWriter("ark,t:" + path)
    w.Write("k1", [5, 5, 2])
    w.Write("k2", [])
    w.Write("k3", [-7])
    w.Close()
    assert open(path).read() == "k1 5 5 2 \nk2 \nk3 -7 \n"
    back = read_int32_vector_ark(path, text=True)
    assert list(back) == ["k1", "k2", "k3"]
    assert back["k1"].tolist() == [5, 5, 2] and back["k2"].tolist() == [] and back["k3"].tolist() == [-7]


@pytest.mark.parametrize("spec", ["ark,scp:%(ark)s,%(scp)s", "scp,ark:%(scp)s,%(ark)s"])
def test_int32_vector_scp_offsets(tmp_path, spec):
    from lstm_ctc_amd.kaldi_io import Int32VectorWriter
    ark, scp = str(tmp_path / "a.ark"), str(tmp_path / "a.scp")
    w = Int32VectorWriter(spec % dict(ark=ark, scp=scp))
    vecs = {"first": [1, 2, 3], "second_key": [], "x": [9] * 11}
    for k, v in vecs.items():
        w.Write(k, v)
    w.Close()
    data = open(ark, "rb").read()
    lines = open(scp).read().splitlines()
    assert [l.split()[0] for l in lines] == list(vecs)
    for line in lines:
        key, where = line.split()
        path, _, offset = where.rpartition(":")
        offset = int(offset)
        assert path == ark
        assert data[offset - len(key) - 1:offset] == (key + " ").encode()        # the byte after the key's space
        assert data[offset:offset + 3] == b"\x00B\x04"
        n = struct.unpack("<i", data[offset + 3:offset + 7])[0]
        assert np.frombuffer(data[offset + 7:offset + 7 + 4 * n], "<i4").tolist() == vecs[key]


def test_int32_vector_writer_rejects_other_specifiers(tmp_path):
    from lstm_ctc_amd.kaldi_io import Int32VectorWriter
    with pytest.raises(ValueError):
        Int32VectorWriter("scp:" + str(tmp_path / "x.scp"))


def test_alignment_segments():
    from lstm_ctc_amd.ops import alignment_segments
    B_ = 4                                                   # blank
    #            t: 0   1   2   3   4   5   6   7   8   9
    ali = np.array([[B_, 2, 2, B_, 2, 3, 3, B_, -1, -1],     # equal labels separated by a blank, then a different one
                    [1, 1, 1, 0, 0, B_, B_, B_, B_, B_],     # starts on a label
                    [B_, B_, B_, -1, -1, -1, -1, -1, -1, -1],  # all blank
                    [-1] * 10,                               # no path
                    [2, 3, 3, 1, 1, 1, 1, 1, 1, 0]], np.int32)   # ends on a label, full length
    idx = np.array([[-1, 0, 0, -1, 1, 2, 2, -1, -1, -1],
                    [0, 0, 1, 2, 2, -1, -1, -1, -1, -1],     # frames 0-1 and frame 2 carry the SAME symbol but two labels
                    [-1] * 10,
                    [-1] * 10,
                    [0, 1, 1, 2, 2, 3, 3, 3, 3, 4]], np.int32)  # ... and here 1,1 | 1,1,1,1 not separated either
    seq = np.array([8, 10, 3, 6, 10], np.int32)
    segs = alignment_segments(ali, idx, seq)
    assert segs[0] == [(2, 1, 2), (2, 4, 1), (3, 5, 2)]
    assert segs[1] == [(1, 0, 2), (1, 2, 1), (0, 3, 2)]
    assert segs[2] == [] and segs[3] == []
    assert segs[4] == [(2, 0, 1), (3, 1, 2), (1, 3, 2), (1, 5, 4), (0, 9, 1)]
    # frames beyond seq_len are ignored even when they hold something
    assert alignment_segments(ali[4:5], idx[4:5], [4]) == [[(2, 0, 1), (3, 1, 2), (1, 3, 1)]]


def _write_utts(tmp_path, with_labels):
    import __graft_entry__ as g
    g.build()
    from lstm_ctc_amd.nnet import write_tfrecord
    rng = np.random.RandomState(5)
    scp, utts = str(tmp_path / "t.scp"), []
    with open(scp, "w") as f:
        for i, (T, lab) in enumerate([(6, [1, 2, 2]), (4, []), (9, [0])]):
            x = rng.randn(T, 3).astype(np.float32)
            path = str(tmp_path / ("utt%d.tfrecords" % i))
            write_tfrecord(path, x, lab if with_labels else None)
            f.write("utt%d %d 3 %d %s\n" % (i, T, int(with_labels), path))
            utts.append((x, lab))
    return scp, utts


def test_sequential_pipeline_with_target_carries_the_labels(tmp_path):
    import lstm_ctc_amd.nnet as nnet
    scp, utts = _write_utts(tmp_path, True)
    filename, ds, _ = nnet.dataset_from_tfrecords(tfrecords_scp=scp)
    _, pipe = nnet.create_pipeline_sequential(filename=filename, tfrecord=ds, with_target=True)
    items = list(pipe)
    assert len(items) == len(utts) == len(pipe)
    for it, (x, lab) in zip(items, utts):
        assert set(it) == {"filename", "nnet_input", "sequence_length", "nnet_target"}
        assert it["nnet_target"].dtype == np.int64 and it["nnet_target"].tolist() == lab
        assert np.array_equal(it["nnet_input"], x) and int(it["sequence_length"]) == x.shape[0]
    # a list without labels: the key is there and empty
    scp0, _ = _write_utts(tmp_path, False)
    filename, ds, _ = nnet.dataset_from_tfrecords(tfrecords_scp=scp0)
    _, pipe = nnet.create_pipeline_sequential(filename=filename, tfrecord=ds, with_target=True)
    assert [it["nnet_target"].tolist() for it in pipe] == [[], [], []]


def test_sequential_pipeline_default_keys_unchanged(tmp_path):
    import lstm_ctc_amd.nnet as nnet
    scp, utts = _write_utts(tmp_path, True)
    filename, ds, _ = nnet.dataset_from_tfrecords(tfrecords_scp=scp)
    for pipe in (nnet.create_pipeline_sequential(filename=filename, tfrecord=ds)[1],
                 nnet.create_pipeline_sequential(filename, ds, 1)[1]):
        items = list(pipe)
        assert [set(it) for it in items] == [{"filename", "nnet_input", "sequence_length"}] * len(utts)
        assert [it["filename"] for it in items] == filename


def test_cli_tables_hold_the_alignment_entries():
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("_common_for_test", os.path.join(root, "bin", "_common.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    p = mod.build_cli(('tfrecords_scp', 'nnet_config', 'nnet_in', 'alignment'),
                      ('--batch-utts', '--report-interval', '--segments', '--scores'))
    a = p.parse_args(["a.scp", "cfg", "in", "ark:out", "--segments", "s.txt"])
    assert (a.alignment, a.segments, a.scores, a.batch_utts, a.report_interval) == ("ark:out", "s.txt", None, 16, 100)
