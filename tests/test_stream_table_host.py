"""Every C entry point that takes an ``lc_stream_t`` has a row in the stream-discipline table (tests/stream_cases.py, run
by tests/test_gpu_stream_discipline.py) or a named test elsewhere that holds it to the caller's stream.  No GPU needed: a
new entry point fails here until it gets a row."""
import os
import re

import stream_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_entries():
    with open(os.path.join(ROOT, "include", "lstm_ctc_hip.h")) as f:
        return stream_cases.stream_entries(f.read())


def test_parser_finds_the_prototypes():
    """The parser against a header it cannot misread: comments, line breaks, a struct argument, a query without a stream."""
    text = """
    typedef void *lc_stream_t; /* int lc_in_a_comment(lc_stream_t stream); */
    size_t lc_a_workspace_bytes(int n);
    int lc_a(const float *x, int n,
             void *workspace, size_t workspace_bytes, lc_stream_t stream);
    int lc_b(const lc_dir_t *dirs /* host array */, int n, lc_stream_t stream);
    void lc_debug_thing(int mask);
    """
    assert stream_cases.stream_entries(text) == ["lc_a", "lc_b"]
    found = _header_entries()
    with open(os.path.join(ROOT, "include", "lstm_ctc_hip.h")) as f:
        mentions = len(re.findall(r"\blc_stream_t\s+stream\s*\)", re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)))
    assert len(found) == len(set(found)) == mentions >= 55, (len(found), mentions)
    for name in ("lc_ctc_loss", "lc_gemm_f32_nt2", "lc_lstm_bwd_x3", "lc_optimizer_step", "lc_conv_bwd", "lc_spec_augment",
                 "lc_debug_spin", "lc_bn_update_moving"):
        assert name in found, name
    assert "lc_edit_distance_host" not in found and "lc_gemm_workspace_bytes" not in found


def test_every_stream_entry_has_a_row_or_a_named_test():
    rows, elsewhere = stream_cases.covered_entries(), stream_cases.COVERED_ELSEWHERE
    missing = [e for e in _header_entries() if e not in rows and e not in elsewhere]
    assert not missing, "no stream-discipline row for: %s" % ", ".join(missing)


def test_the_table_names_only_real_entries_once():
    found = set(_header_entries())
    for r in stream_cases.ROWS:
        assert r.entries and set(r.entries) <= found, (r.name, r.entries)
    names = [r.name for r in stream_cases.ROWS]
    assert len(names) == len(set(names))
    assert not set(stream_cases.COVERED_ELSEWHERE) & stream_cases.covered_entries()
    assert set(stream_cases.COVERED_ELSEWHERE) <= found


def test_covered_elsewhere_names_tests_that_exist():
    for entry, where in stream_cases.COVERED_ELSEWHERE.items():
        path, test = where.split("::")
        with open(os.path.join(ROOT, path)) as f:
            assert re.search(r"^def %s\(" % re.escape(test), f.read(), flags=re.M), (entry, where)


def test_rows_build_on_the_host():
    """Every row's inputs are made without a device, and integer inputs are integers (the GPU test gives them their final
    values before anything is launched, so that an early launch can never read a garbage index)."""
    import numpy as np
    for r in stream_cases.ROWS:
        c = r.make(np.random.default_rng(0))
        assert c.inp or c.prep, r.name
        for k, v in c.ints.items():
            assert np.issubdtype(np.asarray(v).dtype, np.integer), (r.name, k)
        for k, v in c.inp.items():
            assert not hasattr(v, "is_cuda") or not v.is_cuda, (r.name, k)
            assert (v.dtype.is_floating_point if hasattr(v, "is_cuda") else np.issubdtype(v.dtype, np.floating)), (r.name, k)
        assert set(c.io) <= set(c.inp), r.name
        assert not set(c.out) & (set(c.inp) | set(c.ints)), r.name
