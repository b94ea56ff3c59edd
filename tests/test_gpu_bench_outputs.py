"""bench.py's plain run on the GPU: the line carries the headline fields and nothing that needs runs of its own (those
need --full), and --dump-outputs writes what the timed path computed in its last step - the same model, batch and seeds
stepped in this process give the same loss and parameters."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FULL_ONLY = ("secondary", "secondary_protocol", "inference", "cli_corpus", "cpu_baseline", "cpu_baseline_sample",
             "cpu_baseline_c2_full")


def _clean_env(**extra):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", **extra)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "TORCHELASTIC_RUN_ID", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return env


def test_plain_run_dumps_the_last_timed_step(tmp_path):
    name, steps, warmup = "rehearsal_keep1", 2, 1
    out = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", name, "--steps", str(steps),
           "--warmup", str(warmup), "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, timeout=600, env=_clean_env(), cwd=ROOT)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    lines = [l for l in r.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == steps and line["warmup"] == warmup and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "frames/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert not set(FULL_ONLY) & set(line), sorted(set(FULL_ONLY) & set(line))
    assert "large_batch" not in line.get("roofline_ctc", {})
    assert line["config"]["persist_fallbacks"] == 0

    files = sorted(os.listdir(out))
    assert files == ["eval_loss.npy", "grad_norm.npy", "grads.npy", "loss.npy", "params.npy"]
    assert sum(os.path.getsize(out / f) for f in files) <= 64 << 20
    got = {f[:-len(".npy")]: np.load(out / f) for f in files}
    for k in ("loss", "eval_loss", "grad_norm"):
        assert got[k].dtype == np.float64 and got[k].shape == () and np.isfinite(got[k]), k
    assert got["params"].dtype == np.float32 and got["grads"].dtype == np.float32

    # the same steps in this process: one graph, the workload's seeded batch, warm-up + timed steps
    sys.path.insert(0, ROOT)
    import bench
    from lstm_ctc_amd.nnet.graph import create_graph_for_training_ctc
    w = bench.WORKLOADS[name]
    graph = create_graph_for_training_ctc(None, w["cfg"], learn_rate=4e-4, clip_norm=5.0, optimizer="adam",
                                          device=torch.device("cuda", 0), seed=123)
    x, seq, labels, offs = bench.synth_batch(w, 0, "cuda:0")
    size = int(labels.numel())
    init = graph.model.ps.flat.detach().cpu().numpy().copy()
    for _ in range(warmup + steps):
        res = graph.step_device(x, seq, labels, offs, w["L"], size, fetch_eval=False)
    torch.cuda.synchronize()
    ref = graph.model.ps.flat.detach().cpu().numpy()
    assert got["params"].shape == ref.shape == (graph.model.ps.n,)        # small model: the whole vector, no sample
    assert abs(float(got["eval_loss"]) / size - line["config"]["last_loss_per_label"]) < 1e-4
    assert float(got["loss"]) == pytest.approx(res["loss"], rel=1e-5)
    assert float(got["grad_norm"]) == pytest.approx(res["grad_norm"], rel=1e-4)
    # 3 Adam steps move every weight by ~1e-3; the CTC gradient's float atomics leave summation-order noise only
    # (the bounds of test_gpu_round6.py's eight-rank comparison)
    assert float(np.abs(ref - init).max()) > 5e-4
    diff = np.abs(got["params"].astype(np.float64) - ref)
    assert float(diff.max()) < 2e-5 and float(np.sqrt((diff ** 2).mean())) < 1e-6, (float(diff.max()),
                                                                                  float(np.sqrt((diff ** 2).mean())))
