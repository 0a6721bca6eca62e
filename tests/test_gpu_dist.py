"""Data-parallel path of mcl_step on real kernels (SURVEY.md section 8(e) validation: N ranks fed identical batches must
reproduce the 1-GPU update): two fresh child processes share the one GPU and exchange gradients over gloo (the box has
a single GPU; RCCL needs one device per rank), with the chunked / progress-driven exchange of muscle_amd.dist."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_cpu_host import _free_port, ROOT

pytestmark = pytest.mark.gpu
WORKER = os.path.join(ROOT, "tests", "dp_worker.py")


def _run(world, tmp_path, tag, backend="gloo", **extra):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), WORLD_SIZE=str(world), DP_BACKEND=backend,
               HSA_ENABLE_IPC_MODE_LEGACY="0", **extra)
    outs = [str(tmp_path / f"{tag}_{r}.npz") for r in range(world)]
    procs = [subprocess.Popen([sys.executable, WORKER, ROOT, "step", outs[r]], env=dict(env, RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(world)]
    logs = [p.communicate(timeout=600)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), logs
    return [np.load(o) for o in outs]


def _gpu_count():
    import torch
    return torch.cuda.device_count()          # (does not initialise the GPU in this process)


@pytest.mark.parametrize("backend", ["gloo", pytest.param("nccl", marks=pytest.mark.skipif(_gpu_count() < 2, reason="RCCL needs one GPU per rank"))])
def test_two_ranks_same_batch_reproduce_single_process_update(tmp_path, backend):
    """backend='nccl' is the production path (RCCL all_reduce(AVG) issued from the weight-gradient side stream): it runs
    wherever two GPUs are visible; on the one-GPU boxes both ranks share the GPU and exchange over gloo."""
    (single,) = _run(1, tmp_path, "w1")
    r0, r1 = _run(2, tmp_path, "w2", backend)
    assert int(r0["early"]) > 0 and int(r1["early"]) > 0          # chunks went out while backward was still running
    # both ranks hold the same averaged gradient and took the same update (bit for bit: same reduction, same order)
    assert np.array_equal(r0["arena"], r1["arena"]) and np.array_equal(r0["params"], r1["params"])
    # losses are replica-local: the contract tolerance between two fp32 implementations (1e-4) is the
    # bar here; that a run reproduces its own bits is tests/test_gpu_determinism.py's subject, not this test's
    np.testing.assert_allclose(r0["losses"], single["losses"], rtol=1e-4)
    # averaged gradient == the single-process gradient
    g, gs = r0["arena"].astype(np.float64), single["arena"].astype(np.float64)
    scale = np.abs(gs).max()
    assert np.abs(g - gs).max() <= 2e-3 * scale, np.abs(g - gs).max() / scale
    cos = float(g @ gs / (np.linalg.norm(g) * np.linalg.norm(gs)))
    assert cos >= 0.999999, cos
    # parameters: Adam's first update is lr * sign(g): identical except where a round-off gradient changes sign
    d = np.abs(r0["params"].astype(np.float64) - single["params"].astype(np.float64))
    assert d.max() <= 2.05e-4 and (d > 1e-6).mean() < 0.02, (d.max(), (d > 1e-6).mean())


def test_rccl_branch_runs_on_one_rank_and_is_the_identity(tmp_path):
    """The RCCL branch of muscle_amd.dist (`all_reduce(AVG, async_op=True)` of arena chunks issued from the weight-gradient side
    stream as backward fills the arena, `work.wait()` before the optimizer, `broadcast` of every parameter) on the hardware that is
    there: a ONE-rank "nccl" group with the collectives forced on.  The average over one rank is the identity, so the step must equal
    the plain single-process step bit for bit - which also holds the stream ordering: a collective that ran before its chunk was
    complete, or an optimizer step that did not wait for it, would change the update.  (Two ranks over RCCL need two GPUs: the
    parametrised test above runs them where they are visible.)"""
    (plain,) = _run(1, tmp_path, "p1")
    (rccl,) = _run(1, tmp_path, "r1", "nccl", DP_SINGLE_RANK_RCCL="1")
    assert int(rccl["early"]) > 0                                  # chunks went to RCCL while backward was still running
    assert np.array_equal(plain["arena"], rccl["arena"]) and np.array_equal(plain["params"], rccl["params"])
    assert np.array_equal(plain["losses"], rccl["losses"])


def test_bench_two_ranks_on_one_gpu_prints_the_contract_line():
    """`bench.py --gpus 2` as the driver launches it (torch.distributed.run, one process per rank), rehearsed with both ranks on
    the one GPU of the box and the exchange over gloo (MUSCLE_DIST_BACKEND / MUSCLE_SHARE_GPU): the N > 1 flow of bench.py at
    HEAD - barriers, MAX over ranks of both arithmetic legs, rank 0 printing ONE JSON line - must keep working while no
    multi-GPU node is available to run it for real.  The launcher is a fresh child started before this process... it touches
    no GPU itself."""
    import json
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, MUSCLE_DIST_BACKEND="gloo", MUSCLE_SHARE_GPU="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--model", "efficientnet-b3", "--batch", "8", "--size", "224", "--full"]
    r = subprocess.run(cmd, env=env, cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 2 and d["scaling"] == "weak" and d["value"] > 0
    assert d["config"]["parallelism"] == "dp2" and d["config"]["global_batch"] == 16
    assert "fp32_mfma" in d and d["fp32_mfma"]["value"] > 0            # the other arithmetic's leg ran with WORLD_SIZE = 2 as well
    assert d["roofline"]["achieved"] > 0
