"""GPU parity: the HIP MBConv chain (muscle_amd.engine) against the CPU oracle on the same seeded
weights and inputs.  Stated fp32 tolerance: features max-abs <= 1e-3*max|ref| (we hold
2e-4), parameter-gradient vectors cosine >= 0.9999 and max-abs <= 1e-3*max|ref| per tensor norm scale."""
import numpy as np
import pytest
import torch

import golden_util as gu
from muscle_amd import synth
from muscle_amd.arch import net_cfg

pytestmark = [pytest.mark.gpu, pytest.mark.both_arith]


def _build(name, seed, dev):
    from muscle_amd.efficientnet import EfficientNet
    cfg = net_cfg(name, False)
    sd = synth.synth_state_dict(cfg, seed)
    bb = EfficientNet(cfg, 21)
    bb.load_state_dict({k[len("backbone."):]: torch.from_numpy(np.asarray(v)) for k, v in sd.items()
                        if k.startswith("backbone.")}, strict=True)
    return cfg, sd, bb.to(dev)


# B7 is covered through the whole model (tests/test_gpu_model.py::test_model_forward_backward[efficientnet-b7...], which runs
# the same backbone) and by the reference's B7 step fixtures.  The oracle's fp32 + fp64 passes for these cases are stored
# (oracle/gen_oracle_runs.py::backbone_run -> tests/golden/oracle_runs): run inside the test they cost 20-33 s each on the
# GPU box's host share.
_PROBES = {}


@pytest.mark.parametrize("name,n,size,training", [("efficientnet-b0", 3, 64, True), ("efficientnet-b0", 2, 72, False),
                                                   ("efficientnet-b3", 2, 96, True)])
def test_backbone_forward_backward(name, n, size, training):
    _run(name, n, size, training)


@pytest.mark.parametrize("name,n,size", [("efficientnet-b0", 3, 64), ("efficientnet-b3", 2, 96)])
def test_backbone_backward_unfused_stride2_depthwise(name, n, size, monkeypatch):
    """engine.DW_S2_FUSED off (MUSCLE_DW_S2_FUSED=0): every stride-2 block's depthwise backward goes through bn_backward_from_coeffs,
    dwconv_bwd_weight and dwconv_bwd_data instead of dwconv_bwd_fused_s2, and is held to the same oracle at the same tolerance."""
    from muscle_amd import engine, ops
    calls = {"dwconv_bwd_data": 0, "dwconv_bwd_weight": 0, "dwconv_bwd_fused_s2": 0}

    def counted(fname):
        inner = getattr(ops, fname)

        def wrapper(*a, **k):
            calls[fname] += 1
            return inner(*a, **k)
        return wrapper
    for fname in calls:
        monkeypatch.setattr(ops, fname, counted(fname))
    monkeypatch.setattr(engine, "DW_S2_FUSED", False)
    cfg = _run(name, n, size, True)
    s2 = sum(1 for b in cfg.blocks if b.stride == 2)
    assert s2 > 0
    assert calls == {"dwconv_bwd_data": s2, "dwconv_bwd_weight": s2, "dwconv_bwd_fused_s2": 0}


def _run(name, n, size, training):
    from muscle_amd import engine
    from test_gpu_model import run_case
    dev = torch.device("cuda:0")
    seed = 17
    cfg, sd, bb = _build(name, seed, dev)
    x = torch.from_numpy(synth.normal(seed, "x", (n, 3, size, size)).astype(np.float32))
    du = gu.drop_draws(cfg, n, 5)
    F = gu.load_run(run_case("backbone", name, n, size, training))
    cache = _PROBES.setdefault((name, n, size, training), {})

    tape = engine.backbone_forward(bb, cfg, x.to(dev), training, {k: v.to(dev) for k, v in du.items()})
    feats = [blk.out.permute(0, 3, 1, 2).contiguous() for blk in tape.blocks]
    gu.check_outputs(feats, F, "feat", 2e-4, cache)
    if training:   # running statistics
        rs = {str(k): F["rs_vals"][F["rs_off"][i]:F["rs_off"][i + 1]] for i, k in enumerate(F["rs_keys"])}
        seen = 0
        for k, v in bb.state_dict().items():
            if k.endswith("running_mean") or k.endswith("running_var"):
                assert gu.rel_err(v.cpu().flatten(), rs["backbone." + k]) <= 1e-4, k
                seen += 1
        assert seen == len(rs)
    sink = engine.GradSink()
    taps = cfg.taps
    tg = {i: torch.from_numpy(synth.normal(seed, f"probe{i}", tuple(feats[i].shape)).astype(np.float32))
          .permute(0, 2, 3, 1).contiguous().to(dev) for i in (taps[0], taps[2], taps[4], taps[6])}
    engine.backbone_backward(bb, cfg, tape, tg, sink)
    torch.cuda.synchronize()
    worst = gu.check_grads_fixture({"backbone." + k: sink.bufs.get(id(p)) for k, p in bb.named_parameters()}, F, 2e-3, cache)
    print("worst grad rel err", worst)
    return cfg
