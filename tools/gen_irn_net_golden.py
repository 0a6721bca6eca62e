"""Generate tests/golden/irn_net.npz by running the REFERENCE's EdgeDisplacement (src/backbones/resnet50_irn.py) and the
per-image body of infer_irn.py on the CPU (build container only; never on the GPU box).

    python tools/gen_irn_net_golden.py

The reference is imported as oracle/gen_golden.py::load_reference does.  One more accommodation, confined to this script:
`resnet50_irn.Net.__init__` calls `resnet50.resnet50(pretrained=True, ...)`, which fetches ImageNet weights from a URL
(src/backbones/resnet50.py:115); the name is rebound to the same constructor with pretrained=False and synthetic weights are
loaded with load_state_dict(strict=True).  infer_irn.py cannot be imported (its body sits under __main__ behind the VOC
loader): lines 70-92 are taken from the file's AST and executed unmodified, with propagate_to_edge's hard-wired .cuda()
calls made no-ops as in gen_golden.gen_irn_units.

Stored: the reference's state_dict key list with shapes, and per case the OUTPUTS only (edge, dp, [l2, probe-dot]
summaries of x1..x5 and the concatenations, label map and soft array of the end-to-end case) plus the non-degeneracy
figures asserted below.  Weights and inputs are regenerated on either side from muscle_amd.synth by key and seed.
"""
from __future__ import annotations

import ast
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from muscle_amd import synth  # noqa: E402
from oracle import gen_golden as GG  # noqa: E402

# tag: (crop_size, H, W, seed)
CASES = {"a": (128, 93, 125, 1), "b": (512, 375, 500, 1)}
E2E = dict(case="a", beta=8, exp_times=6, bg_thres=0.35)                       # infer_irn.py's defaults
NAMES = ["x1", "x2", "x3", "x4", "x5", "edge_cat", "dp_cat1", "dp_cat2"]


def build_reference_model(crop_size, sd_np):
    import src.backbones.resnet50 as R50
    import src.backbones.resnet50_irn as RIRN
    orig = R50.resnet50
    R50.resnet50 = lambda pretrained=True, **kw: orig(pretrained=False, **kw)
    try:
        m = RIRN.EdgeDisplacement(crop_size=crop_size)
    finally:
        R50.resnet50 = orig
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd_np.items()}, strict=True)
    m.eval()                              # (the reference's train() override returns None, so eval() does too)
    return m


def run_with_taps(model, x):
    """model(x) plus the tensors the summaries are made of, through forward hooks (the reference's forward is not restated)."""
    taps = {}
    hooks = [getattr(model, f"stage{i}").register_forward_hook(lambda m, a, o, i=i: taps.__setitem__(f"x{i}", o)) for i in range(1, 6)]
    hooks.append(model.fc_edge6.register_forward_hook(lambda m, a, o: taps.__setitem__("edge_cat", a[0])))
    hooks.append(model.fc_dp6.register_forward_hook(lambda m, a, o: taps.__setitem__("dp_cat1", a[0])))
    hooks.append(model.fc_dp7.register_forward_hook(lambda m, a, o: taps.__setitem__("dp_cat2", a[0])))
    with torch.no_grad():
        edge, dp = model(x)
    for h in hooks:
        h.remove()
    return edge, dp, taps


def script_body():
    """Statements of infer_irn.py's per-image loop between lines 70 and 92 that compute (the file writes are left out)."""
    with open(os.path.join(GG.REF, "infer_irn.py")) as f:
        tree = ast.parse(f.read())
    loop = [n for n in ast.walk(tree) if isinstance(n, ast.For) and isinstance(n.iter, ast.Call)
            and getattr(n.iter.func, "id", "") == "tqdm"][0]
    head = [s for s in loop.body if 70 <= s.lineno and s.end_lineno <= 82]
    tail = {}
    for s in loop.body:
        if isinstance(s, ast.If):
            for branch, nm in ((s.body, "soft"), (s.orelse, "hard")):
                tail[nm] = [a for a in branch if isinstance(a, ast.Assign) and a.end_lineno <= 92
                            and not (isinstance(a.value, ast.Call) and getattr(a.value.func, "attr", "") == "fromarray")]
    comp = lambda st: compile(ast.Module(st, []), "infer_irn.py", "exec")
    return comp(head), comp(tail["soft"]), comp(tail["hard"])


def main():
    src = GG.load_reference()
    import src.indexing as RI
    torch.set_num_threads(8)
    out = {}
    for tag, (crop, H, W, seed) in CASES.items():
        sd = synth.irn_state_dict(seed)
        model = build_reference_model(crop, sd)
        if tag == "a":
            ref_sd = model.state_dict()
            assert set(ref_sd) == set(synth.irn_state_dict_spec()), "synth.irn_state_dict_spec() != the reference's key set"
            out["keys"] = np.array(list(ref_sd))
            out["shapes"] = np.array([",".join(str(d) for d in v.shape) for v in ref_sd.values()])
        x = torch.from_numpy(synth.irn_image_pair(H, W, seed))
        edge, dp, taps = run_with_taps(model, x)
        # non-degeneracy of the synthetic weights, asserted on the reference's own output (the comparisons mean nothing otherwise)
        amax = max(float(taps[k].abs().max()) for k in NAMES)
        assert all(bool(torch.isfinite(taps[k]).all()) for k in NAMES) and amax < 1e4, (tag, amax)
        p5, p95 = (float(v) for v in np.percentile(edge.numpy(), [5, 95]))
        assert p95 - p5 >= 0.2 and 0.02 < p5 and p95 < 0.98, (tag, p5, p95)
        dstd = [float(dp[c].std()) for c in range(2)]
        assert min(dstd) > 1e-3, (tag, dstd)
        out[f"{tag}_params"] = np.array([crop, H, W, seed], np.int64)
        out[f"{tag}_edge"], out[f"{tag}_dp"] = edge.numpy(), dp.numpy()
        out[f"{tag}_summary"] = GG.tensor_summary([(k, taps[k]) for k in NAMES])
        out[f"{tag}_checks"] = np.array([amax, p5, p95] + dstd)
        print(tag, "max|x|", amax, "edge p5/p95", p5, p95, "std(dp)", dstd, flush=True)
        if tag == E2E["case"]:
            head, soft_c, hard_c = script_body()
            cam = synth.irn_cam_dict(H, W, seed)

            class A:
                beta, exp_times, sem_seg_bg_thres = E2E["beta"], E2E["exp_times"], E2E["bg_thres"]
            ns = dict(np=np, torch=torch, F=F, indexing=RI, cam=cam, orig_img_size=x.shape, edge=edge, args=A)
            orig = torch.Tensor.cuda
            torch.Tensor.cuda = lambda self, *a, **k: self
            try:
                exec(head, ns)
            finally:
                torch.Tensor.cuda = orig
            exec(soft_c, ns)
            soft = ns["res"]
            exec(hard_c, ns)
            label = ns["res"]
            share = np.bincount(label.ravel(), minlength=21) / label.size
            assert int((share > 0.02).sum()) >= 3, share
            out["e2e_params"] = np.array([E2E["beta"], E2E["exp_times"]], np.int64)
            out["e2e_bg_thres"] = np.array(E2E["bg_thres"])
            out["e2e_label"], out["e2e_soft"] = label, soft
            out["e2e_label_share"] = share
            print("e2e label shares", {int(k): round(float(v), 3) for k, v in enumerate(share) if v > 0}, flush=True)
    path = os.path.join(ROOT, "tests", "golden", "irn_net.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
