"""Generate tests/golden/irn_train.npz by running the REFERENCE's AffinityDisplacementLoss (src/backbones/resnet50_irn.py:143-212),
GetAffinityLabelFromIndices (src/data.py:611-637), PolyOptimizer (src/torchutils.py:11-33) and the imutils functions that
VOC12AffinityDataset calls, on the CPU (build container only; never on the GPU box).

    python tools/gen_irn_train_golden.py

The reference is imported as tools/gen_irn_net_golden.py does (resnet50(pretrained=True) rebound, synthetic weights).  The loss
combination is the public IRN training loop's (the reference ships the model, not the loop); it is written out below and in
tests/irn_train_ref.py.  Weights and images are regenerated on either side from muscle_amd.synth by seed; the fixture stores the
label maps, the loss-head inputs of the second case, and the reference's outputs in fp64 and fp32.
"""
from __future__ import annotations

import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from muscle_amd import synth  # noqa: E402
from oracle import gen_golden as GG  # noqa: E402

SEED = 3
CASE_A = dict(crop=128, N=2, radius=10)
CASE_B = dict(H=24, W=37, N=3, radius=5)
LOADER = dict(H=150, W=210, crop=128, seeds=(1, 2, 3, 4))
N_PROBE = 64


def labels_a():
    """Two 32 x 32 maps: background, two object classes, an ignore block."""
    lab = np.zeros((2, 32, 32), np.uint8)
    lab[0, 4:15, 8:22] = 5
    lab[0, 12:26, 18:30] = 12
    lab[0, 20:24, 2:9] = 255
    lab[1, 0:9, 0:32] = 15
    lab[1, 14:20, 10:16] = 2
    lab[1, 26:32, 20:32] = 255
    return lab


def labels_b():
    """Three 24 x 37 maps; every sample has bg-pos, neg pairs and a 255 block; sample 2 has no fg-pos pair: its object pixels are
    single pixels of pairwise different classes."""
    lab = np.zeros((3, 24, 37), np.uint8)
    lab[0, 3:10, 6:17] = 7
    lab[0, 15:20, 25:33] = 255
    lab[1, 2:12, 5:14] = 3
    lab[1, 6:16, 14:30] = 20
    lab[1, 18:24, 0:6] = 255
    for i, (y, x) in enumerate([(2, 8), (5, 20), (9, 13), (12, 27), (15, 9), (7, 30), (17, 18)]):
        lab[2, y, x] = i + 1
    lab[2, 19:24, 28:37] = 255
    return lab


def build_model(path_index, sd_np=None):
    import src.backbones.resnet50 as R50
    import src.backbones.resnet50_irn as RIRN
    orig = R50.resnet50
    R50.resnet50 = lambda pretrained=True, **kw: orig(pretrained=False, **kw)
    try:
        m = RIRN.AffinityDisplacementLoss(path_index)
    finally:
        R50.resnet50 = orig
    if sd_np is not None:
        missing, unexpected = m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd_np.items()}, strict=False)
        assert not unexpected and all(k.startswith("path_indices") or k == "disp_target" for k in missing), (missing, unexpected)
    m.train()
    return m


def affinity_labels(path_index, label):
    from src.data import GetAffinityLabelFromIndices
    f = GetAffinityLabelFromIndices(path_index.src_indices, path_index.dst_indices)
    out = [f(l) for l in label]
    return tuple(torch.stack([o[i] for o in out]) for i in range(3))


def combine(losses, labels):
    """The public IRN training loop's reduction of AffinityDisplacementLoss.forward(x, True)."""
    pos, neg, dp_fg, dp_bg = losses
    bg, fg, ng = (t.to(pos.dtype) for t in labels)
    sums = dict(bg_pos=torch.sum(bg * pos), fg_pos=torch.sum(fg * pos), neg=torch.sum(ng * neg),
                dp_fg=torch.sum(dp_fg * torch.unsqueeze(fg, 1)), dp_bg=torch.sum(dp_bg * torch.unsqueeze(bg, 1)),
                n_bg=torch.sum(bg), n_fg=torch.sum(fg), n_neg=torch.sum(ng))
    bg_pos_aff_loss = sums["bg_pos"] / (sums["n_bg"] + 1e-5)
    fg_pos_aff_loss = sums["fg_pos"] / (sums["n_fg"] + 1e-5)
    pos_aff_loss = bg_pos_aff_loss / 2 + fg_pos_aff_loss / 2
    neg_aff_loss = sums["neg"] / (sums["n_neg"] + 1e-5)
    dp_fg_loss = sums["dp_fg"] / (2 * sums["n_fg"] + 1e-5)
    dp_bg_loss = sums["dp_bg"] / (2 * sums["n_bg"] + 1e-5)
    total = (pos_aff_loss + neg_aff_loss) / 2 + (dp_fg_loss + dp_bg_loss) / 2
    return sums, (pos_aff_loss, neg_aff_loss, dp_fg_loss, dp_bg_loss, total)


SUMS = ("bg_pos", "fg_pos", "neg", "dp_fg", "dp_bg", "n_bg", "n_fg", "n_neg")


def head_only(model, path_index, edge_out, dp_out, label, dtype):
    e = torch.from_numpy(edge_out).to(dtype).requires_grad_(True)
    d = torch.from_numpy(dp_out).to(dtype).requires_grad_(True)
    model = model.to(dtype)
    aff = model.to_affinity(torch.sigmoid(e))
    pair = model.to_pair_displacement(d)
    losses = ((-1) * torch.log(aff + 1e-5), (-1) * torch.log(1. + 1e-5 - aff), model.to_displacement_loss(pair), torch.abs(pair))
    sums, terms = combine(losses, affinity_labels(path_index, label))
    terms[4].backward()
    return (np.array([float(sums[k]) for k in SUMS]), np.array([float(t) for t in terms]), e.grad.numpy(), d.grad.numpy())


def probe_index(name, numel):
    return np.minimum((synth.uniform(SEED, "probe:" + name, (N_PROBE,)) * numel).astype(np.int64), numel - 1)


def main():
    GG.load_reference()
    import src.indexing as RI
    import src.imutils as IM
    import src.torchutils as TU
    from src.data import TorchvisionNormalize
    torch.set_num_threads(8)
    out = {}

    # ---- case a: the whole step at crop 128 ---------------------------------------------------------------------------
    crop, N, radius = CASE_A["crop"], CASE_A["N"], CASE_A["radius"]
    pi = RI.PathIndex(radius=radius, default_size=(crop // 4, crop // 4))
    sd = synth.irn_state_dict(SEED)
    x = synth.irn_image_pair(crop, crop, SEED)
    lab = labels_a()
    out["a_params"] = np.array([crop, N, radius, SEED], np.int64)
    out["a_label"] = lab
    for nm, dt in (("f64", torch.float64), ("f32", torch.float32)):
        model = build_model(pi, sd).to(dt)
        if nm == "f64":
            ref_sd = model.state_dict()
            out["keys"] = np.array(list(ref_sd))
            out["shapes"] = np.array([",".join(str(d) for d in v.shape) for v in ref_sd.values()])
        taps = {}

        def tap(name):
            def hook(_m, _a, o):
                o.retain_grad()
                taps[name] = o
            return hook
        hooks = [model.fc_edge6.register_forward_hook(tap("edge")), model.fc_dp7.register_forward_hook(tap("dp"))]
        losses = model(torch.from_numpy(x).to(dt), True)
        sums, terms = combine(losses, affinity_labels(pi, lab))
        terms[4].backward()
        for h in hooks:
            h.remove()
        out[f"a_{nm}_sums"] = np.array([float(sums[k]) for k in SUMS])
        out[f"a_{nm}_terms"] = np.array([float(t) for t in terms])
        out[f"a_{nm}_edge_out"], out[f"a_{nm}_dp_out"] = taps["edge"].detach().numpy(), taps["dp"].detach().numpy()
        out[f"a_{nm}_dedge"], out[f"a_{nm}_ddp"] = taps["edge"].grad.numpy(), taps["dp"].grad.numpy()
        names, rows, probes = [], [], []
        for k, p in model.named_parameters():
            if not k.startswith("fc_"):
                assert p.grad is None, k                          # the backbone is detached (:110-114)
                continue
            g = p.grad.detach().double().numpy().ravel()
            names.append(k)
            rows.append([np.abs(g).max(), g.sum()])
            probes.append(g[probe_index(k, g.size)])
        out[f"a_{nm}_grad_names"] = np.array(names)
        out[f"a_{nm}_grad_summary"] = np.array(rows)
        out[f"a_{nm}_grad_probe"] = np.array(probes)
        s = out[f"a_{nm}_sums"]
        assert min(s[5:]) > 100, s                                   # all three pair classes present
        print("a", nm, "terms", out[f"a_{nm}_terms"], "counts", s[5:], "max|grad|", float(np.array(rows)[:, 0].min()), flush=True)
        assert float(np.array(rows)[:, 0].min()) > 0, "a trainable tensor has a zero gradient"

    # ---- case b: the loss head alone, 24 x 37, radius 5; b2 = its sample 2 alone (no fg pair: the + 1e-5 denominators) --------
    H, W, N, radius = CASE_B["H"], CASE_B["W"], CASE_B["N"], CASE_B["radius"]
    pib = RI.PathIndex(radius=radius, default_size=(H, W))
    modelb = build_model(pib)
    e = (synth.normal(SEED, "b_edge", (N, 1, H, W)) * 1.5).astype(np.float32)
    d = (synth.normal(SEED, "b_dp", (N, 2, H, W)) * 2.0).astype(np.float32)
    labb = labels_b()
    out["b_params"] = np.array([H, W, N, radius], np.int64)
    out["b_label"], out["b_edge_out"], out["b_dp_out"] = labb, e, d
    for tag, sl in (("b", slice(0, N)), ("b2", slice(2, 3))):
        for nm, dt in (("f64", torch.float64), ("f32", torch.float32)):
            s, t, ge, gd = head_only(modelb, pib, e[sl], d[sl], labb[sl], dt)
            out[f"{tag}_{nm}_sums"], out[f"{tag}_{nm}_terms"], out[f"{tag}_{nm}_dedge"], out[f"{tag}_{nm}_ddp"] = s, t, ge, gd
            print(tag, nm, "terms", t, "counts", s[5:], flush=True)
    assert out["b2_f64_sums"][6] == 0 and out["b2_f64_sums"][5] > 0 and out["b2_f64_sums"][7] > 0
    for n in range(N - 1):
        s = head_only(modelb, pib, e[n:n + 1], d[n:n + 1], labb[n:n + 1], torch.float64)[0]
        assert min(s[5:]) > 0, (n, s)

    # ---- PolyOptimizer: three steps on two groups --------------------------------------------------------------------
    ps = [torch.nn.Parameter(torch.from_numpy(synth.normal(SEED, f"opt_p{i}", (n,)).astype(np.float32))) for i, n in enumerate((7, 5))]
    grads = [[synth.normal(SEED, f"opt_g{st}_{i}", (n,)).astype(np.float32) for i, n in enumerate((7, 5))] for st in range(3)]
    opt = TU.PolyOptimizer([{"params": [ps[0]], "lr": 0.1}, {"params": [ps[1]], "lr": 1.0}], lr=0.1, weight_decay=1e-4, max_step=5)
    out["opt_momentum_wd"] = np.array([opt.param_groups[0]["momentum"], opt.param_groups[0]["weight_decay"]])
    steps = []
    for st in range(3):
        for p, g in zip(ps, grads[st]):
            p.grad = torch.from_numpy(g.copy())
        opt.step()
        steps.append(np.concatenate([p.detach().numpy().copy() for p in ps]))
    out["opt_steps"] = np.array(steps)
    out["opt_lrs"] = np.array([g["lr"] for g in opt.param_groups])

    # ---- the loader: VOC12AffinityDataset.__getitem__'s calls on an in-memory image --------------------------------------
    Hi, Wi, crop = LOADER["H"], LOADER["W"], LOADER["crop"]
    img = (synth.uniform(SEED, "ld_img", (Hi // 10, Wi // 10, 3)) * 255).astype(np.uint8).repeat(10, 0).repeat(10, 1)
    img = (img.astype(np.int32) + (synth.uniform(SEED, "ld_noise", (Hi, Wi, 3)) * 20).astype(np.int32)).clip(0, 255).astype(np.uint8)
    lbl = (synth.uniform(SEED, "ld_lab", (Hi // 15, Wi // 15)) * 6).astype(np.uint8).repeat(15, 0).repeat(15, 1)
    lbl[lbl == 5] = 255
    out["ld_params"] = np.array([Hi, Wi, crop], np.int64)
    out["ld_seeds"] = np.array(LOADER["seeds"], np.int64)
    for s in LOADER["seeds"]:
        random.seed(s)
        a, b = IM.random_scale((img, lbl), scale_range=(0.5, 1.5), order=(3, 0))
        a = TorchvisionNormalize()(a)
        a, b = IM.random_lr_flip((a, b))
        a, b = IM.random_crop((a, b), crop, (0, 255))
        a = IM.HWC_to_CHW(a)
        r = IM.pil_rescale(b, 0.25, 0)
        assert a.dtype == np.float32 and r.dtype == np.uint8, (a.dtype, r.dtype)
        out[f"ld_{s}_img_probe"] = a.ravel()[::97].copy()
        out[f"ld_{s}_img_sum"] = np.array([a.astype(np.float64).sum(), np.abs(a.astype(np.float64)).sum()])
        out[f"ld_{s}_label"] = r
    path = os.path.join(ROOT, "tests", "golden", "irn_train.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
