"""GPU parity of training the IRN heads (muscle_amd/irn.py AffinityDisplacementLoss / irn_step, csrc/irn_train.hip).

Yardstick: the fp64 restatement tests/irn_train_ref.py on the CPU (which tests/test_cpu_irn_train.py ties to the reference's own
run).  err(t) = max|t - t64| / max|t64|; e32 is that error for the fp32 restatement, eHIP for the HIP path.  Required per tensor:
eHIP <= 2 e32 + 2e-7, in exact-fp32 and in split arithmetic - the bound of tests/test_gpu_irn_net.py.  Every figure is printed
before it is asserted.
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import irn_net_ref as R  # noqa: E402
import irn_train_ref as T  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(__file__), "golden", "irn_train.npz")


def err(t, t64):
    t = t.detach().cpu().double() if torch.is_tensor(t) else torch.as_tensor(np.asarray(t, np.float64))
    t64 = t64.detach().double() if torch.is_tensor(t64) else torch.as_tensor(np.asarray(t64, np.float64))
    return float((t.reshape(t64.shape) - t64).abs().max()) / max(float(t64.abs().max()), 1e-30)


def check(name, hip, t32, t64):
    e_hip, e32 = err(hip, t64), err(t32, t64)
    print(f"[irn_train] {name}: eHIP {e_hip:.3e}  e32 {e32:.3e}  bound {2 * e32 + 2e-7:.3e}")
    assert e_hip <= 2 * e32 + 2e-7, (name, e_hip, e32)


def nhwc4(t):
    """[N,C,H,W] (C <= 4) -> the 4-column GEMM output [N,H,W,4] the kernels read with a leading dimension."""
    N, C, H, W = t.shape
    out = torch.full((N, H, W, 4), 3.5, dtype=torch.float32)
    out[..., :C] = t.permute(0, 2, 3, 1)
    return out.to(DEV)


@pytest.fixture(scope="module")
def z():
    return np.load(GOLD)


def head_case(z, tag):
    if tag == "a":
        radius = int(z["a_params"][2])
        return z["a_f32_edge_out"], z["a_f32_dp_out"], z["a_label"], radius
    H, W, N, radius = (int(v) for v in z["b_params"])
    sl = slice(0, N) if tag == "b" else slice(2, 3)
    return z["b_edge_out"][sl], z["b_dp_out"][sl], z["b_label"][sl], radius


def hip_loss_head(e, d, label, radius):
    from muscle_amd import indexing, ops
    N, _, H, W = e.shape
    table = indexing.PathIndex(radius, (H, W)).offsets_table(DEV)
    E, D = nhwc4(torch.from_numpy(e)), nhwc4(torch.from_numpy(d))
    lab = torch.from_numpy(np.ascontiguousarray(label)).to(DEV)
    res, amax = ops.irn_loss_fwd(E, D, lab, table, radius)
    dE, dD = ops.irn_loss_bwd(E, D, lab, table, radius, amax, res)
    assert amax.dtype == torch.uint8 and tuple(amax.shape) == (N, table[3], (H - radius + 1) * (W - 2 * radius + 2))
    assert bool((dE[:, 1:] == 0).all()) and bool((dD[:, 2:] == 0).all())
    return res, dE[:, 0].view(N, 1, H, W), dD[:, :2].view(N, H, W, 2).permute(0, 3, 1, 2)


# ---- 1. the loss head alone ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["a", "b", "b2"])
def test_loss_head_vs_fp64(z, tag):
    e, d, label, radius = head_case(z, tag)
    res, dE, dD = hip_loss_head(e, d, label, radius)
    t64, s64, ge64, gd64 = T.loss_head_grads(e, d, label, radius, torch.float64)
    t32, _s32, ge32, gd32 = T.loss_head_grads(e, d, label, radius, torch.float32)
    res = res.cpu()
    assert [float(v) for v in res[5:8]] == [float(s64[k]) for k in ("n_bg", "n_fg", "n_neg")]      # counts are exact integers
    for i, k in enumerate(T.TERMS):
        check(f"head {tag} {k}", res[i], t32[k], t64[k])
    check(f"head {tag} dedge", dE, ge32, ge64)
    check(f"head {tag} ddp", dD, gd32, gd64)
    if tag != "a":                                                      # the reference's own figures (fp64 run of its classes)
        assert err(res[:5], z[f"{tag}_f64_terms"]) <= 2 * err(z[f"{tag}_f32_terms"], z[f"{tag}_f64_terms"]) + 2e-7


# ---- 2. nothing to learn from: all labels 255 ---------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["a", "b"])
def test_loss_head_all_ignore_is_exactly_zero(z, tag):
    e, d, label, radius = head_case(z, tag)
    res, dE, dD = hip_loss_head(e, d, np.full_like(label, 255), radius)
    assert float(res[4]) == 0.0 and bool((res[:8] == 0).all())
    assert bool((dE == 0).all()) and bool((dD == 0).all())


# ---- 3. GroupNorm -> up-sample -> crop -> ReLU, backward ------------------------------------------------------------------
@pytest.mark.parametrize("scale,crop", [(1, (7, 6)), (2, (15, 13)), (4, (29, 27)), (2, (16, 16)), (4, (32, 32))])
def test_gn_resize_backward_vs_autograd(scale, crop):
    from muscle_amd import ops, synth
    N, Hs, Ws, C, G, ldd, coff = 2, 8, 8, 32, 4, 72, 24
    Hd, Wd = crop
    rnd = lambda nm, shape: torch.from_numpy(synth.normal(17, f"{nm}{scale}{crop}", shape))
    x = rnd("x", (N, C, Hs, Ws)) * 2 + 0.7
    ga, be = rnd("g", (C,)) * 0.3 + 1, rnd("b", (C,)) * 0.2
    gy = rnd("gy", (N, C, Hd, Wd))

    def ref(dt):
        xx, g, b = (t.to(dt).requires_grad_(True) for t in (x, ga, be))
        o = F.group_norm(xx, G, g, b, 1e-5)
        if scale > 1:
            o = F.interpolate(o, scale_factor=scale, mode="bilinear", align_corners=False)
        y = F.relu(o[..., :Hd, :Wd])
        return torch.autograd.grad((y * gy.to(dt)).sum(), (xx, g, b))
    r64, r32 = ref(torch.float64), ref(torch.float32)
    xd = x.float().permute(0, 2, 3, 1).contiguous().to(DEV)
    gamma = ga.float().to(DEV)
    stat = ops.gn_stats(xd, G)
    dst = torch.zeros(N, Hd, Wd, ldd, dtype=torch.float32, device=DEV)
    ops.gn_resize(xd, stat, gamma, be.float().to(DEV), dst, coff, scale)
    gdst = torch.full((N, Hd, Wd, ldd), 9.0, dtype=torch.float32, device=DEV)                 # other slices must not leak in
    gdst[..., coff:coff + C] = gy.float().permute(0, 2, 3, 1).to(DEV)
    dY = ops.gn_resize_bwd(gdst, dst, coff, C, Hs, Ws, scale)
    dX, dgamma, dbeta = ops.gn_bwd(dY, xd, stat, gamma)
    check(f"gn bwd x{scale} {crop} dX", dX.permute(0, 3, 1, 2), r32[0], r64[0])
    check(f"gn bwd x{scale} {crop} dgamma", dgamma, r32[1], r64[1])
    check(f"gn bwd x{scale} {crop} dbeta", dbeta, r32[2], r64[2])


# ---- 4. the whole step -----------------------------------------------------------------------------------------------------
LRS = (0.1, 1.0)


@pytest.fixture(scope="module")
def step_refs(z):
    from muscle_amd import synth
    crop, N, radius, seed = (int(v) for v in z["a_params"])
    sd, x = synth.irn_state_dict(seed), synth.irn_image_pair(crop, crop, seed)
    out = {"sd": sd, "x": x, "crop": crop, "radius": radius, "label": z["a_label"]}
    for nm, dt in (("f32", torch.float32), ("f64", torch.float64)):
        terms, grads, ge, gd = T.step(sd, x, z["a_label"], radius, dt)
        edge_keys, dp_keys = T.trainable_keys()
        after = {}
        for keys, lr in ((edge_keys, LRS[0]), (dp_keys, LRS[1])):                 # first PolyOptimizer step: p - lr * grad
            for k in keys:
                after[k] = torch.as_tensor(np.asarray(sd[k])).to(dt) - lr * grads[k]
        out[nm] = dict(terms=terms, grads=grads, after=after)
    return out


def build(r):
    import muscle_amd
    from muscle_amd import indexing
    f = r["crop"] // 4
    m = muscle_amd.AffinityDisplacementLoss(indexing.PathIndex(r["radius"], (f, f)), crop_size=r["crop"])
    missing, unexpected = m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in r["sd"].items()}, strict=False)
    assert not unexpected and all(k.startswith("path_indices") or k == "disp_target" for k in missing)
    return m.to(DEV).train()


def run_step(r, m, with_opt=True):
    import muscle_amd
    edge, dp = m.trainable_parameters()
    opt = muscle_amd.PolyOptimizer([{"params": edge, "lr": LRS[0]}, {"params": dp, "lr": LRS[1]}], lr=0.1, weight_decay=1e-4, max_step=10)
    batch = {"img": torch.from_numpy(r["x"]).to(DEV), "label": torch.from_numpy(r["label"]).to(DEV)}
    out = muscle_amd.irn_step(m, opt, batch) if with_opt else m.loss_backward(batch["img"], batch["label"])
    return out


@pytest.mark.both_arith
def test_irn_step_vs_fp64(step_refs):
    r = step_refs
    m = build(r)
    out = run_step(r, m)
    named = dict(m.named_parameters())
    for k, name in zip(("pos_aff_loss", "neg_aff_loss", "dp_fg_loss", "dp_bg_loss", "loss"), T.TERMS):
        assert out[k].is_cuda
        check(f"step {name}", out[k], r["f32"]["terms"][name], r["f64"]["terms"][name])
    keys = [k for grp in T.trainable_keys() for k in grp]
    assert all(p.grad is None for k, p in named.items() if not k.startswith("fc_"))
    for k in keys:
        check(f"step grad {k}", named[k].grad, r["f32"]["grads"][k], r["f64"]["grads"][k])
    for k in keys:
        check(f"step param {k}", named[k], r["f32"]["after"][k], r["f64"]["after"][k])


# ---- 5. the same bits every step -----------------------------------------------------------------------------------------
def test_two_identical_steps_give_bit_equal_gradients(step_refs):
    r = step_refs
    got = []
    for _ in range(2):
        m = build(r)
        res = run_step(r, m, with_opt=False)
        got.append((res.clone(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}))
    assert torch.equal(got[0][0], got[1][0]) and len(got[0][1]) == 39
    for k in got[0][1]:
        assert torch.equal(got[0][1][k], got[1][1][k]), k
    m = build(r)                                                        # and twice on one model: the folded backbone is kept
    run_step(r, m, with_opt=False)
    prep = m._prep
    g1 = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    m.eval()
    m.train()
    run_step(r, m, with_opt=False)
    assert m._prep is prep
    for k, p in m.named_parameters():
        if p.grad is not None:
            assert torch.equal(g1[k], p.grad), k


# ---- 6. a saved checkpoint runs through infer_irn --------------------------------------------------------------------------
def test_trained_checkpoint_runs_through_infer_irn(step_refs, tmp_path):
    import muscle_amd
    from muscle_amd import synth
    from muscle_amd.irn import infer_irn
    r = step_refs
    m = build(r)
    run_step(r, m)
    m.eval()
    edge, dp = m(torch.from_numpy(r["x"]).to(DEV))
    m.mean_shift.running_mean = dp.mean(dim=(0, 2, 3))
    path = str(tmp_path / "irn_trained.pth")
    torch.save(m.state_dict(), path)
    net = muscle_amd.EdgeDisplacement(crop_size=r["crop"])
    net.load_state_dict(torch.load(path, map_location="cpu"), strict=False)                     # infer_irn.py:41
    net = net.to(DEV).eval()
    H, W = 93, 125
    pair = torch.from_numpy(synth.irn_image_pair(H, W, 1)).to(DEV)
    label = infer_irn(net, pair, synth.irn_cam_dict(H, W, 1))
    assert label.dtype == torch.uint8 and tuple(label.shape) == (H, W) and int(label.max()) <= 20
    # the heads the checkpoint carries are the trained ones: the inference network's edge logits equal the training model's
    e2, d2 = m(F.pad(pair, [0, r["crop"] - W, 0, r["crop"] - H]))
    e_inf, d_inf = net(pair)
    fh, fw = e_inf.shape[1:]
    want = torch.sigmoid(e2[0, 0, :fh, :fw] / 2 + e2[1, 0, :fh, :fw].flip(-1) / 2)
    assert float((e_inf[0] - want).abs().max()) <= 1e-5
    # features() of the training model reads the live (trained) heads, not the snapshot prepare() took before the step
    x128 = torch.from_numpy(r["x"]).to(DEV)
    for a, b in zip(m.features(x128)[1:], net.features(x128)[1:]):
        assert torch.equal(a, b)
    assert float((d_inf - d2[0, :, :fh, :fw]).abs().max()) <= 1e-4 * max(1.0, float(d2.abs().max()))
