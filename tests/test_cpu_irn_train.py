"""CPU side of training the IRN heads: the plain-torch restatement (tests/irn_train_ref.py) against the reference's own run
(tests/golden/irn_train.npz, tools/gen_irn_train_golden.py), PolyOptimizer, the state_dict key set and the loader restatement."""
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import irn_train_ref as T  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden", "irn_train.npz")
SUMS = ("bg_pos", "fg_pos", "neg", "dp_fg", "dp_bg", "n_bg", "n_fg", "n_neg")


@pytest.fixture(scope="module")
def z():
    return np.load(GOLD)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max()) / max(float(np.abs(b).max()), 1e-30)


@pytest.mark.parametrize("tag", ["b", "b2"])
def test_loss_head_restatement_reproduces_the_reference_fp64(z, tag):
    H, W, N, radius = (int(v) for v in z["b_params"])
    sl = slice(0, N) if tag == "b" else slice(2, 3)
    terms, sums, ge, gd = T.loss_head_grads(z["b_edge_out"][sl], z["b_dp_out"][sl], z["b_label"][sl], radius, torch.float64)
    assert np.array_equal([float(sums[k]) for k in SUMS[5:]], z[f"{tag}_f64_sums"][5:])          # counts are exact
    assert rel([float(sums[k]) for k in SUMS[:5]], z[f"{tag}_f64_sums"][:5]) < 1e-12
    assert rel([float(terms[k]) for k in T.TERMS], z[f"{tag}_f64_terms"]) < 1e-12
    assert rel(ge.numpy(), z[f"{tag}_f64_dedge"]) < 1e-11 and rel(gd.numpy(), z[f"{tag}_f64_ddp"]) < 1e-11
    if tag == "b2":
        assert float(sums["n_fg"]) == 0 and float(terms["dp_fg"]) == 0                          # the + 1e-5 denominators


def test_whole_step_restatement_reproduces_the_reference_fp64(z):
    from muscle_amd import synth
    crop, N, radius, seed = (int(v) for v in z["a_params"])
    torch.set_num_threads(8)
    terms, grads, ge, gd = T.step(synth.irn_state_dict(seed), synth.irn_image_pair(crop, crop, seed), z["a_label"], radius, torch.float64)
    assert rel([float(terms[k]) for k in T.TERMS], z["a_f64_terms"]) < 1e-10
    assert rel(ge.numpy(), z["a_f64_dedge"]) < 1e-9 and rel(gd.numpy(), z["a_f64_ddp"]) < 1e-9
    names = [str(k) for k in z["a_f64_grad_names"]]
    assert set(names) == {k for grp in T.trainable_keys() for k in grp}
    for i, k in enumerate(names):
        g = grads[k].numpy().ravel()
        idx = np.minimum((synth.uniform(seed, "probe:" + k, (64,)) * g.size).astype(np.int64), g.size - 1)
        scale = z["a_f64_grad_summary"][i, 0]
        assert abs(np.abs(g).max() - scale) <= 1e-9 * scale, k
        assert abs(g.sum() - z["a_f64_grad_summary"][i, 1]) <= 1e-9 * scale * g.size, k
        assert np.abs(g[idx] - z["a_f64_grad_probe"][i]).max() <= 1e-9 * scale, k


def test_poly_optimizer_matches_the_reference_steps(z):
    from muscle_amd import synth
    from muscle_amd.optim import PolyOptimizer
    seed = int(z["a_params"][3])
    ps = [torch.nn.Parameter(torch.from_numpy(synth.normal(seed, f"opt_p{i}", (n,)).astype(np.float32))) for i, n in enumerate((7, 5))]
    p0 = [[p.detach().clone()] for p in ps]
    grads = [[torch.from_numpy(synth.normal(seed, f"opt_g{st}_{i}", (n,)).astype(np.float32)) for i, n in enumerate((7, 5))] for st in range(3)]
    opt = PolyOptimizer([{"params": [ps[0]], "lr": 0.1}, {"params": [ps[1]], "lr": 1.0}], lr=0.1, weight_decay=1e-4, max_step=5)
    # the quirk: the value named weight_decay is SGD's momentum, the weight decay is zero
    assert [opt.param_groups[0]["momentum"], opt.param_groups[0]["weight_decay"]] == list(z["opt_momentum_wd"]) == [1e-4, 0]
    written = T.poly_sgd(p0, [[[g] for g in gs] for gs in grads], [0.1, 1.0], 1e-4, 5)
    for st in range(3):
        for p, g in zip(ps, grads[st]):
            p.grad = g.clone()
        opt.step()
        got = np.concatenate([p.detach().numpy() for p in ps])
        assert np.array_equal(got, z["opt_steps"][st]), st
        mine = np.concatenate([grp[0].numpy() for grp in written[st]])
        assert np.abs(mine - z["opt_steps"][st]).max() <= 2e-7 * np.abs(z["opt_steps"][st]).max()
    assert np.allclose([g["lr"] for g in opt.param_groups], z["opt_lrs"], rtol=0, atol=0) and opt.global_step == 3


def test_state_dict_keys_and_checkpoint_loads_into_edge_displacement(z, tmp_path):
    import muscle_amd
    from muscle_amd import indexing
    crop, _N, radius, _seed = (int(v) for v in z["a_params"])
    m = muscle_amd.AffinityDisplacementLoss(indexing.PathIndex(radius, (crop // 4, crop // 4)), crop_size=crop)
    sd = m.state_dict()
    assert list(sd) == [str(k) for k in z["keys"]]
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == [str(s) for s in z["shapes"]]
    assert m.training and not any(s.training for s in m.backbone)
    m.eval()
    m.train()
    assert not any(s.training for s in m.backbone)
    edge, dp = m.trainable_parameters()
    assert len(edge) == 17 and len(dp) == 22 and all(p.requires_grad for p in edge + dp)
    path = str(tmp_path / "irn.pth")
    torch.save(sd, path)
    net = muscle_amd.EdgeDisplacement(crop_size=crop)
    missing, unexpected = net.load_state_dict(torch.load(path, map_location="cpu"), strict=False)       # infer_irn.py:41
    assert not missing and all(k.startswith("path_indices") or k == "disp_target" for k in unexpected)
    assert torch.equal(net.fc_dp7[3].weight, m.fc_dp7[3].weight)


@pytest.mark.parametrize("radius,size", [(10, (32, 32)), (5, (24, 37)), (3, (9, 14))])
def test_path_index_offsets_and_flat_indices_agree(radius, size):
    from muscle_amd import indexing
    pi = indexing.PathIndex(radius, size)
    groups, dst = T.search_paths(radius)
    assert np.array_equal(pi.search_dst, dst) and all(np.array_equal(a, b) for a, b in zip(pi.search_paths, groups))
    H, W = size
    rf = radius - 1
    full = np.arange(H * W).reshape(H, W)
    for grp, ind in zip(groups, pi.path_indices):
        for p, row in zip(grp, ind):
            for (dy, dx), flat in zip(p, row):
                assert np.array_equal(flat, full[dy:dy + H - rf, rf + dx:rf + dx + W - 2 * rf].reshape(-1))
    assert np.array_equal(pi.dst_indices, np.concatenate([i[:, 0] for i in pi.path_indices]))


def test_loader_restatement_equals_the_reference_samples(z):
    from muscle_amd import synth
    from muscle_amd.train_irn import affinity_sample
    seed = int(z["a_params"][3])
    Hi, Wi, crop = (int(v) for v in z["ld_params"])
    img = (synth.uniform(seed, "ld_img", (Hi // 10, Wi // 10, 3)) * 255).astype(np.uint8).repeat(10, 0).repeat(10, 1)
    img = (img.astype(np.int32) + (synth.uniform(seed, "ld_noise", (Hi, Wi, 3)) * 20).astype(np.int32)).clip(0, 255).astype(np.uint8)
    lbl = (synth.uniform(seed, "ld_lab", (Hi // 15, Wi // 15)) * 6).astype(np.uint8).repeat(15, 0).repeat(15, 1)
    lbl[lbl == 5] = 255
    for s in z["ld_seeds"]:
        a, r = affinity_sample(img, lbl, crop, random.Random(int(s)))
        assert a.dtype == np.float32 and a.shape == (3, crop, crop) and r.dtype == np.uint8 and r.shape == (crop // 4, crop // 4)
        assert np.array_equal(r, z[f"ld_{s}_label"]), s
        assert np.array_equal(a.ravel()[::97], z[f"ld_{s}_img_probe"]), s
        assert np.allclose([a.astype(np.float64).sum(), np.abs(a.astype(np.float64)).sum()], z[f"ld_{s}_img_sum"], rtol=1e-12), s
