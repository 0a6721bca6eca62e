"""CPU side of the IRN network (no GPU): the plain-torch restatement tests/irn_net_ref.py against the reference's own
fixture tests/golden/irn_net.npz (made by tools/gen_irn_net_golden.py), the state-dict contract of
muscle_amd.EdgeDisplacement, the command line of `python -m muscle_amd.infer_irn` and the palette writer.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import irn_net_ref as R  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden", "irn_net.npz")
NAMES = ["x1", "x2", "x3", "x4", "x5", "edge_cat", "dp_cat1", "dp_cat2"]


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def test_fixture_inputs_are_not_degenerate(gold):
    """The generator's conditions on the reference's own output, re-read from the file: a saturated sigmoid or a dead
    displacement branch would make every comparison vacuous."""
    for tag in ("a", "b"):
        amax, p5, p95, s0, s1 = (float(v) for v in gold[f"{tag}_checks"])
        assert amax < 1e4 and p95 - p5 >= 0.2 and 0.02 < p5 and p95 < 0.98 and min(s0, s1) > 1e-3
        e = gold[f"{tag}_edge"]
        q5, q95 = np.percentile(e, [5, 95])
        assert abs(q5 - p5) < 1e-6 and abs(q95 - p95) < 1e-6
    assert int((gold["e2e_label_share"] > 0.02).sum()) >= 3


@pytest.mark.parametrize("tag", ["a", "b"])
def test_restatement_fp32_matches_reference_fixture(gold, tag):
    """The restatement in fp32 against the reference's output, every stored tensor.  The two are near-identical op
    sequences on the same library; measured where the fixture was made: max|diff| / max|ref| = 0.0 for edge, dp and all
    eight summaries, in both cases (the same ATen kernels in the same order).  Asserted: 4 x the measured value, i.e.
    equality."""
    from muscle_amd import synth
    crop, H, W, seed = (int(v) for v in gold[f"{tag}_params"])
    sd = R.to_dtype(synth.irn_state_dict(seed), torch.float32)
    x = torch.from_numpy(synth.irn_image_pair(H, W, seed))
    with torch.no_grad():
        edge, dp, named = R.edge_displacement(sd, x, crop, want_named=True)
    measured = 0.0
    for k, got in (("edge", edge), ("dp", dp)):
        ref = gold[f"{tag}_{k}"]
        assert tuple(got.shape) == ref.shape
        e = float(np.abs(got.numpy() - ref).max()) / float(np.abs(ref).max())
        print(f"[irn_net cpu] {tag} {k}: {e:.3e}")
        assert e <= 4 * measured, (k, e)
    named = dict(named)
    for i, k in enumerate(NAMES):
        a = named[k].double().numpy().ravel()
        mine = np.array([np.sqrt((a * a).sum()), (a * synth.normal(123, k, a.shape)).sum()])
        e = np.abs(mine - gold[f"{tag}_summary"][i]) / np.abs(gold[f"{tag}_summary"][i]).max()
        print(f"[irn_net cpu] {tag} {k}: summary {e}")
        assert (e <= 4 * measured).all(), (k, e)


def test_end_to_end_restatement_and_label_margin(gold):
    """infer_irn.py:64-92 restated, fp32 against the fixture, and the condition on the end-to-end inputs: the fp32
    restatement's label map differs from the fp64 restatement's on at most HALF the cap the GPU test allows (2e-3), so the
    GPU test cannot pass by being handed an easy image."""
    from muscle_amd import synth
    crop, H, W, seed = (int(v) for v in gold["a_params"])
    beta, times = (int(v) for v in gold["e2e_params"])
    bg = float(gold["e2e_bg_thres"])
    sd, x, cam = synth.irn_state_dict(seed), synth.irn_image_pair(H, W, seed), synth.irn_cam_dict(H, W, seed)
    with torch.no_grad():
        lab32, soft32, _ = R.infer_irn(R.to_dtype(sd, torch.float32), torch.from_numpy(x), cam, beta, times, bg, crop)
        lab64, soft64, _ = R.infer_irn(R.to_dtype(sd, torch.float64), torch.from_numpy(x).double(), cam, beta, times, bg, crop)
    d_fix = float((lab32 != gold["e2e_label"]).mean())
    s_fix = float(np.abs(soft32.astype(np.float32) - gold["e2e_soft"].astype(np.float32)).max())
    d_64 = float((lab32 != lab64).mean())
    s_64 = float(np.abs(soft32.astype(np.float32) - soft64.astype(np.float32)).max())
    print(f"[irn_net cpu] e2e fp32 vs fixture: labels {d_fix:.3e} soft {s_fix:.3e}; fp32 vs fp64: labels {d_64:.3e} soft {s_64:.3e}")
    assert d_fix <= 2e-3 and s_fix <= 1e-3
    assert d_64 <= 1e-3, d_64
    assert s_64 <= 1e-3
    assert len(set(np.unique(lab64).tolist())) >= 3


def test_state_dict_contract(gold):
    import muscle_amd
    from muscle_amd import synth
    m = muscle_amd.EdgeDisplacement()
    sd = m.state_dict()
    want = {k: tuple(int(d) for d in s.split(",")) if s else () for k, s in zip(gold["keys"].tolist(), gold["shapes"].tolist())}
    assert set(sd) == set(want)
    assert all(tuple(sd[k].shape) == want[k] for k in want)
    assert {k: tuple(v) for k, v in synth.irn_state_dict_spec().items()} == want
    new = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.irn_state_dict(3).items()}
    assert any("num_batches_tracked" in k for k in new)
    res = m.load_state_dict(new, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    after = m.state_dict()
    for key in synth.irn_canonical_spec():
        for alias in synth.irn_aliases(key):
            assert torch.equal(after[key], after[alias]) and torch.equal(after[key], new[key]), (key, alias)
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in new.items() if k != "backbone.1.0.0.conv2.weight"}, strict=True)
    assert m.crop_size == 512 and m.stride == 4 and not m.training


def test_cli_arguments():
    from muscle_amd import infer_irn as cli
    a = cli.parse_args(["--irn_weights_name", "w.pth", "--cam_dir", "cams"])
    assert (a.beta, a.exp_times, a.sem_seg_bg_thres, a.sem_seg_out_dir, a.voc12_root, a.infer_list, a.soft_output) == \
        (8, 6, 0.35, "./irn_rw", "data/VOC2012", "data/train.txt", 0)
    a = cli.parse_args(["--irn_weights_name", "w.pth", "--cam_dir", "c", "--beta", "10", "--exp_times", "8", "--sem_seg_bg_thres",
                        "0.25", "--soft_output", "1", "--irn_network", "some.module", "--sem_seg_out_dir", "o", "--infer_list", "l",
                        "--voc12_root", "v"])
    assert (a.beta, a.exp_times, a.sem_seg_bg_thres, a.soft_output, a.irn_network) == (10, 8, 0.25, 1, "some.module")
    with pytest.raises(SystemExit):
        cli.parse_args(["--irn_weights_name", "w.pth"])              # --cam_dir is required, as in the reference


def test_palette_png_round_trip(tmp_path):
    import PIL.Image
    from muscle_amd.irn import save_palette_png, voc_color_map
    lab = (np.arange(37 * 53).reshape(37, 53) % 21).astype(np.uint8)
    p = str(tmp_path / "x.png")
    save_palette_png(p, torch.from_numpy(lab))
    im = PIL.Image.open(p)
    assert im.mode == "P"
    assert np.array_equal(np.array(im), lab)
    cmap = voc_color_map()
    assert cmap[0].tolist() == [0, 0, 0] and cmap[1].tolist() == [128, 0, 0] and cmap[15].tolist() == [192, 128, 128]
    assert np.array_equal(np.array(im.convert("RGB")), cmap[lab])
    with pytest.raises(ValueError):
        save_palette_png(p, lab.astype(np.int64))
