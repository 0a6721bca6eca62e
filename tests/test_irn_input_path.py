"""Device input path of IRN training (muscle_amd.irndata: nearest_table / plan_irn_item / IrnStager / IrnLoader, csrc/irndata.hip)
and `python -m muscle_amd.train_irn --loader device`, against the host loader of muscle_amd.train_irn (affinity_sample,
top_left_sample - themselves tied to the reference's recorded samples in tests/golden/irn_train.npz) and against PIL.

Every comparison is bit for bit.  The CPU tests check the planner through tests/irn_input_ref.py, the numpy statement of what the
two kernels compute from a plan; the GPU tests check the kernels against the same host functions.  Shapes: a stager has one
crop size, so the case list is staged as one mixed batch per crop size (64: three shapes, 128: one), and one item at a time."""
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import irn_input_ref as R  # noqa: E402

DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(__file__), "golden", "irn_train.npz")
SEEDS = range(8)
# (image size, crop, rescale range): both axes padded / both cropped with an odd width / the identity rescale / width cropped
# or padded by the seed under a padded height
CASES = [((40, 50), 64, (0.5, 1.5)), ((97, 203), 64, (0.5, 1.5)), ((64, 64), 64, (1.0, 1.0)), ((61, 130), 128, (0.5, 1.5))]


def _sources(case_no):
    (h, w), _, _ = CASES[case_no]
    return R.synth_image(h, w, case_no), R.synth_label(h, w, case_no)


@pytest.fixture(scope="module")
def samples():
    """[(case, seed, crop, plan, host image, host label)] over CASES x SEEDS: the host loader's output computed once."""
    from muscle_amd.irndata import plan_irn_item
    from muscle_amd.train_irn import affinity_sample
    out = []
    for c, (_, crop, rescale) in enumerate(CASES):
        img, lab = _sources(c)
        assert set(np.unique(lab).tolist()) == {0, 1, 2, 3, 4, 5, 255}
        for s in SEEDS:
            a, r = affinity_sample(img, lab, crop, random.Random(s), rescale)
            out.append((c, s, crop, plan_irn_item(img, lab, crop, random.Random(s), rescale), a, r))
    return out


def _fixture_items(z):
    from muscle_amd import synth
    seed = int(z["a_params"][3])
    Hi, Wi, crop = (int(v) for v in z["ld_params"])
    img = (synth.uniform(seed, "ld_img", (Hi // 10, Wi // 10, 3)) * 255).astype(np.uint8).repeat(10, 0).repeat(10, 1)
    img = (img.astype(np.int32) + (synth.uniform(seed, "ld_noise", (Hi, Wi, 3)) * 20).astype(np.int32)).clip(0, 255).astype(np.uint8)
    lbl = (synth.uniform(seed, "ld_lab", (Hi // 15, Wi // 15)) * 6).astype(np.uint8).repeat(15, 0).repeat(15, 1)
    lbl[lbl == 5] = 255
    return img, lbl, crop, [int(s) for s in z["ld_seeds"]]


def _assert_fixture(z, s, a, r):
    assert np.array_equal(r, z[f"ld_{s}_label"]), s
    assert np.array_equal(a.ravel()[::97], z[f"ld_{s}_img_probe"]), s
    assert np.allclose([a.astype(np.float64).sum(), np.abs(a.astype(np.float64)).sum()], z[f"ld_{s}_img_sum"], rtol=1e-12), s


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_nearest_table_equals_pil():
    """Per axis, against PIL.Image.resize(NEAREST) of a ramp image whose pixel value is its own index (mode I: 32-bit)."""
    import PIL.Image
    from muscle_amd.irndata import nearest_table
    g = np.random.default_rng(5)
    pairs = [(n, 0.25) for n in (4, 6, 7, 64, 128, 375, 500, 512, 600)] + [(1, 1.0), (1, 1.4), (2, 0.5), (600, 1.5), (600, 0.5)]
    pairs += [(int(g.integers(1, 601)), 0.25 if i % 5 == 0 else float(g.uniform(0.5, 1.5))) for i in range(240)]
    closed_form_wrong = 0
    for n_in, s in pairs:
        n_out = int(np.round(n_in * s))
        if n_out < 1:
            continue
        t = nearest_table(n_in, n_out)
        assert t.dtype == np.int32 and t.shape == (n_out,) and t.min() >= 0 and t.max() < n_in
        ramp = np.arange(n_in, dtype=np.int32)
        wide = PIL.Image.fromarray(np.ascontiguousarray(np.broadcast_to(ramp[None, :], (3, n_in))))
        tall = PIL.Image.fromarray(np.ascontiguousarray(np.broadcast_to(ramp[:, None], (n_in, 3))))
        assert np.array_equal(np.asarray(wide.resize((n_out, 3), PIL.Image.NEAREST))[1], t), (n_in, n_out)
        assert np.array_equal(np.asarray(tall.resize((3, n_out), PIL.Image.NEAREST))[:, 1], t), (n_in, n_out)
        closed_form_wrong += not np.array_equal(np.floor((np.arange(n_out) + 0.5) * (n_in / n_out)).astype(np.int32), t)
    assert len(pairs) >= 200
    print(f"closed form differs from Pillow for {closed_form_wrong} of {len(pairs)} sizes")


@pytest.mark.parametrize("crop", [32, 160])                 # always smaller / always larger than the rescaled 75 x 100 image
def test_planner_follows_the_host_loader_draw_order(crop, monkeypatch):
    from muscle_amd import train_irn
    from muscle_amd.irndata import plan_irn_item
    img, lab = R.synth_image(75, 100, 3), R.synth_label(75, 100, 3)
    boxes = []
    real = train_irn.random_crop_box
    monkeypatch.setattr(train_irn, "random_crop_box", lambda *a: boxes.append(real(*a)) or boxes[-1])
    for s in range(8):
        g_host, g_plan = R.Rec(s), R.Rec(s)
        train_irn.affinity_sample(img, lab, crop, g_host)
        p = plan_irn_item(img, lab, crop, g_plan)
        assert g_plan.log == g_host.log and [e[0] for e in g_plan.log] == ["random", "getrandbits", "randrange", "randrange"]
        assert g_plan.r.random() == g_host.r.random()
        assert p.scale == 0.5 + g_host.log[0][1] and p.flip == bool(g_host.log[1][2]) and tuple(p.box) == tuple(boxes[-1])
        assert p.size == (int(np.round(75 * p.scale)), int(np.round(100 * p.scale)))
    assert len(boxes) == 8                                   # the planner's own box is not the patched one


def test_case_list_reaches_every_edge(samples):
    """The cases do what they are there for: both flips per shape, padded and cropped axes, odd widths, the identity."""
    for c in range(len(CASES)):
        assert {p.flip for cc, _, _, p, _, _ in samples if cc == c} == {False, True}, c
    plans = lambda c: [p for cc, _, _, p, _, _ in samples if cc == c]
    S = 64
    assert any(p.place[0] > 0 and p.place[1] > 0 and p.window[2] < S and p.window[3] < S for p in plans(0))
    assert any(p.place[1] % 4 and p.window[3] % 4 for p in plans(0))                       # quads straddle both window edges
    assert any(p.size[1] % 2 and p.window[2] == S and p.window[3] == S and p.window[0] > 0 and p.window[1] > 0 for p in plans(1))
    assert all(p.resize_to is None and p.tables is None and p.size == (64, 64) for p in plans(2))
    assert all(p.resize_to is not None for c in (0, 1, 3) for p in plans(c))
    assert any(p.window[3] == 128 for p in plans(3)) and any(p.window[3] < 128 for p in plans(3))
    assert all(p.window[2] < 128 for p in plans(3))


def test_emulated_plan_equals_the_host_loader(samples):
    for c, s, crop, p, a, r in samples:
        img, lab = R.emulate(p, crop)
        assert img.dtype == np.float32 and lab.dtype == np.uint8
        assert np.array_equal(img, a), (c, s)
        assert np.array_equal(lab, r), (c, s)


def test_emulated_plan_equals_the_reference_samples():
    from muscle_amd.irndata import plan_irn_item
    z = np.load(GOLD)
    img, lbl, crop, seeds = _fixture_items(z)
    for s in seeds:
        a, r = R.emulate(plan_irn_item(img, lbl, crop, random.Random(s)), crop)
        _assert_fixture(z, s, a, r)


@pytest.mark.parametrize("size", [(40, 50), (97, 203), (64, 80), (80, 33)])      # smaller, larger, one axis each way
def test_emulated_eval_plan_equals_top_left_sample(size):
    from muscle_amd.irndata import plan_irn_eval_item
    from muscle_amd.train_irn import top_left_sample
    img = R.synth_image(*size, 9)
    got, lab = R.emulate(plan_irn_eval_item(img, 64), 64)
    assert lab is None and np.array_equal(got, top_left_sample(img, 64))


def test_planner_refuses_what_the_dataset_refuses():
    from muscle_amd.irndata import IrnStager, plan_irn_item
    img = R.synth_image(20, 30, 0)
    with pytest.raises(ValueError):
        plan_irn_item(img, np.zeros((20, 31), np.uint8), 32)
    with pytest.raises(ValueError):
        plan_irn_item(img, np.zeros((20, 30), np.int32), 32)
    with pytest.raises(ValueError):
        IrnStager(torch.device("cpu"), 2, 72)


def test_loader_switch_is_an_argparse_choice(capsys):
    from muscle_amd.train_irn import parse_args
    base = ["--ir_label_dir", "L", "--irn_weights_name", "w.pth", "--backbone_weights", "b.pth"]
    assert parse_args(base).loader == "host" and parse_args(base + ["--loader", "device"]).loader == "device"
    with pytest.raises(SystemExit) as e:
        parse_args(base + ["--loader", "bogus"])
    assert e.value.code == 2 and "--loader" in capsys.readouterr().err


def test_entry_point_checks_its_arguments_before_any_launch():
    from muscle_amd import _lib
    L = _lib.lib()
    assert "mx_irn_input_stage" in _lib.parse_header()
    one = _lib.ctypes.c_void_p(4096)
    assert L.mx_irn_input_stage(one, one, one, one, one, 1, 72, None) < 0 and b"multiple of 16" in L.mx_last_error()
    assert L.mx_irn_input_stage(None, one, one, one, one, 1, 64, None) < 0 and b"null" in L.mx_last_error()
    assert L.mx_irn_input_stage(one, one, one, one, one, 0, 64, None) < 0


# ---- GPU ----------------------------------------------------------------------------------------------------------------
def _stage(plans, crop, n=None, **kw):
    from muscle_amd.irndata import IrnStager
    out = IrnStager(torch.device(DEV), n or len(plans), crop)(plans, **kw)
    return {k: v.cpu() for k, v in out.items()}


@pytest.mark.gpu
def test_stager_equals_the_reference_samples_as_one_batch():
    from muscle_amd.irndata import plan_irn_item
    z = np.load(GOLD)
    img, lbl, crop, seeds = _fixture_items(z)
    assert len(seeds) == 4
    out = _stage([plan_irn_item(img, lbl, crop, random.Random(s)) for s in seeds], crop)
    assert out["img"].dtype == torch.float32 and out["label"].dtype == torch.uint8
    for i, s in enumerate(seeds):
        _assert_fixture(z, s, out["img"][i].numpy(), out["label"][i].numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("crop", [64, 128])
def test_stager_equals_the_host_loader_bit_for_bit(samples, crop):
    from muscle_amd.irndata import IrnStager
    mine = [t for t in samples if t[2] == crop]
    assert len({t[0] for t in mine}) == (3 if crop == 64 else 1)
    out = _stage([t[3] for t in mine], crop)                                               # one mixed batch
    single = IrnStager(torch.device(DEV), 1, crop)
    for i, (c, s, _, p, a, r) in enumerate(mine):
        assert torch.equal(out["img"][i], torch.from_numpy(a)), (c, s)
        assert torch.equal(out["label"][i], torch.from_numpy(r)), (c, s)
        one = single([p])                                                                  # and one item at a time
        assert torch.equal(one["img"].cpu()[0], torch.from_numpy(a)), (c, s)
        assert torch.equal(one["label"].cpu()[0], torch.from_numpy(r)), (c, s)
    assert 0 < single.last_bytes < 64 * 1024


@pytest.mark.gpu
@pytest.mark.parametrize("eval_view", [False, True])
def test_outputs_are_fully_written_and_nothing_else_is(samples, eval_view):
    """img prefilled with NaN, label with 0xAB (no test label holds 171), both carved out of one buffer of 0x5C bytes: no NaN and
    no 0xAB is left, and the 4 KB before and after each output keep their 0x5C."""
    from muscle_amd.irndata import plan_irn_eval_item
    S, pad = 64, 4096
    if eval_view:
        plans = [plan_irn_eval_item(R.synth_image(h, w, 3), S) for h, w in ((40, 50), (97, 203), (64, 64))]
    else:
        plans = [t[3] for t in samples if t[2] == S]
    n = len(plans)
    nb_img, nb_lab = n * 3 * S * S * 4, n * (S // 4) ** 2
    assert nb_img % pad == 0
    arena = torch.full((pad + nb_img + pad + nb_lab + pad,), 0x5C, dtype=torch.uint8, device=DEV)
    img = arena[pad:pad + nb_img].view(torch.float32).view(n, 3, S, S)
    lab = arena[2 * pad + nb_img:2 * pad + nb_img + nb_lab].view(n, S // 4, S // 4)
    img.fill_(float("nan"))
    lab.fill_(0xAB)
    out = _stage(plans, S, out={"img": img} if eval_view else {"img": img, "label": lab})
    assert sorted(out) == (["img"] if eval_view else ["img", "label"])
    assert not bool(torch.isnan(img).any())
    host = arena.cpu()
    guards = [host[:pad], host[pad + nb_img:2 * pad + nb_img], host[2 * pad + nb_img + nb_lab:]]
    assert all(bool((g == 0x5C).all()) for g in guards)
    if eval_view:
        assert bool((lab == 0xAB).all())                                                   # no label is written for the eval view
    else:
        assert not bool((lab == 0xAB).any())
        assert torch.equal(out["img"], torch.stack([torch.from_numpy(t[4]) for t in samples if t[2] == S]))


@pytest.mark.gpu
def test_eval_view_equals_top_left_sample():
    from muscle_amd.irndata import plan_irn_eval_item
    from muscle_amd.train_irn import top_left_sample
    imgs = [R.synth_image(40, 50, 1), R.synth_image(97, 203, 2)]
    out = _stage([plan_irn_eval_item(im, 64) for im in imgs], 64)
    assert sorted(out) == ["img"]
    for i, im in enumerate(imgs):
        assert torch.equal(out["img"][i], torch.from_numpy(top_left_sample(im, 64))), i


def _seed(s):
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


@pytest.fixture(scope="module")
def voc_tree(tmp_path_factory):
    return R.make_voc_tree(str(tmp_path_factory.mktemp("irn_voc")))


@pytest.mark.gpu
def test_loader_yields_the_host_loaders_batches(voc_tree):
    """Seed 3, batch 2, crop 64, no workers, two epochs and the eval pass: IrnLoader's batches are the batches of the DataLoader
    that train_irn.main builds over VOC12AffinityDataset, bit for bit - `--loader device` trains on the same tensors."""
    from torch.utils.data import DataLoader
    from muscle_amd.irndata import IrnLoader, VOC12AffinityPlans
    from muscle_amd.train_irn import VOC12AffinityDataset
    names, voc, lab, _ = voc_tree
    dev = torch.device(DEV)
    _seed(3)
    host = DataLoader(VOC12AffinityDataset(names, voc, lab, 64), batch_size=2, shuffle=True, num_workers=0, pin_memory=True,
                      drop_last=True)
    want = [(b["img"].clone(), b["label"].clone()) for _ in range(2) for b in host]
    after_host = random.random()
    _seed(3)
    mine = IrnLoader(VOC12AffinityPlans(names, voc, lab, 64), 2, dev, num_workers=0, shuffle=True, drop_last=True,
                     persistent_workers=False)
    got = [(b["img"].cpu(), b["label"].cpu()) for _ in range(2) for b in mine]
    assert random.random() == after_host
    assert len(mine) == len(host) == 3 and len(got) == len(want) == 6
    for (gi, gl), (wi, wl) in zip(got, want):
        assert torch.equal(gi, wi) and torch.equal(gl, wl)
    assert len({float(w[0].sum()) for w in want}) == 6                                     # the epochs differ: not one batch six times
    ev_host = DataLoader(VOC12AffinityDataset(names, voc, lab, 64, train=False), batch_size=4, shuffle=False, num_workers=0,
                         drop_last=False)
    ev_mine = IrnLoader(VOC12AffinityPlans(names, voc, lab, 64, train=False), 4, dev, num_workers=0, shuffle=False, drop_last=False)
    batches = list(ev_mine)
    assert [tuple(b["img"].shape) for b in batches] == [(4, 3, 64, 64), (2, 3, 64, 64)] and all(sorted(b) == ["img"] for b in batches)
    for b, w in zip(batches, ev_host):
        assert torch.equal(b["img"].cpu(), w["img"])


@pytest.mark.gpu
def test_train_script_with_the_device_loader(voc_tree, tmp_path):
    """train_irn.main with --loader device writes a checkpoint EdgeDisplacement loads, and - irn_step repeats its bits
    (tests/test_gpu_irn_train.py::test_two_identical_steps_give_bit_equal_gradients) - the tensors --loader host writes.
    Crop 80, not 64: the script builds PathIndex(radius=10), which has no source window on a map narrower than 20 pixels, so
    80 is the smallest crop either loader can train at."""
    import muscle_amd
    from muscle_amd import synth, train_irn
    names, voc, lab, lst = voc_tree
    bb = str(tmp_path / "backbone.pth")
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in synth.irn_state_dict(2).items()}, bb)
    sds = {}
    for kind in ("device", "host"):
        out = str(tmp_path / f"irn_{kind}.pth")
        assert train_irn.main(["--voc12_root", voc, "--train_list", lst, "--ir_label_dir", lab, "--irn_weights_name", out,
                               "--backbone_weights", bb, "--loader", kind, "--irn_crop_size", "80", "--irn_batch_size", "2",
                               "--irn_num_epoches", "1", "--num_workers", "0", "--seed", "5"]) == 0
        sds[kind] = torch.load(out, map_location="cpu")
    net = muscle_amd.EdgeDisplacement(crop_size=80)
    net.load_state_dict(sds["device"], strict=False)                                      # infer_irn.py:41
    assert sorted(sds["device"]) == sorted(sds["host"])
    trained = [k for k in sds["host"] if k.startswith("fc_") and k.endswith("weight")]
    assert trained
    for k in sds["host"]:
        assert torch.equal(sds["device"][k], sds["host"][k]), k
    before = synth.irn_state_dict(2)
    assert any(not np.array_equal(sds["device"][k].numpy(), before[k]) for k in trained if k in before)   # it did train
    assert bool(torch.isfinite(sds["device"]["mean_shift.running_mean"]).all())
