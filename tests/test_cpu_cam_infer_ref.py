"""CPU checks behind tests/test_gpu_cam_infer_kernels.py: the float64 restatements of tests/cam_infer_ref.py against independent
statements of the same operations (torch's two F.interpolate calls; the oracle's post-processing expressions), the fp32
restatement against the derived bounds on every table case, the input conditions the GPU cases rely on for the committed seeds,
and planted coordinate errors on the restatement's side: each must leave the bound by a factor of 10 or more on some case."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cam_infer_ref as R
from dec_ref import F32, GRID_CAP, U

SINGLES = [(g, f) for g in R.GEOMS for f in (0, 1)]


def _id(c):
    return "-".join(map(str, c[0])) + f"-flip{c[1]}"


def _interp(src, K, Hs, Ws, H, W, flip):
    """The model's F.interpolate(align_corners=True) to Hs x Ws, the script's resize (align_corners=False) to H x W, np.flip."""
    x = src[..., 1:K].permute(2, 0, 1)[None].double()
    up = F.interpolate(x, size=(Hs, Ws), mode="bilinear", align_corners=True)
    v = F.interpolate(up, size=(H, W), mode="bilinear", align_corners=False)[0]
    return torch.flip(v, dims=[2]) if flip else v


@pytest.mark.parametrize("case", SINGLES, ids=_id)
def test_accum_equals_two_interpolates(case):
    (h, w, Hs, Ws, H, W), flip = case
    for K, lds in R.KLDS:
        c = R.single_case(case[0], flip, K, lds)
        for which in ("cam", "sgc"):
            ref, mag = c["rule_" + which]["ref"], c["rule_" + which]["mag"]
            want = _interp(c[which][0], K, Hs, Ws, H, W, flip)
            assert ref.shape == (K - 1, H, W) and not bool(ref.isnan().any())
            assert float(((ref - want).abs() / mag).max()) <= 1e-12
            assert bool((mag >= ref.abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("name", list(R.MULTI))
def test_tables_equal_the_oracles_post_processing(name):
    """oracle.mcl_oracle.infer_cam's statements after the forward, fed the same per-pass maps: resize, flip, drop channel 0, and
    infer_norm's sum, clamp and min-max.  The oracle decides `norm < mn + 1e-6` in float64, the restatement in fp32 on the sums
    rounded to fp32: pixels within those roundings of the threshold are left out (and counted: a handful at most)."""
    from oracle import mcl_oracle as O
    rows, (H, W) = R.MULTI[name]
    K = 21
    c = R.table_case(tuple(rows), (H, W), K, 24)
    for which in ("cam", "sgc"):
        stack = []
        for src, (h, w, Hs, Ws, flip) in zip(c[which], rows):
            raw = F.interpolate(src[..., :K].permute(2, 0, 1)[None].double(), size=(Hs, Ws), mode="bilinear", align_corners=True)
            raw = F.interpolate(raw, size=(H, W), mode="bilinear", align_corners=False)[0].numpy()
            if flip:
                raw = np.flip(raw, axis=2)
            stack.append(raw[1:])
        ref = c["rule_" + which]["ref"]
        total = np.sum(stack, axis=0)
        assert float((np.abs(total - ref.numpy()) / c["rule_" + which]["mag"].numpy()).max()) <= 1e-12
        want = O.infer_norm([s.copy() for s in stack])
        # the normalisation on the oracle's own sums (the two sums differ by their order: 1e-16 of sum |term|, which is not small
        # beside a pixel just above the minimum)
        got, mag, zeroed, (mn, mx) = R.norm(total.astype(np.float32), cont=total, eps=1e-6)
        v = np.maximum(total, 0.0)
        lo = (mn + 1e-6)[:, None, None]
        near = np.abs(v - lo) <= 8 * U * (np.abs(v) + lo)
        assert near.sum() <= 8 and zeroed.any() and not zeroed.all()
        assert float((np.abs(got - want) / mag)[~near].max()) <= 1e-12


def _all_cases():
    for g, f in SINGLES:
        for K, lds in R.KLDS:
            yield f"{_id((g, f))} K={K} lds={lds}", R.single_case(g, f, K, lds)
    for name, (rows, HW) in R.MULTI.items():
        yield name, R.table_case(tuple(rows), HW, 21, 24)
    a = R.ABOVE_CAP
    yield "above_cap", R.single_case(a["geom"], a["flip"], a["K"], a["lds"])


def test_fp32_restatement_meets_the_bound():
    worst = 0.0
    for tag, c in _all_cases():
        for which in ("cam", "sgc"):
            rule = c["rule_" + which]
            got = R.witness_units(c, which)
            worst = max(worst, got / rule["allowed"])
            assert got <= rule["allowed"], (tag, which, got, rule["allowed"])
    print(f"fp32 restatement: at most {worst:.3f} of the bound")
    for HW in R.NORM_HW:
        a, (val, mag, zeroed, _) = R.norm_case(HW)
        e = np.abs(R.norm32(a).astype(np.float64) - val) / (U * mag)
        print(f"norm HW={HW}: {e.max():.3g} units, allowed {R.NORM_OPS}")
        assert e.max() <= R.NORM_OPS


def _coords32(n_out, n_in):
    s = R.hp_source(n_out, n_in, F32)
    return s, R.hp_coords(n_out, n_in, F32)


def test_geometries_are_what_they_claim():
    assert set(R.GEOM_CLAIMS) == set(R.GEOMS)
    for g, claims in R.GEOM_CLAIMS.items():
        h, w, Hs, Ws, H, W = g
        (sy, (y0, y1, fy)), (sx, (x0, x1, fx)) = _coords32(H, Hs), _coords32(W, Ws)
        for cl in claims:
            if cl == "one_pixel_map":
                assert h == w == 1
            elif cl == "ac_out1":
                assert h == 1 and Hs == 1 and float(R.ac_scale(Hs, h, F32)) == 0.0
            elif cl == "one_column":
                assert w == Ws == W == 1
            elif cl == "single_output":
                assert H == W == 1 and float(fy[0]) == 0.5 and float(fx[0]) == 0.5      # between two pixels: both taps count
            elif cl == "hp_identity":
                assert bool((fy == 0).all()) and bool((fx == 0).all()) and y0.tolist() == list(range(H)) and x0.tolist() == list(range(W))
            elif cl == "hp_lo_clamp":
                assert float(sy.min()) < 0 and float(sx.min()) < 0 and float(fy[0]) == 0.0 and float(fx[0]) == 0.0
            elif cl == "hp_hi_clamp":
                assert bool(((y0 == Hs - 1) & (y1 == y0) & (fy > 0)).any()) and bool(((x0 == Ws - 1) & (x1 == x0) & (fx > 0)).any())
            elif cl == "hp_down2":
                assert Hs == 2 * H and Ws == 2 * W and bool((fy == 0.5).all()) and bool((fx == 0.5).all())
            elif cl == "w_odd":
                assert W % 2 == 1 and Hs > H and Ws < W
            elif cl == "w_even":
                assert W % 2 == 0 and Hs > H and Ws < W
            else:
                raise AssertionError(cl)
        # the fp32 taps are the float64 ones except where the fp32 coordinate crosses an integer (the slope term's case)
        for n_out, n_in in ((H, Hs), (W, Ws)):
            i64, i32 = R.hp_coords(n_out, n_in)[0], R.hp_coords(n_out, n_in, F32)[0]
            assert int((i64 - i32).abs().max()) <= 1


def test_channel_tables_and_caps():
    for K, lds, keep in R.CHANNELS:
        assert 1 < K <= lds and lds % 4 == 0 and 0 < len(keep) <= K - 1 and all(0 <= k < K - 1 for k in keep)
    assert [len(c[2]) for c in R.TAIL_CHUNKS] == [5, 23]
    assert all(len(c[2]) % R.CAM_CH != 0 and len(c[2]) > R.CAM_CH for c in R.TAIL_CHUNKS)
    assert any(len(set(c[2])) < len(c[2]) and list(c[2]) != sorted(c[2]) for c in R.CHANNELS)
    a = R.ABOVE_CAP
    H, W = a["geom"][4:]
    assert H * W > GRID_CAP and (a["K"] - 1) * H * W > GRID_CAP and len(a["keep"]) == 1          # both kernels, one channel
    for keep in R.MULTI_KEEPS:
        assert all(0 <= k < 20 for k in keep)
    for rows, (H, W) in R.MULTI.values():
        for f in range(5):
            assert f == 4 or len({r[f] for r in rows}) == (len(rows) if len(rows) == 2 else 4)
    assert [r[4] for r in R.SCRIPT_TABLE] == [0, 1] * 4


def test_script_table_is_the_models_sizes():
    """h, w of the script's rows: efficientnet-b0's static-padding arithmetic down to the last tap (no last pooling), as
    MuSCLe.forward(cam="cam_lr") returns them; Hs, Ws: infer_mcl.py's int(round(size * scale))."""
    from muscle_amd.arch import net_cfg
    cfg = net_cfg("efficientnet-b0", False)

    def lr(n):
        s = cfg.stem_out_size(n)
        for b in cfg.blocks:
            s = b.out_size(s)
        return s
    H, W = R.SCRIPT_HW
    assert [(lr(int(round(H * s))), lr(int(round(W * s))), int(round(H * s)), int(round(W * s))) for s in (0.5, 1.0, 1.5, 2.0)] == \
        R.SCRIPT_SIZES


def test_norm_kinds_are_what_they_claim():
    for HW in R.NORM_HW:
        a, (val, mag, zeroed, (mn, mx)) = R.norm_case(HW)
        ch = dict(zip(R.NORM_KINDS, range(len(R.NORM_KINDS))))
        v = np.maximum(a, 0)
        assert np.array_equal(mn, v.min(1)) and np.array_equal(mx, v.max(1))
        assert np.array_equal(R.norm32(a)[ch["negative"]], np.full(HW, -1.0, np.float32))
        assert np.array_equal(val[ch["negative"]], np.full(HW, -1.0)) and zeroed[ch["negative"]].all()
        assert (a[ch["negative"]] < 0).all() and (a[ch["constant"]] == a[ch["constant"]][0]).all() and zeroed[ch["constant"]].all()
        # zeroed and kept values cannot be confused: a kept value lies far above the zeroed pixels' value
        z = (0.0 - mn - float(R.EPS32)) / (mx - mn + float(R.EPS32))
        for c in range(len(R.NORM_KINDS)):
            assert np.allclose(val[c][zeroed[c]], z[c], rtol=0, atol=0)
            if (~zeroed[c]).any():
                assert val[c][~zeroed[c]].min() > z[c] / 2
        if HW < 63:
            continue
        w4 = R.wave4_index(HW)
        s, p, e = a[ch["spread"]], a[ch["positive"]], a[ch["edge"]]
        assert (s < 0).any() and mn[ch["spread"]] == 0 and s.std() > 1
        lo0, ev0 = R.edge_values(0.0)
        assert s[1:5].tolist() == ev0 and zeroed[ch["spread"]][1:5].tolist() == [True, False, False, False]
        assert (p > 0).all() and (p == p.min()).sum() == 1 and zeroed[ch["positive"]].sum() == 1
        lo, ev = R.edge_values(R.EDGE_MN)
        assert (e > 0).all() and (e == R.EDGE_MN).sum() == 3 and e.min() == R.EDGE_MN and e[1:5].tolist() == ev
        assert ev[0] < lo == ev[1] < ev[2] < ev[3] and ev[0] > R.EDGE_MN
        assert np.nextafter(ev[0], np.float32(np.inf)) == lo and np.nextafter(ev[2], np.float32(np.inf)) == ev[3]
        assert zeroed[ch["edge"]].sum() == 4 and zeroed[ch["edge"]][1:5].tolist() == [True, False, False, False]
        for kind, (i_mx, i_mn) in (("ext_last", (HW - 1, w4)), ("ext_wave4", (w4, HW - 1))):
            x = a[ch[kind]]
            if i_mx is not None:
                assert int(x.argmax()) == i_mx and (x == x.max()).sum() == 1
            if i_mn is not None:
                assert int(x.argmin()) == i_mn and (x == x.min()).sum() == 1
        assert (w4 is None) == (HW <= 193) and (w4 is None or (w4 % 256 >= 192 and w4 < HW - 1))
    assert any(R.wave4_index(HW) is not None and HW % 256 for HW in R.NORM_HW)


# ---- planted errors on the restatement's side ---------------------------------------------------------------------------------------
def _hp_no_half(n_out, n_in, dtype):
    ratio = torch.tensor(float(n_in), dtype=dtype) / torch.tensor(float(n_out), dtype=dtype)
    return R._taps(((torch.arange(n_out, dtype=dtype) + 0.5) * ratio).clamp_min(0.0), n_in, dtype)


def _ac_in_over_out(n_out, n_in, dtype):
    ratio = torch.tensor(float(n_in), dtype=dtype) / torch.tensor(float(n_out), dtype=dtype)
    return R._taps(ratio * torch.arange(n_out, dtype=dtype), n_in, dtype)


def _hp_no_clamp(n_out, n_in, dtype):
    s = R.hp_source(n_out, n_in, dtype)
    i0 = s.floor().long().clamp(min=0, max=n_in - 1)           # the index stays inside; the weight goes negative
    return i0, (i0 + 1).clamp(max=n_in - 1), s - i0.to(dtype)


def _flip_one_off(v, W):
    return v[..., (W - torch.arange(W)).clamp(max=W - 1)]


PLANTS = {"hp without -0.5": dict(hp=_hp_no_half), "align_corners scale in/out": dict(ac=_ac_in_over_out),
          "hp without the clamp at 0": dict(hp=_hp_no_clamp), "flip W - X, clamped": dict(flip=_flip_one_off)}


@pytest.mark.parametrize("plant", list(PLANTS))
def test_planted_coordinate_errors_leave_the_bound(plant):
    rules = dict(R.RULES, **PLANTS[plant])
    factors = {}
    for tag, c in _all_cases():
        if tag == "above_cap":
            continue
        passes = [(m, r[2], r[3], r[4]) for m, r in zip(c["cam"], c["rows"])]
        wrong = R.accum(passes, c["K"], c["H"], c["W"], rules=rules)[0]
        rule = c["rule_cam"]
        factors[tag] = R.worst_units(wrong, rule["ref"], R.tolerance(rule), 1.0)
    seen = {t: f for t, f in factors.items() if f >= 10}
    print(f"{plant}: leaves the bound by 10x or more on {len(seen)} of {len(factors)} cases; largest factor {max(factors.values()):.3g}")
    for t, f in factors.items():
        print(f"    {t}: {f:.3g}")
    assert seen, factors
