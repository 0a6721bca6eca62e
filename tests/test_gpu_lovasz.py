"""The Lovasz-softmax loss on the GPU (muscle_amd.lovasz / mx_lovasz_*) against the numpy restatement of its model in lovasz_ref.py.

Core (mx_lovasz_core on fp32 errors the test makes, so the order is unambiguous): rank equals numpy's stable order integer for
integer, the counts are exact, g is within 1 ulp of float32(closed form in float64) - one rounding after exact integers - and
seg_loss goes under the tolerance rule.  Errors stage and end to end: the rule below.  The loss value is tie-invariant and is
compared with the restatement's own order; the gradient is compared with the restatement evaluated on the kernel's order
(order_from = the kernel's err, itself checked by the errors-stage test), because the larger cases have near ties that fp32
rounding reorders.  1x3x5x7 has none (asserted on the reference alone) and is compared with nothing taken from the kernel.

Tolerance, the convention of tests/test_gpu_crf_loss.py: per case e32 is the error of the float32 restatement against the float64
one for the same input and the same order_from - absolute for losses, max-abs relative to the tensor's max-abs for err and the
gradient - and the kernel must stay within F_TOL * e32 + 1e-7.  F_TOL is twice the worst ratio err / e32 measured once on an
MI355X over the cases below, rounded up (profiles/lovasz_bench.txt lists them); the kernels are deterministic, so the margin is
for other inputs, not for noise.  Worst ratio 1.50 -> F_TOL = 3.  The ratios (loss / err / gseg; - : not compared in that case):
    1x3x5x7               0.09 / -    / 0.75 (0.75 with its own order)      2x21x24x40_present  1.00 / 1.00 / 1.00
    2x21x24x40_all        1.50 / -    / 1.00                                 2x5x96x160          1.00 / -    / 1.00
    3x24x33x10_per_image  0.31 / 0.95 / 0.91
    core seg_loss: at most 2.2e-16 absolute in every case (fp64 sums) against e32 up to 8e-8: ratio 0.00
A ratio of 1.00 means the kernel and the float32 restatement round to the same float32."""
import random

import numpy as np
import pytest
import torch

import lovasz_ref as R

pytestmark = [pytest.mark.gpu]
DEV = "cuda:0"
F_TOL = 3.0
FLOOR = 1e-7
G_UP = 0.37


def _rel(a, ref):
    scale = float(np.abs(ref).max())
    return float(np.abs(np.asarray(a, np.float64) - ref).max()) / scale if scale > 0 else float(np.abs(a).max())


def _ratio(err, e32):
    return err / e32 if e32 > 0 else float("nan")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- core: the sort, the scan and the increments on given errors ------------------------------------------------------------------
def _flags(g, shape, valid=0.85, fg=0.3):
    return (2 * (g.random(shape) < valid) + (g.random(shape) < fg)).astype(np.uint8)          # bit 0 may be set on an invalid element


def _core_inputs(name):
    g = np.random.default_rng(sorted(CORE).index(name) + 100)
    if name == "S1_P1":
        return np.array([[0.3]], np.float32), np.array([[3]], np.uint8)
    if name == "S72_P330":                                    # many short segments, a ragged tail
        return g.random((72, 330), dtype=np.float32), _flags(g, (72, 330))
    if name == "S3_P20011_7values":                           # massive ties across block boundaries: stability
        vals = np.array([0.0, 0.125, 0.3, 0.5, 0.7, 0.99, 1.0], np.float32)
        return vals[g.integers(0, 7, (3, 20011))], _flags(g, (3, 20011), fg=0.5)
    if name == "S2_P70001_equal":                             # pure stability, many blocks
        return np.full((2, 70001), 0.625, np.float32), _flags(g, (2, 70001), valid=1.0, fg=0.4)
    if name == "S5_P30720_bituniform":                        # every digit of every pass populated, low mantissa bits included
        bits = g.integers(0, 0x3F800000, (5, 30720), dtype=np.int64, endpoint=True).astype(np.uint32)
        return bits.view(np.float32), _flags(g, (5, 30720))
    if name == "invalid_and_single":                          # a segment with nothing valid, one with a single valid element
        err, flag = g.random((3, 5000), dtype=np.float32), _flags(g, (3, 5000))
        flag[0] &= 1
        flag[1] &= 1
        flag[1, 4097] = 3
        return err, flag
    if name == "zeros_ones_sentinel":                         # errors exactly 0 and exactly 1 mixed with ignored elements
        return g.integers(0, 2, (2, 9000)).astype(np.float32), _flags(g, (2, 9000), valid=0.6, fg=0.5)
    raise KeyError(name)


CORE = ["S1_P1", "S72_P330", "S3_P20011_7values", "S2_P70001_equal", "S5_P30720_bituniform", "invalid_and_single", "zeros_ones_sentinel"]
_CORE = {}


def _core(name):
    if name not in _CORE:
        err, flag = _core_inputs(name)
        _CORE[name] = (err, flag, R.core(err, flag, np.float64), R.core(err, flag, np.float32))
    return _CORE[name]


def _gpu_core(err, flag):
    from muscle_amd import lovasz as LV
    out = LV.lovasz_core(_dev(err), _dev(flag))
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


@pytest.mark.parametrize("name", CORE)
def test_core_rank_counts_and_increments_are_exact(name):
    err, flag, r64, r32 = _core(name)
    rank, g, seg_loss, counts = _gpu_core(err, flag)
    assert np.array_equal(counts, r64["counts"])
    assert np.array_equal(rank, r64["rank"])
    want = r64["g"].astype(np.float32)
    assert (np.abs(g.astype(np.float64) - want) <= np.spacing(np.abs(want))).all()
    assert not g[rank < 0].any()
    e32 = float(np.abs(r32["seg_loss"].astype(np.float64) - r64["seg_loss"]).max())
    got = float(np.abs(seg_loss - r64["seg_loss"]).max())
    print(f"lovasz core {name} seg_loss: err {got:.3e} e32 {e32:.3e} ratio {_ratio(got, e32):.2f}")
    assert got <= F_TOL * e32 + FLOOR, (name, got, e32)


# ---- errors stage and end to end ---------------------------------------------------------------------------------------------------
# name: (N, K, H, W, classes, per_image, absent classes, seed)
CASES = {
    "1x3x5x7": (1, 3, 5, 7, "present", False, (), 0),
    "2x21x24x40_present": (2, 21, 24, 40, "present", False, (4, 17), 1),
    "2x21x24x40_all": (2, 21, 24, 40, "all", False, (4, 17), 1),
    "3x24x33x10_per_image": (3, 24, 33, 10, "present", True, (), 2),
    "2x5x96x160": (2, 5, 96, 160, "present", False, (), 3),                  # P = 30720: several blocks per segment
}
_IN, _OWN, _KERNEL = {}, {}, {}


def _inputs(name):
    if name not in _IN:
        N, K, H, W, classes, per_image, absent, seed = CASES[name]
        _IN[name] = R.make_case(N, K, H, W, seed, absent=absent) + (classes, per_image)
    return _IN[name]


def _own(name):
    """(float64, float32) restatements with their own order, computed once."""
    if name not in _OWN:
        seg, lab, classes, per_image = _inputs(name)
        _OWN[name] = tuple(R.lovasz(seg, lab, classes, per_image, dt, gup=G_UP) for dt in (np.float64, np.float32))
    return _OWN[name]


def _kernel(name):
    """One run of the stages and of the module: err, flag, loss, gseg (upstream G_UP)."""
    if name not in _KERNEL:
        from muscle_amd import lovasz as LV
        seg, lab, classes, per_image = _inputs(name)
        dseg, dlab = _dev(seg).requires_grad_(True), _dev(lab)
        err, flag = LV.lovasz_errors(dseg.detach(), dlab, per_image)
        loss = LV.LovaszSoftmaxLoss(classes, per_image)(dseg, dlab)
        assert loss.dim() == 0 and loss.is_cuda
        (G_UP * loss).backward()
        torch.cuda.synchronize()
        _KERNEL[name] = (err.cpu().numpy(), flag.cpu().numpy(), float(loss.detach()), dseg.grad.cpu().numpy())
    return _KERNEL[name]


@pytest.mark.parametrize("name", ["2x21x24x40_present", "3x24x33x10_per_image"])
def test_errors_stage_against_the_restatement(name):
    r64, r32 = _own(name)
    err, flag, _, _ = _kernel(name)
    assert np.array_equal(flag, r64["flag"])
    assert (err >= 0).all() and (err <= 1).all() and not err[flag == 0].any()
    got, e32 = _rel(err, r64["err"]), _rel(r32["err"], r64["err"])
    print(f"lovasz {name} err: err {got:.3e} e32 {e32:.3e} ratio {_ratio(got, e32):.2f}")
    assert got <= F_TOL * e32 + FLOOR, (name, got, e32)
    if name == "2x21x24x40_present":
        assert not (flag[[4, 17]] & 1).any() and round(float((flag[0] == 0).mean()), 2) == 0.15       # two absent classes, 15 % ignored


@pytest.mark.parametrize("name", list(CASES))
def test_loss_and_gradient_end_to_end(name):
    seg, lab, classes, per_image = _inputs(name)
    r64, r32 = _own(name)
    err, _, loss, gseg = _kernel(name)
    assert np.isfinite(loss) and np.isfinite(gseg).all()
    got, e32 = abs(loss - float(r64["loss"])), abs(float(r32["loss"]) - float(r64["loss"]))
    print(f"lovasz {name} loss: gpu {loss:.9e} ref {float(r64['loss']):.9e} err {got:.3e} e32 {e32:.3e} ratio {_ratio(got, e32):.2f}")
    assert got <= F_TOL * e32 + FLOOR, (name, got, e32)
    o64, o32 = (R.lovasz(seg, lab, classes, per_image, dt, order_from=err, gup=G_UP) for dt in (np.float64, np.float32))
    got, e32 = _rel(gseg, o64["gseg"]), _rel(o32["gseg"], o64["gseg"])
    print(f"lovasz {name} gseg: err {got:.3e} e32 {e32:.3e} ratio {_ratio(got, e32):.2f}")
    assert got <= F_TOL * e32 + FLOOR, (name, got, e32)
    ignored = np.broadcast_to(((lab == 255) | (lab >= seg.shape[1]))[:, None], gseg.shape)
    assert not gseg[ignored].any() and gseg[~ignored].any()


def test_fully_independent_case():
    """1x3x5x7: rank and gradient against the restatement's own float64 order, nothing taken from the kernel."""
    from muscle_amd import lovasz as LV
    name = "1x3x5x7"
    r64, r32 = _own(name)
    margin = R.order_margin(r64)
    print("lovasz 1x3x5x7 order margin", margin)
    assert margin > 0                                                   # on the reference alone: fp32 rounding reorders nothing
    err, flag, _, gseg = _kernel(name)
    rank = LV.lovasz_core(_dev(err), _dev(flag))[0].cpu().numpy()
    assert np.array_equal(rank, r64["rank"])
    got, e32 = _rel(gseg, r64["gseg"]), _rel(r32["gseg"], r64["gseg"])
    print(f"lovasz {name} gseg, own order: err {got:.3e} e32 {e32:.3e} ratio {_ratio(got, e32):.2f}")
    assert got <= F_TOL * e32 + FLOOR


def test_nothing_valid_gives_zero_loss_and_gradient():
    from muscle_amd import lovasz_softmax
    seg = torch.randn(2, 5, 9, 13, device=DEV, requires_grad=True)
    lab = torch.full((2, 9, 13), 255, dtype=torch.uint8, device=DEV)
    lab[1, 0, 0] = 9                                                    # >= K: ignored, never an index
    for per_image in (False, True):
        seg.grad = None
        loss = lovasz_softmax(seg, lab, "all", per_image)
        loss.backward()
        assert float(loss.detach()) == 0.0 and not bool(seg.grad.any())


# ---- self-comparisons ----------------------------------------------------------------------------------------------------------------
def _run(name, gup=G_UP, view=False):
    from muscle_amd import lovasz as LV
    seg, lab, classes, per_image = _inputs(name)
    if view:
        base = _dev(seg.transpose(0, 2, 3, 1)).requires_grad_(True)                          # [N,H,W,K]
        dseg = base.permute(0, 3, 1, 2)
        assert not dseg.is_contiguous()
    else:
        base = dseg = _dev(seg).requires_grad_(True)
    loss = LV.lovasz_softmax(dseg, _dev(lab), classes, per_image)
    (gup * loss).backward()
    err, flag = LV.lovasz_errors(dseg.detach(), _dev(lab), per_image)
    rank = LV.lovasz_core(err, flag)[0]
    torch.cuda.synchronize()
    grad = base.grad.permute(0, 3, 1, 2) if view else base.grad
    return float(loss.detach()), grad.cpu().numpy(), rank.cpu().numpy()


def test_two_runs_a_view_and_the_upstream_scale():
    for name in ("2x21x24x40_present", "2x5x96x160"):
        l0, g0, r0 = _run(name)
        l1, g1, r1 = _run(name)
        assert l0 == l1 and np.array_equal(g0, g1) and np.array_equal(r0, r1), name          # the same bits every run
        l2, g2, r2 = _run(name, view=True)
        assert l0 == l2 and np.array_equal(g0, g2) and np.array_equal(r0, r2), name          # a non-contiguous seg_map
    _, ga, _ = _run("2x21x24x40_present", gup=1.0)
    _, gb, _ = _run("2x21x24x40_present", gup=2.0)
    assert np.array_equal(2.0 * ga, gb) and ga.any()                                         # gup scales the gradient


# ---- step level: the smallest label batch of tests/test_gpu_label_path.py (B0 decoder, crop 64, batch 2) -------------------------
def _label_batch(n, S, soft=False):
    gen = torch.Generator().manual_seed(1000 * n + S)
    lab = torch.zeros(n, 20)
    mask = torch.zeros(n, S, S, dtype=torch.uint8)
    yy, xx = torch.meshgrid(torch.arange(S), torch.arange(S), indexing="ij")
    for i in range(n):
        c = 3 + 4 * i
        lab[i, c - 1] = 1
        mask[i][(yy - S // 2 + 5 * i) ** 2 + (xx - S // 3) ** 2 < (S // 4) ** 2] = c
        mask[i, :, S - 9:] = 255
    if soft:
        m = torch.nn.functional.one_hot(mask.clamp(max=20).long(), 21).permute(0, 3, 1, 2).float() * (mask != 255)[:, None]
        mask = m.contiguous()
    return {"img": torch.randn(n, 3, S, S, generator=gen).to(DEV), "label": lab.to(DEV), "mask": mask.to(DEV)}


def _model():
    import muscle_amd
    torch.manual_seed(0)
    model = muscle_amd.MuSCLe(21, "efficientnet-b0", layers=3, last_pooling=True, mode="dec").to(DEV)
    opt = muscle_amd.FusedAdam(model.parameters(), lr=1e-4, weight_decay=1e-5)
    torch.manual_seed(1)                                               # the drop_connect draws
    random.seed(5)
    return model, opt


def _step(batch, **kw):
    import muscle_amd
    model, opt = _model()
    out = muscle_amd.muscle_step(model, opt, batch, lamb=0.0, step=7, k=8, **kw)
    torch.cuda.synchronize()
    return out, torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu()


def test_muscle_step_with_the_loss_off_and_on():
    import muscle_amd
    batch = _label_batch(2, 64)
    crit = muscle_amd.LovaszSoftmaxLoss()
    (plain, p0), (none, p1), (off, p2) = _step(batch), _step(batch, lovasz=None), _step(batch, lovasz=crit, lovasz_weight=0.0)
    assert set(plain) == set(none) == set(off) == {"loss_seg", "loss_beacon", "grad_norm"}
    for out, p in ((none, p1), (off, p2)):
        assert torch.equal(p0, p) and float(plain["loss_seg"]) == float(out["loss_seg"])
        assert float(plain["grad_norm"]) == float(out["grad_norm"])
    on, p3 = _step(batch, lovasz=crit, lovasz_weight=0.5)
    assert set(on) == set(plain) | {"loss_lovasz"}
    model, _ = _model()
    model.train()
    seg_map, _ = model(batch["img"], cam="seg_p3")
    want = float(crit(seg_map, batch["mask"]).detach())
    got = float(on["loss_lovasz"].detach())
    print("lovasz muscle_step loss_lovasz", got, "grad_norm", float(on["grad_norm"]), "without", float(plain["grad_norm"]))
    assert got == want and 0.0 < got < 1.0
    assert float(on["loss_seg"]) == float(plain["loss_seg"])           # the forward is the same; the gradient is not
    assert not torch.equal(p0, p3) and bool(torch.isfinite(p3).all())


def test_refusals():
    import muscle_amd
    from muscle_amd import edge
    crit = muscle_amd.LovaszSoftmaxLoss()
    with pytest.raises(ValueError, match="label map"):
        _step(_label_batch(2, 64, soft=True), lovasz=crit, lovasz_weight=0.5)
    model, opt = _model()
    field = edge.FieldLoss(sobel_size=5, beta=1e2, k=8, sampler="device", seed=1)
    with pytest.raises(ValueError, match="Lovasz"):
        muscle_amd.GraphedMuscleStep(model, opt, field, lamb=0.05, step=7, k=8, lovasz=crit)
