"""The hard-label-map path (mask_type="label") on the GPU: mx_label_stage, mx_ce_label and mx_field_mask_label ALONE against the
restatements of tests/label_ref.py, then the loss level (muscle_amd.edge.cross_entropy_label, FieldLoss on a uint8 map) and the
step level (muscle_step on a label batch).  Every kernel case runs twice and must give the same bits; outputs carry canaries (or
NaN) where the kernel must overwrite.

Tolerances: the rules of tests/test_gpu_dec_kernels.py, no new numbers.  Exact regimes (the staged label map, the integer regime
of the loss, untouched and zeroed regions) are asserted with torch.equal; the loss by the sum rule (4 e_ref + 2U) x sum |term|,
the magnitude taken over the valid pixels; the gradient at 4 x dec_ref.ce_bwd_units; the mask rows and the FieldLoss gradient at
4 x the error of the plain fp32 restatement measured on a fixed draw.  No tolerance is taken from a kernel's output."""
import random

import numpy as np
import pytest
import torch

import dec_ref as R
import label_ref as LR
import segdata_ref as SR
from dec_ref import U
from dec_gpu_util import DEV, FLUSH, Profile, check_elementwise, check_sums, twice

pytestmark = pytest.mark.gpu

PROF = Profile("tests/test_gpu_label_path.py")
NAN = float("nan")
BYTE_CANARY = 0xA5


def _call(name, *args):
    from muscle_amd._lib import call, stream
    call(name, *args, stream())


def _p(t):
    from muscle_amd._lib import ptr
    return ptr(t)


def _id(c):
    return "x".join(map(str, c))


def _seed(s):
    random.seed(s)
    torch.manual_seed(s)


# ---- mx_label_stage ---------------------------------------------------------------------------------------------------------------
# an item: (sh, sw, top, left, ch, cw, flip).  S = 96: the window equal to the container, smaller in one axis, smaller in both;
# source widths 7, 125 and 501.  S = 40: a 1 x 1 source, and the 96-pixel items' kinds again at the smaller container.
# S = 41: rows whose last byte is a tail of the 4-byte groups and whose starts are not 4-byte aligned.
STAGE_CASES = {
    "S96-n3": (96, [(20, 7, 0, 0, 96, 96, 0), (33, 125, 0, 20, 96, 50, 1), (9, 501, 13, 30, 40, 17, 0)], 255),
    "S96-n3-flipped": (96, [(20, 7, 0, 0, 96, 96, 1), (33, 125, 0, 20, 96, 50, 0), (9, 501, 13, 30, 40, 17, 1)], 255),
    "S96-n1": (96, [(64, 125, 5, 0, 70, 96, 1)], 255),
    "S40-n1": (40, [(1, 1, 11, 7, 3, 5, 0)], 255),
    "S40-n3-fill7": (40, [(5, 501, 0, 0, 40, 40, 1), (12, 7, 1, 0, 39, 40, 0), (31, 125, 20, 21, 20, 19, 1)], 7),
    "S41-n2": (41, [(6, 7, 0, 0, 41, 41, 1), (17, 125, 2, 3, 30, 37, 0)], 255),
}


def _stage_case(S, items, fill, seed):
    """One device buffer as a stager lays it out - [jobs | tables | source rows] - with source rows at byte offsets that are
    not multiples of 4 and random (not monotone) index tables; returns (the bytes, the numpy restatement per item)."""
    rng = np.random.default_rng(seed)
    n = len(items)
    off = n * 64
    tabs, srcs, want = [], [], []
    for (sh, sw, top, left, ch, cw, flip) in items:
        ys, xs = rng.integers(0, sh, ch).astype(np.int32), rng.integers(0, sw, cw).astype(np.int32)
        ys[0], ys[-1], xs[0], xs[-1] = sh - 1, 0, sw - 1, 0                  # the last row and column are read
        tabs.append((off, ys, off + 4 * ch, xs))
        off += 4 * (ch + cw)
    for i, (sh, sw, *_rest) in enumerate(items):
        off += 1 + i % 3 if (off + 1 + i % 3) % 4 else 2 + i % 3             # never 4-byte aligned
        srcs.append((off, rng.integers(0, 256, sh * sw).astype(np.uint8)))
        off += sh * sw
    buf = np.zeros(off, np.uint8)
    jobs = buf[:n * 64].view(np.int32).reshape(n, 16)
    for i, ((sh, sw, top, left, ch, cw, flip), (yo, ys, xo, xs), (so, src)) in enumerate(zip(items, tabs, srcs)):
        assert so % 4 != 0 and yo % 4 == 0
        jobs[i, :10] = (so, sh, sw, top, left, ch, cw, flip, yo // 4, xo // 4)
        buf[yo:yo + 4 * ch] = ys.view(np.uint8)
        buf[xo:xo + 4 * cw] = xs.view(np.uint8)
        buf[so:so + sh * sw] = src
        want.append(LR.label_stage(src, sh, sw, ys, xs, top, left, flip, S, fill))
    return buf, want


@pytest.mark.parametrize("case", list(STAGE_CASES))
def test_label_stage_equals_the_numpy_restatement(case):
    """dst is fully written over a canary; the guard bytes behind it keep theirs."""
    S, items, fill = STAGE_CASES[case]
    n = len(items)
    buf, want = _stage_case(S, items, fill, R.case_seed(S, n, fill))
    d_buf = torch.from_numpy(buf).to(DEV)

    def run():
        dst = torch.full((n * S * S + 64,), BYTE_CANARY, dtype=torch.uint8, device=DEV)
        _call("mx_label_stage", _p(d_buf), _p(d_buf), _p(d_buf), _p(dst), n, S, fill)
        return dst
    got = twice(run)
    assert bool((got[n * S * S:] == BYTE_CANARY).all()), "bytes behind dst were written"
    got = got[:n * S * S].view(n, S, S).numpy()
    for i in range(n):
        assert np.array_equal(got[i], want[i]), (case, i, int((got[i] != want[i]).sum()))


STAGER_CASES = [(75, 101, 0.6, 0), (96, 73, 1.0, 1), (31, 23, 1.75, 1), (150, 131, 0.5, 0)]


def test_stager_stages_label_plans_and_the_soft_paths_image():
    """Through SegStager: "mask" is the uint8 [n,S,S] restatement of every plan (Pillow NEAREST, container of 255, flip), and
    "img" is bit-equal to the soft stager's for the same seeds."""
    from muscle_amd import segdata as D
    S, dev = 96, torch.device(DEV)
    ims = [SR.synth_image(H, W, 10 + i) for i, (H, W, _, _) in enumerate(STAGER_CASES)]
    maps = [LR.synth_label_map(H, W, 30 + i) for i, (H, W, _, _) in enumerate(STAGER_CASES)]
    plans = {}
    for kind in ("label", "soft"):
        _seed(23)
        plans[kind] = []
        for i, (H, W, s, flip) in enumerate(STAGER_CASES):
            p = D.plan_label_item(ims[i], maps[i], s, s, S) if kind == "label" else \
                D.plan_seg_item(ims[i], SR.synth_label(H, W, 50 + i), s, s, S)
            p.flip = bool(flip)
            plans[kind].append(p)
    labels = torch.zeros(4, 20)
    labels[:, 5] = 1
    stager = D.SegStager(dev, 4, S)
    a = stager(plans["label"], labels=labels)
    b = stager(plans["label"], labels=labels)
    soft_stager = D.SegStager(dev, 4, S)
    soft = soft_stager(plans["soft"], labels=labels)
    torch.cuda.synchronize()
    assert set(a) == {"img", "mask", "label"}
    assert a["mask"].dtype == torch.uint8 and a["mask"].shape == (4, S, S) and a["img"].shape == (4, 3, S, S)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(a["img"], soft["img"])
    got = a["mask"].cpu().numpy()
    padded = 0
    for i, p in enumerate(plans["label"]):
        want = LR.ref_label(maps[i], SR.plan_as_draws(p), S)
        assert np.array_equal(got[i], want), (i, int((got[i] != want).sum()))
        win = SR.window(SR.plan_as_draws(p), S)
        assert bool((got[i][~win] == 255).all())
        padded += int(not win.all())
    assert padded >= 2
    assert stager.last_bytes < soft_stager.last_bytes                  # uint8 rows instead of float16 rows of 21 channels


# ---- mx_ce_label ------------------------------------------------------------------------------------------------------------------
def _ce_forward(seg, label, start):
    N, K, HW = seg.shape
    d_seg, d_lab = seg.to(DEV), label.to(DEV)

    def run():
        loss = torch.full((1,), start, device=DEV)
        ws = torch.full((2,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=DEV)
        _call("mx_ce_label", _p(d_seg), _p(d_lab), LR.IGNORE, None, _p(loss), None, N, K, HW, 0, ws.data_ptr(), 16)
        return loss
    return twice(run)


@pytest.mark.parametrize("kind", ["spread", "confident"])
@pytest.mark.parametrize("shape", R.CE_SHAPES, ids=_id)
def test_ce_label_forward(shape, kind):
    """loss[0] += sum over valid pixels of (log sum exp - seg[label]) / count with about a third of the pixels ignored (255, and
    values in K..254); loss[0] starts at 0.75 and the 16 bytes of scratch hold garbage."""
    seg, label = LR.ce_label_inputs(shape, kind)
    ref, mag, e_ref, rel, cnt = LR.ce_label_rule(seg, label)
    assert 0 < cnt and (cnt < shape[0] * shape[2] or shape[2] == 1)
    got = _ce_forward(seg, label, 0.75).double() - 0.75
    if cnt <= 100000:
        assert rel < 1.0 / (10.0 * cnt)
    check_sums(PROF, f"ce_label fwd {shape} {kind}", got, ref.reshape(1), mag.reshape(1), e_ref, rel,
               extra=2 * U * (0.75 + abs(float(ref))))


@pytest.mark.parametrize("mode", ["one", "none"])
@pytest.mark.parametrize("shape", R.CE_SHAPES, ids=_id)
def test_ce_label_forward_one_valid_and_none(shape, mode):
    """One valid pixel: its own term.  None: loss[0] keeps its start value bit for bit (torch gives NaN there)."""
    seg, label = LR.ce_label_inputs(shape, "spread", mode)
    got = _ce_forward(seg, label, 0.75)
    if mode == "none":
        assert float(got) == 0.75
        return
    ref, mag, e_ref, rel, cnt = LR.ce_label_rule(seg, label)
    assert cnt == 1
    check_sums(PROF, f"ce_label fwd {shape} one valid", got.double() - 0.75, ref.reshape(1), mag.reshape(1), e_ref, rel,
               extra=2 * U * (0.75 + abs(float(ref))))


@pytest.mark.parametrize("mode", ["third", "none"])
@pytest.mark.parametrize("shape", R.CE_SHAPES, ids=_id)
def test_ce_label_forward_exact(shape, mode):
    """The exact regime of dec_ref.ce_exact_inputs with ignored pixels mixed in: every valid term is an integer 20..27 and every
    partial sum is exact, so the loss (from 0) is float32(sum / count) bit for bit - a valid pixel dropped, an ignored one counted
    or a miscounted divisor moves its last places.  All ignored: the loss stays 0."""
    seg, label, want = LR.ce_label_exact_inputs(shape, mode)
    got = _ce_forward(seg, label, 0.0)
    assert torch.equal(got, want), (float(got), float(want))


@pytest.mark.parametrize("kind,mode", [("spread", "third"), ("confident", "third"), ("spread", "one"), ("spread", "none")])
@pytest.mark.parametrize("shape", R.CE_SHAPES, ids=_id)
def test_ce_label_backward(shape, kind, mode):
    """gseg = gup * (softmax - onehot) / count with gup = 0.37 at valid pixels and exactly 0 at ignored ones, over a NaN-filled
    gseg; all ignored: all zeros.  The scratch holds garbage (the call counts for itself)."""
    N, K, HW = shape
    seg, label = LR.ce_label_inputs(shape, kind, mode)
    d_seg, d_lab = seg.to(DEV), label.to(DEV)
    gup = torch.full((1,), 0.37, device=DEV)

    def run():
        gseg = torch.full((N, K, HW), NAN, device=DEV)
        ws = torch.full((2,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=DEV)
        _call("mx_ce_label", _p(d_seg), _p(d_lab), LR.IGNORE, _p(gup), None, _p(gseg), N, K, HW, 1, ws.data_ptr(), 16)
        return gseg
    got = twice(run)
    ignored = ~LR._valid(label, K)
    assert bool((got.permute(0, 2, 1)[ignored] == 0).all()), "an ignored pixel has a gradient"
    assert not bool(got.isnan().any())
    if mode == "none":
        assert bool((got == 0).all())
        return
    ref, mag = LR.ce_label_bwd(seg, label, R.CE_GUP)
    u = R.ce_bwd_units(kind)
    check_elementwise(PROF, f"ce_label bwd {shape} {kind} {mode}", got, ref, mag, 4.0 * u, u, extra_abs=FLUSH)


# ---- mx_field_mask_label ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npts", R.GATHER_NPTS)
@pytest.mark.parametrize("kml", R.GATHER_KML, ids=_id)
def test_field_mask_label(kml, npts):
    """The mask rows at labelled points, ignored points (255 and a value in K..254), the corners, the last row and column and
    repeated points against float64, at 4 x the error of the fp32 restatement on the fixed draw; columns K..ML-1 exactly 0."""
    K, ML = kml
    H = W = 24
    label, pts = LR.mask_label_inputs(K, npts, H, W)
    d_lab, d_pts = label.to(DEV), pts.to(DEV)

    def run():
        mfeat = torch.full((npts, ML), NAN, device=DEV)
        _call("mx_field_mask_label", _p(d_lab), _p(d_pts), npts, _p(mfeat), K, ML, H, W, LR.IGNORE)
        return mfeat
    got = twice(run)
    ref = LR.field_mask_label(label, pts, K, ML, H, W)
    u = LR.mask_label_calib()
    check_elementwise(PROF, f"field_mask_label K={K} ML={ML} npts={npts}", got[:, :K], ref[:, :K], ref[:, :K], 4.0 * u, u,
                      extra_abs=FLUSH)
    assert bool((got[:, K:] == 0).all())
    t = label[pts[:, 0].long(), pts[:, 1].long() // W, pts[:, 1].long() % W]
    if npts >= 5:
        assert bool((t == LR.IGNORE).any()) and bool((t < K).any())               # both kinds of row were among them


# ---- loss level -------------------------------------------------------------------------------------------------------------------
def test_cross_entropy_label_against_float64_and_the_onehot_soft_path():
    """cross_entropy_label on a label map without 255 and cross_entropy_argmax on its one-hot float mask: each loss within the sum
    rule of the float64 reference and each gradient on seg_map within the elementwise rule (both bounded by their distance to
    float64, not to each other's bits)."""
    from muscle_amd import edge
    seg, _, label, _, _ = LR.field_label_case()
    N, K, H, W = seg.shape
    ref, mag, e_ref, rel, cnt = LR.ce_label_rule(seg.view(N, K, H * W), label.view(N, H * W))
    assert cnt == N * H * W and rel < 1.0 / (10.0 * cnt)
    gref, gmag = LR.ce_label_bwd(seg.view(N, K, H * W), label.view(N, H * W), R.CE_GUP)
    u = R.ce_bwd_units("spread")
    d_lab, d_hot = label.to(DEV), LR.onehot_mask(label, K).to(DEV)
    for tag, fn, m in (("label", edge.cross_entropy_label, d_lab), ("onehot", edge.cross_entropy_argmax, d_hot)):
        def run():
            s = seg.to(DEV).requires_grad_()
            loss = fn(s, m)
            (loss * R.CE_GUP).backward()
            return loss.detach().reshape(1), s.grad
        loss, grad = twice(run)
        check_sums(PROF, f"cross_entropy {tag} loss", loss, ref.reshape(1), mag.reshape(1), e_ref, rel, extra=2 * U * abs(float(ref)))
        check_elementwise(PROF, f"cross_entropy {tag} grad", grad.view(N, K, H * W), gref, gmag, 4.0 * u, u, extra_abs=FLUSH)


def test_field_loss_on_a_label_map_against_float64_and_the_onehot_soft_path():
    """FieldLoss (unfused: full-resolution NCHW features) on the uint8 map and on its one-hot float mask, on replayed points
    whose mask decisions are clear of their margins by construction (label_ref.field_label_case): each loss by the sum rule and
    each gradient of the features at 4 x the fp32 restatement's measured error, both against float64."""
    from muscle_amd import edge
    seg, dense, label, lwb, replay = LR.field_label_case()
    c = LR.FIELD_CASE
    rule = LR.field_label_rule()
    ref = rule["ref"]
    assert float(ref["margins"][..., 0].min()) > 1e-4 and float(ref["margins"][..., 1].min()) > 1e-4
    d_seg, d_lwb = seg.to(DEV), lwb.to(DEV)
    for tag, m in (("label", label.to(DEV)), ("onehot", LR.onehot_mask(label, c["K"]).to(DEV))):
        crit = edge.FieldLoss(sobel_size=5, beta=1e2, k=c["k"])
        crit.replay_points = replay

        def run():
            ft = dense.to(DEV).requires_grad_()
            loss, _ = crit(d_seg, ft, m, d_lwb, 7)
            assert torch.is_tensor(loss)
            loss.backward()
            return loss.detach().reshape(1), ft.grad
        loss, grad = (t.cpu() for t in run())      # (once: the unfused scatter adds a repeated point's rows with float atomics)
        print(f"FieldLoss {tag}: loss {float(loss):.9g} (float64 {float(ref['loss']):.9g})")
        check_sums(PROF, f"FieldLoss {tag} loss", loss, ref["loss"].reshape(1), ref["loss_m"].reshape(1), rule["e_loss"], rule["rel_loss"],
                   extra=2 * U * abs(float(ref["loss"])))
        check_elementwise(PROF, f"FieldLoss {tag} grad", grad, ref["grad"], ref["grad_m"], 4.0 * rule["u_grad"], rule["u_grad"],
                          extra_abs=FLUSH)


def test_field_loss_point_lists_do_not_depend_on_the_mask(monkeypatch):
    """Thresholding and random.sample never read the mask: on the golden FieldLoss inputs (a tensor loss) the uint8 map and its
    one-hot mask give identical point lists for equal seeds, on the unfused path, and finite losses."""
    from muscle_amd import edge
    from test_oracle_golden import field_unit_inputs
    _, seg, ft, mask, lwb, kk, step = field_unit_inputs()
    label = mask.argmax(1).to(torch.uint8).contiguous()
    seen = []
    real = edge._FieldLossFn

    class Spy:
        @staticmethod
        def apply(dense, plan):
            seen.append(plan)
            return real.apply(dense, plan)
    monkeypatch.setattr(edge, "_FieldLossFn", Spy)
    crit = edge.FieldLoss(sobel_size=5, beta=1e2, k=kk)
    for m in (label, LR.onehot_mask(label, seg.shape[1])):
        random.seed(77)
        loss, _ = crit(seg.to(DEV), ft.to(DEV), m.to(DEV), lwb.to(DEV), step)
        assert torch.is_tensor(loss) and np.isfinite(float(loss))
    a, b = seen
    assert a.get("label") is not None and a["mask"] is None and b.get("label") is None
    assert a["S"] == b["S"] and all(torch.equal(x, y) for x, y in zip(a["pts"], b["pts"]))


# ---- step level -------------------------------------------------------------------------------------------------------------------
def _label_batch(n, S, all_ignored=False):
    gen = torch.Generator().manual_seed(R.case_seed(n, S, 61))
    lab = torch.zeros(n, 20)
    mask = torch.zeros(n, S, S, dtype=torch.uint8)
    yy, xx = torch.meshgrid(torch.arange(S), torch.arange(S), indexing="ij")
    for i in range(n):
        c = 3 + 4 * i
        lab[i, c - 1] = 1
        mask[i][(yy - S // 2 + 5 * i) ** 2 + (xx - S // 3) ** 2 < (S // 4) ** 2] = c
        mask[i, :, S - 9:] = 255                                      # padding on the right, as a placed window leaves it
    if all_ignored:
        mask[:] = 255
    return {"img": torch.randn(n, 3, S, S, generator=gen).to(DEV), "label": lab.to(DEV), "mask": mask.to(DEV)}


def _step(batch, lamb, replay):
    import muscle_amd
    torch.manual_seed(0)
    model = muscle_amd.MuSCLe(21, "efficientnet-b0", layers=3, last_pooling=True, mode="dec").to(DEV)
    opt = muscle_amd.FusedAdam(model.parameters(), lr=1e-4, weight_decay=1e-5)
    crit = muscle_amd.edge.FieldLoss(sobel_size=5, beta=1e2, k=8)
    crit.replay_points = replay
    torch.manual_seed(1)                                               # the drop_connect draws
    random.seed(5)
    out = muscle_amd.muscle_step(model, opt, batch, lamb=lamb, step=7, k=8, criterion2=crit)
    torch.cuda.synchronize()
    return out, torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu()


@pytest.mark.both_arith            # exact fp32 and the split arithmetic, as tests/test_gpu_determinism.py runs its steps
def test_muscle_step_on_a_label_batch():
    """B0 decoder, crop 64, batch 2, a uint8 "mask": the step runs on the fused path with the BEACON term on replayed points (so
    mx_field_mask_label is on it), returns the same dict, and two runs from equal state give equal bits in the losses, the
    gradient norm and every parameter.  With every pixel 255 and lamb = 0: loss_seg == 0 and grad_norm == 0."""
    n, S = 2, 64
    gen = torch.Generator().manual_seed(R.case_seed(n, S, 62))
    replay = (torch.tensor([0, 1], dtype=torch.int32), torch.randint(0, S * S, (2, 8), generator=gen).int(),
              torch.randint(0, S * S, (2, 8), generator=gen).int())
    batch = _label_batch(n, S)
    (a, pa), (b, pb) = _step(batch, 0.05, replay), _step(batch, 0.05, replay)
    assert set(a) == {"loss_seg", "loss_beacon", "grad_norm"} and torch.is_tensor(a["loss_beacon"])
    for k in a:
        x, y = float(a[k].detach()), float(b[k].detach())
        assert np.isfinite(x) and x == y, (k, x, y)
    assert float(a["loss_seg"]) > 0 and float(a["grad_norm"]) > 0
    assert torch.equal(pa, pb)
    out, _ = _step(_label_batch(n, S, all_ignored=True), 0.0, replay)
    assert float(out["loss_seg"]) == 0.0 and float(out["grad_norm"]) == 0.0


@pytest.fixture(scope="module", autouse=True)
def _profile_file():
    yield
    PROF.write()
