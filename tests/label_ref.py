"""Restatements of the hard-label-map path (mask_type="label": muscle_amd.segdata.plan_label_item / mx_label_stage, mx_ce_label,
mx_field_mask_label) in numpy, PIL and torch on the CPU, for tests/test_cpu_label_path.py and tests/test_gpu_label_path.py.
The conventions are those of tests/dec_ref.py (float64 reference, the same expressions at float32 as the "plain fp32
restatement", magnitudes for the tolerance rules) and of tests/segdata_ref.py (the draws as a dict)."""
import functools

import numpy as np
import torch

import dec_ref as R
from dec_ref import F32, F64

IGNORE = 255


# ---- the input stage --------------------------------------------------------------------------------------------------------------
def pil_nearest_axis(n_in, n_out):
    """The source index of every output coordinate of one axis, read off Pillow itself: a 1 x n_in ramp of mode I resized
    with NEAREST."""
    from PIL import Image
    ramp = Image.fromarray(np.arange(n_in, dtype=np.int32)[None, :])
    assert ramp.mode == "I"
    return np.asarray(ramp.resize((n_out, 1), Image.NEAREST))[0].astype(np.int32)


def ref_label(label, d, crop, fill=IGNORE):
    """Pillow resize (NEAREST) -> crop -> container filled with `fill` -> flip, done directly; d: the draws (segdata_ref)."""
    from PIL import Image
    tw, th = d["target"]
    a = np.asarray(Image.fromarray(label).resize((tw, th), Image.NEAREST))
    (it, il, ch, cw), (ct, cl) = d["img_crop"], d["place"]
    out = np.full((crop, crop), fill, np.uint8)
    out[ct:ct + ch, cl:cl + cw] = a[it:it + ch, il:il + cw]
    return np.fliplr(out).copy() if d["flip"] else out


def label_stage(src, sh, sw, ys, xs, top, left, flip, S, fill):
    """What mx_label_stage writes for one item: src = the shipped rows as a flat uint8 array of sh * sw bytes."""
    rows = np.asarray(src, np.uint8).reshape(sh, sw)
    out = np.full((S, S), fill, np.uint8)
    out[top:top + len(ys), left:left + len(xs)] = rows[np.asarray(ys)[:, None], np.asarray(xs)[None, :]]
    return np.fliplr(out).copy() if flip else out


def plan_label_cpu(p, crop, fill=IGNORE):
    """label_stage on a LabelItemPlan."""
    m = p.label_src
    return label_stage(m.reshape(-1), m.shape[0], m.shape[1], p.label_y, p.label_x, p.place[0], p.place[1], p.flip, crop, fill)


def synth_label_map(H, W, seed, K=21, ignore_share=0.1):
    """A label map [H,W] uint8: blocks of classes 0..K-1 with a band and scattered pixels of 255."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    a = ((yy // 5) * 7 + (xx // 3) * 3 + rng.integers(0, 2, (H, W))) % K
    a[rng.uniform(size=(H, W)) < ignore_share] = IGNORE
    return a.astype(np.uint8)


# ---- cross entropy with an ignore index ---------------------------------------------------------------------------------------
def _valid(label, K, ignore=IGNORE):
    return (label != ignore) & (label < K)


def ce_label(seg, label, dtype=F64, ignore=IGNORE):
    """seg [N,K,HW], label [N,HW] uint8.  (sum of the valid pixels' terms / count, the same mean of |max| + |log sum exp| +
    |seg_t|, count).  No valid pixel: (0, 0, 0)."""
    K = seg.shape[1]
    v = _valid(label, K, ignore)
    cnt = int(v.sum())
    if cnt == 0:
        return torch.zeros((), dtype=dtype), torch.zeros((), dtype=F64), 0
    s = seg.to(dtype)
    mx = s.max(1).values
    lse = mx + torch.log(torch.exp(s - mx[:, None]).sum(1))
    t = torch.where(v, label.long(), torch.zeros_like(label, dtype=torch.long))
    st = s.gather(1, t[:, None]).squeeze(1)
    term, mag = (lse - st)[v], (mx.abs() + (lse - mx).abs() + st.abs()).double()[v]
    return term.sum() / cnt, mag.sum() / cnt, cnt


def ce_label_bwd(seg, label, gup, dtype=F64, ignore=IGNORE):
    """gup * (softmax - onehot) / count at valid pixels, 0 elsewhere; magnitude gup * (softmax + onehot) / count."""
    K = seg.shape[1]
    v = _valid(label, K, ignore)
    cnt = int(v.sum())
    s = seg.to(dtype)
    if cnt == 0:
        return torch.zeros_like(s), torch.zeros_like(s)
    mx = s.max(1, keepdim=True).values
    lse = mx + torch.log(torch.exp(s - mx).sum(1, keepdim=True))
    p = torch.exp(s - lse)
    t = torch.where(v, label.long(), torch.zeros_like(label, dtype=torch.long))
    oh = torch.zeros_like(p).scatter_(1, t[:, None], 1.0)
    g = torch.tensor(gup, dtype=dtype) * (torch.tensor(1.0, dtype=dtype) / cnt)
    keep = v[:, None].to(dtype)
    return g * (p - oh) * keep, g.abs() * (p + oh) * keep


CE_IGNORE_MODES = ["third", "one", "none"]


def ignore_pattern(shape, mode):
    """Boolean [N,HW], True = ignored: about a third of the pixels (whole runs and single pixels), all but one, or all."""
    N, _, HW = shape
    if mode == "none":
        return torch.ones(N, HW, dtype=torch.bool)
    if mode == "one":
        ig = torch.ones(N, HW, dtype=torch.bool)
        ig[N - 1, (HW * 2) // 3] = False
        return ig
    gen = torch.Generator().manual_seed(R.case_seed(N, HW, 31))
    ig = torch.rand(N, HW, generator=gen) < 0.2
    i = torch.arange(HW)
    ig = ig | ((i % 97) < 13)[None, :]             # plus runs of 13 in every 97: about a third in all
    ig[:, HW // 2] = False                         # (a shape of one pixel keeps it)
    return ig


def ce_label_inputs(shape, kind, mode="third"):
    """(seg, label): the logits of dec_ref.ce_inputs and the arg-max of its mask as the label, with `mode`'s pixels set to
    255.  In the "third" mode every tenth ignored pixel holds a value in K..254 instead: ignored by the contract too."""
    seg, mask = R.ce_inputs(shape, kind)
    K = shape[1]
    label = torch.from_numpy(np.argmax(mask.numpy(), axis=1)).to(torch.uint8)
    ig = ignore_pattern(shape, mode)
    label[ig] = IGNORE
    if mode == "third":
        odd = ig & ((torch.arange(shape[2]) % 10) == 3)[None, :]
        label[odd] = min(K + 5, 254)
    return seg, label.contiguous()


def ce_label_rule(seg, label):
    """(reference, magnitude, e_ref, allowance, count) of the sum rule, the magnitude taken over the valid pixels."""
    ref, mag, cnt = ce_label(seg, label)
    if cnt == 0:
        return ref, mag, 0.0, 2.0 * R.U, 0
    e_ref = abs(float(ce_label(seg, label, F32)[0]) - float(ref)) / float(mag)
    return ref, mag, e_ref, 4.0 * e_ref + 2.0 * R.U, cnt


def ce_label_exact_inputs(shape, mode="third"):
    """The exact regime of dec_ref.ce_exact_inputs with ignored pixels mixed in: every valid pixel's term is the integer d in
    20..27 its logits were built from, every partial sum is exact, and the loss is float32(sum d / count).
    Returns (seg, label, the expected loss as a float32 tensor [1] - 0 when nothing is valid)."""
    seg, mask, _ = R.ce_exact_inputs(shape)
    K = shape[1]
    t = torch.from_numpy(np.argmax(mask.numpy(), axis=1))
    d = (seg.gather(1, ((t + 1) % K)[:, None]) - seg.gather(1, t[:, None])).squeeze(1).double()
    assert bool((d == d.round()).all()) and float(d.min()) >= 20 and float(d.max()) <= 27
    label = t.to(torch.uint8)
    ig = ignore_pattern(shape, mode)
    label[ig] = IGNORE
    cnt = int((~ig).sum())
    want = np.float32(np.float64(float(d[~ig].sum())) / np.float64(cnt)) if cnt else np.float32(0.0)
    return seg, label.contiguous(), torch.tensor([want])


# ---- FieldLoss mask rows ------------------------------------------------------------------------------------------------------
def field_mask_label(label, pts, K, ML, H, W, dtype=F64, ignore=IGNORE):
    """label [N,H,W] uint8, pts [npts,2] {n, pixel} -> [npts, ML]: softmax over the K classes of onehot(label) at a labelled
    point, of zeros (uniform 1/K) at an ignored one (255 or any value >= K), zeros in the columns from K on."""
    n, p = pts[:, 0].long(), pts[:, 1].long()
    t = label[n, p // W, p % W].long()
    v = _valid(t, K, ignore)
    oh = torch.zeros(pts.shape[0], K, dtype=dtype)
    oh[v, t[v]] = 1.0
    out = torch.zeros(pts.shape[0], ML, dtype=dtype)
    out[:, :K] = torch.softmax(oh, 1)
    return out


def mask_label_inputs(K, npts, H=24, W=24):
    """(label [2,H,W], pts): the points of dec_ref.field_points_for (corners, last row and column, repeats); the label holds
    every class, 255 on a third of the pixels - the first corner and the last pixel among them - and one value in K..254."""
    N = 2
    gen = torch.Generator().manual_seed(R.case_seed(K, npts, H, W, 41))
    label = torch.randint(0, K, (N, H, W), generator=gen).to(torch.uint8)
    label[torch.rand(N, H, W, generator=gen) < 0.33] = IGNORE
    label[:, 0, 0] = IGNORE
    label[:, H - 1, W - 1] = IGNORE
    label[:, 0, W - 1] = K - 1
    label[:, H - 1, 0] = 0
    label[:, H // 2, W - 1] = min(K + 3, 254)            # out of range: ignored, never an index
    return label.contiguous(), R.field_points_for(N, H, W, npts, gen)


@functools.lru_cache(maxsize=None)
def mask_label_calib():
    """The error of the fp32 restatement of the mask rows on a fixed draw of 1024 points at K = 21, in units of U * value."""
    label, pts = mask_label_inputs(21, 1024)
    ref = field_mask_label(label, pts, 21, 24, 24, 24)
    r32 = field_mask_label(label, pts, 21, 24, 24, 24, F32)
    return R.units(r32[:, :21], ref[:, :21], ref[:, :21])


def field_loss_ref(dense, label, pts_out, pts_in, S, k, K, ML, dtype=F64):
    """The FieldLoss downstream of its point lists, composed from dec_ref's stages, for full-resolution NCHW features `dense` and
    a label map: channel softmax at the points, the mask rows, the two k x k similarity products per slot, the eight terms
    (inv_n = 1/N), and the gradient of the dense map (through the out points only, as the HIP path and the reference have it).
    Returns a dict: loss, loss_m (the sum of the |terms| / N: the magnitude of the loss), grad, grad_m (sum |term| per element
    with |gsim| in the product that feeds the scatter, so that its cancellation counts), margins (dec_ref.field_terms)."""
    N, CH, H, W = dense.shape
    f_out = torch.softmax(R.point_values(dense, 0, pts_out, H, W, dtype)[0], 1)
    f_in = torch.softmax(R.point_values(dense, 0, pts_in, H, W, dtype)[0], 1)
    m_out, m_in = (field_mask_label(label, p, K, ML, H, W, dtype) for p in (pts_out, pts_in))
    sim = torch.bmm(f_out.view(S, k, CH), f_in.view(S, k, CH).transpose(1, 2))
    simm = torch.bmm(m_out.view(S, k, ML), m_in.view(S, k, ML).transpose(1, 2))
    t = R.field_terms(sim, simm, 1.0 / N, dtype)
    gfo = torch.bmm(t["gsim"].to(dtype), f_in.view(S, k, CH)).view(S * k, CH)
    gfo_m = torch.bmm(t["gsim"].to(dtype).abs(), f_in.view(S, k, CH)).view(S * k, CH)
    grad, _ = R.field_scatter(f_out, gfo, pts_out, 0, tuple(dense.shape), 1.0, H, W, dtype)
    _, grad_m = R.field_scatter(f_out, gfo_m, pts_out, 0, tuple(dense.shape), 1.0, H, W, dtype)
    return dict(loss=t["slot_loss"].sum(), loss_m=t["terms"].abs().sum() / N, grad=grad, grad_m=grad_m, margins=t["margins"])


FIELD_CASE = dict(N=2, K=21, CH=16, H=24, W=24, S=3, k=8)


def field_label_case():
    """The loss-level case: seg [2,21,24,24] (the 'spread' logits of dec_ref.ce_inputs), features [2,16,24,24], a label map
    without 255 (two classes per sample, the left and the right half) and three slots of k = 8 replayed points: per slot six
    out points on the left class and two on the right, two in points on the left and six on the right.  Every mask row mean is then 1/4 or 3/4 of the way between the two similarity values and the total mean at 3/8:
    the FP/FN/TP/TN decisions on the mask are clear of their margins by a sixteenth of (p_hit - p_miss)^2 = 3.6e-4, far above
    fp32 round-off; the features' margins are asserted by the tests (tests/test_cpu_label_path.py too).
    Returns (seg, dense, label, label_with_bg [2,21], (slot samples [S], out pixels [S,k], in pixels [S,k]))."""
    c = FIELD_CASE
    N, K, H, W = c["N"], c["K"], c["H"], c["W"]
    seg = R.ce_inputs((N, K, H * W), "spread")[0].view(N, K, H, W).contiguous()
    gen = torch.Generator().manual_seed(R.case_seed(N, K, H, W, 51))
    dense = (torch.randn(N, c["CH"], H, W, generator=gen) * 2.0).contiguous()
    label = torch.zeros(N, H, W, dtype=torch.uint8)
    for n, (a, b) in enumerate(((3, 0), (7, 12))):
        label[n, :, :W // 2], label[n, :, W // 2:] = a, b
    lwb = torch.zeros(N, K)
    lwb[:, 0] = 1.0
    for n in range(N):
        lwb[n, label[n].unique().long()] = 1.0

    def pick(left, cnt):
        y, x = torch.randint(0, H, (cnt,), generator=gen), torch.randint(0, W // 2, (cnt,), generator=gen)
        return (y * W + x + (0 if left else W // 2)).tolist()
    rb = torch.tensor([0, 1, 1], dtype=torch.int32)
    rout = torch.tensor([pick(True, 6) + pick(False, 2) for _ in range(3)], dtype=torch.int32)
    rin = torch.tensor([pick(True, 2) + pick(False, 6) for _ in range(3)], dtype=torch.int32)
    rout[0, 0], rin[0, 7] = 0, H * W - 1                                 # the first and the last pixel
    rout[1, 1] = rout[1, 0]                                              # a repeated point
    rout[2, 7], rin[1, 0] = 2 * W + W - 1, (H - 1) * W + 3               # the last column, the last row
    return seg, dense, label.contiguous(), lwb, (rb, rout, rin)


def replay_pts(replay, k):
    """The two [S*k, 2] int32 lists {n, pixel} FieldLoss builds from replayed points."""
    rb, rout, rin = replay
    nt = rb.repeat_interleave(k)
    return tuple(torch.stack((nt, t.reshape(-1)), 1).int().contiguous() for t in (rout, rin))


def field_label_rule():
    """Everything the loss-level FieldLoss test compares with: the float64 reference of field_label_case, the fp32 restatement's
    errors on it (loss: relative to the sum of |terms|; gradient: in units of U * sum |term|), and the allowances by the rules of
    tests/test_gpu_dec_kernels.py (sum rule for the loss, 4 x the measured error for the gradient)."""
    seg, dense, label, lwb, replay = field_label_case()
    c = FIELD_CASE
    po, pi = replay_pts(replay, c["k"])
    ref = field_loss_ref(dense, label, po, pi, c["S"], c["k"], c["K"], 24)
    r32 = field_loss_ref(dense, label, po, pi, c["S"], c["k"], c["K"], 24, F32)
    e_loss = abs(float(r32["loss"]) - float(ref["loss"])) / float(ref["loss_m"])
    u_grad = R.units(r32["grad"], ref["grad"], ref["grad_m"])
    return dict(ref=ref, e_loss=e_loss, rel_loss=4.0 * e_loss + 2.0 * R.U, u_grad=u_grad)


def onehot_mask(label, K):
    """[N,K,H,W] float32 one-hot of a label map without ignored pixels."""
    assert int(label.max()) < K
    return torch.zeros(label.shape[0], K, *label.shape[1:]).scatter_(1, label.long()[:, None], 1.0).contiguous()
