"""Input path of the decoder-training loop: the reference's `VOC12SegDataset` (src/data.py:69-123) as `train_muscle.py:119-130`
uses it (`mask_type='soft'`), with the per-pixel work moved to the GPU on the host-plan / stager pattern of `muscle_amd.data`.

What the reference does per item in a DataLoader worker:
    img  = ColorJitter(0.1, 0.1, 0.1, 0.05)(PIL image)                                  torch RNG          data.py:81,105
    scale = random.uniform(min_scale, max_scale); target = (round(w*scale), round(h*scale))               imutils.py:43-46
    img  = img.resize(target, BILINEAR);  mask = skimage.transform.resize(float64 [H,W,21], target[::-1])  imutils.py:48-52
    img  = color_norm(np.asarray(img))                                                                    data.py:108
    img, mask = RandomCropWithMask(crop)(img, mask)       random.randrange: width first, then height      imutils.py:85-118
    img, mask = RandomHorizontalFlipWithMask()(img, mask) random.getrandbits(1), np.fliplr of both        imutils.py:287-292
    CHW                                                                                                   data.py:121-122
The skimage resize alone filters and warps 21 channels of the WHOLE rescaled label in float64 (up to 875 x 656 x 21 at scale
1.75) of which the crop keeps 448 x 448.

Here `plan_seg_item` makes the same draws from the same generators in the same order and computes geometry and weight tables
only; `SegStager` ships the decoded uint8 image and the source rows of the label the crop window reads (float16 as
`muscle_amd.infer_irn --soft_output 1` writes them) in ONE pinned copy per batch, and the device does the pixel work:
`mx_color_jitter` -> `mx_resample` (Pillow's bilinear, bit-exact) -> `mx_input_stage` for the image, `mx_mask_stage` for
the label.  A label may also come in its compact form (`muscle_amd.softlabel.CompactSoft`, `<name>.npz`): then the
low-resolution walk maps are shipped (47 KB per present class at 375x500 instead of up to 7.9 MB of rows) and
`mx_soft_expand` re-creates the float16 rows the window reads, bit for bit, in device scratch just before `mx_mask_stage`.

skimage.transform.resize (0.16.2, defaults order=1, mode='reflect', anti_aliasing=True, clip=True) is restated from its
published source: `scipy.ndimage.gaussian_filter(mask, sigma, mode='mirror')` with sigma = max(0, (in/out - 1)/2) per spatial
axis, then a bilinear sample at (Y + 0.5) * in/out - 0.5 with out-of-range taps mirrored about the edge pixel's centre; the
final clip is a no-op for a convex combination.  Both operators are separable and linear, so per axis they fold into one row
of 2 + 2 * radius weights per output coordinate (`mask_axis_table`).  skimage is not installed where this was built: the
tables are pinned against scipy.ndimage (tests/segdata_ref.py), not against skimage itself.

mask_type="label" (ours; the reference's unused 'hard' branch pads with class 0 and has no ignore index) trains on hard label
maps instead - PNGs with one class index per pixel, 255 = ignore: what `infer_irn --soft_output 0` and `infer_seg --out_seg`
write and what SegmentationClass[Aug] holds.  `plan_label_item` makes the same draws, the resize is Pillow's NEAREST as one
int32 source index per window row and column (`nearest_axis_table`), the shipped rows are bytes, and `mx_label_stage` writes a
uint8 [n,S,S] container padded with 255 - which `edge.cross_entropy_label` and `edge.FieldLoss` take as it is.
"""
from __future__ import annotations

import os
import random
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import call, stream
from ._stage import StageBuffer, input_stage_job, jitter_job, resample_job
from .data import _keep, color_jitter_params, random_crop_box, resample_tables
from .edge import IGNORE_LABEL
from .softlabel import CompactSoft, expand_job, load_compact, pack_compact

JITTER = (0.1, 0.1, 0.1, 0.05)          # src/data.py:81


def _mirror(i, n: int):
    """scipy.ndimage's 'mirror' (skimage's 'reflect'): reflection about the centre of the edge pixels, period 2n - 2."""
    if n == 1:
        return np.zeros_like(i)
    p = 2 * n - 2
    i = np.abs(i) % p
    return np.where(i >= n, p - i, i)


def mask_axis_table(n_in: int, n_out: int, lo: int = 0, cnt: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    """One axis of skimage.transform.resize(order=1, mode='reflect', anti_aliasing=True) for the output coordinates
    lo .. lo + cnt - 1 of n_out, as (start int32 [cnt], weights float64 [cnt, K]):
        out[lo + t] = sum_j weights[t, j] * in[start[t] + j],   0 <= start[t], start[t] + K <= n_in.
    K = min(n_in, 2 + 2 * radius): the two bilinear taps, each widened by scipy's Gaussian window (truncate 4.0), the mirror
    boundary of both folded in.  start is non-decreasing."""
    cnt = n_out - lo if cnt is None else cnt
    factor = n_in / n_out
    sigma = max(0.0, (factor - 1.0) / 2.0)
    if sigma > 1e-15:                                       # scipy.ndimage.gaussian_filter skips an axis below that
        radius = int(4.0 * sigma + 0.5)
        x = np.arange(-radius, radius + 1, dtype=np.float64)
        phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
        phi = phi / phi.sum()
    else:
        radius, phi = 0, np.ones(1)
    r = (np.arange(lo, lo + cnt, dtype=np.float64) + 0.5) * factor - 0.5
    f = np.floor(r)
    t = r - f
    f = f.astype(np.int64)
    k = np.arange(-radius, radius + 1, dtype=np.int64)
    # tap b of the bilinear sample reads the filtered signal at mirror(f + b), which is sum_k phi[k] * in[mirror(. + k)]
    idx = np.concatenate([_mirror(_mirror(f + b, n_in)[:, None] + k[None, :], n_in) for b in (0, 1)], axis=1)
    wgt = np.concatenate([(1.0 - t)[:, None] * phi[None, :], t[:, None] * phi[None, :]], axis=1)
    K = min(n_in, 2 + 2 * radius)
    start = np.clip(np.minimum(idx.min(axis=1), n_in - K), 0, None)
    rel = idx - start[:, None]
    if rel.min() < 0 or rel.max() >= K:
        raise AssertionError("mask_axis_table: taps outside their window")
    start = np.maximum.accumulate(start)                    # (already monotone; states the contract)
    w = np.zeros((cnt, K), dtype=np.float64)
    np.add.at(w, (np.repeat(np.arange(cnt), idx.shape[1]), rel.reshape(-1)), wgt.reshape(-1))
    return start.astype(np.int32), w


class SegItemPlan:
    """Sources + geometry of one decoder-training item, ready for `SegStager`."""
    __slots__ = ("img_u8", "jitter", "scale", "resize_to", "tables", "img_crop", "place", "flip",
                 "mask_src", "mask_y", "mask_x", "span_cap", "compact", "mask_rows")
    # img_u8: the ORIGINAL decoded image [h,w,3]; jitter: ColorJitter parameters or None; resize_to: (W, H) of the rescale;
    # tables: Pillow's bilinear coefficient tables for it; img_crop = (top, left, ch, cw): RandomCropWithMask's window inside
    # the rescaled image / label; place = (top, left) of the window inside the [crop, crop] container; flip: fliplr of the
    # containers; mask_src: the source rows [r0:r1] of the label the window reads (float16 / float32, [rows, W, C]);
    # mask_y / mask_x = (start, weights float32) of mask_axis_table for the window, start_y relative to r0;
    # span_cap: the longest run of source columns 64 neighbouring window columns read;
    # mask_rows = (r0, r1); compact: the CompactSoft the rows are expanded from on the device (mask_src is None then), or None.

    @property
    def channels(self) -> int:
        return self.compact.channels if self.compact is not None else self.mask_src.shape[2]


def plan_seg_item(pil_img, soft_mask, min_scale: float = 0.5, max_scale: float = 1.5, crop_size: int = 448,
                  augment: bool = True) -> SegItemPlan:
    """Host side of VOC12SegDataset.__getitem__ (src/data.py:104-112) for one decoded RGB image and its soft label [H,W,C]:
    the draws in the reference's order - ColorJitter parameters (torch), scale (random.uniform), crop box (random.randrange,
    width then height), flip (random.getrandbits) - and the tables of both resizes.  No pixel is touched.
    augment=False leaves the ColorJitter (and its draws) out; scale, crop and flip stay.
    soft_mask may be a `softlabel.CompactSoft`: the same draws and tables from its `size`; no rows are cut on the host."""
    compact = soft_mask if isinstance(soft_mask, CompactSoft) else None
    if compact is None and soft_mask.ndim != 3:
        raise ValueError(f"soft mask must be [H,W,C] (got {soft_mask.shape})")
    p = SegItemPlan()
    _plan_image(p, pil_img, min_scale, max_scale, crop_size, augment)
    (tw, th), (it, il, ch, cw) = p.resize_to, p.img_crop
    hm, wm = compact.size if compact is not None else soft_mask.shape[:2]
    sy, wy = mask_axis_table(hm, th, it, ch)
    sx, wx = mask_axis_table(wm, tw, il, cw)
    r0, r1 = int(sy.min()), int(sy.max()) + wy.shape[1]
    p.compact, p.mask_rows = compact, (r0, r1)
    if compact is not None:
        p.mask_src = None
    else:
        src = soft_mask[r0:r1]
        if src.dtype not in (np.float16, np.float32):       # float64 files: rounded to fp32 (6e-8 relative)
            src = src.astype(np.float32)
        p.mask_src = np.ascontiguousarray(src)
    p.mask_y, p.mask_x = (sy - r0, wy.astype(np.float32)), (sx, wx.astype(np.float32))
    p.span_cap = int((sx[np.minimum(np.arange(cw) + 63, cw - 1)] + wx.shape[1] - sx).max())
    return p


def nearest_axis_table(n_in: int, n_out: int, lo: int = 0, cnt: Optional[int] = None) -> np.ndarray:
    """One axis of `PIL.Image.resize(.., NEAREST)`: the int32 source index of the output coordinates lo .. lo + cnt - 1 of
    n_out.  Pillow (ImagingScaleAffine) steps a double through the axis - xo = 0.5 * a, index = int(xo), xo += a with
    a = n_in / n_out - and the rounding of that running sum is part of the result, so the sum is accumulated here in the
    same order (np.cumsum adds sequentially); the closed form floor((x + 0.5) * a) differs from it for some sizes.  A
    window is a slice of the whole axis: the sum always starts at coordinate 0."""
    cnt = n_out - lo if cnt is None else cnt
    if n_in < 1 or n_out < 1 or lo < 0 or cnt < 0 or lo + cnt > n_out:
        raise ValueError(f"nearest_axis_table: bad extents n_in={n_in} n_out={n_out} lo={lo} cnt={cnt}")
    a = float(n_in) / float(n_out)
    steps = np.full(lo + cnt, a, dtype=np.float64)
    steps[0] = a * 0.5 + 0.0
    idx = np.cumsum(steps)[lo:].astype(np.int64)            # xo >= 0: truncation is floor
    return np.minimum(idx, n_in - 1).astype(np.int32)       # (Pillow skips an index past the end; none occurs for a pure scale)


class LabelItemPlan:
    """Sources + geometry of one decoder-training item whose label is a hard label map (mask_type="label")."""
    __slots__ = ("img_u8", "jitter", "scale", "resize_to", "tables", "img_crop", "place", "flip",
                 "label_src", "label_y", "label_x", "label_rows")
    # the image fields are SegItemPlan's; label_src: the source rows [r0:r1] of the uint8 label map the window reads ([rows, W]);
    # label_y / label_x: nearest_axis_table of the window's rows (relative to r0) / columns; label_rows = (r0, r1).


def _plan_image(p, pil_img, min_scale: float, max_scale: float, crop_size: int, augment: bool):
    """The draws of an item in the reference's order and the image half of its plan (shared by both kinds of label)."""
    w, h = pil_img.size
    p.jitter = color_jitter_params(*JITTER) if augment else None
    p.scale = random.uniform(min_scale, max_scale)
    tw, th = round(w * p.scale), round(h * p.scale)
    if tw < 1 or th < 1:
        raise ValueError(f"scale {p.scale} leaves nothing of a {w}x{h} image")
    p.resize_to = (tw, th)
    ct, cl, it, il, ch, cw = random_crop_box(th, tw, crop_size)
    p.flip = bool(random.getrandbits(1))
    p.img_crop, p.place = (it, il, ch, cw), (ct, cl)
    p.img_u8 = np.ascontiguousarray(np.asarray(pil_img))
    p.tables = resample_tables(w, h, tw, th, "bilinear")


def plan_label_item(pil_img, label, min_scale: float = 0.5, max_scale: float = 1.5, crop_size: int = 448,
                    augment: bool = True) -> LabelItemPlan:
    """`plan_seg_item` for a hard label map [H,W] uint8 of the image's size: the same draws from the same generators in the
    same order (so the staged image equals the soft path's for equal seeds), and per axis the source index of Pillow's
    NEAREST resize for the rows / columns of the crop window.  Only the source rows the window reads are shipped."""
    label = np.asarray(label)
    w, h = pil_img.size
    if label.ndim != 2 or label.dtype != np.uint8 or label.shape != (h, w):
        raise ValueError(f"label map must be uint8 [H,W] = [{h},{w}] (got {label.dtype} {label.shape})")
    p = LabelItemPlan()
    _plan_image(p, pil_img, min_scale, max_scale, crop_size, augment)
    (tw, th), (it, il, ch, cw) = p.resize_to, p.img_crop
    ys, xs = nearest_axis_table(h, th, it, ch), nearest_axis_table(w, tw, il, cw)
    r0, r1 = int(ys.min()), int(ys.max()) + 1
    p.label_rows, p.label_src = (r0, r1), np.ascontiguousarray(label[r0:r1])
    p.label_y, p.label_x = ys - np.int32(r0), xs
    return p


def plan_window(plan, crop_size: int) -> Tuple[int, int, int, int]:
    """(y0, x0, y1, x1), half-open: the rectangle of the [crop_size, crop_size] container of a `SegItemPlan` or `LabelItemPlan`
    that holds image, not padding - `img_crop`'s extent at `place`, mirrored when the container is flipped.  It is where a
    staged label map differs from 255, and what `crf_loss.DenseEnergyLoss` takes as an item's window."""
    (_, _, ch, cw), (ct, cl) = plan.img_crop, plan.place
    x0 = crop_size - cl - cw if plan.flip else cl
    return int(ct), int(x0), int(ct + ch), int(x0 + cw)


class SegStager:
    """Packs the sources, jobs and tables of a batch of `SegItemPlan`s into one pinned buffer (`_stage.StageBuffer`: two
    alternate, they grow to the largest batch seen), copies it once and runs the device half: mx_color_jitter (ColorJitter on
    the original image) -> mx_resample (the bilinear rescale) -> mx_input_stage (color_norm, crop container, flip, CHW,
    fp32), and mx_mask_stage for the label; in front of it ONE mx_soft_expand for the items whose label is compact: their
    walk maps travel in the copy, the float16 rows of their windows are written into device scratch and the item's mask job
    points there.  Dense and compact items may share a batch.
    Returns {"img" [n,3,S,S], "mask" [n,C,S,S]} (+ "label" [n,20]) on the device: the batch `muscle_step` takes.
    A batch of `LabelItemPlan`s (hard label maps) runs the same image half and ONE mx_label_stage instead of the mask
    kernels: "mask" is then uint8 [n,S,S] with 255 outside the window.  The two kinds of plan cannot share a batch.
    windows=True adds "window" (int32 [n,4], `plan_window` per item) to the dict, in a small copy of its own; the staging
    buffer, the launches and the other tensors are the same either way."""

    def __init__(self, device, batch: int, crop_size: int = 448, windows: bool = False):
        self.dev, self.n, self.crop, self.windows = device, batch, crop_size, windows
        self.buf = StageBuffer(device)

    @property
    def last_bytes(self) -> int:
        return self.buf.last_bytes

    @staticmethod
    def is_label_batch(plans) -> bool:
        """True for a batch of `LabelItemPlan`s, False for one of `SegItemPlan`s; a batch that mixes the two is refused."""
        kinds = {isinstance(p, LabelItemPlan) for p in plans}
        if len(kinds) > 1:
            raise ValueError("soft-label plans and label-map plans cannot share a batch")
        return kinds == {True}

    def layout(self, plans: Sequence[SegItemPlan]) -> dict:
        """Plans the staging buffer of a batch (no packing, no GPU): byte offsets of every region.
        [image jobs | jitter jobs | resample jobs | mask jobs | expand jobs | tables | images | labels]; behind it, on the
        device only: [rescaled images | horizontal-pass temporaries | the jitter's sums | expanded label rows].
        "msk": per item the shipped label bytes - the source rows of a dense label, rw then keys (K*h*w*4 + K bytes) of a
        compact one; "exp": per compact item the scratch region of its (r1-r0) x W x channels float16 rows, else None.
        A batch of label maps has the same regions: "mj" holds the label jobs, "mtab" the two int32 index rows per item and
        "msk" the shipped uint8 rows (bytes: no alignment)."""
        n, sb = len(plans), self.buf
        label = self.is_label_batch(plans)
        nc = 0 if label else sum(p.compact is not None for p in plans)
        sb.plan()
        L = {"jobs": sb.reserve(n * 48, 64), "jit": sb.reserve(n * 32, 64), "rs": sb.reserve(n * 32, 64), "mj": sb.reserve(n * 64, 64)}
        L["sj"] = sb.reserve(nc * 64, 64) if nc else None
        L["tab"] = [sb.reserve(p.tables.nbytes) for p in plans]
        if label:
            L["mtab"] = [[sb.reserve(t.nbytes) for t in (p.label_y, p.label_x)] for p in plans]
        else:
            L["mtab"] = [[sb.reserve(s.nbytes + w.nbytes) for s, w in (p.mask_y, p.mask_x)] for p in plans]
        L["img"] = [sb.reserve(p.img_u8.size) for p in plans]
        if label:
            L["msk"] = [sb.reserve(p.label_src.nbytes, 1) for p in plans]
        else:
            L["msk"] = [sb.reserve(p.compact.nbytes if p.compact is not None else p.mask_src.nbytes) for p in plans]
        L["rsz"] = [sb.scratch(p.resize_to[0] * p.resize_to[1] * 3) for p in plans]
        L["tmp"] = [sb.scratch(p.img_u8.shape[0] * p.resize_to[0] * 3) for p in plans]
        L["sums"] = sb.scratch(n * 8)
        L["exp"] = [None if label or p.compact is None else
                    sb.scratch((p.mask_rows[1] - p.mask_rows[0]) * p.compact.size[1] * p.compact.channels * 2) for p in plans]
        return L

    def __call__(self, plans: Sequence[SegItemPlan], labels: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        n, S, sb = len(plans), self.crop, self.buf
        assert 0 < n <= self.n
        label = self.is_label_batch(plans)
        if not label:
            C = plans[0].channels
            if any(p.channels != C for p in plans):
                raise ValueError("every soft mask of a batch must have the same number of channels")
        L = self.layout(plans)
        o_jobs, o_jit, o_rs, o_mj, o_sj, o_sums = L["jobs"], L["jit"], L["rs"], L["mj"], L["sj"], L["sums"]
        tab_at, mtab_at, img_at, msk_at, rs_at, tmp_at, exp_at = L["tab"], L["mtab"], L["img"], L["msk"], L["rsz"], L["tmp"], L["exp"]
        buf = sb.begin()
        jobs = buf[o_jobs:o_jobs + n * 48].view(np.int32).reshape(n, 12)
        jit = buf[o_jit:o_jit + n * 32].view(np.int32).reshape(n, 8)
        rsj = buf[o_rs:o_rs + n * 32].view(np.int32).reshape(n, 8)
        mj = buf[o_mj:o_mj + n * 64].view(np.int32).reshape(n, 16)
        any_jit, jit_px, rs_px, span_cap, nc = False, 1, 1, 1, 0
        for i, p in enumerate(plans):
            h, w = p.img_u8.shape[:2]
            tw, th = p.resize_to
            it, il, ch, cw = p.img_crop
            buf[img_at[i]:img_at[i] + p.img_u8.size] = p.img_u8.reshape(-1)
            buf[tab_at[i]:tab_at[i] + p.tables.nbytes] = p.tables.view(np.uint8)
            rsj[i] = resample_job(img_at[i], h, w, tmp_at[i], rs_at[i], tw, th, tab_at[i])
            rs_px = max(rs_px, h * tw, th * tw)
            jobs[i] = input_stage_job(rs_at[i] + (it * tw + il) * 3, tw, p.place[0], p.place[1], ch, cw,
                                      flip_width=S if p.flip else None)
            jit[i] = jitter_job(img_at[i], h, w, p.jitter)
            if p.jitter is not None:
                any_jit, jit_px = True, max(jit_px, h * w)
            if label:                                       # mx_label_stage's job: uint8 rows and one int32 index row per axis
                m = p.label_src
                buf[msk_at[i]:msk_at[i] + m.nbytes] = m.reshape(-1)
                for o, t in zip(mtab_at[i], (p.label_y, p.label_x)):
                    buf[o:o + t.nbytes] = np.ascontiguousarray(t, dtype=np.int32).view(np.uint8)
                mj[i] = (msk_at[i], m.shape[0], m.shape[1], p.place[0], p.place[1], ch, cw, int(p.flip),
                         mtab_at[i][0] // 4, mtab_at[i][1] // 4, 0, 0, 0, 0, 0, 0)
                continue
            if p.compact is not None:                       # the rows come out of mx_soft_expand: float16, in scratch
                pack_compact(buf, msk_at[i], p.compact)
                buf[o_sj + nc * 64:o_sj + nc * 64 + 64].view(np.int32)[:] = expand_job(p.compact, msk_at[i], exp_at[i], p.mask_rows)
                nc += 1
                m_off, m_rows, m_cols, m_f32 = exp_at[i], p.mask_rows[1] - p.mask_rows[0], p.compact.size[1], 0
            else:
                m = p.mask_src
                buf[msk_at[i]:msk_at[i] + m.nbytes] = m.reshape(-1).view(np.uint8)
                m_off, m_rows, m_cols, m_f32 = msk_at[i], m.shape[0], m.shape[1], int(m.dtype == np.float32)
            for o, (start, wgt) in zip(mtab_at[i], (p.mask_y, p.mask_x)):
                buf[o:o + start.nbytes] = np.ascontiguousarray(start).view(np.uint8)
                buf[o + start.nbytes:o + start.nbytes + wgt.nbytes] = np.ascontiguousarray(wgt).reshape(-1).view(np.uint8)
            mj[i] = (m_off, m_rows, m_cols, m_f32, p.place[0], p.place[1], ch, cw,
                     int(p.flip), p.mask_y[1].shape[1], p.mask_x[1].shape[1], mtab_at[i][0] // 4, mtab_at[i][1] // 4, 0, 0, 0)
            span_cap = max(span_cap, p.span_cap)
        base, st = sb.upload(), stream()
        if any_jit:
            call("mx_color_jitter", base, base + o_jit, base + o_sums, n, int(jit_px), st)
        call("mx_resample", base, base + o_rs, base, base, base, n, int(rs_px), st)
        img = torch.empty(n, 3, S, S, dtype=torch.float32, device=self.dev)
        call("mx_input_stage", base, base + o_jobs, img.data_ptr(), n, S, S, st)
        if label:
            mask = torch.empty(n, S, S, dtype=torch.uint8, device=self.dev)
            call("mx_label_stage", base, base + o_mj, base, mask.data_ptr(), n, S, IGNORE_LABEL, st)
        else:
            mask = torch.empty(n, C, S, S, dtype=torch.float32, device=self.dev)
            if nc:
                call("mx_soft_expand", base, base + o_sj, nc, st)
            call("mx_mask_stage", base, base + o_mj, base, mask.data_ptr(), n, C, S, int(span_cap), st)
        out = {"img": img, "mask": mask}
        if self.windows:
            out["window"] = torch.tensor([plan_window(p, S) for p in plans], dtype=torch.int32).to(self.dev, non_blocking=True)
        if labels is not None:
            out["label"] = labels.to(self.dev, non_blocking=True)
        return out


MASK_FORMATS = ("auto", "dense", "compact")


class VOC12SegDataset:
    """The reference dataset's role (src/data.py:69-123, `inference=False`): `plan(idx)` is the host half of `__getitem__`
    (JPEG decode, np.load of the soft label, the draws, the tables); a batch of plans goes through a `SegStager`.
    Reads `<mask_root>/<name>.npy` as `muscle_amd.infer_irn --soft_output 1` writes it (float16 [H,W,21]); float32 files
    are shipped as they are and float64 files rounded to float32.  mask_format: "dense" reads that file, "compact" reads
    `<mask_root>/<name>.npz` as `infer_irn --soft_output 2` writes it (muscle_amd/softlabel.py), "auto" takes the .npy when it
    exists - a tree of dense files behaves as it always did - and the .npz otherwise.  mask_type='hard' (PNG labels; train_muscle.py does not use
    it) is refused.
    mask_type="label" (ours; not the reference's 'hard', which pads with class 0 and has no ignore index): reads
    `<mask_root>/<name>.png`, a single-channel 8-bit label map (Pillow mode L or P) of the image's size whose values are
    below num_classes or 255 (ignore) - what `infer_irn --soft_output 0` and `infer_seg --out_seg` write and what
    SegmentationClass[Aug] holds; anything else is a ValueError naming the file, raised in `plan`.  `plan` then returns a
    `LabelItemPlan` (NEAREST resize, container filled with 255); mask_format is ignored."""

    def __init__(self, img_name_list_path: str, voc12_root: str, mask_root: str, min_scale: float = 0.5, max_scale: float = 1.5,
                 crop_size: int = 448, mask_type: str = "soft", labels: Optional[Dict[str, np.ndarray]] = None,
                 augment: bool = True, mask_format: str = "auto", num_classes: int = 21):
        if mask_format not in MASK_FORMATS:
            raise ValueError(f"mask_format must be one of {MASK_FORMATS} (got {mask_format!r})")
        if mask_type not in ("soft", "label"):
            raise NotImplementedError(f"mask_type={mask_type!r}: only the soft pseudo-labels train_muscle.py trains on "
                                      "(mask_type='soft', <name>.npy) and label maps with an ignore index "
                                      "(mask_type='label', <name>.png) are built on the HIP path")
        if not 1 < num_classes <= IGNORE_LABEL:
            raise ValueError(f"num_classes must be in 2..{IGNORE_LABEL} (got {num_classes})")
        self.mask_type, self.num_classes = mask_type, num_classes
        self.names = [ln.split(" ")[0].split("/")[-1].split(".")[0] for ln in open(img_name_list_path).read().splitlines()]
        self.root, self.mask_root, self.crop = voc12_root, mask_root, crop_size
        self.min_scale, self.max_scale, self.augment, self.mask_format = min_scale, max_scale, augment, mask_format
        if labels is None and os.path.exists("data/cls_labels.npy"):
            labels = np.load("data/cls_labels.npy", allow_pickle=True).item()          # src/data.py:53-56
        self.labels = labels

    def __len__(self):
        return len(self.names)

    def load_mask(self, name: str):
        """The soft label of `name`: the dense array or a CompactSoft, as mask_format says.  A missing file raises."""
        dense = os.path.join(self.mask_root, name + ".npy")
        if self.mask_format == "dense" or (self.mask_format == "auto" and os.path.exists(dense)):
            return np.load(dense, allow_pickle=True)
        return load_compact(os.path.join(self.mask_root, name + ".npz"))

    def load_label_map(self, name: str, size: Tuple[int, int]) -> np.ndarray:
        """The label map of `name` as uint8 [H,W], checked: mode L or P, `size` = (W, H) of the image, every value below
        num_classes or 255.  A file that fails a check raises ValueError with its path."""
        import PIL.Image
        path = os.path.join(self.mask_root, name + ".png")
        with PIL.Image.open(path) as im:
            if im.mode not in ("L", "P"):
                raise ValueError(f"{path}: a label map must be a single-channel 8-bit image (mode L or P), got mode {im.mode}")
            if im.size != tuple(size):
                raise ValueError(f"{path}: label map of {im.size[0]}x{im.size[1]} for an image of {size[0]}x{size[1]}")
            a = np.array(im, dtype=np.uint8)
        bad = a[(a >= self.num_classes) & (a != IGNORE_LABEL)]
        if bad.size:
            raise ValueError(f"{path}: value {int(bad[0])} is neither a class below {self.num_classes} nor {IGNORE_LABEL} (ignore)")
        return a

    def plan(self, idx: int) -> Tuple[str, SegItemPlan, Optional[np.ndarray]]:
        import PIL.Image
        name = self.names[idx]
        img = PIL.Image.open(os.path.join(self.root, "JPEGImages", name + ".jpg")).convert("RGB")
        lab = None if self.labels is None else np.asarray(self.labels[name], dtype=np.float32)
        if self.mask_type == "label":
            lmap = self.load_label_map(name, img.size)
            return name, plan_label_item(img, lmap, self.min_scale, self.max_scale, self.crop, self.augment), lab
        mask = self.load_mask(name)
        return name, plan_seg_item(img, mask, self.min_scale, self.max_scale, self.crop, self.augment), lab

    __getitem__ = plan          # a torch.utils.data map-style dataset: DataLoader workers run the host half


class SegLoader:
    """The reference's `DataLoader(train_dataset, batch_size, num_workers, pin_memory=True, drop_last=True, shuffle=True,
    prefetch_factor=4)` (train_muscle.py:128-130) for this input path: torch's DataLoader runs `VOC12SegDataset.plan` in
    its worker processes with torch's own per-worker seeding of `torch` / `random` (base seed + worker id, as in the
    reference), and each batch of plans goes through the `SegStager` in the training process.
    Iterating yields `(names, batch)`, `batch` being the dict `muscle_step` takes."""

    def __init__(self, dataset: VOC12SegDataset, batch_size: int, device, num_workers: int = 0, shuffle: bool = True,
                 drop_last: bool = True, generator=None, prefetch_factor: int = 4, windows: bool = False):
        from torch.utils.data import DataLoader
        self.dataset, self.stager = dataset, SegStager(device, batch_size, dataset.crop, windows=windows)
        self.loader = DataLoader(dataset, batch_size=batch_size, shuffle=shuffle, num_workers=num_workers, drop_last=drop_last,
                                 collate_fn=_keep, generator=generator, persistent_workers=bool(num_workers),
                                 prefetch_factor=prefetch_factor if num_workers else None)

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for items in self.loader:
            labels = None
            if items[0][2] is not None:
                labels = torch.from_numpy(np.stack([it[2] for it in items]))
            yield [it[0] for it in items], self.stager([it[1] for it in items], labels=labels)
