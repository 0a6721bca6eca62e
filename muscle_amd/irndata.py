"""Input path of IRN training: the reference's `VOC12AffinityDataset` (src/data.py:639-705) as `muscle_amd.train_irn` uses it,
with the per-pixel work moved to the GPU on the host-plan / stager pattern of `muscle_amd.data` and `muscle_amd.segdata`.
Opt-in: `python -m muscle_amd.train_irn --loader device`; the host loader of `train_irn.py` stays the default.

What the reference does per item in a DataLoader worker (restated in `train_irn.affinity_sample`):
    s = 0.5 + random.random()                                  one draw                                    imutils.py:72-80
    img = pil_rescale(img, s, BICUBIC); label = pil_rescale(label, s, NEAREST)    target = np.round(size * s)   imutils.py:55-69
    img = TorchvisionNormalize(img)                            float64 per channel                         data.py:596-609
    img, label = random_lr_flip((img, label))                  random.getrandbits(1), BEFORE the crop      imutils.py:163-172
    img, label = random_crop((img, label), crop, (0, 255))     random.randrange: width first, then height  imutils.py:183-233
    img CHW; label = pil_rescale(label, 0.25, NEAREST)                                                     data.py:694-697
and ships 12 bytes of float32 per pixel of the container through worker IPC.

Here `plan_irn_item` makes the same draws from the same generator in the same order and computes geometry and index tables
only; `IrnStager` ships the decoded uint8 image and label of every item in ONE pinned copy per batch, and the device does the
pixel work: `mx_resample` (Pillow's bicubic, bit-exact) for the items whose size changes, then `mx_irn_input_stage`, one
launch that writes `img [n,3,S,S]` and `label [n,S/4,S/4]`.  Both are bit-equal to `affinity_sample`.
"""
from __future__ import annotations

import os
import random
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from ._lib import call, stream
from ._stage import StageBuffer, resample_job
from .data import _keep, resample_tables
from .train_irn import random_crop_box

__all__ = ["nearest_table", "IrnItemPlan", "plan_irn_item", "plan_irn_eval_item", "IrnStager", "VOC12AffinityPlans", "IrnLoader"]


def nearest_table(n_in: int, n_out: int) -> np.ndarray:
    """The source index Pillow's NEAREST resize reads per output coordinate of one axis (int32 [n_out]).  Pillow steps an
    accumulated double through the axis - xo = 0.5 * a; idx = floor(xo); xo += a with a = n_in / n_out - and the rounding of
    that running sum is part of the result: the closed form floor((x + 0.5) * a) picks another pixel for many sizes."""
    a = float(n_in) / float(n_out)
    xo = a * 0.5 + 0.0
    idx = np.empty(n_out, dtype=np.int32)
    for x in range(n_out):
        idx[x] = int(xo)                                    # xo >= 0: truncation is floor
        xo += a
    return idx


class IrnItemPlan:
    """Sources + geometry of one IRN training item, ready for `IrnStager`."""
    __slots__ = ("img_u8", "label_u8", "scale", "size", "resize_to", "tables", "ytab", "xtab", "window", "place", "flip", "box")
    # img_u8: the ORIGINAL decoded image [h,w,3]; label_u8: the original label [h,w] (None: the eval view); size = (sh, sw) of
    # the rescaled image; resize_to: (W, H) of the bicubic rescale still to be done on the device with `tables`, or None when
    # pil_rescale returns its input (target size == source size: no resample is run); ytab / xtab: nearest_table of the
    # label's rescale; window = (img_top, img_left, ch, cw) inside the flipped rescaled image; place = (cont_top, cont_left)
    # inside the [crop, crop] container; flip: random_lr_flip's bit; box: random_crop_box's 8 values as the reference lists them.


def _check(img_u8: np.ndarray, label_u8: Optional[np.ndarray]) -> None:
    if img_u8.ndim != 3 or img_u8.shape[2] != 3 or img_u8.dtype != np.uint8:
        raise ValueError(f"the image must be uint8 [H,W,3] (got {img_u8.dtype} {img_u8.shape})")
    if label_u8 is not None and (label_u8.dtype != np.uint8 or label_u8.shape != img_u8.shape[:2]):
        raise ValueError(f"the label must be uint8 of the image's size {img_u8.shape[:2]} (got {label_u8.dtype} {label_u8.shape})")


def plan_irn_item(img_u8: np.ndarray, label_u8: np.ndarray, crop_size: int, rng=random, rescale=(0.5, 1.5)) -> IrnItemPlan:
    """Host side of `train_irn.affinity_sample` for a decoded image uint8 [H,W,3] and its label uint8 [H,W]: the draws in the
    reference's order - scale (rng.random()), flip (rng.getrandbits(1)), crop box (rng.randrange, width then height) - and
    the tables of both rescales.  No pixel is touched."""
    _check(img_u8, label_u8)
    p = IrnItemPlan()
    h, w = img_u8.shape[:2]
    p.scale = rescale[0] + rng.random() * (rescale[1] - rescale[0])
    th, tw = int(np.round(h * p.scale)), int(np.round(w * p.scale))         # pil_rescale, src/imutils.py:55-58
    if th < 1 or tw < 1:
        raise ValueError(f"scale {p.scale} leaves nothing of a {w}x{h} image")
    p.flip = bool(rng.getrandbits(1))
    p.box = random_crop_box(th, tw, crop_size, rng)
    p.size = (th, tw)
    p.place = (p.box[0], p.box[2])
    p.window = (p.box[4], p.box[6], p.box[5] - p.box[4], p.box[7] - p.box[6])
    p.img_u8, p.label_u8 = np.ascontiguousarray(img_u8), np.ascontiguousarray(label_u8)
    if (th, tw) == (h, w):                                                  # pil_rescale returns its input: nothing to resample
        p.resize_to = p.tables = None
    else:
        p.resize_to, p.tables = (tw, th), resample_tables(w, h, tw, th, "bicubic")
    p.ytab, p.xtab = nearest_table(h, th), nearest_table(w, tw)
    return p


def plan_irn_eval_item(img_u8: np.ndarray, crop_size: int) -> IrnItemPlan:
    """The eval pass's view (`train_irn.top_left_sample`): the top-left [crop, crop] of the normalised image, zero fill; no
    draw, no rescale, no flip, no label."""
    _check(img_u8, None)
    p = IrnItemPlan()
    h, w = img_u8.shape[:2]
    p.scale, p.flip, p.size, p.resize_to, p.tables = 1.0, False, (h, w), None, None
    ch, cw = min(crop_size, h), min(crop_size, w)
    p.place, p.window, p.box = (0, 0), (0, 0, ch, cw), (0, ch, 0, cw, 0, ch, 0, cw)
    p.img_u8, p.label_u8, p.ytab, p.xtab = np.ascontiguousarray(img_u8), None, None, None
    return p


class IrnStager:
    """Packs the jobs, tables and uint8 sources of a batch of `IrnItemPlan`s into one pinned buffer (`_stage.StageBuffer`: two
    alternate, they grow to the largest batch seen), copies it once and runs the device half: mx_resample (the bicubic
    rescale, only for the items whose size changes) -> mx_irn_input_stage.
    Returns {"img" [n,3,S,S] fp32, "label" [n,S/4,S/4] uint8} on the device - the batch `irn_step` takes - or
    {"img"} when the plans carry no label (the eval view)."""

    def __init__(self, device, batch: int, crop_size: int = 512):
        if crop_size % 16:
            raise ValueError("crop_size must be a multiple of 16")
        self.dev, self.n, self.crop = device, batch, crop_size
        self.buf = StageBuffer(device)
        self.last_launch = None                             # (o_jobs, o_rs, resample jobs, rs_px) of the last batch, for tools/bench_irn_input.py

    @property
    def last_bytes(self) -> int:
        return self.buf.last_bytes

    def __call__(self, plans: Sequence[IrnItemPlan], out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """out: tensors to write into instead of new ones ({"img"} and, for training items, {"label"}: contiguous, on the
        stager's device, of the shapes and types returned)."""
        n, S, sb = len(plans), self.crop, self.buf
        assert 0 < n <= self.n
        with_label = plans[0].label_u8 is not None
        if any((p.label_u8 is not None) != with_label for p in plans):
            raise ValueError("a batch is either all training items or all eval views")
        rescaled = [p.tables is not None for p in plans]
        # ---- layout: [stage jobs | resample jobs | tables | images | labels]; behind it, on the device only:
        # [rescaled images | horizontal-pass temporaries]
        sb.plan()
        o_jobs, o_rs = sb.reserve(n * 64, 64), sb.reserve(n * 32, 64)
        tab_at = [sb.reserve(p.tables.nbytes) if r else 0 for p, r in zip(plans, rescaled)]
        ntab_at = [sb.reserve(4 * (p.size[0] + p.size[1])) if with_label else 0 for p in plans]
        img_at = [sb.reserve(p.img_u8.size) for p in plans]
        lab_at = [sb.reserve(p.label_u8.size) if with_label else -1 for p in plans]
        rs_at = [sb.scratch(p.size[0] * p.size[1] * 3) if r else 0 for p, r in zip(plans, rescaled)]
        tmp_at = [sb.scratch(p.img_u8.shape[0] * p.size[1] * 3) if r else 0 for p, r in zip(plans, rescaled)]
        buf = sb.begin()
        jobs = buf[o_jobs:o_jobs + n * 64].view(np.int32).reshape(n, 16)
        rsj = buf[o_rs:o_rs + n * 32].view(np.int32).reshape(n, 8)
        m, rs_px = 0, 1                                     # resample jobs are packed: only the items that are rescaled
        for i, p in enumerate(plans):
            h, w = p.img_u8.shape[:2]
            sh, sw = p.size
            buf[img_at[i]:img_at[i] + p.img_u8.size] = p.img_u8.reshape(-1)
            src = img_at[i]
            if rescaled[i]:
                buf[tab_at[i]:tab_at[i] + p.tables.nbytes] = p.tables.view(np.uint8)
                rsj[m] = resample_job(img_at[i], h, w, tmp_at[i], rs_at[i], sw, sh, tab_at[i])
                m, rs_px, src = m + 1, max(rs_px, h * sw, sh * sw), rs_at[i]
            yo = xo = 0
            if with_label:
                buf[lab_at[i]:lab_at[i] + p.label_u8.size] = p.label_u8.reshape(-1)
                o = ntab_at[i]
                buf[o:o + 4 * sh] = p.ytab.view(np.uint8)
                buf[o + 4 * sh:o + 4 * (sh + sw)] = p.xtab.view(np.uint8)
                yo, xo = o // 4, o // 4 + sh
            jobs[i] = (src, sh, sw, p.window[0], p.window[1], p.place[0], p.place[1], p.window[2], p.window[3], int(p.flip),
                       lab_at[i], h, w, yo, xo, 0)
        base, st = sb.upload(), stream()
        self.last_launch = (o_jobs, o_rs, m, int(rs_px))
        if m:
            call("mx_resample", base, base + o_rs, base, base, base, m, int(rs_px), st)
        want = {"img": ((n, 3, S, S), torch.float32)}
        if with_label:
            want["label"] = ((n, S // 4, S // 4), torch.uint8)
        if out is None:
            out = {k: torch.empty(shape, dtype=dt, device=self.dev) for k, (shape, dt) in want.items()}
        for k, (shape, dt) in want.items():
            t = out[k]
            if tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous() or t.device != out["img"].device:
                raise ValueError(f"out[{k!r}] must be a contiguous {dt} tensor of shape {shape}")
        out = {k: out[k] for k in want}
        call("mx_irn_input_stage", base, base + o_jobs, base, out["img"].data_ptr(),
             out["label"].data_ptr() if with_label else None, n, S, st)
        return out


class VOC12AffinityPlans:
    """`train_irn.VOC12AffinityDataset` for this input path: `plan(i)` is the host half of `__getitem__` (JPEG and PNG decode,
    the draws, the tables); a batch of plans goes through an `IrnStager`.  train=False plans the eval view."""

    def __init__(self, names, voc12_root: str, label_dir: str, crop_size: int, train: bool = True):
        self.names, self.root, self.label_dir, self.crop, self.is_train = list(names), voc12_root, label_dir, crop_size, train

    def __len__(self):
        return len(self.names)

    def plan(self, i: int) -> IrnItemPlan:
        import PIL.Image
        name = self.names[i]
        img = np.asarray(PIL.Image.open(os.path.join(self.root, "JPEGImages", name + ".jpg")).convert("RGB"))
        if not self.is_train:
            return plan_irn_eval_item(img, self.crop)
        label = np.asarray(PIL.Image.open(os.path.join(self.label_dir, name + ".png")))
        if label.ndim != 2 or label.shape != img.shape[:2]:
            raise ValueError(f"{name}: the IR label must be a single-channel map of the image's size (got {label.shape})")
        return plan_irn_item(img, label.astype(np.uint8), self.crop)

    __getitem__ = plan          # a torch.utils.data map-style dataset: DataLoader workers run the host half


class IrnLoader:
    """torch's DataLoader over `VOC12AffinityPlans` with `collate_fn=_keep`, built as `segdata.SegLoader` is: the workers
    decode and plan with torch's own per-worker seeding of `random` (base seed + worker id), shuffling comes from the same
    sampler as the host loader's, and each batch of plans goes through the `IrnStager` in the training process.
    Iterating yields the dict `irn_step` takes ({"img"} alone for an eval dataset).
    persistent_workers=False re-creates (and re-seeds) the workers every epoch, as a plain DataLoader does."""

    def __init__(self, dataset: VOC12AffinityPlans, batch_size: int, device, num_workers: int = 0, shuffle: bool = True,
                 drop_last: bool = True, generator=None, prefetch_factor: int = 4, persistent_workers: Optional[bool] = None):
        from torch.utils.data import DataLoader
        self.dataset, self.stager = dataset, IrnStager(device, batch_size, dataset.crop)
        persistent = bool(num_workers) if persistent_workers is None else bool(persistent_workers and num_workers)
        self.loader = DataLoader(dataset, batch_size=batch_size, shuffle=shuffle, num_workers=num_workers, drop_last=drop_last,
                                 collate_fn=_keep, generator=generator, persistent_workers=persistent,
                                 prefetch_factor=prefetch_factor if num_workers else None)

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for plans in self.loader:
            yield self.stager(plans)
