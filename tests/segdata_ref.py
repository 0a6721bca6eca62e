"""numpy / scipy / PIL restatement of the reference's decoder-training input path (VOC12SegDataset.__getitem__,
src/data.py:93-123 with src/imutils.py:35-53, :80-118, :283-292, :383-388), the comparator of tests/test_seg_input_path.py.

skimage.transform.resize (0.16.2: order=1, mode='reflect', anti_aliasing=True, clip=True) is restated from its published
source with the scipy.ndimage calls it makes: gaussian_filter(sigma = max(0, (in/out - 1)/2) per spatial axis, mode='mirror'),
then per channel a bilinear sample (map_coordinates(order=1, mode='mirror')) at (Y + 0.5) * in/out - 0.5.  skimage itself is
not installed here, so this restatement - not skimage - is what the device path is pinned against."""
import random

import numpy as np
import scipy.ndimage as ndi
import torch


def skresize_ref(mask, oh, ow):
    """skimage.transform.resize(mask [H,W,C] float64, (oh, ow)) as described above, in float64."""
    m = np.asarray(mask, dtype=np.float64)
    H, W, C = m.shape
    f = np.array([H / oh, W / ow, 1.0])
    g = ndi.gaussian_filter(m, np.maximum(0, (f - 1) / 2), cval=0, mode='mirror')
    r = (np.arange(oh) + 0.5) * f[0] - 0.5
    c = (np.arange(ow) + 0.5) * f[1] - 0.5
    rr, cc = np.meshgrid(r, c, indexing='ij')
    return np.stack([ndi.map_coordinates(g[..., k], [rr, cc], order=1, mode='mirror') for k in range(C)], -1)


def apply_tables(m, ty, tx):
    """The separable form: (start, weights) of one axis after the other on m [H,W,C], in the dtype of the weights."""
    (sy, wy), (sx, wx) = ty, tx
    m = np.asarray(m, dtype=wy.dtype)
    v = sum(wy[:, i, None, None] * m[sy + i] for i in range(wy.shape[1]))
    return sum(wx[None, :, j, None] * v[:, sx + j] for j in range(wx.shape[1]))


def ref_draws(w, h, min_scale, max_scale, crop, augment=True):
    """The random draws of __getitem__ in the reference's order, issued directly: ColorJitter.get_params of torchvision 0.9.0
    (randperm, then brightness / contrast / saturation / hue from torch's generator), random.uniform, RandomCropWithMask's two
    randrange (width first), getrandbits."""
    jit = None
    if augment:
        order = torch.randperm(4).tolist()
        b = float(torch.empty(1).uniform_(0.9, 1.1))
        c = float(torch.empty(1).uniform_(0.9, 1.1))
        s = float(torch.empty(1).uniform_(0.9, 1.1))
        hue = float(torch.empty(1).uniform_(-0.05, 0.05))
        jit = (order, b, c, s, hue)
    scale = random.uniform(min_scale, max_scale)
    tw, th = round(w * scale), round(h * scale)
    ch, cw = min(crop, th), min(crop, tw)
    w_space, h_space = tw - crop, th - crop
    if w_space > 0:
        cont_left, img_left = 0, random.randrange(w_space + 1)
    else:
        cont_left, img_left = random.randrange(-w_space + 1), 0
    if h_space > 0:
        cont_top, img_top = 0, random.randrange(h_space + 1)
    else:
        cont_top, img_top = random.randrange(-h_space + 1), 0
    flip = bool(random.getrandbits(1))
    return {"jitter": jit, "scale": scale, "target": (tw, th), "img_crop": (img_top, img_left, ch, cw),
            "place": (cont_top, cont_left), "flip": flip}


def color_norm(img):
    """src/imutils.py:383-388"""
    x = np.asarray(img)
    out = np.empty_like(x, np.float64)
    for c, (m, s) in enumerate(zip((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))):
        out[..., c] = (x[..., c] / 255. - m) / s
    return out


def _container(a, d, crop, dtype):
    (it, il, ch, cw), (ct, cl) = d["img_crop"], d["place"]
    out = np.zeros((crop, crop, a.shape[-1]), dtype)
    out[ct:ct + ch, cl:cl + cw] = a[it:it + ch, il:il + cw]
    if d["flip"]:
        out = np.fliplr(out).copy()
    return out.transpose(2, 0, 1)


def ref_image(pil_img, d, crop):
    """jitter -> bilinear resize -> color_norm -> crop container (float32) -> flip -> CHW: the tensor `img.cuda().float()`."""
    from PIL import Image
    from muscle_amd.data import apply_color_jitter           # torchvision's PIL calls (ImageEnhance / HSV), not device code
    if d["jitter"] is not None:
        pil_img = apply_color_jitter(pil_img, d["jitter"])
    return _container(color_norm(pil_img.resize(d["target"], resample=Image.BILINEAR)), d, crop, np.float32)


def ref_mask(mask, d, crop, dtype=np.float64):
    """resize -> crop container -> flip -> CHW; float64 by default (the reference's container is float32)."""
    tw, th = d["target"]
    return _container(skresize_ref(mask, th, tw), d, crop, dtype)


def window(d, crop):
    """Boolean [crop, crop]: where the placed (and possibly flipped) window is."""
    (_, _, ch, cw), (ct, cl) = d["img_crop"], d["place"]
    w = np.zeros((crop, crop), bool)
    w[ct:ct + ch, cl:cl + cw] = True
    return w[:, ::-1] if d["flip"] else w


def plan_as_draws(p):
    return {"jitter": p.jitter, "scale": p.scale, "target": p.resize_to, "img_crop": p.img_crop, "place": p.place, "flip": p.flip}


def synth_label(H, W, seed, C=21):
    """A soft pseudo-label as infer_irn writes it (float16 [H,W,C]): background 0.35, three soft discs, and uniform(0, 0.02)
    texture on every channel so that exactly tied pixels are rare."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.zeros((H, W, C))
    m[..., 0] = 0.35
    for k in rng.choice(np.arange(1, C), 3, replace=False):
        cy, cx, r = rng.uniform(0.2, 0.8) * H, rng.uniform(0.2, 0.8) * W, rng.uniform(0.15, 0.35) * H
        m[..., k] = np.clip(1 - np.hypot(yy - cy, xx - cx) / r, 0, 1)
    m += rng.uniform(0, 0.02, m.shape)
    return m.astype(np.float16)


def synth_image(H, W, seed):
    """A smooth RGB image with some noise, as a PIL image."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([127 + 100 * np.sin(xx / 17.0 + c) * np.cos(yy / 23.0 - c) for c in range(3)], -1)
    return Image.fromarray(np.clip(base + rng.normal(0, 12, base.shape), 0, 255).astype(np.uint8), "RGB")
