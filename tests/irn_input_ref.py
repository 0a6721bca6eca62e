"""What the device half of muscle_amd.irndata computes FROM A PLAN, in numpy: mx_resample's part with Pillow's own bicubic resize,
mx_irn_input_stage's two gathers as include/muscle_hip.h states them.  It lets the planner (draws, geometry, NEAREST tables) be
checked against `train_irn.affinity_sample` / `top_left_sample` without a GPU; the GPU tests then check the kernels against
the same functions.  Also the synthetic images, labels and the small VOC tree the tests share."""
import os
import random

import numpy as np

_MEAN, _STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _axis(S, place, lo, cnt, step=1, first=0):
    """Container coordinates first, first + step, ... below S -> (inside the window, coordinate inside the rescaled image)."""
    c = first + step * np.arange((S - first + step - 1) // step)
    w = c - place
    ok = (w >= 0) & (w < cnt)
    return ok, lo + w


def emulate(p, S):
    """(img float32 [3,S,S], label uint8 [S/4,S/4] or None) of one IrnItemPlan."""
    import PIL.Image
    src = p.img_u8
    if p.resize_to is not None:
        src = np.asarray(PIL.Image.fromarray(src).resize(p.resize_to, PIL.Image.BICUBIC))
    sh, sw = p.size
    assert src.shape[:2] == (sh, sw)
    top, left, ch, cw = p.window
    lut = np.stack([((np.arange(256) / 255. - _MEAN[c]) / _STD[c]).astype(np.float32) for c in range(3)])   # data.py:603-607
    oky, ry = _axis(S, p.place[0], top, ch)
    okx, fx = _axis(S, p.place[1], left, cw)
    rx = sw - 1 - fx if p.flip else fx
    img = np.zeros((3, S, S), np.float32)
    px = src[np.ix_(ry[oky], rx[okx])]
    for c in range(3):
        img[c][np.ix_(oky, okx)] = lut[c][px[..., c]]
    if p.label_u8 is None:
        return img, None
    oky, ry = _axis(S, p.place[0], top, ch, 4, 2)
    okx, fx = _axis(S, p.place[1], left, cw, 4, 2)
    rx = sw - 1 - fx if p.flip else fx
    lab = np.full((S // 4, S // 4), 255, np.uint8)
    lab[np.ix_(oky, okx)] = p.label_u8[np.ix_(p.ytab[ry[oky]], p.xtab[rx[okx]])]
    return img, lab


def synth_image(h, w, seed):
    """Blocks of colour plus noise, uint8 [h,w,3]: edges for the bicubic to ring on, no two neighbouring pixels equal."""
    g = np.random.default_rng(seed)
    base = g.integers(0, 256, ((h + 7) // 8, (w + 7) // 8, 3)).repeat(8, 0).repeat(8, 1)[:h, :w]
    return (base + g.integers(-12, 13, (h, w, 3))).clip(0, 255).astype(np.uint8)


def synth_label(h, w, seed):
    """uint8 [h,w] in 0..5 and 255, in blocks of 5 x 7 with single-pixel speckle (so that a NEAREST index off by one shows)."""
    g = np.random.default_rng(1000 + seed)
    lab = g.integers(0, 7, ((h + 4) // 5, (w + 6) // 7)).repeat(5, 0).repeat(7, 1)[:h, :w]
    speck = g.random((h, w)) < 0.15
    lab = np.where(speck, g.integers(0, 7, (h, w)), lab).astype(np.uint8)
    lab[lab == 6] = 255
    return lab


class Rec:
    """A random.Random behind the three calls the samplers make, with a log of every draw."""

    def __init__(self, seed):
        self.r, self.log = random.Random(seed), []

    def random(self):
        v = self.r.random()
        self.log.append(("random", v))
        return v

    def getrandbits(self, k):
        v = self.r.getrandbits(k)
        self.log.append(("getrandbits", k, v))
        return v

    def randrange(self, n):
        v = self.r.randrange(n)
        self.log.append(("randrange", n, v))
        return v


VOC_SIZES = [(40, 50), (97, 203), (64, 64), (61, 130), (120, 90), (33, 77)]


def make_voc_tree(root):
    """Six JPEGs of VOC_SIZES with IR-label PNGs under root; returns (names, voc12_root, label_dir, list file)."""
    import PIL.Image
    voc, lab = os.path.join(root, "VOC2012"), os.path.join(root, "ir_label")
    os.makedirs(os.path.join(voc, "JPEGImages"))
    os.makedirs(lab)
    names = [f"2007_{i:06d}" for i in range(len(VOC_SIZES))]
    for i, (nm, (h, w)) in enumerate(zip(names, VOC_SIZES)):
        PIL.Image.fromarray(synth_image(h, w, 50 + i), "RGB").save(os.path.join(voc, "JPEGImages", nm + ".jpg"), quality=95)
        PIL.Image.fromarray(synth_label(h, w, 50 + i), "L").save(os.path.join(lab, nm + ".png"))
    lst = os.path.join(root, "train.txt")
    with open(lst, "w") as f:
        f.write("".join(f"/JPEGImages/{nm}.jpg /SegmentationClassAug/{nm}.png\n" for nm in names))
    return names, voc, lab, lst
