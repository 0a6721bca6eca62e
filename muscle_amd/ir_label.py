"""IR labels from CAMs: IRN's `cam_to_ir_label` step around `crf_inference_label` (src/imutils.py:477-491) on the HIP path.

With `cams` float [C,H,W] in [0,1] (the dict `infer_mcl` writes, class indices ascending) and keys = [0, k_1+1, ..., k_C+1]:

    fg_lab  = argmax([conf_fg_thres, cams...], axis=0)            first maximum wins
    fg_conf = keys[crf_inference_label(img, fg_lab, n_labels=C+1)]
    bg_lab  = argmax([conf_bg_thres, cams...], axis=0)
    bg_conf = keys[crf_inference_label(img, bg_lab, n_labels=C+1)]
    conf = fg_conf;  conf[fg_conf == 0] = 255;  conf[bg_conf + fg_conf == 0] = 0          -> uint8 [H,W]

The two CRFs share the image, so one call (`mx_ir_label`) runs them as columns of one stencil-GEMM per pass where
L = C+1 <= 16, and writes `conf` from the last pass's epilogue.  The CRF is the windowed model of muscle_amd.crf: the window is
part of the model, so the maps are not bit-identical with pydensecrf's.  pairwise="lattice" runs the CRFs on permutohedral
lattices instead (`mx_ir_label_lattice`, muscle_amd.lattice): pydensecrf's own approximation, a different model whose cost does not
grow with the bilateral width of 50; parity with pydensecrf itself is not pinned.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import call, ptr, stream
from .crf import LABEL_MODEL, label_workspace
from .lattice import check_pairwise, crf_lattice_workspace, device_image

CONF_FG_THRES, CONF_BG_THRES = 0.30, 0.05
CRF_T, CRF_GT_PROB = 10, 0.7                                   # src/imutils.py:477


def combine_conf(fg_conf: np.ndarray, bg_conf: np.ndarray) -> np.ndarray:
    """The three-line rule: a class where the foreground CRF says so, 0 where both say background, 255 (ignore) between."""
    fg_conf, bg_conf = np.asarray(fg_conf), np.asarray(bg_conf)
    conf = fg_conf.copy()
    conf[fg_conf == 0] = 255
    conf[bg_conf.astype(np.int64) + fg_conf.astype(np.int64) == 0] = 0
    return conf.astype(np.uint8)


def ir_label_run(img, cams, keys: Sequence[int], *, fg_thres: float = CONF_FG_THRES, bg_thres: float = CONF_BG_THRES, t: int = CRF_T,
                 gt_prob: float = CRF_GT_PROB, trunc: float = 4.0, fused: bool = True, want_pred: bool = False, want_q: bool = False,
                 model: Tuple[float, float, float, float, float] = LABEL_MODEL, pairwise: str = "window"
                 ) -> Tuple[torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor]]:
    """One enqueue of mx_ir_label (pairwise="lattice": mx_ir_label_lattice; trunc and fused are ignored) on the current stream.
    cams: float [C,H,W] array or tensor; keys: C+1 ints.  Returns (conf uint8 [H,W], the two argmax maps uint8 [2,H,W] or None,
    Q_t fp32 [2,C+1,H,W] or None), all on the device."""
    lattice = check_pairwise(pairwise)
    c = cams if torch.is_tensor(cams) else torch.from_numpy(np.ascontiguousarray(cams, dtype=np.float32))
    if c.dim() != 3:
        raise ValueError(f"cams must be [C,H,W] (got {tuple(c.shape)})")
    dev = c.device if c.is_cuda else torch.device("cuda", torch.cuda.current_device())
    c = c.to(dev, torch.float32).contiguous()
    C, H, W = c.shape
    if len(keys) != C + 1:
        raise ValueError(f"keys must have C+1 = {C + 1} entries (got {len(keys)})")
    im = device_image(img, dev)
    if tuple(im.shape[:2]) != (H, W):
        raise ValueError(f"img is {tuple(im.shape[:2])}, cams {(H, W)}")
    with torch.cuda.device(dev):
        k = torch.tensor([int(v) for v in keys], dtype=torch.int32).to(dev)
        conf = torch.empty(H, W, dtype=torch.uint8, device=dev)
        pred2 = torch.empty(2, H, W, dtype=torch.uint8, device=dev) if want_pred else None
        q = torch.empty(2, C + 1, H, W, dtype=torch.float32, device=dev) if want_q else None
        if lattice:
            ws = crf_lattice_workspace(dev, C + 1, H, W)
            call("mx_ir_label_lattice", ptr(im), ptr(c), ptr(k), C, H, W, float(fg_thres), float(bg_thres), int(t), float(gt_prob),
                 *model, ptr(ws), ptr(conf), ptr(pred2), ptr(q), stream())
            return conf, pred2, q
        ws = label_workspace(dev, H, W)
        call("mx_ir_label", ptr(im), ptr(c), ptr(k), C, H, W, float(fg_thres), float(bg_thres), int(t), float(gt_prob), *model,
             float(trunc), int(bool(fused)), ptr(ws), ptr(conf), ptr(pred2), ptr(q), stream())
    return conf, pred2, q


def cam_to_ir_label(img, cam_dict: Dict[int, np.ndarray], *, conf_fg_thres: float = CONF_FG_THRES,
                    conf_bg_thres: float = CONF_BG_THRES, trunc: float = 4.0, fused: bool = True,
                    pairwise: str = "window") -> torch.Tensor:
    """img: uint8 [H,W,3] array or tensor; cam_dict: {class index 0..19: [H,W] float}, what infer_mcl writes (keys are taken in
    ascending order).  Returns the uint8 [H,W] map on the device: 0 background, k+1 class k, 255 ignore.  pairwise: "window" or
    "lattice" (see ir_label_run)."""
    check_pairwise(pairwise)
    if len(cam_dict) == 0:
        raise ValueError("cam_dict is empty: an image without a class has no IR label")
    classes = sorted(int(k) for k in cam_dict)
    if classes[0] < 0 or classes[-1] > 19:
        raise ValueError(f"cam_dict keys must be class indices 0..19 (got {classes})")
    by_int = {int(k): v for k, v in cam_dict.items()}
    maps = [by_int[k] for k in classes]
    if torch.is_tensor(maps[0]):
        cams = torch.stack([m.float() for m in maps])
    else:
        cams = np.stack([np.asarray(m, dtype=np.float32) for m in maps])
    return ir_label_run(img, cams, [0] + [k + 1 for k in classes], fg_thres=conf_fg_thres, bg_thres=conf_bg_thres, trunc=trunc,
                        fused=fused, pairwise=pairwise)[0]
