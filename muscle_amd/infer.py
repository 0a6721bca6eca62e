"""CAM generation (infer_mcl.py:107-182) and semantic-segmentation inference (infer_seg.py:88-136) for one image, on the
HIP path.

Per forward pass of the multi-scale / flip list the reference moves the [1,21,Hs,Ws] maps to the host, transposes,
cv2.resize()s them to the original image size, flips the odd passes back, drops the background channel and appends to a
list; after the list it sums, clamps, min-max normalises per channel and keeps the channels of the image's labels.  Here
the model is asked for its 1/16-resolution NHWC maps and one kernel per pass does the model's align_corners upsample,
the half-pixel resize to (H, W), the un-flip and the accumulation into a resident [20,H,W] sum; a second kernel
normalises in place.  Only the kept channels leave the GPU.

The file layout of the result is the reference's: `np.save(path, {class_index: float32[H,W]})`, read back with
`np.load(path, allow_pickle=True).item()` by src/evaluation.py:25-33 and infer_irn.py:68-73.

Segmentation inference (`infer_seg`): per pass the reference runs the decoder's cam='seg' forward, a softmax, moves the
map to the host, cv2.resize()s it to the image size, flips the odd passes back, and after the list takes the mean, scales
the foreground channels by the image's class scores (--cls_dir) and argmaxes.  Here the decoder is asked for its
1/8-resolution logits (cam='seg_lr': no full-resolution seg_map and no 256-channel dense_ft), and ONE kernel over all
passes does the upsample, softmax, resize, un-flip, mean, class scale and argmax (mx_seg_infer).

The dense CRF of infer_seg.py:128-129 (`crf_img=`): the reference hands the mean map and the original image to pydensecrf
(imutils.crf_inference, t=4), a lattice-filter approximation of the fully connected CRF on the CPU.  Here the same model
runs on the device with its pairwise sums evaluated exactly over a square window of half-width ceil(trunc * sxy)
(muscle_amd/crf.py states the model; mx_crf_inference).  Label maps are therefore not bit-identical with pydensecrf's; at
trunc = 4 the windowed result is within 1e-4 of the all-pairs one.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from ._lib import call, ptr, stream

_CPAD = 24


def infer_cam(model, img_list: List[torch.Tensor], label: torch.Tensor, H: int, W: int
              ) -> Tuple[Dict[int, np.ndarray], Dict[int, np.ndarray], torch.Tensor]:
    """img_list: [1,3,Hs,Ws] device tensors in the order of VOC12ClsDatasetMSF (scale-major, plain then flipped);
    label: [1,20].  Returns (cam_dict, sgc_dict, score[20]) exactly as infer_mcl.py builds them."""
    if label.dim() != 2 or label.shape[0] != 1:
        raise ValueError("infer_cam handles one image per call (infer_mcl.py's DataLoader has batch_size 1)")
    model.eval()
    if getattr(model.backbone, "_eval_fold", None) is None and hasattr(model, "fold_eval_bn"):
        model.fold_eval_bn()              # eval BatchNorm folded into the 1x1 weights once, not per pass (train() drops it)
    dev = img_list[0].device
    K = model.classes
    acc_cam = torch.zeros(K - 1, H, W, dtype=torch.float32, device=dev)
    acc_sgc = torch.zeros(K - 1, H, W, dtype=torch.float32, device=dev)
    scores = []
    with torch.no_grad():
        i = 0
        while i < len(img_list):
            img = img_list[i]
            if img.shape[0] != 1:
                raise ValueError("each entry of img_list is one image [1,3,Hs,Ws]")
            # a scale and its flipped copy have the same size: one batch-2 forward instead of two batch-1 forwards (eval
            # mode is per-sample: same maps; at these sizes a B7 forward is launch-bound, so the pass costs the same)
            pair = i % 2 == 0 and i + 1 < len(img_list) and img_list[i + 1].shape == img.shape
            x = torch.cat([img, img_list[i + 1]], dim=0).float() if pair else img.float()
            cam_lr, sgc_lr, _emb, score = model(x, cam="cam_lr")                 # NHWC [b,h,w,24]
            _, h, w, lds = cam_lr.shape
            Hs, Ws = img.shape[2], img.shape[3]
            for b in range(x.shape[0]):
                call("mx_infer_accum", ptr(cam_lr[b]), ptr(acc_cam), h, w, lds, K, Hs, Ws, H, W, (i + b) % 2, stream())
                call("mx_infer_accum", ptr(sgc_lr[b]), ptr(acc_sgc), h, w, lds, K, Hs, Ws, H, W, (i + b) % 2, stream())
                scores.append(score[b:b + 1, 1:])
            i += x.shape[0]
        call("mx_infer_norm", ptr(acc_cam), K - 1, H * W, stream())
        call("mx_infer_norm", ptr(acc_sgc), K - 1, H * W, stream())
        score = torch.sigmoid(torch.mean(torch.cat(scores, dim=0), dim=0))
    keep = [i for i in range(K - 1) if float(label[0, i]) > 1e-5]
    cam_dict: Dict[int, np.ndarray] = {}
    sgc_dict: Dict[int, np.ndarray] = {}
    if keep:
        idx = torch.tensor(keep, device=dev)
        cams = acc_cam.index_select(0, idx).cpu().numpy()
        sgcs = acc_sgc.index_select(0, idx).cpu().numpy()
        for j, i in enumerate(keep):
            cam_dict[i] = cams[j]
            sgc_dict[i] = sgcs[j]
    return cam_dict, sgc_dict, score


def infer_cam_fused(model, img_list: List[torch.Tensor], label: torch.Tensor, H: int, W: int, want_cam: bool = True,
                    want_sgc: bool = True, pamr=None, pamr_img=None
                    ) -> Tuple[Dict[int, np.ndarray], Dict[int, np.ndarray], torch.Tensor]:
    """`infer_cam` with the post-processing in one launch: the same batch-2 forwards of a scale and its flip, then ONE
    mx_cam_infer over all passes, both maps and only the channels of the image's labels (the sum and the min-max are per
    channel, so the other 17-19 of 20 never need to exist), one mx_infer_norm per requested map on the compact
    [nkeep,H,W] buffer and one device->host copy of it.  Same bits as `infer_cam`.  want_cam / want_sgc = False: that map
    is neither read nor computed and its dict is empty.  An image without labels: empty dicts, nothing launched after the
    forwards.
    pamr: a muscle_amd.PAMR, with pamr_img the original uint8 image [H,W,3] (numpy or device tensor).  Each requested map is then
    refined on the device after its mx_infer_norm (muscle_amd/pamr.py states the model; one affinity per image, shared by both
    maps) and normalised once more, so a saved map still spans [0,1].  With pamr=None nothing of it runs: the launches and the
    bits of before."""
    from .pamr import check_pamr_args
    pimg = check_pamr_args(pamr, pamr_img, H, W)
    if label.dim() != 2 or label.shape[0] != 1:
        raise ValueError("infer_cam_fused handles one image per call (infer_mcl.py's DataLoader has batch_size 1)")
    if not img_list:
        raise ValueError("infer_cam_fused needs at least one pass")
    model.eval()
    if getattr(model.backbone, "_eval_fold", None) is None and hasattr(model, "fold_eval_bn"):
        model.fold_eval_bn()              # eval BatchNorm folded into the 1x1 weights once, not per pass (train() drops it)
    dev = img_list[0].device
    K = model.classes
    keep = [i for i in range(K - 1) if float(label[0, i]) > 1e-5]
    maps, rows, scores = [], [], []       # the low-res maps stay referenced until the one launch below is enqueued
    lds = _CPAD
    with torch.no_grad():
        i = 0
        while i < len(img_list):
            img = img_list[i]
            if img.dim() != 4 or img.shape[0] != 1:
                raise ValueError("each entry of img_list is one image [1,3,Hs,Ws]")
            pair = i % 2 == 0 and i + 1 < len(img_list) and img_list[i + 1].shape == img.shape
            x = torch.cat([img, img_list[i + 1]], dim=0).float() if pair else img.float()
            cam_lr, sgc_lr, _emb, score = model(x, cam="cam_lr")                 # NHWC [b,h,w,24]
            _, h, w, lds = cam_lr.shape
            for b in range(x.shape[0]):
                rows.append([cam_lr[b].data_ptr(), sgc_lr[b].data_ptr(), h, w, img.shape[2], img.shape[3], (i + b) % 2, 0])
                scores.append(score[b:b + 1, 1:])
            maps.append((cam_lr, sgc_lr))
            i += x.shape[0]
        score = torch.sigmoid(torch.mean(torch.cat(scores, dim=0), dim=0))
        cam_dict: Dict[int, np.ndarray] = {}
        sgc_dict: Dict[int, np.ndarray] = {}
        if not keep or not (want_cam or want_sgc):
            return cam_dict, sgc_dict, score
        tab = torch.tensor(rows, dtype=torch.int64).to(dev)
        idx = torch.tensor(keep, dtype=torch.int32).to(dev)
        nk = len(keep)
        out_cam = torch.empty(nk, H, W, dtype=torch.float32, device=dev) if want_cam else None
        out_sgc = torch.empty(nk, H, W, dtype=torch.float32, device=dev) if want_sgc else None
        call("mx_cam_infer", ptr(tab), len(rows), lds, K, H, W, ptr(idx), nk, ptr(out_cam), ptr(out_sgc), stream())
        aff = None
        if pimg is not None:
            with torch.cuda.device(dev):
                aff = pamr.affinity(pamr_img)             # once per image, shared by both maps
        for out, d in ((out_cam, cam_dict), (out_sgc, sgc_dict)):
            if out is None:
                continue
            call("mx_infer_norm", ptr(out), nk, H * W, stream())
            if aff is not None:
                out = pamr.apply(aff, out)
                call("mx_infer_norm", ptr(out), nk, H * W, stream())
            host = out.cpu().numpy()
            for j, k in enumerate(keep):
                d[k] = host[j]
    return cam_dict, sgc_dict, score


def save_cam_dict(path: str, d: Dict[int, np.ndarray]) -> None:
    """infer_mcl.py:177-178: np.save of the {class: map} dict (an object array holding the dict)."""
    np.save(path, d)


def load_cam_dict(path: str) -> Dict[int, np.ndarray]:
    """src/evaluation.py:27: np.load(...).item()"""
    return np.load(path, allow_pickle=True).item()


def infer_seg(model, img_list: List[torch.Tensor], H: int, W: int, cls_label=None, return_prob: bool = False, crf_img=None,
              crf_t: int = 4, crf_trunc: float = 4.0, crf_pairwise: str = "window", pamr=None, pamr_img=None
              ) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """infer_seg.py:88-133.  model: MuSCLe(mode='dec'); img_list: [1,3,Hs,Ws] device tensors in the order
    of VOC12ClsDatasetMSF (scale-major, plain then flipped; data.MSFStager builds it); cls_label: optional [K] class scores
    (entry 0, the background, is not used: :125).  Returns (pred uint8 [H,W], the fp32 mean probability map [K,H,W] if
    return_prob else None), both on the device.
    crf_img: the original uint8 image [H,W,3] (numpy or tensor).  With it the dense CRF of :128-129 runs on the mean map
    (crf.crf_inference with crf_t iterations, scale_factor 1.5, window crf_trunc): pred is argmax Q and the returned map
    is Q.  Without it nothing of the CRF runs and the result is what it was before the CRF existed, bit for bit.
    crf_pairwise: "window" (the exact windowed sums, the default) or "lattice" (the permutohedral lattice of muscle_amd.lattice:
    pydensecrf's own approximation, a different model; crf_trunc is ignored).
    pamr: a muscle_amd.PAMR, with pamr_img the original uint8 image [H,W,3]: the mean map is refined by PAMR instead
    (muscle_amd/pamr.py states the model): the returned map is the refined one, still a distribution where the mean map is one
    (every row of weights sums to 1), and pred its argmax, first maximum wins.  Refused together with crf_img.  pamr=None: nothing
    of it runs."""
    from .lattice import check_pairwise
    from .pamr import check_pamr_args
    check_pairwise(crf_pairwise)
    pimg = check_pamr_args(pamr, pamr_img, H, W)
    if pimg is not None and crf_img is not None:
        raise ValueError("pamr and crf_img are two refinements of the same map: give one of them")
    if not img_list:
        raise ValueError("infer_seg needs at least one pass")
    model.eval()
    if getattr(model.backbone, "_eval_fold", None) is None and hasattr(model, "fold_eval_bn"):
        model.fold_eval_bn()              # eval BatchNorm folded into the 1x1 weights once, not per pass (train() drops it)
    dev = img_list[0].device
    K = model.classes
    maps, rows = [], []                   # the low-res logits stay referenced until the one launch below is enqueued
    lds = _CPAD
    with torch.no_grad():
        i = 0
        while i < len(img_list):
            img = img_list[i]
            if img.dim() != 4 or img.shape[0] != 1:
                raise ValueError("each entry of img_list is one image [1,3,Hs,Ws]")
            # a scale and its flipped copy have the same size: one batch-2 forward (eval mode is per-sample)
            pair = i % 2 == 0 and i + 1 < len(img_list) and img_list[i + 1].shape == img.shape
            x = torch.cat([img, img_list[i + 1]], dim=0).float() if pair else img.float()
            seg_lr = model(x, cam="seg_lr")                                          # NHWC [b,h,w,24]
            _, h, w, lds = seg_lr.shape
            for b in range(x.shape[0]):
                rows.append([seg_lr[b].data_ptr(), h, w, img.shape[2], img.shape[3], (i + b) % 2, 0, 0])
            maps.append(seg_lr)
            i += x.shape[0]
        tab = torch.tensor(rows, dtype=torch.int64).to(dev)
        cls = None
        if cls_label is not None:
            cls = torch.as_tensor(np.asarray(cls_label, dtype=np.float32).reshape(-1)).to(dev)
            if cls.numel() != K:
                raise ValueError(f"cls_label has {cls.numel()} entries, the model {K} classes")
        pred = torch.empty(H, W, dtype=torch.uint8, device=dev)
        want_map = return_prob or crf_img is not None or pimg is not None
        prob = torch.empty(K, H, W, dtype=torch.float32, device=dev) if want_map else None
        call("mx_seg_infer", ptr(tab), len(rows), lds, K, H, W, ptr(cls), ptr(pred), ptr(prob), stream())
        if pimg is not None:
            from .pamr import planar_argmax
            with torch.cuda.device(dev):
                prob = pamr(pamr_img, prob)
                pred = planar_argmax(prob)
            if not return_prob:
                prob = None
        if crf_img is not None:
            from .crf import crf_run
            prob, pred = crf_run(crf_img, prob, crf_t, 1.5, K, 0.5, crf_trunc, want_q=return_prob, want_pred=True,
                                 pairwise=crf_pairwise)
    return pred, prob


def infer_seg_batch(model, imgs: torch.Tensor, H: int, W: int, cls_labels=None, crf_imgs=None, return_prob: bool = False,
                    crf_t: int = 4, crf_trunc: float = 4.0, gts: Optional[torch.Tensor] = None,
                    counts: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """`infer_seg` with a single pass per image (the `img_list[:1]` of the per-epoch validation) for B images of one input
    size and one output size: imgs [B,3,Hs,Ws] on the device; one cam='seg_lr' forward and one mx_seg_infer_batch launch.
    cls_labels: optional [B,K] class scores; crf_imgs: optional B uint8 [H,W,3] images, the dense CRF then runs per image
    (mx_crf_inference looped over the batch).  gts uint8 [B,H,W] with counts int64 [K,3] (both or neither, not with the
    CRF): the (TP, P, T) table of `SegEval.add` is accumulated by the same launch.  Returns (pred uint8 [B,H,W], the fp32
    map [B,K,H,W] if return_prob else None); per image the bits of `infer_seg(model, [imgs[b:b+1]], H, W, ...)`."""
    if imgs.dim() != 4 or imgs.shape[0] < 1:
        raise ValueError(f"imgs must be [B,3,Hs,Ws] (got {tuple(imgs.shape)})")
    if (gts is None) != (counts is None):
        raise ValueError("gts and counts go together")
    if crf_imgs is not None and gts is not None:
        raise ValueError("with the CRF the prediction changes after the launch: count with SegEval.add per image")
    B, _, Hs, Ws = imgs.shape
    if crf_imgs is not None and len(crf_imgs) != B:
        raise ValueError(f"crf_imgs has {len(crf_imgs)} images, the batch {B}")
    model.eval()
    if getattr(model.backbone, "_eval_fold", None) is None and hasattr(model, "fold_eval_bn"):
        model.fold_eval_bn()
    dev = imgs.device
    K = model.classes
    with torch.no_grad():
        seg_lr = model(imgs.float(), cam="seg_lr")                                   # NHWC [B,h,w,24]
        _, h, w, lds = seg_lr.shape
        tab = torch.tensor([[seg_lr[b].data_ptr(), h, w, Hs, Ws, 0, b, 0] for b in range(B)], dtype=torch.int64).to(dev)
        cls = None
        if cls_labels is not None:
            cls = torch.as_tensor(np.asarray(cls_labels, dtype=np.float32).reshape(B, -1)).to(dev).contiguous()
            if cls.shape[1] != K:
                raise ValueError(f"cls_labels has {cls.shape[1]} entries per image, the model {K} classes")
        if gts is not None and (gts.dtype != torch.uint8 or tuple(gts.shape) != (B, H, W) or tuple(counts.shape) != (K, 3)
                                or counts.dtype != torch.int64):
            raise ValueError(f"gts must be uint8 [{B},{H},{W}] and counts int64 [{K},3]")
        pred = torch.empty(B, H, W, dtype=torch.uint8, device=dev)
        prob = torch.empty(B, K, H, W, dtype=torch.float32, device=dev) if return_prob or crf_imgs is not None else None
        call("mx_seg_infer_batch", ptr(tab), B, B, lds, K, H, W, ptr(cls), ptr(pred), ptr(prob),
             ptr(gts.contiguous()) if gts is not None else None, ptr(counts), stream())
        if crf_imgs is not None:
            from .crf import crf_run
            qs = []
            for b in range(B):
                q, pb = crf_run(crf_imgs[b], prob[b], crf_t, 1.5, K, 0.5, crf_trunc, want_q=return_prob, want_pred=True)
                pred[b].copy_(pb)
                qs.append(q)
            prob = torch.stack(qs) if return_prob else None
    return pred, prob


def save_seg_png(path: str, pred) -> None:
    """infer_seg.py:129-131: the class-index map as an 8-bit single-channel PNG, the file src/evaluation.py:24-25 reads
    back with np.array(Image.open(path))."""
    import PIL.Image
    a = pred.cpu().numpy() if torch.is_tensor(pred) else np.asarray(pred)
    if a.ndim != 2 or a.dtype != np.uint8:
        raise ValueError(f"pred must be uint8 [H,W] (got {a.dtype} {a.shape})")
    PIL.Image.fromarray(a, mode="L").save(path)
