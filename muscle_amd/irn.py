"""The IRN edge / displacement network of infer_irn.py on the HIP path - `EdgeDisplacement` of
src/backbones/resnet50_irn.py:215-232 on src/backbones/resnet50.py (ResNet-50, frozen BatchNorm, strides (2,2,2,1), five
edge heads and seven displacement heads with GroupNorm) - and `infer_irn`, infer_irn.py:64-92 for one image.

`EdgeDisplacement` is a parameter container plus a HIP forward, like `muscle_amd.MuSCLe`: its sub-modules exist to hold the
tensors under the reference's names, none of them is ever called.  The reference registers the same sub-modules several
times (resnet50.* / stage1..5.* / backbone.*, fc_edge* / edge_layers.*, fc_dp* / dp_layers.*, mean_shift / fc_dp7.4), so
its checkpoints carry every tensor under two or three names; the containers here are shared in the same way, which gives
the same state_dict() key set and lets such a checkpoint load under strict=True.

Forward (inference only, NHWC fp32): stem = mx_stem7_im2col + the 1x1 GEMM with the folded BatchNorm + ReLU, mx_maxpool3s2;
every bottleneck = GEMM, mx_conv3x3_fwd, GEMM with `+ residual, relu` in its epilogue (stride-2 down-sample branches read
their rows through mx_gather_s2); every head = GEMM, mx_gn_stats, mx_gn_resize straight into its slice of the
concatenation; mx_irn_net_finish.  The 1x1 GEMMs follow the GEMM arithmetic mode, the 3x3 convolution is exact fp32.
`prepare()` folds the BatchNorms and packs the 3x3 weights once per checkpoint load.  Nothing here downloads anything.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch
import torch.nn as nn

from . import indexing, ops
from ._lib import MuscleHipError, call, ptr, stream
from .synth import _IRN_DP, _IRN_EDGE, _IRN_LAYERS

_EDGE_UP = (1, 1, 2, 4, 4)                 # resnet50_irn.py:22-49: up-sampling of fc_edge1..5
_DP_UP = (1, 1, 1, 2, 2, 2, 1)             # :53-92: fc_dp1..7


class _Holder(nn.Module):
    def forward(self, *a, **k):
        raise MuscleHipError("this module only holds parameters; EdgeDisplacement.forward runs the HIP kernels")


def _seq(*mods):
    return nn.Sequential(*mods)


class _Block(_Holder):                      # resnet50.py:20-32
    def __init__(self, inplanes, planes, down):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.downsample = _seq(nn.Conv2d(inplanes, planes * 4, 1, bias=False), nn.BatchNorm2d(planes * 4)) if down else None


class _Trunk(_Holder):                      # resnet50.py:59-70
    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.Identity()
        self.maxpool = nn.Identity()
        inplanes = 64
        for li, (planes, blocks, _stride) in enumerate(_IRN_LAYERS, 1):
            layer = []
            for b in range(blocks):
                layer.append(_Block(inplanes, planes, b == 0))
                inplanes = planes * 4
            setattr(self, f"layer{li}", _seq(*layer))


class _MeanShift(_Holder):                  # resnet50_irn.py:98-107
    def __init__(self):
        super().__init__()
        self.register_buffer("running_mean", torch.zeros(2))


def _fold(bn: nn.BatchNorm2d):
    """eval-mode BatchNorm as y = s*x + t (FixedBatchNorm, resnet50.py:11-14), computed in fp64."""
    s = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    t = bn.bias.detach().double() - bn.running_mean.detach().double() * s
    return s, t


def _fold_1x1(conv: nn.Conv2d, bn: nn.BatchNorm2d):
    s, t = _fold(bn)
    w = conv.weight.detach().double().reshape(conv.out_channels, -1) * s[:, None]
    return w.float().contiguous(), t.float().contiguous()


_KCHUNK = 512


def _chunks(w: torch.Tensor):
    """A 1x1 weight [Co, K] as contiguous column blocks of at most _KCHUNK input channels (see _pw)."""
    K = w.shape[1]
    return [w[:, k:min(k + _KCHUNK, K)].contiguous() for k in range(0, K, _KCHUNK)]


def _pw(A: torch.Tensor, ws, n_out: int, *, bias=None, residual=None, relu=False):
    """A [M,K] x W^T (+bias) (+residual) (relu) through mx_pw_fwd.  The GEMM kernels add K in one fp32 chain; for K > 512 (the
    1024- and 2048-channel inputs of layers 3-4 and of the heads) the columns are walked in blocks of 512, each launch adding the
    previous partial result through the `residual` epilogue: a blocked sum, as a CPU BLAS does with its K panels, whose
    rounding error stays that of K = 512 instead of growing through sixteen residual blocks."""
    if len(ws) == 1:
        return ops.pw_fwd(A, ws[0], n_out, bias=bias, residual=residual, relu=relu)
    if residual is not None:
        raise MuscleHipError("_pw: a blocked GEMM keeps the residual slot for its own partial sums")
    M, K = A.shape
    acc, k0 = None, 0
    for i, w in enumerate(ws):
        last = i == len(ws) - 1
        out = torch.empty(M, n_out, dtype=torch.float32, device=A.device)
        call("mx_pw_fwd", ptr(A) + 4 * k0, 0, None, None, None, 1, ptr(w), ptr(out), M, w.shape[1], n_out, K, n_out,
             ptr(bias) if last else None, ptr(acc), int(relu and last), None, stream())
        acc, k0 = out, k0 + w.shape[1]
    return acc


class EdgeDisplacement(nn.Module):
    def __init__(self, crop_size: int = 512, stride: int = 4):
        super().__init__()
        self.crop_size, self.stride = int(crop_size), int(stride)
        self.resnet50 = _Trunk()
        r = self.resnet50
        self.stage1 = _seq(r.conv1, r.bn1, r.relu, r.maxpool)
        self.stage2, self.stage3, self.stage4, self.stage5 = _seq(r.layer1), _seq(r.layer2), _seq(r.layer3), _seq(r.layer4)
        self.mean_shift = _MeanShift()
        for i, (ci, co, g) in enumerate(_IRN_EDGE, 1):
            mods = [nn.Conv2d(ci, co, 1, bias=False), nn.GroupNorm(g, co)] + [nn.Identity()] * (2 if _EDGE_UP[i - 1] > 1 else 1)
            setattr(self, f"fc_edge{i}", _seq(*mods))
        self.fc_edge6 = nn.Conv2d(160, 1, 1, bias=True)
        for i, (ci, co, g) in enumerate(_IRN_DP, 1):
            mods = [nn.Conv2d(ci, co, 1, bias=False), nn.GroupNorm(g, co)] + [nn.Identity()] * (2 if _DP_UP[i - 1] > 1 else 1)
            if i == 7:
                mods += [nn.Conv2d(256, 2, 1, bias=False), self.mean_shift]
            setattr(self, f"fc_dp{i}", _seq(*mods))
        self.backbone = nn.ModuleList([self.stage1, self.stage2, self.stage3, self.stage4, self.stage5])
        self.edge_layers = nn.ModuleList([getattr(self, f"fc_edge{i}") for i in range(1, 7)])
        self.dp_layers = nn.ModuleList([getattr(self, f"fc_dp{i}") for i in range(1, 8)])
        self._prep: Optional[Dict] = None
        self.eval()

    # -- the folded / packed weights live exactly as long as the parameters they were made from ------------------------
    def load_state_dict(self, *a, **k):
        self._prep = None
        return super().load_state_dict(*a, **k)

    def train(self, mode: bool = True):
        self._prep = None
        return super().train(mode)

    def _apply(self, fn, *a, **k):
        self._prep = None
        return super()._apply(fn, *a, **k)

    def prepare(self) -> Dict:
        """Fold every frozen BatchNorm into its convolution (weight * s, bias t) and pack the 3x3 weights into the kernel's
        K-major layout, once; dropped by load_state_dict() / train() / .to()."""
        dev = self.fc_edge6.weight.device
        if dev.type != "cuda":
            raise MuscleHipError("EdgeDisplacement runs on the HIP kernels only: move it to the GPU first")
        with torch.no_grad():
            r = self.resnet50
            w, b = _fold_1x1(r.conv1, r.bn1)
            p: Dict = {"stem_w": torch.cat([w, w.new_zeros(64, 1)], dim=1).contiguous(), "stem_b": b, "layers": []}
            for li, (_planes, _blocks, stride) in enumerate(_IRN_LAYERS, 1):
                blocks = []
                for bi, blk in enumerate(getattr(r, f"layer{li}")):
                    w1, b1 = _fold_1x1(blk.conv1, blk.bn1)
                    s2, t2 = _fold(blk.bn2)
                    w3, b3 = _fold_1x1(blk.conv3, blk.bn3)
                    d = dict(w1=_chunks(w1), planes=w1.shape[0], b1=b1, w2=ops.conv3x3_pack(blk.conv2.weight.detach().float(), s2.float().contiguous()),
                             b2=t2.float().contiguous(), w3=w3, b3=b3, stride=stride if bi == 0 else 1, wd=None, bd=None)
                    if blk.downsample is not None:
                        wd, d["bd"] = _fold_1x1(blk.downsample[0], blk.downsample[1])
                        d["wd"] = _chunks(wd)
                    blocks.append(d)
                p["layers"].append(blocks)

            def head(seq):
                conv, gn = seq[0], seq[1]
                return dict(w=_chunks(conv.weight.detach().float().reshape(conv.out_channels, -1)), co=conv.out_channels,
                            g=gn.num_groups, eps=gn.eps, gamma=gn.weight.detach().float().contiguous(),
                            beta=gn.bias.detach().float().contiguous())
            p["edge"] = [head(getattr(self, f"fc_edge{i}")) for i in range(1, 6)]
            p["dp"] = [head(getattr(self, f"fc_dp{i}")) for i in range(1, 8)]
            # the 1- and 2-channel tails as 4-column GEMMs (zero rows)
            we = torch.zeros(4, 160, device=dev)
            we[:1] = self.fc_edge6.weight.detach().float().reshape(1, 160)
            be = torch.zeros(4, device=dev)
            be[:1] = self.fc_edge6.bias.detach().float()
            wd = torch.zeros(4, 256, device=dev)
            wd[:2] = self.fc_dp7[3].weight.detach().float().reshape(2, 256)
            p.update(edge6_w=we, edge6_b=be, dp7_w=wd, mean=self.mean_shift.running_mean.detach().float().contiguous())
        self._prep = p
        return p

    @staticmethod
    def _bottleneck(x, d):
        N, H, W, C = x.shape
        planes = d["planes"]
        o = _pw(x.view(-1, C), d["w1"], planes, bias=d["b1"], relu=True).view(N, H, W, planes)
        o = ops.conv3x3(o, d["w2"], bias=d["b2"], stride=d["stride"], relu=True)
        _, Ho, Wo, _ = o.shape
        if d["wd"] is not None:
            xs = ops.gather_s2(x) if d["stride"] == 2 else x
            res = _pw(xs.view(-1, C), d["wd"], 4 * planes, bias=d["bd"])
        else:
            res = x.view(-1, C)
        return ops.pw_fwd(o.view(-1, planes), d["w3"], 4 * planes, bias=d["b3"], residual=res, relu=True).view(N, Ho, Wo, 4 * planes)

    @staticmethod
    def _head(x, hd, dst, coff, scale):
        N, H, W, C = x.shape
        o = _pw(x.view(-1, C), hd["w"], hd["co"]).view(N, H, W, hd["co"])
        ops.gn_resize(o, ops.gn_stats(o, hd["g"], hd["eps"]), hd["gamma"], hd["beta"], dst, coff, scale, relu=True)

    def features(self, x: torch.Tensor):
        """resnet50_irn.py:109-130 on the zero-padded frame, NHWC: ([x1..x5], edge_cat, dp_cat1, dp_cat2)."""
        p = self._prep or self.prepare()
        if x.dim() != 4 or x.shape[1] != 3 or not x.is_cuda:
            raise MuscleHipError("EdgeDisplacement.forward takes a CUDA [N,3,H,W] tensor")
        N, _, H, W = x.shape
        S = self.crop_size
        if H > S or W > S:
            raise ValueError(f"image {H}x{W} exceeds crop_size {S} (resnet50_irn.py:225 pads up to it)")
        x = x.float().contiguous()
        H1 = (S - 1) // 2 + 1
        a = ops.pw_fwd(ops.stem7_im2col(x, H1, H1), p["stem_w"], 64, bias=p["stem_b"], relu=True).view(N, H1, H1, 64)
        h = ops.maxpool3s2(a)
        xs = [h]
        for blocks in p["layers"]:
            for d in blocks:
                h = self._bottleneck(h, d)
            xs.append(h)
        dev = x.device
        _, h2, w2, _ = xs[1].shape
        _, h3, w3, _ = xs[2].shape
        ecat = torch.empty(N, h2, w2, 160, dtype=torch.float32, device=dev)
        for i in range(5):
            self._head(xs[i], p["edge"][i], ecat, 32 * i, _EDGE_UP[i])
        cat1 = torch.empty(N, h3, w3, 768, dtype=torch.float32, device=dev)
        for j, i in enumerate((2, 3, 4)):
            self._head(xs[i], p["dp"][i], cat1, 256 * j, _DP_UP[i])
        cat2 = torch.empty(N, h2, w2, 448, dtype=torch.float32, device=dev)
        self._head(xs[0], p["dp"][0], cat2, 0, 1)
        self._head(xs[1], p["dp"][1], cat2, 64, 1)
        self._head(cat1, p["dp"][5], cat2, 192, _DP_UP[5])
        return xs, ecat, cat1, cat2

    def forward(self, x: torch.Tensor):
        """x: the [2,3,H,W] pair (image, flipped image).  Returns (edge [1,h,w], dp [2,h,w]), h = (H-1)//stride + 1, on the device."""
        if self.training:
            raise MuscleHipError("EdgeDisplacement is inference only (the reference ships no IRN training script): call .eval()")
        if x.shape[0] != 2:
            raise ValueError("EdgeDisplacement.forward takes the pair [image, flipped image] (resnet50_irn.py:229)")
        with torch.no_grad():
            p = self._prep or self.prepare()
            _xs, ecat, _cat1, cat2 = self.features(x)
            N, h2, w2, _ = ecat.shape
            fh, fw = (x.shape[2] - 1) // self.stride + 1, (x.shape[3] - 1) // self.stride + 1
            if fh > h2 or fw > w2:
                raise ValueError(f"stride {self.stride}: the {fh}x{fw} crop exceeds the network's {h2}x{w2} output")
            eo = ops.pw_fwd(ecat.view(-1, 160), p["edge6_w"], 4, bias=p["edge6_b"]).view(N, h2, w2, 4)
            o7 = torch.empty(N, h2, w2, 256, dtype=torch.float32, device=x.device)
            self._head(cat2, p["dp"][6], o7, 0, 1)
            do = ops.pw_fwd(o7.view(-1, 256), p["dp7_w"], 4).view(N, h2, w2, 4)
            return ops.irn_net_finish(eo, do, p["mean"], fh, fw)


def cam_stack(cam_dict, H: int, W: int, device) -> torch.Tensor:
    """infer_irn.py:70-75: the {class: [H,W]} dict of infer_mcl.py as a dense [20,H,W] stack, zeros for absent classes."""
    a = np.zeros((20, H, W), np.float32)
    for k, v in cam_dict.items():
        a[int(k)] = v
    return torch.from_numpy(a).to(device)


def infer_irn(model: EdgeDisplacement, img_pair: torch.Tensor, cam_dict, *, beta=8, exp_times=6, bg_thres=0.35,
              soft_output: bool = False):
    """infer_irn.py:64-92 for one image: the network, the CAM down-scaling (:76), the random walk (:77) and the label step
    (:79-92).  img_pair: [2,3,H,W] on the device; cam_dict: {class index: float32 [H,W]}.  Returns the uint8 label map [H,W]
    (and the fp16 [H,W,21] array with soft_output) on the device."""
    H, W = img_pair.shape[2:]
    edge, _dp = model(img_pair)
    with torch.no_grad():
        cams = cam_stack(cam_dict, H, W, img_pair.device)
        down = ops.resize_planar_halfpixel(cams, edge.shape[1], edge.shape[2])
        rw = indexing.propagate_to_edge(down, edge, beta=beta, exp_times=exp_times, radius=5)
        return indexing.finish_semseg(rw, H, W, bg_thres, soft_output=soft_output)


def voc_color_map(n: int = 256) -> np.ndarray:
    """The PASCAL VOC palette (src/imutils.py color_map): the bits of the class index dealt round-robin to R, G, B from the
    top bit of each channel down."""
    cmap = np.zeros((n, 3), dtype=np.uint8)
    for i in range(n):
        c, rgb = i, [0, 0, 0]
        for j in range(8):
            for ch in range(3):
                rgb[ch] |= ((c >> ch) & 1) << (7 - j)
            c >>= 3
        cmap[i] = rgb
    return cmap


def save_palette_png(path: str, label) -> None:
    """infer_irn.py:92-95: the label map as a palette PNG (mode 'P', VOC colour map); np.array(Image.open(path)) gives the
    class indices back, which is what src/evaluation.py and src/data.py read."""
    import PIL.Image
    a = label.cpu().numpy() if torch.is_tensor(label) else np.asarray(label)
    if a.ndim != 2 or a.dtype != np.uint8:
        raise ValueError(f"label must be uint8 [H,W] (got {a.dtype} {a.shape})")
    im = PIL.Image.fromarray(a, mode="P")
    im.putpalette(voc_color_map().reshape(-1).tolist())
    im.save(path)
