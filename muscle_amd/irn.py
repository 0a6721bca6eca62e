"""The IRN edge / displacement network of infer_irn.py on the HIP path - `EdgeDisplacement` of
src/backbones/resnet50_irn.py:215-232 on src/backbones/resnet50.py (ResNet-50, frozen BatchNorm, strides (2,2,2,1), five
edge heads and seven displacement heads with GroupNorm) - and `infer_irn`, infer_irn.py:64-92 for one image.

`EdgeDisplacement` is a parameter container plus a HIP forward, like `muscle_amd.MuSCLe`: its sub-modules exist to hold the
tensors under the reference's names, none of them is ever called.  The reference registers the same sub-modules several
times (resnet50.* / stage1..5.* / backbone.*, fc_edge* / edge_layers.*, fc_dp* / dp_layers.*, mean_shift / fc_dp7.4), so
its checkpoints carry every tensor under two or three names; the containers here are shared in the same way, which gives
the same state_dict() key set and lets such a checkpoint load under strict=True.

Forward (NHWC fp32): stem = mx_stem7_im2col + the 1x1 GEMM with the folded BatchNorm + ReLU, mx_maxpool3s2;
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

    def stages(self, x: torch.Tensor):
        """resnet50_irn.py:110-114 on the zero-padded frame, NHWC: [x1..x5] of the frozen, folded backbone."""
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
        return xs

    def features(self, x: torch.Tensor):
        """resnet50_irn.py:109-130 on the zero-padded frame, NHWC: ([x1..x5], edge_cat, dp_cat1, dp_cat2)."""
        p = self._prep or self.prepare()
        xs = self.stages(x)
        N = x.shape[0]
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
            raise MuscleHipError("EdgeDisplacement is the inference network: call .eval(), or train the heads with AffinityDisplacementLoss / irn_step")
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


class AffinityDisplacementLoss(EdgeDisplacement):
    """resnet50_irn.py:143-212 on the HIP path: the network with its loss head, for training the twelve 1x1-conv + GroupNorm heads,
    fc_edge6 and the tail of fc_dp7.  Same containers and state_dict() keys as the reference class (the `path_indices{i}` and
    `disp_target` buffers included), so a checkpoint saved here loads into EdgeDisplacement with strict=False as infer_irn.py:41
    loads the reference's.

    The backbone stays frozen and folded (:109-114 detach every stage, :138-140 keep it in eval()): train() / eval() do not drop
    the folded weights, load_state_dict() and .to() do.  The head parameters are read live on every call.  The unreduced loss
    tensors of the reference's forward(x, True) do not exist here: `loss_backward` returns the four reduced terms and the total
    (the combination of the public IRN training loop; include/muscle_hip.h, mx_irn_loss_fwd) and leaves the gradients in .grad."""

    path_indices_prefix = "path_indices"

    def __init__(self, path_index, crop_size: int = 512):
        super().__init__(crop_size=crop_size)
        self.path_index = path_index
        self.n_path_lengths = len(path_index.path_indices)
        for i, pi in enumerate(path_index.path_indices):
            self.register_buffer(self.path_indices_prefix + str(i), torch.from_numpy(pi))
        self.register_buffer("disp_target", torch.from_numpy(path_index.search_dst).transpose(1, 0).unsqueeze(0).unsqueeze(-1).float())
        self._table = None
        self.train()

    def train(self, mode: bool = True):                                  # :138-140, without dropping the folded backbone
        nn.Module.train(self, mode)
        self.backbone.eval()
        return self

    def _apply(self, fn, *a, **k):
        self._table = None
        return super()._apply(fn, *a, **k)

    def trainable_parameters(self):                                      # :134-136
        return tuple(self.edge_layers.parameters()), tuple(self.dp_layers.parameters())

    # -- forward with the live head parameters; keeps what the backward needs --------------------------------------------
    @staticmethod
    def _live_head(x, seq, dst, coff, scale):
        conv, gn = seq[0], seq[1]
        N, H, W, C = x.shape
        co = conv.out_channels
        o = _pw(x.view(-1, C), _chunks(conv.weight.detach().reshape(co, -1)), co).view(N, H, W, co)
        stat = ops.gn_stats(o, gn.num_groups, gn.eps)
        ops.gn_resize(o, stat, gn.weight.detach(), gn.bias.detach(), dst, coff, scale, relu=True)
        return dict(seq=seq, x=x, o=o, stat=stat, dst=dst, coff=coff, scale=scale)

    def _run(self, x: torch.Tensor):
        xs = self.stages(x)
        N, dev = x.shape[0], x.device
        _, h2, w2, _ = xs[1].shape
        _, h3, w3, _ = xs[2].shape
        ecat = torch.empty(N, h2, w2, 160, dtype=torch.float32, device=dev)
        cat1 = torch.empty(N, h3, w3, 768, dtype=torch.float32, device=dev)
        cat2 = torch.empty(N, h2, w2, 448, dtype=torch.float32, device=dev)
        o7 = torch.empty(N, h2, w2, 256, dtype=torch.float32, device=dev)
        ctx = {"edge": [self._live_head(xs[i], getattr(self, f"fc_edge{i + 1}"), ecat, 32 * i, _EDGE_UP[i]) for i in range(5)]}
        dp = [None] * 7
        for j, i in enumerate((2, 3, 4)):
            dp[i] = self._live_head(xs[i], getattr(self, f"fc_dp{i + 1}"), cat1, 256 * j, _DP_UP[i])
        dp[0] = self._live_head(xs[0], self.fc_dp1, cat2, 0, 1)
        dp[1] = self._live_head(xs[1], self.fc_dp2, cat2, 64, 1)
        dp[5] = self._live_head(cat1, self.fc_dp6, cat2, 192, _DP_UP[5])
        dp[6] = self._live_head(cat2, self.fc_dp7, o7, 0, 1)
        we = torch.zeros(4, 160, device=dev)                              # the 1- and 2-channel tails as 4-column GEMMs (zero rows)
        we[:1] = self.fc_edge6.weight.detach().reshape(1, 160)
        be = torch.zeros(4, device=dev)
        be[:1] = self.fc_edge6.bias.detach()
        wd = torch.zeros(4, 256, device=dev)
        wd[:2] = self.fc_dp7[3].weight.detach().reshape(2, 256)
        eo = ops.pw_fwd(ecat.view(-1, 160), we, 4, bias=be).view(N, h2, w2, 4)
        do = ops.pw_fwd(o7.view(-1, 256), wd, 4).view(N, h2, w2, 4)
        ctx.update(xs=xs, dp=dp, ecat=ecat, cat1=cat1, cat2=cat2, o7=o7, we=we, wd=wd, eo=eo, do=do)
        return ctx

    def features(self, x: torch.Tensor):
        """([x1..x5], edge_cat, dp_cat1, dp_cat2) like EdgeDisplacement.features, but from the LIVE head parameters: the head
        weights that prepare() snapshots go stale with the first optimizer step (train() keeps the folded backbone on purpose)."""
        with torch.no_grad():
            c = self._run(x)
        return c["xs"], c["ecat"], c["cat1"], c["cat2"]

    def forward(self, x: torch.Tensor):
        """(edge_out [N,1,h,w] logits, dp_out [N,2,h,w]) of resnet50_irn.py:109-132 on the crop_size frame, no gradient; the mean
        shift is the identity in training mode and `- running_mean` in eval mode (:104-107)."""
        with torch.no_grad():
            c = self._run(x)
            edge = c["eo"][..., :1].permute(0, 3, 1, 2).contiguous()
            dp = c["do"][..., :2].permute(0, 3, 1, 2).contiguous()
            if not self.training:
                dp = dp - self.mean_shift.running_mean.view(1, 2, 1, 1)
            return edge, dp

    def _path_table(self, device):
        if self._table is None or self._table[0].device != device:
            self._table = self.path_index.offsets_table(device)
        return self._table

    @staticmethod
    def _head_backward(h, gdst):
        """Backward of one head from the gradient of the concatenation it wrote into: sets .grad of its convolution and GroupNorm,
        returns dX of the convolution's output (for a data gradient below, where a trainable head sits there)."""
        conv, gn = h["seq"][0], h["seq"][1]
        N, Hs, Ws, co = h["o"].shape
        dY = ops.gn_resize_bwd(gdst, h["dst"], h["coff"], co, Hs, Ws, h["scale"])
        dX, dgamma, dbeta = ops.gn_bwd(dY, h["o"], h["stat"], gn.weight.detach())
        gn.weight.grad, gn.bias.grad = dgamma, dbeta
        x2 = h["x"].view(-1, h["x"].shape[3])
        dW = torch.zeros(co, x2.shape[1], dtype=torch.float32, device=x2.device)
        ops.pw_wgrad(dX.view(-1, co), x2, dW)
        conv.weight.grad = dW.view_as(conv.weight)
        return dX.view(-1, co)

    def loss_backward(self, img: torch.Tensor, label: torch.Tensor) -> torch.Tensor:
        """Forward, loss and backward for img [N,3,S,S] and the reduced label map uint8 [N,S/4,S/4] (0..20, 255 = ignore).  Returns
        the device tensor float64 [5] = (pos_aff, neg_aff, dp_fg, dp_bg, total); every trainable parameter gets a fresh .grad.
        Every sum runs in this library's kernels in a fixed order except one: fc_edge6's bias gradient is torch's column sum of
        dE, whose order is torch's (a tree reduction without atomics, the same bits from run to run on one build of torch).
        Data gradients are formed only where a trainable head sits below (fc_dp7 -> cat2 -> fc_dp6 -> cat1); none into x1..x5."""
        if not self.training:
            raise MuscleHipError("AffinityDisplacementLoss.loss_backward: call .train() first (the mean shift is the identity in training)")
        with torch.no_grad():
            c = self._run(img)
            eo, do = c["eo"], c["do"]
            N, H, W, _ = eo.shape
            if label.dtype != torch.uint8 or tuple(label.shape) != (N, H, W) or not label.is_cuda:
                raise ValueError(f"label must be a CUDA uint8 [{N},{H},{W}] map (got {label.dtype} {tuple(label.shape)})")
            if tuple(self.path_index.size) != (H, W):
                raise ValueError(f"path_index was built for {self.path_index.size}, the network's output is {(H, W)}")
            label = label.contiguous()
            table, radius = self._path_table(img.device), self.path_index.radius
            res, amax = ops.irn_loss_fwd(eo, do, label, table, radius)
            dE, dD = ops.irn_loss_bwd(eo, do, label, table, radius, amax, res)
            del amax
            # fc_edge6 (160 -> 1, bias) as a 4-row weight
            dW = torch.zeros(4, 160, device=img.device)
            ops.pw_wgrad(dE, c["ecat"].view(-1, 160), dW)
            self.fc_edge6.weight.grad = dW[:1].reshape(1, 160, 1, 1).clone()
            self.fc_edge6.bias.grad = dE.sum(0)[:1]
            g_ecat = ops.pw_dgrad(dE, c["we"], 160).view(N, H, W, 160)
            for h in c["edge"]:
                self._head_backward(h, g_ecat)
            # the tail of fc_dp7 (256 -> 2), then fc_dp7 -> cat2 -> fc_dp1, fc_dp2, fc_dp6 -> cat1 -> fc_dp3..5
            dW = torch.zeros(4, 256, device=img.device)
            ops.pw_wgrad(dD, c["o7"].view(-1, 256), dW)
            self.fc_dp7[3].weight.grad = dW[:2].reshape(2, 256, 1, 1).clone()
            g_o7 = ops.pw_dgrad(dD, c["wd"], 256).view(N, H, W, 256)
            dp = c["dp"]
            dX7 = self._head_backward(dp[6], g_o7)
            g_cat2 = ops.pw_dgrad(dX7, self.fc_dp7[0].weight.detach().reshape(256, 448), 448).view(N, H, W, 448)
            self._head_backward(dp[0], g_cat2)
            self._head_backward(dp[1], g_cat2)
            dX6 = self._head_backward(dp[5], g_cat2)
            cat1 = dp[5]["x"]
            g_cat1 = ops.pw_dgrad(dX6, self.fc_dp6[0].weight.detach().reshape(256, 768), 768).view(cat1.shape)
            for i in (2, 3, 4):
                self._head_backward(dp[i], g_cat1)
            return res[:5]


_LOSS_NAMES = ("pos_aff_loss", "neg_aff_loss", "dp_fg_loss", "dp_bg_loss", "loss")


def irn_step(model: AffinityDisplacementLoss, optimizer, batch) -> Dict[str, torch.Tensor]:
    """One training step of the IRN heads: forward, loss, backward (gradients in .grad of the head parameters), optimizer.step().
    batch: {"img": [N,3,S,S] float, "label": uint8 [N,S/4,S/4]} on the device.  Returns the four loss terms and their total
    `loss` = (pos_aff + neg_aff)/2 + (dp_fg + dp_bg)/2 as device scalars (float64); nothing is read back to the host."""
    res = model.loss_backward(batch["img"], batch["label"])
    optimizer.step()
    return {k: res[i] for i, k in enumerate(_LOSS_NAMES)}


def cam_stack(cam_dict, H: int, W: int, device) -> torch.Tensor:
    """infer_irn.py:70-75: the {class: [H,W]} dict of infer_mcl.py as a dense [20,H,W] stack, zeros for absent classes."""
    a = np.zeros((20, H, W), np.float32)
    for k, v in cam_dict.items():
        a[int(k)] = v
    return torch.from_numpy(a).to(device)


def infer_irn(model: EdgeDisplacement, img_pair: torch.Tensor, cam_dict, *, beta=8, exp_times=6, bg_thres=0.35,
              soft_output=False, method: str = "dense", ins_seg=None):
    """infer_irn.py:64-92 for one image: the network, the CAM down-scaling (:76), the random walk (:77) and the label step
    (:79-92).  img_pair: [2,3,H,W] on the device; cam_dict: {class index: float32 [H,W]}.  Returns the uint8 label map [H,W]
    (and the fp16 [H,W,21] array with soft_output) on the device; soft_output="compact" gives the `softlabel.CompactSoft` (host
    arrays) in the array's place.  method: the walk of indexing.propagate_to_edge, "dense" (matrix squarings) or "stencil"
    (matrix-free).  ins_seg: None, or the keyword arguments {bg_thres, iterations, dp_thres} of
    `ins_seg.instances_from_field`: the same forward then also feeds the instance path (with this call's beta, exp_times and
    method) and (the result above, ins_seg.InstanceLabels) is returned."""
    H, W = img_pair.shape[2:]
    edge, dp = model(img_pair)
    with torch.no_grad():
        cams = cam_stack(cam_dict, H, W, img_pair.device)
        down = ops.resize_planar_halfpixel(cams, edge.shape[1], edge.shape[2])
        rw = indexing.propagate_to_edge(down, edge, beta=beta, exp_times=exp_times, radius=5, method=method)
        res = indexing.finish_semseg(rw, H, W, bg_thres, soft_output=soft_output)
    if ins_seg is None:
        return res
    from .ins_seg import instances_from_field
    keys = sorted(int(k) for k in cam_dict)                    # the planes of `down` the instance path needs: no second upload or resize
    return res, instances_from_field(edge, dp, cam_dict, H, W, beta=beta, exp_times=exp_times, method=method,
                                     down=down[keys].contiguous() if keys else None, **ins_seg)


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
