"""Plain-torch restatement of the IRN edge / displacement network (src/backbones/resnet50_irn.py:215-232 on
src/backbones/resnet50.py) and of infer_irn.py:64-92 for one image, dtype-generic: the CPU yardstick of the HIP path
(fp64) and its fp32 partner.  Written from the layer shapes; it reads a state dict by its first (canonical) names and
owns no module.  The random walk and the label step are the oracle's (oracle/mcl_oracle.py), which are dtype-generic too.
"""
import numpy as np
import torch
import torch.nn.functional as F

LAYERS = ((64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 1))          # planes, blocks, stride: strides (2,2,2,1), :12
EDGE_UP = (1, 1, 2, 4, 4)                                              # resnet50_irn.py:22-49
EDGE_G = 4
DP_G = (8, 16, 16, 16, 16, 16, 16)                                     # :53-92
DP_UP = (1, 1, 1, 2, 2, 2, 1)


def to_dtype(sd, dtype, device="cpu"):
    return {k: (torch.as_tensor(np.asarray(v)).to(device) if str(np.asarray(v).dtype).startswith("int")
                else torch.as_tensor(np.asarray(v)).to(device=device, dtype=dtype)) for k, v in sd.items()}


def _bn(sd, p, x):                                                     # FixedBatchNorm, resnet50.py:11-14 (eps 1e-5)
    return F.batch_norm(x, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], False, 0.0, 1e-5)


def bottleneck(sd, p, x, stride, down):                                # resnet50.py:34-54
    o = F.relu(_bn(sd, p + "bn1", F.conv2d(x, sd[p + "conv1.weight"])))
    o = F.relu(_bn(sd, p + "bn2", F.conv2d(o, sd[p + "conv2.weight"], stride=stride, padding=1)))
    o = _bn(sd, p + "bn3", F.conv2d(o, sd[p + "conv3.weight"]))
    r = _bn(sd, p + "downsample.1", F.conv2d(x, sd[p + "downsample.0.weight"], stride=stride)) if down else x
    return F.relu(o + r)


def stages(sd, x):
    """x [B,3,S,S] (already padded) -> [x1..x5] (resnet50_irn.py:110-114)."""
    x1 = F.relu(_bn(sd, "resnet50.bn1", F.conv2d(x, sd["resnet50.conv1.weight"], stride=2, padding=3)))
    x1 = F.max_pool2d(x1, 3, 2, 1)
    out = [x1]
    h = x1
    for li, (_planes, blocks, stride) in enumerate(LAYERS, 1):
        for b in range(blocks):
            h = bottleneck(sd, f"resnet50.layer{li}.{b}.", h, stride if b == 0 else 1, b == 0)
        out.append(h)
    return out


def head(sd, p, x, groups, up, relu=True):
    """Conv1x1 -> GroupNorm -> [Upsample] -> ReLU (the order of resnet50_irn.py:32-37)."""
    o = F.group_norm(F.conv2d(x, sd[p + ".0.weight"]), groups, sd[p + ".1.weight"], sd[p + ".1.bias"], 1e-5)
    if up != 1:
        o = F.interpolate(o, scale_factor=up, mode="bilinear", align_corners=False)
    return F.relu(o) if relu else o


def net(sd, x):
    """resnet50_irn.py:109-132 in eval mode on the padded frame: (edge_out [B,1,h,w], dp_out [B,2,h,w], named intermediates)."""
    xs = stages(sd, x)
    e = [head(sd, f"fc_edge{i + 1}", xs[i], EDGE_G, EDGE_UP[i]) for i in range(5)]
    hh, ww = e[1].shape[2:]
    ecat = torch.cat([e[0], e[1]] + [t[..., :hh, :ww] for t in e[2:]], dim=1)
    edge_out = F.conv2d(ecat, sd["fc_edge6.weight"], sd["fc_edge6.bias"])
    d = [head(sd, f"fc_dp{i + 1}", xs[i], DP_G[i], DP_UP[i]) for i in range(5)]
    h3, w3 = d[2].shape[2:]
    cat1 = torch.cat([d[2], d[3][..., :h3, :w3], d[4][..., :h3, :w3]], dim=1)
    h2, w2 = d[1].shape[2:]
    up3 = head(sd, "fc_dp6", cat1, DP_G[5], DP_UP[5])[..., :h2, :w2]
    cat2 = torch.cat([d[0], d[1], up3], dim=1)
    o = head(sd, "fc_dp7", cat2, DP_G[6], 1)
    dp_out = F.conv2d(o, sd["fc_dp7.3.weight"]) - sd["mean_shift.running_mean"].view(1, 2, 1, 1)
    named = [(f"x{i + 1}", t) for i, t in enumerate(xs)] + [("edge_cat", ecat), ("dp_cat1", cat1), ("dp_cat2", cat2)]
    return edge_out, dp_out, named


def edge_displacement(sd, x, crop_size=512, stride=4, want_named=False):
    """EdgeDisplacement.forward (resnet50_irn.py:222-232): x [2,3,H,W] -> (edge [1,h,w], dp [2,h,w])."""
    fh, fw = (x.shape[2] - 1) // stride + 1, (x.shape[3] - 1) // stride + 1
    xp = F.pad(x, [0, crop_size - x.shape[3], 0, crop_size - x.shape[2]])
    e, d, named = net(sd, xp)
    e, d = e[..., :fh, :fw], d[..., :fh, :fw]
    edge = torch.sigmoid(e[0] / 2 + e[1].flip(-1) / 2)
    return (edge, d[0], named) if want_named else (edge, d[0])


def cam_stack(cam_dict, H, W, dtype):
    a = np.zeros((20, H, W), np.float32)                                # infer_irn.py:70-73
    for k, v in cam_dict.items():
        a[k] = v
    return torch.from_numpy(a).to(dtype)


def infer_irn(sd, x, cam_dict, beta=8, exp_times=6, bg_thres=0.35, crop_size=512):
    """infer_irn.py:64-92 for one image: (label uint8 [H,W], soft fp16 [H,W,21], rw_up_bg [21,H,W] in the working dtype)."""
    from oracle import mcl_oracle as O
    H, W = x.shape[2:]
    edge, _dp = edge_displacement(sd, x, crop_size)
    cams = cam_stack(cam_dict, H, W, x.dtype)
    down = F.interpolate(cams.unsqueeze(0), size=edge.shape[1:], mode="bilinear", align_corners=False)
    rw = O.irn_propagate_to_edge(down, edge, 5, beta, exp_times)
    label, soft = O.irn_finish(rw, H, W, bg_thres)
    return label, soft, edge
