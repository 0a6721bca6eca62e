"""Plain-torch restatement of training the IRN heads: AffinityDisplacementLoss (src/backbones/resnet50_irn.py:143-212), the
affinity labels of GetAffinityLabelFromIndices (src/data.py:611-637), and the loss combination of the public IRN training loop
(the reference ships the model, not the loop):

    pos_aff = S(bg*pos)/(S bg + 1e-5)/2 + S(fg*pos)/(S fg + 1e-5)/2        neg_aff = S(neg*neg_loss)/(S neg + 1e-5)
    dp_fg = S(fg*fg_loss)/(2 S fg + 1e-5)     dp_bg = S(bg*bg_loss)/(2 S bg + 1e-5)     total = (pos_aff+neg_aff)/2 + (dp_fg+dp_bg)/2

dtype-generic: the fp64 CPU yardstick of the HIP path and its fp32 partner.  Builds on irn_net_ref (the network) without
editing it; tests/golden/irn_train.npz (tools/gen_irn_train_golden.py, the reference's own classes) pins it down.
"""
import numpy as np
import torch
import torch.nn.functional as F

import irn_net_ref as R

TERMS = ("pos_aff", "neg_aff", "dp_fg", "dp_bg", "total")


def search_paths(radius):
    """src/indexing.py:13-48: [(n_paths, length, 2) arrays by ascending length], destinations [n_dst, 2] as (dy, dx)."""
    dirs = [(0, x) for x in range(1, radius)]
    dirs += [(y, x) for y in range(1, radius) for x in range(-radius + 1, radius) if x * x + y * y < radius ** 2]
    by_len = {}
    for dy, dx in dirs:
        pts = [(y, x) for y in range(min(0, dy), max(0, dy) + 1) for x in range(min(0, dx), max(0, dx) + 1)
               if (dy * x - dx * y) ** 2 / (dy * dy + dx * dx) < 1]
        pts.sort(key=lambda c: -abs(c[0]) - abs(c[1]))
        by_len.setdefault(len(pts), []).append(pts)
    groups = [np.asarray(by_len[k]) for k in sorted(by_len)]
    return groups, np.concatenate([g[:, 0] for g in groups], axis=0)


def trainable_keys():
    """Canonical state_dict names of resnet50_irn.py:134-136, edge branch then displacement branch."""
    edge = [f"fc_edge{i}.{j}" for i in range(1, 6) for j in ("0.weight", "1.weight", "1.bias")] + ["fc_edge6.weight", "fc_edge6.bias"]
    dp = [f"fc_dp{i}.{j}" for i in range(1, 8) for j in ("0.weight", "1.weight", "1.bias")] + ["fc_dp7.3.weight"]
    return edge, dp


def window(t, dy, dx, rf):
    H, W = t.shape[-2:]
    return t[..., dy:dy + H - rf, rf + dx:rf + dx + W - 2 * rf]


def affinity_labels(label, radius):
    """label: integer array [N,H,W] -> (bg_pos, fg_pos, neg) boolean tensors [N, n_dst, n_src] (src/data.py:620-634)."""
    rf = radius - 1
    _groups, dst = search_paths(radius)
    lab = torch.as_tensor(np.asarray(label)).long()
    N = lab.shape[0]
    frm = window(lab, 0, 0, rf).reshape(N, 1, -1)
    to = torch.stack([window(lab, int(dy), int(dx), rf).reshape(N, -1) for dy, dx in dst], dim=1)
    valid = (frm < 21) & (to < 21)
    eq = frm == to
    return eq & valid & (frm == 0), eq & valid & (frm > 0), (~eq) & valid


def loss_head(edge_out, dp_out, label, radius):
    """edge_out [N,1,H,W] logits, dp_out [N,2,H,W] -> {sums: the five label-weighted sums and three counts, terms: TERMS}."""
    rf = radius - 1
    groups, dst = search_paths(radius)
    N = edge_out.shape[0]
    sig = torch.sigmoid(edge_out[:, 0])
    affs = []
    for g in groups:                                                          # to_affinity, :161-174
        dist = torch.stack([torch.stack([window(sig, int(dy), int(dx), rf).reshape(N, -1) for dy, dx in p], dim=1) for p in g], dim=1)
        affs.append(1 - F.max_pool2d(dist, (dist.shape[2], 1)).squeeze(2))
    aff = torch.cat(affs, dim=1)
    pos = -torch.log(aff + 1e-5)
    neg = -torch.log(1. + 1e-5 - aff)
    src = window(dp_out, 0, 0, rf)                                            # to_pair_displacement, :176-192
    pair = src.unsqueeze(2) - torch.stack([window(dp_out, int(dy), int(dx), rf) for dy, dx in dst], dim=2)
    pair = pair.reshape(N, 2, len(dst), -1)
    target = torch.as_tensor(dst.T.copy()).to(device=pair.device, dtype=pair.dtype).view(1, 2, -1, 1)    # disp_target, :157-159: component 0 = dy, 1 = dx
    fg_loss, bg_loss = (pair - target).abs(), pair.abs()
    bg, fg, ng = (t.to(pair.dtype) for t in affinity_labels(label, radius))
    s = dict(bg_pos=(bg * pos).sum(), fg_pos=(fg * pos).sum(), neg=(ng * neg).sum(), dp_fg=(fg_loss * fg.unsqueeze(1)).sum(),
             dp_bg=(bg_loss * bg.unsqueeze(1)).sum(), n_bg=bg.sum(), n_fg=fg.sum(), n_neg=ng.sum())
    pos_aff = s["bg_pos"] / (s["n_bg"] + 1e-5) / 2 + s["fg_pos"] / (s["n_fg"] + 1e-5) / 2
    neg_aff = s["neg"] / (s["n_neg"] + 1e-5)
    dp_fg = s["dp_fg"] / (2 * s["n_fg"] + 1e-5)
    dp_bg = s["dp_bg"] / (2 * s["n_bg"] + 1e-5)
    total = (pos_aff + neg_aff) / 2 + (dp_fg + dp_bg) / 2
    return dict(sums=s, terms=dict(zip(TERMS, (pos_aff, neg_aff, dp_fg, dp_bg, total))))


def loss_head_grads(edge_out, dp_out, label, radius, dtype):
    """The loss head alone: (terms as floats-in-dtype tensors, d total / d edge_out, d total / d dp_out)."""
    e = torch.as_tensor(np.asarray(edge_out)).to(dtype).requires_grad_(True)
    d = torch.as_tensor(np.asarray(dp_out)).to(dtype).requires_grad_(True)
    out = loss_head(e, d, label, radius)
    ge, gd = torch.autograd.grad(out["terms"]["total"], (e, d), allow_unused=True)
    ge = torch.zeros_like(e) if ge is None else ge
    gd = torch.zeros_like(d) if gd is None else gd
    return {k: v.detach() for k, v in out["terms"].items()}, {k: v.detach() for k, v in out["sums"].items()}, ge, gd


def train_forward(sd, x):
    """resnet50_irn.py:109-132 in training mode: R.net with the mean shift the identity (:105-106)."""
    sd = dict(sd)
    sd["mean_shift.running_mean"] = torch.zeros_like(sd["mean_shift.running_mean"])
    e, d, _named = R.net(sd, x)
    return e, d


def step(sd_np, x, label, radius, dtype):
    """Forward, loss, backward of the whole network on the (already crop_size) frame x: (terms, {key: grad}, dedge, ddp)."""
    sd = R.to_dtype(sd_np, dtype)
    keys = [k for grp in trainable_keys() for k in grp]
    for k in keys:
        sd[k] = sd[k].clone().requires_grad_(True)
    e, d = train_forward(sd, torch.as_tensor(np.asarray(x)).to(dtype))
    e.retain_grad()
    d.retain_grad()
    out = loss_head(e, d, label, radius)
    out["terms"]["total"].backward()
    return {k: v.detach() for k, v in out["terms"].items()}, {k: sd[k].grad for k in keys}, e.grad, d.grad


def poly_sgd(params, grads_per_step, lrs, momentum, max_step, power=0.9):
    """torch.optim.SGD(params, lr, momentum) with zero weight decay under src/torchutils.py:23-33's schedule, written out:
    params / grads: lists of lists (one list per group) of float tensors.  Returns the parameters after every step."""
    params = [[p.clone() for p in grp] for grp in params]
    bufs = [[None] * len(grp) for grp in params]
    out = []
    for step_i, grads in enumerate(grads_per_step):
        mult = (1 - step_i / max_step) ** power if step_i < max_step else None
        for gi, grp in enumerate(params):
            if mult is not None:
                lr = lrs[gi] * mult
            for pi, p in enumerate(grp):
                g = grads[gi][pi]
                bufs[gi][pi] = g.clone() if bufs[gi][pi] is None else bufs[gi][pi] * momentum + g
                grp[pi] = p - lr * bufs[gi][pi]
        out.append([[p.clone() for p in grp] for grp in params])
    return out
