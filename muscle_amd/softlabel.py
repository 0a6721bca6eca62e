"""The compact soft pseudo-label: what `infer_irn --soft_output 2` writes and `train_muscle --mask_root` reads instead of the
float16 [H,W,21] array of `infer_irn.py:79-88`.

The dense array is a deterministic function of the random-walk maps of the classes that are present: their 4x bilinear
upsample, cropped to [H,W], divided by one global maximum, with a constant threshold plane in front.  `CompactSoft` keeps
exactly those inputs - the fp32 maps `rw [K,h,w]` as the device held them, their class indices, the maximum
`mx_irn_finish` divided by and the threshold - and `mx_soft_expand` (csrc/softlabel.hip) re-creates the float16 rows with
the arithmetic of `mx_irn_finish` (csrc/irn_soft.h, included by both), bit for bit.  At 375x500 that is 47 KB per present
class instead of 7.9 MB.

One uncompressed `<name>.npz` per image, plain arrays only (read with allow_pickle=False):
    version int32 (1) | keys uint8 [K] ascending | rw float32 [K,h,w] | size int32 [2] = (H, W) | vmax float32 | bg float32 |
    channels int32

  python -m muscle_amd.softlabel unpack IN_DIR OUT_DIR [--list LIST]
writes the reference's `<name>.npy` (float16 [H,W,21]) from compact files, on the GPU: what the reference's own
train_muscle.py reads.  The expansion exists as the HIP kernel only.
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import List, Optional, Tuple

import numpy as np
import torch

from ._lib import MuscleHipError, call, stream

VERSION = 1
JOB_WORDS = 16


class CompactSoft:
    """keys uint8 [K] ascending: class indices 0..channels-2 of the stored maps (channel keys[i] + 1 of the dense label);
    rw float32 [K,h,w] C-contiguous: the walk result of those classes; size = (H, W) of the dense label; vmax: the value
    mx_irn_finish divides by; bg: the background threshold (both float32); channels: width of the dense label."""
    __slots__ = ("keys", "rw", "size", "vmax", "bg", "channels")

    def __init__(self, keys, rw, size, vmax, bg, channels: int = 21):
        self.keys = np.ascontiguousarray(keys, dtype=np.uint8)
        self.rw = np.ascontiguousarray(rw, dtype=np.float32)
        self.size = (int(size[0]), int(size[1]))
        self.vmax, self.bg, self.channels = np.float32(vmax), np.float32(bg), int(channels)

    @property
    def nbytes(self) -> int:
        """Bytes a stager ships for this label: rw, then keys."""
        return self.rw.nbytes + self.keys.nbytes


def _check(cs: CompactSoft, what: str) -> CompactSoft:
    H, W = cs.size
    if cs.rw.ndim != 3 or cs.keys.ndim != 1 or cs.keys.shape[0] != cs.rw.shape[0]:
        raise ValueError(f"{what}: keys {cs.keys.shape} / rw {cs.rw.shape} are not [K] / [K,h,w]")
    if not 2 <= cs.channels <= 256:
        raise ValueError(f"{what}: channels={cs.channels} outside 2..256")
    k = cs.keys.astype(np.int64)
    if np.any(np.diff(k) <= 0) or (k.size and k[-1] >= cs.channels - 1):
        raise ValueError(f"{what}: keys {k.tolist()} must ascend and stay below channels - 1 = {cs.channels - 1}")
    h, w = cs.rw.shape[1:]
    if H < 1 or W < 1 or H > 4 * h or W > 4 * w:
        raise ValueError(f"{what}: size {cs.size} is not a crop of the 4x upsampled {h}x{w} maps")
    if not np.isfinite(cs.vmax) or cs.vmax <= 0:
        raise ValueError(f"{what}: vmax={cs.vmax} must be finite and positive")
    return cs


def save_compact(path: str, cs: CompactSoft) -> None:
    """One uncompressed .npz of plain arrays (np.savez appends '.npz' to a path without it)."""
    _check(cs, "save_compact")
    np.savez(path, version=np.int32(VERSION), keys=cs.keys, rw=cs.rw, size=np.asarray(cs.size, dtype=np.int32),
             vmax=np.float32(cs.vmax), bg=np.float32(cs.bg), channels=np.int32(cs.channels))


_FIELDS = {"version": np.int32, "keys": np.uint8, "rw": np.float32, "size": np.int32, "vmax": np.float32, "bg": np.float32,
           "channels": np.int32}


def load_compact(path: str) -> CompactSoft:
    """Raises ValueError on an unknown version, a field of another dtype, keys that do not ascend or reach channels - 1, a size
    beyond the 4x upsampled maps, or a vmax that is not finite and positive."""
    with np.load(path, allow_pickle=False) as z:
        missing = [k for k in _FIELDS if k not in z.files]
        if missing:
            raise ValueError(f"{path}: not a compact soft label (no {missing})")
        a = {k: z[k] for k in _FIELDS}
    for k, dt in _FIELDS.items():
        if a[k].dtype != dt:
            raise ValueError(f"{path}: {k} is {a[k].dtype}, not {np.dtype(dt)}")
    if a["version"].shape != () or int(a["version"]) != VERSION:
        raise ValueError(f"{path}: version {a['version']} (this build reads {VERSION})")
    if a["size"].shape != (2,) or any(a[k].shape != () for k in ("vmax", "bg", "channels")):
        raise ValueError(f"{path}: size / vmax / bg / channels have the wrong shape")
    return _check(CompactSoft(a["keys"], a["rw"], a["size"], a["vmax"], a["bg"], int(a["channels"])), path)


def expand_job(cs: CompactSoft, src_off: int, dst_off: int, rows: Tuple[int, int]) -> np.ndarray:
    """One mx_soft_expand job (include/muscle_hip.h) for rw at byte src_off, keys straight behind it, the float16
    [r1-r0, W, channels] output at byte dst_off."""
    r0, r1 = rows
    H, W = cs.size
    if not 0 <= r0 < r1 <= H:
        raise ValueError(f"rows {rows} outside the {H} rows of the label")
    if src_off % 4 or dst_off % 16:
        raise ValueError("mx_soft_expand: rw must be 4-byte and the output 16-byte aligned")
    K, h, w = cs.rw.shape
    job = np.zeros(JOB_WORDS, dtype=np.int32)
    job[:11] = (src_off, src_off + cs.rw.nbytes, K, h, w, H, W, r0, r1 - r0, dst_off, cs.channels)
    job.view(np.float32)[11:13] = (cs.vmax, cs.bg)
    return job


def pack_compact(buf: np.ndarray, off: int, cs: CompactSoft) -> None:
    """rw, then keys, at byte `off` of a uint8 staging buffer: cs.nbytes bytes."""
    n = cs.rw.nbytes
    buf[off:off + n] = cs.rw.reshape(-1).view(np.uint8)
    buf[off + n:off + n + cs.keys.size] = cs.keys


def expand(cs: CompactSoft, device, rows: Optional[Tuple[int, int]] = None) -> torch.Tensor:
    """Rows r0:r1 (default all) of the dense label as a float16 [r1-r0, W, channels] tensor on `device`, through
    mx_soft_expand: the bits mx_irn_finish wrote into the dense array."""
    device = torch.device(device)
    if device.type != "cuda":
        raise MuscleHipError("softlabel.expand runs on the HIP kernel only; there is no CPU path")
    _check(cs, "expand")
    r0, r1 = (0, cs.size[0]) if rows is None else (int(rows[0]), int(rows[1]))
    src_off = 64
    dst_off = (src_off + cs.nbytes + 15) // 16 * 16
    n_out = (r1 - r0) * cs.size[1] * cs.channels * 2
    host = np.zeros(dst_off, dtype=np.uint8)
    host[:64].view(np.int32)[:] = expand_job(cs, src_off, dst_off, (r0, r1))
    pack_compact(host, src_off, cs)
    if dst_off + n_out >= 2 ** 31:
        raise ValueError("label exceeds 2 GiB")
    buf = torch.empty(dst_off + n_out, dtype=torch.uint8, device=device)
    buf[:dst_off].copy_(torch.from_numpy(host))
    with torch.cuda.device(device):
        call("mx_soft_expand", buf.data_ptr(), buf.data_ptr(), 1, stream())
    return buf[dst_off:].view(torch.float16).view(r1 - r0, cs.size[1], cs.channels)


def unpack(in_dir: str, out_dir: str, names: Optional[List[str]] = None, device="cuda:0") -> int:
    """<in_dir>/<name>.npz -> <out_dir>/<name>.npy, float16 [H,W,channels]: the files infer_irn.py --soft_output 1 writes."""
    if names is None:
        names = sorted(f[:-4] for f in os.listdir(in_dir) if f.endswith(".npz"))
    os.makedirs(out_dir, exist_ok=True)
    for it, name in enumerate(names):
        cs = load_compact(os.path.join(in_dir, name + ".npz"))
        np.save(os.path.join(out_dir, name + ".npy"), expand(cs, device).cpu().numpy())
        print(name, it, flush=True)
    return len(names)


def parse_args(argv: Optional[List[str]] = None):
    ap = argparse.ArgumentParser(prog="python -m muscle_amd.softlabel", description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    up = sub.add_parser("unpack", help="write the dense <name>.npy (float16 [H,W,21]) of every compact <name>.npz")
    up.add_argument("in_dir")
    up.add_argument("out_dir")
    up.add_argument("--list", default=None, help="image list (one name or VOC path per line); default: every .npz of IN_DIR")
    return ap.parse_args(argv)


def main(argv: Optional[List[str]] = None) -> int:
    args = parse_args(argv)
    names = None
    if args.list:
        from .infer_seg import read_names
        names = read_names(args.list)
    unpack(args.in_dir, args.out_dir, names)
    return 0


if __name__ == "__main__":
    sys.exit(main())
