"""What the device input paths share (`data.InputStager` / `MSFStager`, `segdata.SegStager`, `irndata.IrnStager`): the one
staging buffer of a batch and the writers of the job formats more than one stager uses.

A stager plans the layout of a batch, packs jobs, tables and uint8 sources into pinned memory, uploads them in ONE copy and
launches the `mx_*` kernels with the buffer's base pointer: every offset in a job is a byte offset from that base (int32 in
the job structs, hence the 2 GiB guard), table offsets are int32 words from it.
"""
from __future__ import annotations

import numpy as np
import torch


def _al(n: int, a: int = 16) -> int:
    return (n + a - 1) // a * a


class StageBuffer:
    """Two pinned host buffers that alternate (packing batch t+1 does not wait for the copy of batch t), one device buffer,
    one event per pinned buffer; all three grow to the largest batch seen.  Per batch:
        plan();  off = reserve(nbytes) ...;  off = scratch(nbytes) ...;  buf = begin();  <pack buf>;  base = upload()
    `reserve`d regions are copied; `scratch` regions exist on the device only, behind the copied bytes (resized images,
    horizontal-pass temporaries, the jitter's sums).  The copy goes on the current stream, as the kernels that follow do.
    Without a GPU the "pinned" buffers are plain memory and no event is made: layout and packing run anywhere."""

    def __init__(self, device):
        self.dev = device
        self._pin = [None, None]
        self._evt = [None, None]
        self._dev_buf = None
        self._k = 1
        self.copied = self.total = 0                        # planned bytes: the copy, the copy + scratch
        self.last_bytes = 0                                 # bytes of the last batch's one host-to-device copy
        self.base = None                                    # device address of the last upload

    def plan(self) -> None:
        self.copied = self.total = 0

    def reserve(self, nbytes: int, align: int = 16) -> int:
        """Byte offset of a new copied region (64-byte alignment for job arrays)."""
        if self.total != self.copied:
            raise RuntimeError("copied regions come before all scratch regions")
        off = _al(self.copied, align)
        self.copied = self.total = off + int(nbytes)
        return off

    def scratch(self, nbytes: int, align: int = 16) -> int:
        """Byte offset of a new device-only region."""
        off = _al(self.total, align)
        self.total = off + int(nbytes)
        return off

    def begin(self) -> np.ndarray:
        """The pinned bytes [copied] to pack this batch into."""
        if self.total >= 2 ** 31:
            raise ValueError("batch sources exceed 2 GiB")
        self._k ^= 1
        k = self._k
        if self._evt[k] is not None:
            self._evt[k].synchronize()                      # the copy out of this pinned buffer two batches ago is done
        if self._pin[k] is None or self._pin[k].numel() < self.copied:
            t = torch.empty(_al(self.copied * 5 // 4, 4096), dtype=torch.uint8)
            self._pin[k] = t.pin_memory() if torch.cuda.is_available() else t
        return self._pin[k].numpy()[:self.copied]

    def upload(self) -> int:
        """One non-blocking copy of the packed bytes; returns the device base address of the batch."""
        if self._dev_buf is None or self._dev_buf.numel() < self.total:
            self._dev_buf = torch.empty(_al(self.total * 5 // 4, 4096), dtype=torch.uint8, device=self.dev)
        k = self._k
        self._dev_buf[:self.copied].copy_(self._pin[k][:self.copied], non_blocking=True)
        self.last_bytes = self.copied
        if torch.cuda.is_available():
            self._evt[k] = torch.cuda.Event()
            self._evt[k].record()
        self.base = self._dev_buf.data_ptr()
        return self.base


# ---- job formats (include/muscle_hip.h) ----------------------------------------------------------------------------------
def resample_job(src_off: int, hin: int, win: int, tmp_off: int, dst_off: int, wout: int, hout: int, tab_off: int):
    """mx_resample: {src_off, Hin, Win, tmp_off, dst_off, Wout, Hout, tab_off} - uint8 HWC [Hin,Win,3] at src_off through
    the horizontal pass ([Hin,Wout,3] at tmp_off) to [Hout,Wout,3] at dst_off; byte offsets, but the table (`tab_off` is
    given in bytes here) in int32 words."""
    return src_off, hin, win, tmp_off, dst_off, wout, hout, tab_off // 4


def jitter_job(off: int, h: int, w: int, params) -> np.ndarray:
    """mx_color_jitter: {off, h, w, order, brightness, contrast, saturation (float32), hue shift 0..255} as 8 int32 words -
    `params` of `data.color_jitter_params` for the image [h,w,3] at byte offset off; order holds one nibble per position
    (0 brightness, 1 contrast, 2 saturation, 3 hue, 15 nothing).  params None: a job that does nothing."""
    job = np.zeros(8, dtype=np.int32)
    if params is None:
        job[3] = 0xFFFF
        return job
    order, fb, fc, fs, fh = params
    code = 0
    for pos in range(4):
        fn = order[pos]
        code |= (fn if (fb, fc, fs, fh)[fn] is not None else 15) << (4 * pos)
    job[:4] = (off, h, w, code)
    job.view(np.float32)[4:7] = (fb or 0.0, fc or 0.0, fs or 0.0)
    job[7] = (int(fh * 255) & 0xFF) if fh is not None else 0
    return job


def input_stage_job(src_off: int, row_stride: int, top: int, left: int, h: int, w: int, flip_width=None, erase=None):
    """mx_input_stage: {src_off, row_stride, col_step, top, left, h, w, ey | ex << 16, eh | ew << 16, 0, 0, 0} for the crop
    [h,w] whose first pixel is at byte src_off of a uint8 HWC image with `row_stride` pixels per row, pasted at (top, left)
    of the container.  flip_width: the container's width when the container is then flipped (np.fliplr): the window moves
    to flip_width - left - w and is read from the crop's last column backwards.  erase = (y, x, h, w) of RandomErasing's
    box in output coordinates."""
    step = 1
    if flip_width is not None:
        src_off, left, step = src_off + (w - 1) * 3, flip_width - left - w, -1
    ey, ex, eh, ew = erase if erase is not None else (0, 0, 0, 0)
    return src_off, row_stride, step, top, left, h, w, ey | (ex << 16), eh | (ew << 16), 0, 0, 0
