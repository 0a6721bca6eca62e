"""What the device input paths share (muscle_amd._stage): the layout and the pinned double buffering of StageBuffer, the image
job of mx_input_stage as its one writer makes it (against the numpy restatement of the header's rule, tests/input_stage_ref.py),
and the one random_crop_box behind both of its forms.  No GPU."""
import random

import numpy as np
import pytest
import torch

from input_stage_ref import MEAN, STD, input_stage_ref


def _buffer():
    from muscle_amd._stage import StageBuffer
    return StageBuffer(torch.device("cpu"))


def test_layout_alignment_order_and_last_bytes():
    sb = _buffer()
    sb.plan()
    want = [(3 * 48, 64), (5, 16), (32, 64), (1001, 16), (7, 4), (64, 64)]
    copied = [(sb.reserve(n, a), n, a) for n, a in want]
    scratch = [(sb.scratch(n, a), n, a) for n, a in ((333, 16), (24, 8), (100, 64))]
    for off, n, a in copied + scratch:
        assert off % a == 0
    spans = sorted((off, off + n) for off, n, _ in copied + scratch)
    assert all(e0 <= s1 for (_, e0), (s1, _) in zip(spans, spans[1:]))                    # disjoint
    end = max(off + n for off, n, _ in copied)
    assert all(off >= end for off, _, _ in scratch)                                        # scratch behind the copied bytes
    assert sb.copied == end and sb.total == max(off + n for off, n, _ in scratch)
    with pytest.raises(RuntimeError):
        sb.reserve(4)                                                                      # no copied region after scratch
    buf = sb.begin()
    assert buf.dtype == np.uint8 and buf.shape == (end,)
    buf[:] = np.arange(end, dtype=np.uint8)
    sb.upload()
    assert sb.last_bytes == end and sb._dev_buf.numel() >= sb.total
    assert np.array_equal(sb._dev_buf[:end].numpy(), np.arange(end, dtype=np.uint8))
    sb.plan()
    assert sb.reserve(8) == 0                                                              # a new batch starts over


def test_2gib_is_refused_before_any_allocation():
    for copied, scratch in ((2 ** 31, 0), (2 ** 31 - 4096, 4096), (1024, 2 ** 31)):
        sb = _buffer()
        sb.plan()
        sb.reserve(copied)
        if scratch:
            sb.scratch(scratch)
        with pytest.raises(ValueError, match="batch sources exceed 2 GiB"):
            sb.begin()
        assert sb._pin == [None, None] and sb._dev_buf is None
    sb = _buffer()
    sb.plan()
    sb.reserve(64)
    sb.scratch(2 ** 31 - 1 - 64)                                                           # the largest total int32 offsets reach
    assert sb.begin().size == 64


def test_pinned_buffers_alternate_and_grow():
    sb = _buffer()
    seen = []
    for _ in range(3):
        sb.plan()
        sb.reserve(1000)
        seen.append(sb.begin())
        sb.upload()
    assert not np.shares_memory(seen[0], seen[1]) and np.shares_memory(seen[0], seen[2])
    assert seen[0].ctypes.data == seen[2].ctypes.data
    cap = sb._pin[0].numel()
    assert cap >= 1000 and cap % 4096 == 0
    sb.plan()
    sb.reserve(10 * cap)
    sb.scratch(123)
    big = sb.begin()                                                                       # a larger batch after a smaller one
    assert big.size == 10 * cap and sb._pin[1].numel() >= 10 * cap * 5 // 4 and sb._pin[1].numel() % 4096 == 0
    big[-1] = 7
    sb.upload()
    assert sb.last_bytes == 10 * cap and sb._dev_buf.numel() >= 10 * cap + 123 and int(sb._dev_buf[10 * cap - 1]) == 7


# ---- the image job -------------------------------------------------------------------------------------------------------
def _norm(a):
    return np.ascontiguousarray(((a / 255.0 - MEAN) / STD).astype(np.float32).transpose(2, 0, 1))


def test_image_job_places_flips_strides_and_erases():
    from muscle_amd._stage import input_stage_job
    g = np.random.default_rng(3)
    Hd, Wd, pre = 13, 17, 5                                                                # the image starts 5 bytes into src
    img = g.integers(0, 256, (9, 11, 3), dtype=np.uint8)
    src = np.concatenate([np.full(pre, 255, np.uint8), img.reshape(-1)])
    # a packed crop with a zero border on all four sides
    top, left = 2, 3
    plain = input_stage_ref(src, input_stage_job(pre, 11, top, left, 9, 11), Hd, Wd)
    want = np.zeros((3, Hd, Wd), np.float32)
    want[:, top:top + 9, left:left + 11] = _norm(img)
    assert plain.dtype == np.float32 and np.array_equal(plain, want)
    assert (want[:, 0] == 0).all() and (want[:, -1] == 0).all() and (want[:, :, 0] == 0).all() and (want[:, :, -1] == 0).all()
    # the same crop, the container flipped
    flipped = input_stage_ref(src, input_stage_job(pre, 11, top, left, 9, 11, flip_width=Wd), Hd, Wd)
    assert np.array_equal(flipped, np.ascontiguousarray(np.flip(plain, -1)))
    assert np.array_equal(flipped.transpose(1, 2, 0), np.fliplr(plain.transpose(1, 2, 0)))
    # a crop [4, 6] at (3, 2) inside the image: the row stride exceeds the window width; plain and flipped
    it, il, ch, cw = 3, 2, 4, 6
    off = pre + (it * 11 + il) * 3
    want = np.zeros((3, Hd, Wd), np.float32)
    want[:, 1:1 + ch, 8:8 + cw] = _norm(img[it:it + ch, il:il + cw])
    inner = input_stage_ref(src, input_stage_job(off, 11, 1, 8, ch, cw), Hd, Wd)
    assert np.array_equal(inner, want)
    assert np.array_equal(input_stage_ref(src, input_stage_job(off, 11, 1, 8, ch, cw, flip_width=Wd), Hd, Wd), np.flip(want, -1))
    # an erase box over the window's right edge and one over the container's bottom-right corner
    for box in ((0, 12, 5, 4), (9, 10, 30, 30)):
        ey, ex, eh, ew = box
        want = plain.copy()
        want[:, ey:ey + eh, ex:ex + ew] = 0
        got = input_stage_ref(src, input_stage_job(pre, 11, top, left, 9, 11, erase=box), Hd, Wd)
        assert np.array_equal(got, want) and not np.array_equal(got, plain)
    job = input_stage_job(pre, 11, top, left, 9, 11, flip_width=Wd, erase=(1, 2, 3, 4))
    assert len(job) == 12 and job[2] == -1 and job[7:] == (1 | 2 << 16, 3 | 4 << 16, 0, 0, 0)


def test_one_random_crop_box_behind_both_forms():
    from muscle_amd import data, train_irn
    for seed, (h, w, crop) in enumerate([(75, 100, 32), (75, 100, 160), (90, 40, 64), (64, 64, 64), (33, 200, 100)] * 3):
        a, b = random.Random(seed), random.Random(seed)
        ct, cl, it, il, ch, cw = data.random_crop_box(h, w, crop, a)
        assert train_irn.random_crop_box(h, w, crop, b) == (ct, ct + ch, cl, cl + cw, it, it + ch, il, il + cw)
        assert a.getstate() == b.getstate() and (ch, cw) == (min(crop, h), min(crop, w))
    random.seed(11)
    box = data.random_crop_box(75, 100, 64)                                                # the default generator is `random`
    assert box == data.random_crop_box(75, 100, 64, random.Random(11))
