"""numpy restatement of the image-stage rule of include/muscle_hip.h (mx_input_stage), for the tests of the job format."""
import numpy as np

MEAN, STD = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])


def input_stage_ref(src: np.ndarray, job, Hd: int, Wd: int) -> np.ndarray:
    """float32 [3, Hd, Wd] of one 12-word job over the uint8 bytes `src`."""
    src_off, stride, step, top, left, h, w, eyx, ehw = (int(v) for v in job[:9])
    y, x = np.mgrid[0:Hd, 0:Wd]
    inside = (y >= top) & (y < top + h) & (x >= left) & (x < left + w)
    at = np.where(inside, src_off + ((y - top) * stride + (x - left) * step) * 3, 0)
    px = src[at[..., None] + np.arange(3)]
    out = np.where(inside[..., None], ((px / 255.0 - MEAN) / STD).astype(np.float32), np.float32(0))
    ey, ex, eh, ew = eyx & 0xFFFF, eyx >> 16, ehw & 0xFFFF, ehw >> 16
    out[(y >= ey) & (y < ey + eh) & (x >= ex) & (x < ex + ew)] = 0
    return np.ascontiguousarray(out.transpose(2, 0, 1))
