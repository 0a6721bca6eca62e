"""Writes tests/golden/ir_label.npz from the fp64 restatement in tests/ir_label_ref.py alone (no GPU, no reference code):
for every case of ir_label_ref.CASES the inputs (img uint8, cams as float16 - the values are float16-exact -, keys) and the fp64
results (Q_t [2,L,H,W], pred [2,H,W], conf [H,W]) at t = 10.  tests/test_cpu_ir_label.py reproduces the file.

    python tools/gen_ir_label_golden.py [--out tests/golden/ir_label.npz]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ir_label_ref as IR  # noqa: E402

MAX_BYTES = 1 << 20                                            # the project's limit for a committed file


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "ir_label.npz"))
    args = ap.parse_args(argv)
    out = {}
    for name in IR.CASES:
        img, cams, keys, trunc = IR.case(name)
        assert np.array_equal(cams.astype(np.float16).astype(np.float32), cams)
        r = IR.ir_label(img, cams, keys, trunc=trunc)
        gap = IR.top2_gap(r["q"])
        changed = float((r["pred"] != r["labs"]).mean())
        print(f"{name}: conf values {np.unique(r['conf']).tolist()}  min top-2 gap {gap.min():.3e}  labels changed {changed:.3f}")
        if name.startswith("b_"):                              # the cut-window case exercises every branch of the combination
            vals = set(np.unique(r["conf"]).tolist())
            assert 0 in vals and 255 in vals and len(vals - {0, 255}) >= 2, vals
        out[name + "/img"], out[name + "/cams"], out[name + "/keys"] = img, cams.astype(np.float16), keys.astype(np.int32)
        out[name + "/q"], out[name + "/pred"], out[name + "/conf"] = r["q"], r["pred"].astype(np.uint8), r["conf"]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    np.savez_compressed(args.out, **out)
    size = os.path.getsize(args.out)
    print(f"{args.out}: {size} bytes")
    assert size <= MAX_BYTES, size
    return 0


if __name__ == "__main__":
    sys.exit(main())
