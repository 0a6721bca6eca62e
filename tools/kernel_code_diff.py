#!/usr/bin/env python3
"""Compare the compiled device code of every kernel between two checkouts of muscle_amd/csrc.  CPU only.

    python tools/kernel_code_diff.py PARENT_DIR BRANCH_DIR [--keep OUT_DIR]

Each DIR is a csrc directory (every *.hip in it is compiled here as an unbundled gfx950 device object with the library's own
flags, muscle_amd/_build.py FLAGS plus -DMX_ABI_HASH=0) or a directory of such objects already built (NAME.hip.co).
For every kernel of every file the tool compares
  * the bytes of the kernel symbol's code range, and
  * the kernel's entry in the AMDGPU metadata note (VGPR / SGPR / AGPR counts, LDS, scratch, kernarg size, argument layout),
and prints one line per kernel: file, kernel name, code bytes on both sides, `same` or `differs` (with what differs).
It reads bytes and numbers only: no instruction text is produced or looked at.  Exit status 1 if any kernel differs.

A source-only refactor of a kernel is proven by `same` here; a change that is meant to move code shows exactly which
instantiations moved (profiles/knobs_folded_code_diff.txt is the record of the first use).
"""
from __future__ import annotations

import argparse
import os
import struct
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from muscle_amd._build import FLAGS  # noqa: E402

META_KEYS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
             ".kernarg_segment_size", ".max_flat_workgroup_size", ".wavefront_size", ".uses_dynamic_stack", ".args")


def unpack_msgpack(b: bytes, i: int = 0):
    """Decode one MessagePack value (the subset the metadata note uses) -> (value, next offset)."""
    t = b[i]
    if t <= 0x7F:
        return t, i + 1
    if t >= 0xE0:
        return t - 256, i + 1
    if 0xA0 <= t <= 0xBF:
        n = t & 31
        return b[i + 1:i + 1 + n].decode(), i + 1 + n
    if 0x80 <= t <= 0x8F or t in (0xDE, 0xDF):
        n, i = (t & 15, i + 1) if t <= 0x8F else (int.from_bytes(b[i + 1:i + 1 + (2 if t == 0xDE else 4)], "big"), i + 1 + (2 if t == 0xDE else 4))
        d = {}
        for _ in range(n):
            k, i = unpack_msgpack(b, i)
            d[k], i = unpack_msgpack(b, i)
        return d, i
    if 0x90 <= t <= 0x9F or t in (0xDC, 0xDD):
        n, i = (t & 15, i + 1) if t <= 0x9F else (int.from_bytes(b[i + 1:i + 1 + (2 if t == 0xDC else 4)], "big"), i + 1 + (2 if t == 0xDC else 4))
        a = []
        for _ in range(n):
            v, i = unpack_msgpack(b, i)
            a.append(v)
        return a, i
    if t in (0xC0, 0xC2, 0xC3):
        return {0xC0: None, 0xC2: False, 0xC3: True}[t], i + 1
    if t in (0xCC, 0xCD, 0xCE, 0xCF, 0xD0, 0xD1, 0xD2, 0xD3):
        w = 1 << ((t - 0xCC) & 3)
        return int.from_bytes(b[i + 1:i + 1 + w], "big", signed=t >= 0xD0), i + 1 + w
    if t in (0xD9, 0xDA, 0xDB, 0xC4, 0xC5, 0xC6):
        w = 1 << ((t - 0xD9) if t >= 0xD9 else (t - 0xC4))
        n = int.from_bytes(b[i + 1:i + 1 + w], "big")
        s = b[i + 1 + w:i + 1 + w + n]
        return (s.decode() if t >= 0xD9 else s), i + 1 + w + n
    if t in (0xCA, 0xCB):
        w = 4 if t == 0xCA else 8
        return struct.unpack(">f" if w == 4 else ">d", b[i + 1:i + 1 + w])[0], i + 1 + w
    raise ValueError(f"msgpack type 0x{t:02x} not handled")


def read_kernels(path: str) -> dict:
    """{kernel name: (code bytes, {metadata key: value})} of one ELF64 little-endian AMDGPU code object."""
    with open(path, "rb") as f:
        e = f.read()
    assert e[:6] == b"\x7fELF\x02\x01", f"{path}: not a 64-bit little-endian ELF"
    shoff, = struct.unpack_from("<Q", e, 0x28)
    shentsize, shnum, _ = struct.unpack_from("<HHH", e, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", e, shoff + k * shentsize) for k in range(shnum)]   # name type flags addr off size link info align entsize
    meta, funcs = None, {}
    for (_, typ, _, _, off, size, link, _, _, entsize) in secs:
        if typ == 7:                                   # SHT_NOTE
            p = off
            while p < off + size:
                namesz, descsz, ntype = struct.unpack_from("<III", e, p)
                name = e[p + 12:p + 12 + namesz]
                d0 = p + 12 + ((namesz + 3) & ~3)
                if ntype == 32 and name.startswith(b"AMDGPU"):                                   # NT_AMDGPU_METADATA
                    meta, _ = unpack_msgpack(e[d0:d0 + descsz])
                p = d0 + ((descsz + 3) & ~3)
        elif typ == 2:                                 # SHT_SYMTAB
            stroff = secs[link][4]
            for q in range(off, off + size, entsize):
                st_name, st_info, _, st_shndx, st_value, st_size = struct.unpack_from("<IBBHQQ", e, q)
                if (st_info & 15) == 2 and 0 < st_shndx < shnum:                                  # STT_FUNC
                    nm = e[stroff + st_name:e.index(b"\0", stroff + st_name)].decode()
                    sec = secs[st_shndx]
                    start = sec[4] + st_value - sec[3]
                    funcs[nm] = e[start:start + st_size]
    out = {}
    for k in (meta or {}).get("amdhsa.kernels", []):
        out[k[".name"]] = (funcs[k[".name"]], {key: k.get(key) for key in META_KEYS})
    return out


def compile_dir(src: str, out: str) -> None:
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    files = sorted(f for f in os.listdir(src) if f.endswith(".hip"))

    def cc(f):
        cmd = [hipcc, *FLAGS, "-DMX_ABI_HASH=0", "--cuda-device-only", "--no-gpu-bundle-output", "-x", "hip", "-c",
               os.path.join(src, f), "-o", os.path.join(out, f + ".co")]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed for {f}:\n{r.stderr}")

    with ThreadPoolExecutor(max_workers=4) as ex:
        list(ex.map(cc, files))


def objects(d: str, keep: str | None, tag: str) -> str:
    if any(f.endswith(".co") for f in os.listdir(d)):
        return d
    out = os.path.join(keep, tag) if keep else tempfile.mkdtemp(prefix=f"kcd_{tag}_")
    os.makedirs(out, exist_ok=True)
    compile_dir(d, out)
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("parent")
    ap.add_argument("branch")
    ap.add_argument("--keep", help="directory that keeps the compiled objects (parent/, branch/) instead of a temporary one")
    a = ap.parse_args()
    po, bo = objects(a.parent, a.keep, "parent"), objects(a.branch, a.keep, "branch")
    files = sorted(set(os.listdir(po)) | set(os.listdir(bo)))
    n_same = n_diff = 0
    for f in (f for f in files if f.endswith(".co")):
        pk = read_kernels(os.path.join(po, f)) if os.path.exists(os.path.join(po, f)) else {}
        bk = read_kernels(os.path.join(bo, f)) if os.path.exists(os.path.join(bo, f)) else {}
        for name in sorted(set(pk) | set(bk)):
            if name not in pk or name not in bk:
                verdict, sizes = ("differs: only in " + ("branch" if name in bk else "parent")), (len(pk.get(name, (b"",))[0]), len(bk.get(name, (b"",))[0]))
            else:
                (pc, pm), (bc, bm) = pk[name], bk[name]
                sizes = (len(pc), len(bc))
                what = []
                if pc != bc:
                    if len(pc) == len(bc):
                        words = sum(pc[i:i + 4] != bc[i:i + 4] for i in range(0, len(pc), 4))
                        what.append(f"code ({words} of {len(pc) // 4} words)")
                    else:
                        what.append("code")
                what += [f"{key[1:]} {pm[key]} -> {bm[key]}" for key in META_KEYS if pm[key] != bm[key] and key != ".args"]
                if pm[".args"] != bm[".args"]:
                    what.append(f"args {len(pm['.args'] or [])} -> {len(bm['.args'] or [])}")
                verdict = "differs: " + ", ".join(what) if what else "same"
            n_same += verdict == "same"
            n_diff += verdict != "same"
            print(f"{f[:-3]:<16} {sizes[0]:>7} {sizes[1]:>7}  {verdict:<8}  {name}")
    print(f"# {n_same} kernels same, {n_diff} differ")
    return 1 if n_diff else 0


if __name__ == "__main__":
    sys.exit(main())
