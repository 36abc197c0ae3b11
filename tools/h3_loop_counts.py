"""Static instruction counts of the h3 engine's main loops (CPU; disassembles the built library).

For every h3k_kernel instantiation: the code object's register counts (VGPRs, spills), and the
barrier-to-barrier segments of the code that hold MFMAs, grouped by their (MFMA, VALU,
v_pk_mul_f16, ds_read) counts. One main-loop step is one segment (a step opens with the counted
wait and the workgroup barrier), so the steady steps show up as the most frequent groups; the
prologue step of a chunk and the epilogue's contraction as rarer ones. VALU = vector ALU
instructions that are not MFMAs (v_* minus v_mfma*).

The narrow-activation form (csrc/engine_h3.hip, NARROW) scales the one activation fragment of a
step by 2^11 — 4 v_pk_mul_f16 — where the general form scales the weight fragments — 4 per
32-channel tile; this tool is how DESIGN §0b's counts were taken.

  python tools/h3_loop_counts.py [libiclr17.so] [name filter] [--all]

--all lists every segment group, not the eight most frequent: the GDN / IGDN epilogue's channel
contraction is four segments per body (one per γ stage: 54 MFMAs at N = 192, 24 at N = 128; the
last one runs on into the output phase), which the main loop's steps outnumber.
"""
from __future__ import annotations

import collections
import os
import re
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dma_sync_check as dsc  # noqa: E402

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"


def demangle(names):
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not filt:   # the mangled names then (the filter applies to them)
        return {n: n for n in names}
    out = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True,
                         check=True).stdout.split("\n")
    return dict(zip(names, out))


def metadata(co: bytes) -> dict:
    """kernel name → {vgpr, agpr, spill, lds} from the code object's notes."""
    with tempfile.NamedTemporaryFile(suffix=".elf") as f:
        f.write(co)
        f.flush()
        text = subprocess.run([READELF, "--notes", f.name], capture_output=True, text=True).stdout
    recs, cur = [], {}
    for ln in text.splitlines():
        m = re.match(r"\s*-?\s*\.(\w+):\s*(\S+)", ln)
        if not m:
            continue
        k, v = m.group(1), m.group(2)
        if k == "agpr_count":   # the first key of a kernel's record (the keys are sorted)
            cur = {}
            recs.append(cur)
        if k in ("vgpr_count", "agpr_count", "vgpr_spill_count", "sgpr_spill_count",
                 "group_segment_fixed_size"):
            cur[k] = int(v)
        elif k == "symbol":
            cur["symbol"] = v.removesuffix(".kd")
    return {r["symbol"]: r for r in recs if "symbol" in r}


def segments(body):
    """(mfma, valu, pk_mul, ds_read) per barrier-to-barrier segment that holds an MFMA."""
    segs, cur = [], [0, 0, 0, 0]
    for _, op, _ in body:
        if op == "s_barrier":
            if cur[0]:
                segs.append(tuple(cur))
            cur = [0, 0, 0, 0]
        elif op.startswith("v_mfma"):
            cur[0] += 1
        elif op.startswith("v_"):
            cur[1] += 1
            cur[2] += op.startswith("v_pk_mul_f16")
        elif op.startswith("ds_read"):
            cur[3] += 1
    if cur[0]:
        segs.append(tuple(cur))
    return segs


def main(argv):
    every = "--all" in argv
    argv = [a for a in argv if a != "--all"]
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = argv[1] if len(argv) > 1 else os.path.join(here, "iclr_17_compression_amd", "libiclr17.so")
    flt = argv[2] if len(argv) > 2 else "h3k_kernel"
    for co in dsc.code_objects(lib):
        ks = dsc.kernels(co)
        md = metadata(co)
        names = demangle([k for k in ks])
        for k, body in sorted(ks.items()):
            nm = names.get(k, k)
            if flt not in nm:
                continue
            m = md.get(k, {})
            scratch = sum(op.startswith("scratch_") for _, op, _ in body)
            print(f"{nm}\n  vgpr {m.get('vgpr_count')} agpr {m.get('agpr_count')} "
                  f"vgpr_spill {m.get('vgpr_spill_count')} sgpr_spill {m.get('sgpr_spill_count')} "
                  f"scratch_instructions {scratch} lds {m.get('group_segment_fixed_size')}  "
                  f"instructions {len(body)}")
            hist = collections.Counter(segments(body))
            for (mf, va, pk, ds), n in sorted(hist.items(), key=lambda kv: -kv[1])[:None if every else 8]:
                print(f"  {n:4d} segments: {mf:3d} MFMA {va:4d} VALU ({pk:3d} v_pk_mul_f16) {ds:3d} ds_read"
                      f"   VALU/MFMA {va / mf:.2f}")


if __name__ == "__main__":
    main(sys.argv)
