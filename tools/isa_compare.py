#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds symbol by symbol (no GPU needed).

    tools/isa_compare.py --old OLD.co ... --new NEW.co ... [--lib-old A.so --lib-new B.so]

Each .co is one source compiled with the Makefile's flags plus
`--offload-device-only --no-gpu-bundle-output -c`. For every kernel of the old objects the same
symbol must exist in exactly one new object with identical metadata (VGPRs, SGPRs, scratch, LDS,
kernarg bytes) and identical disassembly; no kernel may be new. Code addresses are dropped from the
comparison (kernels move), and the 32-bit literals of an `s_getpc_b64` / `s_add_u32` /
`s_addc_u32` address computation are masked: they are the pc-relative distance to a unit's own
zero line, which depends on where the kernel sits in its object. Prints one line per kernel and the
two symbol lists; exit status 1 on any difference."""
import argparse
import re
import subprocess
import sys

LLVM = "/opt/rocm/llvm/bin/"


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def metadata(co):
    """symbol -> (vgpr, agpr, sgpr, scratch, lds, kernarg) from the code object's notes."""
    out = {}
    # one "  - .key: value" block per kernel, its scalar keys at four spaces of indentation
    for block in re.split(r"^  - (?=\.)", run(LLVM + "llvm-readelf", "--notes", co), flags=re.M)[1:]:
        cur = dict(re.findall(r"^(?:    )?\.(\w+):\s*(\S+)\s*$", block, flags=re.M))
        if "name" in cur and "kernarg_segment_size" in cur:
            out[cur["name"]] = tuple(int(cur.get(f, 0)) for f in (
                "vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size",
                "group_segment_fixed_size", "kernarg_segment_size"))
    return out


INSN = re.compile(r"^\s+(\S.*?)\s*//\s*[0-9A-Fa-f]+:\s*((?:[0-9A-Fa-f]{8}\s*)+)")


def kernels(co):
    """symbol -> list of (text, encoding words) per instruction."""
    out, cur = {}, None
    for line in run(LLVM + "llvm-objdump", "-d", co).splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        m = INSN.match(line)
        if m and cur is not None:
            text = re.sub(r"<[^>]*>", "", m.group(1)).strip()
            cur.append((text, m.group(2).split()))
    return out


def normalise(insns):
    """Mask the literal of pc-relative address arithmetic; returns (lines, masked count)."""
    res, masked, pcregs = [], 0, set()
    for text, words in insns:
        op = text.split()[0]
        if op == "s_getpc_b64":
            m = re.search(r"s\[(\d+):(\d+)\]", text)
            pcregs.update((f"s{m.group(1)}", f"s{m.group(2)}"))
        elif op in ("s_add_u32", "s_addc_u32") and len(words) == 2:
            dst, src = [t.strip(",") for t in text.split()[1:3]]
            if dst == src and dst in pcregs:
                pcregs.discard(dst)
                text = re.sub(r"0x[0-9a-fA-F]+|\b\d+$", "LIT", text)
                words = [words[0], "LIT"]
                masked += 1
        if op in ("s_branch",) or op.startswith("s_cbranch"):
            text = op   # the target is in the encoding as a relative offset
        res.append(text + " ; " + " ".join(words))
    return res, masked


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", nargs="+", required=True)
    ap.add_argument("--new", nargs="+", required=True)
    ap.add_argument("--lib-old")
    ap.add_argument("--lib-new")
    args = ap.parse_args()
    old_k, old_m, new_k, new_m, where = {}, {}, {}, {}, {}
    bad = 0
    for co in args.old:
        old_m.update(metadata(co))
        old_k.update({k: v for k, v in kernels(co).items()})
    for co in args.new:
        md = metadata(co)
        for name, ins in kernels(co).items():
            if name in md:
                if name in where:
                    print(f"DUPLICATE {name} in {where[name]} and {co}")
                    bad += 1
                where[name] = co.split("/")[-1]
                new_k[name] = ins
        new_m.update(md)
    print("# symbol  unit  vgpr agpr sgpr scratch lds kernarg  code_bytes  masked_literals  verdict")
    for name in sorted(old_m):
        if name not in new_m:
            print(f"{name} MISSING")
            bad += 1
            continue
        a, na = normalise(old_k[name])
        b, nb = normalise(new_k[name])
        nbytes = 4 * sum(len(w) for _, w in old_k[name])
        same = old_m[name] == new_m[name] and a == b
        bad += not same
        detail = ""
        if not same:
            diff = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            detail = f" meta {old_m[name]} vs {new_m[name]}, first difference at instruction {diff}"
        print(name, where[name], *old_m[name], nbytes, na, "same" if same else "DIFFERENT" + detail)
    extra = sorted(set(new_m) - set(old_m))
    for name in extra:
        print(f"{name} NEW (absent from the old objects)")
    bad += len(extra)
    print(f"# kernels: old {len(old_m)}, new {len(new_m)}, differing or missing {bad}")
    if args.lib_old and args.lib_new:
        syms = [sorted(l.split()[-1] for l in run("nm", "-D", "--defined-only", lib).splitlines()
                       if "iclr17_" in l) for lib in (args.lib_old, args.lib_new)]
        print(f"# exported iclr17_ symbols: old {len(syms[0])}, new {len(syms[1])}, "
              f"{'identical' if syms[0] == syms[1] else 'DIFFERENT'}")
        bad += syms[0] != syms[1]
        print("# old:", " ".join(syms[0]))
        print("# new:", " ".join(syms[1]))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
