#!/usr/bin/env python3
"""Did a change move a kernel?  Compares two sets of device assemblies (`make -C greenlight-gym2_amd/csrc asm` writes one per
translation unit, /tmp/glgym.s, /tmp/glgym_env.s, ...; keep the parent commit's under other names) kernel by kernel: instruction streams with labels and symbol names normalised, registers,
scratch, LDS, whether any loop holds a scratch instruction, the four largest loop blocks, and -- where the streams differ -- whether the
floating-point opcode histogram did.
A side is one .s file or several joined by commas: a kernel is found whichever translation unit holds it, so a kernel that
only moved between files compares as itself.  The default filter shows the kernels that inline gl_envlayer.hpp; "." shows all.
    python tools/isa_compare.py parent.s[,parent2.s,...] change.s[,change2.s,...] [filter]      (profiles/tu_split.txt section 1)"""
import collections
import re
import subprocess
import sys

DEFAULT_FILTER = "step_kernel<|reset_kernel|obs_kernel"


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    res = []
    for dn in out[:len(names)]:
        dn = dn.replace("(anonymous namespace)::", "")
        dn = re.sub(r"^void ", "", dn)
        res.append(re.sub(r"\(.*$", "", dn))
    return res


def scan_body(lines):
    """Normalised instructions of one kernel, and per basic block [loop depth, instructions, packed, transcendental, holds scratch]."""
    ins, blocks, cur = [], [], None
    for line in lines:
        if re.match(r"^\.LBB\d+_\d+:", line):
            m = re.search(r"Depth=(\d+)", line)
            cur = [int(m.group(1)) if m else 0, 0, 0, 0, False]
            blocks.append(cur)
            continue
        if "Loop Header" in line or "Inner Loop" in line or "Parent Loop" in line:
            m = re.search(r"Depth=(\d+)", line)
            if cur is not None and m:
                cur[0] = int(m.group(1))
        if not line.startswith("\t") or line.strip().startswith((".", ";")):
            continue
        t = line.split(";")[0].strip()
        t = re.sub(r"\.LBB\d+_", ".LBB_", t)
        t = re.sub(r"_ZN?\S+", "SYM", t)
        ins.append(t)
        if cur is None:
            continue
        op = t.split()[0]
        cur[1] += 1
        if op.startswith("v_pk_"):
            cur[2] += 1
        if re.match(r"v_(exp|log|rcp|rsq|sqrt|sin|cos)_", op):
            cur[3] += 1
        if "scratch_" in op:
            cur[4] = True
    return ins, blocks


def kernels(paths):
    s = "\n".join(open(p).read() for p in paths.split(","))
    names = re.findall(r"^\s*\.amdhsa_kernel (\S+)", s, flags=re.M)
    out = {}
    for name, dn in zip(names, demangle(names)):
        i = s.index(".amdhsa_kernel " + name)
        desc = s[i:s.index(".end_amdhsa_kernel", i)]

        def field(k):
            return int(re.search(r"\.amdhsa_" + k + r" (\d+)", desc).group(1))

        start = re.search(r"^" + re.escape(name) + r":", s, flags=re.M).start()
        body = s[start:]
        body = body[:body.index(".Lfunc_end")]
        ins, blocks = scan_body(body.split("\n"))
        nv, acc = field("next_free_vgpr"), field("accum_offset")
        big = sorted([b for b in blocks if b[0] >= 2], key=lambda b: -b[1])[:4]
        fp = collections.Counter(t.split()[0] for t in ins if re.match(r"v_\S*f(16|32|64)", t.split()[0]))
        out[dn] = dict(mangled=name, ins=ins, vgpr=min(nv, acc), agpr=max(0, nv - acc), scratch=field("private_segment_fixed_size"),
                       lds=field("group_segment_fixed_size"), big=[(b[1], b[0], b[2], b[3]) for b in big], fp=fp,
                       loop_scratch=any(b[4] for b in blocks if b[0] >= 1))
    return out


def status(p, c):
    if p is None:
        return "new"
    if p["mangled"] != c["mangled"]:
        return "MANGLED NAME CHANGED: %s -> %s" % (p["mangled"], c["mangled"])
    if p["ins"] == c["ins"]:
        res = [k for k in ("vgpr", "agpr", "scratch", "lds") if p[k] != c[k]]
        return "= parent, instruction for instruction" + ("".join("; %s WAS %d" % (k, p[k]) for k in res))
    if p["fp"] == c["fp"]:
        hist = "unchanged"
    else:
        hist = "CHANGED %s" % ((c["fp"] - p["fp"]) + (p["fp"] - c["fp"]))
    return "DIFFERS: instr %d -> %d; fp histogram %s" % (len(p["ins"]), len(c["ins"]), hist)


def main(argv):
    parent, change = kernels(argv[1]), kernels(argv[2])
    flt = argv[3] if len(argv) > 3 else DEFAULT_FILTER
    for dn in sorted(change):
        if not re.search(flt, dn):
            continue
        c = change[dn]
        loops = "; ".join("%d (depth %d, %d pk, %d trans)" % b for b in c["big"])
        print("%-52s vgpr %3d agpr %3d scratch %4d B lds %6d B instr %6d scratch in loops %d | loop blocks: %s | %s" % (
            dn, c["vgpr"], c["agpr"], c["scratch"], c["lds"], len(c["ins"]), c["loop_scratch"], loops, status(parent.get(dn), c)))
    print("missing in change:", [d for d in parent if d not in change and re.search(flt, d)])


if __name__ == "__main__":
    main(sys.argv)
