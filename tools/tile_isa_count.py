#!/usr/bin/env python3
"""Static instruction counts of the NTT / LDE tile kernels, phase by phase, from hipcc's assembly of csrc/ntt.hip
(hipcc <the Makefile's flags for ntt.o> --cuda-device-only -S csrc/ntt.hip -o ntt.s).

A kernel is cut at its s_barrier instructions: the phases of ntt_pass_kernel<.., 8, 16> are load + tables | tile write | first
radix-16 step | second step | store; lde_mid_kernel<16, 16> has the inverse steps in front and then, per coset, scale + tile write |
two steps | store + scale update.  Vector instructions are classed by what wrote them:
  butterfly  the 4-word add / sub chains of gl_fermat.cuh (inline asm on vcc) and the constant shifts between them
             (v_perm, v_alignbit, v_ashrrev, v_lshlrev_b32_e32 inside a step)
  prod_asm   the other inline-asm instructions: the carry-out product mul_lazy_x (5 of its instructions are the compiler's and are
             counted under mad / other)
  mad        v_mad_u64_u32 the compiler wrote: 3 per product, 1 per reduction, 2 per 64-bit row address
  other      everything else: reductions' compares and selects, addressing, index arithmetic, bounds
Usage: tile_isa_count.py ntt.s [name-substring ...]      (default: the four 16-slot instances)"""
import collections
import re
import sys

DEFAULT = ("ntt_pass_kernelILb0ELb1ELi8ELi16", "ntt_pass_kernelILb1ELb0ELi8ELi16", "ntt_pass_kernelILb0ELb0ELi8ELi16", "lde_mid_kernelILi16ELi16")
SHIFTS = ("v_perm_b32", "v_alignbit_b32", "v_ashrrev_i32_e32")
CHAIN = ("v_add_co_u32", "v_addc_co_u32", "v_sub_co_u32", "v_subb_co_u32")


def kernels(path):
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is not None:
            if line.lstrip().startswith((".section", ".amdhsa_kernel")):
                cur = None
                continue
            cur.append(line.rstrip("\n"))
    return out


def phases(lines):
    ph, cur, in_asm = [], collections.Counter(), False
    for l in lines:
        t = l.strip()
        if t.startswith(";;#ASMSTART"):
            in_asm = True
            continue
        if t.startswith(";;#ASMEND"):
            in_asm = False
            continue
        t = t.split(";")[0].strip()
        if not t or t.endswith(":") or t.startswith("."):
            continue
        op = t.split()[0]
        if op == "s_barrier":
            ph.append(cur)
            cur = collections.Counter()
            continue
        if op.startswith("v_"):
            cur["valu"] += 1
            if in_asm and op in CHAIN:
                cur["butterfly"] += 1
            elif in_asm:
                cur["prod_asm"] += 1
            elif op in SHIFTS:
                cur["butterfly"] += 1
            elif op == "v_mad_u64_u32":
                cur["mad"] += 1
            else:
                cur["other"] += 1
                cur["other:" + op] += 1
        elif op.startswith(("ds_", "global_", "flat_", "buffer_")):
            cur[op] += 1
        elif op in ("s_nop", "s_waitcnt"):
            cur[op] += 1
        elif op.startswith("s_cbranch") or op == "s_branch":
            cur["branch"] += 1
        elif op.startswith("s_"):
            cur["salu"] += 1
    ph.append(cur)
    return ph


def main():
    ks = kernels(sys.argv[1])
    want = sys.argv[2:] or DEFAULT
    for sub in want:
        for name, lines in ks.items():
            if sub not in name:
                continue
            meta = {}
            for key in ("vgpr_count", "sgpr_count", "vgpr_spill_count", "private_segment_fixed_size"):
                m = re.search(r"\.name:\s+%s\n(?:.*\n){0,12}?\s+\.%s:\s+(\d+)" % (re.escape(name), key), open(sys.argv[1]).read())
                meta[key] = m.group(1) if m else "?"
            print("%s   vgpr %s sgpr %s spills %s scratch %s" % (name, meta["vgpr_count"], meta["sgpr_count"], meta["vgpr_spill_count"], meta["private_segment_fixed_size"]))
            tot = collections.Counter()
            for i, c in enumerate(phases(lines)):
                tot.update(c)
                mem = " ".join("%s=%d" % (k, v) for k, v in sorted(c.items()) if k.startswith(("ds_", "global_")))
                print("  phase %d: valu %4d = butterfly %4d + prod_asm %4d + mad %3d + other %4d | s_nop %3d waitcnt %3d salu %3d branch %3d | %s" % (
                    i, c["valu"], c["butterfly"], c["prod_asm"], c["mad"], c["other"], c["s_nop"], c["s_waitcnt"], c["salu"], c["branch"], mem))
            print("  total  : valu %4d = butterfly %4d + prod_asm %4d + mad %3d + other %4d | s_nop %3d waitcnt %3d salu %3d branch %3d" % (
                tot["valu"], tot["butterfly"], tot["prod_asm"], tot["mad"], tot["other"], tot["s_nop"], tot["s_waitcnt"], tot["salu"], tot["branch"]))
            print("  other, by opcode: " + " ".join("%s=%d" % (k[6:], v) for k, v in sorted(tot.items(), key=lambda kv: -kv[1]) if k.startswith("other:")))


if __name__ == "__main__":
    main()
