#!/usr/bin/env python3
"""Device code of one build against another's, as text, from hipcc -S dumps (made as for tools/isa_regs_compare.py).

    python tools/isa_text_compare.py [--mnemonics] PARENT_DIR THIS_DIR rn_conv ...

The compiler's per-build hash (__hip_cuid_*) and the function number in local labels (.LBB<n>_3) are replaced
and .file / .ident / .loc lines are dropped.  Then each dump is
cut into one piece per kernel (code, kernel descriptor, register comment block) and the entries of its
metadata list, and the two builds must hold the same pieces: every instruction, every kernel-argument offset and
every register count of every kernel; the pixel-major instantiations of conv_gemm_kernel (a fifth template
flag, true) exist in this tree only and are counted apart, and an instantiation whose fifth flag is false is compared
under its four-flag name.  roi_align_kernel's store-layout flag (a third template argument) is treated the same way
against a parent that has none: the NHWC instantiations are counted apart, the others go by the parent's names.  The order the compiler emitted the kernels in is reported separately: it
follows the order the host code first names the instantiations in and is no property of any kernel.

--mnemonics: the same cut into kernels, but of a kernel's code only the first token of every instruction line --
the opcode without its operands -- is compared, in order: the two builds must hold the same kernels and every
kernel the same sequence of mnemonics (same length, same order).  What the full text holds against a build and this
mode does not: which register the allocator picked, an immediate, a label's number."""
import re
import sys


FIVE_FLAGS = r"conv_gemm_kernelI\w+?Li\d+ELi\d+E(?:Lb[01]E){5}EEvN7rn_gemm"
ROI_FLAG = r"roi_align_kernelI\w+?Li\d+ELb[01]EEEvNS_8roi_args"


def pieces(path, parent_names=False, roi_parent_names=False):
    txt = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", open(path).read())
    if parent_names:
        # an instantiation of conv_gemm_kernel that gained the trailing PM = false template flag goes by the name
        # the parent gave it (four flags); the parent's own dump has no name this matches
        txt = re.sub(r"(conv_gemm_kernelI\w+?Li\d+ELi\d+E(?:Lb[01]E){4})Lb0E(EEvN7rn_gemm)", r"\1\2", txt)
    if roi_parent_names:
        txt = re.sub(r"(roi_align_kernelI\w+?Li\d+E)Lb0E(EEvNS_8roi_args)", r"\1\2", txt)
    # local labels carry the number of their function in emission order: .LBB12_3, .Lfunc_end12, .Ltmp7
    txt = re.sub(r"\.L(BB|func_begin|func_end|tmp|JTI)\d+", r".L\1N", txt)
    txt = re.sub(r"\bBB\d+_(\d+)", r"BBN_\1", txt)  # (the same labels in loop comments)
    txt = re.sub(r"[ \t]+;", " ;", txt)  # (the comment column behind a label moves with the label's length)
    lines = [l for l in txt.splitlines() if not re.match(r"\s*\.(ident|file|loc)\b", l)]
    out, cur, meta = [], [], False
    for l in lines:
        if l.startswith("\t.section\t.AMDGPU.gpr_maximums"):  # the module's trailer, the metadata list behind it
            meta = True
            out.append("\n".join(cur))
            cur = []
        elif meta and re.match(r"  - \.|amdhsa\.target", l):
            out.append("\n".join(cur))
            cur = []
        elif not meta and "; -- Begin function" in l:
            # a kernel's piece starts at the section line in front of its .globl line
            at = max((i for i, c in enumerate(cur) if re.match(r"\t\.(section|text)\b", c)), default=len(cur))
            out.append("\n".join(cur[:at]))
            cur = cur[at:]
        cur.append(l)
    out.append("\n".join(cur))
    return out


def has_five_flags(path):
    return re.search(FIVE_FLAGS, open(path).read()) is not None


def has_roi_flag(path):
    return re.search(ROI_FLAG, open(path).read()) is not None


def mnemonics(path, parent_names=False, roi_parent_names=False):
    """kernel name -> the mnemonics of its code, from the symbol's label to its s_endpgm / .Lfunc_end"""
    out = {}
    for p in pieces(path, parent_names, roi_parent_names):
        m = re.search(r"^(\S+):\s*; @\1\n(.*?)^\.Lfunc_endN:", p, re.S | re.M)
        if not m or ".amdhsa_kernel " + m.group(1) not in p:
            continue
        seq = []
        for l in m.group(2).splitlines():
            l = l.split(";")[0].strip()
            if l and not l.startswith(".") and not l.endswith(":"):  # no directive, no label
                seq.append(l.split()[0])
        out[m.group(1)] = seq
    return out


def main_mnemonics(a_dir, b_dir, names):
    bad = 0
    for n in names:
        a, b = mnemonics(f"{a_dir}/{n}.s"), mnemonics(f"{b_dir}/{n}.s", parent_names=not has_five_flags(f"{a_dir}/{n}.s"),
                                                      roi_parent_names=not has_roi_flag(f"{a_dir}/{n}.s"))
        nhwc = sorted(k for k in set(b) - set(a) if re.search(r"roi_align_kernelI\w+?Li\d+ELb1EEEvNS_8roi_args", k))
        if nhwc:
            print(f"{n}.s: {len(nhwc)} NHWC instantiations of roi_align_kernel only this tree has")
            b = {k: v for k, v in b.items() if k not in nhwc}
        missing, new = sorted(set(a) - set(b)), sorted(set(b) - set(a))
        differ = [k for k in a if k in b and a[k] != b[k]]
        same = not missing and not new and not differ
        bad += not same
        print(f"{n}.s: kernels {len(a)} / {len(b)}, missing {len(missing)}, new {len(new)}, mnemonics "
              f"{sum(map(len, a.values()))} / {sum(map(len, b.values()))}, kernels whose sequence differs {len(differ)}: "
              f"{'same mnemonics' if same else 'DIFFERENT'}")
        for k in missing:
            print("   missing:", k[:150])
        for k in new:
            print("   new:", k[:150])
        for k in differ:
            at = next((i for i, (x, y) in enumerate(zip(a[k], b[k])) if x != y), min(len(a[k]), len(b[k])))
            print(f"   differs: {k[:120]}: {len(a[k])} / {len(b[k])} instructions, first difference at {at}: "
                  f"{' '.join(a[k][at:at + 3])} / {' '.join(b[k][at:at + 3])}")
    return 1 if bad else 0


def main():
    if sys.argv[1] == "--mnemonics":
        return main_mnemonics(sys.argv[2], sys.argv[3], sys.argv[4:])
    a_dir, b_dir, names = sys.argv[1], sys.argv[2], sys.argv[3:]
    bad = 0
    for n in names:
        # (a parent that has the fifth flag itself is compared name against name)
        a, b = pieces(f"{a_dir}/{n}.s"), pieces(f"{b_dir}/{n}.s", parent_names=not has_five_flags(f"{a_dir}/{n}.s"),
                                                roi_parent_names=not has_roi_flag(f"{a_dir}/{n}.s"))
        kernels = sum(p.count(".amdhsa_kernel ") for p in a), sum(p.count(".amdhsa_kernel ") for p in b)
        only_a, only_b = set(a) - set(b), set(b) - set(a)
        # kernels only this tree has (the pixel-major instantiations) are reported, not held against it
        new = {p for p in only_b if "conv_gemm_kernelI" in p and re.search(r"(?:Lb[01]E){4}Lb1EEEvN7rn_gemm", p)}
        only_b -= new
        nhwc = {p for p in only_b if re.search(r"roi_align_kernelI\w+?Li\d+ELb1EEEvNS_8roi_args", p)}
        only_b -= nhwc
        same = not only_a and not only_b
        if new:
            print(f"{n}.s: {len(new)} pieces (code or metadata entry) of pixel-major instantiations only this tree has")
        if nhwc:
            print(f"{n}.s: {len(nhwc)} pieces (code or metadata entry) of NHWC instantiations of roi_align_kernel only this tree has")
        bad += not same
        print(f"{n}.s: kernels {kernels[0]} / {kernels[1]}, pieces {len(a)} / {len(b)}, "
              f"differing pieces {len(only_a)} / {len(only_b)}: {'same text' if same else 'DIFFERENT'}; "
              f"emission order {'same' if a == b else 'differs'}")
        for p in sorted(only_a | only_b)[:4]:
            print("   differs:", p.strip().splitlines()[0][:160])
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
