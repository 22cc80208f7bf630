#!/usr/bin/env python3
"""Register budget of every kernel of one build against another's, from hipcc -S dumps (as tools/isa_regs.py).

    for f in rn_conv rn_conv_wide ...; do hipcc -O3 -std=c++17 --offload-arch=gfx950 -Iinclude -Iresnet.c_amd/csrc \\
        -S --cuda-device-only -o DIR/$f.s resnet.c_amd/csrc/$f.hip; done        (in both trees)
    python tools/isa_regs_compare.py PARENT_DIR THIS_DIR rn_conv rn_conv_wide ...

Per kernel of the parent: VGPRs, AGPRs, scratch bytes and occupancy, "same" or "DIFF" against this tree's kernel of
that name.  An instantiation that gained the trailing DIL = false template flag (conv_gemm_kernel,
conv_group_kernel) is compared with the parent's kernel without the flag where the parent has no kernel of its
own name; kernels only this tree has are "new"."""
import re
import sys
def parse(path):
    out, name = {}, None
    txt = open(path).read()
    # per kernel: .amdhsa_kernel NAME ... next_free_vgpr, accum_offset ; then "; ScratchSize", "; Occupancy" in the comment block
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", txt, re.S):
        k, body = m.group(1), m.group(2)
        nv = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1))
        acc = re.search(r"\.amdhsa_accum_offset (\d+)", body)
        out[k] = {"total_vgpr": nv, "accum_offset": int(acc.group(1)) if acc else None}
    # the symbol's body ends with "; -- End function" followed by the "; Kernel info:" comment block
    for m in re.finditer(r"^(\S+):\s*; @\1\n(.*?); -- End function\n(.*?); Occupancy: (\d+)", txt, re.S | re.M):
        k, info = m.group(1), m.group(3)
        if k in out:
            g = lambda key: int(re.search(key + r": (\d+)", info).group(1))
            out[k].update(vgpr=g("NumVgprs"), agpr=g("NumAgprs"), scratch=g("ScratchSize"), occupancy=int(m.group(4)))
    return out
def norm(k):
    k = re.sub(r"_ZN\d+_GLOBAL__N_\d+", "", k)
    return k
def strip_dil(k):
    # this tree's undilated instantiation of a kernel that gained the DIL flag -> the parent's name
    k2 = re.sub(r"(conv_gemm_kernelI.*?Lb[01]ELb[01]ELb[01]E)Lb0E(EEvN7rn_gemm)", r"\1\2", k)
    k2 = k2.replace("conv_group_kernelILb0EEEvNS_11GroupParamsE", "conv_group_kernelENS_11GroupParamsE")
    # ... or the trailing PM = false flag (the parent then has four flags)
    if k2 == k:
        k2 = re.sub(r"(conv_gemm_kernelI.*?(?:Lb[01]E){4})Lb0E(EEvN7rn_gemm)", r"\1\2", k)
    return k2
parent_dir, this_dir, files = sys.argv[1], sys.argv[2], sys.argv[3:]
bad = 0
for f in files:
    p, t = parse(f"{parent_dir}/{f}.s"), parse(f"{this_dir}/{f}.s")
    tmap = {strip_dil(k): v for k, v in t.items()}
    tmap.update(t)      # a parent that has the flag too: name against name
    print(f"== {f}.hip: {len(p)} kernels at the parent, {len(t)} in this tree")
    for k, v in p.items():
        w = tmap.get(k)
        same = w is not None and all(v.get(x) == w.get(x) for x in ("vgpr", "agpr", "scratch", "occupancy"))
        bad += not same
        print(f"{'same ' if same else 'DIFF '} {norm(k)[:78]:78s} vgpr {v.get('vgpr')} agpr {v.get('agpr')} scratch {v.get('scratch')} occupancy {v.get('occupancy')}" + ("" if same else f"  -> {w}"))
    new = [k for k in t if k not in p and strip_dil(k) not in p]
    for k in new:
        v = t[k]
        print(f"new   {norm(k)[:78]:78s} vgpr {v.get('vgpr')} agpr {v.get('agpr')} scratch {v.get('scratch')} occupancy {v.get('occupancy')}")
print(f"kernels of the parent whose figures differ: {bad}")
