#!/usr/bin/env python3
"""Compare the gfx950 listings of the sampled and render kernels of two builds, kernel by kernel: were the lens-family
kernels of a parent (rt_dof_kernel, rt_soft_kernel, rt_motion_kernel, one listing each per depth) compiled to the same
code as the instances of rt_lens_kernel (rt_lens_k<kind>_b<B>.s)?

  python tools/isa_compare.py PARENT_DIR BRANCH_DIR > profiles/lens/isa_compare.md

Each directory holds rt_render_b<B>.s, rt_adaptive_b<B>.s and the lens family's listings for B = 0..7, made with the
Makefile's flags and --cuda-device-only -S (the `isa` target's command, for every depth).  A kernel's instruction
stream is its lines from its label to the section of its descriptor, comments and blank lines dropped, after three
normalisations:
the kernel's own symbol, the function number in .LBB<n>_<m> labels, and the immediate offset of scalar loads from the
kernarg pointer s[0:1] (the lens kernel has one parameter list for all kinds, so the offsets move).  The resource
figures are the kernel descriptor's.  Exit status 1 if any kernel differs."""
import os
import re
import sys

FIGURES = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "private_segment_fixed_size", "group_segment_fixed_size")
KINDS = {"dof": (0, 0), "soft": (1, 0), "motion": (1, 1)}


def kernels(path):
    """-> {symbol: (stream, figures)} of the kernels in the listing `path`."""
    lines = open(path).read().split("\n")
    out = {}
    for k, ln in enumerate(lines):
        m = re.match(r"\t\.amdhsa_kernel (\S+)", ln)
        if not m:
            continue
        sym = m.group(1)
        fig = {}
        for d in lines[k:]:
            if d.startswith("\t.end_amdhsa_kernel"):
                break
            f = re.match(r"\s+\.amdhsa_(\w+) (\S+)", d)
            if f and f.group(1) in FIGURES:
                fig[f.group(1)] = f.group(2)
        start = next(n for n, s in enumerate(lines) if s.startswith(sym + ":"))
        stream = []
        for ln2 in lines[start + 1:]:
            if ln2.startswith("\t.section"):                # the kernel descriptor follows the code
                break
            code = ln2.split(";")[0].rstrip()
            if not code.strip():
                continue
            code = code.replace(sym, "KERNEL")
            code = re.sub(r"\.LBB\d+_", ".LBB_", code)
            code = re.sub(r"(s_load_dword\w*\s+\S+ s\[0:1\], )\S+", r"\1KERNARG", code)
            stream.append(code)
        out[sym] = (stream, fig)
    return out


def lens_key(sym):
    """(B, TRANSP, TREE, AREA, MOTION) of a lens-family kernel symbol of either build, or None."""
    m = re.search(r"rt_(dof|soft|motion)_kernelILi(\d)ELb(\d)ELb(\d)EE", sym)
    if m:
        return (int(m.group(2)), int(m.group(3)), int(m.group(4))) + KINDS[m.group(1)]
    m = re.search(r"rt_lens_kernelILi(\d)ELb(\d)ELb(\d)ELb(\d)ELb(\d)EE", sym)
    return tuple(int(g) for g in m.groups()) if m else None


def load(d, prefix):
    out = {}
    for f in sorted(os.listdir(d)):
        if f.startswith(prefix) and f.endswith(".s"):
            out.update(kernels(os.path.join(d, f)))
    return out


def verdict(a, b):
    """"equal", or what differs between two (stream, figures)."""
    diffs = [f"{f} {a[1].get(f)} -> {b[1].get(f)}" for f in FIGURES if a[1].get(f) != b[1].get(f)]
    if len(a[0]) != len(b[0]):
        diffs.append(f"{len(a[0])} -> {len(b[0])} lines")
    else:
        bad = [k for k in range(len(a[0])) if a[0][k] != b[0][k]]
        if bad:
            diffs.append(f"{len(bad)} lines differ, first `{a[0][bad[0]].strip()}` -> `{b[0][bad[0]].strip()}`")
    return "; ".join(diffs) or "equal"


def main():
    parent, branch = sys.argv[1:3]
    kind_name = {v: k for k, v in KINDS.items()}
    inst = {(0, 0): "opaque", (1, 0): "FULL", (1, 1): "tree"}
    differ = 0
    print("# The lens-family kernels before and after the fold into rt_lens_kernel\n")
    print("Made by `tools/isa_compare.py` (its docstring says what is compared and what is normalised).  Lines counts the")
    print("lines of the instruction stream, labels included; VGPRs is `.amdhsa_next_free_vgpr`.  \"equal\": the streams are")
    print("equal line by line and the five resource figures are equal.\n")
    print("| kind | depth | instance | lines | VGPRs | SGPRs | accum_offset | scratch | LDS | parent vs. rt_lens_kernel |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    P = {lens_key(s): v for s, v in load(parent, "rt_").items() if lens_key(s)}
    B = {lens_key(s): v for s, v in load(branch, "rt_lens_").items() if lens_key(s)}
    assert len(P) == 72 and sorted(P) == sorted(B), (len(P), len(B))
    for key in sorted(P, key=lambda k: (k[3] + k[4], k[0], k[1] + k[2])):
        v = verdict(P[key], B[key])
        differ += v != "equal"
        f = B[key][1]
        print(f"| {kind_name[key[3:]]} | {key[0]} | {inst[key[1:3]]} | {len(B[key][0])} | " +
              " | ".join(f[x] for x in FIGURES) + f" | {v} |")
    print("\n## The kernels the fold does not touch\n")
    print("| listings | kernels | differing |")
    print("|---|---|---|")
    for prefix in ("rt_adaptive_", "rt_render_"):
        p, b = load(parent, prefix), load(branch, prefix)
        assert sorted(p) == sorted(b) and p
        bad = [s for s in p if verdict(p[s], b[s]) != "equal"]
        differ += len(bad)
        print(f"| `{prefix}b<0..7>.s` | {len(p)} | {len(bad)}" + "".join(f" `{s}`" for s in bad) + " |")
    print(f"\n{differ} kernels differ.")
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
