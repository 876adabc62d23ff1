#!/usr/bin/env python3
"""Compare the gfx950 listings of two builds, kernel by kernel.

  python tools/isa_compare.py --by-symbol PARENT_DIR BRANCH_DIR > profiles/split/isa_compare.md

Directory against directory, keyed by symbol: every kernel of every listing of PARENT_DIR against the kernel of the
same symbol wherever it lies among the listings of BRANCH_DIR (a change that moves kernels between translation units
and should change none); a kernel missing from the branch, or found in more than one of its listings, is a difference.

  python tools/isa_compare.py PARENT_DIR BRANCH_DIR > profiles/lens/isa_compare.md

The record of the lens fold (reproducible from the trees of that change only, whose parent still had the three kernels):
were the lens-family kernels of a parent (rt_dof_kernel, rt_soft_kernel, rt_motion_kernel, one listing each per depth)
compiled to the same code as the instances of rt_lens_kernel (rt_lens_k<kind>_b<B>.s)?

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


def listing_group(f):
    """rt_render_b3.s -> rt_render_b<B>.s: the per-depth listings of one source are one row of the table."""
    return re.sub(r"_k\d_b\d\.s$", "_k<K>_b<B>.s", re.sub(r"(?<!_k\d)_b\d\.s$", "_b<B>.s", f))


def main_by_symbol(parent, branch):
    files = lambda d: sorted(f for f in os.listdir(d) if f.endswith(".s"))
    where = {}                                              # symbol -> [(branch listing, kernel)]
    for f in files(branch):
        for sym, v in kernels(os.path.join(branch, f)).items():
            where.setdefault(sym, []).append((f, v))
    rows, detail, differ, seen = {}, [], 0, set()
    for f in files(parent):
        for sym, v in sorted(kernels(os.path.join(parent, f)).items()):
            seen.add(sym)
            hits = where.get(sym, [])
            verd = verdict(v, hits[0][1]) if len(hits) == 1 else f"in {len(hits)} listings of the branch"
            differ += verd != "equal"
            r = rows.setdefault(listing_group(f), {"n": 0, "bad": [], "to": set()})
            r["n"] += 1
            r["to"].update(listing_group(h[0]) for h in hits)
            if verd != "equal":
                r["bad"].append(sym)
            if listing_group(f) == f:                       # a listing that is not one of a per-depth family: by kernel
                if re.search(r"\d+rt_\w+_kernel", sym):
                    detail.append((f, sym, v, hits[0][0] if hits else "-", verd))
                else:                                       # the sort's and the scan's (rocprim, through hipcub)
                    lib = rows.setdefault(f"`{f}`: library kernels", {"n": 0, "bad": [], "to": set()})
                    lib["n"] += 1
                    lib["to"].update(h[0] for h in hits)
                    if verd != "equal":
                        lib["bad"].append(sym)
    new = sorted(s for s in where if s not in seen)
    print("# Parent against branch, kernel by kernel\n")
    print("Made by `tools/isa_compare.py --by-symbol` (its docstring says what is compared and what is normalised).  \"equal\":")
    print("the kernel of that symbol is in exactly one listing of the branch, the instruction streams are equal line by line")
    print("and the five resource figures are equal.\n")
    print("| parent listings | kernels | found in the branch's | differing |")
    print("|---|---|---|---|")
    for g, r in rows.items():
        print(f"| {g if '`' in g else '`' + g + '`'} | {r['n']} | " + ", ".join(f"`{t}`" for t in sorted(r["to"])) + f" | {len(r['bad'])}" +
              "".join(f" `{s}`" for s in r["bad"]) + " |")
    print("\n(The library kernels are also counted in their listing's row.)")
    print("\n## The project's kernels of the listings that are not per depth\n")
    print("| parent listing | kernel | lines | VGPRs | SGPRs | accum_offset | scratch | LDS | branch listing | verdict |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for f, sym, v, to, verd in detail:
        name = sym if len(sym) <= 72 else sym[:69] + "..."
        print(f"| `{f}` | `{name}` | {len(v[0])} | " + " | ".join(v[1].get(x, "-") for x in FIGURES) + f" | `{to}` | {verd} |")
    print(f"\nKernels of the branch with no counterpart in the parent: {len(new)}" + "".join(f" `{s}`" for s in new) + ".")
    print(f"\n{differ} kernels differ.")
    sys.exit(1 if differ or new else 0)


def main():
    if sys.argv[1] == "--by-symbol":
        return main_by_symbol(*sys.argv[2:4])
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
