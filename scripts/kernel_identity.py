"""Are the kernels of two builds the same code? Compares gfx950 assembly, kernel by kernel.
usage: python scripts/kernel_identity.py <dir A of .s files> <dir B of .s files> [unit name regex]

Make the .s files with the Makefile's HIPFLAGS plus `--cuda-device-only -S`, one per csrc/*.hip.
For every kernel of A (of the units the regex selects, by file stem; default all) three things
must equal B's, wherever in B the kernel lives: the text from its label to its .Lfunc_end, its
.amdhsa_kernel block, and the resource figures of its metadata entry. Only the function index the
assembler puts into local labels (.LBB<n>_, .Lfunc_end<n>, BB<n>_ in comments) is normalised, and
the padding between such a label and its comment, which moves with the index's digit count.
Also reported: kernels of A missing from B, kernels only in B, and any kernel name that two units
of one directory define (it would be registered twice). Exit status 1 if anything differs."""
import glob
import os
import re
import subprocess
import sys

META = (".vgpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size",
        ".group_segment_fixed_size", ".kernarg_segment_size")
NORM = ((re.compile(r"\.LBB\d+_"), ".LBB_"), (re.compile(r"\.Lfunc_end\d+"), ".Lfunc_end"),
        (re.compile(r"\bBB\d+_"), "BB_"),
        # (a label's comment is padded to a column: the padding changes with the index's digits)
        (re.compile(r"^(\.LBB_\d+:) +;", re.M), r"\1 ;"))


def norm(lines):
    s = "\n".join(lines)
    for pat, rep in NORM:
        s = pat.sub(rep, s)
    return s


def parse(path):
    """kernel name -> {"text", "desc", "meta"} of one .s file"""
    lines = open(path).read().split("\n")
    desc, meta, cur = {}, {}, None
    for i, ln in enumerate(lines):
        if ln.startswith("\t.amdhsa_kernel "):
            cur = (ln.split()[1], i)
        elif ln.startswith("\t.end_amdhsa_kernel") and cur:
            desc[cur[0]] = norm(lines[cur[1]:i + 1])
            cur = None
    starts = [i for i, ln in enumerate(lines) if ln.startswith("  - .")]  # metadata entries
    for a, b in zip(starts, starts[1:] + [len(lines)]):
        ent = {}
        for ln in lines[a:b]:
            m = re.match(r"\s+(?:- )?(\.\w+):\s+(\S+)$", ln)
            if m and len(ln) - len(ln.lstrip()) == 4 - 2 * ln.lstrip().startswith("- "):
                ent[m.group(1)] = m.group(2)
        if ".name" in ent:
            meta[ent[".name"]] = tuple(ent.get(k) for k in META)
    label = {}
    for i, ln in enumerate(lines):
        m = re.match(r"(\w+):", ln)
        if m and m.group(1) in desc:
            label[m.group(1)] = i
    out = {}
    for name, a in label.items():
        b = a
        while not lines[b].startswith(".Lfunc_end"):
            b += 1
        out[name] = {"text": norm(lines[a:b + 1]), "desc": desc[name], "meta": meta.get(name)}
    missing = set(desc) - set(out)
    if missing:
        sys.exit(f"{path}: no label for {sorted(missing)[:3]}")
    return out


def load(d, unit_re=None):
    ks, dup = {}, []
    for p in sorted(glob.glob(os.path.join(d, "*.s"))):
        unit = os.path.splitext(os.path.basename(p))[0]
        for name, k in parse(p).items():
            if name in ks:
                dup.append((name, ks[name]["unit"], unit))
            k["unit"] = unit
            ks[name] = k
    sel = {n for n, k in ks.items() if unit_re is None or re.search(unit_re, k["unit"])}
    return ks, sel, dup


def demangle(names):
    if not names:
        return {}
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return dict(zip(names, out))


a_dir, b_dir = sys.argv[1], sys.argv[2]
unit_re = sys.argv[3] if len(sys.argv) > 3 else None
A, selA, dupA = load(a_dir, unit_re)
B, _, dupB = load(b_dir)
bad = 0
for tag, dup in ((a_dir, dupA), (b_dir, dupB)):
    for name, u1, u2 in dup:
        bad += 1
        print(f"TWICE in {tag}: {name} in {u1} and {u2}")
diff = {}
for name in sorted(selA):
    if name not in B:
        diff[name] = ["missing"]
        continue
    what = [w for w in ("text", "desc", "meta") if A[name][w] != B[name][w]]
    if what:
        diff[name] = what
dm = demangle(sorted(diff))
for name, what in sorted(diff.items()):
    extra = ""
    if "meta" in what:
        extra = f"  {dict(zip(META, A[name]['meta']))} -> {dict(zip(META, B[name]['meta']))}"
    print(f"DIFFERS ({', '.join(what)}) [{A[name]['unit']}]: {dm[name]}{extra}")
selB_units = {B[n]["unit"] for n in selA if n in B}
only_b = sorted(n for n, k in B.items() if n not in A and (unit_re is None or k["unit"] in selB_units))
for name, d in demangle(only_b).items():
    print(f"ONLY IN {b_dir} [{B[name]['unit']}]: {d}")
units = {}
for n in selA:
    if n in B:
        units.setdefault((A[n]["unit"], B[n]["unit"]), []).append(n)
for (ua, ub), ns in sorted(units.items()):
    print(f"{ua} -> {ub}: {len(ns)} kernels, {sum(n not in diff for n in ns)} identical")
print(f"{len(selA)} kernels compared, {len(diff)} differ or are missing, {len(only_b)} only in B, "
      f"{len(dupA) + len(dupB)} defined twice")
sys.exit(1 if bad or diff else 0)
