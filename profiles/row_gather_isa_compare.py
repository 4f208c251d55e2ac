#!/usr/bin/env python3
"""Same machine code?  Compiles translation units of two source trees for the device only (the Makefile's flags +
--cuda-device-only -S, no GPU needed) and compares the gfx950 assembly kernel by kernel.  Without --files: gat_kernels.hip,
gcn2_kernels.hip and pna_kernels.hip, as for the row-gather scaffold.

    python profiles/row_gather_isa_compare.py PARENT_CSRC [RESULT_CSRC] > profiles/row_gather_isa_compare.txt
    python profiles/row_gather_isa_compare.py --files hop_unity.hip,loss_kernels.hip --no-diffs PARENT_CSRC > report.txt

  --files A,B,...  the translation units to compare; then a rise of ANY kernel's count fails, not only a GAT *_chunks_k kernel's
  --no-diffs       list the kernels that differ with their counts, without the instruction diffs
  --table          before each file's report, one line per kernel whose counts differ, with both sides' counts

  - every kernel of the parent must exist in the result, and no new one may appear; kernels are named as the demangler prints
    them, RENAME maps the parent's names of the kernels that moved into row_sum.h to the result's, and TYPE_RENAME the epilogue
    and scale types of SAGEConv's and ClusterGCNConv's aggregation to the one type that replaced each pair;
  - a file that one tree lacks holds no kernel there, and a parent's kernel is looked for in every compared file of the result:
    the aggregation moved from sage_kernels.hip and cluster_kernels.hip to rootsum_kernels.hip;
  - a kernel's instruction stream is compared after comments are dropped and basic-block labels renumbered in order of appearance;
  - the three GAT *_chunks_k families took the strict item decode on purpose: for them the register, scratch and LDS counts of
    the code object's metadata must not rise;
  - every other kernel that differs — in its instructions, or in its counts alone — is listed with its counts; the diff itself
    is printed for the first instantiation of each kernel template (the others of a template differ the same way; --all-diffs
    prints them all);
  - a renamed kernel changed on purpose: its counts in the parent and in the result are listed side by side, with any rise marked,
    and the opcodes whose number changed stand in for the diff.
The occupancy (waves per SIMD, from -Rpass-analysis=kernel-resource-usage) is listed beside the counts; a fall counts as a rise.
Exit status 1 when a symbol is missing or new, a count of a GAT *_chunks_k kernel rises or, with --files, any kernel's."""
import argparse
import collections
import difflib
import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CXXFILT = os.environ.get("CXXFILT", "c++filt")
FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-Wall", "-Wno-unused-function", "--cuda-device-only", "-S"]
FILES = ["gat_kernels.hip", "gcn2_kernels.hip", "pna_kernels.hip"]
EXTRA = {"sampler_kernels.hip": ["-ffp-contract=off"]}                      # (the Makefile's EXTRA_<unit>)
EXPECTED = ("gat_fwd_chunks_k", "gat_bwd_dst_chunks_k", "gat_bwd_src_chunks_k")
# parent kernel -> (result kernel, trailing template argument): the plain-sum gather GCN2Conv and SAGEConv share (row_sum.h)
RENAME = {"gcn2_rows_k": ("row_sum_rows_k", "G2Epi"), "gcn2_chunks_k": ("row_sum_chunks_k", None), "gcn2_combine_k": ("row_sum_combine_k", "G2Epi"),
          "sage_rows_k": ("row_sum_rows_k", "SageEpi"), "sage_chunks_k": ("row_sum_chunks_k", None), "sage_combine_k": ("row_sum_combine_k", "SageEpi")}
# parent template argument -> the result's: SageEpi and ClusterEpi became RootSumEpi, their row-scale functors RootSumScale
TYPE_RENAME = {"SageEpi": "RootSumEpi", "ClusterEpi": "RootSumEpi", "SageScale": "RootSumScale", "ClusterScale": "RootSumScale"}
COUNTS = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")
OCC = "occupancy"


def worse(a, b):
    """the counts of b that are worse than a's: a resource count that rose, or the occupancy where it fell"""
    return [c for c in COUNTS if b[c] > a[c]] + [OCC + " FALLS" for _ in (0,) if b[OCC] < a[OCC]]


def counts_line(a, b):
    return ", ".join(f"{c} {a[c]} -> {b[c]}" for c in COUNTS + (OCC,))


def assembly(csrc, name, tmp):
    """(the assembly text, {mangled kernel: occupancy in waves per SIMD as -Rpass-analysis=kernel-resource-usage reports it})"""
    out = os.path.join(tmp, name + ".s")
    if not os.path.exists(os.path.join(csrc, name)):                        # (a file of the other tree alone)
        return "", {}
    run = subprocess.run([HIPCC] + FLAGS + ["-Rpass-analysis=kernel-resource-usage"] + EXTRA.get(name, []) +
                         [os.path.join(csrc, name), "-o", out], stderr=subprocess.PIPE, text=True)
    if run.returncode:
        sys.stderr.write(run.stderr)
        raise subprocess.CalledProcessError(run.returncode, run.args)
    occ, name_now = {}, None
    for ln in run.stderr.split("\n"):
        m = re.search(r"remark: +(Function Name: (\S+)|Occupancy \[waves/SIMD\]: (\d+))", ln)
        if m and m.group(2):
            name_now = m.group(2)
        elif m:
            occ[name_now] = int(m.group(3))
    return open(out).read(), occ


def renamed(key):
    """The result's name of the parent's kernel `key` ('name' or 'name<args>'), or None where it keeps its name."""
    name, _, args = key.partition("<")
    if name not in RENAME:
        to = re.sub(r"\b(%s)\b" % "|".join(TYPE_RENAME), lambda t: TYPE_RENAME[t.group(0)], key)
        return to if to != key else None
    new, last = RENAME[name]
    targs = [t for t in (args[:-1], last) if t]
    return new + ("<" + ", ".join(targs) + ">" if targs else "")


def kernels(text_occ):
    """{kernel as the demangler prints it, without return type and parameters: (normalised instruction lines, {count: value})};
    the counts hold OCC as well, the one that must not FALL"""
    text, occ = text_occ
    meta = {}
    for blk in text.split("- .agpr_count:")[1:]:
        nm = re.search(r"\.name:\s+(\S+)", blk).group(1)
        meta[nm] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1)) for k in COUNTS}
        meta[nm][OCC] = occ[nm]
    body = {}
    for nm in meta:
        m = re.search(r"^%s:[^\n]*\n(.*?)^\s*\.section\s" % re.escape(nm), text, re.S | re.M)
        labels, lines = {}, []
        for ln in m.group(1).split("\n"):
            ln = ln.split(";")[0].rstrip()
            if ln.strip():
                lines.append(re.sub(r"\.LBB\d+_\d+", lambda t: labels.setdefault(t.group(0), ".L%d" % len(labels)), ln))
        body[nm] = lines
    names = list(meta)
    plain = subprocess.run([CXXFILT], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    keys = {nm: re.sub(r"^void ", "", d.split("(")[0]) for nm, d in zip(names, plain)}
    assert len(set(keys.values())) == len(names), "two kernels demangle to one name"
    return {keys[nm]: (body[nm], meta[nm]) for nm in meta}


def table_rows(name, a, b):
    """One line per kernel whose counts differ, in the format of profiles/row_list_resources.txt (SGPR VGPR LDS scratch occupancy,
    parent | new), then one line for the file's other kernels."""
    cols = ("sgpr_count", "vgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", OCC)
    same = 0
    for k in sorted(set(a) & set(b)):
        ca, cb = ([m[1][c] for c in cols] for m in (a[k], b[k]))
        fmt = lambda v: f"{v[0]:4d} {v[1]:4d} {v[2]:5d} {v[3]:7d} {v[4]:3d}"
        if ca == cb:
            same += 1
            continue
        w = worse(a[k][1], b[k][1])
        yield f"{name.split('_')[0]:8s} {k:42s} | {fmt(ca)} | {fmt(cb)} |" + (" worse: " + ", ".join(w) if w else "")
    yield f"{name.split('_')[0]:8s} ({same} other kernels: the same counts on both sides)"


def main(parent, result, all_diffs=False, files=None, no_diffs=False, table=False):
    bad, other, shown = 0, 0, set()
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        both = {name: (kernels(assembly(parent, name, ta)), kernels(assembly(result, name, tb))) for name in files or FILES}
        pool = {k: v for _, b in both.values() for k, v in b.items()}      # (a template two files instantiate is one kernel)
        wanted = {name: {to for k in a for to in (k, renamed(k)) if to} for name, (a, _) in both.items()}
        for name, (a, own) in both.items():
            # the result's side of this file: its own kernels but those that only another file's parent accounts for, and the
            # kernels this file's parent names that another compared file of the result holds
            others = set().union(*(w for n, w in wanted.items() if n != name))
            b = {k: v for k, v in own.items() if k in wanted[name] or k not in others}
            b.update({k: pool[k] for k in wanted[name] if k not in own and k in pool})
            moved = {k: renamed(k) for k in a if k not in b and renamed(k) in b}
            if table:
                print("\n".join(table_rows(name, a, b)))
            missing, new = sorted(set(a) - set(b) - set(moved)), sorted(set(b) - set(a) - set(moved.values()))
            same = [k for k in a if k in b and a[k][0] == b[k][0]]
            print(f"== {name}: {len(a)} kernels in the parent, {len(b)} in the result, {len(same)} with identical instruction streams")
            for k, to in sorted(moved.items()):
                rises = worse(a[k][1], b[to][1])
                print(f"  renamed (changed on purpose): {k} -> {to}")
                print(f"      instructions {len(a[k][0])} -> {len(b[to][0])}; " +
                      counts_line(a[k][1], b[to][1]) + ("; RISES: " + ", ".join(rises) if rises else ""))
                ha, hb = (collections.Counter(ln.split()[0] for ln in side if not ln.endswith(":")) for side in (a[k][0], b[to][0]))
                print("      opcodes: " + ", ".join(f"{op} {ha[op]} -> {hb[op]}" for op in sorted(set(ha) | set(hb)) if ha[op] != hb[op]))
            for k in missing:
                print("  MISSING in the result:", k)
            for k in new:
                print("  NEW in the result:", k)
            bad += len(missing) + len(new)
            for k in sorted(set(a) & set(b)):
                if a[k][0] == b[k][0] and a[k][1] == b[k][1]:
                    continue
                expected = any(e in k for e in EXPECTED)
                rises = worse(a[k][1], b[k][1])
                if a[k][0] == b[k][0]:
                    print(f"  same instructions, other counts: {k}")
                else:
                    print(f"  {'differs (strict item decode)' if expected else 'DIFFERS'}: {k}")
                print(f"      instructions {len(a[k][0])} -> {len(b[k][0])}; " +
                      counts_line(a[k][1], b[k][1]) + ("; RISES: " + ", ".join(rises) if rises else ""))
                if expected:
                    bad += 1 if rises else 0
                    continue
                other += 1
                bad += 1 if files and rises else 0
                if no_diffs:
                    continue
                diff = list(difflib.unified_diff(a[k][0], b[k][0], "parent", "result", lineterm="", n=1))
                template = k.split("<")[0]
                if all_diffs or template not in shown:
                    print("\n".join("      " + d for d in diff))
                else:
                    print(f"      ({sum(d[0] == '-' for d in diff[2:])} lines removed, {sum(d[0] == '+' for d in diff[2:])} added: like the template's first instantiation above)")
                shown.add(template)
    print(f"result: {'FAIL' if bad else 'ok'} (symbols equal and no count of {'any' if files else 'a GAT *_chunks_k'} kernel rises); "
          f"{other} other kernels differ, listed above")
    return 1 if bad else 0


if __name__ == "__main__":
    here = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "grapes_amd", "csrc")
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("parent"); ap.add_argument("result", nargs="?", default=here)
    ap.add_argument("--files", type=lambda v: v.split(","))
    ap.add_argument("--all-diffs", action="store_true"); ap.add_argument("--no-diffs", action="store_true")
    ap.add_argument("--table", action="store_true")
    a = ap.parse_args()
    sys.exit(main(a.parent, a.result, all_diffs=a.all_diffs, files=a.files, no_diffs=a.no_diffs, table=a.table))
