"""Instruction identity of two source trees (CPU only: hipcc cross-compiles the gfx950 assembly, nothing runs).

For a change that must not move the device code -- a rewrite of launchers, dispatch or host entry points -- compile every device translation unit
of both trees to gfx950 assembly and compare, kernel by kernel under the demangled name:
  (a) the set of kernels: none added, none lost (a translation unit that only one tree has counts as all its kernels added or lost);
  (b) the instruction stream, after normalising only what cannot matter: assembler comments and directives, the function index in local labels
      (.LBB<function>_<n>, .Lfunc_end<function>: it follows the order of the functions in the file), and pc-relative literal offsets (sym@rel32@lo+<k>);
  (c) the amdhsa.kernels metadata: VGPR / AGPR / SGPR counts, both spill counts, scratch and LDS bytes.

usage: python tools/isa_diff.py PARENT_CSRC NEW_CSRC [-j JOBS] [-D MACRO ...]     exit code 1 on any difference
"""
import difflib, glob, os, re, subprocess, sys
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spill_exec_check as S  # noqa: E402
import static_mix as M  # noqa: E402

META = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")


def normalise(body):
    out = []
    for l in body:
        t = l.split(";")[0].strip()
        if not t or (t.startswith(".") and not t.endswith(":")):   # comments, directives (labels stay)
            continue
        t = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", t)
        t = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", t)
        t = re.sub(r"@rel32@(lo|hi)\+\d+", r"@rel32@\1", t)
        out.append(re.sub(r"\s+", " ", t))
    return out


def kernel_table(asm):
    """demangled kernel name -> (normalised instructions, metadata fields)"""
    meta = M.metadata(asm)
    bodies = {n: b for n, b in S.kernels(asm) if n in meta}
    names = sorted(bodies)
    dem = subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.splitlines() if names else []
    return {d: (normalise(bodies[n]), tuple(meta[n].get(k) for k in META)) for n, d in zip(names, dem)}


def compare(label, old, new, show=6):
    """print the differences of two kernel tables -> number of kernels that differ (added and lost ones included)"""
    nbad = 0
    for k in sorted(set(old) - set(new)):
        print("%s: LOST   %s" % (label, k)); nbad += 1
    for k in sorted(set(new) - set(old)):
        print("%s: ADDED  %s" % (label, k)); nbad += 1
    for k in sorted(set(old) & set(new)):
        (io, mo), (in_, mn) = old[k], new[k]
        if mo != mn:
            print("%s: METADATA %s\n    %s\n    parent %s\n    new    %s" % (label, k, META, mo, mn))
        if io != in_:
            d = [l for l in difflib.unified_diff(io, in_, "parent", "new", lineterm="", n=0) if not l.startswith(("---", "+++"))]
            print("%s: INSTRUCTIONS %s: %d / %d lines, %d diff lines" % (label, k, len(io), len(in_), len(d)))
            for l in d[:show]:
                print("    " + l)
        nbad += mo != mn or io != in_
    print("%-20s %3d kernels in the parent, %3d in the new tree, %6d instructions compared, %d differ" %
          (label, len(old), len(new), sum(len(new[k][0]) for k in set(old) & set(new)), nbad))
    return nbad


def main(argv):
    defs, jobs = [], min(8, len(os.sched_getaffinity(0)))
    while "-D" in argv:
        k = argv.index("-D"); defs.append(argv[k + 1]); del argv[k:k + 2]
    if "-j" in argv:
        k = argv.index("-j"); jobs = int(argv[k + 1]); del argv[k:k + 2]
    if len(argv) != 2:
        print(__doc__); return 2
    old_dir, new_dir = argv
    units = sorted(set(os.path.basename(f) for d in (old_dir, new_dir) for f in glob.glob(os.path.join(d, "*.hip"))))
    work = [(d, u) for u in units for d in (old_dir, new_dir) if os.path.exists(os.path.join(d, u))]   # a unit only one tree has: all ADDED / LOST
    with ThreadPoolExecutor(jobs) as ex:   # the longest units first
        order = sorted(work, key=lambda w: -os.path.getsize(os.path.join(*w)))
        asm = dict(zip(order, ex.map(lambda w: kernel_table(S.device_asm(os.path.join(*w), defs)), order)))
    nbad = sum(compare(u, asm.get((old_dir, u), {}), asm.get((new_dir, u), {})) for u in units)
    print("kernels that differ:", nbad)
    return 1 if nbad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
