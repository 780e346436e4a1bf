"""Static instruction mix of the solve kernels (CPU only: hipcc cross-compiles the gfx950 assembly, nothing runs).

For every kernel of the given translation units whose name matches a filter: vector instructions by class, readlane / writelane,
exec-mask regions (s_and_saveexec / s_andn2_saveexec / s_or_saveexec) and s_cbranch_execz, s_nop, s_waitcnt, SGPR / VGPR spill counts, scratch,
VGPRs (AGPRs included), LDS and the occupancy that registers and LDS allow (one-wave workgroups: waves per CU = min(4 x waves per
SIMD by VGPRs, 160 KiB / LDS, 32); for the four-wave and generic kernels, whose workgroups are larger or use dynamic LDS, read it as waves per CU by registers).  Counts are static (instructions in the code object), not executed ones.

usage: python tools/static_mix.py [file.hip ...] [-k substring ...] [--json]
       default: every solve kernel (name contains `kmpc_solve`) of the four translation units that instantiate the solve --
       kmpc_fast.hip (one wave per problem, Cartesian, its three-waves-per-SIMD build and the Frenet functor), kmpc_wide.hip,
       kmpc_quad.hip and kmpc_kernels.hip (generic)
"""
import json, os, re, sys
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spill_exec_check as S  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mkz_mpc_path_follower_amd", "csrc")

# vector classes, first match wins; the data-movement classes are the ones that do no arithmetic
VCLASSES = [("mfma", re.compile(r"v_mfma_")),
            ("dpp", re.compile(r"v_\w+_dpp\b|\b(row_shr|row_shl|row_bcast|row_ror|wave_shr|wave_shl|quad_perm|row_mirror|row_half_mirror|row_newbcast):")),
            ("readlane", re.compile(r"v_readlane_b32|v_readfirstlane_b32")),
            ("writelane", re.compile(r"v_writelane_b32")),
            ("cndmask", re.compile(r"v_cndmask_")),
            ("mov", re.compile(r"v_mov_b(32|64)|v_accvgpr_(read|write|mov)")),
            ("f64", re.compile(r"v_\w+_f64")),
            ("f32", re.compile(r"v_\w+_f32")),
            ("other", re.compile(r"v_"))]
MOVE_CLASSES = ("dpp", "readlane", "writelane", "cndmask", "mov")


def metadata(asm):
    """kernel symbol -> fields of the amdhsa.kernels metadata (counts as int)"""
    out, cur = {}, None
    meta = asm[asm.find("amdhsa.kernels:"):]
    for l in meta.splitlines():
        m = re.match(r"^\s+-?\s*\.(\w+):\s+(\S+)\s*$", l)
        if not m:
            continue
        k, v = m.groups()
        if l.lstrip().startswith("- .agpr_count") or (k == "agpr_count" and cur is None):
            cur = {}
        if cur is None:
            continue
        cur[k] = int(v) if re.fullmatch(r"-?\d+", v) else v
        if k == "name":
            out[v] = cur
        if k == "wavefront_size":
            cur = None
    return out


def mix(body):
    c = {k: 0 for k, _ in VCLASSES}
    c.update(salu=0, exec_regions=0, execz_branches=0, s_nop=0, waitcnt=0, lines=0)
    for l in body:
        t = l.strip()
        if not t or t.startswith((";", ".")) or t.endswith(":"):
            continue
        op = t.split()[0]
        c["lines"] += 1
        if op.startswith("v_"):
            for name, rx in VCLASSES:
                if rx.search(t):
                    c[name] += 1
                    break
        elif op.startswith("s_"):
            if op == "s_nop":
                c["s_nop"] += 1
            elif op == "s_waitcnt":
                c["waitcnt"] += 1
            elif op.startswith(("s_and_saveexec", "s_andn2_saveexec", "s_or_saveexec")):
                c["exec_regions"] += 1
            elif op == "s_cbranch_execz":
                c["execz_branches"] += 1
            if not op.startswith(("s_cbranch", "s_branch", "s_waitcnt", "s_nop", "s_endpgm", "s_barrier", "s_setprio", "s_sleep")):
                c["salu"] += 1
    c["valu"] = sum(c[k] for k, _ in VCLASSES)
    c["valu_moves"] = sum(c[k] for k in MOVE_CLASSES)
    return c


def occupancy(vgprs, lds):
    """vgprs: the metadata's .vgpr_count, which on gfx950 already counts the AGPRs of the unified register file"""
    alloc = -(-vgprs // 8) * 8
    per_simd = min(8, 512 // max(alloc, 8))
    by_lds = 163840 // lds if lds else 32
    return min(4 * per_simd, by_lds, 32)


def analyse(src, filters):
    asm = S.device_asm(src)
    md = metadata(asm)
    rows = []
    names = [k for k, _ in S.kernels(asm)]
    dem = dict(zip(names, S.demangle(names))) if names else {}
    for k, body in S.kernels(asm):
        d = dem[k]
        if filters and not any(f in d for f in filters):
            continue
        if k not in md:
            continue
        m = md[k]
        r = {"kernel": d, "file": os.path.basename(src)}
        r.update(mix(body))
        r.update(sgpr_spill=m.get("sgpr_spill_count", 0), vgpr_spill=m.get("vgpr_spill_count", 0),
                 scratch=m.get("private_segment_fixed_size", 0), sgprs=m.get("sgpr_count", 0), vgprs=m.get("vgpr_count", 0),
                 agprs=m.get("agpr_count", 0), lds=m.get("group_segment_fixed_size", 0))
        r["waves_per_cu"] = occupancy(r["vgprs"], r["lds"])
        rows.append(r)
    return rows


COLS = [("valu", 6), ("valu_moves", 6), ("dpp", 5), ("readlane", 5), ("writelane", 5), ("cndmask", 5), ("mov", 5), ("mfma", 5),
        ("salu", 6), ("exec_regions", 5), ("execz_branches", 5), ("s_nop", 5), ("waitcnt", 5), ("sgpr_spill", 5), ("vgpr_spill", 5), ("scratch", 5),
        ("sgprs", 5), ("vgprs", 5), ("lds", 6), ("waves_per_cu", 4)]
HEAD = ["VALU", "moves", "dpp", "rdln", "wrln", "cndm", "mov", "mfma", "SALU", "exec", "execz", "nop", "wait", "sSpl", "vSpl", "scr",
        "SGPR", "VGPR", "LDS", "w/CU"]


def main(argv):
    files, filters, as_json = [], [], False
    i = 0
    while i < len(argv):
        if argv[i] == "-k":
            filters.append(argv[i + 1]); i += 2; continue
        if argv[i] == "--json":
            as_json = True
        else:
            files.append(argv[i])
        i += 1
    if not files:
        files = [os.path.join(CSRC, f) for f in ("kmpc_fast.hip", "kmpc_wide.hip", "kmpc_quad.hip", "kmpc_kernels.hip")]
    filters = filters or ["kmpc_solve"]
    with ThreadPoolExecutor(4) as ex:
        rows = [r for rs in ex.map(lambda f: analyse(f, filters), files) for r in rs]
    if as_json:
        print(json.dumps(rows, indent=1))
        return
    print("%-52s " % "kernel" + " ".join("%*s" % (w, h) for (_, w), h in zip(COLS, HEAD)))
    for r in rows:
        print("%-52s " % r["kernel"][:52] + " ".join("%*d" % (w, r[k]) for k, w in COLS))


if __name__ == "__main__":
    main(sys.argv[1:])
