#!/usr/bin/env python3
"""Static instruction counts of the kernels of one .hip file, on a CPU-only box (no GPU needed, about ten seconds).

Cross-compiles stereo_vo_amd/csrc/<file> to gfx950 assembly with the Makefile's FLAGS (`--cuda-device-only -S`, output in a
temp dir) and prints, per kernel symbol: total instructions, VALU / SALU / LDS / VMEM / SMEM totals, .vgpr_count, .sgpr_count,
scratch bytes, LDS bytes and the most frequent VALU opcodes.  STATIC counts: a loop body counts once, both sides of a branch
count.  They compare two forms of straight-line code; what a launch executes is SQ_INSTS_VALU (tools/pmc_passes.py).

Usage: python tools/isa_count.py k_detect.hip [--kernels k_resize,k_fast] [--top 12] [--ops v_lshrrev_b32,v_lshl_or_b32] [--json] [--src PATH]
  --kernels  names of the kernels to keep (demangled, with or without template arguments); default: every kernel of the file
  --ops      opcodes whose count is printed for every kernel, whether frequent or not
  --src      compile this file instead (another version of the same source; headers still come from csrc/ and include/)
"""
import argparse, collections, json, os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stereo_vo_amd", "csrc")


def make_var(name):
    """the value `make` gives a Makefile variable (FLAGS contains a probed option, so ask make itself)"""
    out = subprocess.run(["make", "-s", "-C", CSRC, "-f", "Makefile", "-f", "-", "_print"], input="_print:\n\t@echo $(%s)\n" % name,
                         capture_output=True, text=True, check=True).stdout
    return out.strip().split()


def classify(op):
    if op.startswith("v_"):
        return "VALU"
    if op.startswith(("ds_",)):
        return "LDS"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "VMEM"
    if op.startswith(("s_load", "s_buffer_load")):
        return "SMEM"
    if op.startswith("s_"):
        return "SALU"
    return "other"


def parse(asm):
    """assembly text -> {symbol: {"ops": Counter, "meta": {...}}}"""
    kernels, cur = {}, None
    for line in asm.splitlines():
        s = line.strip()
        m = re.match(r"^([A-Za-z_$][\w$.]*):", s)
        if m and not s.startswith(".L"):
            sym = m.group(1)
            cur = kernels.setdefault(sym, {"ops": collections.Counter(), "meta": {}}) if not sym.startswith(("__hip", ".")) else None
            continue
        if s.startswith(".end_amdhsa_kernel") or s.startswith(".Lfunc_end"):
            cur = None
            continue
        if cur is None or not s or s.startswith((".", ";", "/")) or s.endswith(":"):
            continue
        cur["ops"][s.split()[0]] += 1
    # the metadata note at the end of the file: one YAML record per kernel
    for rec in re.split(r"\n\s*- \.agpr_count:", asm)[1:]:
        name = re.search(r"\.name:\s+(\S+)", rec)
        if not name or name.group(1) not in kernels:
            continue
        meta = kernels[name.group(1)]["meta"]
        for key in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count"):
            v = re.search(r"\.%s:\s+(\d+)" % key, rec)
            if v:
                meta[key] = int(v.group(1))
        ag = re.match(r"\s*(\d+)", rec)
        if ag:
            meta["agpr_count"] = int(ag.group(1))
    return {k: v for k, v in kernels.items() if v["meta"]}


def demangle(names):
    try:
        out = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("file", help="a .hip file of stereo_vo_amd/csrc")
    ap.add_argument("--kernels", default="")
    ap.add_argument("--top", type=int, default=12)
    ap.add_argument("--ops", default="")
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--src", default=None)
    a = ap.parse_args()
    src = a.src or os.path.join(CSRC, a.file)
    hipcc = (make_var("HIPCC") or ["/opt/rocm/bin/hipcc"])[0]
    flags = make_var("FLAGS")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "out.s")
        # -I csrc: a --src copy outside the tree still finds svo_device.h / svo_kernels.h
        subprocess.run([hipcc] + flags + ["-I", CSRC, "-x", "hip", "--cuda-device-only", "-S", os.path.abspath(src), "-o", out], cwd=CSRC, check=True, stderr=subprocess.DEVNULL)
        kernels = parse(open(out).read())
    names = demangle(sorted(kernels))
    want = [w for w in a.kernels.split(",") if w]
    extra = [o for o in a.ops.split(",") if o]
    res = {}
    for sym in sorted(kernels):
        nm = re.sub(r"^void ", "", names[sym])
        short = nm.split("(")[0]
        if want and not any(w == short or w == short.split("<")[0] for w in want):
            continue
        ops, meta = kernels[sym]["ops"], kernels[sym]["meta"]
        cls = collections.Counter()
        for op, n in ops.items():
            cls[classify(op)] += n
        res[short] = {"total": sum(ops.values()), "classes": dict(cls), "vgpr_count": meta.get("vgpr_count"), "agpr_count": meta.get("agpr_count", 0), "sgpr_count": meta.get("sgpr_count"),
                      "scratch_bytes": meta.get("private_segment_fixed_size", 0), "lds_bytes": meta.get("group_segment_fixed_size", 0),
                      "vgpr_spills": meta.get("vgpr_spill_count", 0), "ops": dict(ops)}
    if a.json:
        print(json.dumps(res, indent=1, sort_keys=True))
        return 0
    for short, r in res.items():
        c = r["classes"]
        print("%s: %d instructions | VALU %d  SALU %d  LDS %d  VMEM %d  SMEM %d | .vgpr_count %s  .sgpr_count %s  scratch %d B  LDS %d B  spills %d" % (
            short, r["total"], c.get("VALU", 0), c.get("SALU", 0), c.get("LDS", 0), c.get("VMEM", 0), c.get("SMEM", 0), r["vgpr_count"], r["sgpr_count"], r["scratch_bytes"], r["lds_bytes"], r["vgpr_spills"]))
        valu = sorted(((n, op) for op, n in r["ops"].items() if op.startswith("v_")), reverse=True)
        print("    " + "  ".join("%s %d" % (op, n) for n, op in valu[:a.top]))
        if extra:
            # an opcode asked for without its encoding suffix counts every encoding of it
            enc = lambda op: sum(n for o, n in r["ops"].items() if o == op or o in (op + "_e32", op + "_e64", op + "_sdwa", op + "_dpp"))
            print("    asked for: " + "  ".join("%s %d" % (op, enc(op)) for op in extra))
    if not res:
        print("no kernel matched", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
