#!/usr/bin/env python3
"""usage: python3 tools/isa_counts.py [--asm FILE.s] [--kernel REGEX] [--label NAME]
Opcode-class counts of ONE kernel's view loop from the gfx950 assembly of the solver's translation unit (no GPU needed).
Without --asm the unit is compiled to assembly first (device side only, the flags of csrc/Makefile).  A view loop is the
smallest backward-branch range around an MFMA -- k_eval_gram4 has two, the full path and the constant-pose path, reported one
after the other; inside it the MFMAs are the landmarks of the phases the
wave timeline stamps: geometry (loop top .. first MFMA), MFMA u (first half of the MFMAs), copy (between the halves), MFMA v,
epilogue (last MFMA .. loop end).  The scheduler moves instructions across those landmarks, so the split is where the
instructions ARE ISSUED, not where the source wrote them; the totals per iteration do not depend on it.  Blocks the loop jumps
over (the zeroing of a lost corner's rows) are counted where they stand.  Default kernel: k_eval_gram4<14, false, false>."""
import argparse, os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tscm_calib_amd", "csrc")
PHASES = ["geometry", "mfma_u", "copy", "mfma_v", "epilogue"]
CLASSES = ["mfma", "valu_fp64", "valu_dpp_mov", "valu_cndmask", "valu_int_mov", "valu_accvgpr", "valu_lane", "lds", "vmem", "smem",
           "salu", "wait_nop", "branch"]
VALU = ["valu_fp64", "valu_dpp_mov", "valu_cndmask", "valu_int_mov", "valu_accvgpr", "valu_lane"]


def classify(op, rest):
    if op.startswith("v_mfma"): return "mfma"
    if op.startswith("v_accvgpr"): return "valu_accvgpr"
    if op.startswith("v_"):
        if "quad_perm" in rest or "row_" in rest or "dpp" in op:
            if op.startswith("v_mov"): return "valu_dpp_mov"
            return "valu_fp64" if "f64" in op else "valu_int_mov"
        if op.startswith("v_cndmask"): return "valu_cndmask"
        if op.startswith(("v_readlane", "v_readfirstlane", "v_writelane")): return "valu_lane"
        if "f64" in op: return "valu_fp64"
        return "valu_int_mov"
    if op.startswith("ds_"): return "lds"
    if op.startswith(("buffer_", "global_", "flat_", "scratch_")): return "vmem"
    if op.startswith(("s_load", "s_buffer_load")): return "smem"
    if op.startswith(("s_waitcnt", "s_nop", "s_barrier", "s_setprio", "s_sleep")): return "wait_nop"
    if op.startswith(("s_cbranch", "s_branch", "s_endpgm")): return "branch"
    if op.startswith("s_"): return "salu"
    return None


def compile_asm(out):
    cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function", "-I" + os.path.join(ROOT, "include"),
           "-I" + CSRC, "--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, "tscm_solver.hip")]
    subprocess.check_call(cmd)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--asm"); ap.add_argument("--kernel", default=r"k_eval_gram4<14, false, false>"); ap.add_argument("--label", default="")
    a = ap.parse_args()
    if a.asm:
        lines = open(a.asm).read().split("\n")
    else:
        with tempfile.TemporaryDirectory() as tmp:
            compile_asm(os.path.join(tmp, "tscm_solver.s"))
            lines = open(os.path.join(tmp, "tscm_solver.s")).read().split("\n")
    # the kernel's text: from its label to its .Lfunc_end
    syms = [m.group(1) for l in lines for m in [re.match(r"^(_Z\w+):", l)] if m]
    dem = subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True, text=True).stdout.split("\n")
    sym = [s for s, d in zip(syms, dem) if re.search(re.escape(a.kernel) + r"\(", d)]
    if len(sym) != 1: sys.exit(f"kernel pattern matches {len(sym)} symbols")
    sym = sym[0]
    beg = next(i for i, l in enumerate(lines) if l.startswith(sym + ":"))
    end = next(i for i in range(beg, len(lines)) if lines[i].startswith(".Lfunc_end"))
    body = lines[beg:end]
    ins, labels = [], {}            # (op, rest) in order; label -> index of the next instruction
    for l in body:
        m = re.match(r"^(\.LBB\w+):", l)
        if m: labels[m.group(1)] = len(ins); continue
        m = re.match(r"^\s+([a-z]\w+)\s*(.*?)\s*(;.*)?$", l)
        if m and classify(m.group(1), m.group(2)): ins.append((m.group(1), m.group(2)))
    mf = [k for k, (op, _) in enumerate(ins) if op.startswith("v_mfma")]
    loops = []                      # backward branches: (first instruction of the target block, the branch)
    for k, (op, r) in enumerate(ins):
        target = r.split()[-1] if r else ""
        if op.startswith(("s_cbranch", "s_branch")) and target in labels and labels[target] <= k:
            loops.append((labels[target], k))
    # the view loop of each path: the smallest backward-branch range around an MFMA (one range for a kernel with one loop; two
    # for k_eval_gram4: the full path and, with two thirds of its MFMAs, the constant-pose path)
    paths = {}
    for m in mf:
        around = [lp for lp in loops if lp[0] <= m <= lp[1]]
        if not around: sys.exit("an MFMA of the kernel stands outside every loop")
        paths.setdefault(min(around, key=lambda lp: lp[1] - lp[0]), []).append(m)
    paths = sorted(paths.items(), key=lambda kv: -len(kv[1]))
    names = ["full path", "constant-pose path"] if len(paths) == 2 else [f"loop {k}" for k in range(len(paths))]
    tabs = []
    for (lo, hi), pm in paths:
        half = len(pm) // 2
        marks = [pm[0], pm[half - 1] + 1, pm[half], pm[-1] + 1]      # first instruction of mfma_u, copy, mfma_v, epilogue
        tab = {p: dict.fromkeys(CLASSES, 0) for p in PHASES}
        for k in range(lo, hi + 1):
            tab[PHASES[sum(k >= m for m in marks)]][classify(*ins[k])] += 1
        tabs.append((lo, hi, pm, tab))
    # resources: the kernel descriptor's directives and the compiler's remarks behind the function
    txt = "\n".join(lines[end:end + 400])
    remarks = [("vgpr", r"; NumVgprs: (\d+)"), ("agpr", r"; NumAgprs: (\d+)"), ("sgpr", r"; TotalNumSgprs: (\d+)"), ("scratch", r"; ScratchSize: (\d+)"),
               ("occupancy", r"; Occupancy: (\d+)"), ("lds_static", r"; LDSByteSize: (\d+)"), ("code_bytes", r"; codeLenInByte = (\d+)")]
    res = {k: (re.search(p, txt) or [None, "?"])[1] for k, p in remarks}
    for name, (lo, hi, pm, tab) in zip(names, tabs):
        print(f"# {a.kernel}{'  [' + a.label + ']' if a.label else ''}, {name}: one iteration of the view loop ({hi - lo + 1} instructions, {len(pm)} MFMAs)")
        print(f"{'class':14s}" + "".join(f"{p:>10s}" for p in PHASES) + f"{'total':>10s}")
        for c in CLASSES:
            print(f"{c:14s}" + "".join(f"{tab[p][c]:10d}" for p in PHASES) + f"{sum(tab[p][c] for p in PHASES):10d}")
        print(f"{'VALU (all)':14s}" + "".join(f"{sum(tab[p][c] for c in VALU):10d}" for p in PHASES) + f"{sum(tab[p][c] for p in PHASES for c in VALU):10d}")
    print("resources: " + "  ".join(f"{k} {v}" for k, v in res.items()))


if __name__ == "__main__":
    main()
