#!/usr/bin/env python3
"""K1's frame, static instruction counts (a recipe, not a test: they move with the compiler): compiles eval_kernel.hip as the production
build does plus -DGMK_K1_MARKERS, which turns every GMK_STAMP(k) of the board loop into an assembly comment `; gmk_mark k`, and counts the
vector, scalar, LDS and global-memory instructions in the text from a mark to the next mark (or the kernel's end); two more marks exist in
this build only: 10 at the top of the board loop, 12 in front of phase 5; what lies between the kernel's entry and mark 0 is counted as region -1.  A region is named by what the source holds behind its opening
mark.  The text is counted as it lies: a block the compiler moved out of line counts where it was put (the density bursts lie behind
mark 8, phase 5 behind them), and a loop's body counts once, so the figures are good for the straight-line frame regions (loop head,
phase 0 with ONE pass of its stone loop, phase 5) and for comparing two builds of the same source, not as per-board dynamic counts.  A mark is a scheduling barrier, so the marked build is not the production one instruction for instruction.
usage: k1_frame_counts.py [file.s | file.hip] ...   (default: gomokuai_amd/csrc/eval_kernel.hip; needs hipcc for a .hip)"""
import os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {-1: "entry, staging", 0: "prologue", 9: "loop tail", 10: "loop head", 11: "phase 0", 1: "scan", 2: "deposits", 3: "phase 3", 4: "phase 3b", 5: "rescans", 6: "planes wait", 7: "burst hand-out",
         8: "phase D bursts", 12: "phase 5"}
FRAME = (10, 11, 12)


def assembly(src):
    if src.endswith(".s"):
        return open(src).read()
    sys.path.insert(0, ROOT)
    from gomokuai_amd import build as B
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k1.s")
        flags = [f for f in B.FLAGS if f != "-fPIC"] + ["-DGMK_K1_MARKERS"]
        subprocess.check_call([B.HIPCC] + flags + ["--cuda-device-only", "-S", "-x", "hip", src, "-o", out], stderr=subprocess.DEVNULL)
        return open(out).read()


def classify(op):
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "vmem"
    if op.startswith("v_"):
        return "valu"
    return "salu"


def report(src):
    text = assembly(src)
    print("== %s" % src)
    for key in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
        m = re.search(r"\.%s:\s*(\d+)" % key, text)
        print("%s %s" % (key, m.group(1) if m else "?"))
    order, cur = [], None
    for line in (l.strip() for l in text.splitlines()):
        if re.match(r"^_Z\w*eval_positions_kernel\w*:", line):         # the kernel's entry: what lies in front of mark 0 (the tables' staging)
            cur = {"valu": 0, "salu": 0, "lds": 0, "vmem": 0, "lanes": 0, "opens": -1}
            order.append(cur)
            continue
        m = re.match(r"^; gmk_mark (\d+)", line)
        if m:
            cur = {"valu": 0, "salu": 0, "lds": 0, "vmem": 0, "lanes": 0, "opens": int(m.group(1))}
            order.append(cur)
            continue
        if line.startswith("s_endpgm"):
            cur = None
        if cur is None or not re.match(r"^(v_|s_|ds_|global_|flat_|scratch_|buffer_)", line):
            continue
        op = line.split()[0]
        cur[classify(op)] += 1
        cur["lanes"] += op.startswith(("v_readlane", "v_writelane"))
    total = {"valu": 0, "salu": 0, "lds": 0, "vmem": 0, "lanes": 0}
    for r in order:
        print("mark %2d -> (%-14s): vector %4d (of them %2d v_readlane/v_writelane), scalar %4d, LDS %3d, global %3d"
              % (r["opens"], NAMES.get(r["opens"], "?"), r["valu"], r["lanes"], r["salu"], r["lds"], r["vmem"]))
        for k in total:
            total[k] += r[k]
    frame = [r for r in order if r["opens"] in FRAME]
    print("frame (loop head + phase 0 + phase 5): vector %d, scalar %d, LDS %d; all marked regions: vector %d, scalar %d, LDS %d"
          % (sum(r["valu"] for r in frame), sum(r["salu"] for r in frame), sum(r["lds"] for r in frame), total["valu"], total["salu"], total["lds"]))


if __name__ == "__main__":
    for s in sys.argv[1:] or [os.path.join(ROOT, "gomokuai_amd", "csrc", "eval_kernel.hip")]:
        report(s)
