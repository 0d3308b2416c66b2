#!/usr/bin/env python3
"""K1 phase D, static instruction counts (a recipe, not a test: they move with the compiler): disassembles the production build of
eval_kernel.hip and counts, per copy of the density burst's fourteen passes (62 v_mfma each: from the first MFMA's operand reads to
the last pass's last store; the burst's prologue -- plane loads, occupied words, cell 224 -- is not in the range), the vector, scalar, LDS,
global-memory and branch instructions.  A copy without conditional branches is the full-group form.
usage: k1_burst_counts.py [file.s | file.hip]   (default: gomokuai_amd/csrc/eval_kernel.hip; needs hipcc for a .hip)"""
import os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
src = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "gomokuai_amd", "csrc", "eval_kernel.hip")
if src.endswith(".s"):
    text = open(src).read()
else:
    sys.path.insert(0, ROOT)
    from gomokuai_amd import build as B
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k1.s")
        flags = [f for f in B.FLAGS if f != "-fPIC"]
        subprocess.check_call([B.HIPCC] + flags + ["--cuda-device-only", "-S", "-x", "hip", src, "-o", out], stderr=subprocess.DEVNULL)
        text = open(out).read()
for key in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
    m = re.search(r"\.%s:\s*(\d+)" % key, text)
    print("%s %s" % (key, m.group(1) if m else "?"))
lines = [l.strip() for l in text.splitlines()]
insts = [(i, l.split()[0]) for i, l in enumerate(lines) if re.match(r"^(v_|s_|ds_|global_|flat_|scratch_|buffer_)", l)]
mfma = [k for k, (_, op) in enumerate(insts) if op.startswith("v_mfma")]
for c in range(len(mfma) // 62):
    first, last = mfma[62 * c], mfma[62 * c + 61]
    start = first
    while start > 0 and insts[start - 1][1].startswith("ds_read"):      # the first MFMA's operand reads
        start -= 1
    end = last
    stores = 0
    while stores < 16:                                                  # the last pass's eight store pairs
        end += 1
        stores += insts[end][1].startswith("global_store")
    ops = [op for _, op in insts[start:end + 1]]
    count = lambda pred: sum(1 for op in ops if pred(op))
    branches = count(lambda op: op.startswith(("s_cbranch", "s_branch")))
    print("burst copy %d (%s): vector %d (of them %d v_mfma, %d v_readlane/v_writelane), scalar %d (of them %d branches, %d s_waitcnt, %d s_nop), LDS %d (%d ds_bpermute), global stores %d"
          % (c, "full groups" if branches == 0 else "guarded", count(lambda op: op.startswith("v_")), count(lambda op: op.startswith("v_mfma")),
             count(lambda op: op.startswith(("v_readlane", "v_writelane"))), count(lambda op: op.startswith("s_")), branches, count(lambda op: op == "s_waitcnt"),
             count(lambda op: op == "s_nop"), count(lambda op: op.startswith("ds_")), count(lambda op: op == "ds_bpermute_b32"), count(lambda op: op.startswith("global_store"))))
