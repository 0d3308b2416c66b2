"""Times the training step on the device (K11) and writes profiles/train_time.json.

At batch 512: ms per gmk_train_step and per five-pass Trainer.train_step, the share of im2col / col2im, the GEMMs, the loss and Adam in a
step (from a rocprofv3 kernel trace when one is given with --trace CSV; otherwise left out), the achieved TFLOP/s on the 65 GFLOP count of
a step (3 x 42 MFLOP x 512: forward, input gradients, weight gradients), gmk_train_export against destroying and creating the fused
network through the host, and the yardstick: the same step on PolicyValueNetwork through torch autograd (MIOpen / rocBLAS) with an
equivalent hand-written TF1 Adam -- what a user could do before this kernel existed.

Method: settle (a second of the step itself), warm up, then HIP events around `--steps` steps, `--repeats` times; the median is reported,
with the spread.      python tools/train_time.py [--batch 512] [--steps 20] [--repeats 5] [--trace kernel_trace.csv]"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gomokuai_amd.network import FusedPolicyValueNetwork, PolicyValueNetwork, Trainer          # noqa: E402

STEP_GFLOP = 3 * 42e-3 * 512                       # the issue's count at batch 512, scaled by the batch below


def timed(fn, steps, repeats, settle_s=1.0):
    t0 = time.time()
    while time.time() - t0 < settle_s:
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / steps)
    return {"ms": float(np.median(out)), "min_ms": float(min(out)), "max_ms": float(max(out)), "repeats": repeats, "steps": steps}


class TorchStep:
    """The yardstick: autograd on the module + TF1 Adam with the L2 gradient, written with torch's foreach kernels."""

    def __init__(self, net):
        self.net, self.t = net, 0
        self.params = list(net.parameters())
        self.is_weight = [p.dim() > 1 for p in self.params]
        self.m = [torch.zeros_like(p) for p in self.params]
        self.v = [torch.zeros_like(p) for p in self.params]

    def step(self, states, values, pi, lr):
        x = states
        for conv in self.net.conv:
            x = torch.relu(conv(x))
        n = x.shape[0]
        p = torch.relu(self.net.policy_conv(x)).permute(0, 2, 3, 1).reshape(n, -1)
        v = torch.relu(self.net.value_conv(x)).permute(0, 2, 3, 1).reshape(n, -1)
        logits = self.net.policy_dense(p)
        value = torch.tanh(self.net.value_out(torch.relu(self.net.value_hidden(v)))).reshape(-1)
        loss = ((value - values) ** 2).mean() + (-(pi * torch.log_softmax(logits, 1)).sum(1)).mean()
        grads = torch.autograd.grad(loss, self.params)
        self.t += 1
        lr_t = lr * np.sqrt(1 - 0.999 ** self.t) / (1 - 0.9 ** self.t)
        with torch.no_grad():
            grads = [g + 1e-4 * p if w else g for g, p, w in zip(grads, self.params, self.is_weight)]
            torch._foreach_mul_(self.m, 0.9)
            torch._foreach_add_(self.m, grads, alpha=0.1)
            torch._foreach_mul_(self.v, 0.999)
            torch._foreach_addcmul_(self.v, grads, grads, value=0.001)
            denom = torch._foreach_sqrt(self.v)
            torch._foreach_add_(denom, 1e-8)
            torch._foreach_addcdiv_(self.params, self.m, denom, value=-lr_t)


def kernel_shares(path):
    """{group: share of the GPU time} from a rocprofv3 --kernel-trace CSV of this script."""
    groups = {"im2col / col2im": ("im2col3x3", "col2im3x3"), "GEMMs": ("train_gemm", "train_reduce"), "loss": ("train_loss", "train_metrics"), "Adam": ("train_adam",)}
    total, out = 0.0, {k: 0.0 for k in groups}
    for row in csv.DictReader(open(path)):
        name, dur = row.get("Kernel_Name", ""), float(row["End_Timestamp"]) - float(row["Start_Timestamp"])
        for g, keys in groups.items():
            if any(k in name for k in keys):
                out[g] += dur
                total += dur
    return {g: round(v / total, 4) for g, v in out.items()} if total else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--trace", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_time.json"))
    a = ap.parse_args()
    n = a.batch
    g = torch.Generator(device="cuda").manual_seed(1)
    states = (torch.rand((n, 6, 15, 15), device="cuda", generator=g) > 0.7).float()
    values = torch.rand(n, device="cuda", generator=g) * 2 - 1
    pi = torch.softmax(torch.randn((n, 225), device="cuda", generator=g), 1)
    net = PolicyValueNetwork(seed=1).cuda()
    trainer, fused = Trainer(net, max_batch=n), FusedPolicyValueNetwork(net)
    res = {"batch": n, "device": torch.cuda.get_device_name(0), "scratch_bytes": trainer._h.info()["scratch_bytes"]}
    res["gmk_train_step"] = timed(lambda: trainer.step(states, values, pi, 2e-3), a.steps, a.repeats)
    res["train_step_5_passes"] = timed(lambda: trainer.train_step(states, values, pi, 1e-9, 1e9, 5), max(1, a.steps // 5), a.repeats)
    res["tflops_on_the_65_gflop_count"] = STEP_GFLOP * n / 512 / res["gmk_train_step"]["ms"]
    res["gmk_train_export"] = timed(lambda: trainer.export(fused), a.steps, a.repeats, settle_s=0.2)

    def through_the_host():
        FusedPolicyValueNetwork(trainer.sync_to(net)).close()
    res["export_through_the_host"] = timed(through_the_host, 3, 3, settle_s=0.2)
    yard = TorchStep(PolicyValueNetwork(seed=1).cuda())
    res["torch_autograd_step"] = timed(lambda: yard.step(states, values, pi, 2e-3), a.steps, a.repeats)
    res["hip_over_torch"] = res["gmk_train_step"]["ms"] / res["torch_autograd_step"]["ms"]
    if a.trace:
        res["kernel_shares"] = kernel_shares(a.trace)
    json.dump(res, open(a.out, "w"), indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
