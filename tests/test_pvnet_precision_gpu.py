"""K9 against float64: gmk_pvnet_forward (pflat / vflat) and gmk_pvnet_evaluate (value / probs) held to the float64 forward pass of
tests/pvnet_reference.py under its element-wise rounding bound, on every input class and weight variant, at batch sizes around the dense
kernel's groups of 16 and the trunk's grid (grid = min(n, cu_count), workgroup w takes positions w, w + grid, ...).  Then batch isolation: a
position's outputs are the same bits whatever else is in the batch and wherever it sits, even next to a position whose head activations
overflow to +Inf."""
import numpy as np
import pytest
import torch

import pvnet_reference as R
from gomokuai_amd import lib as G
from gomokuai_amd.network import FusedPolicyValueNetwork

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cu_count():
    G.init()
    return G.device_info()["cu_count"]


def _run(fused, x):
    """-> dict pflat, vflat (gmk_pvnet_forward), value, probs (gmk_pvnet_evaluate), as CPU tensors"""
    s = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    p, v = fused.trunk(s)
    value, probs = fused(s)
    torch.cuda.synchronize()
    return {"pflat": p.cpu(), "vflat": v.cpu(), "value": value.cpu(), "probs": probs.cpu()}


def _same_bits(a, b, what, rows=None):
    """a and b bit for bit; `rows` names the batch rows that theirs are, for the message"""
    for k in a:
        x, y = a[k].numpy().view(np.uint32), b[k].numpy().view(np.uint32)
        bad = np.argwhere(x != y)
        if rows is not None:
            bad[:, 0] = rows[bad[:, 0]]
        assert bad.size == 0, "%s: %s differs at (row, element) %s" % (what, k, bad[:4].tolist())


@pytest.mark.parametrize("variant", R.WEIGHT_VARIANTS)
def test_input_classes_against_float64(variant):
    """17 positions of each input class (one dense group and one more) under LIMIT x the bound; prints the worst ratio per class."""
    G.init()
    net = R.make_net(variant, seed=5)
    w = R.weights(net)
    fused = FusedPolicyValueNetwork(net)
    worst = {}
    for i, kind in enumerate(R.INPUT_CLASSES):
        x = R.inputs(kind, 17, seed=200 + i)
        ref = R.forward(w, x)
        R.not_vacuous(ref, variant)
        worst[kind] = R.check(ref, _run(fused, x), what="%s / %s" % (variant, kind))
    fused.close()
    print("\nK9 error / tolerance, %s:" % variant)
    for kind, r in worst.items():
        print("  %-13s %s" % (kind, "  ".join("%s %.3f" % kv for kv in r.items())))


_AROUND_GRID = {"cu-1": lambda cu: cu - 1, "cu": lambda cu: cu, "cu+1": lambda cu: cu + 1, "2cu+1": lambda cu: 2 * cu + 1}


def _sample_rows(n, grid):
    """every row of a small batch; of a large one the first and last row of each 16-group boundary, each workgroup's second and third
    positions, and the first and last row"""
    if n <= 64:
        return np.arange(n)
    rows = {0, n - 1}
    for b in range(16, n, 16):
        rows |= {b - 1, b}
    for wg in range(grid):
        rows |= {p for p in (wg + grid, wg + 2 * grid) if p < n}
    return np.array(sorted(rows))


@pytest.mark.parametrize("size", [1, 15, 16, 17, 33, *_AROUND_GRID, 4096])
def test_batch_sizes_against_float64(size, cu_count):
    n = size if isinstance(size, int) else _AROUND_GRID[size](cu_count)
    net = R.make_net("glorot", seed=6)
    fused = FusedPolicyValueNetwork(net)
    half = n // 2
    x = np.concatenate([R.inputs("random", half, seed=n), R.inputs("planes", n - half, seed=n + 1)]) if n > 1 else R.inputs("late", 1, seed=1)
    got = _run(fused, x)
    fused.close()
    rows = _sample_rows(n, min(n, cu_count))
    ref = R.forward(R.weights(net), x[rows])
    R.not_vacuous(ref, "glorot")
    r = R.check(ref, {k: v[rows] for k, v in got.items()}, what="n = %d" % n)
    print("\nn = %d (%d rows in float64): %s" % (n, len(rows), "  ".join("%s %.3f" % kv for kv in r.items())))


def test_rows_are_isolated(cu_count):
    """Bit for bit: alone, in the batch, permuted, shifted by one row of a 16-group, shifted by cu_count (a later iteration of the same
    trunk workgroup) -- both API calls."""
    G.init()
    net = R.make_net("glorot", seed=7)
    fused = FusedPolicyValueNetwork(net)
    n = 2 * cu_count + 21
    x = np.concatenate([R.inputs("random", n // 2, seed=1), R.inputs("planes", n - n // 2, seed=2)])
    full = _run(fused, x)
    for i in (0, 1, 14, 15, 16, 17, cu_count - 1, cu_count, n - 1):
        _same_bits({k: v[i:i + 1] for k, v in full.items()}, _run(fused, x[i:i + 1]), "row %d alone" % i)
    perm = np.random.RandomState(3).permutation(n)
    _same_bits({k: v[perm] for k, v in full.items()}, _run(fused, x[perm]), "permuted")
    for shift in (1, cu_count):
        other = R.inputs("random", shift, seed=9)
        got = _run(fused, np.concatenate([other, x]))
        _same_bits(full, {k: v[shift:] for k, v in got.items()}, "shifted by %d" % shift)
    fused.close()


def _overflow_net():
    """non-negative convolutions without biases and head convolutions x 1e28: 0/1 planes stay finite everywhere, planes x 1e10 overflow
    every head activation to +Inf"""
    net = R.make_net("glorot", seed=8)
    with torch.no_grad():
        for conv in list(net.conv) + [net.policy_conv, net.value_conv]:
            conv.weight.abs_()
            conv.bias.zero_()
        net.policy_conv.weight.mul_(1e28)
        net.value_conv.weight.mul_(1e28)
    return net


@pytest.mark.parametrize("poisoned", [16, 17, 31, 39])
def test_overflowed_neighbour_changes_nothing(poisoned):
    """One position's head activations are +Inf (a diverged net): every other position's outputs keep their bits.  40 positions = dense
    groups 0..15, 16..31, 32..39: the poisoned one is row 0, 1 or 15 of a group, or the batch's last row."""
    G.init()
    fused = FusedPolicyValueNetwork(_overflow_net())
    n = 40
    x = R.inputs("planes", n, seed=4)
    clean = _run(fused, x)
    assert all(torch.isfinite(v).all() for v in clean.values()), "the clean batch must stay finite"
    xp = x.copy()
    xp[poisoned] *= np.float32(1e10)
    got = _run(fused, xp)
    inf = {"pflat": got["pflat"][:, :12], "vflat": got["vflat"][:, :28]}
    for k, v in inf.items():               # the precondition, from gmk_pvnet_forward: +Inf in the poisoned row's leading activations only
        assert (v[poisoned] == float("inf")).all(), k
    for k in ("pflat", "vflat"):
        others = torch.cat([got[k][:poisoned], got[k][poisoned + 1:]])
        assert torch.isfinite(others).all(), k
    keep = np.array([i for i in range(n) if i != poisoned])
    _same_bits({k: v[keep] for k, v in clean.items()}, {k: v[keep] for k, v in got.items()}, "next to row %d" % poisoned, keep)
    fused.close()
