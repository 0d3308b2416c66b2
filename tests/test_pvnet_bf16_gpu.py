""""K9 in bf16" on the GPU: FusedPolicyValueNetwork(precision="bf16") -- gmk_pvnet_forward (pflat / vflat) and gmk_pvnet_evaluate (value /
probs) with pvnet_bf16_trunk_kernel in the trunk's place -- held to tests/pvnet_bf16_reference.py: bit for bit on the exact-integer net, under
LIMIT x the bf16 bound on every input class and weight variant and at batch sizes around the dense kernel's groups of 16 and the trunk's grid
(grid = min(n, cu_count); the bf16 trunk takes P = 1 position per workgroup at a time, workgroup w takes positions w, w + grid, ...).  Then
the float32 battery's row isolation bit for bit, precision switching, gmk_train_export into a bf16 handle, and a search."""
import numpy as np
import pytest
import torch

import pvnet_bf16_reference as B
import pvnet_reference as R
from gomokuai_amd import lib as G
from gomokuai_amd.network import FusedPolicyValueNetwork, PolicyValueNetwork, Trainer

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
    for k in a:
        x, y = a[k].numpy().view(np.uint32), b[k].numpy().view(np.uint32)
        bad = np.argwhere(x != y)
        if rows is not None:
            bad[:, 0] = rows[bad[:, 0]]
        assert bad.size == 0, "%s: %s differs at (row, element) %s" % (what, k, bad[:4].tolist())


@pytest.fixture(scope="module")
def exact_cases(cu_count):
    """per seed: the exact net, 2 cu + 1 positions of 0/1 planes and their float64 pflat / vflat (premise asserted inside), computed once"""
    n = 2 * cu_count + 1
    cases = []
    for seed in B.EXACT_SEEDS:
        net = B.exact_net(seed)
        x = B.exact_inputs(n, seed)
        cases.append((net, x, B.exact_forward(net, x)))
    return cases


@pytest.mark.parametrize("size", [1, 17, "2cu+1"])
def test_exact_net_bit_for_bit(size, exact_cases, cu_count):
    """Integer activations that bf16 holds exactly: no rounding of the contract changes anything, every float32 sum is exact in any order, so
    the float64 pflat / vflat are the one right answer -- a wrong tap, channel, lane map or a single wrong weight shows as a wrong integer."""
    n = size if isinstance(size, int) else 2 * cu_count + 1
    for net, x, ref in exact_cases:
        fused = FusedPolicyValueNetwork(net, precision="bf16")
        assert fused.precision == "bf16"
        s = torch.from_numpy(np.ascontiguousarray(x[:n])).cuda()
        p, v = fused.trunk(s)
        torch.cuda.synchronize()
        fused.close()
        for name, got in (("pflat", p), ("vflat", v)):
            g = got.cpu().numpy().astype(np.float64)
            bad = np.argwhere(g != ref[name][:n])
            assert bad.size == 0, "%s differs at (row, element) %s: got %s, float64 %s" % (
                name, bad[:4].tolist(), g[tuple(bad[:4].T)].tolist(), ref[name][:n][tuple(bad[:4].T)].tolist())


@pytest.mark.parametrize("variant", R.WEIGHT_VARIANTS)
def test_input_classes_against_float64(variant):
    """17 positions of each input class under LIMIT x the bf16 bound; prints the worst ratio per class."""
    G.init()
    net = R.make_net(variant, seed=5)
    w = R.weights(net)
    fused = FusedPolicyValueNetwork(net, precision="bf16")
    worst = {}
    for i, kind in enumerate(R.INPUT_CLASSES):
        x = R.inputs(kind, 17, seed=200 + i)
        ref = B.forward(w, x)
        R.not_vacuous(ref, variant)
        r = R.ratios(ref, _run(fused, x))
        print("K9 bf16 error / tolerance, %s / %-13s %s" % (variant, kind, "  ".join("%s %.3f" % kv for kv in r.items())))
        worst[kind] = r
    fused.close()
    for kind, r in worst.items():
        bad = {k: v for k, v in r.items() if not v <= R.LIMIT}
        assert not bad, "%s / %s: error / tolerance above %.2f: %s" % (variant, kind, R.LIMIT, bad)


_AROUND_GRID = {"cu-1": lambda cu: cu - 1, "cu": lambda cu: cu, "cu+1": lambda cu: cu + 1, "2cu+1": lambda cu: 2 * cu + 1}


def _sample_rows(n, grid):
    if n <= 64:
        return np.arange(n)
    rows = {0, n - 1}
    for b in range(16, n, 16):
        rows |= {b - 1, b}
    for wg in range(grid):
        rows |= {p for p in (wg + grid, wg + 2 * grid) if p < n}
    return np.array(sorted(rows))


@pytest.mark.parametrize("size", [1, 2, 15, 16, 17, 33, *_AROUND_GRID])
def test_batch_sizes_against_float64(size, cu_count):
    """P = 1 position per workgroup: P - 1 = 0 is the empty batch (below), P and P + 1 are 1 and 2, P cu + 1 is cu + 1."""
    n = size if isinstance(size, int) else _AROUND_GRID[size](cu_count)
    net = R.make_net("glorot", seed=6)
    fused = FusedPolicyValueNetwork(net, precision="bf16")
    half = n // 2
    x = np.concatenate([R.inputs("random", half, seed=n), R.inputs("planes", n - half, seed=n + 1)]) if n > 1 else R.inputs("late", 1, seed=1)
    got = _run(fused, x)
    fused.close()
    rows = _sample_rows(n, min(n, cu_count))
    ref = B.forward(R.weights(net), x[rows])
    R.not_vacuous(ref, "glorot")
    r = R.ratios(ref, {k: v[rows] for k, v in got.items()})
    print("\nn = %d (%d rows in float64): %s" % (n, len(rows), "  ".join("%s %.3f" % kv for kv in r.items())))
    R.check(ref, {k: v[rows] for k, v in got.items()}, what="n = %d" % n)


def test_empty_batch_is_a_no_op():
    G.init()
    fused = FusedPolicyValueNetwork(R.make_net("glorot", seed=6), precision="bf16")
    got = _run(fused, np.zeros((0, 6, 15, 15), np.float32))
    assert got["pflat"].shape == (0, 900) and got["probs"].shape == (0, 225)
    fused.close()


def test_rows_are_isolated(cu_count):
    """Bit for bit: alone, in the batch, permuted, shifted by one row of a 16-group, shifted by cu_count (a later iteration of the same
    trunk workgroup) -- both API calls."""
    G.init()
    net = R.make_net("glorot", seed=7)
    fused = FusedPolicyValueNetwork(net, precision="bf16")
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
    _same_bits(full, _run(fused, x), "the same batch again")
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
    """One position's head activations are +Inf (a diverged net): every other position's outputs keep their bits."""
    G.init()
    fused = FusedPolicyValueNetwork(_overflow_net(), precision="bf16")
    n = 40
    x = R.inputs("planes", n, seed=4)
    clean = _run(fused, x)
    assert all(torch.isfinite(v).all() for v in clean.values()), "the clean batch must stay finite"
    xp = x.copy()
    xp[poisoned] *= np.float32(1e10)
    got = _run(fused, xp)
    inf = {"pflat": got["pflat"][:, :12], "vflat": got["vflat"][:, :28]}
    for k, v in inf.items():
        assert (v[poisoned] == float("inf")).all(), k
    for k in ("pflat", "vflat"):
        others = torch.cat([got[k][:poisoned], got[k][poisoned + 1:]])
        assert torch.isfinite(others).all(), k
    keep = np.array([i for i in range(n) if i != poisoned])
    _same_bits({k: v[keep] for k, v in clean.items()}, {k: v[keep] for k, v in got.items()}, "next to row %d" % poisoned, keep)
    fused.close()


def test_precision_switching_returns_the_float32_bits():
    """f32 -> bf16 -> f32 on one handle: the float32 bits of a handle that was never switched; and bf16 differs from float32 (it ran)."""
    G.init()
    net = R.make_net("glorot", seed=9)
    x = np.concatenate([R.inputs("random", 20, seed=1), R.inputs("planes", 21, seed=2)])
    fresh = FusedPolicyValueNetwork(net)
    want = _run(fresh, x)
    fresh.close()
    fused = FusedPolicyValueNetwork(net)
    assert fused.precision == "f32"
    _same_bits(want, _run(fused, x), "before any switch")
    fused.set_precision("bf16")
    assert fused.precision == "bf16"
    low = _run(fused, x)
    assert not torch.equal(low["pflat"], want["pflat"])
    made_bf16 = FusedPolicyValueNetwork(net, precision="bf16")
    _same_bits(low, _run(made_bf16, x), "switched to bf16 against made in bf16")
    made_bf16.close()
    fused.set_precision("f32")
    assert fused.precision == "f32"
    _same_bits(want, _run(fused, x), "back in f32")
    with pytest.raises(ValueError):
        fused.set_precision("fp8")
    assert G.load().gmk_pvnet_set_precision(fused.h, 2) == -3 and fused.precision == "f32"
    fused.close()


def test_export_refreshes_the_bf16_weights():
    """Trainer.step + export into a bf16 handle (the device's repack and rounding) equals, bit for bit, a fresh bf16 handle made from
    trainer.params() (the host's packers) -- and differs from the handle before the export."""
    G.init()
    net = R.make_net("glorot", seed=10).cuda()
    fused = FusedPolicyValueNetwork(net, precision="bf16")
    trainer = Trainer(net, max_batch=33)
    rng = np.random.RandomState(5)
    states = torch.from_numpy(R.inputs("late", 33, seed=40)).cuda()
    values = torch.from_numpy(rng.choice([-1.0, 0.0, 1.0], 33).astype(np.float32)).cuda()
    pi = torch.from_numpy(rng.dirichlet(np.full(225, 0.05), 33).astype(np.float32)).cuda()
    for _ in range(3):
        trainer.step(states, values, pi, lr=2e-3)
    x = R.inputs("late", 19, seed=1)
    old = _run(fused, x)
    fused.load_from(trainer)
    assert fused.precision == "bf16"
    new = _run(fused, x)
    fresh = FusedPolicyValueNetwork(trainer.sync_to(PolicyValueNetwork().cuda()), precision="bf16")
    _same_bits(new, _run(fresh, x), "exported against fresh")
    assert not torch.equal(new["pflat"], old["pflat"])
    for h in (trainer, fused, fresh):
        h.close()


def test_search_with_the_bf16_network():
    """64 games x 32 playouts of AlphaZeroMCTS.search: completes, visits exactly `playouts` per game, repeats bit for bit."""
    G.init()
    n, playouts = 64, 32
    fused = FusedPolicyValueNetwork(R.make_net("glorot", seed=11), precision="bf16")
    moves, lens, _ = G.synth_boards(n, 0)
    lens = np.minimum(lens, 4).astype(np.int32)
    planes = G.moves_to_planes(moves, lens)
    last = np.stack([moves[np.arange(n), lens - 1], moves[np.arange(n), lens - 2]], 1).astype(np.int16)
    runs = []
    for _ in range(2):
        tree = G.AlphaZeroMCTS(n, node_capacity=playouts * 225 + 1)
        tree.set_roots(planes, last)
        with torch.no_grad():
            tree.search(fused, playouts)
        runs.append(tree.root_stats())
        tree.close()
    fused.close()
    a, b = runs
    assert (a["root_visits"] == playouts).all() and (a["status"] == 0).all()
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
