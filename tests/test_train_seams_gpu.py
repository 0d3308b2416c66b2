"""K11 at its seams (train_kernel.hip: kKSlabPos = 8 positions per split-K slab, kSlabPos = 32 per im2col slab, 128 rows per workgroup, 256
samples per round of the batch sums), on reused handles and on degenerate nets and targets.

Exact where the kernel's header promises it -- every sum runs in an order that depends on the shapes only, a GEMM's k order does not depend on M,
the tile variant is chosen by N alone, max_batch sizes buffers and nothing else -- so a handle's capacity, its history and a row's neighbours
must not change one bit.  Against float64 elsewhere, by the five-order yardstick of tests/train_reference.py (sturdy_ratios), whose cases
tests/test_train_reference.py pins on the CPU."""
import json
import os

import numpy as np
import pytest
import torch

from gomokuai_amd import lib as G
from gomokuai_amd.network import Trainer

import pvnet_reference as R
import train_reference as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
PROFILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "train_parity.json")
METRICS = ("loss", "entropy", "value_loss", "policy_loss")


@pytest.fixture(autouse=True, scope="module")
def _device():
    G.init(0)


def _cuda(batch):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in batch)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _same(a, b):
    a, b = _bits(a), _bits(b)
    return a.shape == b.shape and bool((a == b).all())


def _trainer(params, max_batch):
    """A trainer that holds `params` ({name: array}), fresh moments, step 0."""
    trainer = Trainer(T.make_net(0), max_batch=max_batch)
    state = trainer.state_dict()
    state["params"] = params
    trainer.load_state_dict(state)
    return trainer


def _host(grads):
    return {k: grads[k].cpu().numpy() for k in T.NAMES}


# ---------------- exact: no tolerance ----------------
def _grads_then_step(trainer, state, d, old):
    """grads, then one step from `state` -> {what: array} of everything the two calls give and leave behind"""
    trainer.load_state_dict(state)
    grads, metrics = trainer.grads(*d)
    out = {"grad " + k: a for k, a in _host(grads).items()}
    out["grads metrics"] = metrics.cpu().numpy()
    trainer.load_state_dict(state)
    probs, metrics = trainer.step(*d, lr=2e-3, old_probs=old)
    out["step probs"], out["step metrics"] = probs.cpu().numpy(), metrics.cpu().numpy()
    after, update = trainer.state_dict(), trainer.last_update()
    for k in T.NAMES:
        out["param " + k], out["m " + k], out["v " + k], out["update " + k] = after["params"][k], after["m"][k], after["v"][k], update[k]
    assert after["step"] == state["step"] + 1
    return out


def test_capacity_and_history_independence():
    """A handle for 96 positions (three im2col slabs) that has run 96 foreign samples gives, on the first n samples of a batch, bit for bit what a
    fresh handle for n gives: stale activations, columns and split-K partials are never read."""
    net = T.make_net(11)
    batch, foreign = T.make_batch(96, seed=61), _cuda(T.make_batch(96, seed=62))
    old = torch.from_numpy(T.sparse_old_probs(96)).to(DEV)
    big = Trainer(net, max_batch=96)
    state = big.state_dict()
    assert state["step"] == 0
    big.grads(*foreign)
    big.step(*foreign, lr=2e-3)
    assert not _same(big.params()["w3"], state["params"]["w3"])
    bad = []
    for n in (65, 1, 33, 8, 32, 9):
        d = _cuda(tuple(a[:n] for a in batch))
        got = _grads_then_step(big, state, d, old[:n].contiguous())
        fresh = Trainer(net, max_batch=n)
        want = _grads_then_step(fresh, state, d, old[:n].contiguous())
        fresh.close()
        assert all(np.isfinite(a).all() for a in want.values()) and np.abs(want["grad w1"]).max() > 0 and np.abs(want["update w1"]).max() > 0
        assert want["step metrics"][4] != 0
        bad += [(n, what) for what in want if not _same(got[what], want[what])]
    big.close()
    assert not bad, (sorted({n for n, _ in bad}), bad[:8])


@pytest.fixture(scope="module")
def forward_65():
    """(net, states [65, 6, 15, 15], a handle for 65 positions, its value and probabilities on them)"""
    net = R.make_net("glorot", 2)
    states = T.make_batch(65, seed=71)[0]
    trainer = Trainer(net, max_batch=65)
    value, probs = trainer.forward(torch.from_numpy(states).to(DEV))
    yield net, states, trainer, value.cpu().numpy(), probs.cpu().numpy()
    trainer.close()


ROWS = (0, 31, 32, 63, 64)     # first and last of both full column slabs, the one position of the third


def test_forward_rows_equal_the_position_alone(forward_65):
    net, states, _, value, probs = forward_65
    assert np.isfinite(value).all() and np.isfinite(probs).all()
    for r in ROWS:
        alone = Trainer(net, max_batch=1)
        v, p = alone.forward(torch.from_numpy(states[r:r + 1].copy()).to(DEV))
        v, p = v.cpu().numpy(), p.cpu().numpy()
        alone.close()
        assert _same(v[0], value[r]) and _same(p[0], probs[r]), r


@pytest.mark.parametrize("fill", [float("nan"), 1e30])
def test_forward_rows_ignore_their_neighbours(forward_65, fill):
    """Every other row's planes replaced by NaN or 1e30 (plain data: a GEMM row reads its own row of A): the five rows do not change a bit."""
    _, states, trainer, value, probs = forward_65
    poisoned = np.full_like(states, fill)
    poisoned[list(ROWS)] = states[list(ROWS)]
    v, p = trainer.forward(torch.from_numpy(poisoned).to(DEV))
    v, p = v.cpu().numpy(), p.cpu().numpy()
    for r in ROWS:
        assert _same(v[r], value[r]) and _same(p[r], probs[r]), r
    assert not _same(p[1], probs[1])                                                  # the poison did reach the network (fmaxf(NaN, 0) = 0: no NaN comes out)


def test_step_with_lr_zero():
    net = T.make_net(4)
    d = _cuda(T.make_batch(33, seed=21))
    trainer = Trainer(net, max_batch=33)
    before = trainer.params()
    grads, _ = trainer.grads(*d)
    grads = _host(grads)
    trainer.step(*d, lr=0.0)
    after, update, state = trainer.params(), trainer.last_update(), trainer.state_dict()
    trainer.close()
    assert state["step"] == 1
    for k in T.NAMES:
        assert _same(after[k], before[k]), k
        assert not np.any(update[k]), k
        g = grads[k].astype(np.float64).reshape(before[k].shape) + (0.0 if k in T.BIASES else 1e-4 * before[k].astype(np.float64))
        m, v = 0.1 * g, 0.001 * g * g
        assert np.abs(m).max() > 0
        assert np.abs(state["m"][k].reshape(m.shape) - m).max() <= 1e-6 * np.abs(m).max() + 1e-12, k
        assert np.abs(state["v"][k].reshape(v.shape) - v).max() <= 1e-6 * np.abs(v).max() + 1e-12, k


@pytest.mark.parametrize("kind,zeros", [("dead_layer3", T.DEAD_ZEROS), ("dead_layer2", T.DEAD2_ZEROS), ("saturated_tanh", T.SATURATED_ZEROS)])
def test_exact_zeros(kind, zeros):
    """Nothing passes a layer that never fires (the ReLU masks' > 0) or a saturated tanh (1 - v v): those gradients are 0.0, not small; the rest
    is not zero.  tests/test_train_reference.py holds float64 and torch float32 to the same sets.
    The non-zero tensors are not held to the yardstick here: on these two nets four samples' order moves nothing in torch float32's b_policy_conv
    (four numbers), so its five evaluations are one, and that one is 2.3e-8 with 8 CPU threads and 4.5e-9 with 16; the kernel's 3.9e-8 on the
    saturated net -- what a float32 restatement of its sums in numpy gives too -- is 1.6 of the one and 8.04 of the other."""
    ref = T.case_reference(kind)
    trainer = _trainer(ref["params"], 4)
    grads, metrics = trainer.grads(*_cuda(ref["batch"]))
    grads, metrics = _host(grads), metrics.cpu().numpy().astype(np.float64)
    trainer.close()
    assert sorted(k for k in T.NAMES if not np.any(grads[k])) == sorted(zeros)
    assert all(np.isfinite(grads[k]).all() for k in T.NAMES) and np.isfinite(metrics).all()
    if kind == "saturated_tanh":
        want = float(np.mean((1.0 - ref["batch"][1].astype(np.float64)) ** 2))       # b_out = +30: every value is +1 (|s| >= 20 on the CPU)
        assert abs(metrics[2] - want) <= 1e-6, (metrics[2], want)


# ---------------- against float64, by the five-order yardstick ----------------
def _record(key, ratios):
    try:
        record = json.load(open(PROFILE)) if os.path.exists(PROFILE) else {}
        record[key] = {k: round(v, 4) for k, v in ratios.items()}
        json.dump(record, open(PROFILE, "w"), indent=1, sort_keys=True)
    except OSError:
        pass


def _parity(name, key, loose=()):
    """grads of case `name` on a handle of exactly its size: every tensor within GRAD_LIMIT of the five-order yardstick, every output finite, the
    four loss terms to 1e-5 relative -- those in `loose` to max(1e-5 relative, GRAD_LIMIT x what torch float32 misses float64 by)."""
    ref = T.case_reference(name)
    n = len(ref["batch"][0])
    trainer = _trainer(ref["params"], n)
    grads, metrics = trainer.grads(*_cuda(ref["batch"]))
    grads, metrics = _host(grads), metrics.cpu().numpy().astype(np.float64)
    trainer.close()
    ratios = T.sturdy_ratios(grads, ref["g64"], ref["yard"])
    _record(key, ratios)
    print("%s: worst ratio %.3f (%s), metrics %s against %s (torch float32 %s)" % (name, max(ratios.values()), max(ratios, key=ratios.get), metrics.tolist(),
                                                                                    ref["terms"], ref["terms32"]))
    assert all(np.isfinite(grads[k]).all() for k in T.NAMES) and np.isfinite(metrics).all()
    assert max(ratios.values()) <= T.GRAD_LIMIT, ratios
    for i, term in enumerate(METRICS):
        want = ref["terms"][term]
        tol = 1e-5 * abs(want)
        if term in loose:
            tol = max(tol, T.GRAD_LIMIT * abs(ref["terms32"][term] - want))
        assert abs(metrics[i] - want) <= tol, (term, metrics[i], want, tol)
    return grads


@pytest.mark.parametrize("n", T.SEAM_BATCHES)
def test_gradient_parity_at_the_seams(n):
    """8, 32, 64: a k slab, a column slab and two of them exactly full; 9, 65: one position beyond; 257: the second round of
    train_metrics_kernel's batch sums, a third row of workgroups in the dense GEMMs, 33 k slabs.  Ratios go to profiles/train_parity.json."""
    _parity("seam-%d" % n, "seam-%d" % n)


def test_underflowing_softmax():
    """A logit spread above 200 (float32's exp is 0 below about -104) with every target on the least likely cell: the cross-entropy comes from the
    log-softmax, the entropy from log(p + 1e-10) at p = 0, and nothing is NaN or Inf."""
    _parity("underflow", "degenerate-underflow", loose=("policy_loss", "entropy"))


def test_targets_that_are_not_distributions():
    """An all-zero pi row, a row x 0.5 and a one-hot row: d CE / d logits is p sum(pi) - pi, as autograd has it."""
    grads = _parity("not_distributions", "degenerate-not_distributions")
    assert np.abs(grads["b_policy"]).max() > 0


def test_kl_with_exact_zeros_on_both_sides():
    ref = T.case_reference("underflow")
    old = T.sparse_old_probs(4)
    trainer = _trainer(ref["params"], 4)
    probs, metrics = trainer.step(*_cuda(ref["batch"]), lr=2e-3, old_probs=torch.from_numpy(old).to(DEV))
    probs, metrics, after = probs.cpu().numpy(), metrics.cpu().numpy().astype(np.float64), trainer.params()
    trainer.close()
    want = T.kl_divergence(old, probs)
    print("kl %.6f, float64 from the kernel's probabilities %.6f" % (metrics[4], want))
    assert (probs == 0).any() and (old == 0).any() and ((old > 0) & (probs == 0)).any()
    assert np.isfinite(probs).all() and np.isfinite(metrics).all() and all(np.isfinite(after[k]).all() for k in T.NAMES)
    assert abs(metrics[4] - want) <= 1e-5 * abs(want) + 1e-5, (metrics[4], want)


def test_step_at_257_reports_the_kl_of_its_own_probabilities():
    """Batch 257 through gmk_train_step: the fifth metric (what stops train_step early and moves TrainingLoop's learning rate) is summed over
    two rounds of the batch sums; the returned probabilities are the float64 forward pass's within its bound."""
    net = T.make_net(257)
    ref = T.case_reference("seam-257")
    _, _, old = T.gradients(T.module_arrays(T.make_net(258)), ref["batch"], torch.float32)
    old = np.ascontiguousarray(old.astype(np.float32))
    trainer = Trainer(net, max_batch=257)
    probs, metrics = trainer.step(*_cuda(ref["batch"]), lr=2e-3, old_probs=torch.from_numpy(old).to(DEV))
    probs, metrics = probs.cpu().numpy(), metrics.cpu().numpy().astype(np.float64)
    assert trainer.steps == 1
    trainer.close()
    want = T.kl_divergence(old, probs)
    print("kl %.6f, float64 from the kernel's probabilities %.6f; metrics %s against %s" % (metrics[4], want, metrics.tolist(), ref["terms"]))
    assert want > 1e-3 and abs(metrics[4] - want) <= 1e-5, (metrics[4], want)
    R.check(R.forward(R.weights(net), ref["batch"][0]), {"probs": probs}, R.LIMIT, "gmk_train_step probabilities at 257")
    for i, term in enumerate(METRICS):
        assert abs(metrics[i] - ref["terms"][term]) <= 1e-5 * abs(ref["terms"][term]), (term, metrics[i], ref["terms"][term])
