"""K11 on the GPU: the trainer's kernels (gmk_train_*, gomokuai_amd.network.Trainer, gomokuai_amd.training.TrainingLoop) against the float64
restatement of the training step (tests/train_reference.py), and the export of trained weights into the search's network (K9 / K7)."""
import json
import os

import numpy as np
import pytest
import torch

from gomokuai_amd import lib as G
from gomokuai_amd import selfplay
from gomokuai_amd.network import FusedPolicyValueNetwork, PolicyValueNetwork, Trainer, module_arrays
from gomokuai_amd.training import TrainingLoop

import pvnet_reference as R
import train_reference as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
PROFILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "train_parity.json")


@pytest.fixture(autouse=True, scope="module")
def _device():
    G.init(0)


def _cuda(batch):
    return tuple(torch.from_numpy(a).to(DEV) for a in batch)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _params_equal(a, b):
    return all((_bits(a[k]) == _bits(b[k])).all() for k in T.NAMES)


@pytest.mark.parametrize("n", [1, 2, 31, 33, 130])
def test_gradient_parity(n):
    """Every tensor's gradient within GRAD_LIMIT x the error torch float32 makes on the same batch (+ 1e-7 of the largest gradient); the four
    loss terms to 1e-5 relative.  The worst ratio per tensor goes to profiles/train_parity.json (a record; the limit is not tuned from it)."""
    net = T.make_net(n)
    params, batch = module_arrays(net), T.make_batch(n, seed=10 + n)
    g64, terms, _ = T.gradients(params, batch, torch.float64)
    g32, _, _ = T.gradients(params, batch, torch.float32)
    trainer = Trainer(net, max_batch=n)
    grads, metrics = trainer.grads(*_cuda(batch))
    got = {k: grads[k].cpu().numpy() for k in T.NAMES}
    metrics = metrics.cpu().numpy().astype(np.float64)
    trainer.close()
    ratios = T.gradient_ratios(got, g64, g32)
    try:
        record = json.load(open(PROFILE)) if os.path.exists(PROFILE) else {}
        record[str(n)] = {k: round(v, 4) for k, v in ratios.items()}
        json.dump(record, open(PROFILE, "w"), indent=1, sort_keys=True)
    except OSError:
        pass
    print("batch %d: worst ratio %.3f, metrics %s against %s" % (n, max(ratios.values()), metrics.tolist(), terms))
    assert max(ratios.values()) <= T.GRAD_LIMIT, ratios
    for i, name in enumerate(("loss", "entropy", "value_loss", "policy_loss")):
        assert abs(metrics[i] - terms[name]) <= 1e-5 * abs(terms[name]), (name, metrics[i], terms[name])


@pytest.mark.parametrize("kind", ["early", "full"])
def test_forward_against_fused_and_float64(kind):
    net = R.make_net("glorot", 2)
    states = R.inputs(kind, 37, seed=3)
    ref = R.forward(R.weights(net), states)
    d_states = torch.from_numpy(states).to(DEV)
    trainer, fused = Trainer(net, max_batch=64), FusedPolicyValueNetwork(net.to(DEV))
    tv, tp = trainer.forward(d_states)
    fv, fp = fused(d_states)
    assert float((tv - fv).abs().max()) <= 2e-5 and float((tp - fp).abs().max()) <= 2e-5
    R.check(ref, {"value": tv, "probs": tp}, R.LIMIT, "Trainer.forward " + kind)
    R.check(ref, {"value": fv, "probs": fp}, R.LIMIT, "FusedPolicyValueNetwork " + kind)
    trainer.close()
    fused.close()


def test_update_is_tf1_adam_with_l2():
    """Steps 1 and 2: every parameter's change equals TF1 Adam + L2 computed in float64 from the kernel's float32 gradients, to 1e-6 relative
    with a floor of 1e-12.  The change is taken from the trainer's record of the update it applied (Trainer.last_update): the difference of
    two stored float32 parameters carries half an ulp of the PARAMETER (up to 1.5e-8 here) on a change of lr = 2e-3, 7e-6 of it, so no
    float32 parameter can show its change to 1e-6; the stored parameter must equal w_old - update in float32 exactly instead."""
    net = T.make_net(4)
    batch = T.make_batch(33, seed=21)
    d = _cuda(batch)
    trainer = Trainer(net, max_batch=33)
    m = {k: np.zeros(s) for k, s in G.TRAIN_TENSORS}
    v = {k: np.zeros(s) for k, s in G.TRAIN_TENSORS}
    for t in (1, 2):
        before = trainer.params()
        grads, _ = trainer.grads(*d)
        grads = {k: grads[k].cpu().numpy() for k in T.NAMES}
        trainer.step(*d, lr=2e-3)
        after, update, state = trainer.params(), trainer.last_update(), trainer.state_dict()
        want, m, v = T.adam_step(before, grads, m, v, t, 2e-3)
        assert state["step"] == t
        for k in T.NAMES:
            change = update[k].astype(np.float64)
            want_change = before[k].astype(np.float64) - want[k]
            err = np.abs(change - want_change)
            assert (err <= 1e-6 * np.abs(want_change) + 1e-12).all(), (t, k, float((err / (np.abs(want_change) + 1e-30)).max()))
            assert (_bits(after[k]) == _bits(before[k] - update[k])).all(), (t, k)
            assert np.abs(state["m"][k] - m[k]).max() <= 1e-6 * np.abs(m[k]).max() + 1e-12
            assert np.abs(state["v"][k] - v[k]).max() <= 1e-6 * np.abs(v[k]).max() + 1e-12
            if t == 1:                                   # no L2 term on a bias (they are not zero here), and a weight's first moment shows it
                g = grads[k].astype(np.float64)
                l2 = 0.0 if k in T.BIASES else 1e-4 * before[k]
                assert np.abs(state["m"][k] - 0.1 * (g + l2)).max() <= 1e-6 * np.abs(m[k]).max() + 1e-12
                assert np.abs(before[k]).max() > 0
        # the moments continue from the kernel's float32 values, as the kernel's next step does
        m = {k: state["m"][k].astype(np.float64) for k in T.NAMES}
        v = {k: state["v"][k].astype(np.float64) for k in T.NAMES}
    trainer.close()


def test_reproducible():
    net = T.make_net(5)
    batches = [_cuda(T.make_batch(33, seed=30 + i)) for i in range(3)]
    runs = []
    for _ in range(2):
        trainer = Trainer(net, max_batch=33)
        metrics = [trainer.step(*b, lr=2e-3)[1].cpu().numpy() for b in batches]
        runs.append((trainer.params(), metrics))
        g1, _ = trainer.grads(*batches[0])
        g1 = {k: g1[k].cpu().numpy() for k in T.NAMES}
        g2, _ = trainer.grads(*batches[0])
        assert all((_bits(g1[k]) == _bits(g2[k].cpu().numpy())).all() for k in T.NAMES)
        trainer.close()
    assert _params_equal(runs[0][0], runs[1][0])
    assert all((_bits(a) == _bits(b)).all() for a, b in zip(runs[0][1], runs[1][1]))


EARLY_STOP_LR = 2e-2           # chosen on the CPU: the float64 reference stops after pass 2 with KL 0.30 (bar 0.08); at 1e-2 it stops there with 0.088


def test_train_step_passes_and_kl():
    net = T.make_net(0)
    batch = T.make_batch(64, seed=5)
    d = _cuda(batch)
    trainer = Trainer(net, max_batch=64)
    _, p0 = trainer.forward(d[0])
    loss, entropy, kl, epochs = trainer.train_step(*d, lr=2e-3, kl_target=0.02, num_epoches=5)
    assert epochs == 5 and trainer.steps == 5
    twin = Trainer(net, max_batch=64)                    # the same four updates, then the probabilities the fifth pass saw
    twin.train_step(*d, lr=2e-3, kl_target=0.02, num_epoches=4)
    _, p4 = twin.forward(d[0])
    want = T.kl_divergence(p0.cpu().numpy(), p4.cpu().numpy())
    print("kl %.6f, float64 from forward %.6f; float64 reference run %s" % (kl, want, T.RefTrainer(net).train_step(batch, 2e-3, 0.02, 5)))
    assert abs(kl - want) <= 1e-5 and kl <= 4 * 0.02
    trainer.close()
    twin.close()
    ref_epochs = T.RefTrainer(net).train_step(batch, EARLY_STOP_LR, 0.02, 5)[3]
    assert ref_epochs < 5
    trainer = Trainer(net, max_batch=64)
    _, _, kl, epochs = trainer.train_step(*d, lr=EARLY_STOP_LR, kl_target=0.02, num_epoches=5)
    assert abs(epochs - ref_epochs) <= 1 and (epochs == 5 or kl > 0.08)
    trainer.close()


def test_learning():
    """64 golden tuples, 30 steps at lr 2e-3: the loss ends below its start and below the float64 run's loss at step 15."""
    ref = T.learning_curve("float64")
    d = _cuda(T.learning_batch())
    trainer = Trainer(T.make_net(0), max_batch=T.LEARN_BATCH)
    losses = [float(trainer.step(*d, lr=T.LEARN_LR)[1][0]) for _ in range(T.LEARN_STEPS)]
    _, metrics = trainer.grads(*d)
    last = float(metrics[0])
    trainer.close()
    print("loss %.5f -> %.5f; float64 %.5f -> %.5f (step 15) -> %.5f" % (losses[0], last, ref[0], ref[T.LEARN_MID], ref[-1]))
    assert abs(losses[0] - ref[0]) <= 1e-5 * ref[0]
    assert last < losses[0] and last < ref[T.LEARN_MID]


def _search(network, n=8, playouts=16):
    moves, lens, _ = G.synth_boards(n, 0)
    lens = np.minimum(lens, 4).astype(np.int32)
    planes = G.moves_to_planes(moves, lens)
    last = np.stack([moves[np.arange(n), lens - 1], moves[np.arange(n), lens - 2]], 1).astype(np.int16)
    tree = G.AlphaZeroMCTS(n, node_capacity=playouts * 225 + 1)
    tree.set_roots(planes, last)
    with torch.no_grad():
        tree.search(network, playouts)
    stats = tree.root_stats()
    tree.close()
    return stats


def test_export_equals_a_fresh_network():
    net = T.make_net(6).to(DEV)
    fused = FusedPolicyValueNetwork(net)
    trainer = Trainer(net, max_batch=33)
    d = _cuda(T.make_batch(33, seed=40))
    for _ in range(3):
        trainer.step(*d, lr=2e-3)
    states = torch.from_numpy(R.inputs("late", 19, seed=1)).to(DEV)
    v_old, p_old = fused(states)
    fused.load_from(trainer)
    fresh = FusedPolicyValueNetwork(trainer.sync_to(PolicyValueNetwork().to(DEV)))
    v_new, p_new = fused(states)
    v_fresh, p_fresh = fresh(states)
    assert not torch.equal(p_new, p_old)
    assert torch.equal(v_new.view(torch.int32), v_fresh.view(torch.int32)) and torch.equal(p_new.view(torch.int32), p_fresh.view(torch.int32))
    a, b = _search(fused), _search(fresh)
    assert (a["visits"] == b["visits"]).all() and (a["root_visits"] == b["root_visits"]).all()
    for x in (trainer, fused, fresh):
        x.close()


def _golden_records():
    """The six recorded games of tests/golden/reference_tuples.npz as GameRecords with visit counts (the tuples' probabilities x 1000)."""
    d = np.load(T.GOLDEN)
    n = len(d["lens"])
    visits = np.zeros((n, 225, 225), np.int16)
    ply = np.zeros(n, np.int64)
    for g, probs in zip(d["game"], d["probs"]):
        visits[g, ply[g]] = np.round(probs * 1000).astype(np.int16)
        ply[g] += 1
    return selfplay.GameRecords(torch.from_numpy(d["moves"]).to(DEV), torch.from_numpy(d["lens"]).to(DEV), torch.from_numpy(d["winner"]).to(DEV),
                                torch.from_numpy(visits).to(DEV))


def test_training_loop():
    net = T.make_net(7).to(DEV)
    fused, trainer = FusedPolicyValueNetwork(net), Trainer(net, max_batch=32)
    replay = selfplay.ReplayBuffer(4096, max_games=16, seed=3)
    replay.extend(_golden_records())
    assert replay.status()[0] == 0 and len(replay) > 32
    states = torch.from_numpy(R.inputs("late", 5, seed=2)).to(DEV)
    loop = TrainingLoop(replay, trainer, fused, batch_size=32, lr=2e-3, kl_target=0.02, num_epoches=5, export_every=2)
    outputs, mult = [fused(states)[1].clone()], 1.0
    for i in range(4):
        rec = loop.step()
        assert rec["lr"] == 2e-3 * mult and rec["exported"] == (i % 2 == 1) and 1 <= rec["epochs"] <= 5 and np.isfinite(rec["loss"])
        if rec["kl"] > 0.04 and mult > 0.1:              # train.py:73-77
            mult /= 1.5
        elif rec["kl"] < 0.01 and mult < 10:
            mult *= 1.5
        assert loop.lr_multiplier == mult
        outputs.append(fused(states)[1].clone())
    changed = [not torch.equal(a, b) for a, b in zip(outputs, outputs[1:])]
    assert changed == [False, True, False, True]
    assert trainer.steps == sum(r["epochs"] for r in loop.history) and loop.total_steps == 4
    assert loop.run(1) and len(loop.history) == 5
    for x in (trainer, fused, replay):
        x.close()


def test_state_dict_round_trip():
    net = T.make_net(8)
    d = _cuda(T.make_batch(9, seed=50))
    a = Trainer(net, max_batch=9)
    a.step(*d, lr=2e-3)
    b = Trainer(T.make_net(9), max_batch=9)
    b.load_state_dict(a.state_dict())
    a.step(*d, lr=2e-3)
    b.step(*d, lr=2e-3)
    assert _params_equal(a.params(), b.params()) and a.steps == b.steps == 2
    with pytest.raises(ValueError):
        a.forward(torch.zeros((10, 6, 15, 15), device=DEV))
    a.close()
    b.close()
