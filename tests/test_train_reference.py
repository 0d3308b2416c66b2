"""The float64 training-step reference (tests/train_reference.py) earns its trust on the CPU before the trainer's kernels are held to it."""
import numpy as np
import pytest
import torch

import train_reference as T


def _numpy_loss(params, batch):
    """The loss of model_tf.py:77-89 written out by hand in numpy float64, one sample at a time."""
    p = {k: np.asarray(v, np.float64) for k, v in params.items()}
    states, values, pi = (np.asarray(a, np.float64) for a in batch)

    def conv3(x, w, b):                                    # x [cin,15,15], w [cout,cin,3,3] -> relu [cout,15,15]
        xp = np.zeros((x.shape[0], 17, 17))
        xp[:, 1:16, 1:16] = x
        out = np.zeros((w.shape[0], 15, 15))
        for ky in range(3):
            for kx in range(3):
                out += np.einsum("oc,chw->ohw", w[:, :, ky, kx], xp[:, ky:ky + 15, kx:kx + 15])
        return np.maximum(out + b[:, None, None], 0)

    value_terms, policy_terms, entropy_terms = [], [], []
    for i in range(len(states)):
        x = states[i]
        for l in (1, 2, 3):
            x = conv3(x, p["w%d" % l], p["b%d" % l])
        x = x.reshape(128, 225)
        pf = np.maximum(p["w_policy_conv"] @ x + p["b_policy_conv"][:, None], 0).T.reshape(-1)          # (pixel, channel)
        vf = np.maximum(p["w_value_conv"] @ x + p["b_value_conv"][:, None], 0).T.reshape(-1)
        logits = p["w_policy"] @ pf + p["b_policy"]
        hidden = np.maximum(p["w_hidden"] @ vf + p["b_hidden"], 0)
        value = np.tanh(p["w_out"] @ hidden + p["b_out"][0])
        z = logits - logits.max()
        log_softmax = z - np.log(np.exp(z).sum())
        probs = np.exp(log_softmax)
        value_terms.append((value - values[i]) ** 2)
        policy_terms.append(-(pi[i] * log_softmax).sum())
        entropy_terms.append(-(probs * np.log(probs + 1e-10)).sum())
    l2 = 1e-4 * sum((p[k] ** 2).sum() / 2 for k in T.NAMES if k not in T.BIASES)
    return np.mean(value_terms) + np.mean(policy_terms) + l2, np.mean(entropy_terms), np.mean(value_terms), np.mean(policy_terms)


def test_float64_loss_equals_a_numpy_restatement():
    from gomokuai_amd.network import module_arrays
    params = module_arrays(T.make_net(1))
    batch = T.make_batch(3, seed=2)
    _, terms, _ = T.gradients(params, batch)
    loss, entropy, value_loss, policy_loss = _numpy_loss(params, batch)
    for name, want in (("loss", loss), ("entropy", entropy), ("value_loss", value_loss), ("policy_loss", policy_loss)):
        assert abs(terms[name] - want) <= 1e-12 * max(1.0, abs(want)), (name, terms[name], want)
    assert len(T.BIASES) == 8 and policy_loss > 0 and value_loss > 0


def test_batches_hold_the_edge_cases():
    s, v, p = T.make_batch(33, seed=1)
    assert s.shape == (33, 6, 15, 15) and s.dtype == np.float32 and v.shape == (33,) and p.shape == (33, 225)
    rim = s[0, 0] + s[0, 1]
    assert rim[0, 0] == rim[0, 14] == rim[14, 0] == rim[14, 14] == 1 and rim[0, 7] == rim[7, 0] == rim[7, 14] == rim[14, 7] == 1
    assert (p[0] == 1).sum() == 1 and (p[0] == 0).sum() == 224 and (p[2] == 1).sum() == 1          # one-hot rows: exact zeros
    assert s[1, 2].sum() == 225 and s[2, 2].sum() == 1                                              # the empty board, the full board
    assert np.abs(p.sum(1) - 1).max() < 1e-5


def test_float32_yardstick_and_criterion():
    from gomokuai_amd.network import module_arrays
    params = module_arrays(T.make_net(0))
    batch = T.make_batch(31, seed=4)
    g64, _, _ = T.gradients(params, batch, torch.float64)
    g32, _, _ = T.gradients(params, batch, torch.float32)
    ratios = T.gradient_ratios(g32, g64, g32)
    assert max(ratios.values()) <= 1.0, ratios                         # LIMIT 1 by construction
    assert all(np.abs(g64[k]).max() > 0 for k in T.NAMES)
    broken = dict(g64)
    broken["w2"] = g64["w2"] * 0.5                                     # half a gradient is far outside, however many ReLUs float32 flipped
    assert T.gradient_ratios(broken, g64, g32)["w2"] > 2 * T.GRAD_LIMIT


def test_float32_learns_with_room():
    """torch float32 on the CPU meets the learning criterion using at most a quarter of its room."""
    c64, c32 = T.learning_curve("float64"), T.learning_curve("float32")
    assert c64[-1] < c64[T.LEARN_MID] < c64[0]
    assert c32[-1] < c32[0]
    assert T.learning_margin(c32[0], c32[-1]) <= 0.25, (c32[-1], c64[-1], c64[T.LEARN_MID])


def test_adam_reproduces_a_scalar_worked_by_hand():
    """w = 1 (a weight: L2 applies), data gradients 0.5 then -0.25, lr 0.1; and a bias with the same gradients (no L2)."""
    zero = {k: np.zeros(shape) for k, shape in T.G.TRAIN_TENSORS}
    params = {k: a.copy() for k, a in zero.items()}
    params["w_out"][0], params["b_out"][0] = 1.0, 1.0
    grads = {k: a.copy() for k, a in zero.items()}
    grads["w_out"][0], grads["b_out"][0] = 0.5, 0.5
    p1, m1, v1 = T.adam_step(params, grads, zero, zero, 1, 0.1)
    # step 1: g = 0.5 + 1e-4 = 0.5001; m = 0.05001; v = 0.5001^2 / 1000; lr_1 = 0.1 sqrt(0.001) / 0.1 = sqrt(0.001)
    g = 0.5001
    w1 = 1.0 - np.sqrt(0.001) * (0.1 * g) / (np.sqrt(0.001 * g * g) + 1e-8)
    assert abs(p1["w_out"][0] - w1) < 1e-15 and abs(w1 - 0.9) < 1e-6       # Adam's first step is lr, whatever the gradient
    b1 = 1.0 - np.sqrt(0.001) * 0.05 / (np.sqrt(0.001 * 0.25) + 1e-8)
    assert abs(p1["b_out"][0] - b1) < 1e-15
    grads["w_out"][0], grads["b_out"][0] = -0.25, -0.25
    p2, m2, v2 = T.adam_step(p1, grads, m1, v1, 2, 0.1)
    g2 = -0.25 + 1e-4 * w1
    m = 0.9 * 0.1 * g + 0.1 * g2
    v = 0.999 * 0.001 * g * g + 0.001 * g2 * g2
    lr2 = 0.1 * np.sqrt(1 - 0.999 ** 2) / (1 - 0.81)
    assert abs(p2["w_out"][0] - (w1 - lr2 * m / (np.sqrt(v) + 1e-8))) < 1e-15
    mb = 0.9 * 0.05 - 0.1 * 0.25
    vb = 0.999 * 0.00025 + 0.001 * 0.0625
    assert abs(p2["b_out"][0] - (b1 - lr2 * mb / (np.sqrt(vb) + 1e-8))) < 1e-15
    assert p2["w1"].max() == 0 and p2["w1"].min() == 0


# ---------------- the five-order yardstick and the cases of tests/test_train_seams_gpu.py ----------------
PARITY_CASES = ["seam-%d" % n for n in T.SEAM_BATCHES] + ["underflow", "not_distributions"]


@pytest.mark.parametrize("name", PARITY_CASES)
def test_five_order_yardstick_holds_float32_itself(name):
    """torch float32 in a sixth and a seventh sample order, neither among the yardstick's five, stays within GRAD_LIMIT / 4 of it at every case the
    kernel is held to GRAD_LIMIT on (largest seen with 1, 8 and 16 threads: 1.35); half a w2 gradient is still far outside.  A case that misses this gets another seed."""
    ref = T.case_reference(name)
    n = len(ref["batch"][0])
    orders = [T.sample_order(n, i) for i in range(T.YARD_ORDERS + 2)]
    if n > 4:                                              # 4! = 24 orders: two seeded draws may coincide there
        assert len({tuple(o) for o in orders}) == len(orders)
    for i in (T.YARD_ORDERS, T.YARD_ORDERS + 1):
        g32, _, _ = T.gradients(ref["params"], T.reordered(ref["batch"], orders[i]), torch.float32)
        ratios = T.sturdy_ratios(g32, ref["g64"], ref["yard"])
        print("%s order %d: worst %.3f (%s)" % (name, i, max(ratios.values()), max(ratios, key=ratios.get)))
        assert max(ratios.values()) <= T.GRAD_LIMIT / 4, ratios
    broken = dict(ref["g64"])
    broken["w2"] = ref["g64"]["w2"] * 0.5
    assert T.sturdy_ratios(broken, ref["g64"], ref["yard"])["w2"] > 2 * T.GRAD_LIMIT
    assert all(y > 0 for y in ref["yard"].values())


def test_five_order_yardstick_is_the_largest_of_five_and_exact_where_float32_is():
    ref = T.case_reference("dead_layer3")
    errs = T.float32_errors(ref["params"], ref["batch"], ref["g64"])
    g32, _, _ = T.gradients(ref["params"], ref["batch"], torch.float32)
    for k in T.NAMES:
        assert len(errs[k]) == T.YARD_ORDERS and ref["yard"][k] == max(errs[k])
        assert errs[k][0] == float(np.abs(g32[k] - ref["g64"][k]).max())             # order 0 is the batch as given: gradient_ratios' yardstick
    assert max(T.sturdy_ratios(ref["g64"], ref["g64"], ref["yard"]).values()) == 0.0
    off = dict(ref["g64"])
    off["w1"] = ref["g64"]["w1"] + 1e-30                                               # all five yardsticks are 0 there: nothing but 0 passes
    assert ref["yard"]["w1"] == 0.0 and T.sturdy_ratios(off, ref["g64"], ref["yard"])["w1"] == float("inf")


def _pre_activations(params, states):
    with torch.no_grad():
        logits, s = T.forward({k: torch.tensor(params[k], dtype=torch.float64) for k in T.NAMES}, torch.tensor(states, dtype=torch.float64))
    return logits.numpy(), s.numpy()


def test_degenerate_cases_are_what_they_claim():
    """The premises of the exact-zero and degenerate GPU tests, in float64 and in torch float32, without a GPU."""
    for kind, zeros in (("dead_layer3", T.DEAD_ZEROS), ("dead_layer2", T.DEAD2_ZEROS), ("saturated_tanh", T.SATURATED_ZEROS)):
        ref = T.case_reference(kind)
        g32, _, _ = T.gradients(ref["params"], ref["batch"], torch.float32)
        for g in (ref["g64"], g32):
            assert sorted(k for k in T.NAMES if not np.any(g[k])) == sorted(zeros), kind
    sat = T.case_reference("saturated_tanh")
    _, s = _pre_activations(sat["params"], sat["batch"][0])
    assert (np.abs(s) >= 20).all(), s
    want = float(np.mean((np.sign(s) - sat["batch"][1].astype(np.float64)) ** 2))
    assert abs(sat["terms"]["value_loss"] - want) <= 1e-12 and abs(sat["terms32"]["value_loss"] - want) <= 1e-6

    under = T.case_reference("underflow")
    logits, _ = _pre_activations(under["params"], under["batch"][0])
    assert ((logits.max(1) - logits.min(1)) >= 200).all(), logits.max(1) - logits.min(1)
    pi = under["batch"][2]
    assert ((pi == 1).sum(1) == 1).all() and ((pi == 0).sum(1) == 224).all() and (pi.argmax(1) == logits.argmin(1)).all()
    assert (under["probs"].astype(np.float32) == 0).mean() > 0.25                      # float32 holds exact zeros where float64 holds 1e-60
    assert all(np.isfinite(v) for v in under["terms"].values()) and all(np.isfinite(v) for v in under["terms32"].values())

    pi = T.case_reference("not_distributions")["batch"][2]
    sums = pi.sum(1)
    assert sums[0] == 0 and abs(sums[1] - 0.5) < 1e-5 and sums[2] == 1 and (pi[2] == 1).sum() == 1 and abs(sums[3] - 1) < 1e-5

    old = T.sparse_old_probs(4)
    assert old.dtype == np.float32 and old.shape == (4, 225) and ((old == 0).sum(1) > 0).all() and ((old > 0).sum(1) > 0).all()
    assert T.kl_divergence(old, under["probs"]) > 1.0                                  # mass where the underflowing net has none: a KL that matters
