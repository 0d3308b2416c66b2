"""The float64 network reference and its tolerance (tests/pvnet_reference.py) earn their trust on the CPU before the K9 kernels are held to
them: torch's float32 (standing in for a kernel) stays well inside the bound on every input and weight class, and a net with one weight
zeroed lands far outside it.  The feature planes the tests feed are the oracle's."""
import ctypes as C

import numpy as np
import pytest
import torch

import pvnet_reference as R


@pytest.mark.parametrize("variant", R.WEIGHT_VARIANTS)
def test_float32_within_a_quarter_of_the_bound(variant):
    net = R.make_net(variant, seed=1)
    w = R.weights(net)
    worst = {}
    for i, kind in enumerate(R.INPUT_CLASSES):
        x = R.inputs(kind, 17, seed=10 + i)
        ref = R.forward(w, x)
        R.not_vacuous(ref, variant)
        worst[kind] = R.check(ref, R.torch_float32(net, x), R.F32_LIMIT, "%s / %s" % (variant, kind))
    print(variant, {k: round(max(v.values()), 4) for k, v in worst.items()})


def _mutations():
    out = []
    for layer in range(3):
        for tap in ((0, 0), (0, 1)):                   # a corner tap, an edge tap
            out.append(("conv.%d.weight" % layer, tap))
    return out + [("policy_conv.weight", (0, 0)), ("value_conv.weight", (0, 0))]


@pytest.mark.parametrize("name,tap", _mutations())
def test_one_zeroed_weight_is_far_outside_the_bound(name, tap):
    """Zeroing the weight of one tap of one layer that carries the most (|weight| x its input channel's mean activation) moves some output by
    more than 100 x its bound."""
    x = R.inputs("random", 8, seed=3)
    net = R.make_net("glorot", seed=1)
    ref = R.forward(R.weights(net), x)
    assert max(R.ratios(ref, R.torch_float32(net, x)).values()) < R.F32_LIMIT
    with torch.no_grad():
        a = torch.as_tensor(x)                          # the layer's input activations: the weight of a channel that never fires would change nothing
        for conv in net.conv[:int(name[5]) if name.startswith("conv") else 3]:
            a = torch.relu(conv(a))
        wt = net.state_dict()[name]
        plane = wt[:, :, tap[0], tap[1]] * a.mean((0, 2, 3))[None, :]
        o, c = np.unravel_index(int(plane.abs().argmax()), tuple(plane.shape))
        wt[o, c, tap[0], tap[1]] = 0
    r = R.ratios(ref, R.torch_float32(net, x))
    assert max(r.values()) > 100, r


def test_dead_channels_have_closed_forms():
    net = R.make_net("dead", seed=2)
    x = R.inputs("random_x1e4", 5, seed=4)
    ref = R.forward(R.weights(net), x)
    b = net.policy_dense.bias.detach().double()
    np.testing.assert_allclose(ref["probs"], np.broadcast_to(torch.softmax(b, 0).numpy(), (5, 225)), rtol=1e-12)
    np.testing.assert_allclose(ref["value"], np.tanh(float(net.value_out.bias.detach())), rtol=1e-12)
    assert (ref["tol_pflat"] == 0).all() and (ref["tol_vflat"] == 0).all()


def test_bound_scales_with_the_inputs():
    """Scaling the inputs scales the trunk's bound (the biases aside): it is relative to the activations, not one absolute number."""
    net = R.make_net("glorot", seed=1)
    with torch.no_grad():
        for m in net.modules():
            if hasattr(m, "bias") and m.bias is not None:
                m.bias.zero_()
    w = R.weights(net)
    x = R.inputs("random", 3, seed=7)
    a, b = R.forward(w, x), R.forward(w, x * np.float32(1e4))
    np.testing.assert_allclose(b["tol_pflat"], 1e4 * a["tol_pflat"], rtol=1e-4)       # x * 1e4 rounds in float32
    np.testing.assert_allclose(b["pflat"], 1e4 * a["pflat"], rtol=1e-5, atol=1e-9)


def test_planes_are_the_oracles(oracle):
    """planes() restates go_board_encoded_states: the same six planes on positions of every length up to a few moves short of any win."""
    rng = np.random.RandomState(1)
    for k in range(0, 9):
        moves = [int(c) for c in rng.permutation(225)[:k]]
        b = oracle.new_board()
        for mv in moves:
            assert oracle.lib().go_board_apply(C.byref(b), mv, 1) != 0
        out = np.zeros(6 * 225, np.uint8)
        oracle.lib().go_board_encoded_states(C.byref(b), out.ctypes.data)
        np.testing.assert_array_equal(R.planes(moves).reshape(-1), out.astype(np.float32), "after %d moves" % k)


def test_input_classes():
    for kind in R.INPUT_CLASSES:
        x = R.inputs(kind, 6, seed=2)
        assert x.shape == (6, 6, 15, 15) and x.dtype == np.float32
        nz = np.abs(x[x != 0])
        assert nz.size and nz.min() > 1e-30                        # clear of denormals
    stones = R.inputs("full", 4)[:, :2].sum((1, 2, 3))
    assert (stones >= 190).all()
    assert (R.inputs("empty", 2)[:, 2] == 1).all()
