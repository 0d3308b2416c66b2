"""The float64 restatement of "K9 in bf16" and its bound (tests/pvnet_bf16_reference.py) earn their trust on the CPU before the kernel is held
to them: the calibration of C_B by the file's own rule, wrong implementations that must land outside the bound, the exact-integer net's
premise, and the packers' rounding (gmk_bf16_round_host, which needs no GPU) against torch's."""
import ctypes as C

import numpy as np
import pytest
import torch

import pvnet_bf16_reference as B
import pvnet_reference as R
from gomokuai_amd import lib as G


@pytest.fixture(scope="module")
def calibration_cases():
    """(variant, kind, weights, inputs, stand-in outputs) of every weight variant x input class, 17 positions each: computed once"""
    cases = []
    for variant in R.WEIGHT_VARIANTS:
        w = R.weights(R.make_net(variant, seed=5))
        for i, kind in enumerate(R.INPUT_CLASSES):
            x = R.inputs(kind, 17, seed=200 + i)
            cases.append((variant, kind, w, x, B.standin(w, x)))
    return cases


def _worst(cases, c_b):
    worst = {}
    for variant, kind, w, x, got in cases:
        ref = B.forward(w, x, c_b)
        R.not_vacuous(ref, variant)
        r = R.ratios(ref, got)
        k = max(r, key=r.get)
        if r[k] >= worst.get(variant, (-1.0,))[0]:
            worst[variant] = (r[k], k, kind)
    return worst


def test_c_b_is_the_smallest_power_of_two_that_keeps_the_standin_within_a_quarter(calibration_cases):
    """The rule of pvnet_bf16_reference: at C_B every variant x class is within F32_LIMIT, at C_B / 2 some is not.  Prints what the
    module's docstring records."""
    assert B.C_B == 2.0 ** round(np.log2(B.C_B))
    at = _worst(calibration_cases, B.C_B)
    below = _worst(calibration_cases, B.C_B / 2)
    print("\nstand-in / bound at C_B = %g: %s\n               at C_B = %g: %s" % (B.C_B, at, B.C_B / 2, below))
    assert max(v[0] for v in at.values()) <= R.F32_LIMIT, at
    assert max(v[0] for v in below.values()) > R.F32_LIMIT, below


def _zero_tap(w): w["conv.2.weight"][:, :, 2, 1] = 0
def _zero_tap_layer1(w): w["conv.0.weight"][:, :, 0, 0] = 0
def _zero_input_channel(w): w["conv.1.weight"][:, 7] = 0
def _swap_output_channels(w): w["conv.2.weight"][[3, 4]] = w["conv.2.weight"][[4, 3]]
def _swap_head_rows(w): w["policy_conv.weight"][[0, 1]] = w["policy_conv.weight"][[1, 0]]


@pytest.mark.parametrize("mutate", [_zero_tap, _zero_tap_layer1, _zero_input_channel, _swap_output_channels, _swap_head_rows], ids=lambda f: f.__name__[1:])
def test_wrong_implementations_fail_the_check(mutate):
    """The mistakes a kernel of this shape can make -- a tap's address offset, a channel group, the register-to-channel map -- are outside
    the bound at the chosen C_B.  Prints by how much."""
    w = R.weights(R.make_net("glorot", seed=5))
    x = R.inputs("late", 17, seed=3)
    ref = B.forward(w, x)
    assert max(R.ratios(ref, B.standin(w, x)).values()) <= R.F32_LIMIT
    got = B.standin(w, x, mutate)
    with pytest.raises(AssertionError):
        R.check(ref, got, what=mutate.__name__)
    print("\n%s, error / bound: %s" % (mutate.__name__[1:], {k: round(v, 2) for k, v in R.ratios(ref, got).items()}))


def test_one_zeroed_weight_is_below_bf16_resolution():
    """NOT detectable, on record: one zeroed 3x3 weight of layer 3 moves the outputs by less than the bf16 roundings of the activations that feed
    the same sums, so the bound (rightly) admits it.  The exact-integer net is what catches a single wrong weight."""
    w = R.weights(R.make_net("glorot", seed=5))
    x = R.inputs("late", 17, seed=3)
    def one(w): w["conv.2.weight"][5, 9, 1, 1] = 0
    r = R.ratios(B.forward(w, x), B.standin(w, x, one))
    print("\none zeroed weight, error / bound:", r)
    assert max(r.values()) <= R.LIMIT, r


@pytest.mark.parametrize("seed", B.EXACT_SEEDS)
def test_exact_net_premise_and_sensitivity(seed):
    """Every activation of the exact net is an integer that bf16 holds, about half of them positive, the heads fire (asserted inside
    exact_forward) -- so the stand-in, roundings included, gives the float64 answer bit for bit, and ONE flipped weight does not."""
    net = B.exact_net(seed)
    x = B.exact_inputs(9, seed)
    ref = B.exact_forward(net, x)
    w = R.weights(net)
    got = B.standin(w, x)
    for k in ("pflat", "vflat"):
        assert (got[k].astype(np.float64) == ref[k]).all(), k
    c = int(np.argmax(w["policy_conv.weight"].abs().sum(0).reshape(-1).numpy() > 0))       # a layer-3 channel the policy head reads
    def one(w): w["conv.2.weight"][c, 9, 1, 1] += 1
    bad = B.standin(w, x, one)
    assert (bad["pflat"].astype(np.float64) != ref["pflat"]).any()


def _round_host(values):
    src = np.ascontiguousarray(values, np.float32)
    dst = np.zeros(src.size, np.uint16)
    assert G.load().gmk_bf16_round_host(src.ctypes.data, src.size, dst.ctypes.data) == 0
    return dst


def _torch_bits(values):
    return torch.from_numpy(np.ascontiguousarray(values, np.float32)).bfloat16().view(torch.int16).numpy().view(np.uint16)


def test_round_host_is_torchs_conversion():
    rng = np.random.RandomState(0)
    bits = lambda u: np.array(u, np.uint32).view(np.float32)
    groups = {
        "random": (rng.standard_normal(4096) * np.exp(rng.uniform(-40, 40, 4096))).astype(np.float32),
        "random bits": rng.randint(0, 2 ** 32, 4096, dtype=np.uint64).astype(np.uint32).view(np.float32),
        # exact ties (low half 0x8000) above an even and above an odd bf16, both signs, and their neighbours
        "ties": bits([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001, 0x00008000, 0x00018000]),
        "denormals": bits([0x00000001, 0x00007FFF, 0x00008001, 0x00010000, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x007F8000, 0x007F7FFF]),
        "zeros and infinities": bits([0x00000000, 0x80000000, 0x7F800000, 0xFF800000]),
        # the largest bf16 is 0x7F7F; from 0x7F7F8000 up a finite float rounds to Inf
        "rounds up to Inf": bits([0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF, 0xFF7F7FFF, 0xFF7F8000, 0xFF7FFFFF]),
    }
    for name, v in groups.items():
        keep = ~np.isnan(v)
        np.testing.assert_array_equal(_round_host(v[keep]), _torch_bits(v[keep]), name)
    assert _round_host(bits([0x7F7F8000]))[0] == 0x7F80 and _round_host(bits([0xFF7FFFFF]))[0] == 0xFF80
    assert _round_host(bits([0x3F808000]))[0] == 0x3F80 and _round_host(bits([0x3F818000]))[0] == 0x3F82
    nans = bits([0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF, 0xFF80FFFF])
    got, want = _round_host(nans), _torch_bits(nans)
    assert ((got & 0x7F80) == 0x7F80).all() and ((got & 0x007F) != 0).all(), "NaN stays NaN"
    assert ((want & 0x7F80) == 0x7F80).all() and ((want & 0x007F) != 0).all()          # torch's are NaNs too; which NaN is each implementation's own
    assert (got == 0x7FC0).all(), "the packers' NaN is the positive quiet NaN"
    assert G.load().gmk_bf16_round_host(None, 0, None) == 0
