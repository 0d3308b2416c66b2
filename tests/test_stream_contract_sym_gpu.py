"""gmk_pvnet_evaluate_sym ("K22") held to its stream behind a delayed producer, with the harness of tests/test_stream_contract_gpu.py: its
expand kernel, the network's two kernels and its reduce kernel all follow the delayed copy that brings the real input, in all three modes and
both precisions; a launch on another stream would evaluate the decoy."""
import pytest

from gomokuai_amd import lib as G
from stream_harness import Harness
from test_stream_contract_gpu import N, stateless

pytestmark = pytest.mark.gpu

SEED = 777


@pytest.fixture(scope="module")
def H():
    G.init(0)
    return Harness()                                             # (the report of the stream contract is test_stream_contract_gpu.py's to write)


@pytest.fixture(scope="module")
def nets():
    import torch
    from gomokuai_amd.network import FusedPolicyValueNetwork, PolicyValueNetwork
    G.init(0)
    module = PolicyValueNetwork(seed=3).cuda().eval()
    out = {"f32": FusedPolicyValueNetwork(module), "bf16": FusedPolicyValueNetwork(module, precision="bf16")}
    torch.cuda.synchronize()
    yield out
    out["f32"].close()
    out["bf16"].close()


def _case(net, mode, n=17):                                      # ALL: 136 expanded rows, eight dense groups of 16 and half of one
    import torch
    g = torch.Generator(device="cuda").manual_seed(9)
    real = (torch.rand((n, 6, 15, 15), generator=g, device="cuda") > 0.6).float()
    decoy = (torch.rand((n, 6, 15, 15), generator=g, device="cuda") > 0.6).float()
    buf = real.clone()
    outs = (torch.zeros(n, device="cuda"), torch.zeros((n, N), device="cuda"))
    entry = lambda s: G._check(G.load().gmk_pvnet_evaluate_sym(net.h, buf.data_ptr(), n, G.PVNET_SYMMETRIES[mode], SEED, outs[0].data_ptr(), outs[1].data_ptr(), s))
    return buf, decoy, real, outs, entry


def test_a_misplaced_evaluate_sym_is_seen(H, nets):
    buf, decoy, real, outs, entry = _case(nets["f32"], "all")
    H.sensitivity("gmk_pvnet_evaluate_sym", buf, decoy, real, entry, lambda: {"value": outs[0], "probs": outs[1]})


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("mode", ["none", "all", "random"])
def test_evaluate_sym(H, nets, precision, mode):
    buf, decoy, real, outs, entry = _case(nets[precision], mode)
    out = H.check("gmk_pvnet_evaluate_sym[%s, %s]" % (mode, precision), stateless([(buf, decoy, real)], outs, entry))
    import numpy as np
    probs = out["out1"].view(np.float32).reshape(17, N)
    assert abs(probs.sum(axis=1) - 1).max() < 1e-5               # (what came out is a policy, not the fill pattern)
