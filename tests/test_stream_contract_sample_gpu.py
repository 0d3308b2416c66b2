"""The two sampled K7 entries (gmk_az_root_choice_sampled, gmk_az_advance_sampled) held to their stream behind a delayed producer, with the
harness and the K7 + K9 chain of tests/test_stream_contract_gpu.py: the sampled call stands straight behind the search that makes the visit
counts it draws from, so a launch that left the stream would read roots without children."""
import numpy as np
import pytest

from gomokuai_amd import lib as G
from stream_harness import Call, Harness, Scenario
from test_stream_contract_gpu import COUNTER, N, _evaluate, dev, flat, positions

pytestmark = pytest.mark.gpu

SAMPLE = (225, 1, 777, 20)                                       # every ply is drawn, keyed like the chain's root noise


@pytest.fixture(scope="module")
def H():
    G.init(0)
    return Harness()                                             # (the report of the stream contract is test_stream_contract_gpu.py's to write)


@pytest.fixture(scope="module")
def net():
    import torch
    from gomokuai_amd.network import FusedPolicyValueNetwork, PolicyValueNetwork
    G.init(0)
    fused = FusedPolicyValueNetwork(PolicyValueNetwork(seed=3).cuda().eval())
    torch.cuda.synchronize()
    yield fused
    fused.close()


def _chain(net, entry, solver):
    import torch
    n, cap = 6, 4096
    moves, lens, planes, last = positions(n, 12)
    options = dict(vcf_depth=4, vcf_budget=64, proof=True) if solver else {}

    def make():
        tree = G.AlphaZeroMCTS(n, node_capacity=cap, c_puct=5.0, **options)
        tree.set_option(G.OPT_NOISE_SAMPLER, COUNTER)
        tree.set_roots(planes, last)
        value, probs = torch.zeros(n, device="cuda"), torch.zeros((n, N), device="cuda")
        for live in range(n, 0, -1):                             # the first call of a batch size waits for its stream: made here
            _evaluate(net, tree.states, live, value, probs, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        value.zero_(); probs.zero_()
        cells, rows = torch.full((n,), -1, dtype=torch.int16, device="cuda"), torch.zeros((n, N), dtype=torch.int16, device="cuda")
        rec = (dev(moves), torch.zeros((n, N, N), dtype=torch.int16, device="cuda"), dev(lens), torch.zeros(n, dtype=torch.int8, device="cuda"))
        host, calls = {}, []

        def playouts(k):
            for _ in range(k):
                calls.append(Call(lambda s: tree.select(s)))
                calls.append(Call(lambda s: _evaluate(net, tree.states, tree.live, value, probs, s)))
                calls.append(Call(lambda s: tree.expand(value[:tree.live], probs[:tree.live], s)))
        playouts(12)
        if entry == "root_choice":
            calls.append(Call(lambda s: tree.root_choice(cells, rows, s, sample=SAMPLE)))
            playouts(2)
            calls.append(Call(lambda s: host.update(flat("a", tree.root_stats())), waits=True))
        else:
            calls.append(Call(lambda s: host.update(unfinished=tree.advance(rec[0], rec[1], rec[2], rec[3], True, s, sample=SAMPLE)), waits=True))
            calls.append(Call(lambda s: tree.add_root_noise(0.3, 0.25, seed=777, first_game_id=20, stream=s)))
            playouts(6)
            calls.append(Call(lambda s: host.update(unfinished2=tree.advance(rec[0], rec[1], rec[2], rec[3], True, s, sample=SAMPLE)), waits=True))
            calls.append(Call(lambda s: host.update(flat("a", tree.root_stats())), waits=True))
        outputs = lambda: dict(host, value=value, probs=probs, cells=cells, rows=rows, **{"rec%d" % i: t for i, t in enumerate(rec)})
        return Scenario(calls, outputs, tree.close)
    return make, lens


@pytest.mark.parametrize("solver", [False, True], ids=["plain", "solver-proofs"])
@pytest.mark.parametrize("entry", ["root_choice", "advance"])
def test_sampled_entry_behind_its_search(H, net, entry, solver):
    make, lens = _chain(net, entry, solver)
    out = H.check("K7 sampled %s [%s]" % (entry, "solver-proofs" if solver else "plain"), make)
    if entry == "root_choice":
        cells = out["cells"].view(np.int16)
        assert (cells >= 0).all() and out["rows"].any()          # (a launch ahead of the search would have found childless roots: -1)
    else:
        assert (out["rec2"].view(np.int32) >= lens + 1).all() and out["rec1"].any()
