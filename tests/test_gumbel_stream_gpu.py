"""K21's stream-taking entries held to their stream behind a delayed producer, with tests/stream_harness.py as it is and the chains of
tests/test_stream_contract_gpu.py: gmk_az_select under Gumbel, gmk_az_root_choice_gumbel and gmk_az_advance_gumbel stand in a K7 + K9 chain
straight behind the search whose statistics they read, and the three _target entries behind the copy that brings their records."""
import numpy as np
import pytest

from gomokuai_amd import lib as G
from stream_harness import Call, Harness, Scenario
from test_stream_contract_gpu import COUNTER, N, _evaluate, _records, dev, flat, positions, stateless

pytestmark = pytest.mark.gpu

GUMBEL = (8, 12, 50.0, 1.0, 777, 20)


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


def _chain(net, entry):
    import torch
    n, cap = 6, 4096
    moves, lens, planes, last = positions(n, 12)

    def make():
        tree = G.AlphaZeroMCTS(n, node_capacity=cap, c_puct=5.0, gumbel=GUMBEL)
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
                calls.append(Call(lambda s: tree.select(s)))     # (the Gumbel select: its set-up and every root step read what the expand before it wrote)
                calls.append(Call(lambda s: _evaluate(net, tree.states, tree.live, value, probs, s)))
                calls.append(Call(lambda s: tree.expand(value[:tree.live], probs[:tree.live], s)))
        playouts(12)
        if entry == "root_choice":
            calls.append(Call(lambda s: tree.root_choice(cells, rows, s, gumbel=True)))
            playouts(2)                                          # (a second set-up, behind the choice that voided the first)
            calls.append(Call(lambda s: host.update(flat("a", tree.root_stats())), waits=True))
        else:
            calls.append(Call(lambda s: host.update(unfinished=tree.advance(rec[0], rec[1], rec[2], rec[3], True, s, gumbel=True)), waits=True))
            playouts(6)
            calls.append(Call(lambda s: host.update(unfinished2=tree.advance(rec[0], rec[1], rec[2], rec[3], True, s, gumbel=True)), waits=True))
            calls.append(Call(lambda s: host.update(flat("a", tree.root_stats())), waits=True))
        outputs = lambda: dict(host, value=value, probs=probs, cells=cells, rows=rows, **{"rec%d" % i: t for i, t in enumerate(rec)})
        return Scenario(calls, outputs, tree.close)
    return make, lens


@pytest.mark.parametrize("entry", ["root_choice", "advance"])
def test_gumbel_entry_behind_its_search(H, net, entry):
    make, lens = _chain(net, entry)
    out = H.check("K7 Gumbel %s" % entry, make)
    if entry == "root_choice":
        cells = out["cells"].view(np.int16)
        assert (cells >= 0).all() and out["rows"].any()          # (a launch ahead of the search would have found childless roots: -1 and zeros)
    else:
        assert (out["rec2"].view(np.int32) >= lens + 1).all() and out["rec1"].any()


def test_target_entries(H):
    """gmk_samples_from_records_target, gmk_samples_from_packed_target and gmk_replay_sample_target in GMK_TARGET_POLICY, as one chain behind the
    copy that brings the records: 3 games, 8 samples, augment on (the chain of test_records_wire_and_samples with the policy target)."""
    import torch
    n, lens = 3, [40, 7, 225]
    real, decoy = _records(n, 15, lens), _records(n, 16, lens)
    rec = [t.clone() for t in real]
    n_bytes = 5 * n + sum(lens) * 451
    offsets, packed, status = torch.zeros(n + 1, dtype=torch.int64, device="cuda"), torch.zeros(n_bytes + 3, dtype=torch.uint8, device="cuda"), torch.zeros(3, dtype=torch.int32, device="cuda")
    s_game = torch.tensor([0, 0, 1, 1, 2, 2, 2, 2], dtype=torch.int32, device="cuda")
    s_move = torch.tensor([0, 39, 3, 6, 0, 100, 223, 224], dtype=torch.int32, device="cuda")
    S = 8 * 8
    samples = [(torch.zeros((S, 6, N), dtype=torch.uint8, device="cuda"), torch.zeros(S, device="cuda"), torch.zeros((S, N), device="cuda")) for _ in range(2)]
    batch = 32
    drawn = (torch.zeros((batch, 6, N), device="cuda"), torch.zeros(batch, device="cuda"), torch.zeros((batch, N), device="cuda"), torch.zeros((batch, 3), dtype=torch.int64, device="cuda"))
    replay = G.ReplayHandle(4096, 16, seed=3)
    p = lambda t: t.data_ptr()
    entries = [Call(lambda s: G.records_scan(p(rec[1]), n, p(offsets), s)),
               Call(lambda s: G.records_pack(p(rec[0]), p(rec[1]), p(rec[2]), p(rec[3]), n, p(offsets), p(packed), n_bytes, p(status[:1]), s)),
               Call(lambda s: G.samples_from_records(p(rec[0]), p(rec[1]), p(rec[3]), p(rec[2]), p(s_game), p(s_move), 8, 1, *[p(t) for t in samples[0]], s, target="policy")),
               Call(lambda s: G.samples_from_packed(p(packed), n, p(offsets), p(s_game), p(s_move), 8, 1, *[p(t) for t in samples[1]], s, target="policy")),
               Call(lambda s: replay.reset(s)),
               Call(lambda s: replay.append(p(rec[0]), p(rec[1]), p(rec[2]), p(rec[3]), n, 0, p(status[1:2]), s)),
               Call(lambda s: replay.sample(batch, 0, True, True, p(drawn[0]), p(drawn[1]), p(drawn[2]), p(drawn[3]), p(status[2:]), s, target="policy"))]
    finals = list(samples[0]) + list(samples[1]) + list(drawn) + [status]
    try:
        out = H.check("gmk_*_target (policy)", stateless([(b, d, r) for b, d, r in zip(rec, decoy, real)], finals, entries, extra=[offsets, packed]))
        assert not out["out%d" % (len(finals) - 1)].view(np.int32).any()         # the three status words
    finally:
        replay.close()
