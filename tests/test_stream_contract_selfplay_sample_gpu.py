"""The two stream-taking sampled entries of K3 and K6 / K8 (gmk_mcts_advance_sampled, gmk_trad_root_choice_sampled) held to their stream behind
a delayed producer, with the harness and the chains of tests/test_stream_contract_gpu.py: the sampled call stands straight behind the search
that makes the visit counts it draws from, so a launch that left the stream would read roots without children.
gmk_selfplay_run_sampled and gmk_trad_selfplay_run_sampled are synchronous like their unsampled forms (they return with the games played and
the stream drained); what the harness can hold them to -- record buffers produced on the stream -- is test_stream_contract_gpu.py's
test_k3_selfplay_run / test_trad_selfplay_run, whose host code they share, and is repeated here with the first plies drawn."""
import numpy as np
import pytest

from gomokuai_amd import lib as G
from stream_harness import Call, Harness, Scenario
from test_stream_contract_gpu import COUNTER, N, TRAD, _k3_records, dev, fill, flat, positions

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def H():
    G.init(0)
    return Harness()                                             # (the report of the stream contract is test_stream_contract_gpu.py's to write)


@pytest.mark.parametrize("reuse", [False, True], ids=["fresh", "reuse"])
def test_k3_run_advance_sampled(H, reuse):
    """K3: run -> advance(sample=) for three plies on the stream, every ply drawn, then the root statistics"""
    n, playouts = 6, 64
    moves, lens, planes, last = positions(n, 10, first_board=40)

    def make():
        tree = G.BatchedMCTS(n, playouts_capacity=4 * playouts, seed=11)
        tree.set_option(G.OPT_NOISE_SAMPLER, COUNTER)
        tree.set_roots(planes, last[:, 0], first_game_id=70)
        rec = _k3_records(n)
        rec[0].copy_(dev(moves)); rec[2].copy_(dev(lens))
        ptrs = [t.data_ptr() for t in rec]
        host, calls = {}, []
        for _ in range(3):
            calls.append(Call(lambda s: tree.run(playouts, s)))
            calls.append(Call(lambda s: tree.advance(*ptrs, reuse, s, sample=(225, 1))))
        calls.append(Call(lambda s: tree.run(playouts, s)))
        calls.append(Call(lambda s: host.update({"stats%d" % i: a for i, a in enumerate(tree.root_stats())}), waits=True))
        return Scenario(calls, lambda: dict(host, **{"rec%d" % i: t for i, t in enumerate(rec)}), tree.close)
    out = H.check("K3 run/advance_sampled x 3 [%s]" % ("reuse" if reuse else "fresh"), make)
    assert (out["rec2"].view(np.int32) >= lens + 1).all() and out["rec1"].any()      # (a step ahead of its search finds no child and plays nothing)


@pytest.mark.parametrize("kind", sorted(TRAD))
def test_k6_k8_root_choice_sampled(H, kind):
    """K6 / K6 + RAVE / K8: root_choice(sample=) straight behind the run that makes the root's children, with and without the rows, and the
    step that follows its cells"""
    import torch
    n, playouts = 4, 200
    moves, lens, _, _ = positions(n, 8, first_board=20)
    sample = (225, 1, 9, 50)

    def make():
        tree = TRAD[kind](n)
        tree.set_option(G.OPT_NOISE_SAMPLER, COUNTER)
        tree.set_positions(moves, lens)
        cells, bare = torch.full((n,), -1, dtype=torch.int16, device="cuda"), torch.full((n,), -1, dtype=torch.int16, device="cuda")
        rows, verdict = torch.zeros((n, N), dtype=torch.int16, device="cuda"), torch.ones(n, dtype=torch.int32, device="cuda")
        host = {}
        calls = [Call(lambda s: tree.run(playouts, s)),
                 Call(lambda s: tree.root_choice(cells, rows, s, sample=sample)),
                 Call(lambda s: tree.root_choice(bare, None, s, sample=sample)),
                 Call(lambda s: verdict.zero_()),                 # every game MOVED: produced on the stream as the referee would
                 Call(lambda s: tree.step_device(cells, verdict, False, s)),
                 Call(lambda s: tree.run(playouts, s)),
                 Call(lambda s: host.update(flat("b", tree.root_stats())), waits=True)]
        return Scenario(calls, lambda: dict(host, cells=cells, bare=bare, rows=rows), tree.close)
    out = H.check("K6/K8 run/root_choice_sampled x 2/step_device/run [%s]" % kind, make)
    cells = out["cells"].view(np.int16)
    assert (cells >= 0).all() and out["rows"].any() and (out["bare"].view(np.int16) == cells).all()      # (ahead of the search: childless roots, -1)
    assert not out["b.status"].any() and out["b.root_visits"].view(np.uint32).min() >= playouts


@pytest.mark.parametrize("lockstep", [0, 1], ids=["persistent", "lockstep"])
def test_k3_selfplay_run_sampled(H, lockstep):
    """gmk_selfplay_run_sampled on the stream, its record buffers zeroed by a delayed fill there (one call that waits: one segment)"""
    n, playouts = 4, 20

    def make():
        tree = G.BatchedMCTS(2, playouts_capacity=3 * playouts, seed=5)
        tree.set_option(G.OPT_NOISE_SAMPLER, COUNTER)
        tree.set_option(G.OPT_LOCKSTEP, lockstep)
        rec = _k3_records(n)[:4]
        fill(rec, 0x77)
        host = {}
        calls = [Call(lambda s: fill(rec, 0)),
                 Call(lambda s: host.update(steps=tree.selfplay_run(n, 900, playouts, *[t.data_ptr() for t in rec], reuse_subtree=True, root_noise=(0.3, 0.25), stream=s,
                                                                    sample=(6, 1))), waits=True)]
        return Scenario(calls, lambda: dict(host, **{"rec%d" % i: t for i, t in enumerate(rec)}), tree.close)
    out = H.check("gmk_selfplay_run_sampled [%s]" % ("lockstep" if lockstep else "persistent"), make)
    assert (out["rec2"].view(np.int32) > 0).all()


@pytest.mark.parametrize("persistent", [True, False], ids=["persistent", "lockstep"])
def test_trad_selfplay_run_sampled(H, persistent):
    n, playouts = 4, 20

    def make():
        tree = G.TraditionalMCTS(2, node_capacity=1 << 14)
        tree.set_option(G.OPT_NOISE_SAMPLER, COUNTER)
        rec = _k3_records(n)[:4]
        fill(rec, 0x77)
        host = {}
        ptrs = [t.data_ptr() for t in rec]
        calls = [Call(lambda s: fill(rec, 0)),
                 Call(lambda s: host.update(run=np.array(tree.selfplay_run(n, 900, playouts, *ptrs, reuse_subtree=True, root_noise=(0.3, 0.25), seed=17, stream=s,
                                                                           persistent=persistent, sample=(6, 1)), dtype=np.int64)), waits=True)]
        return Scenario(calls, lambda: dict(host, **{"rec%d" % i: t for i, t in enumerate(rec)}), tree.close)
    out = H.check("gmk_trad_selfplay_run_sampled [%s]" % ("persistent" if persistent else "lockstep"), make)
    assert (out["rec2"].view(np.int32) > 0).all()
