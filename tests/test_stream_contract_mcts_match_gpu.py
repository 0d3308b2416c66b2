"""The two calls a device-resident match makes of a K3 handle (gmk_mcts_root_choice, gmk_mcts_step_device) held to their stream behind a
delayed producer, with the harness and the positions of tests/test_stream_contract_gpu.py: the root choice stands straight behind the search
that makes the visit counts it reads, the step straight behind the verdicts that steer it -- a launch that left the stream would find
roots without children, or verdicts that say REFUSED."""
import numpy as np
import pytest

from gomokuai_amd import lib as G
from stream_harness import Call, Harness, Scenario
from test_stream_contract_gpu import COUNTER, N, positions

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def H():
    G.init(0)
    return Harness()                                             # (the report of the stream contract is test_stream_contract_gpu.py's to write)


@pytest.mark.parametrize("fresh", [False, True], ids=["reuse", "fresh"])
def test_k3_root_choice_step_device(H, fresh):
    """K3: run -> root_choice (with and without the rows) -> verdicts -> step_device -> run, then the root statistics"""
    import torch
    n, playouts = 6, 64
    _, lens, planes, last = positions(n, 10, first_board=40)

    def make():
        tree = G.BatchedMCTS(n, playouts_capacity=4 * playouts, seed=11)
        tree.set_option(G.OPT_NOISE_SAMPLER, COUNTER)
        tree.set_roots(planes, last[:, 0], first_game_id=70)
        cells, bare = torch.full((n,), -1, dtype=torch.int16, device="cuda"), torch.full((n,), -1, dtype=torch.int16, device="cuda")
        rows, verdict = torch.zeros((n, N), dtype=torch.int16, device="cuda"), torch.ones(n, dtype=torch.int32, device="cuda")
        host = {}
        calls = [Call(lambda s: tree.run(playouts, s)),
                 Call(lambda s: tree.root_choice(cells, rows, s)),
                 Call(lambda s: tree.root_choice(bare, None, s)),
                 Call(lambda s: verdict.zero_()),                 # every game MOVED: produced on the stream as the referee would
                 Call(lambda s: tree.step_device(cells, verdict, fresh, s)),
                 Call(lambda s: tree.run(playouts, s)),
                 Call(lambda s: host.update({"stats%d" % i: a for i, a in enumerate(tree.root_stats())}), waits=True)]
        return Scenario(calls, lambda: dict(host, cells=cells, bare=bare, rows=rows), tree.close)
    out = H.check("K3 run/root_choice x 2/step_device/run [%s]" % ("fresh" if fresh else "reuse"), make)
    cells = out["cells"].view(np.int16)
    assert (cells >= 0).all() and out["rows"].any() and (out["bare"].view(np.int16) == cells).all()      # (ahead of the search: childless roots, -1)
    # every game followed its move: one stone more on the root board is one child fewer to visit, and the second search's playouts are the root's
    visits, root_visits, status = out["stats0"].view(np.uint32).reshape(n, N), out["stats2"].view(np.uint32), out["stats4"].view(np.int32)
    assert not status.any() and (visits[np.arange(n), cells] == 0).all()
    assert (root_visits >= playouts).all() and ((root_visits == playouts) | (not fresh)).all()
