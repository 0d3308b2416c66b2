"""K13 on the GPU: the device merge of root tables (gmk_mcts_ensemble_merge / gmk_trad_ensemble_merge) and the layers on top of it
(gomokuai_amd/ensemble.py, interface.EnsembleAgent).  The replicas' searches are held to the CPU oracle one by one under their game ids, the
merge to the numpy restatement of tests/ensemble_reference.py and to gmk_ensemble_merge_host: everything bit for bit."""
import ctypes as C

import numpy as np
import pytest

from gomokuai_amd import lib as G
from gomokuai_amd.ensemble import EnsembleSearch
from ensemble_reference import assert_same, numpy_merge

pytestmark = pytest.mark.gpu

SEED = G.DEFAULT_SEED


@pytest.fixture(scope="module")
def torch():
    import torch
    G.init()
    return torch


def _openings(n, plies, first):
    moves, lens, _ = G.synth_boards(n, 0, first_board=first)
    return [[int(c) for c in moves[g, :min(int(lens[g]), plies)]] for g in range(n)]


def _clustered(n, plies, first):
    moves, lens, _ = G.synth_boards(n, 1, first_board=first)
    return [[int(c) for c in moves[g, :min(int(lens[g]), plies)]] for g in range(n)]


def _nearly_full(empty):
    """A board with `empty` free cells on which neither colour has five (two colour classes that cannot line up five), black first."""
    rng = np.random.RandomState(5)
    cls = lambda c: ((c % 15) // 2 + c // 15) % 2
    b = list(rng.permutation([c for c in range(225) if cls(c) == 0]))
    w = list(rng.permutation([c for c in range(225) if cls(c) == 1]))
    seq = []
    while b or w:
        if b:
            seq.append(int(b.pop()))
        if w:
            seq.append(int(w.pop()))
    return seq[:225 - empty]


def _board(O, moves):
    b = O.new_board()
    for mv in moves:
        O.lib().go_board_apply(C.byref(b), int(mv), 1)
    return b


def _tables(rows):
    """[(visits, values, root_visits, root_value)] per replica -> the arrays of the merge"""
    return (np.array([r[0] for r in rows], np.uint32), np.array([r[1] for r in rows], np.float32),
            np.array([r[2] for r in rows], np.uint32), np.array([r[3] for r in rows], np.float32))


def _as_reference(m):
    return {"visits": m["visits"], "values": m["values"], "cells": m["cell"], "root_visits": m["root_visits"], "root_value": m["root_value"], "status": m["status"]}


def _device_merge(torch, tree, group):
    """every output of the merge call, as host arrays in the reference's shape"""
    E, dev = tree.n // group, torch.device("cuda")
    out = {"visits": torch.empty((E, 225), dtype=torch.int32, device=dev), "values": torch.empty((E, 225), dtype=torch.float32, device=dev),
           "cells": torch.empty(E, dtype=torch.int16, device=dev), "cells_per_game": torch.empty(tree.n, dtype=torch.int16, device=dev),
           "root_visits": torch.empty(E, dtype=torch.int32, device=dev), "root_value": torch.empty(E, dtype=torch.float32, device=dev),
           "status": torch.empty(E, dtype=torch.int32, device=dev)}
    tree.ensemble_merge(group, **out)
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in out.items()}
    host["visits"], host["root_visits"] = host["visits"].view(np.uint32), host["root_visits"].view(np.uint32)
    return host


def test_k3_against_the_oracle(torch, oracle):
    O, R, P, first = oracle, 5, 48, 1000
    positions = [[], _openings(1, 6, 21)[0], _nearly_full(2)]
    assert [len(p) for p in positions] == [0, 6, 223]
    es = EnsembleSearch("random", R, seed=SEED, first_game_id=first, playouts_capacity=P)
    es.set_positions(positions)
    es.search(P)
    got = es.merged()
    rows = []
    for k, pos in enumerate(positions):
        for r in range(R):
            m = O.MCTS(P, 5.0, 5, SEED, first + k * R + r)
            m.eval_state(_board(O, pos))
            v, q, _ = m.root_children()
            rows.append((v, q, m.root_visits, m.root_value))
    assert_same(_as_reference(got), numpy_merge(R, *_tables(rows)), "against the oracle's replicas:")
    assert not got["status"].any() and (got["root_visits"] == R * P).all()
    assert np.count_nonzero(got["visits"][2]) <= 2 and got["visits"][2].sum() >= R * (P - 1)
    # ... and the host merge of what the handle itself reports (K3's root statistics carry the visits and the root pair)
    visits, root_q, root_n, _, _ = es.tree.root_stats()
    host = G.ensemble_merge_host(R, visits, np.zeros(visits.shape, np.float32), root_n, root_q)
    for k in ("visits", "cells", "root_visits", "status"):
        np.testing.assert_array_equal(host[k], _as_reference(got)[k], k)
    np.testing.assert_array_equal(host["root_value"].view(np.uint32), got["root_value"].view(np.uint32))
    es.close()


def test_group_sizes(torch):
    """group = 1 is the identity on the handle's own tables; group = 70 -- more replicas than lanes, two ensembles -- is the host merge."""
    group, P = 70, 16
    positions = _openings(2, 4, 90)
    es = EnsembleSearch("random", group, first_game_id=5, playouts_capacity=P)
    es.set_positions(positions)
    es.search(P)
    visits, root_q, root_n, _, _ = es.tree.root_stats()
    zeros = np.zeros(visits.shape, np.float32)
    got = _device_merge(torch, es.tree, group)
    host = G.ensemble_merge_host(group, visits, zeros, root_n, root_q)
    for k in ("visits", "cells", "root_visits", "status"):
        np.testing.assert_array_equal(got[k], host[k], k)
    np.testing.assert_array_equal(got["root_value"].view(np.uint32), host["root_value"].view(np.uint32))
    np.testing.assert_array_equal(got["cells_per_game"], np.repeat(host["cells"], group))
    assert (got["root_visits"] == group * P).all() and not got["status"].any()
    one = _device_merge(torch, es.tree, 1)
    np.testing.assert_array_equal(one["visits"], visits)
    np.testing.assert_array_equal(one["root_visits"], root_n)
    np.testing.assert_array_equal(one["cells"], np.where(visits.max(axis=1) > 0, visits.argmax(axis=1), -1))
    np.testing.assert_array_equal(one["cells_per_game"], one["cells"])
    np.testing.assert_array_equal(one["root_value"].view(np.uint32), G.ensemble_merge_host(1, visits, zeros, root_n, root_q)["root_value"].view(np.uint32))
    # a value goes through one rounding to 2^-24 / N and one to float32 (|V| <= 1: half a step of 2^-24 at most)
    assert np.abs(one["root_value"].astype(np.float64) - root_q.astype(np.float64)).max() <= 2.0 ** -25 / P + 2.0 ** -25
    es.close()


def test_k6_against_the_oracle(torch, oracle):
    O, R, P, first, seed = oracle, 4, 64, 50, 4242
    positions = [p if len(p) >= 2 else [112, 113] for p in _clustered(2, 14, 900)]
    es = EnsembleSearch("traditional", R, seed=seed, first_game_id=first, root_noise=(0.05, 0.25), playouts_capacity=P)
    es.set_positions(positions)
    es.search(P)
    got = es.merged()
    rows = []
    for k, pos in enumerate(positions):
        for r in range(R):
            o = O.TraditionalMCTS(5.0)
            o.set_noise(0.05, 0.25, seed, first + k * R + r, sampler=1)
            o.run(pos, 1)                                # AddNoise does nothing on a root without children: one playout expands it,
            o.run(pos, P - 1)                            # the second runPlayouts draws the noise
            v, q, _, _ = o.root_children()
            rows.append((v, q, o.root_visits, o.root_value))
    assert_same(_as_reference(got), numpy_merge(R, *_tables(rows)), "against the oracle's replicas:")
    stats = es.tree.root_stats()
    assert not got["status"].any() and (stats["priors"][0] != stats["priors"][1]).any()          # every replica drew its own noise
    assert_same(_as_reference(got), G.ensemble_merge_host(R, stats["visits"], stats["values"], stats["root_visits"], stats["root_value"]), "against the host merge:")
    es.close()
    # without noise the replicas are copies of one tree
    t = G.TraditionalMCTS(2 * R, node_capacity=P * 225 + 1)
    t.set_positions([positions[0]] * R + [positions[1]] * R)
    t.run(P)
    plain, stats = _device_merge(torch, t, R), t.root_stats()
    np.testing.assert_array_equal(plain["visits"], R * stats["visits"][[0, R]])
    np.testing.assert_array_equal(plain["root_visits"], R * stats["root_visits"][[0, R]])
    t.close()


def test_k8_against_the_oracle(torch, oracle):
    O, R, P, first = oracle, 3, 64, 300
    positions = [p if len(p) >= 2 else [112, 113] for p in _clustered(2, 10, 40)]
    es = EnsembleSearch("poolrave", R, seed=SEED, first_game_id=first, playouts_capacity=P)
    es.set_positions(positions)
    es.search(P)
    got = es.merged()
    rows = []
    for k, pos in enumerate(positions):
        for r in range(R):
            o = O.PoolRAVEMCTS(2.0, 0.0, SEED, first + k * R + r)
            o.run(pos, P)
            rc = o.root_children()
            rows.append((rc[0], rc[1], o.root_visits, o.root_value))
    assert_same(_as_reference(got), numpy_merge(R, *_tables(rows)), "against the oracle's replicas:")
    assert not got["status"].any()
    es.close()


def test_refusals(torch):
    R, P = 3, 24
    a, b = [112, 113, 127], [112, 113, 128]
    # K6, one launch: ensemble 0 whole, ensemble 1 with one replica elsewhere, ensemble 2 positioned again and never searched
    t = G.TraditionalMCTS(3 * R, node_capacity=P * 225 + 1)
    t.set_positions([a] * 3 + [a, b, a] + [b] * 3)
    t.run(P)
    moves = np.zeros((9, 225), np.uint8)
    lens = np.full(9, -1, np.int32)
    moves[6:, :3], lens[6:] = a, 3
    t.set_positions(moves, lens)
    got, stats = _device_merge(torch, t, R), t.root_stats()
    assert got["status"].tolist() == [0, G.ENSEMBLE_MISMATCH, 0]
    assert got["cells"].tolist()[1:] == [-1, -1] and got["cells"][0] >= 0
    assert got["cells_per_game"].tolist() == [int(got["cells"][0])] * 3 + [-1] * 6
    assert not got["visits"][1:].any() and not got["values"][1:].any() and not got["root_visits"][1:].any()
    whole = G.ensemble_merge_host(R, stats["visits"][:3], stats["values"][:3], stats["root_visits"][:3], stats["root_value"][:3])
    assert_same({k: v[:1] for k, v in got.items() if k != "cells_per_game"}, whole, "the neighbour of a refused ensemble:")
    # the same stones in another order are the same position
    t.set_positions([a] * 3 + [[127, 113, 112]] * 3 + [b] * 3)
    t.run(P)
    assert _device_merge(torch, t, R)["status"].tolist() == [0, 0, 0]
    t.set_positions([a] * 3 + [a, [127, 113, 112], a] + [b] * 3)
    t.run(P)
    assert _device_merge(torch, t, R)["status"].tolist() == [0, 0, 0]
    for group in (0, 2, 4, 4097):                            # 2 and 4 do not divide nine games
        with pytest.raises(G.GmkError):
            t.ensemble_merge(group)
    t.close()
    # K3: a replica elsewhere, and a handle that was never searched
    m = G.BatchedMCTS(2 * R, playouts_capacity=P)
    lists = [a] * 3 + [a, a, b]
    mv = np.zeros((6, 225), np.uint8)
    mv[:, :3] = lists
    m.set_roots(G.moves_to_planes(mv, np.full(6, 3, np.int32)), np.array([l[-1] for l in lists], np.int16), 11)
    idle = _device_merge(torch, m, R)
    assert idle["cells"].tolist() == [-1, -1] and idle["status"].tolist() == [0, G.ENSEMBLE_MISMATCH] and not idle["visits"].any()
    m.run(P)
    got = _device_merge(torch, m, R)
    assert got["status"].tolist() == [0, G.ENSEMBLE_MISMATCH] and got["cells"][0] >= 0 and got["cells"][1] == -1
    assert got["cells_per_game"].tolist() == [int(got["cells"][0])] * 3 + [-1] * 3
    assert got["visits"][0].sum() == R * (P - 1) and not got["visits"][1].any() and not got["values"][1].any()
    with pytest.raises(G.GmkError):
        m.ensemble_merge(4)
    m.close()


def test_step_keeps_the_subtrees(torch, oracle):
    O, R, P, first = oracle, 3, 32, 700
    positions = _openings(2, 4, 33)
    es = EnsembleSearch("random", R, seed=SEED, first_game_id=first, playouts_capacity=2 * P)
    es.set_positions(positions)
    es.search(P)
    before = es.merged()
    es.step()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(es._cells_per_game.cpu().numpy(), np.repeat(before["cell"], R))
    es.search(P)
    got = es.merged()
    rows = []
    for k, pos in enumerate(positions):
        for r in range(R):
            m = O.MCTS(P, 5.0, 5, SEED, first + k * R + r)
            board = _board(O, pos)
            m.eval_state(board)
            m.step_forward(int(before["cell"][k]))
            O.lib().go_board_apply(C.byref(board), int(before["cell"][k]), 1)
            m.eval_state(board)
            v, q, _ = m.root_children()
            rows.append((v, q, m.root_visits, m.root_value))
    assert_same(_as_reference(got), numpy_merge(R, *_tables(rows)), "after the step:")
    assert not got["status"].any() and (got["root_visits"] > R * P).all()          # kept subtrees: more than the second search's visits
    assert es.stones == [5, 5]
    es.close()


@pytest.mark.parametrize("policy,noise", [("random", None), ("traditional", (0.05, 0.25))])
def test_facade_is_reproducible_and_ids_are_global(torch, policy, noise):
    R, P = 4, 40
    positions = [p if len(p) >= 2 else [112, 113] for p in _clustered(3, 8, 610)]
    es = EnsembleSearch(policy, R, first_game_id=9, root_noise=noise, playouts_capacity=P)
    runs = []
    for _ in range(2):
        es.set_positions(positions)
        es.search(P)
        runs.append(es.merged())
    assert_same(_as_reference(runs[0]), _as_reference(runs[1]), "the same search twice:")
    es.close()
    alone = EnsembleSearch(policy, R, first_game_id=9, root_noise=noise, playouts_capacity=P)
    alone.set_positions([positions[2]], ensemble_ids=[2])
    alone.search(P)
    got = alone.merged()
    assert_same(_as_reference(got), {k: v[2:3] for k, v in _as_reference(runs[0]).items()}, "ensemble 2 alone:")
    value, pi = alone.eval_state()[0]
    assert value == float(got["root_value"][0])
    np.testing.assert_array_equal(pi, G.visits_to_pi(got["visits"][0], len(positions[2])))
    alone.close()


def test_agent(torch):
    from gomokuai_amd import core
    from gomokuai_amd import interface as I
    agent = I.make_agent("random-mcts:5:5", iterations=32, quiet=True, replicas=8)
    assert isinstance(agent, I.EnsembleAgent)
    board = core.Board()
    for cell in (112, 113, 127):
        board.apply_move(core.Position(cell))
    agent.sync_with_board(board)
    move = agent.get_action(board)
    assert int(move.id) == int(np.argmax(agent.search.eval_state()[0][1]))
    debug = agent.debug_message()
    assert debug["replicas"] == 8 and debug["playouts_per_replica"] == 32 and debug["total_playouts"] == 256 and debug["duration"].endswith("ms")
    board.apply_move(move)
    taken = {int(p.id) for p in board.move_record}
    reply = next(c for c in range(225) if c not in taken)
    board.apply_move(core.Position(reply))
    agent.sync_with_board(board)                             # two played moves: the trees follow them
    assert agent.search.stones == [5]
    second = agent.get_action(board)
    assert 0 <= int(second.id) < 225 and int(second.id) not in taken | {reply}
    assert agent.debug_message()["total_playouts"] == 256
    agent.search.close()
