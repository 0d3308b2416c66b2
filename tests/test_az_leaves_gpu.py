"""K7 with several leaves per game per step and virtual loss (GMK_OPT_AZ_LEAVES, az_select_leaves_kernel / az_expand_leaves_kernel) against
tests/az_leaves_reference.py, a plain Python restatement of the rules that tests/test_az_leaves_reference.py ties to the oracle at one leaf per
step.  The network is a host function of the batch (every one of the live x L rows goes through the same numpy evaluator the reference calls), so
the search itself is compared exactly: visit counts, value and prior bits, tree size, status."""
import ctypes as C
import functools

import numpy as np
import pytest

import az_leaves_reference as R
from gomokuai_amd import lib as G
from gomokuai_amd import selfplay

pytestmark = pytest.mark.gpu

N = 225
ERR_ARG, ERR_STATE = -3, -4


def _roots(openings):
    moves, lens = np.zeros((len(openings), N), np.uint8), np.array([len(p) for p in openings], np.int32)
    last = np.full((len(openings), 2), -1, np.int16)
    for g, p in enumerate(openings):
        moves[g, :len(p)] = p
        last[g, :min(2, len(p))] = p[::-1][:2]
    return G.moves_to_planes(moves, lens), last


def _host_network(evaluator):
    import torch

    def network(states):                                         # the batch goes to the host, through the evaluator row by row, and back
        s = states.cpu().numpy()
        vp = [evaluator(s[r]) for r in range(s.shape[0])]
        return (torch.tensor([float(v) for v, _ in vp], dtype=torch.float32, device="cuda"), torch.from_numpy(np.stack([p for _, p in vp])).cuda())
    return network


def _tree(openings, leaves, c_puct, node_capacity=1 << 16):
    G.init()
    tree = G.AlphaZeroMCTS(len(openings), node_capacity=node_capacity, c_puct=c_puct, leaves=leaves)
    tree.set_roots(*_roots(openings))
    return tree


def _same(st, refs, where=""):
    for g, ref in enumerate(refs):
        rs, at = ref.root_stats(), "%s game %d" % (where, g)
        np.testing.assert_array_equal(st["visits"][g], rs["visits"], at)
        np.testing.assert_array_equal(st["values"][g].view(np.uint32), rs["values"].view(np.uint32), at)
        np.testing.assert_array_equal(st["priors"][g].view(np.uint32), rs["priors"].view(np.uint32), at)
        assert st["root_visits"][g] == rs["root_visits"] and st["n_nodes"][g] == rs["n_nodes"] and st["status"][g] == rs["status"], at
        assert np.float32(st["root_value"][g]).view(np.uint32) == np.float32(rs["root_value"]).view(np.uint32), at


@functools.lru_cache(maxsize=None)
def _reference(name, leaves, playouts, c_puct, node_capacity=1 << 16):
    openings, evaluator = {"sharpened": (R.OPENINGS, R.sharpened), "open_four": ([R.OPEN_FOUR], R.uniform), "late": (_late_boards(), R.surrogate),
                           "small": ([[112, 113, 127], R.OPENINGS[4]], R.sharpened)}[name]
    out = []
    for moves in openings:
        ref = R.LeavesSearch(moves, evaluator, c_puct=c_puct, leaves=leaves, node_capacity=node_capacity)
        ref.search(playouts)
        out.append(ref)
    return out


# ---------------- 1. parity ----------------
@pytest.mark.parametrize("leaves", [2, 4, 8])
@pytest.mark.parametrize("playouts", [96, 50])
def test_search_matches_the_reference(leaves, playouts):
    refs = _reference("sharpened", leaves, playouts, 1.0)
    tree = _tree(R.OPENINGS, leaves, 1.0)
    tree.search(_host_network(R.sharpened), playouts)
    st = tree.root_stats()
    assert (st["root_visits"] == playouts).all() and (st["status"] == 0).all() and tree.playouts_owed() == 0
    _same(st, refs)
    tree.close()


def _late_boards():
    """Four shuffled tie games cut 2 .. 5 cells before the full board (no five on the board: two colour classes that never line up)"""
    rng = np.random.RandomState(29)
    cls = lambda c: ((c % 15) // 2 + c // 15) % 2
    blacks, whites = [c for c in range(N) if cls(c) == 0], [c for c in range(N) if cls(c) == 1]
    out = []
    for g in range(4):
        b, w = list(rng.permutation(blacks)), list(rng.permutation(whites))
        seq = []
        while b or w:
            if b:
                seq.append(int(b.pop()))
            if w:
                seq.append(int(w.pop()))
        out.append(seq[:N - 2 - g])
    return out


@pytest.mark.parametrize("leaves", [3, 8])
def test_few_empty_cells(leaves):
    """Trees that run out of leaves: more descents in a step than the tree has open leaves, so steps end in collisions below the root, and
    full boards (ties) are backed up between the descents of a step."""
    refs = _reference("late", leaves, 60, 5.0)
    assert sum(ref.collisions for ref in refs) > len(refs) and sum(ref.terminal_playouts for ref in refs) > 0
    tree = _tree(_late_boards(), leaves, 5.0, node_capacity=4096)
    tree.search(_host_network(R.surrogate), 60)
    _same(tree.root_stats(), refs)
    tree.close()


# ---------------- 2. one leaf per step is the search there was ----------------
def test_one_leaf_is_the_default_handle():
    stats = []
    for kw in ({}, {"leaves": 1}):
        G.init()
        tree = G.AlphaZeroMCTS(len(R.OPENINGS), node_capacity=1 << 16, c_puct=5.0, **kw)
        if kw:
            tree.set_option(G.OPT_AZ_LEAVES, 1)                  # set explicitly, through the C entry as well
        tree.set_roots(*_roots(R.OPENINGS))
        tree.search(_host_network(R.surrogate), 60)
        assert tree.playouts_owed() == 0 and tree.states.shape[0] == len(R.OPENINGS)
        stats.append(tree.root_stats())
        tree.close()
    for k in stats[0]:
        assert (stats[0][k].view(np.uint32) == stats[1][k].view(np.uint32)).all(), k
    assert (stats[0]["root_visits"] == 60).all()


# ---------------- 3. terminal leaves inside a step ----------------
def test_a_won_root_takes_every_playout():
    tree = _tree([R.WON], 8, 5.0, node_capacity=256)
    tree.search(_host_network(R.uniform), 40)
    st = tree.root_stats()
    assert st["root_visits"][0] == 40 and st["root_value"][0] == 1.0 and st["n_nodes"][0] == 1 and st["status"][0] == 0
    tree.close()


@pytest.mark.parametrize("leaves", [4, 8])
def test_fives_below_the_root(leaves):
    refs = _reference("open_four", leaves, 160, 5.0)
    assert refs[0].terminal_playouts > 0
    tree = _tree([R.OPEN_FOUR], leaves, 5.0)
    tree.search(_host_network(R.uniform), 160)
    _same(tree.root_stats(), refs)
    tree.close()


# ---------------- 4. arena full ----------------
def test_dropped_playouts_give_their_marks_back():
    refs = _reference("small", 4, 40, 1.0, 256)
    openings = [[112, 113, 127], R.OPENINGS[4]]
    tree = _tree(openings, 4, 1.0, node_capacity=256)
    network = _host_network(R.sharpened)
    tree.search(network, 40)
    st = tree.root_stats()
    assert (st["status"] & G.AlphaZeroMCTS.STATUS_ARENA_FULL).all() and (st["n_nodes"] <= 256).all() and tree.playouts_owed() == 0
    _same(st, refs)
    tree.set_option(G.OPT_AZ_LEAVES, 1)                          # a mark left behind by a dropped playout would bend the one-leaf search
    tree.search(network, 10)
    again = []
    for moves in openings:
        ref = R.LeavesSearch(moves, R.sharpened, c_puct=1.0, leaves=4, node_capacity=256)
        ref.search(40)
        ref.leaves = 1
        ref.search(10)
        again.append(ref)
    _same(tree.root_stats(), again)
    tree.close()


# ---------------- 5. kept subtrees ----------------
def test_kept_subtrees_and_back_to_one_leaf():
    network = _host_network(R.sharpened)
    refs = [R.LeavesSearch(moves, R.sharpened, c_puct=1.0, leaves=4, node_capacity=1 << 16) for moves in R.OPENINGS]
    tree = _tree(R.OPENINGS, 4, 1.0)

    def search(playouts, where):
        tree.search(network, playouts)
        for ref in refs:
            ref.search(playouts)
        _same(tree.root_stats(), refs, where)
    search(64, "first search")
    tree.step(None)
    for ref in refs:
        assert ref.reroot() is not None
    kept = [ref.root_stats()["root_visits"] for ref in refs]
    assert max(kept) > 1
    search(64, "after the step to the most visited child")
    reply = np.zeros(len(refs), np.int16)
    for g, ref in enumerate(refs):
        st = ref.root_stats()
        free = [c for c in range(N) if c not in ref.moves]
        reply[g] = int(st["visits"].argmax()) if g % 2 == 0 else next(c for c in free if st["priors"][c] == 0)      # a child, or a cell without one
        assert ref.reroot(int(reply[g])) == reply[g]
    tree.step(reply)
    assert sorted(set(ref.n_nodes == 1 for ref in refs)) == [False, True]
    search(64, "after the step to a given reply")
    tree.set_option(G.OPT_AZ_LEAVES, 1)
    for ref in refs:
        ref.leaves = 1
    search(32, "one leaf per step again")
    assert (tree.root_stats()["status"] == 0).all()
    tree.close()


# ---------------- 6. root noise ----------------
def test_root_noise_before_a_search():
    tree = _tree(R.OPENINGS, 4, 1.0)
    tree.set_option(G.OPT_NOISE_SAMPLER, G.NOISE_SAMPLERS["counter"])
    network = _host_network(R.sharpened)
    tree.search(network, 9)
    before = tree.root_stats()
    tree.add_root_noise(0.05, 0.25, seed=777, first_game_id=20)
    tree.search(network, 50)
    st = tree.root_stats()
    assert (st["root_visits"] == before["root_visits"] + 50).all() and (before["root_visits"] == 9).all() and (st["status"] == 0).all()
    assert (st["priors"].view(np.uint32) != before["priors"].view(np.uint32)).any(1).all()
    tree.close()


# ---------------- 7. misuse ----------------
def test_misuse_is_refused_and_the_handle_goes_on():
    import torch
    L = G.load()
    tree = _tree(R.OPENINGS, 1, 1.0)
    n = len(R.OPENINGS)
    for bad in (0, 9, -1):
        assert L.gmk_az_set_option(tree.h, G.OPT_AZ_LEAVES, bad) == ERR_ARG
        with pytest.raises(G.GmkError):
            tree.set_option(G.OPT_AZ_LEAVES, bad)
    assert tree.leaves == 1
    tree.set_option(G.OPT_AZ_LEAVES, 4)
    assert tree.states.shape[0] == 4 * n
    network = _host_network(R.sharpened)
    tree.add_playouts(8)
    assert tree.playouts_owed() == 8
    states = tree.select()
    assert states.shape[0] == 4 * n and tree.playouts_owed() == 7               # the first step: the root, then a collision
    d_moves, d_lens, d_winner = torch.zeros((n, N), dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int8, device="cuda")
    d_cells, d_verdict = torch.zeros(n, dtype=torch.int16, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    left = C.c_int32(0)
    stream = torch.cuda.current_stream().cuda_stream
    assert L.gmk_az_step(tree.h, None) == ERR_STATE
    assert L.gmk_az_advance(tree.h, d_moves.data_ptr(), None, d_lens.data_ptr(), d_winner.data_ptr(), 1, C.byref(left), stream) == ERR_STATE
    assert L.gmk_az_step_device(tree.h, d_cells.data_ptr(), d_verdict.data_ptr(), 0, None, None, stream) == ERR_STATE
    assert L.gmk_az_set_option(tree.h, G.OPT_AZ_LEAVES, 2) == ERR_STATE
    assert L.gmk_az_set_option(tree.h, G.OPT_NOISE_SAMPLER, 1) == ERR_STATE
    assert L.gmk_az_add_root_noise(tree.h, 0.05, 0.25, 1, 0, stream) == ERR_STATE
    assert L.gmk_az_select(tree.h, tree.states.data_ptr(), stream) == ERR_STATE
    assert b"gmk_az_expand" in L.gmk_last_error()
    values, probs = network(states)
    tree.expand(values, probs)
    paths, lens = np.zeros((n, 226), np.int16), np.zeros(n, np.int32)
    assert L.gmk_az_select_host(tree.h, paths.ctypes.data, lens.ctypes.data) == ERR_STATE
    assert L.gmk_az_expand_host(tree.h, values.cpu().numpy().ctypes.data, probs.cpu().numpy().ctypes.data) == ERR_STATE
    tree.search(network, 20)                                                     # the seven still owed and twenty more
    st = tree.root_stats()
    assert (st["root_visits"] == 28).all() and (st["status"] == 0).all() and tree.playouts_owed() == 0
    refs = []
    for moves in R.OPENINGS:
        ref = R.LeavesSearch(moves, R.sharpened, c_puct=1.0, leaves=4)
        ref.quota = 8
        ref.step()
        ref.search(20)
        refs.append(ref)
    _same(st, refs)
    tree.step(None)                                                              # and the calls that were refused work now
    tree.close()


# ---------------- 8. hipGraph ----------------
def test_a_captured_step_replays_the_search():
    import torch
    from gomokuai_amd.network import FusedPolicyValueNetwork, PolicyValueNetwork
    G.init()
    fused = FusedPolicyValueNetwork(PolicyValueNetwork(seed=4).cuda().eval())
    stats = []
    for graph in (False, True):
        tree = _tree(R.OPENINGS, 4, 5.0)
        with torch.no_grad():
            tree.search(fused, 50, graph=graph)
        torch.cuda.synchronize()
        stats.append(tree.root_stats())
        tree.close()
    assert (stats[0]["root_visits"] == 50).all() and (stats[0]["status"] == 0).all()
    for k in stats[0]:
        assert (stats[0][k].view(np.uint32) == stats[1][k].view(np.uint32)).all(), k
    fused.close()


# ---------------- 9. the loops ----------------
def test_network_self_play_with_leaves_through_slots():
    from gomokuai_amd.network import FusedPolicyValueNetwork, PolicyValueNetwork
    from helpers import PaddedNetwork
    net = FusedPolicyValueNetwork(PolicyValueNetwork(seed=8).cuda().eval())
    fused = PaddedNetwork(net, 5 * 4)
    kw = dict(opening_plies=2, first_game_id=70, seed=2, reuse_subtree=True, root_noise=(0.05, 0.25), leaves=4)
    few = selfplay.play_network_games(5, fused, 16, slots=2, **kw).cpu()
    full = selfplay.play_network_games(5, fused, 16, **kw).cpu()
    assert not few.overflow and not full.overflow
    assert (few.lens == full.lens).all() and (few.winner == full.winner).all() and int(few.lens.min()) >= 9
    for g in range(5):
        n = int(few.lens[g])
        assert n == N or int(few.winner[g]) != 0                                 # every game ends
        assert (few.moves[g, :n] == full.moves[g, :n]).all() and (few.visits[g, :n] == full.visits[g, :n]).all()
    assert int(few.visits[:, 2].to(int).sum(1).min()) == 16 - 1                  # a first move's row: every playout but the root's own
    net.close()


def test_evaluation_match_with_leaves_on_both_loops():
    from gomokuai_amd.network import FusedPolicyValueNetwork, PolicyValueNetwork
    from helpers import PaddedNetwork
    net = FusedPolicyValueNetwork(PolicyValueNetwork(seed=12).cuda().eval())
    fused = PaddedNetwork(net, 2 * 4)
    opponent = ("traditional_mcts", {"c_puct": 5.0, "c_iterations": 50})
    kw = dict(playouts=16, seed=9, first_game_id=40, leaves=4)
    (rd, bd, sd), (rh, bh, sh) = (selfplay.play_evaluation_games(4, fused, opponent, device_loop=loop, **kw) for loop in (True, False))
    cd, ch = rd.cpu(), rh.cpu()
    assert (bd == bh).all() and (sd == sh).all() and not rd.overflow and not rh.overflow
    assert (cd.lens == ch.lens).all() and (cd.winner == ch.winner).all() and int(cd.lens.min()) >= 9
    for g in range(4):
        k = int(cd.lens[g])
        assert (cd.moves[g, :k] == ch.moves[g, :k]).all() and (cd.visits[g, :k] == ch.visits[g, :k]).all(), g
    assert all(g["unfinished"] == 0 for g in rd.groups)
    net.close()
