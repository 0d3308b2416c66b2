"""K7 with forced wins by fours solved at its leaves (GMK_OPT_AZ_VCF_DEPTH / _BUDGET, az_vcf_leaves_kernel and the verdict-reading expand
kernels) against tests/az_vcf_reference.py, the restatement tests/test_az_vcf_reference.py holds to hand-checked facts.  The network is a host
function of the batch, the same numpy evaluator the restatement calls, so the searches are compared exactly: visits, value and prior bits, root
statistics, tree size, status; the per-leaf verdicts are compared with lib.vcf_solve on the leaves' move lists."""

import numpy as np
import pytest

import az_leaves_reference as R
import az_vcf_reference as A
import vcf_reference as V
from gomokuai_amd import lib as G
from gomokuai_amd import selfplay
from test_az_vcf_reference import parity_reference

pytestmark = pytest.mark.gpu

N = 225
ERR_ARG, ERR_STATE = -3, -4
FIVE = [R._c(7, 2), R._c(0, 0), R._c(7, 3), R._c(0, 2), R._c(7, 4), R._c(0, 4), R._c(7, 5), R._c(0, 6), R._c(7, 6), R._c(0, 8)]     # black has five: OVER


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


def _tree(openings, leaves, c_puct, depth, budget, node_capacity=1 << 16):
    G.init()
    tree = G.AlphaZeroMCTS(len(openings), node_capacity=node_capacity, c_puct=c_puct, leaves=leaves, vcf_depth=depth, vcf_budget=budget)
    tree.set_roots(*_roots(openings))
    return tree


def _same(st, refs, where="", games=None):
    for g, ref in zip(range(len(refs)) if games is None else games, refs):
        rs, at = ref.root_stats(), "%s game %d" % (where, g)
        np.testing.assert_array_equal(st["visits"][g], rs["visits"], at)
        np.testing.assert_array_equal(st["values"][g].view(np.uint32), rs["values"].view(np.uint32), at)
        np.testing.assert_array_equal(st["priors"][g].view(np.uint32), rs["priors"].view(np.uint32), at)
        assert st["root_visits"][g] == rs["root_visits"] and st["n_nodes"][g] == rs["n_nodes"] and st["status"][g] == rs["status"], at
        assert np.float32(st["root_value"][g]).view(np.uint32) == np.float32(rs["root_value"]).view(np.uint32), at


def _same_counters(stats, refs, games=None):
    for g, ref in zip(range(len(refs)) if games is None else games, refs):
        assert (stats["leaves"][g], stats["wins"][g], stats["cut"][g], stats["nodes"][g]) == (ref.solved, ref.wins, ref.cut, ref.nodes), g


def _solve(move_lists, depth, budget):
    moves, lens = np.zeros((len(move_lists), N), np.uint8), np.array([len(p) for p in move_lists], np.int32)
    for g, p in enumerate(move_lists):
        moves[g, :len(p)] = p
    return G.vcf_solve(moves, lens, max_depth=depth, budget=budget)


# ---------------- 1. parity with the restatement, and the counters ----------------
@pytest.mark.parametrize("leaves", [1, 4])
@pytest.mark.parametrize("depth,budget", A.PARITY_SETTINGS)
def test_search_matches_the_restatement(leaves, depth, budget):
    refs = parity_reference(leaves, depth, budget)
    tree = _tree(A.PARITY_OPENINGS, leaves, 1.0, depth, budget)
    tree.search(_host_network(R.sharpened), 48)
    st = tree.root_stats()
    assert (st["root_visits"] == 48).all() and (st["status"] == 0).all()
    _same(st, refs)
    stats = tree.vcf_stats()
    _same_counters(stats, refs)
    assert stats["wins"].sum() > 0 and stats["cut"].sum() > 0 and stats["nodes"].dtype == np.uint64
    tree.set_roots(*_roots(A.PARITY_OPENINGS))
    assert all(int(v.sum()) == 0 for v in tree.vcf_stats().values())
    tree.close()


# ---------------- 2. per-leaf verdicts ----------------
def _positions(n):
    import random
    rng = random.Random(5)
    pool = [A.QUIET, A.BLACK_THREE, A.WHITE_THREE, R.OPEN_FOUR, A.HARD, A.WHITE_THREE_BLACK_TO_MOVE, [], FIVE]
    while len(pool) < n:
        moves = V.random_position(rng, rng.choice([14, 17, 20]), 3)
        if moves is not None:
            pool.append(moves)
    return pool[:n]


@pytest.mark.parametrize("n", [1, 3, 4, 5, 17])
def test_root_verdicts_are_the_solvers(n):
    positions = _positions(8)[1:1 + n] if n < 5 else _positions(n)              # few games: the ones with a verdict other than NONE
    for depth, budget in ((8, 64), (1, 64), (8, 3)):
        tree = _tree(positions, 1, 1.0, depth, budget)
        tree.select()
        got, want = tree.vcf_verdicts(), _solve(positions, depth, budget)
        for k in ("status", "move", "length", "nodes"):
            np.testing.assert_array_equal(got[k], want[k], "%s at (%d, %d)" % (k, depth, budget))
        tree.close()
    assert n < 5 or len(set(want["status"])) >= 3


def test_verdicts_at_eight_leaves_on_one_game():
    tree = _tree([A.BLACK_THREE], 8, 1.0, 8, 64)
    tree.add_playouts(20)
    tree.select()                                                # the root, then a collision: one pending leaf, seven rows without one
    got = tree.vcf_verdicts()
    assert got["status"].shape == (8,)
    assert (got["status"][0], got["move"][0], got["length"][0], got["nodes"][0]) == (G.VCF_WIN, 4, 2, 4)
    assert (got["status"][1:] == G.VCF_NONE).all() and (got["move"][1:] == -1).all() and (got["length"][1:] == 0).all() and (got["nodes"][1:] == 0).all()
    values, probs = _host_network(R.sharpened)(tree.states[:8])
    tree.expand(values, probs)
    tree.close()


@pytest.mark.parametrize("leaves", [1, 4])
def test_verdicts_below_the_root_step_by_step(leaves):
    """Twelve steps of five games beside the restatement: every step's verdicts are lib.vcf_solve's on the pending leaves' move lists, row
    game * L + k, and the rows without a leaf read NONE / -1 / 0 / 0."""
    refs = [A.VcfLeavesSearch(moves, R.sharpened, 8, 64, c_puct=1.0, leaves=leaves) for moves in A.PARITY_OPENINGS]
    tree = _tree(A.PARITY_OPENINGS, leaves, 1.0, 8, 64)
    network = _host_network(R.sharpened)
    if leaves > 1:
        tree.add_playouts(48)
    for ref in refs:
        ref.quota = 48
    seen = set()
    for step in range(12):
        states = tree.select()
        got = tree.vcf_verdicts()
        lists, rows = [], []
        for g, ref in enumerate(refs):
            ref.select_step()
            for k, (node, moves) in enumerate(ref.pending):
                lists.append(moves)
                rows.append(g * leaves + k)
        want = _solve(lists, 8, 64)
        empty = np.setdiff1d(np.arange(len(refs) * leaves), rows)
        for k in ("status", "move", "length", "nodes"):
            np.testing.assert_array_equal(got[k][rows], want[k], "%s in step %d" % (k, step))
        assert (got["status"][empty] == G.VCF_NONE).all() and (got["move"][empty] == -1).all() and (got["length"][empty] == 0).all() and (got["nodes"][empty] == 0).all()
        seen |= set(int(s) for s in want["status"])
        values, probs = network(states)
        tree.expand(values, probs)
        for ref in refs:
            out = ref.answers([R._planes(moves) for _, moves in ref.pending])
            ref.expand_step([v for v, _ in out], [p for _, p in out])
    assert {G.VCF_NONE, G.VCF_WIN, G.VCF_BUDGET} <= seen
    _same(tree.root_stats(), refs)
    _same_counters(tree.vcf_stats(), refs)
    tree.close()


# ---------------- 3. row seams: a finished game has no row ----------------
@pytest.mark.parametrize("leaves", [1, 4])
def test_rows_after_a_game_has_ended(leaves):
    import torch
    openings = [A.QUIET, R.OPEN_FOUR, A.BLACK_THREE, A.WHITE_THREE, A.HARD]
    tree = _tree(openings, leaves, 1.0, 8, 64)
    network = _host_network(R.sharpened)
    refs = [A.VcfLeavesSearch(moves, R.sharpened, 8, 64, c_puct=1.0, leaves=leaves) for moves in openings]
    tree.search(network, 8)
    for ref in refs:
        ref.search(8)
    d_moves, d_lens = torch.zeros((5, N), dtype=torch.uint8, device="cuda"), torch.tensor([len(p) for p in openings], dtype=torch.int32, device="cuda")
    for g, p in enumerate(openings):
        d_moves[g, :len(p)] = torch.tensor(p, dtype=torch.uint8)
    d_winner = torch.zeros(5, dtype=torch.int8, device="cuda")
    assert tree.advance(d_moves, None, d_lens, d_winner, reuse_subtree=True) == 4           # game 1 plays the five and is over
    assert tree.live == 4 and int(d_winner[1]) == 1 and (tree.root_stats()["status"] == [0, 1, 0, 0, 0]).all()
    live = [0, 2, 3, 4]
    for g in live:
        assert refs[g].reroot() == int(d_moves[g, len(openings[g])])
    if leaves > 1:
        tree.add_playouts(16)
    for g in live:
        refs[g].quota = 16
    states = tree.select()
    assert states.shape[0] == 4 * leaves
    got = tree.vcf_verdicts()
    lists, rows = [], []
    for r, g in enumerate(live):
        refs[g].select_step()
        for k, (node, moves) in enumerate(refs[g].pending):
            lists.append(moves)
            rows.append(r * leaves + k)
    want = _solve(lists, 8, 64)
    for k in ("status", "move", "length", "nodes"):
        np.testing.assert_array_equal(got[k][rows], want[k], k)
    values, probs = network(states)
    tree.expand(values, probs)
    for g in live:
        out = refs[g].answers([R._planes(moves) for _, moves in refs[g].pending])
        refs[g].expand_step([v for v, _ in out], [p for _, p in out])
    if leaves > 1:
        while tree.playouts_owed() > 0:
            values, probs = network(tree.select())
            tree.expand(values, probs)
    else:
        tree.search(network, 15)
    for g in live:
        while refs[g].quota > 0:
            refs[g].step()
    _same(tree.root_stats(), [refs[g] for g in live], "after the end of game 1", live)
    _same_counters(tree.vcf_stats(), [refs[g] for g in live], live)
    tree.close()


# ---------------- 4. the loops ----------------
def test_network_self_play_through_slots_and_on_both_loops():
    from gomokuai_amd.network import FusedPolicyValueNetwork, PolicyValueNetwork
    from helpers import PaddedNetwork
    net = FusedPolicyValueNetwork(PolicyValueNetwork(seed=8).cuda().eval())
    fused = PaddedNetwork(net, 11)
    kw = dict(opening_plies=2, first_game_id=70, seed=2, root_noise=(0.05, 0.25), vcf=(8, 64))
    few = selfplay.play_network_games(11, fused, 12, slots=4, reuse_subtree=True, **kw).cpu()
    full = selfplay.play_network_games(11, fused, 12, slots=11, reuse_subtree=True, **kw).cpu()
    host = selfplay.play_network_games(11, fused, 12, reuse_subtree=True, device_loop=False, **kw).cpu()
    for other in (full, host):
        assert not few.overflow and not other.overflow
        assert (few.lens == other.lens).all() and (few.winner == other.winner).all() and int(few.lens.min()) >= 9
        for g in range(11):
            n = int(few.lens[g])
            assert n == N or int(few.winner[g]) != 0                             # every game ends
            assert (few.moves[g, :n] == other.moves[g, :n]).all() and (few.visits[g, :n] == other.visits[g, :n]).all()
    net.close()


def test_evaluation_match_on_both_loops():
    from gomokuai_amd.network import FusedPolicyValueNetwork, PolicyValueNetwork
    from helpers import PaddedNetwork
    net = FusedPolicyValueNetwork(PolicyValueNetwork(seed=12).cuda().eval())
    fused = PaddedNetwork(net, 2 * 4)
    opponent = ("traditional_mcts", {"c_puct": 5.0, "c_iterations": 50})
    kw = dict(playouts=16, seed=9, first_game_id=40, leaves=4, vcf=(8, 64))
    (rd, bd, sd), (rh, bh, sh) = (selfplay.play_evaluation_games(4, fused, opponent, device_loop=loop, **kw) for loop in (True, False))
    cd, ch = rd.cpu(), rh.cpu()
    assert (bd == bh).all() and (sd == sh).all() and not rd.overflow and not rh.overflow
    assert (cd.lens == ch.lens).all() and (cd.winner == ch.winner).all()
    for g in range(4):
        k = int(cd.lens[g])
        assert (cd.moves[g, :k] == ch.moves[g, :k]).all() and (cd.visits[g, :k] == ch.visits[g, :k]).all(), g
    net.close()


# ---------------- 5. kept subtrees and root noise ----------------
@pytest.mark.parametrize("leaves", [1, 4])
def test_kept_subtrees_and_root_noise_across_three_moves(leaves):
    openings = [A.QUIET, A.WHITE_THREE_BLACK_TO_MOVE, A.HARD, A.BLACK_THREE]
    refs = [A.VcfLeavesSearch(moves, R.sharpened, 8, 64, c_puct=1.0, leaves=leaves) for moves in openings]
    tree = _tree(openings, leaves, 1.0, 8, 64)
    tree.set_option(G.OPT_NOISE_SAMPLER, G.NOISE_SAMPLERS["counter"])
    network = _host_network(R.sharpened)
    for move in range(3):
        if move:
            tree.add_root_noise(0.05, 0.25, seed=777, first_game_id=20)
            noisy = tree.root_stats()["priors"]
            for g, ref in enumerate(refs):                      # the restatement has no sampler: it takes the device's noisy root priors
                for i in range(ref.first[0], ref.first[0] + ref.nkids[0]):
                    ref.prior[i] = np.float32(noisy[g][ref.cell[i]])
        tree.search(network, 24)
        for ref in refs:
            ref.search(24)
        _same(tree.root_stats(), refs, "move %d" % move)
        tree.step(None)
        for ref in refs:
            assert ref.reroot() is not None
    assert max(ref.root_stats()["root_visits"] for ref in refs) > 1 and sum(ref.wins for ref in refs) > 0
    _same(tree.root_stats(), refs, "after the last step")
    _same_counters(tree.vcf_stats(), refs)
    tree.close()


# ---------------- 6. hipGraph ----------------
@pytest.mark.parametrize("leaves", [1, 4])
def test_a_captured_step_replays_the_search(leaves):
    import torch
    from gomokuai_amd.network import FusedPolicyValueNetwork, PolicyValueNetwork
    G.init()
    fused = FusedPolicyValueNetwork(PolicyValueNetwork(seed=4).cuda().eval())
    stats, counters = [], []
    for graph in (False, True):
        tree = _tree(A.PARITY_OPENINGS, leaves, 5.0, 8, 64)
        with torch.no_grad():
            tree.search(fused, 40, graph=graph)
        torch.cuda.synchronize()
        stats.append(tree.root_stats())
        counters.append(tree.vcf_stats())
        tree.close()
    assert (stats[0]["root_visits"] == 40).all() and (stats[0]["status"] == 0).all() and counters[0]["wins"].sum() > 0
    for k in stats[0]:
        assert (stats[0][k].view(np.uint32) == stats[1][k].view(np.uint32)).all(), k
    for k in counters[0]:
        assert (counters[0][k] == counters[1][k]).all(), k
    fused.close()


# ---------------- 7. the arena: room for exactly the one child, and one node short of it ----------------
def far_rows(states):
    """Value 0 and the same probability on the 150 cells of rows 5 .. 14, none on rows 0 .. 4"""
    probs = np.zeros(N, dtype=np.float32)
    probs[75:] = np.float32(1.0) / np.float32(150.0)
    return np.float32(0.0), probs


@pytest.mark.parametrize("leaves", [1, 4])
def test_the_one_child_fits_exactly_and_then_does_not(leaves):
    """White holds the open three and black moves far from it: the root gets 147 children from the network, and every one of them is a leaf
    white wins, worth one node.  The 108th of them fills the arena of 256 to the last node; the next one is a node short, sets status bit 1
    and is not backed up."""
    cap, playouts = 256, 120
    ref = A.VcfLeavesSearch(A.WHITE_THREE_BLACK_TO_MOVE, far_rows, 8, 64, c_puct=5.0, leaves=leaves, node_capacity=cap)
    ref.search(playouts)
    rs = ref.root_stats()
    assert ref.n_nodes == cap and rs["status"] == R.STATUS_ARENA_FULL and ref.wins > 108 and rs["root_visits"] == 1 + 108 < playouts
    tree = _tree([A.WHITE_THREE_BLACK_TO_MOVE], leaves, 5.0, 8, 64, node_capacity=cap)
    tree.search(_host_network(far_rows), playouts)
    _same(tree.root_stats(), [ref])
    _same_counters(tree.vcf_stats(), [ref])
    tree.close()


# ---------------- 8. the caller's tensors ----------------
@pytest.mark.parametrize("leaves", [1, 4])
def test_values_and_probs_are_not_written(leaves):
    import torch
    tree = _tree(A.PARITY_OPENINGS, leaves, 1.0, 8, 64)
    if leaves > 1:
        tree.add_playouts(4)
    states = tree.select()
    values, probs = _host_network(R.sharpened)(states)
    v0, p0 = values.clone(), probs.clone()
    tree.expand(values, probs)
    torch.cuda.synchronize()
    assert torch.equal(values.view(torch.int32), v0.view(torch.int32)) and torch.equal(probs.view(torch.int32), p0.view(torch.int32))
    st = tree.root_stats()
    assert st["n_nodes"][1] == 2 and st["priors"][1][4] == 1.0 and float(p0[1 * leaves][4]) != 1.0        # although the leaf was answered by the solver
    tree.close()


# ---------------- 9. option state ----------------
def test_switched_off_again_is_the_plain_search():
    network = _host_network(R.sharpened)
    used = _tree(A.PARITY_OPENINGS, 1, 1.0, 8, 64)
    used.search(network, 10)
    assert used.vcf_stats()["wins"].sum() > 0
    used.set_option(G.OPT_AZ_VCF_DEPTH, 0)
    used.set_roots(*_roots(A.PARITY_OPENINGS))
    used.search(network, 30)
    with pytest.raises(G.GmkError):
        used.vcf_verdicts()                                      # GMK_ERR_STATE: nothing is solved
    fresh = G.AlphaZeroMCTS(len(A.PARITY_OPENINGS), node_capacity=1 << 16, c_puct=1.0)
    fresh.set_roots(*_roots(A.PARITY_OPENINGS))
    fresh.search(network, 30)
    a, b = used.root_stats(), fresh.root_stats()
    for k in a:
        assert (a[k].view(np.uint32) == b[k].view(np.uint32)).all(), k
    assert all(int(v.sum()) == 0 for v in used.vcf_stats().values())
    used.close()
    fresh.close()


@pytest.mark.parametrize("leaves", [1, 4])
def test_misuse_is_refused_and_the_handle_goes_on(leaves):
    L = G.load()
    tree = _tree(A.PARITY_OPENINGS, leaves, 1.0, 0, 64)
    n = len(A.PARITY_OPENINGS)
    for bad in (-1, 33):
        assert L.gmk_az_set_option(tree.h, G.OPT_AZ_VCF_DEPTH, bad) == ERR_ARG
    for bad in (0, -5, (1 << 20) + 1):
        assert L.gmk_az_set_option(tree.h, G.OPT_AZ_VCF_BUDGET, bad) == ERR_ARG
    assert L.gmk_az_vcf_verdicts_host(tree.h, None, None, None, None) == ERR_STATE                 # D = 0
    for good in (1, 1 << 20, 64):
        assert L.gmk_az_set_option(tree.h, G.OPT_AZ_VCF_BUDGET, good) == 0
    for good in (32, 8):
        assert L.gmk_az_set_option(tree.h, G.OPT_AZ_VCF_DEPTH, good) == 0
    network = _host_network(R.sharpened)
    if leaves > 1:
        tree.add_playouts(1)
    states = tree.select()
    assert L.gmk_az_set_option(tree.h, G.OPT_AZ_VCF_DEPTH, 0) == ERR_STATE
    assert L.gmk_az_set_option(tree.h, G.OPT_AZ_VCF_DEPTH, 4) == ERR_STATE
    assert L.gmk_az_set_option(tree.h, G.OPT_AZ_VCF_BUDGET, 9) == ERR_STATE
    assert b"gmk_az_expand" in L.gmk_last_error()
    values, probs = network(states)
    tree.expand(values, probs)
    assert L.gmk_az_set_option(tree.h, G.OPT_AZ_VCF_BUDGET, 64) == 0
    if leaves == 1:                                              # the host-driven one-leaf entries do not solve
        paths, lens = np.zeros((n, 226), np.int16), np.zeros(n, np.int32)
        hv, hp = values.cpu().numpy(), probs.cpu().numpy()
        assert L.gmk_az_select_host(tree.h, paths.ctypes.data, lens.ctypes.data) == ERR_STATE
        assert b"GMK_OPT_AZ_VCF_DEPTH" in L.gmk_last_error()
        assert L.gmk_az_expand_host(tree.h, hv.ctypes.data, hp.ctypes.data) == ERR_STATE
        assert L.gmk_az_set_leaf_host(tree.h, 0, 0, None, 0) == ERR_STATE
        assert L.gmk_az_expand_stages_host(tree.h, hv.ctypes.data, hp.ctypes.data, 1, 1) == ERR_STATE
        tree.set_option(G.OPT_AZ_VCF_DEPTH, 0)
        assert L.gmk_az_select_host(tree.h, paths.ctypes.data, lens.ctypes.data) == 0
        assert L.gmk_az_expand_host(tree.h, hv.ctypes.data, hp.ctypes.data) == 0
        tree.close()
        return
    tree.search(network, 47)
    refs = parity_reference(leaves, 8, 64)
    _same(tree.root_stats(), refs)
    tree.close()
