"""K7 with the defence solver at its leaves (GMK_OPT_AZ_VCF_DEFEND: az_threat_leaves_kernel, az_defend_leaves_kernel and the <true, true, true>
expand kernels) against tests/az_defend_reference.py, the restatement tests/test_az_defend_reference.py holds to hand-checked facts and to a full
minimax.  The network is a host function of the batch, the numpy evaluator the restatement calls, so everything is compared exactly: visits,
value and prior bits, root statistics, tree size, status, the proofs and every counter; the per-leaf tables are compared with lib.vcf_defend on
the leaves' move lists."""
import functools

import numpy as np
import pytest

import az_defend_reference as Z
import az_leaves_reference as R
import az_proof_reference as P
import az_vcf_reference as A
import vcf_defend_reference as D
from gomokuai_amd import lib as G
from gomokuai_amd import selfplay
from test_az_defend_reference import peaked
from test_az_proof_gpu import _same_proofs
from test_az_vcf_gpu import FIVE, _host_network, _roots, _same, _same_counters

pytestmark = pytest.mark.gpu

N = 225
ERR_ARG, ERR_STATE = -3, -4
OPENINGS = A.PARITY_OPENINGS + Z.TABLE                           # nine games


def mixed(states):
    """uniform where white is to move on a board of at most eleven stones -- the table's positions as roots: every free cell gets a child, so
    a root without a holding reply is proven --, the peaked surrogate elsewhere"""
    s = np.asarray(states).reshape(6, N)
    return R.uniform(states) if s[5].sum() == 0 and N - int(s[2].sum()) <= 11 else R.sharpened(states)


def _tree(openings, leaves, c_puct, depth=8, budget=64, proof=True, defend=True, node_capacity=1 << 16):
    G.init()
    tree = G.AlphaZeroMCTS(len(openings), node_capacity=node_capacity, c_puct=c_puct, leaves=leaves, vcf_depth=depth, vcf_budget=budget, proof=proof,
                           vcf_defend=defend)
    tree.set_roots(*_roots(openings))
    return tree


def _ref(moves, evaluator, leaves, c_puct, depth=8, budget=64, **kw):
    return Z.DefendSearch(moves, evaluator, depth, budget, proof=True, defend=True, c_puct=c_puct, leaves=leaves, **kw)


def _same_defend(tree, refs, where=""):
    ds = tree.defend_stats()
    assert ds["nodes"].dtype == np.uint64
    for g, ref in enumerate(refs):
        got = {k: int(ds[k][g]) for k in ("threatened", "marked", "searched", "nodes")}
        assert got == ref.defend_stats(), "%s game %d" % (where, g)


def _same_all(tree, refs, where=""):
    _same(tree.root_stats(), refs, where)
    _same_proofs(tree, refs, where)
    _same_counters(tree.vcf_stats(), refs)
    _same_defend(tree, refs, where)


def _defend(move_lists, depth, budget):
    moves, lens = np.zeros((len(move_lists), N), np.uint8), np.array([len(p) for p in move_lists], np.int32)
    for g, p in enumerate(move_lists):
        moves[g, :len(p)] = p
    return G.vcf_defend(moves, lens, max_depth=depth, budget=budget, iterative=False)


def _same_tables(tree, move_lists, depth, budget, where=""):
    """defend_verdicts() of the last select against lib.vcf_defend, row by row; move_lists[r] is None for a row without a pending leaf.  A row
    the solver answered WIN or OVER itself reads NONE and zeros."""
    got, own = tree.defend_verdicts(), tree.vcf_verdicts()
    assert got["verdict"].shape == (len(move_lists), N) and got["nodes"].dtype == np.uint32
    asked = [r for r, p in enumerate(move_lists) if p is not None and own["status"][r] not in (G.VCF_WIN, G.VCF_OVER)]
    want = _defend([move_lists[r] for r in asked], depth, budget) if asked else None
    seen = set()
    for r in range(len(move_lists)):
        at = "%s row %d at (%d, %d)" % (where, r, depth, budget)
        if r not in asked:
            assert got["threat_status"][r] == G.VCF_NONE and got["threat_length"][r] == 0 and not got["verdict"][r].any() and not got["nodes"][r].any(), at
            continue
        i = asked.index(r)
        assert (got["threat_status"][r], got["threat_length"][r]) == (want["threat_status"][i], want["threat_length"][i]), at
        np.testing.assert_array_equal(got["verdict"][r].astype(np.uint8), want["verdict"][i], at)
        np.testing.assert_array_equal(got["nodes"][r], want["nodes"][i], at)
        seen.add(int(got["threat_status"][r]))
    return seen


# ---------------- 1. parity with the restatement ----------------
@functools.lru_cache(maxsize=None)
def parity_reference(leaves, depth, budget):
    out = []
    for moves in OPENINGS:
        ref = _ref(moves, mixed, leaves, 1.0, depth, budget)
        ref.search(48)
        out.append(ref)
    return out


@pytest.mark.parametrize("leaves", [1, 4, 8])
@pytest.mark.parametrize("depth,budget", A.PARITY_SETTINGS)
def test_search_matches_the_restatement(leaves, depth, budget):
    import torch
    refs = parity_reference(leaves, depth, budget)
    if (depth, budget) == (8, 64):                               # the table's roots: lost, two replies, lost, one reply
        assert [ref.proof[0] for ref in refs[5:]] == [P.LOSES, P.NONE, P.LOSES, P.NONE] and sum(ref.searched for ref in refs) > 0
    tree = _tree(OPENINGS, leaves, 1.0, depth, budget)
    network = _host_network(mixed)
    kept = []

    def keeping(states):                                         # the caller's tensors: read, never written
        values, probs = network(states)
        kept.append((values, probs, values.clone(), probs.clone()))
        return values, probs
    tree.search(keeping, 48)
    torch.cuda.synchronize()
    for values, probs, v0, p0 in kept:
        assert torch.equal(values.view(torch.int32), v0.view(torch.int32)) and torch.equal(probs.view(torch.int32), p0.view(torch.int32))
    st = tree.root_stats()
    assert (st["root_visits"] == 48).all() and (st["status"] == 0).all()
    _same_all(tree, refs)
    tree.set_roots(*_roots(OPENINGS))                            # new roots: no bit, no count
    assert all(int(v.sum()) == 0 for v in tree.defend_stats().values()) and not tree.root_proofs()["children"].any()
    tree.close()


# ---------------- 2. per-leaf tables ----------------
def _positions(n):
    import random
    import vcf_reference as V
    rng = random.Random(11)
    pool = Z.TABLE + [Z.ONE_PLY_UP + [Z.ONE_PLY_UP_MOVE], A.WHITE_THREE_BLACK_TO_MOVE, A.QUIET, A.BLACK_THREE, A.HARD, FIVE, []]
    while len(pool) < n:
        moves = V.random_position(rng, rng.choice([14, 17, 20]), 3)
        if moves is not None:
            pool.append(moves)
    return pool[:n]


@pytest.mark.parametrize("n", [1, 3, 5, 17])
def test_root_tables_are_the_defence_solvers(n):
    positions = _positions(n)
    seen = set()
    for depth, budget in ((8, 64), (3, 2), (8, 3)):
        tree = _tree(positions, 1, 1.0, depth, budget)
        tree.select()
        seen |= _same_tables(tree, positions, depth, budget)
        tree.close()
    assert G.VCF_WIN in seen and (n < 3 or G.VCF_BUDGET in seen) and (n < 17 or G.VCF_NONE in seen)


# Branches of the shared walk (vcf_device.h) that the positions above do not take in the two K7 + K15 kernels; found and confirmed on
# tests/vcf_reference.py.  TANGLE at (8, 64): the threat's walk and a cell's search both meet a forced reply that makes two completing cells,
# a search starts from a root where the defender's stone did, and one runs out of budget.  At depth 1 a walk is cut at its root: the threat's
# on OPEN_THREE, and on CLOSED_FOUR the search of the one cell that blocks the four.
TANGLE = [65, 128, 144, 115, 110, 67, 85, 66, 141, 111, 83, 154, 143, 140, 98, 100, 69, 126, 159, 156, 95, 130, 113, 94]
CLOSED_FOUR = [110, 109, 111, 194, 112, 149, 113, 150, 210]      # black's four with one end closed, white to move


def test_root_tables_on_the_walks_rarer_branches():
    positions = [TANGLE, CLOSED_FOUR, Z.OPEN_THREE]
    for depth, budget, threats in ((8, 64, [G.VCF_WIN, G.VCF_WIN, G.VCF_WIN]), (1, 64, [G.VCF_DEPTH, G.VCF_WIN, G.VCF_DEPTH])):
        tree = _tree(positions, 1, 1.0, depth, budget)
        tree.select()
        _same_tables(tree, positions, depth, budget)
        got = tree.defend_verdicts()
        assert list(got["threat_status"]) == threats, (depth, budget)
        if depth == 1:                                           # every other cell loses at once; the block's search is cut: UNKNOWN, no node
            block = int(np.flatnonzero(got["verdict"][1] == D.CELL_UNKNOWN)[0])
            assert block == 114 and got["nodes"][1][block] == 0 and (got["verdict"][1] == D.CELL_LOSES).sum() == N - len(CLOSED_FOUR) - 1
        tree.close()


def test_tables_at_eight_leaves_on_one_game():
    tree = _tree([Z.OPEN_THREE], 8, 1.0)
    tree.add_playouts(20)
    tree.select()                                                # the root, then a collision: one pending leaf, seven rows without one
    assert _same_tables(tree, [Z.OPEN_THREE] + [None] * 7, 8, 64) == {G.VCF_WIN}
    values, probs = _host_network(R.uniform)(tree.states[:8])
    tree.expand(values, probs)
    tree.select()                                                # eight descents now: white's two holding replies and what follows them
    assert tree.defend_verdicts()["verdict"].shape == (8, N)
    values, probs = _host_network(R.uniform)(tree.states[:8])
    tree.expand(values, probs)
    assert tree.defend_stats()["marked"][0] == N - len(Z.OPEN_THREE) - 2
    tree.close()


def test_tables_after_a_game_has_ended():
    """Five games, the second ends with black's five: the leaf batch has four rows from then on, and rows 1 .. 3 belong to games 2 .. 4"""
    import torch
    openings = [Z.ONE_PLY_UP, R.OPEN_FOUR, Z.OPEN_THREE, A.QUIET, A.HARD]
    tree = _tree(openings, 1, 5.0)
    network = _host_network(peaked(Z.ONE_PLY_UP_MOVE))
    tree.search(network, 4)
    d_moves = torch.zeros((5, N), dtype=torch.uint8, device="cuda")
    for g, p in enumerate(openings):
        d_moves[g, :len(p)] = torch.tensor(p, dtype=torch.uint8)
    d_lens = torch.tensor([len(p) for p in openings], dtype=torch.int32, device="cuda")
    d_winner = torch.zeros(5, dtype=torch.int8, device="cuda")
    assert tree.advance(d_moves, None, d_lens, d_winner, reuse_subtree=False) == 4 and tree.live == 4
    moves, lens = d_moves.cpu().numpy(), d_lens.cpu().numpy()
    assert int(d_winner[1]) == 1 and int(moves[0, lens[0] - 1]) == Z.ONE_PLY_UP_MOVE
    positions = [[int(c) for c in moves[g, :lens[g]]] for g in (0, 2, 3, 4)]
    states = tree.select()                                       # fresh roots: the leaves are the roots
    assert states.shape[0] == 4
    assert G.VCF_WIN in _same_tables(tree, positions, 8, 64)     # game 0: white faces two open threes
    tree.expand(*network(states))
    pr = tree.root_proofs()
    assert pr["root"][0] == P.LOSES and not pr["root"][1]
    tree.close()


# ---------------- 3. re-rooting ----------------
@pytest.mark.parametrize("leaves", [1, 4])
def test_kept_subtrees_and_root_noise_across_three_moves(leaves):
    import torch
    openings = Z.TABLE + [Z.ONE_PLY_UP, A.HARD]
    refs = [_ref(moves, mixed, leaves, 1.0) for moves in openings]
    tree = _tree(openings, leaves, 1.0)
    tree.set_option(G.OPT_NOISE_SAMPLER, G.NOISE_SAMPLERS["counter"])
    network = _host_network(mixed)
    cells = torch.full((len(openings),), -7, dtype=torch.int16, device="cuda")
    carried = 0
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
        _same_all(tree, refs, "move %d" % move)
        tree.root_choice(cells)
        want = [ref.choice_cell() for ref in refs]
        assert cells.cpu().tolist() == want
        tree.step(None)
        for ref, cell in zip(refs, want):
            assert ref.reroot() == (cell if cell >= 0 else None)
        _same(tree.root_stats(), refs, "after step %d" % move)
        _same_proofs(tree, refs, "after step %d" % move)        # the marked children travel with the subtree
        carried += sum(ref.proof[0] != P.NONE or any(ref.root_proofs()["children"]) for ref in refs)
    assert carried > 0 and sum(ref.marked for ref in refs) > 0
    tree.close()


# ---------------- 4. the loops ----------------
def test_network_self_play_through_slots_and_on_both_loops():
    from gomokuai_amd.network import FusedPolicyValueNetwork, PolicyValueNetwork
    from helpers import PaddedNetwork
    net = FusedPolicyValueNetwork(PolicyValueNetwork(seed=8).cuda().eval())
    fused = PaddedNetwork(net, 11)
    # (the arena: forced replies keep the subtree nearly whole from move to move, three searches' worth is not enough)
    kw = dict(opening_plies=2, first_game_id=70, seed=2, root_noise=(0.05, 0.25), vcf=(8, 64), proof=True, vcf_defend=True, node_capacity=1 << 16)
    few = selfplay.play_network_games(11, fused, 12, slots=4, reuse_subtree=True, **kw).cpu()
    full = selfplay.play_network_games(11, fused, 12, slots=11, reuse_subtree=True, **kw).cpu()
    host = selfplay.play_network_games(11, fused, 12, reuse_subtree=True, device_loop=False, **kw).cpu()
    for other in (full, host):
        assert not few.overflow and not other.overflow
        assert (few.lens == other.lens).all() and (few.winner == other.winner).all() and int(few.lens.min()) >= 9
        for g in range(11):
            n = int(few.lens[g])
            assert n == N or int(few.winner[g]) != 0
            assert (few.moves[g, :n] == other.moves[g, :n]).all() and (few.visits[g, :n] == other.visits[g, :n]).all()
    net.close()


def test_evaluation_match_on_both_loops():
    from gomokuai_amd.network import FusedPolicyValueNetwork, PolicyValueNetwork
    from helpers import PaddedNetwork
    net = FusedPolicyValueNetwork(PolicyValueNetwork(seed=12).cuda().eval())
    fused = PaddedNetwork(net, 2 * 4)
    opponent = ("traditional_mcts", {"c_puct": 5.0, "c_iterations": 50})
    kw = dict(playouts=16, seed=9, first_game_id=40, leaves=4, vcf=(8, 64), proof=True, vcf_defend=True, node_capacity=1 << 16)
    (rd, bd, sd), (rh, bh, sh) = (selfplay.play_evaluation_games(4, fused, opponent, device_loop=loop, **kw) for loop in (True, False))
    cd, ch = rd.cpu(), rh.cpu()
    assert (bd == bh).all() and (sd == sh).all() and not rd.overflow and not rh.overflow
    assert (cd.lens == ch.lens).all() and (cd.winner == ch.winner).all()
    for g in range(4):
        k = int(cd.lens[g])
        assert (cd.moves[g, :k] == ch.moves[g, :k]).all() and (cd.visits[g, :k] == ch.visits[g, :k]).all(), g
    net.close()


# ---------------- 5. hipGraph ----------------
@pytest.mark.parametrize("leaves", [1, 4])
def test_a_captured_step_replays_the_search(leaves):
    import torch
    from gomokuai_amd.network import FusedPolicyValueNetwork, PolicyValueNetwork
    G.init()
    fused = FusedPolicyValueNetwork(PolicyValueNetwork(seed=4).cuda().eval())
    results = []
    for graph in (False, True):
        tree = _tree(OPENINGS, leaves, 5.0)
        with torch.no_grad():
            tree.search(fused, 40, graph=graph)
        torch.cuda.synchronize()
        results.append([tree.root_stats(), tree.root_proofs(), tree.proof_stats(), tree.vcf_stats(), tree.defend_stats()])
        tree.close()
    assert (results[0][0]["root_visits"] == 40).all() and results[0][4]["threatened"].sum() > 0 and results[0][4]["marked"].sum() > 0
    for eager, replayed in zip(*results):
        for k in eager:
            assert (eager[k].view(np.uint8) == replayed[k].view(np.uint8)).all(), k
    fused.close()


# ---------------- 6. the arena's edge ----------------
@pytest.mark.parametrize("leaves", [1, 4])
@pytest.mark.parametrize("short", [0, 1])
def test_the_threatened_leafs_children_at_the_arenas_last_node(leaves, short):
    root, move = Z.ONE_PLY_UP, Z.ONE_PLY_UP_MOVE
    cap = 1 + (N - len(root)) + (N - len(root) - 1) - short
    ref = _ref(root, peaked(move), leaves, 5.0, node_capacity=cap)
    ref.search(2)
    if short:
        assert ref.status == R.STATUS_ARENA_FULL and not any(ref.proof) and ref.marked == 0 and ref.threatened == 0
    else:
        assert ref.status == 0 and ref.n_nodes == cap and ref.proof[0] == P.WINS and ref.marked == N - len(root) - 1
    tree = _tree([root], leaves, 5.0, node_capacity=cap)
    tree.search(_host_network(peaked(move)), 2)
    _same_all(tree, [ref])
    tree.close()


# ---------------- 7. switching ----------------
@pytest.mark.parametrize("depth,proof", [(8, False), (0, True), (0, False)])
def test_inert_without_the_solver_or_without_proofs(depth, proof):
    network = _host_network(mixed)
    stats = []
    for defend in (False, True):
        tree = _tree(OPENINGS, 4, 1.0, depth, 64, proof=proof, defend=defend)
        tree.search(network, 32)
        stats.append([tree.root_stats(), tree.root_proofs(), tree.proof_stats(), tree.defend_stats()])
        if defend:
            with pytest.raises(G.GmkError):
                tree.defend_verdicts()                           # GMK_ERR_STATE: the option does not act
        tree.close()
    for off, on in zip(*stats):
        for k in off:
            assert (off[k].view(np.uint8) == on[k].view(np.uint8)).all(), k
    assert not stats[1][3]["threatened"].any() and not stats[1][3]["marked"].any()


@pytest.mark.parametrize("leaves", [1, 4])
def test_on_off_and_on_again(leaves):
    network = _host_network(mixed)
    openings = [Z.OPEN_THREE, Z.THREE_AND_THREE, Z.ONE_PLY_UP, A.HARD]
    refs = [_ref(moves, mixed, leaves, 1.0) for moves in openings]
    tree = _tree(openings, leaves, 1.0)
    for stage, on in enumerate((True, False, True)):
        tree.set_option(G.OPT_AZ_VCF_DEFEND, int(on))
        tree.search(network, 16)
        for ref in refs:
            ref.defend_on = on
            ref.search(16)
        _same_all(tree, refs, "stage %d" % stage)
    assert sum(ref.marked for ref in refs) > 0
    tree.close()


@pytest.mark.parametrize("leaves", [1, 4])
def test_misuse_is_refused_and_the_handle_goes_on(leaves):
    L = G.load()
    n = len(A.PARITY_OPENINGS)
    tree = _tree(A.PARITY_OPENINGS, leaves, 1.0, defend=False)
    for bad in (-1, 2, 7):
        assert L.gmk_az_set_option(tree.h, G.OPT_AZ_VCF_DEFEND, bad) == ERR_ARG
    assert L.gmk_az_set_option(tree.h, G.OPT_AZ_VCF_DEFEND, 1) == 0
    network = _host_network(R.sharpened)
    if leaves > 1:
        tree.add_playouts(1)
    states = tree.select()
    for value in (0, 1):
        assert L.gmk_az_set_option(tree.h, G.OPT_AZ_VCF_DEFEND, value) == ERR_STATE      # the marks are up / a select waits for its expand
    assert b"gmk_az_expand" in L.gmk_last_error()
    values, probs = network(states)
    tree.expand(values, probs)
    assert L.gmk_az_set_option(tree.h, G.OPT_AZ_VCF_DEFEND, 1) == 0
    assert L.gmk_az_defend_stats(None, None, None, None, None) == ERR_ARG and L.gmk_az_defend_verdicts_host(None, None, None, None, None) == ERR_ARG
    assert L.gmk_az_defend_stats(tree.h, None, None, None, None) == 0 and L.gmk_az_defend_verdicts_host(tree.h, None, None, None, None) == 0
    if leaves == 1:                                              # the host-driven one-leaf entries do not ask the defence solver
        tree.set_option(G.OPT_AZ_PROOF, 0)
        tree.set_option(G.OPT_AZ_VCF_DEPTH, 0)
        paths, lens = np.zeros((n, 226), np.int16), np.zeros(n, np.int32)
        hv, hp = values.cpu().numpy(), probs.cpu().numpy()
        assert L.gmk_az_select_host(tree.h, paths.ctypes.data, lens.ctypes.data) == ERR_STATE
        assert b"GMK_OPT_AZ_VCF_DEFEND" in L.gmk_last_error()
        assert L.gmk_az_expand_host(tree.h, hv.ctypes.data, hp.ctypes.data) == ERR_STATE
        assert L.gmk_az_set_leaf_host(tree.h, 0, 0, None, 0) == ERR_STATE
        assert L.gmk_az_expand_stages_host(tree.h, hv.ctypes.data, hp.ctypes.data, 1, 1) == ERR_STATE
        tree.set_option(G.OPT_AZ_VCF_DEFEND, 0)
        assert L.gmk_az_select_host(tree.h, paths.ctypes.data, lens.ctypes.data) == 0
        assert L.gmk_az_expand_host(tree.h, hv.ctypes.data, hp.ctypes.data) == 0
        tree.close()
        return
    tree.search(network, 15)
    assert (tree.root_stats()["root_visits"] == 16).all()
    tree.close()
