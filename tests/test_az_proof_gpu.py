"""K7 with proven wins and losses carried up the tree (GMK_OPT_AZ_PROOF: the <true> select, expand, step, advance and choice kernels) against
tests/az_proof_reference.py, the restatement tests/test_az_proof_reference.py holds to hand-checked facts and to a full minimax.  The network
is a host function of the batch, the numpy evaluator the restatement calls, so everything is compared exactly: visits, value and prior bits,
root statistics, tree size, status, the root's and its children's proofs, and the proved / stops counters."""
import functools

import numpy as np
import pytest

import az_leaves_reference as R
import az_proof_reference as P
import az_vcf_reference as A
from gomokuai_amd import lib as G
from gomokuai_amd import selfplay
from test_az_proof_reference import FIVE, cases
from test_az_vcf_gpu import _host_network, _roots, _same, _same_counters, far_rows

pytestmark = pytest.mark.gpu

N = 225
ERR_ARG, ERR_STATE = -3, -4


def mixed(states):
    """uniform on the nearly full fixture boards (every free cell gets a child: proofs by exhaustion), the peaked surrogate elsewhere"""
    return R.uniform(states) if int(np.asarray(states).reshape(6, N)[2].sum()) <= 6 else R.sharpened(states)


def parity_openings():
    return A.PARITY_OPENINGS + [c["moves"] for c in cases()["cases"] if c["chain"]]


@functools.lru_cache(maxsize=None)
def parity_reference(leaves, depth):
    out = []
    for moves in parity_openings():
        ref = P.ProofSearch(moves, mixed, depth, 64, proof=True, c_puct=1.0, leaves=leaves)
        ref.search(64)
        out.append(ref)
    return out


def _tree(openings, leaves, c_puct, depth, proof=True, node_capacity=1 << 16):
    G.init()
    tree = G.AlphaZeroMCTS(len(openings), node_capacity=node_capacity, c_puct=c_puct, leaves=leaves, vcf_depth=depth, vcf_budget=64, proof=proof)
    tree.set_roots(*_roots(openings))
    return tree


def _same_proofs(tree, refs, where=""):
    pr, ps = tree.root_proofs(), tree.proof_stats()
    for g, ref in enumerate(refs):
        want = ref.root_proofs()
        assert pr["root"][g] == want["root"], "%s game %d" % (where, g)
        np.testing.assert_array_equal(pr["children"][g], want["children"], "%s game %d" % (where, g))
        assert (ps["proved"][g], ps["stops"][g]) == (ref.proved, ref.stops), "%s game %d" % (where, g)


# ---------------- 1. parity with the restatement ----------------
@pytest.mark.parametrize("leaves", [1, 4, 8])
@pytest.mark.parametrize("depth", [0, 8])
def test_search_matches_the_restatement(leaves, depth):
    refs = parity_reference(leaves, depth)
    assert sum(ref.proved for ref in refs) > 3                   # (without the solver only the nearly full boards meet fives in 64 playouts)
    assert depth == 0 or (sum(ref.stops for ref in refs) > 0 and sum(ref.proof[0] == P.WINS for ref in refs) > 2)
    tree = _tree(parity_openings(), leaves, 1.0, depth)
    tree.search(_host_network(mixed), 64)
    st = tree.root_stats()
    assert (st["root_visits"] == 64).all() and (st["status"] == 0).all()
    _same(st, refs)
    _same_proofs(tree, refs)
    if depth:
        _same_counters(tree.vcf_stats(), refs)
    tree.set_roots(*_roots(parity_openings()))                   # new roots: no bit, no count
    pr, ps = tree.root_proofs(), tree.proof_stats()
    assert not pr["root"].any() and not pr["children"].any() and not ps["proved"].any() and not ps["stops"].any()
    tree.close()


@pytest.mark.parametrize("depth", [0, 8])
def test_an_open_four_between_the_descents_of_one_step(depth):
    """L = 8, uniform priors: the five is met and proven in the middle of a step, and the step's later descents stop at it"""
    ref = P.ProofSearch(R.OPEN_FOUR, R.uniform, depth, 64, proof=True, c_puct=5.0, leaves=8)
    ref.search(160)
    assert ref.proof[0] == P.WINS and ref.stops > 0 and ref.choice_cell() == FIVE
    tree = _tree([R.OPEN_FOUR], 8, 5.0, depth)
    tree.search(_host_network(R.uniform), 160)
    _same(tree.root_stats(), [ref])
    _same_proofs(tree, [ref])
    tree.close()


def faint_and_lost(states):
    """every leaf is lost for the side that moved into it, and the priors are too small to lift a score off -1.0 in float64"""
    return np.float32(1.0), np.full(N, np.float32(2.0) ** -100, dtype=np.float32)


@pytest.mark.parametrize("leaves", [1, 4])
@pytest.mark.parametrize("proof", [False, True])
def test_nothing_beats_the_initial_score(leaves, proof):
    """Boards with 2 .. 5 empty cells: once every child of a node has come back lost (Q = -1.0, or all in flight at L = 4) no score is
    above the -1.0 the maximum starts from, and the descent takes the first child.  The proof option runs the same search here (no five is
    met); it is the other instantiation of the descent."""
    from test_az_leaves_gpu import _late_boards
    refs = [P.ProofSearch(moves, faint_and_lost, 0, 64, proof=proof, c_puct=5.0, leaves=leaves) for moves in _late_boards()]
    for ref in refs:
        ref.search(40)
    assert all(ref.floor_picks > 0 for ref in refs) and not any(ref.proved for ref in refs)
    tree = _tree(_late_boards(), leaves, 5.0, 0, proof=proof)
    tree.search(_host_network(faint_and_lost), 40)
    st = tree.root_stats()
    assert (st["root_visits"] == 40).all() and (st["status"] == 0).all()
    _same(st, refs)
    _same_proofs(tree, refs)
    tree.close()


# ---------------- 2. the arena ----------------
@pytest.mark.parametrize("leaves", [1, 4])
def test_a_win_leaf_that_does_not_fit_gets_no_bit(leaves):
    """tests/test_az_vcf_gpu.py's arena of 256: the 108th WIN leaf fills it, the next one's child is dropped with its playout -- and its proof"""
    cap, playouts = 256, 120
    ref = P.ProofSearch(A.WHITE_THREE_BLACK_TO_MOVE, far_rows, 8, 64, proof=True, c_puct=5.0, leaves=leaves, node_capacity=cap)
    ref.search(playouts)
    assert ref.n_nodes == cap and ref.status == R.STATUS_ARENA_FULL and ref.wins > 108 and ref.proved == 108 and ref.proof[0] == P.NONE
    tree = _tree([A.WHITE_THREE_BLACK_TO_MOVE], leaves, 5.0, 8, node_capacity=cap)
    tree.search(_host_network(far_rows), playouts)
    _same(tree.root_stats(), [ref])
    _same_proofs(tree, [ref])
    assert int((tree.root_proofs()["children"][0] == P.WINS).sum()) == 108
    tree.close()


# ---------------- 3. re-rooting ----------------
@pytest.mark.parametrize("leaves", [1, 4])
def test_kept_subtrees_and_root_noise_across_three_moves(leaves):
    import torch
    openings = [A.QUIET, A.WHITE_THREE_BLACK_TO_MOVE, A.HARD, A.BLACK_THREE, R.OPEN_FOUR]
    refs = [P.ProofSearch(moves, R.sharpened, 8, 64, proof=True, c_puct=1.0, leaves=leaves) for moves in openings]
    tree = _tree(openings, leaves, 1.0, 8)
    tree.set_option(G.OPT_NOISE_SAMPLER, G.NOISE_SAMPLERS["counter"])
    network = _host_network(R.sharpened)
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
        _same(tree.root_stats(), refs, "move %d" % move)
        _same_proofs(tree, refs, "move %d" % move)
        tree.root_choice(cells)
        want = [ref.choice_cell() for ref in refs]
        assert cells.cpu().tolist() == want
        tree.step(None)
        for ref, cell in zip(refs, want):
            assert ref.reroot() == (cell if cell >= 0 else None)
        _same(tree.root_stats(), refs, "after step %d" % move)
        _same_proofs(tree, refs, "after step %d" % move)        # the bits travel with the subtree
        carried += sum(ref.proof[0] != P.NONE or any(ref.root_proofs()["children"]) for ref in refs)
    assert carried > 0 and sum(ref.stops for ref in refs) > 0
    tree.close()


@pytest.mark.parametrize("proof", [False, True])
def test_step_from_unvisited_children_takes_the_first(proof):
    """One playout expands the root and visits no child: the root choice has nothing to play, gmk_az_step(NULL) follows the first child
    (max_element over equal counts), and the next search shows which cell it was."""
    import torch
    openings = [R.OPENINGS[1], R.OPENINGS[2]]
    refs = [P.ProofSearch(moves, R.surrogate, 0, 64, proof=proof, c_puct=5.0) for moves in openings]
    for ref in refs:
        ref.search(1)
    assert all(ref.nkids[0] > 1 and ref.choice() == P.NO_NODE for ref in refs)
    tree = _tree(openings, 1, 5.0, 0, proof=proof)
    network = _host_network(R.surrogate)
    tree.search(network, 1)
    cells = torch.full((len(refs),), -7, dtype=torch.int16, device="cuda")
    tree.root_choice(cells)
    assert cells.cpu().tolist() == [-1] * len(refs)
    tree.step(None)
    for ref in refs:
        first = ref.cell[ref.first[0]]
        assert ref.reroot() == first and ref.n_nodes == 1
    _same(tree.root_stats(), refs, "after the step")
    tree.search(network, 8)
    for ref in refs:
        ref.search(8)
    _same(tree.root_stats(), refs, "the search after the step")
    tree.close()


def test_step_choice_and_advance_agree_on_a_losing_child():
    """The open four under uniform priors: the five's child is a proven loss for white and far from the most visited child."""
    import torch
    ref = P.ProofSearch(R.OPEN_FOUR, R.uniform, 0, 64, proof=True, c_puct=5.0)
    while not any(ref.proof):                                    # up to the playout that meets the five: every visited child has one visit
        ref.search(1)
    playouts = ref.visits[0]
    assert 100 < playouts <= 160 and ref.choice_cell() == FIVE and ref.cell[ref.plain_choice()] != FIVE
    network = _host_network(R.uniform)
    trees = [_tree([R.OPEN_FOUR], 1, 5.0, 0) for _ in range(2)]
    cells = torch.full((1,), -7, dtype=torch.int16, device="cuda")
    for tree in trees:
        tree.search(network, playouts)
        _same(tree.root_stats(), [ref])
        assert int(tree.root_stats()["visits"][0].argmax()) != FIVE
        tree.root_choice(cells)
        assert int(cells[0]) == FIVE
    trees[0].step(None)
    assert ref.reroot() == FIVE
    _same(trees[0].root_stats(), [ref])
    assert trees[0].root_proofs()["root"][0] == P.LOSES
    d_moves, d_lens = torch.zeros((1, N), dtype=torch.uint8, device="cuda"), torch.tensor([len(R.OPEN_FOUR)], dtype=torch.int32, device="cuda")
    d_moves[0, :len(R.OPEN_FOUR)] = torch.tensor(R.OPEN_FOUR, dtype=torch.uint8)
    d_winner = torch.zeros(1, dtype=torch.int8, device="cuda")
    assert trees[1].advance(d_moves, None, d_lens, d_winner, reuse_subtree=True) == 0
    assert int(d_moves[0, len(R.OPEN_FOUR)]) == FIVE and int(d_winner[0]) == 1 and int(d_lens[0]) == len(R.OPEN_FOUR) + 1
    off = _tree([R.OPEN_FOUR], 1, 5.0, 0, proof=False)           # the same search without the option: no bit, the old choice
    off.search(network, playouts)
    off.root_choice(cells)
    assert int(cells[0]) == int(off.root_stats()["visits"][0].argmax()) != FIVE and not off.root_proofs()["children"].any()
    for tree in trees + [off]:
        tree.close()


# ---------------- 4. the loops ----------------
def test_network_self_play_through_slots_and_on_both_loops():
    from gomokuai_amd.network import FusedPolicyValueNetwork, PolicyValueNetwork
    from helpers import PaddedNetwork
    net = FusedPolicyValueNetwork(PolicyValueNetwork(seed=8).cuda().eval())
    fused = PaddedNetwork(net, 11)
    kw = dict(opening_plies=2, first_game_id=70, seed=2, root_noise=(0.05, 0.25), vcf=(8, 64), proof=True)
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
    kw = dict(playouts=16, seed=9, first_game_id=40, leaves=4, vcf=(8, 64), proof=True)
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
    stats, proofs, counters = [], [], []
    for graph in (False, True):
        tree = _tree(A.PARITY_OPENINGS, leaves, 5.0, 8)
        with torch.no_grad():
            tree.search(fused, 40, graph=graph)
        torch.cuda.synchronize()
        stats.append(tree.root_stats())
        proofs.append(tree.root_proofs())
        counters.append(tree.proof_stats())
        tree.close()
    assert (stats[0]["root_visits"] == 40).all() and (stats[0]["status"] == 0).all() and counters[0]["proved"].sum() > 0 and counters[0]["stops"].sum() > 0
    for many in (stats, proofs, counters):
        for k in many[0]:
            assert (many[0][k].view(np.uint8) == many[1][k].view(np.uint8)).all(), k
    fused.close()


# ---------------- 6. option state ----------------
@pytest.mark.parametrize("leaves", [1, 4])
def test_on_off_and_on_again(leaves):
    """Off: the bits stay, are not read and not written.  On again: they are used."""
    network = _host_network(R.sharpened)
    openings = [A.BLACK_THREE, R.OPEN_FOUR, A.HARD]
    refs = [P.ProofSearch(moves, R.sharpened, 8, 64, proof=True, c_puct=1.0, leaves=leaves) for moves in openings]
    tree = _tree(openings, leaves, 1.0, 8)
    for stage, on in enumerate((True, False, True)):
        tree.set_option(G.OPT_AZ_PROOF, int(on))
        tree.search(network, 16)
        for ref in refs:
            ref.proof_on = on
            ref.search(16)
        _same(tree.root_stats(), refs, "stage %d" % stage)
        _same_proofs(tree, refs, "stage %d" % stage)
    assert sum(ref.proved for ref in refs) > 0 and sum(ref.stops for ref in refs) > 0
    tree.close()


@pytest.mark.parametrize("leaves", [1, 4])
def test_misuse_is_refused_and_the_handle_goes_on(leaves):
    L = G.load()
    tree = _tree(A.PARITY_OPENINGS, leaves, 1.0, 0, proof=False)
    n = len(A.PARITY_OPENINGS)
    for bad in (-1, 2, 3):
        assert L.gmk_az_set_option(tree.h, G.OPT_AZ_PROOF, bad) == ERR_ARG
    assert L.gmk_az_set_option(tree.h, G.OPT_AZ_PROOF, 1) == 0
    network = _host_network(R.sharpened)
    if leaves > 1:
        tree.add_playouts(1)
    states = tree.select()
    for value in (0, 1):
        assert L.gmk_az_set_option(tree.h, G.OPT_AZ_PROOF, value) == ERR_STATE       # the marks are up / a select waits for its expand
    assert b"gmk_az_expand" in L.gmk_last_error()
    values, probs = network(states)
    tree.expand(values, probs)
    assert L.gmk_az_set_option(tree.h, G.OPT_AZ_PROOF, 1) == 0
    assert L.gmk_az_root_proofs(None, None, None) == ERR_ARG and L.gmk_az_proof_stats(None, None, None) == ERR_ARG
    if leaves == 1:                                              # the host-driven one-leaf entries carry no proofs
        paths, lens = np.zeros((n, 226), np.int16), np.zeros(n, np.int32)
        hv, hp = values.cpu().numpy(), probs.cpu().numpy()
        assert L.gmk_az_select_host(tree.h, paths.ctypes.data, lens.ctypes.data) == ERR_STATE
        assert b"GMK_OPT_AZ_PROOF" in L.gmk_last_error()
        assert L.gmk_az_expand_host(tree.h, hv.ctypes.data, hp.ctypes.data) == ERR_STATE
        assert L.gmk_az_set_leaf_host(tree.h, 0, 0, None, 0) == ERR_STATE
        assert L.gmk_az_expand_stages_host(tree.h, hv.ctypes.data, hp.ctypes.data, 1, 1) == ERR_STATE
        tree.set_option(G.OPT_AZ_PROOF, 0)
        assert L.gmk_az_select_host(tree.h, paths.ctypes.data, lens.ctypes.data) == 0
        assert L.gmk_az_expand_host(tree.h, hv.ctypes.data, hp.ctypes.data) == 0
        tree.close()
        return
    tree.search(network, 15)
    assert (tree.root_stats()["root_visits"] == 16).all()
    tree.close()
