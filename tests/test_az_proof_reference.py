"""tests/az_proof_reference.py held to facts that can be checked by hand and, on nearly full boards, to a full minimax: on the CPU.  The GPU
parity test (tests/test_az_proof_gpu.py) compares the kernels with this restatement, so what is shown here is shown of them."""
import functools
import json
import os

import numpy as np
import pytest

import az_leaves_reference as R
import az_proof_reference as P
import az_vcf_reference as A

HERE = os.path.dirname(os.path.abspath(__file__))
FIVE = R.OPEN_FOUR[0] - 1                                        # the lower end of the open four; the upper one is OPEN_FOUR[6] + 1


@functools.lru_cache(maxsize=None)
def cases():
    with open(os.path.join(HERE, "golden", "az_proof_cases.json")) as fh:
        return json.load(fh)


def same_tree(a, b):
    for k in ("visits", "value", "prior", "parent", "first", "nkids", "cell", "inflight"):
        assert getattr(a, k) == getattr(b, k), k
    assert (a.status, a.quota, a.steps, a.leaves_per_step, a.terminal_playouts, a.collisions) == (b.status, b.quota, b.steps, b.leaves_per_step, b.terminal_playouts, b.collisions)
    assert (a.solved, a.wins, a.cut, a.nodes) == (b.solved, b.wins, b.cut, b.nodes)


@pytest.mark.parametrize("leaves", [1, 4])
@pytest.mark.parametrize("depth", [0, 8])
def test_proof_off_is_the_vcf_search(leaves, depth):
    for moves in (A.BLACK_THREE, R.OPEN_FOUR, A.QUIET, A.HARD):
        a = P.ProofSearch(moves, R.sharpened, depth, 64, proof=False, c_puct=1.0, leaves=leaves)
        b = A.VcfLeavesSearch(moves, R.sharpened, depth, 64, c_puct=1.0, leaves=leaves)
        a.search(40), b.search(40)
        same_tree(a, b)
        assert not any(a.proof) and (a.proved, a.stops) == (0, 0)
        assert a.reroot() == b.reroot()
        a.search(10), b.search(10)
        same_tree(a, b)


@pytest.mark.parametrize("leaves", [1, 4])
def test_a_quiet_position_sets_no_bit(leaves):
    a = P.ProofSearch(A.QUIET, R.sharpened, 8, 64, proof=True, c_puct=1.0, leaves=leaves)
    b = A.VcfLeavesSearch(A.QUIET, R.sharpened, 8, 64, c_puct=1.0, leaves=leaves)
    a.search(48), b.search(48)
    same_tree(a, b)
    assert not any(a.proof) and (a.proved, a.stops) == (0, 0) and a.choice() == a.plain_choice()


def test_an_open_four_is_proven_at_the_first_five():
    """uniform priors, c_puct = 5: the root's 217 children are visited in cell order, the five at cell FIVE = 110 included.  No solver."""
    s = P.ProofSearch(R.OPEN_FOUR, R.uniform, 0, 64, proof=True, c_puct=5.0)
    while not any(s.proof):
        before = s.n_nodes
        s.search(1)
    kid = next(i for i in range(s.first[0], s.first[0] + s.nkids[0]) if s.cell[i] == FIVE)
    assert s.n_nodes == before and s.visits[kid] == 1             # the five's node was proven at its first visit, by a descent that ended there
    assert s.proof[kid] == P.LOSES and s.proof[0] == P.WINS and s.proved == 2 and s.stops == 0
    playouts = s.visits[0]
    most = s.plain_choice()
    assert s.cell[most] != FIVE and s.visits[most] >= s.visits[kid]          # the completing cell is not the most visited child ...
    assert s.choice() == kid and s.choice_cell() == FIVE          # ... and is the choice
    s.search(25)                                                  # every later playout takes the LOSES child and stops there
    assert s.n_nodes == before and s.stops == 25 and s.visits[kid] == 26 and s.visits[0] == playouts + 25
    assert s.value[kid] == np.float32(1.0) and s.terminal_playouts == 1
    pr = s.root_proofs()
    assert pr["root"] == P.WINS and pr["children"][FIVE] == P.LOSES and int((pr["children"] != 0).sum()) == 1
    assert s.reroot() == FIVE and s.proof[0] == P.LOSES           # the bit travels with the child


@pytest.mark.parametrize("leaves", [1, 4, 8])
def test_an_open_four_between_the_descents_of_one_step(leaves):
    s = P.ProofSearch(R.OPEN_FOUR, R.uniform, 0, 64, proof=True, c_puct=5.0, leaves=leaves)
    s.search(160)
    kid = next(i for i in range(s.first[0], s.first[0] + s.nkids[0]) if s.cell[i] == FIVE)
    assert s.proof[kid] == P.LOSES and s.proof[0] == P.WINS and s.stops > 0 and s.visits[0] == 160 and not any(s.inflight) and s.quota == 0
    assert s.choice_cell() == FIVE


@pytest.mark.parametrize("moves", [A.BLACK_THREE, A.WHITE_THREE])
@pytest.mark.parametrize("leaves", [1, 4])
def test_the_solvers_win_proves_the_root(moves, leaves):
    """Rule (b) at the root; uniform priors, so that the single child gets a child for every free cell and can be proven by exhaustion."""
    s = P.ProofSearch(moves, R.uniform, 8, 64, proof=True, c_puct=5.0, leaves=leaves)
    s.search(1)
    assert s.n_nodes == 2 and s.proof == [P.WINS, P.NONE] and s.proved == 1 and s.cell[1] == 4
    replies = 225 - len(moves) - 1
    s.search(replies)                                             # the child's own expansion, then every reply but one: each a WIN leaf
    assert s.nkids[1] == replies and s.proof[1] == P.NONE and s.proved == replies and s.stops == 0
    assert sum(s.proof[i] == P.WINS for i in range(s.first[1], s.first[1] + replies)) == replies - 1
    s.search(1)
    assert s.proof[1] == P.LOSES and s.proved == replies + 2 and s.proof[0] == P.WINS      # the last reply: the child loses against every move
    s.search(5)
    assert s.stops == 5 and s.visits[0] == replies + 7 and s.quota == 0 and not any(s.inflight) and s.proved == replies + 2


def test_a_dropped_free_cell_keeps_the_parent_unproven():
    """An evaluator that gives some free cells a zero probability: every child WINS does not prove the parent."""
    moves = A.WHITE_THREE_BLACK_TO_MOVE                          # white wins below every black reply that does not block

    def two_cells(states):
        p = np.zeros(225, dtype=np.float32)
        p[[100, 101]] = np.float32(0.5)                          # far from the three: white's win stands
        return np.float32(0.0), p
    s = P.ProofSearch(moves, two_cells, 8, 64, proof=True, c_puct=1.0)
    s.search(12)
    kids = range(s.first[0], s.first[0] + s.nkids[0])
    assert [s.cell[i] for i in kids] == [100, 101] and all(s.proof[i] == P.WINS for i in kids)
    assert s.proof[0] == P.NONE and s.proved == 2 and s.stops == 12 - 3 and s.choice() == s.plain_choice()


def _check_bits(s):
    """every proof bit of the tree against the minimax of its node's position -> the number of bits"""
    bits = 0
    for i in range(s.n_nodes):
        if s.proof[i] != P.NONE:
            bits += 1
            assert P.minimax(s.moves + s.path_to(i)) == (1 if s.proof[i] == P.WINS else -1), (i, s.proof[i])
    return bits


def test_soundness_by_brute_force():
    data = cases()
    seen = {"exhaustion": 0, "chain": 0, "choice": 0}
    assert [tuple(x) for x in data["settings"]] == [(1, 0), (4, 0), (1, 8), (4, 8)]
    for case in data["cases"]:
        moves = case["moves"]
        assert 225 - len(moves) <= 6 and P.minimax(moves) == case["minimax"]
        for leaves, depth in data["settings"]:
            s = P.ProofSearch(moves, R.uniform, depth, 64, proof=True, c_puct=data["c_puct"], leaves=leaves)
            s.search(data["playouts"])
            assert _check_bits(s) == s.proved and s.visits[0] == data["playouts"]
            for i in range(s.n_nodes):
                p = s.parent[i]
                seen["exhaustion"] += s.proof[i] == P.LOSES and s.nkids[i] > 0
                seen["chain"] += s.proof[i] != P.NONE and p != P.NO_NODE and s.proof[p] != P.NONE and s.parent[p] != P.NO_NODE and s.proof[s.parent[p]] != P.NONE
            seen["choice"] += s.choice() != s.plain_choice()
    assert seen["exhaustion"] > 0 and seen["chain"] > 0 and seen["choice"] > 0, seen


def test_the_schedule_and_the_loops_take_proof():
    import inspect
    from gomokuai_amd import selfplay
    from gomokuai_amd.training import EvaluationSchedule
    assert EvaluationSchedule().proof is False and EvaluationSchedule(proof=True).proof is True
    for fn in (selfplay.play_network_games, selfplay.play_evaluation_games):
        assert inspect.signature(fn).parameters["proof"].default is False
    visits = np.zeros((3, 225), np.uint32)
    visits[0, [5, 9]], visits[1, [5, 9]], visits[2, 7] = (3, 8), (3, 8), 2
    proofs = np.zeros((3, 225), np.int8)
    proofs[0, 5], proofs[1, 9] = P.LOSES, P.WINS
    assert list(selfplay._root_choice(visits, None)) == [9, 9, 7]
    assert list(selfplay._root_choice(visits, proofs)) == [5, 5, 7]
    proofs[2, 7] = P.WINS
    assert list(selfplay._root_choice(visits, proofs)) == [5, 5, 7]          # nothing else has a visit: the old rule
    assert list(selfplay._root_choice(np.zeros((1, 225), np.uint32), proofs[:1])) == [5] and list(selfplay._root_choice(np.zeros((1, 225), np.uint32), None)) == [-1]
