"""tests/az_vcf_reference.py held to facts that can be checked by hand, on the CPU, and the inputs of the GPU parity test
(tests/test_az_vcf_gpu.py) shown to reach what the solver adds: WIN leaves below the root and leaves cut by the budget.  Plus the plumbing that
needs no GPU: the schedule's setting."""
import functools

import numpy as np
import pytest

import az_leaves_reference as R
import az_vcf_reference as A
import vcf_reference as V
from gomokuai_amd import selfplay
from gomokuai_amd.training import EvaluationSchedule, TrainingLoop


@functools.lru_cache(maxsize=None)
def parity_reference(leaves, depth, budget):
    """The searches the GPU parity test compares with (5 games, 48 playouts, c_puct = 1, R.sharpened); tests/test_az_vcf_gpu.py imports it."""
    out = []
    for moves in A.PARITY_OPENINGS:
        ref = A.VcfLeavesSearch(moves, R.sharpened, depth, budget, c_puct=1.0, leaves=leaves)
        ref.search(48)
        out.append(ref)
    return out


@pytest.mark.parametrize("moves", [A.BLACK_THREE, A.WHITE_THREE])
@pytest.mark.parametrize("leaves", [1, 4])
def test_the_side_that_holds_the_open_three_wins_at_the_root(moves, leaves):
    playouts = 24
    ref = A.VcfLeavesSearch(moves, R.sharpened, 8, 64, c_puct=1.0, leaves=leaves)
    assert (len(moves) % 2 == 1) == (moves is A.WHITE_THREE)                 # a white-to-move root attacks as white
    ref.search(1)
    st = ref.root_stats()
    assert ref.verdicts[0]["status"] == V.WIN and ref.verdicts[0]["pv"] == [4, 3, 8] and ref.verdicts[0]["nodes"] == 4
    assert st["n_nodes"] == 2 and st["priors"][4] == 1.0 and int((st["priors"] != 0).sum()) == 1
    assert st["root_visits"] == 1 and st["root_value"] == -1.0               # -(+1) goes up: the node's value is the mover-before's
    ref.search(playouts - 1)
    st = ref.root_stats()
    assert st["root_visits"] == playouts and st["visits"][4] == playouts - 1 and int(st["visits"].sum()) == playouts - 1
    assert ref.quota == 0 and not any(ref.inflight) and st["status"] == 0


def test_white_to_move_does_not_take_blacks_three():
    """The same stones with the colours' turn swapped: the side to move holds nothing, so the root is the network's."""
    black_holds_white_moves = A.BLACK_THREE + [A.FAR[3]]
    ref = A.VcfLeavesSearch(black_holds_white_moves, R.sharpened, 8, 64, c_puct=1.0)
    ref.search(1)
    assert ref.verdicts[0]["status"] == V.NONE and ref.n_nodes > 2 and ref.wins == 0


@pytest.mark.parametrize("leaves", [1, 4])
def test_depth_zero_is_the_leaves_search(leaves):
    for moves in (A.BLACK_THREE, A.HARD, A.QUIET):
        a = A.VcfLeavesSearch(moves, R.sharpened, 0, 64, c_puct=1.0, leaves=leaves)
        b = R.LeavesSearch(moves, R.sharpened, c_puct=1.0, leaves=leaves)
        a.search(40), b.search(40)
        sa, sb = a.root_stats(), b.root_stats()
        for k in sa:
            assert (np.asarray(sa[k]) == np.asarray(sb[k])).all(), k
        assert a.solved == 0 and a.visits == b.visits and a.cell == b.cell


def test_a_budget_too_small_leaves_the_row_to_the_network():
    ref = A.VcfLeavesSearch(A.BLACK_THREE, R.sharpened, 8, 3, c_puct=1.0)      # the win costs four nodes
    plain = R.LeavesSearch(A.BLACK_THREE, R.sharpened, c_puct=1.0)
    ref.search(1), plain.search(1)
    assert ref.verdicts[0]["status"] == V.BUDGET and ref.verdicts[0]["nodes"] == 3 and (ref.solved, ref.wins, ref.cut, ref.nodes) == (1, 0, 1, 3)
    assert ref.n_nodes == plain.n_nodes > 2 and ref.prior == plain.prior and ref.value == plain.value
    enough = A.VcfLeavesSearch(A.BLACK_THREE, R.sharpened, 8, 4, c_puct=1.0)
    enough.search(1)
    assert enough.verdicts[0]["status"] == V.WIN and enough.n_nodes == 2
    shallow = A.VcfLeavesSearch(A.BLACK_THREE, R.sharpened, 1, 64, c_puct=1.0)
    shallow.search(1)
    assert shallow.verdicts[0]["status"] == V.DEPTH and shallow.cut == 1 and shallow.n_nodes == plain.n_nodes


def test_an_open_four_is_won_in_one():
    ref = A.VcfLeavesSearch(R.OPEN_FOUR, R.uniform, 8, 64, c_puct=5.0, leaves=4)
    ref.search(30)
    st = ref.root_stats()
    five = R.OPEN_FOUR[0] - 1                                                # the lower end of the four
    assert ref.verdicts == [] or ref.verdicts[0]["status"] == V.WIN
    assert st["n_nodes"] == 2 and st["priors"][five] == 1.0 and st["visits"][five] == 29 and ref.terminal_playouts == 29 and ref.solved == 1


@pytest.mark.parametrize("leaves", [1, 4])
def test_the_parity_inputs_reach_what_the_solver_adds(leaves):
    """So that the GPU parity cannot pass emptily: WIN leaves strictly below the root, leaves cut by the budget, a root the network keeps."""
    for depth, budget in A.PARITY_SETTINGS:
        refs = parity_reference(leaves, depth, budget)
        assert all(ref.root_stats()["root_visits"] == 48 and ref.quota == 0 and not any(ref.inflight) for ref in refs)
        assert sum(ref.wins_below_root for ref in refs) >= 2
        assert sum(ref.budget_leaves for ref in refs) >= 2
        assert refs[0].solved == 48 and refs[0].wins == 0                    # the quiet game: every leaf solved, none won
        assert refs[3].solved == 1 and refs[3].wins == 1                     # the open four: the root, then fives
    deep, tight = parity_reference(leaves, 8, 64), parity_reference(leaves, 3, 2)
    assert deep[4].verdicts is not None and deep[4].budget_leaves >= 1 and deep[4].wins_below_root >= 1     # the hard one: over budget at the root, won below it
    assert deep[1].wins > tight[1].wins == 0                                 # two nodes do not find the three's win
    assert [ref.n_nodes for ref in deep] != [ref.n_nodes for ref in tight]


class _Replay:
    def sample(self, batch_size):
        return "states", "values", "pi"


class _Trainer:
    max_batch = 64

    def train_step(self, *a):
        return 1.0, 2.0, 0.02, 3

    def export(self, fused):
        pass


def test_the_schedule_hands_vcf_to_the_match(monkeypatch):
    asked = []

    def match(n_games, network, opponent, playouts=400, **kw):
        asked.append(kw)
        return None, selfplay.evaluation_sides(n_games), np.full(n_games, 0.5)
    monkeypatch.setattr(selfplay, "play_evaluation_games", match)
    for sch, options, want in ((EvaluationSchedule(eval_rounds=2, vcf=(16, 64)), {"max_moves": 9}, {"max_moves": 9, "vcf": (16, 64)}),
                               (EvaluationSchedule(eval_rounds=2), {"max_moves": 9}, {"max_moves": 9}),
                               (EvaluationSchedule(eval_rounds=2, leaves=4, vcf=(8, 32)), {"vcf": None}, {"leaves": 4, "vcf": None})):
        loop = TrainingLoop(_Replay(), _Trainer(), object(), batch_size=8, eval_period=1, schedule=sch, eval_options=options)
        loop.step()
        assert asked[-1] == want
    for bad in ((0, 64), (33, 64), (8, 0), (8,)):
        with pytest.raises(ValueError):
            EvaluationSchedule(vcf=bad)
    assert selfplay._vcf_options(None) == {} and selfplay._vcf_options((8, 32)) == {"vcf_depth": 8, "vcf_budget": 32}
