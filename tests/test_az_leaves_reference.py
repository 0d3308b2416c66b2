"""tests/az_leaves_reference.py held to account, on the CPU: at one leaf per step it is the oracle's MCTS with an external evaluator bit for
bit; with several leaves it completes exactly the playouts asked for and leaves no in-flight mark behind; and the inputs of the GPU parity
test (tests/test_az_leaves_gpu.py) really exercise what several leaves add -- collisions, trees of some depth, visit rows that differ from
the one-leaf search.  Plus the host-side plumbing that needs no GPU: the binding's constants and the evaluation schedule's setting."""
import ctypes as C
import functools

import numpy as np
import pytest

import az_leaves_reference as R
from gomokuai_amd import lib as G
from gomokuai_amd import selfplay
from gomokuai_amd.training import EvaluationSchedule, TrainingLoop


def test_one_leaf_is_the_oracles_search(oracle):
    O = oracle
    playouts = 160
    assert sorted(len(m) for m in R.OPENINGS) == [0, 2, 3, 6, 9, 12]
    for moves in R.OPENINGS:
        b = O.new_board()
        for c in moves:
            O.lib().go_board_apply(C.byref(b), int(c), 1)
        om = O.MCTS(playouts, 5.0, 5, 0, 0)
        om.set_evaluator(R.surrogate)
        om.run_playouts(b)
        v, q, p = om.root_children()
        ref = R.LeavesSearch(moves, R.surrogate, c_puct=5.0, leaves=1)
        ref.search(playouts)
        st = ref.root_stats()
        np.testing.assert_array_equal(st["visits"], v)
        np.testing.assert_array_equal(st["values"].view(np.uint32), q.view(np.uint32))
        np.testing.assert_array_equal(st["priors"].view(np.uint32), p.view(np.uint32))
        assert st["root_visits"] == om.root_visits == playouts and st["n_nodes"] == om.size and st["status"] == 0
        assert np.float32(st["root_value"]).view(np.uint32) == np.float32(om.root_value).view(np.uint32)
        assert ref.steps == playouts and ref.collisions == 0 and set(ref.leaves_per_step) <= {0, 1}


@functools.lru_cache(maxsize=None)
def _sharpened(leaves, playouts):
    out = []
    for moves in R.OPENINGS:
        ref = R.LeavesSearch(moves, R.sharpened, c_puct=1.0, leaves=leaves)
        ref.search(playouts)
        out.append(ref)
    return out


@pytest.mark.parametrize("leaves", [2, 4, 8])
@pytest.mark.parametrize("playouts", [50, 96])
def test_counts(leaves, playouts):
    for ref in _sharpened(leaves, playouts):
        st = ref.root_stats()
        assert st["root_visits"] == playouts and ref.quota == 0 and st["status"] == 0
        assert not any(ref.inflight) and not ref.pending
        assert sum(ref.leaves_per_step) + ref.terminal_playouts == playouts and max(ref.leaves_per_step) <= leaves
        assert ref.steps >= -(-playouts // leaves)
        assert int(st["visits"].sum()) == playouts - 1               # every playout but the root's own went through a root child


@pytest.mark.parametrize("leaves", [4, 8])
def test_the_parity_inputs_cover_what_leaves_add(leaves):
    """Conditions on the GPU parity test's inputs (the sharpened evaluator at c_puct = 1, 96 playouts), asserted here where they are cheap.
    The plain surrogate would not do: it is so flat that every playout opens a new root child and all leaves counts give the same row."""
    one = _sharpened(1, 96)
    many = _sharpened(leaves, 96)
    assert sum(ref.collisions for ref in many) >= 1                   # at least one step cut short by a collision
    assert all(min(ref.leaves_per_step) < leaves for ref in many)
    assert all(ref.max_depth >= 3 for ref in many)                    # descents of at least three plies below the root
    differ = sum(int((a.root_stats()["visits"] != b.root_stats()["visits"]).any()) for a, b in zip(one, many))
    assert differ >= len(R.OPENINGS) // 2                             # and not the one-leaf search's visit rows
    flat_one = R.LeavesSearch(R.OPENINGS[1], R.surrogate, c_puct=5.0, leaves=1)
    flat_many = R.LeavesSearch(R.OPENINGS[1], R.surrogate, c_puct=5.0, leaves=leaves)
    flat_one.search(96), flat_many.search(96)
    assert (flat_one.root_stats()["visits"] == flat_many.root_stats()["visits"]).all() and flat_many.max_depth < min(ref.max_depth for ref in many)


def test_terminal_leaves_are_backed_up_inside_a_step():
    won = R.LeavesSearch(R.WON, R.uniform, leaves=8)
    won.search(40)
    st = won.root_stats()
    assert st["root_visits"] == 40 and st["root_value"] == 1.0 and st["n_nodes"] == 1 and won.terminal_playouts == 40 and won.steps == 5
    for leaves in (4, 8):
        four = R.LeavesSearch(R.OPEN_FOUR, R.uniform, c_puct=5.0, leaves=leaves)
        four.search(160)
        assert four.root_stats()["root_visits"] == 160 and four.terminal_playouts > 0 and not any(four.inflight)


def test_dropped_playouts_give_their_marks_back():
    ref = R.LeavesSearch([112, 113, 127], R.sharpened, c_puct=1.0, leaves=4, node_capacity=256)
    ref.search(40)
    st = ref.root_stats()
    assert st["status"] & R.STATUS_ARENA_FULL and st["n_nodes"] <= 256 and st["root_visits"] < 40 and ref.quota == 0 and not any(ref.inflight)


def test_rerooting_keeps_the_subtree():
    ref = R.LeavesSearch(R.OPENINGS[2], R.sharpened, c_puct=1.0, leaves=4)
    ref.search(64)
    st = ref.root_stats()
    best = int(st["visits"].argmax())
    kept_visits, kept_value = st["visits"][best], st["values"][best]
    assert ref.reroot() == best and ref.moves == R.OPENINGS[2] + [best]
    after = ref.root_stats()
    assert after["root_visits"] == kept_visits and after["root_value"] == kept_value and after["n_nodes"] < st["n_nodes"]
    assert all(ref.parent[i] < i for i in range(1, ref.n_nodes))
    free = next(c for c in range(225) if c not in ref.moves and after["visits"][c] == 0 and after["priors"][c] == 0)
    assert ref.reroot(free) == free and ref.n_nodes == 1 and ref.root_stats()["root_visits"] == 0       # not a child: a new node
    assert ref.reroot(free) is None and ref.status & R.STATUS_ILLEGAL_STEP


def test_the_binding_names_the_option():
    assert G.OPT_AZ_LEAVES == 3 and G.AZ_MAX_LEAVES == 8
    assert "gmk_az_add_playouts" in G.EXPORTS and "gmk_az_playouts_owed" in G.EXPORTS
    L = G.load()
    assert hasattr(L, "gmk_az_add_playouts") and hasattr(L, "gmk_az_playouts_owed")


class _Replay:
    def sample(self, batch_size):
        return "states", "values", "pi"


class _Trainer:
    max_batch = 64

    def train_step(self, *a):
        return 1.0, 2.0, 0.02, 3

    def export(self, fused):
        pass


def test_the_schedule_hands_leaves_to_the_match(monkeypatch):
    asked = []

    def match(n_games, network, opponent, playouts=400, **kw):
        asked.append(kw)
        return None, selfplay.evaluation_sides(n_games), np.full(n_games, 0.5)
    monkeypatch.setattr(selfplay, "play_evaluation_games", match)
    for sch, options, want in ((EvaluationSchedule(eval_rounds=2, leaves=4), {"max_moves": 9}, {"max_moves": 9, "leaves": 4}),
                               (EvaluationSchedule(eval_rounds=2), {"max_moves": 9}, {"max_moves": 9}),
                               (EvaluationSchedule(eval_rounds=2, leaves=4), {"leaves": 2}, {"leaves": 2})):
        loop = TrainingLoop(_Replay(), _Trainer(), object(), batch_size=8, eval_period=1, schedule=sch, eval_options=options)
        loop.step()
        assert asked[-1] == want
    with pytest.raises(ValueError):
        EvaluationSchedule(leaves=9)
