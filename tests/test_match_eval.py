"""The evaluation match without a GPU: the win-rate schedule (training.EvaluationSchedule) against a restatement of the reference's
rules, the score arithmetic and side alternation of selfplay.play_evaluation_games, TrainingLoop's switch, and the header."""
import os
import re

import numpy as np
import pytest

from gomokuai_amd import selfplay, training
from gomokuai_amd.training import EvaluationSchedule, TrainingLoop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class ReferenceSchedule:
    """network/train.py:30-32, 93-99, 105-123, restated: the state and the update of evaluate_network.  candidates[level] None = the
    supervisor; every agent here is an MCTS agent by name.  The last level stays where the reference would index past its list."""

    def __init__(self, candidates, supervisor, c_iterations):
        self.candidates, self.supervisor, self.c_iterations = candidates, supervisor, c_iterations
        self.schedule_level, self.ref_iterations, self.best_win_rate = 0, c_iterations, 0.0

    def update(self, win_rate):
        meta = self.candidates[self.schedule_level]
        if meta is None:
            meta = self.supervisor
        is_mcts = "mcts" in meta[0]
        saved = None
        if win_rate > self.best_win_rate:
            saved = "best_model-{}-{}".format(meta[0], self.ref_iterations)
            if win_rate >= 1.0 - 0.05 * self.schedule_level:
                if is_mcts:
                    self.ref_iterations += 2 * self.c_iterations
                if not is_mcts or self.ref_iterations > 20000:
                    self.ref_iterations = self.c_iterations
                    if self.schedule_level + 1 < len(self.candidates):
                        self.schedule_level += 1
                self.best_win_rate = 0.0
            else:
                self.best_win_rate = win_rate
        return saved


def _script():
    """(win rate, what the step is there to cross)"""
    s = [(0.3, "a plain new best"), (0.2, "no improvement"), (0.3, "equal is no improvement")]
    s += [(1.0, "level-up at the iteration step")] * 24
    s += [(1.0, "the 25th level-up in a row: 20 400 > 20 000, back to 400 and on to level 1")]
    s += [(0.94, "level 1: below the decayed threshold"), (0.95, "level 1: at the decayed threshold")]
    s += [(1.0, "power-ups of level 1")] * 23
    s += [(1.0, "on to the last level")]
    s += [(0.5, "last level: a new best"), (0.9, "last level: level-up at 1 - 0.05 * 2")]
    s += [(1.0, "power-ups of the last level")] * 23
    s += [(1.0, "the wrap at the last level: it stays")]
    s += [(0.1, "after the wrap")]
    return s


def test_schedule_follows_the_reference_rules():
    sch = EvaluationSchedule()
    assert sch.eval_rounds == 11 and sch.c_iterations == 400 and [c and c[0] for c in sch.candidates] == ["random_mcts", "rave_mcts", None]
    ref = ReferenceSchedule(list(training.CANDIDATES), training.SUPERVISOR, 400)
    seen = {}
    for i, (rate, what) in enumerate(_script()):
        before = (sch.schedule_level, sch.ref_iterations)
        name, kwargs = sch.opponent()
        expect = ref.candidates[ref.schedule_level] or ref.supervisor
        assert name == expect[0] and kwargs["c_iterations"] == ref.ref_iterations and kwargs["c_puct"] == expect[1]["c_puct"]
        saved = ref.update(rate)
        events = sch.update(rate)
        assert (sch.schedule_level, sch.ref_iterations, sch.best_win_rate) == (ref.schedule_level, ref.ref_iterations, ref.best_win_rate), (i, what)
        assert events["new_best"] == (saved is not None), (i, what)
        assert events["level_up"] == (saved is not None and ref.best_win_rate == 0.0 and rate > 0), (i, what)
        assert events["next_candidate"] == (sch.schedule_level != before[0]), (i, what)
        seen[what] = (before, (sch.schedule_level, sch.ref_iterations, sch.best_win_rate), events)
    # the script did cross what it was written to cross
    assert seen["a plain new best"][1] == (0, 400, 0.3) and seen["a plain new best"][2]["new_best"] and not seen["a plain new best"][2]["level_up"]
    assert seen["no improvement"][1] == (0, 400, 0.3) and not seen["no improvement"][2]["new_best"]
    assert not seen["equal is no improvement"][2]["new_best"]
    wrap = seen["the 25th level-up in a row: 20 400 > 20 000, back to 400 and on to level 1"]
    assert wrap[0] == (0, 19600) and wrap[1] == (1, 400, 0.0) and wrap[2]["next_candidate"]
    assert seen["level 1: below the decayed threshold"][1] == (1, 400, 0.94) and not seen["level 1: below the decayed threshold"][2]["level_up"]
    assert seen["level 1: at the decayed threshold"][1] == (1, 1200, 0.0) and seen["level 1: at the decayed threshold"][2]["level_up"]
    assert seen["on to the last level"][1] == (2, 400, 0.0)
    assert seen["last level: level-up at 1 - 0.05 * 2"][1] == (2, 1200, 0.0)
    last = seen["the wrap at the last level: it stays"]
    assert last[0] == (2, 19600) and last[1] == (2, 400, 0.0) and last[2]["level_up"] and not last[2]["next_candidate"]
    assert sch.opponent() == ("traditional_mcts", {"c_puct": 5.0, "c_iterations": 400})           # None = the supervisor, powered to ref_iterations
    assert training.SUPERVISOR[1]["c_iterations"] == 20000                                          # (opponent() copies: the configuration is not written to)


def test_first_level_up_is_the_iteration_step():
    sch = EvaluationSchedule()
    events = sch.update(1.0)
    assert events == {"new_best": True, "level_up": True, "next_candidate": False}
    assert (sch.schedule_level, sch.ref_iterations, sch.best_win_rate) == (0, 1200, 0.0)


def test_scores_and_win_rate():
    winner = np.array([1, -1, 1, -1, 0, 0, 1, -1], dtype=np.int8)
    black = np.array([True, True, False, False, True, False, True, False])
    scores = selfplay.evaluation_scores(winner, black)
    assert scores.tolist() == [1.0, 0.0, 0.0, 1.0, 0.5, 0.5, 1.0, 1.0]
    assert scores.mean() == 5.0 / 8.0
    # eval_agents (agents/utils.py:82-95), restated: players.index(winner) after i reversals, ties give both half a point
    counts, players = np.zeros(2), [1, -1]
    for w in winner[[0, 1, 4, 5]]:              # a four-game match with alternating sides: network black, white, black, white
        if w == 0:
            counts += 0.5
        else:
            counts[players.index(w)] += 1
        players.reverse()
    mine = selfplay.evaluation_scores(winner[[0, 1, 4, 5]], selfplay.evaluation_sides(4))
    assert mine.sum() == counts[0] and mine.mean() == counts[0] / 4


def test_sides_alternate():
    for n in (0, 1, 2, 7, 11):
        black = selfplay.evaluation_sides(n)
        assert black.dtype == bool and black.shape == (n,)
        assert all(bool(black[i]) == (i % 2 == 0) for i in range(n))


def test_random_mcts_is_refused_on_the_device_loop_before_any_gpu_work():
    with pytest.raises(ValueError, match="random_mcts.*host loop"):
        selfplay.play_evaluation_games(2, None, ("random_mcts", {"c_iterations": 40}), device_loop=True)
    with pytest.raises(ValueError, match="unknown opponent"):
        selfplay.play_evaluation_games(2, None, ("botzone", {"program": "genm"}))


class _Replay:
    def __init__(self):
        self.draws = []

    def sample(self, batch_size):
        self.draws.append(batch_size)
        return "states", "values", "pi"

    def __len__(self):
        return 1000


class _Trainer:
    max_batch = 64

    def __init__(self, kls):
        self.kls, self.calls, self.exports = list(kls), [], 0

    def train_step(self, states, values, pi, lr, kl_target, num_epoches):
        self.calls.append((states, values, pi, lr, kl_target, num_epoches))
        return 1.0, 2.0, self.kls[len(self.calls) - 1], 3

    def export(self, fused):
        self.exports += 1


def test_loop_without_eval_period_takes_the_same_steps(monkeypatch):
    def no_match(*a, **k):
        raise AssertionError("eval_period=None must not play")
    monkeypatch.setattr(selfplay, "play_evaluation_games", no_match)
    kls = [0.001, 0.1, 0.02, 0.1, 0.001, 0.001]
    loops = []
    for kw in ({}, {"eval_period": None, "on_best": no_match, "on_checkpoint": no_match}):
        loop = TrainingLoop(_Replay(), _Trainer(kls), object(), batch_size=32, lr=1e-3, kl_target=0.02, num_epoches=4, export_every=2, **kw)
        taken = loop.run(len(kls))
        assert taken == loop.history and len(taken) == len(kls)
        loops.append(loop)
    a, b = loops
    assert a.history == b.history and a.trainer.calls == b.trainer.calls and a.replay.draws == b.replay.draws == [32] * 6
    assert a.trainer.exports == b.trainer.exports == 3 and a.lr_multiplier == b.lr_multiplier and b.schedule is None
    # the steps themselves: TrainPipeline.train_network's learning-rate rule (train.py:73-77)
    mult = 1.0
    for rec, call, kl in zip(b.history, b.trainer.calls, kls):
        assert sorted(rec) == ["entropy", "epochs", "exported", "kl", "loss", "lr"]
        assert rec["lr"] == 1e-3 * mult == call[3] and call[4:] == (0.02, 4)
        if kl > 0.04 and mult > 0.1:
            mult /= 1.5
        elif kl < 0.01 and mult < 10:
            mult *= 1.5
    with pytest.raises(ValueError):
        TrainingLoop(_Replay(), _Trainer(kls), object(), batch_size=32, eval_period=0)


def test_loop_evaluates_every_eval_period_steps(monkeypatch):
    """The loop's bookkeeping around a match that is scripted here: when it plays, against whom, and the names it hands to the callbacks
    (train.py:106-110, 126-134)."""
    rates = iter([0.5, 1.0, 0.25])
    asked = []

    def match(n_games, network, opponent, playouts=400, **kw):
        asked.append((n_games, network, opponent, playouts, kw))
        rate = next(rates)
        scores = np.full(n_games, rate)
        return None, selfplay.evaluation_sides(n_games), scores
    monkeypatch.setattr(selfplay, "play_evaluation_games", match)
    best, checkpoints = [], []
    fused = object()
    sch = EvaluationSchedule(candidates=[("rave_mcts", {"c_puct": 2.0, "c_iterations": 7}), None], eval_rounds=4, c_iterations=100)
    loop = TrainingLoop(_Replay(), _Trainer([0.02] * 6), fused, batch_size=32, export_every=4, eval_period=2, schedule=sch, eval_playouts=24,
                        eval_options={"max_moves": 40}, on_best=best.append, on_checkpoint=checkpoints.append)
    loop.run(6)
    assert [(a[0], a[1] is fused, a[2], a[3], a[4]) for a in asked] == [
        (4, True, ("rave_mcts", {"c_puct": 2.0, "c_iterations": 100}), 24, {"max_moves": 40}),
        (4, True, ("rave_mcts", {"c_puct": 2.0, "c_iterations": 100}), 24, {"max_moves": 40}),
        (4, True, ("rave_mcts", {"c_puct": 2.0, "c_iterations": 300}), 24, {"max_moves": 40})]
    assert best == ["best_model-rave_mcts-100", "best_model-rave_mcts-100", "best_model-rave_mcts-300"]
    assert checkpoints == ["current_model-2-0-100-0.50", "current_model-4-0-300-0.00", "current_model-6-0-300-0.25"]
    evals = [r for r in loop.history if r.get("evaluation")]
    assert [r["step"] for r in evals] == [2, 4, 6] and [r["win_rate"] for r in evals] == [0.5, 1.0, 0.25] and len(loop.history) == 9
    assert loop.trainer.exports == 3          # steps 2 and 6 export for the match, step 4 exported anyway


def test_header_declares_the_match_calls():
    text = open(os.path.join(ROOT, "include", "gomoku_hip.h")).read()
    declared = set(re.findall(r"\b(gmk_[a-z0-9_]+)\s*\(", text))
    from gomokuai_amd import lib as G
    for name in ("gmk_az_root_choice", "gmk_trad_root_choice", "gmk_match_referee", "gmk_az_step_device", "gmk_trad_step_device"):
        assert name in declared and name in G.EXPORTS, name
    for name, value in (("GMK_MATCH_MOVED", G.MATCH_MOVED), ("GMK_MATCH_REFUSED", G.MATCH_REFUSED), ("GMK_MATCH_ENDED", G.MATCH_ENDED), ("GMK_MATCH_OVER", G.MATCH_OVER)):
        assert re.search(r"#define %s %d\b" % (name, value), text), name
