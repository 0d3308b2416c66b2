"""The replay buffer's image on the host: gmk_replay_image_check_host against a numpy restatement of the format written from the text of
include/gomoku_hip.h ("The image"), each rule it must refuse by, parse_checkpoint_name, and EvaluationSchedule's state."""
import copy
import os

import numpy as np
import pytest

from gomokuai_amd import lib as G
from gomokuai_amd.training import EvaluationSchedule, parse_checkpoint_name

N = 225


def _roundup8(x):
    return (x + 7) // 8 * 8


def build_image(games, head=0):
    """games: [(len, first, winner, moves uint8[len], visit rows 2-byte [max(0, len - first), 225])], oldest first -> the image, uint8."""
    n = len(games)
    T = sum(g[0] for g in games)
    S = sum(max(0, g[0] - g[1]) for g in games)
    size = 64 + 8 * n + _roundup8(T) + _roundup8(450 * S)
    img = np.zeros(size, dtype=np.uint8)
    img[0:8] = np.frombuffer(b"GMKRPLY1", dtype=np.uint8)
    img[8:48] = np.array([n, T, S, head, size], dtype="<u8").view(np.uint8)
    at_m, at_v = 64 + 8 * n, 64 + 8 * n + _roundup8(T)
    for g, (length, first, winner, moves, rows) in enumerate(games):
        img[64 + 8 * g: 64 + 8 * g + 4] = np.array([length, first], dtype="<u2").view(np.uint8)
        img[64 + 8 * g + 4] = np.array([winner], dtype=np.int8).view(np.uint8)[0]
        moves = np.asarray(moves, dtype=np.uint8).reshape(-1)
        assert moves.size == length
        img[at_m: at_m + length] = moves
        at_m += length
        k = max(0, length - first)
        rows = np.ascontiguousarray(np.asarray(rows)).reshape(-1).view(np.uint8) if k else np.zeros(0, dtype=np.uint8)
        assert rows.size == 450 * k
        img[at_v: at_v + 450 * k] = rows
        at_v += 450 * k
    return img


def _games(spec, seed=0):
    rng = np.random.default_rng(seed)
    return [(length, first, winner, rng.permutation(N)[:length].astype(np.uint8),
             rng.integers(0, 65536, (max(0, length - first), N)).astype("<u2")) for length, first, winner in spec]


SPEC = [(3, 5, -1), (0, 0, 0), (7, 2, 1), (225, 224, 1), (40, 0, -1)]          # a game with len <= first, an empty one, a full one


def _put_u64(img, at, value):
    img[at: at + 8] = np.array([value], dtype="<u8").view(np.uint8)


def test_check_accepts_valid_images():
    empty = build_image([], head=12)
    assert empty.size == 64
    assert G.replay_image_check_host(empty) == {"games": 0, "plies": 0, "population": 0, "head": 12}
    img = build_image(_games(SPEC), head=3)
    assert img.size == 64 + 40 + 280 + _roundup8(450 * 46)
    assert G.replay_image_check_host(img) == {"games": 5, "plies": 275, "population": 46, "head": 3}
    assert G.replay_image_check_host(img.tobytes()) == G.replay_image_check_host(img)
    one = build_image(_games([(2, 2, 1)]), head=1 << 62)                          # len <= first alone: no visit section at all
    assert one.size == 64 + 8 + 8
    assert G.replay_image_check_host(one) == {"games": 1, "plies": 2, "population": 0, "head": 1 << 62}
    winners = build_image(_games([(4, 0, 77), (4, 0, -128)]))                     # the winner byte is copied, not judged
    assert G.replay_image_check_host(winners)["games"] == 2


def _damaged():
    good = build_image(_games(SPEC), head=3)
    moves_at = 64 + 8 * len(SPEC)
    cases = {}

    def case(name, rule):
        img = good.copy()
        cases[name] = (img, rule)
        return img

    case("magic", "magic")[7] ^= 1
    case("reserved word 0", "reserved")[48] = 1
    case("reserved word 1", "reserved")[63] = 0x80
    case("descriptor pad", "pad bytes")[64 + 8 * 2 + 6] = 1
    case("moves pad", "padding")[moves_at + 275] = 1
    case("visits pad", "padding")[good.size - 1] = 1
    case("len 226", "length")[64 + 8 * 3] = 226
    case("first 226", "first sampled ply")[64 + 8 * 4 + 2] = 226
    _put_u64(case("T + 1", "add up to T"), 16, 276)                               # (280 either way: the size cannot tell)
    _put_u64(case("T - 1", "add up to T"), 16, 274)
    _put_u64(case("S + 1", "size is not"), 24, 47)
    _put_u64(case("S - 1", "size is not"), 24, 45)
    _put_u64(case("bytes field", "bytes field"), 40, good.size + 8)
    _put_u64(case("n above 2^40", "n is above"), 8, (1 << 40) + 1)
    _put_u64(case("head above 2^62", "head is above"), 32, (1 << 62) + 1)
    case("move 225", "move")[moves_at + 10] = 225
    cases["one short"] = (good[:-1].copy(), "bytes field")
    cases["one long"] = (np.concatenate([good, np.zeros(1, dtype=np.uint8)]), "bytes field")
    # S off by one with a size that agrees: one game of 8 plies, first 1, claimed as S = 7 but described with first 0
    lie = build_image(_games([(8, 1, 0)]))
    lie[64 + 2] = 0
    cases["S off by one, size agreeing"] = (lie, "add up to S")
    return cases


@pytest.mark.parametrize("name", sorted(_damaged()))
def test_check_rejects(name):
    img, rule = _damaged()[name]
    with pytest.raises(ValueError, match=rule):
        G.replay_image_check_host(img)


def test_check_argument_errors():
    with pytest.raises(G.GmkError):
        G.replay_image_check_host(build_image([])[:63])
    with pytest.raises(ValueError):
        G.replay_image_check_host(build_image([]).astype(np.uint16))
    L = G.load()
    assert L.gmk_replay_image_check_host(None, 64, None) == -3
    good = build_image([])
    assert L.gmk_replay_image_check_host(good.ctypes.data, 64, None) == 0         # info may be NULL
    good[0] = 0
    assert L.gmk_replay_image_check_host(good.ctypes.data, 64, None) == G.REPLAY_BAD_IMAGE == 3
    assert G.REPLAY_NO_ROOM == 4


# ---------------- checkpoint names ----------------
def test_parse_checkpoint_name():
    for steps, level, ref, rate in ((1200, 2, 2000, 0.4545454), (0, 0, 400, 0.0), (7, 1, 20400, 1.0)):
        name = "current_model-{}-{}-{}-{:.2f}".format(steps, level, ref, rate)  # the format string of TrainingLoop.evaluate
        for path in (name, os.path.join("some", "dir-with-dashes", name), "/abs/" + name):
            assert parse_checkpoint_name(path) == {"total_steps": steps, "schedule_level": level, "ref_iterations": ref,
                                                   "best_win_rate": float("{:.2f}".format(rate))}
    for bad in ("best_model-rave_mcts-400", "current_model-12-0-400", "current_model-12-0-four-0.50", "current_model-12-0-400-0.50-1", "", "dir/"):
        with pytest.raises(ValueError):
            parse_checkpoint_name(bad)


# ---------------- the schedule's state ----------------
def test_schedule_state_follows_every_event():
    rates = [0.5, 0.3, 1.0, 0.2, 1.0, 0.4, 1.0, 0.96, 0.5, 0.95, 0.1]             # 4000 -> 12000 -> 20000 -> 28000 > 20000: the third level-up moves on
    a = EvaluationSchedule(eval_rounds=3, c_iterations=4000)
    seen = []
    for i, rate in enumerate(rates):
        events = a.update(rate)
        seen.append(tuple(sorted(k for k, v in events.items() if v)))
        state = a.state_dict()
        assert sorted(state) == ["best_win_rate", "ref_iterations", "schedule_level"]
        b = EvaluationSchedule(eval_rounds=3, c_iterations=4000)
        b.load_state_dict(state)
        twin = copy.deepcopy(a)
        assert b.opponent() == twin.opponent() and b.state_dict() == state
        for later in rates[i + 1:] + [1.0, 0.99]:                                 # ... and they update identically from there on
            assert b.update(later) == twin.update(later)
            assert b.opponent() == twin.opponent() and b.state_dict() == twin.state_dict()
    assert ("new_best",) in seen and ("level_up", "new_best") in seen and ("level_up", "new_best", "next_candidate") in seen and () in seen
    assert (a.schedule_level, a.ref_iterations, a.best_win_rate) == (1, 20000, 0.1)
    with pytest.raises(ValueError):
        EvaluationSchedule(candidates=[None]).load_state_dict({"schedule_level": 1, "ref_iterations": 400, "best_win_rate": 0.0})
