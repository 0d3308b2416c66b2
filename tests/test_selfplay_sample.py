"""K20 in the K3 and K6 / K8 self-play loops, the part that needs no GPU: the sampled entries refuse bad schedules before they touch a handle
or the device, and play_games / play_supervisor_games refuse them as play_network_games does.  (tests/test_selfplay_sample_gpu.py holds the
kernels' choice.)"""
import pytest

from gomokuai_amd import lib as G
from gomokuai_amd import selfplay

ERR_ARG = -3
BAD = ((-1, 1), (226, 1), (6, 0), (6, 4))


def test_the_entries_refuse_bad_schedules_without_a_device():
    L = G.load()
    entries = {
        "gmk_mcts_advance_sampled": lambda S, k: L.gmk_mcts_advance_sampled(None, None, None, None, None, None, 0, S, k, None),
        "gmk_selfplay_run_sampled": lambda S, k: L.gmk_selfplay_run_sampled(None, 4, 0, 20, 1, 0.05, 0.25, S, k, None, 0, None, None, None, None, None, None, None),
        "gmk_trad_selfplay_run_sampled": lambda S, k: L.gmk_trad_selfplay_run_sampled(None, 0, 4, 0, 20, 5.0, 7, 1, 0.05, 0.25, S, k, None, 0, None, None, None, None, None, 1, 0,
                                                                                      None, None, None),
        "gmk_trad_root_choice_sampled": lambda S, k: L.gmk_trad_root_choice_sampled(None, None, None, S, k, 7, 0, None),
    }
    for name, entry in entries.items():
        assert name in G.EXPORTS
        for S, k in BAD + ((6, 1),):                             # (a good schedule: the NULL handle is refused)
            assert entry(S, k) == ERR_ARG, (name, S, k)
            assert name.encode() in L.gmk_last_error(), (name, S, k)


@pytest.mark.parametrize("play", [selfplay.play_games, selfplay.play_supervisor_games])
def test_the_game_loops_refuse_bad_schedules(play):
    for S, k in BAD:
        with pytest.raises(ValueError, match="sample_plies takes 0 .. 225"):
            play(2, 4, sample_plies=S, sample_power=k)
    assert selfplay._sample_schedule("x", 0, 3) is None and selfplay._sample_schedule("x", 225, 3) == (225, 3)
