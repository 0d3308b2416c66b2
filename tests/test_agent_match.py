"""selfplay.play_agent_match without a GPU: every refusal of a spec or of the match's shape comes before the library is initialised, so
these pass on a machine without a device; and the header carries the two K3 entries the device loop calls."""
import os
import re

import pytest

from gomokuai_amd import lib as G
from gomokuai_amd import selfplay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Net:
    """Stands for a network: the validation only asks that there is one."""


NET = ("network", {"network": _Net(), "playouts": 16})
TRAD = ("traditional_mcts", {"c_iterations": 40})


@pytest.fixture(autouse=True)
def no_device(monkeypatch):
    def touched(*a, **k):
        raise AssertionError("the library was initialised before the arguments were checked")
    monkeypatch.setattr(G, "init", touched)
    monkeypatch.setattr(selfplay, "_device", touched)


def _net(**kw):
    return ("network", dict(NET[1], **kw))


def test_unknown_agents_and_missing_networks():
    with pytest.raises(ValueError, match="unknown agent 'pattern'"):
        selfplay.play_agent_match(2, ("pattern", {}), TRAD)
    with pytest.raises(ValueError, match="unknown agent 'alphazero'"):
        selfplay.play_agent_match(2, TRAD, ("alphazero", {}))
    with pytest.raises(ValueError, match="needs its network"):
        selfplay.play_agent_match(2, ("network", {"playouts": 16}), TRAD)
    with pytest.raises(ValueError, match="needs its network"):
        selfplay.play_agent_match(2, TRAD, ("network", {"network": None}))
    with pytest.raises(ValueError, match="not playout"):
        selfplay.play_agent_match(2, _net(playout=3), TRAD)
    with pytest.raises(ValueError, match=r"\(kind, kwargs\)"):
        selfplay.play_agent_match(2, "traditional_mcts", TRAD)
    with pytest.raises(ValueError, match="symmetry"):
        selfplay.play_agent_match(2, _net(symmetry="mirror"), TRAD)
    with pytest.raises(ValueError, match="sample_plies"):
        selfplay.play_agent_match(2, _net(sample_plies=4, sample_power=4), TRAD)
    with pytest.raises(ValueError, match="c_iterations >= 2"):
        selfplay.play_agent_match(2, NET, ("random_mcts", {"c_iterations": 1}))


def test_the_shape_of_the_match():
    with pytest.raises(ValueError, match="even number of games"):
        selfplay.play_agent_match(3, NET, TRAD)
    with pytest.raises(ValueError, match="even number of games"):
        selfplay.play_agent_match(1, NET, TRAD, paired=True)
    with pytest.raises(ValueError, match="at most 8 plies"):
        selfplay.play_agent_match(2, NET, TRAD, opening_plies=9)
    with pytest.raises(ValueError, match="at most 8 plies"):
        selfplay.play_agent_match(3, NET, TRAD, opening_plies=9, paired=False)


@pytest.mark.parametrize("name,options", [("leaves > 1", {"leaves": 4}), ("proof", {"proof": True}), ("vcf_defend", {"vcf_defend": True}),
                                          ("sample_plies > 0", {"sample_plies": 6})])
@pytest.mark.parametrize("side", [0, 1])
def test_gumbel_refuses_what_play_network_games_refuses(name, options, side):
    """... with the same words, on whichever side it stands"""
    spec = _net(gumbel=(8, 50.0, 1.0), **options)
    sides = (spec, TRAD) if side == 0 else (NET, spec)
    with pytest.raises(ValueError) as here:
        selfplay.play_agent_match(2, *sides)
    with pytest.raises(ValueError) as there:
        selfplay.play_network_games(2, _Net(), 16, root_noise=None, gumbel=(8, 50.0, 1.0), **options)
    assert name in str(here.value)
    assert str(here.value).split(": ", 1)[1] == str(there.value).split(": ", 1)[1]
    assert str(here.value).startswith("play_agent_match: ") and str(there.value).startswith("play_network_games: ")


@pytest.mark.parametrize("side", [0, 1])
def test_gumbel_refuses_root_noise(side):
    spec = _net(gumbel=(8, 50.0, 1.0))
    sides = (spec, TRAD) if side == 0 else (TRAD, spec)
    with pytest.raises(ValueError) as here:
        selfplay.play_agent_match(2, *sides, root_noise=(0.05, 0.25))
    with pytest.raises(ValueError) as there:
        selfplay.play_network_games(2, _Net(), 16, gumbel=(8, 50.0, 1.0))
    assert "root noise" in str(here.value) and str(here.value).split(": ", 1)[1] == str(there.value).split(": ", 1)[1]
    with pytest.raises(ValueError, match="max_considered, c_visit, c_scale"):
        selfplay.play_agent_match(2, _net(gumbel=(8, 50.0)), TRAD)


def test_header_and_exports_carry_the_k3_entries():
    header = open(os.path.join(ROOT, "include", "gomoku_hip.h")).read()
    for name, args in (("gmk_mcts_root_choice", r"gmk_mcts\* m, int16_t\* d_cells, uint16_t\* d_visits, void\* stream"),
                       ("gmk_mcts_step_device", r"gmk_mcts\* m, const int16_t\* d_cells, const int32_t\* d_verdict, int fresh_root, void\* stream")):
        assert re.search(r"\bint %s\(%s\);" % (name, args), header), name
        assert name in G.EXPORTS
    for method in ("root_choice", "step_device", "step_host"):
        assert callable(getattr(G.BatchedMCTS, method))
    assert selfplay._MATCH_AGENTS == ("traditional_mcts", "rave_mcts", "random_mcts", "network")
