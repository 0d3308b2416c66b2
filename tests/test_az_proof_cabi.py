"""K7 + proofs at the C boundary, without a GPU: the two read-out entries are declared, exported and bound, the option number is the header's,
the Python layers take proof= with the defaults that reproduce the calls without it, and without a device nothing falls back to the CPU."""
import inspect
import os
import re

import pytest

from gomokuai_amd import lib as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gmk_az_root_proofs", "gmk_az_proof_stats")


def test_entries_are_declared_exported_and_listed():
    text = open(os.path.join(ROOT, "include", "gomoku_hip.h")).read()
    declared = set(re.findall(r"\b(gmk_[a-z0-9_]+)\s*\(", text))
    L = G.load()
    for name in NAMES:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in G.EXPORTS, name
    assert "K7 + proofs" in text


def test_option_number_and_values():
    text = open(os.path.join(ROOT, "include", "gomoku_hip.h")).read()
    for name, value in (("GMK_OPT_AZ_PROOF", 6), ("GMK_AZ_PROOF_NONE", 0), ("GMK_AZ_PROOF_WINS", 1), ("GMK_AZ_PROOF_LOSES", 2)):
        assert re.search(r"\b%s = %d\b" % (name, value), text), name
    assert G.OPT_AZ_PROOF == 6 and (G.AZ_PROOF_NONE, G.AZ_PROOF_WINS, G.AZ_PROOF_LOSES) == (0, 1, 2)
    assert len({G.OPT_NOISE_SAMPLER, G.OPT_LOCKSTEP, G.OPT_AZ_LEAVES, G.OPT_AZ_VCF_DEPTH, G.OPT_AZ_VCF_BUDGET, G.OPT_AZ_PROOF}) == 6


def test_python_layer_is_there():
    from gomokuai_amd import selfplay, training
    assert inspect.signature(G.AlphaZeroMCTS.__init__).parameters["proof"].default is False
    assert callable(G.AlphaZeroMCTS.root_proofs) and callable(G.AlphaZeroMCTS.proof_stats)
    for fn in (selfplay.play_network_games, selfplay.play_evaluation_games, training.EvaluationSchedule.__init__):
        assert inspect.signature(fn).parameters["proof"].default is False
    assert list(inspect.signature(selfplay._root_choice).parameters) == ["visits", "proofs"]


def test_no_cpu_fallback_without_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    L = G.load()
    assert L.gmk_az_root_proofs(None, None, None) == -4          # GMK_ERR_STATE
    assert b"no CPU fallback" in L.gmk_last_error()
    assert L.gmk_az_proof_stats(None, None, None) == -4
    assert b"no CPU fallback" in L.gmk_last_error()
    with pytest.raises(G.GmkError) as err:
        G.AlphaZeroMCTS(2, proof=True)
    assert "no CPU fallback" in str(err.value)
