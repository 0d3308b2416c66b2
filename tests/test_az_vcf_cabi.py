"""K7 + K14 at the C boundary, without a GPU: the two read-out entries are declared, exported and bound, the option numbers are the header's,
and without a device the entries refuse to run instead of falling back to the CPU."""
import os
import re

import pytest

from gomokuai_amd import lib as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gmk_az_vcf_stats", "gmk_az_vcf_verdicts_host")


def test_entries_are_declared_exported_and_listed():
    text = open(os.path.join(ROOT, "include", "gomoku_hip.h")).read()
    declared = set(re.findall(r"\b(gmk_[a-z0-9_]+)\s*\(", text))
    L = G.load()
    for name in NAMES:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in G.EXPORTS, name
    assert "K7 + K14" in text


def test_option_numbers():
    text = open(os.path.join(ROOT, "include", "gomoku_hip.h")).read()
    for name, value in (("GMK_OPT_AZ_VCF_DEPTH", 4), ("GMK_OPT_AZ_VCF_BUDGET", 5), ("GMK_OPT_AZ_LEAVES", 3)):
        assert re.search(r"\b%s = %d\b" % (name, value), text), name
    assert (G.OPT_AZ_VCF_DEPTH, G.OPT_AZ_VCF_BUDGET) == (4, 5)
    assert len({G.OPT_NOISE_SAMPLER, G.OPT_LOCKSTEP, G.OPT_AZ_LEAVES, G.OPT_AZ_VCF_DEPTH, G.OPT_AZ_VCF_BUDGET}) == 5


def test_no_cpu_fallback_without_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    L = G.load()
    assert L.gmk_az_vcf_stats(None, None, None, None, None) == -4           # GMK_ERR_STATE
    assert b"no CPU fallback" in L.gmk_last_error()
    assert L.gmk_az_vcf_verdicts_host(None, None, None, None, None) == -4
    assert b"no CPU fallback" in L.gmk_last_error()
    with pytest.raises(G.GmkError):
        G.AlphaZeroMCTS(2, vcf_depth=8)


def test_python_layer_is_there():
    import inspect
    from gomokuai_amd import selfplay, training
    sig = inspect.signature(G.AlphaZeroMCTS.__init__).parameters
    assert sig["vcf_depth"].default == 0 and sig["vcf_budget"].default == 64
    assert callable(G.AlphaZeroMCTS.vcf_stats) and callable(G.AlphaZeroMCTS.vcf_verdicts)
    for fn in (selfplay.play_network_games, selfplay.play_evaluation_games, training.EvaluationSchedule.__init__):
        assert inspect.signature(fn).parameters["vcf"].default is None
