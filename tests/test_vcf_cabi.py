"""K14 at the C boundary, without a GPU: the two gmk_vcf_* entries are declared, exported and bound, and they refuse to run without a
device instead of falling back to the CPU."""
import os
import re

import pytest

from gomokuai_amd import lib as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gmk_vcf_solve", "gmk_vcf_solve_host")


def test_entries_are_declared_exported_and_listed():
    text = open(os.path.join(ROOT, "include", "gomoku_hip.h")).read()
    declared = set(re.findall(r"\b(gmk_[a-z0-9_]+)\s*\(", text))
    L = G.load()
    for name in NAMES:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in G.EXPORTS, name
    assert "K14" in text
    for name, value in (("GMK_VCF_MAX_DEPTH", 32), ("GMK_VCF_PV", 64), ("GMK_VCF_OPPONENT", 1), ("GMK_VCF_ITERATIVE", 2), ("GMK_VCF_NONE", 0),
                        ("GMK_VCF_WIN", 1), ("GMK_VCF_DEPTH", 2), ("GMK_VCF_BUDGET", 3), ("GMK_VCF_OVER", 4), ("GMK_VCF_BAD", 5)):
        assert re.search(r"\b%s = %d\b" % (name, value), text), name


def test_no_cpu_fallback_without_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    L = G.load()
    assert L.gmk_vcf_solve(None, 225, None, 4, 16, 1000, 0, None, None, None, None, None, None) == -4          # GMK_ERR_STATE
    assert b"no CPU fallback" in L.gmk_last_error()
    assert L.gmk_vcf_solve_host(None, 225, None, 4, 16, 1000, 0, None, None, None, None, None) == -4
    with pytest.raises(G.GmkError):
        G.vcf_solve([[112, 113, 0, 0]], [2])


def test_python_layer_is_there():
    from gomokuai_amd import interface
    assert callable(G.vcf_solve) and callable(G.vcf_solve_device)
    assert (G.VCF_NONE, G.VCF_WIN, G.VCF_DEPTH, G.VCF_BUDGET, G.VCF_OVER, G.VCF_BAD) == (0, 1, 2, 3, 4, 5)
    assert (G.VCF_OPPONENT, G.VCF_ITERATIVE, G.VCF_MAX_DEPTH, G.VCF_PV) == (1, 2, 32, 64)
    assert G.VCF_STATUS_NAMES == ("NONE", "WIN", "DEPTH", "BUDGET", "OVER", "BAD")
    agent = interface.VCFAgent(interface.RandomAgent(), depth=9, budget=77)
    assert agent.name() == "VCF(RandomAgent)" and (agent.depth, agent.budget) == (9, 77)
    assert type(interface.make_agent("random")) is interface.RandomAgent and type(interface.make_agent("random", vcf=8)) is interface.RandomAgent
    wrapped = interface.make_agent("pattern", vcf=5)
    assert type(wrapped) is interface.VCFAgent and wrapped.depth == 5 and type(wrapped.inner) is interface.PatternEvalAgent
    assert type(interface.make_agent("pattern")) is interface.PatternEvalAgent and type(interface.make_agent("pattern", vcf=0)) is interface.PatternEvalAgent
