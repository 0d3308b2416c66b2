"""K17 at the C boundary, without a GPU: the four gmk_vcf_threats* / gmk_vct_solve* entries are declared, exported and bound, and they refuse
to run without a device instead of falling back to the CPU."""
import os
import re

import pytest

from gomokuai_amd import lib as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gmk_vcf_threats", "gmk_vcf_threats_host", "gmk_vct_solve", "gmk_vct_solve_host")


def test_entries_are_declared_exported_and_listed():
    text = open(os.path.join(ROOT, "include", "gomoku_hip.h")).read()
    declared = set(re.findall(r"\b(gmk_[a-z0-9_]+)\s*\(", text))
    L = G.load()
    for name in NAMES:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in G.EXPORTS, name
    assert text.count("K17") >= 2
    for value, name in enumerate(("NONE", "QUIET", "WINS", "UNKNOWN", "FIVE", "FOUR", "IGNORES")):
        assert re.search(r"\bGMK_VCF_THREAT_%s = %d\b" % (name, value), text), name
    for name, value in (("GMK_VCT_MAX_THREATS", 8), ("GMK_VCT_PV", 80), ("GMK_VCT_BUDGET", 6)):
        assert re.search(r"\b%s = %d\b" % (name, value), text), name


def test_no_cpu_fallback_without_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    L = G.load()
    assert L.gmk_vcf_threats(None, 225, None, 4, 16, 1000, 0, None, None, None, None, None, None, None, None, None) == -4      # GMK_ERR_STATE
    assert b"no CPU fallback" in L.gmk_last_error()
    assert L.gmk_vcf_threats_host(None, 225, None, 4, 16, 1000, 0, None, None, None, None, None, None, None, None) == -4
    assert L.gmk_vct_solve(None, 225, None, 4, 16, 1000, 0, 1, 64, None, None, None, None, None, None) == -4
    assert L.gmk_vct_solve_host(None, 225, None, 4, 16, 1000, 0, 1, 64, None, None, None, None, None) == -4
    with pytest.raises(G.GmkError):
        G.vcf_threats([[112, 113, 0, 0]], [2])
    with pytest.raises(G.GmkError):
        G.vct_solve([[112, 113, 0, 0]], [2])


def test_python_layer_is_there():
    from gomokuai_amd import interface
    import vct_reference as V
    assert all(callable(f) for f in (G.vcf_threats, G.vcf_threats_device, G.vct_solve, G.vct_solve_device))
    names = ("NONE", "QUIET", "WINS", "UNKNOWN", "FIVE", "FOUR", "IGNORES")
    assert G.VCF_THREAT_NAMES == names == tuple(V.THREAT_NAMES)
    assert [getattr(G, "VCF_THREAT_" + k) for k in names] == list(range(7)) == [getattr(V, "THREAT_" + k) for k in names]
    assert (G.VCT_MAX_THREATS, G.VCT_PV, G.VCT_BUDGET) == (8, 80, 6) == (V.MAX_THREATS, V.PV, V.VCT_BUDGET)
    assert G.VCT_STATUS_NAMES == G.VCF_STATUS_NAMES + ("VCT_BUDGET",) and list(G.VCT_STATUS_NAMES) == V.STATUS_NAMES
    plain = interface.VCFAgent(interface.RandomAgent(), depth=9, budget=77)
    assert plain.threats == 0
    agent = interface.VCFAgent(interface.RandomAgent(), depth=9, budget=77, threats=2)
    assert agent.name() == "VCF(RandomAgent)" and (agent.depth, agent.budget, agent.defend, agent.threats) == (9, 77, False, 2)
    wrapped = interface.make_agent("pattern", vcf=5, vct=3)
    assert type(wrapped) is interface.VCFAgent and wrapped.threats == 3 and wrapped.depth == 5 and wrapped.defend is False
    assert interface.make_agent("pattern", vcf=5).threats == 0
    assert type(interface.make_agent("pattern", vct=0)) is interface.PatternEvalAgent
    with pytest.raises(ValueError):
        interface.make_agent("pattern", vct=1)
    for bad in (9, -1):
        with pytest.raises(ValueError):
            interface.make_agent("pattern", vcf=8, vct=bad)
        with pytest.raises(ValueError):
            interface.VCFAgent(interface.RandomAgent(), threats=bad)
    assert interface.make_agent("pattern", vcf=8, vct=G.VCT_MAX_THREATS).threats == 8 and interface.VCFAgent(interface.RandomAgent(), threats=1).max_positions == 512
    for argv in (["botzone", "--vct", "1"], ["botzone", "--vcf", "8", "--vct", "9"]):
        with pytest.raises(SystemExit):
            interface.main(argv)
