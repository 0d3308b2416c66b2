"""K15 at the C boundary, without a GPU: the two gmk_vcf_defend* entries are declared, exported and bound, and they refuse to run without a
device instead of falling back to the CPU."""
import os
import re

import pytest

from gomokuai_amd import lib as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gmk_vcf_defend", "gmk_vcf_defend_host")


def test_entries_are_declared_exported_and_listed():
    text = open(os.path.join(ROOT, "include", "gomoku_hip.h")).read()
    declared = set(re.findall(r"\b(gmk_[a-z0-9_]+)\s*\(", text))
    L = G.load()
    for name in NAMES:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in G.EXPORTS, name
    assert "K15" in text
    for name, value in (("GMK_VCF_CELL_NONE", 0), ("GMK_VCF_CELL_HOLDS", 1), ("GMK_VCF_CELL_LOSES", 2), ("GMK_VCF_CELL_UNKNOWN", 3), ("GMK_VCF_CELL_FIVE", 4)):
        assert re.search(r"\b%s = %d\b" % (name, value), text), name


def test_no_cpu_fallback_without_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    L = G.load()
    assert L.gmk_vcf_defend(None, 225, None, 4, 16, 1000, 0, None, None, None, None, None, None, None, None) == -4          # GMK_ERR_STATE
    assert b"no CPU fallback" in L.gmk_last_error()
    assert L.gmk_vcf_defend_host(None, 225, None, 4, 16, 1000, 0, None, None, None, None, None, None, None) == -4
    with pytest.raises(G.GmkError):
        G.vcf_defend([[112, 113, 0, 0]], [2])


def test_python_layer_is_there():
    from gomokuai_amd import interface
    assert callable(G.vcf_defend) and callable(G.vcf_defend_device)
    assert (G.VCF_CELL_NONE, G.VCF_CELL_HOLDS, G.VCF_CELL_LOSES, G.VCF_CELL_UNKNOWN, G.VCF_CELL_FIVE) == (0, 1, 2, 3, 4)
    assert G.VCF_CELL_NAMES == ("NONE", "HOLDS", "LOSES", "UNKNOWN", "FIVE")
    plain = interface.VCFAgent(interface.RandomAgent(), depth=9, budget=77)
    assert plain.defend is False
    agent = interface.VCFAgent(interface.RandomAgent(), depth=9, budget=77, defend=True)
    assert agent.name() == "VCF(RandomAgent)" and (agent.depth, agent.budget, agent.defend) == (9, 77, True)
    wrapped = interface.make_agent("pattern", vcf=5, vcf_defend=True)
    assert type(wrapped) is interface.VCFAgent and wrapped.defend is True and wrapped.depth == 5
    assert interface.make_agent("pattern", vcf=5).defend is False
    with pytest.raises(ValueError):
        interface.make_agent("pattern", vcf_defend=True)
    with pytest.raises(SystemExit):
        interface.main(["botzone", "--vcf-defend"])
