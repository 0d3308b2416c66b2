"""K7 + K15 at the C boundary, without a GPU: the two read-out entries are declared, exported and bound, the option number is the header's,
the Python layers take vcf_defend= with the defaults that reproduce the calls without it, and without a device nothing falls back to the CPU."""
import ctypes as C
import inspect
import os
import re

import pytest

from gomokuai_amd import lib as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gmk_az_defend_stats", "gmk_az_defend_verdicts_host")


def test_entries_are_declared_exported_and_listed():
    text = open(os.path.join(ROOT, "include", "gomoku_hip.h")).read()
    declared = set(re.findall(r"\b(gmk_[a-z0-9_]+)\s*\(", text))
    L = G.load()
    for name in NAMES:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in G.EXPORTS, name
    assert "K7 + K15" in text and "GMK_VCF_CELL_FIVE cannot occur" in text


def test_option_number_and_signatures():
    text = open(os.path.join(ROOT, "include", "gomoku_hip.h")).read()
    assert re.search(r"\bGMK_OPT_AZ_VCF_DEFEND = 7\b", text)
    assert G.OPT_AZ_VCF_DEFEND == 7
    assert len({G.OPT_NOISE_SAMPLER, G.OPT_LOCKSTEP, G.OPT_AZ_LEAVES, G.OPT_AZ_VCF_DEPTH, G.OPT_AZ_VCF_BUDGET, G.OPT_AZ_PROOF, G.OPT_AZ_VCF_DEFEND}) == 7
    flat = " ".join(text.split())
    assert "int gmk_az_defend_stats(gmk_az* a, uint32_t* h_threatened, uint32_t* h_marked, uint32_t* h_searched, uint64_t* h_nodes);" in flat
    assert ("int gmk_az_defend_verdicts_host(gmk_az* a, int32_t* h_threat_status, int32_t* h_threat_length, int8_t* h_verdict, "
            "uint32_t* h_nodes);") in flat
    L = G.load()
    for name in NAMES:
        assert list(getattr(L, name).argtypes) == [C.c_void_p] * 5, name


def test_python_layer_is_there():
    from gomokuai_amd import selfplay, training
    assert inspect.signature(G.AlphaZeroMCTS.__init__).parameters["vcf_defend"].default is False
    assert callable(G.AlphaZeroMCTS.defend_stats) and callable(G.AlphaZeroMCTS.defend_verdicts)
    for fn in (selfplay.play_network_games, selfplay.play_evaluation_games, training.EvaluationSchedule.__init__):
        assert inspect.signature(fn).parameters["vcf_defend"].default is False


def test_no_cpu_fallback_without_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    L = G.load()
    assert L.gmk_az_defend_stats(None, None, None, None, None) == -4          # GMK_ERR_STATE
    assert b"no CPU fallback" in L.gmk_last_error()
    assert L.gmk_az_defend_verdicts_host(None, None, None, None, None) == -4
    assert b"no CPU fallback" in L.gmk_last_error()
    with pytest.raises(G.GmkError) as err:
        G.AlphaZeroMCTS(2, vcf_depth=8, proof=True, vcf_defend=True)
    assert "no CPU fallback" in str(err.value)
