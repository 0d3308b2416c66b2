"""K10 at the C boundary, without a GPU: the three gmk_pattern_* entries are declared, exported and bound, and they refuse to run
without a device instead of falling back to the CPU."""
import os
import re

import pytest

from gomokuai_amd import lib as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gmk_pattern_policy", "gmk_pattern_policy_host", "gmk_pattern_play")


def test_entries_are_declared_exported_and_listed():
    text = open(os.path.join(ROOT, "include", "gomoku_hip.h")).read()
    declared = set(re.findall(r"\b(gmk_[a-z0-9_]+)\s*\(", text))
    L = G.load()
    for name in NAMES:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in G.EXPORTS, name
    assert "K10" in text


def test_no_cpu_fallback_without_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    L = G.load()
    assert L.gmk_pattern_policy(None, 225, None, 4, 1, None, None, None, None, None) == -4          # GMK_ERR_STATE
    assert b"no CPU fallback" in L.gmk_last_error()
    assert L.gmk_pattern_policy_host(None, 225, None, 4, 1, None, None, None, None) == -4
    assert L.gmk_pattern_play(None, None, 4, 1, 0, None, None, None, None) == -4
    with pytest.raises(G.GmkError):
        G.pattern_policy([[112, 113, 0, 0]], [2])


def test_python_layer_is_there():
    from gomokuai_amd import selfplay
    assert callable(G.pattern_policy) and callable(G.pattern_policy_device) and callable(G.pattern_play)
    assert callable(selfplay.play_pattern_games)
    assert (G.PATTERN_OVER, G.PATTERN_EVALUATOR_ERROR, G.PATTERN_ILLEGAL, G.PATTERN_STALLED) == (1, 2, 4, 8)
