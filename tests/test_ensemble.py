"""K13 on the host: the ensemble merge's arithmetic (gmk_ensemble_merge_host, one text with the device kernels: csrc/ensemble_merge.h)
against a numpy restatement, bit for bit, and the argument checks of the new layers.  Needs no GPU."""
import os
import re

import numpy as np
import pytest

from gomokuai_amd import lib as G
from ensemble_reference import LIMIT, assert_same, numpy_merge

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gmk_mcts_ensemble_merge", "gmk_trad_ensemble_merge", "gmk_ensemble_merge_host")


def test_symbols_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "gomoku_hip.h")).read()
    L = G.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % name, text), "%s is not declared in include/gomoku_hip.h" % name
        assert hasattr(L, name) and name in G.EXPORTS


@pytest.mark.parametrize("group", [1, 2, 5, 70, 4096])
def test_random_tables(group):
    rng = np.random.default_rng(group)
    E = 3 if group < 4096 else 1
    n = rng.integers(0, 5000, (E * group, 225)).astype(np.uint32)
    n[rng.random(n.shape) < 0.3] = 0                                       # cells without a child
    q = rng.uniform(-1, 1, n.shape).astype(np.float32)
    q[rng.random(n.shape) < 0.05] *= np.float32(1e-6)                     # values whose fixed-point term rounds
    rn = n.sum(axis=1).astype(np.uint32) + 1
    rq = rng.uniform(-1, 1, E * group).astype(np.float32)
    assert_same(G.ensemble_merge_host(group, n, q, rn, rq), numpy_merge(group, n, q, rn, rq), "group %d" % group)
    assert_same(G.ensemble_merge_host(group, n, q), numpy_merge(group, n, q), "group %d, no root pair" % group)


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_largest_counts_do_not_overflow(sign):
    """n = 2^24 - 1 and q = +-1 in all 4 096 replicas: |S| = 4096 (2^24 - 1) 2^24 < 2^60 fits int64 and the value is exactly +-1.  The
    count sums are 2^36 - 4096: kept exactly (the division uses them), reported as 2^32 - 1 with status bit 2."""
    n = np.full((4096, 225), LIMIT - 1, np.uint32)
    q = np.full((4096, 225), sign, np.float32)
    rn = np.full(4096, LIMIT - 1, np.uint32)
    rq = np.full(4096, sign, np.float32)
    got = G.ensemble_merge_host(4096, n, q, rn, rq)
    assert_same(got, numpy_merge(4096, n, q, rn, rq))
    assert (got["values"] == np.float32(sign)).all() and got["root_value"][0] == np.float32(sign)
    assert (got["visits"] == 0xFFFFFFFF).all() and got["status"][0] == G.ENSEMBLE_SATURATED and got["cells"][0] == 0


def test_largest_counts_without_saturation():
    """256 replicas of 2^24 - 1 sum to 2^32 - 256: the uint32 outputs are exact and no status bit is set."""
    n = np.full((256, 225), LIMIT - 1, np.uint32)
    q = np.full((256, 225), -1.0, np.float32)
    got = G.ensemble_merge_host(256, n, q, n[:, 0], q[:, 0])
    assert_same(got, numpy_merge(256, n, q, n[:, 0], q[:, 0]))
    assert (got["visits"] == 256 * (LIMIT - 1)).all() and got["status"][0] == 0 and (got["values"] == np.float32(-1)).all()


def test_count_out_of_range_sets_status():
    rng = np.random.default_rng(7)
    n = rng.integers(1, 100, (3 * 4, 225)).astype(np.uint32)
    q = rng.uniform(-1, 1, n.shape).astype(np.float32)
    rn = np.full(12, 1000, np.uint32)
    rq = np.zeros(12, np.float32)
    n[5, 17] = LIMIT                                                       # ensemble 1, replica 1: a child count of 2^24
    rn[10] = LIMIT                                                         # ensemble 2, replica 2: a root count of 2^24
    got = G.ensemble_merge_host(4, n, q, rn, rq)
    assert_same(got, numpy_merge(4, n, q, rn, rq))
    assert got["status"].tolist() == [0, G.ENSEMBLE_RANGE, G.ENSEMBLE_RANGE]
    assert got["visits"][1, 17] == n[[4, 6, 7], 17].sum()                 # the flagged replica added nothing


def test_first_maximum_wins_ties():
    n = np.zeros((2 * 3, 225), np.uint32)
    q = np.zeros(n.shape, np.float32)
    n[0, 200] = 4; n[1, 30] = 3; n[2, 30] = 1; n[2, 31] = 4                # ensemble 0: cells 30, 31 and 200 tie at 4
    n[3, 224] = 2; n[4, 224] = 1; n[5, 0] = 3                              # ensemble 1: cells 0 and 224 tie at 3
    got = G.ensemble_merge_host(3, n, q)
    assert_same(got, numpy_merge(3, n, q))
    assert got["cells"].tolist() == [30, 0]


def test_all_zero_tables():
    n = np.zeros((2 * 5, 225), np.uint32)
    q = np.ones(n.shape, np.float32)
    got = G.ensemble_merge_host(5, n, q, np.zeros(10, np.uint32), np.ones(10, np.float32))
    assert got["cells"].tolist() == [-1, -1] and not got["values"].any() and not got["visits"].any()
    assert not got["root_value"].any() and not got["status"].any()


def test_one_cell_visited_by_one_replica():
    n = np.zeros((70, 225), np.uint32)
    q = np.zeros(n.shape, np.float32)
    n[41, 113] = 9
    q[41, 113] = np.float32(-0.3)
    got = G.ensemble_merge_host(70, n, q)
    assert_same(got, numpy_merge(70, n, q))
    assert got["cells"][0] == 113 and got["visits"][0, 113] == 9 and np.count_nonzero(got["visits"]) == 1
    # one term, one rounding to 2^-24, one division: within half a step of 2^-24 / 9 and a float32 rounding of the value it came from
    assert abs(float(got["values"][0, 113]) - float(np.float32(-0.3))) <= 2.0 ** -25 / 9 + 2.0 ** -26


def test_argument_errors():
    n = np.zeros((12, 225), np.uint32)
    q = np.zeros(n.shape, np.float32)
    for group in (0, 4097, -1):
        with pytest.raises(G.GmkError):
            G.ensemble_merge_host(group, n, q)
    with pytest.raises(G.GmkError):
        G.ensemble_merge_host(5, n, q)                                     # 5 does not divide 12 games
    assert G.load().gmk_ensemble_merge_host(1, 1, None, None, None, None, None, None, None, None, None, None) == -3      # GMK_ERR_ARG


def test_deterministic_policies_need_noise():
    """K6 and K6 + RAVE replicas differ through root noise only: refused before any device call (this test runs without a device)."""
    from gomokuai_amd.ensemble import EnsembleSearch
    for policy in ("traditional", "traditional-rave"):
        with pytest.raises(ValueError, match="root_noise"):
            EnsembleSearch(policy, replicas=4, root_noise=None)
        assert EnsembleSearch(policy, replicas=1, root_noise=None).tree is None            # one replica: nothing to tell apart
        assert EnsembleSearch(policy, replicas=4, root_noise=(0.05, 0.25)).tree is None    # (the handle is made by set_positions)
    assert EnsembleSearch("random", replicas=4).tree is None and EnsembleSearch("poolrave", replicas=4).tree is None
    for bad in (dict(policy="alphazero", replicas=2), dict(policy="random", replicas=0), dict(policy="random", replicas=4097)):
        with pytest.raises(ValueError):
            EnsembleSearch(**bad)


def test_make_agent_with_one_replica_is_the_agent_of_today():
    from gomokuai_amd import interface as I
    for spec in ("random", "pattern", "random-mcts:5:5", "traditional:5", "poolrave"):
        assert type(I.make_agent(spec, iterations=10, replicas=1)) is type(I.make_agent(spec, iterations=10))
    assert type(I.make_agent("random", replicas=8)) is I.RandomAgent       # not an MCTS kind: unchanged
