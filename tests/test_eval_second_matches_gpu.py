"""K1 (gmk_eval_batch) against the oracle's from-scratch evaluator on tests/golden/k1_second_matches.npz: boards on which transitions
report two matches, in every position against the 64-lane deposit rounds that the CPU half (test_eval_second_matches.py) checks the fixture
for.  Integer outputs and the whole status word: exact, every board compared."""
import os

import numpy as np
import pytest

from gomokuai_amd import lib as G

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "k1_second_matches.npz")
NAMES = ("scores", "density", "totals", "status")
STRIDE = 232


@pytest.fixture(scope="module")
def boards(oracle):
    with np.load(FIXTURE) as f:
        moves, lens = f["moves"], f["lens"]
    return moves, lens, oracle.scratch_batch(moves, lens, 1, 2)


def compare(ref, got, what):
    for name, a, b in zip(NAMES, ref, got):
        bad = np.nonzero((a.reshape(len(a), -1) != b.reshape(len(b), -1)).any(axis=1))[0]
        print("%s %s: %d of %d boards differ" % (what, name, len(bad), len(a)))
        assert len(bad) == 0, "%s: %s differs on %d of %d boards, first %d" % (what, name, len(bad), len(a), bad[0])


def test_fixture_boards_alone(boards):
    moves, lens, ref = boards
    assert len(lens) % 16 != 0, "the batch is meant to end in a partial group"
    compare(ref, G.eval_batch_host(G.moves_to_planes(moves, lens)), "second matches alone (%d boards)" % len(lens))


def test_fixture_boards_spread_through_4097(oracle, boards):
    """A partial last group and more boards than one workgroup's fixed first two per wavefront: the dynamic hand-out deals the fixture's boards."""
    fx_moves, fx_lens, fx_ref = boards
    n = 4097
    moves, lens, _ = G.synth_boards(n, 1, first_board=660000, stride=STRIDE)
    at = (np.arange(len(fx_lens)) * (n - 1)) // (len(fx_lens) - 1)          # the first and the last board among them
    assert len(set(at.tolist())) == len(at) and at[-1] == n - 1
    moves[at] = fx_moves
    lens[at] = fx_lens
    ref = oracle.scratch_batch(moves, lens, 1, 2)
    for a, b in zip(ref, fx_ref):
        assert (a[at] == b).all()
    compare(ref, G.eval_batch_host(G.moves_to_planes(moves, lens)), "spread through %d boards" % n)
