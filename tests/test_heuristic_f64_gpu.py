"""The kernels that compile gomokuai_amd/csrc/heuristic_device.h -- K10 (gmk_pattern_policy, gmk_pattern_play) and the playout of K6
(gmk_trad_*) -- against the independent float64 statement of Heuristic.hpp (tests/heuristic_f64_reference.py): the support exactly,
probabilities and value within the derived rounding bound, the norm, the best move.  The same assertions hold the CPU restatements in
tests/test_heuristic_f64.py, where the bound is checked (and eight mutants are shown to break it) before a GPU sees it; the bit parity
of kernel and oracle stays with tests/test_pattern_gpu.py and tests/test_trad_gpu.py.

Sign convention of K6's root value (checked against oracle.TraditionalMCTS in tests/test_heuristic_f64.py): the root belongs to the
player who has just moved, the heuristic's value v is the player to move's, and the first playout backs -v up into the root, so
after run(1) root_value = -v."""
import functools

import numpy as np
import pytest

import heuristic_f64_inputs as inputs
import heuristic_f64_reference as H
from gomokuai_amd import lib as G

pytestmark = pytest.mark.gpu

F32 = np.float32
N = 225
OVER, STALLED = 1, 8
EDGES = ("high_cells", "low_cells", "empty", "corner", "corner_far", "own_four", "rival_four", "own_three", "searched")


@pytest.fixture(scope="module")
def gmk():
    G.init()
    return G


@functools.lru_cache(maxsize=None)
def _selection():
    """512 of the CPU test's positions: the edge cases by name first, every hand-made position, both 224-stone ties, and an even draw
    of the rest; -> (names, moves u8[512, 225], lens, the float64 statement at each)"""
    from oracle import oracle as O
    every = inputs.positions()
    by_name = {name: i for i, (_, name, _) in enumerate(every)}
    chosen = [by_name[e] for e in EDGES]
    chosen += [i for i, (group, _, moves) in enumerate(every) if (group == "hand" or len(moves) == 224) and i not in chosen]
    rest = [i for i in range(len(every)) if i not in set(chosen)]
    step = len(rest) / (512 - len(chosen))
    chosen += [rest[int(k * step)] for k in range(512 - len(chosen))]
    assert len(chosen) == len(set(chosen)) == 512
    names, f64 = [every[i][1] for i in chosen], []
    moves, lens = np.zeros((512, N), np.uint8), np.zeros(512, np.int32)
    for row, i in enumerate(chosen):
        ml = every[i][2]
        moves[row, :len(ml)], lens[row] = ml, len(ml)
        f64.append(H.Position(inputs.replay(O, ml)))
    assert {every[i][0] for i in chosen} == {"random", "clustered", "greedy", "hand", "tie"}
    assert set(p.exit for p in f64) == set(range(6)), "every exit of the automaton, and the path that runs out"
    hi, lo = f64[0].filtered, f64[1].filtered                    # probabilities in the last of a lane's four values alone / the first alone
    assert hi[192:].any() and not hi[:192].any() and lo[:64].any() and not lo[64:].any()
    return names, moves, lens, f64


def _check_rows(out, filt, n):
    names, _, _, f64 = _selection()
    assert out["probs"].shape == (n, N) and not out["status"].any()
    for g in range(n):
        H.check(f64[g], filt, out["probs"][g], out["value"][g], "K10 filter=%d at %s (row %d of %d)" % (filt, names[g], g, n))
        p64, bound = f64[g].side(filt)
        best = int(out["best"][g])
        assert p64[best] >= p64.max() - bound[best] - bound[int(np.argmax(p64))], (names[g], best)


# ---------------- K10: probabilities and value ----------------
@pytest.mark.parametrize("filt", [1, 0])
@pytest.mark.parametrize("n", [512, 1, 63, 64, 65])
def test_pattern_policy_meets_the_float64_statement(gmk, oracle, n, filt):
    """1, 63, 64, 65: around a wavefront's worth of positions; the edge cases lead the batch, so every size but 1 has them all"""
    _, moves, lens, _ = _selection()
    _check_rows(G.pattern_policy(moves[:n], lens[:n], filter=filt), filt, n)


def test_finished_positions_keep_their_contract(gmk, oracle):
    rng = np.random.RandomState(5)
    cases = [inputs.OWN_FOUR + [inputs.c(7, 6)], inputs.tie_order(rng), inputs.HIGH_CELLS + [inputs.c(13, 8)]]
    moves, lens = np.zeros((3, N), np.uint8), np.zeros(3, np.int32)
    for g, ml in enumerate(cases):
        moves[g, :len(ml)], lens[g] = ml, len(ml)
    for filt in (1, 0):
        out = G.pattern_policy(moves, lens, filter=filt)
        assert (out["status"] == OVER).all() and not out["probs"].any() and not out["value"].view(np.uint32).any() and (out["best"] == -1).all()


# ---------------- K10: whole games ----------------
@pytest.mark.parametrize("filt", [1, 0])
def test_pattern_play_meets_the_float64_statement_at_every_ply(gmk, oracle, filt):
    import torch
    rng = np.random.RandomState(17)
    opens = [[int(q) for q in rng.permutation(N)[:g % 9]] for g in range(32)]
    moves, lens = np.zeros((32, N), np.uint8), np.zeros(32, np.int32)
    for g, op in enumerate(opens):
        moves[g, :len(op)], lens[g] = op, len(op)
    dm, dl = torch.from_numpy(moves).cuda(), torch.from_numpy(lens).cuda()
    values = torch.full((32, N), -7.0, dtype=torch.float32, device="cuda")
    status = torch.full((32,), -7, dtype=torch.int32, device="cuda")
    G.pattern_play(dm.data_ptr(), dl.data_ptr(), 32, filt, 0, None, values.data_ptr(), status.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    played, length, values, status = dm.cpu().numpy(), dl.cpu().numpy(), values.cpu().numpy(), status.cpu().numpy()
    assert (status == OVER).all()                                 # every game ran to its end: none stalled, none met an error
    plies = 0
    for g, op in enumerate(opens):
        assert list(played[g, :len(op)]) == op and length[g] > len(op)
        ev = inputs.replay(oracle, op)
        for k in range(len(op), int(length[g])):
            assert not ev.check_end(), (g, k)
            pos = H.Position(ev)
            p64, bound = pos.side(filt)
            cell = int(played[g, k])
            assert p64[cell] > 0 and p64[cell] >= p64.max() - bound[cell] - bound[int(np.argmax(p64))], (g, k, cell)
            assert abs(float(values[g, k]) - pos.value) <= pos.value_bound, (g, k)
            assert not ev.apply(cell)[1]
            plies += 1
        assert ev.check_end()
    assert plies >= 32 * 9


# ---------------- K6: the same text inside the playout ----------------
def test_supervisor_root_meets_the_float64_statement(gmk, oracle):
    names, moves, lens, f64 = _selection()
    rows = list(range(16)) + list(range(16, 512, 31))            # the edge cases and hand-made positions, then a draw of the rest
    assert len(rows) == 32
    t = G.TraditionalMCTS(32, node_capacity=1 << 16)
    try:
        for playouts in (1, 64):
            t.set_positions(moves[rows], lens[rows])
            t.run(playouts)
            st = t.root_stats()
            assert not st["status"].any() and (st["root_visits"] == playouts).all()
            for g, row in enumerate(rows):
                pos, where = f64[row], "K6 after run(%d) at %s" % (playouts, names[row])
                # the expanded root: a child exactly on each cell of the filtered support, its prior the filtered probability
                H.check(pos, 1, st["priors"][g], None, where)
                assert not (st["visits"][g] != 0)[pos.filtered == 0].any(), where
                assert int(st["visits"][g].sum()) == playouts - 1, where
                if playouts == 1:
                    assert abs(float(st["root_value"][g]) + pos.value) <= pos.value_bound, where      # root_value = -v, see the docstring
    finally:
        t.close()
