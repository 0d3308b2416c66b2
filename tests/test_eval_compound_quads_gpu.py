"""K1's phase 3b -- four lanes per (candidate cell, colour) pair, sixteen pairs per round, one rescan entry per lane, phase 4 early once more
than 192 entries are queued -- against the oracle's from-scratch evaluator (oracle.scratch_batch): all four outputs and the whole status word,
exact, no board left out.  Every set goes through the kernel one board per launch, seventeen per launch and all at once, into buffers with
sixteen boards of a sentinel behind every output, which must stay.  The sets, chosen by how their pairs fall on the rounds
(tests/test_eval_compound_quads.py checks on the CPU that they hold what is said here):
  counts      1 .. 20 candidate cells on a board (tests/golden/k1_compound_quads.npz): 14, 16, 18 and 30, 32, 34 pairs lie on either side
              of a round's end; boards on which white alone, black alone and both colours have candidates, a cell of both among them
  edge rows   compounds whose cell lies in rows 0 .. 2 and 12 .. 14
  directions  compounds of two components along directions (0, 3) and (1, 2): the quad's lanes 0 and 1 queue different entries, in direction order
  flush       the positions of tests/golden/k1_saturated.npz that queue more than 96 compounds: phase 4 runs before phase 3b's last round"""
import os

import numpy as np
import pytest

import eval_compound_quads_boards as B
from gomokuai_amd import lib as G

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ("scores", "density", "totals", "status")
WORDS = (900, 900, 11, 1)
SENTINEL = np.int32(0x5A5A5A5A)
EXTRA = 16

_sets = {}


def board_set(oracle, name):
    """move lists and the oracle's answer, once per set (shared by the cases, never written to)"""
    if name not in _sets:
        if name == "counts":
            with np.load(os.path.join(GOLDEN, "k1_compound_quads.npz")) as f:
                moves, lens = f["moves"], f["lens"]
        elif name == "flush":
            with np.load(os.path.join(GOLDEN, "k1_saturated.npz")) as f:
                heavy = f["load"][:, list(f["fields"]).index("queued")] > 96
                moves, lens = f["moves"][heavy], f["lens"][heavy]
        else:
            boards = B.edge_row_boards() if name == "edge rows" else B.direction_order_boards()
            moves, lens = B.pack(boards)
            if name == "edge rows":                               # (only the boards on which the lines make a compound that close to the edge)
                keep = oracle.scratch_load(moves, lens)[:, oracle.LOAD_FIELDS.index("compounds")] > 0
                moves, lens = moves[keep], lens[keep]
        ref = oracle.scratch_batch(moves, lens)
        for a in ref:
            a.setflags(write=False)
        _sets[name] = (G.moves_to_planes(moves, lens), ref)
    return _sets[name]


def launch_and_check(planes, ref, what):
    import torch
    dev = torch.device("cuda", 0)
    n = len(planes)
    d_planes = torch.from_numpy(np.ascontiguousarray(planes).view(np.int16).reshape(n, 32)).to(dev)
    bufs = [torch.full(((n + EXTRA) * w,), int(SENTINEL), dtype=torch.int32, device=dev) for w in WORDS]
    G.eval_batch(d_planes.data_ptr(), n, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), bufs[3].data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    host = [b.cpu().numpy() for b in bufs]
    for name, h, w in zip(NAMES, host, WORDS):
        touched = int((h[n * w:] != SENTINEL).sum())
        assert touched == 0, "%s: %d words of %s behind board %d were written" % (what, touched, name, n - 1)
    got = (host[0][:n * 900].reshape(n, 4, 225), host[1][:n * 900].reshape(n, 2, 2, 225), host[2][:n * 11].view(np.uint32).reshape(n, 11), host[3][:n])
    for name, a, b in zip(NAMES, ref, got):
        bad = np.nonzero((a.reshape(n, -1) != b.reshape(n, -1)).any(axis=1))[0]
        assert len(bad) == 0, "%s: %s differs on %d of %d boards, first %d" % (what, name, len(bad), n, bad[0])


@pytest.mark.parametrize("per_launch", [1, 17, 0], ids=["one-per-launch", "seventeen-per-launch", "all-at-once"])
@pytest.mark.parametrize("name", ["counts", "edge rows", "directions", "flush"])
def test_set_matches_scratch_oracle(oracle, name, per_launch):
    G.init(0)
    planes, ref = board_set(oracle, name)
    n = len(planes)
    assert n >= 20
    step = per_launch or n
    for first in range(0, n, step):
        last = min(first + step, n)
        launch_and_check(planes[first:last], [a[first:last] for a in ref], "%s, boards %d .. %d" % (name, first, last - 1))
    print("%s: %d boards in %d launches" % (name, n, (n + step - 1) // step))
