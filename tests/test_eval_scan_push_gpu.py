"""K1's scan queues the emission of step s behind the lookup of step s + 2, the last two behind the loop, and phase 0's fourth score-block write
has no lane mask (eval_kernel.hip, phase 1 and late_piece).  Here are the boards on which a step has no emitter at all, one or two, and as
many as legal play and the synthetic generators give, and a board that overflows the queue.

The set, none left out: the empty board; the 225 boards with one stone; 225 x 2 boards with two stones, the second next to the first (the
direction turns with the cell, so all four kinds of line carry the pair; off the edge it goes the other way); the positions of
tests/golden/k1_saturated.npz that queue more than 320 transitions (338 at most: from 320 on, a step's 64 slots reach into the queue's last
64 words); 200 boards of each synthetic kind.  Against oracle.scratch_batch: scores, density, totals and the WHOLE status word, in one
launch, in launches of 17 and in launches of one board.  Integer outputs: exact.

The overflow board is a filling no game reaches (black stones only), found by a CPU search with oracle.scratch_load_cells over dense
fillings: 401 queued transitions, the queue flags at 384.  It stands between ordinary boards in one launch of 48: its status has bit 1 set,
every other board equals the oracle, the words around the four output buffers are untouched."""
import os

import numpy as np
import pytest

from gomokuai_amd import lib as G

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "k1_saturated.npz")
NAMES = ("scores", "density", "totals", "status")
WORDS = (900, 900, 11, 1)
SENTINEL = 0x5A5A5A5A
STRIDE = 232
QUEUE_FLAG_AT = 384                                                         # kQueueCap - 64 (eval_kernel.hip)
NEIGHBOURS = ((1, 0), (0, 1), (1, 1), (-1, 1))

OVERFLOW_BOARD = ("XXXXXX.XXXX.XXX",
                  "X.XXXX.XXXX.XX.",
                  "XXXX.XXXX.XX.XX",
                  ".XXX...XXX.XXXX",
                  "XXX.XXXX.XX.X.X",
                  "XX.XXXX.XXX.XXX",
                  "X.XX...XX.X.XX.",
                  "XXXXX.XXXXX.XXX",
                  ".XXX...XXX.XXXX",
                  "XXXX.X.X...XX.X",
                  "X..XX...X.XXXX.",
                  "XXXX.X.XX...XXX",
                  "XXXXXX.XXXXX.XX",
                  "XX.XXXXXX.XXXXX",
                  ".XXX.XXXXX.XXXX")


def small_boards():
    """-> move lists: no stone, one stone at every cell, two stones (the second next to the first) twice for every cell."""
    out = [[]]
    out += [[c] for c in range(225)]
    for c in range(225):
        x, y = c % 15, c // 15
        for k in (0, 2):
            dx, dy = NEIGHBOURS[(c + k) % 4]
            if not 0 <= x + dx < 15:
                dx = -dx
            if not 0 <= y + dy < 15:
                dy = -dy
            out.append([c, 15 * (y + dy) + x + dx])
    return out


def pack(seqs):
    moves = np.zeros((len(seqs), STRIDE), np.uint8)
    lens = np.zeros(len(seqs), np.int32)
    for i, seq in enumerate(seqs):
        moves[i, :len(seq)] = seq
        lens[i] = len(seq)
    return moves, lens


@pytest.fixture(scope="module")
def push_boards(oracle):
    T = oracle.LOAD_FIELDS.index("transitions")
    moves, lens = pack(small_boards())
    assert len(lens) == 1 + 225 + 450
    with np.load(FIXTURE) as f:
        sat_moves, sat_lens = f["moves"], f["lens"]
    sat_load = oracle.scratch_load(sat_moves, sat_lens)[:, T]
    heavy = np.nonzero(sat_load > 320)[0]
    assert sat_moves.shape[1] == STRIDE and len(heavy) > 0 and int(sat_load.max()) == 338
    parts = [(moves, lens), (sat_moves[heavy], sat_lens[heavy])]
    for kind in (0, 1):
        m, l, _ = G.synth_boards(200, kind, first_board=1300000 + kind, stride=STRIDE)
        parts.append((m, l))
    moves = np.concatenate([p[0] for p in parts])
    lens = np.concatenate([p[1] for p in parts])
    legal, end_ply, _ = oracle.replay_games(moves, lens)
    assert legal.all() and ((end_ply < 0) | (end_ply == lens)).all()
    load = oracle.scratch_load(moves, lens)[:, T]
    print("boards: %d (%d small, %d saturated above 320, 400 synthetic); queued transitions 0 .. %d, %d boards with none"
          % (len(lens), 676, len(heavy), int(load.max()), int((load == 0).sum())))
    assert int(load[0]) == 0 and int(load.max()) == 338 and int(load.max()) < QUEUE_FLAG_AT
    ref = oracle.scratch_batch(moves, lens)
    for a in ref:
        a.setflags(write=False)
    assert int(((ref[3] & 2) != 0).sum()) == 0
    return G.moves_to_planes(moves, lens), ref


def compare(ref, got, rows, what):
    for name, a, b in zip(NAMES, ref, got):
        a = a[rows]
        bad = np.nonzero((a.reshape(len(a), -1) != b.reshape(len(b), -1)).any(axis=1))[0]
        print("%s %s: %d of %d boards differ" % (what, name, len(bad), len(a)))
        assert len(bad) == 0, "%s: %s differs on %d of %d boards, first %d" % (what, name, len(bad), len(a), bad[0])


def launches_of(planes, n):
    parts = [G.eval_batch_host(planes[i:i + n]) for i in range(0, len(planes), n)]
    return [np.concatenate(p) for p in zip(*parts)]


def test_whole_set_in_one_launch(push_boards):
    planes, ref = push_boards
    got = G.eval_batch_host(planes)
    assert len(got[3]) == len(planes)
    compare(ref, got, slice(None), "one launch of %d" % len(planes))


def test_launches_of_seventeen(push_boards):
    """a partial group behind a full one, the last launch shorter still"""
    planes, ref = push_boards
    compare(ref, launches_of(planes, 17), slice(None), "launches of 17 (%d boards)" % len(planes))


def test_launches_of_one(push_boards):
    """one wavefront at work, every board of the set"""
    planes, ref = push_boards
    compare(ref, launches_of(planes, 1), slice(None), "launches of 1 (%d boards)" % len(planes))


def test_overflow_board_between_ordinary_boards(oracle):
    import torch
    G.init(0)
    dev = torch.device("cuda", 0)
    cells = np.array([[1 if ch == "X" else 0 for ch in row] for row in OVERFLOW_BOARD], np.int8)
    assert cells.shape == (15, 15)
    load = dict(zip(oracle.LOAD_FIELDS, oracle.scratch_load_cells(cells.reshape(1, 225))[0].tolist()))
    print("overflow board: %s" % load)
    assert load["transitions"] == 401 and load["transitions"] > QUEUE_FLAG_AT
    n, at = 48, 23
    moves, lens, planes = G.synth_boards(n, 1, first_board=1400000, stride=STRIDE)
    ref = oracle.scratch_batch(moves, lens)
    assert (planes == G.moves_to_planes(moves, lens)).all()
    # (a plane is sixteen row words, bit x of word y is cell (x, y): restated here and held against moves_to_planes on the board in front)
    rows_of = lambda c: np.array([sum(int(c[y, x]) << x for x in range(15)) for y in range(15)] + [0], np.uint16)
    before = np.zeros((2, 15, 15), np.int8)
    for ply, mv in enumerate(moves[at - 1, :lens[at - 1]]):
        before[ply & 1, mv // 15, mv % 15] = 1
    assert (planes[at - 1, 0] == rows_of(before[0])).all() and (planes[at - 1, 1] == rows_of(before[1])).all()
    planes = planes.copy()
    planes[at, 0] = rows_of(cells)
    planes[at, 1] = 0
    front, extra = 1, 16
    d_planes = torch.from_numpy(planes.view(np.int16).reshape(n, 32)).to(dev)
    sentinel = np.int32(SENTINEL)
    bufs = [torch.full(((front + n + extra) * words,), int(sentinel), dtype=torch.int32, device=dev) for words in WORDS]
    ptrs = [b.data_ptr() + 4 * front * words for b, words in zip(bufs, WORDS)]
    G.eval_batch(d_planes.data_ptr(), n, ptrs[0], ptrs[1], ptrs[2], ptrs[3], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    host = [b.cpu().numpy() for b in bufs]
    for name, h, words in zip(NAMES, host, WORDS):
        outside = np.concatenate([h[:front * words], h[(front + n) * words:]])
        assert int((outside != sentinel).sum()) == 0, "%s: words outside boards 0 .. %d were written" % (name, n - 1)
    body = [h[front * words:(front + n) * words] for h, words in zip(host, WORDS)]
    got = (body[0].reshape(n, 4, 225), body[1].reshape(n, 2, 2, 225), body[2].view(np.uint32).reshape(n, 11), body[3])
    print("overflow board's status %#x" % int(got[3][at]))
    assert int(got[3][at]) & 2, "the board with %d queued transitions is not flagged" % load["transitions"]
    others = np.array([i for i in range(n) if i != at])
    compare(ref, [g[others] for g in got], others, "launch of 48, the 47 ordinary boards")
