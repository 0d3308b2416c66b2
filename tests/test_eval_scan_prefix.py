"""K1's scan reads the state behind a lane's first four symbols from a table and queues nothing for them (eval_kernel.hip, phase 1): a
lane's stream is `cellsA ? ? cellsB ? ? ...` walked from S, the state the root reaches on '?'; every first line has five or more cells, so
the first four symbols are cells, and entry s0 | s1 << 2 | s2 << 4 | s3 << 6 of the table is the state S reaches over them.  That is right
only if no walk of four cells from S reports a match on any of its transitions; the host checks it when it builds the kernel's image
(scan_prefix_table) and refuses a table without the property.

On the CPU, with the host's transition table (lib.tables_copy):
  * the property, for all 81 sequences of four cell symbols, and that it ends at four: some sequence of five cells does report;
  * the table as the kernel indexes it, every entry against four single steps from S, and how many keys the root's table would get wrong;
  * the stream with the prefix -- steps 0..3 report nothing, step 4 starts from the table's state -- reports, segment by segment, exactly the
    (pattern, end cell, segment) set that `? cells ? ?` reports from the root: for every line of 5 to 9 cells over {black, white, blank}
    and for 20 000 seeded random pairs of lines of 5 to 15 cells of every density.

Symbols are the device's codes: 0 black, 1 white, 2 '?' (off the board), 3 blank.  A transition's emissions are a list of (pattern, back):
the match ends on the symbol just consumed (back 0) or on the one before it (back 1).  Step s of a stream belongs to the second segment iff
s >= seg_a = len_a + 2, and its place there is s - seg_a, as in the kernel's phase 2."""
import itertools

import numpy as np

from gomokuai_amd import lib as G

PAD, ROOT = 2, 0
CELLS = (0, 1, 3)
PREFIX = 4


def _tables():
    trans, emit, _ = G.tables_copy()
    nxt = (trans & 0x3FF).astype(np.int64).reshape(-1, 4)
    lst = ((trans >> 10) & 0x3FF).astype(np.int64).reshape(-1, 4)
    # an emission list as the set of its (pattern, back) pairs; lists with the same set get the same id (0: nothing)
    ids, sets = {frozenset(): 0}, {}
    canon = np.zeros(int(lst.max()) + 1, dtype=np.int64)
    for i in np.unique(lst):
        if i == 0:
            continue
        count = int(emit[i])
        s = frozenset((int(e) & 0x7FFF, int(e) >> 15) for e in emit[i + 1:i + 1 + count])
        assert count > 0 and len(s) == count
        canon[i] = ids.setdefault(s, len(ids))
        sets[canon[i]] = s
    return nxt, canon[lst], sets


def _prefix_table(nxt, state):
    """entry s0 | s1 << 2 | s2 << 4 | s3 << 6: the state reached from `state` over s0 s1 s2 s3, all 256 keys at once"""
    keys = np.arange(256)
    st = np.full(256, state, dtype=np.int64)
    for i in range(PREFIX):
        st = nxt[st, (keys >> (2 * i)) & 3]
    return st


def _walk(nxt, em, syms, state, first=0):
    """syms [n, steps], state a number or [n] -> the emission id of every step from `first` on, [n, steps] (zero in front of it)"""
    out = np.zeros(syms.shape, dtype=np.int64)
    st = np.broadcast_to(np.asarray(state, dtype=np.int64), (len(syms),)).copy()
    for k in range(first, syms.shape[1]):
        out[:, k] = em[st, syms[:, k]]
        st = nxt[st, syms[:, k]]
    return out


def test_no_four_cells_from_the_start_state_report_and_five_do():
    nxt, em, _ = _tables()
    s = int(nxt[ROOT, PAD])
    four = np.array(list(itertools.product(CELLS, repeat=PREFIX)), dtype=np.int64)
    assert len(four) == 81
    got = _walk(nxt, em, four, s)
    print("states %d, S = %d; of 81 walks of four cells from S, %d report" % (len(nxt), s, int(got.any(axis=1).sum())))
    assert not got.any(), "four cells from S report a match: %s" % four[got.any(axis=1)][:3].tolist()
    five = np.array(list(itertools.product(CELLS, repeat=PREFIX + 1)), dtype=np.int64)
    reporting = int(_walk(nxt, em, five, s).any(axis=1).sum())
    print("of 243 walks of five cells from S, %d report" % reporting)
    assert reporting > 0, "a fifth symbol could join the prefix: the test's premise is out of date"


def test_every_entry_is_four_steps_from_the_start_state():
    nxt, em, _ = _tables()
    s = int(nxt[ROOT, PAD])
    table = _prefix_table(nxt, s)
    for key in range(256):
        st = s
        for sym in (key & 3, (key >> 2) & 3, (key >> 4) & 3, (key >> 6) & 3):
            st = int(nxt[st, sym])
        assert table[key] == st, "key 0x%02x" % key
    assert (table >= 0).all() and (table < len(nxt)).all() and (table * 16 < 1 << 16).all()      # (a row offset fits the entry's 16 bits)
    other = int((_prefix_table(nxt, ROOT) != table).sum())
    print("the root's table differs from S's on %d of 256 keys" % other)
    assert other > 0 or s == ROOT


def _reported(ids, sets):
    return {(p, place - back) for place, i in enumerate(ids.tolist()) if i for p, back in sets[i]}


def _check(nxt, em, sets, cells_a, len_a, cells_b, len_b, what):
    """cells_x [n, max len] (what lies beyond a line's length is never looked at), len_x [n]; every len_a >= PREFIX"""
    n = len(len_a)
    rows = np.arange(n)
    assert (len_a >= PREFIX).all()
    width = int((len_a + len_b).max()) + 4 + 2                  # two filler symbols behind the longest stream
    stream = np.full((n, width), PAD, dtype=np.int64)
    ref = []
    for cells, length, at in ((cells_a, len_a, np.zeros(n, dtype=np.int64)), (cells_b, len_b, len_a + 2)):
        one = np.full((n, cells.shape[1] + 3), PAD, dtype=np.int64)
        for k in range(cells.shape[1]):
            on = k < length
            one[on, 1 + k] = cells[on, k]
            stream[rows[on], at[on] + k] = cells[on, k]
        r = _walk(nxt, em, one, ROOT)
        assert not r[:, 0].any()
        ref.append(r[:, 1:])                                    # place 0 = the first cell; places len and len + 1 are the trailing pads
    # the kernel: one read at the stream's first eight bits, then steps 4.. from the state it gives
    key = sum(stream[:, i] << (2 * i) for i in range(PREFIX))
    assert (stream[:, :PREFIX] != PAD).all() and (key < 256).all()
    got = _walk(nxt, em, stream, _prefix_table(nxt, int(nxt[ROOT, PAD]))[key], first=PREFIX)
    seg_a = (len_a + 2)[:, None]
    steps = np.arange(width)[None, :]
    second = steps >= seg_a
    place = steps - np.where(second, seg_a, 0)
    bad = 0
    for seg in (0, 1):
        mine = np.zeros_like(ref[seg])
        length = (len_a, len_b)[seg]
        inside = (second == bool(seg)) & (place < (length + 2)[:, None])
        r_idx, s_idx = np.nonzero(inside)
        mine[r_idx, place[r_idx, s_idx]] = got[r_idx, s_idx]
        beyond = np.arange(ref[seg].shape[1])[None, :] >= (length + 2)[:, None]
        assert not ref[seg][beyond].any()
        differ = np.nonzero((mine != ref[seg]).any(axis=1))[0]
        for i in differ:                                        # (ids are sets already: a difference is a different set; spelled out for the message)
            a, b = _reported(mine[i], sets), _reported(ref[seg][i], sets)
            assert a == b, "%s %d segment %d: stream %s, `? cells ? ?` %s" % (what, i, seg, sorted(a), sorted(b))
        bad += len(differ)
    outside = second & (place >= (len_b + 2)[:, None])
    assert not got[outside].any(), "%s: the filler reports a match" % what
    matches = sum(int((r != 0).sum()) for r in ref)
    early = int((ref[0][:, PREFIX] != 0).sum())
    print("%s: %d streams, %d emitting transitions, %d of them on the first step behind the prefix, %d segments differ" % (what, n, matches, early, bad))
    assert bad == 0
    return matches, early


def test_every_line_of_5_to_9_cells():
    nxt, em, sets = _tables()
    total = first = 0
    for length in range(5, 10):
        cells = np.array(list(itertools.product(CELLS, repeat=length)), dtype=np.int64)
        n = len(cells)
        assert n == 3 ** length
        none = np.zeros(n, dtype=np.int64)
        # alone (the lane's second job is "no line": no cells, two pads) and in front of its mirror image
        for m, e in (_check(nxt, em, sets, cells, none + length, np.zeros((n, 1), dtype=np.int64), none, "%d cells, alone" % length),
                     _check(nxt, em, sets, cells, none + length, cells[:, ::-1].copy(), none + length, "%d cells, in front of its mirror image" % length)):
            total += m
            first += e
    assert total > 0 and first > 0                              # (the step right behind the prefix does report: its push is needed)


def test_random_pairs_of_5_to_15_cells():
    nxt, em, sets = _tables()
    rng = np.random.default_rng(20252)
    n = 20000
    len_a, len_b = rng.integers(5, 16, n), rng.integers(5, 16, n)
    cells = []
    for _ in range(2):
        stone = rng.random((n, 15)) < rng.random((n, 1))       # every density, from empty to full
        cells.append(np.where(stone, rng.integers(0, 2, (n, 15)), 3).astype(np.int64))
    assert _check(nxt, em, sets, cells[0], len_a, cells[1], len_b, "random pairs")[0] > 10000
