"""K1's scan walks a lane's one or two lines as ONE symbol stream without leading pads, `cellsA ? ? cellsB ? ? ? ...`, from the state S the
root reaches on '?' (eval_kernel.hip, phase 1).  On the CPU, with the host's transition table (lib.tables_copy): the three properties of the
automaton that allow it -- the host checks the same three when it builds the kernel's image and refuses a table without them -- and that the
stream reports, segment by segment, exactly the (pattern, end cell, segment) set that `? cells ? ?` reports from the root: for every line of
5 to 9 cells over {black, white, blank} and for 20 000 seeded random pairs of lines of 5 to 15 cells of every density.

Symbols are the device's codes: 0 black, 1 white, 2 '?' (off the board), 3 blank.  A transition's emissions are a list of (pattern, back):
the match ends on the symbol just consumed (back 0) or on the one before it (back 1), so its end cell is the symbol's place in its segment
minus back.  The kernel finds segment and place from the step as mirrored here: with seg_a = len_a + 2 symbols in the first segment, step s
belongs to the second segment iff s >= seg_a, and its place is s - (second ? seg_a : 0)."""
import itertools

import numpy as np

from gomokuai_amd import lib as G

PAD, ROOT = 2, 0


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


def _start(nxt, em):
    return int(nxt[ROOT, PAD])


def test_the_three_properties_the_stream_rests_on():
    nxt, em, _ = _tables()
    n = len(nxt)
    s = _start(nxt, em)
    print("states %d, the root goes to state %d on '?'" % (n, s))
    assert em[ROOT, PAD] == 0, "the root emits on '?'"
    assert nxt[s, PAD] == s and em[s, PAD] == 0, "state %d does not loop on '?' without emitting" % s
    image = nxt[nxt[:, PAD], PAD]
    assert (image == s).all(), "'??' leads to states %s, not to %d alone" % (sorted(set(image.tolist())), s)


def _walk(nxt, em, syms, state):
    """syms [n, steps] -> the emission id of every step, [n, steps]"""
    out = np.zeros(syms.shape, dtype=np.int64)
    st = np.full(len(syms), state, dtype=np.int64)
    for k in range(syms.shape[1]):
        out[:, k] = em[st, syms[:, k]]
        st = nxt[st, syms[:, k]]
    return out


def _reported(ids, sets):
    """the (pattern, end cell) pairs of one segment from its per-place emission ids"""
    return {(p, place - back) for place, i in enumerate(ids.tolist()) if i for p, back in sets[i]}


def _check(nxt, em, sets, cells_a, len_a, cells_b, len_b, what):
    """cells_x [n, max len] (blank beyond a line's length is never looked at), len_x [n]"""
    n = len(len_a)
    rows = np.arange(n)
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
    got = _walk(nxt, em, stream, _start(nxt, em))
    # the kernel's step -> (segment, place)
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
    # nothing is reported outside the two segments (the filler)
    outside = second & (place >= (len_b + 2)[:, None])
    assert not got[outside].any(), "%s: the filler reports a match" % what
    matches = sum(int((r != 0).sum()) for r in ref)
    late = sum(int((r[rows, l + 1] != 0).sum()) for r, l in zip(ref, (len_a, len_b)))
    print("%s: %d streams, %d emitting transitions, %d of them on the second trailing pad, %d segments differ" % (what, n, matches, late, bad))
    assert bad == 0
    return matches


def test_every_line_of_5_to_9_cells():
    nxt, em, sets = _tables()
    total = 0
    for length in range(5, 10):
        cells = np.array(list(itertools.product((0, 1, 3), repeat=length)), dtype=np.int64)
        n = len(cells)
        assert n == 3 ** length
        none = np.zeros(n, dtype=np.int64)
        # alone (the lane's second job is "no line": no cells, two pads) and as the second segment behind itself reversed
        total += _check(nxt, em, sets, cells, none + length, np.zeros((n, 1), dtype=np.int64), none, "%d cells, alone" % length)
        total += _check(nxt, em, sets, cells[:, ::-1].copy(), none + length, cells, none + length, "%d cells, behind its mirror image" % length)
    assert total > 0


def test_random_pairs_of_5_to_15_cells():
    nxt, em, sets = _tables()
    rng = np.random.default_rng(20251)
    n = 20000
    len_a, len_b = rng.integers(5, 16, n), rng.integers(5, 16, n)
    cells = []
    for _ in range(2):
        stone = rng.random((n, 15)) < rng.random((n, 1))       # every density, from empty to full
        cells.append(np.where(stone, rng.integers(0, 2, (n, 15)), 3).astype(np.int64))
    assert _check(nxt, em, sets, cells[0], len_a, cells[1], len_b, "random pairs") > 10000
