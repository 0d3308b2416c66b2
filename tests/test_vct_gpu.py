"""K17 on the device, second half: the forced win by continuous threats (gmk_vct_solve) against the plain-Python restatement of its contract
(tests/vct_reference.py) -- its committed results on the random set (tests/golden/vct_cases.json), the hand positions of
tests/test_vct_reference.py with the numbers given there, and the restatement itself where it is quick.  Integer work on both sides: every
comparison is exact, over status, move, threats, positions and the whole pv."""
import functools
import random

import numpy as np
import pytest

import vcf_reference as R
import vct_reference as V
from gomokuai_amd import lib as G
from test_vcf_defend_gpu import Stub, board_after
from test_vcf_gpu import cell, full_board, interleave, pack
from test_vct_reference import DOUBLE_THREE, FOUR_THREE, OPEN_TWO, WHITE_FOUR, cases, limits

pytestmark = pytest.mark.gpu

FIELDS = ("status", "move", "threats", "positions")


@pytest.fixture(scope="module")
def gmk():
    G.init()
    return G


def row_of(out, i):
    """root i of a result as the committed cases write it: [status, move, threats, positions, pv]"""
    pv = [int(c) for c in out["pv"][i]]
    cells = pv.index(255) if 255 in pv else len(pv)
    assert all(c == 255 for c in pv[cells:]), "pv cells past the end are 255"
    return [int(out[k][i]) for k in FIELDS] + [pv[:cells]]


def wanted(q, max_depth, budget, iterative, max_threats, max_positions):
    r = V.vct_solve(q, max_depth, budget, iterative, max_threats, max_positions)
    return [r["status"], r["move"], r["threats"], r["positions"], r["pv"]]


def search(lists, max_depth, budget, iterative, max_threats, max_positions, stride=None, fill=0):
    moves, lens = pack(lists, stride, fill)
    out = G.vct_solve(moves, lens, max_depth, budget, iterative=iterative, max_threats=max_threats, max_positions=max_positions)
    return [row_of(out, i) for i in range(len(lists))]


def roots():
    return cases()["positions"][:cases()["roots"]]


def committed(k):
    """search k of the committed cases -> (its arguments for search(), its results)"""
    s = cases()["searches"][k]
    return (*limits(s["run"]), s["max_threats"], s["max_positions"]), s["results"]


SEARCHES = range(5)
DEEP_1, SHALLOW_1, DEEP_2, SHALLOW_2 = 0, 1, 2, 3


# ---------------- the random set and the hand positions against the restatement ----------------
def test_the_sets_cover_the_contract():
    """On the restatement alone: the committed searches end in NONE, WIN, DEPTH and VCT_BUDGET, T is 1 and 2, roots that hit max_positions
    stand among roots that do not, and wins have depth 0 and 1; the committed hand search adds a win of depth 2.  (OVER and BAD roots are
    in test_full_board_empty_board_and_over and test_bad_lists_do_not_disturb_their_neighbours.)"""
    statuses, depths, ts = set(), set(), set()
    for k in SEARCHES:
        args, results = committed(k)
        ts.add(args[3])
        here = {r[0] for r in results}
        statuses |= here
        depths |= {r[2] for r in results if r[0] == R.WIN}
        if args[3] == 2:
            assert V.VCT_BUDGET in here and len(here) >= 3
    assert statuses == {R.NONE, R.WIN, R.DEPTH, V.VCT_BUDGET} and {0, 1} <= depths and ts == {1, 2}
    assert cases()["hand"]["counter_four_2"][:3] == [R.WIN, 113, 2]


@pytest.mark.parametrize("k", SEARCHES)
def test_random_roots_match_the_restatement(gmk, k):
    args, want = committed(k)
    got = search(roots(), *args)
    wrong = [(i, got[i], want[i]) for i in range(len(want)) if got[i] != want[i]]
    assert not wrong, (len(wrong), wrong[:3])


def test_the_hand_positions(gmk):
    """The numbers of tests/test_vct_reference.py, which are the restatement's: the double three is won in one threat move after 47
    positions, the open two is cut after 11 and after 39, a four-three is K14's own line, nothing threatens against a four."""
    lists = [DOUBLE_THREE, OPEN_TWO, FOUR_THREE, WHITE_FOUR]
    own = R.solve(FOUR_THREE)
    for max_threats, open_two in ((1, 11), (2, 39)):
        assert search(lists, 16, 100000, False, max_threats, 4096) == [[R.WIN, 113, 1, 47, [113]], [R.DEPTH, -1, 0, open_two, []],
                                                                      [R.WIN, own["move"], 0, 1, own["pv"]], [R.NONE, -1, 0, 1, []]]
    assert search([DOUBLE_THREE], 16, 100000, True, 1, 4096) == [[R.WIN, 113, 1, 47, [113]]]


def test_a_counter_four_costs_a_threat_move(gmk):
    from golden.make_vct_cases import COUNTER_FOUR
    hand = cases()["hand"]
    assert search([COUNTER_FOUR], 16, 100000, False, 1, 1 << 20) == [hand["counter_four_1"][:5]]
    assert search([COUNTER_FOUR], 16, 100000, False, 2, 1 << 20) == [hand["counter_four_2"][:5]]
    assert hand["counter_four_2"][:5] == [R.WIN, 113, 2, sum(hand["counter_four_2"][5]), [113, cell(5, 12), cell(6, 12)]]
    assert search([COUNTER_FOUR], 16, 100000, False, 3, 1 << 20)[0][:3] == [R.WIN, 113, 2]      # a root with a depth is not searched further


def test_max_positions(gmk):
    """Level 1 of the open two has 10 positions and of the double three 46: a cap ends the one root and leaves the other alone, and the
    discarded level is not counted."""
    lists = [OPEN_TWO, DOUBLE_THREE, OPEN_TWO, []]
    assert search(lists, 16, 100000, False, 1, 9) == [[V.VCT_BUDGET, -1, 0, 1, []]] * 3 + [[R.NONE, -1, 0, 1, []]]
    assert search(lists, 16, 100000, False, 1, 10) == [[R.DEPTH, -1, 0, 11, []], [V.VCT_BUDGET, -1, 0, 1, []], [R.DEPTH, -1, 0, 11, []], [R.NONE, -1, 0, 1, []]]
    assert search(lists, 16, 100000, False, 2, 27) == [[V.VCT_BUDGET, -1, 0, 11, []], [V.VCT_BUDGET, -1, 0, 1, []], [V.VCT_BUDGET, -1, 0, 11, []], [R.NONE, -1, 0, 1, []]]
    assert search(lists, 16, 100000, False, 2, 46) == [[R.DEPTH, -1, 0, 39, []], [R.WIN, 113, 1, 47, [113]], [R.DEPTH, -1, 0, 39, []], [R.NONE, -1, 0, 1, []]]


# ---------------- batch seams ----------------
@functools.lru_cache(maxsize=None)
def alone():
    """each root in a call of its own"""
    args, _ = committed(SHALLOW_2)
    return [search([q], *args)[0] for q in roots()]


@pytest.mark.parametrize("n", [1, 3, 4, 5, 17, 65])
def test_a_batch_is_its_roots_alone(gmk, n):
    args, want = committed(SHALLOW_2)
    index = [(23 - i) % 24 for i in range(n)]
    assert search([roots()[i] for i in index], *args) == [alone()[i] for i in index]
    assert alone() == want


def test_order_in_the_batch_does_not_matter(gmk):
    index = list(range(24))
    random.Random(3).shuffle(index)
    for k in (DEEP_1, DEEP_2):
        args, want = committed(k)
        assert search([roots()[i] for i in index], *args) == [want[i] for i in index]


def test_stride_beyond_the_longest_list(gmk):
    args, want = committed(DEEP_1)
    assert search(roots(), *args, stride=97, fill=0xEE) == want


def test_full_board_empty_board_and_over(gmk):
    over = interleave([cell(x, 7) for x in range(2, 7)], [cell(0, 14), cell(4, 13), cell(9, 14), cell(14, 12)])
    lists = [full_board(), full_board()[:224], [], over, [112]]
    for iterative in (False, True):
        got = search(lists, 8, 1000, iterative, 2, 64)
        assert got == [[R.NONE, -1, 0, 1, []]] * 3 + [[R.OVER, -1, 0, 1, []], [R.NONE, -1, 0, 1, []]]
    assert wanted(lists[1], 8, 1000, False, 2, 64) == [R.NONE, -1, 0, 1, []] and wanted(over, 8, 1000, False, 2, 64) == [R.OVER, -1, 0, 1, []]


def test_bad_lists_do_not_disturb_their_neighbours(gmk):
    args, want = committed(SHALLOW_2)
    good = roots()[8:12]
    moves, lens = pack([good[0], [1, 2, 3], good[1], [4, 5], [7, 225, 9], [30, 31, 30], good[2], good[3]], stride=225)
    lens[1], lens[3] = -1, 226
    out = G.vct_solve(moves, lens, args[0], args[1], iterative=args[2], max_threats=args[3], max_positions=args[4])
    got = [row_of(out, i) for i in range(8)]
    assert [got[i] for i in (1, 3, 4, 5)] == [[R.BAD, -1, 0, 1, []]] * 4
    assert [got[i] for i in (0, 2, 6, 7)] == want[8:12]
    # a length above the stride cannot be a list of this buffer: refused the same way, nothing outside the row is read
    moves, lens = pack([good[0], [1, 2, 3]], stride=len(good[0]))
    lens[1] = len(good[0]) + 1
    out = G.vct_solve(moves, lens, args[0], args[1], iterative=args[2], max_threats=args[3], max_positions=args[4])
    assert [row_of(out, 0), row_of(out, 1)] == [want[8], [R.BAD, -1, 0, 1, []]]


def test_borders_and_corners(gmk):
    """Both colours along all four borders and into the corners: the committed border set (two stones of the side to move, black and white
    in turn) searched at T = 1 and 2, every output of every root compared with the restatement's committed row; the two corner-most roots
    also with the restatement itself."""
    borders = cases()["borders"]
    max_depth, budget, _ = borders["limits"]
    assert [s["max_threats"] for s in borders["searches"]] == [1, 2]
    for s in borders["searches"]:
        assert len(s["results"]) == 10 and all(r[3] > 1 for r in s["results"])
        assert search(borders["positions"], max_depth, budget, False, s["max_threats"], s["max_positions"]) == s["results"], s["max_threats"]
    for i in (4, 9):
        assert wanted(borders["positions"][i], max_depth, budget, False, 1, 64) == borders["searches"][0]["results"][i], i


# ---------------- the device form ----------------
def test_null_outputs_and_device_form_on_a_side_stream(gmk):
    """The device form on a stream of its own with every output and with some missing, and the host form: the same numbers, and what was not
    asked for is not touched.  The call has synchronised the stream when it returns."""
    import torch
    args, want = committed(SHALLOW_2)
    moves, lens = pack(roots())
    n = len(roots())
    d_moves, d_lens = torch.from_numpy(moves).cuda(), torch.from_numpy(lens).cuda()
    side = torch.cuda.Stream()
    host = G.vct_solve(moves, lens, args[0], args[1], iterative=args[2], max_threats=args[3], max_positions=args[4])
    assert [row_of(host, i) for i in range(n)] == want

    def run(which):
        bufs = {k: torch.full((n,), -7, dtype=torch.int32, device="cuda") for k in FIELDS}
        bufs["pv"] = torch.full((n, 80), 7, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ptr = {k: (v.data_ptr() if k in which else None) for k, v in bufs.items()}
        G.vct_solve_device(d_moves.data_ptr(), moves.shape[1], d_lens.data_ptr(), n, args[0], args[1], iterative=args[2], max_threats=args[3],
                           max_positions=args[4], d_status=ptr["status"], d_move=ptr["move"], d_threats=ptr["threats"], d_positions=ptr["positions"],
                           d_pv=ptr["pv"], stream=side.cuda_stream)
        return {k: v.cpu().numpy() for k, v in bufs.items()}

    for which in (FIELDS + ("pv",), ("status", "pv"), ("positions",), ("move", "threats"), ()):
        part = run(which)
        for k in part:
            if k in which:
                assert (part[k].astype(np.int64) == host[k].astype(np.int64)).all(), (which, k)
            else:
                assert (part[k] == (7 if k == "pv" else -7)).all(), (which, k)      # untouched


def test_arguments(gmk):
    import torch
    L = G.load()
    moves, lens = pack(roots()[:4])
    d_moves, d_lens = torch.from_numpy(moves).cuda(), torch.from_numpy(lens).cuda()
    out = torch.zeros(1024, dtype=torch.int32, device="cuda")
    m, l, o, s = d_moves.data_ptr(), d_lens.data_ptr(), out.data_ptr(), moves.shape[1]
    ARG = -3

    def call(moves_=m, stride=s, lens_=l, n=4, max_depth=3, budget=8, flags=0, max_threats=1, max_positions=64, status=o, move=None, threats=None,
             positions=None, pv=None):
        return L.gmk_vct_solve(moves_, stride, lens_, n, max_depth, budget, flags, max_threats, max_positions, status, move, threats, positions, pv, None)

    assert call() == 0
    assert call(move=o + 64, threats=o + 128, positions=o + 192, pv=o + 1024) == 0
    assert call(status=None) == 0                                  # every output may be NULL
    assert call(n=0) == 0 and call(n=0, moves_=None, lens_=None) == 0
    assert call(moves_=None) == ARG and call(lens_=None) == ARG
    assert call(n=-1) == ARG
    assert call(stride=0) == ARG and call(stride=-5) == ARG
    assert call(max_depth=0) == ARG and call(max_depth=33) == ARG
    assert call(flags=1) == ARG and call(flags=3) == ARG and call(flags=4) == ARG and call(flags=-1) == ARG and call(flags=2) == 0
    assert call(max_threats=0) == ARG and call(max_threats=9) == ARG and call(max_threats=-1) == ARG and call(max_threats=8, max_positions=2) == 0
    assert call(max_positions=0) == ARG and call(max_positions=-4) == ARG and call(max_positions=1) == 0
    assert call(lens_=l + 2) == ARG
    for name in FIELDS:
        assert call(**{name: o + 2}) == ARG, name
    assert call(pv=o + 1025, moves_=m + 1, stride=s - 1) == 0       # the byte arrays need no alignment
    assert b"gmk_vct_solve" in L.gmk_last_error()
    h_moves, h_lens = moves.ctypes.data, lens.ctypes.data
    status = np.zeros(4, np.int32)

    def host(moves_=h_moves, stride=s, lens_=h_lens, n=4, max_depth=3, flags=0, max_threats=2, max_positions=24):
        return L.gmk_vct_solve_host(moves_, stride, lens_, n, max_depth, 8, flags, max_threats, max_positions, status.ctypes.data, None, None, None, None)

    assert host(moves_=None) == ARG and host(lens_=None) == ARG and host(stride=0) == ARG and host(n=-1) == ARG and host(max_depth=33) == ARG
    assert host(flags=1) == ARG and host(flags=8) == ARG and host(max_threats=0) == ARG and host(max_threats=9) == ARG and host(max_positions=0) == ARG
    assert host(n=0) == 0 and host() == 0
    assert [int(v) for v in status] == [r[0] for r in committed(SHALLOW_2)[1][:4]]


# ---------------- the agent ----------------
def test_agent_plays_the_double_three(gmk):
    from gomokuai_amd import interface
    board = board_after(DOUBLE_THREE)
    stub = Stub(30)
    agent = interface.VCFAgent(stub, threats=1)
    agent.sync_with_board(board)
    assert int(agent.get_action(board).id) == 113 and stub.asked == 1      # the inner agent was still asked: its tree stays in step
    message = agent.debug_message()
    assert message["vct"] == {"status": "WIN", "move": 113, "threats": 1, "positions": 47, "pv": [113]}
    assert message["vcf"]["status"] == "NONE" and message["stub"] == 30
    for defend in (False, True):
        wrapped = interface.make_agent("pattern", vcf=16, vcf_defend=defend, vct=2)
        assert type(wrapped) is interface.VCFAgent and wrapped.threats == 2 and wrapped.defend is defend
        wrapped.sync_with_board(board)
        assert int(wrapped.get_action(board).id) == 113


def test_agent_without_threats_plays_the_inner_move(gmk):
    from gomokuai_amd import interface
    board = board_after(DOUBLE_THREE)
    for agent in (interface.VCFAgent(Stub(30), threats=0), interface.VCFAgent(Stub(30))):
        agent.sync_with_board(board)
        assert int(agent.get_action(board).id) == 30 and "vct" not in agent.debug_message()
    # a search that finds no win leaves the inner move, and reports
    quiet = board_after(OPEN_TWO)
    agent = interface.VCFAgent(Stub(30), threats=1)
    agent.sync_with_board(quiet)
    assert int(agent.get_action(quiet).id) == 30
    assert agent.debug_message()["vct"] == {"status": "DEPTH", "move": -1, "threats": 0, "positions": 11, "pv": []}
    # a win by fours is played before anything else is asked
    won = board_after(FOUR_THREE)
    stub = Stub(30)
    agent = interface.VCFAgent(stub, threats=1)
    agent.sync_with_board(won)
    assert int(agent.get_action(won).id) == cell(7, 7) and stub.asked == 0 and "vct" not in agent.debug_message()
