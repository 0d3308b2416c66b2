"""K17 on the device, first half: what a stone of the side to move threatens on every cell (gmk_vcf_threats) against the plain-Python
restatement of its contract (tests/vct_reference.py) -- its committed results on the random set (tests/golden/vct_cases.json) and the
restatement itself on the hand positions.  Integer work on both sides: every comparison is exact, over the own status, move, length, nodes and
whole pv and over the verdict, length and nodes of all 225 cells."""
import functools
import random

import numpy as np
import pytest

import vcf_reference as R
import vct_reference as V
from gomokuai_amd import lib as G
from test_vcf_gpu import cell, full_board, interleave, pack
from test_vct_reference import DOUBLE_THREE, FOUR_THREE, WHITE_FOUR, cases, limits
from test_vct_reference import FAR as EDGE

pytestmark = pytest.mark.gpu

RUNS = ("shallow", "deep")          # the committed runs: (3, 8) on all 40 positions, (8, 2000) on the first 8; iterative is checked live


@pytest.fixture(scope="module")
def gmk():
    G.init()
    return G


def row_of(out, i):
    """position i of a result as wanted() writes the restatement's"""
    length = int(out["own_length"][i])
    pv = out["own_pv"][i]
    cells = 2 * length - 1 if length else 0
    assert (pv[cells:] == 255).all(), "pv cells past the end are 255"
    return {"own": [int(out["own_status"][i]), int(out["own_move"][i]), length, int(out["own_nodes"][i]), [int(c) for c in pv[:cells]]],
            "verdict": [int(v) for v in out["verdict"][i]], "length": [int(v) for v in out["length"][i]], "nodes": [int(v) for v in out["nodes"][i]]}


def wanted(q, max_depth, budget, iterative=False):
    t = V.threats(q, max_depth, budget, iterative)
    own = t["own"]
    return {"own": [own["status"], own["move"], own["length"], own["nodes"], list(own["pv"])], "verdict": t["verdict"], "length": t["length"], "nodes": t["nodes"]}


def threats(lists, max_depth, budget, iterative=False, stride=None, fill=0):
    moves, lens = pack(lists, stride, fill)
    out = G.vcf_threats(moves, lens, max_depth, budget, iterative=iterative)
    return [row_of(out, i) for i in range(len(lists))]


def differing(got, want):
    return [(i, [k for k in want[i] if got[i][k] != want[i][k]]) for i in range(len(want)) if got[i] != want[i]]


def selection():
    return cases()["positions"]


def reference(run):
    """the committed results of the restatement, as rows"""
    return [{k: t[k] for k in ("own", "verdict", "length", "nodes")} for t in cases()["threats"][run]]


# the double three, the four-three, white's four (IGNORES), black's four closed on one side with black to move (FIVE) and with white to move
# (IGNORES but for the block), black's open three (FOUR cells of length 1 and 2)
BLACK_FOUR = interleave([110, 111, 112, 113], [109, EDGE[1], EDGE[2], EDGE[3]])
HAND = [DOUBLE_THREE, FOUR_THREE, WHITE_FOUR, BLACK_FOUR, BLACK_FOUR + [EDGE[0]], interleave([110, 111, 112, EDGE[0]], [EDGE[4], EDGE[1], EDGE[2], EDGE[3]])]


# ---------------- the random set and the hand positions against the restatement ----------------
def test_the_sets_cover_the_contract():
    """On the restatement alone: the committed random set has NONE, QUIET, WINS, UNKNOWN and FOUR, cells with nodes, and every status a search
    of the side to move can end in; the hand positions add FIVE and IGNORES."""
    verdicts, statuses, with_nodes = set(), set(), 0
    for run in RUNS:
        for r in reference(run):
            verdicts |= set(r["verdict"])
            statuses.add(r["own"][0])
            with_nodes += sum(v > 0 for v in r["nodes"])
    assert verdicts == {V.THREAT_NONE, V.THREAT_QUIET, V.THREAT_WINS, V.THREAT_UNKNOWN, V.THREAT_FOUR} and with_nodes >= 1000
    assert statuses == {R.NONE, R.WIN, R.DEPTH, R.BUDGET}
    hand = set()
    for r in hand_reference():
        hand |= set(r["verdict"])
    assert {V.THREAT_FIVE, V.THREAT_IGNORES, V.THREAT_FOUR, V.THREAT_WINS, V.THREAT_QUIET} <= hand


@functools.lru_cache(maxsize=None)
def hand_reference():
    return [wanted(q, 16, 100000) for q in HAND]


@pytest.mark.parametrize("run", RUNS)
def test_random_positions_match_the_restatement(gmk, run):
    want = reference(run)
    wrong = differing(threats(selection()[:len(want)], *limits(run)), want)
    assert not wrong, (len(wrong), wrong[:5])


def test_iterative_matches_the_restatement(gmk):
    pool = [selection()[i] for i in (3, 17, 30)]
    assert threats(pool, *limits("deep_iterative")) == [wanted(q, *limits("deep_iterative")) for q in pool]


def test_hand_positions_match_the_restatement(gmk):
    got = threats(HAND, 16, 100000)
    assert got == hand_reference()
    assert sum(v == V.THREAT_WINS for v in got[0]["verdict"]) == 18 and got[0]["own"][0] == R.NONE       # the double three
    assert threats(HAND[:1], 16, 100000, iterative=True) == [wanted(q, 16, 100000, True) for q in HAND[:1]]


def test_the_own_verdict_is_the_solver(gmk):
    pool = selection() + HAND
    moves, lens = pack(pool)
    for run in ("deep", "shallow", "deep_iterative"):
        max_depth, budget, iterative = limits(run)
        out = G.vcf_threats(moves, lens, max_depth, budget, iterative=iterative)
        own = G.vcf_solve(moves, lens, max_depth, budget, iterative=iterative)
        for name in ("status", "move", "length", "nodes", "pv"):
            assert out["own_" + name].dtype == own[name].dtype and (out["own_" + name] == own[name]).all(), (run, name)


# ---------------- batch seams ----------------
@functools.lru_cache(maxsize=None)
def alone():
    """each position of the selection in a launch of its own"""
    return [threats([q], *limits("shallow"))[0] for q in selection()]


@pytest.mark.parametrize("n", [1, 3, 4, 5, 17, 65])
def test_a_batch_is_its_positions_alone(gmk, n):
    index = [(39 - i) % 40 for i in range(n)]                    # the tail of the set first: the heavy positions are there
    got = threats([selection()[i] for i in index], *limits("shallow"))
    assert got == [alone()[i] for i in index]
    assert alone() == reference("shallow")


def test_order_in_the_batch_does_not_matter(gmk):
    index = list(range(40))
    random.Random(3).shuffle(index)
    assert threats([selection()[i] for i in index], *limits("shallow")) == [reference("shallow")[i] for i in index]


def test_a_large_batch(gmk):
    """Above 32 jobs per compute unit a wavefront's slice is 64 jobs, not four, and a group keeps a position's planes over its cells."""
    times = 8
    assert 40 * times * 225 > 32 * G.device_info()["cu_count"]
    assert threats(selection() * times, *limits("shallow")) == reference("shallow") * times


def test_stride_beyond_the_longest_list(gmk):
    assert threats(selection(), *limits("shallow"), stride=97, fill=0xEE) == reference("shallow")


def test_full_board_one_empty_cell_and_the_empty_board(gmk):
    lists = [full_board(), full_board()[:224], [], [112]]
    want = [wanted(q, 8, 1000) for q in lists]
    assert want[0]["verdict"] == [V.THREAT_NONE] * 225 and sum(v != V.THREAT_NONE for v in want[1]["verdict"]) == 1
    assert want[2]["verdict"] == [V.THREAT_QUIET] * 225
    for iterative in (False, True):
        assert threats(lists, 8, 1000, iterative) == [wanted(q, 8, 1000, iterative) for q in lists]


# ---------------- rows and corners ----------------
def test_threats_along_the_borders_and_into_the_corners(gmk):
    """The committed border set: two stones of the side to move (the third makes a three: WINS cells) along all four borders, touching the
    corners and on the diagonals into them, black and white in turn."""
    borders = cases()["borders"]
    want = [{k: t[k] for k in ("own", "verdict", "length", "nodes")} for t in borders["threats"]]
    assert len(want) == 10 and [len(q) % 2 for q in borders["positions"]] == [0, 1] * 5
    assert all(V.THREAT_WINS in r["verdict"] and r["own"][0] == R.NONE for r in want)
    max_depth, budget, iterative = borders["limits"]
    wrong = differing(threats(borders["positions"], max_depth, budget, bool(iterative)), want)
    assert not wrong, (len(wrong), wrong[:5])
    for i in (4, 9):                                              # into the corners, against the restatement itself, iterative
        assert threats([borders["positions"][i]], max_depth, budget, True) == [wanted(borders["positions"][i], max_depth, budget, True)], i


@pytest.mark.parametrize("colour", [1, 2])
def test_rows_do_not_wrap(gmk, colour):
    """(13,3), (14,3), (0,4), (1,4): four consecutive cell ids and no line; nor (12,3) .. (14,3), (0,4)"""
    traps = [[cell(13, 3), cell(14, 3), cell(0, 4), cell(1, 4)], [cell(12, 3), cell(13, 3), cell(14, 3), cell(0, 4)]]
    scattered = [cell(7, 7), cell(3, 9), cell(11, 6), cell(6, 11), cell(9, 12)]
    lists = [interleave(t, scattered[:4]) if colour == 1 else interleave(scattered, t) for t in traps]
    got = threats(lists, 8, 1000)
    assert V.THREAT_FIVE not in got[0]["verdict"] and V.THREAT_FOUR not in got[0]["verdict"]
    assert got == [wanted(q, 8, 1000) for q in lists]


def test_bad_lists_do_not_disturb_their_neighbours(gmk):
    good = selection()[4:8]
    moves, lens = pack([good[0], [1, 2, 3], good[1], [4, 5], [7, 225, 9], [30, 31, 30], good[2], good[3]], stride=225)
    lens[1], lens[3] = -1, 226
    out = G.vcf_threats(moves, lens, *limits("deep")[:2])
    got = [row_of(out, i) for i in range(8)]
    bad = {"own": [R.BAD, -1, 0, 0, []], "verdict": [0] * 225, "length": [0] * 225, "nodes": [0] * 225}
    assert [got[i] for i in (1, 3, 4, 5)] == [bad] * 4
    assert [got[i] for i in (0, 2, 6, 7)] == reference("deep")[4:8]
    # a length above the stride cannot be a list of this buffer: refused the same way, nothing outside the row is read
    moves, lens = pack([good[0], [1, 2, 3]], stride=len(good[0]))
    lens[1] = len(good[0]) + 1
    out = G.vcf_threats(moves, lens, *limits("deep")[:2])
    assert [row_of(out, 0), row_of(out, 1)] == [reference("deep")[4], bad]


def test_over_is_settled_by_one_job(gmk):
    over = interleave([cell(x, 7) for x in range(2, 7)], [cell(0, 14), cell(4, 13), cell(9, 14), cell(14, 12)])
    got = threats([selection()[0], over, selection()[1]], *limits("deep")[:2])
    assert got[1] == {"own": [R.OVER, -1, 0, 0, []], "verdict": [0] * 225, "length": [0] * 225, "nodes": [0] * 225}
    assert [got[0], got[2]] == reference("deep")[:2]


# ---------------- the device form ----------------
OPTIONAL = ("own_move", "own_length", "own_nodes", "own_pv", "length", "nodes")


def test_null_outputs_and_device_form_on_a_side_stream(gmk):
    """The device form on a stream of its own with every output and with optional ones missing, and the host form: the same numbers, and what
    was not asked for is not touched."""
    import torch
    pool = selection()
    moves, lens = pack(pool)
    n = len(pool)
    max_depth, budget, _ = limits("shallow")
    d_moves, d_lens = torch.from_numpy(moves).cuda(), torch.from_numpy(lens).cuda()
    side = torch.cuda.Stream()
    host = G.vcf_threats(moves, lens, max_depth, budget)
    assert [row_of(host, i) for i in range(n)] == reference("shallow")

    def run(which):
        bufs = {k: torch.full((n,), -7, dtype=torch.int32, device="cuda") for k in ("own_status", "own_move", "own_length", "own_nodes")}
        bufs.update({"own_pv": torch.full((n, 64), 7, dtype=torch.uint8, device="cuda"), "verdict": torch.full((n, 225), 7, dtype=torch.uint8, device="cuda"),
                     "length": torch.full((n, 225), 7, dtype=torch.uint8, device="cuda"), "nodes": torch.full((n, 225), -7, dtype=torch.int32, device="cuda")})
        torch.cuda.synchronize()
        ptr = {k: (v.data_ptr() if k not in OPTIONAL or k in which else None) for k, v in bufs.items()}
        G.vcf_threats_device(d_moves.data_ptr(), moves.shape[1], d_lens.data_ptr(), n, max_depth, budget, d_own_status=ptr["own_status"],
                             d_own_move=ptr["own_move"], d_own_length=ptr["own_length"], d_own_nodes=ptr["own_nodes"], d_own_pv=ptr["own_pv"],
                             d_verdict=ptr["verdict"], d_cell_length=ptr["length"], d_cell_nodes=ptr["nodes"], stream=side.cuda_stream)
        side.synchronize()
        return {k: v.cpu().numpy() for k, v in bufs.items()}

    for which in (OPTIONAL, (), ("own_pv", "nodes"), ("own_move", "length"), ("own_length", "own_nodes")):
        part = run(which)
        for k in part:
            if k not in OPTIONAL or k in which:
                assert (part[k].astype(np.int64) == host[k].astype(np.int64)).all(), (which, k)
            else:
                assert (part[k] == (7 if part[k].dtype == np.uint8 else -7)).all(), (which, k)      # untouched


def test_arguments(gmk):
    import torch
    L = G.load()
    moves, lens = pack(selection()[:4])
    d_moves, d_lens = torch.from_numpy(moves).cuda(), torch.from_numpy(lens).cuda()
    out = torch.zeros(4096, dtype=torch.int32, device="cuda")
    m, l, o, s = d_moves.data_ptr(), d_lens.data_ptr(), out.data_ptr(), moves.shape[1]
    # status at o, move at o + 64, length at o + 128, nodes at o + 192, pv at o + 1024 (256 B), verdict at o + 2048 (900 B), cell length at o + 3072,
    # cell nodes at o + 4096 (3600 B)
    ARG = -3

    def call(moves_=m, stride=s, lens_=l, n=4, max_depth=8, budget=100, flags=0, status=o, move=None, length=None, nodes=None, pv=None, verdict=o + 2048,
             cell_length=None, cell_nodes=None):
        return L.gmk_vcf_threats(moves_, stride, lens_, n, max_depth, budget, flags, status, move, length, nodes, pv, verdict, cell_length, cell_nodes, None)

    assert call() == 0
    assert call(move=o + 64, length=o + 128, nodes=o + 192, pv=o + 1024, cell_length=o + 3072, cell_nodes=o + 4096) == 0
    assert call(n=0) == 0 and call(n=0, moves_=None, lens_=None, status=None, verdict=None) == 0
    assert call(moves_=None) == ARG and call(lens_=None) == ARG
    assert call(status=None) == ARG and call(verdict=None) == ARG
    assert call(n=-1) == ARG
    assert call(stride=0) == ARG and call(stride=-5) == ARG
    assert call(max_depth=0) == ARG and call(max_depth=33) == ARG and call(max_depth=-1) == ARG
    assert call(max_depth=1) == 0 and call(max_depth=32) == 0
    assert call(flags=1) == ARG and call(flags=3) == ARG and call(flags=4) == ARG and call(flags=-1) == ARG and call(flags=2) == 0
    assert call(lens_=l + 2) == ARG
    for name, at in (("status", 2), ("move", 66), ("length", 130), ("nodes", 194), ("cell_nodes", 4098)):
        assert call(**{name: o + at}) == ARG, name
    assert call(pv=o + 1025, verdict=o + 2049, cell_length=o + 3073, moves_=m + 1, stride=s - 1) == 0       # the byte arrays need no alignment
    torch.cuda.synchronize()
    assert b"gmk_vcf_threats" in L.gmk_last_error()
    h_moves, h_lens = moves.ctypes.data, lens.ctypes.data
    status, verdict = np.zeros(4, np.int32), np.zeros((4, 225), np.uint8)
    S, V_ = status.ctypes.data, verdict.ctypes.data

    def host(moves_=h_moves, stride=s, lens_=h_lens, n=4, max_depth=8, flags=0, status_=S, verdict_=V_):
        return L.gmk_vcf_threats_host(moves_, stride, lens_, n, max_depth, 100, flags, status_, None, None, None, None, verdict_, None, None)

    assert host(moves_=None) == ARG and host(lens_=None) == ARG and host(stride=0) == ARG and host(n=-1) == ARG and host(max_depth=33) == ARG
    assert host(flags=1) == ARG and host(flags=8) == ARG
    assert host(status_=None) == ARG and host(verdict_=None) == ARG
    assert host(n=0) == 0 and host() == 0 and host(flags=2) == 0
    want = [wanted(q, 8, 100, True) for q in selection()[:4]]
    assert [int(v) for v in status] == [r["own"][0] for r in want] and [[int(v) for v in verdict[i]] for i in range(4)] == [r["verdict"] for r in want]
