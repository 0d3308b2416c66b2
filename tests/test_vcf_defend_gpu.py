"""K15 on the device: the defence against a forced win by continuous fours (gmk_vcf_defend) against the plain-Python restatement of its
contract (tests/vcf_defend_reference.py).  Integer work on both sides: every comparison is exact, over the threat's status, length, nodes and
whole pv and over the verdict, length and nodes of all 225 cells."""
import functools
import random

import numpy as np
import pytest

import vcf_defend_reference as DR
import vcf_reference as R
from gomokuai_amd import lib as G
from test_vcf_gpu import BORDER_LINES, FAR, SHAPES, cell, full_board, interleave, pack, positions

pytestmark = pytest.mark.gpu

# (max_depth, budget, iterative)
RUNS = {"deep_iterative": (12, 5000, True), "shallow": (3, 8, False), "medium": (6, 40, False)}
OPEN_THREE = [cell(5, 7), cell(0, 0), cell(6, 7), cell(14, 0), cell(7, 7)]


@pytest.fixture(scope="module")
def gmk():
    G.init()
    return G


def row_of(out, i):
    """position i of a result as wanted() writes the restatement's"""
    length = int(out["threat_length"][i])
    pv = out["threat_pv"][i]
    cells = 2 * length - 1 if length else 0
    assert (pv[cells:] == 255).all(), "pv cells past the end are 255"
    return {"status": int(out["threat_status"][i]), "threat_length": length, "threat_nodes": int(out["threat_nodes"][i]), "pv": [int(c) for c in pv[:cells]],
            "verdict": [int(v) for v in out["verdict"][i]], "length": [int(v) for v in out["length"][i]], "nodes": [int(v) for v in out["nodes"][i]]}


def wanted(q, max_depth, budget, iterative=False):
    d = DR.defend(q, max_depth, budget, iterative)
    t = d["threat"]
    return {"status": t["status"], "threat_length": t["length"], "threat_nodes": t["nodes"], "pv": list(t["pv"]),
            "verdict": d["verdict"], "length": d["length"], "nodes": d["nodes"]}


def defend(lists, max_depth, budget, iterative=False, stride=None, fill=0):
    moves, lens = pack(lists, stride, fill)
    out = G.vcf_defend(moves, lens, max_depth, budget, iterative=iterative)
    return [row_of(out, i) for i in range(len(lists))]


def differing(got, want):
    return [(i, [k for k in want[i] if got[i][k] != want[i][k]]) for i in range(len(want)) if got[i] != want[i]]


@functools.lru_cache(maxsize=None)
def selection():
    """the first 12 positions of each of the six shapes"""
    return [positions()[60 * k + i] for k in range(len(SHAPES)) for i in range(12)]


@functools.lru_cache(maxsize=None)
def reference(run):
    return [wanted(q, *RUNS[run]) for q in selection()]


# ---------------- random sets against the restatement ----------------
def test_the_random_sets_cover_the_contract():
    """On the restatement alone: every status a threat's search can end in occurs over the runs; HOLDS, LOSES, UNKNOWN and cells with nodes at
    least 100 times each; losing lengths 2 to 5."""
    statuses, lengths = set(), set()
    count = {v: 0 for v in (DR.CELL_HOLDS, DR.CELL_LOSES, DR.CELL_UNKNOWN)}
    with_nodes = 0
    for run in RUNS:
        for r in reference(run):
            statuses.add(r["status"])
            for c in range(225):
                v = r["verdict"][c]
                if v in count:
                    count[v] += 1
                if v == DR.CELL_LOSES:
                    lengths.add(r["length"][c])
                with_nodes += r["nodes"][c] > 0
    assert {R.NONE, R.WIN, R.DEPTH, R.BUDGET} <= statuses, statuses
    assert all(v >= 100 for v in count.values()) and with_nodes >= 100, (count, with_nodes)
    assert {2, 3, 4, 5} <= lengths, sorted(lengths)


@pytest.mark.parametrize("run", list(RUNS))
def test_random_positions_match_the_restatement(gmk, run):
    max_depth, budget, iterative = RUNS[run]
    wrong = differing(defend(selection(), max_depth, budget, iterative), reference(run))
    assert not wrong, (len(wrong), wrong[:5])


def test_unfiltered_openings_match_the_restatement(gmk):
    """The sets above hold no position with a completing cell; whole random-opening lists do: FIVE cells, fours at the root, finished games."""
    moves, lens, _ = G.synth_boards(48, 0, first_board=0)
    lists = [[int(c) for c in moves[i, :lens[i]]] for i in range(48)]
    want = [wanted(q, 6, 60) for q in lists]
    wrong = differing(defend(lists, 6, 60), want)
    assert not wrong, (len(wrong), wrong[:5])
    assert any(DR.CELL_FIVE in r["verdict"] for r in want)
    assert any(r["status"] == R.WIN and r["threat_length"] == 1 for r in want) and any(r["status"] == R.OVER for r in want)


def test_the_threat_is_the_solver_with_opponent(gmk):
    moves, lens = pack(selection())
    for run in ("deep_iterative", "medium"):
        max_depth, budget, iterative = RUNS[run]
        out = G.vcf_defend(moves, lens, max_depth, budget, iterative=iterative)
        threat = G.vcf_solve(moves, lens, max_depth, budget, opponent=True, iterative=iterative)
        for ours, theirs in (("threat_status", "status"), ("threat_length", "length"), ("threat_nodes", "nodes"), ("threat_pv", "pv")):
            assert out[ours].dtype == threat[theirs].dtype and (out[ours] == threat[theirs]).all(), (run, ours)


# ---------------- batch seams ----------------
@functools.lru_cache(maxsize=None)
def alone():
    """each position of the selection in a launch of its own"""
    return [defend([q], *RUNS["shallow"])[0] for q in selection()]


@pytest.mark.parametrize("n", [1, 3, 4, 5, 16, 17, 65, 257])
def test_a_batch_is_its_positions_alone(gmk, n):
    index = [(71 - i) % 72 for i in range(n)]                    # the tail of the set first: the heavy positions are there
    got = defend([selection()[i] for i in index], *RUNS["shallow"])
    assert got == [alone()[i] for i in index]
    assert alone() == reference("shallow")


def test_order_in_the_batch_does_not_matter(gmk):
    index = list(range(72))
    random.Random(3).shuffle(index)
    assert defend([selection()[i] for i in index], *RUNS["medium"]) == [reference("medium")[i] for i in index]


def test_a_heavy_position_among_trivial_ones(gmk):
    want = reference("deep_iterative")
    heavy = max(range(72), key=lambda i: sum(want[i]["nodes"]))
    assert sum(want[heavy]["nodes"]) >= 1000
    trivial = [[], [112], selection()[0], [112, 113]]
    small = [wanted(q, *RUNS["deep_iterative"]) for q in trivial]
    order = [0, 1, 2] * 7 + [None] + [0, 3] * 20                  # the heavy one is the 22nd of 62
    got = defend([selection()[heavy] if k is None else trivial[k] for k in order], *RUNS["deep_iterative"])
    assert got == [want[heavy] if k is None else small[k] for k in order]


def test_stride_beyond_the_longest_list(gmk):
    assert defend(selection()[20:60], *RUNS["medium"], stride=97, fill=0xEE) == reference("medium")[20:60]


def test_full_board_one_empty_cell_and_the_empty_board(gmk):
    lists = [full_board(), full_board()[:224], [], OPEN_THREE]
    want = [wanted(q, 8, 1000) for q in lists]
    assert want[0]["verdict"] == [DR.CELL_NONE] * 225 and sum(v != DR.CELL_NONE for v in want[1]["verdict"]) == 1
    assert want[2]["verdict"] == [DR.CELL_HOLDS] * 225
    for iterative in (False, True):
        assert defend(lists, 8, 1000, iterative) == [wanted(q, 8, 1000, iterative) for q in lists]


def test_the_open_three_by_hand(gmk):
    r = defend([OPEN_THREE], 8, 1000)[0]
    assert (r["status"], r["pv"], r["threat_length"], r["threat_nodes"]) == (R.WIN, [109, 108, 113], 2, 4)
    assert [c for c in range(225) if r["verdict"][c] == DR.CELL_HOLDS] == [109, 113]
    loses = [c for c in range(225) if r["verdict"][c] == DR.CELL_LOSES]
    assert len(loses) == 218 and 108 in loses and all(r["length"][c] == 2 for c in loses)
    assert [(c, r["nodes"][c]) for c in range(225) if r["nodes"][c]] == [(108, 2), (109, 2), (113, 2)]


# ---------------- rows and corners ----------------
def threatened_by_three(cells_, colour):
    """an open-ended three of `colour` on the given cells with the OTHER colour to move; everything else is scattered fillers"""
    if colour == 1:
        return interleave(list(cells_) + [FAR[3]], FAR[:3])
    return interleave(FAR[:4], list(cells_) + [FAR[4]])


@pytest.mark.parametrize("colour", [1, 2])
def test_threats_along_the_borders_and_into_the_corners(gmk, colour):
    lists = [threatened_by_three(c, colour) for c in BORDER_LINES.values()]
    want = [wanted(q, 4, 100) for q in lists]
    assert all(r["status"] == R.WIN and r["threat_length"] == 2 and DR.CELL_HOLDS in r["verdict"] for r in want), [r["status"] for r in want]
    assert defend(lists, 4, 100) == want
    assert defend(lists, 4, 100, iterative=True) == [wanted(q, 4, 100, True) for q in lists]


@pytest.mark.parametrize("colour", [1, 2])
def test_rows_do_not_wrap(gmk, colour):
    """(13,3), (14,3), (0,4), (1,4): four consecutive cell ids and no line; nor (12,3) .. (14,3), (0,4)"""
    traps = [[cell(13, 3), cell(14, 3), cell(0, 4), cell(1, 4)], [cell(12, 3), cell(13, 3), cell(14, 3), cell(0, 4)]]
    scattered = [cell(7, 7), cell(3, 9), cell(11, 6), cell(6, 11), cell(9, 12), cell(2, 12)]
    lists = [interleave(t + [scattered[4]], scattered[:4]) if colour == 1 else interleave(scattered[:5], t + [scattered[5]]) for t in traps]
    got = defend(lists, 8, 1000)
    assert got[0]["status"] == R.NONE and sum(got[0]["nodes"]) == 0 and set(got[0]["verdict"]) == {DR.CELL_NONE, DR.CELL_HOLDS}
    assert got == [wanted(q, 8, 1000) for q in lists]


def test_bad_lists_do_not_disturb_their_neighbours(gmk):
    good = selection()[40:44]
    moves, lens = pack([good[0], [1, 2, 3], good[1], [4, 5], [7, 225, 9], [30, 31, 30], good[2], good[3]], stride=225)
    lens[1], lens[3] = -1, 226
    out = G.vcf_defend(moves, lens, *RUNS["medium"][:2])
    got = [row_of(out, i) for i in range(8)]
    bad = {"status": R.BAD, "threat_length": 0, "threat_nodes": 0, "pv": [], "verdict": [0] * 225, "length": [0] * 225, "nodes": [0] * 225}
    assert [got[i] for i in (1, 3, 4, 5)] == [bad] * 4
    assert [got[i] for i in (0, 2, 6, 7)] == reference("medium")[40:44]
    # a length above the stride cannot be a list of this buffer: refused the same way, nothing outside the row is read
    moves, lens = pack([good[0], [1, 2, 3]], stride=len(good[0]))
    lens[1] = len(good[0]) + 1
    out = G.vcf_defend(moves, lens, *RUNS["medium"][:2])
    assert [row_of(out, 0), row_of(out, 1)] == [reference("medium")[40], bad]


# ---------------- the device form ----------------
OPTIONAL = ("threat_nodes", "length", "nodes")


def test_null_outputs_and_device_form_on_a_side_stream(gmk):
    """The device form on a stream of its own with every output and with every combination of the optional ones missing, and the host form: the
    same numbers, and what was not asked for is not touched."""
    import torch
    pool = selection()[7:72]
    moves, lens = pack(pool)
    n = len(pool)
    max_depth, budget, _ = RUNS["medium"]
    d_moves, d_lens = torch.from_numpy(moves).cuda(), torch.from_numpy(lens).cuda()
    side = torch.cuda.Stream()
    host = G.vcf_defend(moves, lens, max_depth, budget)
    assert [row_of(host, i) for i in range(n)] == reference("medium")[7:72]

    def run(which):
        bufs = {"threat_status": torch.full((n,), -7, dtype=torch.int32, device="cuda"), "threat_length": torch.full((n,), -7, dtype=torch.int32, device="cuda"),
                "threat_nodes": torch.full((n,), -7, dtype=torch.int32, device="cuda"), "threat_pv": torch.full((n, 64), 7, dtype=torch.uint8, device="cuda"),
                "verdict": torch.full((n, 225), 7, dtype=torch.uint8, device="cuda"), "length": torch.full((n, 225), 7, dtype=torch.uint8, device="cuda"),
                "nodes": torch.full((n, 225), -7, dtype=torch.int32, device="cuda")}
        torch.cuda.synchronize()
        ptr = {k: (v.data_ptr() if k not in OPTIONAL or k in which else None) for k, v in bufs.items()}
        G.vcf_defend_device(d_moves.data_ptr(), moves.shape[1], d_lens.data_ptr(), n, max_depth, budget, d_threat_status=ptr["threat_status"],
                            d_threat_length=ptr["threat_length"], d_threat_pv=ptr["threat_pv"], d_threat_nodes=ptr["threat_nodes"],
                            d_verdict=ptr["verdict"], d_cell_length=ptr["length"], d_cell_nodes=ptr["nodes"], stream=side.cuda_stream)
        side.synchronize()
        return {k: v.cpu().numpy() for k, v in bufs.items()}

    for mask in range(8):
        which = tuple(k for b, k in enumerate(OPTIONAL) if mask >> b & 1)
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
    # status at o, length at o + 64, pv at o + 1024 (256 B), nodes at o + 128, verdict at o + 2048 (900 B), cell length at o + 3072, cell nodes at o + 4096 (3600 B)
    ARG = -3

    def call(moves_=m, stride=s, lens_=l, n=4, max_depth=8, budget=100, flags=0, status=o, length=o + 64, pv=o + 1024, nodes=None, verdict=o + 2048,
             cell_length=None, cell_nodes=None):
        return L.gmk_vcf_defend(moves_, stride, lens_, n, max_depth, budget, flags, status, length, pv, nodes, verdict, cell_length, cell_nodes, None)

    assert call() == 0
    assert call(nodes=o + 128, cell_length=o + 3072, cell_nodes=o + 4096) == 0
    assert call(n=0) == 0 and call(n=0, moves_=None, lens_=None, status=None, length=None, pv=None, verdict=None) == 0
    assert call(moves_=None) == ARG and call(lens_=None) == ARG
    for name in ("status", "length", "pv", "verdict"):
        assert call(**{name: None}) == ARG, name
    assert call(n=-1) == ARG
    assert call(stride=0) == ARG and call(stride=-5) == ARG
    assert call(max_depth=0) == ARG and call(max_depth=33) == ARG and call(max_depth=-1) == ARG
    assert call(max_depth=1) == 0 and call(max_depth=32) == 0
    assert call(flags=1) == ARG and call(flags=3) == ARG and call(flags=4) == ARG and call(flags=-1) == ARG and call(flags=2) == 0
    assert call(lens_=l + 2) == ARG
    assert call(status=o + 2) == ARG and call(length=o + 66) == ARG and call(nodes=o + 130) == ARG and call(cell_nodes=o + 4098) == ARG
    assert call(pv=o + 1025, verdict=o + 2049, cell_length=o + 3073, moves_=m + 1, stride=s - 1) == 0       # the byte arrays need no alignment
    torch.cuda.synchronize()
    assert b"gmk_vcf_defend" in L.gmk_last_error()
    h_moves, h_lens = moves.ctypes.data, lens.ctypes.data
    status, length, pv, verdict = np.zeros(4, np.int32), np.zeros(4, np.int32), np.zeros((4, 64), np.uint8), np.zeros((4, 225), np.uint8)
    S, Ln, P, V = status.ctypes.data, length.ctypes.data, pv.ctypes.data, verdict.ctypes.data

    def host(moves_=h_moves, stride=s, lens_=h_lens, n=4, max_depth=8, flags=0, status_=S, length_=Ln, pv_=P, verdict_=V):
        return L.gmk_vcf_defend_host(moves_, stride, lens_, n, max_depth, 100, flags, status_, length_, pv_, None, verdict_, None, None)

    assert host(moves_=None) == ARG and host(lens_=None) == ARG and host(stride=0) == ARG and host(n=-1) == ARG and host(max_depth=33) == ARG
    assert host(flags=1) == ARG and host(flags=8) == ARG
    assert host(status_=None) == ARG and host(length_=None) == ARG and host(pv_=None) == ARG and host(verdict_=None) == ARG
    assert host(n=0) == 0 and host() == 0 and host(flags=2) == 0
    assert [int(v) for v in status] == [r["status"] for r in (wanted(q, 8, 100, True) for q in selection()[:4])]


# ---------------- the agent ----------------
class Stub:
    """an inner agent that always answers one cell"""

    def __init__(self, answer):
        self.answer, self.asked = answer, 0

    def name(self):
        return "Stub"

    def sync_with_board(self, board):
        pass

    def reset(self):
        pass

    def get_action(self, board):
        from gomokuai_amd import core
        self.asked += 1
        return core.Position(self.answer)

    def debug_message(self):
        return {"stub": self.answer}


def board_after(moves):
    from gomokuai_amd import core
    board = core.Board()
    for c in moves:
        board.apply_move(core.Position(int(c)), False)
    return board


def test_agent_overrules_a_losing_move(gmk):
    from gomokuai_amd import interface
    board = board_after(OPEN_THREE)
    stub = Stub(108)                                              # the far end of the three: loses in 2
    agent = interface.VCFAgent(stub, depth=8, budget=1000, defend=True)
    agent.sync_with_board(board)
    played = int(agent.get_action(board).id)
    assert played in (109, 113) and stub.asked == 1               # the inner agent was still asked
    moves, lens = pack([OPEN_THREE])
    probs = G.pattern_policy(moves, lens, filter=False)["probs"][0]
    assert played == (109 if probs[109] >= probs[113] else 113)   # the higher pattern probability, the lowest cell on a tie
    message = agent.debug_message()
    assert message["vcf_defence"] == {"holds": [109, 113], "unknown": 0, "loses": 218, "searched": 3, "overruled": True}
    assert message["vcf"]["status"] == "NONE" and message["vcf_opponent"]["status"] == "WIN" and message["vcf_opponent"]["pv"] == [109, 108, 113]
    assert message["vcf_opponent"]["move"] == 109 and message["stub"] == 108


def test_agent_keeps_a_move_that_holds(gmk):
    from gomokuai_amd import interface
    board = board_after(OPEN_THREE)
    for answer in (113, 109):
        agent = interface.VCFAgent(Stub(answer), depth=8, budget=1000, defend=True)
        agent.sync_with_board(board)
        assert int(agent.get_action(board).id) == answer
        assert agent.debug_message()["vcf_defence"] == {"holds": [109, 113], "unknown": 0, "loses": 218, "searched": 3, "overruled": False}
    # no threat: no defence, nothing in the message
    quiet = board_after([cell(7, 7), cell(8, 8), cell(6, 8)])
    agent = interface.VCFAgent(Stub(0), depth=8, budget=1000, defend=True)
    agent.sync_with_board(quiet)
    assert int(agent.get_action(quiet).id) == 0 and "vcf_defence" not in agent.debug_message()


def test_agent_without_defend_plays_the_losing_move(gmk):
    from gomokuai_amd import interface
    board = board_after(OPEN_THREE)
    agent = interface.VCFAgent(Stub(108), depth=8, budget=1000)
    agent.sync_with_board(board)
    assert int(agent.get_action(board).id) == 108
    message = agent.debug_message()
    assert "vcf_defence" not in message and message["vcf_opponent"]["status"] == "WIN" and message["vcf_opponent"]["pv"] == [109, 108, 113]
    wrapped = interface.make_agent("pattern", vcf=8, vcf_defend=True)
    assert type(wrapped) is interface.VCFAgent and wrapped.defend and wrapped.depth == 8
    wrapped.sync_with_board(board)
    assert int(wrapped.get_action(board).id) in (109, 113)
