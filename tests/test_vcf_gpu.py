"""K14 on the device: the forced-win solver by continuous fours (gmk_vcf_solve) against the plain-Python restatement of its contract
(tests/vcf_reference.py).  Integer work on both sides: every comparison is exact, over status, move, length, nodes and the whole pv."""
import functools
import random

import numpy as np
import pytest

import vcf_reference as R
from gomokuai_amd import lib as G

pytestmark = pytest.mark.gpu

SEED = 1
SHAPES = ((10, 2), (16, 3), (24, 3), (30, 4), (40, 4), (60, 5))      # (plies, half-width of the square around the centre), 60 positions each
# (max_depth, budget, opponent, iterative)
RUNS = {"deep": (12, 5000, False, False), "deep_iterative": (12, 5000, False, True), "shallow": (3, 8, False, False), "shallow_opponent": (3, 8, True, False)}
FIELDS = ("status", "move", "length", "nodes")


@pytest.fixture(scope="module")
def gmk():
    G.init()
    return G


def cell(x, y):
    return y * 15 + x


def interleave(black, white):
    assert len(black) - len(white) in (0, 1)
    moves = []
    for i, b in enumerate(black):
        moves.append(b)
        if i < len(white):
            moves.append(white[i])
    return moves


def pack(lists, stride=None, fill=0):
    stride = stride or max(1, max(len(q) for q in lists))
    moves = np.full((len(lists), stride), fill, np.uint8)
    for i, q in enumerate(lists):
        moves[i, :len(q)] = q
    return moves, np.array([len(q) for q in lists], np.int32)


def row_of(out, i):
    """position i of a result as the restatement writes it"""
    length = int(out["length"][i])
    pv = out["pv"][i]
    cells = 2 * length - 1 if length else 0
    assert (pv[cells:] == 255).all(), "pv cells past the end are 255"
    return {"status": int(out["status"][i]), "move": int(out["move"][i]), "length": length, "nodes": int(out["nodes"][i]), "pv": [int(c) for c in pv[:cells]]}


def solve(lists, max_depth, budget, opponent=False, iterative=False, stride=None, fill=0):
    moves, lens = pack(lists, stride, fill)
    out = G.vcf_solve(moves, lens, max_depth, budget, opponent=opponent, iterative=iterative)
    return [row_of(out, i) for i in range(len(lists))]


@functools.lru_cache(maxsize=None)
def positions():
    rng = random.Random(SEED)
    out = []
    for plies, spread in SHAPES:
        kept = 0
        while kept < 60:
            q = R.random_position(rng, plies, spread)
            if q is not None:
                out.append(q)
                kept += 1
    return out


@functools.lru_cache(maxsize=None)
def reference(run):
    max_depth, budget, opponent, iterative = RUNS[run]
    return [R.solve(q, max_depth, budget, opponent=opponent, iterative=iterative) for q in positions()]


# ---------------- random sets against the restatement ----------------
def test_the_random_sets_cover_the_contract():
    """On the restatement alone: every status a search can end in occurs at least ten times over the runs, and wins of 2 .. 8 and more moves."""
    count = {s: 0 for s in (R.WIN, R.NONE, R.DEPTH, R.BUDGET)}
    lengths = set()
    for run in RUNS:
        for q, r in zip(positions(), reference(run)):
            count[r["status"]] += 1
            if r["status"] == R.WIN:
                lengths.add(r["length"])
                R.check_pv(q, r, RUNS[run][2])
    assert all(v >= 10 for v in count.values()), count
    assert set(range(2, 9)) <= lengths, sorted(lengths)


@pytest.mark.parametrize("run", list(RUNS))
def test_random_positions_match_the_restatement(gmk, run):
    max_depth, budget, opponent, iterative = RUNS[run]
    got = solve(positions(), max_depth, budget, opponent, iterative)
    want = reference(run)
    wrong = [i for i in range(len(want)) if got[i] != want[i]]
    assert not wrong, (len(wrong), wrong[:5], got[wrong[0]], want[wrong[0]])


def test_unfiltered_openings_match_the_restatement(gmk):
    """The sets above hold no position with a completing cell; whole random-opening lists do: wins in one, defender fours at the root,
    finished games."""
    moves, lens, _ = G.synth_boards(96, 0, first_board=0)
    lists = [[int(c) for c in moves[i, :lens[i]]] for i in range(96)]
    seen = set()
    for kw in ({}, {"opponent": True}, {"iterative": True}):
        want = [R.solve(q, 8, 2000, **kw) for q in lists]
        assert solve(lists, 8, 2000, **kw) == want, kw
        seen |= {(r["status"], r["length"]) for r in want}
    assert {(R.WIN, 1), (R.OVER, 0), (R.NONE, 0)} <= seen


# ---------------- batch seams ----------------
@functools.lru_cache(maxsize=None)
def alone():
    """the first 257 positions, each solved in a launch of its own"""
    return [solve([q], 12, 5000)[0] for q in positions()[:257]]


@pytest.mark.parametrize("n", [1, 3, 4, 5, 63, 64, 65, 257])
def test_a_batch_is_its_positions_alone(gmk, n):
    # the tail of the set first: the heavy positions are there
    pool = positions()[:257]
    index = list(range(256, 256 - n, -1))
    got = solve([pool[i] for i in index], 12, 5000)
    assert got == [alone()[i] for i in index]
    assert alone()[:257] == reference("deep")[:257]


def test_order_in_the_batch_does_not_matter(gmk):
    pool = positions()[:257]
    index = list(range(257))
    random.Random(3).shuffle(index)
    assert solve([pool[i] for i in index], 12, 5000) == [alone()[i] for i in index]


def test_a_heavy_position_among_trivial_ones(gmk):
    want = reference("deep")
    heavy = max(range(len(want)), key=lambda i: want[i]["nodes"])
    assert want[heavy]["nodes"] >= 1000
    trivial = [[], [112], positions()[0], [112, 113]]
    small = [R.solve(q, 12, 5000) for q in trivial]
    order = [0, 1, 2] * 7 + [None] + [0, 3] * 20                  # the heavy one is the 22nd of 62
    got = solve([positions()[heavy] if k is None else trivial[k] for k in order], 12, 5000)
    assert got == [want[heavy] if k is None else small[k] for k in order]


def test_a_large_batch(gmk):
    """Above 32 positions per compute unit a wavefront's slice is sixteen positions, not four: the set thirty times over, heavy ones included."""
    times = 30
    assert len(positions()) * times > 32 * G.device_info()["cu_count"]
    assert solve(positions() * times, 12, 5000) == reference("deep") * times


def test_stride_beyond_the_longest_list(gmk):
    pool = positions()[100:140]
    assert solve(pool, 12, 5000, stride=97, fill=0xEE) == reference("deep")[100:140]


def test_null_outputs_and_device_form(gmk):
    """The device form with every output, with some outputs missing, and the host form: the same numbers."""
    import torch
    pool = positions()[180:245]
    moves, lens = pack(pool)
    n = len(pool)
    d_moves, d_lens = torch.from_numpy(moves).cuda(), torch.from_numpy(lens).cuda()
    stream = torch.cuda.current_stream().cuda_stream

    def run(which):
        bufs = {"status": torch.full((n,), -7, dtype=torch.int32, device="cuda"), "move": torch.full((n,), -7, dtype=torch.int32, device="cuda"),
                "length": torch.full((n,), -7, dtype=torch.int32, device="cuda"), "nodes": torch.full((n,), -7, dtype=torch.int32, device="cuda"),
                "pv": torch.full((n, 64), 7, dtype=torch.uint8, device="cuda")}
        ptr = {k: (v.data_ptr() if k in which else None) for k, v in bufs.items()}
        G.vcf_solve_device(d_moves.data_ptr(), moves.shape[1], d_lens.data_ptr(), n, 12, 5000, d_status=ptr["status"], d_move=ptr["move"],
                           d_length=ptr["length"], d_nodes=ptr["nodes"], d_pv=ptr["pv"], stream=stream)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in bufs.items()}

    host = G.vcf_solve(moves, lens, 12, 5000)
    everything = run(FIELDS + ("pv",))
    for k in FIELDS + ("pv",):
        assert (everything[k].astype(np.int64) == host[k].astype(np.int64)).all(), k
    assert [row_of(host, i) for i in range(n)] == reference("deep")[180:245]
    for which in (("status", "pv"), ("nodes",), ("move", "length"), ()):
        part = run(which)
        for k in FIELDS + ("pv",):
            if k in which:
                assert (part[k].astype(np.int64) == host[k].astype(np.int64)).all(), (which, k)
            else:
                assert (part[k] == (7 if k == "pv" else -7)).all(), (which, k)      # untouched


# ---------------- edges ----------------
FAR = [cell(7, 7), cell(3, 8), cell(11, 6), cell(6, 11), cell(9, 3), cell(5, 5)]      # scattered fillers in the middle, off every line used below


def three(cells_, colour):
    """an open-ended three of `colour` on the given cells, that colour to move; the other colour's stones are scattered fillers"""
    if colour == 1:
        return interleave(list(cells_), FAR[:3])
    return interleave(FAR[:4], list(cells_))


BORDER_LINES = {
    "top": [cell(x, 0) for x in (5, 6, 7)], "bottom": [cell(x, 14) for x in (9, 10, 11)],
    "left": [cell(0, y) for y in (5, 6, 7)], "right": [cell(14, y) for y in (1, 2, 3)],
    "top_touching_left": [cell(x, 0) for x in (1, 2, 3)], "bottom_touching_right": [cell(x, 14) for x in (11, 12, 13)],
    "diagonal_top_left": [cell(i, i) for i in (1, 2, 3)], "diagonal_bottom_right": [cell(i, i) for i in (11, 12, 13)],
    "diagonal_top_right": [cell(14 - i, i) for i in (1, 2, 3)], "diagonal_bottom_left": [cell(i, 14 - i) for i in (1, 2, 3)],
}


@pytest.mark.parametrize("colour", [1, 2])
def test_wins_along_the_borders_and_into_the_corners(gmk, colour):
    lists = [three(c, colour) for c in BORDER_LINES.values()]
    want = [R.solve(q, 8, 1000) for q in lists]
    assert all(r["status"] == R.WIN and r["length"] == 2 for r in want), [r["status"] for r in want]
    assert solve(lists, 8, 1000) == want
    assert solve(lists, 8, 1000, opponent=True) == [R.solve(q, 8, 1000, opponent=True) for q in lists]
    assert solve(lists, 8, 1000, iterative=True) == [R.solve(q, 8, 1000, iterative=True) for q in lists]


@pytest.mark.parametrize("colour", [1, 2])
def test_rows_do_not_wrap(gmk, colour):
    """(13,3), (14,3), (0,4), (1,4): four consecutive cell ids and no line; nor (12,3) .. (14,3), (0,4)"""
    traps = [[cell(13, 3), cell(14, 3), cell(0, 4), cell(1, 4)], [cell(12, 3), cell(13, 3), cell(14, 3), cell(0, 4)]]
    scattered = [cell(7, 7), cell(3, 9), cell(11, 6), cell(6, 11), cell(9, 12)]
    lists = [interleave(t, scattered[:4]) if colour == 1 else interleave(scattered, t) for t in traps]
    got = solve(lists, 8, 1000)
    assert [(r["status"], r["nodes"]) for r in got[:1]] == [(R.NONE, 0)]
    assert got == [R.solve(q, 8, 1000) for q in lists]


def full_board():
    black = [cell(x, y) for y in range(15) for x in range(15) if (x + 2 * y) % 4 < 2]      # 113 cells, runs of two at most (tests/test_vcf_reference.py)
    return interleave(black, [c for c in range(225) if c not in black])


def test_full_and_empty_board_and_over(gmk):
    six = interleave([cell(x, 7) for x in (2, 3, 4, 6, 7, 5)], [cell(0, 14), cell(4, 13), cell(9, 14), cell(14, 12), cell(14, 9)])
    white_five = interleave([cell(0, 14), cell(4, 13), cell(9, 14), cell(14, 12), cell(14, 9)], [cell(i, 14 - i) for i in range(3, 8)])
    lists = [full_board(), [], six, white_five, full_board()[:224]]
    for kw in ({}, {"opponent": True}, {"iterative": True}):
        got = solve(lists, 8, 1000, **kw)
        assert got == [R.solve(q, 8, 1000, **kw) for q in lists], kw
        assert [(r["status"], r["nodes"]) for r in got[:4]] == [(R.NONE, 0), (R.NONE, 0), (R.OVER, 0), (R.OVER, 0)]


def test_bad_lists_do_not_disturb_their_neighbours(gmk):
    good = positions()[200:204]
    moves, lens = pack([good[0], [1, 2, 3], good[1], [4, 5], [7, 225, 9], [30, 31, 30], good[2], good[3]], stride=225)
    lens[1], lens[3] = -1, 226
    out = G.vcf_solve(moves, lens, 12, 5000)
    got = [row_of(out, i) for i in range(8)]
    bad = {"status": R.BAD, "move": -1, "length": 0, "nodes": 0, "pv": []}
    assert [got[i] for i in (1, 3, 4, 5)] == [bad] * 4
    assert [got[i] for i in (0, 2, 6, 7)] == reference("deep")[200:204]
    # a length above the stride cannot be a list of this buffer: refused the same way, nothing outside the row is read
    moves, lens = pack([good[0], [1, 2, 3]], stride=len(good[0]))
    lens[1] = len(good[0]) + 1
    out = G.vcf_solve(moves, lens, 12, 5000)
    assert [row_of(out, 0), row_of(out, 1)] == [reference("deep")[200], bad]


def test_the_longest_win_at_depth_32(gmk):
    """The generator yields no win of 32 moves (a pv of 63 cells): over its 360 positions the longest at max_depth 32 has 18 moves, 35 cells
    (position 350 of seed 1).  That one is used, with the limit at 32, at exactly its length and one below."""
    q = positions()[350]
    want = R.solve(q, 32, 5000)
    assert want["status"] == R.WIN and want["length"] == 18 and len(want["pv"]) == 35
    assert solve([q], 32, 5000)[0] == want
    for limit in (18, 17):
        for iterative in (False, True):
            assert solve([q], limit, 5000, iterative=iterative)[0] == R.solve(q, limit, 5000, iterative=iterative), (limit, iterative)


def test_budget_edge(gmk):
    want = reference("deep")
    i = next(i for i, r in enumerate(want) if r["status"] == R.WIN and r["nodes"] >= 20)
    q, k = positions()[i], want[i]["nodes"]
    assert solve([q, q, q], 12, k)[0] == want[i]
    short = solve([q], 12, k - 1)[0]
    assert (short["status"], short["nodes"]) == (R.BUDGET, k - 1) and short == R.solve(q, 12, k - 1)
    assert solve([q], 12, 0)[0] == R.solve(q, 12, 0)


# ---------------- arguments ----------------
def test_arguments(gmk):
    import torch
    L = G.load()
    moves, lens = pack(positions()[:4])
    d_moves, d_lens = torch.from_numpy(moves).cuda(), torch.from_numpy(lens).cuda()
    out = torch.zeros(256, dtype=torch.int32, device="cuda")
    m, l, o, s = d_moves.data_ptr(), d_lens.data_ptr(), out.data_ptr(), moves.shape[1]
    ARG = -3

    def call(moves_=m, stride=s, lens_=l, n=4, max_depth=8, budget=100, flags=0, status=o, move=None, length=None, nodes=None, pv=None):
        return L.gmk_vcf_solve(moves_, stride, lens_, n, max_depth, budget, flags, status, move, length, nodes, pv, None)

    assert call() == 0
    assert call(n=0) == 0 and call(n=0, moves_=None, lens_=None) == 0
    assert call(moves_=None) == ARG and call(lens_=None) == ARG
    assert call(n=-1) == ARG
    assert call(stride=0) == ARG and call(stride=-5) == ARG
    assert call(max_depth=0) == ARG and call(max_depth=33) == ARG and call(max_depth=-1) == ARG
    assert call(max_depth=1) == 0 and call(max_depth=32) == 0
    assert call(flags=4) == ARG and call(flags=-1) == ARG and call(flags=3) == 0
    assert call(lens_=l + 2) == ARG
    for name in ("status", "move", "length", "nodes"):
        assert call(**{name: o + 2}) == ARG, name
    assert call(pv=o + 257, moves_=m + 1, stride=s - 1) == 0       # the byte arrays need no alignment
    torch.cuda.synchronize()
    assert b"gmk_vcf_solve" in L.gmk_last_error()
    h_moves, h_lens = moves.ctypes.data, lens.ctypes.data
    assert L.gmk_vcf_solve_host(None, s, h_lens, 4, 8, 100, 0, None, None, None, None, None) == ARG
    assert L.gmk_vcf_solve_host(h_moves, s, None, 4, 8, 100, 0, None, None, None, None, None) == ARG
    assert L.gmk_vcf_solve_host(h_moves, 0, h_lens, 4, 8, 100, 0, None, None, None, None, None) == ARG
    assert L.gmk_vcf_solve_host(h_moves, s, h_lens, -1, 8, 100, 0, None, None, None, None, None) == ARG
    assert L.gmk_vcf_solve_host(h_moves, s, h_lens, 4, 33, 100, 0, None, None, None, None, None) == ARG
    assert L.gmk_vcf_solve_host(h_moves, s, h_lens, 4, 8, 100, 8, None, None, None, None, None) == ARG
    assert L.gmk_vcf_solve_host(h_moves, s, h_lens, 0, 8, 100, 0, None, None, None, None, None) == 0
    assert L.gmk_vcf_solve_host(h_moves, s, h_lens, 4, 8, 100, 0, None, None, None, None, None) == 0


# ---------------- the agent ----------------
def board_after(moves):
    from gomokuai_amd import core
    board = core.Board()
    for c in moves:
        board.apply_move(core.Position(int(c)), False)
    return board


def test_agent_plays_the_forced_win(gmk):
    from gomokuai_amd import interface
    agent = interface.VCFAgent(interface.make_agent("pattern"))
    assert agent.name() == "VCF(PatternEvalAgent)"
    board = board_after(interleave([5, 6, 7], [cell(0, 14), cell(4, 13), cell(9, 14)]))
    agent.sync_with_board(board)
    assert int(agent.get_action(board).id) == 4
    message = agent.debug_message()
    assert message["vcf"]["status"] == "WIN" and message["vcf"]["length"] == 2 and message["vcf"]["nodes"] == 4 and message["vcf"]["pv"] == [4, 3, 8]
    assert message["vcf_opponent"]["status"] == "NONE" and message["vcf_opponent"]["length"] == 0


def test_agent_defers_on_a_quiet_position(gmk):
    from gomokuai_amd import interface
    quiet = [cell(7, 7), cell(8, 8), cell(6, 8)]
    inner, agent = interface.make_agent("pattern"), interface.make_agent("pattern", vcf=12)
    assert isinstance(agent, interface.VCFAgent) and agent.depth == 12
    board = board_after(quiet)
    inner.sync_with_board(board)
    agent.sync_with_board(board)
    assert int(agent.get_action(board).id) == int(inner.get_action(board).id)
    message = agent.debug_message()
    assert message["vcf"]["status"] == "NONE" and message["vcf_opponent"]["status"] == "NONE"
    assert message["before"] == inner.debug_message()["before"]      # the inner agent's message is still there


def test_make_agent_without_vcf_is_unchanged(gmk):
    from gomokuai_amd import interface
    kinds = {"random": interface.RandomAgent, "human": interface.HumanAgent, "pattern": interface.PatternEvalAgent, "traditional:5": interface.MCTSAgent,
             "random-mcts:5:5": interface.MCTSAgent, "poolrave": interface.MCTSAgent}
    for spec, cls in kinds.items():
        assert type(interface.make_agent(spec, iterations=8, quiet=True)) is cls, spec
        assert type(interface.make_agent(spec, iterations=8, quiet=True, vcf=0)) is cls, spec
    assert type(interface.make_agent("random", vcf=8)) is interface.RandomAgent
    assert type(interface.make_agent("human", vcf=8)) is interface.HumanAgent
    wrapped = interface.make_agent("traditional:5", iterations=8, quiet=True, vcf=8)
    assert type(wrapped) is interface.VCFAgent and type(wrapped.inner) is interface.MCTSAgent and wrapped.name().startswith("VCF(MCTSAgent:")
