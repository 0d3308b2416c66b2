"""K23 on the device: gmk_pattern_evaluate_states (pattern_states_kernel in pattern_kernel.hip) against K10 on the canonical lists of the
numpy restatement (tests/pattern_states_reference.py) and against the CPU oracle's heuristic replayed in that order, on BITS; the sum
normalisation against its numpy statement; rows alone and in a batch; K7, the self-play loops and the front end with PatternEvaluator."""
import functools

import numpy as np
import pytest

import pattern_states_reference as R
from gomokuai_amd import lib as G

pytestmark = pytest.mark.gpu

N, F32 = 225, np.float32
OVER, EVAL_ERROR, ILLEGAL = 1, 2, 4
pos = lambda x, y: y * 15 + x
BLACK_FIVE = [pos(3, 3), pos(3, 4), pos(4, 4), pos(3, 5), pos(5, 5), pos(3, 6), pos(6, 6), pos(3, 7), pos(7, 7)]


@pytest.fixture(scope="module")
def gmk():
    G.init()
    return G


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _tie_order():
    """a full board without a five (tests/test_pattern_gpu.py)"""
    order = []
    for j in range(15):
        y = 2 * j if j <= 7 else 2 * (j - 7) - 1
        order += [y * 15 + i for i in range(15)]
    return order


@functools.lru_cache(maxsize=None)
def _pool():
    """The rows every comparison draws from: the edge rows first, then random openings of 0 .. 60 plies with and without the last-move planes.
    -> (rows f32[n, 6, 225], the canonical lists: moves, lens, status)"""
    rng = np.random.RandomState(23)
    order = _tie_order()
    rows = [R.planes([]),                                         # an empty board: the centre one-hot
            R.planes(BLACK_FIVE),                                 # a five on the board, completed by the last ply: OVER
            R.planes(BLACK_FIVE + [0]),                           # ... completed before the last ply of the canonical list: ILLEGAL, as K10 says
            R.planes(order),                                      # a full board
            R.planes(order[:224]),                                # one empty cell
            R.planes([224]), R.planes([112, 224]), R.planes([224, 0, 63, 64, 191, 192], last=False, last2=False),
            R.planes(BLACK_FIVE[:8]),                             # one move before the five
            np.zeros((6, N), F32)]                                # the row of a finished K7 leaf
    for kind in (0, 1):
        m, l, _ = G.synth_boards(24, kind, first_board=2300 + 1000 * kind)
        for g in range(24):
            cut = min(int(l[g]), int(rng.randint(0, 61)))
            ml = [int(c) for c in m[g, :cut]]
            rows.append(R.planes(ml, last=g % 3 != 2, last2=g % 3 == 0))
    rows = np.stack(rows)
    moves, lens, status = R.lists(rows)
    assert lens.max() == 225 and (status != 0).sum() == 1
    return rows, moves, lens, status


@functools.lru_cache(maxsize=None)
def _k10(filt):
    """K10 on the canonical lists of the pool; a row that is no position: ILLEGAL and zeros"""
    rows, moves, lens, status = _pool()
    out = G.pattern_policy(moves, lens, filter=filt)
    bad = status != 0
    out["status"][bad] = ILLEGAL
    out["probs"][bad], out["value"][bad] = 0, 0
    return out


def _device(rows, filt, norm, with_status=True, pad=3):
    """gmk_pattern_evaluate_states on device tensors that are `pad` rows longer than the batch and start from a sentinel"""
    import torch
    rows = np.ascontiguousarray(rows, F32).reshape(-1, 6, 15, 15)
    n = len(rows)
    d_rows = torch.from_numpy(rows).cuda()
    before = d_rows.clone()
    value = torch.full((n + pad,), -7.0, dtype=torch.float32, device="cuda")
    probs = torch.full((n + pad, N), -7.0, dtype=torch.float32, device="cuda")
    status = torch.full((n + pad,), -7, dtype=torch.int32, device="cuda")
    G.pattern_evaluate_states(d_rows, filt, norm, value=value, probs=probs, status=status if with_status else False)
    torch.cuda.synchronize()
    assert torch.equal(d_rows.view(torch.int32), before.view(torch.int32))               # the states are not written
    v, p, s = value.cpu().numpy(), probs.cpu().numpy(), status.cpu().numpy()
    assert (v[n:] == -7).all() and (p[n:] == -7).all() and (s[n:] == -7).all()           # nothing past row n
    if not with_status:
        assert (s == -7).all()
    return {"value": v[:n], "probs": p[:n], "status": s[:n]}


def _same(got, want, rows=slice(None)):
    assert (got["status"] == want["status"][rows]).all(), (got["status"], want["status"][rows])
    bad = np.nonzero((_bits(got["probs"]) != _bits(want["probs"][rows])).any(axis=1))[0]
    assert len(bad) == 0, "probs differ on rows %s" % bad
    assert (_bits(got["value"]) == _bits(want["value"][rows])).all()


# ---------------- against K10 and the oracle, bit for bit ----------------
@pytest.mark.parametrize("filt", [1, 0])
def test_whole_pool_matches_k10_on_the_canonical_lists(gmk, filt):
    rows, moves, lens, status = _pool()
    want = _k10(filt)
    _same(_device(rows, filt, "l2"), want)
    centre = np.zeros(N, F32)
    centre[112] = 1.0
    assert want["status"][0] == 0 and (_bits(want["probs"][0]) == _bits(centre)).all()   # the edge rows are what they are meant to be
    assert want["status"][1] == OVER and want["status"][2] & ILLEGAL and want["status"][3] == OVER and want["status"][4] == 0
    assert list(want["status"][5:9]) == [0, 0, 0, 0] and want["status"][9] == ILLEGAL
    assert (want["status"][10:] == 0).sum() >= 40


@pytest.mark.parametrize("filt", [1, 0])
@pytest.mark.parametrize("n", [1, 9, 10, 19])
def test_batches_around_a_workgroup(gmk, n, filt):
    rows = _pool()[0]
    for first in (0, 7, 30):
        _same(_device(rows[first:first + n], filt, "l2"), _k10(filt), slice(first, first + n))


@pytest.mark.parametrize("filt", [1, 0])
def test_matches_the_oracle_replayed_in_canonical_order(gmk, oracle, filt):
    import trad_rave_reference as T
    rows, moves, lens, status = _pool()
    got = _device(rows, filt, "l2")
    checked = 0
    for g in range(len(rows)):
        if status[g]:                                             # no position
            continue
        ml = moves[g, :lens[g]]
        ev, bad, after_the_end = oracle.Evaluator(), 0, False
        for m in ml:
            if ev.check_end():                                    # the canonical order completes a five before its last ply: K10's bit 2
                after_the_end = True
                break
            bad |= ev.apply(int(m))[1]
        assert not bad
        if after_the_end:
            assert got["status"][g] & ILLEGAL and not got["probs"][g].any() and _bits(got["value"][g]) == 0
            assert g != 1
            continue
        if ev.check_end():
            assert got["status"][g] == OVER and not got["probs"][g].any() and _bits(got["value"][g]) == 0
            continue
        cur = int(ev.board.cur_player)
        scores, density = ev.scores(), ev.density()
        probs = T.evaluation_probs(scores, density, int(ev.board.nrec), cur)
        if filt:
            probs = T.decisive_filter(ev.pattern_dist(), ev.compound_dist(), cur, probs)
            c_probs, c_value = oracle.trad_heuristic(ml)           # the C oracle says the same
            assert (_bits(c_probs) == _bits(probs)).all()
        value = F32(T.evaluation_value(scores, density, cur))
        assert got["status"][g] == 0, g
        assert (_bits(got["probs"][g]) == _bits(probs)).all(), g
        assert _bits(got["value"][g]) == _bits(value), g
        checked += 1
    assert checked >= 40 and got["status"][2] & ILLEGAL


# ---------------- norm SUM ----------------
@pytest.mark.parametrize("filt", [1, 0])
def test_sum_normalisation(gmk, filt):
    rows, moves, lens, status = _pool()
    k10 = _k10(filt)
    got = _device(rows, filt, "sum")
    want = np.stack([R.finish(k10["probs"][g], rows[g], R.NORM_SUM, live=k10["status"][g] == 0) for g in range(len(rows))])
    assert (got["status"] == k10["status"]).all()
    assert (_bits(got["probs"]) == _bits(want)).all()
    assert (_bits(got["value"]) == _bits(k10["value"])).all()
    live = k10["status"] == 0
    sums = got["probs"][live].astype(np.float64).sum(axis=1)
    assert (np.abs(sums - 1.0) <= 225 * 2.0 ** -24).all()         # 225 roundings to float of terms below 1
    assert ((got["probs"][live] == 0) == (k10["probs"][live] == 0)).all()
    assert not got["probs"][~live].any()
    # the host form is the same call
    host = G.pattern_evaluate_states_host(rows, filt, "sum")
    for k in ("value", "probs", "status"):
        assert host[k].tobytes() == got[k].tobytes(), k


# ---------------- isolation and bounds ----------------
def test_rows_alone_and_among_poisoned_rows(gmk):
    rows = _pool()[0]
    batch = np.full((19, 6, N), np.nan, F32)
    live = [int(g) for g in np.flatnonzero((_k10(1)["status"] == 0) & (_pool()[2] >= 8))]
    picks = {0: live[0], 8: live[1], 9: live[7], 18: live[-1]}   # a wavefront's first row, a workgroup's last, the next one's first, the third's first
    for at, src in picks.items():
        batch[at] = rows[src]
    for norm in ("l2", "sum"):
        got = _device(batch, 1, norm)
        for at, src in picks.items():
            alone = _device(rows[src:src + 1], 1, norm)
            assert alone["status"][0] == 0
            for k in ("value", "probs", "status"):
                assert got[k][at].tobytes() == alone[k][0].tobytes(), (norm, at, k)
        others = [i for i in range(19) if i not in picks]
        assert (got["status"][others] == ILLEGAL).all()
        assert (_bits(got["probs"][others]) == 0).all() and (_bits(got["value"][others]) == 0).all()


def test_null_status_and_empty_batch(gmk):
    import torch
    rows = _pool()[0]
    got = _device(rows[:11], 1, "sum", with_status=False)
    want = _device(rows[:11], 1, "sum")
    assert got["probs"].tobytes() == want["probs"].tobytes() and got["value"].tobytes() == want["value"].tobytes()
    L = G.load()
    stream = torch.cuda.current_stream().cuda_stream
    assert L.gmk_pattern_evaluate_states(None, 0, 1, 1, None, None, None, stream) == 0
    value = torch.full((2,), -7.0, device="cuda")
    probs = torch.full((2, N), -7.0, device="cuda")
    d_rows = torch.from_numpy(np.ascontiguousarray(rows[:2])).cuda()
    assert L.gmk_pattern_evaluate_states(d_rows.data_ptr(), 0, 1, 1, value.data_ptr(), probs.data_ptr(), None, stream) == 0
    torch.cuda.synchronize()
    assert (value == -7).all() and (probs == -7).all()
    assert L.gmk_pattern_evaluate_states_host(None, 0, 1, 1, None, None, None) == 0
    assert L.gmk_pattern_evaluate_states(d_rows.data_ptr(), 2, 1, 7, value.data_ptr(), probs.data_ptr(), None, stream) == -3      # GMK_ERR_ARG
    assert L.gmk_pattern_evaluate_states(d_rows.data_ptr(), 2, 3, 1, value.data_ptr(), probs.data_ptr(), None, stream) == -3
    torch.cuda.synchronize()
    assert (value == -7).all() and (probs == -7).all()


# ---------------- through K7 ----------------
class _ThroughTheHost:
    """network(states) the long way round: states -> host -> canonical lists (numpy) -> lib.pattern_policy -> the numpy finish -> tensors"""

    def __init__(self, filt=True, norm=R.NORM_SUM):
        self.filt, self.norm, self.zero_rows, self.calls = filt, norm, 0, 0

    def __call__(self, states):
        import torch
        rows = states.cpu().numpy().reshape(-1, 6, N)
        moves, lens, status = R.lists(rows)
        out = G.pattern_policy(moves, lens, filter=self.filt)
        live = (status == 0) & (out["status"] == 0)
        probs = np.stack([R.finish(out["probs"][g], rows[g], self.norm, live=bool(live[g])) for g in range(len(rows))])
        value = np.where(live, out["value"], F32(0)).astype(F32)
        self.zero_rows += int((~rows.any(axis=(1, 2))).sum())
        self.calls += 1
        return torch.from_numpy(value).cuda(), torch.from_numpy(probs).cuda()


def _openings(n):
    moves, lens, _ = G.synth_boards(n, 1, first_board=640)
    lens = np.array([min(int(lens[g]), 2 + 5 * g) for g in range(n)], np.int32)
    for g in range(n):
        moves[g, lens[g]:] = 0
    last = np.full((n, 2), -1, np.int16)
    for g in range(n):
        if lens[g] >= 1: last[g, 0] = moves[g, lens[g] - 1]
        if lens[g] >= 2: last[g, 1] = moves[g, lens[g] - 2]
    return moves, lens, last


def _search(network, playouts=24, graph=False, moves_lens_last=None, **options):
    moves, lens, last = moves_lens_last or _openings(4)
    tree = G.AlphaZeroMCTS(len(lens), node_capacity=1 << 14, **options)
    try:
        tree.set_roots(G.moves_to_planes(moves, lens), last)
        tree.search(network, playouts, graph=graph)
        import torch
        torch.cuda.synchronize()
        return tree.root_stats()
    finally:
        tree.close()


def _same_stats(a, b):
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("options", [{"leaves": 1}, {"leaves": 4}, {"leaves": 1, "vcf_depth": 8, "proof": True}], ids=["leaves1", "leaves4", "vcf8-proof"])
def test_k7_search_equals_the_search_through_the_host(gmk, options):
    from gomokuai_amd.network import PatternEvaluator
    got = _search(PatternEvaluator(), **options)
    want = _search(_ThroughTheHost(), **options)
    _same_stats(got, want)
    assert (got["root_visits"] >= 24).all() and not got["status"].any()


def test_k7_graph_search_equals_eager(gmk):
    from gomokuai_amd.network import PatternEvaluator
    ev = PatternEvaluator()
    _same_stats(_search(ev, graph=True), _search(ev))
    _same_stats(_search(ev, graph=True, leaves=4), _search(ev, leaves=4))


def test_k7_game_that_ends_inside_the_search(gmk):
    """Game 0 is one move from black's five: its leaves beyond that move are finished games, for which K7 writes zero rows; the evaluator
    calls them ILLEGAL, K7 ignores the row, and the other games' statistics are what they are without game 0 in the batch."""
    from gomokuai_amd.network import PatternEvaluator
    moves, lens, last = _openings(3)
    moves, lens, last = np.concatenate([np.zeros((1, moves.shape[1]), np.uint8), moves]), np.concatenate([[8], lens]).astype(np.int32), np.concatenate([[[-1, -1]], last]).astype(np.int16)
    moves[0, :8] = BLACK_FIVE[:8]
    last[0] = (BLACK_FIVE[7], BLACK_FIVE[6])
    slow = _ThroughTheHost()
    want = _search(slow, 32, moves_lens_last=(moves, lens, last))
    assert slow.zero_rows > 0                                     # the search did reach finished leaves
    got = _search(PatternEvaluator(), 32, moves_lens_last=(moves, lens, last))
    _same_stats(got, want)
    assert int(np.argmax(got["visits"][0])) in (pos(7, 7), pos(2, 2))           # either end of black's four
    alone = _search(PatternEvaluator(), 32, moves_lens_last=(moves[1:], lens[1:], last[1:]))
    for k in alone:
        assert alone[k].tobytes() == got[k][1:].tobytes(), k


# ---------------- the loops ----------------
def test_self_play_loops_play_the_same_games(gmk):
    from gomokuai_amd import selfplay
    from gomokuai_amd.network import PatternEvaluator
    ev = PatternEvaluator()
    a = selfplay.play_network_games(4, ev, 8, root_noise=None, max_moves=12, device_loop=True).cpu()
    b = selfplay.play_network_games(4, ev, 8, root_noise=None, max_moves=12, device_loop=False).cpu()
    for name in ("moves", "lens", "winner", "visits"):
        x, y = getattr(a, name), getattr(b, name)
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), name
    assert (np.asarray(a.lens) == 12).all() or (np.asarray(a.winner) != 0).any()
    assert np.asarray(a.visits).any()


def test_agent_match_takes_the_evaluator(gmk):
    from gomokuai_amd import selfplay
    from gomokuai_amd.network import PatternEvaluator
    records, first_is_black, scores = selfplay.play_agent_match(4, ("network", {"network": PatternEvaluator(), "playouts": 8}),
                                                                ("traditional_mcts", {"c_iterations": 8}), max_moves=16)
    records = records.cpu()
    assert len(records) == 4 and len(scores) == 4 and set(np.asarray(scores).tolist()) <= {0.0, 0.5, 1.0}
    assert (np.asarray(records.lens) > 4).all() and not records.overflow
    with pytest.raises(ValueError):
        selfplay.play_agent_match(4, ("network", {"network": PatternEvaluator(), "playouts": 8, "symmetry": "all"}), ("traditional_mcts", {"c_iterations": 8}))


# ---------------- the stream ----------------
def test_the_entry_reads_its_producers_rows():
    """tests/test_stream_contract_gpu.py's producer-decoy form: the buffer holds a valid decoy, the real rows arrive by a delayed copy on the
    side stream and the outputs are filled there behind the delay, so a launch on any other stream evaluates the decoy and is overwritten"""
    import torch
    from stream_harness import Call, Harness, Scenario
    G.init(0)
    H = Harness()
    rows = _pool()[0]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    real, decoy = dev(rows[10:27].reshape(17, 6, 15, 15)), dev(rows[27:44].reshape(17, 6, 15, 15))
    buf = real.clone()
    outs = (torch.zeros(17, device="cuda"), torch.zeros((17, N), device="cuda"), torch.zeros(17, dtype=torch.int32, device="cuda"))
    entry = lambda s: G.pattern_evaluate_states(buf, True, "sum", value=outs[0], probs=outs[1], status=outs[2], stream=s)

    def fill(byte):
        for o in outs:
            o.view(-1).view(torch.uint8).fill_(byte)

    def make():
        buf.copy_(decoy)
        torch.cuda.synchronize()
        entry(torch.cuda.current_stream().cuda_stream)            # f(decoy), eagerly: the counter ring exists from here on
        torch.cuda.synchronize()
        fill(0x11)
        calls = [Call(lambda s: buf.copy_(real, non_blocking=True)), Call(lambda s: fill(0x5A)), Call(entry)]
        return Scenario(calls, lambda: {"value": outs[0], "probs": outs[1], "status": outs[2], "states": buf})

    H.check("gmk_pattern_evaluate_states", make)
    torch.cuda.synchronize()
    want = _device(rows[10:27], 1, "sum")
    assert outs[1].cpu().numpy().tobytes() == want["probs"].tobytes() and outs[0].cpu().numpy().tobytes() == want["value"].tobytes()
    assert outs[2].cpu().numpy().tobytes() == want["status"].tobytes()


# ---------------- the front end ----------------
def test_front_end(gmk):
    from gomokuai_amd import interface
    from gomokuai_amd.network import PatternEvaluator
    core = interface._core()
    board = core.Board()
    for cell in (112, 113, 97):
        board.apply_move(core.Position(cell))
    agent = interface.make_agent("pattern-az", iterations=16, quiet=True, leaves=4)
    try:
        assert isinstance(agent, interface.NetworkAgent) and agent.symmetry is None and agent.leaves == 4
        agent.sync_with_board(board)
        move = agent.get_action(board)
        assert 0 <= int(move.id) < N and int(move.id) not in (112, 113, 97)
        assert agent.debug_message()["playouts"] == 16
    finally:
        agent.close()
    with pytest.raises(ValueError, match="not a learned function"):
        PatternEvaluator().symmetric("all")
    value, probs = PatternEvaluator().eval_state(board)
    assert -1.0 <= value <= 1.0 and probs.shape == (N,) and abs(float(probs.astype(np.float64).sum()) - 1.0) <= 225 * 2.0 ** -24
    assert not probs[[112, 113, 97]].any()
