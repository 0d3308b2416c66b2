"""K7 self-play moves drawn from the root's visit counts on the device (gmk_az_advance_sampled, gmk_az_root_choice_sampled: the sampled
instantiations of az_advance_kernel and az_root_choice_kernel) against the host form gmk_move_sample_host and against
tests/move_sample_reference.py, the restatement tests/test_move_sample.py holds the host form to.  Everything is compared exactly."""
import functools

import numpy as np
import pytest

import az_leaves_reference as R
import az_proof_reference as P
import move_sample_reference as M
from gomokuai_amd import lib as G
from gomokuai_amd import selfplay
from helpers import PaddedNetwork
from test_az_proof_gpu import _tree, mixed, parity_openings
from test_az_proof_reference import FIVE
from test_az_vcf_gpu import _host_network, _roots

pytestmark = pytest.mark.gpu

N = 225
SEED = 0x9E3779B97F4A7C15
ERR_ARG, ERR_STATE = -3, -4


def _cells(n):
    import torch
    return torch.full((n,), -7, dtype=torch.int16, device="cuda")


def _records(openings):
    import torch
    n = len(openings)
    moves, lens = np.zeros((n, N), np.uint8), np.array([len(p) for p in openings], np.int32)
    for g, p in enumerate(openings):
        moves[g, :len(p)] = p
    return [torch.from_numpy(moves).cuda(), torch.zeros((n, N, N), dtype=torch.int16, device="cuda"), torch.from_numpy(lens).cuda(), torch.zeros(n, dtype=torch.int8, device="cuda")]


# ---------------- 1. the choice against the host form ----------------
@pytest.mark.parametrize("proof", [False, True])
def test_root_choice_equals_the_host_form(proof):
    """64 games on the eight parity openings (each eight times: the trees repeat, the games' ids and so their draws do not)"""
    openings = (parity_openings() * 8)[:64]
    first = 1000
    tree = _tree(openings, 1, 1.0, 8 if proof else 0, proof=proof)
    tree.search(_host_network(mixed), 48)
    st = tree.root_stats()
    assert (st["root_visits"] == 48).all() and (st["status"] == 0).all()
    proofs = tree.root_proofs()["children"] if proof else None
    assert not proof or (proofs == P.WINS).any()
    stones, ids = np.array([len(p) for p in openings], np.int32), first + np.arange(64)
    cells, rows = _cells(64), _cells(64 * N).view(64, N)
    tree.root_choice(cells)
    greedy = cells.cpu().numpy().copy()
    assert greedy.tolist() == selfplay._root_choice(st["visits"], proofs).tolist()
    for power in (1, 3):
        cells.fill_(-7)
        tree.root_choice(cells, rows, sample=(225, power, SEED, first))
        got = cells.cpu().numpy()
        assert got.tolist() == G.move_sample_host(st["visits"], stones, ids, 225, power, SEED, proofs).tolist()
        assert got.tolist() == [M.choose(st["visits"][g], int(stones[g]), int(ids[g]), 225, power, SEED, None if proofs is None else proofs[g]) for g in range(64)]
        assert (got != greedy).any()                            # a draw, not the maximum
        assert (got >= 0).all() and (st["visits"][np.arange(64), got] > 0).all()
        np.testing.assert_array_equal(rows.cpu().numpy().view(np.uint16), np.minimum(st["visits"], 65535))
    # the stones decide: with S at the stone count of the longest of the short openings only the shorter ones are drawn
    cells.fill_(-7)
    tree.root_choice(cells, sample=(7, 1, SEED, first))
    got = cells.cpu().numpy()
    assert got.tolist() == G.move_sample_host(st["visits"], stones, ids, 7, 1, SEED, proofs).tolist()
    assert (stones >= 7).sum() >= 32 and (stones < 7).sum() >= 16 and (got[stones >= 7] == greedy[stones >= 7]).all()
    # ... and so do the ids of gmk_az_set_game_ids
    other = (np.arange(64)[::-1] * 3).astype(np.uint32)
    tree.set_game_ids(other)
    tree.root_choice(cells, sample=(225, 1, SEED, 5))
    assert cells.cpu().numpy().tolist() == G.move_sample_host(st["visits"], stones, 5 + other, 225, 1, SEED, proofs).tolist()
    tree.close()


def test_a_losing_child_is_played_not_drawn():
    """tests/test_az_proof_gpu.py's open four under uniform priors: the five's child is a proven loss for white and has one visit of > 100"""
    ref = P.ProofSearch(R.OPEN_FOUR, R.uniform, 0, 64, proof=True, c_puct=5.0)
    while not any(ref.proof):
        ref.search(1)
    playouts = ref.visits[0]
    assert ref.choice_cell() == FIVE and ref.cell[ref.plain_choice()] != FIVE
    network = _host_network(R.uniform)
    tree = _tree([R.OPEN_FOUR] * 3, 1, 5.0, 0)
    tree.search(network, playouts)
    st, proofs = tree.root_stats(), tree.root_proofs()["children"]
    assert int(st["visits"][0].argmax()) != FIVE and proofs[0, FIVE] == P.LOSES
    cells = _cells(3)
    for power in (1, 3):
        tree.root_choice(cells, sample=(225, power, SEED, 0))
        assert cells.cpu().tolist() == [FIVE] * 3 == G.move_sample_host(st["visits"], [len(R.OPEN_FOUR)] * 3, [0, 1, 2], 225, power, SEED, proofs).tolist()
    rec = _records([R.OPEN_FOUR] * 3)
    assert tree.advance(rec[0], None, rec[2], rec[3], reuse_subtree=True, sample=(225, 1, SEED, 0)) == 0
    assert rec[0][:, len(R.OPEN_FOUR)].cpu().tolist() == [FIVE] * 3 and rec[3].cpu().tolist() == [1] * 3
    off = _tree([R.OPEN_FOUR] * 3, 1, 5.0, 0, proof=False)       # without the option the five is one child of > 100 with one visit: drawn, rarely
    off.search(network, playouts)
    off.root_choice(cells, sample=(225, 1, SEED, 0))
    assert cells.cpu().tolist() == G.move_sample_host(off.root_stats()["visits"], [len(R.OPEN_FOUR)] * 3, [0, 1, 2], 225, 1, SEED).tolist() != [FIVE] * 3
    tree.close()
    off.close()


# ---------------- 2. off is off ----------------
@pytest.mark.parametrize("proof", [False, True])
def test_zero_plies_is_the_unsampled_entry(proof):
    openings = parity_openings()[:5]
    network = _host_network(mixed)
    trees = [_tree(openings, 1, 1.0, 8 if proof else 0, proof=proof) for _ in range(2)]
    recs = [_records(openings) for _ in range(2)]
    cells = [_cells(5), _cells(5)]
    rows = [_cells(5 * N).view(5, N), _cells(5 * N).view(5, N)]
    for ply in range(3):
        for tree in trees:
            tree.search(network, 16)
        trees[0].root_choice(cells[0], rows[0])
        trees[1].root_choice(cells[1], rows[1], sample=(0, 1, SEED + ply, 40))
        assert cells[0].cpu().tolist() == cells[1].cpu().tolist() and (rows[0] == rows[1]).all()
        left = [trees[0].advance(*recs[0], reuse_subtree=True), trees[1].advance(*recs[1], reuse_subtree=True, sample=(0, 3, SEED + ply, 40))]
        assert left[0] == left[1]
        a, b = trees[0].root_stats(), trees[1].root_stats()
        for k in a:
            np.testing.assert_array_equal(a[k].view(np.uint32) if a[k].dtype == np.float32 else a[k], b[k].view(np.uint32) if b[k].dtype == np.float32 else b[k], "%s, ply %d" % (k, ply))
        for x, y in zip(*recs):
            assert (x == y).all()
    assert int(recs[0][2].sum()) > sum(len(p) for p in openings)
    for tree in trees:
        tree.close()


# ---------------- 3. the loops ----------------
@pytest.fixture(scope="module")
def net():
    from gomokuai_amd.network import FusedPolicyValueNetwork, PolicyValueNetwork
    G.init()
    net = FusedPolicyValueNetwork(PolicyValueNetwork(seed=8).cuda().eval())
    yield net
    net.close()


@pytest.fixture(scope="module")
def fused(net):
    return PaddedNetwork(net, 11)


@functools.lru_cache(maxsize=None)
def _greedy_games(fused):
    return selfplay.play_network_games(11, fused, 12, opening_plies=2, first_game_id=70, seed=2).cpu()


@pytest.mark.parametrize("power", [1, 2])
def test_every_move_follows_from_its_visit_row(fused, power):
    S = 6
    rec = selfplay.play_network_games(11, fused, 12, opening_plies=2, first_game_id=70, seed=2, sample_plies=S, sample_power=power).cpu()
    moves, visits, lens = rec.moves.numpy(), rec.visits.numpy().view(np.uint16), rec.lens.numpy()
    assert not rec.overflow and int(lens.min()) >= 9
    drawn = 0
    for g in range(11):
        for t in range(2, int(lens[g])):
            row = visits[g, t].astype(np.uint32)
            if t < S:
                want = M.choose(row, t, 70 + g, S, power, 2)
                drawn += want != int(row.argmax())
            else:
                want = int(row.argmax())                         # the first maximum
            assert int(moves[g, t]) == want, (g, t)
    assert drawn > 0
    plain = _greedy_games(fused)
    assert any(int(plain.lens[g]) != int(lens[g]) or (plain.moves[g].numpy() != moves[g]).any() for g in range(11))


@pytest.mark.parametrize("options", [dict(vcf=(8, 64), proof=True), dict(leaves=4)], ids=["solver-proofs", "L4"])
def test_one_set_of_games_on_every_loop(net, options):
    """tests/test_az_proof_gpu.py's test_network_self_play_through_slots_and_on_both_loops with the first six plies drawn; the host-driven slots
    (fresh roots only) against the device loop with fresh roots"""
    fused = PaddedNetwork(net, 11 * options.get("leaves", 1))
    kw = dict(opening_plies=2, first_game_id=70, seed=2, root_noise=(0.05, 0.25), sample_plies=6, sample_power=1, **options)
    few = selfplay.play_network_games(11, fused, 12, slots=4, reuse_subtree=True, **kw).cpu()
    full = selfplay.play_network_games(11, fused, 12, slots=11, reuse_subtree=True, **kw).cpu()
    host = selfplay.play_network_games(11, fused, 12, reuse_subtree=True, device_loop=False, **kw).cpu()
    kw["root_noise"] = None                                      # (the host-driven slots take no root noise)
    fresh = selfplay.play_network_games(11, fused, 12, slots=11, reuse_subtree=False, **kw).cpu()
    fresh_slots = selfplay.play_network_games(11, fused, 12, slots=4, reuse_subtree=False, device_loop=False, **kw).cpu()
    for one, others in ((few, (full, host)), (fresh, (fresh_slots,))):
        for other in others:
            assert not one.overflow and not other.overflow
            assert (one.lens == other.lens).all() and (one.winner == other.winner).all() and int(one.lens.min()) >= 9
            for g in range(11):
                n = int(one.lens[g])
                assert n == N or int(one.winner[g]) != 0
                assert (one.moves[g, :n] == other.moves[g, :n]).all() and (one.visits[g, :n] == other.visits[g, :n]).all()


# ---------------- 4. misuse ----------------
def test_misuse_is_refused_and_the_handle_goes_on():
    import torch
    L = G.load()
    openings = parity_openings()[:3]
    G.init()
    tree = G.AlphaZeroMCTS(3, node_capacity=1 << 12, c_puct=1.0, leaves=4)
    rec = _records(openings)
    cells = _cells(3)
    stream = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()
    advance = lambda plies, power, a=tree.h, m=p(rec[0]): L.gmk_az_advance_sampled(a, m, p(rec[1]), p(rec[2]), p(rec[3]), 1, plies, power, SEED, 0, None, stream)
    choice = lambda plies, power, a=tree.h, c=p(cells): L.gmk_az_root_choice_sampled(a, c, None, plies, power, SEED, 0, stream)
    assert advance(6, 1) == ERR_STATE and choice(6, 1) == ERR_STATE                    # no roots yet
    assert b"gmk_az_root_choice_sampled" in L.gmk_last_error()
    tree.set_roots(*_roots(openings))
    for plies, power in ((-1, 1), (226, 1), (6, 0), (6, 4)):
        assert advance(plies, power) == ERR_ARG and choice(plies, power) == ERR_ARG
    assert advance(6, 1, None) == ERR_ARG and advance(6, 1, tree.h, None) == ERR_ARG and choice(6, 1, None) == ERR_ARG and choice(6, 1, tree.h, None) == ERR_ARG
    network = _host_network(mixed)
    tree.add_playouts(8)
    states = tree.select()                                       # L = 4: the marks are up until the expand
    assert advance(6, 1) == ERR_STATE and b"gmk_az_advance_sampled" in L.gmk_last_error()
    assert choice(0, 1) == 0                                     # (gmk_az_root_choice reads the roots whatever is pending, and so does this)
    values, probs = network(states)
    tree.expand(values.contiguous(), probs.contiguous())
    torch.cuda.synchronize()
    assert rec[2].cpu().tolist() == [len(o) for o in openings] and not rec[1].any()    # nothing was played by the refused calls
    tree.search(network, 24)
    st = tree.root_stats()
    tree.root_choice(cells, sample=(225, 1, SEED, 0))
    want = G.move_sample_host(st["visits"], [len(o) for o in openings], [0, 1, 2], 225, 1, SEED).tolist()
    assert cells.cpu().tolist() == want
    tree.advance(*rec, reuse_subtree=True, sample=(225, 1, SEED, 0))
    assert [int(rec[0][g, len(o)]) for g, o in enumerate(openings)] == want
    tree.close()
