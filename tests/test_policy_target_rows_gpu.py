"""The policy target's second mode (GMK_TARGET_POLICY, K21): a record's row read as a distribution, pi = (float)((double)w / (double)sum w), through the
fixed-stride, packed and replay entries against numpy, bit for bit, with the augmentation on and off, on rows written by the Gumbel entries and on
hand-made rows; and GMK_TARGET_VISITS through the new entries against the entries there were, byte for byte."""
import numpy as np
import pytest

import az_leaves_reference as R
from gomokuai_amd import lib as G
from gomokuai_amd import selfplay
from policy_target_reference import symmetry_perms

pytestmark = pytest.mark.gpu

N = 225
LENS = [9, 40, 225, 17]


def _gumbel_rows():
    """Improved-policy rows as gmk_az_root_choice_gumbel writes them: six roots, sixteen playouts of a host network"""
    import torch
    from test_az_gumbel_gpu import _host_network, _roots
    tree = G.AlphaZeroMCTS(len(R.OPENINGS), node_capacity=1 << 14, gumbel=(8, 16, 50.0, 1.0, 99, 0))
    tree.set_roots(*_roots(R.OPENINGS))
    tree.search(_host_network(R.sharpened), 16)
    cells, rows = torch.zeros(tree.n, dtype=torch.int16, device="cuda"), torch.zeros((tree.n, N), dtype=torch.int16, device="cuda")
    tree.root_choice(cells, rows, gumbel=True)
    out = rows.cpu().numpy().view(np.uint16)
    tree.close()
    assert (np.abs(out.astype(np.int64).sum(1) - 65535) <= 225).all()
    return out


@pytest.fixture(scope="module")
def records():
    """Four games whose rows cycle through: one-hot, uniform, saturated, all zeros, random counts, and the Gumbel entries' rows"""
    import torch
    G.init()
    rng = np.random.RandomState(8)
    one_hot = np.zeros(N, np.uint16); one_hot[77] = 65535
    pool = [one_hot, np.full(N, 291, np.uint16), np.full(N, 65535, np.uint16), np.zeros(N, np.uint16), rng.randint(0, 1000, N).astype(np.uint16),
            (rng.randint(0, 2, N) * rng.randint(1, 65536, N)).astype(np.uint16)] + list(_gumbel_rows())
    n = len(LENS)
    moves = np.stack([rng.permutation(N) for _ in range(n)]).astype(np.uint8)
    visits = np.zeros((n, N, N), np.uint16)
    k = 0
    for g in range(n):
        for t in range(LENS[g]):
            visits[g, t] = pool[k % len(pool)]
            k += 1
    winner = np.array([1, -1, 0, 1], np.int8)
    rec = selfplay.GameRecords(torch.from_numpy(moves).cuda(), torch.tensor(LENS, dtype=torch.int32, device="cuda"), torch.from_numpy(winner).cuda(),
                               torch.from_numpy(visits.view(np.int16)).cuda())
    return rec, visits


def _expected(rows):
    total = rows.astype(np.int64).sum(-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        pi = (rows.astype(np.float64) / total.astype(np.float64)).astype(np.float32)
    return np.where(total > 0, pi, np.float32(0.0))


def _sample_rows(visits):
    return np.concatenate([visits[g, :LENS[g]] for g in range(len(LENS))])


@pytest.mark.parametrize("augment", [False, True])
def test_policy_target_from_records_and_packed(records, augment):
    rec, visits = records
    want = _expected(_sample_rows(visits))
    if augment:
        want = want[:, symmetry_perms()].reshape(-1, N)
    states, values, pi = rec.to_samples(augment=augment, target="policy")
    np.testing.assert_array_equal(pi.cpu().numpy().view(np.uint32), want.view(np.uint32))
    old = rec.to_samples(augment=augment)
    assert np.array_equal(states.cpu().numpy(), old[0].cpu().numpy()) and np.array_equal(values.cpu().numpy(), old[1].cpu().numpy())      # K4 does not depend on the mode
    assert not np.array_equal(pi.cpu().numpy(), old[2].cpu().numpy())
    # the wire form
    import torch
    buf = selfplay.pack_records_device(rec)
    n = len(rec)
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    G.records_scan(buf.data_ptr(), n, offsets.data_ptr(), stream)
    game, move = selfplay._sample_lists(np.array(LENS, np.int32), 0)
    d_game, d_move = torch.from_numpy(game).cuda(), torch.from_numpy(move).cuda()
    copies = 8 if augment else 1
    out = (torch.zeros((len(game) * copies, 6, N), dtype=torch.uint8, device="cuda"), torch.zeros(len(game) * copies, device="cuda"), torch.zeros((len(game) * copies, N), device="cuda"))
    G.samples_from_packed(buf.data_ptr(), n, offsets.data_ptr(), d_game.data_ptr(), d_move.data_ptr(), len(game), augment, *[t.data_ptr() for t in out], stream, target="policy")
    np.testing.assert_array_equal(out[2].cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert np.array_equal(out[0].cpu().numpy().reshape(states.shape), states.cpu().numpy())


@pytest.mark.parametrize("augment", [False, True])
def test_policy_target_from_the_replay_buffer(records, augment):
    rec, visits = records
    rows = _expected(_sample_rows(visits))
    perms = symmetry_perms()
    starts = np.concatenate([[0], np.cumsum(LENS)])
    population = sum(LENS) * (8 if augment else 1)
    for target in ("policy", "visits"):
        buf = selfplay.ReplayBuffer(4096, 16, seed=5, target=target)
        buf.extend(rec)
        states, values, pi, picked = buf.sample(min(200, population), step=3, augment=augment, return_picked=True)
        plain = selfplay.ReplayBuffer(4096, 16, seed=5)
        plain.extend(rec)
        s0, v0, p0, k0 = plain.sample(min(200, population), step=3, augment=augment, return_picked=True)
        assert buf.status() == (0, 0) and plain.status() == (0, 0)
        assert np.array_equal(picked.cpu().numpy(), k0.cpu().numpy()) and np.array_equal(states.cpu().numpy(), s0.cpu().numpy())     # the draw does not depend on the mode
        if target == "visits":                                   # the new entry in the old mode: byte for byte what gmk_replay_sample writes
            assert np.array_equal(pi.cpu().numpy().view(np.uint32), p0.cpu().numpy().view(np.uint32)) and np.array_equal(values.cpu().numpy(), v0.cpu().numpy())
        else:
            pk = picked.cpu().numpy()
            want = np.stack([rows[starts[g] + t][perms[a]] for g, t, a in pk])
            np.testing.assert_array_equal(pi.cpu().numpy().view(np.uint32), want.view(np.uint32))
        buf.close(); plain.close()


def test_visits_target_through_the_new_entries_is_the_old_output(records):
    import torch
    rec, _ = records
    L = G.load()
    n = len(rec)
    game, move = selfplay._sample_lists(np.array(LENS, np.int32), 0)
    d_game, d_move = torch.from_numpy(game).cuda(), torch.from_numpy(move).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    buf = selfplay.pack_records_device(rec)
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    G.records_scan(buf.data_ptr(), n, offsets.data_ptr(), stream)
    S = len(game) * 8
    make = lambda: (torch.zeros((S, 6, N), dtype=torch.uint8, device="cuda"), torch.zeros(S, device="cuda"), torch.zeros((S, N), device="cuda"))
    old, new, old_p, new_p = make(), make(), make(), make()
    p = lambda t: t.data_ptr()
    G.samples_from_records(p(rec.moves), p(rec.lens), p(rec.visits), p(rec.winner), p(d_game), p(d_move), len(game), 1, *[p(t) for t in old], stream)
    G.samples_from_records(p(rec.moves), p(rec.lens), p(rec.visits), p(rec.winner), p(d_game), p(d_move), len(game), 1, *[p(t) for t in new], stream, target=G.TARGET_VISITS)
    G.samples_from_packed(p(buf), n, p(offsets), p(d_game), p(d_move), len(game), 1, *[p(t) for t in old_p], stream)
    G.samples_from_packed(p(buf), n, p(offsets), p(d_game), p(d_move), len(game), 1, *[p(t) for t in new_p], stream, target="visits")
    torch.cuda.synchronize()
    for a, b in list(zip(old, new)) + list(zip(old_p, new_p)):
        assert np.array_equal(a.cpu().numpy().view(np.uint8), b.cpu().numpy().view(np.uint8))
    assert L.gmk_samples_from_records_target(p(rec.moves), p(rec.lens), p(rec.visits), p(rec.winner), p(d_game), p(d_move), len(game), 1, 2, *[p(t) for t in new], stream) == -3
    assert L.gmk_samples_from_packed_target(p(buf), n, p(offsets), p(d_game), p(d_move), len(game), 1, -1, *[p(t) for t in new_p], stream) == -3
    with pytest.raises(ValueError):
        selfplay.ReplayBuffer(4096, 16, target="rows")
