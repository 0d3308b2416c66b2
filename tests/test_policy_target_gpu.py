"""The policy target pi of every copy of the formula against float64 (tests/policy_target_reference.py: pi64, its derived bound, the cut),
at search-scale visit counts: K5 on fixed-stride records and on their wire form (records_kernel.hip), the replay draw
(replay_kernel.hip) and the host copy (gmk_visits_to_pi).  Each path is compared with float64, not with another copy; the three device
paths are, in addition, the same bits -- which is replay_kernel.hip's summation-order claim tested where squares are inexact in float32.
tests/test_policy_target_reference.py shows on the CPU that the bound holds for a float32 emulation and refuses the listed mistakes."""
import numpy as np
import pytest
import torch

import helpers
import policy_target_reference as R
from gomokuai_amd import lib as G
from gomokuai_amd import selfplay

pytestmark = pytest.mark.gpu

N = R.N
DEV = "cuda"
STONES = (0, 14, 15, 60)


@pytest.fixture(autouse=True, scope="module")
def _device():
    G.init(0)


def _to_device(records):
    return selfplay.GameRecords(torch.from_numpy(records["moves"]).to(DEV), torch.from_numpy(records["lens"]).to(DEV),
                                torch.from_numpy(records["winner"]).to(DEV), torch.from_numpy(records["visits"].view(np.int16)).to(DEV))


def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.fixture(scope="module")
def perms():
    """int [8, 225]: where helpers.symmetries takes each cell of pi from"""
    return np.stack([pi for _, pi in helpers.symmetries(np.zeros((1, 15, 15)), np.arange(N))]).astype(np.int64)


@pytest.fixture(scope="module")
def refs(perms):
    ref = R.records_reference()
    return {False: ref, True: R.augmented(ref, perms)}


@pytest.fixture(scope="module")
def rec():
    return _to_device(R.RECORDS)


@pytest.fixture(scope="module")
def k5(rec):
    """(states, values, pi) of K5 on the fixed-stride records, plain and augmented; made once, never written to"""
    return {augment: rec.to_samples(augment=augment) for augment in (False, True)}


@pytest.mark.parametrize("augment", [False, True])
def test_k5_fixed_stride(refs, k5, augment):
    worst = R.check_by_class(refs[augment], k5[augment][2].cpu().numpy(), "K5 fixed-stride, augment=%s" % augment)
    R.show("K5 fixed-stride, augment=%s" % augment, worst)
    assert set(worst) == set(R.CLASS_NAMES)


@pytest.mark.parametrize("augment", [False, True])
def test_k5_wire_form(refs, rec, k5, augment):
    wire = selfplay.pack_records_device(rec)
    got = selfplay.samples_from_packed(wire, len(rec), augment=augment)
    R.show("K5 wire form, augment=%s" % augment, R.check_by_class(refs[augment], got[2].cpu().numpy(), "K5 wire form, augment=%s" % augment))
    assert all(_bits_equal(a, b) for a, b in zip(got, k5[augment]))


@pytest.mark.parametrize("augment", [False, True])
def test_replay_draw(refs, rec, k5, augment):
    """Every sample once (a full sweep): each drawn pi against float64, and bit for bit the K5 row of the (game, ply, symmetry) it names."""
    plies = int(R.RECORDS["lens"].sum())
    buf = selfplay.ReplayBuffer(max(plies, N), max_games=len(rec), seed=9)
    buf.extend(rec)
    assert buf.status()[0] == 0 and buf.stats()["population"] == plies
    M = plies * (8 if augment else 1)
    _, _, pi, picked = buf.sample(M, step=2, augment=augment, dtype=torch.uint8, return_picked=True)
    assert buf.status()[1] == 0
    buf.close()
    cum = np.concatenate([[0], np.cumsum(R.RECORDS["lens"])])
    p = picked.cpu().numpy()
    rows = cum[p[:, 0]] + p[:, 1]
    rows = 8 * rows + p[:, 2] if augment else rows
    assert np.array_equal(np.sort(rows), np.arange(M))
    worst = R.check_by_class(R.take(refs[augment], rows), pi.cpu().numpy(), "replay draw, augment=%s" % augment)
    R.show("replay draw, augment=%s" % augment, worst)
    assert _bits_equal(pi, k5[augment][2][torch.from_numpy(rows).to(DEV)])


def test_host_on_every_class():
    per = 12
    v = np.concatenate([np.repeat(R.rows(kind, per, seed=1), len(STONES), 0) for kind in R.CLASS_NAMES])
    stones = np.tile(np.array(STONES), per * len(R.CLASS_NAMES))
    ref = R.reference(v, stones, np.repeat(np.array(R.CLASS_NAMES), per * len(STONES)))
    got = np.stack([G.visits_to_pi(row, int(s)) for row, s in zip(ref["visits"], ref["stones"])])
    R.show("gmk_visits_to_pi", R.check_by_class(ref, got, "gmk_visits_to_pi"))


def test_host_samples_of_one_game(refs, rec):
    g = R.GAME_LENS.index(17)
    game, _ = R.sample_lists()
    tuples = rec.samples(g)
    assert len(tuples) == 17
    ref = R.take(refs[False], np.nonzero(game == g)[0])
    R.show("GameRecords.samples", R.check_by_class(ref, np.stack([t[2] for t in tuples]), "GameRecords.samples(%d)" % g))


# ---------------- the edges, by name ----------------
EDGE_PLIES = {"switch": (14, 15), "all_zero": (3, 17), "one_cell": (4, 18), "tied_max": (5, 19)}


def _edge_records():
    """One game of 20 plies: the same kept-subtree row at plies 14 and 15, and a row without visits, a row with one visited cell and a row
    with tied maxima on either side of them; small counts elsewhere."""
    records = {"moves": R.RECORDS["moves"][:1].copy(), "lens": np.array([20], np.int32), "winner": np.array([1], np.int8),
               "visits": R.RECORDS["visits"][:1].copy()}
    for t in range(20):
        records["visits"][0, t] = R.row("small", 500 + t)
    rows = {"switch": R.row("kept_subtree", 77), "all_zero": R.row("all_zero", 0), "one_cell": R.row("one_cell", 4), "tied_max": R.row("tied_max", 6)}
    assert rows["one_cell"].max() > 4096 and rows["tied_max"].max() > 4096 and (rows["tied_max"] == rows["tied_max"].max()).sum() >= 2
    for name, plies in EDGE_PLIES.items():
        for t in plies:
            records["visits"][0, t] = rows[name]
    return records


def _edge_pi(path, records):
    """pi float32 [20, 225] of the edge game by one of the four paths"""
    if path == "host":
        return np.stack([G.visits_to_pi(records["visits"][0, t].astype(np.uint32), t) for t in range(20)])
    rec = _to_device(records)
    if path == "k5":
        return rec.to_samples()[2].cpu().numpy()
    if path == "wire":
        return selfplay.samples_from_packed(selfplay.pack_records_device(rec), 1)[2].cpu().numpy()
    assert path == "replay"
    buf = selfplay.ReplayBuffer(N, max_games=1, seed=1)
    buf.extend(rec)
    _, _, pi, picked = buf.sample(20, step=0, augment=False, dtype=torch.uint8, return_picked=True)
    assert buf.status() == (0, 0)
    buf.close()
    order = np.argsort(picked.cpu().numpy()[:, 1])
    assert np.array_equal(picked.cpu().numpy()[order, 1], np.arange(20))
    return pi.cpu().numpy()[order]


@pytest.mark.parametrize("path", ["k5", "wire", "replay", "host"])
def test_edges(path):
    records = _edge_records()
    v = records["visits"][0]
    pi = _edge_pi(path, records)
    ref = R.reference(v[:20], np.arange(20), ["ply %d" % t for t in range(20)])
    R.check(ref, pi, "edges, %s" % path)

    # tau = 1 at 14 stones and 0.01 at 15, on the same row
    early, late = EDGE_PLIES["switch"]
    assert np.array_equal(v[early], v[late])
    R.check(R.reference(v[early], 14), pi[early:early + 1], "%s, t = 14 against tau = 1" % path)
    R.check(R.reference(v[late], 15), pi[late:late + 1], "%s, t = 15 against tau = 0.01" % path)
    assert R.rejects(R.reference(v[early], 15), pi[early:early + 1]) and R.rejects(R.reference(v[late], 14), pi[late:late + 1])

    # no visits: uniform below 15 stones, all zeros from 15 on (0 / 0 fails `> eps`)
    early, late = EDGE_PLIES["all_zero"]
    assert np.array_equal(pi[early], np.full(N, np.float32(1.0 / N))) and np.array_equal(pi[late], np.zeros(N, np.float32))

    # one visited cell: exactly 1 there and 0 elsewhere from 15 stones on
    early, late = EDGE_PLIES["one_cell"]
    cell = int(np.argmax(v[late]))
    assert pi[late, cell] == 1.0 and np.count_nonzero(pi[late]) == 1
    assert np.count_nonzero(pi[early]) == 1 and 0.9999 < pi[early, cell] < 1.0      # (2 + eps) / (2 + 225 eps)

    # tied maxima: identical bits
    for t in EDGE_PLIES["tied_max"]:
        top = pi[t][v[t] == v[t].max()]
        assert len(top) >= 2 and len(set(top.view(np.uint32).tolist())) == 1 and top[0] == pi[t].max()

    _check_sums(ref, pi)


def _check_sums(ref, pi):
    """Outside the rows without visits, sum(pi) is within the summed bound of 1 (the mass the cut removes is the reference's, not an error)."""
    rows = ref["visits"].sum(1) > 0
    total = np.asarray(pi, np.float64)[rows].sum(1)
    cut_mass = (ref["raw"] - ref["pi"])[rows].sum(1)
    assert (cut_mass >= 0).all() and (cut_mass < N * R.EPS).all()
    slack = ref["bound"][rows].sum(1) + np.where(ref["exempt"][rows], ref["raw"][rows], 0.0).sum(1) + 1e-15
    assert (np.abs(total - (1.0 - cut_mass)) <= slack).all(), np.abs(total - (1.0 - cut_mass)).max()
    assert (np.abs(total - 1.0) <= slack + cut_mass).all()


def test_sums_are_one(refs, k5):
    _check_sums(refs[False], k5[False][2].cpu().numpy())
    _check_sums(refs[True], k5[True][2].cpu().numpy())
