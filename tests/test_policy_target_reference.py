"""The float64 policy target and its bound (tests/policy_target_reference.py) earn their trust on the CPU before the device paths are held to
them (tests/test_policy_target_gpu.py): a float32 emulation of the formula stays inside the bound with either association of the sum of
squares, the band around the cut in which an element is excused is small, every listed mistake lands outside the bound, and the oracle's
restatement passes."""
import numpy as np
import pytest

import policy_target_reference as R

STONES = (0, 14, 15, 60)
ROWS_PER_CLASS = 12


@pytest.fixture(scope="module")
def class_ref():
    """reference() of ROWS_PER_CLASS rows of every class at each of STONES"""
    v = np.concatenate([np.repeat(R.rows(kind, ROWS_PER_CLASS, seed=1), len(STONES), 0) for kind in R.CLASS_NAMES])
    stones = np.tile(np.array(STONES), ROWS_PER_CLASS * len(R.CLASS_NAMES))
    cls = np.repeat(np.array(R.CLASS_NAMES), ROWS_PER_CLASS * len(STONES))
    return R.reference(v, stones, cls)


@pytest.mark.parametrize("order", ["tree", "seq"])
def test_float32_emulation_is_inside_the_bound(class_ref, order):
    for name, ref in (("classes", class_ref), ("records", R.records_reference())):
        worst = R.check_by_class(ref, R.emulate32(ref["visits"], ref["stones"], order), "%s, %s sum" % (name, order))
        R.show("emulation (%s sum) on %s" % (order, name), worst)
        assert set(worst) == set(R.CLASS_NAMES)


def test_exempt_band_is_small(class_ref):
    ref = R.records_reference()
    R.not_vacuous(ref)
    R.not_vacuous(R.augmented(ref, R.symmetry_perms()))
    R.not_vacuous(class_ref)
    print("exempt elements: %d of %d in the records, %d of %d in the class rows"
          % (ref["exempt"].sum(), ref["exempt"].size, class_ref["exempt"].sum(), class_ref["exempt"].size))


def test_records_cover_the_plies_and_classes():
    game, ply = R.sample_lists()
    ref = R.records_reference()
    assert len(R.GAME_LENS) <= 6 and {1, 16, 17, 225} <= set(R.GAME_LENS)
    assert {0, 1, 13, 14, 15, 16, 224} <= set(ply.tolist())
    for name in R.CLASS_NAMES:
        t = ply[ref["cls"] == name]
        assert (t < R.LATE).any() and (t >= R.LATE).any(), name
    same_game = game[1:] == game[:-1]
    assert (ref["cls"][1:][same_game] != ref["cls"][:-1][same_game]).all()
    assert R.RECORDS["visits"].nbytes <= 640 * 1024
    for kind in R.CLASS_NAMES:                                   # the generators are seeded
        assert np.array_equal(R.row(kind, 5), R.row(kind, 5))
    assert (R.rows("uint16_edges", 4) >= 32768).any() and R.rows("flat_4096", 1).min() >= 4090


@pytest.mark.parametrize("mistake", sorted(R.MISTAKES))
def test_mistakes_in_the_formula_are_rejected(class_ref, mistake):
    for order in ("tree", "seq"):
        refused = R.rejects(class_ref, R.emulate32(class_ref["visits"], class_ref["stones"], order, **R.MISTAKES[mistake]))
        print("%s (%s sum) is refused on: %s" % (mistake, order, ", ".join(refused)))
        assert refused, mistake
        ref = R.records_reference()
        assert R.rejects(ref, R.emulate32(ref["visits"], ref["stones"], order, **R.MISTAKES[mistake])), mistake


def test_the_row_of_the_ply_before_is_rejected():
    game, ply = R.sample_lists()
    ref = R.records_reference()
    wrong = R.emulate32(R.RECORDS["visits"][game, np.maximum(ply - 1, 0)], ply)
    refused = R.rejects(ref, wrong)
    print("the visit row of ply t - 1 is refused on: %s" % ", ".join(refused))
    assert set(refused) == set(R.CLASS_NAMES)                     # every class has a neighbour of another class


def test_pi_left_in_place_under_the_symmetry_is_rejected():
    ref = R.records_reference()
    perms = R.symmetry_perms()
    aug = R.augmented(ref, perms)
    right = R.emulate32(ref["visits"], ref["stones"])
    R.check(aug, right[:, perms].reshape(-1, R.N), "emulation, augmented")
    refused = R.rejects(aug, np.repeat(right, 8, 0))
    print("pi not moved with the symmetry is refused on: %s" % ", ".join(refused))
    assert refused
    for a in range(1, 8):                                        # ... under each of the seven symmetries that move anything
        rows = np.arange(a, aug["pi"].shape[0], 8)
        assert R.rejects(R.take(aug, rows), right), a


def test_symmetry_perms_are_the_helpers():
    import helpers
    got = np.stack([pi for _, pi in helpers.symmetries(np.zeros((1, 15, 15)), np.arange(R.N))]).astype(np.int64)
    assert np.array_equal(got, R.symmetry_perms())


def test_closed_forms():
    """pi64 on rows whose answer is known without it."""
    zero = np.zeros(R.N, np.uint16)
    assert np.allclose(R.pi64(zero, 14), 1.0 / R.N, rtol=1e-12) and (R.pi64(zero, 15) == 0).all()
    assert R.reference(zero, 15)["bound"].max() == 0
    one = R.row("one_cell", 3)
    late = R.pi64(one, 15)[0]
    assert late[one > 0] == 1.0 and late.sum() == 1.0
    early = R.pi64(one, 0)[0]                                      # (2 + eps) / (2 + 225 eps) on the cell, eps / that cut to 0 elsewhere
    assert np.isclose(early[one > 0], (2 + R.EPS) / (2 + R.N * R.EPS), rtol=1e-12) and (early[one == 0] == 0).all()
    flat = R.pi64(R.row("all_65535", 0), 60)[0]
    assert np.allclose(flat, 1.0 / R.N, rtol=1e-12)
    tied = R.row("tied_max", 2)
    p = R.pi64(tied, 60)[0]
    assert len(set(p[tied == tied.max()].tolist())) == 1
    # below 2^24 the sum of squares is exact in float32 in any order: no error term for it
    assert R.sum_error(np.full((1, R.N), 272.0))[0] == 0 and R.sum_error(np.full((1, R.N), 274.0))[0] > 0
    v = np.zeros((1, R.N))
    v[0, 7] = 4095
    assert R.sum_error(v)[0] == 0


def test_bound_has_the_issue_scale():
    """The bound is a relative one of the order of 1e-4 at tau = 0.01 and 1e-5 at tau = 1 -- neither a flat 1e-6 nor loose enough to hide a digit."""
    ref = R.records_reference()
    big = ref["raw"] > 1e-4
    rel = np.where(big, ref["bound"] / np.where(big, ref["raw"], 1.0), 0.0)
    late = (ref["stones"] >= R.LATE)[:, None]
    assert rel[late & big].max() < 1e-3 and rel[~late & big].max() < 2e-5, (rel[late & big].max(), rel[~late & big].max())


def test_oracle_is_inside_the_bound(oracle, class_ref):
    got = np.stack([oracle.visits_to_pi(v, int(s)) for v, s in zip(class_ref["visits"], class_ref["stones"])])
    R.show("oracle.visits_to_pi", R.check_by_class(class_ref, got, "oracle"))
