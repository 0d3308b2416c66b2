"""gomokuai_amd.rating without a GPU: summary, elo, elo_interval and sprt against a float64 restatement written here, and hand cases.
Where a quantity's operations are exact in float64 (counts, sums and means of multiples of 1/4 over a few games) the comparison is exact;
elsewhere it is to 1e-12 relative."""
import math

import numpy as np
import pytest

from gomokuai_amd import rating

REL = 1e-12


def close(a, b):
    if math.isinf(a) or math.isinf(b) or a == b:
        return a == b
    return abs(a - b) <= REL * max(abs(a), abs(b))


# ---- the restatement: plain Python floats (IEEE float64), loops instead of numpy ----
def ref_observations(scores, paired):
    s = [float(v) for v in scores]
    return [(s[2 * p] + s[2 * p + 1]) / 2.0 for p in range(len(s) // 2)] if paired else s


def ref_summary(scores, paired):
    s = [float(v) for v in scores]
    x = ref_observations(s, paired)
    mean = math.fsum(s) / len(s)
    var = math.fsum((v - mean) ** 2 for v in x) / len(x)
    pairs = [sum(1 for v in x if v == q) for q in (0.0, 0.25, 0.5, 0.75, 1.0)] if paired else None
    return {"games": len(s), "wins": s.count(1.0), "draws": s.count(0.5), "losses": s.count(0.0), "score": mean, "stderr": math.sqrt(var / len(x)), "pairs": pairs}


def ref_elo(score):
    return -math.inf if score == 0.0 else math.inf if score == 1.0 else -400.0 * math.log10(1.0 / score - 1.0)


def ref_sprt(scores, elo0, elo1, alpha, beta, paired):
    x = ref_observations(scores, paired)
    s0, s1 = 1.0 / (1.0 + 10.0 ** (-elo0 / 400.0)), 1.0 / (1.0 + 10.0 ** (-elo1 / 400.0))
    n = len(x)
    mean = math.fsum(x) / n
    var = math.fsum((v - mean) ** 2 for v in x) / n
    llr = n * (s1 - s0) * (2.0 * mean - s0 - s1) / (2.0 * var) if var > 0.0 else 0.0
    lower, upper = math.log(beta / (1.0 - alpha)), math.log((1.0 - beta) / alpha)
    return {"llr": llr, "lower": lower, "upper": upper, "decision": "H1" if llr >= upper else "H0" if llr <= lower else None}


def _sequences():
    rng = np.random.RandomState(5)
    out = [rng.choice([0.0, 0.5, 1.0], size=n, p=p) for n in (2, 10, 64, 250) for p in ([0.3, 0.2, 0.5], [0.6, 0.1, 0.3], [0.05, 0.9, 0.05])]
    return out + [np.array([1.0, 0.0]), np.array([0.5, 1.0, 1.0, 0.0])]


@pytest.mark.parametrize("paired", [False, True])
def test_summary_and_sprt_follow_the_restatement(paired):
    for s in _sequences():
        got, want = rating.summary(s, paired=paired), ref_summary(s, paired)
        for key in ("games", "wins", "draws", "losses", "pairs"):
            assert got[key] == want[key], key
        assert got["score"] == want["score"]                      # a sum of multiples of 1/2 below 2^53 and one division: exact
        assert close(got["stderr"], want["stderr"]), (got["stderr"], want["stderr"])
        assert got["wins"] + got["draws"] + got["losses"] == got["games"] and (not paired or sum(got["pairs"]) == got["games"] // 2)
        for elo0, elo1, alpha, beta in ((0.0, 20.0, 0.05, 0.05), (-10.0, 5.0, 0.01, 0.1), (-100.0, 100.0, 0.05, 0.05)):
            g, w = rating.sprt(s, elo0, elo1, alpha, beta, paired=paired), ref_sprt(s, elo0, elo1, alpha, beta, paired)
            assert close(g["llr"], w["llr"]) and close(g["lower"], w["lower"]) and close(g["upper"], w["upper"]) and g["decision"] == w["decision"], (g, w)
            assert g["lower"] < 0.0 < g["upper"]


def test_elo_and_its_interval():
    for score in (0.0, 1.0, 0.5, 0.7, 0.25, 1e-9, 1.0 - 1e-9, 0.5 + 1e-12):
        assert close(rating.elo(score), ref_elo(score)), score
    assert rating.elo(0.5) == 0.0 and rating.elo(0.0) == -math.inf and rating.elo(1.0) == math.inf
    assert close(rating.elo(0.7), 400.0 * math.log10(7.0 / 3.0))          # the closed form: -400 log10(3 / 7)
    assert close(rating.elo(0.25), -400.0 * math.log10(3.0)) and close(rating.elo(10.0 / 11.0), 400.0)
    assert close(rating.expected_score(rating.elo(0.7)), 0.7) and rating.expected_score(0.0) == 0.5
    for mean, stderr, z in ((0.5, 0.05, 1.96), (0.7, 0.1, 1.96), (0.9, 0.1, 1.96), (0.02, 0.05, 2.0), (0.5, 0.0, 1.96), (1.0, 0.0, 1.96)):
        lo, mid, hi = rating.elo_interval(mean, stderr, z)
        assert close(lo, ref_elo(max(mean - z * stderr, 0.0))) and close(mid, ref_elo(mean)) and close(hi, ref_elo(min(mean + z * stderr, 1.0)))
        assert lo <= mid <= hi
    assert rating.elo_interval(0.9, 0.1)[2] == math.inf and rating.elo_interval(0.02, 0.05, 2.0)[0] == -math.inf
    assert rating.elo_interval(0.5, 0.0) == (0.0, 0.0, 0.0)
    for bad in (-0.1, 1.1, math.nan):
        with pytest.raises(ValueError):
            rating.elo(bad)


def test_hand_cases():
    draws = [0.5] * 12                                            # all draws: score 1/2, Elo 0, no variance, no evidence
    for paired in (False, True):
        s = rating.summary(draws, paired=paired)
        assert (s["wins"], s["draws"], s["losses"], s["score"], s["stderr"]) == (0, 12, 0, 0.5, 0.0)
        assert rating.sprt(draws, 0.0, 10.0, paired=paired) == {"llr": 0.0, "lower": math.log(0.05 / 0.95), "upper": math.log(0.95 / 0.05), "decision": None}
    assert rating.summary(draws, paired=True)["pairs"] == [0, 0, 6, 0, 0] and rating.elo(rating.summary(draws)["score"]) == 0.0
    split = [1.0, 0.0] * 10                                       # ten pairs, each won once by either colour: the pairs say nothing, the games look noisy
    p, u = rating.summary(split, paired=True), rating.summary(split, paired=False)
    assert p["pairs"] == [0, 0, 10, 0, 0] and p["stderr"] == 0.0 and p["score"] == u["score"] == 0.5
    assert u["stderr"] == math.sqrt(0.25 / 20) and u["pairs"] is None
    assert rating.sprt(split, 0.0, 10.0, paired=True)["llr"] == 0.0 and rating.sprt(split, 0.0, 10.0, paired=False)["llr"] != 0.0
    seven = [1.0] * 7 + [0.0] * 3                                 # 7 wins in 10, unpaired
    s = rating.summary(seven)
    assert (s["wins"], s["draws"], s["losses"], s["score"]) == (7, 0, 3, 0.7) and close(s["stderr"], math.sqrt(0.7 * 0.3 / 10))
    assert close(rating.elo(s["score"]), 400.0 * math.log10(7.0 / 3.0))
    assert rating.summary([], paired=True)["games"] == 0 and math.isnan(rating.summary([])["score"]) and rating.sprt([], 0.0, 5.0)["decision"] is None
    with pytest.raises(ValueError):
        rating.summary([1.0, 0.0, 0.5], paired=True)              # an odd number of games has no pairs
    with pytest.raises(ValueError):
        rating.summary([1.0, 0.3])


def _first_crossing(x, elo0, elo1, paired):
    """The N at which the restatement's LLR first leaves (lower, upper), and the side it leaves on"""
    per = 2 if paired else 1
    for n in range(1, len(x) // per + 1):
        r = ref_sprt(x[:per * n], elo0, elo1, 0.05, 0.05, paired)
        if r["decision"] is not None:
            return n, r["decision"]
    return None, None


@pytest.mark.parametrize("paired", [True, False])
def test_sprt_decides_at_the_known_observation(paired):
    """Scores built to cross the upper bound: a block of pairs (games) of which three in four are won and one lost.  Where the restatement
    crosses is worked out prefix by prefix; the module decides "H1" there and nothing before, and the mirrored scores decide "H0" at the same N."""
    unit = [1.0, 1.0] if paired else [1.0]
    lost = [0.0, 0.0] if paired else [0.0]
    x = (unit * 3 + lost) * 60
    per = len(unit)
    n_star, side = _first_crossing(x, 0.0, 100.0, paired)
    assert side == "H1" and n_star is not None and 4 < n_star < 200
    for n in range(1, n_star + 1):
        got = rating.sprt(x[:per * n], 0.0, 100.0, paired=paired)
        assert got["decision"] == ("H1" if n == n_star else None), n
        assert (got["llr"] >= got["upper"]) == (n == n_star)
    mirror = [1.0 - v for v in x]
    for n in range(1, n_star + 1):
        got, up = rating.sprt(mirror[:per * n], -100.0, 0.0, paired=paired), rating.sprt(x[:per * n], 0.0, 100.0, paired=paired)
        assert got["decision"] == ("H0" if n == n_star else None), n
        assert close(got["llr"], -up["llr"])                      # the mirrored hypotheses about the mirrored scores: the same evidence, signed
