"""What a match's scores say: score statistics, Elo differences and a sequential test (host only: numpy and math, no GPU, no torch).

The scores are those of selfplay.play_agent_match and selfplay.play_evaluation_games: per game 1 for a win of the first agent, 0.5 for a
tie, 0 for a loss.  In a paired match the games 2p and 2p + 1 start from the same opening with the colours exchanged, so their scores are
not independent: the unit of observation is the pair, and its mean y_p = (s_2p + s_2p+1) / 2 takes one of five values (the "pentanomial"
of engine testing).  All arithmetic is float64; every docstring states its formula in full, so that a test can restate it.
"""
import math

import numpy as np

_PAIR_VALUES = (0.0, 0.25, 0.5, 0.75, 1.0)


def _scores(scores):
    s = np.asarray(scores, dtype=np.float64).reshape(-1)
    if not np.isin(s, (0.0, 0.5, 1.0)).all():
        raise ValueError("rating: a score is 1 (win), 0.5 (tie) or 0 (loss)")
    return s


def _observations(scores, paired):
    """x_i: the pair means (s_2p + s_2p+1) / 2 of a paired match (an even number of games), else the game scores"""
    s = _scores(scores)
    if not paired:
        return s
    if s.shape[0] % 2:
        raise ValueError("rating: a paired match has an even number of games")
    return (s[0::2] + s[1::2]) / 2.0


def summary(scores, paired=False):
    """The first agent's results: {"games" n, "wins", "draws", "losses" (counts of 1, 0.5, 0), "score" = sum(s) / n, "stderr", "pairs"}.
    Unpaired: stderr = sqrt(var(s) / n) with the population variance var(s) = sum((s_i - score)^2) / n over the games; "pairs" is None.
    Paired (n even): with y_p = (s_2p + s_2p+1) / 2 and P = n / 2 pairs, stderr = sqrt(var(y) / P), var(y) = sum((y_p - score)^2) / P -- the
    mean of the y_p is the score -- and "pairs" = the five counts of y_p = 0, 0.25, 0.5, 0.75, 1.
    No games: score and stderr are nan."""
    s = _scores(scores)
    x = _observations(s, paired)
    n = int(s.shape[0])
    out = {"games": n, "wins": int((s == 1.0).sum()), "draws": int((s == 0.5).sum()), "losses": int((s == 0.0).sum()),
           "score": float(s.sum() / n) if n else math.nan, "stderr": math.nan,
           "pairs": [int((x == v).sum()) for v in _PAIR_VALUES] if paired else None}
    if n:
        out["stderr"] = math.sqrt(float(((x - out["score"]) ** 2).sum() / x.shape[0]) / x.shape[0])
    return out


def elo(score):
    """The rating difference at which the logistic model expects `score`: -400 log10(1 / score - 1); -inf at 0, +inf at 1."""
    score = float(score)
    if not 0.0 <= score <= 1.0:
        raise ValueError("rating.elo: a score lies in [0, 1]")
    if score == 0.0:
        return -math.inf
    if score == 1.0:
        return math.inf
    return -400.0 * math.log10(1.0 / score - 1.0)


def elo_interval(mean, stderr, z=1.96):
    """(elo(lo), elo(mean), elo(hi)) with lo = max(mean - z stderr, 0) and hi = min(mean + z stderr, 1): the normal interval of the score,
    clipped to [0, 1] and mapped through elo (an end at 0 or 1 maps to -inf or +inf)."""
    mean, stderr, z = float(mean), float(stderr), float(z)
    return elo(max(mean - z * stderr, 0.0)), elo(min(max(mean, 0.0), 1.0)), elo(min(mean + z * stderr, 1.0))


def expected_score(elo_difference):
    """s = 1 / (1 + 10^(-elo / 400)): elo()'s inverse"""
    return 1.0 / (1.0 + 10.0 ** (-float(elo_difference) / 400.0))


def sprt(scores, elo0, elo1, alpha=0.05, beta=0.05, paired=True):
    """The generalised sequential probability ratio test of H0: elo = elo0 against H1: elo = elo1 (elo0 < elo1) in its normal form.
    Observations x_i (N of them): the pair means when paired, the game scores otherwise; s_k = 1 / (1 + 10^(-elo_k / 400));
    mean = sum(x) / N, var = sum((x_i - mean)^2) / N (population variance);
        LLR = N (s1 - s0) (2 mean - s0 - s1) / (2 var),        LLR = 0 while var = 0 (or N = 0);
    bounds lower = ln(beta / (1 - alpha)) and upper = ln((1 - beta) / alpha).
    Returns {"llr", "lower", "upper", "decision"}: "H1" once llr >= upper, "H0" once llr <= lower, else None."""
    x = _observations(scores, paired)
    s0, s1 = expected_score(elo0), expected_score(elo1)
    lower, upper = math.log(beta / (1.0 - alpha)), math.log((1.0 - beta) / alpha)
    n = int(x.shape[0])
    llr = 0.0
    if n:
        mean = float(x.sum() / n)
        var = float(((x - mean) ** 2).sum() / n)
        if var > 0.0:
            llr = n * (s1 - s0) * (2.0 * mean - s0 - s1) / (2.0 * var)
    return {"llr": llr, "lower": lower, "upper": upper, "decision": "H1" if llr >= upper else "H0" if llr <= lower else None}
