"""The hand-written pattern heuristic in float64, stated from the reference's own text, and a derived bound on how far a float32
evaluation of it in one fixed order may lie from that statement.

TEST INFRASTRUCTURE ONLY.  Written from core/lib/include/algorithms/Heuristic.hpp:16-45 (EvaluationProbs, EvaluationValue,
DensityWeight), :94-161 (DecisiveFilter), policies/Traditional.h:49-69 (hybridSimulate: probabilities, filter, then the value; the
filter's report is never anything but None) and Pattern.cpp:408-416 (Record::get).  It shares no float code with the three float32
restatements it judges (the kernels' heuristic_device.h, oracle/go_trad.c, tests/trad_rave_reference.py): only the INTEGER
evaluator state comes from oracle.Evaluator (scores, density words, pattern and compound flag words, the record length, the player
to move), which the K1 / K2 suites hold bit for bit.  There is no fixed summation order here: np.dot, np.linalg.norm and math.fsum.

The statement
-------------
  DW(q)   = normalized(3 W / (1 + 2 N)),  N = max(counts_q, 0), W = max(weights_q, 0)              Heuristic.hpp:39-45
  probs   = one-hot(centre)                                     on an empty record
          = normalized(c6 * scores(p,p) o DW(p) + c4 * scores(-p,p) o DW(-p))                       Heuristic.hpp:16-27
  value   = tanh((1.2 * dot(scores(p,p), DW(p)) - dot(scores(-p,-p), DW(-p))) / 500)                Heuristic.hpp:32-36
  filter  = the automaton of Heuristic.hpp:94-161 over a std::deque of (pattern, player); the first candidate with a non-zero
            total stops it; every cell where no remaining candidate has a flag is zeroed and the vector is normalised again.
normalized() / normalize() are Eigen 3.3's: x / sqrt(squaredNorm) if squaredNorm > 0, otherwise x as it is.
c6, c4: `0.6 * self_worthy` multiplies a VectorXf by a double literal; Eigen converts the literal to the vector's scalar type, so
the factors are float(0.6) and float(0.4), widened here to double.  1.2 and 500 meet a float in a double expression: doubles.

The rounding bound (u = 2^-24, round to nearest, gamma(k) = k u / (1 - k u))
--------------------------------------------------------------------------
What is bounded is the float32 path all three restatements take: every operation once in float32, sums of 225 terms as three
strided adds into 64 partial sums, a four-level tree in each group of sixteen and (g0 + g1) + (g2 + g3): no term passes through
more than 3 + 4 + 2 = 9 additions.  A product of k factors (1 + d)^(+-1), |d| <= u, is 1 + t with |t| <= gamma(k) (Higham, Accuracy
and Stability of Numerical Algorithms, lemma 3.1); "k roundings" below means such a factor.  Contracting a product and an
addition into one fused operation only removes a factor.  Integers below 2^24 convert exactly (asserted), 3 W and 1 + 2 N are
exact, products with an exact zero are exact, and nothing underflows (asserted: every non-zero magnitude that is squared lies
above 2^-60, so its square is a normal float32).

 1. x_j = 3 W_j / (1 + 2 N_j): the division, 1 rounding.  Hence also ||x^|| = ||x|| (1 + t1): a norm moves by no more, relatively,
    than its components do.
 2. normalized(x^): the squares, 1; the tree sum of NON-NEGATIVE terms, 9: squaredNorm carries 10, its square root half of that, 5
    (the square root of a number in [(1-u)^10, (1+u)^10] lies in [(1-u)^5, (1+u)^5]); sqrtf, 1; the division by the norm, 1.
    DW^_j = DW_j (1 + t), K_DW = 1 + 1 + 5 + 1 + 1 = 9 roundings, of which K_NORM = 5 + 1 + 1 = 7 belong to the normalisation.
 3. sw_j = s_j DW_j: the score product, 1: 10 roundings; the same for ra_j.
 4. t_j = c6 sw_j + c4 ra_j: each literal product 1, the sum 1: t^_j = c6 sw_j (1 + t12) + c4 ra_j (1 + t12'), K_T = 12:
        |t^_j - t_j| <= gamma(12) a_j,   a_j = c6 |sw_j| + c4 |ra_j|.
    The absolute form stays: nothing in the code promises scores >= 0.  Where they are, a_j = |t_j| and the bound is relative.
 5. the second normalisation, p = t / ||t||.  With T = ||t||, rho = gamma(12) ||a|| / T the relative movement of the norm
    (| ||t^|| - T | <= ||t^ - t|| <= gamma(12) ||a||):
        | t^_j / ||t^|| - p_j | <= (gamma(12) a_j / T + rho |p_j|) / (1 - rho) =: E_j,
    and the normalisation's own K_NORM roundings on top:
        bound_j = E_j + gamma(7) (|p_j| + E_j)
    which is the form  k u (c6 |sw_j| + c4 |ra_j|) / ||.|| + k' u |p_j|  with k = 12 and k' = 12 ||a|| / T + 7, second-order
    terms kept.  rho >= 1 (cancellation ate the vector) gives an infinite bound: nothing is claimed there.
 6. the third normalisation, after the filter: f = m o p / ||m o p||, the mask m exact.  The same step with e = m o bound in the
    place of gamma(12) a and M = ||m o p||:  rho' = ||e|| / M,
        bound'_j = E'_j + gamma(7) (|f_j| + E'_j),   E'_j = (e_j / M + rho' |f_j|) / (1 - rho').
 7. the norm of a float32 result: the last normalisation alone gives p^_j = y_j / ||y|| (1 + t7) for the vector y it was handed,
    so | ||p^|| - 1 | <= gamma(7) =: NORM_BOUND, whatever went before.
 8. the value: A = dot(s, DW) in float32 is a tree sum of the products s_j DW^_j: DW^ 9, the product 1, the additions 9:
        |A^ - A| <= gamma(19) sum_j |s_j DW_j|,
    absolute again.  (1.2 A^ - B^) / 500 and tanh run in double (a few 2^-53, covered by one 2^-50 of the argument's scale), tanh
    has Lipschitz constant 1, and the cast of the result to float32 adds u |v|:
        value_bound = gamma(19) (1.2 sum |s DW|_self + sum |s DW|_rival) / 500 + 2^-50 (1 + scale) + u |v|.
 9. the best move: with i = argmax p^ and k = argmax p,  p_i >= p^_i - bound_i >= p^_k - bound_i >= p_k - bound_k - bound_i.
    Ties need no exception.
The support needs no bound: a cell is zero in float32 exactly where it is zero here, as long as nothing underflows and no t_j
cancels to zero with a_j > 0 (then the statement's own zero is an accident of float64 too; the tests would show it)."""
import collections
import math

import numpy as np

N = 225
WHITE, BLACK = -1, 1
U = 2.0 ** -24
C6, C4 = float(np.float32(0.6)), float(np.float32(0.4))         # Eigen casts the double literal to the vector's float
K_NORM, K_DW, K_T, K_DOT = 7, 9, 12, 19
DEAD_THREE, LIVE_THREE, DEAD_FOUR, LIVE_FOUR, PATTERN_SIZE = 4, 5, 6, 7, 9      # Pattern::Type (Pattern.h:33-39)
S4, SL3, STO44, STO43, STO33, SEND = range(6)
# AutomataTable[anti][state] = (next state, next anti), Heuristic.hpp:101-105
AUTOMATA_TABLE = (((S4, 1), (STO44, 0), (SL3, 1), (STO43, 1), (STO33, 1), (SEND, 0)),
                  ((SL3, 0), (STO44, 1), (STO43, 0), (STO33, 0), (SEND, 0), (SEND, 1)))
EXIT_NAMES = ("_4", "L3", "To44", "To43", "To33", "none")


def gamma(k):
    return k * U / (1.0 - k * U)


NORM_BOUND = gamma(K_NORM)


def group1(player):                                               # Evaluator::Group(player), Pattern.h:154-156
    return int(player == BLACK)


def group2(favour, perspective):                                  # Evaluator::Group(favour, perspective), Pattern.h:159-161
    return (int(favour == BLACK) << 1) | int(perspective == BLACK)


def _exact(ints):
    assert np.abs(ints).max(initial=0) < 1 << 24                 # int -> float32 is exact
    return ints.astype(np.float64)


def _no_underflow(x):
    nz = np.abs(x[x != 0])
    assert nz.min(initial=1.0) > 2.0 ** -60 and nz.max(initial=1.0) < 2.0 ** 60


def normalized(x):
    z = float(np.linalg.norm(x))
    return x / z if z > 0.0 else x


def density_weight(density, player):
    counts, weights = density[group1(player)]
    n, w = _exact(np.maximum(counts, 0)), _exact(np.maximum(weights, 0))
    x = 3.0 * w / (1.0 + 2.0 * n)
    _no_underflow(x)
    return normalized(x)


def evaluation_probs(scores, density, nrec, player):
    """-> (probs f64[225], bound f64[225])"""
    if nrec == 0:
        probs = np.zeros(N)
        probs[(15 // 2) * 15 + 15 // 2] = 1.0
        return probs, np.zeros(N)                                # written, not computed
    sw = _exact(scores[group2(player, player)]) * density_weight(density, player)
    ra = _exact(scores[group2(-player, player)]) * density_weight(density, -player)
    t = C6 * sw + C4 * ra
    a = C6 * np.abs(sw) + C4 * np.abs(ra)
    _no_underflow(sw), _no_underflow(ra)
    return _normalise_with_bound(t, gamma(K_T) * a)


def _normalise_with_bound(y, err):
    """normalized(y) and the bound on a float32 normalisation of y^ with |y^ - y| <= err (steps 5 and 6 of the derivation)"""
    norm = float(np.linalg.norm(y))
    if norm == 0.0:
        return y, np.where(err > 0, np.inf, 0.0)
    p = y / norm
    _no_underflow(p)
    rho = float(np.linalg.norm(err)) / norm
    if rho >= 1.0:
        return p, np.full(N, np.inf)
    e = (err / norm + rho * np.abs(p)) / (1.0 - rho)
    return p, e + gamma(K_NORM) * (np.abs(p) + e)


def evaluation_value(scores, density, player):
    """-> (value, bound)"""
    ts = _exact(scores[group2(player, player)]) * density_weight(density, player)
    tr = _exact(scores[group2(-player, -player)]) * density_weight(density, -player)
    _no_underflow(ts), _no_underflow(tr)
    a, b = math.fsum(ts), math.fsum(tr)
    v = math.tanh((1.2 * a - b) / 500.0)
    scale = (1.2 * math.fsum(np.abs(ts)) + math.fsum(np.abs(tr))) / 500.0
    return v, gamma(K_DOT) * scale + 2.0 ** -50 * (1.0 + scale) + U * abs(v)


def _total(pdist, cdist, pattern, player):                       # m_patternDist.back()[pattern].get(player): the 16-bit count
    field = int(pdist[N, pattern]) if pattern < PATTERN_SIZE else int(cdist[N, pattern - PATTERN_SIZE])
    return (field >> (16 * group1(player))) & 0xFFFF


def _flags(pdist, cdist, pattern, player, cur):                  # m_patternDist[i][pattern].get(player, cur_player): 4 x 2 direction bits
    field = pdist[:N, pattern] if pattern < PATTERN_SIZE else cdist[:N, pattern % PATTERN_SIZE]
    return (field.astype(np.int64) >> (8 * group2(player, cur))) & 0xFF


def decisive_mask(pdist, cdist, cur):
    """-> (mask bool[225] or None when the automaton runs out, the state it stopped in (SEND: it ran out))"""
    candidates = collections.deque()
    state, anti = S4, False
    while state != SEND:
        player = -cur if anti else cur
        if state == S4:
            candidates.append((LIVE_FOUR, player))
            candidates.append((DEAD_FOUR, player))
        elif state == SL3:
            candidates.append((LIVE_THREE, player))
        else:
            candidates.append((PATTERN_SIZE + (STO33 - state), player))
        while candidates:
            pattern, pl = candidates[0]
            if _total(pdist, cdist, pattern, pl) != 0:
                if anti and state != S4:
                    candidates.append((DEAD_THREE, -pl))
                break
            candidates.popleft()
        if candidates:
            mask = np.zeros(N, bool)
            for pattern, pl in candidates:
                mask |= _flags(pdist, cdist, pattern, pl, cur) != 0
            return mask, state
        state, anti = AUTOMATA_TABLE[int(anti)][state]
    return None, SEND


def decisive_filter(pdist, cdist, cur, probs, bound):
    """-> (filtered probs, their bound, the exit state)"""
    mask, state = decisive_mask(pdist, cdist, cur)
    if mask is None:
        return probs, bound, state
    y = np.where(mask, probs, 0.0)
    err = np.where(mask & (probs != 0), bound, 0.0)              # a zero of the statement is a zero of float32: the mask adds no error
    p, b = _normalise_with_bound(y, err)
    return p, b, state


class Position:
    """Everything the tests compare at one live position of an oracle.Evaluator."""

    def __init__(self, ev):
        b = ev.board
        self.cur, self.nrec = int(b.cur_player), int(b.nrec)
        scores, density = ev.scores(), ev.density()
        pdist, cdist = ev.pattern_dist(), ev.compound_dist()
        self.probs, self.probs_bound = evaluation_probs(scores, density, self.nrec, self.cur)
        self.filtered, self.filtered_bound, self.exit = decisive_filter(pdist, cdist, self.cur, self.probs, self.probs_bound)
        self.value, self.value_bound = evaluation_value(scores, density, self.cur)

    def side(self, filt):
        return (self.filtered, self.filtered_bound) if filt else (self.probs, self.probs_bound)


def check(pos, filt, p32, v32, where=""):
    """The assertions of the comparison; -> (largest probability err / bound, value err / bound).  Written so that a NaN fails."""
    p64, bound = pos.side(filt)
    p32 = np.asarray(p32, np.float32).astype(np.float64)
    assert p32.shape == (N,)
    assert ((p32 != 0) == (p64 != 0)).all(), "support %s" % (where,)
    err = np.abs(p32 - p64)
    assert (err <= bound).all(), "probabilities %s: err / bound up to %g" % (where, np.nanmax(err / np.maximum(bound, 1e-300)))
    if p32.any():
        assert abs(float(np.linalg.norm(p32)) - 1.0) <= NORM_BOUND, "norm %s" % (where,)
    i32, i64 = int(np.argmax(p32)), int(np.argmax(p64))          # no position is left out: on a zero vector both are cell 0
    assert p64[i32] >= p64[i64] - bound[i32] - bound[i64], "best move %s" % (where,)
    nz = bound > 0
    margin_p = float((err[nz] / bound[nz]).max()) if nz.any() else 0.0
    margin_v = None
    if v32 is not None:
        ev = abs(float(v32) - pos.value)
        assert ev <= pos.value_bound, "value %s: err / bound %g" % (where, ev / pos.value_bound)
        margin_v = ev / pos.value_bound
    return margin_p, margin_v
