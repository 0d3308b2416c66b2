"""Float64 restatement of the policy target pi (MCTS::evalState, core/lib/src/MCTS.cpp:104-117, with Stats::TempBasedProbs,
core/lib/include/algorithms/Statistical.hpp:37-42) and an element-wise rounding bound for a float32 implementation of it.

TEST INFRASTRUCTURE ONLY.  It shares no code with the product or with oracle/.

    pi = softmax(log(v / |v|_2 + [v != 0] + eps) / tau),   tau = 1 below 15 stones, float32(0.01) from 15 on,   elements <= eps set to 0

with eps = float32 epsilon.  The reference computes the logits in float32 and the softmax (exp, sum, division) in double; so do the five
copies in this repository.  pi64() is the whole formula in float64; the cut is applied to the float64 value.

THE BOUND on |p32_i - p64_i| (bound()).  Write u = 2^-24, q_i = z_i / tau for the exponent of cell i, and let d be the largest absolute
error of any computed q_i.  Then e32_i / e64_i and sum32 / sum64 both lie in [e^-d, e^d], so p32_i / p64_i lies in [e^-2d, e^2d], and

    |p32_i - p64_i| <= p_i (e^2d - 1) + 2^-24 p_i + 2^-40 p_i

where the second term is the final rounding to float32 and the third stands for double's exp, its 225-term sum and its division.
A relative error of "k ulp" is at most 2 k u.  d is the maximum over the cells of the following chain (all first-order terms kept whole):

  1. S = sum v^2 in float32.  Counts are integers, so every partial sum is an integer, and a product or partial sum below 2^24 is EXACT:
     a row whose sum of squares stays below 2^24 (counts up to 4 095 in one cell, 272 in all 225) has no error here, whatever the order.
     Above that, a product or an addition with two non-zero operands costs at most half an ulp of its result.  These are added up along the
     two associations the copies use -- records_kernel.hip's tree over 256 slots (slot[i] += slot[i + w], w = 128 .. 1, depth 8) and the
     sequential sum of the host copy and the oracle -- and the WORSE of the two is taken as eS, relative to S: the host copy is held to
     the same bound.
  2. x = v / sqrtf(S): relative error ex = (1 + 2 DIV_ULPS u) / (sqrt(1 - eS) (1 - 2 SQRT_ULPS u)) - 1.
  3. y = (x + 1) + eps: each rounding is at most u (2 u once the result reaches 2): dy = x ex + u + u.
  4. z = logf(y): dz = dy / (y - dy) + 2 LOGF_ULPS u (|z| + dy / (y - dy)).
  5. q = z / tau: dq = (dz + 2 DIV_ULPS u (|z| + dz)) / tau.  At tau = 0.01 the division's own rounding, |z / tau| times a few u, and the
     100-fold dz are what the bound is made of.

A cell without visits is treated separately: y = eps is an exact input, and z = logf(eps) = -15.94 is held to 1 ulp of its output, 2^-20.
Cells whose exponent is below -700 even with its error (the unvisited cells at tau = 0.01, q = -1594) contribute less than 1e-300 to either
sum and take no part in d.  A row without any visit at tau = 0.01 is 0 / 0 in every implementation: it fails `> eps` and is all zeros,
exactly (bound 0); below 15 stones the same row is uniform, 1 / 225.

ASSUMPTIONS.  gomokuai_amd/build.py compiles with -O3 -ffp-contract=off and without any fast-math switch; the compiler's help names the
switch for correctly rounded float32 divide and sqrt in device code but not its default, and the ROCm installation carries no accuracy
table for logf.  So, as assumptions and not as documented facts: LOGF_ULPS = 2, SQRT_ULPS = DIV_ULPS = 2.5.  The host copy and the oracle
(correctly rounded sqrt and division, a libm logf below 1 ulp) are inside the same bound a fortiori.

THE CUT.  An element whose p64 lies within its own bound of eps is exempt: it may be 0 or the value.  Every other element must match the
reference exactly on this point: p64 > eps gives a non-zero output (within the bound), p64 <= eps gives exactly 0.0f.

Also here: the row classes the tests draw from (ROW_CLASSES, row()), the game records every device path is run on (RECORDS), a float32
emulation of the formula in numpy with either association (emulate32()) and its wrong variants (MISTAKES)."""
import functools

import numpy as np

N = 225
U = 2.0 ** -24                          # unit roundoff of float32
EPS = float(np.finfo(np.float32).eps)   # Eigen::NumTraits<float>::epsilon()
TAU_LATE = float(np.float32(0.01))      # `float temperature` given 1e-2
LATE = 15                               # stones from which tau = 0.01 (MCTS.cpp:114)
LOGF_ULPS = 2.0                         # assumed (see above)
SQRT_ULPS = 2.5                         # assumed
DIV_ULPS = 2.5                          # assumed
F64_TERMS = 2.0 ** -40                  # double's exp, sum of 225 and division, relative
DEAD = -700.0                           # exponents below this contribute < 1e-300
LIMIT = 1.0                             # do-not-exceed fraction of the bound


def _rel(ulps):
    return 2.0 * ulps * U


def _tau(stones):
    return np.where(np.asarray(stones) < LATE, 1.0, TAU_LATE)[:, None]


def _as_rows(visits, stones):
    v = np.asarray(visits)
    assert v.dtype in (np.uint16, np.uint32) and v.shape[-1] == N, (v.dtype, v.shape)
    v = v.reshape(-1, N).astype(np.float64)
    s = np.broadcast_to(np.asarray(stones, np.int64).reshape(-1), (v.shape[0],))
    return v, s


# ---------------- the formula in float64 ----------------
def pi64(visits, stones, cut=True):
    """visits uint16/uint32 [..., 225], stones int [...] or scalar -> float64 [R, 225].  cut=False: the softmax before `> eps`
    (NaN on a row that is 0 / 0)."""
    v, stones = _as_rows(visits, stones)
    norm = np.sqrt((v * v).sum(1, keepdims=True))
    with np.errstate(invalid="ignore", divide="ignore"):
        x = np.where(norm > 0, v / norm, v)                      # VectorXf::normalized(): a zero vector stays
        x = np.where(x != 0, x + 1.0, x)                         # MCTS.cpp:112
        e = np.exp(np.log(x + EPS) / _tau(stones))               # Statistical.hpp:38, 18
        p = e / e.sum(1, keepdims=True)                          # Statistical.hpp:19
        return np.where(p > EPS, p, 0.0) if cut else p           # Statistical.hpp:39-41 (NaN > eps is false)


# ---------------- the bound ----------------
def _half_ulp32(x):
    """Half a float32 ulp at x (1 + 2^-14): x's own rounding errors (at most 225 u) cannot move it to a binade this misses."""
    _, e = np.frexp(x * (1.0 + 2.0 ** -14))
    return np.ldexp(1.0, e - 25)                                  # x in [2^(e-1), 2^e): ulp 2^(e-24)


def _add_error(a, b):
    s = a + b
    return np.where((a != 0) & (b != 0) & (s >= 2.0 ** 24), _half_ulp32(s), 0.0), s


def sum_error(v):
    """Relative error bound of the float32 sum of squares of float64 integer rows v [R, 225]: the worse of the tree and the sequential sum."""
    sq = v * v
    mul = np.where(sq >= 2.0 ** 24, _half_ulp32(sq), 0.0).sum(1)
    part = np.cumsum(sq, 1)
    seq = mul + _add_error(part[:, :-1], sq[:, 1:])[0].sum(1)
    slots = np.zeros((v.shape[0], 256))
    slots[:, :N] = sq
    tree = mul.copy()
    w = 128
    while w > 0:
        err, slots = _add_error(slots[:, :w], slots[:, w:2 * w])
        tree += err.sum(1)
        w >>= 1
    total = sq.sum(1)
    assert np.array_equal(slots[:, 0], total)
    return np.divide(np.maximum(seq, tree), total, out=np.zeros_like(total), where=total > 0) * (1.0 + 2.0 ** -14)


def exponent_error(visits, stones):
    """(q float64 [R, 225], dq [R, 225]): the exponents z / tau and the bound on a float32 implementation's error in each."""
    v, stones = _as_rows(visits, stones)
    tau = _tau(stones)
    total = (v * v).sum(1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        x = np.where(total > 0, v / np.sqrt(total), 0.0)
    e_sum = sum_error(v)[:, None]
    ex = (1.0 + _rel(DIV_ULPS)) / (np.sqrt(1.0 - e_sum) * (1.0 - _rel(SQRT_ULPS))) - 1.0
    y = x + 1.0 + EPS
    dy = x * ex + U + np.where(y >= 2.0 - 8 * U, 2 * U, U)
    z = np.log(y)
    dlog = dy / (y - dy)
    dz = dlog + _rel(LOGF_ULPS) * (np.abs(z) + dlog)
    z0, dz0 = np.log(EPS), 2.0 ** -20                             # a cell without visits: logf of an exact eps, 1 ulp in [8, 16)
    z = np.where(v > 0, z, z0)
    dz = np.where(v > 0, dz, dz0)
    return z / tau, (dz + _rel(DIV_ULPS) * (np.abs(z) + dz)) / tau


def bound(p64, visits, stones):
    """Element-wise bound on |p32 - p64| for p64 = pi64(visits, stones, cut=False).  0 on a row that is 0 / 0."""
    q, dq = exponent_error(visits, stones)
    live = q + dq > DEAD
    d = np.where(live, dq, 0.0).max(1, keepdims=True)
    p = np.asarray(p64, np.float64).reshape(q.shape)
    b = p * np.expm1(2.0 * d) + (U + F64_TERMS) * p + 1e-300
    return np.where(live.any(1, keepdims=True), b, 0.0)


def reference(visits, stones, cls=None):
    """Everything check() needs about rows of visits: {"pi" (cut), "raw" (uncut), "bound", "exempt", "visits", "stones", "cls"}."""
    v, s = _as_rows(visits, stones)
    raw = pi64(visits, stones, cut=False)
    b = bound(raw, visits, stones)
    dead = np.isnan(raw).any(1)
    assert np.array_equal(dead, (v.sum(1) == 0) & (s >= LATE))    # 0 / 0 happens on rows without visits from 15 stones on, nowhere else
    raw = np.where(dead[:, None], 0.0, raw)
    cls = np.broadcast_to(np.asarray("" if cls is None else cls), (v.shape[0],)).copy()
    return {"pi": np.where(raw > EPS, raw, 0.0), "raw": raw, "bound": b, "exempt": (np.abs(raw - EPS) <= b) & ~dead[:, None],
            "visits": v.astype(np.uint32), "stones": s.copy(), "cls": cls}


def take(ref, rows):
    return {k: a[rows] for k, a in ref.items()}


def symmetry_perms():
    """int [8, 225]: copy a of the augmentation (network/data_helper.py:36-55: rot90^i, then its left-right mirror) shows source cell
    perms[a][j] at cell j."""
    grid = np.arange(N).reshape(15, 15)
    out = []
    for turns in range(4):
        g = np.rot90(grid, turns)
        out += [g.reshape(-1), np.fliplr(g).reshape(-1)]
    return np.stack(out)


def augmented(ref, perms):
    """The reference of the eight-fold augmented samples, ordered (sample, symmetry); perms int [8, 225] as symmetry_perms()."""
    perms = np.asarray(perms, np.int64)
    assert perms.shape == (8, N) and all(np.array_equal(np.sort(p), np.arange(N)) for p in perms)
    return {k: (a[:, perms].reshape(-1, N) if a.ndim == 2 else np.repeat(a, 8)) for k, a in ref.items()}


# ---------------- comparing ----------------
def ratios(ref, got):
    """|got - ref| / bound per element, the cut included: inf for a NaN, for any value where exactly 0 is due, and for a 0 where a
    value is due; an exempt element may be 0 or within the bound of the uncut value."""
    g = np.asarray(got, np.float64)
    assert g.shape == ref["pi"].shape, (g.shape, ref["pi"].shape)
    raw, b, exempt = ref["raw"], ref["bound"], ref["exempt"]
    zero_due = ~exempt & (raw <= EPS)
    err = np.where(np.isfinite(g), np.abs(g - np.where(zero_due, 0.0, raw)), np.inf)
    err = np.where(exempt & (g == 0), 0.0, err)
    err = np.where(~exempt & (raw > EPS) & (g == 0), np.inf, err)
    tol = np.where(zero_due, 0.0, b)
    return np.divide(err, tol, out=np.where(err == 0, 0.0, np.inf), where=tol > 0)


def check(ref, got, what=""):
    """Asserts the bound and the cut on every element; returns the worst ratio of error to bound."""
    q = ratios(ref, got)
    worst = float(q.max()) if q.size else 0.0
    if not worst <= LIMIT:
        r, c = np.unravel_index(int(np.argmax(q)), q.shape)
        raise AssertionError("%s: error / bound = %g at row %d (class %s, %d stones) cell %d: got %r, float64 %r (uncut %r), bound %g, visits %d"
                             % (what, worst, r, ref["cls"][r], ref["stones"][r], c, float(np.asarray(got)[r, c]), ref["pi"][r, c],
                                ref["raw"][r, c], ref["bound"][r, c], ref["visits"][r, c]))
    return worst


def check_by_class(ref, got, what=""):
    """check() per row class -> {class: worst ratio}"""
    got = np.asarray(got)
    out = {}
    for name in sorted(set(ref["cls"].tolist())):
        rows = np.nonzero(ref["cls"] == name)[0]
        out[name] = check(take(ref, rows), got[rows], "%s / %s" % (what, name))
    return out


def rejects(ref, got):
    """The classes on which check() refuses `got`."""
    q = ratios(ref, got).max(1)
    return sorted(set(ref["cls"][~(q <= LIMIT)].tolist()))


def show(what, worst):
    print("%s: worst error / bound per class: %s" % (what, ", ".join("%s %.3f" % (k, v) for k, v in sorted(worst.items()))))


def not_vacuous(ref):
    """The comparison exercises what it claims to: both temperatures, elements removed by the cut next to kept ones, and an exempt band
    that hides nothing -- at most 1 % of the elements, never one of a row's two largest, never all visited elements of a class."""
    stones, raw, exempt = ref["stones"], ref["raw"], ref["exempt"]
    assert (stones < LATE).any() and (stones >= LATE).any()
    assert ((raw > 0) & (raw <= EPS)).any() and (raw > EPS).any()
    assert exempt.mean() <= 0.01, exempt.mean()
    second = np.sort(raw, 1)[:, -2][:, None]
    assert not (exempt & (raw >= second) & (raw > 0)).any()
    visited = ref["visits"] > 0
    for name in sorted(set(ref["cls"].tolist())):
        rows = ref["cls"] == name
        if visited[rows].any():
            assert (visited[rows] & ~exempt[rows]).any(), name


# ---------------- row classes ----------------
def _small(rng):
    v = np.zeros(N, np.int64)
    v[rng.choice(N, 120, replace=False)] = rng.randint(0, 60, 120)
    return v


def _playouts_800(rng):
    v = np.zeros(N, np.int64)
    cells = rng.choice(N, rng.randint(30, 121), replace=False)
    v[cells] = rng.multinomial(800, rng.dirichlet(np.full(len(cells), 0.3)))
    return v


def _kept_subtree(rng):
    v = np.zeros(N, np.int64)
    cells = rng.choice(N, rng.randint(20, 101), replace=False)
    v[cells] = rng.randint(0, 200, len(cells))
    k = rng.randint(1, 3)
    v[cells[:k]] = rng.randint(5000, 30001, k)
    return v


def _two_large_close(rng):
    v = np.zeros(N, np.int64)
    cells = rng.choice(N, rng.randint(2, 41), replace=False)
    v[cells] = rng.randint(0, 300, len(cells))
    a = rng.randint(20000, 65536 - 30)
    v[cells[0]], v[cells[1]] = a, a + rng.randint(1, 31)
    return v


def _flat_4096(rng):
    return rng.randint(4090, 4103, N)


def _uint16_edges(rng):
    return rng.choice(np.array([0, 1, 32767, 32768, 65535]), N)


def _all_65535(rng):
    return np.full(N, 65535)


def _one_cell(rng):
    v = np.zeros(N, np.int64)
    v[rng.randint(N)] = rng.choice([1, 7, 4095, 4097, 40000, 65535])
    return v


def _tied_max(rng):
    v = np.zeros(N, np.int64)
    cells = rng.choice(N, rng.randint(6, 61), replace=False)
    top = int(rng.choice([9, 700, 5001, 40000]))
    v[cells] = rng.randint(0, top, len(cells))
    v[cells[:rng.randint(2, 5)]] = top
    return v


def _all_zero(rng):
    return np.zeros(N, np.int64)


def _ramp(rng):
    """every count from 1 to 225 once: all cells visited, probabilities on both sides of the cut at tau = 0.01"""
    return rng.permutation(N) + 1


ROW_CLASSES = {"small": _small, "playouts_800": _playouts_800, "kept_subtree": _kept_subtree, "two_large_close": _two_large_close,
               "flat_4096": _flat_4096, "uint16_edges": _uint16_edges, "all_65535": _all_65535, "one_cell": _one_cell,
               "tied_max": _tied_max, "all_zero": _all_zero, "ramp": _ramp}
CLASS_NAMES = tuple(ROW_CLASSES)


def row(kind, seed):
    """uint16[225] of one class; the same (kind, seed) gives the same row."""
    v = ROW_CLASSES[kind](np.random.RandomState([CLASS_NAMES.index(kind), seed]))
    assert v.shape == (N,) and v.min() >= 0 and v.max() <= 65535
    return v.astype(np.uint16)


def rows(kind, n, seed=0):
    return np.stack([row(kind, seed * 1000 + i) for i in range(n)])


# ---------------- the game records the device paths run on ----------------
GAME_LENS = (1, 16, 17, 225, 224, 40)


def _build_records():
    """Six games: plies 0, 1, 13, 14, 15, 16 and 224 are all sampled.  Ply t of game g takes class (t + 4 g) mod 11, so neighbouring plies of
    a game never share a class and every class sits on both sides of t = 15.  Past a game's length the rows are garbage that must not be read."""
    n = len(GAME_LENS)
    rng = np.random.RandomState(2024)
    moves = np.stack([rng.permutation(N) for _ in range(n)]).astype(np.uint8)
    winner = np.array([1, -1, 0, 1, -1, 0], np.int8)
    visits = rng.randint(0, 65536, (n, N, N)).astype(np.uint16)
    cls = np.full((n, N), "", dtype="U16")
    for g, length in enumerate(GAME_LENS):
        for t in range(length):
            cls[g, t] = CLASS_NAMES[(t + 4 * g) % len(CLASS_NAMES)]
            visits[g, t] = row(cls[g, t], 100000 + 1000 * g + t)
    return {"moves": moves, "lens": np.array(GAME_LENS, np.int32), "winner": winner, "visits": visits, "cls": cls}


RECORDS = _build_records()


def sample_lists(records=RECORDS, first_move=0):
    """(game, ply) of every sample in (game, ply) order"""
    game = np.concatenate([np.full(max(int(l) - first_move, 0), g, np.int64) for g, l in enumerate(records["lens"])])
    ply = np.concatenate([np.arange(first_move, int(l), dtype=np.int64) for l in records["lens"]])
    return game, ply


@functools.lru_cache(maxsize=None)
def records_reference():
    """reference() of every sample of RECORDS in (game, ply) order; computed once, shared, never written to."""
    game, ply = sample_lists()
    ref = reference(RECORDS["visits"][game, ply], ply, RECORDS["cls"][game, ply])
    for a in ref.values():
        a.setflags(write=False)
    return ref


# ---------------- float32 emulation, right and wrong ----------------
MISTAKES = {
    "counts_as_int16": {"signed": True},
    "switch_at_t<=15": {"late": 16},
    "switch_at_t<14": {"late": 14},
    "tau_1_everywhere": {"late": 1 << 30},
    "plus_1_on_every_cell": {"plus": "all"},
    "plus_1_on_no_cell": {"plus": "none"},
    "l1_normalisation": {"norm": "l1"},
    "cut_left_out": {"cut": False},
}


def _sum32(a, order):
    if order == "seq":
        s = np.zeros(a.shape[0], np.float32)
        for k in range(a.shape[1]):
            s = s + a[:, k]
        return s
    assert order == "tree", order
    slots = np.zeros((a.shape[0], 256), a.dtype)
    slots[:, :a.shape[1]] = a
    w = 128
    while w > 0:
        slots = slots[:, :w] + slots[:, w:2 * w]
        w >>= 1
    return slots[:, 0]


def emulate32(visits, stones, order="tree", signed=False, late=LATE, plus="visited", norm="l2", cut=True):
    """The formula as the copies compute it: float32 up to the exponent (numpy's float32 arithmetic is correctly rounded; logf is float64's
    log rounded once), double from exp on.  order: "tree" = records_kernel.hip's association of the sum of squares, "seq" = the host's.
    The other arguments switch on one mistake each (MISTAKES)."""
    v = np.asarray(visits)
    v = v.reshape(-1, N)
    stones = np.broadcast_to(np.asarray(stones, np.int64).reshape(-1), (v.shape[0],))
    f = (v.astype(np.uint16).view(np.int16) if signed else v).astype(np.float32)
    eps = np.float32(EPS)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if norm == "l1":
            nrm = _sum32(np.abs(f), order)[:, None]
        else:
            nrm = np.sqrt(_sum32(f * f, order))[:, None]
        x = np.where(nrm > 0, f / nrm, f).astype(np.float32)
        one = np.float32(1)
        x = {"visited": np.where(x != 0, x + one, x), "all": x + one, "none": x}[plus].astype(np.float32)
        z = np.log((x + eps).astype(np.float64)).astype(np.float32)
        tau = np.where(stones < late, np.float32(1), np.float32(0.01)).astype(np.float32)[:, None]
        e = np.exp((z / tau).astype(np.float64))
        total = _sum32(e, "tree") if order == "tree" else e.cumsum(1)[:, -1]
        p = (e / total[:, None]).astype(np.float32)
        return np.where(p > eps, p, np.float32(0)) if cut else np.where(np.isnan(p), np.float32(0), p)
