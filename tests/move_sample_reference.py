"""The move-sampling rule of self-play ("K20") restated in Python integers, from the rule's text alone: its own Philox4x32-10, its own
weights, prefix sums and greedy fall-back.  Nothing here calls the library; tests/test_move_sample.py and tests/test_az_sample_gpu.py hold the
host form and the kernels to it."""

M32 = 0xFFFFFFFF
SAMPLE_TAG = int.from_bytes(b"samp", "big")                      # 0x73616d70
PROOF_WINS, PROOF_LOSES = 1, 2


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): counter and result are four words, key two."""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def draw(seed, game_id, stones):
    """r: the first two words of the block of (game id, stones, 'samp', 0) under the seed, low word first"""
    out = philox4x32_10((game_id & M32, stones & M32, SAMPLE_TAG, 0), (seed & M32, (seed >> 32) & M32))
    return out[0] | out[1] << 32


def greedy(visits, proofs=None):
    """today's choice from rows by cell: the first LOSES child; else the most visited child that is not WINS and has a visit; else the most
    visited child; first maximum in cell order; -1 without one"""
    if proofs is not None:
        for c, p in enumerate(proofs):
            if p == PROOF_LOSES:
                return c
        top = max((v for v, p in zip(visits, proofs) if p != PROOF_WINS), default=0)
        if top > 0:
            return next(c for c, (v, p) in enumerate(zip(visits, proofs)) if p != PROOF_WINS and v == top)
    top = max(visits)
    return list(visits).index(top) if top > 0 else -1


def choose(visits, stones, game_id, plies, power, seed, proofs=None):
    """the cell a root plays; visits (and proofs) are rows by cell of 225 integers"""
    visits = visits.tolist() if hasattr(visits, "tolist") else [int(v) for v in visits]
    proofs = None if proofs is None else (proofs.tolist() if hasattr(proofs, "tolist") else [int(p) for p in proofs])
    if plies == 0 or stones >= plies:
        return greedy(visits, proofs)
    if proofs is not None and PROOF_LOSES in proofs:
        return proofs.index(PROOF_LOSES)
    weights = [min(v, 65535) ** power for v in visits]
    if proofs is not None:
        weights = [0 if p == PROOF_WINS else w for w, p in zip(weights, proofs)]
    total = sum(weights)
    if total == 0:
        return greedy(visits, proofs)
    target = (draw(seed, game_id, stones) * total) >> 64
    prefix = 0
    for c, w in enumerate(weights):
        prefix += w
        if prefix > target:
            return c
    raise AssertionError("target < total")
