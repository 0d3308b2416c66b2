"""K23 restated in numpy: include/gomoku_pattern_states.h -- how a row of network planes float32 [6][225] becomes a canonical move list, and
how K10's vector becomes a prior.  Written from the header's comment, not from its code: sets and sorted lists where the header walks bit
masks, so that the two only agree when both say what the comment says."""
import numpy as np

N = 225
ILLEGAL = 4
NORM_L2, NORM_SUM = 0, 1
F32 = np.float32


def is_set(x):
    """a cell is set iff x != 0.0f: NaN is set, -0.0 is not"""
    x = np.asarray(x, F32)
    return ~(x == 0)


def decode(row):
    """row f32[6, 225] -> None when it is no position, else (black_to_move, black cells, white cells, last or -1, last2 or -1)"""
    row = np.asarray(row, F32).reshape(6, N)
    own, opp = set(np.flatnonzero(is_set(row[0]))), set(np.flatnonzero(is_set(row[1])))
    last, last2 = np.flatnonzero(is_set(row[3])), np.flatnonzero(is_set(row[4]))
    btm = bool(is_set(row[5, 0]))
    if own & opp:
        return None
    black, white = (own, opp) if btm else (opp, own)
    if len(black) != len(white) + (0 if btm else 1):
        return None
    if len(last) > 1 or (len(last) == 1 and last[0] not in opp):
        return None
    if len(last2) > 1 or (len(last2) == 1 and (last2[0] not in own or len(last) == 0)):
        return None
    return btm, black, white, (int(last[0]) if len(last) else -1), (int(last2[0]) if len(last2) else -1)


def canonical_list(row):
    """(status, moves): 0 and the canonical list, or ILLEGAL and []"""
    d = decode(row)
    if d is None:
        return ILLEGAL, []
    _, black, white, last, last2 = d
    T = len(black) + len(white)
    moves = [None] * T
    rest = {0: sorted(black - {last, last2}), 1: sorted(white - {last, last2})}
    if last >= 0:
        moves[T - 1] = last
    if last2 >= 0:
        moves[T - 2] = last2
    for ply in range(T):
        if moves[ply] is None:
            moves[ply] = int(rest[ply & 1].pop(0))
    assert not rest[0] and not rest[1]
    return 0, moves


def lists(rows):
    """what gmk_pattern_states_list_host writes: (moves u8[n, 225] zero past the length, lens i32[n], status i32[n])"""
    rows = np.asarray(rows, F32).reshape(-1, 6, N)
    moves, lens, status = np.zeros((len(rows), N), np.uint8), np.zeros(len(rows), np.int32), np.zeros(len(rows), np.int32)
    for i, row in enumerate(rows):
        status[i], ml = canonical_list(row)
        moves[i, :len(ml)] = ml
        lens[i] = len(ml)
    return moves, lens, status


def planes(moves, last=True, last2=True):
    """Board.encoded_states of the position after `moves` (black first): own, opp, empty, last move, the move before, colour"""
    row = np.zeros((6, N), F32)
    btm = len(moves) % 2 == 0
    for ply, c in enumerate(moves):
        black_stone = ply % 2 == 0
        row[0 if black_stone == btm else 1, c] = 1.0
    row[2] = 1.0 - row[0] - row[1]
    if last and len(moves) >= 1:
        row[3, moves[-1]] = 1.0
    if last2 and len(moves) >= 2:
        row[4, moves[-2]] = 1.0
    row[5] = 1.0 if btm else 0.0
    return row


def sum225_f64(v):
    """gmk_noise_sum225's association in binary64"""
    v = np.asarray(v, np.float64)
    p = np.zeros(64, np.float64)
    for l in range(64):
        p[l] = v[l]
        for j in range(1, 4):
            if l + 64 * j < N:
                p[l] = p[l] + v[l + 64 * j]
    for off in (8, 4, 2, 1):
        q = p.copy()
        for l in range(64):
            q[l] = p[l] + (p[l + off] if (l & 15) + off < 16 else 0.0)
        p = q
    return (p[0] + p[16]) + (p[32] + p[48])


def finish(v, row, norm, live=None):
    """K10's vector f32[225] of `row` -> the prior f32[225].  live None: the row decodes (what the host form takes for it)"""
    v = np.asarray(v, F32)
    d = decode(row)
    if live is None:
        live = d is not None
    if not live:
        return np.zeros(N, F32)
    if norm == NORM_L2:
        return v.copy()
    s = sum225_f64(v.astype(np.float64))
    if s == 0.0:
        _, black, white, _, _ = d
        out = np.zeros(N, F32)
        empty = sorted(set(range(N)) - black - white)
        if empty:
            out[empty] = F32(1.0 / float(len(empty)))
        return out
    with np.errstate(all="ignore"):
        return (v.astype(np.float64) / s).astype(F32)
