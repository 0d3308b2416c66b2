"""The wire form of game records on the device (records_wire.hip, gmk_samples_from_packed) against the torch reference in selfplay.py:
pack byte for byte, unpack into uncleared rows, training tuples bit for bit, errors that leave memory untouched, side streams."""
import ctypes as C

import pytest
import torch

from gomokuai_amd import lib as G
from gomokuai_amd import selfplay

pytestmark = pytest.mark.gpu

N = 225
DEV = "cuda"


@pytest.fixture(autouse=True, scope="module")
def _device():
    G.init(0)


def _synth(n, seed, visits=True, lens=None):
    """Fixed-stride records with garbage past every length (pack must not read it): moves a permutation of the cells per game."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    if lens is None:
        lens = torch.randint(0, N + 1, (n,), generator=g, device=DEV, dtype=torch.int32)
        edge = torch.tensor([0, 1, 224, 225], dtype=torch.int32, device=DEV)
        lens[: min(n, 4)] = edge[: min(n, 4)]
        if n > 8:
            lens[n // 2: n // 2 + 4] = edge.flip(0)
    else:
        lens = torch.as_tensor(lens, dtype=torch.int32, device=DEV)
    moves = torch.argsort(torch.rand((n, N), generator=g, device=DEV), dim=1).to(torch.uint8)
    winner = torch.randint(-1, 2, (n,), generator=g, device=DEV, dtype=torch.int8)
    vis = torch.randint(-32768, 32768, (n, N, N), generator=g, device=DEV, dtype=torch.int16) if visits else None
    return selfplay.GameRecords(moves, lens, winner, vis)


def _unpack_into_ff(buf, n, has_visits, n_bytes=None):
    """gmk_records_unpack into rows pre-filled with 0xFF -> (moves, lens, winner, visits, status)."""
    moves = torch.full((n, N), 0xFF, dtype=torch.uint8, device=DEV)
    lens = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    winner = torch.full((n,), -1, dtype=torch.int8, device=DEV)
    visits = torch.full((n, N, N), -1, dtype=torch.int16, device=DEV) if has_visits else None
    offsets = torch.empty(n + 1, dtype=torch.int64, device=DEV)
    status = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    G.records_unpack(buf.data_ptr(), buf.numel() if n_bytes is None else n_bytes, n, has_visits, offsets.data_ptr(), moves.data_ptr(),
                     lens.data_ptr(), winner.data_ptr(), None if visits is None else visits.data_ptr(), status.data_ptr(),
                     torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return moves, lens, winner, visits, int(status.item())


def _masked(rec):
    """The source records with every byte past a game's length zeroed (what an unpack must give back)."""
    played = torch.arange(N, device=DEV)[None, :] < rec.lens[:, None]
    moves = torch.where(played, rec.moves, torch.zeros_like(rec.moves))
    vis = None if rec.visits is None else torch.where(played[:, :, None], rec.visits, torch.zeros_like(rec.visits))
    return moves, vis


def _check_roundtrip(rec, buf, has_visits):
    n = len(rec)
    moves, lens, winner, visits, status = _unpack_into_ff(buf, n, has_visits)
    assert status == 0
    ref = selfplay.unpack_records(buf, n, has_visits)
    m_src, v_src = _masked(rec)
    assert torch.equal(lens, rec.lens) and torch.equal(lens, ref.lens)
    assert torch.equal(winner, rec.winner) and torch.equal(winner, ref.winner)
    assert torch.equal(moves, m_src) and torch.equal(moves, ref.moves)
    if has_visits:
        assert torch.equal(visits, v_src) and torch.equal(visits, ref.visits)
    dev = selfplay.unpack_records_device(buf, n, has_visits)
    assert torch.equal(dev.moves, ref.moves) and torch.equal(dev.lens, ref.lens) and torch.equal(dev.winner, ref.winner)
    assert (dev.visits is None) == (not has_visits)
    if has_visits:
        assert torch.equal(dev.visits, ref.visits)


def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def test_pack_unpack_real_games():
    rec = selfplay.play_games(6, 30, seed=5, first_game_id=0)
    buf = selfplay.pack_records_device(rec)
    assert torch.equal(buf, selfplay.pack_records(rec))
    _check_roundtrip(rec, buf, True)
    for augment in (False, True):
        ref = rec.to_samples(augment=augment)
        got = selfplay.samples_from_packed(buf, len(rec), augment=augment)
        assert all(_bits_equal(a, b) for a, b in zip(got, ref))


@pytest.mark.parametrize("has_visits", [True, False])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097, 32768])
def test_pack_matches_torch(n, has_visits):
    rec = _synth(n, seed=n, visits=has_visits)
    buf = selfplay.pack_records_device(rec)
    ref = selfplay.pack_records(rec)
    assert buf.numel() == ref.numel() and torch.equal(buf, ref)
    _check_roundtrip(rec, buf, has_visits)


@pytest.mark.parametrize("parity", [0, 1])
def test_both_parities_of_the_visit_section(parity):
    n = 65
    rec = _synth(n, seed=11)
    if (5 * n + int(rec.lens.sum())) % 2 != parity:
        rec.lens[5] = rec.lens[5] + (1 if int(rec.lens[5]) < N else -1)
    assert (5 * n + int(rec.lens.sum())) % 2 == parity
    buf = selfplay.pack_records_device(rec)
    assert torch.equal(buf, selfplay.pack_records(rec))
    _check_roundtrip(rec, buf, True)
    got = selfplay.samples_from_packed(buf, n, augment=True, first_move=2)
    ref = selfplay.unpack_records(buf, n, True).to_samples(augment=True, first_move=2)
    assert all(_bits_equal(a, b) for a, b in zip(got, ref))


@pytest.mark.parametrize("augment", [False, True])
@pytest.mark.parametrize("first_move", [0, 5])
def test_samples_from_packed_bit_equal(augment, first_move):
    n = 37
    rec = _synth(n, seed=3 + first_move)
    buf = selfplay.pack_records(rec)
    ref = selfplay.unpack_records(buf, n, True).to_samples(augment=augment, first_move=first_move)
    got = selfplay.samples_from_packed(buf, n, augment=augment, first_move=first_move)
    assert got[0].shape[0] == ref[0].shape[0] > 0
    assert all(_bits_equal(a, b) for a, b in zip(got, ref))


@pytest.mark.parametrize("augment", [False, True])
def test_samples_hand_picked(augment):
    lens = [225, 0, 1, 224, 17, 225, 2]
    rec = _synth(len(lens), seed=21, lens=lens)
    n = len(lens)
    buf = selfplay.pack_records(rec)
    pairs = [(0, 224), (0, 0), (2, 0), (3, 223), (5, 224), (5, 1), (4, 16), (6, 1), (0, 15), (0, 14)]
    game = torch.tensor([p[0] for p in pairs], dtype=torch.int32, device=DEV)
    move = torch.tensor([p[1] for p in pairs], dtype=torch.int32, device=DEV)
    s, copies = len(pairs), 8 if augment else 1

    def outs():
        return (torch.empty((s * copies, 6, 15, 15), dtype=torch.uint8, device=DEV), torch.empty(s * copies, dtype=torch.float32, device=DEV),
                torch.empty((s * copies, N), dtype=torch.float32, device=DEV))
    stream = torch.cuda.current_stream().cuda_stream
    ref = outs()
    up = selfplay.unpack_records(buf, n, True)
    G.samples_from_records(up.moves.data_ptr(), up.lens.data_ptr(), up.visits.data_ptr(), up.winner.data_ptr(), game.data_ptr(), move.data_ptr(),
                           s, augment, *(t.data_ptr() for t in ref), stream)
    offsets = torch.empty(n + 1, dtype=torch.int64, device=DEV)
    G.records_scan(buf.data_ptr(), n, offsets.data_ptr(), stream)
    got = outs()
    G.samples_from_packed(buf.data_ptr(), n, offsets.data_ptr(), game.data_ptr(), move.data_ptr(), s, augment, *(t.data_ptr() for t in got), stream)
    torch.cuda.synchronize()
    assert all(_bits_equal(a, b) for a, b in zip(got, ref))


def test_scan_large():
    n = 262144 + 123
    g = torch.Generator(device=DEV).manual_seed(9)
    lens = torch.randint(0, N + 1, (n,), generator=g, device=DEV, dtype=torch.int32)
    offsets = torch.full((n + 1,), -7, dtype=torch.int64, device=DEV)
    G.records_scan(lens.data_ptr(), n, offsets.data_ptr(), torch.cuda.current_stream().cuda_stream)
    ref = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    ref[1:] = torch.cumsum(lens.to(torch.int64), 0)
    assert torch.equal(offsets, ref)
    assert G.records_packed_bytes(offsets.data_ptr(), n, True) == 5 * n + int(ref[-1]) * 451
    assert G.records_packed_bytes(offsets.data_ptr(), n, False) == 5 * n + int(ref[-1])


@pytest.mark.parametrize("bad", [-1, 226])
def test_bad_length(bad):
    n = 70
    rec = _synth(n, seed=4)
    good = selfplay.pack_records(rec)
    stream = torch.cuda.current_stream().cuda_stream
    # scan + packed_bytes: GMK_ERR_ARG
    lens = rec.lens.clone()
    lens[40] = bad
    offsets = torch.empty(n + 1, dtype=torch.int64, device=DEV)
    G.records_scan(lens.data_ptr(), n, offsets.data_ptr(), stream)
    b = C.c_uint64(0)
    assert G.load().gmk_records_packed_bytes(offsets.data_ptr(), n, 1, C.byref(b), stream) == -3
    assert b"outside [0, 225]" in G.load().gmk_last_error()
    # pack with that scan: status, nothing written
    out = torch.full((good.numel() + 64,), 0x5A, dtype=torch.uint8, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    G.records_pack(rec.moves.data_ptr(), lens.data_ptr(), rec.winner.data_ptr(), rec.visits.data_ptr(), n, offsets.data_ptr(), out.data_ptr(),
                   out.numel(), status.data_ptr(), stream)
    torch.cuda.synchronize()
    assert int(status.item()) == G.WIRE_BAD_LENGTH and bool((out == 0x5A).all())
    with pytest.raises(G.GmkError):
        selfplay.pack_records_device(selfplay.GameRecords(rec.moves, lens, rec.winner, rec.visits))
    # unpack of a block that carries it: status, records untouched
    buf = good.clone()
    buf[4 * 40: 4 * 41] = torch.tensor([bad], dtype=torch.int32).view(torch.uint8).to(DEV)
    moves, lens_o, winner, visits, st = _unpack_into_ff(buf, n, True)
    assert st == G.WIRE_BAD_LENGTH
    assert bool((moves == 0xFF).all()) and bool((lens_o == -1).all()) and bool((winner == -1).all()) and bool((visits == -1).all())
    with pytest.raises(ValueError):
        selfplay.unpack_records_device(buf, n, True)


def test_sizes_and_guard_bytes():
    n = 65
    rec = _synth(n, seed=8)
    good = selfplay.pack_records(rec)
    size = good.numel()
    stream = torch.cuda.current_stream().cuda_stream
    offsets = torch.empty(n + 1, dtype=torch.int64, device=DEV)
    G.records_scan(rec.lens.data_ptr(), n, offsets.data_ptr(), stream)
    assert G.records_packed_bytes(offsets.data_ptr(), n, True, stream) == size
    out = torch.full((size + 64,), 0x5A, dtype=torch.uint8, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    args = (rec.moves.data_ptr(), rec.lens.data_ptr(), rec.winner.data_ptr(), rec.visits.data_ptr(), n, offsets.data_ptr(), out.data_ptr())
    G.records_pack(*args, size - 1, status.data_ptr(), stream)                 # one byte short
    torch.cuda.synchronize()
    assert int(status.item()) == G.WIRE_BAD_SIZE and bool((out == 0x5A).all())
    G.records_pack(*args, size, status.data_ptr(), stream)
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    assert torch.equal(out[:size], good) and bool((out[size:] == 0x5A).all())
    # unpack: a block one byte longer or shorter than its lengths say is refused, records untouched
    for n_bytes in (size + 1, size - 1):
        moves, lens, winner, visits, st = _unpack_into_ff(out, n, True, n_bytes=n_bytes)
        assert st == G.WIRE_BAD_SIZE
        assert bool((moves == 0xFF).all()) and bool((lens == -1).all()) and bool((visits == -1).all())
    with pytest.raises(ValueError):
        selfplay.unpack_records_device(out, n, True)
    with pytest.raises(ValueError):
        selfplay.unpack_records_device(good, n, False)


def test_n_zero_is_a_no_op():
    L = G.load()
    b = C.c_uint64(99)
    assert L.gmk_records_scan(None, 0, None, None) == 0
    assert L.gmk_records_packed_bytes(None, 0, 1, C.byref(b), None) == 0 and b.value == 0
    assert L.gmk_records_pack(None, None, None, None, 0, None, None, 0, None, None) == 0
    assert L.gmk_records_unpack(None, 0, 0, 1, None, None, None, None, None, None, None) == 0
    assert L.gmk_samples_from_packed(None, 0, None, None, None, 0, 0, None, None, None, None) == 0
    empty = selfplay.GameRecords(torch.zeros((0, N), dtype=torch.uint8, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV),
                                 torch.zeros(0, dtype=torch.int8, device=DEV), torch.zeros((0, N, N), dtype=torch.int16, device=DEV))
    buf = selfplay.pack_records_device(empty)
    assert buf.numel() == 0
    assert len(selfplay.unpack_records_device(buf, 0, True)) == 0
    assert selfplay.samples_from_packed(buf, 0)[0].shape == (0, 6, 15, 15)


def test_side_stream():
    """Records made, packed, unpacked and turned into tuples on a non-default stream, with no device-wide synchronise in between."""
    n = 4097
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        rec = _synth(n, seed=77)
        buf = selfplay.pack_records_device(rec)
        up = selfplay.unpack_records_device(buf, n, True)
        got = selfplay.samples_from_packed(buf, n, augment=False, first_move=1)
    side.synchronize()
    torch.cuda.synchronize()
    ref_buf = selfplay.pack_records(rec)
    assert torch.equal(buf, ref_buf)
    ref = selfplay.unpack_records(ref_buf, n, True)
    assert torch.equal(up.moves, ref.moves) and torch.equal(up.lens, ref.lens) and torch.equal(up.winner, ref.winner)
    assert torch.equal(up.visits, ref.visits)
    ref_s = ref.to_samples(augment=False, first_move=1)
    assert all(_bits_equal(a, b) for a, b in zip(got, ref_s))
