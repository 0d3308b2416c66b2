"""The replay buffer's image on the device (gmk_replay_snapshot / gmk_replay_restore, ReplayBuffer.state_dict / load_state_dict): the
snapshot of wrapped rings byte for byte against the numpy restatement of the format, restores into other capacities that draw and evict
as the source does, refusals that change nothing, the empty image, side streams and poisoned pool blocks."""
import numpy as np
import pytest
import torch

from gomokuai_amd import lib as G
from gomokuai_amd import selfplay
from test_replay_gpu import Mirror, _bits_equal, _check_draw, _synth
from test_replay_image import build_image

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEED = 17


@pytest.fixture(autouse=True, scope="module")
def _device():
    G.init(0)


def _stats(buf):
    s = buf.stats()
    return {k: s[k] for k in ("games", "plies", "population", "evicted_games")}


def _mirror_image(mirror):
    """The image of what a Mirror holds, from the records it was fed."""
    games = []
    for h in mirror.held:
        rec, g, length, first = h["src"].rec, h["game"], h["len"], h["first"]
        games.append((length, first, int(rec.winner[g]), rec.moves[g, :length].cpu().numpy(), rec.visits[g, first:length].cpu().numpy()))
    return build_image(games, head=mirror.stats()["evicted_games"])


def _copy_mirror(mirror, capacity_plies, max_games):
    m = Mirror(capacity_plies, max_games)
    m.tail, m.held, m.sources = mirror.tail, list(mirror.held), list(mirror.sources)
    return m


APPENDS = (([40, 0, 225, 3, 60], 0), ([9, 225, 1, 100], 4), ([150, 30, 225], 0))


@pytest.fixture(scope="module")
def wrapped():
    """Capacity 700, max_games 12, three appends: the third evicts seven games and its first game straddles the end of both rings."""
    buf = selfplay.ReplayBuffer(700, max_games=12, seed=SEED)
    mirror = Mirror(700, 12)
    for i, (lens, fm) in enumerate(APPENDS):
        rec = _synth(len(lens), 300 + i, lens=lens)
        buf.extend(rec, first_move=fm)
        mirror.append(rec, fm)
    assert buf.status()[0] == 0
    # checked by hand against the eviction rule; the 150-ply game starts at stored ply 663 and sampled ply 650 of rings of 700
    assert _stats(buf) == mirror.stats() == {"games": 5, "plies": 506, "population": 501, "evicted_games": 7}
    assert [h["len"] for h in mirror.held] == [1, 100, 150, 30, 225]
    state = buf.state_dict()
    yield buf, mirror, state
    buf.close()


def test_snapshot_is_the_documented_image(wrapped):
    buf, mirror, state = wrapped
    image = state["image"]
    assert image.dtype == torch.uint8 and image.device.type == "cpu" and image.numel() == 64 + 40 + 512 + 225456 == buf._h.image_bytes()
    assert np.array_equal(image.numpy(), _mirror_image(mirror))
    assert G.replay_image_check_host(image.numpy()) == {"games": 5, "plies": 506, "population": 501, "head": 7}
    assert (state["seed"], state["step"], state["capacity_plies"], state["max_games"]) == (SEED, buf._step, 700, 12)
    assert _stats(buf) == mirror.stats()                                          # the handle did not change
    assert torch.equal(buf.state_dict()["image"], image)


@pytest.mark.parametrize("cap,max_games", [(700, 12), (506, 5), (2000, 50)])
def test_restore_draws_as_the_source(wrapped, cap, max_games):
    src, mirror, state = wrapped
    buf = selfplay.ReplayBuffer.from_state_dict(state, capacity_plies=cap, max_games=max_games)
    assert (buf.capacity_plies, buf.max_games, buf.seed, buf._step) == (cap, max_games, SEED, state["step"])
    assert _stats(buf) == _stats(src)
    for step in (0, 1, 7):
        for augment in (True, False):
            M = 501 * (8 if augment else 1)
            _check_draw(buf, mirror, 64, step, augment)
            _check_draw(buf, mirror, M, step, augment, float_too=False)
    assert torch.equal(buf.state_dict()["image"], state["image"])
    buf.close()


def test_default_sizes_are_the_saved_ones(wrapped):
    _, _, state = wrapped
    buf = selfplay.ReplayBuffer.from_state_dict(state)
    assert (buf.capacity_plies, buf.max_games) == (700, 12) and _stats(buf)["evicted_games"] == 7
    buf.close()


def test_a_later_append_evicts_the_same_games(wrapped):
    _, mirror0, state = wrapped
    copy = selfplay.ReplayBuffer.from_state_dict(state)
    source = selfplay.ReplayBuffer(700, max_games=12, seed=SEED)                  # (the fixture's own buffer stays as it is for the other tests)
    for i, (lens, fm) in enumerate(APPENDS):
        source.extend(_synth(len(lens), 300 + i, lens=lens), first_move=fm)
    big = selfplay.ReplayBuffer.from_state_dict(state, capacity_plies=2000, max_games=50)
    mirror, big_mirror = _copy_mirror(mirror0, 700, 12), _copy_mirror(mirror0, 2000, 50)
    rec = _synth(2, 310, lens=[225, 50])
    for b in (source, copy, big):
        b.extend(rec, first_move=2)
        assert b.status()[0] == 0
    mirror.append(rec, 2)
    big_mirror.append(rec, 2)
    assert [h["len"] for h in mirror.held] == [150, 30, 225, 225, 50]             # the 1- and 100-ply games left
    assert _stats(source) == _stats(copy) == mirror.stats() == {"games": 5, "plies": 680, "population": 676, "evicted_games": 9}
    assert _stats(big) == big_mirror.stats() == {"games": 7, "plies": 781, "population": 772, "evicted_games": 7}
    for step, augment, batch in ((0, True, 64), (3, False, 676), (3, True, 8 * 676)):
        x = source.sample(batch, step=step, augment=augment, return_picked=True)
        y = copy.sample(batch, step=step, augment=augment, return_picked=True)
        assert all(_bits_equal(p, q) for p, q in zip(x, y))
        _check_draw(copy, mirror, batch, step, augment, float_too=False)
    assert torch.equal(source.state_dict()["image"], copy.state_dict()["image"])
    _check_draw(big, big_mirror, 64, 2, True)
    _check_draw(big, big_mirror, 772, 2, False, float_too=False)
    for b in (source, copy, big):
        b.close()


def _other(cap, max_games):
    """A buffer that holds other games, with what it says and draws now."""
    buf = selfplay.ReplayBuffer(cap, max_games=max_games, seed=SEED)
    buf.extend(_synth(3, 320, lens=[20, 30, 40]), first_move=1)
    return buf, _stats(buf), buf.sample(87, step=2, augment=False, return_picked=True), buf.state_dict()["image"]


def _unchanged(buf, stats, draw, image):
    return _stats(buf) == stats and all(_bits_equal(p, q) for p, q in zip(buf.sample(87, step=2, augment=False, return_picked=True), draw)) \
        and torch.equal(buf.state_dict()["image"], image)


def test_refused_restores_change_nothing(wrapped):
    _, _, state = wrapped
    good = state["image"]
    stream = torch.cuda.current_stream().cuda_stream
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    for cap, max_games in ((505, 12), (700, 4)):
        buf, *before = _other(cap, max_games)
        with pytest.raises(ValueError, match="do not fit"):
            buf.load_state_dict(state)
        assert _unchanged(buf, *before)
        d = good.to(DEV)
        buf._h.restore(d.data_ptr(), d.numel(), status.data_ptr(), stream)
        assert int(status.item()) == G.REPLAY_NO_ROOM and _unchanged(buf, *before)
        buf.close()

    def flipped_magic(img):
        img[3] ^= 0x20

    def long_game(img):
        img[64 + 8 * 2: 64 + 8 * 2 + 2] = torch.tensor([226, 0], dtype=torch.uint8)

    def more_samples(img):
        img[24:32] = torch.from_numpy(np.array([502], dtype="<u8").view(np.uint8).copy())

    buf, *before = _other(700, 12)
    for damage in (flipped_magic, long_game, more_samples):
        bad = good.clone()
        damage(bad)
        with pytest.raises(ValueError):
            G.replay_image_check_host(bad.numpy())
        with pytest.raises(ValueError):
            buf.load_state_dict(dict(state, image=bad))
        assert _unchanged(buf, *before)
        d = bad.to(DEV)                                                           # past the Python check, straight to the handle
        status.fill_(-1)
        buf._h.restore(d.data_ptr(), d.numel(), status.data_ptr(), stream)
        assert int(status.item()) == G.REPLAY_BAD_IMAGE and _unchanged(buf, *before)
    with pytest.raises(ValueError, match="seed"):
        buf.load_state_dict(dict(state, seed=SEED + 1))
    assert _unchanged(buf, *before) and buf._step == 0
    d = good.to(DEV)
    L = G.load()
    assert L.gmk_replay_restore(buf._h.h, d.data_ptr(), 63, status.data_ptr(), None) == -3
    assert L.gmk_replay_restore(buf._h.h, d.data_ptr() + 4, d.numel() - 8, status.data_ptr(), None) == -3           # misaligned image
    assert L.gmk_replay_restore(buf._h.h, None, d.numel(), status.data_ptr(), None) == -3
    assert L.gmk_replay_restore(buf._h.h, d.data_ptr(), d.numel(), None, None) == -3
    assert L.gmk_replay_snapshot(buf._h.h, d.data_ptr(), -1, status.data_ptr(), None) == -3
    assert L.gmk_replay_snapshot(buf._h.h, d.data_ptr() + 1, d.numel() - 1, status.data_ptr(), None) == -3
    assert L.gmk_replay_image_bytes(None, None, None) == -3
    assert _unchanged(buf, *before)
    buf.close()


def test_short_snapshot_writes_nothing(wrapped):
    buf, _, state = wrapped
    size = state["image"].numel()
    dst = torch.full((size,), 0xA5, dtype=torch.uint8, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    buf._h.snapshot(dst.data_ptr(), size - 1, status.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert int(status.item()) == G.REPLAY_NO_ROOM and bool((dst == 0xA5).all())
    buf._h.snapshot(dst.data_ptr(), size, status.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert int(status.item()) == 0 and torch.equal(dst.cpu(), state["image"])


def test_empty_image():
    empty = selfplay.ReplayBuffer(700, max_games=12, seed=SEED)
    state = empty.state_dict()
    assert state["image"].numel() == 64 and np.array_equal(state["image"].numpy(), build_image([]))
    buf, *_ = _other(700, 12)
    buf.load_state_dict(state)
    assert _stats(buf) == {"games": 0, "plies": 0, "population": 0, "evicted_games": 0}
    # an empty image with a head: the buffer is empty and goes on counting from there
    buf.extend(_synth(2, 330, lens=[5, 6]))
    buf.load_state_dict(dict(state, image=torch.from_numpy(build_image([], head=5))))
    assert _stats(buf) == {"games": 0, "plies": 0, "population": 0, "evicted_games": 5}
    assert np.array_equal(buf.state_dict()["image"].numpy(), build_image([], head=5))
    rec = _synth(2, 331, lens=[12, 9])
    mirror = Mirror(700, 12)
    mirror.tail = 5
    buf.extend(rec)
    mirror.append(rec, 0)
    assert _stats(buf) == mirror.stats() == {"games": 2, "plies": 21, "population": 21, "evicted_games": 5}
    picked = _check_draw(buf, mirror, 21, 0, False).cpu().numpy()
    assert set(picked[:, 0].tolist()) == {5, 6}
    empty.close()
    buf.close()


def test_side_stream_and_poisoned_pool():
    rec = selfplay.play_games(6, 30, seed=5, first_game_id=0)
    cap = 40000                                                           # 18 MB of visit rows: a block of the library's pool
    ref = selfplay.ReplayBuffer(cap, max_games=64, seed=13)
    mirror = Mirror(cap, 64)
    ref.extend(rec, first_move=1)
    mirror.append(rec, 1)
    want = ref.sample(256, step=4, return_picked=True)
    state = ref.state_dict()
    torch.cuda.synchronize()
    ref.close()
    G.pool_poison(True)
    try:
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            buf = selfplay.ReplayBuffer.from_state_dict(state)           # the block ref gave back, filled with 0xA5
            got = buf.sample(256, step=4, return_picked=True)
            _check_draw(buf, mirror, 256, 5, True)
            again = buf.state_dict()
        side.synchronize()
        assert all(_bits_equal(x, y) for x, y in zip(want, got))
        assert torch.equal(again["image"], state["image"])
        buf.close()
    finally:
        G.pool_poison(False)
