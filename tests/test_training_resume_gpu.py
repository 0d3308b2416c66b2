"""Checkpoint and resume of the training loop (TrainingLoop.save / load): a run that stops after two steps, is rebuilt from the file in new
objects and goes on, against a run that never stopped -- trainer, counters, history, the buffer's next draw and the exported network
bit for bit; with games appended (and evicted) after the restore; config mismatches and a truncated file."""
import numpy as np
import pytest
import torch

from gomokuai_amd import lib as G
from gomokuai_amd import selfplay
from gomokuai_amd.network import FusedPolicyValueNetwork, PolicyValueNetwork, Trainer
from gomokuai_amd.training import TrainingLoop
from test_replay_gpu import _bits_equal, _synth

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(autouse=True, scope="module")
def _device():
    G.init(0)


def _records(seed, lens):
    rec = _synth(len(lens), seed, lens=lens)
    rec.visits = rec.visits & 0x7FFF                                              # visit counts are not negative
    return rec


def _loop(net_seed, fill=True, **kw):
    net = PolicyValueNetwork(seed=net_seed).to(DEV)
    fused, trainer = FusedPolicyValueNetwork(net), Trainer(net, max_batch=16)
    replay = selfplay.ReplayBuffer(2000, seed=5)
    if fill:
        replay.extend(_records(400, [60, 80, 100, 120, 90, 70]), first_move=1)
    return TrainingLoop(replay, trainer, fused, **{"batch_size": 16, "num_epoches": 2, "export_every": 1, **kw})


def _close(loop):
    loop.replay.close()
    loop.trainer.close()


def _trainer_equal(a, b):
    sa, sb = a.trainer.state_dict(), b.trainer.state_dict()
    assert sa["step"] == sb["step"] == a.trainer.steps
    for key in ("params", "m", "v"):
        assert sorted(sa[key]) == sorted(sb[key])
        for name in sa[key]:
            x, y = np.ascontiguousarray(sa[key][name]), np.ascontiguousarray(sb[key][name])
            assert x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32)), (key, name)


def _runs_equal(a, b):
    _trainer_equal(a, b)
    assert (a.total_steps, a.lr_multiplier) == (b.total_steps, b.lr_multiplier) and a.history == b.history
    assert a.replay.stats() == b.replay.stats() and a.replay._step == b.replay._step
    x = a.replay.sample(16, return_picked=True)                                   # the buffer's next draw
    y = b.replay.sample(16, return_picked=True)
    assert all(_bits_equal(p, q) for p, q in zip(x, y))
    (va, pa), (vb, pb) = a.fused(x[0]), b.fused(y[0])                             # the exported network on 16 drawn states
    assert _bits_equal(va, vb) and _bits_equal(pa, pb)


def test_resumed_steps_are_the_uninterrupted_ones(tmp_path):
    a = _loop(0)
    for _ in range(4):
        a.step()
    b = _loop(0)
    for _ in range(2):
        b.step()
    path = tmp_path / "ck.pt"
    b.save(path)
    assert [p.name for p in tmp_path.iterdir()] == ["ck.pt"]                      # the temporary file is gone
    _close(b)
    c = _loop(1, fill=False)                                                      # everything new: another network, an empty buffer
    c.load(path)
    assert c.total_steps == 2 and len(c.history) == 2 and c.trainer.steps > 0
    for _ in range(2):
        c.step()
    assert a.total_steps == 4 and len(a.history) == 4
    _runs_equal(a, c)
    state = torch.load(path, weights_only=True)                                   # plain containers and tensors only
    assert sorted(state) == ["config", "history", "lr_multiplier", "replay", "schedule", "total_steps", "trainer"] and state["schedule"] is None
    _close(a)
    _close(c)


def test_resume_with_games_played_after_the_restore(tmp_path):
    def play_for(loop):
        return lambda: _records(500 + loop.total_steps, [200, 180, 150])          # a resumable play: made from loop.total_steps

    a = _loop(0)
    assert len(a.run(5, play=play_for(a))) == 5
    b = _loop(0)
    b.run(2, play=play_for(b))
    b.save(tmp_path / "ck.pt")
    _close(b)
    c = _loop(1, fill=False)
    c.load(tmp_path / "ck.pt")
    before = c.replay.stats()["evicted_games"]
    c.run(3, play=play_for(c))
    assert c.replay.stats()["evicted_games"] > before                             # appends and evictions happened after the restore
    _runs_equal(a, c)
    _close(a)
    _close(c)


def test_config_mismatch_names_the_key():
    a = _loop(0)
    a.step()
    state = a.state_dict()
    b = _loop(1, batch_size=8)
    before = b.trainer.state_dict()
    with pytest.raises(ValueError, match="batch_size"):
        b.load_state_dict(state)
    assert b.total_steps == 0 and b.history == [] and b.trainer.steps == 0
    assert all(np.array_equal(before["params"][k], v) for k, v in b.trainer.state_dict()["params"].items())
    c = _loop(1, kl_target=0.05, num_epoches=3)
    with pytest.raises(ValueError, match="kl_target.*num_epoches"):
        c.load_state_dict(state)
    for loop in (a, b, c):
        _close(loop)


def test_truncated_file_leaves_the_loop_as_it_was(tmp_path):
    a = _loop(0)
    a.step()
    path = tmp_path / "ck.pt"
    a.save(path)
    a.step()
    data = path.read_bytes()
    path.write_bytes(data[: len(data) // 2])
    twin = _loop(0)
    twin.step()
    twin.step()
    with pytest.raises(Exception):
        a.load(path)
    _runs_equal(a, twin)
    _close(a)
    _close(twin)
