"""network.load_weights without a device: the two file forms a trained network is kept in -- a torch.save'd PolicyValueNetwork.state_dict() and a
TrainingLoop.save checkpoint, whose trainer block holds the sixteen tensors under the trainer's names and shapes -- give the same module."""
import numpy as np
import pytest
import torch

from gomokuai_amd import lib as G
from gomokuai_amd.network import _MODULE_TENSORS, PolicyValueNetwork, load_weights, module_arrays


def _checkpoint(net):
    """what TrainingLoop.state_dict() keeps of a trainer whose parameters are net's (training.py), without the trainer: plain containers and tensors"""
    params = {name: torch.from_numpy(np.array(a, dtype=np.float32)) for name, a in module_arrays(net).items()}
    zeros = {name: torch.zeros_like(t) for name, t in params.items()}
    return {"total_steps": 3, "lr_multiplier": 1.5, "history": [], "config": {"batch_size": 8}, "schedule": None, "replay": {"step": 0},
            "trainer": {"step": 3, "params": params, "m": zeros, "v": dict(zeros)}}


def test_both_file_forms_give_the_same_tensors(tmp_path):
    net = PolicyValueNetwork(seed=41)
    with torch.no_grad():
        for p in net.parameters():                               # (the biases start at zero: give every tensor content)
            p.add_(torch.randn(p.shape, generator=torch.Generator().manual_seed(p.numel())) * 0.01)
    torch.save(net.state_dict(), tmp_path / "module.pt")
    torch.save(_checkpoint(net), tmp_path / "run.pt")
    shapes = dict(G.TRAIN_TENSORS)
    assert tuple(_checkpoint(net)["trainer"]["params"]["w_policy_conv"].shape) == tuple(shapes["w_policy_conv"]) != tuple(net.policy_conv.weight.shape)
    a, b = load_weights(tmp_path / "module.pt"), load_weights(str(tmp_path / "run.pt"))
    want = net.state_dict()
    for loaded in (a, b):
        assert isinstance(loaded, PolicyValueNetwork)
        got = loaded.state_dict()
        assert sorted(got) == sorted(want) == sorted(key for _, key in _MODULE_TENSORS)
        for key in want:
            assert got[key].dtype == torch.float32 and got[key].shape == want[key].shape and torch.equal(got[key], want[key]), key
    x = (torch.rand((3, 6, 15, 15), generator=torch.Generator().manual_seed(1)) > 0.7).float()
    with torch.no_grad():
        for u, w in zip(a(x), net(x)):
            assert torch.equal(u, w)


def test_other_files_are_refused(tmp_path):
    torch.save({"conv.0.weight": torch.zeros(32, 6, 3, 3)}, tmp_path / "part.pt")
    with pytest.raises(ValueError):
        load_weights(tmp_path / "part.pt")
    ck = _checkpoint(PolicyValueNetwork(seed=1))
    del ck["trainer"]["params"]["w_out"]
    torch.save(ck, tmp_path / "short.pt")
    with pytest.raises(ValueError):
        load_weights(tmp_path / "short.pt")
    import fractions
    import pickle
    with open(tmp_path / "pickle.pt", "wb") as f:
        pickle.dump(fractions.Fraction(1, 2), f, protocol=2)
    with pytest.raises(Exception):                               # weights_only=True: an arbitrary pickle is not executed
        load_weights(tmp_path / "pickle.pt")
