"""PolicyValueNetwork in PyTorch-ROCm: the architecture of the reference's TF1 graph (network/model_tf.py:28-66), for
inference at the leaves of the network-guided search (K7, lib.AlphaZeroMCTS: FusedPolicyValueNetwork, K9) and for training on
the device (Trainer, K11: the loss, the optimiser and the multi-pass train_step of model_tf.py:73-135 as HIP kernels).
Weights are randomly initialised like `tf.global_variables_initializer()` does when no checkpoint exists
(model_tf.py:165-172: glorot-uniform kernels, zero biases), or loaded from a state dict.

    inputs   float32 [B, 6, 15, 15]   Board.encoded_states() (core/py_ext/src/game_ext.hpp:87-104)
    shared   conv3x3 'same' + ReLU: 6 -> 32 -> 64 -> 128
    policy   conv1x1 -> 4 + ReLU, flatten, dense 225, softmax
    value    conv1x1 -> 2 + ReLU, flatten, dense 64 + ReLU, dense 1, tanh
The TF graph runs channels-last and flattens (h, w, c); this module keeps NCHW tensors and permutes before the dense
layers, so a TF checkpoint's dense kernels can be loaded without reordering.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F


class PolicyValueNetwork(nn.Module):
    def __init__(self, seed=0):
        super().__init__()
        self.conv = nn.ModuleList([nn.Conv2d(6, 32, 3, padding=1), nn.Conv2d(32, 64, 3, padding=1), nn.Conv2d(64, 128, 3, padding=1)])
        self.policy_conv = nn.Conv2d(128, 4, 1)
        self.policy_dense = nn.Linear(4 * 225, 225)
        self.value_conv = nn.Conv2d(128, 2, 1)
        self.value_hidden = nn.Linear(2 * 225, 64)
        self.value_out = nn.Linear(64, 1)
        gen = torch.Generator().manual_seed(seed)
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                fan_out = m.weight.shape[0] * (m.weight[0][0].numel() if m.weight.dim() == 4 else 1)
                fan_in = m.weight.shape[1] * (m.weight[0][0].numel() if m.weight.dim() == 4 else 1)
                limit = float(np.sqrt(6.0 / (fan_in + fan_out)))                        # glorot_uniform, TF's default
                with torch.no_grad():
                    m.weight.copy_((torch.rand(m.weight.shape, generator=gen) * 2 - 1) * limit)
                    m.bias.zero_()

    def forward(self, states):
        """states float32 [B, 6, 15, 15] -> (value [B], probs [B, 225])."""
        x = states
        for conv in self.conv:
            x = F.relu(conv(x))
        p = F.relu(self.policy_conv(x)).permute(0, 2, 3, 1).reshape(x.shape[0], -1)     # tf.layers.flatten of an NHWC tensor
        probs = F.softmax(self.policy_dense(p), dim=1)
        v = F.relu(self.value_conv(x)).permute(0, 2, 3, 1).reshape(x.shape[0], -1)
        value = torch.tanh(self.value_out(F.relu(self.value_hidden(v)))).reshape(-1)
        return value, probs

    @torch.no_grad()
    def eval_state(self, board):
        """PolicyValueNetwork.eval_state (model_tf.py:136-145): one position -> (value, probs[225]) on the host."""
        dev = next(self.parameters()).device
        states = torch.from_numpy(np.asarray(board.encoded_states(), dtype=np.float32)[None]).to(dev)
        value, probs = self(states)
        return float(value[0]), probs[0].cpu().numpy()


class FusedPolicyValueNetwork:
    """The same function as PolicyValueNetwork.forward in two HIP kernels on the f32 matrix cores (gmk_pvnet_evaluate): the convolutions (99 % of
    the arithmetic) as ONE fused kernel whose activations never leave LDS (K9), and the three dense layers with softmax / tanh as a second one.
    float32 throughout; sums run in a different order than MIOpen's / rocBLAS's, so outputs agree with the module's to rounding
    (tests/test_pvnet_gpu.py: 2e-5), not bit for bit.  Takes the weights of `net` at construction.

    precision="bf16" runs the convolutions on the bf16 matrix cores instead ("K9 in bf16", include/gomoku_hip.h: weights, inputs and
    activations rounded to bf16, float32 accumulation, the dense layers unchanged): faster, and within the rounding bound of
    tests/pvnet_bf16_reference.py of the float64 network rather than float32's.  set_precision() switches an existing handle either way."""

    def __init__(self, net, precision="f32"):
        import ctypes as C
        from . import lib as G
        if precision not in G.PVNET_PRECISIONS:
            raise ValueError("FusedPolicyValueNetwork: precision must be one of %s, not %r" % (sorted(G.PVNET_PRECISIONS), precision))
        G.init()
        self.net, self.G, self.h = net, G, C.c_void_p()
        host = lambda t: np.ascontiguousarray(t.detach().float().cpu().numpy())
        arrays = [host(net.conv[0].weight), host(net.conv[0].bias), host(net.conv[1].weight), host(net.conv[1].bias),
                  host(net.conv[2].weight), host(net.conv[2].bias), host(net.policy_conv.weight).reshape(4, 128), host(net.policy_conv.bias),
                  host(net.value_conv.weight).reshape(2, 128), host(net.value_conv.bias)]
        arrays = [np.ascontiguousarray(a) for a in arrays]
        G._check(G.load().gmk_pvnet_create(*[a.ctypes.data for a in arrays], C.byref(self.h)))
        dense = [host(net.policy_dense.weight), host(net.policy_dense.bias), host(net.value_hidden.weight), host(net.value_hidden.bias),
                 host(net.value_out.weight).reshape(64)]
        assert dense[0].shape == (225, 900) and dense[2].shape == (64, 450)
        G._check(G.load().gmk_pvnet_set_dense(self.h, *[a.ctypes.data for a in dense], float(net.value_out.bias.detach().cpu().reshape(-1)[0])))
        if precision != "f32":
            self.set_precision(precision)

    @property
    def precision(self):
        """"f32" or "bf16": what the handle's trunk runs in (gmk_pvnet_get_precision)"""
        import ctypes as C
        out = C.c_int(0)
        self.G._check(self.G.load().gmk_pvnet_get_precision(self.h, C.byref(out)))
        return {v: k for k, v in self.G.PVNET_PRECISIONS.items()}[out.value]

    def set_precision(self, precision):
        """Switches the trunk between "f32" and "bf16" (gmk_pvnet_set_precision: blocking, packs the bf16 weights from the handle's current ones;
        not while a call on this network is in flight on another stream)."""
        if precision not in self.G.PVNET_PRECISIONS:
            raise ValueError("FusedPolicyValueNetwork: precision must be one of %s, not %r" % (sorted(self.G.PVNET_PRECISIONS), precision))
        self.G._check(self.G.load().gmk_pvnet_set_precision(self.h, self.G.PVNET_PRECISIONS[precision]))
        return self

    def close(self):
        if getattr(self, "h", None) and getattr(self, "G", None) is not None and self.G.load is not None:
            self.G.load().gmk_pvnet_destroy(self.h)
            self.h = None

    __del__ = close

    def load_from(self, trainer):
        """Takes the weights a Trainer holds now (gmk_train_export: one repack kernel on the current stream, no trip through the host).  `self.net`
        keeps the weights it had: call trainer.sync_to(self.net) as well where dense_reference() or the module itself is used afterwards."""
        trainer.export(self)
        return self

    @torch.no_grad()
    def trunk(self, states):
        """states float32 [B, 6, 15, 15] on the GPU -> (relu(policy conv) [B, 900], relu(value conv) [B, 450]), flattened (pixel, channel)."""
        assert states.is_cuda and states.dtype == torch.float32 and states.is_contiguous() and tuple(states.shape[1:]) == (6, 15, 15)
        n = states.shape[0]
        pflat = torch.empty((n, 900), dtype=torch.float32, device=states.device)
        vflat = torch.empty((n, 450), dtype=torch.float32, device=states.device)
        self.G._check(self.G.load().gmk_pvnet_forward(self.h, states.data_ptr(), n, pflat.data_ptr(), vflat.data_ptr(),
                                                      torch.cuda.current_stream(states.device).cuda_stream))
        return pflat, vflat

    @torch.no_grad()
    def __call__(self, states):
        """states float32 [B, 6, 15, 15] on the GPU -> (value [B], probs [B, 225]); both kernels go to torch's current stream."""
        assert states.is_cuda and states.dtype == torch.float32 and states.is_contiguous() and tuple(states.shape[1:]) == (6, 15, 15)
        n = states.shape[0]
        value = torch.empty((n,), dtype=torch.float32, device=states.device)
        probs = torch.empty((n, 225), dtype=torch.float32, device=states.device)
        self.G._check(self.G.load().gmk_pvnet_evaluate(self.h, states.data_ptr(), n, value.data_ptr(), probs.data_ptr(),
                                                       torch.cuda.current_stream(states.device).cuda_stream))
        return value, probs

    def symmetric(self, mode, seed=None):
        """This network evaluated over the board's symmetries (gmk_pvnet_evaluate_sym, K22) -> a SymmetricNetwork with this network's __call__
        and eval_state.  mode "all": the average over the eight orientations; "random": one orientation per position, picked from the position's
        content and `seed` (default lib.DEFAULT_SEED); "none": this network's own outputs.  An unknown mode is a ValueError."""
        return SymmetricNetwork(self, mode, seed)

    @torch.no_grad()
    def dense_reference(self, states):
        """The dense layers through PyTorch on the kernel's trunk outputs (what __call__ did before the second kernel existed): a check, not a path."""
        pflat, vflat = self.trunk(states)
        probs = F.softmax(self.net.policy_dense(pflat), dim=1)
        value = torch.tanh(self.net.value_out(F.relu(self.net.value_hidden(vflat)))).reshape(-1)
        return value, probs

    @torch.no_grad()
    def eval_state(self, board):
        """PolicyValueNetwork.eval_state (model_tf.py:136-145) through the fused kernel: one position -> (value, probs[225]) on the
        host; what MCTS(policy=Policy(eval_state=network.eval_state, c_puct)) -- the reference's PyConvNetAgent, agents/alphazero.py:5-9 -- calls once per playout."""
        dev = next(self.net.parameters()).device
        states = torch.from_numpy(np.asarray(board.encoded_states(), dtype=np.float32)[None]).to(dev)
        value, probs = self(states)
        return float(value[0]), probs[0].cpu().numpy()


class SymmetricNetwork:
    """FusedPolicyValueNetwork.symmetric(mode, seed): the callable every self-play and match loop takes, network(states) -> (value, probs), through
    gmk_pvnet_evaluate_sym (include/gomoku_symmetry.h states the rule).  It holds no weights and no handle of its own: it evaluates with whatever
    `fused` holds when it is called, so later load_from() / set_precision() calls on `fused` are followed.  Capturable: the expand kernel, the
    network's two kernels and the reduce kernel go to torch's current stream, nothing synchronises (the handle's workspace grows at the first
    call of a batch size, which AlphaZeroMCTS.search(graph=True) makes eagerly)."""

    def __init__(self, fused, mode, seed=None):
        from . import lib as G
        if mode not in G.PVNET_SYMMETRIES:                                  # before anything touches the device: a typo is a ValueError on any machine
            raise ValueError("symmetric: mode must be one of %s, not %r" % (sorted(G.PVNET_SYMMETRIES), mode))
        self.fused, self.G, self.mode = fused, G, mode
        self.seed = (G.DEFAULT_SEED if seed is None else int(seed)) & 0xFFFFFFFFFFFFFFFF

    @property
    def net(self):
        return self.fused.net

    @torch.no_grad()
    def __call__(self, states):
        """states float32 [B, 6, 15, 15] on the GPU -> (value [B], probs [B, 225]); every kernel goes to torch's current stream."""
        assert states.is_cuda and states.dtype == torch.float32 and states.is_contiguous() and tuple(states.shape[1:]) == (6, 15, 15)
        n = states.shape[0]
        value = torch.empty((n,), dtype=torch.float32, device=states.device)
        probs = torch.empty((n, 225), dtype=torch.float32, device=states.device)
        self.G._check(self.G.load().gmk_pvnet_evaluate_sym(self.fused.h, states.data_ptr(), n, self.G.PVNET_SYMMETRIES[self.mode], self.seed, value.data_ptr(),
                                                           probs.data_ptr(), torch.cuda.current_stream(states.device).cuda_stream))
        return value, probs

    @torch.no_grad()
    def eval_state(self, board):
        """FusedPolicyValueNetwork.eval_state through the symmetries: one position -> (value, probs[225]) on the host."""
        dev = next(self.fused.net.parameters()).device
        states = torch.from_numpy(np.asarray(board.encoded_states(), dtype=np.float32)[None]).to(dev)
        value, probs = self(states)
        return float(value[0]), probs[0].cpu().numpy()


class PatternEvaluator:
    """The reference's hand-written pattern heuristic where a network goes (K23, gmk_pattern_evaluate_states): network(states) -> (value, probs)
    for K7 (lib.AlphaZeroMCTS.search), the self-play and match loops of selfplay.py and NetworkAgent, with no weights and nothing to train.
    A row of planes is decoded into its canonical move list and evaluated as K10 evaluates a list (include/gomoku_pattern_states.h states the
    rule): probs = Heuristic::EvaluationProbs, after DecisiveFilter when `filter`; value = EvaluationValue for the player to move.
    norm "sum" (default): the prior sums to 1, uniform over the empty cells where the heuristic sees nothing; "l2": K10's L2-normalised vector
    as it is.  A row that is not a position -- the zero row of a leaf whose game is over -- gets zeros, which K7 ignores.
    One kernel on torch's current stream, nothing synchronises: capturable after one eager call.  The output tensors are kept per device and
    batch size and written again by the next call of that size: take a copy of what has to outlive it."""

    def __init__(self, filter=True, norm="sum"):
        from . import lib as G
        self.G, self.filter, self.norm = G, bool(filter), norm
        self._norm = G._pattern_norm(norm)                                   # a typo is a ValueError on any machine
        self._outputs = {}

    @torch.no_grad()
    def __call__(self, states):
        """states float32 [B, 6, 15, 15] on the GPU -> (value [B], probs [B, 225]) on torch's current stream."""
        assert states.is_cuda and states.dtype == torch.float32 and states.is_contiguous() and tuple(states.shape[1:]) == (6, 15, 15)
        n = states.shape[0]
        key = (states.device, n)
        if key not in self._outputs:
            self._outputs[key] = (torch.zeros((n,), dtype=torch.float32, device=states.device),
                                  torch.zeros((n, 225), dtype=torch.float32, device=states.device))
        value, probs = self._outputs[key]
        self.G.pattern_evaluate_states(states, self.filter, self._norm, value=value, probs=probs, status=False)
        return value, probs

    def symmetric(self, mode, seed=None):
        """None or "none": this evaluator.  Anything else is a ValueError: the heuristic is a fixed rule, not a learned function whose
        orientations are worth averaging or drawing from."""
        if mode in (None, "none"):
            return self
        raise ValueError("PatternEvaluator.symmetric: mode is None or \"none\", not %r -- the pattern heuristic is not a learned function to "
                         "average over the board's symmetries" % (mode,))

    @torch.no_grad()
    def eval_state(self, board):
        """One position -> (value, probs[225]) on the host: what CorePyExt.MCTS's Policy(eval_state=...) and NetworkAgent call."""
        states = torch.from_numpy(np.ascontiguousarray(np.asarray(board.encoded_states(), dtype=np.float32).reshape(1, 6, 15, 15))).cuda()
        value, probs = self(states)
        return float(value[0]), probs[0].cpu().numpy()


# the trainer's tensor names (lib.TRAIN_TENSORS) -> how a PolicyValueNetwork holds them
_MODULE_TENSORS = (("w1", "conv.0.weight"), ("b1", "conv.0.bias"), ("w2", "conv.1.weight"), ("b2", "conv.1.bias"), ("w3", "conv.2.weight"), ("b3", "conv.2.bias"),
                   ("w_policy_conv", "policy_conv.weight"), ("b_policy_conv", "policy_conv.bias"), ("w_value_conv", "value_conv.weight"), ("b_value_conv", "value_conv.bias"),
                   ("w_policy", "policy_dense.weight"), ("b_policy", "policy_dense.bias"), ("w_hidden", "value_hidden.weight"), ("b_hidden", "value_hidden.bias"),
                   ("w_out", "value_out.weight"), ("b_out", "value_out.bias"))


def load_weights(path):
    """A PolicyValueNetwork (on the host) with the weights in `path`: either a torch.save'd PolicyValueNetwork.state_dict(), or a file
    TrainingLoop.save wrote, whose state["trainer"]["params"] holds the sixteen tensors under the trainer's names.  Read with weights_only=True."""
    import os
    state = torch.load(os.fspath(path), map_location="cpu", weights_only=True)
    net = PolicyValueNetwork()
    if isinstance(state, dict) and isinstance(state.get("trainer"), dict) and "params" in state["trainer"]:
        params, sd = state["trainer"]["params"], net.state_dict()
        missing = [name for name, _ in _MODULE_TENSORS if name not in params]
        if missing:
            raise ValueError("load_weights: %s is a training checkpoint without %s" % (path, ", ".join(missing)))
        with torch.no_grad():
            for name, key in _MODULE_TENSORS:
                sd[key].copy_(torch.as_tensor(params[name], dtype=torch.float32).reshape(sd[key].shape))
    elif isinstance(state, dict) and all(key in state for _, key in _MODULE_TENSORS):
        net.load_state_dict(state)
    else:
        raise ValueError("load_weights: %s holds neither a PolicyValueNetwork.state_dict() nor a TrainingLoop checkpoint" % (path,))
    return net


def module_arrays(net):
    """{trainer tensor name: float32 numpy array in the trainer's shape} of a PolicyValueNetwork."""
    from . import lib as G
    sd, shapes = net.state_dict(), dict(G.TRAIN_TENSORS)
    return {name: np.ascontiguousarray(sd[key].detach().float().cpu().numpy()).reshape(shapes[name]) for name, key in _MODULE_TENSORS}


class Trainer:
    """The network's training step on the device (gmk_train_*, train_kernel.hip; K11): compile() and train_step() of the reference's
    PolicyValueNetwork (model_tf.py:73-135).  Holds its own float32 copy of `net`'s parameters, Adam's moments and the activations of up
    to max_batch positions in HBM; float32 throughout and bit-reproducible.  All inputs are contiguous float32 CUDA tensors -- what
    selfplay.ReplayBuffer.sample returns -- and every kernel goes to torch's current stream."""

    def __init__(self, net, max_batch=512):
        from . import lib as G
        G.init()
        self.G, self.max_batch = G, int(max_batch)
        self.device = next(net.parameters()).device
        if self.device.type != "cuda":
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._h = G.TrainerHandle(module_arrays(net), max_batch)

    def close(self):
        if getattr(self, "_h", None) is not None:
            self._h.close()
            self._h = None

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _batch(self, states, values=None, pi=None):
        n = states.shape[0]
        if not (states.is_cuda and states.dtype == torch.float32 and states.is_contiguous() and tuple(states.shape[1:]) == (6, 15, 15)):
            raise ValueError("Trainer: states must be a contiguous float32 CUDA tensor [n, 6, 15, 15]")
        if not 1 <= n <= self.max_batch:
            raise ValueError("Trainer: the batch must hold 1 .. max_batch = %d positions" % self.max_batch)
        if values is not None and not (values.is_cuda and values.dtype == torch.float32 and values.is_contiguous() and tuple(values.shape) == (n,)):
            raise ValueError("Trainer: values must be a contiguous float32 CUDA tensor [n]")
        if pi is not None and not (pi.is_cuda and pi.dtype == torch.float32 and pi.is_contiguous() and tuple(pi.shape) == (n, 225)):
            raise ValueError("Trainer: pi must be a contiguous float32 CUDA tensor [n, 225]")
        return n

    def forward(self, states):
        """-> (value [n], probs [n, 225]) with the trainer's current parameters."""
        n = self._batch(states)
        value = torch.empty((n,), dtype=torch.float32, device=states.device)
        probs = torch.empty((n, 225), dtype=torch.float32, device=states.device)
        self._h.forward(states.data_ptr(), n, value.data_ptr(), probs.data_ptr(), self._stream())
        return value, probs

    def grads(self, states, values, pi):
        """Forward, loss and backward without an update -> ({name: gradient of the data loss, no L2 term}, metrics float32[4] on the device =
        loss including L2, entropy, value loss, policy loss).  The gradients are views of one block in lib.TRAIN_BLOCK_ORDER."""
        n = self._batch(states, values, pi)
        block = torch.empty(self.G.TRAIN_PARAMS, dtype=torch.float32, device=states.device)
        metrics = torch.empty(4, dtype=torch.float32, device=states.device)
        self._h.grads(states.data_ptr(), values.data_ptr(), pi.data_ptr(), n, block.data_ptr(), metrics.data_ptr(), self._stream())
        return self.G.split_block(block), metrics

    def step(self, states, values, pi, lr, old_probs=None):
        """One optimiser step -> (probs [n, 225] from BEFORE the update, metrics float32[5] on the device = loss, entropy, value loss, policy
        loss, KL against old_probs (0 without))."""
        n = self._batch(states, values, pi)
        if old_probs is not None and not (old_probs.is_cuda and old_probs.dtype == torch.float32 and old_probs.is_contiguous() and tuple(old_probs.shape) == (n, 225)):
            raise ValueError("Trainer.step: old_probs must be a contiguous float32 CUDA tensor [n, 225]")
        probs = torch.empty((n, 225), dtype=torch.float32, device=states.device)
        metrics = torch.empty(5, dtype=torch.float32, device=states.device)
        self._h.step(states.data_ptr(), values.data_ptr(), pi.data_ptr(), n, lr, None if old_probs is None else old_probs.data_ptr(),
                     probs.data_ptr(), metrics.data_ptr(), self._stream())
        return probs, metrics

    def train_step(self, states, values, pi, lr, kl_target, num_epoches=5):
        """PolicyValueNetwork.train_step (model_tf.py:111-135): up to num_epoches optimiser steps on one minibatch.  The first pass's
        probabilities are `old`; every later pass reports its KL against them and the passes stop once kl > 4 kl_target.  One four-byte
        read-back per pass (the KL) decides that; loss and entropy are read once at the end.  -> (loss, entropy, kl, epochs)."""
        old, kl, metrics, done = None, 0.0, None, 0
        for i in range(int(num_epoches)):
            probs, metrics = self.step(states, values, pi, lr, old)
            done = i + 1
            if i == 0:
                old, kl = probs, 0.0                      # "KL divergence is apparently zero"; the one read-back of this pass is skipped with it
            else:
                kl = float(metrics[4])
            if kl > 4 * kl_target:
                break
        if metrics is None:
            return 0.0, 0.0, 0.0, 0
        loss, entropy = metrics[:2].tolist()
        return loss, entropy, kl, done

    def params(self):
        """{name: float32 numpy array} of the current parameters (lib.TRAIN_TENSORS); synchronises."""
        return self._h.params()

    def sync_to(self, module):
        """The trainer's parameters back into a PolicyValueNetwork (on whichever device it lives)."""
        arrays = self._h.params()
        sd = module.state_dict()
        with torch.no_grad():
            for name, key in _MODULE_TENSORS:
                sd[key].copy_(torch.from_numpy(arrays[name]).reshape(sd[key].shape))
        return module

    def last_update(self):
        """{name: what the last step subtracted from the tensor}: w_new = w_old - update exactly, in float32."""
        return self.G.split_block(self._h.get_block(self.G.BLOCK_UPDATE))

    def state_dict(self):
        """Parameters, both moments (blocks in lib.TRAIN_BLOCK_ORDER, split by name) and Adam's step count."""
        G = self.G
        return {"params": self._h.params(), "m": dict(G.split_block(self._h.get_block(G.BLOCK_M))), "v": dict(G.split_block(self._h.get_block(G.BLOCK_V))),
                "step": self._h.info()["step"]}

    def load_state_dict(self, state):
        G = self.G
        self._h.set_params(state["params"])
        self._h.set_block(G.BLOCK_M, G.join_block(state["m"]))
        self._h.set_block(G.BLOCK_V, G.join_block(state["v"]))
        self._h.set_step_count(state["step"])

    @property
    def steps(self):
        return self._h.info()["step"]

    def export(self, fused):
        """The current parameters into an existing FusedPolicyValueNetwork's device buffers (gmk_train_export), ordered on the current stream."""
        self._h.export(fused.h, self._stream())
