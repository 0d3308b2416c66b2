"""Float64 restatement of one training step of PolicyValueNetwork (network/model_tf.py:73-135) on the CPU, the float32 yardstick next to it, and
the minibatches the trainer's tests run on.

TEST INFRASTRUCTURE ONLY.
  * loss_terms(): the loss exactly as model_tf.py:77-89 states it -- mean squared value error + mean softmax cross-entropy against pi (from the
    log-softmax) + 1e-4 * sum(w^2) / 2 over everything that is not a bias -- and the entropy mean(-sum p log(p + 1e-10)).
  * gradients(): of the DATA loss (no L2 term; what gmk_train_grads returns) by torch autograd, in float64 or float32.
  * adam_step(): TF1's Adam as tf.train.AdamOptimizer documents it, in numpy float64, with the L2 gradient 1e-4 w on the weights.
  * RefTrainer: the multi-pass train_step of model_tf.py:111-135 with its early stop, on those.
  * The criteria: gradient_ratios() -- per tensor (max|g - g64| - 1e-7 max|g64|) / max|g32 - g64|, to be held below a LIMIT; the yardstick is
    torch's float32 against float64 on the same batch, never the kernel -- and learning_margin().
Tensor names are the trainer's (gomokuai_amd.lib.TRAIN_TENSORS)."""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

from gomokuai_amd import lib as G
from gomokuai_amd.network import module_arrays

import pvnet_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_tuples.npz")
NAMES = tuple(name for name, _ in G.TRAIN_TENSORS)
BIASES = G.TRAIN_BIASES
L2 = 1e-4
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8
GRAD_LIMIT = 8.0               # the kernel's gradient error, in units of torch float32's on the same batch
LEARN_STEPS, LEARN_BATCH, LEARN_LR, LEARN_MID = 30, 64, 2e-3, 15


# ---------------- minibatches ----------------
@functools.lru_cache(maxsize=None)
def golden_tuples():
    """(states float32 [706,6,15,15], values float32 [706], pi float32 [706,225]) of the reference's recorded games."""
    d = np.load(GOLDEN)
    return d["states"].astype(np.float32), d["values"].astype(np.float32), d["probs"].astype(np.float32)


def _one_hot(cell):
    pi = np.zeros(225, np.float32)
    pi[cell] = 1.0
    return pi


def specials():
    """Synthetic samples: stones on all four edges and corners with a one-hot pi on a corner; the empty board; a full board with a one-hot pi."""
    rim = [0, 14, 210, 224, 7, 105, 119, 217, 1, 13, 15, 29, 195, 209, 211, 223]
    full = list(np.random.RandomState(7).permutation(225)[:224])
    _, _, pi = golden_tuples()
    return [(R.planes(rim), np.float32(1.0), _one_hot(224)),
            (R.planes([]), np.float32(0.0), pi[0]),
            (R.planes([int(c) for c in full]), np.float32(-1.0), _one_hot(int(sorted(set(range(225)) - set(full))[0])))]


def make_batch(n, seed=0, with_specials=True):
    """A minibatch of n samples: golden tuples drawn without replacement by `seed`, the first min(n, 3) replaced by specials()."""
    states, values, pi = golden_tuples()
    idx = np.random.RandomState(seed).permutation(len(states))[:n]
    s, v, p = states[idx].copy(), values[idx].copy(), pi[idx].copy()
    if with_specials:
        for j, (ss, vv, pp) in enumerate(specials()[:n]):
            s[j], v[j], p[j] = ss, vv, pp
    return np.ascontiguousarray(s), np.ascontiguousarray(v), np.ascontiguousarray(p)


def make_net(seed=0):
    """glorot weights with random biases (pvnet_reference.make_net): every bias gradient meets a non-zero bias."""
    return R.make_net("glorot", seed)


# ---------------- the step in torch ----------------
def _tensors(params, dtype):
    """{name: array} -> {name: leaf tensor of dtype that wants a gradient}"""
    return {k: torch.tensor(np.asarray(params[k]), dtype=dtype, requires_grad=True) for k in NAMES}


def forward(w, states):
    """-> (logits [n,225], value pre-activation [n]) from tensors {name: tensor} and states [n,6,15,15] of the same dtype."""
    x = states
    for i in (1, 2, 3):
        x = F.relu(F.conv2d(x, w["w%d" % i], w["b%d" % i], padding=1))
    n = x.shape[0]
    pc = F.relu(F.conv2d(x, w["w_policy_conv"].reshape(4, 128, 1, 1), w["b_policy_conv"])).permute(0, 2, 3, 1).reshape(n, -1)
    vc = F.relu(F.conv2d(x, w["w_value_conv"].reshape(2, 128, 1, 1), w["b_value_conv"])).permute(0, 2, 3, 1).reshape(n, -1)
    logits = pc @ w["w_policy"].T + w["b_policy"]
    hidden = F.relu(vc @ w["w_hidden"].T + w["b_hidden"])
    s = hidden @ w["w_out"].reshape(64) + w["b_out"].reshape(())
    return logits, s


def loss_terms(w, states, values, pi):
    """-> dict of torch scalars: loss (with L2), entropy, value_loss, policy_loss, data_loss (= value + policy), and probs [n,225]."""
    logits, s = forward(w, states)
    value_loss = ((torch.tanh(s) - values) ** 2).mean()
    policy_loss = (-(pi * F.log_softmax(logits, 1)).sum(1)).mean()
    l2 = L2 * sum((w[k] ** 2).sum() / 2 for k in NAMES if k not in BIASES)
    probs = F.softmax(logits, 1)
    entropy = (-(probs * torch.log(probs + 1e-10)).sum(1)).mean()
    return {"loss": value_loss + policy_loss + l2, "entropy": entropy, "value_loss": value_loss, "policy_loss": policy_loss,
            "data_loss": value_loss + policy_loss, "probs": probs}


def gradients(params, batch, dtype=torch.float64):
    """-> ({name: gradient of the data loss, float64 numpy}, {loss, entropy, value_loss, policy_loss: float}, probs float64 numpy)."""
    w = _tensors(params, dtype)
    states, values, pi = (torch.tensor(a, dtype=dtype) for a in batch)
    t = loss_terms(w, states, values, pi)
    t["data_loss"].backward()
    grads = {k: w[k].grad.detach().double().numpy() for k in NAMES}
    return grads, {k: float(t[k].detach()) for k in ("loss", "entropy", "value_loss", "policy_loss")}, t["probs"].detach().double().numpy()


def gradient_ratios(got, g64, g32):
    """Per tensor: (max|got - g64| - 1e-7 max|g64|) / max|g32 - g64| -- what the criterion holds below LIMIT.  A tensor on which float32 is exact
    (yardstick 0) must be matched within the floor: 0 then, else inf."""
    out = {}
    for k in NAMES:
        err = float(np.abs(np.asarray(got[k], np.float64).reshape(g64[k].shape) - g64[k]).max()) - 1e-7 * float(np.abs(g64[k]).max())
        yard = float(np.abs(g32[k] - g64[k]).max())
        out[k] = 0.0 if err <= 0 else (err / yard if yard > 0 else float("inf"))
    return out


def adam_step(params, grads, m, v, t, lr):
    """TF1 Adam + L2 in float64 numpy, step t >= 1: -> (new params, new m, new v), dicts by name; inputs are not changed."""
    lr_t = lr * np.sqrt(1 - BETA2 ** t) / (1 - BETA1 ** t)
    new, nm, nv = {}, {}, {}
    for k in NAMES:
        w = np.asarray(params[k], np.float64)
        g = np.asarray(grads[k], np.float64).reshape(w.shape) + (0.0 if k in BIASES else L2 * w)
        nm[k] = BETA1 * np.asarray(m[k], np.float64) + (1 - BETA1) * g
        nv[k] = BETA2 * np.asarray(v[k], np.float64) + (1 - BETA2) * g * g
        new[k] = w - lr_t * nm[k] / (np.sqrt(nv[k]) + EPS)
    return new, nm, nv


def kl_divergence(old_probs, new_probs):
    """(old * log(old / new)).sum(1).mean() with both sides + 1e-10 (model_tf.py:122-127)."""
    o, p = np.asarray(old_probs, np.float64) + 1e-10, np.asarray(new_probs, np.float64) + 1e-10
    return float((o * np.log(o / p)).sum(1).mean())


class RefTrainer:
    """compile() + train_step() of the reference on the CPU; dtype torch.float64 (the reference) or torch.float32 (the yardstick: float32
    gradients from autograd, the optimiser in float32 numpy)."""

    def __init__(self, net_or_params, dtype=torch.float64):
        params = net_or_params if isinstance(net_or_params, dict) else module_arrays(net_or_params)
        self.dtype, self.np_dtype = dtype, np.float64 if dtype == torch.float64 else np.float32
        self.params = {k: np.asarray(params[k], self.np_dtype).copy() for k in NAMES}
        self.m = {k: np.zeros_like(self.params[k]) for k in NAMES}
        self.v = {k: np.zeros_like(self.params[k]) for k in NAMES}
        self.t = 0

    def step(self, batch, lr):
        """-> (probs from before the update, loss, entropy)"""
        grads, terms, probs = gradients(self.params, batch, self.dtype)
        self.t += 1
        new, self.m, self.v = adam_step(self.params, grads, self.m, self.v, self.t, lr)
        cast = lambda d: {k: a.astype(self.np_dtype) for k, a in d.items()}
        self.params, self.m, self.v = cast(new), cast(self.m), cast(self.v)
        return probs, terms["loss"], terms["entropy"]

    def train_step(self, batch, lr, kl_target, num_epoches=5):
        old, kl = None, 0.0
        for i in range(num_epoches):
            probs, loss, entropy = self.step(batch, lr)
            if i == 0:
                old, kl = probs, 0.0
            else:
                kl = kl_divergence(old, probs)
            if kl > 4 * kl_target:
                break
        return loss, entropy, kl, i + 1


@functools.lru_cache(maxsize=None)
def learning_curve(dtype_name):
    """The loss before each of LEARN_STEPS steps and after the last (LEARN_STEPS + 1 values) on make_batch(LEARN_BATCH, seed=3, no specials) from
    make_net(0) at LEARN_LR, in "float64" or "float32" on the CPU."""
    dtype = torch.float64 if dtype_name == "float64" else torch.float32
    batch = learning_batch()
    ref = RefTrainer(make_net(0), dtype)
    losses = [ref.step(batch, LEARN_LR)[1] for _ in range(LEARN_STEPS)]
    losses.append(gradients(ref.params, batch, dtype)[1]["loss"])
    return tuple(losses)


def learning_batch():
    return make_batch(LEARN_BATCH, seed=3, with_specials=False)


def learning_margin(first, last):
    """The learning criterion: the loss must end below its start and below the float64 run's loss at step LEARN_MID.  Returns the share of the
    room between the float64 run's own end and that bar which `last` uses: <= 0 is as good as float64, 1 is the bar."""
    ref = learning_curve("float64")
    bar = min(ref[LEARN_MID], first)
    return (last - ref[-1]) / (bar - ref[-1])
