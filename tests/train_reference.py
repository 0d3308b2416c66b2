"""Float64 restatement of one training step of PolicyValueNetwork (network/model_tf.py:73-135) on the CPU, the float32 yardstick next to it, and
the minibatches the trainer's tests run on.

TEST INFRASTRUCTURE ONLY.
  * loss_terms(): the loss exactly as model_tf.py:77-89 states it -- mean squared value error + mean softmax cross-entropy against pi (from the
    log-softmax) + 1e-4 * sum(w^2) / 2 over everything that is not a bias -- and the entropy mean(-sum p log(p + 1e-10)).
  * gradients(): of the DATA loss (no L2 term; what gmk_train_grads returns) by torch autograd, in float64 or float32.
  * adam_step(): TF1's Adam as tf.train.AdamOptimizer documents it, in numpy float64, with the L2 gradient 1e-4 w on the weights.
  * RefTrainer: the multi-pass train_step of model_tf.py:111-135 with its early stop, on those.
  * The criteria: gradient_ratios() -- per tensor (max|g - g64| - 1e-7 max|g64|) / max|g32 - g64|, to be held below a LIMIT; the yardstick is
    torch's float32 against float64 on the same batch, never the kernel -- and learning_margin().  sturdy_ratios() is the same formula over
    yardstick(): the largest float32 error of five sample orders of the batch, for the cases of tests/test_train_seams_gpu.py (seam_case(),
    degenerate_case()); the single-evaluation yardstick is kept for the cases that were recorded with it.
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


YARD_ORDERS = 5               # float32 evaluations behind the sturdier yardstick: the batch as given + four seeded permutations of its samples


def sample_order(n, i):
    """Sample order i of a batch of n: 0 is the batch as given, i >= 1 a permutation seeded by (n, i).  Orders 0 .. YARD_ORDERS - 1 make the
    yardstick; the criterion's own test holds orders YARD_ORDERS and YARD_ORDERS + 1 against it."""
    return np.arange(n) if i == 0 else np.random.RandomState(7919 * n + i).permutation(n)


def reordered(batch, order):
    return tuple(np.ascontiguousarray(a[order]) for a in batch)


def float32_errors(params, batch, g64, orders=range(YARD_ORDERS)):
    """-> {name: [max|g32 - g64| of torch float32 on the batch in each of `orders`]}.  The batch mean does not depend on the sample order in
    exact arithmetic, so one g64 serves every order; float32's rounding does, and that is the spread the single yardstick does not see."""
    out = {k: [] for k in NAMES}
    for i in orders:
        g32, _, _ = gradients(params, reordered(batch, sample_order(len(batch[0]), i)), torch.float32)
        for k in NAMES:
            out[k].append(float(np.abs(g32[k] - g64[k]).max()))
    return out


def yardstick(params, batch, g64):
    """-> {name: the LARGEST max|g32 - g64| over YARD_ORDERS torch-float32 evaluations of the same batch}.  On b_out (1 element), b_value_conv
    (2) and b_policy_conv (4) one evaluation's error is the maximum over one to four numbers and can come out many times smaller than the next
    order's; the largest of five is what float32 demonstrably does on this batch."""
    return {k: max(v) for k, v in float32_errors(params, batch, g64).items()}


def sturdy_ratios(got, g64, yard):
    """gradient_ratios() with the yardstick() of five sample orders in place of one evaluation's error: per tensor
    (max|got - g64| - 1e-7 max|g64|) / yard, to be held below GRAD_LIMIT.  A tensor whose five yardsticks are all 0 must be matched within the
    floor: 0 then, else inf."""
    out = {}
    for k in NAMES:
        err = float(np.abs(np.asarray(got[k], np.float64).reshape(g64[k].shape) - g64[k]).max()) - 1e-7 * float(np.abs(g64[k]).max())
        out[k] = 0.0 if err <= 0 else (err / yard[k] if yard[k] > 0 else float("inf"))
    return out


# ---------------- the cases of tests/test_train_seams_gpu.py, pinned on the CPU by tests/test_train_reference.py ----------------
SEAM_BATCHES = (8, 9, 32, 64, 65, 257)         # a full k slab and one beyond, a full column slab, two and one beyond; 257: second round of the batch
#                                                sums, a third row of workgroups in the dense GEMMs, 33 k slabs
DEGENERATE = ("underflow", "not_distributions", "dead_layer3", "dead_layer2", "saturated_tanh")
DEAD_ZEROS = ("w1", "b1", "w2", "b2", "w3", "b3", "w_policy_conv", "w_value_conv")
# layer 3 still fires on its biases (b3's gradient is not 0), so its input's gradient is not 0 until col2im's mask makes it so; on make_net(3) the
# policy head's four constant pre-activations are all negative, the value head's are not
DEAD2_ZEROS = ("w1", "b1", "w2", "b2", "w3", "w_policy_conv", "b_policy_conv", "w_policy")
SATURATED_ZEROS = ("w_value_conv", "b_value_conv", "w_hidden", "b_hidden", "w_out", "b_out")


SEAM_BATCH_SEED = {9: 119}     # batch seed 19 puts float32's own sixth order at 1.97 (2.06 on one thread) of the yardstick on b3: above GRAD_LIMIT / 4


def seam_case(n):
    """-> (params, batch) of the parity case at batch n: make_net(n) on make_batch(n, seed=10 + n), as test_gradient_parity draws its own,
    but for SEAM_BATCH_SEED.  Seeds are chosen on the CPU by test_five_order_yardstick_holds_float32_itself, never by what a kernel gives."""
    return module_arrays(make_net(n)), make_batch(n, seed=SEAM_BATCH_SEED.get(n, 10 + n))


def degenerate_case(kind):
    """-> (params, batch), n = 4, from make_net(3) and make_batch(4, seed=77):
    underflow          b_policy = linspace(0, -250, 225): the logits spread over more than 200, float32's exp underflows below about -104;
                       every pi row is one-hot on the sample's least likely cell
    not_distributions  pi rows: all zero, a row x 0.5, a one-hot row, a row as recorded
    dead_layer3        b3 = -100: layer 3 never fires, nothing reaches the trunk (the GEMM epilogue's mask)
    dead_layer2        b2 = -100: layer 2 never fires, layer 3 sees zeros and fires on its biases; nothing passes layer 2 (col2im's mask)
    saturated_tanh     b_out = 30: tanh(s) = 1 exactly in float32 and float64, nothing reaches the value path"""
    params = {k: a.copy() for k, a in module_arrays(make_net(3)).items()}
    states, values, pi = make_batch(4, seed=77)
    if kind == "underflow":
        params["b_policy"][:] = np.linspace(0.0, -250.0, 225).astype(np.float32)
        with torch.no_grad():
            logits, _ = forward({k: torch.tensor(params[k], dtype=torch.float64) for k in NAMES}, torch.tensor(states, dtype=torch.float64))
        pi = np.stack([_one_hot(int(c)) for c in logits.argmin(1)])
    elif kind == "not_distributions":
        pi = pi.copy()
        pi[0] = 0.0
        pi[1] *= np.float32(0.5)
        pi[2] = _one_hot(112)
    elif kind == "dead_layer3":
        params["b3"][:] = -100.0
    elif kind == "dead_layer2":
        params["b2"][:] = -100.0
    else:
        assert kind == "saturated_tanh", kind
        params["b_out"][:] = 30.0
    return params, (states, values, np.ascontiguousarray(pi))


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """"seam-<n>" or one of DEGENERATE -> dict(params, batch, g64, terms (float64), terms32 (torch float32, the batch as given), probs (float64),
    yard (the five-order yardstick)).  Computed once per process and shared; callers do not write into it."""
    params, batch = seam_case(int(name[5:])) if name.startswith("seam-") else degenerate_case(name)
    g64, terms, probs = gradients(params, batch, torch.float64)
    _, terms32, _ = gradients(params, batch, torch.float32)
    return {"params": params, "batch": batch, "g64": g64, "terms": terms, "terms32": terms32, "probs": probs, "yard": yardstick(params, batch, g64)}


def sparse_old_probs(n, seed=12):
    """float32 [n, 225]: the probabilities of make_net(seed) on make_batch(n, seed), every entry below 1/225 set to exactly 0 (the rows no
    longer sum to one, as the replay buffer's thresholded rows do not)."""
    _, _, probs = gradients(module_arrays(make_net(seed)), make_batch(n, seed=seed), torch.float64)
    probs = probs.astype(np.float32)
    probs[probs < 1.0 / 225] = 0.0
    return np.ascontiguousarray(probs)


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
