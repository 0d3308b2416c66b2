"""gmk_pvnet_evaluate_sym ("K22") on the device against the composition that defines it: tests/pvnet_sym_reference.py's transforms (np.rot90 /
np.fliplr, no index table) around the existing fused network, whose rows are bit-isolated in both precisions
(tests/test_pvnet_precision_gpu.py).  GMK_PVNET_SYM_ALL, GMK_PVNET_SYM_RANDOM and GMK_PVNET_SYM_NONE are compared bit for bit; the invariance of
ALL under a transform of its input holds within the rounding of an eight-term float32 sum taken in two orders."""
import ctypes as C

import numpy as np
import pytest

import pvnet_sym_reference as S
from gomokuai_amd import lib as G

pytestmark = pytest.mark.gpu

N = 225
SEED = 0x9E3779B97F4A7C15
NONE, ALL, RANDOM = 0, 1, 2
ERR_ARG, ERR_STATE = -3, -4
PRECISIONS = ["f32", "bf16"]
BOARDS = S.positions(33, 7)                                      # 33 rows: ALL hands the dense kernel 264 = 16 groups of 16 and half of one


@pytest.fixture(scope="module")
def nets():
    import torch
    from gomokuai_amd.network import FusedPolicyValueNetwork, PolicyValueNetwork
    G.init(0)
    module = PolicyValueNetwork(seed=3).cuda().eval()
    out = {"f32": FusedPolicyValueNetwork(module), "bf16": FusedPolicyValueNetwork(module, precision="bf16")}
    torch.cuda.synchronize()
    yield out
    out["f32"].close()
    out["bf16"].close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(got, want, what=""):
    np.testing.assert_array_equal(u32(got), u32(want), what)


def evaluate_sym(net, x, mode, seed=SEED):
    """the entry itself on x float32 [n, 6, 15, 15] (numpy) -> (value [n], probs [n, 225]) as numpy; the rows behind n and the input are checked"""
    import torch
    n = x.shape[0]
    xs = dev(x) if n else torch.zeros((1, 6, 15, 15), device="cuda")
    keep = xs.clone()
    value, probs = torch.full((n + 2,), -7.5, device="cuda"), torch.full((n + 2, N), -7.5, device="cuda")
    G._check(G.load().gmk_pvnet_evaluate_sym(net.h, xs.data_ptr(), n, mode, seed, value.data_ptr(), probs.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert torch.equal(xs, keep), "the input was written"
    assert (value[n:] == -7.5).all() and (probs[n:] == -7.5).all(), "rows behind n were written"
    return value[:n].cpu().numpy(), probs[:n].cpu().numpy()


_TERMS = {}


def terms(nets, precision):
    """(v_a [8][33], p_a [8][33, 225]): the plain fused network on T_a(BOARDS), the policy rows back-transformed; computed once per precision"""
    if precision not in _TERMS:
        vs, ps = [], []
        for a in range(8):
            v, q = nets[precision](dev(S.transform(BOARDS, a)))
            vs.append(v.cpu().numpy())
            ps.append(S.back(q.cpu().numpy(), a))
        _TERMS[precision] = (vs, ps)
    return _TERMS[precision]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", [1, 2, 17, 33])
def test_all_is_the_ordered_average_of_the_eight_evaluations(nets, precision, n):
    vs, ps = terms(nets, precision)
    want_v, want_p = S.combine_all([v[:n] for v in vs], [p[:n] for p in ps])
    got_v, got_p = evaluate_sym(nets[precision], BOARDS[:n], ALL)
    same_bits(got_v, want_v, "value")
    same_bits(got_p, want_p, "probs")
    assert abs(got_p.sum(axis=1) - 1).max() < 1e-5
    plain = nets[precision](dev(BOARDS[:n]))[1].cpu().numpy()
    assert (u32(got_p) != u32(plain)).mean() > 0.5               # (an average, not the plain row)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_random_is_the_one_evaluation_the_host_pick_names(nets, precision):
    pick = G.pvnet_sym_pick_host(BOARDS, SEED)
    assert sorted(set(pick.tolist())) == list(range(8)), "BOARDS were chosen so that every symmetry is picked"
    assert pick.tolist() == S.pick(BOARDS, SEED).tolist()
    vs, ps = terms(nets, precision)
    got_v, got_p = evaluate_sym(nets[precision], BOARDS, RANDOM)
    rows = np.arange(33)
    same_bits(got_v, np.stack(vs)[pick, rows], "value")
    same_bits(got_p, np.stack(ps)[pick, rows], "probs")
    other = G.pvnet_sym_pick_host(BOARDS, SEED + 1)
    assert (other != pick).sum() > 16
    got_v, got_p = evaluate_sym(nets[precision], BOARDS, RANDOM, SEED + 1)
    same_bits(got_v, np.stack(vs)[other, rows], "value, another seed")
    same_bits(got_p, np.stack(ps)[other, rows], "probs, another seed")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_none_is_the_plain_entry(nets, precision):
    value, probs = nets[precision](dev(BOARDS))
    got_v, got_p = evaluate_sym(nets[precision], BOARDS, NONE, 12345)
    same_bits(got_v, value.cpu().numpy())
    same_bits(got_p, probs.cpu().numpy())
    vs, ps = terms(nets, precision)
    same_bits(got_v, vs[0])                                      # symmetry 0 is the identity
    same_bits(got_p, ps[0])


@pytest.mark.parametrize("precision", PRECISIONS)
def test_all_is_invariant_under_the_symmetries_to_rounding(nets, precision):
    """evaluate_sym(T_b(x), ALL) adds the same eight terms as evaluate_sym(x, ALL) in another order: per element the two differ by at most
    16 * 2^-24 * sum_a |term_a| (7 additions and the order, twice: (n - 1) u sum|t| bounds one order's error)"""
    vs, ps = terms(nets, precision)
    base_v, base_p = evaluate_sym(nets[precision], BOARDS, ALL)
    bound_v = 16 * 2.0 ** -24 * np.abs(np.stack(vs)).astype(np.float64).sum(axis=0)
    bound_p = 16 * 2.0 ** -24 * np.abs(np.stack(ps)).astype(np.float64).sum(axis=0)
    for b in range(1, 8):
        got_v, got_p = evaluate_sym(nets[precision], S.transform(BOARDS, b), ALL)
        assert (np.abs(got_v.astype(np.float64) - base_v) <= bound_v).all(), b
        want_p = S.transform(base_p.reshape(33, 15, 15), b).reshape(33, N)
        limit = S.transform(bound_p.reshape(33, 15, 15), b).reshape(33, N)
        assert (np.abs(got_p.astype(np.float64) - want_p) <= limit).all(), b
        assert (u32(got_p) != u32(base_p)).mean() > 0.5         # (the rows did move)


@pytest.mark.parametrize("mode", [ALL, RANDOM], ids=["all", "random"])
def test_a_row_alone_and_inside_a_batch(nets, mode):
    for precision in PRECISIONS:
        full_v, full_p = evaluate_sym(nets[precision], BOARDS, mode)
        for g in (0, 15, 16, 32):
            v, p = evaluate_sym(nets[precision], BOARDS[g:g + 1], mode)
            same_bits(v, full_v[g:g + 1], "value of row %d" % g)
            same_bits(p, full_p[g:g + 1], "probs of row %d" % g)
        order = np.random.RandomState(5).permutation(33)
        v, p = evaluate_sym(nets[precision], BOARDS[order], mode)
        same_bits(v, full_v[order])
        same_bits(p, full_p[order])


def test_the_workspace_grows_and_is_reused():
    """a fresh handle: 2 rows, then 130 (ALL: 1 040 expanded rows, past the first block of 1 024), 2 again, 200, 130 -- every call the same bits as
    the calls before it, in both modes"""
    import torch
    from gomokuai_amd.network import FusedPolicyValueNetwork, PolicyValueNetwork
    G.init(0)
    boards = S.positions(200, 11)
    net = FusedPolicyValueNetwork(PolicyValueNetwork(seed=3).cuda().eval())
    try:
        assert evaluate_sym(net, boards[:0], ALL)[0].shape == (0,)                     # n = 0 before anything was allocated
        seen = {}
        for n in (2, 130, 2, 200, 130):
            for mode in (ALL, RANDOM):
                v, p = evaluate_sym(net, boards[:n], mode)
                if mode not in seen or len(seen[mode][0]) < n:
                    if mode in seen:
                        k = len(seen[mode][0])
                        same_bits(v[:k], seen[mode][0]); same_bits(p[:k], seen[mode][1])
                    seen[mode] = (v, p)
                else:
                    same_bits(v, seen[mode][0][:n], "n = %d" % n); same_bits(p, seen[mode][1][:n], "n = %d" % n)
        for mode in (NONE, ALL, RANDOM):
            assert evaluate_sym(net, boards[:0], mode)[1].shape == (0, N)              # n = 0 is a no-op
        pick = G.pvnet_sym_pick_host(boards, SEED)
        for a in range(8):                                                             # ... and they are the composition's bits
            rows = np.nonzero(pick == a)[0]
            v, q = net(dev(S.transform(boards[rows], a)))
            same_bits(seen[RANDOM][0][rows], v.cpu().numpy()); same_bits(seen[RANDOM][1][rows], S.back(q.cpu().numpy(), a))
        torch.cuda.synchronize()
    finally:
        net.close()


def test_errors_follow_the_plain_entry(nets):
    import torch
    L = G.load()
    x, v, p = dev(BOARDS[:2]), torch.zeros(2, device="cuda"), torch.zeros((2, N), device="cuda")
    h = nets["f32"].h
    stream = torch.cuda.current_stream().cuda_stream
    assert L.gmk_pvnet_evaluate_sym(None, x.data_ptr(), 2, ALL, SEED, v.data_ptr(), p.data_ptr(), stream) == ERR_ARG
    assert L.gmk_pvnet_evaluate_sym(h, None, 2, ALL, SEED, v.data_ptr(), p.data_ptr(), stream) == ERR_ARG
    assert L.gmk_pvnet_evaluate_sym(h, x.data_ptr(), 2, 3, SEED, v.data_ptr(), p.data_ptr(), stream) == ERR_ARG
    assert L.gmk_pvnet_evaluate_sym(h, x.data_ptr(), -2, RANDOM, SEED, v.data_ptr(), p.data_ptr(), stream) == ERR_ARG
    assert b"gmk_pvnet_evaluate_sym" in L.gmk_last_error()
    sd = nets["f32"].net.state_dict()
    host = lambda key, *shape: np.ascontiguousarray(sd[key].detach().float().cpu().numpy().reshape(*shape) if shape else sd[key].detach().float().cpu().numpy())
    arrays = [host("conv.0.weight"), host("conv.0.bias"), host("conv.1.weight"), host("conv.1.bias"), host("conv.2.weight"), host("conv.2.bias"),
              host("policy_conv.weight", 4, 128), host("policy_conv.bias"), host("value_conv.weight", 2, 128), host("value_conv.bias")]
    bare = C.c_void_p()
    G._check(L.gmk_pvnet_create(*[a.ctypes.data for a in arrays], C.byref(bare)))
    try:
        for mode in (NONE, ALL, RANDOM):                         # before gmk_pvnet_set_dense
            assert L.gmk_pvnet_evaluate_sym(bare, x.data_ptr(), 2, mode, SEED, v.data_ptr(), p.data_ptr(), stream) == ERR_STATE
    finally:
        L.gmk_pvnet_destroy(bare)
    torch.cuda.synchronize()
    assert not v.any() and not p.any()
    v2, p2 = evaluate_sym(nets["f32"], BOARDS[:2], ALL)          # the handle goes on
    assert np.isfinite(v2).all() and abs(p2.sum(axis=1) - 1).max() < 1e-5


def test_the_wrapper_follows_its_handle(nets):
    """symmetric() holds no weights of its own: set_precision on the fused network changes what it computes, and back"""
    import torch
    from gomokuai_amd.network import FusedPolicyValueNetwork, PolicyValueNetwork
    module = PolicyValueNetwork(seed=3).cuda().eval()
    fused = FusedPolicyValueNetwork(module)
    try:
        sym = fused.symmetric("all")
        x = dev(BOARDS[:5])
        v, p = sym(x)
        same_bits(v.cpu().numpy(), evaluate_sym(nets["f32"], BOARDS[:5], ALL)[0])
        fused.set_precision("bf16")
        v16, p16 = sym(x)
        same_bits(p16.cpu().numpy(), evaluate_sym(nets["bf16"], BOARDS[:5], ALL)[1])
        assert not torch.equal(p16, p)
        fused.set_precision("f32")
        assert torch.equal(sym(x)[1], p) and torch.equal(sym(x)[0], v)
        from gomokuai_amd import core
        board = core.Board()
        for cell in (112, 113, 97, 128):
            board.apply_move(core.Position(cell))
        value, probs = sym.eval_state(board)
        wv, wp = sym(dev(np.asarray(board.encoded_states(), np.float32)[None]))
        assert value == float(wv[0]) and probs.shape == (N,) and (probs == wp[0].cpu().numpy()).all()
    finally:
        fused.close()
