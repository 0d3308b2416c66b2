"""The host-form entries and the root read-outs on their one staging block (gomokuai_amd/csrc/host_staging.h).

The batch host forms (gmk_vcf_solve_host, gmk_vcf_defend_host, gmk_vcf_threats_host, gmk_vct_solve_host, gmk_pattern_policy_host,
gmk_eval_batch_host) against their device-pointer forms, byte for byte; their optional outputs through raw ctypes; n = 0; the inner error
text; and the root read-outs on a block that comes back from the library's pool filled with 0xA5.

The shapes put every part of a block behind padding: n in {1, 3, 5}, and stride in {7, 225} for the move lists, so that none of n * stride,
4 n and 225 n is a multiple of the 16 bytes the parts are aligned to."""
import numpy as np
import pytest

from gomokuai_amd import lib as G

pytestmark = pytest.mark.gpu

MAX_DEPTH, BUDGET = 4, 64
ERR_ARG, ERR_CAPACITY = -3, -5
CANARY = 0x5C
NS, STRIDES = (1, 3, 5), (7, 225)


@pytest.fixture(scope="module")
def gmk():
    G.init()
    return G


def cell(x, y):
    return y * 15 + x


# black's open three on row 7, black to move: a four, the answer, the five -- WIN in two moves, and a pv
FORCED = [cell(5, 7), cell(0, 0), cell(6, 7), cell(14, 14), cell(7, 7), cell(0, 14)]


def move_lists(n, stride):
    """n positions of at most six plies: the forced win first, then the synthetic boards' openings"""
    boards, lens, _ = G.synth_boards(max(n - 1, 1), 0)
    moves = np.zeros((n, stride), np.uint8)
    out_lens = np.zeros(n, np.int32)
    moves[0, :6], out_lens[0] = FORCED, 6
    for g in range(1, n):
        out_lens[g] = min(int(lens[g - 1]), 3 + g % 4)
        moves[g, :out_lens[g]] = boards[g - 1, :out_lens[g]]
    return moves, out_lens


# name -> (host entry, device entry, arguments between n and the outputs, outputs as (key, dtype, row width, required))
I32, U32, U8, F32 = np.int32, np.uint32, np.uint8, np.float32
FORMS = {
    "vcf_solve": ("gmk_vcf_solve_host", "gmk_vcf_solve", (MAX_DEPTH, BUDGET, 0),
                  (("status", I32, 1, False), ("move", I32, 1, False), ("length", I32, 1, False), ("nodes", U32, 1, False), ("pv", U8, 64, False))),
    "vcf_defend": ("gmk_vcf_defend_host", "gmk_vcf_defend", (MAX_DEPTH, BUDGET, 0),
                   (("threat_status", I32, 1, True), ("threat_length", I32, 1, True), ("threat_pv", U8, 64, True), ("threat_nodes", U32, 1, False),
                    ("verdict", U8, 225, True), ("length", U8, 225, False), ("nodes", U32, 225, False))),
    "vcf_threats": ("gmk_vcf_threats_host", "gmk_vcf_threats", (MAX_DEPTH, BUDGET, 0),
                    (("own_status", I32, 1, True), ("own_move", I32, 1, False), ("own_length", I32, 1, False), ("own_nodes", U32, 1, False),
                     ("own_pv", U8, 64, False), ("verdict", U8, 225, True), ("length", U8, 225, False), ("nodes", U32, 225, False))),
    "vct_solve": ("gmk_vct_solve_host", "gmk_vct_solve", (MAX_DEPTH, BUDGET, 0, 1, 64),
                  (("status", I32, 1, False), ("move", I32, 1, False), ("threats", I32, 1, False), ("positions", U32, 1, False), ("pv", U8, 80, False))),
    "pattern_policy": ("gmk_pattern_policy_host", "gmk_pattern_policy", (1,),
                       (("probs", F32, 225, False), ("value", F32, 1, False), ("best", I32, 1, False), ("status", I32, 1, False))),
    "eval_batch": ("gmk_eval_batch_host", "gmk_eval_batch", (),
                   (("scores", I32, 900, False), ("density", I32, 900, False), ("totals", U32, 11, False), ("status", I32, 1, False))),
}
CASES = [(name, n, stride) for name in FORMS for n in NS for stride in (STRIDES if name != "eval_batch" else (225,))]


def inputs_of(name, n, stride):
    """the input arrays of a form and its arguments up to and including n, given the inputs' addresses"""
    moves, lens = move_lists(max(n, 1), stride)
    if name == "eval_batch":
        planes = np.ascontiguousarray(G.moves_to_planes(moves, lens), dtype=np.uint16)
        return [planes], lambda ptrs: (ptrs[0], n)
    return [moves, lens], lambda ptrs: (ptrs[0], stride, ptrs[1], n)


def canaries(name, n):
    """an entry's output buffers, every byte CANARY (four rows for an empty batch, which must leave them alone)"""
    rows = n if n else 4
    return {key: np.full(rows * width * np.dtype(dtype).itemsize, CANARY, U8).view(dtype).reshape(rows, width) for key, dtype, width, _ in FORMS[name][3]}


def call_host(name, n, stride, absent=()):
    """-> (return code, the outputs: canary-filled where the entry wrote nothing)"""
    host, _, extra, outs = FORMS[name]
    arrays, head = inputs_of(name, n, stride)
    out = canaries(name, n)
    rc = getattr(G.load(), host)(*head([a.ctypes.data for a in arrays]), *extra, *[None if key in absent else out[key].ctypes.data for key, *_ in outs])
    return rc, out


def call_device(name, n, stride):
    import torch
    _, dev, extra, outs = FORMS[name]
    arrays, head = inputs_of(name, n, stride)
    d_in = [torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda() for a in arrays]
    d_out = {key: torch.from_numpy(v.view(U8)).cuda() for key, v in canaries(name, n).items()}
    rc = getattr(G.load(), dev)(*head([t.data_ptr() for t in d_in]), *extra, *[d_out[key].data_ptr() for key, *_ in outs],
                                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, {key: v.cpu().numpy() for key, v in d_out.items()}


@pytest.mark.parametrize("name,n,stride", CASES)
def test_host_form_is_the_device_form(gmk, name, n, stride):
    rc_host, host = call_host(name, n, stride)
    rc_dev, dev = call_device(name, n, stride)
    assert rc_host == 0 and rc_dev == 0, G.load().gmk_last_error()
    for key in host:
        assert host[key].tobytes() == dev[key].tobytes(), key
        assert not (host[key].view(U8) == CANARY).all(), key         # (it was written)
    if name == "vcf_solve":
        cells = 2 * int(host["length"][0, 0]) - 1                   # the forced win: a status, a first move and a line
        assert host["status"][0, 0] == G.VCF_WIN and cells >= 3 and host["pv"][0, 0] == host["move"][0, 0] and (host["pv"][0, cells:] == 255).all()
    if name == "vcf_threats":
        assert host["own_status"][0, 0] == G.VCF_WIN and host["own_pv"][0, 0] != 255


@pytest.mark.parametrize("name,n,stride", [(name, 3, 7 if name != "eval_batch" else 225) for name in FORMS])
def test_optional_outputs_may_be_null(gmk, name, n, stride):
    """every output present, then each optional one NULL in turn: the others do not change, and what is required stays required"""
    rc, full = call_host(name, n, stride)
    assert rc == 0
    for key, _, _, required in FORMS[name][3]:
        rc, part = call_host(name, n, stride, absent=(key,))
        if required:
            assert rc == ERR_ARG, key
            continue
        assert rc == 0, (key, G.load().gmk_last_error())
        for other in full:
            if other == key:
                assert (part[other].view(U8) == CANARY).all(), key
            else:
                assert part[other].tobytes() == full[other].tobytes(), (key, other)
    if not any(required for *_, required in FORMS[name][3]):
        rc, _ = call_host(name, n, stride, absent=tuple(key for key, *_ in FORMS[name][3]))
        assert rc == 0                                               # nothing asked for: nothing comes back


@pytest.mark.parametrize("name", list(FORMS))
def test_an_empty_batch_writes_nothing(gmk, name):
    rc, out = call_host(name, 0, 7)
    assert rc == 0
    for key in out:
        assert (out[key].view(U8) == CANARY).all(), key


def test_the_device_forms_error_text_survives_the_host_form(gmk):
    """More roots than a level may hold: gmk_vct_solve refuses with GMK_ERR_CAPACITY and its own words, and the host form hands both on."""
    n = (1 << 22) + 1
    moves, lens = np.zeros((n, 1), np.uint8), np.zeros(n, np.int32)
    rc = G.load().gmk_vct_solve_host(moves.ctypes.data, 1, lens.ctypes.data, n, MAX_DEPTH, BUDGET, 0, 1, 64, None, None, None, None, None)
    assert rc == ERR_CAPACITY
    assert G.load().gmk_last_error() == b"gmk_vct_solve: %d roots, more than %d" % (n, 1 << 22)


# ---------------- the root read-outs on a block that was used before ----------------
# The library's pool keeps blocks of 16 MiB = 16 777 216 bytes and more, and hands them out again uncleared (0xA5-filled under pool_poison).  A
# read-out's block is its parts, each rounded up to 16 bytes; with n a multiple of 64 nothing is rounded, a [n, 225] part of 4-byte words is
# 900 n bytes and an [n] part 4 n.  The smallest n, a multiple of 64, at which the parts alone fill a block of the pool's (K6's and K7's
# read-outs ask for 16 MiB at any n, so theirs is the pool's below that too; K3's is the pool's from here on):
#   K3  gmk_mcts_root_stats   900 n + 4 * 4 n = 916 n     >= 16 777 216  from n = 18 316: 18 368 = 287 * 64
#   K6  gmk_trad_root_stats   3 * 900 n + 3 * 4 n = 2 712 n              from n = 6 187:   6 208 = 97 * 64
#   K7  gmk_az_root_stats     3 * 900 n + 2 * 4 n = 2 708 n              from n = 6 196:   6 208
#   K6  gmk_trad_root_amaf    2 * 900 n = 1 800 n                        from n = 9 321:   9 344 = 146 * 64
POOL_MIN = 16 << 20
N_K3, N_K6, N_K7, N_AMAF = 18368, 6208, 6208, 9344
assert 916 * (N_K3 - 64) < POOL_MIN <= 916 * N_K3 and 2712 * (N_K6 - 64) < POOL_MIN <= 2712 * N_K6
assert 2708 * (N_K7 - 64) < POOL_MIN <= 2708 * N_K7 and 1800 * (N_AMAF - 64) < POOL_MIN <= 1800 * N_AMAF
POISON_WORD = 0xA5A5A5A5
NODES = 256                                                          # the smallest arena K6 and K7 accept


def root_position(n):
    """the same five-ply position in every game -> (moves u8[n, 225], lens, planes, the occupied cells)"""
    stones = [cell(7, 7), cell(8, 8), cell(6, 8), cell(8, 6), cell(9, 7)]
    moves = np.zeros((n, 225), np.uint8)
    moves[:, :5] = stones
    lens = np.full(n, 5, np.int32)
    return moves, lens, G.moves_to_planes(moves, lens), stones


def read_twice_under_poison(read):
    """read() twice with the pool's poison on: the first call's block goes to the pool, the second gets it back filled with 0xA5"""
    G.pool_poison(True)
    try:
        return read(), read()
    finally:
        G.pool_poison(False)


def check_cells(first, second, keys, stones):
    for key in first:
        assert first[key].tobytes() == second[key].tobytes(), key
    for key in keys:
        words = second[key].view(U32)
        assert not (words == POISON_WORD).any(), key                 # no cell shows what the block held before
        assert not words[:, stones].any(), key                       # a stone's cell has no child: 0
    assert (second["visits"].sum(axis=1, dtype=np.uint64) <= second["root_visits"]).all()      # the children's visits are visits of the root


def test_k3_root_stats_on_a_reused_block(gmk):
    tree = G.BatchedMCTS(N_K3, node_capacity=NODES)
    _, _, planes, stones = root_position(N_K3)
    tree.set_roots(planes, np.full(N_K3, stones[-1], np.int16))
    tree.run(2)
    names = ("visits", "root_value", "root_visits", "nodes", "status")
    first, second = read_twice_under_poison(lambda: dict(zip(names, tree.root_stats())))
    check_cells(first, second, ("visits",), stones)
    assert (second["root_visits"] > 0).all()
    tree.close()


def test_k6_root_stats_on_a_reused_block(gmk):
    tree = G.TraditionalMCTS(N_K6, node_capacity=NODES)
    moves, lens, _, stones = root_position(N_K6)
    tree.set_positions(moves, lens)
    tree.run(2)
    first, second = read_twice_under_poison(tree.root_stats)
    check_cells(first, second, ("visits", "values", "priors"), stones)
    assert (second["priors"] >= 0).all() and (second["priors"].sum(axis=1) > 0).all()      # the roots were expanded
    tree.close()


def test_k6_root_amaf_on_a_reused_block(gmk):
    tree = G.TraditionalRAVEMCTS(N_AMAF, node_capacity=NODES)
    moves, lens, _, stones = root_position(N_AMAF)
    tree.set_positions(moves, lens)
    tree.run(2)
    first, second = read_twice_under_poison(tree.root_stats)
    check_cells(first, second, ("visits", "values", "priors", "amaf_visits", "amaf_values"), stones)
    tree.close()


def test_k7_root_stats_on_a_reused_block(gmk):
    import torch
    tree = G.AlphaZeroMCTS(N_K7, node_capacity=NODES)
    _, _, planes, stones = root_position(N_K7)
    tree.set_roots(planes, np.tile(np.array([stones[-1], stones[-2]], np.int16), (N_K7, 1)))
    states = tree.select()                                           # fresh roots: the leaves are the roots
    rows = states.shape[0]
    tree.expand(torch.zeros(rows, dtype=torch.float32, device="cuda"), torch.full((rows, 225), 1.0 / 225, dtype=torch.float32, device="cuda"))
    torch.cuda.synchronize()
    first, second = read_twice_under_poison(tree.root_stats)
    check_cells(first, second, ("visits", "values", "priors"), stones)
    empty = np.setdiff1d(np.arange(225), stones)
    assert (second["priors"][:, empty] > 0).all()                    # every empty cell got a child with its share of the uniform priors
    tree.close()


def test_pattern_policy_on_a_reused_block(gmk):
    """gmk_pattern_policy_host asks for 16 MiB whatever the batch: its block is the pool's from the first call on."""
    moves, lens = move_lists(3, 7)
    first, second = read_twice_under_poison(lambda: G.pattern_policy(moves, lens))
    for key in first:
        assert first[key].tobytes() == second[key].tobytes(), key
        assert not (second[key].view(U32) == POISON_WORD).any(), key
