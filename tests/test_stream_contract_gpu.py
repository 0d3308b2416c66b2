"""Every stream-taking entry held to its stream, behind a delayed producer (tests/stream_harness.py).

Each scenario runs twice from the same initial state: eagerly, every call drained before the next, and on a non-blocking side stream behind a
delay, with no synchronisation added.  The outputs must be the same bits.  A launch that goes to another stream than the one it was given
(the NULL stream, say) runs during the delay, before its producers, and gives the answer for the wrong state; a stream-less reader that
does not wait for the device reads a tree its search has not written yet.

Stateless entries take the producer-decoy form: their input buffers hold a valid decoy, the real input arrives by a delayed copy on the side
stream, and their outputs are pre-filled by a delayed fill there, so that a launch elsewhere computes f(decoy) and is then overwritten.
Buffers a later call of the chain reads are not filled with a pattern: they keep what the eager warm-up on the decoy left there, so that
even a misplaced launch reads indices that are valid.  Handle chains put the calls that matter behind asynchronous producers of the same
segment: root noise behind the expand that makes the root's children, a reader straight behind a search."""
import numpy as np
import pytest

from gomokuai_amd import lib as G
from stream_harness import Call, Harness, Scenario

pytestmark = pytest.mark.gpu

N = 225
STD, COUNTER = 0, 1
cell = lambda y, x: 15 * y + x


@pytest.fixture(scope="module")
def H():
    G.init(0)
    h = Harness()
    yield h
    h.write()


@pytest.fixture(scope="module")
def nets():
    """{"f32", "bf16"}: the fused network in both precisions, and the module whose weights they hold"""
    import torch
    from gomokuai_amd.network import FusedPolicyValueNetwork, PolicyValueNetwork
    G.init(0)
    module = PolicyValueNetwork(seed=3).cuda().eval()
    out = {"module": module, "f32": FusedPolicyValueNetwork(module), "bf16": FusedPolicyValueNetwork(module, precision="bf16")}
    torch.cuda.synchronize()
    yield out
    out["f32"].close()
    out["bf16"].close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def fill(tensors, byte):
    for t in tensors:
        t.view(-1).view(_u8()).fill_(byte)


def _u8():
    import torch
    return torch.uint8


def flat(prefix, d):
    return {"%s.%s" % (prefix, k): v for k, v in d.items()}


def positions(n, max_len, first_board=500, stride=N):
    """n openings of 0 .. max_len moves -> moves u8[n, stride], lens i32[n], planes, the last two moves"""
    moves, lens, _ = G.synth_boards(n, 1, first_board=first_board, stride=stride)
    lens = np.array([min(int(lens[g]), (3 * g + 2) % (max_len + 1)) for g in range(n)], dtype=np.int32)
    for g in range(n):
        moves[g, lens[g]:] = 0
    planes = G.moves_to_planes(moves, lens)
    last = np.full((n, 2), -1, np.int16)
    for g in range(n):
        if lens[g] >= 1: last[g, 0] = moves[g, lens[g] - 1]
        if lens[g] >= 2: last[g, 1] = moves[g, lens[g] - 2]
    return moves, lens, planes, last


def stateless(inputs, finals, entry, waits=False, extra=()):
    """The producer-decoy form.  inputs: [(buffer, decoy, real)]; finals: the outputs no later call reads; entry(stream): the call(s) under test,
    a Call or a list of Calls; extra: further tensors to compare (outputs that a later call of the chain reads)."""
    import torch
    entries = entry if isinstance(entry, (list, tuple)) else [Call(entry, waits)]

    def make():
        for buf, decoy, _ in inputs:
            buf.copy_(decoy)
        torch.cuda.synchronize()
        for c in entries:                                        # f(decoy), eagerly: first-call allocations happen here, and every buffer holds a valid state
            c.fn(torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
        for buf, decoy, _ in inputs:                             # (an entry may work in place)
            buf.copy_(decoy)
        fill(finals, 0x11)
        calls = [Call(lambda s: [buf.copy_(real, non_blocking=True) for buf, _, real in inputs]), Call(lambda s: fill(finals, 0x5A))] + list(entries)
        return Scenario(calls, lambda: {"out%d" % i: t for i, t in enumerate(list(finals) + list(extra) + [b for b, _, _ in inputs])})
    return make


# ---------------------------------------------------------------- the sensitivity check ----------------------------------------------------------------
def _eval_buffers(n):
    import torch
    return (torch.zeros((n, 4, N), dtype=torch.int32, device="cuda"), torch.zeros((n, 2, 2, N), dtype=torch.int32, device="cuda"),
            torch.zeros((n, 11), dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda"))


def _eval_case():
    n = 37                                                       # one full group of boards and a partial one
    real, decoy = dev(G.synth_boards(n, 1, first_board=42)[2].view(np.int16)), dev(G.synth_boards(n, 1, first_board=4242)[2].view(np.int16))
    buf, outs = real.clone(), _eval_buffers(n)
    entry = lambda s: G.eval_batch(buf.data_ptr(), n, *[o.data_ptr() for o in outs], s)
    return buf, decoy, real, outs, entry


def _pvnet_case(net, n=17, forward=False):                       # one dense group of 16 rows and one more
    import torch
    g = torch.Generator(device="cuda").manual_seed(9)
    real = (torch.rand((n, 6, 15, 15), generator=g, device="cuda") > 0.6).float()
    decoy = (torch.rand((n, 6, 15, 15), generator=g, device="cuda") > 0.6).float()
    buf = real.clone()
    outs = (torch.zeros((n, 900), device="cuda"), torch.zeros((n, 450), device="cuda")) if forward else (torch.zeros(n, device="cuda"), torch.zeros((n, N), device="cuda"))
    fn = G.load().gmk_pvnet_forward if forward else G.load().gmk_pvnet_evaluate
    entry = lambda s: G._check(fn(net.h, buf.data_ptr(), n, outs[0].data_ptr(), outs[1].data_ptr(), s))
    return buf, decoy, real, outs, entry


def test_a_misplaced_eval_batch_is_seen(H):
    buf, decoy, real, outs, entry = _eval_case()
    H.sensitivity("gmk_eval_batch", buf, decoy, real, entry, lambda: {"out%d" % i: o for i, o in enumerate(outs)})


def test_a_misplaced_pvnet_evaluate_is_seen(H, nets):
    buf, decoy, real, outs, entry = _pvnet_case(nets["f32"])
    H.sensitivity("gmk_pvnet_evaluate", buf, decoy, real, entry, lambda: {"value": outs[0], "probs": outs[1]})


# ---------------------------------------------------------------- stateless entries ----------------------------------------------------------------
def test_eval_batch(H):
    buf, decoy, real, outs, entry = _eval_case()
    H.check("gmk_eval_batch", stateless([(buf, decoy, real)], outs, entry))


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("forward", [False, True], ids=["evaluate", "forward"])
def test_pvnet(H, nets, precision, forward):
    buf, decoy, real, outs, entry = _pvnet_case(nets[precision], forward=forward)
    H.check("gmk_pvnet_%s[%s]" % ("forward" if forward else "evaluate", precision), stateless([(buf, decoy, real)], outs, entry))


def test_pattern_policy_and_play(H):
    import torch
    n = 5
    moves, lens, _, _ = positions(n, 14, first_board=90)
    dm, dl, _, _ = positions(n, 14, first_board=190)
    b_moves, b_lens = dev(moves), dev(lens)
    outs = (torch.zeros((n, N), device="cuda"), torch.zeros(n, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda"))
    entry = lambda s: G.pattern_policy_device(b_moves.data_ptr(), N, b_lens.data_ptr(), n, True, *[o.data_ptr() for o in outs], s)
    H.check("gmk_pattern_policy", stateless([(b_moves, dev(dm), dev(moves)), (b_lens, dev(dl), dev(lens))], outs, entry))
    n = 3                                                        # whole games in place, cut at twelve more plies
    p_moves, p_lens = dev(moves[:n]), dev(lens[:n])
    outs = (torch.zeros(n, dtype=torch.int8, device="cuda"), torch.zeros((n, N), device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda"))
    entry = lambda s: G.pattern_play(p_moves.data_ptr(), p_lens.data_ptr(), n, True, 12, *[o.data_ptr() for o in outs], s)
    H.check("gmk_pattern_play", stateless([(p_moves, dev(dm[:n]), dev(moves[:n])), (p_lens, dev(dl[:n]), dev(lens[:n]))], outs, entry))


def _records(n, seed, lens):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    moves = torch.argsort(torch.rand((n, N), generator=g, device="cuda"), dim=1).to(torch.uint8)
    winner = torch.randint(-1, 2, (n,), generator=g, device="cuda", dtype=torch.int8)
    visits = torch.randint(0, 1000, (n, N, N), generator=g, device="cuda", dtype=torch.int16)
    return moves, torch.tensor(lens, dtype=torch.int32, device="cuda"), winner, visits


def test_records_wire_and_samples(H):
    """gmk_records_scan, _pack, _unpack, gmk_samples_from_records and _from_packed as one chain on the stream: 3 games, 8 samples, augment on.
    The decoy games have the real games' lengths (other moves, winners and visit counts), so that offsets and sample lists fit both."""
    import torch
    n, lens = 3, [40, 7, 225]
    real, decoy = _records(n, 5, lens), _records(n, 6, lens)
    rec = [t.clone() for t in real]
    total = sum(lens)
    n_bytes = 5 * n + total * 451
    offsets, packed, status = torch.zeros(n + 1, dtype=torch.int64, device="cuda"), torch.zeros(n_bytes + 3, dtype=torch.uint8, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
    up = (torch.zeros((n, N), dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int8, device="cuda"),
          torch.zeros((n, N, N), dtype=torch.int16, device="cuda"))
    up_offsets = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    s_game = torch.tensor([0, 0, 1, 1, 2, 2, 2, 2], dtype=torch.int32, device="cuda")
    s_move = torch.tensor([0, 39, 3, 6, 0, 100, 223, 224], dtype=torch.int32, device="cuda")
    S = 8 * 8
    samples = [(torch.zeros((S, 6, N), dtype=torch.uint8, device="cuda"), torch.zeros(S, device="cuda"), torch.zeros((S, N), device="cuda")) for _ in range(2)]
    p = lambda t: t.data_ptr()
    entries = [Call(lambda s: G.records_scan(p(rec[1]), n, p(offsets), s)),
               Call(lambda s: G.records_pack(p(rec[0]), p(rec[1]), p(rec[2]), p(rec[3]), n, p(offsets), p(packed), n_bytes, p(status[:1]), s)),
               Call(lambda s: G.records_unpack(p(packed), n_bytes, n, True, p(up_offsets), p(up[0]), p(up[1]), p(up[2]), p(up[3]), p(status[1:]), s)),
               Call(lambda s: G.samples_from_records(p(rec[0]), p(rec[1]), p(rec[3]), p(rec[2]), p(s_game), p(s_move), 8, 1, *[p(t) for t in samples[0]], s)),
               Call(lambda s: G.samples_from_packed(p(packed), n, p(offsets), p(s_game), p(s_move), 8, 1, *[p(t) for t in samples[1]], s))]
    finals = list(up) + list(samples[0]) + list(samples[1]) + [status]
    H.check("gmk_records_* + gmk_samples_*", stateless([(b, d, r) for b, d, r in zip(rec, decoy, real)], finals, entries, extra=[offsets, packed, up_offsets]))
    # the scan on lengths that differ between decoy and real: its offsets are a final output here
    b_lens, offs = rec[1], torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    H.check("gmk_records_scan", stateless([(b_lens, torch.tensor([1, 225, 0], dtype=torch.int32, device="cuda"), real[1])], [offs],
                                          lambda s: G.records_scan(p(b_lens), n, p(offs), s)))


def _vcf_positions():
    """four roots with fours and threes on the board, and four others as the decoy: move lists, black first"""
    inter = lambda b, w: [c for pair in zip(b, w) for c in pair] + list(b[len(w):])
    real = [inter([cell(7, 5), cell(7, 6), cell(7, 7), cell(7, 8)], [cell(0, 0), cell(0, 2), cell(0, 4)]),                      # white faces an open four
            inter([cell(7, 5), cell(7, 6), cell(7, 7)], [cell(0, 0), cell(0, 2), cell(0, 4)]),                                  # black to move with an open three
            inter([cell(3, 3), cell(4, 4), cell(5, 5), cell(9, 9), cell(9, 10)], [cell(3, 4), cell(4, 5), cell(5, 6), cell(6, 7), cell(14, 14)]),
            inter([cell(7, 7), cell(8, 8), cell(6, 6), cell(2, 2)], [cell(7, 8), cell(8, 9), cell(6, 7), cell(5, 6)])]
    decoy = [inter([cell(10, 4), cell(10, 5), cell(10, 6)], [cell(1, 1), cell(1, 3)]),
             inter([cell(2, 7), cell(3, 7), cell(4, 7), cell(5, 7)], [cell(12, 0), cell(12, 2), cell(12, 4), cell(6, 7)]),
             [cell(7, 7)],
             inter([cell(4, 10), cell(5, 9), cell(6, 8)], [cell(0, 0), cell(0, 1), cell(0, 3)])]

    def pack(lists):
        moves, lens = np.zeros((len(lists), 16), np.uint8), np.array([len(l) for l in lists], np.int32)
        for i, l in enumerate(lists):
            moves[i, :len(l)] = l
        return dev(moves), dev(lens)
    return pack(real), pack(decoy)


def test_vcf_solvers(H):
    import torch
    (r_moves, r_lens), (d_moves, d_lens) = _vcf_positions()
    n, stride = 4, 16
    moves, lens = r_moves.clone(), r_lens.clone()
    inputs = [(moves, d_moves, r_moves), (lens, d_lens, r_lens)]
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device="cuda")
    u8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device="cuda")
    p = lambda t: t.data_ptr()
    outs = [i32(n), i32(n), i32(n), i32(n), u8(n, 64)]
    H.check("gmk_vcf_solve", stateless(inputs, outs, lambda s: G.vcf_solve_device(p(moves), stride, p(lens), n, 8, 200, False, True, *[p(o) for o in outs], s)))
    outs = [i32(n), i32(n), u8(n, 64), i32(n), u8(n, N), u8(n, N), i32(n, N)]
    H.check("gmk_vcf_defend", stateless(inputs, outs, lambda s: G.vcf_defend_device(p(moves), stride, p(lens), n, 6, 40, False, *[p(o) for o in outs], s)))
    outs = [i32(n), i32(n), i32(n), i32(n), u8(n, 64), u8(n, N), u8(n, N), i32(n, N)]
    H.check("gmk_vcf_threats", stateless(inputs, outs, lambda s: G.vcf_threats_device(p(moves), stride, p(lens), n, 6, 40, False, *[p(o) for o in outs], s)))
    n = 2                                                        # gmk_vct_solve waits for its stream between the levels: one segment
    outs = [i32(n), i32(n), i32(n), i32(n), u8(n, 80)]
    H.check("gmk_vct_solve", stateless([(moves, d_moves, r_moves), (lens, d_lens, r_lens)], outs,
                                       lambda s: G.vct_solve_device(p(moves), stride, p(lens), n, 6, 40, False, 1, 256, *[p(o) for o in outs], s), waits=True))


def test_train_kernels(H):
    import torch
    g = torch.Generator(device="cuda").manual_seed(21)
    rnd = lambda *shape: torch.randn(shape, generator=g, device="cuda")
    M, Nn, K = 19, 33, 70                                        # no multiple of a tile, two column tiles
    a_real, a_decoy, b = rnd(M, K), rnd(M, K), rnd(K, Nn)
    a, c = a_real.clone(), torch.zeros((M, Nn), device="cuda")
    desc = G.train_gemm_desc(A=a, sam=K, sak=1, B=b, sbk=Nn, sbn=1, M=M, N=Nn, K=K, C=c, ldc=Nn)
    H.check("gmk_train_kernel_gemm", stateless([(a, a_decoy, a_real)], [c], lambda s: G.train_kernel_gemm(desc, s)))
    nz, mn = 3, 1125
    part_real, part_decoy = rnd(nz * mn), rnd(nz * mn)
    part, out = part_real.clone(), torch.zeros(mn, device="cuda")
    H.check("gmk_train_kernel_reduce", stateless([(part, part_decoy, part_real)], [out], lambda s: G.train_kernel_reduce(part, nz, mn, out, s)))
    Cc, npos = 5, 3
    in_real, in_decoy = rnd(npos * N * Cc), rnd(npos * N * Cc)
    inp, col = in_real.clone(), torch.zeros(npos * N * 9 * Cc, device="cuda")
    H.check("gmk_train_kernel_im2col", stateless([(inp, in_decoy, in_real)], [col], lambda s: G.train_kernel_im2col(inp, npos * N * Cc, N * Cc, Cc, 1, Cc, npos, col, s)))
    d_real, d_decoy, mask = rnd(npos * N * 9 * Cc), rnd(npos * N * 9 * Cc), rnd(npos * N * Cc)
    dcol, out2 = d_real.clone(), torch.zeros(npos * N * Cc, device="cuda")
    H.check("gmk_train_kernel_col2im", stateless([(dcol, d_decoy, d_real)], [out2], lambda s: G.train_kernel_col2im(dcol, Cc, npos, mask, out2, s)))


def test_match_referee(H):
    import torch
    n = 4
    moves, lens, _, _ = positions(n, 9, first_board=700)
    free = [[c for c in range(N) if c not in set(moves[g, :lens[g]].tolist())] for g in range(n)]
    real = torch.tensor([free[g][3 * g] for g in range(n)], dtype=torch.int16, device="cuda")
    decoy = torch.tensor([free[g][50 + g] for g in range(n)], dtype=torch.int16, device="cuda")
    rows_real = torch.arange(n * N, device="cuda").reshape(n, N).to(torch.int16)
    rows_decoy = rows_real.flip(1).contiguous()
    cells, rows = real.clone(), rows_real.clone()
    rec0 = (dev(moves), dev(lens), torch.zeros(n, dtype=torch.int8, device="cuda"), torch.zeros((n, N, N), dtype=torch.int16, device="cuda"))
    rec = [t.clone() for t in rec0]
    verdict, status, unfinished = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    zero = torch.zeros(n, dtype=torch.int32, device="cuda")
    # the records and the verdicts are read and written: each is its own input, put back to the opening before every run
    inputs = [(cells, decoy, real), (rows, rows_decoy, rows_real)] + [(b, r, r) for b, r in zip(rec, rec0)] + [(verdict, zero, zero), (status, zero, zero)]
    H.check("gmk_match_referee", stateless(inputs, [unfinished], lambda s: G.match_referee(cells, rows, None, rec[0], rec[1], rec[2], rec[3], verdict, status, unfinished, s)))


# ---------------------------------------------------------------- handle chains ----------------------------------------------------------------
def test_evalstate_updates_then_read(H):
    """K2: three updates whose move buffers are produced on the stream, then the stream-less read"""
    import torch
    n, k = 6, 4
    moves, lens, _, _ = positions(n, 12, first_board=300)
    real = [np.full((n, k), -1, np.int16) for _ in range(3)]
    for g in range(n):
        seq = list(moves[g, :12]) if lens[g] >= 12 else list(moves[g, :lens[g]]) + [-1] * (12 - lens[g])
        for i in range(3):
            real[i][g] = seq[4 * i:4 * i + 4]
    real[2][:, 3] = -2                                           # ... and the last move of every game is taken back
    real[2][lens < 11, 3] = -1
    real_d = [dev(r) for r in real]
    nothing = torch.full((n, k), -1, dtype=torch.int16, device="cuda")

    def make():
        es = G.EvaluatorStates(n)
        bufs = [nothing.clone() for _ in range(3)]
        host = {}
        calls = []
        for i in range(3):
            calls.append(Call(lambda s, i=i: bufs[i].copy_(real_d[i], non_blocking=True)))
            calls.append(Call(lambda s, i=i: G._check(G.load().gmk_evalstate_update(es.h, bufs[i].data_ptr(), k, s))))
        calls.append(Call(lambda s: host.update(es.read()), waits=True))
        return Scenario(calls, lambda: host, es.close)
    out = H.check("gmk_evalstate_update x 3 + read", make)
    assert out["record"].any()


def _k3_records(n):
    import torch
    return (torch.zeros((n, N), dtype=torch.uint8, device="cuda"), torch.zeros((n, N, N), dtype=torch.int16, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda"),
            torch.zeros(n, dtype=torch.int8, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"))


@pytest.mark.parametrize("reuse", [False, True], ids=["fresh", "reuse"])
@pytest.mark.parametrize("sampler", [STD, COUNTER], ids=["std", "counter"])
def test_k3_noise_run_advance(H, sampler, reuse):
    """K3: add_root_noise -> run -> advance for three plies on the stream, a forced gmk_mcts_step whose moves are produced there, and the root
    statistics, which wait for the stream of the handle's last call"""
    import torch
    n, playouts = 6, 64
    moves, lens, planes, last = positions(n, 10, first_board=40)
    forced_real = torch.full((n,), -1, dtype=torch.int16, device="cuda")
    forced_real[0], forced_real[3] = cell(0, 14), cell(14, 0)

    def make():
        tree = G.BatchedMCTS(n, playouts_capacity=4 * playouts, seed=11)
        tree.set_option(G.OPT_NOISE_SAMPLER, sampler)
        tree.set_roots(planes, last[:, 0], first_game_id=70)
        rec = _k3_records(n)
        rec[0].copy_(dev(moves)); rec[2].copy_(dev(lens))
        forced = torch.full((n,), cell(7, 7) + 1, dtype=torch.int16, device="cuda")       # the decoy: another legal request
        ptrs = [t.data_ptr() for t in rec]
        host, calls = {}, []
        for _ in range(3):
            calls.append(Call(lambda s: tree.add_root_noise(0.3, 0.25, s), waits=sampler == STD))     # (the std sampler draws on the host)
            calls.append(Call(lambda s: tree.run(playouts, s)))
            calls.append(Call(lambda s: tree.advance(*ptrs, reuse, s)))
        calls.append(Call(lambda s: tree.run(playouts, s)))
        calls.append(Call(lambda s: forced.copy_(forced_real, non_blocking=True)))
        calls.append(Call(lambda s: tree.step(forced.data_ptr(), *ptrs, reuse, s)))
        calls.append(Call(lambda s: tree.run(playouts, s)))
        calls.append(Call(lambda s: host.update({"stats%d" % i: a for i, a in enumerate(tree.root_stats())}), waits=True))
        return Scenario(calls, lambda: dict(host, **{"rec%d" % i: t for i, t in enumerate(rec)}), tree.close)
    out = H.check("K3 noise/run/advance x 3 + step [%s, %s]" % ("counter" if sampler else "std", "reuse" if reuse else "fresh"), make)
    assert out["stats2"].view(np.uint32).sum() > 0               # root visits: the last search ran


@pytest.mark.parametrize("lockstep", [0, 1], ids=["persistent", "lockstep"])
def test_k3_selfplay_run(H, lockstep):
    """gmk_selfplay_run on the stream, its record buffers zeroed by a delayed fill there: 4 whole games (one call that waits: one segment)"""
    n, playouts = 4, 20

    def make():
        tree = G.BatchedMCTS(2, playouts_capacity=3 * playouts, seed=5)
        tree.set_option(G.OPT_NOISE_SAMPLER, COUNTER)
        tree.set_option(G.OPT_LOCKSTEP, lockstep)
        rec = _k3_records(n)[:4]
        fill(rec, 0x77)
        host = {}
        calls = [Call(lambda s: fill(rec, 0)),
                 Call(lambda s: host.update(steps=tree.selfplay_run(n, 900, playouts, *[t.data_ptr() for t in rec], reuse_subtree=True, root_noise=(0.3, 0.25), stream=s)), waits=True)]
        return Scenario(calls, lambda: dict(host, **{"rec%d" % i: t for i, t in enumerate(rec)}), tree.close)
    out = H.check("gmk_selfplay_run [%s]" % ("lockstep" if lockstep else "persistent"), make)
    assert (out["rec2"].view(np.int32) > 0).all()


TRAD = {"trad": lambda n: G.TraditionalMCTS(n, node_capacity=1 << 18), "rave": lambda n: G.TraditionalRAVEMCTS(n, node_capacity=1 << 18),
        "poolrave": lambda n: G.PoolRAVEMCTS(n, node_capacity=1 << 18, seed=3, first_game_id=50)}


@pytest.mark.parametrize("sampler", [STD, COUNTER], ids=["std", "counter"])
@pytest.mark.parametrize("kind", sorted(TRAD))
def test_k6_k8_chain(H, kind, sampler):
    """K6 / K6 + RAVE / K8: root noise between two runs with no step between them (the first run makes the children the noise needs), the
    stream-less root statistics straight behind a run, root_choice and step_device from device memory, and gmk_trad_step"""
    import torch
    n, playouts = 4, 200
    moves, lens, _, _ = positions(n, 8, first_board=20)

    def make():
        tree = TRAD[kind](n)
        tree.set_option(G.OPT_NOISE_SAMPLER, sampler)
        tree.set_positions(moves, lens)
        cells, rows, verdict = torch.full((n,), -1, dtype=torch.int16, device="cuda"), torch.zeros((n, N), dtype=torch.int16, device="cuda"), torch.ones(n, dtype=torch.int32, device="cuda")
        host = {}
        calls = [Call(lambda s: tree.run(playouts, s)),
                 Call(lambda s: tree.add_root_noise(0.3, 0.25, seed=9, first_game_id=50, stream=s), waits=sampler == STD),
                 Call(lambda s: tree.run(playouts, s)),
                 Call(lambda s: host.update(flat("a", tree.root_stats())), waits=True),
                 Call(lambda s: tree.root_choice(cells, rows, s)),
                 Call(lambda s: verdict.zero_()),                 # every game MOVED: produced on the stream as the referee would
                 Call(lambda s: tree.step_device(cells, verdict, False, s)),
                 Call(lambda s: tree.run(playouts, s)),
                 Call(lambda s: tree.step(None), waits=True),
                 Call(lambda s: tree.run(playouts, s)),
                 Call(lambda s: host.update(flat("b", tree.root_stats())), waits=True)]
        return Scenario(calls, lambda: dict(host, cells=cells, rows=rows), tree.close)
    out = H.check("K6/K8 run/noise/run/root_stats/root_choice/step_device/step [%s, %s]" % (kind, "counter" if sampler else "std"), make)
    assert out["a.priors"].any() and not out["a.status"].any() and out["b.root_visits"].view(np.uint32).min() >= playouts


@pytest.mark.parametrize("persistent", [True, False], ids=["persistent", "lockstep"])
def test_trad_selfplay_run(H, persistent):
    n, playouts = 4, 20

    def make():
        tree = G.TraditionalMCTS(2, node_capacity=1 << 14)
        tree.set_option(G.OPT_NOISE_SAMPLER, COUNTER)
        rec = _k3_records(n)[:4]
        fill(rec, 0x77)
        host = {}
        ptrs = [t.data_ptr() for t in rec]
        calls = [Call(lambda s: fill(rec, 0)),
                 Call(lambda s: host.update(run=np.array(tree.selfplay_run(n, 900, playouts, *ptrs, reuse_subtree=True, root_noise=(0.3, 0.25), seed=17, stream=s,
                                                                           persistent=persistent), dtype=np.int64)), waits=True)]
        return Scenario(calls, lambda: dict(host, **{"rec%d" % i: t for i, t in enumerate(rec)}), tree.close)
    out = H.check("gmk_trad_selfplay_run [%s]" % ("persistent" if persistent else "lockstep"), make)
    assert (out["rec2"].view(np.int32) > 0).all()


def _evaluate(net, states, rows, value, probs, stream):
    G._check(G.load().gmk_pvnet_evaluate(net.h, states.data_ptr(), rows, value.data_ptr(), probs.data_ptr(), stream))


def _k7(net, sampler, leaves, solver):
    import torch
    n, cap = 6, 4096
    moves, lens, planes, last = positions(n, 12)
    options = dict(vcf_depth=4, vcf_budget=64, proof=True, vcf_defend=True) if solver else {}

    def make():
        tree = G.AlphaZeroMCTS(n, node_capacity=cap, c_puct=5.0, leaves=leaves, **options)
        tree.set_option(G.OPT_NOISE_SAMPLER, sampler)
        tree.set_roots(planes, last)
        value, probs = torch.zeros(n * leaves, device="cuda"), torch.zeros((n * leaves, N), device="cuda")
        for live in range(n, 0, -1):                             # the first call of a batch size waits for its stream: made here
            _evaluate(net, tree.states, live * leaves, value, probs, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        value.zero_(); probs.zero_()
        cells, rows, verdict = torch.full((n,), -1, dtype=torch.int16, device="cuda"), torch.zeros((n, N), dtype=torch.int16, device="cuda"), torch.ones(n, dtype=torch.int32, device="cuda")
        rec = (dev(moves), torch.zeros((n, N, N), dtype=torch.int16, device="cuda"), dev(lens), torch.zeros(n, dtype=torch.int8, device="cuda"))
        host, calls = {}, []
        noise = lambda: calls.append(Call(lambda s: tree.add_root_noise(0.3, 0.25, seed=777, first_game_id=20, stream=s), waits=sampler == STD))

        def playouts(k, then=None):
            """k playouts per game: k select / evaluate / expand steps, or with several leaves a quota and k / leaves steps; `then` after the first"""
            if leaves > 1:
                calls.append(Call(lambda s: tree.add_playouts(k, s)))
            for i in range(-(-k // leaves)):
                calls.append(Call(lambda s: tree.select(s)))
                calls.append(Call(lambda s: _evaluate(net, tree.states, tree.live * leaves, value, probs, s)))
                calls.append(Call(lambda s: tree.expand(value[:tree.live * leaves], probs[:tree.live * leaves], s)))
                if i == 0 and then is not None:
                    then()
        playouts(24, then=noise)                                 # the noise needs the children the first expand makes
        if leaves > 1:
            calls.append(Call(lambda s: host.update(owed=tree.playouts_owed(s)), waits=True))
        calls.append(Call(lambda s: host.update(flat("a", tree.root_stats())), waits=True))       # stream-less readers straight behind asynchronous work
        playouts(4)
        calls.append(Call(lambda s: host.update(flat("proofs", tree.root_proofs())), waits=True))
        playouts(4)
        calls.append(Call(lambda s: tree.step(None), waits=True))                                # gmk_az_step: stream-less as well
        noise()                                                  # ... and on the kept subtree
        playouts(8)
        calls.append(Call(lambda s: tree.root_choice(cells, rows, s)))
        calls.append(Call(lambda s: verdict.zero_()))
        calls.append(Call(lambda s: host.update(live=tree.step_device(cells, verdict, False, None, s) or tree.live), waits=True))
        playouts(8)
        calls.append(Call(lambda s: host.update(unfinished=tree.advance(rec[0], rec[1], rec[2], rec[3], True, s)), waits=True))
        playouts(4)
        calls.append(Call(lambda s: host.update(flat("b", tree.root_stats())), waits=True))
        outputs = lambda: dict(host, value=value, probs=probs, states=tree.states, cells=cells, rows=rows, **{"rec%d" % i: t for i, t in enumerate(rec)})
        return Scenario(calls, outputs, tree.close)
    return make


@pytest.mark.parametrize("sampler", [STD, COUNTER], ids=["std", "counter"])
@pytest.mark.parametrize("leaves,solver", [(1, False), (4, False), (4, True)], ids=["L1", "L4", "L4-solver"])
def test_k7_with_k9_as_the_evaluator(H, nets, leaves, solver, sampler):
    """K7 with K9 on the same stream: select -> gmk_pvnet_evaluate -> expand per playout; root noise behind the first expand and again behind a
    gmk_az_step; gmk_az_root_stats, gmk_az_root_proofs and gmk_az_step straight behind asynchronous work; root_choice, step_device, advance.
    With the solver, the proofs and the defence on, the az_*_leaves kernels ride behind every select."""
    out = H.check("K7 + K9 [%s, %s]" % ("L%d%s" % (leaves, "-solver" if solver else ""), "counter" if sampler else "std"), _k7(nets["f32"], sampler, leaves, solver))
    assert out["a.priors"].any() and (out["a.root_visits"].view(np.uint32) >= 16).all()        # (4096 nodes: the arenas fill up near 18 expansions)


def test_replay_trainer_network(H, nets):
    """Replay -> K11 -> K9: append -> sample -> three training steps -> export -> evaluate, all on the stream"""
    import torch
    from gomokuai_amd.network import FusedPolicyValueNetwork, module_arrays
    n, batch = 3, 8
    lens = [40, 7, 225]
    rec_real, rec_decoy = _records(n, 5, lens), _records(n, 6, lens)
    p = lambda t: t.data_ptr()

    def make():
        replay = G.ReplayHandle(4096, 16, seed=3)
        trainer = G.TrainerHandle(module_arrays(nets["module"]), batch)
        net = FusedPolicyValueNetwork(nets["module"])
        rec = [t.clone() for t in rec_decoy]
        states, values, pi = torch.zeros((batch, 6, N), device="cuda"), torch.zeros(batch, device="cuda"), torch.zeros((batch, N), device="cuda")
        picked, status = torch.zeros((batch, 3), dtype=torch.int64, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
        probs_out, metrics = torch.zeros((3, batch, N), device="cuda"), torch.zeros((3, 5), device="cuda")
        value, probs = torch.zeros(batch, device="cuda"), torch.zeros((batch, N), device="cuda")
        _evaluate(net, states, batch, value, probs, torch.cuda.current_stream().cuda_stream)      # (the first call of a batch size waits)
        torch.cuda.synchronize()
        host = {}
        calls = [Call(lambda s: [b.copy_(r, non_blocking=True) for b, r in zip(rec, rec_real)]),
                 Call(lambda s: replay.append(p(rec[0]), p(rec[1]), p(rec[2]), p(rec[3]), n, 0, p(status[:1]), s)),
                 Call(lambda s: replay.sample(batch, 0, True, True, p(states), p(values), p(pi), p(picked), p(status[1:]), s))]
        for i in range(3):
            calls.append(Call(lambda s, i=i: trainer.step(p(states), p(values), p(pi), batch, 2e-3, None, p(probs_out[i]), p(metrics[i]), s)))
        calls.append(Call(lambda s: trainer.export(net.h, s), waits=True))                        # (it reads four bytes back: it returns behind the stream)
        calls.append(Call(lambda s: _evaluate(net, states, batch, value, probs, s)))
        calls.append(Call(lambda s: host.update(flat("params", trainer.params())), waits=True))

        def close():
            replay.close(); trainer.close(); net.close()
        return Scenario(calls, lambda: dict(host, states=states, values=values, pi=pi, picked=picked, status=status, probs_out=probs_out, metrics=metrics, value=value, probs=probs), close)
    out = H.check("replay append/sample -> gmk_train_step x 3 -> export -> gmk_pvnet_evaluate", make)
    assert not out["status"].any() and out["pi"].any()


def test_k12_match_plies(H, nets):
    """Three plies of a match, K7 against K6: search, root_choice -> gmk_match_referee -> step_device of both trees, all on the stream"""
    import torch
    n = 4
    moves, lens, planes, last = positions(n, 0, first_board=60)   # empty boards: the network's side has black
    net = nets["f32"]

    def make():
        az = G.AlphaZeroMCTS(n, node_capacity=4096)
        az.set_option(G.OPT_NOISE_SAMPLER, COUNTER)
        az.set_roots(planes, last)
        tr = G.TraditionalMCTS(n, node_capacity=1 << 14)
        tr.set_positions(moves, lens)
        value, probs = torch.zeros(n, device="cuda"), torch.zeros((n, N), device="cuda")
        for live in range(n, 0, -1):
            _evaluate(net, az.states, live, value, probs, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        cells, rows = torch.full((n,), -1, dtype=torch.int16, device="cuda"), torch.zeros((n, N), dtype=torch.int16, device="cuda")
        rec = (dev(moves), dev(lens), torch.zeros(n, dtype=torch.int8, device="cuda"), torch.zeros((n, N, N), dtype=torch.int16, device="cuda"))
        verdict, status, unfinished = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
        host, calls = {}, []
        for ply in range(3):
            if ply % 2 == 0:
                for i in range(12):
                    calls.append(Call(lambda s: az.select(s)))
                    calls.append(Call(lambda s: _evaluate(net, az.states, az.live, value, probs, s)))
                    calls.append(Call(lambda s: az.expand(value[:az.live], probs[:az.live], s)))
                calls.append(Call(lambda s: az.root_choice(cells, rows, s)))
            else:
                calls.append(Call(lambda s: tr.run(100, s)))
                calls.append(Call(lambda s: tr.root_choice(cells, rows, s)))
            calls.append(Call(lambda s: G.match_referee(cells, rows, None, rec[0], rec[1], rec[2], rec[3], verdict, status, unfinished, s)))
            calls.append(Call(lambda s: tr.step_device(cells, verdict, False, s)))
            calls.append(Call(lambda s, ply=ply: host.update({"unfinished%d" % ply: az.step_device(cells, verdict, False, unfinished, s)}), waits=True))
        calls.append(Call(lambda s: host.update(flat("az", az.root_stats())), waits=True))
        calls.append(Call(lambda s: host.update(flat("tr", tr.root_stats())), waits=True))

        def close():
            az.close(); tr.close()
        return Scenario(calls, lambda: dict(host, cells=cells, rows=rows, verdict=verdict, status=status, **{"rec%d" % i: t for i, t in enumerate(rec)}), close)
    out = H.check("K12 match plies, K7 against K6", make)
    assert (out["rec1"].view(np.int32) == 3).all()


@pytest.mark.parametrize("kind", ["mcts", "trad"])
def test_ensemble_merge(H, kind):
    """gmk_mcts_ensemble_merge / gmk_trad_ensemble_merge behind the search that makes the roots they read: 2 ensembles of 3"""
    import torch
    n, group = 6, 3
    moves, lens, planes, last = positions(2, 8, first_board=80)
    rep = lambda a: np.repeat(a, group, axis=0)

    def make():
        if kind == "mcts":
            tree = G.BatchedMCTS(n, playouts_capacity=64, seed=13)
            tree.set_roots(rep(planes), rep(last[:, 0]), first_game_id=5)
            run = lambda s: tree.run(48, s)
        else:
            tree = G.PoolRAVEMCTS(n, node_capacity=1 << 14, seed=13, first_game_id=5)
            tree.set_positions(rep(moves), rep(lens))
            run = lambda s: tree.run(100, s)
        E = n // group
        outs = dict(visits=torch.zeros((E, N), dtype=torch.int32, device="cuda"), values=torch.zeros((E, N), device="cuda"), cells=torch.zeros(E, dtype=torch.int16, device="cuda"),
                    cells_per_game=torch.zeros(n, dtype=torch.int16, device="cuda"), root_visits=torch.zeros(E, dtype=torch.int32, device="cuda"),
                    root_value=torch.zeros(E, device="cuda"), status=torch.zeros(E, dtype=torch.int32, device="cuda"))
        fill(outs.values(), 0x11)
        calls = [Call(lambda s: fill(outs.values(), 0x5A)), Call(run), Call(lambda s: tree.ensemble_merge(group, stream=s, **outs))]
        return Scenario(calls, lambda: outs, tree.close)
    out = H.check("gmk_%s_ensemble_merge" % kind, make)
    assert not out["status"].any() and (out["root_visits"].view(np.uint32) > 0).all()
