"""K1 hands a workgroup's boards and the density bursts of its groups out inside the workgroup; the workgroup's run of groups comes from
two numbers the host works out.  Board counts at which either can go wrong -- fewer boards than a workgroup has wavefronts, one group and a
board, the counts around which the workgroups of a 256-workgroup grid own 0, 1 and 2 groups, a run whose last group is partial -- against
the oracle's from-scratch evaluator (oracle/go_scratch.c): all four outputs, the status word among them.  Every case launches the same
input twice into buffers refilled with a sentinel (the second launch starts from the LDS and the hand-out state the first one left) with
sixteen boards of the sentinel behind every output, which must stay.  Integer outputs: exact."""
import numpy as np
import pytest

from gomokuai_amd import lib as G

pytestmark = pytest.mark.gpu

NAMES = ("scores", "density", "totals", "status")
WORDS = (900, 900, 11, 1)
COUNTS = (1, 15, 16, 17, 32, 33, 16 * 255, 16 * 256 - 1, 16 * 256, 16 * 256 + 1, 16 * 257, 16 * 512 + 5)
SENTINEL = np.int32(0x5A5A5A5A)
EXTRA = 16

_cases = {}


def _case(oracle, n):
    """boards and the oracle's answer, once per board count (shared by the tests, never written to)"""
    if n not in _cases:
        moves, lens, planes = G.synth_boards(n, n & 1, first_board=310000 + 7 * n)
        ref = oracle.scratch_batch(moves, lens)
        for a in ref:
            a.setflags(write=False)
        _cases[n] = (planes, ref)
    return _cases[n]


def _launch_twice_and_check(planes, ref, n, stream, what):
    import torch
    dev = torch.device("cuda", 0)
    d_planes = torch.from_numpy(planes.view(np.int16).reshape(n, 32)).to(dev)
    bufs = [torch.empty(((n + EXTRA) * w,), dtype=torch.int32, device=dev) for w in WORDS]
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for launch in range(2):
            for b in bufs:
                b.fill_(int(SENTINEL))
            G.eval_batch(d_planes.data_ptr(), n, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), bufs[3].data_ptr(), stream.cuda_stream)
            stream.synchronize()
            host = [b.cpu().numpy() for b in bufs]
            for name, h, w in zip(NAMES, host, WORDS):
                touched = int((h[n * w:] != SENTINEL).sum())
                print("%s launch %d %s: %d of %d sentinel words overwritten" % (what, launch, name, touched, EXTRA * w))
                assert touched == 0, "%s launch %d: %d words of %s behind board %d were written" % (what, launch, touched, name, n - 1)
            got = (host[0][:n * 900].reshape(n, 4, 225), host[1][:n * 900].reshape(n, 2, 2, 225), host[2][:n * 11].view(np.uint32).reshape(n, 11), host[3][:n])
            for name, a, b in zip(NAMES, ref, got):
                bad = np.nonzero((a.reshape(n, -1) != b.reshape(n, -1)).any(axis=1))[0]
                print("%s launch %d %s: %d of %d boards differ" % (what, launch, name, len(bad), n))
                assert len(bad) == 0, "%s launch %d: %s differs on %d boards, first %d" % (what, launch, name, len(bad), bad[0])


@pytest.mark.parametrize("n", COUNTS)
def test_handout_matches_scratch_oracle(oracle, n):
    import torch
    G.init(0)
    planes, ref = _case(oracle, n)
    info = G.eval_launch_info(n)
    print("n=%d: launch %s" % (n, info))
    _launch_twice_and_check(planes, ref, n, torch.cuda.current_stream(), "n=%d" % n)


@pytest.mark.parametrize("side", [False, True], ids=["current-stream", "side-stream"])
def test_handout_on_either_stream(oracle, side):
    """about 4 100 boards: every workgroup of a 256-workgroup grid owns one group, the first one two (the second of them partial)"""
    import torch
    G.init(0)
    n = 4101
    planes, ref = _case(oracle, n)
    stream = torch.cuda.Stream() if side else torch.cuda.current_stream()
    _launch_twice_and_check(planes, ref, n, stream, "n=%d %s" % (n, "side stream" if side else "current stream"))
