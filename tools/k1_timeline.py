#!/usr/bin/env python3
"""K1, the timeline of one launch (profiling aid): where a launch's time goes OUTSIDE the board loop.  The profiling flavour of the library
(GMK_HIP_LIB=prof, the default here; or another build of it by path) leaves eight s_memtime values per wavefront in the file that
GMK_EVAL_TIMELINE names: [0] entry, [1] end of the prologue, [2] arrival at the barrier, [3] leaving it, [4] end of the wavefront's last
board, [5] exit, [6] density bursts taken in or behind the iteration of the last board | boards done << 16, [7] the clocks of those bursts;
in front of them the grid, the wavefronts per workgroup, the slots and the launch's time between two HIP events.  Reported per workgroup
from its first stamp, as median and worst over the workgroups, in clocks and as a share of the workgroup's own span.
usage: k1_timeline.py [boards [kind]]   (default 65536 0; the last of five launches is the one reported)"""
import os, sys, tempfile
os.environ.setdefault("GMK_HIP_LIB", "prof")
path = os.environ.setdefault("GMK_EVAL_TIMELINE", os.path.join(tempfile.mkdtemp(), "k1_timeline.bin"))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from gomokuai_amd import lib as G


def stats(name, clocks, span):
    """clocks: one value per workgroup (or [workgroup, wavefront]); span: the workgroups' spans"""
    c = np.asarray(clocks, dtype=np.float64)
    share = c / (span.reshape(-1, *([1] * (c.ndim - 1))))
    print("  %-64s median %8.0f  worst %8.0f clocks   %5.2f %% / %5.2f %% of the workgroup's span"
          % (name, np.median(c), c.max(), 100 * np.median(share), 100 * share.max()))


def report(raw, n):
    grid, waves, slots, wall_ns = (int(x) for x in raw[:4])
    t = raw[4:].reshape(grid, waves, slots).astype(np.int64)
    entry, prologue, arrive, leave, last_board, exit_ = (t[:, :, k] for k in range(6))
    late_bursts, boards, late_clocks = t[:, :, 6] & 0xFFFF, t[:, :, 6] >> 16, t[:, :, 7]
    t0 = entry.min(axis=1)
    end = exit_.max(axis=1)
    span = (end - t0).astype(np.float64)
    # (s_memtime is a clock of the workgroup's own part of the chip: values of different workgroups are not comparable, differences within one are)
    print("launch: %d boards, %d workgroups x %d wavefronts; %.1f us between HIP events; a workgroup's span: median %.0f, worst %.0f clocks (the worst span = %.0f clocks per us of event time)"
          % (n, grid, waves, wall_ns / 1e3, np.median(span), span.max(), span.max() / (wall_ns / 1e3)))
    print("dispatch: a workgroup's wavefronts enter within median %.0f, worst %.0f clocks" % (np.median(entry.max(axis=1) - t0), (entry.max(axis=1) - t0).max()))
    print("(a) the prologue")
    stats("entry -> end of the prologue, per wavefront", prologue - entry, span)
    stats("workgroup's first stamp -> its last wavefront's prologue end", prologue.max(axis=1) - t0, span)
    print("(b) the barrier")
    stats("first stamp -> arrival, per wavefront", arrive - t0[:, None], span)
    stats("first stamp -> the last wavefront's arrival", arrive.max(axis=1) - t0, span)
    stats("wait at the barrier, per wavefront", leave - arrive, span)
    stats("wait at the barrier, mean over the workgroup's wavefronts", (leave - arrive).mean(axis=1), span)
    print("(c) the end")
    stats("first stamp -> a wavefront's last board ends", last_board - t0[:, None], span)
    stats("first stamp -> a wavefront exits", exit_ - t0[:, None], span)
    stats("first stamp -> the workgroup's last wavefront exits (its span)", span, span)
    print("(d) idle wavefront-time at the end")
    first_out = exit_.min(axis=1)
    idle = (end[:, None] - exit_).sum(axis=1) / waves
    stats("first exit -> last exit of the workgroup", end - first_out, span)
    stats("idle behind a wavefront's exit, mean over the wavefronts", idle, span)
    between = np.maximum(end - first_out, 1)
    print("  of the wavefront-time between the first and the last exit, idle: median %.1f %%, worst %.1f %%" % (100 * np.median(idle / between), 100 * (idle / between).max()))
    print("(e) density bursts in or behind the iteration of a wavefront's last board")
    print("  per workgroup: median %.1f, worst %d bursts; %d of %d wavefronts took one; they took median %.0f, worst %.0f clocks each"
          % (np.median(late_bursts.sum(axis=1)), late_bursts.sum(axis=1).max(), int((late_bursts > 0).sum()), grid * waves,
             np.median(late_clocks[late_bursts > 0]) if (late_bursts > 0).any() else 0, late_clocks.max()))
    on_last = late_bursts > 0
    if on_last.any():
        print("  a wavefront that took one exits %.0f clocks (median) behind one that did not" % (np.median((exit_ - t0[:, None])[on_last]) - np.median((exit_ - t0[:, None])[~on_last])))
    print("boards per wavefront: min %d, median %.0f, max %d" % (boards.min(), np.median(boards), boards.max()))
    print("across workgroups (not this tool's subject): the longest span is %.2f %% above the median one" % (100 * (span.max() / np.median(span) - 1)))


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
    kind = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    torch.cuda.set_device(0); G.init(0)
    dev = torch.device("cuda", 0)
    _, _, planes = G.synth_boards(n, kind)
    d_planes = torch.from_numpy(planes.view(np.int16).reshape(n, 32)).to(dev)
    outs = [torch.empty((n, w), dtype=torch.int32, device=dev) for w in (900, 900, 11, 1)]
    stream = torch.cuda.current_stream().cuda_stream
    for _ in range(5):
        G.eval_batch(d_planes.data_ptr(), n, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(), stream)
        torch.cuda.synchronize()
    if not os.path.exists(path):
        sys.exit("k1_timeline: %s was not written: is GMK_HIP_LIB a -DGMK_PROFILE build?" % path)
    report(np.fromfile(path, dtype=np.uint64), n)


if __name__ == "__main__":
    main()
