#!/usr/bin/env python3
"""One line per configuration of the game loops of gomokuai_amd/selfplay.py: a name and a sha256 over what the call returned -- per game
lens, winner, moves[:len], visits[:len], then overflow; for match and evaluation also the sides and the scores.  Small configurations
(at most 12 games, 40 playouts, one shared network) that between them reach every loop body of every entry point: run it on two
commits and compare the outputs to show that a change to the loops left every record as it was (profiles/selfplay_loops_digest.txt).
    python tools/selfplay_digest.py [name prefix]          (seconds per configuration go to stderr)"""
import hashlib, itertools, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from gomokuai_amd import lib as G, selfplay
from gomokuai_amd.network import FusedPolicyValueNetwork, PolicyValueNetwork
torch.cuda.set_device(0); G.init(0)
NET = FusedPolicyValueNetwork(PolicyValueNetwork(seed=4).cuda().eval())
NOISE = (0.05, 0.25)


def digest(rec, *extra):
    r = rec.cpu()
    lens, h = r.lens.numpy(), hashlib.sha256()
    h.update(np.ascontiguousarray(lens).tobytes() + np.ascontiguousarray(r.winner.numpy()).tobytes())
    for g, l in enumerate(lens):
        h.update(np.ascontiguousarray(r.moves[g, :l].numpy()).tobytes())
        if r.visits is not None:
            h.update(np.ascontiguousarray(r.visits[g, :l].numpy()).tobytes())
    h.update(bytes([bool(rec.overflow)]))
    for a in extra:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def configs():
    yield "games default", lambda: digest(selfplay.play_games(8, 40, seed=5, first_game_id=3))
    yield "games lockstep opening=3", lambda: digest(selfplay.play_games(8, 40, seed=5, first_game_id=3, lockstep=True, opening_plies=3))
    yield "games slots=3", lambda: digest(selfplay.play_games(8, 40, seed=5, first_game_id=3, slots=3, opening_plies=2))
    yield "games max_moves=7", lambda: digest(selfplay.play_games(8, 40, seed=5, first_game_id=3, max_moves=7, opening_plies=12))
    for lockstep in (False, True):
        yield "games reuse noise lockstep=%s" % lockstep, lambda l=lockstep: digest(selfplay.play_games(
            8, 40, seed=5, first_game_id=3, reuse_subtree=True, root_noise=NOISE, lockstep=l))
    for policy, loop, slots, (reuse, noise) in itertools.product(selfplay._POLICIES, (True, "lockstep", False), (None, 3),
                                                                 ((False, None), (True, None), (True, NOISE))):
        yield "supervisor %s loop=%s slots=%s reuse=%s noise=%s" % (policy, loop, slots, reuse, noise), lambda p=policy, l=loop, s=slots, r=reuse, z=noise: digest(
            selfplay.play_supervisor_games(7, 24, seed=11, first_game_id=20, opening_plies=3, policy=p, device_loop=l, slots=s, reuse_subtree=r, root_noise=z))
    for loop in (True, False):
        yield "supervisor max_moves=6 loop=%s" % loop, lambda l=loop: digest(selfplay.play_supervisor_games(
            7, 24, seed=11, first_game_id=20, opening_plies=3, max_moves=6, device_loop=l, reuse_subtree=True, root_noise=NOISE))
    yield "supervisor max_moves=6 loop=False slots=3", lambda: digest(selfplay.play_supervisor_games(
        7, 24, seed=11, first_game_id=20, opening_plies=3, max_moves=6, device_loop=False, slots=3))
    for loop, slots in itertools.product((True, False), (None, 3)):
        host_slots = not loop and slots is not None                 # (the host-driven slot loop takes fresh roots only)
        kw = dict(seed=3, first_game_id=9, opening_plies=2, device_loop=loop, slots=slots)
        name = "network loop=%s slots=%s " % (loop, slots)
        for reuse, noise in ((False, None), (False, NOISE)) + (() if host_slots else ((True, None), (True, NOISE))):
            yield name + "reuse=%s noise=%s" % (reuse, noise), lambda kw=kw, r=reuse, z=noise: digest(selfplay.play_network_games(7, NET, 16, reuse_subtree=r, root_noise=z, **kw))
        tree = dict(reuse_subtree=False, root_noise=None) if host_slots else {}
        for label, more in (("leaves=2", dict(leaves=2)), ("vcf proof", dict(vcf=(8, 32), proof=True)), ("sample_plies=4", dict(sample_plies=4))):
            yield name + label, lambda kw=kw, tree=tree, more=more: digest(selfplay.play_network_games(7, NET, 16, **kw, **tree, **more))
        if slots is None:
            yield name + "max_moves=5", lambda kw=kw: digest(selfplay.play_network_games(7, NET, 16, max_moves=5, **kw))
    sup = ("traditional_mcts", {"c_puct": 5.0, "c_iterations": 30})
    candidates = (("random_mcts", {"c_iterations": 24}), ("rave_mcts", {"c_iterations": 24}), ("traditional_mcts", {"c_iterations": 24}),
                  ("traditional_mcts", {"c_iterations": 24, "use_rave": True, "c_bias": 0.0}))
    for cand, slots in itertools.product(candidates, (None, 2)):
        def match(cand=cand, slots=slots):
            rec, sup_black = selfplay.play_match_games(9, sup, cand, seed=77, first_game_id=5, opening_plies=2, slots=slots)
            return digest(rec, sup_black)
        yield "match %s%s slots=%s" % (cand[0], " use_rave" if cand[1].get("use_rave") else "", slots), match
    for opp, reuse in itertools.product(candidates, (True, False)):
        for loop in ((False,) if opp[0] == "random_mcts" else (True, False)):
            def evaluation(opp=opp, reuse=reuse, loop=loop):
                rec, black, scores = selfplay.play_evaluation_games(5, NET, opp, playouts=16, seed=21, first_game_id=2, opening_plies=2, reuse_subtree=reuse, device_loop=loop)
                return digest(rec, black, scores, *[np.concatenate([g["games"], [g["unfinished"], g["live_games"]]]).astype(np.int64) for g in rec.groups])
            yield "evaluation %s%s reuse=%s loop=%s" % (opp[0], " use_rave" if opp[1].get("use_rave") else "", reuse, loop), evaluation
    yield "evaluation proof max_moves=9", lambda: digest(*selfplay.play_evaluation_games(
        5, NET, candidates[2], playouts=16, seed=21, opening_plies=1, max_moves=9, device_loop=False, vcf=(8, 32), proof=True, root_noise=None))

    def pattern():
        rec, values = selfplay.play_pattern_games(12, opening_plies=4, seed=9, first_game_id=6)
        return digest(rec, values.cpu().numpy(), rec.status.cpu().numpy())
    yield "pattern", pattern


only = sys.argv[1] if len(sys.argv) > 1 else ""
t_all = time.time()
for name, fn in configs():
    if name.startswith(only):
        t0 = time.time(); d = fn()
        print("%-72s %s" % (name, d), flush=True)
        print("    %.2f s" % (time.time() - t0), file=sys.stderr, flush=True)
print("total %.1f s" % (time.time() - t_all), file=sys.stderr)
NET.close()
