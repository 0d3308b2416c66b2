"""The training loop on the device: TrainPipeline.train_network (network/train.py:62-86) over a ReplayBuffer and a Trainer (K11).

Play, keep, draw, learn, hand the new weights to the searcher -- all in HBM on one stream:

    net = PolicyValueNetwork().cuda()
    fused, trainer = FusedPolicyValueNetwork(net), Trainer(net, max_batch=512)
    replay = selfplay.ReplayBuffer(200_000)
    loop = TrainingLoop(replay, trainer, fused, export_every=1)
    if os.path.exists("run.pt"):
        loop.load("run.pt")                      # trainer, buffer, schedule and counters: the run goes on with the bits it would have had
    play = lambda: selfplay.play_network_games(32, fused, playouts=400, seed=SEED + loop.total_steps, first_game_id=32 * loop.total_steps)
    loop.run(100, play=play)

`play` returns a GameRecords with visit counts on the buffer's device (or None); the loop appends it before every step.  The loop does not
save `play`: one that derives its seed and first_game_id from loop.total_steps, as above, plays after a resume what it would have played.

The win-rate schedule of the reference (evaluate_network / eval_agents, train.py:88-126) is EvaluationSchedule; with eval_period the loop
plays its match every eval_period steps (selfplay.play_evaluation_games: K7 + K9 against the current opponent, refereed on the device),
and on_checkpoint is where a run saves itself (save() replaces the file atomically: a job killed in the middle leaves the old one):

    loop = TrainingLoop(replay, trainer, fused, eval_period=100, on_best=save_model, on_checkpoint=lambda name: loop.save("run.pt"))

parse_checkpoint_name reads the counters back from the name on_checkpoint gets, as TrainingPipeline.restore_model does (train.py:137-145).
"""
import os

import numpy as np
import torch

# DATA_CONFIG["schedule"] of the reference (config.py:8-20) without its two botzone programs, which do not exist here
SUPERVISOR = ("traditional_mcts", {"c_puct": 5.0, "c_iterations": 20000})
CANDIDATES = (("random_mcts", {"c_puct": 5.0, "c_iterations": 400}), ("rave_mcts", {"c_puct": 5.0, "c_iterations": 400}), None)


class EvaluationSchedule:
    """The state evaluate_network keeps (train.py:30-32) and its rules (:93-123): the network meets candidates[schedule_level] (None = the
    supervisor) at ref_iterations playouts; a win rate above best_win_rate is a new best, and one that reaches 1 - 0.05 * level powers an
    MCTS opponent up by 2 * c_iterations or, past 20 000, moves on to the next candidate.  leaves: the leaves per game per step of the
    network's searches in the match (selfplay.play_evaluation_games(leaves=); 1 = the reference's search, one leaf at a time).  vcf: (depth,
    budget) of the forced-win solver at the leaves of those searches (selfplay.play_evaluation_games(vcf=)), None = off.  proof: those searches
    carry proven wins and losses up their trees (selfplay.play_evaluation_games(proof=)).  vcf_defend: with vcf and proof, they prove the replies
    that lose to the opponent's forced win by fours (selfplay.play_evaluation_games(vcf_defend=)).  symmetry: "random" or "all" -- the network's
    leaves evaluated in one orientation of the board or averaged over all eight (selfplay.play_evaluation_games(symmetry=), K22); None = as they stand."""

    def __init__(self, supervisor=SUPERVISOR, candidates=CANDIDATES, eval_rounds=11, c_iterations=400, leaves=1, vcf=None, proof=False, vcf_defend=False,
                 symmetry=None):
        if not candidates:
            raise ValueError("EvaluationSchedule: at least one candidate (None = the supervisor)")
        if not 1 <= int(leaves) <= 8:
            raise ValueError("EvaluationSchedule: leaves must be in [1, 8]")
        self.leaves = int(leaves)
        if vcf is not None and not (len(vcf) == 2 and 1 <= int(vcf[0]) <= 32 and 1 <= int(vcf[1]) <= 1 << 20):
            raise ValueError("EvaluationSchedule: vcf is (depth in [1, 32], budget in [1, 2^20]) or None")
        self.vcf = None if vcf is None else (int(vcf[0]), int(vcf[1]))
        self.proof = bool(proof)
        self.vcf_defend = bool(vcf_defend)
        if symmetry not in (None, "random", "all"):
            raise ValueError("EvaluationSchedule: symmetry is None, \"random\" or \"all\"")
        self.symmetry = symmetry
        self.supervisor, self.candidates = supervisor, list(candidates)
        self.eval_rounds, self.c_iterations = int(eval_rounds), int(c_iterations)
        self.schedule_level, self.ref_iterations, self.best_win_rate = 0, self.c_iterations, 0.0

    def opponent(self):
        """(name, kwargs) of the agent to play now; an MCTS agent is powered up to ref_iterations (train.py:93-99)."""
        spec = self.candidates[self.schedule_level]
        name, kwargs = spec if spec is not None else self.supervisor
        kwargs = dict(kwargs)
        if "mcts" in name:
            kwargs["c_iterations"] = self.ref_iterations
        return name, kwargs

    def update(self, win_rate):
        """train.py:105-123 for one evaluation's win rate.  -> {"new_best", "level_up", "next_candidate"}; the opponent that was played is
        the one opponent() named BEFORE the call."""
        events = {"new_best": False, "level_up": False, "next_candidate": False}
        if win_rate > self.best_win_rate:
            events["new_best"] = True
            if win_rate >= 1.0 - 0.05 * self.schedule_level:        # levelup threshold decay
                events["level_up"] = True
                is_mcts = "mcts" in self.opponent()[0]
                if is_mcts:
                    self.ref_iterations += 2 * self.c_iterations
                if not is_mcts or self.ref_iterations > 20000:
                    self.ref_iterations = self.c_iterations
                    if self.schedule_level + 1 < len(self.candidates):      # (the reference would index past its list: the last level stays)
                        self.schedule_level += 1
                        events["next_candidate"] = True
                self.best_win_rate = 0.0
            else:
                self.best_win_rate = win_rate
        return events

    def state_dict(self):
        """The three numbers restore_model reads back (train.py:141-144).  The candidates and eval_rounds are configuration: not saved."""
        return {"schedule_level": self.schedule_level, "ref_iterations": self.ref_iterations, "best_win_rate": self.best_win_rate}

    def load_state_dict(self, state):
        level = int(state["schedule_level"])
        if not 0 <= level < len(self.candidates):
            raise ValueError("EvaluationSchedule.load_state_dict: schedule_level %d, but there are %d candidates" % (level, len(self.candidates)))
        self.schedule_level, self.ref_iterations, self.best_win_rate = level, int(state["ref_iterations"]), float(state["best_win_rate"])


def parse_checkpoint_name(name):
    """The counters in the name TrainingLoop.evaluate gives on_checkpoint, "current_model-<steps>-<level>-<ref_iterations>-<rate>", with or
    without directories in front (restore_model, train.py:140-144) -> {"total_steps", "schedule_level", "ref_iterations", "best_win_rate"}.
    Anything else raises ValueError."""
    parts = os.path.basename(str(name)).split("-")
    try:
        if len(parts) != 5 or parts[0] != "current_model":
            raise ValueError
        out = {"total_steps": int(parts[1]), "schedule_level": int(parts[2]), "ref_iterations": int(parts[3]), "best_win_rate": float(parts[4])}
        if min(out["total_steps"], out["schedule_level"], out["ref_iterations"]) < 0 or not 0.0 <= out["best_win_rate"] <= 1.0:
            raise ValueError
    except ValueError:
        raise ValueError("parse_checkpoint_name: %r is not current_model-<steps>-<level>-<ref_iterations>-<rate>" % (name,)) from None
    return out


def _plain(value):
    """A history value as Python numbers, strings, lists, dicts and tensors only -- what torch.load(weights_only=True) reads back."""
    if isinstance(value, dict):
        return {str(k): _plain(v) for k, v in value.items()}
    if isinstance(value, (list, tuple)):
        return [_plain(v) for v in value]
    if isinstance(value, np.ndarray):
        return value.tolist()
    if isinstance(value, np.generic):
        return value.item()
    if torch.is_tensor(value):
        return value.detach().cpu()
    return value


class TrainingLoop:
    def __init__(self, replay, trainer, fused=None, batch_size=512, lr=2e-3, kl_target=0.02, num_epoches=5, export_every=1,
                 eval_period=None, schedule=None, eval_playouts=400, eval_options=None, on_best=None, on_checkpoint=None):
        if batch_size < 1 or batch_size > trainer.max_batch:
            raise ValueError("TrainingLoop: batch_size must be in [1, trainer.max_batch]")
        if export_every < 1:
            raise ValueError("TrainingLoop: export_every must be at least 1")
        self.replay, self.trainer, self.fused = replay, trainer, fused
        self.batch_size, self.lr, self.kl_target, self.num_epoches, self.export_every = int(batch_size), float(lr), float(kl_target), int(num_epoches), int(export_every)
        self.lr_multiplier = 1.0
        self.total_steps = 0
        self.history = []                         # one dict per step: loss, entropy, kl, epochs, lr (the rate the step used), exported
        if eval_period is not None and eval_period < 1:
            raise ValueError("TrainingLoop: eval_period must be at least 1 (None: no evaluation)")
        # every eval_period steps: schedule.eval_rounds games of `fused` (eval_playouts playouts a move) against schedule.opponent();
        # eval_options: further keywords of selfplay.play_evaluation_games; on_best(name) / on_checkpoint(name) are where a caller saves the model
        self.eval_period = None if eval_period is None else int(eval_period)
        self.schedule = schedule if schedule is not None or eval_period is None else EvaluationSchedule()
        self.eval_playouts, self.eval_options, self.on_best, self.on_checkpoint = int(eval_playouts), dict(eval_options or {}), on_best, on_checkpoint

    def step(self):
        """One train_network: draw a minibatch, train_step on it, tune the learning-rate multiplier by the KL (train.py:73-77), and every
        export_every steps hand the parameters to `fused`.  -> the step's record (also appended to self.history)."""
        states, values, pi = self.replay.sample(self.batch_size)
        lr = self.lr * self.lr_multiplier
        loss, entropy, kl, epochs = self.trainer.train_step(states, values, pi, lr, self.kl_target, self.num_epoches)
        if kl > self.kl_target * 2 and self.lr_multiplier > 0.1:
            self.lr_multiplier /= 1.5
        elif kl < self.kl_target / 2 and self.lr_multiplier < 10:
            self.lr_multiplier *= 1.5
        self.total_steps += 1
        exported = self.fused is not None and self.total_steps % self.export_every == 0
        if exported:
            self.trainer.export(self.fused)
        record = {"loss": loss, "entropy": entropy, "kl": kl, "epochs": epochs, "lr": lr, "exported": exported}
        self.history.append(record)
        if self.eval_period is not None and self.total_steps % self.eval_period == 0:
            if self.fused is None:
                raise ValueError("TrainingLoop: eval_period needs `fused`, the network the evaluation plays with")
            if not exported:
                self.trainer.export(self.fused)
            self.evaluate(self.fused)
        return record

    def evaluate(self, network):
        """evaluate_network (train.py:88-126): eval_rounds games of `network` against the schedule's current opponent, the schedule's update,
        on_best("best_model-<opponent>-<ref_iterations>") on a new best (:106-110, named before the level-up as the reference names it) and
        on_checkpoint("current_model-<steps>-<level>-<ref_iterations>-<best win rate, two decimals>") after every evaluation (:126-134).
        -> the evaluation's record (also appended to self.history)."""
        from . import selfplay
        if self.schedule is None:
            self.schedule = EvaluationSchedule()
        sch = self.schedule
        name, kwargs = sch.opponent()
        played_at = sch.ref_iterations
        options = dict(self.eval_options)
        if getattr(sch, "leaves", 1) != 1:
            options.setdefault("leaves", sch.leaves)              # (eval_options may name its own)
        if getattr(sch, "vcf", None) is not None:
            options.setdefault("vcf", sch.vcf)
        if getattr(sch, "proof", False):
            options.setdefault("proof", True)
        if getattr(sch, "vcf_defend", False):
            options.setdefault("vcf_defend", True)
        if getattr(sch, "symmetry", None) is not None:
            options.setdefault("symmetry", sch.symmetry)
        rec, network_is_black, scores = selfplay.play_evaluation_games(sch.eval_rounds, network, (name, kwargs), playouts=self.eval_playouts, **options)
        win_rate = float(scores.mean())
        events = sch.update(win_rate)
        if events["new_best"] and self.on_best is not None:
            self.on_best("best_model-{}-{}".format(name, played_at))
        checkpoint = "current_model-{}-{}-{}-{:.2f}".format(self.total_steps, sch.schedule_level, sch.ref_iterations, sch.best_win_rate)
        if self.on_checkpoint is not None:
            self.on_checkpoint(checkpoint)
        record = {"evaluation": True, "step": self.total_steps, "opponent": name, "ref_iterations": played_at, "win_rate": win_rate, "scores": scores,
                  "network_is_black": network_is_black, "schedule_level": sch.schedule_level, "best_win_rate": sch.best_win_rate, "checkpoint": checkpoint, **events}
        self.history.append(record)
        return record

    def run(self, n_steps, play=None, first_move=0):
        """n_steps steps; before each, play() (if given) supplies new games for the buffer.  A step is skipped -- nothing is drawn -- while
        the buffer holds no more samples than a batch (generate_batch, data_helper.py:133-139).  -> the records of the steps taken.
        `play` stays the caller's business and is not part of a checkpoint: a resumable one derives its seed and first_game_id from
        self.total_steps, so that a resumed run plays the games the uninterrupted one would have played."""
        taken = []
        for _ in range(int(n_steps)):
            if play is not None:
                records = play()
                if records is not None and len(records):
                    self.replay.extend(records, first_move=first_move)
            if len(self.replay) <= self.batch_size:
                continue
            taken.append(self.step())
        return taken

    # ---- checkpoint and resume: everything a run needs to go on with the bits it would have had ----
    def config(self):
        """The loop's hyperparameters, as a checkpoint keeps them under "config"."""
        return {"batch_size": self.batch_size, "lr": self.lr, "kl_target": self.kl_target, "num_epoches": self.num_epoches,
                "export_every": self.export_every, "eval_period": self.eval_period, "eval_playouts": self.eval_playouts}

    def state_dict(self):
        """{"total_steps", "lr_multiplier", "history", "config", "trainer", "replay", "schedule" (None without one)}: Python numbers, strings,
        lists, dicts and torch tensors only, so torch.load(weights_only=True) reads it back.  Synchronises."""
        t = self.trainer.state_dict()
        trainer = {"step": int(t["step"]), **{k: {name: torch.from_numpy(np.array(a, dtype=np.float32)) for name, a in t[k].items()} for k in ("params", "m", "v")}}
        return {"total_steps": self.total_steps, "lr_multiplier": self.lr_multiplier, "history": _plain(self.history), "config": self.config(),
                "trainer": trainer, "replay": self.replay.state_dict(), "schedule": None if self.schedule is None else self.schedule.state_dict()}

    def load_state_dict(self, state):
        """Restores a state_dict() into this loop's own trainer, replay and schedule, and exports the restored parameters into `fused` if
        there is one.  Raises ValueError, naming the keys, if the saved "config" differs from this loop's -- before anything is changed;
        so does a buffer state that the replay refuses (ReplayBuffer.load_state_dict)."""
        mine, saved = self.config(), dict(state["config"])
        differ = sorted(k for k in set(mine) | set(saved) if k not in mine or k not in saved or mine[k] != saved[k])
        if differ:
            raise ValueError("TrainingLoop.load_state_dict: the saved config differs in " + ", ".join(
                "%s (saved %r, here %r)" % (k, saved.get(k), mine.get(k)) for k in differ))
        if state["schedule"] is not None and self.schedule is None:
            self.schedule = EvaluationSchedule()
        self.replay.load_state_dict(state["replay"])                  # the one part that can refuse: first
        if state["schedule"] is not None:
            self.schedule.load_state_dict(state["schedule"])
        t = state["trainer"]
        self.trainer.load_state_dict({"step": int(t["step"]), **{k: {name: a.numpy() for name, a in t[k].items()} for k in ("params", "m", "v")}})
        self.total_steps, self.lr_multiplier, self.history = int(state["total_steps"]), float(state["lr_multiplier"]), list(state["history"])
        if self.fused is not None:
            self.trainer.export(self.fused)

    def save(self, path):
        """state_dict() to `path` with torch.save, through a temporary file beside it and os.replace: a job killed in the middle leaves the
        old file."""
        path = os.fspath(path)
        tmp = "%s.tmp.%d" % (path, os.getpid())
        try:
            torch.save(self.state_dict(), tmp)
            os.replace(tmp, path)
        finally:
            if os.path.exists(tmp):
                os.remove(tmp)

    def load(self, path):
        """load_state_dict() of a file save() wrote, read with weights_only=True.  A file that cannot be read leaves the loop as it was."""
        self.load_state_dict(torch.load(os.fspath(path), map_location="cpu", weights_only=True))
