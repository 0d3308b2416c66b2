"""The training loop on the device: TrainPipeline.train_network (network/train.py:62-86) over a ReplayBuffer and a Trainer (K11).

Play, keep, draw, learn, hand the new weights to the searcher -- all in HBM on one stream:

    net = PolicyValueNetwork().cuda()
    fused, trainer = FusedPolicyValueNetwork(net), Trainer(net, max_batch=512)
    replay = selfplay.ReplayBuffer(200_000)
    loop = TrainingLoop(replay, trainer, fused, export_every=1)
    loop.run(100, play=lambda: selfplay.play_network_games(32, fused, playouts=400))

`play` returns a GameRecords with visit counts on the buffer's device (or None); the loop appends it before every step.  The win-rate
schedule of the reference (evaluate_network / eval_agents, train.py:88-126) is not part of this loop.
"""


class TrainingLoop:
    def __init__(self, replay, trainer, fused=None, batch_size=512, lr=2e-3, kl_target=0.02, num_epoches=5, export_every=1):
        if batch_size < 1 or batch_size > trainer.max_batch:
            raise ValueError("TrainingLoop: batch_size must be in [1, trainer.max_batch]")
        if export_every < 1:
            raise ValueError("TrainingLoop: export_every must be at least 1")
        self.replay, self.trainer, self.fused = replay, trainer, fused
        self.batch_size, self.lr, self.kl_target, self.num_epoches, self.export_every = int(batch_size), float(lr), float(kl_target), int(num_epoches), int(export_every)
        self.lr_multiplier = 1.0
        self.total_steps = 0
        self.history = []                         # one dict per step: loss, entropy, kl, epochs, lr (the rate the step used), exported

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
        return record

    def run(self, n_steps, play=None, first_move=0):
        """n_steps steps; before each, play() (if given) supplies new games for the buffer.  A step is skipped -- nothing is drawn -- while
        the buffer holds no more samples than a batch (generate_batch, data_helper.py:133-139).  -> the records of the steps taken."""
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
