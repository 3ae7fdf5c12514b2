"""Parameter update -- drop-in for the reference's train_network.py, on the GNN, with the whole optimisation step in HIP.

Call surface kept (train_network.py:14-107): NUM_EPOCH, BATCH_SIZE, load_data, train_network.  One step = one C call (trainers.py).
The parameters updated are the model's own state_dict tensors; torch is used for memory, shuffling and the .pth / .history files only.

What is here reads this module's settings (NUM_EPOCH, BATCH_SIZE, PV_NETWORK_PATH, TRAIN_*) when it is called: the rows of an update,
the held-out side, the epoch loop.  What takes everything it needs as arguments lives beside it and is imported back, so every name
is still found here: the trainers (trainers.py), the weight average (weight_average.py), the mirror launch (train_augment.py) and
the numpy statements the tests compare with (train_reference.py).
"""
import pickle
from pathlib import Path

import numpy as np
import torch

from . import distributed as aqd
from .constants import PV_NETWORK_PATH, BOARD_SIZE  # noqa: F401
from .pv_network_gnn import STATE_DICT_KEYS, HIDDEN_DIM, NUM_FEATURES, load_network, pack_states  # noqa: F401
from .train_augment import draw_mirror_flips, _mirror_arguments, _augment_launch, augment_gather  # noqa: F401
from .train_reference import (LEARNING_RATE, clip_coefficient, adam_reference, weight_average_reference,  # noqa: F401
                              weight_average_due, check_average_controls, _checked_average_controls, check_loss_controls,
                              loss_reference)
from .trainers import BATCH_SIZE, default_decay_mask, grad_norm, _Trainer, GNNTrainer, GeneralTrainer, CNNTrainer  # noqa: F401
from .weight_average import weight_average_table, WeightAverage  # noqa: F401

NUM_EPOCH = 100    # train_network.py:14
# Mirror-symmetry augmentation (the reference has none): every epoch trains on each position either as recorded or mirrored left
# to right, drawn per (TRAIN_MIRROR_SEED, epoch, position) -- one fused gather + flip launch in place of the epoch's three gathers.
TRAIN_MIRROR = False      # False = off: the reference's epochs
TRAIN_MIRROR_SEED = 0
# Replay window (the reference trains on the newest file alone; replay.ReplayWindow): the rows of the last generations, resident on
# the GPU.  An epoch shuffles the window's valid slots; with the mirror on, a flip is keyed by SOURCE row, which for a window is the
# ring slot (so a row keeps its draw for as long as it stays in the ring, and a file route's row i is keyed by i).
TRAIN_WINDOW = None        # a ReplayWindow (self_play.SP_REPLAY fills it); None or empty = the file route
TRAIN_GENERATIONS = 1      # K > 1 without a window: a temporary window over the newest K .history files
TRAIN_EPOCH_ROWS = None    # E: an epoch trains on the first min(E, n) rows of its shuffle, so an update's cost does not grow with K
# Position merge (replay.merge_positions): the rows of an update that hold the same position -- every game's opening, and much of the
# early game on small boards -- become ONE row with the mean policy and value target, once per update; the epochs, TRAIN_EPOCH_ROWS and
# the mirror then run on the merged rows (a flip is keyed by merged row).  Every position weighs the same.
TRAIN_MERGE_POSITIONS = False    # False = off: one row per occurrence
# Policy surprise weighting (replay.surprise_index): the rows of an update drawn by KL(row's policy target || the network the update
# starts from), once per update, after the merge when that is on: an expected number of copies per row -- the uniform share dealt out
# evenly, the rest in proportion to the surprise -- rounded by a draw keyed by (seed, update, ring slot), at most MAX_COPIES of a row.
# The epochs, TRAIN_EPOCH_ROWS, the mirror and the data-parallel deal then run on the expanded index.
TRAIN_SURPRISE_WEIGHTING = False         # False = off: nothing is launched
TRAIN_SURPRISE_UNIFORM_SHARE = 0.5       # U: the share of the rows dealt out evenly (1 = every row once: the option off)
TRAIN_SURPRISE_MAX_COPIES = 8            # C: the most copies of one row, 1..255
TRAIN_SURPRISE_SEED = 0
_surprise_updates = 0                    # surprise-weighted updates drawn without a window: the `update` of the draw's key
# Optimiser controls (the reference's optimiser is a bare Adam(lr=0.001)): weight decay on the weight matrices and conv kernels, and
# global-norm gradient clipping, both inside the HIP step (include/aqgnn.h "optimiser controls").  All off = the reference's update.
TRAIN_WEIGHT_DECAY = 0.0      # c of the AlphaZero loss term c * ||theta||^2, as torch's weight_decay
TRAIN_DECOUPLED = True        # True: torch.optim.AdamW's decay; False: torch.optim.Adam(weight_decay=)'s
TRAIN_MAX_GRAD_NORM = None    # M: torch.nn.utils.clip_grad_norm_(params, M) in front of every update; None = off
# Weight averaging (the reference saves the last Adam iterate): an exponential moving average of the parameters, updated inside the
# HIP steps (include/aqgnn.h "weight averaging", weight_average.WeightAverage) and saved as latest.pth in place of the last iterate.
TRAIN_EMA_DECAY = None        # d in [0, 1): e <- d e + (1 - d) p behind every TRAIN_EMA_EVERY-th Adam update; None = off, no object built
TRAIN_EMA_EVERY = 1           # K >= 1: the updates are made at the Adam steps whose number is a multiple of K
# Held-out validation (validation.row_metrics / holdout_split; the reference has no held-out set): a share of the POSITIONS -- a
# position's side is a function of (TRAIN_HOLDOUT_SEED, its record's key bytes) alone, so it is the same in every update and every
# generation -- is kept out of the update, split off the recorded rows before the merge and the surprise draw, and the network that
# would be saved now is measured on those rows (one row per occurrence, unmerged, unmirrored) after the epochs.
TRAIN_HOLDOUT_SHARE = None        # S in (0, 1); None = off: nothing is launched, latest.pth is what it was
TRAIN_HOLDOUT_SEED = 0
TRAIN_HOLDOUT_EVERY = 1           # V >= 1: validate after every V-th epoch, and always after the last
TRAIN_HOLDOUT_KEEP_BEST = False   # True: save the snapshot of the validated epoch with the least policy_loss + value_mse (first minimum)
TRAIN_HOLDOUT_LOG = None          # a path: one JSON line per update is appended (curve, table, counts, options)
# Loss form (the reference applies CrossEntropyLoss to the already-softmaxed policy; include/aqgnn.h "loss form"): the cross-entropy
# between the target and softmax(logits), taken from the logits inside the HIP steps, and a weight on the value term's gradient.
TRAIN_POLICY_LOSS = 'reference'   # 'reference' = the reference's double softmax; 'cross_entropy' = the AlphaZero policy loss
TRAIN_VALUE_LOSS_WEIGHT = 1.0     # w >= 0: the loss minimised is policy + w * value (the value loss printed stays unweighted)


def load_data():
    """Load the latest training data (train_network.py:19-23).  The file is this build's own self_play.write_data()
    output (same schema as the reference's)."""
    history_path = sorted(Path('./data').glob('*.history'))[-1]
    with history_path.open(mode='rb') as f:
        return pickle.load(f)


def _training_rows(dev, board_size, model=None):
    """(s, p, v, index) an update trains on, on `dev`: uint8 [rows,72] records, float32 [rows,A] policy and [rows] value targets, and
    the int64 rows of them that are valid, oldest first -- or None when all are (the file route).  A non-empty TRAIN_WINDOW gives its
    rings and index(); TRAIN_GENERATIONS = K > 1 without one a temporary window over the newest K files; otherwise the newest file
    (train_network.py:19-23,:31-39).  TRAIN_MERGE_POSITIONS: whichever of the three it is, merged once (replay.merge_positions) into
    compact rows, one per distinct position, with index None; every rank merges the same rows to the same result.
    TRAIN_SURPRISE_WEIGHTING (needs `model`, the network the update starts from): behind the merge, the index expanded by policy
    surprise (replay.surprise_index) -- some rows named several times, some not at all; every rank draws the same index, with no
    collective, and advances the update counter (the window's when one is trained on, else the module's) alike."""
    return _update_rows(dev, board_size, model)[:4]


def _update_rows(dev, board_size, model=None):
    """_training_rows with the held-out side beside it: (s, p, v, index, held).  TRAIN_HOLDOUT_SHARE None: held is None and nothing
    is launched.  Otherwise the recorded rows' index is split by position (validation.holdout_split) BEFORE the merge and the surprise
    draw, which -- like TRAIN_EPOCH_ROWS, the mirror and the trainers -- then act on the training side alone; held = dict(rows=(s, p,
    v) as recorded, index=the held-out rows of them in input order, one per occurrence, counts=dict(rows, held, train, distinct)).
    Every rank splits alike, with no collective.  An empty side is a ValueError naming the share."""
    s, p, v, index = _recorded_rows(dev, board_size)
    rank0 = aqd.rank_world()[0] == 0
    held = None
    if TRAIN_HOLDOUT_SHARE is not None:
        index, held = _held_out_rows(s, p, v, index, board_size, rank0)
    s, p, v, index = _merged_and_drawn(s, p, v, index, board_size, model, rank0)
    return s, p, v, index, held


def _held_out_rows(s, p, v, index, board_size, rank0):
    """(the training side's index, the held dict of _update_rows) of the recorded rows (s, p, v, index)."""
    from .replay_reference import KEY_BYTES
    from .validation import holdout_split
    n = int(s.shape[0] if index is None else index.shape[0])
    train_index, held_index = holdout_split(s, index, TRAIN_HOLDOUT_SHARE, TRAIN_HOLDOUT_SEED, board_size)
    h = int(held_index.shape[0])
    if h == 0 or h == n:
        raise ValueError(f"TRAIN_HOLDOUT_SHARE = {TRAIN_HOLDOUT_SHARE}: of {n} rows {h} are held out and {n - h} trained on under seed "
                         f"{TRAIN_HOLDOUT_SEED}; both sides need a row")
    key_bytes = torch.from_numpy(KEY_BYTES).to(s.device)
    distinct = int(torch.unique(s.index_select(0, held_index).index_select(1, key_bytes), dim=0).shape[0])
    if rank0:
        print(f"held out: {h} of {n} rows ({distinct} distinct positions)")
    return train_index, dict(rows=(s, p, v), index=held_index, counts=dict(rows=n, held=h, train=n - h, distinct=distinct))


def _merged_and_drawn(s, p, v, index, board_size, model, rank0):
    """The merge and the surprise draw of _training_rows, on the rows (s, p, v, index)."""
    if TRAIN_MERGE_POSITIONS:
        from .replay import merge_positions
        n = int(s.shape[0] if index is None else index.shape[0])
        s, p, v, count = merge_positions(s, p, v, index=index, board_size=board_size)
        index = None
        if rank0:
            print(f"merged positions: {n} rows, {int(s.shape[0])} positions, longest run {int(count.max()) if n else 0}")
    if TRAIN_SURPRISE_WEIGHTING:
        index = _surprise_rows(model, s, p, index, rank0)
    return s, p, v, index


def _surprise_rows(model, s, p, index, rank0):
    """The surprise-weighted index of the rows (s, p, index), drawn under the next update number of the window or of the module."""
    global _surprise_updates
    from .replay import surprise_index
    if model is None:
        raise ValueError("TRAIN_SURPRISE_WEIGHTING: _training_rows needs the network the update starts from (model=)")
    window = _active_window()
    if window is not None:
        update = window.surprise_updates
        window.surprise_updates += 1
    else:
        update = _surprise_updates
        _surprise_updates += 1
    stats = {}
    index, _, _ = surprise_index(model, s, p, index, seed=TRAIN_SURPRISE_SEED, update=update, uniform_share=TRAIN_SURPRISE_UNIFORM_SHARE,
                                 max_copies=TRAIN_SURPRISE_MAX_COPIES, stats=stats)
    if rank0:
        print(f"surprise weighting: {stats['rows']} rows -> {stats['expanded']} rows, {stats['left_out']} left out, most copies "
              f"{stats['most_copies']}, mean KL {stats['mean_kl']:.4f}")
    return index


def _active_window():
    """TRAIN_WINDOW when it holds a row, else None: an empty window is the file route."""
    return TRAIN_WINDOW if TRAIN_WINDOW is not None and len(TRAIN_WINDOW) > 0 else None


def _recorded_rows(dev, board_size):
    """_training_rows before any merge: one row per occurrence."""
    from .replay import ReplayWindow
    window = _active_window()
    if window is None and TRAIN_GENERATIONS > 1:
        window = ReplayWindow(board_size, max_generations=TRAIN_GENERATIONS, device=dev)
        window.extend_from_files(sorted(Path('./data').glob('*.history'))[-TRAIN_GENERATIONS:])
    if window is not None:
        if window.board_size != board_size:
            raise ValueError(f"the replay window holds {window.board_size}x{window.board_size} rows; the network plays "
                             f"{board_size}x{board_size}")
        s, p, v = (x.to(dev) for x in window.tensors())
        return s, p, v, window.index().to(dev)
    history = load_data()
    s, p, v = zip(*history)
    s = torch.from_numpy(pack_states(s, board_size)).to(dev)                       # uint8 [n,72]
    p = torch.tensor(np.array(p), dtype=torch.float32, device=dev)                 # policy targets
    v = torch.tensor(np.array(v), dtype=torch.float32, device=dev)                 # value targets
    return s, p, v, None


def _epoch_order(perm, index):
    """The rows an epoch trains on, in order, from its shuffle of 0 .. n-1: the first TRAIN_EPOCH_ROWS of it, as rows of the arrays."""
    if TRAIN_EPOCH_ROWS is not None:
        perm = perm[:max(int(TRAIN_EPOCH_ROWS), 0)]
    return perm if index is None else index[perm]


def lr_lambda(epoch):
    """train_network.py:59-65."""
    if epoch >= 80:
        return 0.25
    elif epoch >= 50:
        return 0.5
    return 1.0



def _configured_controls():
    """The trainers' optimiser keyword arguments from TRAIN_WEIGHT_DECAY, TRAIN_DECOUPLED and TRAIN_MAX_GRAD_NORM."""
    return dict(weight_decay=TRAIN_WEIGHT_DECAY, decoupled=TRAIN_DECOUPLED, max_grad_norm=TRAIN_MAX_GRAD_NORM)


def _configured_loss():
    """The trainers' loss keyword arguments from TRAIN_POLICY_LOSS and TRAIN_VALUE_LOSS_WEIGHT, passed beside the controls'."""
    return dict(policy_loss=TRAIN_POLICY_LOSS, value_loss_weight=TRAIN_VALUE_LOSS_WEIGHT)


def _loss_form(trainer):
    """(policy form 0 / 1, value weight) of `trainer`; one that does not know the option (None included) has the reference's."""
    return check_loss_controls(getattr(trainer, "policy_loss", "reference"), getattr(trainer, "value_loss_weight", 1.0))


def _cross_entropy(trainer):
    """Whether `trainer` minimises the cross-entropy form (what the progress line and the validation then print and score)."""
    return _loss_form(trainer)[0] == 1


def _validation_loss(metrics, trainer):
    """(the held-out policy loss in the form `trainer` minimises, the score of TRAIN_HOLDOUT_KEEP_BEST = the loss the update
    minimises) of a validation.Metrics: policy_loss and policy_loss + value_mse with the reference's form and weight 1, as always;
    under the cross-entropy the table's ce column and ce + w * value_mse."""
    form, w = _loss_form(trainer)
    policy = metrics.policy_ce if form == 1 else metrics.policy_loss
    return policy, (policy + metrics.value_mse if w == 1.0 else policy + w * metrics.value_mse)


def _progress_line(epoch, policy_loss, value_loss, trainer, val=None):
    """The per-epoch progress line (train_network.py:100); with clipping on, the epoch's mean gradient norm beside it (one host read of
    grad_norms per epoch); val (a validation.Metrics of this epoch): the held-out numbers behind it."""
    name = "Policy Loss (CE)" if _cross_entropy(trainer) else "Policy Loss"
    line = f"\rEpoch {epoch + 1}/{NUM_EPOCH} | {name}: {float(policy_loss):.4f} | Value Loss: {float(value_loss):.4f}"
    if trainer.max_grad_norm and trainer.grad_norms.numel():
        line += f" | Grad Norm: {float(trainer.grad_norms.mean()):.4f}"
    if val is not None:
        line += f" | Val Loss: {_validation_loss(val, trainer)[0]:.4f} / {val.value_mse:.4f} | Val KL: {val.kl:.4f} | Top-1: {val.top1:.3f}"
    return line


class _Holdout:
    """The held-out side of one update (_update_rows' held dict): validates the network that would be saved now, keeps the curve and,
    with TRAIN_HOLDOUT_KEEP_BEST, the snapshot of the best validated epoch.  With a weight average the network validated is a twin
    module, built once through `load` and filled by average.copy_to(twin) at every validation; otherwise the model itself.  Every rank
    holds one and decides alike: no collective."""

    def __init__(self, held, model, average, load, dev, trainer=None):
        from .replay_reference import check_holdout_options
        self.trainer = trainer                  # its loss form decides the score; None: the reference's
        self.share, self.seed, self.every = check_holdout_options(TRAIN_HOLDOUT_SHARE, TRAIN_HOLDOUT_SEED, TRAIN_HOLDOUT_EVERY)
        self.keep_best = bool(TRAIN_HOLDOUT_KEEP_BEST)
        self.rows, self.index, self.counts = held["rows"], held["index"], held["counts"]
        self.model, self.average = model, average
        self.twin = None if average is None else load(PV_NETWORK_PATH + 'best.pth', dev)
        self.curve, self.last, self.best, self.best_epoch, self.best_score, self.snapshot = [], None, None, None, None, None

    def due(self, epoch):
        return (epoch + 1) % self.every == 0 or epoch + 1 == NUM_EPOCH

    def validate(self, epoch):
        """The Metrics of the network that would be saved after `epoch` (0-based), added to the curve."""
        from .validation import row_metrics
        target = self.model
        if self.average is not None:
            self.average.copy_to(self.twin)
            target = self.twin
        self.last = row_metrics(target, *self.rows, self.index)
        score = _validation_loss(self.last, self.trainer)[1]            # the loss the update minimises, in the trainer's form
        self.curve.append(dict(epoch=epoch + 1, score=score, **self.last.totals()))
        if self.best_score is None or score < self.best_score:          # on ties the first minimum stays
            self.best, self.best_epoch, self.best_score = self.last, epoch + 1, score
            if self.keep_best:
                self.snapshot = self._saved_now()
        return self.last

    def _saved_now(self):
        """What torch.save would write now, as device clones: the average's tensors with a weight average, else the model's."""
        if self.average is not None:
            return self.average.state_dict()
        state = self.model.state_dict()                                  # the OrderedDict itself is kept: its _metadata is saved too
        for k in state:
            state[k] = state[k].detach().clone()
        return state

    def saved(self):
        """The Metrics of the network that is saved: the kept epoch's with TRAIN_HOLDOUT_KEEP_BEST, else the last validation's."""
        return self.best if self.keep_best else self.last

    def report(self):
        lines = []
        if self.keep_best:
            form, w = _loss_form(self.trainer)
            what = "policy loss + value MSE"
            if (form, w) != (0, 1.0):
                what = f"{'policy CE' if form == 1 else 'policy loss'} + {w:g} x value MSE"
            lines.append(f"kept epoch {self.best_epoch}/{NUM_EPOCH}: held-out {what} = {self.best_score:.4f}")
        lines.append(self.saved().table())
        return "\n".join(lines)

    def log_line(self):
        """The JSON line of TRAIN_HOLDOUT_LOG: the curve, the per-bucket table of the saved network, the split's counts, the options
        in force.  A number that is not finite (a ratio over no row) is written as null."""
        import json
        options = dict(share=self.share, seed=self.seed, every=self.every, keep_best=self.keep_best, epochs=NUM_EPOCH,
                       ema_decay=TRAIN_EMA_DECAY, ema_every=TRAIN_EMA_EVERY, merge_positions=bool(TRAIN_MERGE_POSITIONS),
                       surprise_weighting=bool(TRAIN_SURPRISE_WEIGHTING), mirror=bool(TRAIN_MIRROR), epoch_rows=TRAIN_EPOCH_ROWS,
                       weight_decay=TRAIN_WEIGHT_DECAY, max_grad_norm=TRAIN_MAX_GRAD_NORM)
        form, w = _loss_form(self.trainer)
        if (form, w) != (0, 1.0):                                         # (the line is what it was with the option off)
            options.update(policy_loss="cross_entropy" if form == 1 else "reference", value_loss_weight=w)
        record = dict(curve=self.curve, saved_epoch=self.best_epoch if self.keep_best else self.curve[-1]["epoch"],
                      table=self.saved().as_dict(), split=self.counts, options=options)
        return json.dumps(_finite_or_none(record))


def _finite_or_none(x):
    if isinstance(x, dict):
        return {k: _finite_or_none(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_finite_or_none(v) for v in x]
    if isinstance(x, float) and not np.isfinite(x):
        return None
    return x


CNN_TRAINING_NOT_BUILT = ("training the residual CNN through train_network() / trainer_for(), the GNN entry points, is not built "
                          "yet: use CNNTrainer / train_cnn_network(), or train_cycle, which dispatches")


def trainer_for(model, max_batch=BATCH_SIZE):
    """GNNTrainer for the default 6/128/3 network (the fused step), GeneralTrainer for every other shape, with the configured
    optimiser controls (TRAIN_WEIGHT_DECAY, TRAIN_DECOUPLED, TRAIN_MAX_GRAD_NORM) and loss form (TRAIN_POLICY_LOSS,
    TRAIN_VALUE_LOSS_WEIGHT)."""
    from .pv_network_cnn import CNNNetwork
    if isinstance(model, CNNNetwork):
        raise NotImplementedError(CNN_TRAINING_NOT_BUILT)
    kind = GNNTrainer if getattr(model, "fused", False) else GeneralTrainer
    return kind(model, max_batch=max_batch, **_configured_controls(), **_configured_loss())


def train_network():
    """train_network.py:26-107 on the GNN: best.pth -> NUM_EPOCH epochs over the newest .history -> latest.pth.

    Under torch.distributed rank 0 trains ALONE by default and the others wait at the barrier: a step at the reference's batch
    size (128) is a latency-bound 0.083 ms on one GPU; dealt over W ranks every rank would still run its (shorter-gridded but
    equally long) board kernel and add two collectives per step, i.e. data parallelism makes this loop slower, not faster.
    AQG_TRAIN_DATA_PARALLEL=1 selects the data-parallel form anyway (same shuffle on all ranks, the positions of every batch
    dealt out over the ranks, one all-reduce of the flat gradient buffer per step, GNNTrainer.step); rank 0 writes latest.pth."""
    import os
    from .pv_network_cnn import is_cnn_state_dict
    best = PV_NETWORK_PATH + 'best.pth'
    if os.path.exists(best) and is_cnn_state_dict(torch.load(best, map_location="cpu", weights_only=True)):
        raise NotImplementedError(CNN_TRAINING_NOT_BUILT)
    _train(load_network, trainer_for, data_parallel=os.environ.get("AQG_TRAIN_DATA_PARALLEL", "0") == "1")


def train_cnn_network():
    """train_network.py:26-107 on the reference's residual CNN: best.pth (a CNNNetwork of any shape) -> NUM_EPOCH epochs over the
    newest .history, every step on HIP (CNNTrainer) -> latest.pth with every state_dict key (202 at 128 filters x 16 blocks).
    Under torch.distributed rank 0 trains alone and the others wait (synchronised BatchNorm is not built)."""
    from .pv_network_cnn import load_network as load_cnn
    _train(load_cnn, lambda model, max_batch: CNNTrainer(model, max_batch=max_batch, **_configured_controls(), **_configured_loss()),
           data_parallel=False)


def _train(load, make_trainer, data_parallel):
    """The epochs of _train_loop on this process alone, on every rank of the process group (data_parallel), or else on rank 0 ALONE
    while the other ranks wait."""
    import torch.distributed as dist
    rank, world = aqd.rank_world()
    if world == 1 or data_parallel:
        return _train_loop(load, make_trainer, rank, world)
    tag = aqd.next_tag("train")
    if rank == 0:
        with aqd.single_rank_stage(tag):       # published on failure too (value b"fail"): the idle ranks raise instead of waiting
            _train_loop(load, make_trainer, 0, 1)
    else:
        aqd.wait_for_rank0(tag)     # host-side wait on the rendezvous store: no collective is pending while rank 0 trains, so
                                    # the stage may outlast the process group's watchdog timeout (distributed.py)
    dist.barrier()          # latest.pth is complete before any rank moves on to the evaluation stage


def _train_loop(load, make_trainer, rank, world):
    """best.pth through `load`, NUM_EPOCH epochs on the trainer `make_trainer(model, max_batch=)` gives, latest.pth.  world > 1: the
    data-parallel form, every batch dealt out over the ranks."""
    import torch.distributed as dist
    dev = aqd.device()                                                             # this rank's GPU, explicitly
    model = load(PV_NETWORK_PATH + 'best.pth', dev)                                # GNNNetwork, or the shape best.pth holds
    s, p, v, index, held = _update_rows(dev, model.board_size, model=model)
    n = s.shape[0] if index is None else index.shape[0]
    trainer = make_trainer(model, max_batch=BATCH_SIZE)
    # every rank keeps its own average of its own (identical) parameters: no collective
    average = None if TRAIN_EMA_DECAY is None else WeightAverage(trainer, decay=TRAIN_EMA_DECAY, every=TRAIN_EMA_EVERY)
    holdout = None if held is None else _Holdout(held, model, average, load, dev, trainer)      # every rank validates and decides alike
    for epoch in range(NUM_EPOCH):
        lr = LEARNING_RATE * lr_lambda(epoch)                                      # LambdaLR, stepped once per epoch (:98)
        perm = torch.randperm(n, device=dev)                                    # DataLoader(shuffle=True), last batch kept
        if world > 1:
            if dist.get_backend() == 'nccl':
                dist.broadcast(perm, src=0)
            else:                                                                  # gloo (tests): host tensors only
                perm_h = perm.cpu()
                dist.broadcast(perm_h, src=0)
                perm = perm_h.to(dev)
        mirror = (TRAIN_MIRROR_SEED, epoch) if TRAIN_MIRROR else None
        order = _epoch_order(perm, index)
        if world == 1:
            epoch_policy_loss, epoch_value_loss = trainer.run_epoch(s, p, v, order, lr=lr, mirror=mirror)
        else:
            epoch_policy_loss = torch.zeros((), device=dev)
            epoch_value_loss = torch.zeros((), device=dev)
            for i in range(0, int(order.shape[0]), BATCH_SIZE):
                idx = order[i:i + BATCH_SIZE][rank::world]
                if mirror is None:
                    pl, vl = trainer.step(s[idx], p[idx], v[idx], lr=lr)
                else:       # this rank's slice, gathered and flipped by SOURCE row under the key every rank shares: no collective
                    pl, vl = trainer.step(*_augment_launch(model.board_size, s, p, v, idx.contiguous(), mirror), lr=lr)
                epoch_policy_loss += pl
                epoch_value_loss += vl
        val = holdout.validate(epoch) if holdout is not None and holdout.due(epoch) else None
        if rank == 0:
            print(_progress_line(epoch, epoch_policy_loss, epoch_value_loss, trainer, val), end='')
    if rank == 0:
        print('')
        if average is not None:
            print(average.summary_line())
        if holdout is not None and NUM_EPOCH > 0:
            print(holdout.report())
            if TRAIN_HOLDOUT_LOG is not None:
                with open(TRAIN_HOLDOUT_LOG, "a") as f:
                    f.write(holdout.log_line() + "\n")
        if holdout is not None and holdout.keep_best and holdout.snapshot is not None:
            torch.save(holdout.snapshot, PV_NETWORK_PATH + 'latest.pth')
        else:
            torch.save(model.state_dict() if average is None else average.state_dict(), PV_NETWORK_PATH + 'latest.pth')
    if world > 1:
        dist.barrier()          # latest.pth is complete before any rank moves on to the evaluation stage


if __name__ == '__main__':
    train_network()
