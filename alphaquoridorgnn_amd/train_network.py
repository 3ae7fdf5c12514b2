"""Parameter update -- drop-in for the reference's train_network.py, on the GNN, with the whole optimisation step in HIP.

Call surface kept (train_network.py:14-107): NUM_EPOCH, BATCH_SIZE, load_data, train_network.  One step = one C call
(`aqg_gcn_train_step`, csrc/gcn_train.hip): forward, the reference's losses (CrossEntropyLoss on the already-softmaxed
policy + MSELoss, train_network.py:54-55,85-86), backward, Adam (:56,:90-92), all fp32.  The parameters updated are the
model's own state_dict tensors; torch is used for memory, shuffling and the .pth / .history files only.
"""
import ctypes
import pickle
from pathlib import Path

import numpy as np
import torch

from . import _lib
from .constants import PV_NETWORK_PATH, BOARD_SIZE, num_actions
from .pv_network_gnn import STATE_DICT_KEYS, HIDDEN_DIM, NUM_FEATURES, load_network, pack_states

NUM_EPOCH = 100    # train_network.py:14
BATCH_SIZE = 128   # train_network.py:15
LEARNING_RATE = 0.001   # train_network.py:56
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
# HIP steps (include/aqgnn.h "weight averaging", WeightAverage below) and saved as latest.pth in place of the last iterate.
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
    import torch.distributed as dist
    s, p, v, index = _recorded_rows(dev, board_size)
    rank0 = not (dist.is_available() and dist.is_initialized()) or dist.get_rank() == 0
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
    window = TRAIN_WINDOW if TRAIN_WINDOW is not None and len(TRAIN_WINDOW) > 0 else None
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


def _recorded_rows(dev, board_size):
    """_training_rows before any merge: one row per occurrence."""
    from .replay import ReplayWindow
    window = TRAIN_WINDOW if TRAIN_WINDOW is not None and len(TRAIN_WINDOW) > 0 else None
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


def draw_mirror_flips(seed, epoch, n):
    """The flips of source rows 0 .. n-1 in epoch `epoch` under `seed`, uint8 [n] -- the seeded draw of aqg_augment_gather in numpy
    (include/aqgnn.h): row r is mirrored iff f(K(seed, epoch), r) < 0.5 with the counter-based generator of agents.draw_uniforms.
    A pure function of (seed, epoch, r): a prefix of a longer draw is the shorter draw."""
    from .agents import draw_uniforms
    return (draw_uniforms(seed, epoch, n) < 0.5).astype(np.uint8)


def _mirror_arguments(mirror, rows, dev):
    """(flips tensor or None, use_seed, seed, epoch) of a `mirror` argument: a uint8 [rows] device table indexed by source row, or
    (seed, epoch).  Shapes and types only -- nothing is read back from the device."""
    if isinstance(mirror, torch.Tensor):
        if mirror.dtype != torch.uint8 or mirror.dim() != 1 or mirror.shape[0] != rows or mirror.device != dev:
            raise ValueError(f"a mirror table is a uint8 [{rows}] tensor on {dev}, one entry per source row")
        return mirror.contiguous(), 0, 0, 0
    try:
        seed, epoch = mirror
        seed, epoch = int(seed), int(epoch)
    except (TypeError, ValueError):
        raise ValueError("mirror is None, a uint8 device table indexed by source row, or (seed, epoch)") from None
    if epoch < 0:
        raise ValueError("mirror: the epoch must be >= 0")
    return None, 1, seed & ((1 << 64) - 1), epoch


def _augment_launch(board_size, states72, pi, z, order, mirror):
    """The fused launch on contiguous device tensors of one device: (out72, out_pi, out_z), None where the input is None.  order:
    int64 source rows, NOT checked here (augment_gather checks them); mirror: as _mirror_arguments, or None for a plain gather."""
    src = next(x for x in (states72, pi, z) if x is not None)
    dev, rows = src.device, int(src.shape[0])
    n = rows if order is None else int(order.shape[0])
    flips, use_seed, seed, epoch = (None, 0, 0, 0) if mirror is None else _mirror_arguments(mirror, rows, dev)
    outs = [None if x is None else torch.empty((n,) + tuple(x.shape[1:]), dtype=x.dtype, device=dev) for x in (states72, pi, z)]
    A = num_actions(board_size)
    _lib.check(_lib.load().aqg_augment_gather(board_size, A, _lib.ptr(states72), _lib.ptr(pi), _lib.ptr(z), _lib.ptr(order),
                                              _lib.ptr(flips), use_seed, seed, epoch, n, _lib.ptr(outs[0]), _lib.ptr(outs[1]),
                                              _lib.ptr(outs[2]), _lib.stream_ptr(dev)), "aqg_augment_gather")
    return tuple(outs)


def augment_gather(states72, pi, z, order=None, flips=None, seed=None, epoch=0, board_size=BOARD_SIZE):
    """Gather and mirror training rows in one launch (aqg_augment_gather): output row i is source row order[i] (None: row i),
    mirrored iff flips[that source row] is set -- or, with flips None and a seed, iff draw_mirror_flips(seed, epoch, rows) says so.
    With neither it is a plain gather.  states72 uint8 [rows,72], pi float32 [rows,A], z float32 [rows]: device tensors, each may be
    None (and so is its output).  Returns (out72, out_pi, out_z), freshly allocated, with len(order) rows (any number, none
    included).  order is checked against the row count with one host read."""
    given = [x for x in (states72, pi, z) if x is not None]
    if not given:
        raise ValueError("augment_gather: at least one of states72, pi, z is needed")
    dev = _lib.require_gpu(given[0].device)
    rows = int(given[0].shape[0])
    A = num_actions(board_size)
    for x, name, dtype, tail in ((states72, "states72", torch.uint8, (72,)), (pi, "pi", torch.float32, (A,)), (z, "z", torch.float32, ())):
        if x is not None and (x.device != dev or x.dtype != dtype or tuple(x.shape) != (rows,) + tail):
            raise ValueError(f"augment_gather: {name} must be a {dtype} {[rows, *tail]} tensor on {dev} ({board_size}x{board_size} board)")
    states72, pi, z = (None if x is None else x.contiguous() for x in (states72, pi, z))
    if order is not None:
        order = order.to(dev, torch.int64).contiguous()
        if order.dim() != 1:
            raise ValueError("augment_gather: order is a 1-D tensor of source rows")
        if order.numel():
            lo, hi = torch.stack((order.min(), order.max())).tolist()          # the one host read
            if lo < 0 or hi >= rows:
                raise ValueError(f"augment_gather: order holds a row outside 0..{rows - 1}")
    if flips is not None and seed is not None:
        raise ValueError("augment_gather: give flips or seed, not both")
    mirror = flips if flips is not None else None if seed is None else (seed, epoch)
    return _augment_launch(board_size, states72, pi, z, order, mirror)


def clip_coefficient(norm, max_norm):
    """The factor torch.nn.utils.clip_grad_norm_(params, max_norm) multiplies every gradient by, in float32 as the kernels take it:
    min(1, max_norm / (norm + 1e-6)) -- exactly 1.0 when nothing is clipped; a NaN norm gives NaN (torch.clamp's minimum)."""
    c = np.float32(max_norm) / (np.float32(norm) + np.float32(1e-6))
    return np.float32(1.0) if c > np.float32(1.0) else np.float32(c)


def adam_reference(p, g, m, v, step, lr=LEARNING_RATE, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=True, coef=1.0):
    """One update of one tensor as the finish kernels take it (csrc/train_adam.hpp), in numpy float32: clip (g <- coef g), weight
    decay (decoupled, torch.optim.AdamW: p <- p (1 - lr wd); coupled, torch.optim.Adam(weight_decay=): g <- g + wd p), then
    torch.optim.Adam's update with the bias corrections of `step` (1-based) computed in float64.  Returns (p, m, v), new arrays."""
    f = np.float32
    p, g, m, v = (np.asarray(x, dtype=f) for x in (p, g, m, v))
    lr, b1, b2, eps, wd = f(lr), f(betas[0]), f(betas[1]), f(eps), f(weight_decay)
    g = f(coef) * g
    if wd != 0:
        if decoupled:
            p = p * (f(1) - lr * wd)
        else:
            g = g + wd * p
    bc1 = f(1.0 - float(b1) ** step)
    bc2_sqrt = f(np.sqrt(1.0 - float(b2) ** step))
    m = b1 * m + (f(1) - b1) * g
    v = b2 * v + (f(1) - b2) * g * g
    denom = np.sqrt(v) / bc2_sqrt + eps
    return p - (lr / bc1) * (m / denom), m, v


def default_decay_mask(params, decay_all=False):
    """Which tensors weight decay applies to: those of two or more dimensions (GCN and linear weights, conv kernels) -- not biases,
    not BatchNorm weight and bias -- unless decay_all."""
    return [bool(decay_all) or p.dim() >= 2 for p in params]


def grad_norm(t):
    """The L2 norm of a contiguous float32 device tensor (or view), as a 0-dim device tensor: the deterministic two-stage reduction
    of gradient clipping (aqg_grad_norm, csrc/grad_norm.hip), no host read."""
    if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() < 1:
        raise ValueError("grad_norm takes a non-empty contiguous float32 tensor")
    dev = _lib.require_gpu(t.device)
    lib = _lib.load()
    n = int(t.numel())
    nws = int(lib.aqg_optim_workspace_floats(n))
    if nws == 0:
        _lib.check(-1, "aqg_optim_workspace_floats (more elements than the reduction takes)")
    ws = torch.empty((nws,), dtype=torch.float32, device=dev)
    out = torch.empty((1,), dtype=torch.float32, device=dev)
    _lib.check(lib.aqg_grad_norm(_lib.ptr(t), n, _lib.ptr(out), _lib.ptr(ws), nws, _lib.stream_ptr(dev)), "aqg_grad_norm")
    return out[0]


def weight_average_reference(avg, src, decay):
    """One update of the weight average (include/aqgnn.h "weight averaging") in numpy float32: with d = float32(decay) and
    w = float32(1.0 - float(d)), e' = f32(d * e) + f32(w * p) -- two rounded products and one rounded sum, bit for bit
    torch.optim.swa_utils.get_ema_avg_fn(float(d)) on CPU tensors.  Returns a new array."""
    f = np.float32
    d = f(decay)
    w = f(1.0 - float(d))
    return d * np.asarray(avg, dtype=f) + w * np.asarray(src, dtype=f)


def weight_average_due(step, every):
    """Whether the average is updated behind the Adam update of 1-based step `step`: at the multiples of `every`, wherever an epoch
    or a library call ends."""
    return int(step) % int(every) == 0


def weight_average_table(averages, sources):
    """The launch's tensor table (include/aqgnn.h "weight averaging") of device tensors averages[i] <- sources[i]: (the host copy, a
    ctypes int64 array of 4 T + 1 words; the device copy, an int64 tensor; the total number of chunks).  Pointers, element counts
    and the prefix of the per-tensor chunk counts, a chunk being 4,096 floats of the 16-byte grid the average's base sits in."""
    T, C = len(averages), _lib.WEIGHT_AVERAGE_CHUNK
    prefix = [0]
    for e in averages:
        prefix.append(prefix[-1] + (e.numel() + ((e.data_ptr() >> 2) & 3) + C - 1) // C)
    words = [e.data_ptr() for e in averages] + [p.data_ptr() for p in sources] + [p.numel() for p in sources] + prefix
    return (ctypes.c_int64 * (4 * T + 1))(*words), torch.tensor(words, dtype=torch.int64, device=averages[0].device), prefix[-1]


def _checked_average_controls(decay, every):
    """(decay as the float32 the kernel takes, every as int), refused as the library refuses them."""
    try:
        d = np.float32(decay)
    except (TypeError, ValueError):
        raise ValueError("the weight average's decay is a number in [0, 1)") from None
    if not (d >= 0 and d < 1):                               # a NaN fails both; a decay that rounds to 1.0f is refused too
        raise ValueError(f"the weight average's decay must be in [0, 1) as a float32 (got {decay!r})")
    if isinstance(every, bool) or not isinstance(every, (int, np.integer)) or every < 1:
        raise ValueError(f"the weight average's every must be an integer >= 1 (got {every!r})")
    return float(d), int(every)


class _Trainer:
    """What the three trainers share: the Adam state and the flat gradient buffer, the optimiser controls, step() (single process or
    data parallel), outputs() and run_epoch().  A subclass names its library calls (_STEP, _STEPS) and provides the batch-mean losses
    of a single-process step (_batch_losses) and what an update must tell the model (_updated).

    Optimiser controls (all off by default: the plain entry points, the same launches as ever): weight_decay (torch's coefficient) on
    the tensors default_decay_mask picks (every tensor with decay_all), decoupled as torch.optim.AdamW (True) or coupled as
    torch.optim.Adam(weight_decay=) (False), and max_grad_norm = torch.nn.utils.clip_grad_norm_'s max_norm (None or 0 = off).  They
    are plain attributes read at every call, so a schedule may change them between steps.  With clipping on, last_grad_norm is the
    unclipped global gradient norm of the last step (0-dim device tensor) and grad_norms that of every step of the last run_epoch
    (device tensor [steps]); neither is read by the host."""

    _GPU_REFUSAL = None       # a subclass's own words for a model that is not on the GPU (raised in front of require_gpu's)

    def _setup(self, model, params, max_batch, betas, eps, controls, buffers=(), workspace=None):
        """The constructors' shared part: the checks of `params` (and `buffers`, tensors the kernels write besides them), the Adam
        state with every gradient a view of ONE flat buffer (the data-parallel exchange is a single all-reduce), the optimiser
        controls and the counters.  workspace, for the two workspace trainers: (the library's workspace-size call, its shape
        arguments in front of the batch); their outputs and workspace are allocated here."""
        self.model, self.lib, self.params, self.buffers = model, _lib.load(), list(params), list(buffers)
        what = "parameters and running statistics" if self.buffers else "parameters"
        for x in self.params + self.buffers:
            if x.dtype != torch.float32 or not x.is_contiguous():
                raise ValueError(f"training needs contiguous float32 {what}")
        if self._GPU_REFUSAL and self.params[0].device.type != "cuda":
            raise ValueError(self._GPU_REFUSAL)
        self.dev = _lib.require_gpu(self.params[0].device)
        if any(x.device != self.dev for x in self.params + self.buffers):
            raise ValueError(f"every {'parameter and running statistic' if self.buffers else 'parameter'} must be on the trainer's GPU")
        self.flat_grads = torch.zeros((sum(p.numel() for p in self.params),), dtype=torch.float32, device=self.dev)
        self.grads, off = [], 0
        for p in self.params:
            self.grads.append(self.flat_grads[off:off + p.numel()].view_as(p))
            off += p.numel()
        self.adam_m = [torch.zeros_like(p) for p in self.params]
        self.adam_v = [torch.zeros_like(p) for p in self.params]
        self.weight_decay, self.decoupled, self.decay_all, self.max_grad_norm = controls
        self.last_grad_norm = torch.zeros((), dtype=torch.float32, device=self.dev)
        self.grad_norms = torch.zeros((0,), dtype=torch.float32, device=self.dev)
        self._optim_ws = None
        self.average = None                       # a WeightAverage attaches itself here: the calls then take their _avg forms
        self.N, self.A = model.board_size, model.policy_output_size
        self.max_batch, self.step_count = int(max_batch), 0
        self.betas, self.eps = betas, eps
        if workspace is not None:
            if self.max_batch < 1:
                raise ValueError("max_batch must be >= 1")
            name, shape = workspace
            nws = int(getattr(self.lib, name)(self.N, *shape, self.A, self.max_batch))
            if nws == 0:
                _lib.check(-1, f"{name} (shape or board size outside the kernels' limits)")
            f = dict(dtype=torch.float32, device=self.dev)
            self.ws = dict(workspace=torch.empty((nws,), **f), pol=torch.empty((self.max_batch, self.A), **f),
                           val=torch.empty((self.max_batch,), **f), loss=torch.empty((self.max_batch, 2), **f),
                           loss_mean=torch.zeros((2,), **f))

    def _fill(self, t):
        """What every trainer's struct takes the same way: the board, Adam's constants, the params / grads / adam_m / adam_v pointer
        arrays where the struct has them, and the workspace trainers' outputs and workspace."""
        self.t = t
        t.board_size, t.policy_size = self.N, self.A
        t.beta1, t.beta2, t.eps = float(self.betas[0]), float(self.betas[1]), float(self.eps)
        for name in ("params", "grads", "adam_m", "adam_v"):
            for i, x in enumerate(getattr(self, name) if hasattr(t, name) else ()):
                getattr(t, name)[i] = x.data_ptr()
        if "workspace" in self.ws:
            t.policy, t.value, t.loss, t.loss_mean = (self.ws[k].data_ptr() for k in ("pol", "val", "loss", "loss_mean"))
            t.workspace, t.workspace_floats = self.ws["workspace"].data_ptr(), self.ws["workspace"].numel()

    def _optim(self, steps):
        """(aqg_optim for a call of `steps` steps, the device tensor its norms go to) -- (None, None) with every control off."""
        wd = float(self.weight_decay or 0.0)
        clip = float(self.max_grad_norm or 0.0)
        if wd == 0.0 and clip == 0.0:
            return None, None
        o = _lib.OptimStruct()
        o.decoupled = 1 if self.decoupled else 0
        if wd != 0.0:
            mask = default_decay_mask(self.params, self.decay_all)
            o.num_tensors = len(mask)
            o._wd = (ctypes.c_float * len(mask))(*[wd if d else 0.0 for d in mask])       # kept alive by the struct object
            o.weight_decay = ctypes.cast(o._wd, ctypes.POINTER(ctypes.c_float))
        norms = None
        if clip != 0.0:
            if self._optim_ws is None:
                nws = int(self.lib.aqg_optim_workspace_floats(self.flat_grads.numel()))
                self._optim_ws = torch.empty((nws,), dtype=torch.float32, device=self.dev)
            norms = torch.zeros((steps,), dtype=torch.float32, device=self.dev)
            o.max_grad_norm = clip
            o.grad_norm = norms.data_ptr()
            o.workspace, o.workspace_floats = self._optim_ws.data_ptr(), self._optim_ws.numel()
        return o, norms

    def _invoke(self, name, args, steps, plain=False, updating=True):
        """One library call of `steps` steps: `name` itself when plain or with every control off (no aqg_optim is built), its
        _optim form otherwise -- or, with a weight average attached and a call that updates, its _avg form (the controls' struct or
        NULL beside the average's).  Returns the device tensor the call's norms went to, or None."""
        o, norms = (None, None) if plain else self._optim(steps)
        average = None if plain or not updating else self.average
        if average is not None:
            a = average._struct()
            name, controls = name + "_avg", (None if o is None else ctypes.byref(o), ctypes.byref(a))
        else:
            name, controls = (name, ()) if o is None else (name + "_optim", (ctypes.byref(o),))
        _lib.check(getattr(self.lib, name)(ctypes.byref(self.t), *args, *controls, _lib.stream_ptr(self.dev)), name)
        if average is not None:
            average._stepped(int(self.t.step), steps, a.every)
        return norms

    def _call(self, states72, pi_target, z_target, mode, plain=False):
        norms = self._invoke(self._STEP, (_lib.ptr(states72), _lib.ptr(pi_target), _lib.ptr(z_target), mode), 1, plain,
                             updating=mode >= 1)
        if norms is not None:
            self.last_grad_norm = norms[0]

    def step(self, states72, pi_target, z_target, lr=LEARNING_RATE, update=True, group=None, mirror=None):
        """One optimisation step.  states72 uint8 [B,72], pi_target float32 [B,A], z_target float32 [B] (device tensors).
        Returns (policy_loss, value_loss) as 0-dim device tensors -- no host synchronisation.
        mirror (None = off): a uint8 [B] device table, or (seed, epoch) for the seeded draw keyed by the row's index in THIS batch:
        the step trains on the batch with those rows mirrored left to right (one launch in front of it, aqg_augment_gather).

        Data parallel (torch.distributed initialised, world > 1): every rank passes ITS shard of the global batch; the
        local mean-loss gradients are weighted by B_local / B_global, summed with ONE all-reduce of the flat gradient buffer
        (RCCL over xGMI with backend nccl) and applied by every rank, so all replicas take the step a single process would
        take on the whole batch (up to fp32 summation order)."""
        import torch.distributed as dist
        B = int(states72.shape[0])
        if B > self.max_batch:
            raise ValueError("batch larger than the trainer's workspace")
        states72 = states72.to(self.dev, torch.uint8).contiguous()
        pi_target = pi_target.to(self.dev, torch.float32).contiguous()
        z_target = z_target.to(self.dev, torch.float32).contiguous()
        if mirror is not None:
            states72, pi_target, z_target = _augment_launch(self.N, states72, pi_target, z_target, None, mirror)
        world = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
        if update:
            self.step_count += 1
        self.t.batch, self.t.step, self.t.lr = B, max(self.step_count, 1), float(lr)
        if world == 1:
            self._call(states72, pi_target, z_target, 1 if update else 0)
            loss = self._batch_losses(B) if B else torch.zeros((2,), device=self.dev)
        else:
            if B:
                self._call(states72, pi_target, z_target, 0, plain=True)      # the norm that counts is the all-reduced gradient's
                lsum = self.ws["loss"][:B].sum(dim=0)
            else:                                                  # a rank may hold no position of a ragged last batch
                self.flat_grads.zero_()
                lsum = torch.zeros((2,), device=self.dev)
            tot = torch.cat([lsum, torch.tensor([float(B)], device=self.dev)])
            dist.all_reduce(tot, group=group)                      # global loss sums and global batch size
            self.flat_grads.mul_(float(B) / tot[2])                # local mean-loss gradient -> its share of the global mean
            dist.all_reduce(self.flat_grads, group=group)
            if update:
                self._call(states72, pi_target, z_target, 2)
            loss = tot[:2] / tot[2]
        if update:
            self._updated()
        return loss[0], loss[1]

    def outputs(self, B):
        """(policy [B,A], value [B]) of the last step's forward pass."""
        return self.ws["pol"][:B], self.ws["val"][:B]

    def run_epoch(self, states72, pi_target, z_target, order, lr=LEARNING_RATE, batch=None, pre_shuffle=True, mirror=None):
        """All optimisation steps of one epoch in ONE library call (single process): step i trains on the positions
        order[i*batch:(i+1)*batch] of the resident device arrays (train_network.py:72-95; the short last batch is kept, as
        DataLoader does).  Returns the epoch's summed (policy_loss, value_loss) as a device tensor [2] -- no host sync.
        mirror (None = off): a uint8 device table with one entry per row of states72, or (seed, epoch) for the seeded draw
        (draw_mirror_flips): the rows it selects are trained on mirrored left to right.  The epoch's three gathers become one fused
        gather + flip launch (aqg_augment_gather), so a mirrored epoch needs pre_shuffle=True."""
        if mirror is not None and not pre_shuffle:
            raise ValueError("a mirrored epoch trains on the shuffled and flipped copies: it needs pre_shuffle=True")
        batch = self.max_batch if batch is None else int(batch)
        if batch > self.max_batch:
            raise ValueError("batch larger than the trainer's workspace")
        n = int(order.shape[0])
        sums = torch.zeros((2,), dtype=torch.float32, device=self.dev)
        if n == 0:
            return sums
        # The shuffle is applied ONCE per epoch (three gathers, ~1 KB per position) and the steps then index the shuffled
        # copies directly: every kernel of a step starts with cold loads, and reading order[] first would put one more
        # HBM round trip in front of each of them.  (The C entry points also take the order itself: order != NULL.)
        order = order.to(self.dev, torch.int64).contiguous()
        states72 = states72.to(self.dev, torch.uint8).contiguous()
        pi_target = pi_target.to(self.dev, torch.float32).contiguous()
        z_target = z_target.to(self.dev, torch.float32).contiguous()
        if mirror is not None:
            states72, pi_target, z_target = _augment_launch(self.N, states72, pi_target, z_target, order, mirror)
        elif pre_shuffle:
            states72, pi_target, z_target = (x.index_select(0, order).contiguous() for x in (states72, pi_target, z_target))
        self.t.batch, self.t.step, self.t.lr = batch, self.step_count + 1, float(lr)
        steps = (n + batch - 1) // batch
        norms = self._invoke(self._STEPS, (_lib.ptr(states72), _lib.ptr(pi_target), _lib.ptr(z_target),
                                           _lib.ptr(None if pre_shuffle else order), n, _lib.ptr(sums)), steps)
        if norms is not None:
            self.grad_norms, self.last_grad_norm = norms, norms[-1]
        self.step_count += steps
        self._updated()
        return sums


class GNNTrainer(_Trainer):
    """Adam state + workspace for optimisation steps of up to `max_batch` positions on `model` (a GNNNetwork on the GPU)."""

    _STEP, _STEPS = "aqg_gcn_train_step", "aqg_gcn_train_steps"

    def __init__(self, model, max_batch=BATCH_SIZE, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=True, decay_all=False,
                 max_grad_norm=None):
        if not getattr(model, "fused", True):
            model._require_fused("GNNTrainer (the fused training kernels)")
        sd = model.state_dict()
        self._setup(model, [sd[k] for k in STATE_DICT_KEYS], max_batch, betas, eps, (weight_decay, decoupled, decay_all, max_grad_norm))
        self.V = self.N * self.N
        B, A, H = self.max_batch, self.A, HIDDEN_DIM
        f = dict(dtype=torch.float32, device=self.dev)
        self.ws = dict(
            h1=torch.empty((B * 96, H), **f), h2=torch.empty((B * 96, H), **f),    # 96 rows per position: include/aqgnn.h
            g=torch.empty((B, H), **f), hp=torch.empty((B, H // 2), **f),
            hv=torch.empty((B, H // 2), **f), dhp=torch.empty((B, H // 2), **f), dhv=torch.empty((B, H // 2), **f),
            lg=torch.empty((B, A), **f), pol=torch.empty((B, A), **f), vp=torch.empty((B,), **f), val=torch.empty((B,), **f),
            loss=torch.empty((B, 2), **f), part=torch.empty((B * _lib.TRAIN_PART_FLOATS,), **f))
        self._fill(_lib.TrainStruct())
        for name, x in self.ws.items():
            setattr(self.t, name, x.data_ptr())

    def _batch_losses(self, B):
        return self.ws["loss"][:B].mean(dim=0)

    def positions_redone_in_f32(self, reset=False):
        """How many positions the split-precision step (9x9, train_fused 2) has handed to its f32 body since the count was last reset
        (aqg_gcn_train_fallbacks; one count per process, not per trainer).  Zero for weights of ordinary scale.  A count that grows
        by the batch size every step means the weights left the split's range -- a value beyond 65504, or 16 consecutive output
        features of a GCN layer with no weight of 2^-6 or more, as weight decay can leave them -- and every step runs both bodies:
        correct, and about twice the time.  One host read (a device synchronise)."""
        return int(self.lib.aqg_gcn_train_fallbacks(1 if reset else 0))

    def _updated(self):
        self.model.invalidate_packed()


class GeneralTrainer(_Trainer):
    """Adam state + workspace for optimisation steps of up to `max_batch` positions on a GraphPolicyValueNetwork of ANY shape with
    6 input features (the default 6/128/3 included) -- aqg_gcn_train_step_general (csrc/gcn_train_general.hip): the arithmetic
    of GNNTrainer's step on the width-generic kernels.  The surface is GNNTrainer's.  The module's own parameters are updated in
    place (and their version counters advanced), so an engine built with evaluator='general' only needs refresh_weights() to
    search with the new weights -- its evaluation cache included."""

    _STEP, _STEPS = "aqg_gcn_train_step_general", "aqg_gcn_train_steps_general"

    def __init__(self, model, max_batch=BATCH_SIZE, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=True, decay_all=False,
                 max_grad_norm=None):
        if getattr(model, "num_features", NUM_FEATURES) != NUM_FEATURES:
            raise ValueError(f"GeneralTrainer trains on board records, which have {NUM_FEATURES} feature planes; this network takes "
                             f"num_features={model.num_features}")
        self._setup(model, [p for _, p in model._ordered_params()], max_batch, betas, eps,
                    (weight_decay, decoupled, decay_all, max_grad_norm),
                    workspace=("aqg_gcn_train_general_workspace_floats", (model.hidden_dim, model.num_gcn_layers)))
        self._fill(_lib.TrainGeneralStruct())
        self.t.num_features, self.t.hidden, self.t.num_layers = NUM_FEATURES, model.hidden_dim, model.num_gcn_layers

    def _batch_losses(self, B):
        return self.ws["loss_mean"].clone()          # summed in position order by the library

    def _updated(self):
        # The kernels wrote the parameters behind torch's back: advance their version counters, which general_weights_key()
        # (and with it a 'general' engine's refresh_weights(), evaluation cache included) reads; drop any packed copy.
        torch.autograd.graph.increment_version(self.params)
        if hasattr(self.model, "invalidate_packed"):
            self.model.invalidate_packed()


CNN_TRAINING_NOT_BUILT = ("training the residual CNN through train_network() / trainer_for(), the GNN entry points, is not built "
                          "yet: use CNNTrainer / train_cnn_network(), or train_cycle, which dispatches")


class CNNTrainer(_Trainer):
    """Adam state + workspace for optimisation steps of up to `max_batch` positions on a CNNNetwork (pv_network_cnn.py) on the GPU --
    aqg_cnn_train_step (csrc/cnn_train.hip): the reference's step (train_network.py:26-107) with every BatchNorm2d in train mode.
    The surface is GeneralTrainer's.  A step always normalises with the batch statistics, whatever model.training is (the mode is
    left as it was), and updates every running_mean / running_var in place and num_batches_tracked by one, as the module's own
    train-mode forward does; parameters are updated in place.  Version counters are advanced, so packed_weights() and a 'cnn'
    engine's refresh_weights() pick up the new weights.  BatchNorm statistics over a sharded batch would need synchronised
    BatchNorm: a step under a process group of more than one rank raises ValueError."""

    _STEP, _STEPS = "aqg_cnn_train_step", "aqg_cnn_train_steps"
    _GPU_REFUSAL = "CNNTrainer trains a model on the GPU: move it there first (model.to('cuda'))"

    def __init__(self, model, max_batch=BATCH_SIZE, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=True, decay_all=False,
                 max_grad_norm=None):
        from .pv_network_cnn import CNNNetwork
        if not isinstance(model, CNNNetwork):
            raise ValueError("CNNTrainer trains a pv_network_cnn.CNNNetwork")
        self.bns = [cb.bn for cb in model._convs()]
        for bn in self.bns:
            if bn.momentum is None:
                raise ValueError("BatchNorm2d(momentum=None) (a cumulative moving average) is not supported")
            if not bn.track_running_stats or bn.running_mean is None:
                raise ValueError("BatchNorm2d(track_running_stats=False) is not supported")
        self._setup(model, model.parameters(), max_batch, betas, eps, (weight_decay, decoupled, decay_all, max_grad_norm),
                    buffers=[b for bn in self.bns for b in (bn.running_mean, bn.running_var)],
                    workspace=("aqg_cnn_train_workspace_floats", (model.num_filters, model.num_residual_blocks)))
        # the Adam launch's tensor table, on the device: params | grads | adam_m | adam_v
        self.table = torch.tensor([x.data_ptr() for x in self.params + self.grads + self.adam_m + self.adam_v], dtype=torch.int64,
                                  device=self.dev)
        t = _lib.CnnTrainStruct()
        self._fill(t)
        t.num_filters, t.num_blocks, t.adam_table = model.num_filters, model.num_residual_blocks, self.table.data_ptr()
        for i, bn in enumerate(self.bns):
            t.bn_eps[i], t.bn_momentum[i] = float(bn.eps), float(bn.momentum)
            t.running_mean[i], t.running_var[i] = bn.running_mean.data_ptr(), bn.running_var.data_ptr()

    def step(self, states72, pi_target, z_target, lr=LEARNING_RATE, update=True, group=None, mirror=None):
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            raise ValueError("CNNTrainer.step: data-parallel CNN training would need synchronised BatchNorm, which is not built; "
                             "train on one rank")
        out = super().step(states72, pi_target, z_target, lr=lr, update=update, group=group, mirror=mirror)
        if int(states72.shape[0]) > 0:
            self._forwarded(1)
        return out

    def run_epoch(self, states72, pi_target, z_target, order, lr=LEARNING_RATE, batch=None, pre_shuffle=True, mirror=None):
        sums = super().run_epoch(states72, pi_target, z_target, order, lr=lr, batch=batch, pre_shuffle=pre_shuffle, mirror=mirror)
        batch = self.max_batch if batch is None else int(batch)
        self._forwarded((int(order.shape[0]) + batch - 1) // batch)
        return sums

    def _batch_losses(self, B):
        return self.ws["loss_mean"].clone()          # summed in position order by the library

    def _updated(self):
        # the kernels wrote the parameters behind torch's back: advance their version counters (CNNNetwork.weights_key())
        torch.autograd.graph.increment_version(self.params)
        self.model.invalidate_packed()

    def _forwarded(self, steps):
        # every train-mode forward updated the running statistics in place and counts in num_batches_tracked
        torch.autograd.graph.increment_version(self.buffers)
        for bn in self.bns:
            bn.num_batches_tracked.add_(steps)
        self.model.invalidate_packed()


class WeightAverage:
    """An exponential moving average of a trainer's parameters, updated inside its HIP steps (include/aqgnn.h "weight averaging",
    csrc/weight_average.hip): e <- f32(d e) + f32(w p) with d = float32(decay), w = float32(1 - d), behind the Adam update of every
    step whose 1-based number is a multiple of `every` -- weight_average_reference in numpy, torch.optim.swa_utils.AveragedModel
    (get_ema_avg_fn, use_buffers=True) in torch.  The average starts as a copy of the parameters: no bias correction, no warm-up.

    WeightAverage(trainer) allocates the shadow tensors, builds the launch's tensor table once and attaches itself as
    trainer.average; from then on step(update=True) and run_epoch call the library's _avg entry points.  For a CNNTrainer every
    running_mean / running_var is shadowed too, with the same d.  decay and every are plain attributes read at every call.
    Nothing the trainer computes changes: parameters, moments and losses are those of a trainer without an average."""

    def __init__(self, trainer, decay=0.999, every=1):
        if getattr(trainer, "average", None) is not None:
            raise ValueError("this trainer already keeps a weight average (trainer.average)")
        self._build(trainer.model, list(trainer.params) + list(trainer.buffers), decay, every)
        self.trainer = trainer
        trainer.average = self

    @classmethod
    def for_module(cls, module, decay=0.999, every=1):
        """The average of any module's float32 parameters, updated by update() alone (every call is an update; `every` is kept for
        the caller's own schedule).  A module on the GPU is averaged by the HIP launch, a CPU module by weight_average_reference."""
        self = cls.__new__(cls)
        sources = [p.detach() for p in module.parameters() if p.dtype == torch.float32]
        if not sources:
            raise ValueError("WeightAverage.for_module: the module has no float32 parameter")
        self._build(module, sources, decay, every)
        self.trainer = None
        return self

    def _build(self, model, sources, decay, every):
        self.decay, self.every = decay, every
        _checked_average_controls(decay, every)
        if not 1 <= len(sources) <= _lib.WEIGHT_AVERAGE_MAX_TENSORS:
            raise ValueError(f"a weight average takes 1..{_lib.WEIGHT_AVERAGE_MAX_TENSORS} tensors (got {len(sources)})")
        for x in sources:
            if x.dtype != torch.float32 or not x.is_contiguous() or x.numel() < 1:
                raise ValueError("a weight average takes non-empty contiguous float32 tensors")
        if any(x.device != sources[0].device for x in sources):
            raise ValueError("every tensor of a weight average must be on one device")
        names = {t.data_ptr(): k for k, t in model.state_dict().items() if t.numel()}
        self.keys = [names.get(x.data_ptr()) for x in sources]
        if any(k is None for k in self.keys) or len(set(self.keys)) != len(self.keys):
            raise ValueError("every averaged tensor must be an entry of the model's state_dict, each once")
        self.model, self.sources, self.dev, self.updates = model, sources, sources[0].device, 0
        self.shadows = [x.detach().clone() for x in sources]
        self.host = self.dev.type != "cuda"                    # the numpy statement as the backend of a CPU module
        if self.host:
            return
        self.lib = _lib.load()
        _lib.require_gpu(self.dev)
        self._host_table, self.table, self.total_chunks = weight_average_table(self.shadows, sources)

    def _struct(self):
        """aqg_weight_average of the next call, with decay and every as they are now."""
        d, k = _checked_average_controls(self.decay, self.every)
        a = _lib.WeightAverageStruct()
        a.table, a.host_table = self.table.data_ptr(), ctypes.cast(self._host_table, ctypes.POINTER(ctypes.c_int64))
        a.num_tensors, a.every, a.total_chunks, a.decay = len(self.shadows), k, self.total_chunks, d
        return a

    def _stepped(self, first_step, steps, every):
        """Count the averaging launches of a library call over the steps first_step .. first_step + steps - 1."""
        self.updates += (first_step + steps - 1) // every - (first_step - 1) // every

    def update(self):
        """The stand-alone update, now: one launch over all tensors (aqg_weight_average_update), or numpy for a CPU module."""
        if self.host:
            d, _ = _checked_average_controls(self.decay, self.every)
            for e, p in zip(self.shadows, self.sources):
                e.copy_(torch.from_numpy(weight_average_reference(e.numpy(), p.detach().numpy(), d)))
        else:
            a = self._struct()
            _lib.check(self.lib.aqg_weight_average_update(ctypes.byref(a), _lib.stream_ptr(self.dev)), "aqg_weight_average_update")
        self.updates += 1

    def tensors(self):
        """The shadow tensors, in the order of the trainer's parameters (then its running statistics)."""
        return list(self.shadows)

    def state_dict(self):
        """The model's state_dict with every shadowed entry replaced by a copy of its average -- same keys, same order; what is not
        averaged (a BatchNorm's num_batches_tracked) is copied from the model as it is now."""
        from collections import OrderedDict
        shadow = dict(zip(self.keys, self.shadows))
        return OrderedDict((k, (shadow[k] if k in shadow else v).detach().clone()) for k, v in self.model.state_dict().items())

    def copy_to(self, model):
        """Write the average into `model`, a module of the averaged model's shape (the averaged model itself included); entries that
        are not averaged are left alone.  Version counters advance and any packed copy of the weights is dropped, as after a step."""
        target = model.state_dict()
        for k, e in zip(self.keys, self.shadows):
            if k not in target or tuple(target[k].shape) != tuple(e.shape) or target[k].dtype != e.dtype:
                raise ValueError(f"copy_to: the module has no float32 entry {k!r} of shape {tuple(e.shape)}")
        with torch.no_grad():
            for k, e in zip(self.keys, self.shadows):
                target[k].copy_(e)                               # (an in-place torch op: the version counter advances)
        if hasattr(model, "invalidate_packed"):
            model.invalidate_packed()

    def distance(self):
        """|avg - raw| / |raw| over all averaged tensors, as a float: one host read."""
        with torch.no_grad():
            diff = torch.stack([(e - p).double().pow(2).sum() for e, p in zip(self.shadows, self.sources)]).sum()
            raw = torch.stack([p.double().pow(2).sum() for p in self.sources]).sum()
            return float((diff / raw).sqrt())

    def summary_line(self):
        d, k = _checked_average_controls(self.decay, self.every)
        return f"weight average: decay {d:g}, every {k}, {self.updates} updates, |avg - raw| / |raw| = {self.distance():.3e}"


def _configured_controls():
    """The trainers' optimiser keyword arguments from TRAIN_WEIGHT_DECAY, TRAIN_DECOUPLED and TRAIN_MAX_GRAD_NORM."""
    return dict(weight_decay=TRAIN_WEIGHT_DECAY, decoupled=TRAIN_DECOUPLED, max_grad_norm=TRAIN_MAX_GRAD_NORM)


def _progress_line(epoch, policy_loss, value_loss, trainer, val=None):
    """The per-epoch progress line (train_network.py:100); with clipping on, the epoch's mean gradient norm beside it (one host read of
    grad_norms per epoch); val (a validation.Metrics of this epoch): the held-out numbers behind it."""
    line = f"\rEpoch {epoch + 1}/{NUM_EPOCH} | Policy Loss: {float(policy_loss):.4f} | Value Loss: {float(value_loss):.4f}"
    if trainer.max_grad_norm and trainer.grad_norms.numel():
        line += f" | Grad Norm: {float(trainer.grad_norms.mean()):.4f}"
    if val is not None:
        line += f" | Val Loss: {val.policy_loss:.4f} / {val.value_mse:.4f} | Val KL: {val.kl:.4f} | Top-1: {val.top1:.3f}"
    return line


class _Holdout:
    """The held-out side of one update (_update_rows' held dict): validates the network that would be saved now, keeps the curve and,
    with TRAIN_HOLDOUT_KEEP_BEST, the snapshot of the best validated epoch.  With a weight average the network validated is a twin
    module, built once through `load` and filled by average.copy_to(twin) at every validation; otherwise the model itself.  Every rank
    holds one and decides alike: no collective."""

    def __init__(self, held, model, average, load, dev):
        from .replay_reference import check_holdout_options
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
        score = self.last.policy_loss + self.last.value_mse             # the loss the update minimises
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
            lines.append(f"kept epoch {self.best_epoch}/{NUM_EPOCH}: held-out policy loss + value MSE = {self.best_score:.4f}")
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


def trainer_for(model, max_batch=BATCH_SIZE):
    """GNNTrainer for the default 6/128/3 network (the fused step), GeneralTrainer for every other shape, with the configured
    optimiser controls (TRAIN_WEIGHT_DECAY, TRAIN_DECOUPLED, TRAIN_MAX_GRAD_NORM)."""
    from .pv_network_cnn import CNNNetwork
    if isinstance(model, CNNNetwork):
        raise NotImplementedError(CNN_TRAINING_NOT_BUILT)
    kind = GNNTrainer if getattr(model, "fused", False) else GeneralTrainer
    return kind(model, max_batch=max_batch, **_configured_controls())


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
    _train(load_cnn, lambda model, max_batch: CNNTrainer(model, max_batch=max_batch, **_configured_controls()), data_parallel=False)


def _train(load, make_trainer, data_parallel):
    """The epochs of _train_loop on this process alone, on every rank of the process group (data_parallel), or else on rank 0 ALONE
    while the other ranks wait."""
    import torch.distributed as dist
    rank, world = (dist.get_rank(), dist.get_world_size()) if dist.is_available() and dist.is_initialized() else (0, 1)
    if world == 1 or data_parallel:
        return _train_loop(load, make_trainer, rank, world)
    from . import distributed as aqd
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
    from . import distributed as aqd
    dev = aqd.device()                                                             # this rank's GPU, explicitly
    model = load(PV_NETWORK_PATH + 'best.pth', dev)                                # GNNNetwork, or the shape best.pth holds
    s, p, v, index, held = _update_rows(dev, model.board_size, model=model)
    n = s.shape[0] if index is None else index.shape[0]
    trainer = make_trainer(model, max_batch=BATCH_SIZE)
    # every rank keeps its own average of its own (identical) parameters: no collective
    average = None if TRAIN_EMA_DECAY is None else WeightAverage(trainer, decay=TRAIN_EMA_DECAY, every=TRAIN_EMA_EVERY)
    holdout = None if held is None else _Holdout(held, model, average, load, dev)      # every rank validates and decides alike
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
