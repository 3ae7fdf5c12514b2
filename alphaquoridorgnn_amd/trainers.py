"""The three trainers: Adam state, workspace and the library calls of one optimisation step or one epoch of steps, for the fused
default GNN (GNNTrainer), a GraphPolicyValueNetwork of any shape (GeneralTrainer) and the reference's residual CNN (CNNTrainer).
One step = one C call (`aqg_gcn_train_step`, csrc/gcn_train.hip): forward, the reference's losses (CrossEntropyLoss on the
already-softmaxed policy + MSELoss, train_network.py:54-55,85-86), backward, Adam (:56,:90-92), all fp32.  Nothing here reads a
setting of train_network: what a trainer does is in its arguments."""
import ctypes

import torch

from . import _lib
from .distributed import rank_world
from .pv_network_gnn import STATE_DICT_KEYS, HIDDEN_DIM, NUM_FEATURES
from .train_augment import _augment_launch
from .train_reference import LEARNING_RATE, check_loss_controls

BATCH_SIZE = 128   # train_network.py:15


def default_decay_mask(params, decay_all=False):
    """Which tensors weight decay applies to: those of two or more dimensions (GCN and linear weights, conv kernels) -- not biases,
    not BatchNorm weight and bias -- unless decay_all."""
    return [bool(decay_all) or p.dim() >= 2 for p in params]


def _contiguous_f32(t):
    """Whether the kernels can take `t` as it lies: float32, contiguous."""
    return t.dtype == torch.float32 and t.is_contiguous()


def grad_norm(t):
    """The L2 norm of a contiguous float32 device tensor (or view), as a 0-dim device tensor: the deterministic two-stage reduction
    of gradient clipping (aqg_grad_norm, csrc/grad_norm.hip), no host read."""
    if not _contiguous_f32(t) or t.numel() < 1:
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


class _Trainer:
    """What the three trainers share: the constructor's arguments, the Adam state and the flat gradient buffer, the optimiser
    controls, step() (single process or data parallel), outputs() and run_epoch().  A subclass names its library calls (_STEP,
    _STEPS) and builds itself on a model (_build); it may say what an update must tell the model (_updated) and, where a forward
    pass leaves more than outputs, what that must (_forwarded).

    Optimiser controls (all off by default: the plain entry points, the same launches as ever): weight_decay (torch's coefficient) on
    the tensors default_decay_mask picks (every tensor with decay_all), decoupled as torch.optim.AdamW (True) or coupled as
    torch.optim.Adam(weight_decay=) (False), and max_grad_norm = torch.nn.utils.clip_grad_norm_'s max_norm (None or 0 = off).  They
    are plain attributes read at every call, so a schedule may change them between steps.  With clipping on, last_grad_norm is the
    unclipped global gradient norm of the last step (0-dim device tensor) and grad_norms that of every step of the last run_epoch
    (device tensor [steps]); neither is read by the host.

    Loss form (include/aqgnn.h "loss form"; off by default: the calls above, by the names they have always had): policy_loss =
    'reference' (CrossEntropyLoss on the already-softmaxed policy, train_network.py:54,85) or 'cross_entropy' (the cross-entropy
    between the target and softmax(logits), taken from the logits inside the HIP steps), and value_loss_weight = w >= 0, which scales
    the value term's gradient (the loss minimised is Lp + w Lv; the value loss REPORTED stays the unweighted mean squared error).
    Plain attributes read at every call, as the controls are."""

    _GPU_REFUSAL = None       # a subclass's own words for a model that is not on the GPU (raised in front of require_gpu's)

    def __init__(self, model, max_batch=BATCH_SIZE, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=True, decay_all=False,
                 max_grad_norm=None, policy_loss="reference", value_loss_weight=1.0):
        self.max_batch, self.betas, self.eps = max_batch, betas, eps
        self.policy_loss, self.value_loss_weight = policy_loss, value_loss_weight
        check_loss_controls(policy_loss, value_loss_weight)
        self.weight_decay, self.decoupled, self.decay_all, self.max_grad_norm = weight_decay, decoupled, decay_all, max_grad_norm
        self._build(model)

    def _setup(self, model, params, buffers=(), workspace=None):
        """The part of _build all three share: the checks of `params` (and `buffers`, tensors the kernels write besides them), the
        Adam state with every gradient a view of ONE flat buffer (the data-parallel exchange is a single all-reduce) and the
        counters.  workspace, for the two workspace trainers: (the library's workspace-size call, its shape arguments in front of
        the batch); their outputs and workspace are allocated here."""
        self.model, self.lib, self.params, self.buffers = model, _lib.load(), list(params), list(buffers)
        what = "parameters and running statistics" if self.buffers else "parameters"
        for x in self.params + self.buffers:
            if not _contiguous_f32(x):
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
        self.last_grad_norm = torch.zeros((), dtype=torch.float32, device=self.dev)
        self.grad_norms = torch.zeros((0,), dtype=torch.float32, device=self.dev)
        self._optim_ws = None
        self.average = None                       # a WeightAverage attaches itself here: the calls then take their _avg forms
        self.N, self.A = model.board_size, model.policy_output_size
        self.max_batch, self.step_count = int(self.max_batch), 0
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

    def _loss(self):
        """aqg_loss of the trainer's loss form -- None with the default form (the reference's loss, weight 1)."""
        form, w = check_loss_controls(self.policy_loss, self.value_loss_weight)
        if form == 0 and w == 1.0:
            return None
        s = _lib.LossStruct()
        s.policy_form, s.value_weight = form, w
        return s

    def _invoke(self, name, args, steps, plain=False, updating=True):
        """One library call of `steps` steps: `name` itself when plain or with every control off (no aqg_optim is built), its
        _optim form otherwise -- or, with a weight average attached and a call that updates, its _avg form (the controls' struct or
        NULL beside the average's).  With a loss form that is not the default, the _loss form of any of these (the controls' and the
        average's structs or NULL in front of the form's).  Returns the device tensor the call's norms went to, or None."""
        o, norms = (None, None) if plain else self._optim(steps)
        average = None if plain or not updating else self.average
        form = self._loss()
        if form is not None:
            a = None if average is None else average._struct()
            name, controls = name + "_loss", (None if o is None else ctypes.byref(o), None if a is None else ctypes.byref(a),
                                              ctypes.byref(form))
        elif average is not None:
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

    def _resident(self, states72, pi_target, z_target):
        """The three arrays as the kernels take them: on the trainer's GPU, uint8 / float32 / float32, contiguous."""
        return (states72.to(self.dev, torch.uint8).contiguous(), pi_target.to(self.dev, torch.float32).contiguous(),
                z_target.to(self.dev, torch.float32).contiguous())

    def step(self, states72, pi_target, z_target, lr=LEARNING_RATE, update=True, group=None, mirror=None):
        """One optimisation step.  states72 uint8 [B,72], pi_target float32 [B,A], z_target float32 [B] (device tensors).
        Returns (policy_loss, value_loss) as 0-dim device tensors -- no host synchronisation.
        mirror (None = off): a uint8 [B] device table, or (seed, epoch) for the seeded draw keyed by the row's index in THIS batch:
        the step trains on the batch with those rows mirrored left to right (one launch in front of it, aqg_augment_gather).

        Data parallel (torch.distributed initialised, world > 1): every rank passes ITS shard of the global batch; the
        local mean-loss gradients are weighted by B_local / B_global, summed with ONE all-reduce of the flat gradient buffer
        (RCCL over xGMI with backend nccl) and applied by every rank, so all replicas take the step a single process would
        take on the whole batch (up to fp32 summation order)."""
        B = int(states72.shape[0])
        if B > self.max_batch:
            raise ValueError("batch larger than the trainer's workspace")
        check_loss_controls(self.policy_loss, self.value_loss_weight)       # refused before anything is counted or launched
        states72, pi_target, z_target = self._resident(states72, pi_target, z_target)
        if mirror is not None:
            states72, pi_target, z_target = _augment_launch(self.N, states72, pi_target, z_target, None, mirror)
        world = rank_world(group)[1]
        if update:
            self.step_count += 1
        self.t.batch, self.t.step, self.t.lr = B, max(self.step_count, 1), float(lr)
        if world == 1:
            self._call(states72, pi_target, z_target, 1 if update else 0)
            loss = self._batch_losses(B) if B else torch.zeros((2,), device=self.dev)
        else:
            import torch.distributed as dist
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
        if B:                                                      # an empty batch ran no forward pass
            self._forwarded(1)
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
        check_loss_controls(self.policy_loss, self.value_loss_weight)
        n = int(order.shape[0])
        sums = torch.zeros((2,), dtype=torch.float32, device=self.dev)
        if n == 0:
            self._forwarded(0)
            return sums
        # The shuffle is applied ONCE per epoch (three gathers, ~1 KB per position) and the steps then index the shuffled
        # copies directly: every kernel of a step starts with cold loads, and reading order[] first would put one more
        # HBM round trip in front of each of them.  (The C entry points also take the order itself: order != NULL.)
        order = order.to(self.dev, torch.int64).contiguous()
        states72, pi_target, z_target = self._resident(states72, pi_target, z_target)
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
        self._forwarded(steps)
        return sums

    def _batch_losses(self, B):
        """The batch-mean (policy, value) losses of a single-process step, as a device tensor [2]."""
        return self.ws["loss_mean"].clone()          # summed in position order by the library

    def _updated(self):
        # The kernels wrote the parameters behind torch's back: advance their version counters, which general_weights_key() and
        # CNNNetwork.weights_key() (and with them an engine's refresh_weights(), evaluation cache included) read; drop any packed copy.
        torch.autograd.graph.increment_version(self.params)
        if hasattr(self.model, "invalidate_packed"):
            self.model.invalidate_packed()

    def _forwarded(self, steps):
        """Told after `steps` forward passes of a call (0: an epoch over no row).  Nothing to do where a forward pass writes only
        the trainer's own outputs."""


class GNNTrainer(_Trainer):
    """Adam state + workspace for optimisation steps of up to `max_batch` positions on `model` (a GNNNetwork on the GPU)."""

    _STEP, _STEPS = "aqg_gcn_train_step", "aqg_gcn_train_steps"

    def _build(self, model):
        if not getattr(model, "fused", True):
            model._require_fused("GNNTrainer (the fused training kernels)")
        sd = model.state_dict()
        self._setup(model, [sd[k] for k in STATE_DICT_KEYS])
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

    def _build(self, model):
        if getattr(model, "num_features", NUM_FEATURES) != NUM_FEATURES:
            raise ValueError(f"GeneralTrainer trains on board records, which have {NUM_FEATURES} feature planes; this network takes "
                             f"num_features={model.num_features}")
        self._setup(model, [p for _, p in model._ordered_params()],
                    workspace=("aqg_gcn_train_general_workspace_floats", (model.hidden_dim, model.num_gcn_layers)))
        self._fill(_lib.TrainGeneralStruct())
        self.t.num_features, self.t.hidden, self.t.num_layers = NUM_FEATURES, model.hidden_dim, model.num_gcn_layers


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

    def _build(self, model):
        from .pv_network_cnn import CNNNetwork
        if not isinstance(model, CNNNetwork):
            raise ValueError("CNNTrainer trains a pv_network_cnn.CNNNetwork")
        self.bns = [cb.bn for cb in model._convs()]
        for bn in self.bns:
            if bn.momentum is None:
                raise ValueError("BatchNorm2d(momentum=None) (a cumulative moving average) is not supported")
            if not bn.track_running_stats or bn.running_mean is None:
                raise ValueError("BatchNorm2d(track_running_stats=False) is not supported")
        self._setup(model, model.parameters(), buffers=[b for bn in self.bns for b in (bn.running_mean, bn.running_var)],
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
        if rank_world(group)[1] > 1:
            raise ValueError("CNNTrainer.step: data-parallel CNN training would need synchronised BatchNorm, which is not built; "
                             "train on one rank")
        return super().step(states72, pi_target, z_target, lr=lr, update=update, group=group, mirror=mirror)

    def _forwarded(self, steps):
        # every train-mode forward updated the running statistics in place and counts in num_batches_tracked
        torch.autograd.graph.increment_version(self.buffers)
        for bn in self.bns:
            bn.num_batches_tracked.add_(steps)
        self.model.invalidate_packed()
