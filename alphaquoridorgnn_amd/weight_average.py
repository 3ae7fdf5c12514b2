"""Weight averaging: WeightAverage, of a trainer's parameters inside its HIP steps or of any module's on call."""
import ctypes

import torch

from . import _lib
from .train_reference import check_average_controls, weight_average_reference
from .trainers import _contiguous_f32


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
        check_average_controls(decay, every)
        if not 1 <= len(sources) <= _lib.WEIGHT_AVERAGE_MAX_TENSORS:
            raise ValueError(f"a weight average takes 1..{_lib.WEIGHT_AVERAGE_MAX_TENSORS} tensors (got {len(sources)})")
        for x in sources:
            if not _contiguous_f32(x) or x.numel() < 1:
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
        d, k = check_average_controls(self.decay, self.every)
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
            d, _ = check_average_controls(self.decay, self.every)
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
        d, k = check_average_controls(self.decay, self.every)
        return f"weight average: decay {d:g}, every {k}, {self.updates} updates, |avg - raw| / |raw| = {self.distance():.3e}"
