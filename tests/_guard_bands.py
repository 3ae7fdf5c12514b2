"""Poisoned guard bands around the package's device allocations (test infrastructure).

The kernels take raw pointers into torch tensors whose sizes Python and C agree on by convention only, and the caching
allocator hides a first-order slip: it rounds every allocation up to 512 bytes and hands out neighbours of the same pool, so a
tail store one element too long lands in slack or in another tensor and every comparison still passes.

GuardBands(pattern) serves allocations from the middle of a larger uint8 buffer it owns:

    [ front pad | view: exactly the requested bytes | slack to the next 512 bytes + rear pad ]

- each pad is a multiple of 512 bytes and the view starts on a 512-byte boundary, as the allocator would have placed it;
- each pad is at least 64 KiB and at least twice the tensor's leading-dimension stride in bytes: an off-by-one leading index or
  one misplaced workgroup tile still lands in memory the test owns;
- the pads are filled in the guarded tensor's OWN dtype (an overrunning reader reads them with that type): floating tensors
  get a quiet NaN (pattern 0) or +1e30 (pattern 1; the largest finite value where the format cannot hold 1e30), integer, uint8
  and bool tensors get 0 or 1 -- small on purpose, a stray index read from a pad must never become a wild address;
- a tensor asked for with `empty` / `empty_like` holds the pattern too: what a kernel reads before anyone wrote it then
  differs between the two patterns like an out-of-bounds read does.

proxy(name) stands in for the name `torch` inside one package module (monkeypatch.setattr(module, "torch", proxy)): it forwards
every attribute to the real torch, except zeros / empty / full / ones / zeros_like / empty_like when they are called for a
device the predicate accepts (CUDA by default) with no keyword beyond dtype, device, size, fill_value and
requires_grad=False.  Anything else -- CPU allocations, out=, pin_memory=, memory_format=, layout=, tensor methods such as
new_zeros, .to(device), torch.tensor -- falls through untouched and is not audited.

What this instrument cannot see: an out-of-bounds READ whose value is masked before it reaches a result leaves no trace here
(the pads stay intact and the results agree); a write that lands further away than the pads is not contained by them; and
memory that is not allocated through a wrapped module's `torch` name (local `import torch`, tensor methods) is not guarded.
"""
import numpy as np

PAD_MIN = 64 * 1024
ALIGN = 512
INTERCEPTED = ("zeros", "empty", "full", "ones", "zeros_like", "empty_like")
_PLAIN_KW = {"dtype", "device", "size", "fill_value", "requires_grad"}


def _up(n, a=ALIGN):
    return (int(n) + a - 1) // a * a


def pad_bytes(shape, itemsize):
    """Bytes of each pad for a contiguous tensor of `shape`: >= 64 KiB, >= twice the leading stride, a multiple of 512."""
    shape = tuple(int(s) for s in shape)
    row = int(np.prod(shape[1:], dtype=np.int64)) * itemsize if len(shape) >= 1 else itemsize
    return _up(max(PAD_MIN, 2 * row))


def pad_value(torch, dtype, pattern):
    """The element the pads of a tensor of `dtype` hold under `pattern` (0 or 1)."""
    if dtype.is_floating_point:
        if pattern == 0:
            return float("nan")
        return min(1e30, torch.finfo(dtype).max)
    if dtype.is_complex:
        raise TypeError("complex tensors are not guarded")
    return int(pattern)


class _Record:
    __slots__ = ("module", "shape", "dtype", "buf", "start", "nbytes", "view", "elem")


class GuardBands:
    def __init__(self, pattern, is_device=None):
        import torch
        if pattern not in (0, 1):
            raise ValueError("pattern is 0 or 1")
        self.torch = torch
        self.pattern = pattern
        self.is_device = is_device if is_device is not None else (lambda dev: dev.type == "cuda")
        self.buffers = []          # every _Record served, alive until the check

    # ------------------------------------------------------------------ allocation
    def _serve(self, module, shape, dtype, device):
        torch = self.torch
        shape = tuple(int(s) for s in shape)
        item = torch.empty((), dtype=dtype).element_size()
        nbytes = int(np.prod(shape, dtype=np.int64)) * item
        pad = pad_bytes(shape, item)
        total = pad + _up(nbytes) + pad
        buf = torch.empty((total + ALIGN,), dtype=torch.uint8, device=device)
        base = (-buf.data_ptr()) % ALIGN          # 0 from the caching allocator; host memory is aligned by hand
        start = base + pad
        r = _Record()
        r.module, r.shape, r.dtype, r.buf, r.start, r.nbytes = module, shape, dtype, buf, start, nbytes
        val = pad_value(torch, dtype, self.pattern)
        as_int = torch.uint8 if dtype == torch.bool else dtype
        r.elem = torch.full((1,), val, dtype=as_int).view(torch.uint8).to(device)      # the pad element's bytes
        buf[base:base + total].view(as_int).fill_(val)
        r.view = buf[start:start + nbytes].view(dtype).view(shape)
        assert r.view.data_ptr() % ALIGN == 0 and r.view.is_contiguous()
        self.buffers.append(r)
        return r.view

    def place(self, tensor, module="test"):
        """A test-made input, copied into a guarded view of its shape and dtype on its own device."""
        v = self._serve(module, tuple(tensor.shape), tensor.dtype, tensor.device)
        v.copy_(tensor)
        return v

    # ------------------------------------------------------------------ check
    def _sides(self, r):
        base = r.start - pad_bytes(r.shape, r.elem.numel())
        end = r.start + _up(r.nbytes) + pad_bytes(r.shape, r.elem.numel())
        return (("front", r.buf[base:r.start]), ("rear", r.buf[r.start + r.nbytes:end]))

    def intact(self):
        """[(module, shape, dtype, side)] of the pads that no longer hold their pattern (empty = all intact)."""
        bad = []
        for r in self.buffers:
            for side, region in self._sides(r):
                if not bool((region.view(-1, r.elem.numel()) == r.elem).all()):
                    bad.append((r.module, r.shape, r.dtype, side))
        return bad

    def rear_slack(self, view):
        """(record, byte offset into record.buf of the first byte behind `view`) -- for tests that plant a write."""
        for r in self.buffers:
            if r.view.data_ptr() == view.data_ptr() and r.shape == tuple(view.shape):
                return r, r.start + r.nbytes
        raise KeyError("not a guarded view")

    # ------------------------------------------------------------------ the stand-in for `torch`
    def proxy(self, module_name):
        return _TorchProxy(self, module_name)

    def install(self, monkeypatch, modules):
        """Put a proxy in place of the name `torch` in each of `modules` (module objects)."""
        for m in modules:
            assert hasattr(m, "torch"), f"{m.__name__} has no module-level torch"
            monkeypatch.setattr(m, "torch", self.proxy(m.__name__.rsplit(".", 1)[-1]))

    def _call(self, module, name, args, kwargs):
        torch = self.torch
        real = getattr(torch, name)
        if not set(kwargs) <= _PLAIN_KW or kwargs.get("requires_grad", False):
            return real(*args, **kwargs)
        kw = dict(kwargs)
        fill = None
        if name.endswith("_like"):
            if len(args) != 1 or not isinstance(args[0], torch.Tensor) or "size" in kw or "fill_value" in kw:
                return real(*args, **kwargs)
            src = args[0]
            if not src.is_contiguous() or src.layout != torch.strided:
                return real(*args, **kwargs)        # preserve_format would keep the strides
            shape, dtype, device = tuple(src.shape), kw.get("dtype") or src.dtype, kw.get("device", src.device)
        else:
            rest = list(args)
            if name == "full":
                if "fill_value" in kw:
                    fill = kw["fill_value"]
                elif len(rest) == 2:
                    fill = rest.pop()
                else:
                    return real(*args, **kwargs)
            if "size" in kw:
                if rest:
                    return real(*args, **kwargs)
                shape = kw["size"]
            elif len(rest) == 1 and isinstance(rest[0], (tuple, list, torch.Size)):
                shape = rest[0]
            else:
                shape = rest
            try:
                shape = tuple(int(s) for s in shape)
            except (TypeError, ValueError):
                return real(*args, **kwargs)
            if "dtype" in kw and kw["dtype"] is not None:
                dtype = kw["dtype"]
            elif name == "full" and not isinstance(fill, float):      # torch infers the dtype from the fill value
                if isinstance(fill, bool):
                    dtype = torch.bool
                elif isinstance(fill, int):
                    dtype = torch.int64
                else:
                    return real(*args, **kwargs)
            else:
                dtype = torch.get_default_dtype()
            device = kw.get("device")
        if device is None:
            return real(*args, **kwargs)
        device = torch.device(device)
        if not self.is_device(device) or dtype.is_complex or any(s < 0 for s in shape):
            return real(*args, **kwargs)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        view = self._serve(module, shape, dtype, device)
        if name in ("zeros", "zeros_like"):
            view.zero_()
        elif name == "ones":
            view.fill_(1)
        elif name == "full":
            view.fill_(fill)
        return view


class _TorchProxy:
    """Forwards every attribute to torch; the allocation functions go through the GuardBands that made it."""

    def __init__(self, bands, module_name):
        object.__setattr__(self, "_bands", bands)
        object.__setattr__(self, "_module", module_name)

    def __getattr__(self, name):
        bands = object.__getattribute__(self, "_bands")
        if name in INTERCEPTED:
            module = object.__getattribute__(self, "_module")
            return lambda *a, **k: bands._call(module, name, a, k)
        return getattr(bands.torch, name)

    def __setattr__(self, name, value):
        setattr(object.__getattribute__(self, "_bands").torch, name, value)


# ---------------------------------------------------------------------- the same bands around numpy arrays (host entries)
def np_pad_value(dtype, pattern):
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        return np.nan if pattern == 0 else min(1e30, float(np.finfo(dtype).max))
    return pattern


class NumpyBands:
    """guard(array) -> a view of the array's shape and dtype between two pads of pad_bytes() each, in the host's memory;
    at_end=True leaves no slack behind the view (the view's last byte is the byte before the rear pad)."""

    def __init__(self, pattern):
        self.pattern = pattern
        self.records = []

    def guard(self, array, name="", at_end=False):
        array = np.ascontiguousarray(array)
        item, nbytes = array.dtype.itemsize, array.nbytes
        pad = pad_bytes(array.shape, item)
        body = nbytes if at_end else _up(nbytes)
        body = (body + item - 1) // item * item
        buf = np.empty(pad + body + pad, dtype=np.uint8)
        val = np_pad_value(array.dtype, self.pattern)
        buf.view(array.dtype)[:] = val
        view = buf[pad:pad + nbytes].view(array.dtype).reshape(array.shape)
        view[...] = array
        elem = np.full(1, val, dtype=array.dtype).view(np.uint8)
        self.records.append((name, buf, pad, nbytes, elem))
        return view

    def intact(self):
        bad = []
        for name, buf, pad, nbytes, elem in self.records:
            for side, region in (("front", buf[:pad]), ("rear", buf[pad + nbytes:])):
                if not np.array_equal(region.reshape(-1, elem.size), np.broadcast_to(elem, (region.size // elem.size, elem.size))):
                    bad.append((name, side))
        return bad
