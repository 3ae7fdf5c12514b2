"""CPU tests (no GPU) of the bounds audit: the allocation shim of tests/_guard_bands.py on host tensors, the scan that derives
which package modules the audit wraps (and writes its blind spots down), and the host entry points run inside numpy guard bands."""
import ast
import ctypes
import glob
import os
import types

import numpy as np
import pytest
import torch

from tests import _guard_bands as G
from tests import _util as U
from tests import witness_cases as W

PKG = os.path.join(U.REPO, "alphaquoridorgnn_amd")
# every dtype the package allocates through zeros / empty / full / ones (engine, trainers, replay, agents, openings)
DTYPES = (torch.float32, torch.float64, torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8, torch.bool)
SHAPES = ((7,), (3, 136), (0, 72), (5, 3, 9), (), (1000, 209))


def _module(bands):
    """A throw-away module whose `torch` is the proxy; 'the device' is whatever the test's predicate says."""
    m = types.ModuleType("throwaway")
    m.torch = bands.proxy("throwaway")
    return m


# ---------------------------------------------------------------------- the shim
@pytest.mark.parametrize("pattern", (0, 1))
def test_view_layout_and_fills(pattern):
    bands = G.GuardBands(pattern, is_device=lambda dev: True)
    t = _module(bands).torch
    for dtype in DTYPES:
        for shape in SHAPES:
            for make in (lambda: t.zeros(shape, dtype=dtype, device="cpu"), lambda: t.empty(shape, dtype=dtype, device="cpu"),
                         lambda: t.ones(*shape, dtype=dtype, device="cpu") if shape else t.ones((), dtype=dtype, device="cpu"),
                         lambda: t.full(shape, 1, dtype=dtype, device=torch.device("cpu")),
                         lambda: t.zeros_like(torch.empty(shape, dtype=dtype), device="cpu"),
                         lambda: t.empty_like(torch.empty(shape, dtype=dtype), device="cpu")):
                n0 = len(bands.buffers)
                v = make()
                assert len(bands.buffers) == n0 + 1
                r = bands.buffers[-1]
                assert tuple(v.shape) == shape and v.dtype == dtype and v.is_contiguous()
                assert v.storage_offset() * v.element_size() == r.start and (r.buf.data_ptr() + r.start) % 512 == 0
                assert v.numel() == 0 or v.data_ptr() == r.buf.data_ptr() + r.start        # (an empty tensor has no address)
                item = v.element_size()
                pad = G.pad_bytes(shape, item)
                row = int(np.prod(shape[1:])) * item if shape else item
                assert pad % 512 == 0 and pad >= 64 * 1024 and pad >= 2 * row
                assert r.start >= pad and r.buf.numel() - (r.start + r.nbytes) >= pad
    assert bands.intact() == []
    # what the calls promise: zeros are zeros, ones are ones, full is full; empty holds the pattern
    z, o, f = t.zeros((5, 3), dtype=torch.float32, device="cpu"), t.ones((4,), dtype=torch.int32, device="cpu"), t.full((3,), 2.5, device="cpu")
    assert not z.any() and bool((o == 1).all()) and bool((f == 2.5).all()) and f.dtype == torch.float32
    assert t.full((3,), 7, device="cpu").dtype == torch.int64 and t.full((3,), True, device="cpu").dtype == torch.bool
    e = t.empty((9,), dtype=torch.float32, device="cpu")
    assert bool(torch.isnan(e).all()) if pattern == 0 else bool((e == 1e30).all())
    e = t.empty((9,), dtype=torch.int16, device="cpu")
    assert bool((e == pattern).all())
    # the pads hold the tensor's own type
    r = bands.buffers[-1]
    front = r.buf[r.start - 64:r.start].view(torch.int16)
    assert bool((front == pattern).all())
    # writes through the view never show
    for r in bands.buffers:
        if r.dtype != torch.bool:
            r.view.zero_()
            r.view.fill_(3)
    assert bands.intact() == []


@pytest.mark.parametrize("pattern", (0, 1))
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_one_byte_write_is_reported_with_its_side(pattern, dtype):
    shape = (3, 37)            # 111 elements: slack behind the view for every dtype
    for where in ("before", "slack", "last"):
        bands = G.GuardBands(pattern, is_device=lambda dev: True)
        t = _module(bands).torch
        other = t.zeros((4,), dtype=torch.float32, device="cpu")
        v = t.zeros(shape, dtype=dtype, device="cpu")
        placed = bands.place(torch.arange(6, dtype=torch.float32).view(2, 3), module="mine")
        assert bands.intact() == [] and placed.tolist() == [[0, 1, 2], [3, 4, 5]] and other.numel() == 4
        r = bands.buffers[1]
        assert r.nbytes % 512 != 0
        pad = G.pad_bytes(shape, v.element_size())
        at = {"before": r.start - 1, "slack": r.start + r.nbytes, "last": r.start + G._up(r.nbytes) + pad - 1}[where]
        r.buf[at] ^= 0x40
        assert bands.intact() == [("throwaway", shape, dtype, "front" if where == "before" else "rear")]
        r.buf[at] ^= 0x40
        assert bands.intact() == []
    # the byte one past the rear pad is not the shim's (alignment reserve): the layout above is all it owns
    assert r.start + G._up(r.nbytes) + pad <= r.buf.numel()


def test_everything_else_passes_through():
    bands = G.GuardBands(0, is_device=lambda dev: dev.type == "cuda")       # the real predicate: nothing here is on a GPU
    t = _module(bands).torch
    assert t.float32 is torch.float32 and t.Tensor is torch.Tensor and t.nn is torch.nn and t.from_numpy is torch.from_numpy
    a = t.zeros((3, 4), dtype=torch.int32, device="cpu")
    b = t.zeros(3, 4)
    c = t.empty_like(a)
    assert a.shape == b.shape == c.shape == (3, 4) and a.dtype == torch.int32 and b.dtype == torch.float32
    assert t.full((2,), 3.0).tolist() == [3.0, 3.0] and t.ones(2, dtype=torch.uint8).tolist() == [1, 1]
    assert bands.buffers == []
    # unusual keywords pass through even for the device
    bands = G.GuardBands(1, is_device=lambda dev: True)
    t = _module(bands).torch
    out = torch.empty((4,))
    assert t.zeros((4,), out=out, device="cpu") is out
    t.empty((4,), device="cpu", pin_memory=False)
    t.empty((2, 3, 4, 5), device="cpu", memory_format=torch.contiguous_format)
    t.empty_like(torch.empty((2, 3, 4, 5)), device="cpu", memory_format=torch.preserve_format)
    t.zeros((3,), device="cpu", layout=torch.strided)
    t.zeros((3,), device="cpu", requires_grad=True)
    t.zeros((3,))                                        # no device named: the default device is not the audit's business
    t.empty_like(torch.empty((4, 6)).t(), device="cpu")  # a strided source keeps its strides with torch
    assert bands.buffers == []
    assert t.zeros((3,), device="cpu", requires_grad=False).shape == (3,) and len(bands.buffers) == 1
    with pytest.raises(ValueError):
        G.GuardBands(2)


# ---------------------------------------------------------------------- which modules the audit wraps, and what it cannot see
ALLOC = {"zeros", "empty", "full", "ones", "zeros_like", "empty_like"}
MAKES = ALLOC | {"from_numpy", "tensor", "as_tensor", "arange"}
# functions that `import torch` locally and make tensors: their `torch` is not the module's, a proxy cannot stand in for it
BLIND_SPOTS = {
    "selfplay_options.check_start_table",      # from_numpy(...).to(device) of the start table and its index
    "train_cycle._evaluate_once",              # a one-element flag for the collective: no kernel of the package reads it
}


def scan_package():
    """(modules with a module-level `import torch` that allocate through it, modules that allocate through the global name
    without having it, {module.function: calls} for functions with a local `import torch` that make tensors)."""
    wrappable, unwrappable, local = [], [], {}
    for path in sorted(glob.glob(os.path.join(PKG, "*.py"))):
        name = os.path.basename(path)[:-3]
        tree = ast.parse(open(path).read())
        has_torch = any(isinstance(n, ast.Import) and any(a.name == "torch" and a.asname is None for a in n.names) for n in tree.body)

        def torch_calls(node, names):
            return sorted({c.func.attr for c in ast.walk(node) if isinstance(c, ast.Call) and isinstance(c.func, ast.Attribute)
                           and isinstance(c.func.value, ast.Name) and c.func.value.id == "torch" and c.func.attr in names})

        locals_here = set()
        for fn in ast.walk(tree):
            if isinstance(fn, (ast.FunctionDef, ast.AsyncFunctionDef)):
                if any(isinstance(n, ast.Import) and any(a.name == "torch" for a in n.names) for n in ast.walk(fn)):
                    locals_here.add(fn)
                    calls = torch_calls(fn, MAKES)
                    if calls:
                        local[f"{name}.{fn.name}"] = calls
        shadowed = {id(c) for fn in locals_here for c in ast.walk(fn)}
        through_global = any(isinstance(c, ast.Call) and id(c) not in shadowed and isinstance(c.func, ast.Attribute)
                             and isinstance(c.func.value, ast.Name) and c.func.value.id == "torch" and c.func.attr in ALLOC
                             for c in ast.walk(tree))
        if through_global:
            (wrappable if has_torch else unwrappable).append(name)
    return wrappable, unwrappable, local


def test_module_scan():
    wrappable, unwrappable, local = scan_package()
    print("wrapped by the audit:", wrappable)
    print("local `import torch` that makes tensors:", local)
    assert unwrappable == []
    for m in ("engine", "pv_network_gnn", "pv_network_cnn", "game_logic", "agents", "train_network", "validation", "replay",
              "replay_merge", "replay_surprise", "openings", "pv_mcts", "trainers", "train_augment"):
        assert m in wrappable, m
    assert set(local) == BLIND_SPOTS, local
    # none of the blind spots allocates with the intercepted functions: they copy host arrays over
    assert all(not (set(calls) & ALLOC) for calls in local.values())


# ---------------------------------------------------------------------- host entries under numpy guard bands
def _host_records():
    recs = [(9, W.most_crowded())] + [(N, W.plugged_corridor(N)) for N in (5, 9)]
    for N in (3, 5, 7, 9):
        recs += [(N, r) for r in W.random_walk_states(N, 6, 10 + N)]
    return recs


def _under_both(run):
    outs = []
    for pattern in (0, 1):
        b = G.NumpyBands(pattern)
        outs.append(run(b))
        assert b.intact() == [], b.intact()
    assert len(outs[0]) == len(outs[1])
    for x, y in zip(outs[0], outs[1]):
        assert x.tobytes() == y.tobytes()
    return outs[0]


def test_numpy_bands_report_a_planted_write():
    for pattern in (0, 1):
        b = G.NumpyBands(pattern)
        v = b.guard(np.zeros(136, dtype=np.uint8), "out136")
        f = b.guard(np.zeros((3, 5), dtype=np.float32), "f", at_end=True)
        assert b.intact() == [] and v.shape == (136,) and f.shape == (3, 5)
        name, buf, pad, nbytes, _ = b.records[0]
        assert nbytes == 136 and pad >= 64 * 1024
        buf[pad + 136] ^= 1
        assert b.intact() == [("out136", "rear")]
        buf[pad + 136] ^= 1
        buf[pad - 1] ^= 1
        assert b.intact() == [("out136", "front")]
        buf[pad - 1] ^= 1
        _, buf, pad, nbytes, _ = b.records[1]
        buf[pad + nbytes] ^= 1                   # the first byte behind a view placed at the end
        assert b.intact() == [("f", "rear")]


def test_host_rules_stay_inside_their_buffers():
    from alphaquoridorgnn_amd import _lib
    from alphaquoridorgnn_amd.constants import board_params
    lib = _lib.load()

    def run(b):
        outs = []
        for N, rec in _host_records():
            r = b.guard(np.ascontiguousarray(rec, dtype=np.uint8), "rec72", at_end=True)       # exactly 72 bytes, the pad right behind
            out136 = b.guard(np.zeros(136, dtype=np.uint8), "out136", at_end=True)
            n = lib.aqg_host_legal_actions(N, U._p(r), U._p(out136))
            assert 0 <= n <= 136
            outs.append(np.array([n], dtype=np.int32))
            outs.append(out136[:n].copy())
            walls, draw = board_params(N)
            outs.append(np.array([lib.aqg_host_check_state(N, U._p(r), walls, draw)], dtype=np.int32))
            for a in out136[:n][[0, n // 2, n - 1]] if n else []:
                out72 = b.guard(np.zeros(72, dtype=np.uint8), "out72", at_end=True)
                assert lib.aqg_host_next(N, U._p(r), int(a), U._p(out72)) == 0
                outs.append(out72.copy())
            assert r.tobytes() == np.ascontiguousarray(rec, dtype=np.uint8).tobytes()
        return outs

    outs = _under_both(run)
    # and they are the answers of the unguarded calls
    k = 0
    for N, rec in _host_records():
        rec = np.ascontiguousarray(rec, dtype=np.uint8)
        out = np.zeros(136, dtype=np.uint8)
        n = lib.aqg_host_legal_actions(N, U._p(rec), U._p(out))
        assert int(outs[k][0]) == n and np.array_equal(outs[k + 1], out[:n])
        k += 3 + (3 if n else 0)
    assert k == len(outs)


def test_host_weight_packing_stays_inside_its_buffer():
    from alphaquoridorgnn_amd import _lib
    from oracle import gnn as og
    lib = _lib.load()
    p = og.init_params(5)
    n = lib.aqg_gcn_packed_floats(9)

    def run(b):
        host = [b.guard(np.ascontiguousarray(p[k], dtype=np.float32), k, at_end=True) for k in og.KEYS]
        arr = (ctypes.c_void_p * 14)(*[h.ctypes.data_as(ctypes.c_void_p) for h in host])
        out = b.guard(np.zeros(n, dtype=np.float32), "packed", at_end=True)
        assert lib.aqg_gcn_pack_weights_host(9, arr, U._p(out)) == 0
        return [out.copy()]

    out = _under_both(run)[0]
    assert np.isfinite(out).all()
    plain = np.zeros(n, dtype=np.float32)
    host = [np.ascontiguousarray(p[k], dtype=np.float32) for k in og.KEYS]
    arr = (ctypes.c_void_p * 14)(*[h.ctypes.data_as(ctypes.c_void_p) for h in host])
    assert lib.aqg_gcn_pack_weights_host(9, arr, U._p(plain)) == 0
    assert plain.tobytes() == out.tobytes()
