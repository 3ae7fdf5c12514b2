"""Replay window -- the last K self-play generations as training rows in a ring that stays on the GPU (the reference trains on the
newest .history file alone).

The ring is three arrays of `capacity` rows -- states72 uint8 [capacity,72], pi float32 [capacity,A], z float32 [capacity] -- in the
layout the trainers read.  A generation is appended in one launch (aqg_replay_append, csrc/replay.hip) either as the engine leaves it
(visit counts and int8 outcomes: `append_counts`, converted on the way to the bits the .history route produces) or as finished rows
(`append_rows`, `append_history`, `extend_from_files`).  Which slots hold rows, and of which generation, is bookkeeping on the host:
nothing here reads anything back from the device.

`append_reference` is the kernel's statement in numpy on host arrays; a window on the CPU (device None or 'cpu') runs the same
bookkeeping over it.

Blended value target (`append_counts(..., search_value=q, value_blend=L)`, aqg_replay_append_blend): z' = (1 - L) z + L q with q the
search value the engine recorded beside the row (engine.history_values).  `blend_targets` is the arithmetic in numpy.
"""
import pickle

import numpy as np
import torch

from . import _lib
from .constants import BOARD_SIZE


def policy_size(board_size):
    return board_size ** 2 + 2 * (board_size - 1) ** 2


def check_value_blend(blend):
    """Validate a value blend as the library does, on the f32 value the kernel is given: in [0, 1], not NaN.  Returns it as a float."""
    blend = float(np.float32(blend))
    if not 0.0 <= blend <= 1.0:
        raise ValueError(f"value_blend must be in [0, 1] as a float32, not {blend}")
    return blend


def blend_targets(z_i8, search_value, blend):
    """The blended value target of aqg_replay_append_blend in numpy, float32 [n]: keep * float32(z) + blend * v with keep =
    float32(1) - blend -- one f32 subtraction, two f32 products and one f32 sum, each rounded (no fused multiply-add).  z_i8 the
    outcomes (any integer or float array of -1 / 0 / 1), search_value float32 [n]."""
    b = np.float32(check_value_blend(blend))
    keep = np.float32(1.0) - b
    z = np.asarray(z_i8).astype(np.float32)
    v = np.asarray(search_value)
    if v.dtype != np.float32 or v.shape != z.shape:
        raise ValueError("blend_targets: search_value must be float32 with one value per outcome")
    x = (keep * z).astype(np.float32)
    y = (b * v).astype(np.float32)
    return (x + y).astype(np.float32)


def append_reference(board_size, states72, visits, z_i8, pi, z_f32, head, ring72, ring_pi, ring_z, search_value=None, value_blend=0.0):
    """aqg_replay_append in numpy, on host arrays, in place (include/aqgnn.h, "replay window"): source row i goes to ring slot
    (head + i) % capacity, n and capacity being the row counts of states72 and ring72.  Counts form (visits [n,A] int16 or uint16,
    read as UNSIGNED, and z_i8 [n] int8; pi and z_f32 None): ring_pi = float32(float64(v) / float64(tot)) with tot the row's integer
    sum, zeros where tot == 0, ring_z = float32(z).  Rows form (pi [n,A] float32, z_f32 [n] float32; the other two None): a copy.
    The 72 record bytes are copied verbatim.  search_value (float32 [n]; counts form only) makes it aqg_replay_append_blend:
    ring_z = blend_targets(z_i8, search_value, value_blend).  Refuses what the C entry points refuse, with ValueError."""
    A = policy_size(board_size)
    if search_value is None and value_blend != 0.0:
        raise ValueError("append_reference: a value_blend needs search_value")
    if search_value is not None:
        check_value_blend(value_blend)
    if board_size not in (3, 5, 7, 9):
        raise ValueError("append_reference: unsupported board_size (odd 3..9)")
    n, capacity = int(states72.shape[0]), int(ring72.shape[0])
    counts = visits is not None and z_i8 is not None and pi is None and z_f32 is None
    finished = pi is not None and z_f32 is not None and visits is None and z_i8 is None
    if not counts and not finished:
        raise ValueError("append_reference: give the counts form (visits, z_i8) or the rows form (pi, z_f32), whole, and not both")
    if search_value is not None and not counts:
        raise ValueError("append_reference: search_value goes with the counts form (visits, z_i8)")
    if capacity < 1 or not 0 <= head < capacity or n > capacity:
        raise ValueError("append_reference: needs capacity >= 1, 0 <= head < capacity and n <= capacity")
    for x, name, dtypes, shape in ((states72, "states72", (np.uint8,), (n, 72)), (ring72, "ring72", (np.uint8,), (capacity, 72)),
                                   (ring_pi, "ring_pi", (np.float32,), (capacity, A)), (ring_z, "ring_z", (np.float32,), (capacity,)),
                                   (visits, "visits", (np.int16, np.uint16), (n, A)), (z_i8, "z_i8", (np.int8,), (n,)),
                                   (pi, "pi", (np.float32,), (n, A)), (z_f32, "z_f32", (np.float32,), (n,)),
                                   (search_value, "search_value", (np.float32,), (n,))):
        if x is not None and (x.dtype not in dtypes or tuple(x.shape) != shape):
            raise ValueError(f"append_reference: {name} must be {np.dtype(dtypes[0]).name} {list(shape)} ({board_size}x{board_size} board)")
    slots = (head + np.arange(n)) % capacity
    ring72[slots] = states72
    if counts:
        v = visits.view(np.uint16).astype(np.int64)
        tot = v.sum(axis=1, keepdims=True)
        quotient = v.astype(np.float64) / np.where(tot > 0, tot, 1).astype(np.float64)
        ring_pi[slots] = quotient.astype(np.float32)                # a row without a visit: 0 / 1 = A zeros
        ring_z[slots] = z_i8.astype(np.float32) if search_value is None else blend_targets(z_i8, search_value, value_blend)
    else:
        ring_pi[slots] = pi
        ring_z[slots] = z_f32


class ReplayWindow:
    """A ring of training rows holding the newest generations, with per-generation bookkeeping on the host.

    max_generations: generations kept at most.  capacity_rows: rows of the ring; None sizes it at the first append of m rows to
    max_generations * ceil(1.5 * m) -- game lengths drift as the network trains, and when a later generation does not fit beside
    the others, more old generations are dropped: the window then holds FEWER than max_generations.  device: the GPU the ring lives
    on (appends are one aqg_replay_append launch on its current stream); None or a CPU device keeps the ring in host memory and
    appends with append_reference.

    Appending a generation of m rows: if m > capacity only its newest `capacity` rows are kept; the oldest generations are dropped
    while there are max_generations of them or while the new one does not fit; the rows are then written at the slot after the
    newest row.  The valid rows therefore always form ONE circular interval of the ring."""

    def __init__(self, board_size=BOARD_SIZE, max_generations=1, capacity_rows=None, device=None):
        if board_size not in (3, 5, 7, 9):
            raise ValueError("ReplayWindow: unsupported board_size (odd 3..9)")
        if int(max_generations) < 1:
            raise ValueError("ReplayWindow: max_generations must be >= 1")
        if capacity_rows is not None and int(capacity_rows) < 1:
            raise ValueError("ReplayWindow: capacity_rows must be >= 1")
        self.board_size = int(board_size)
        self.policy_size = policy_size(self.board_size)
        self.max_generations = int(max_generations)
        self.capacity = None if capacity_rows is None else int(capacity_rows)
        dev = torch.device("cpu") if device is None else torch.device(device)
        self.device = dev if dev.type == "cpu" else _lib.require_gpu(dev)
        self._rings = None
        self._generations = []          # row counts, oldest first
        self._start = 0                 # slot of the oldest valid row
        self._valid = 0
        self._index = torch.zeros((0,), dtype=torch.int64, device=self.device)
        if self.capacity is not None:
            self._allocate()

    def _allocate(self):
        z = dict(device=self.device)
        self._rings = (torch.zeros((self.capacity, 72), dtype=torch.uint8, **z),
                       torch.zeros((self.capacity, self.policy_size), dtype=torch.float32, **z),
                       torch.zeros((self.capacity,), dtype=torch.float32, **z))

    # ---- what it holds
    def __len__(self):
        return self._valid

    @property
    def generations(self):
        """Row counts of the generations held, oldest first."""
        return list(self._generations)

    def tensors(self):
        """The three whole rings (states72, pi, z) -- valid and stale slots alike; index() says which are valid."""
        if self._rings is None:
            raise ValueError("ReplayWindow: the ring is sized by the first append (capacity_rows=None)")
        return self._rings

    def index(self):
        """int64 tensor on the window's device: the valid slots, the oldest row first.  Rebuilt once per append."""
        return self._index

    def rows(self):
        """Gathered copies (states72, pi, z) of the valid rows in age order."""
        if self._rings is None:
            return (torch.zeros((0, 72), dtype=torch.uint8, device=self.device),
                    torch.zeros((0, self.policy_size), dtype=torch.float32, device=self.device),
                    torch.zeros((0,), dtype=torch.float32, device=self.device))
        return tuple(x.index_select(0, self._index) for x in self._rings)

    def clear(self):
        """Empty the window; the ring keeps its size."""
        self._generations, self._start, self._valid = [], 0, 0
        self._index = torch.zeros((0,), dtype=torch.int64, device=self.device)

    # ---- appending
    def _checked(self, what, states72, second, third, second_dtypes, third_dtype):
        """Shapes and dtypes against the board, before anything is written; returns contiguous tensors on the window's device."""
        names = ("states72",) + (("visits", "z") if what == "append_counts" else ("pi", "z"))
        xs = [torch.as_tensor(x) for x in (states72, second, third)]
        m = int(xs[0].shape[0]) if xs[0].dim() else -1
        for x, name, dtypes, tail in zip(xs, names, ((torch.uint8,), second_dtypes, (third_dtype,)), ((72,), (self.policy_size,), ())):
            if x.dtype not in dtypes or tuple(x.shape) != (m,) + tail:
                raise ValueError(f"ReplayWindow.{what}: {name} must be a {dtypes[0]} {['n', *tail]} tensor with one row per position "
                                 f"of a {self.board_size}x{self.board_size} board; got {x.dtype} {list(x.shape)}")
        return [x.to(self.device).contiguous() for x in xs], m

    def _make_room(self, m):
        """The eviction rule for a generation of m rows: (rows of it to skip, slot to write at).  Sizes a lazy ring."""
        if self.capacity is None:
            if m == 0:
                raise ValueError("ReplayWindow: capacity_rows=None sizes the ring by the first generation, which cannot be empty")
            self.capacity = self.max_generations * -(-3 * m // 2)          # max_generations * ceil(1.5 m)
            self._allocate()
        keep = min(m, self.capacity)
        while self._generations and (len(self._generations) >= self.max_generations or self._valid + keep > self.capacity):
            g = self._generations.pop(0)
            self._start = (self._start + g) % self.capacity
            self._valid -= g
        return m - keep, (self._start + self._valid) % self.capacity

    def _appended(self, keep):
        self._generations.append(keep)
        self._valid += keep
        self._index = (self._start + torch.arange(self._valid, dtype=torch.int64, device=self.device)) % self.capacity

    def _append(self, states72, visits, z_i8, pi, z_f32, m, search_value=None, value_blend=0.0):
        skip, head = self._make_room(m)
        if skip:
            states72, visits, z_i8, pi, z_f32, search_value = (None if x is None else x[skip:].contiguous()
                                                               for x in (states72, visits, z_i8, pi, z_f32, search_value))
        n = m - skip
        r72, rpi, rz = self._rings
        if self.device.type == "cpu":
            h = lambda x: None if x is None else x.numpy()          # noqa: E731   (views: the rings are written in place)
            append_reference(self.board_size, h(states72), h(visits), h(z_i8), h(pi), h(z_f32), head, h(r72), h(rpi), h(rz),
                             h(search_value), value_blend)
        elif search_value is not None:
            _lib.check(_lib.load().aqg_replay_append_blend(self.board_size, self.policy_size, _lib.ptr(states72), _lib.ptr(visits),
                                                           _lib.ptr(z_i8), _lib.ptr(search_value), value_blend, n, self.capacity, head,
                                                           _lib.ptr(r72), _lib.ptr(rpi), _lib.ptr(rz), _lib.stream_ptr(self.device)),
                       "aqg_replay_append_blend")
        else:
            _lib.check(_lib.load().aqg_replay_append(self.board_size, self.policy_size, _lib.ptr(states72), _lib.ptr(visits),
                                                     _lib.ptr(z_i8), _lib.ptr(pi), _lib.ptr(z_f32), n, self.capacity, head,
                                                     _lib.ptr(r72), _lib.ptr(rpi), _lib.ptr(rz), _lib.stream_ptr(self.device)),
                       "aqg_replay_append")
        self._appended(n)

    def append_counts(self, states72, visits, z, search_value=None, value_blend=0.0):
        """One generation as the engine leaves it (engine.history_tensors / gather_history): states72 uint8 [n,72], visit counts
        int16 (or uint16; read as unsigned) [n,A], z int8 [n].  pi = counts / their sum, with the bits of the .history route.
        search_value (float32 [n], engine.history_values) with value_blend L in [0, 1]: the value target becomes (1 - L) z + L q
        (blend_targets; one aqg_replay_append_blend launch).  Without search_value the call is the plain append."""
        (s, v, zz), m = self._checked("append_counts", states72, visits, z, (torch.int16, torch.uint16), torch.int8)
        if search_value is None:
            if value_blend != 0.0:
                raise ValueError("ReplayWindow.append_counts: a value_blend needs search_value")
            return self._append(s, v, zz, None, None, m)
        value_blend = check_value_blend(value_blend)
        q = torch.as_tensor(search_value)
        if q.dtype != torch.float32 or tuple(q.shape) != (m,):
            raise ValueError(f"ReplayWindow.append_counts: search_value must be a torch.float32 ['n'] tensor with one value per "
                             f"position; got {q.dtype} {list(q.shape)}")
        self._append(s, v, zz, None, None, m, q.to(self.device).contiguous(), value_blend)

    def append_rows(self, states72, pi, z):
        """One generation of finished rows: states72 uint8 [n,72], pi float32 [n,A], z float32 [n]."""
        (s, p, zz), m = self._checked("append_rows", states72, pi, z, (torch.float32,), torch.float32)
        self._append(s, None, None, p, zz, m)

    def append_history(self, history):
        """One generation in the .history schema, [[player, enemy, walls], policy, z] per row (self_play.write_data): packed by
        pack_states and converted as the trainers convert a file, then appended as finished rows."""
        from .pv_network_gnn import pack_states
        history = list(history)
        nw = (self.board_size - 1) ** 2
        for row in history:
            if len(row) != 3 or len(row[0]) != 3 or len(row[0][2]) != nw or len(row[1]) != self.policy_size:
                raise ValueError(f"ReplayWindow.append_history: a row is not [[player, enemy, walls], policy, z] of a "
                                 f"{self.board_size}x{self.board_size} board")
        s, p, v = zip(*history) if history else ((), (), ())
        self.append_rows(torch.from_numpy(pack_states(s, self.board_size)),
                         torch.tensor(np.array(p, dtype=np.float64).reshape(len(history), self.policy_size), dtype=torch.float32),
                         torch.tensor(np.array(v, dtype=np.float64).reshape(len(history)), dtype=torch.float32))

    def extend_from_files(self, paths):
        """Each .history file as one generation, in the order given: oldest first."""
        for path in paths:
            with open(path, mode='rb') as f:
                self.append_history(pickle.load(f))
