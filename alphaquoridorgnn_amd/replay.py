"""Replay window -- the last K self-play generations as training rows in a ring that stays on the GPU (the reference trains on the
newest .history file alone).  The ring is three arrays of `capacity` rows -- states72 uint8 [capacity,72], pi float32 [capacity,A], z
float32 [capacity] -- in the layout the trainers read; which slots hold rows, and of which generation, is bookkeeping on the host.

This module holds ReplayWindow.  The rest of the family, every name importable from here as before:
  replay_reference.py  every kernel stated in numpy (what a window on the CPU runs): the append and its blend (csrc/replay.hip),
                       Reanalyse's refresh in both forms and the draw of its rows (csrc/replay_refresh.hip), the position merge
                       (csrc/replay_merge.hip), policy surprise weighting (csrc/replay_surprise.hip), with their option checks;
  replay_merge.py      merge_positions, the position merge on the GPU (ReplayWindow.merged());
  replay_surprise.py   surprise_index, the rows of an update drawn by KL(target || network) on the GPU (ReplayWindow.surprise_index);
  validation.py        row_metrics and holdout_split (csrc/row_metrics.hip): a network's held-out metrics per ply bucket, and the
                       split of rows by position (ReplayWindow.row_metrics, ReplayWindow.holdout_split).
The definitions are in include/aqgnn.h.
"""
import pickle

import numpy as np
import torch

from . import _lib
from .constants import BOARD_SIZE, check_board_size, num_actions as policy_size
from .replay_merge import merge_positions
from .replay_reference import (KEY_BYTES, MERGE_CHUNK, SURPRISE_K_MAX, SURPRISE_MAX_ROWS, SURPRISE_Q_SCALE, SURPRISE_TINY,  # noqa: F401
                               append_reference, blend_targets, check_surprise_options, check_value_blend, draw_reanalyse_rows,
                               merge_depth, merge_reference, merge_runs_reference, position_keys, refresh_policy_reference,
                               refresh_reference, surprise_counts_reference, surprise_reference, surprise_weights)
from .replay_reference import (HOLDOUT_STREAM, ROW_METRICS_CHUNK, ROW_METRICS_MAX_BUCKETS, ROW_METRICS_MAX_ROWS,  # noqa: F401
                               ROW_METRICS_TINY, TAG_HIT, TAG_SIGN_AGREES, TAG_SIGN_COUNTED, check_holdout_options,
                               check_row_metrics_options, holdout_reference, holdout_split_reference, row_metrics_reduce_reference,
                               row_metrics_reference, row_metrics_workspace_doubles)
from .replay_surprise import expand_rows, surprise_index  # noqa: F401
from .validation import holdout_split, row_metrics


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
        check_board_size(board_size, "ReplayWindow")
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
        self.reanalyse_updates = 0      # reanalyse passes self_play() has run on this window: the `update` of draw_reanalyse_rows
        self.surprise_updates = 0       # surprise-weighted updates drawn on this window: the `update` of surprise_index's key
        self.fork_updates = 0           # generations self_play() has forked from this window: the `update` of openings.fork_table
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

    def merged(self):
        """The valid rows with repeated positions merged: (states72, pi, z, count) tensors on the window's device, one row per distinct
        position in the order of its oldest row, pi and z the mean over the position's rows, count (int32) how many there were
        (merge_positions; merge_reference on a host window).  Without repeats it is rows(), bit for bit, with a count of ones.  The
        ring, the bookkeeping and rows() are unchanged; stale slots are never read."""
        if self._rings is None or self._valid == 0:
            return self.rows() + (torch.zeros((0,), dtype=torch.int32, device=self.device),)
        if self.device.type == "cpu":
            return tuple(torch.from_numpy(x) for x in merge_reference(*(x.numpy() for x in self._rings), index=self._index.numpy()))
        return merge_positions(*self._rings, index=self._index, board_size=self.board_size)

    def surprise_index(self, model, *, seed, update=None, expected_rows=None, uniform_share=0.5, max_copies=8, chunk_rows=16384,
                       stats=None):
        """surprise_index on the ring: (index int64 [M], k float32 [m], count int32 [m]) over the m valid rows in age order, the index
        naming ring slots -- a row's draw is keyed by its slot, so it keeps it for as long as it stays in the ring.  update None: the
        window's own counter surprise_updates, which the call then advances.  A window on the GPU only; the ring, the bookkeeping and
        rows() are unchanged."""
        if self.device.type == "cpu":
            raise ValueError("ReplayWindow.surprise_index: the network's forward runs on the GPU; this window is in host memory")
        if update is None:
            update = self.surprise_updates
            self.surprise_updates += 1
        if self._rings is None or self._valid == 0:         # no row: empty tensors, and no index
            s72, pi, _ = self.rows()
            index = None
        else:
            s72, pi, index = self._rings[0], self._rings[1], self._index
        return surprise_index(model, s72, pi, index, seed=seed, update=update, expected_rows=expected_rows, uniform_share=uniform_share,
                              max_copies=max_copies, chunk_rows=chunk_rows, stats=stats)

    def holdout_split(self, share, seed=0):
        """validation.holdout_split on the ring: (train_index, holdout_index) of the valid rows in age order, both naming ring slots.
        A position held out under a seed is held out in every update, wherever it sits in the ring.  A host window runs the numpy
        statements.  The ring, the bookkeeping and rows() are unchanged."""
        if self._rings is None or self._valid == 0:
            check_holdout_options(share, seed)
            return self._index.clone(), self._index.clone()
        return holdout_split(self._rings[0], self._index, share, seed, self.board_size)

    def row_metrics(self, model, index=None, *, bucket_plies=8, buckets=16, chunk_rows=16384):
        """validation.row_metrics on the ring: the Metrics of `model` on the ring slots `index` (None: every valid row, in age order)."""
        s72, pi, z = self.rows() if self._rings is None else self._rings
        if index is None and self._rings is not None:
            index = self._index
        return row_metrics(model, s72, pi, z, index, bucket_plies=bucket_plies, buckets=buckets, chunk_rows=chunk_rows)

    def clear(self):
        """Empty the window; the ring keeps its size."""
        self._generations, self._start, self._valid = [], 0, 0
        self._index = torch.zeros((0,), dtype=torch.int64, device=self.device)

    # ---- appending
    def _checked(self, what, states72, second, third, second_dtypes, third_dtype):
        """Shapes and dtypes against the board, before anything is written; returns contiguous tensors on the window's device."""
        names = ("states72",) + {"append_counts": ("visits", "z"), "append_policy": ("policy", "z")}.get(what, ("pi", "z"))
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

    def _append(self, states72, visits, z_i8, pi, z_f32, m, search_value=None, value_blend=0.0, policy=None):
        skip, head = self._make_room(m)
        if skip:
            states72, visits, z_i8, pi, z_f32, search_value, policy = (None if x is None else x[skip:].contiguous()
                                                                       for x in (states72, visits, z_i8, pi, z_f32, search_value, policy))
        n = m - skip
        r72, rpi, rz = self._rings
        if self.device.type == "cpu":
            h = lambda x: None if x is None else x.numpy()          # noqa: E731   (views: the rings are written in place)
            append_reference(self.board_size, h(states72), h(visits), h(z_i8), h(pi), h(z_f32), head, h(r72), h(rpi), h(rz),
                             h(search_value), value_blend, h(policy))
        else:                                       # the three entry points differ in their four source arguments alone
            ptr = _lib.ptr
            if policy is not None:
                name, source = "aqg_replay_append_policy", (ptr(policy), ptr(z_i8), ptr(search_value), value_blend)
            elif search_value is not None:
                name, source = "aqg_replay_append_blend", (ptr(visits), ptr(z_i8), ptr(search_value), value_blend)
            else:
                name, source = "aqg_replay_append", (ptr(visits), ptr(z_i8), ptr(pi), ptr(z_f32))
            _lib.check(getattr(_lib.load(), name)(self.board_size, self.policy_size, ptr(states72), *source, n, self.capacity, head,
                                                  ptr(r72), ptr(rpi), ptr(rz), _lib.stream_ptr(self.device)), name)
        self._appended(n)

    def append_counts(self, states72, visits, z, search_value=None, value_blend=0.0):
        """One generation as the engine leaves it (engine.history_tensors / gather_history): states72 uint8 [n,72], visit counts
        int16 (or uint16; read as unsigned) [n,A], z int8 [n].  pi = counts / their sum, with the bits of the .history route.
        search_value (float32 [n], engine.history_values) with value_blend L in [0, 1]: the value target becomes (1 - L) z + L q
        (blend_targets; one aqg_replay_append_blend launch).  Without search_value the call is the plain append."""
        (s, v, zz), m = self._checked("append_counts", states72, visits, z, (torch.int16, torch.uint16), torch.int8)
        q, value_blend = self._checked_blend("append_counts", m, search_value, value_blend)
        self._append(s, v, zz, None, None, m, q, value_blend)

    def append_policy(self, states72, policy, z, search_value=None, value_blend=0.0):
        """One generation whose policy target the engine recorded itself (engine.history_policies): states72 uint8 [n,72], policy
        float32 [n,A] -- copied verbatim -- and z int8 [n].  The value target, search_value and value_blend, the eviction and the
        bookkeeping are append_counts'.  One aqg_replay_append_policy launch (append_reference(policy=) on a host window)."""
        (s, p, zz), m = self._checked("append_policy", states72, policy, z, (torch.float32,), torch.int8)
        q, value_blend = self._checked_blend("append_policy", m, search_value, value_blend)
        self._append(s, None, zz, None, None, m, q, value_blend, policy=p)

    def _checked_blend(self, what, m, search_value, value_blend):
        """The blend arguments of an append of m rows: (search_value on the window's device or None, the blend as the kernel gets it)."""
        if search_value is None:
            if value_blend != 0.0:
                raise ValueError(f"ReplayWindow.{what}: a value_blend needs search_value")
            return None, 0.0
        value_blend = check_value_blend(value_blend)
        q = torch.as_tensor(search_value)
        if q.dtype != torch.float32 or tuple(q.shape) != (m,):
            raise ValueError(f"ReplayWindow.{what}: search_value must be a torch.float32 ['n'] tensor with one value per "
                             f"position; got {q.dtype} {list(q.shape)}")
        return q.to(self.device).contiguous(), value_blend

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

    # ---- reanalyse
    def refresh_counts(self, slots, visits, actions, count, search_value=None, value_blend=0.0):
        """Overwrite the targets of the valid rows in ring slots `slots` (int64 [n], distinct; e.g. index()[positions]) with fresh
        search results as engine.search returns them -- visits int32 [n,MAX_LEGAL], actions uint8 [n,MAX_LEGAL], count int32 [n]:
        pi = counts / their sum scattered by action, with the bits of the append.  search_value (float32 [n], engine.root_values)
        with value_blend L in (0, 1]: the value target becomes (1 - L) z + L q, z being the value the ring holds now -- which may
        already be a blend.  One aqg_replay_refresh launch on the window's stream (refresh_reference on a host window); a row without
        a visit keeps its targets.  Shapes, dtypes and the slots -- each a valid slot, none twice: one device-to-host read -- are
        checked before anything is written.  The records, the bookkeeping, index() and rows() do not change."""
        self._refresh("refresh_counts", "visits", torch.int32, slots, visits, actions, count, search_value, value_blend)

    def refresh_policy(self, slots, policy, actions, count, search_value=None, value_blend=0.0):
        """refresh_counts with finished policy entries for the source: policy float32 [n,MAX_LEGAL] in legal_actions() order, as
        engine.root_improved_policy returns it, copied verbatim to the action ids of a zero row -- no total, no division.  A row is
        written iff 1 <= count <= MAX_LEGAL, every entry inside the count is finite and >= 0 and one is > 0; any other row keeps
        its targets.  One aqg_replay_refresh_policy launch on the window's stream (refresh_policy_reference on a host window); the
        checks, the blend and everything that does not change are refresh_counts'."""
        self._refresh("refresh_policy", "policy", torch.float32, slots, policy, actions, count, search_value, value_blend)

    def _refresh(self, what, source, source_dtype, slots, rows, actions, count, search_value, value_blend):
        """refresh_counts and refresh_policy behind one set of checks: `rows` is the visit rows or the policy rows."""
        xs = [torch.as_tensor(x) for x in (slots, rows, actions, count)]
        n = int(xs[0].shape[0]) if xs[0].dim() == 1 else -1
        specs = (("slots", torch.int64, ()), (source, source_dtype, (_lib.MAX_LEGAL,)), ("actions", torch.uint8, (_lib.MAX_LEGAL,)),
                 ("count", torch.int32, ()))
        if search_value is not None:
            xs.append(torch.as_tensor(search_value))
            specs += (("search_value", torch.float32, ()),)
        for x, (name, dtype, tail) in zip(xs, specs):
            if x.dtype != dtype or tuple(x.shape) != (n,) + tail:
                raise ValueError(f"ReplayWindow.{what}: {name} must be a {dtype} {['n', *tail]} tensor with one row per slot; "
                                 f"got {x.dtype} {list(x.shape)}")
        value_blend = check_value_blend(value_blend)
        if search_value is None and value_blend != 0.0:
            raise ValueError(f"ReplayWindow.{what}: a value_blend needs search_value")
        if n == 0:
            return
        if self._rings is None or self._valid == 0:
            raise ValueError(f"ReplayWindow.{what}: the window holds no row")
        xs = [x.to(self.device).contiguous() for x in xs]
        s = xs[0]
        valid = torch.zeros((self.capacity,), dtype=torch.bool, device=self.device)
        valid[self._index] = True
        inside = (s >= 0) & (s < self.capacity)
        stale = ~(inside & valid[s.clamp(0, self.capacity - 1)])
        ordered = torch.sort(s).values
        bad_slot, repeated = torch.stack((stale.any(), (ordered[1:] == ordered[:-1]).any())).tolist()      # the one read
        if bad_slot:
            raise ValueError(f"ReplayWindow.{what}: a slot holds no valid row of the window")
        if repeated:
            raise ValueError(f"ReplayWindow.{what}: a slot is named twice")
        q = xs[4] if search_value is not None and value_blend != 0.0 else None
        _, rpi, rz = self._rings
        as_policy = source == "policy"
        if self.device.type == "cpu":
            (refresh_policy_reference if as_policy else refresh_reference)(
                self.board_size, xs[1].numpy(), xs[2].numpy(), xs[3].numpy(), None if q is None else q.numpy(), value_blend, s.numpy(),
                rpi.numpy(), rz.numpy())
            return
        name = "aqg_replay_refresh_policy" if as_policy else "aqg_replay_refresh"
        entry = getattr(_lib.load(), name)
        with torch.cuda.device(self.device):
            _lib.check(entry(self.board_size, self.policy_size, _lib.ptr(xs[1]), _lib.ptr(xs[2]), _lib.ptr(xs[3]), _lib.ptr(q), value_blend,
                             _lib.ptr(s), n, self.capacity, _lib.ptr(rpi), _lib.ptr(rz), _lib.stream_ptr(self.device)), name)

    def extend_from_files(self, paths):
        """Each .history file as one generation, in the order given: oldest first."""
        for path in paths:
            with open(path, mode='rb') as f:
                self.append_history(pickle.load(f))
