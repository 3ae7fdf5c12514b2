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

Policy rows (`append_policy`, aqg_replay_append_policy): a generation whose policy target the engine recorded itself, as f32 rows
(engine.history_policies, the completed-Q target of self-play) -- the row is copied verbatim, z is converted or blended as the counts
form's.  `append_reference(..., policy=)` is the statement.

Position merge (`ReplayWindow.merged()`, `merge_positions`; csrc/replay_merge.hip): the window holds one row per OCCURRENCE of a
position -- every game's opening, and on the small boards many plies after it, thousands of times.  Merged, each distinct position is
one row whose targets are the mean of its occurrences' (each position then weighs the same; `count` is returned for another
weighting).  A position and its left-right mirror are NOT merged.  `merge_reference` and `position_keys` are the statements in numpy.

Reanalyse (`ReplayWindow.refresh_counts`, aqg_replay_refresh, csrc/replay_refresh.hip; the stage is reanalyse.reanalyse): the targets
of chosen valid rows overwritten, in one launch, by the results of a fresh search of their positions.  `refresh_reference` is the
kernel in numpy, `draw_reanalyse_rows` picks the rows of one pass.  `ReplayWindow.refresh_policy` (aqg_replay_refresh_policy,
`refresh_policy_reference`) is the same launch with finished f32 policy entries for the source, copied verbatim: the completed-Q
targets of engine.root_improved_policy.

Policy surprise weighting (`surprise_index`, `ReplayWindow.surprise_index`; csrc/replay_surprise.hip): which rows an update trains
on.  k = KL(the row's policy target || the policy of the network the update starts from), taken at training time -- so it is always
about the target the row holds now, whatever Reanalyse, the merge or a blend did to it -- becomes an expected number of copies, half
of the update's rows dealt out evenly and half in proportion to k (KataGo's policy surprise weighting); a counter-based draw per ring
slot rounds it to a count, and the update's `index` names each row that many times.  `surprise_reference` and
`surprise_counts_reference` are the two launches in numpy; the definition is in include/aqgnn.h.
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


def append_reference(board_size, states72, visits, z_i8, pi, z_f32, head, ring72, ring_pi, ring_z, search_value=None, value_blend=0.0,
                     policy=None):
    """aqg_replay_append in numpy, on host arrays, in place (include/aqgnn.h, "replay window"): source row i goes to ring slot
    (head + i) % capacity, n and capacity being the row counts of states72 and ring72.  Counts form (visits [n,A] int16 or uint16,
    read as UNSIGNED, and z_i8 [n] int8; pi and z_f32 None): ring_pi = float32(float64(v) / float64(tot)) with tot the row's integer
    sum, zeros where tot == 0, ring_z = float32(z).  Rows form (pi [n,A] float32, z_f32 [n] float32; the other two None): a copy.
    The 72 record bytes are copied verbatim.  search_value (float32 [n]; counts form only) makes it aqg_replay_append_blend:
    ring_z = blend_targets(z_i8, search_value, value_blend).  policy (float32 [n,A], with z_i8; visits, pi and z_f32 None) makes it
    aqg_replay_append_policy: ring_pi takes the row verbatim, ring_z is the counts form's, blended when search_value is given.
    Refuses what the C entry points refuse, with ValueError."""
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
    if policy is not None:
        if z_i8 is None or visits is not None or pi is not None or z_f32 is not None:
            raise ValueError("append_reference: policy goes with z_i8 alone (visits, pi and z_f32 None)")
    elif not counts and not finished:
        raise ValueError("append_reference: give the counts form (visits, z_i8) or the rows form (pi, z_f32), whole, and not both")
    if search_value is not None and not counts and policy is None:
        raise ValueError("append_reference: search_value goes with the counts form (visits, z_i8) or with policy")
    if capacity < 1 or not 0 <= head < capacity or n > capacity:
        raise ValueError("append_reference: needs capacity >= 1, 0 <= head < capacity and n <= capacity")
    for x, name, dtypes, shape in ((states72, "states72", (np.uint8,), (n, 72)), (ring72, "ring72", (np.uint8,), (capacity, 72)),
                                   (ring_pi, "ring_pi", (np.float32,), (capacity, A)), (ring_z, "ring_z", (np.float32,), (capacity,)),
                                   (visits, "visits", (np.int16, np.uint16), (n, A)), (z_i8, "z_i8", (np.int8,), (n,)),
                                   (pi, "pi", (np.float32,), (n, A)), (z_f32, "z_f32", (np.float32,), (n,)),
                                   (search_value, "search_value", (np.float32,), (n,)), (policy, "policy", (np.float32,), (n, A))):
        if x is not None and (x.dtype not in dtypes or tuple(x.shape) != shape):
            raise ValueError(f"append_reference: {name} must be {np.dtype(dtypes[0]).name} {list(shape)} ({board_size}x{board_size} board)")
    slots = (head + np.arange(n)) % capacity
    ring72[slots] = states72
    if policy is not None:
        ring_pi[slots] = policy
        ring_z[slots] = z_i8.astype(np.float32) if search_value is None else blend_targets(z_i8, search_value, value_blend)
    elif counts:
        v = visits.view(np.uint16).astype(np.int64)
        tot = v.sum(axis=1, keepdims=True)
        quotient = v.astype(np.float64) / np.where(tot > 0, tot, 1).astype(np.float64)
        ring_pi[slots] = quotient.astype(np.float32)                # a row without a visit: 0 / 1 = A zeros
        ring_z[slots] = z_i8.astype(np.float32) if search_value is None else blend_targets(z_i8, search_value, value_blend)
    else:
        ring_pi[slots] = pi
        ring_z[slots] = z_f32


# ---- reanalyse: chosen slots' targets overwritten by fresh search results (csrc/replay_refresh.hip)

def refresh_reference(board_size, visits, actions, count, search_value, blend, slots, ring_pi, ring_z):
    """aqg_replay_refresh in numpy, on host arrays, in place (include/aqgnn.h, "reanalyse") -- the kernel's statement and the backend
    of a host window.  Source row i is a searched root as engine.search returns it: visits int32 [n,MAX_LEGAL] and actions uint8
    [n,MAX_LEGAL] in legal_actions() order, count int32 [n]; slots int64 [n], distinct.  With c = count[i] and tot = the sum of
    visits[i, :c]: a row with c <= 0, c > MAX_LEGAL, tot <= 0 or a slot outside the ring is skipped; otherwise the whole row
    ring_pi[slots[i]] becomes zeros with float32(float64(v_j) / float64(tot)) at actions[i, j], j < c (an action >= A is dropped).
    search_value (float32 [n]) with blend L != 0: ring_z[slot] = blend_targets' arithmetic on the value the ring holds NOW --
    keep * ring_z[slot] + L * search_value[i], keep = float32(1) - L, every operation rounded to f32; search_value None or L == 0:
    ring_z is neither read nor written (and may be None).  Refuses what the C entry point refuses, with ValueError."""
    if board_size not in (3, 5, 7, 9):
        raise ValueError("refresh_reference: unsupported board_size (odd 3..9)")
    A = policy_size(board_size)
    b = np.float32(check_value_blend(blend))
    if search_value is None and b != 0:
        raise ValueError("refresh_reference: a blend needs search_value")
    blended = search_value is not None and b != 0
    n, capacity = int(np.shape(slots)[0]), int(ring_pi.shape[0])
    if capacity < 1:
        raise ValueError("refresh_reference: capacity must be >= 1")
    if blended and ring_z is None:
        raise ValueError("refresh_reference: a blend needs ring_z")
    for x, name, dtype, shape in ((visits, "visits", np.int32, (n, _lib.MAX_LEGAL)), (actions, "actions", np.uint8, (n, _lib.MAX_LEGAL)),
                                  (count, "count", np.int32, (n,)), (slots, "slots", np.int64, (n,)),
                                  (search_value, "search_value", np.float32, (n,)), (ring_pi, "ring_pi", np.float32, (capacity, A)),
                                  (ring_z, "ring_z", np.float32, (capacity,))):
        if x is not None and (x.dtype != dtype or tuple(x.shape) != shape):
            raise ValueError(f"refresh_reference: {name} must be {np.dtype(dtype).name} {list(shape)} ({board_size}x{board_size} board)")
    keep = np.float32(1.0) - b
    for i in range(n):
        c, slot = int(count[i]), int(slots[i])
        if c <= 0 or c > _lib.MAX_LEGAL or not 0 <= slot < capacity:
            continue
        v = visits[i, :c].astype(np.int64)
        tot = int(v.sum())
        if tot <= 0:
            continue
        row = np.zeros((A,), dtype=np.float32)
        inside = actions[i, :c] < A
        row[actions[i, :c][inside]] = (v[inside].astype(np.float64) / np.float64(tot)).astype(np.float32)
        ring_pi[slot] = row
        if blended:
            x, y = np.float32(keep * ring_z[slot]), np.float32(b * search_value[i])
            ring_z[slot] = np.float32(x + y)


def refresh_policy_reference(board_size, policy, actions, count, search_value, blend, slots, ring_pi, ring_z):
    """aqg_replay_refresh_policy in numpy, on host arrays, in place (include/aqgnn.h, "completed-Q policy targets") -- refresh_reference
    with finished policy entries for the source: policy float32 [n,MAX_LEGAL] in legal_actions() order (engine.root_improved_policy),
    copied VERBATIM to their action ids over a zero row, no total and no division.  With c = count[i], a row is written iff 1 <= c <=
    MAX_LEGAL, the slot is inside the ring, every entry j < c is finite and >= 0, and one of them is > 0 (an action >= A is dropped,
    but its entry counts in these tests).  The blend is refresh_reference's.  Refuses what the C entry point refuses, with ValueError."""
    if board_size not in (3, 5, 7, 9):
        raise ValueError("refresh_policy_reference: unsupported board_size (odd 3..9)")
    A = policy_size(board_size)
    b = np.float32(check_value_blend(blend))
    if search_value is None and b != 0:
        raise ValueError("refresh_policy_reference: a blend needs search_value")
    blended = search_value is not None and b != 0
    n, capacity = int(np.shape(slots)[0]), int(ring_pi.shape[0])
    if capacity < 1:
        raise ValueError("refresh_policy_reference: capacity must be >= 1")
    if blended and ring_z is None:
        raise ValueError("refresh_policy_reference: a blend needs ring_z")
    for x, name, dtype, shape in ((policy, "policy", np.float32, (n, _lib.MAX_LEGAL)), (actions, "actions", np.uint8, (n, _lib.MAX_LEGAL)),
                                  (count, "count", np.int32, (n,)), (slots, "slots", np.int64, (n,)),
                                  (search_value, "search_value", np.float32, (n,)), (ring_pi, "ring_pi", np.float32, (capacity, A)),
                                  (ring_z, "ring_z", np.float32, (capacity,))):
        if x is not None and (x.dtype != dtype or tuple(x.shape) != shape):
            raise ValueError(f"refresh_policy_reference: {name} must be {np.dtype(dtype).name} {list(shape)} ({board_size}x{board_size} board)")
    keep = np.float32(1.0) - b
    for i in range(n):
        c, slot = int(count[i]), int(slots[i])
        if c <= 0 or c > _lib.MAX_LEGAL or not 0 <= slot < capacity:
            continue
        v = policy[i, :c]
        if not (np.isfinite(v) & (v >= 0)).all() or not (v > 0).any():
            continue
        row = np.zeros((A,), dtype=np.float32)
        inside = actions[i, :c] < A
        row[actions[i, :c][inside]] = v[inside]
        ring_pi[slot] = row
        if blended:
            x, y = np.float32(keep * ring_z[slot]), np.float32(b * search_value[i])
            ring_z[slot] = np.float32(x + y)


def draw_reanalyse_rows(seed, update, eligible, rows):
    """Which of the `eligible` oldest valid rows of a window one reanalyse pass refreshes: int64 positions in age order, ascending.
    Row i's key is u_i = counter_uniform(stream_key(seed, update), i); the min(rows, eligible) rows of the smallest keys are taken
    (stable argsort).  A row's key depends on (seed, update, i) alone -- not on how many rows are asked for, nor on rank or slot
    count -- so the draw for R rows is a subset of the draw for R + 1, and every caller draws the same rows."""
    from .counter_rng import counter_uniform, stream_key
    eligible, rows = int(eligible), int(rows)
    if eligible < 0 or rows < 0:
        raise ValueError("draw_reanalyse_rows: eligible and rows must be >= 0")
    keys = counter_uniform(stream_key(int(seed), int(update)), np.arange(eligible, dtype=np.uint64))
    order = np.argsort(np.asarray(keys, dtype=np.float64).reshape(eligible), kind="stable")
    return np.sort(order[:min(rows, eligible)]).astype(np.int64)


# ---- position merge: rows that hold the same position become one row with the mean targets (csrc/replay_merge.hip)

KEY_BYTES = np.array([k for k in range(72) if k not in (68, 69, 71)])      # 68-69: the ply counter; 71: spare
MERGE_CHUNK = 64        # rows of one chunk of the summation order (MRG_CHUNK)


def _splitmix64(x):
    x = (np.asarray(x, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15))
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def position_keys(states72, index=None):
    """aqg_replay_position_keys in numpy, bit for bit: int64 [n], one hash of the key bytes (0..67 and 70) of each row index[i]
    (index None: every row): sum_k (b_k + 1) * (splitmix64(k) | 1) mod 2^64, then one splitmix64 step.  Changing one key byte always
    changes the key; bytes 68, 69 and 71 never do.  The hash only groups rows: merge_reference compares the bytes."""
    s = np.asarray(states72)
    if s.dtype != np.uint8 or s.ndim != 2 or s.shape[1] != 72:
        raise ValueError("position_keys: states72 must be uint8 [rows,72]")
    if index is not None:
        s = s[np.asarray(index, dtype=np.int64)]
    with np.errstate(over="ignore"):
        m = _splitmix64(KEY_BYTES.astype(np.uint64)) | np.uint64(1)
        h = ((s[:, KEY_BYTES].astype(np.uint64) + np.uint64(1)) * m[None, :]).sum(axis=1, dtype=np.uint64)
        return _splitmix64(h).view(np.int64)


def merge_depth(length):
    """The largest number of additions between a term and its run's total in the merge's summation order, for a run of `length`
    rows: min(L, 64) - 1 inside its chunk, ceil(L / 64) - 1 across the chunk sums."""
    length = int(length)
    return min(length, MERGE_CHUNK) - 1 + -(-length // MERGE_CHUNK) - 1


def _sum_in_order(x):
    """((x[0] + x[1]) + x[2]) + ... over the first axis, every sum rounded to f32."""
    acc = x[0].copy()
    for k in range(1, x.shape[0]):
        acc = acc + x[k]
    return acc


def merge_reference(states72, pi, z, index=None, perm=None):
    """The position merge in numpy on host arrays -- the kernels' statement, and what a CPU window runs.  Returns (out72, out_pi,
    out_z, count).

    The input is the rows index[0..n) of (states72 uint8 [rows,72], pi float32 [rows,A], z float32 [rows]) in the order given (index
    None: all rows).  perm (int64 [n], places of that input; None: the stable sort of position_keys) brings equal positions
    together; a run is a maximal stretch of perm whose rows have equal key bytes (bytes 0..67 and 70 -- a full compare, so rows that
    merely share a hash never merge).  One output row per run, the runs ordered by the place of their first row in the input: the
    record is the run's first row's 72 bytes verbatim, count (int32) its length L, pi and z the mean of its rows' in f32.  L == 1 is a
    copy.  Summation order: chunks of 64 rows of the run, each summed left to right from its first row, the chunk sums summed left
    to right, the total divided by float32(L) -- merge_depth(L) additions at most between a term and the total."""
    s, p, v = np.asarray(states72), np.asarray(pi), np.asarray(z)
    if s.dtype != np.uint8 or s.ndim != 2 or s.shape[1] != 72:
        raise ValueError("merge_reference: states72 must be uint8 [rows,72]")
    if p.dtype != np.float32 or p.ndim != 2 or p.shape[0] != s.shape[0] or v.dtype != np.float32 or v.shape != (s.shape[0],):
        raise ValueError("merge_reference: pi must be float32 [rows,A] and z float32 [rows]")
    rows = np.arange(s.shape[0], dtype=np.int64) if index is None else np.asarray(index, dtype=np.int64)
    n = rows.shape[0]
    if n and (rows.min() < 0 or rows.max() >= s.shape[0]):
        raise ValueError("merge_reference: index names a row the arrays do not have")
    if perm is None:
        perm = np.argsort(position_keys(s, rows), kind="stable")
    perm = np.asarray(perm, dtype=np.int64)
    if perm.shape != (n,) or not np.array_equal(np.sort(perm), np.arange(n)):
        raise ValueError("merge_reference: perm must be a permutation of the input's places")
    if n == 0:
        return s[:0].copy(), p[:0].copy(), v[:0].copy(), np.zeros((0,), dtype=np.int32)
    src = rows[perm]
    kb = s[src][:, KEY_BYTES]
    heads = np.ones((n,), dtype=bool)
    heads[1:] = (kb[1:] != kb[:-1]).any(axis=1)
    starts = np.flatnonzero(heads)
    lengths = np.diff(np.append(starts, n))
    rank = np.argsort(perm[starts], kind="stable")          # runs by the place of their first row (a stable sort's perm: the least)
    moved = np.concatenate([src[starts[r]:starts[r] + lengths[r]] for r in rank])
    return merge_runs_reference(s, p, v, moved, np.cumsum(lengths[rank]) - lengths[rank])


def merge_runs_reference(states72, pi, z, perm, starts):
    """aqg_replay_merge_runs in numpy: output row o is the run of rows perm[starts[o]], ..., perm[starts[o + 1] - 1] (the last run
    ends at len(perm)), summed in the order perm gives them.  Returns (out72, out_pi, out_z, count); merge_reference states the order."""
    perm, starts = np.asarray(perm, dtype=np.int64), np.asarray(starts, dtype=np.int64)
    ends = np.append(starts[1:], perm.shape[0])
    u = starts.shape[0]
    out72 = np.empty((u, 72), dtype=np.uint8)
    out_pi = np.empty((u, pi.shape[1]), dtype=np.float32)
    out_z = np.empty((u,), dtype=np.float32)
    count = (ends - starts).astype(np.int32)
    single = count == 1
    out72[:], out_pi[single], out_z[single] = states72[perm[starts]], pi[perm[starts[single]]], z[perm[starts[single]]]
    for o in np.flatnonzero(~single):
        run = perm[starts[o]:ends[o]]
        x = np.concatenate([pi[run], z[run][:, None]], axis=1)                                 # z is column A of the row
        if run.shape[0] > MERGE_CHUNK:
            x = np.stack([_sum_in_order(x[c:c + MERGE_CHUNK]) for c in range(0, run.shape[0], MERGE_CHUNK)])
        mean = _sum_in_order(x) / np.float32(run.shape[0])
        out_pi[o], out_z[o] = mean[:-1], mean[-1]
    return out72, out_pi, out_z, count


def merge_positions(states72, pi, z, index=None, board_size=BOARD_SIZE):
    """The position merge on the GPU: (out72 uint8 [u,72], out_pi float32 [u,A], out_z float32 [u], count int32 [u]) of the rows
    index[0..n) (int64, on the tensors' device; None: all rows) of the device tensors (states72, pi, z) -- merge_reference's result bit
    for bit.  aqg_replay_position_keys hashes the rows, torch sorts the keys (stable), aqg_replay_run_heads marks where the key BYTES
    change, torch turns that into runs in first-occurrence order, aqg_replay_merge_runs writes the rows.  Host reads: the bounds of
    index, and the run starts (whose number sizes the outputs)."""
    if board_size not in (3, 5, 7, 9):
        raise ValueError("merge_positions: unsupported board_size (odd 3..9)")
    A = policy_size(board_size)
    rows = int(states72.shape[0]) if states72.dim() == 2 else -1
    for x, name, dtype, shape in ((states72, "states72", torch.uint8, (rows, 72)), (pi, "pi", torch.float32, (rows, A)),
                                  (z, "z", torch.float32, (rows,))):
        if x.dtype != dtype or tuple(x.shape) != shape or not x.is_cuda or x.device != states72.device:
            raise ValueError(f"merge_positions: {name} must be a {dtype} {list(shape)} tensor on the GPU ({board_size}x{board_size} board)")
    dev = states72.device
    states72, pi, z = states72.contiguous(), pi.contiguous(), z.contiguous()
    if index is not None:
        if index.dtype != torch.int64 or index.dim() != 1 or index.device != dev:
            raise ValueError("merge_positions: index must be an int64 [n] tensor on the rows' device")
        index = index.contiguous()
        if index.numel():
            lo, hi = torch.stack((index.min(), index.max())).tolist()
            if lo < 0 or hi >= rows:
                raise ValueError("merge_positions: index names a row the arrays do not have")
    n = rows if index is None else int(index.numel())
    lib, st = _lib.load(), _lib.stream_ptr(dev)
    with torch.cuda.device(dev):
        if n == 0:
            return (torch.zeros((0, 72), dtype=torch.uint8, device=dev), torch.zeros((0, A), dtype=torch.float32, device=dev),
                    torch.zeros((0,), dtype=torch.float32, device=dev), torch.zeros((0,), dtype=torch.int32, device=dev))
        keys = torch.empty((n,), dtype=torch.int64, device=dev)
        _lib.check(lib.aqg_replay_position_keys(_lib.ptr(states72), _lib.ptr(index), n, _lib.ptr(keys), st), "aqg_replay_position_keys")
        perm = torch.sort(keys, stable=True).indices                    # places of the input; equal keys stay in input order
        src = perm if index is None else index[perm]                    # the same, as rows of the arrays
        heads = torch.empty((n,), dtype=torch.uint8, device=dev)
        _lib.check(lib.aqg_replay_run_heads(_lib.ptr(states72), _lib.ptr(src), n, _lib.ptr(heads), st), "aqg_replay_run_heads")
        starts = heads.nonzero().squeeze(1)                             # the one device-to-host read: u sizes the outputs
        u = int(starts.numel())
        if u == n:                                                      # no repeats: every run is its own row, in input order
            src = torch.arange(n, dtype=torch.int64, device=dev) if index is None else index
            starts = torch.arange(n, dtype=torch.int64, device=dev)
        else:
            # runs into first-occurrence order (a stable sort keeps a run's rows in input order, so its first place is perm[start])
            lengths = torch.diff(starts, append=torch.tensor([n], dtype=torch.int64, device=dev))
            rank = torch.sort(perm[starts]).indices                     # rank[o] = the run that becomes output row o
            lengths_out = lengths[rank]
            starts_out = torch.cumsum(lengths_out, 0) - lengths_out
            where = torch.empty_like(rank)
            where[rank] = starts_out                                    # where[r] = the first place of run r in the new order
            run_of = torch.cumsum(heads, 0, dtype=torch.int64) - 1
            place = where[run_of] + (torch.arange(n, dtype=torch.int64, device=dev) - starts[run_of])
            moved = torch.empty_like(src)
            moved[place] = src
            src, starts = moved, starts_out.contiguous()
        out = (torch.empty((u, 72), dtype=torch.uint8, device=dev), torch.empty((u, A), dtype=torch.float32, device=dev),
               torch.empty((u,), dtype=torch.float32, device=dev), torch.empty((u,), dtype=torch.int32, device=dev))
        floats = int(lib.aqg_replay_merge_workspace_floats(board_size, n, u))
        work = torch.empty((floats,), dtype=torch.float32, device=dev) if floats else None
        _lib.check(lib.aqg_replay_merge_runs(board_size, A, _lib.ptr(states72), _lib.ptr(pi), _lib.ptr(z), _lib.ptr(src), _lib.ptr(starts),
                                             n, u, *(_lib.ptr(x) for x in out), _lib.ptr(work), floats, st), "aqg_replay_merge_runs")
    return out


# ---- policy surprise weighting: the rows of an update drawn by KL(target || network) (csrc/replay_surprise.hip)

SURPRISE_MAX_ROWS = 1 << 24         # m at most (SPR_MAX_ROWS): S = sum q < 2^51
SURPRISE_TINY = np.float32(2.0 ** -126)     # the least p a logarithm is taken of (SPR_TINY)
SURPRISE_K_MAX = 88.0               # > 126 ln 2 (SPR_K_MAX): never reached by a row whose target sums to 1
SURPRISE_Q_SCALE = 2.0 ** 20


def check_surprise_options(expected_rows, uniform_share, max_copies):
    """Validate the options of steps 3 and 4 as the library does: expected_rows None or an int >= 1, uniform_share in [0, 1] and not
    NaN, max_copies an int in 1..255.  Returns them as (int or None, float, int)."""
    share = float(uniform_share)
    if not 0.0 <= share <= 1.0:
        raise ValueError(f"uniform_share must be in [0, 1], not {uniform_share}")
    if int(max_copies) != max_copies or not 1 <= int(max_copies) <= 255:
        raise ValueError(f"max_copies must be an integer in 1 .. 255, not {max_copies}")
    if expected_rows is not None and (int(expected_rows) != expected_rows or not 1 <= int(expected_rows) <= 1 << 40):
        raise ValueError(f"expected_rows must be an integer in 1 .. 2^40, not {expected_rows}")
    return None if expected_rows is None else int(expected_rows), share, int(max_copies)


def surprise_reference(pi, net_policy, index=None):
    """aqg_replay_surprise_rows in numpy (include/aqgnn.h, "policy surprise weighting", steps 1 and 2): (k float32 [m], q int32 [m]) of
    the rows index[0..m) of pi float32 [rows,A] (index None: rows 0..m-1) against net_policy float32 [m,A], the network's softmaxed
    policy of each of those rows.  KL = sum over t_a > 0 of t_a (ln t_a - ln max(p_a, 2^-126)) in float64, in the kernel's order: a
    lane's own entries a = lane, lane + 64, ... in ascending order, then the xor-shuffle reduction 32, 16, ..., 1; k = f32(min(max(KL,
    0), 88)), q = floor(k 2^20).  k = q = 0 for a row with a non-finite entry in t or p, a negative target entry, no positive target
    entry, or an index entry outside pi."""
    t_all, p = np.asarray(pi), np.asarray(net_policy)
    if t_all.dtype != np.float32 or t_all.ndim != 2 or p.dtype != np.float32 or p.ndim != 2 or p.shape[1] != t_all.shape[1]:
        raise ValueError("surprise_reference: pi must be float32 [rows,A] and net_policy float32 [m,A]")
    m, A = p.shape
    rows = np.arange(m, dtype=np.int64) if index is None else np.asarray(index, dtype=np.int64)
    if rows.shape != (m,) or m > SURPRISE_MAX_ROWS or (index is None and m > t_all.shape[0]):
        raise ValueError("surprise_reference: one network policy row per row of index (or of pi), 2^24 at most")
    inside = (rows >= 0) & (rows < t_all.shape[0])
    t = np.zeros((m, A), dtype=np.float32)
    t[inside] = t_all[rows[inside]]
    with np.errstate(all="ignore"):
        bad = ~np.isfinite(t).all(axis=1) | ~np.isfinite(p).all(axis=1) | (t < 0).any(axis=1)
        positive = t > 0
        ok = inside & ~bad & positive.any(axis=1)
        pc = np.where(p > SURPRISE_TINY, p, SURPRISE_TINY)
        ts = np.where(positive, t, np.float32(1.0)).astype(np.float64)
        d = np.log(ts) - np.log(pc.astype(np.float64))
        term = np.where(positive, ts * d, 0.0)
        passes = -(-A // 64)
        lanes = np.zeros((m, passes * 64), dtype=np.float64)
        lanes[:, :A] = term
        lanes = lanes.reshape(m, passes, 64)
        acc = np.zeros((m, 64), dtype=np.float64)
        for s in range(passes):                                 # +0.0 + term is the term: an entry that adds nothing changes nothing
            acc = acc + lanes[:, s]
        lane = np.arange(64)
        for off in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[:, lane ^ off]
        kl = np.where(ok, acc[:, 0], 0.0)
        k = np.minimum(np.maximum(kl, 0.0), SURPRISE_K_MAX).astype(np.float32)
    k[~ok] = 0                                                  # (a NaN sum of a rejected row)
    return k, surprise_weights(k)


def surprise_weights(k):
    """Step 2 in numpy: q = floor(float64(k) * 2^20) as int32, for k float32 in [0, 88] -- an exact product, q < 2^27."""
    k = np.asarray(k)
    if k.dtype != np.float32:
        raise ValueError("surprise_weights: k must be float32")
    return np.floor(k.astype(np.float64) * SURPRISE_Q_SCALE).astype(np.int32)


def expand_rows(base, count, total=None):
    """Step 5 on torch tensors of one device: base int64 [m] (the rows in input order) with row j repeated count[j] times.  total: the
    sum of count when the caller has it (it then costs no read of the device)."""
    return torch.repeat_interleave(base, count.to(torch.int64), output_size=None if total is None else int(total))


def surprise_counts_reference(q, rows_of_q, seed, update, expected_rows, uniform_share, max_copies):
    """aqg_replay_surprise_counts in numpy (steps 3 and 4), int32 [m]: q int32 [m], rows_of_q the place of each of its rows in the
    arrays (int64 [m]; for a window the ring slots; None: 0..m-1), which keys the row's draw.  f = (E U) / m + ((E (1 - U)) q) / S
    in float64 in that order (S = sum q; S == 0: f = E / m), count = min(floor(f) + [u < f - floor(f)], C) with u =
    counter_uniform(stream_key(seed, update), row)."""
    from .counter_rng import counter_uniform, stream_key
    q = np.asarray(q)
    if q.dtype != np.int32 or q.ndim != 1 or q.shape[0] > SURPRISE_MAX_ROWS:
        raise ValueError("surprise_counts_reference: q must be int32 [m], m <= 2^24")
    m = q.shape[0]
    rows = np.arange(m, dtype=np.int64) if rows_of_q is None else np.asarray(rows_of_q, dtype=np.int64)
    if rows.shape != (m,):
        raise ValueError("surprise_counts_reference: one row per entry of q")
    E, U, C = check_surprise_options(expected_rows, uniform_share, max_copies)
    if E is None:
        raise ValueError("surprise_counts_reference: expected_rows must be given")
    if m == 0:
        return np.zeros((0,), dtype=np.int32)
    E, U, md = np.float64(E), np.float64(U), np.float64(m)
    S = int(q.astype(np.int64).sum())
    if S > 0:
        uniform = (E * U) / md
        rest = E * (np.float64(1.0) - U)
        f = uniform + (rest * q.astype(np.float64)) / np.float64(S)
    else:
        f = np.full((m,), E / md, dtype=np.float64)
    whole = np.floor(f)
    u = counter_uniform(stream_key(int(seed), int(update)), rows.astype(np.uint64))
    c = whole + (np.asarray(u, dtype=np.float64).reshape(m) < f - whole)
    return np.minimum(c, np.float64(C)).astype(np.int32)


def surprise_index(model, states72, pi, index=None, *, seed, update, expected_rows=None, uniform_share=0.5, max_copies=8,
                   chunk_rows=16384, stats=None):
    """The rows an update trains on, drawn by policy surprise, on the GPU: (index int64 [M], k float32 [m], count int32 [m]) for the rows
    index[0..m) (int64, on the tensors' device; None: all rows) of the device tensors states72 uint8 [rows,72] and pi float32 [rows,A].
    The returned index names those rows in input order, row j count[j] times -- a valid `index` for every trainer's epoch.

    model.forward_states runs over the records in chunks of at most chunk_rows rows (the policy buffer stays at most chunk_rows * 4A
    bytes), in eval mode, without autograd, with its fp16-range guard, and the module's mode is left as it was; one
    aqg_replay_surprise_rows launch per chunk, the exact integer sum of q on the device, one aqg_replay_surprise_counts launch, and
    torch.cumsum / torch.repeat_interleave for the expansion.  expected_rows None: m.  One device-to-host read of its own (besides the
    forward's guard): M with the statistics, which a dict given as `stats` receives -- rows, expanded, left_out, most_copies, mean_kl.
    surprise_reference and surprise_counts_reference are the two launches in numpy."""
    E, U, C = check_surprise_options(expected_rows, uniform_share, max_copies)
    if int(chunk_rows) < 1:
        raise ValueError("surprise_index: chunk_rows must be >= 1")
    board_size, A = int(model.board_size), int(model.policy_output_size)
    if board_size not in (3, 5, 7, 9) or A != policy_size(board_size):
        raise ValueError("surprise_index: unsupported board_size (odd 3..9)")
    rows = int(states72.shape[0]) if states72.dim() == 2 else -1
    for x, name, dtype, shape in ((states72, "states72", torch.uint8, (rows, 72)), (pi, "pi", torch.float32, (rows, A))):
        if x.dtype != dtype or tuple(x.shape) != shape or not x.is_cuda or x.device != states72.device:
            raise ValueError(f"surprise_index: {name} must be a {dtype} {list(shape)} tensor on the GPU ({board_size}x{board_size} board)")
    dev = states72.device
    states72, pi = states72.contiguous(), pi.contiguous()
    if index is not None:
        if index.dtype != torch.int64 or index.dim() != 1 or index.device != dev:
            raise ValueError("surprise_index: index must be an int64 [m] tensor on the rows' device")
        index = index.contiguous()
    m = rows if index is None else int(index.numel())
    if m > SURPRISE_MAX_ROWS:
        raise ValueError(f"surprise_index: {m} rows; 2^24 at most")
    if m == 0:
        if stats is not None:
            stats.update(rows=0, expanded=0, left_out=0, most_copies=0, mean_kl=0.0)
        return (torch.zeros((0,), dtype=torch.int64, device=dev), torch.zeros((0,), dtype=torch.float32, device=dev),
                torch.zeros((0,), dtype=torch.int32, device=dev))
    E = m if E is None else E
    lib, st = _lib.load(), _lib.stream_ptr(dev)
    chunk = int(chunk_rows)
    was_training = bool(getattr(model, "training", False))
    with torch.cuda.device(dev):
        k = torch.empty((m,), dtype=torch.float32, device=dev)
        q = torch.empty((m,), dtype=torch.int32, device=dev)
        count = torch.empty((m,), dtype=torch.int32, device=dev)
        model.eval()
        try:
            with torch.no_grad():
                for off in range(0, m, chunk):
                    n = min(chunk, m - off)
                    records = states72[off:off + n] if index is None else states72.index_select(0, index[off:off + n])
                    net_policy = model.forward_states(records.contiguous())[0].contiguous()
                    _lib.check(lib.aqg_replay_surprise_rows(board_size, A, _lib.ptr(net_policy), _lib.ptr(pi), _lib.ptr(index), rows, m, off, n,
                                                            _lib.ptr(k), _lib.ptr(q), st), "aqg_replay_surprise_rows")
        finally:
            model.train(was_training)
        total = q.sum(dtype=torch.int64).reshape(1)                    # exact, and it stays on the device
        _lib.check(lib.aqg_replay_surprise_counts(_lib.ptr(q), _lib.ptr(index), _lib.ptr(total), m, E, U, C, int(seed) & ((1 << 64) - 1),
                                                  int(update) & ((1 << 64) - 1), _lib.ptr(count), st), "aqg_replay_surprise_counts")
        ends = torch.cumsum(count, 0, dtype=torch.int64)
        M, left_out, most, kl_sum = torch.stack((ends[-1].double(), (count == 0).sum().double(), count.max().double(),
                                                 k.sum(dtype=torch.float64))).tolist()          # the one read
        base = torch.arange(m, dtype=torch.int64, device=dev) if index is None else index
        expanded = expand_rows(base, count, M)
    if stats is not None:
        stats.update(rows=m, expanded=int(M), left_out=int(left_out), most_copies=int(most), mean_kl=kl_sum / m)
    return expanded, k, count


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
        if self._rings is None or self._valid == 0:
            s72 = torch.zeros((0, 72), dtype=torch.uint8, device=self.device)
            pi = torch.zeros((0, self.policy_size), dtype=torch.float32, device=self.device)
            return surprise_index(model, s72, pi, seed=seed, update=update, expected_rows=expected_rows, uniform_share=uniform_share,
                                  max_copies=max_copies, chunk_rows=chunk_rows, stats=stats)
        return surprise_index(model, self._rings[0], self._rings[1], self._index, seed=seed, update=update, expected_rows=expected_rows,
                              uniform_share=uniform_share, max_copies=max_copies, chunk_rows=chunk_rows, stats=stats)

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
        elif policy is not None:
            _lib.check(_lib.load().aqg_replay_append_policy(self.board_size, self.policy_size, _lib.ptr(states72), _lib.ptr(policy),
                                                            _lib.ptr(z_i8), _lib.ptr(search_value), value_blend, n, self.capacity, head,
                                                            _lib.ptr(r72), _lib.ptr(rpi), _lib.ptr(rz), _lib.stream_ptr(self.device)),
                       "aqg_replay_append_policy")
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
