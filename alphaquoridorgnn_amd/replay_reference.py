"""The replay window's kernels stated in numpy, on host arrays (numpy only: neither torch nor the library is imported) -- what the tests
hold the launches to bit for bit, and what a ReplayWindow in host memory runs.  In the order of csrc/: the append and its blend
(replay.hip), Reanalyse's refresh in both forms and the draw of its rows (replay_refresh.hip), the position merge (replay_merge.hip),
policy surprise weighting (replay_surprise.hip), row metrics and the hold-out split (row_metrics.hip).  Every name here is importable from alphaquoridorgnn_amd.replay as well."""
import numpy as np

from .constants import MAX_LEGAL, check_board_size, num_actions
from .counter_rng import counter_uniform, stream_key


def _check_arrays(what, board_size, specs):
    """specs: (array or None, name, dtypes, shape) each; a given array must have one of the dtypes and the shape."""
    for x, name, dtypes, shape in specs:
        if x is not None and (x.dtype not in dtypes or tuple(x.shape) != shape):
            raise ValueError(f"{what}: {name} must be {np.dtype(dtypes[0]).name} {list(shape)} ({board_size}x{board_size} board)")


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
    A = num_actions(board_size)
    if search_value is None and value_blend != 0.0:
        raise ValueError("append_reference: a value_blend needs search_value")
    if search_value is not None:
        check_value_blend(value_blend)
    check_board_size(board_size, "append_reference")
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
    _check_arrays("append_reference", board_size, (
        (states72, "states72", (np.uint8,), (n, 72)), (ring72, "ring72", (np.uint8,), (capacity, 72)),
        (ring_pi, "ring_pi", (np.float32,), (capacity, A)), (ring_z, "ring_z", (np.float32,), (capacity,)),
        (visits, "visits", (np.int16, np.uint16), (n, A)), (z_i8, "z_i8", (np.int8,), (n,)),
        (pi, "pi", (np.float32,), (n, A)), (z_f32, "z_f32", (np.float32,), (n,)),
        (search_value, "search_value", (np.float32,), (n,)), (policy, "policy", (np.float32,), (n, A))))
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

def _count_entries(v):         # a visit row's entries, v_j / tot; None (the row is skipped) unless tot > 0
    v = v.astype(np.int64)
    tot = int(v.sum())
    return None if tot <= 0 else (v.astype(np.float64) / np.float64(tot)).astype(np.float32)


def _policy_entries(v):        # a finished policy row's entries, verbatim; None unless all are finite and >= 0 and one is > 0
    return v if (np.isfinite(v) & (v >= 0)).all() and (v > 0).any() else None


def _refresh(what, source_name, source_dtype, entries, board_size, source, actions, count, search_value, blend, slots, ring_pi, ring_z):
    """Both forms of the refresh: `what` names the entry in the messages, `source` is its [n,MAX_LEGAL] array of source_dtype, and
    entries(source[i, :c]) gives the float32 values written at the row's action ids, or None for a row that keeps its targets."""
    check_board_size(board_size, what)
    A = num_actions(board_size)
    b = np.float32(check_value_blend(blend))
    if search_value is None and b != 0:
        raise ValueError(f"{what}: a blend needs search_value")
    blended = search_value is not None and b != 0
    n, capacity = int(np.shape(slots)[0]), int(ring_pi.shape[0])
    if capacity < 1:
        raise ValueError(f"{what}: capacity must be >= 1")
    if blended and ring_z is None:
        raise ValueError(f"{what}: a blend needs ring_z")
    _check_arrays(what, board_size, (
        (source, source_name, (source_dtype,), (n, MAX_LEGAL)), (actions, "actions", (np.uint8,), (n, MAX_LEGAL)),
        (count, "count", (np.int32,), (n,)), (slots, "slots", (np.int64,), (n,)),
        (search_value, "search_value", (np.float32,), (n,)), (ring_pi, "ring_pi", (np.float32,), (capacity, A)),
        (ring_z, "ring_z", (np.float32,), (capacity,))))
    keep = np.float32(1.0) - b
    for i in range(n):
        c, slot = int(count[i]), int(slots[i])
        if c <= 0 or c > MAX_LEGAL or not 0 <= slot < capacity:
            continue
        values = entries(source[i, :c])
        if values is None:
            continue
        row = np.zeros((A,), dtype=np.float32)
        inside = actions[i, :c] < A
        row[actions[i, :c][inside]] = values[inside]
        ring_pi[slot] = row
        if blended:
            x, y = np.float32(keep * ring_z[slot]), np.float32(b * search_value[i])
            ring_z[slot] = np.float32(x + y)


def refresh_reference(board_size, visits, actions, count, search_value, blend, slots, ring_pi, ring_z):
    """aqg_replay_refresh in numpy, on host arrays, in place (include/aqgnn.h, "reanalyse") -- the kernel's statement and the backend
    of a host window.  Source row i is a searched root as engine.search returns it: visits int32 [n,MAX_LEGAL] and actions uint8
    [n,MAX_LEGAL] in legal_actions() order, count int32 [n]; slots int64 [n], distinct.  With c = count[i] and tot = the sum of
    visits[i, :c]: a row with c <= 0, c > MAX_LEGAL, tot <= 0 or a slot outside the ring is skipped; otherwise the whole row
    ring_pi[slots[i]] becomes zeros with float32(float64(v_j) / float64(tot)) at actions[i, j], j < c (an action >= A is dropped).
    search_value (float32 [n]) with blend L != 0: ring_z[slot] = blend_targets' arithmetic on the value the ring holds NOW --
    keep * ring_z[slot] + L * search_value[i], keep = float32(1) - L, every operation rounded to f32; search_value None or L == 0:
    ring_z is neither read nor written (and may be None).  Refuses what the C entry point refuses, with ValueError."""
    _refresh("refresh_reference", "visits", np.int32, _count_entries, board_size, visits, actions, count, search_value, blend, slots,
             ring_pi, ring_z)


def refresh_policy_reference(board_size, policy, actions, count, search_value, blend, slots, ring_pi, ring_z):
    """aqg_replay_refresh_policy in numpy, on host arrays, in place (include/aqgnn.h, "completed-Q policy targets") -- refresh_reference
    with finished policy entries for the source: policy float32 [n,MAX_LEGAL] in legal_actions() order (engine.root_improved_policy),
    copied VERBATIM to their action ids over a zero row, no total and no division.  With c = count[i], a row is written iff 1 <= c <=
    MAX_LEGAL, the slot is inside the ring, every entry j < c is finite and >= 0, and one of them is > 0 (an action >= A is dropped,
    but its entry counts in these tests).  The blend is refresh_reference's.  Refuses what the C entry point refuses, with ValueError."""
    _refresh("refresh_policy_reference", "policy", np.float32, _policy_entries, board_size, policy, actions, count, search_value, blend,
             slots, ring_pi, ring_z)


def draw_reanalyse_rows(seed, update, eligible, rows):
    """Which of the `eligible` oldest valid rows of a window one reanalyse pass refreshes: int64 positions in age order, ascending.
    Row i's key is u_i = counter_uniform(stream_key(seed, update), i); the min(rows, eligible) rows of the smallest keys are taken
    (stable argsort).  A row's key depends on (seed, update, i) alone -- not on how many rows are asked for, nor on rank or slot
    count -- so the draw for R rows is a subset of the draw for R + 1, and every caller draws the same rows."""
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


def surprise_counts_reference(q, rows_of_q, seed, update, expected_rows, uniform_share, max_copies):
    """aqg_replay_surprise_counts in numpy (steps 3 and 4), int32 [m]: q int32 [m], rows_of_q the place of each of its rows in the
    arrays (int64 [m]; for a window the ring slots; None: 0..m-1), which keys the row's draw.  f = (E U) / m + ((E (1 - U)) q) / S
    in float64 in that order (S = sum q; S == 0: f = E / m), count = min(floor(f) + [u < f - floor(f)], C) with u =
    counter_uniform(stream_key(seed, update), row)."""
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


# ---- row metrics: what a network scores on held-out rows, and the split by position (csrc/row_metrics.hip)

ROW_METRICS_MAX_ROWS = 1 << 24      # m at most (RM_MAX_ROWS)
ROW_METRICS_MAX_BUCKETS = 64        # buckets at most (RM_MAX_BUCKETS); the tag's bucket field is 8 bits
ROW_METRICS_TINY = np.float32(2.0 ** -126)      # the least p a logarithm is taken of (RM_TINY)
ROW_METRICS_CHUNK = 4096            # rows of one workgroup column of the reduction's first launch (RMR_CHUNK)
ROW_METRICS_LANES = 256             # lanes of such a workgroup (RMR_LANES)
TAG_HIT, TAG_SIGN_COUNTED, TAG_SIGN_AGREES = 1 << 8, 1 << 9, 1 << 10
HOLDOUT_STREAM = 0x686F6C646F7574   # AQG_HOLDOUT_STREAM: the sub-stream of a seed that splits positions


def check_row_metrics_options(bucket_plies, buckets):
    """Validate the bucket options as the library does: bucket_plies an int >= 1 (below 2^31), buckets an int in 1 .. 64.  Returns
    them as ints."""
    if int(bucket_plies) != bucket_plies or not 1 <= int(bucket_plies) < 1 << 31:
        raise ValueError(f"bucket_plies must be an integer >= 1, not {bucket_plies}")
    if int(buckets) != buckets or not 1 <= int(buckets) <= ROW_METRICS_MAX_BUCKETS:
        raise ValueError(f"buckets must be an integer in 1 .. 64, not {buckets}")
    return int(bucket_plies), int(buckets)


def check_holdout_options(share, seed=0, every=1):
    """Validate the hold-out options as the library and the loop do: share a float strictly inside (0, 1) and not NaN, seed an
    integer (taken mod 2^64), every an integer >= 1.  Returns them as (float, int, int)."""
    s = float(share)
    if not 0.0 < s < 1.0:
        raise ValueError(f"holdout share must be in (0, 1), not {share}")
    if int(seed) != seed:
        raise ValueError(f"holdout seed must be an integer, not {seed}")
    if int(every) != every or int(every) < 1:
        raise ValueError(f"holdout every must be an integer >= 1, not {every}")
    return s, int(seed) & ((1 << 64) - 1), int(every)


def _lane_sums(term):
    """The kernel's sum of each row of term float64 [m,A]: lane l adds its entries l, l + 64, ... ascending to +0.0, then the
    xor-shuffle reduction 32, 16, ..., 1.  float64 [m]."""
    m, A = term.shape
    passes = -(-A // 64)
    lanes = np.zeros((m, passes * 64), dtype=np.float64)
    lanes[:, :A] = term
    lanes = lanes.reshape(m, passes, 64)
    acc = np.zeros((m, 64), dtype=np.float64)
    for s in range(passes):                                     # +0.0 + term is the term: an entry that adds nothing changes nothing
        acc = acc + lanes[:, s]
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lane ^ off]
    return acc[:, 0]


def row_metrics_reference(states72, pi, z, net_policy, net_value, index=None, bucket_plies=8, buckets=16):
    """aqg_replay_row_metrics in numpy (include/aqgnn.h, "row metrics"): (vals float64 [m,4], tag int32 [m]) of the rows index[0..m) of
    (states72 uint8 [rows,72], pi float32 [rows,A], z float32 [rows]) (index None: rows 0..m-1) against net_policy float32 [m,A] and
    net_value float32 [m], the network's outputs for each of those rows.  vals = {ce, ent, lp, se}, tag = bucket | hit << 8 | sign
    counted << 9 | sign agrees << 10; a rejected row -- a non-finite entry in t, p, v or z, a negative target entry, no positive target
    entry, an index entry outside the arrays -- has zeros and the tag `buckets`.  Every sum in float64 in the kernel's order
    (_lane_sums); where the kernel's libm and numpy's differ (ln, exp) the results differ by their rounding, everything else is the
    kernel's bits."""
    bucket_plies, buckets = check_row_metrics_options(bucket_plies, buckets)
    s72, t_all, z_all, p, v = np.asarray(states72), np.asarray(pi), np.asarray(z), np.asarray(net_policy), np.asarray(net_value)
    if s72.dtype != np.uint8 or s72.ndim != 2 or s72.shape[1] != 72:
        raise ValueError("row_metrics_reference: states72 must be uint8 [rows,72]")
    rows = s72.shape[0]
    if (t_all.dtype != np.float32 or t_all.ndim != 2 or t_all.shape[0] != rows or z_all.dtype != np.float32 or z_all.shape != (rows,)
            or p.dtype != np.float32 or p.ndim != 2 or p.shape[1] != t_all.shape[1] or v.dtype != np.float32 or v.shape != p.shape[:1]):
        raise ValueError("row_metrics_reference: pi float32 [rows,A], z float32 [rows], net_policy float32 [m,A], net_value float32 [m]")
    m, A = p.shape
    where = np.arange(m, dtype=np.int64) if index is None else np.asarray(index, dtype=np.int64)
    if where.shape != (m,) or m > ROW_METRICS_MAX_ROWS or (index is None and m > rows):
        raise ValueError("row_metrics_reference: one network row per row of index (or of pi), 2^24 at most")
    inside = (where >= 0) & (where < rows)
    t = np.zeros((m, A), dtype=np.float32)
    zz = np.zeros((m,), dtype=np.float32)
    ply = np.zeros((m,), dtype=np.int64)
    t[inside], zz[inside] = t_all[where[inside]], z_all[where[inside]]
    ply[inside] = s72[where[inside], 68].astype(np.int64) | (s72[where[inside], 69].astype(np.int64) << 8)
    vals, tag = np.zeros((m, 4), dtype=np.float64), np.full((m,), buckets, dtype=np.int32)
    if m == 0:
        return vals, tag
    with np.errstate(all="ignore"):
        bad = (~np.isfinite(t).all(axis=1) | ~np.isfinite(p).all(axis=1) | (t < 0).any(axis=1) | ~np.isfinite(v) | ~np.isfinite(zz))
        positive = t > 0
        ok = inside & ~bad & positive.any(axis=1)
        pc = np.where(p > ROW_METRICS_TINY, p, ROW_METRICS_TINY).astype(np.float64)
        td, pd = t.astype(np.float64), p.astype(np.float64)
        ts = np.where(positive, td, 1.0)
        s_ce = _lane_sums(np.where(positive, ts * np.log(pc), 0.0))
        s_ent = _lane_sums(np.where(positive, ts * np.log(ts), 0.0))
        s_t, s_e, s_tp = _lane_sums(td), _lane_sums(np.exp(pd)), _lane_sums(td * pd)
        lp = s_t * np.log(s_e)
        d = v.astype(np.float64) - zz.astype(np.float64)
        full = np.stack((0.0 - s_ce, 0.0 - s_ent, lp - s_tp, d * d), axis=1)
        first = (p == p.max(axis=1, keepdims=True)).argmax(axis=1)         # the least index that holds the maximum
        hit = t[np.arange(m), first] == t.max(axis=1)
        counted = zz != 0
        agrees = counted & (v.astype(np.float64) * zz.astype(np.float64) > 0)
    bucket = np.minimum(ply // bucket_plies, buckets - 1)
    word = bucket | np.where(hit, TAG_HIT, 0) | np.where(counted, TAG_SIGN_COUNTED, 0) | np.where(agrees, TAG_SIGN_AGREES, 0)
    vals[ok], tag[ok] = full[ok], word[ok].astype(np.int32)
    return vals, tag


def row_metrics_workspace_doubles(m, buckets):
    """aqg_row_metrics_workspace_doubles: ceil(m / 4096) * (buckets + 1) * 8, or 0 for m == 0 or an argument out of range."""
    if not 1 <= m <= ROW_METRICS_MAX_ROWS or not 1 <= buckets <= ROW_METRICS_MAX_BUCKETS:
        return 0
    return -(-m // ROW_METRICS_CHUNK) * (buckets + 1) * 8


def row_metrics_reduce_reference(vals, tag, buckets=16):
    """aqg_row_metrics_reduce in numpy, both launches: (sums float64 [buckets+1,4], counts int64 [buckets+1,4]) -- per bucket the sums
    of vals {ce, ent, lp, se} and the counts {rows, hits, signs counted, signs agreeing}; row `buckets` is the rejected rows'.
    Launch one: for every chunk of 4,096 rows and every bucket, lane l of 256 adds the rows l, l + 256, ... of the chunk in ascending
    order whose tag names the bucket to +0.0; each wavefront's 64 lanes reduce by the xor-shuffle 32, 16, ..., 1; the four wave results
    are added in wave order.  Launch two: per bucket, lane l of 64 adds the chunk partials l, l + 64, ... ascending to +0.0, then the
    same shuffle.  A tag whose bucket field is above `buckets` belongs to no bucket."""
    _, buckets = check_row_metrics_options(1, buckets)
    x, w = np.asarray(vals), np.asarray(tag)
    if x.dtype != np.float64 or x.ndim != 2 or x.shape[1] != 4 or w.dtype != np.int32 or w.shape != x.shape[:1]:
        raise ValueError("row_metrics_reduce_reference: vals must be float64 [m,4] and tag int32 [m]")
    m = x.shape[0]
    if m > ROW_METRICS_MAX_ROWS:
        raise ValueError("row_metrics_reduce_reference: 2^24 rows at most")
    C, L = ROW_METRICS_CHUNK, ROW_METRICS_LANES
    chunks = -(-m // C)
    field = w & 255
    flags = np.stack((np.ones((m,), np.int64), (w >> 8) & 1, (w >> 9) & 1, (w >> 10) & 1), axis=1).astype(np.int64)
    lane64 = np.arange(64)
    partial = np.zeros((chunks, buckets + 1, 4), dtype=np.float64)
    counts = np.zeros((buckets + 1, 4), dtype=np.int64)
    with np.errstate(all="ignore"):
        for c in range(chunks):
            xs = np.zeros((C, 4), dtype=np.float64)
            fs = np.full((C,), -1, dtype=np.int64)
            k = min(C, m - c * C)
            xs[:k], fs[:k] = x[c * C:c * C + k], field[c * C:c * C + k]
            xs, fs = xs.reshape(C // L, L, 4), fs.reshape(C // L, L)
            for b in np.unique(fs[fs >= 0]):
                if b > buckets:
                    continue
                acc = np.zeros((L, 4), dtype=np.float64)
                for r in range(C // L):                         # a row of another bucket adds nothing: the accumulator keeps its bits
                    acc = np.where((fs[r] == b)[:, None], acc + xs[r], acc)
                acc = acc.reshape(L // 64, 64, 4)
                for off in (32, 16, 8, 4, 2, 1):
                    acc = acc + acc[:, lane64 ^ off]
                waves = acc[:, 0]
                partial[c, b] = ((waves[0] + waves[1]) + waves[2]) + waves[3]
        sums = np.zeros((buckets + 1, 4), dtype=np.float64)
        for b in range(buckets + 1):
            padded = np.zeros((-(-max(chunks, 1) // 64) * 64, 4), dtype=np.float64)
            padded[:chunks] = partial[:, b]
            acc = np.zeros((64, 4), dtype=np.float64)
            for r in range(padded.shape[0] // 64):
                acc = acc + padded[r * 64:(r + 1) * 64]
            for off in (32, 16, 8, 4, 2, 1):
                acc = acc + acc[lane64 ^ off]
            sums[b] = acc[0]
            counts[b] = flags[field == b].sum(axis=0)
    return sums, counts


def holdout_reference(keys, seed, share):
    """aqg_replay_holdout_mask in numpy, bit for bit: uint8 [n], 1 where counter_uniform(stream_key(seed, HOLDOUT_STREAM), key) <
    share -- keys int64 [n] from position_keys, read as unsigned.  A position's side depends on (seed, its key bytes) alone."""
    share, seed, _ = check_holdout_options(share, seed)
    k = np.asarray(keys)
    if k.dtype != np.int64 or k.ndim != 1:
        raise ValueError("holdout_reference: keys must be int64 [n]")
    u = counter_uniform(stream_key(seed, HOLDOUT_STREAM), k.view(np.uint64))
    return (np.asarray(u, dtype=np.float64).reshape(k.shape) < share).astype(np.uint8)


def holdout_split_reference(states72, index, share, seed):
    """The split on host arrays: (train_index, holdout_index), both int64 in input order, of the rows index[0..n) (None: all rows)
    of states72 uint8 [rows,72] -- position_keys, holdout_reference and two nonzeros."""
    s = np.asarray(states72)
    rows = np.arange(s.shape[0], dtype=np.int64) if index is None else np.asarray(index, dtype=np.int64)
    mask = holdout_reference(position_keys(s, rows), seed, share).astype(bool)
    return rows[~mask], rows[mask]
