"""Opening books and paired matches: tables of records that games start from (include/aqgnn.h, "start positions").

random_book: `count` positions `plies` random plies behind the opening, played on the device, every row clean by the checker, even in
its ply counter and distinct (also from the mirror images of the rows before it); random_book_reference is the same function in numpy
over the host rules.  from_window: start rows drawn from a ReplayWindow.  fork_table: the table and index of a self-play generation
that forks a share of its games from the window.  save / load: a book as .npz.  pair_report: the statistics of a paired match -- each
opening played twice with the colours exchanged, the error taken over pairs.
"""
import math

import numpy as np
import torch

from . import _lib
from .constants import board_params
from .counter_rng import counter_uniform, stream_key
from .replay_reference import KEY_BYTES

CANDIDATES_PER_ROW = 16        # random_book looks at 16 * count candidates at most


def _check_book_args(board_size, plies, count):
    if board_size not in (3, 5, 7, 9):
        raise ValueError("random_book: board_size must be 3, 5, 7 or 9")
    if isinstance(plies, bool) or int(plies) != plies or plies < 2 or plies % 2:
        raise ValueError(f"random_book: plies must be even and >= 2, not {plies!r} (a start record has an even ply counter)")
    if isinstance(count, bool) or int(count) != count or count < 1:
        raise ValueError(f"random_book: count must be an integer >= 1, not {count!r}")
    return int(plies), int(count)


def book_uniforms(seed, first, n, plies):
    """float64 [n, plies]: the draw of candidate first + i at ply p is counter_uniform(stream_key(seed, first + i), p) -- keyed by
    (seed, candidate, ply) alone, whatever the chunking."""
    keys = stream_key(int(seed), np.arange(first, first + n, dtype=np.uint64))
    return counter_uniform(keys[:, None], np.arange(plies, dtype=np.uint64)[None, :])


def opening_record(board_size):
    """The opening record of a board: both pawns on the middle of their back rows, every wall in hand, ply 0."""
    from .game_logic import pack_state72
    N, walls = int(board_size), board_params(board_size)[0]
    start = N * (N - 1) + N // 2
    return pack_state72([start, walls], [start, walls], [], 0, N)


class _Picker:
    """The book's rows among the candidates, in candidate order: a candidate is taken when it is alive (its walk met no ended
    position), clean by the checker, and its key bytes are those of no row taken before -- nor, with drop_mirrors, of the mirror image
    of one."""

    def __init__(self, count, drop_mirrors):
        self.count, self.drop_mirrors = count, drop_mirrors
        self.rows, self.seen = [], set()

    def offer(self, recs, mirrors, ok):
        for i in np.flatnonzero(ok):
            if len(self.rows) == self.count:
                break
            key = recs[i, KEY_BYTES].tobytes()
            if key in self.seen:
                continue
            self.rows.append(recs[i].copy())
            self.seen.add(key)
            if self.drop_mirrors:
                self.seen.add(mirrors[i, KEY_BYTES].tobytes())
        return len(self.rows) == self.count

    def book(self, what, looked_at):
        if len(self.rows) < self.count:
            raise ValueError(f"{what}: only {len(self.rows)} of {self.count} distinct clean positions among {looked_at} candidates")
        return np.stack(self.rows)


def random_book(board_size, plies, count, seed, drop_mirrors=True, device=None):
    """uint8 [count, 72] device tensor: the first `count` candidates, in candidate order, that can start a game and are distinct.
    Candidate i plays `plies` (even, >= 2) uniformly random legal plies from the opening -- index min(cnt - 1, floor(u * cnt)) into
    legal_actions(), u = book_uniforms' draw of (seed, i, ply) -- through aqg_agent_random, aqg_state_next and aqg_state_status; a
    candidate whose walk meets an ended position is dropped.  Distinct: by the merge's key bytes (0..67 and 70), and with drop_mirrors
    also from the game_logic.mirror_batch image of every row taken before.  Candidates come in chunks, 16 * count at most; ValueError
    when they hold fewer than `count` rows -- a short book is never returned."""
    from .game_logic import check_states_batch, mirror_batch, next_batch, status_batch
    plies, count = _check_book_args(board_size, plies, count)
    dev = _lib.require_gpu(device)
    lib = _lib.load()
    draw = board_params(board_size)[1]
    opening = torch.from_numpy(opening_record(board_size)).to(dev)
    pick = _Picker(count, drop_mirrors)
    limit, first = CANDIDATES_PER_ROW * count, 0
    chunk = min(limit, max(2 * count, 1024))
    while first < limit:
        n = min(chunk, limit - first)
        u = torch.from_numpy(book_uniforms(seed, first, n, plies)).to(dev)
        recs = opening.unsqueeze(0).repeat(n, 1).contiguous()
        alive = torch.ones((n,), dtype=torch.bool, device=dev)
        actions = torch.empty((n,), dtype=torch.int32, device=dev)
        for p in range(plies):
            up = u[:, p].contiguous()
            _lib.check(lib.aqg_agent_random(board_size, _lib.ptr(recs), n, _lib.ptr(up), 1, 0, _lib.ptr(actions), _lib.stream_ptr(dev)),
                       "aqg_agent_random")
            alive &= actions >= 0
            recs = next_batch(recs, actions.clamp(min=0), board_size)
            alive &= status_batch(recs, board_size, draw) == 0
        ok = alive & (check_states_batch(recs, board_size) == 0)
        mirrors = mirror_batch(recs, board_size) if drop_mirrors else recs
        first += n
        if pick.offer(recs.cpu().numpy(), mirrors.cpu().numpy(), ok.cpu().numpy()):
            break
    return torch.from_numpy(pick.book("random_book", first)).to(dev)


def random_book_reference(board_size, plies, count, seed, drop_mirrors=True):
    """random_book in numpy over the host rules (aqg_host_legal_actions, aqg_host_next, aqg_host_check_state, mirror_record): uint8
    [count, 72], bit for bit the device's book."""
    import ctypes
    from .game_logic import check_state_host, mirror_record
    plies, count = _check_book_args(board_size, plies, count)
    lib = _lib.load()
    N, draw = int(board_size), board_params(board_size)[1]
    opening = opening_record(N)
    pick = _Picker(count, drop_mirrors)
    limit, first = CANDIDATES_PER_ROW * count, 0
    legal, nxt = np.empty(_lib.MAX_LEGAL, dtype=np.uint8), np.empty(72, dtype=np.uint8)
    while first < limit:
        n = min(max(2 * count, 256), limit - first)
        u = book_uniforms(seed, first, n, plies)
        recs, ok = np.empty((n, 72), dtype=np.uint8), np.zeros(n, dtype=bool)
        for i in range(n):
            rec, alive = opening.copy(), True
            for p in range(plies):
                cnt = lib.aqg_host_legal_actions(N, rec.ctypes.data_as(ctypes.c_void_p), legal.ctypes.data_as(ctypes.c_void_p))
                if cnt <= 0:
                    alive = False
                    break
                action = int(legal[min(cnt - 1, int(math.floor(u[i, p] * cnt)))])
                lib.aqg_host_next(N, rec.ctypes.data_as(ctypes.c_void_p), action, nxt.ctypes.data_as(ctypes.c_void_p))
                rec = nxt.copy()
                if int(rec[2]) // N == 0 or (int(rec[68]) | (int(rec[69]) << 8)) >= draw:      # is_lose / is_draw
                    alive = False
                    break
            recs[i] = rec
            ok[i] = alive and check_state_host(rec, N) == 0
        first += n
        if pick.offer(recs, mirror_record(recs) if drop_mirrors else recs, ok):
            break
    return pick.book("random_book_reference", first)


def _host_flags(recs, board_size, device):
    """The checker's flags of uint8 [n,72] host records: on `device` when it is a GPU, else by the host build of the same predicate."""
    from .game_logic import check_state_host, check_states_batch
    if recs.shape[0] == 0:
        return np.zeros((0,), dtype=np.uint8)
    if torch.device(device).type != "cpu":
        return check_states_batch(torch.from_numpy(recs).to(device), board_size).cpu().numpy()
    return np.asarray([check_state_host(r, board_size) for r in recs], dtype=np.uint8)


def from_window(window, count, seed, update=0, return_slots=False):
    """At most `count` start rows from a replay.ReplayWindow: uint8 [n, 72] numpy, n <= count -- this one may return fewer, and its
    length says how many.  Of the window's valid rows those with an even ply counter that the checker passes, in ascending order of the
    key counter_uniform(stream_key(seed, update), ring slot) (as replay.draw_reanalyse_rows keys its rows), a position (the merge's
    key bytes) taken once.  return_slots: also the rows' ring slots, int64 [n]."""
    count = int(count)
    if count < 0:
        raise ValueError("from_window: count must be >= 0")
    slots = window.index().cpu().numpy().astype(np.int64)
    if slots.size == 0 or count == 0:
        empty = np.zeros((0, 72), dtype=np.uint8)
        return (empty, np.zeros((0,), dtype=np.int64)) if return_slots else empty
    recs = window.tensors()[0].index_select(0, window.index()).cpu().numpy()
    plies = recs[:, 68].astype(np.int64) | (recs[:, 69].astype(np.int64) << 8)
    ok = (plies % 2 == 0) & (_host_flags(recs, window.board_size, window.device) == 0)
    keys = np.asarray(counter_uniform(stream_key(int(seed), int(update)), slots.astype(np.uint64)), dtype=np.float64)
    rows, taken, seen = [], [], set()
    for i in np.argsort(keys, kind="stable"):
        if len(rows) == count:
            break
        if not ok[i]:
            continue
        key = recs[i, KEY_BYTES].tobytes()
        if key not in seen:
            seen.add(key)
            rows.append(recs[i])
            taken.append(slots[i])
    rows = np.stack(rows) if rows else np.zeros((0, 72), dtype=np.uint8)
    return (rows, np.asarray(taken, dtype=np.int64)) if return_slots else rows


def check_window_share(share):
    """The share of a generation's games that fork from the window: a float in [0, 1] (ValueError otherwise; NaN fails)."""
    if isinstance(share, bool) or not isinstance(share, (int, float)) or not 0.0 <= float(share) <= 1.0:
        raise ValueError(f"the share of games started from the window must be in [0, 1], not {share!r}")
    return float(share)


def fork_draws(seed, generation, games, share, rows):
    """int32 [games]: the table row of every game of a forked generation, 0 = the opening record, r >= 1 = window row r - 1 of `rows`
    drawn rows.  Game j -- its index over ALL ranks -- forks iff counter_uniform(key_j, 0) < share and then takes row
    1 + min(rows - 1, floor(counter_uniform(key_j, 1) * rows)), key_j = stream_key(stream_key(seed, generation), j): a function of
    (seed, generation, game index) alone, never of rank count or slots."""
    keys = stream_key(stream_key(int(seed), int(generation)), np.arange(int(games), dtype=np.uint64))
    if rows <= 0 or share <= 0.0:
        return np.zeros((int(games),), dtype=np.int32)
    fork = np.asarray(counter_uniform(keys, 0), dtype=np.float64) < share
    pick = np.minimum(rows - 1, np.floor(np.asarray(counter_uniform(keys, 1), dtype=np.float64) * rows).astype(np.int64))
    return np.where(fork, 1 + pick, 0).astype(np.int32)


def fork_table(window, games, share, seed, generation):
    """The start table of one self-play generation that forks from `window`: (rows uint8 [1 + n, 72], index int32 [games]) -- row 0 the
    opening record, rows 1.. from_window(window, games, seed, generation), index by fork_draws -- or None when the share is 0 or the
    window holds no usable row (no table is built).  Every rank computes the same table from its own copy of the window."""
    share = check_window_share(share)
    if share <= 0.0 or window is None or len(window) == 0:
        return None
    rows = from_window(window, games, seed, generation)
    if rows.shape[0] == 0:
        return None
    table = np.concatenate([opening_record(window.board_size)[None, :], rows], 0)
    return table, fork_draws(seed, generation, games, share, rows.shape[0])


def save(path, book, board_size=None):
    """A book as .npz (no pickle): `states72` uint8 [S, 72] and `board_size`."""
    rows = book.cpu().numpy() if isinstance(book, torch.Tensor) else np.asarray(book)
    if rows.dtype != np.uint8 or rows.ndim != 2 or rows.shape[1] != 72:
        raise ValueError("save: a book is a uint8 [S, 72] tensor or array")
    N = int(rows[0, 70]) if board_size is None and rows.shape[0] else int(board_size or 0)
    with open(path, "wb") as f:
        np.savez(f, states72=rows, board_size=np.int32(N))


def load(path):
    """(uint8 [S, 72] numpy array, board_size) of a book written by save; read with allow_pickle=False."""
    with np.load(path, allow_pickle=False) as z:
        rows, N = np.ascontiguousarray(z["states72"], dtype=np.uint8), int(z["board_size"])
    if rows.ndim != 2 or rows.shape[1] != 72:
        raise ValueError(f"{path}: states72 is not a [S, 72] array")
    return rows, N


def pair_report(points):
    """The statistics of a paired match, all float64.  points: side 0's points of an even number of games, games 2j and 2j + 1 the two
    games of opening j with the colours exchanged.  d_j = (points[2j] + points[2j+1]) / 2;
      pairs, mean = mean(d), se = std(d, ddof=1) / sqrt(pairs) (NaN for a single pair: one pair has no error estimate, and elo_se
      and los are NaN with it),
      elo = -400 log10(1 / mean - 1) (-inf at 0, +inf at 1), elo_se = se * 400 / (ln 10 * mean * (1 - mean)) (inf at 0 and 1 unless
      se is 0, then 0), los = Phi((mean - 0.5) / se), the likelihood of superiority (1, 0.5 or 0 when se == 0)."""
    p = np.asarray(points, dtype=np.float64).reshape(-1)
    if p.size == 0 or p.size % 2:
        raise ValueError(f"pair_report: a paired match has an even number of games (>= 2), not {p.size}")
    d = (p[0::2] + p[1::2]) / 2.0
    pairs = int(d.size)
    mean = float(d.mean())
    se = float(d.std(ddof=1) / math.sqrt(pairs)) if pairs > 1 else math.nan
    if mean <= 0.0:
        elo = -math.inf
    elif mean >= 1.0:
        elo = math.inf
    else:
        elo = -400.0 * math.log10(1.0 / mean - 1.0) + 0.0
    if math.isnan(se):
        elo_se = los = math.nan
    elif se == 0.0:
        elo_se = 0.0
        los = 1.0 if mean > 0.5 else 0.0 if mean < 0.5 else 0.5
    else:
        elo_se = se * 400.0 / (math.log(10.0) * mean * (1.0 - mean)) if 0.0 < mean < 1.0 else math.inf
        los = 0.5 * (1.0 + math.erf((mean - 0.5) / se / math.sqrt(2.0)))
    return dict(pairs=pairs, mean=mean, se=se, elo=elo, elo_se=elo_se, los=los)
