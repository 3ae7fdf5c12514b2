"""Batched self-play engine: thousands of concurrent PV-MCTS games per MI355X, lock-step simulations.

Host side of aqg_engine_* (include/aqgnn.h).  All state lives in HBM as torch tensors owned by this object;
every simulation of every game is enqueued by one C call per move (no per-simulation Python, no host sync
inside a move).  Per-game semantics equal the reference's sequential `pv_mcts_policy` + `play()`
(pv_mcts.py:20-95, self_play.py:40-68); see csrc/mcts.hip (the map of mcts_step.hip, mcts_move.hip, mcts_tree.hpp).

Sharding: games are independent, so rank r of W simply owns its own BatchedSelfPlay with its own
uniform stream; `gather_history` is the single exchange step per generation (all-gather over RCCL/xGMI).
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib
from .constants import BOARD_SIZE, board_params
from .evaluators import BINDINGS


ROOT_NOISE_ATTEMPTS = 64      # cap of the gamma sampler's rejection loop (csrc/mcts_move.hip ROOT_NOISE_ATTEMPTS)
_MASK64 = (1 << 64) - 1


def default_root_noise_alpha(board_size):
    """The usual "10 / typical number of legal moves" rule, with the board's action count N^2 + 2 (N - 1)^2 for the moves."""
    return 10.0 / (board_size ** 2 + 2 * (board_size - 1) ** 2)


def check_root_noise(eps, alpha):
    """Validate the root-noise options as the library does, on the f32 values its struct holds: eps in [0, 1); alpha in (0, 100]
    when eps > 0.  Returns them as floats (alpha 0.0 when the noise is off)."""
    eps = float(np.float32(eps))
    if not 0.0 <= eps < 1.0:
        raise ValueError(f"root_noise_eps must be in [0, 1) as a float32, not {eps}")
    if eps == 0.0:
        return 0.0, 0.0
    alpha = float(np.float32(alpha))
    if not 0.0 < alpha <= 100.0:
        raise ValueError(f"root_noise_alpha must be in (0, 100] as a float32, not {alpha}")
    return eps, alpha


def refuse_root_noise(what, **options):
    """Evaluation paths never add noise: an option that asks for it is a mistake, not something to drop silently."""
    bad = sorted(k for k, v in options.items() if v is not None)
    if bad:
        raise ValueError(f"{what} never adds root exploration noise: {', '.join(bad)} is a self-play option")


def check_target_options(temperature_plies, record_search_value=False, record_history=True):
    """Validate the self-play target options (include/aqgnn.h, "self-play targets"): temperature_plies an integer >= 0 (0 = off);
    record_search_value needs the history it is a column of.  Returns (temperature_plies, record_search_value)."""
    if isinstance(temperature_plies, bool) or int(temperature_plies) != temperature_plies or not 0 <= int(temperature_plies) < 2 ** 31:
        raise ValueError(f"temperature_plies must be an integer >= 0, not {temperature_plies!r}")
    if record_search_value and not record_history:
        raise ValueError("record_search_value needs record_history: the search value is a column of the history")
    return int(temperature_plies), bool(record_search_value)


def check_tree_reuse(tree_reuse, tree_reuse_visits, sims, evaluator="gnn"):
    """Validate the tree-reuse options as the library does (include/aqgnn.h, "tree reuse").  Returns keep_visits, or None when the
    option is off.  tree_reuse_visits None = `sims`; 0 is legal: on, never keeps."""
    if not tree_reuse:
        if tree_reuse_visits is not None:
            raise ValueError("tree_reuse_visits needs tree_reuse=True")
        return None
    if evaluator == "external":
        raise ValueError("tree_reuse is not offered with evaluator='external': its host loop has no keep step")
    keep = sims if tree_reuse_visits is None else tree_reuse_visits
    if isinstance(keep, bool) or int(keep) != keep or int(keep) < 0:
        raise ValueError(f"tree_reuse_visits must be an integer >= 0, not {tree_reuse_visits!r}")
    keep = int(keep)
    if keep + int(sims) > 32767:
        raise ValueError("tree_reuse_visits + sims must be <= 32767: the visit row is read out as int16")
    if 1 + (keep + int(sims)) * _lib.MAX_LEGAL >= 1 << 24:
        raise ValueError("tree_reuse_visits + sims is too large: the tree pool must stay below 2**24 records")
    return keep


def refuse_tree_reuse(what, **options):
    """Matches and evaluation paths search from a fresh tree every move (two alternating searchers would need a two-ply descent
    into per-model trees): an option that asks for tree reuse is a mistake, not something to drop silently."""
    bad = sorted(k for k, v in options.items() if v is not None)
    if bad:
        raise ValueError(f"{what} never keeps a subtree between moves: {', '.join(bad)} is a self-play option")


def check_resign(resign_threshold, resign_min_ply=0, resign_disable_fraction=0.1, record_history=True):
    """Validate the resignation options as the library does (include/aqgnn.h, "resignation"), on the values its struct holds.
    Returns (threshold, min_ply, disable_fraction), or None when the option is off (resign_threshold None).  A threshold of 1.0 is
    legal: on, never resigns -- the statistics are still kept."""
    if resign_threshold is None:
        return None
    if isinstance(resign_threshold, (bool, str)):
        raise ValueError(f"resign_threshold must be a number in (0, 1], not {resign_threshold!r}")
    thr = float(np.float32(resign_threshold))
    if not 0.0 < thr <= 1.0:
        raise ValueError(f"resign_threshold must be in (0, 1] as a float32, not {resign_threshold!r}")
    if isinstance(resign_min_ply, bool) or int(resign_min_ply) != resign_min_ply or not 0 <= int(resign_min_ply) < 2 ** 31:
        raise ValueError(f"resign_min_ply must be an integer >= 0, not {resign_min_ply!r}")
    frac = float(resign_disable_fraction)
    if not 0.0 <= frac <= 1.0:
        raise ValueError(f"resign_disable_fraction must be in [0, 1], not {resign_disable_fraction!r}")
    if not record_history:
        raise ValueError("resignation needs record_history: a resigned game ends in a history row")
    return thr, int(resign_min_ply), frac


def refuse_resign(what, **options):
    """Matches, evaluation paths and moves the engine does not search play every game to its rule end: an option that asks for
    resignation is a mistake, not something to drop silently."""
    bad = sorted(k for k, v in options.items() if v is not None)
    if bad:
        raise ValueError(f"{what} never resigns a game: {', '.join(bad)} is a self-play option")


def default_resign_seed(seed):
    """The resignation seed of an engine that was given none: `seed` through the mixer (see default_root_noise_seed)."""
    return _mix64_int((int(seed) & _MASK64) ^ 0x52455349474E4544)


def draw_resign_enabled(seed, k, disable_fraction=0.1):
    """Whether game k may resign under the resignation seed `seed`: counter_uniform(stream_key(seed, k), 0) >= disable_fraction --
    the draw of engine_finish_move_kernel in numpy (include/aqgnn.h, "resignation").  k may be an array of game indices."""
    from .agents import _mix64
    G = np.uint64(_GOLDEN)
    kk = np.asarray(k, dtype=np.int64).astype(np.uint64)
    with np.errstate(over="ignore"):
        key = _mix64(np.uint64(int(seed) & _MASK64) + G * (kk + np.uint64(1)))
        z = _mix64(key + G)
    u = (z >> np.uint64(11)).astype(np.float64) * (2.0 ** -53)
    out = u >= float(disable_fraction)
    return bool(out) if np.ndim(k) == 0 else out


def _side_loses(game_result):
    """bool [K, 2]: side s of game k (s = ply parity: 0 the first player) lost."""
    z = np.asarray(game_result).astype(np.int64).reshape(-1)
    return np.stack([z < 0, z > 0], axis=1)


def resign_false_positives(resign_min, game_result, enabled, threshold):
    """The calibration count over the DISABLED games (they were played to their rule end): (would_resign, false_positives,
    eligible_sides) = the sides whose running minimum is below -threshold (f32), how many of those did not lose, and the number of
    sides that did not lose.  resign_min [K, 2] f32, game_result [K] the first player's value, enabled [K] bool."""
    lo = np.asarray(resign_min, dtype=np.float32).reshape(-1, 2)
    off = ~np.asarray(enabled, dtype=bool).reshape(-1)
    would = (lo < -np.float32(threshold)) & off[:, None]
    fine = ~_side_loses(game_result) & off[:, None]
    return int(would.sum()), int((would & fine).sum()), int(fine.sum())


def suggest_resign_threshold(resign_min, game_result, enabled, max_false_positive, min_sides=None, min_threshold=0.05):
    """The threshold that resigns the most while the false-positive rate of resign_false_positives -- of the played-out (disabled)
    games' sides that would have resigned, the share that did not lose -- stays at or under `max_false_positive`.  The cut is
    m < -T, so the candidates are T = -x for every distinct minimum x of those sides in [-1, -min_threshold), and T = min_threshold
    itself: at T = -x exactly the sides with a minimum below x would have resigned (ties fall on one side of the cut together).  The
    rate need not fall steadily as T grows, so every candidate is counted and the smallest T that qualifies wins -- the largest cut
    value -T.  A candidate qualifies only if at least `min_sides` sides would have resigned at it (default max(20, ceil(1 / bound)):
    with fewer than 1 / bound of them one false positive already exceeds the bound).  None when no candidate qualifies: too few sides
    to say, or the network's lost-looking games are not lost (a network whose games end in draws never resigns)."""
    bound = float(max_false_positive)
    if not 0.0 <= bound < 1.0:
        raise ValueError(f"max_false_positive must be in [0, 1), not {max_false_positive!r}")
    floor = np.float32(min_threshold)
    if not 0.0 < float(floor) <= 1.0:
        raise ValueError(f"min_threshold must be in (0, 1], not {min_threshold!r}")
    lo = np.asarray(resign_min, dtype=np.float32).reshape(-1, 2)
    off = ~np.asarray(enabled, dtype=bool).reshape(-1)
    every = np.sort(lo[np.broadcast_to(off[:, None], lo.shape)])
    fine = np.sort(lo[~_side_loses(game_result) & off[:, None]])
    if min_sides is None:
        min_sides = max(20, int(np.ceil(1.0 / bound))) if bound > 0.0 else 20
    cuts = np.unique(np.concatenate([every[every < -floor], np.asarray([-floor], dtype=np.float32)]))
    would = np.searchsorted(every, cuts, side="left")              # sides with a minimum strictly below the cut
    wrong = np.searchsorted(fine, cuts, side="left")
    ok = (would >= max(1, int(min_sides))) & (wrong <= bound * would + 1e-9)
    if not ok.any():
        return None
    return float(np.float32(-cuts[np.flatnonzero(ok)[-1]]))


NODE_DTYPE = np.dtype([("w", "<f8"), ("p", "<f4"), ("action", "<u4"), ("n", "<i4"), ("kids", "<u4"), ("q", "<f4"), ("cp", "<f4")])
assert NODE_DTYPE.itemsize == 32      # csrc/mcts_tree.hpp NodeRec


def keep_subtree_reference(pool_records, node_count, child_index, keep_visits):
    """The keep launch (csrc/mcts_reuse.hip) for one slot, in numpy.  pool_records: the slot's pool, NODE_DTYPE [cap] (or anything
    of 32 bytes per record, e.g. float64 [cap, 4]); node_count: its used records; child_index: index of the chosen child in the root's
    child block, < 0 = do not keep.  Returns (records, count, kept): kept is True iff the index names a child that is expanded with
    n <= keep_visits; then records[:count] is the child's subtree re-rooted -- the child at 0 with a fresh root's action / p / cp, every
    kept child block behind it in ascending order of its old first index, child ranges renamed -- and records[count:] is unspecified
    (here: the input's).  Not kept: the input's records and count."""
    src = np.ascontiguousarray(pool_records).view(NODE_DTYPE).reshape(-1)
    out = src.copy()
    count = min(int(node_count), src.shape[0])
    idx = int(child_index)
    if idx < 0 or count <= 1:
        return out, int(node_count), False
    rcnt, rfirst = int(src["kids"][0]) >> 24, int(src["kids"][0]) & 0xFFFFFF
    if idx >= rcnt or rfirst < 1 or rfirst + rcnt > count:
        return out, int(node_count), False
    c = src[rfirst + idx]
    ccnt, cfirst = int(c["kids"]) >> 24, int(c["kids"]) & 0xFFFFFF
    if ccnt == 0 or int(c["n"]) > int(keep_visits) or cfirst < rfirst + rcnt or cfirst + ccnt > count:
        return out, int(node_count), False
    keep = np.zeros(count, dtype=bool)
    keep[cfirst:cfirst + ccnt] = True
    kids = src["kids"][:count].astype(np.int64)
    for i in range(cfirst, count):            # a node's child block lies behind the node: one ascending pass decides every record
        if keep[i] and kids[i] >> 24:
            first, cnt = int(kids[i] & 0xFFFFFF), int(kids[i] >> 24)
            assert first > i, "a child block lies behind its parent"
            keep[first:min(first + cnt, count)] = True
    new_index = np.cumsum(keep)               # 1-based among the kept records == the new index (0 is the new root)
    old = np.nonzero(keep)[0]
    moved = src[old].copy()
    exp = (moved["kids"] >> 24) != 0
    firsts = (moved["kids"][exp] & 0xFFFFFF).astype(np.int64)
    moved["kids"][exp] = (new_index[firsts].astype(np.uint32) & 0xFFFFFF) | (moved["kids"][exp] & np.uint32(0xFF000000))
    total = 1 + old.shape[0]
    out[1:total] = moved
    root = np.zeros((), dtype=NODE_DTYPE)
    root["w"], root["n"], root["q"] = c["w"], c["n"], c["q"]
    root["action"], root["kids"] = 0xFF, 1 | (ccnt << 24)
    out[0] = root
    return out, total, True


def _mix64_int(z):
    """The splitmix64 finaliser on a Python int (include/aqgnn.h)."""
    z &= _MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK64
    return z ^ (z >> 31)


_GOLDEN = 0x9E3779B97F4A7C15


def default_root_noise_seed(seed):
    """The noise seed of an engine that was given none: `seed` through the mixer.  NOT a linear map: the generator's stream of game
    k is keyed by mix(noise_seed + GOLDEN * (k + 1)), so noise seeds that differ by a multiple of GOLDEN -- what any affine map of
    consecutive engine seeds onto them risks -- would hand game k of one engine the stream of another game of the next."""
    return _mix64_int((int(seed) & _MASK64) ^ 0x524F4F544E4F4953)


def set_noise_seeds(seed, root_noise_seed, sizes, quotas):
    """The noise seeds of MultiSetSelfPlay's sets (slots `sizes`, games `quotas`).  The sets' games are numbered through -- set i's
    game k is game first_i + k of the whole engine -- and the numbering rides in the seed: the stream of game k under
    base + GOLDEN * first is the stream of game first + k under base.  Every set has a seed of its own and no two games share one."""
    base = default_root_noise_seed(seed) if root_noise_seed is None else int(root_noise_seed) & _MASK64
    firsts = [sum(max(q, g) for q, g in zip(quotas[:i], sizes[:i])) for i in range(len(sizes))]
    return [(base + _GOLDEN * f) & _MASK64 for f in firsts]


def root_noise_stream_key(seed, k, ply):
    """The 64-bit key of the noise stream of game k's root at `ply` under the noise seed `seed` (include/aqgnn.h: K(K(seed, k), ply))."""
    return _mix64_int(_mix64_int(int(seed) + _GOLDEN * (int(k) + 1)) + _GOLDEN * (int(ply) + 1))


def draw_root_noise(seed, k, ply, count, alpha, return_exhausted=False):
    """The gamma variates g_0 .. g_{count-1} of the root of game k at ply `ply`, float64 [count] -- the generator of
    engine_root_noise_kernel in numpy (the recipe is in include/aqgnn.h, "root exploration noise").  k may be an array of game
    indices: the result is then [len(k), count].  Component i draws from its own sub-stream, so the first c components do not
    depend on count.  return_exhausted: also return how many variates took the fallback of the capped rejection loop."""
    from .agents import _mix64, _GOLDEN
    G = np.uint64(_GOLDEN)

    def key_of(base, b):
        with np.errstate(over="ignore"):
            return _mix64(base + G * (np.asarray(b, dtype=np.uint64) + np.uint64(1)))

    def uniform(key, j):
        with np.errstate(over="ignore"):
            z = _mix64(key + G * np.uint64(j + 1))
        return (z >> np.uint64(11)).astype(np.float64) * (2.0 ** -53)

    scalar = np.ndim(k) == 0
    kk = np.atleast_1d(np.asarray(k, dtype=np.int64)).astype(np.uint64)
    root = np.asarray([root_noise_stream_key(seed, int(x), ply) for x in kk], dtype=np.uint64)
    key = key_of(root[:, None], np.arange(int(count), dtype=np.uint64)[None, :])
    alpha = float(np.float32(alpha))          # the struct field is f32
    boost = alpha < 1.0
    a = alpha + 1.0 if boost else alpha
    d = a - 1.0 / 3.0
    c = 1.0 / np.sqrt(9.0 * d)
    val = np.full(key.shape, d, dtype=np.float64)
    todo = np.ones(key.shape, dtype=bool)
    for t in range(ROOT_NOISE_ATTEMPTS):
        if not todo.any():
            break
        kt = key[todo]
        u1, u2, u3 = uniform(kt, 1 + 3 * t), uniform(kt, 2 + 3 * t), uniform(kt, 3 + 3 * t)
        x = np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos(2.0 * np.pi * u2)
        v1 = 1.0 + c * x
        ok = v1 > 0.0
        v = np.where(ok, v1 * v1 * v1, 1.0)
        ok &= np.log(1.0 - u3) < 0.5 * x * x + d - d * v + d * np.log(v)
        idx = np.flatnonzero(todo.ravel())
        val.ravel()[idx[ok]] = d * v[ok]
        todo.ravel()[idx[ok]] = False
    exhausted = int(todo.sum())
    if boost:
        val = val * np.power(1.0 - uniform(key, 0), 1.0 / alpha)
    val = np.maximum(val, np.finfo(np.float64).tiny)
    if scalar:
        val = val[0]
    return (val, exhausted) if return_exhausted else val


def resign_stats_of(parts, threshold):
    """resign_stats over the (resign_min, game_result, enabled, game_resigned, game_plies, game_done) tuples of one or more engines."""
    lo, res, enabled, flag, plies, done = (np.concatenate([np.asarray(p[i]) for p in parts], 0) for i in range(6))
    fin = done != 0
    would, wrong, fine = resign_false_positives(lo[fin], res[fin], enabled[fin], threshold)
    return dict(games=int(fin.sum()), games_resigned=int(flag[fin].astype(bool).sum()), plies=int(plies[fin].sum()),
                disabled_games=int((~enabled[fin]).sum()), would_resign=would, false_positives=wrong,
                false_positive_rate=wrong / would if would else 0.0, eligible_sides=fine)


def suggest_from_arrays(parts, max_false_positive, **kw):
    lo, res, enabled, _, _, done = (np.concatenate([np.asarray(p[i]) for p in parts], 0) for i in range(6))
    fin = done != 0
    return suggest_resign_threshold(lo[fin], res[fin], enabled[fin], max_false_positive, **kw)


class BatchedSelfPlay:
    def __init__(self, model=None, num_games=2048, sims=50, board_size=BOARD_SIZE, device=None, temperature=1.0,
                 c_puct=1.25, evaluator="gnn", fake_bias=0, seed=0, record_history=True, quota=None, eval_cache_slots=None,
                 root_noise_eps=0.0, root_noise_alpha=None, root_noise_seed=None, temperature_plies=0, record_search_value=False,
                 tree_reuse=False, tree_reuse_visits=None, resign_threshold=None, resign_min_ply=0, resign_disable_fraction=0.1,
                 resign_seed=None):
        """model: GraphPolicyValueNetwork/GNNNetwork (evaluator='gnn'); evaluator='fake' runs the integer-hash
        evaluator used by the parity tests (oracle/mcts.py FakeModel); evaluator='external' calls `model.predict(state,
        device)` -- ANY object honouring the reference's BaseNetwork contract (BaseNetwork.py:36-40), e.g. a stock CNN --
        once per simulation and game from the host, exactly like pv_mcts.py:47 (plumbing path: one host round trip per
        simulation).  evaluator='cnn' runs the reference's residual CNNNetwork (pv_network_cnn.py) on the library's own kernels
        (prior_mode 4, aqg_cnn_forward_boards).  evaluator='general' runs a GraphPolicyValueNetwork of ANY shape (6 input features) on the library's own
        kernels (prior_mode 3, aqg_gcn_forward_boards_general): the per-move cost of 'gnn', no host work per simulation.
        eval_cache_slots (evaluator='gnn', 'general' or 'cnn'; a power of two >= 64, 0 = off; None = the environment's AQG_EVAL_CACHE_SLOTS, else
        off): entries per game slot of the evaluation cache
        (include/aqgnn.h, `eval_cache_keys`): a leaf whose position this slot has already sent through the network is expanded from
        the stored priors / value / legal list -- bit-identical searches and game records, fewer network evaluations (736 bytes of
        HBM per entry).
        root_noise_eps (0 = off, the default: nothing changes): every move mixes Dir(root_noise_alpha) into the root's priors on the
        device, p' = (1 - eps) p + eps eta (include/aqgnn.h, "root exploration noise").  root_noise_alpha None = 10 / (N^2 + 2 (N - 1)^2),
        the usual "10 / typical number of moves" rule; root_noise_seed None = derived from `seed`.  The noise of a game's root is
        keyed by (seed, game index, ply) -- draw_root_noise is the generator in numpy -- unless move() / search() are given a table.
        temperature_plies K (0 = off, the default): a root at ply < K is sampled at `temperature` as always, one at ply >= K takes
        the first maximum of the visit counts; the recorded visit rows do not change, only the choice.  record_search_value (needs
        record_history): every searched move also records the root's search value w / n from the mover's side, float32, beside its
        history row -- history_values().  With both off move() makes the calls it always made.
        tree_reuse (off by default: nothing changes; include/aqgnn.h, "tree reuse"): the next move's search starts from the subtree
        of the child this move chose -- when the game goes on, the child is expanded and holds at most tree_reuse_visits visits
        (None = `sims`; 0 = on, never keeps) -- and runs the same `sims` simulations on top.  The recorded visit rows and search
        values include the kept visits.  The tree pool and the path are sized for tree_reuse_visits + sims.  Not with
        evaluator='external', and search() refuses it; tree_reuse_stats() counts the kept moves.
        resign_threshold T (None = off, the default: move() makes the calls it makes today; include/aqgnn.h, "resignation"): after a
        searched move at ply >= resign_min_ply the mover resigns when max(root value, most visited child's q) < -T; the game ends
        there with the mover as loser, its last row's action 0xFF.  A share resign_disable_fraction of the games -- drawn per GAME
        index from resign_seed (None = derived from `seed`), draw_resign_enabled -- never resigns, and every game keeps the running
        minimum of that maximum per side, so resign_stats() can count false positives and suggest_resign_threshold() can pick T.
        T = 1.0 never resigns and only collects.  apply_actions() and search() refuse the option."""
        self.resign_options = check_resign(resign_threshold, resign_min_ply, resign_disable_fraction, record_history)
        self.resign_seed = default_resign_seed(seed) if resign_seed is None else int(resign_seed) & _MASK64
        self.keep_visits = check_tree_reuse(tree_reuse, tree_reuse_visits, sims, evaluator)
        self.tree_reuse = self.keep_visits is not None
        self.temperature_plies, self.record_search_value = check_target_options(temperature_plies, record_search_value, record_history)
        self.root_noise_eps, self.root_noise_alpha = check_root_noise(
            root_noise_eps, default_root_noise_alpha(board_size) if root_noise_alpha is None else root_noise_alpha)
        self.root_noise_seed = default_root_noise_seed(seed) if root_noise_seed is None else int(root_noise_seed) & _MASK64
        b = self.binding = BINDINGS[evaluator]
        b.check(model)          # before anything is allocated or launched
        self.dev = _lib.require_gpu(device)
        self.lib = _lib.load()
        self.N = board_size
        self.A = board_size ** 2 + 2 * (board_size - 1) ** 2
        self.num_walls, self.plies_for_draw = board_params(board_size)
        self.G, self.sims = int(num_games), int(sims)
        # quota > G: the slots are refilled -- a slot whose game has ended takes the next game not yet handed out (in slot
        # order, deterministic) until `quota` games have been started: the reference's loop over games (self_play.py:81-84)
        # on G concurrent slots instead of lock-step generations that idle every finished slot until the longest game ends
        self.quota = self.G if quota is None else int(quota)
        if self.quota < self.G:
            raise ValueError("quota must be >= num_games")
        depth = self.sims + (self.keep_visits or 0)                # visits a tree can hold: its expanded nodes and its depth
        self.node_cap = 1 + depth * _lib.MAX_LEGAL
        self.max_plies = self.plies_for_draw
        self.model = model
        self.evaluator = evaluator
        self.gen = torch.Generator(device=self.dev)
        self.gen.manual_seed(int(seed))
        G, cap, dev, Q = self.G, self.node_cap, self.dev, self.quota

        def z(shape, dtype):
            return torch.zeros(shape, dtype=dtype, device=dev)

        t = self.t = {}
        t["node_rec"] = z((G * cap, 4), torch.float64)     # 32-byte node records (csrc/mcts_tree.hpp NodeRec)
        t["node_count"] = z((G,), torch.int32)
        t["root_state"] = z((G, 24), torch.uint8)
        t["path"] = z((G, depth + 2), torch.int32)
        t["path_len"] = z((G,), torch.int32)
        t["leaf_flag"] = z((G,), torch.uint8)
        t["leaf_state"] = z((G, 24), torch.uint8)
        t["game_active"] = z((G,), torch.uint8)
        t["slot_game"] = z((G,), torch.int32)
        t["game_plies"] = z((Q,), torch.int32)
        t["game_result"] = z((Q,), torch.int8)
        t["game_done"] = z((Q,), torch.uint8)
        t["game_slot"] = z((Q,), torch.int32)
        t["game_first_move"] = z((Q,), torch.int32)
        t["legal_order"] = z((G, _lib.MAX_LEGAL), torch.uint8)
        t["legal_count"] = z((G,), torch.int32)
        t["pooled"] = z((G, 128), torch.float32)
        t["policy"] = z((G, self.A), torch.float32)   # also holds the fake evaluator's legal-ordered priors (count <= A)
        t["value"] = z((G,), torch.float32)
        hp = self.max_plies if record_history else 1
        t["hist_state72"] = z((Q, hp, 72), torch.uint8)
        t["hist_visits"] = z((Q, hp, self.A), torch.int16)
        t["hist_action"] = z((Q, hp), torch.uint8)
        if self.record_search_value:
            t["hist_value"] = z((Q, hp), torch.float32)    # rows of apply_actions are never written: they read 0
        t["counters"] = z((8,), torch.int32)
        t["stat_leaf_evals"] = z((G,), torch.int32)
        t["stat_terminal_sims"] = z((G,), torch.int32)
        e = self.e = _lib.EngineStructGeneral()
        e.fake_bias = int(fake_bias)
        self._handle = b.handle(model, dev, (self.N, self.A))      # kept alive: the struct points into it
        b.point(self, self._handle)
        self._gnn_flags = int(e.gnn_flags)
        if "packed_weights" not in t:
            t["packed_weights"] = z((4,), torch.float32)
        floats = b.workspace_floats(self.lib, model, self.N, self.A, G)
        if floats:
            t["gnn_workspace"] = z((floats,), torch.float32)

        if eval_cache_slots is None:              # opt-in for whole programs (self_play, train_cycle, pv_mcts): one environment variable
            eval_cache_slots = int(os.environ.get("AQG_EVAL_CACHE_SLOTS", "0")) if b.network else 0
        self.eval_cache_slots = int(eval_cache_slots)
        if self.eval_cache_slots:
            if not b.network:
                raise ValueError("eval_cache_slots needs an evaluator of the library's own networks (the table stores network outputs)")
            if self.eval_cache_slots < 64 or self.eval_cache_slots & (self.eval_cache_slots - 1) or self.eval_cache_slots > (1 << 20):
                raise ValueError("eval_cache_slots must be a power of two in 64 .. 2**20")
            t["eval_cache_keys"] = z((G * self.eval_cache_slots, 32), torch.uint8)
            t["eval_cache_rows"] = torch.empty((G * self.eval_cache_slots, 704), dtype=torch.uint8, device=dev)
            t["eval_cache_slot"] = torch.full((G,), -1, dtype=torch.int32, device=dev)
            t["eval_mask"] = z((G,), torch.uint8)
            t["stat_cache_hits"] = z((G,), torch.int32)
            t["eval_list"] = z((G,), torch.int32)
            t["eval_count"] = z((self.sims + 1,), torch.int32)

        e.board_size, e.num_walls, e.plies_for_draw = self.N, self.num_walls, self.plies_for_draw
        e.num_games, e.quota, e.sims, e.node_cap = G, Q, self.sims, cap
        e.max_plies = hp if record_history else 0
        e.prior_mode = b.prior_mode
        e.c_puct, e.temperature = float(c_puct), float(temperature)
        for name in ("node_rec", "node_count", "root_state", "path",
                     "path_len", "leaf_flag", "leaf_state", "game_active", "slot_game", "game_plies", "game_result", "game_done",
                     "game_slot", "game_first_move", "legal_order",
                     "legal_count", "pooled", "policy", "value", "hist_state72", "hist_visits", "hist_action", "counters",
                     "stat_leaf_evals", "stat_terminal_sims", "packed_weights"):
            setattr(e, name, t[name].data_ptr())
        e.gnn_workspace = t["gnn_workspace"].data_ptr() if "gnn_workspace" in t else None
        if self.eval_cache_slots:
            for name in ("eval_cache_keys", "eval_cache_rows", "eval_cache_slot", "eval_mask", "stat_cache_hits", "eval_list", "eval_count"):
                setattr(e, name, t[name].data_ptr())
            e.eval_cache_log2 = self.eval_cache_slots.bit_length() - 1
        e.root_noise_eps, e.root_noise_alpha = self.root_noise_eps, self.root_noise_alpha
        e.root_noise_seed = self.root_noise_seed if self.root_noise_eps else 0      # off: the four fields are zero
        self.reuse = None
        if self.tree_reuse:
            t["kept"] = z((G,), torch.uint8)
            t["child_index"] = torch.full((G,), -1, dtype=torch.int32, device=dev)
            t["stat_moves_kept"] = z((G,), torch.int32)
            t["stat_visits_kept"] = z((G,), torch.int32)
            ru = self.reuse = _lib.TreeReuseStruct()
            ru.keep_visits = self.keep_visits
            for name in ("kept", "child_index", "stat_moves_kept", "stat_visits_kept"):
                setattr(ru, name, t[name].data_ptr())
        self.resign = None
        if self.resign_options:
            t["resign_min"] = torch.full((Q, 2), float("inf"), dtype=torch.float32, device=dev)
            t["game_resigned"] = z((Q,), torch.uint8)
            rs = self.resign = _lib.ResignStruct()
            rs.threshold, rs.min_ply, rs.disable_fraction = self.resign_options
            rs.seed = self.resign_seed
            rs.resign_min, rs.game_resigned = t["resign_min"].data_ptr(), t["game_resigned"].data_ptr()
        self.record_history = record_history
        self.moves_done = 0
        self.reset()

    # ------------------------------------------------------------------
    def _stream(self):
        return _lib.stream_ptr(self.dev)

    def reset(self):
        _lib.check(self.lib.aqg_engine_reset(ctypes.byref(self.e), self._stream()), "aqg_engine_reset")
        if self.tree_reuse:
            self._forget_kept_trees()
            self.t["stat_moves_kept"].zero_()
            self.t["stat_visits_kept"].zero_()
        if self.resign is not None:
            _lib.check(self.lib.aqg_engine_reset_resign(ctypes.byref(self.e), ctypes.byref(self.resign), self._stream()), "aqg_engine_reset_resign")
        self.moves_done = 0

    # ------------------------------------------------------------------ resignation
    def set_resign_threshold(self, threshold):
        """Another threshold from the next move on (the option must be on: it is a kernel argument, nothing is rebuilt)."""
        if self.resign is None:
            raise ValueError("set_resign_threshold needs resign_threshold")
        self.resign_options = check_resign(threshold, *self.resign_options[1:])
        self.resign.threshold = self.resign_options[0]

    def resign_arrays(self):
        """(resign_min f32 [quota, 2], game_result i8 [quota], enabled bool [quota], game_resigned u8 [quota], game_plies i32 [quota],
        game_done u8 [quota]) as numpy arrays: what the calibration is computed from.  Needs resign_threshold."""
        if self.resign is None:
            raise ValueError("the resignation statistics need resign_threshold")
        lo, res, flag, plies, done = (self.t[k].cpu().numpy() for k in ("resign_min", "game_result", "game_resigned", "game_plies", "game_done"))
        enabled = draw_resign_enabled(self.resign_seed, np.arange(self.quota), self.resign_options[2])
        return lo, res, enabled, flag, plies, done

    def resign_stats(self):
        """Since the last reset, over the finished games: dict(games, games_resigned, plies = the plies played, disabled_games, and over
        the disabled games would_resign = the sides whose running minimum fell below -threshold, false_positives = how many of those
        did not lose, false_positive_rate = their ratio (0.0 without one), eligible_sides = the sides that did not lose)."""
        return resign_stats_of([self.resign_arrays()], self.resign_options[0])

    def suggest_resign_threshold(self, max_false_positive, **kw):
        """suggest_resign_threshold (above) on this engine's finished games; None when there are too few sides to say."""
        return suggest_from_arrays([self.resign_arrays()], max_false_positive, **kw)

    def _forget_kept_trees(self):
        """Clear the "kept" marker: behind everything but a searched move that changes a slot's root."""
        _lib.check(self.lib.aqg_engine_reset_reuse(ctypes.byref(self.e), ctypes.byref(self.reuse), self._stream()), "aqg_engine_reset_reuse")

    def tree_reuse_stats(self):
        """Since the last reset: dict(moves_kept = searched moves that started from a kept subtree, mean_kept_visits = the visits
        such a subtree held on average, 0.0 without one).  Needs tree_reuse=True."""
        if not self.tree_reuse:
            raise ValueError("tree_reuse_stats needs tree_reuse=True")
        moves = int(self.t["stat_moves_kept"].sum().item())
        visits = int(self.t["stat_visits_kept"].to(torch.int64).sum().item())
        return dict(moves_kept=moves, mean_kept_visits=visits / moves if moves else 0.0)

    def refresh_weights(self):
        """Point the engine at the model's current weights; the evaluation cache is cleared when they are not the cached ones."""
        if not self.binding.network:
            return
        handle = self.binding.handle(self.model, self.dev)
        if self.eval_cache_slots and self.binding.stale(self, handle):      # the table holds the OLD weights' (or the other kernel build's) outputs
            self._clear_eval_cache()
        self.binding.point(self, handle)
        self._handle = handle

    def _clear_eval_cache(self):
        _lib.check(self.lib.aqg_engine_clear_eval_cache(ctypes.byref(self.e), self._stream()), "aqg_engine_clear_eval_cache")

    def _set_root_noise(self, table):
        """Table mode: the gamma variates of this move's roots, float64 [G, MAX_LEGAL] (None = the generator).  The table is copied
        into one buffer the engine keeps, so that the struct -- the captured graph's key -- does not change from move to move."""
        if table is None:
            self.e.root_noise = None
            return
        if not self.root_noise_eps:
            raise ValueError("a root_noise table needs root_noise_eps > 0")
        table = torch.as_tensor(table, dtype=torch.float64).to(self.dev).contiguous().view(self.G, _lib.MAX_LEGAL)
        if "root_noise" not in self.t:
            self.t["root_noise"] = torch.zeros((self.G, _lib.MAX_LEGAL), dtype=torch.float64, device=self.dev)
        self.t["root_noise"].copy_(table)        # stream-ordered behind the previous move's reads
        self.e.root_noise = self.t["root_noise"].data_ptr()

    def move(self, uniforms=None, root_noise=None):
        """One move for every active game.  uniforms: float64 [G] in [0,1) (default: device RNG stream).  root_noise: float64
        [G, MAX_LEGAL] gamma variates of this move's roots (default: the counter-based generator; needs root_noise_eps > 0)."""
        self._set_root_noise(root_noise)
        if uniforms is None:
            uniforms = torch.rand((self.G,), dtype=torch.float64, device=self.dev, generator=self.gen)
        else:
            uniforms = torch.as_tensor(uniforms, dtype=torch.float64).to(self.dev).contiguous()
        self._u = uniforms  # keep alive until the stream has consumed it
        targets = self.temperature_plies or self.record_search_value          # either option: the _targets entry points
        extra = (self.temperature_plies, _lib.ptr(self.t.get("hist_value")))
        if self.evaluator == "external":
            self._external_sims()
            if self.resign is not None:
                _lib.check(self.lib.aqg_engine_finish_move_resign(ctypes.byref(self.e), _lib.ptr(uniforms), *extra, None,
                                                                  ctypes.byref(self.resign), self._stream()), "aqg_engine_finish_move_resign")
            elif targets:
                _lib.check(self.lib.aqg_engine_finish_move_targets(ctypes.byref(self.e), _lib.ptr(uniforms), *extra, self._stream()),
                           "aqg_engine_finish_move_targets")
            else:
                _lib.check(self.lib.aqg_engine_finish_move(ctypes.byref(self.e), _lib.ptr(uniforms), self._stream()), "aqg_engine_finish_move")
        elif self.resign is not None:
            _lib.check(self.lib.aqg_engine_move_resign(ctypes.byref(self.e), _lib.ptr(uniforms), *extra,
                                                       ctypes.byref(self.reuse) if self.tree_reuse else None, ctypes.byref(self.resign),
                                                       self._stream()), "aqg_engine_move_resign")
        elif self.tree_reuse:
            _lib.check(self.lib.aqg_engine_move_reuse(ctypes.byref(self.e), _lib.ptr(uniforms), *extra, ctypes.byref(self.reuse), self._stream()),
                       "aqg_engine_move_reuse")
        elif targets:
            _lib.check(self.lib.aqg_engine_move_targets(ctypes.byref(self.e), _lib.ptr(uniforms), *extra, self._stream()),
                       "aqg_engine_move_targets")
        else:
            _lib.check(self.lib.aqg_engine_move(ctypes.byref(self.e), _lib.ptr(uniforms), self._stream()), "aqg_engine_move")
        self.moves_done += 1

    # ------------------------------------------------------------------ moves the engine does not search (evaluate_agents.py)
    def root_states72(self):
        """The current position of every slot: uint8 [G,72] device tensor (rows of inactive slots: valid records, content
        unspecified)."""
        out = torch.empty((self.G, 72), dtype=torch.uint8, device=self.dev)
        _lib.check(self.lib.aqg_engine_root_states72(ctypes.byref(self.e), _lib.ptr(out), self._stream()), "aqg_engine_root_states72")
        return out

    def apply_actions(self, actions):
        """Play actions[g] (int32 [G]; -1 = this active slot has no legal action: its game ends as a draw) in every active slot
        without a search: history row, next(), terminal handling exactly as move() does them."""
        if self.resign is not None:
            raise ValueError("apply_actions() plays moves nobody searched: build the engine without resign_threshold")
        actions = torch.as_tensor(actions, dtype=torch.int32).to(self.dev).contiguous().view(self.G)
        self._applied = actions  # keep alive until the stream has consumed it
        _lib.check(self.lib.aqg_engine_apply_actions(ctypes.byref(self.e), _lib.ptr(actions), self._stream()), "aqg_engine_apply_actions")
        if self.tree_reuse:
            self._forget_kept_trees()      # the roots changed without a search: the next move starts from fresh trees
        self.moves_done += 1

    # ------------------------------------------------------------------ external evaluator (prior_mode 2)
    def _leaf_states(self, idx):
        """game_logic.State objects of the leaves of games `idx` (24-byte packed records: wall masks, pawns, plies)."""
        from .game_logic import State
        raw = self.t["leaf_state"][idx].cpu().numpy().view(np.uint64).reshape(-1, 3)
        nw = (self.N - 1) ** 2
        out = []
        for hw, vw, m in raw:
            hw, vw, m = int(hw), int(vw), int(m)
            walls = [(1 if (hw >> i) & 1 else 0) + (2 if (vw >> i) & 1 else 0) for i in range(nw)]
            out.append(State(board_size=self.N, player=[m & 0xFF, (m >> 8) & 0xFF], enemy=[(m >> 16) & 0xFF, (m >> 24) & 0xFF],
                             walls=walls, plies_played=(m >> 32) & 0xFFFF))
        return out

    def _external_sims(self, device=None):
        """pv_mcts.py:84-85 with the caller's model: per simulation the engine selects a leaf per game, the host asks
        model.predict(state, device) for each (pv_mcts.py:47) and hands the PMF over the leaf's legal actions + the value back."""
        e, st = ctypes.byref(self.e), self._stream()
        _lib.check(self.lib.aqg_engine_begin_move(e, st), "aqg_engine_begin_move")
        for sim in range(self.sims):
            _lib.check(self.lib.aqg_engine_step(e, 1 if sim else 0, 1, st), "aqg_engine_step")
            idx = torch.nonzero(self.t["leaf_flag"] == 1).flatten()
            if idx.numel() == 0:
                continue
            counts = self.t["legal_count"][idx].cpu().numpy()
            pol = torch.zeros((idx.numel(), self.A), dtype=torch.float32)
            val = torch.zeros((idx.numel(),), dtype=torch.float32)
            for j, state in enumerate(self._leaf_states(idx)):
                p, v = self.model.predict(state, device if device is not None else "cpu")
                p = np.asarray(p, dtype=np.float32)
                if p.shape[0] != counts[j]:
                    raise ValueError("model.predict must return one prior per legal action (BaseNetwork.py:36-40)")
                pol[j, :p.shape[0]] = torch.from_numpy(p)
                val[j] = float(v)
            self.t["policy"][idx] = pol.to(self.dev)
            self.t["value"][idx] = val.to(self.dev)
            if sim == 0 and self.root_noise_eps:
                _lib.check(self.lib.aqg_engine_root_noise(e, st), "aqg_engine_root_noise")
        _lib.check(self.lib.aqg_engine_step(e, 1, 0, st), "aqg_engine_step")

    def counters(self):
        c = self.t["counters"].cpu().numpy()
        return dict(active=int(c[0]), finished=int(c[1]), dead_ends=int(c[2]), started=int(c[3]), moves=int(c[4]),
                    gnn_saturated=int(c[5]),      # the split kernels' fp16-range guard fired during this generation (aqgnn.h counters[5])
                    leaf_evals=int(self.t["stat_leaf_evals"].sum().item()),
                    cache_hits=int(self.t["stat_cache_hits"].sum().item()) if self.eval_cache_slots else 0,
                    terminal_sims=int(self.t["stat_terminal_sims"].sum().item()))

    def deferred_legal_searches(self):
        """Leaves whose legal-move search ran beside the trunk, in the evaluation launch, since the last reset (aqgnn.h counters[6];
        option "legal_beside_trunk").  0 wherever the step kernel searches itself: option off, evaluation cache on, other evaluators."""
        return int(self.t["counters"][6].item())

    def switch_to_exact_kernels(self, keep_roots=False):
        """The range guard fired: this weight set leaves fp16 range on positions of this generation.  Its evaluations so far were
        finite but not the network's, so the model is marked and the engine moves to the exact f32-input kernels (the reference's fp32
        has no such cliff, pv_network_gnn.py:53-64).  The play paths then start again from the first ply (reset); search() keeps its
        roots (keep_roots) and drops only the cached evaluations, which are the split kernels' clamped ones."""
        if self.model is not None and hasattr(self.model, "mark_saturated"):
            self.model.mark_saturated(self.dev)
        self._gnn_flags = self.e.gnn_flags = _lib.GNN_EXACT_F32
        self.t["counters"][5] = 0
        if not keep_roots:
            self.reset()
        elif self.eval_cache_slots:
            self._clear_eval_cache()

    def play_generation(self, uniforms=None, check_every=4, root_noise=None):
        """Play the whole quota (== every slot once when quota == num_games: one self_play generation's worth of games
        on this rank).  uniforms: optional float64 [moves, G]; root_noise: optional float64 [moves, G, MAX_LEGAL] gamma variates
        (parity tests).  Returns the counters dict."""
        ply = 0
        limit = self.max_plies * (-(-self.quota // self.G))          # every slot plays at most ceil(quota / G) games
        while True:
            self.move(None if uniforms is None else uniforms[ply], None if root_noise is None else root_noise[ply])
            ply += 1
            if ply >= limit or ply % check_every == 0:
                c = self.counters()
                if c["gnn_saturated"] and not (self.e.gnn_flags & _lib.GNN_EXACT_F32):
                    self.switch_to_exact_kernels()
                    ply = 0
                    continue
                if c["active"] == 0 or ply >= limit:
                    break
        return self.counters()

    # ------------------------------------------------------------------ search only (pv_mcts_policy)
    def search(self, root_states72, check_saturation=True, root_noise=None):
        """pv_mcts_policy for G roots at once: (visits i32 [G, MAX_LEGAL], actions u8, count i32).
        root_noise: float64 [G, MAX_LEGAL] gamma variates of the roots (root_noise_eps > 0; default: the generator, keyed by slot).
        check_saturation (GNN evaluator): the fp16-range guard's word (counters[5]) is cleared before the search and read back after it
        (one 4-byte copy: the callers read the visit counts back anyway); if a launch of this search met a value outside fp16 range its
        evaluations were finite but not the network's, so the weight set is marked (model.mark_saturated), the engine switches to the
        exact f32-input kernels and the search is repeated -- the caller never receives visit counts of clamped evaluations."""
        if self.tree_reuse:
            raise ValueError("search() looks at caller-given roots from fresh trees: build the engine without tree_reuse")
        if self.resign is not None:
            raise ValueError("search() plays no game: build the engine without resign_threshold")
        roots = torch.as_tensor(root_states72, dtype=torch.uint8).to(self.dev).contiguous().view(self.G, 72)
        self._roots = roots
        self._set_root_noise(root_noise)
        for attempt in range(2):
            guarded = check_saturation and self.binding.guarded and not (self.e.gnn_flags & _lib.GNN_EXACT_F32)
            if guarded:
                self.t["counters"][5] = 0          # a cached engine (pv_mcts._engines) must not inherit an earlier search's word
            if self.evaluator == "external":
                _lib.check(self.lib.aqg_engine_set_roots(ctypes.byref(self.e), _lib.ptr(roots), self._stream()), "aqg_engine_set_roots")
                self._external_sims()
            else:
                _lib.check(self.lib.aqg_engine_search(ctypes.byref(self.e), _lib.ptr(roots), self._stream()), "aqg_engine_search")
            if not guarded or int(self.t["counters"][5].item()) == 0:
                break
            self.switch_to_exact_kernels(keep_roots=True)
        visits = torch.empty((self.G, _lib.MAX_LEGAL), dtype=torch.int32, device=self.dev)
        actions = torch.empty((self.G, _lib.MAX_LEGAL), dtype=torch.uint8, device=self.dev)
        count = torch.empty((self.G,), dtype=torch.int32, device=self.dev)
        _lib.check(self.lib.aqg_engine_root_visits(ctypes.byref(self.e), _lib.ptr(visits), _lib.ptr(actions), _lib.ptr(count),
                                                   self._stream()), "aqg_engine_root_visits")
        return visits, actions, count

    def root_priors(self):
        """The priors the last search or move built the root's children from: (priors f32 [G, MAX_LEGAL] in legal_actions() order,
        0 past the count; count i32 [G]) -- with root noise on, the mixed priors."""
        priors = torch.empty((self.G, _lib.MAX_LEGAL), dtype=torch.float32, device=self.dev)
        count = torch.empty((self.G,), dtype=torch.int32, device=self.dev)
        _lib.check(self.lib.aqg_engine_root_priors(ctypes.byref(self.e), _lib.ptr(priors), _lib.ptr(count), self._stream()),
                   "aqg_engine_root_priors")
        return priors, count

    # ------------------------------------------------------------------ history
    def _history_valid(self):
        """(valid bool [quota, hp], ply index [1, hp]): the recorded rows of the finished games."""
        plies = self.t["game_plies"].long()
        hp = self.t["hist_state72"].shape[1]
        idx = torch.arange(hp, device=self.dev).unsqueeze(0)
        return (idx < plies.unsqueeze(1)) & (self.t["game_done"] != 0).unsqueeze(1), idx

    def history_values(self):
        """The recorded search values, float32 [P], row-aligned with history_tensors(): the root's w / n from the mover's side after
        the move's simulations (0 for a move that was applied, not searched).  Needs record_search_value."""
        if not self.record_search_value:
            raise ValueError("history_values needs record_search_value=True")
        return self.t["hist_value"][self._history_valid()[0]]

    def history_tensors(self):
        """(states72 u8 [P,72], visits i16 [P,A], z i8 [P]) for all finished games on this rank, game-major (game index =
        order in which the games were started)."""
        valid, idx = self._history_valid()
        z0 = self.t["game_result"].to(torch.int8).unsqueeze(1)
        sign = torch.where(idx % 2 == 0, 1, -1).to(torch.int8)      # z alternates down the history (self_play.py:63-66)
        z = (z0 * sign)[valid]
        return self.t["hist_state72"][valid], self.t["hist_visits"][valid], z

    def history(self):
        """Reference-format history: list of [[player, enemy, walls], policy list[A] (python floats), z]
        (self_play.py:51-54,:63-66).  policy_i = n_i / sum(n) in float64, exactly like boltzman at T=1."""
        st, vis, z = (x.cpu().numpy() for x in self.history_tensors())
        nw = (self.N - 1) ** 2
        out = []
        for s, v, zz in zip(st, vis, z):
            v = v.astype(np.float64)
            tot = v.sum()
            pol = (v / tot).tolist() if tot > 0 else [0.0] * self.A
            out.append([[[int(s[0]), int(s[1])], [int(s[2]), int(s[3])], [int(x) for x in s[4:4 + nw]]], pol, int(zz)])
        return out


_SET_STREAMS = {}     # (device index, number of sets) -> the streams every MultiSetSelfPlay of that shape runs on


class MultiSetSelfPlay:
    """K independent BatchedSelfPlay sets of a rank's games, each on its own HIP stream.

    One set is a strictly serial chain per simulation (step -> trunk -> heads): while its step / heads kernels run, most of
    the chip idles, and the trunk's last boards leave CUs empty.  Games are independent, so splitting them into K sets whose
    move() calls are enqueued round-robin on K streams lets the GPU fill those holes with another set's kernels (2048 games x
    200 sims, hipGraph replay on: K = 1 / 2 / 3 / 4: ~1,000 / 1,330 / 1,360 / 1,590 games/s, one hardware queue per
    stream).  Streams that share a hardware queue serialise, so the default set count follows the queue count that the
    environment variable GPU_MAX_HW_QUEUES grants the process:
    two sets when it grants fewer than five queues, four when it is unset.  K >= 5 collapses (~550-600 games/s): the GPU
    runs four compute queues concurrently.  What the overlap can and cannot do is measured in DESIGN.md section 4 K4 (a round of the four sets
    costs about the SUM of their trunk launches: two resident trunk workgroups fill a CU's register file, so the other
    sets' kernels run in the trunks' shadow).  Set k is bit-identical to a stand-alone
    BatchedSelfPlay(num_games_k, seed = seed * 64 + k): nothing is shared but the read-only packed weights (and the K
    streams, which every engine of the process reuses -- see _SET_STREAMS)."""

    def __init__(self, model=None, num_games=2048, sims=50, num_sets=None, seed=0, device=None, quota=None, root_noise_seed=None,
                 resign_seed=None, **kw):
        check_resign(kw.get("resign_threshold"), kw.get("resign_min_ply", 0), kw.get("resign_disable_fraction", 0.1),
                     kw.get("record_history", True))          # before anything is allocated
        self.dev = _lib.require_gpu(device)
        if num_sets is None:                      # one hardware queue per set + the default stream, or fall back to 2
            queues = os.environ.get("GPU_MAX_HW_QUEUES")
            num_sets = 4 if queues is None or int(queues) >= 5 else 2
        k = max(1, min(int(num_sets), int(num_games)))
        sizes = [num_games // k + (1 if i < num_games % k else 0) for i in range(k)]
        quota = num_games if quota is None else int(quota)
        quotas = [quota // k + (1 if i < quota % k else 0) for i in range(k)]      # each set refills its own slots
        # The K streams are created once per device and reused by every MultiSetSelfPlay: torch hands out streams from a pool
        # that is never destroyed, and the runtime maps streams onto its hardware queues round-robin -- a second engine
        # with four NEW streams (e.g. the next generation's) would share queues with the first one's idle streams, two of its
        # sets would serialise, and the generation would run 35 % slower (measured: 1,030 vs 1,530 games/s).
        key = (self.dev.index, k)
        if key not in _SET_STREAMS:
            _SET_STREAMS[key] = [torch.cuda.Stream(device=self.dev) for _ in sizes]
        self.streams = _SET_STREAMS[key]
        if model is not None and BINDINGS[kw.get("evaluator", "gnn")].packed:
            model.packed_weights(self.dev)        # pack (+ calibrate) (two forwards and a host sync) on the caller's stream, not inside set 0's
        noise_seeds = set_noise_seeds(seed, root_noise_seed, sizes, [max(q, g) for q, g in zip(quotas, sizes)])
        # the sets' games are numbered through for the enabled / disabled draw as they are for the noise: the numbering rides in the seed
        resign_seeds = set_noise_seeds(seed, default_resign_seed(seed) if resign_seed is None else resign_seed, sizes,
                                       [max(q, g) for q, g in zip(quotas, sizes)])
        self.sets = []
        ready = torch.cuda.current_stream(self.dev).record_event()   # e.g. the model's weight upload on the caller's stream
        for i, g in enumerate(sizes):
            with torch.cuda.stream(self.streams[i]):
                self.streams[i].wait_event(ready)
                self.sets.append(BatchedSelfPlay(model, num_games=g, sims=sims, seed=int(seed) * 64 + i, device=self.dev,
                                                 quota=max(quotas[i], g),
                                                 root_noise_seed=noise_seeds[i], resign_seed=resign_seeds[i], **kw))
        self.G, self.sims = int(num_games), int(sims)
        self.quota = self.G if quota is None else int(quota)
        if self.quota < self.G:
            raise ValueError("quota must be >= num_games")
        self.max_plies = self.sets[0].max_plies
        self.A, self.N = self.sets[0].A, self.sets[0].N
        self._live = [True] * k
        self.sync()

    def _each(self, live_only=False):
        for i, (st, eng) in enumerate(zip(self.streams, self.sets)):
            if live_only and not self._live[i]:
                continue
            with torch.cuda.stream(st):
                yield i, eng

    def sync(self):
        for st in self.streams:
            st.synchronize()

    def reset(self):
        for _, eng in self._each():
            eng.reset()
        self._live = [True] * len(self.sets)

    def move(self):
        """One move for every active game of every live set (a set whose games have all ended is skipped)."""
        for _, eng in self._each(live_only=True):
            eng.move()

    def move_exclusive(self, k, before=None, after=None):
        """Measurement aid (bench.py): one move in which set k runs ALONE on the GPU -- every stream is drained, set k
        makes its move (callbacks `before(set)` / `after(set)` run on its stream around it), is drained again, and only
        then do the other live sets move.  Per-kernel durations taken inside are those of the kernel itself, not of a
        kernel sharing the chip with the other sets' launches.  Results are identical to move()."""
        self.sync()
        k %= len(self.sets)
        if self._live[k]:
            with torch.cuda.stream(self.streams[k]):
                if before:
                    before(self.sets[k])
                self.sets[k].move()
                if after:
                    after(self.sets[k])
            self.streams[k].synchronize()
        for i, eng in self._each(live_only=True):
            if i != k:
                eng.move()
        return self._live[k]

    def counters(self):
        tot = dict(active=0, finished=0, dead_ends=0, started=0, moves=0, gnn_saturated=0, leaf_evals=0, cache_hits=0, terminal_sims=0)
        for i, eng in self._each():
            c = eng.counters()                    # .cpu() inside synchronises this set's stream only
            self._live[i] = self._live[i] and c["active"] > 0
            for key in tot:
                tot[key] += c[key]
        return tot

    def deferred_legal_searches(self):
        return sum(eng.deferred_legal_searches() for _, eng in self._each())

    def tree_reuse_stats(self):
        """The sets' tree_reuse_stats() together (needs tree_reuse=True)."""
        parts = [eng.tree_reuse_stats() for _, eng in self._each()]
        moves = sum(p["moves_kept"] for p in parts)
        visits = sum(p["moves_kept"] * p["mean_kept_visits"] for p in parts)
        return dict(moves_kept=moves, mean_kept_visits=visits / moves if moves else 0.0)

    def set_resign_threshold(self, threshold):
        for eng in self.sets:
            eng.set_resign_threshold(threshold)

    def resign_arrays(self):
        """The sets' resign_arrays() in set order, concatenated (needs resign_threshold)."""
        parts = [eng.resign_arrays() for _, eng in self._each()]
        return tuple(np.concatenate([p[i] for p in parts], 0) for i in range(6))

    def resign_stats(self):
        """The sets' resign_stats() together (needs resign_threshold)."""
        return resign_stats_of([self.resign_arrays()], self.sets[0].resign_options[0])

    def suggest_resign_threshold(self, max_false_positive, **kw):
        return suggest_from_arrays([self.resign_arrays()], max_false_positive, **kw)

    def play_generation(self, check_every=4):
        ply = 0
        limit = self.max_plies * max(-(-e.quota // e.G) for e in self.sets)
        while True:
            self.move()
            ply += 1
            if ply >= limit or ply % check_every == 0:
                c = self.counters()
                if c["gnn_saturated"] and any(not (e.e.gnn_flags & _lib.GNN_EXACT_F32) for e in self.sets):
                    for _, eng in self._each():          # fp16-range guard: replay the generation on the exact f32 kernels
                        eng.switch_to_exact_kernels()
                    self._live = [True] * len(self.sets)
                    ply = 0
                    continue
                if c["active"] == 0 or ply >= limit:
                    break
        return self.counters()

    def history_tensors(self):
        parts = []
        for _, eng in self._each():
            parts.append(eng.history_tensors())
        self.sync()
        cur = torch.cuda.current_stream(self.dev)
        for st in self.streams:
            cur.wait_stream(st)
        for p in parts:
            for x in p:
                x.record_stream(cur)              # the caching allocator must not recycle them under the concatenation
        return tuple(torch.cat([p[j] for p in parts], 0) for j in range(3))

    def history_values(self):
        """The sets' history_values() in set order: float32 [P], row-aligned with history_tensors()."""
        parts = []
        for _, eng in self._each():
            parts.append(eng.history_values())
        self.sync()
        cur = torch.cuda.current_stream(self.dev)
        for st in self.streams:
            cur.wait_stream(st)
        for p in parts:
            p.record_stream(cur)
        return torch.cat(parts, 0)


class TwoEngineMatch:
    """`num_games` games between two sides, game i with side (i % 2) moving first, on two engines: engine `first` holds the games
    in which side `first` moves first.  The loop of evaluate_network.BatchedMatch and evaluate_agents.BatchedAgentMatch; a subclass
    says how an engine is built (`_engine(first, **kw)`) and how engine `first` makes ply `ply` (`_ply(eng, first, ply, *draws)`)."""

    def _build_engines(self, num_games, seed, **kw):
        self.num_games = int(num_games)
        counts = [(self.num_games + 1) // 2, self.num_games // 2]          # games with side 0 first / side 1 first
        self.engines = [self._engine(first, num_games=g, seed=2 * int(seed) + first, **kw) if g else None
                        for first, g in enumerate(counts)]

    def _switch_to_exact_kernels(self):
        for eng in filter(None, self.engines):
            eng.switch_to_exact_kernels()

    def _play(self, *draws):
        """Play every game to the end; side 0's points per game in game order.  fp16-range guard: the counters are read after every
        ply anyway; if a split-kernel launch met a value outside fp16 range (counters()['gnn_saturated']) the moves so far were searched
        with clamped evaluations, so every evaluation switches to the exact f32-input kernels and the match is replayed from ply 0."""
        live = [e is not None for e in self.engines]
        ply = 0
        while any(live):
            for first, eng in enumerate(self.engines):      # every live engine moves ...
                if live[first]:
                    self._ply(eng, first, ply, *draws)
            ply += 1
            for first, eng in enumerate(self.engines):      # ... before any counter is read: the host does not serialise the two
                if not live[first]:
                    continue
                c = eng.counters()
                if eng.binding.guarded and c["gnn_saturated"] and not (eng.e.gnn_flags & _lib.GNN_EXACT_F32):
                    self._switch_to_exact_kernels()
                    return self._play(*draws)               # (once: the exact kernels have no guard to fire)
                if c["active"] == 0 or ply >= eng.max_plies:
                    live[first] = False
        # the first mover's result, +1 / -1 / 0, of every game of each engine
        z0 = [np.zeros((0,)) if eng is None else eng.t["game_result"].cpu().numpy().astype(np.float64) for eng in self.engines]
        per = [(z0[0] + 1.0) / 2.0, 1.0 - (z0[1] + 1.0) / 2.0]      # first_player_point, as side 0's (evaluate_network.py:71-74)
        return [float(per[i % 2][i // 2]) for i in range(self.num_games)]


def gather_history(states72, visits, z, group=None, force_collective=None, values=None):
    """The one exchange step per generation: all-gather the ragged (s, pi, z) tuples of every rank.
    Counts are gathered first, payloads are padded to the max count (RCCL needs equal sizes) and trimmed after.
    Works on any torch.distributed backend (nccl == RCCL on ROCm; gloo in the CPU tests).
    force_collective (default: AQG_DIST_FORCE_GROUP=1): run the two collectives at world size 1 as well instead of returning the
    inputs -- the RCCL code path on the one GPU a developer box has (the result is the same rows, bit for bit).
    values (float32 [P], engine.history_values): every packed row carries its four bytes as well, and a fourth tensor is returned."""
    import torch.distributed as dist
    same = (states72, visits, z) if values is None else (states72, visits, z, values)
    if not (dist.is_available() and dist.is_initialized()):
        return same
    if force_collective is None:
        from .distributed import force_group
        force_collective = force_group()
    if dist.get_world_size(group) == 1 and not force_collective:
        return same
    W = dist.get_world_size(group)
    dev = states72.device
    n = torch.tensor([states72.shape[0]], dtype=torch.int64, device=dev)
    counts = [torch.zeros_like(n) for _ in range(W)]
    dist.all_gather(counts, n, group=group)
    counts = [int(c.item()) for c in counts]
    m = max(counts)
    A = visits.shape[1]
    row = 72 + 2 * A + 1 + (0 if values is None else 4)
    buf = torch.zeros((m, row), dtype=torch.uint8, device=dev)
    k = states72.shape[0]
    if k:
        buf[:k, :72] = states72
        buf[:k, 72:72 + 2 * A] = visits.contiguous().view(torch.uint8).view(k, 2 * A)
        buf[:k, 72 + 2 * A] = z.view(torch.uint8)
        if values is not None:
            buf[:k, 73 + 2 * A:] = values.to(torch.float32).contiguous().view(torch.uint8).view(k, 4)
    out = torch.empty((W * m, row), dtype=torch.uint8, device=dev)
    dist.all_gather_into_tensor(out, buf, group=group)
    out = out.view(W, m, row)
    parts = [out[r, :counts[r]] for r in range(W)]
    allrows = torch.cat(parts, 0)
    s = allrows[:, :72].contiguous()
    v = allrows[:, 72:72 + 2 * A].contiguous().view(torch.int16).view(-1, A)
    zz = allrows[:, 72 + 2 * A].contiguous().view(torch.int8)
    if values is not None:
        return s, v, zz, allrows[:, 73 + 2 * A:].contiguous().view(torch.float32).view(-1)
    return s, v, zz


def gather_resign_arrays(arrays, group=None, device="cpu"):
    """The resignation statistics of every rank, over the exchange of gather_history: a game's record -- its two minima, result,
    enabled flag, resigned flag, done flag and plies -- rides in the 72 bytes of a state row, one row per game.  arrays: the tuple of
    resign_arrays(), or None on a rank that played no game.  Returns the tuple over all ranks, in rank order (the inputs when no
    group is up).  device: where the exchange's tensors live ('cpu' for gloo, the rank's GPU for RCCL)."""
    if arrays is None:
        arrays = (np.zeros((0, 2), np.float32), np.zeros((0,), np.int8), np.zeros((0,), bool), np.zeros((0,), np.uint8),
                  np.zeros((0,), np.int32), np.zeros((0,), np.uint8))
    lo, res, enabled, flag, plies, done = arrays
    K = int(np.asarray(res).shape[0])
    rec = np.zeros((K, 72), dtype=np.uint8)
    rec[:, 0:8] = np.ascontiguousarray(lo, dtype="<f4").reshape(K, 2).view(np.uint8).reshape(K, 8)
    rec[:, 8], rec[:, 9], rec[:, 10] = np.asarray(enabled, dtype=np.uint8), np.asarray(flag, dtype=np.uint8), np.asarray(done, dtype=np.uint8)
    rec[:, 12:16] = np.ascontiguousarray(plies, dtype="<i4").reshape(K, 1).view(np.uint8).reshape(K, 4)
    st = torch.from_numpy(rec).to(device)
    vis = torch.zeros((K, 1), dtype=torch.int16, device=device)
    z = torch.from_numpy(np.ascontiguousarray(res, dtype=np.int8)).to(device)
    st, _, z = gather_history(st, vis, z, group=group)
    rec, res = st.cpu().numpy(), z.cpu().numpy()
    K = rec.shape[0]
    return (np.ascontiguousarray(rec[:, 0:8]).view("<f4").reshape(K, 2), res.astype(np.int8), rec[:, 8].astype(bool), rec[:, 9].copy(),
            np.ascontiguousarray(rec[:, 12:16]).view("<i4").reshape(K), rec[:, 10].copy())
