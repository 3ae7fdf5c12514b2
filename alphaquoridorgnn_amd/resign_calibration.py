"""The resignation calibration (include/aqgnn.h, "resignation"): false positives over the games that were not allowed to resign, and
the threshold they suggest.  Host statistics over the arrays of BatchedSelfPlay.resign_arrays()."""
import numpy as np


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


def _finished(parts):
    """(resign_min, game_result, enabled, game_resigned, game_plies) of the finished games of one or more engines' resign_arrays()."""
    *cols, done = (np.concatenate([np.asarray(p[i]) for p in parts], 0) for i in range(6))
    return [c[done != 0] for c in cols]


def resign_stats_of(parts, threshold):
    """resign_stats over the (resign_min, game_result, enabled, game_resigned, game_plies, game_done) tuples of one or more engines."""
    lo, res, enabled, flag, plies = _finished(parts)
    would, wrong, fine = resign_false_positives(lo, res, enabled, threshold)
    return dict(games=len(res), games_resigned=int(flag.astype(bool).sum()), plies=int(plies.sum()),
                disabled_games=int((~enabled).sum()), would_resign=would, false_positives=wrong,
                false_positive_rate=wrong / would if would else 0.0, eligible_sides=fine)


def suggest_from_arrays(parts, max_false_positive, **kw):
    lo, res, enabled, _, _ = _finished(parts)
    return suggest_resign_threshold(lo, res, enabled, max_false_positive, **kw)
