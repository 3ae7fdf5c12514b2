"""Pawn jumps and side-steps, case by case (test infrastructure): the fixtures tests/golden/jumps_NxN.npz (tools/gen_golden_jumps.py),
a classifier and a pawn-move rule written over blocked EDGES between tiles -- independent of oracle/quoridor_oracle.c and of
csrc/quoridor_core.hpp, which both ask per step which wall SLOTS block it -- the enumerator of family A for a board size without
reference constants, and the one-state-per-class selection the GPU tests search from.

A jump class: the direction U/D/L/R in which the other pawn stands on an unwalled neighbour of the mover, the state of the straight
landing behind it and, where that is not free, the states of the two side-steps in list order (left, right of a vertical jump; up,
down of a horizontal one): F free, E off the board, W behind a wall.  4 x (1 + 2 x 9) = 76 combinations; the 8 with both
side-steps off the board need a board one tile wide, 68 remain."""
import functools
import itertools

import numpy as np

from tests import _util as U

DIRS = [(-1, 0), (1, 0), (0, -1), (0, 1)]          # U, D, L, R
WALLS = {3: 1, 5: 2, 7: 6, 9: 10}
DRAW = {3: 14, 5: 28, 7: 70, 9: 116}
ALL_CLASSES = frozenset(d + "F" for d in "UDLR") | frozenset(
    d + s + a + b for d in "UDLR" for s in "EW" for a in "FEW" for b in "FEW" if (a, b) != ("E", "E"))
assert len(ALL_CLASSES) == 68


def _sides(dx, dy):
    return [(0, -1), (0, 1)] if dx else [(-1, 0), (1, 0)]


def blocked_edges(rec):
    """The pairs of neighbouring tiles a wall of the record separates: a horizontal wall in the 2x2 block with top-left tile t cuts
    t | t + N and t + 1 | t + 1 + N, a vertical one t | t + 1 and t + N | t + N + 1."""
    N = int(rec[70])
    cut = set()
    for s in np.flatnonzero(rec[4:4 + (N - 1) ** 2]):
        t = int(s) // (N - 1) * N + int(s) % (N - 1)
        cut |= {(t, t + N), (t + 1, t + 1 + N)} if rec[4 + s] == 1 else {(t, t + 1), (t + N, t + N + 1)}
    return cut


def _step(N, cut, x, y, dx, dy):
    """F / E / W for the step from tile (x, y) by (dx, dy)."""
    tx, ty = x + dx, y + dy
    if not (0 <= tx < N and 0 <= ty < N):
        return "E"
    a, b = sorted((x * N + y, tx * N + ty))
    return "W" if (a, b) in cut else "F"


def _pawns(rec):
    N = int(rec[70])
    return N, divmod(int(rec[0]), N), divmod(N * N - 1 - int(rec[2]), N)


def classify(rec):
    """The jump class of a record, None where the pawns are not on neighbouring tiles or a wall stands between them."""
    N, (x, y), (ex, ey) = _pawns(rec)
    if abs(ex - x) + abs(ey - y) != 1:
        return None
    cut = blocked_edges(rec)
    dx, dy = ex - x, ey - y
    if _step(N, cut, x, y, dx, dy) != "F":
        return None
    d = "UDLR"[DIRS.index((dx, dy))]
    straight = _step(N, cut, ex, ey, dx, dy)
    if straight == "F":
        return d + "F"
    return d + straight + "".join(_step(N, cut, ex, ey, sx, sy) for sx, sy in _sides(dx, dy))


def pawn_moves(rec):
    """The ordered pawn moves of a record by the edge rule: U, D, L, R; over the other pawn straight, else the side-steps."""
    N, (x, y), (ex, ey) = _pawns(rec)
    cut = blocked_edges(rec)
    out = []
    for dx, dy in DIRS:
        if _step(N, cut, x, y, dx, dy) != "F":
            continue
        nx, ny = x + dx, y + dy
        if (nx, ny) != (ex, ey):
            out.append(nx * N + ny)
        elif _step(N, cut, nx, ny, dx, dy) == "F":
            out.append((nx + dx) * N + ny + dy)
        else:
            out += [(nx + sx) * N + ny + sy for sx, sy in _sides(dx, dy) if _step(N, cut, nx, ny, sx, sy) == "F"]
    return out


def _slots(N, x, y, dx, dy):
    """(slot, orientation) of the walls that block the step from tile (x, y) by (dx, dy), in the order the rule code reads them."""
    W = N - 1
    if dx:
        r = x if dx > 0 else x - 1
        return [(r * W + c, 1) for c in (y, y - 1) if 0 <= c < W]
    c = y if dy > 0 else y - 1
    return [(r * W + c, 2) for r in (x, x - 1) if 0 <= r < W]


def enumerate_family_a(N):
    """Family A of tools/gen_golden_jumps.py for any board size, as records: every tile of the mover, every neighbour for the other
    pawn, each of the three steps out of it with no wall / its first / its second blocking slot; no slot with two orientations, no two
    overlapping collinear walls; walls in hand max(num_walls - placed, 1) and num_walls, 4 plies played."""
    W, out = N - 1, []
    for p in range(N * N):
        x, y = divmod(p, N)
        for dx, dy in DIRS:
            ex, ey = x + dx, y + dy
            if not (0 <= ex < N and 0 <= ey < N):
                continue
            options = [[None] + _slots(N, ex, ey, sx, sy) for sx, sy in [(dx, dy)] + _sides(dx, dy)
                       if 0 <= ex + sx < N and 0 <= ey + sy < N]
            for combo in itertools.product(*options):
                walls = {}
                for w in combo:
                    if w is not None and walls.setdefault(w[0], w[1]) != w[1]:
                        break
                else:
                    if any((o == 1 and s % W < W - 1 and walls.get(s + 1) == 1) or (o == 2 and walls.get(s + W) == 2)
                           for s, o in walls.items()):
                        continue
                    rec = np.zeros(72, dtype=np.uint8)
                    rec[0], rec[1] = p, max(WALLS[N] - len(walls), 1)
                    rec[2], rec[3] = N * N - 1 - (ex * N + ey), WALLS[N]
                    for s, o in walls.items():
                        rec[4 + s] = o
                    rec[68], rec[70] = 4, N
                    out.append(rec)
    return np.stack(out)


def flipped(recs):
    """The positions seen by the other side without a move: the walls rotated, the pawns swapped."""
    recs = np.asarray(recs)
    nw = (int(recs.reshape(-1, 72)[0, 70]) - 1) ** 2
    out = recs.copy()
    out[..., 4:4 + nw] = recs[..., 4:4 + nw][..., ::-1]
    out[..., 0:2], out[..., 2:4] = recs[..., 2:4], recs[..., 0:2]
    return out


def pawn_next(recs, actions):
    """State.next for pawn actions, in numpy: the pawn moved, the board turned by 180 degrees, the sides swapped, one more ply."""
    recs = np.asarray(recs)
    out = flipped(recs)
    out[:, 2] = actions
    plies = (recs[:, 68].astype(np.int64) | (recs[:, 69].astype(np.int64) << 8)) + 1
    out[:, 68], out[:, 69] = plies & 0xFF, plies >> 8
    return out


def pawn_count(N, legal):
    """Length of the pawn-move prefix of every row of a padded legal list."""
    return ((legal >= 0) & (legal < N * N)).sum(1)


class Cases:
    """One fixture file with everything derived from it once: `cls` (class per state, None outside), `npawn`, `one_per_class`,
    `first_of_class`."""

    def __init__(self, N):
        g = U.golden(f"jumps_{N}x{N}.npz")
        self.N = N
        for k in ("states", "family", "legal", "counts", "paths", "status"):
            setattr(self, k, g[k])
        self.cls = [classify(r) for r in self.states]
        self.npawn = pawn_count(N, self.legal)
        picked, seen = [], set()
        for i, c in enumerate(self.cls):                 # family A comes first in the file; the mover off row 0, nobody has lost
            if c is not None and (int(self.family[i]), c) not in seen and self.status[i] == 0 and self.states[i, 0] >= N:
                seen.add((int(self.family[i]), c))
                picked.append(i)
        self.one_per_class = np.asarray(picked)
        first = {}
        for i in np.flatnonzero(self.family == 0):       # every class, lost positions and the mover on row 0 included: lists only
            first.setdefault(self.cls[i], int(i))
        self.first_of_class = np.asarray(sorted(first.values()))
        self.one_per_class_counts = tuple(len({c for f, c in seen if f == fam}) for fam in (0, 1))

    def mask(self, rows=slice(None)):
        legal = self.legal[rows]
        A = self.N ** 2 + 2 * (self.N - 1) ** 2
        m = np.zeros((len(legal), A + 1), dtype=np.uint8)
        m[np.arange(len(legal))[:, None], np.where(legal >= 0, legal, A)] = 1
        return m[:, :A]


@functools.lru_cache(maxsize=None)
def cases(N):
    return Cases(N)


# What `one_per_class` must hold per board size: (classes of family A, classes of family B).  Of the 68 classes, 24 have no state a
# search can start from: D with the straight landing off the board (8) and L / R with the lower side-step off the board (8) put the
# other pawn on its goal row -- the mover has lost --, L / R with the upper side-step off the board (8) put the mover on row 0.  That
# leaves 44; a 3x3 board has no live state either for the 9 other D classes (the mover on row 0, or the other pawn on row 2).  The
# tests over whole files reach all 68.
ONE_PER_CLASS = {9: (44, 39), 5: (44, 25), 3: (35, 0)}
