"""Positions for the tests of the wall searches' task layouts and of the witness-path filter experiment (test infrastructure):
hand-built records, random-walk states, and the host build of tests/hostcheck/witnesscheck.cpp -- how many candidates a position
leaves to search, and what the (host-only, not shipped) witness-path filter would make of them."""
import ctypes
import os
import subprocess

import numpy as np

from tests import _util as U

_wc = None


def witnesscheck():
    global _wc
    if _wc is None:
        src = os.path.join(U.HERE, "hostcheck", "witnesscheck.cpp")
        hdr = os.path.join(U.REPO, "alphaquoridorgnn_amd", "csrc", "quoridor_core.hpp")
        so = os.path.join(U.HERE, "hostcheck", "libwitnesscheck.so")
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", so, src])
        _wc = ctypes.CDLL(so)
    return _wc


def survivors(N, rec):
    """(candidates left by the prefilter = what the kernels search, candidates the witness filter would leave, plain-path bits:
    1 mover, 2 enemy)."""
    pre, post, paths, _ = _survivors(N, rec)
    return pre, post, paths


def wrongly_cleared(N, rec):
    """Candidates the witness filter clears although one of the two searches rejects them: must be 0."""
    return _survivors(N, rec)[3]


def _survivors(N, rec):
    rec = np.ascontiguousarray(rec, dtype=np.uint8)
    out = np.zeros(5, dtype=np.uint64)
    paths = witnesscheck().wc_survivors(N, U._p(rec), U._p(out))
    assert paths >= 0
    pc = [bin(int(x)).count("1") for x in out[:4]]
    return pc[0] + pc[1], pc[2] + pc[3], paths, int(out[4])


def rec(N, me, other, walls, pwl=5, ewl=5, plies=10):
    """A state72 record.  me / other: (row, col) of the mover and of the enemy in the MOVER's frame; walls: {(sx, sy): 1 (H) | 2 (V)}."""
    S = N - 1
    r = np.zeros(72, dtype=np.uint8)
    r[0], r[1] = me[0] * N + me[1], pwl
    r[2], r[3] = N * N - 1 - (other[0] * N + other[1]), ewl
    for (sx, sy), o in walls.items():
        assert 0 <= sx < S and 0 <= sy < S and r[4 + sx * S + sy] == 0
        r[4 + sx * S + sy] = o
    r[68], r[69], r[70] = plies & 0xFF, plies >> 8, N
    return r


H, V = 1, 2


def plugged_corridor(N, extra=None):
    """The mover stands at the bottom of a one-tile corridor along column 0 (V walls on its right, an H wall below) and the
    enemy pawn stands in the corridor above it: no plain path for the mover, only the jump."""
    walls = {(0, 0): V, (2, 0): V, (3, 0): H}
    walls.update(extra or {})
    return rec(N, (3, 0), (2, 0), walls)


def hand_positions(N):
    """name -> record, for N = 5 and 9."""
    S = N - 1
    out = {"plugged_corridor": plugged_corridor(N)}
    # pawns adjacent (mover below the enemy), an H wall behind the enemy: the straight jump is closed, the diagonal ones are open
    out["adjacent_diagonal_jump"] = rec(N, (2, 2), (1, 2), {(0, 2): H, (2, 0): V})
    # an H wall line across the board except the last column: the only way up runs along the right border
    out["border_path"] = rec(N, (3, 1), (0, 2), _line_with_gap(N))
    # the same line: the candidate V / H walls at the gap close it -- true blockers among the survivors
    out["last_gap"] = rec(N, (2, 0), (0, 1), _line_with_gap(N))
    out["no_walls_in_hand"] = rec(N, (3, 1), (0, 2), _line_with_gap(N), pwl=0)
    return out


def _line_with_gap(N):
    """H walls under row 1 over columns 0 .. N-2 (slots (1, 0), (1, 2), ...): only column N-1 is open, so every way up runs
    along the right border, and the candidates at the gap close the line."""
    S = N - 1
    return {(1, y): H for y in range(0, S, 2)}


def random_walk_states(N, count, seed):
    """`count` states of wall-heavy random play from the oracle's rules (walls in hand or not, as they come)."""
    from oracle import quoridor as oq
    rng = np.random.RandomState(seed)
    out = []
    while len(out) < count:
        s = oq.State(N=N)
        while not s.is_done() and len(out) < count:
            out.append(s.rec.copy())
            la = s.legal_actions()
            walls = [a for a in la if a >= N * N]
            pick = walls if (walls and rng.rand() < 0.5) else la
            s = s.next(pick[rng.randint(len(pick))])
    return np.stack(out)


def crowded(N, more_than, seed):
    """A plugged-corridor position with walls added one by one
    wherever that does not lower the number of candidates to search, until it exceeds `more_than`."""
    rng = np.random.RandomState(seed)
    S = N - 1
    extra = {}
    best = survivors(N, plugged_corridor(N))[0]
    for _ in range(4000):
        if best > more_than:
            break
        slot, o = (rng.randint(S), rng.randint(S)), int(rng.randint(1, 3))
        if slot in extra or slot in ((0, 0), (2, 0), (3, 0)):
            continue
        trial = dict(extra)
        trial[slot] = o
        if not _geometry_ok(N, plugged_corridor(N, extra), slot, o):
            continue
        n = survivors(N, plugged_corridor(N, trial))[0]
        if n >= best:                       # sideways steps too: a wall that touches nothing yet gives the next ones something to touch
            best, extra = n, trial
    return plugged_corridor(N, extra)


def _geometry_ok(N, r, slot, o):
    """can_place_wall's geometry: the slot is free and no wall of the same orientation lies on the neighbouring slot of its line."""
    S = N - 1
    w = r[4:4 + S * S].reshape(S, S)
    sx, sy = slot
    if w[sx, sy]:
        return False
    if o == H:
        return not ((sy > 0 and w[sx, sy - 1] == H) or (sy < S - 1 and w[sx, sy + 1] == H))
    return not ((sx > 0 and w[sx - 1, sy] == V) or (sx < S - 1 and w[sx + 1, sy] == V))


def most_crowded():
    """The 9x9 position with the most candidates to search that is known: 63.  tools/crowded_search.cpp (an annealing search over
    wall sets and pawn tiles, with and without the placement rules for the walls) ends at 63 in every run, so a wavefront's 64 task
    lanes are not exceeded at the largest board size; this position fills all but one of them."""
    hw, vw = 0x4422882288049104, 0x100006000
    walls = {(i // 8, i % 8): (H if (hw >> i) & 1 else V) for i in range(64) if ((hw | vw) >> i) & 1}
    return rec(9, (2, 7), (3, 6), walls)
