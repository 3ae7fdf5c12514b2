#!/usr/bin/env python3
"""Golden vectors for pawn jumps and side-steps, case by case, from the REAL reference game_logic.py / agents.py -- generation-time
tooling only, like tools/gen_golden_alpha_beta.py (the reference is imported read-only through tools/gen_golden.py's harness; none
of its text is copied).  One board size per run:

    python tools/gen_golden_jumps.py --board 9        -> tests/golden/jumps_9x9.npz
    python tools/gen_golden_jumps.py --board 5        -> tests/golden/jumps_5x5.npz
    python tools/gen_golden_jumps.py --board 3        -> tests/golden/jumps_3x3.npz

A jump class is (direction U/D/L/R of the other pawn, state of the straight landing) and, where the straight landing is not free,
the states of the two side-steps in list order: F free, E off the board, W behind a wall.  4 x (1 + 2 x 9) = 76 combinations,
68 of them possible on a board (a pawn is never against two opposite rims).

Family A (`family` 0), enumerated: every tile p of the mover, every direction d whose neighbour e = p + d is on the board (the
other pawn stands on e, the step p -> e is never walled); each of the three steps out of e that stays on the board -- straight
(e + d), the two side-steps -- takes no wall, the first or the second wall slot that blocks it (one slot at the rim); the product
of the options, minus the combinations that give one slot two orientations or place two overlapping collinear walls.  Mover's
walls in hand max(num_walls - placed, 1), the other side's num_walls, 4 plies played.  The positions with the other pawn on its
goal row (lost) and with the mover on row 0 stay in: the reference still defines their lists and transitions.

Family B (`family` 1; 9x9 and 5x5), crowded boards: the 8 distinct wall layouts of walk_NxN.npz with the most walls (stable sort
by wall count, descending, over the states in which both sides still hold a wall; walls in hand and plies of the first state that
shows the layout), and on each every ordered pair (mover, other) of neighbouring tiles with the mover off row 0 and the other pawn
off its goal row; kept when both sides still have a path (the reference's breadth-first search); at most 5 % may go (asserted).

Stored per state: `states` u8 [n,72], `family` u8 [n], `legal` i16 [n,136] (State.legal_actions(), -1 past the count), `counts`
i32 [n], `paths` i16 [n,2] (plies to the goal row of the mover and of the other side in the flipped position, -1 = none: a
breadth-first search over State.legal_actions_pos as in tools/gen_golden_alpha_beta.py, checked against heuristic_eval), `status`
u8 [n] (bit 0 is_lose, bit 1 is_draw).  Prints the case, class and pawn-move-count figures that tools/README.md quotes."""
import argparse, itertools, os, sys
sys.dont_write_bytecode = True
os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import gen_golden as gg  # noqa: E402
import gen_golden_alpha_beta as gab  # noqa: E402

DIRS = [(-1, 0), (1, 0), (0, -1), (0, 1)]          # U, D, L, R: the reference's MOVEMENT_DIRECTIONS


def blocking_slots(N, x, y, dx, dy):
    """(slot, orientation) of the walls that block the step from tile (x, y) by (dx, dy), first slot first: the slots
    State.legal_actions_pos's is_wall_blocking reads, in its order."""
    W = N - 1
    if dx:
        r = x if dx > 0 else x - 1
        return [(r * W + c, 1) for c in (y, y - 1) if 0 <= c < W]
    c = y if dy > 0 else y - 1
    return [(r * W + c, 2) for r in (x, x - 1) if 0 <= r < W]


def side_steps(dx, dy):
    return [(0, -1), (0, 1)] if dx else [(-1, 0), (1, 0)]


def overlapping(N, walls):
    W = N - 1
    for s, o in walls.items():
        if o == 1 and s % W < W - 1 and walls.get(s + 1) == 1:
            return True
        if o == 2 and walls.get(s + W) == 2:
            return True
    return False


def family_a(gl, N, num_walls):
    out = []
    for p in range(N * N):
        x, y = divmod(p, N)
        for dx, dy in DIRS:
            ex, ey = x + dx, y + dy
            if not (0 <= ex < N and 0 <= ey < N):
                continue
            options = []
            for sx, sy in [(dx, dy)] + side_steps(dx, dy):
                if 0 <= ex + sx < N and 0 <= ey + sy < N:
                    options.append([None] + blocking_slots(N, ex, ey, sx, sy))
            for combo in itertools.product(*options):
                walls, clash = {}, False
                for w in combo:
                    if w is not None:
                        clash |= walls.get(w[0], w[1]) != w[1]
                        walls[w[0]] = w[1]
                if clash or overlapping(N, walls):
                    continue
                w = [0] * ((N - 1) ** 2)
                for s, o in walls.items():
                    w[s] = o
                out.append(gl.State(board_size=N, player=[p, max(num_walls - len(walls), 1)],
                                    enemy=[N * N - 1 - (ex * N + ey), num_walls], walls=w, plies_played=4))
    return out


def family_b(gl, N):
    g = np.load(os.path.join(REPO, "tests", "golden", f"walk_{N}x{N}.npz"))
    recs, nw = g["states"], (N - 1) ** 2
    ok = np.flatnonzero((recs[:, 1] >= 1) & (recs[:, 3] >= 1))
    placed = (recs[ok, 4:4 + nw] != 0).sum(1)
    layouts, seen = [], set()
    for i in ok[np.argsort(-placed, kind="stable")]:
        key = recs[i, 4:4 + nw].tobytes()
        if key not in seen:
            seen.add(key)
            layouts.append(recs[i])
            if len(layouts) == 8:
                break
    kept, total = [], 0
    for r in layouts:
        plies = int(r[68]) | (int(r[69]) << 8)
        for p in range(N, N * N):                                            # the mover off row 0
            x, y = divmod(p, N)
            for dx, dy in DIRS:
                ex, ey = x + dx, y + dy
                if not (0 <= ex < N - 1 and 0 <= ey < N):                    # the other pawn on the board and off its goal row
                    continue
                total += 1
                s = gl.State(board_size=N, player=[p, int(r[1])], enemy=[N * N - 1 - (ex * N + ey), int(r[3])],
                             walls=[int(v) for v in r[4:4 + nw]], plies_played=plies)
                if min(gab.both_paths(s)) >= 0:
                    kept.append(s)
    assert len(layouts) == 8 and (total - len(kept)) * 20 <= total, (len(layouts), total, len(kept))
    print(f"family B: {len(kept)} kept of {total} ({100.0 * (total - len(kept)) / total:.1f} % dropped), walls per layout",
          [int((r[4:4 + nw] != 0).sum()) for r in layouts])
    return kept


def jump_class(s):
    """The class of a state with the pawns on neighbouring tiles and no wall between them, by the reference's own rule code
    (figures for the print-out only; the tests classify from the walls on their own)."""
    N = s.N
    x, y = divmod(s.player[0], N)
    ex, ey = divmod(N * N - 1 - s.enemy[0], N)
    d = DIRS.index((ex - x, ey - y))
    here = s.legal_actions_pos(ex * N + ey)           # the steps out of e that neither the rim nor a wall stops (the mover is no obstacle:
    #                                                   it stands behind e, never on one of the three landings)

    def state(sx, sy):
        tx, ty = ex + sx, ey + sy
        if not (0 <= tx < N and 0 <= ty < N):
            return "E"
        if any((sl, o) in walled for sl, o in blocking_slots(N, ex, ey, sx, sy)):
            return "W"
        assert tx * N + ty in here
        return "F"
    walled = {(i, o) for i, o in enumerate(s.walls) if o}
    straight = state(*DIRS[d])
    if straight == "F":
        return "UDLR"[d] + "F"
    return "UDLR"[d] + straight + "".join(state(sx, sy) for sx, sy in side_steps(*DIRS[d]))


def save_npz(path, arrays):
    """np.savez_compressed with a fixed time stamp on every member: a second run writes the same bytes."""
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, "w", force_zip64=True) as f:
                np.lib.format.write_array(f, np.ascontiguousarray(a), allow_pickle=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--board", type=int, default=9)
    args = ap.parse_args()
    N = args.board
    gl, pv_mcts, self_play, cnn = gg.import_reference(N)
    import agents
    num_walls = gg.BOARDS[N][0]
    a = family_a(gl, N, num_walls)
    assert len(a) == {9: 4524, 5: 940, 3: 156}[N], len(a)
    b = family_b(gl, N) if N >= 5 else []
    states = a + b
    recs, legal, paths, status, pawn_counts, classes = [], [], [], [], [], ([], [])
    for i, s in enumerate(states):
        la = s.legal_actions()
        recs.append(gg.rec_of(s))
        legal.append(la)
        paths.append(gab.both_paths(s))
        assert agents.heuristic_eval(s) == (paths[-1][1] - paths[-1][0]) / agents.MAX_DIST_FROM_GOAL
        assert recs[-1].tobytes() == gg.rec_of(s).tobytes()                   # both_paths / heuristic_eval put the state back
        status.append((1 if s.is_lose() else 0) | (2 if s.is_draw() else 0))
        pawn = s.legal_actions_pos(s.player[0])
        assert la[:len(pawn)] == pawn
        fam = 0 if i < len(a) else 1
        x, y = divmod(s.player[0], N)
        ex, ey = divmod(N * N - 1 - s.enemy[0], N)
        if not any((sl, o) in {(j, w) for j, w in enumerate(s.walls) if w} for sl, o in blocking_slots(N, x, y, ex - x, ey - y)):
            classes[fam].append(jump_class(s))
        if fam == 0:
            pawn_counts.append(len(pawn))
    out = dict(states=np.stack(recs), family=np.asarray([0] * len(a) + [1] * len(b), dtype=np.uint8), legal=gg.pack_lists(legal, 136),
               counts=np.asarray([len(l) for l in legal], dtype=np.int32), paths=np.asarray(paths, dtype=np.int16),
               status=np.asarray(status, dtype=np.uint8))
    path = os.path.join(REPO, "tests", "golden", f"jumps_{N}x{N}.npz")
    save_npz(path, out)
    print(f"{N}x{N}: family A {len(a)} cases, {len(set(classes[0]))} classes ({len({c for c in classes[0] if c[1] != 'F'})} not straight);",
          f"family B {len(b)} cases, {len(classes[1])} of them unwalled, {len(set(classes[1]))} classes;",
          f"pawn moves in family A {np.bincount(pawn_counts, minlength=6).tolist()};",
          f"lost {int((out['status'] & 1).sum())}, mover on row 0 {int((out['states'][:, 0] < N).sum())},",
          f"no path {int((out['paths'] < 0).any(1).sum())} (family A {int((out['paths'][:len(a)] < 0).any(1).sum())});",
          f"{os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
