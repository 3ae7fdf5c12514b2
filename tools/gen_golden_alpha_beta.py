#!/usr/bin/env python3
"""Golden vectors for the alpha-beta agent on positions WITH WALLS IN HAND, from the real reference agents.py -- generation-time
tooling only, like tools/gen_golden_agents.py (the reference is imported read-only through tools/gen_golden.py's harness; none of
its text is copied).  One board size per run:

    python tools/gen_golden_alpha_beta.py --board 5        -> tests/golden/ab_walls_5x5.npz
    python tools/gen_golden_alpha_beta.py --board 9        -> tests/golden/ab_walls_9x9.npz

agents_NxN.npz pins the search on trees of pawn moves only (no 9x9 state and 4 of 30 5x5 states there hold a wall); these files
pin the wall branch.  In every stored state at least one side holds walls.  Stored per state: the state72 record, the reference's
heuristic_eval, both shortest paths (a breadth-first search over the reference's State.legal_actions_pos, mover then other side,
checked against heuristic_eval before it is written), alpha_beta_action at depth 1, and -- for the states listed in `ab2_index` --
at depth 2.  Flags recorded with each state: `both_walls` (both sides hold walls), `adjacent` (the pawns stand on neighbouring
tiles), `diagonal` (the mover's pawn moves include a diagonal jump: a wall or the edge lies behind the jumped pawn).

  5x5   24 states of seeded random walks; >= 8 with both_walls, >= 4 adjacent, >= 1 diagonal (asserted below); depth 2 on all.
  9x9   12 states of seeded random walks with walls in hand at depth 1, followed by late positions with at most 3 walls left per
        side at depth 1 AND 2 (`ab2_count` of them; the reference's pure-Python search needs minutes per position on anything
        earlier).

Run times in the build container (one CPU): 5x5 4 s, 9x9 100 s, 88 s of them in the six depth-2 searches."""
import argparse, os, sys, time
sys.dont_write_bytecode = True
os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import gen_golden as gg  # noqa: E402


def shortest_path(state):
    """Plies to row 0 over State.legal_actions_pos from the mover's tile, first in first out; -1 = none."""
    seen, queue, head = {state.player[0]}, [(state.player[0], 0)], 0
    while head < len(queue):
        pos, depth = queue[head]
        head += 1
        if pos // state.N == 0:
            return depth
        for nxt in state.legal_actions_pos(pos):
            if nxt not in seen:
                seen.add(nxt)
                queue.append((nxt, depth + 1))
    return -1


def both_paths(state):
    sp = shortest_path(state)
    state.rotate_walls()
    state.player, state.enemy = state.enemy, state.player
    se = shortest_path(state)
    state.rotate_walls()
    state.player, state.enemy = state.enemy, state.player
    return sp, se


def flags(state):
    N = state.N
    me, other = state.player[0], N * N - 1 - state.enemy[0]
    adjacent = abs(me // N - other // N) + abs(me % N - other % N) == 1
    diagonal = any(abs(t // N - me // N) == 1 and abs(t % N - me % N) == 1 for t in state.legal_actions_pos(me))
    return state.player[1] > 0 and state.enemy[1] > 0, adjacent, diagonal


def walk_pool(gl, rng, games, p_wall, p_forward, keep):
    """Positions of random legal play.  A pawn move goes forward (to a smaller row) with probability p_forward when it can, so
    that the pawns meet while walls are still in hand."""
    pool = []
    for _ in range(games):
        s = gl.State()
        while not s.is_done():
            la = s.legal_actions()
            N2 = s.N * s.N
            pawn, wall = [a for a in la if a < N2], [a for a in la if a >= N2]
            fwd = [a for a in pawn if a // s.N < s.player[0] // s.N]
            if wall and (not pawn or rng.rand() < p_wall):
                a = wall[rng.randint(len(wall))]
            elif fwd and rng.rand() < p_forward:
                a = fwd[rng.randint(len(fwd))]
            else:
                a = pawn[rng.randint(len(pawn))]
            s = s.next(a)
            if not s.is_done() and keep(s):
                pool.append(s)
    return pool


def pick(pool, count, quotas):
    """`count` states of the pool in pool order: first what each quota (flag index, minimum) still lacks, then whatever comes."""
    chosen = []
    for flag, need in quotas:
        for i, s in enumerate(pool):
            if sum(1 for j in chosen if flags(pool[j])[flag]) >= need:
                break
            if i not in chosen and flags(s)[flag]:
                chosen.append(i)
    for i in range(len(pool)):
        if len(chosen) >= count:
            break
        if i not in chosen:
            chosen.append(i)
    return [pool[i] for i in sorted(chosen[:count])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--board", type=int, default=5)
    args = ap.parse_args()
    board = args.board
    gl, pv_mcts, self_play, cnn = gg.import_reference(board)
    import agents
    rng = np.random.RandomState(17)
    holds = lambda s: s.player[1] > 0 or s.enemy[1] > 0
    if board == 5:
        pool = walk_pool(gl, rng, 60, 0.15, 0.8, lambda s: holds(s) and rng.rand() < 0.5)
        states = pick(pool, 24, [(2, 1), (1, 4), (0, 8)])
        deep = list(range(len(states)))
    else:
        pool = walk_pool(gl, rng, 6, 0.3, 0.6, lambda s: holds(s) and s.plies_played <= 30 and rng.rand() < 0.3)
        states = pick(pool, 12, [(1, 1), (0, 8)])
        late = walk_pool(gl, rng, 30, 0.85, 0.5,
                         lambda s: holds(s) and s.player[1] <= 3 and s.enemy[1] <= 3 and s.player[1] + s.enemy[1] <= 4)
        seen, lates = set(), []
        for s in late:                                  # one position per (mover's walls, other's walls), in pool order
            key = (s.player[1], s.enemy[1])
            if key not in seen:
                seen.add(key)
                lates.append(s)
        lates = lates[:6]
        deep = list(range(len(states), len(states) + len(lates)))
        states = states + lates
    fl = np.asarray([flags(s) for s in states], dtype=bool)
    assert all(holds(s) for s in states)
    if board == 5:
        assert len(states) == 24 and fl[:, 0].sum() >= 8 and fl[:, 1].sum() >= 4 and (fl[:, 1] & fl[:, 2]).sum() >= 1, fl.sum(0)
    else:
        assert len(states) - len(deep) == 12 and len(deep) >= 4
        assert all(states[i].player[1] <= 3 and states[i].enemy[1] <= 3 for i in deep)
    recs, heur, paths, ab1, ab2 = [], [], [], [], []
    t0 = time.time()
    for i, s in enumerate(states):
        recs.append(gg.rec_of(s))
        heur.append(agents.heuristic_eval(s))
        paths.append(both_paths(s))
        assert heur[-1] == (paths[-1][1] - paths[-1][0]) / agents.MAX_DIST_FROM_GOAL
        ab1.append(-1 if (a1 := agents.alpha_beta_action(s, 1)) is None else a1)
        if i in deep:
            ab2.append(-1 if (a2 := agents.alpha_beta_action(s, 2)) is None else a2)
        print(i, "walls", s.player[1], s.enemy[1], "legal", len(s.legal_actions()), "flags", fl[i].astype(int), "paths", paths[-1],
              "ab1", ab1[-1], "ab2", ab2[-1] if i in deep else "-", f"{time.time() - t0:.0f}s", flush=True)
    out = dict(board=np.asarray([board]), max_dist=np.asarray([agents.MAX_DIST_FROM_GOAL]), states=np.stack(recs),
               heuristic=np.asarray(heur, dtype=np.float64), paths=np.asarray(paths, dtype=np.int16),
               ab1=np.asarray(ab1, dtype=np.int16), ab2_index=np.asarray(deep, dtype=np.int64), ab2=np.asarray(ab2, dtype=np.int16),
               ab2_count=np.asarray([len(deep)]), both_walls=fl[:, 0], adjacent=fl[:, 1], diagonal=fl[:, 2])
    path = os.path.join(REPO, "tests", "golden", f"ab_walls_{board}x{board}.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, len(states), "states,", len(deep), "at depth 2,", f"{time.time() - t0:.0f}s")


if __name__ == "__main__":
    main()
