"""Host statement of self-play with resignation (include/aqgnn.h, "resignation") -- shared by test_resign_cpu.py and test_resign.py.
`play_game` is oracle.mcts.play's loop with the rule of the option, built from the oracle's PV-MCTS pieces the way tests/_tree_reuse.py
builds its statement (whose search, tree-reuse and root-noise pieces it takes, so that the options combine as they do on the device).
The case lists of the GPU tests live here too, so that the CPU test can assert what they contain."""
import functools
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from oracle import mcts as om, quoridor as oq   # noqa: E402
from tests import _tree_reuse as T   # noqa: E402
from tests._util import MAX_LEGAL   # noqa: E402

INF = np.float32(np.inf)


def uniform_scalar(seed, k):
    """counter_uniform(stream_key(seed, k), 0) on Python ints: the scalar restatement of the enabled / disabled draw."""
    M = (1 << 64) - 1
    G = 0x9E3779B97F4A7C15

    def mix(z):
        z &= M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)
    key = mix((seed & M) + G * (k + 1))
    return (mix(key + G) >> 11) * 2.0 ** -53


def resign_value(root, visits):
    """m = max(v_root, v_best) in float32: the root's w / n from the mover's side, and q of the child at the first maximum of the
    visit counts (-w_c / n_c, 0 without a visit)."""
    v_root = np.float32(root.w / root.n) if root.n else np.float32(0.0)
    c = root.children[int(np.argmax(visits))]
    v_best = np.float32(-c.w / c.n) if c.n else np.float32(0.0)
    return np.float32(max(v_root, v_best))


def play_game(N, sims, uniforms, threshold=None, min_ply=0, enabled=True, bias=2, keep_visits=None, temperature_plies=0, noise=None,
              eps=None):
    """One game (threshold None = the option off: oracle.mcts.play's loop, or tests/_tree_reuse.play_game's with its options).
    Returns (rows, z, resigned, minima): per ply dict(rec, visits dense int16 [A], action -- 0xFF on the resigning row --, value
    float32 = root.w / root.n), the first player's value, whether the game ended by resignation, and the running minimum of m per side,
    float32 [2] from +inf, over the searched plies >= min_ply."""
    from tests.test_root_noise_cpu import mix_statement
    model, state, rows, clock = om.FakeModel(bias), oq.State(N=N), [], T.Clock()
    root, kept = T.Node(state, 0), False
    A = T.action_count(N)
    minima = np.array([INF, INF], dtype=np.float32)
    thr = None if threshold is None else np.float32(threshold)
    while not state.is_done():
        ply = state.plies_played
        first_priors = None
        if noise is not None:
            if kept:
                mixed = mix_statement(np.asarray([c.p for c in root.children], dtype=np.float32), noise[ply], eps)
                for c, p in zip(root.children, mixed):
                    c.p = p
            else:
                first_priors = lambda p, ply=ply: mix_statement(p, noise[ply], eps)      # noqa: E731
        T.search_from(model, root, sims, clock, first_priors)
        visits = [c.n for c in root.children]
        legal = state.legal_actions()
        draw = om.choice_index(om.boltzman(visits, 1.0), uniforms[ply])
        idx = draw if not (temperature_plies and ply >= temperature_plies) else int(np.argmax(visits))
        dense = np.zeros(A, dtype=np.int16)
        dense[list(legal)] = visits
        row = dict(rec=state.rec.copy(), visits=dense, action=int(legal[idx]), value=np.float32(root.w / root.n), kept=kept)
        rows.append(row)
        if thr is not None and ply >= min_ply:
            m = resign_value(root, visits)
            minima[ply & 1] = min(minima[ply & 1], m)
            if enabled and m < -thr:
                row["action"] = 0xFF
                return rows, (-1 if ply % 2 == 0 else 1), True, minima
        child = root.children[idx]
        state = child.state
        kept = keep_visits is not None and T.keeps(child, state.is_done(), keep_visits)
        root = T.reroot(child) if kept else T.Node(state, 0)
    return rows, om.first_player_value(state), False, minima


# ------------------------------------------------------------------ the cases of the GPU tests
THRESHOLD = 0.25
SIMS = 16
G = 8
RESIGN_SEED = 2024


def uniforms_of(N, G=G):
    from alphaquoridorgnn_amd.constants import board_params
    return np.random.RandomState(700 + N).random_sample(size=(G, board_params(N)[1]))


@functools.lru_cache(maxsize=None)
def generation(N, threshold=THRESHOLD, min_ply=0, disable_fraction=0.0, seed=RESIGN_SEED, G=G, sims=SIMS, keep=None, K=0, noise_seed=None,
               eps=None):
    """G games of the statement: game g drawn with uniforms_of(N)[g], enabled by the scalar draw of (seed, g).  Returns a dict of the
    rows in game order, the per-game records and the per-game lists (`games`)."""
    u = uniforms_of(N, G)
    tables = None
    if noise_seed is not None:
        tables = np.random.RandomState(noise_seed).randint(1, 1025, size=(u.shape[1], G, MAX_LEGAL)).astype(np.float64)
    enabled = [threshold is not None and uniform_scalar(seed, g) >= disable_fraction for g in range(G)]
    S, V, Z, ACT, Q, games = [], [], [], [], [], []
    plies, result, resigned, minima = [], [], [], []
    for g in range(G):
        rows, z0, res, lo = play_game(N, sims, u[g], threshold, min_ply, enabled[g], keep_visits=keep, temperature_plies=K,
                                      noise=None if tables is None else tables[:, g], eps=eps)
        games.append(rows)
        plies.append(len(rows)); result.append(z0); resigned.append(res); minima.append(lo)
        for ply, r in enumerate(rows):
            S.append(r["rec"]); V.append(r["visits"]); ACT.append(r["action"]); Q.append(r["value"])
            Z.append(z0 if ply % 2 == 0 else -z0)
    return dict(u=u, tables=tables, enabled=np.asarray(enabled), states=np.stack(S), visits=np.stack(V), z=np.asarray(Z, dtype=np.int8),
                actions=np.asarray(ACT, dtype=np.uint8), values=np.asarray(Q, dtype=np.float32), plies=np.asarray(plies, dtype=np.int32),
                result=np.asarray(result, dtype=np.int8), resigned=np.asarray(resigned, dtype=np.uint8),
                minima=np.stack(minima).astype(np.float32), games=games)


def game_rows_of(want, k):
    """One game of a generation in the layout of test_resign._game_rows."""
    rows = want["games"][k]
    return (int(want["plies"][k]), int(want["result"][k]), int(want["resigned"][k]), want["minima"][k].tobytes(),
            np.stack([r["rec"] for r in rows])[:, :70].tobytes(), np.stack([r["visits"] for r in rows]).tobytes(),
            np.asarray([r["action"] for r in rows], dtype=np.uint8).tobytes(),
            np.asarray([r["value"] for r in rows], dtype=np.float32).tobytes())
