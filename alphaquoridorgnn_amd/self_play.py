"""Self-play -- drop-in for the reference's self_play.py, running whole generations on the batched HIP engine.

Call surface kept (self_play.py:19-95): SP_GAME_COUNT, SP_TEMPERATURE, first_player_value, write_data, play,
self_play.  `self_play()` plays SP_GAME_COUNT games CONCURRENTLY on this rank's GPU (sharded over ranks when
torch.distributed is initialised: rank r plays its share, then one all-gather of (s, pi, z) over RCCL/xGMI and
rank 0 writes the single history file, like self_play.py:84,:91).
"""
import os
import pickle
from datetime import datetime

import numpy as np
import torch

from . import distributed as aqd
from . import pv_mcts
from .constants import PV_NETWORK_PATH, BOARD_SIZE
from .engine import BatchedSelfPlay, MultiSetSelfPlay, gather_history, gather_resign_arrays
from .pv_network_gnn import GNNNetwork, POLICY_OUTPUT_SIZE, load_network
from .pv_network_cnn import CNNNetwork
from .reanalyse import check_reanalyse_options, eligible_rows, reanalyse
from .selfplay_options import check_policy_record, check_policy_target, check_value_lambda
from .replay import blend_targets, check_value_blend
from .resign_calibration import resign_stats_of, suggest_from_arrays

SP_GAME_COUNT = 50    # Number of games for self-play (self_play.py:19; 25000 in the original version)
SP_TEMPERATURE = 1.0  # Temperature parameter for Boltzmann distribution (self_play.py:20)
# Root exploration noise (the reference has none; engine.BatchedSelfPlay): p' = (1 - eps) p + eps Dir(alpha) at every move's root.
SP_ROOT_NOISE_EPS = 0.0      # 0 = off: the reference's games
SP_ROOT_NOISE_ALPHA = None   # None = 10 / (N^2 + 2 (N - 1)^2), the "10 / typical number of moves" rule
# Training targets (the reference has neither; engine.BatchedSelfPlay, replay.blend_targets).  SP_TEMPERATURE_PLIES K > 0: plies 0 .. K - 1
# of a game are sampled at SP_TEMPERATURE, every later one takes the most visited move.  SP_VALUE_BLEND L > 0: a row's value target is
# (1 - L) z + L q, q the search value of its root -- a float32 in the window and, with the same bits, a float in the .history file.
SP_TEMPERATURE_PLIES = 0     # 0 = off: every ply at SP_TEMPERATURE
SP_VALUE_BLEND = 0.0         # 0 = off: z alone, an int
# SP_VALUE_LAMBDA X in [0, 1] (needs SP_VALUE_BLEND > 0; include/aqgnn.h "lambda-return value targets"): q in that target becomes the
# lambda-return G of the game's later search values, G_t = (1 - X) q_t + X (-G_{t+1}), bootstrapped into the outcome -- q at 0, z at 1.
SP_VALUE_LAMBDA = None       # None = off: q is the search value of the row's own root, and no launch is added
# Tree reuse (the reference has none; engine.BatchedSelfPlay, include/aqgnn.h "tree reuse"): the next move's search starts from the chosen
# child's subtree when that holds at most SP_TREE_REUSE_VISITS visits (None = the simulation count) and runs the same simulations on top.
SP_TREE_REUSE = False        # off: a fresh tree every move, the reference's search
SP_TREE_REUSE_VISITS = None
# Resignation (the reference has none; engine.BatchedSelfPlay, include/aqgnn.h "resignation"): a mover whose search value and most visited
# child's value are both below -SP_RESIGN_THRESHOLD at a ply >= SP_RESIGN_MIN_PLY gives the game up; a share SP_RESIGN_DISABLE_FRACTION of
# the games never resigns, and from those the false positives are counted.  'auto': the first generation only collects (every game is
# played out), and after each generation the next threshold is engine.suggest_resign_threshold at SP_RESIGN_MAX_FALSE_POSITIVE over the
# newest SP_RESIGN_WINDOW generations' statistics (SP_RESIGN_AUTO holds them; no suggestion = the next generation collects again).
SP_RESIGN_THRESHOLD = None   # None = off: every game is searched to its rule end; a float in (0, 1]; or 'auto'
SP_RESIGN_MIN_PLY = 0
SP_RESIGN_DISABLE_FRACTION = 0.1
SP_RESIGN_MAX_FALSE_POSITIVE = 0.05
SP_RESIGN_WINDOW = 8
SP_RESIGN_AUTO = {"threshold": None, "parts": []}
SP_RESIGN_LAST = None        # the last generation's dict(threshold, stats, arrays, next_threshold), gathered over the ranks
# Slots (SP_SLOTS G, None = one slot per game: a finished slot idles until the longest game ends): the rank's games run on G slots with
# the engine's refill, so that a slot freed by a short -- or a resigned -- game takes the next one.
SP_SLOTS = None
# Replay window (the reference has none; replay.ReplayWindow): every rank appends the gathered generation to SP_REPLAY, straight from
# the engine's device tensors, for train_network.TRAIN_WINDOW to train on.  The .history file stays the reference's hand-over.
SP_REPLAY = None             # None = off
SP_WRITE_HISTORY = True      # False (needs a window): rank 0 writes no file
# Reanalyse (the reference has none; reanalyse.reanalyse, include/aqgnn.h "reanalyse"): after the generation is appended, every rank
# searches SP_REANALYSE_ROWS of the window's older rows again with the model that just played and overwrites their targets.  The
# .history file never changes: it holds the generation as it was played.
SP_REANALYSE_ROWS = 0        # 0 = off: no search engine is built
SP_REANALYSE_SIMS = None     # None = pv_mcts.PV_EVALUATE_COUNT
SP_REANALYSE_VALUE_BLEND = 0.0      # L in [0, 1]: a refreshed row's value target becomes (1 - L) z + L q of the fresh search; 0 = z stays
SP_REANALYSE_SLOTS = 2048    # roots searched at once
# how a refreshed row's policy target is formed: 'visits' = the normalised visit counts; 'completed_q' = the improved policy
# softmax(log p + sigma(completedQ)) of the searched root (include/aqgnn.h "completed-Q policy targets"), with the transform's constants
SP_REANALYSE_POLICY_TARGET = 'visits'
SP_REANALYSE_C_VISIT = 50.0
SP_REANALYSE_C_SCALE = 1.0
# The policy target of the generation's OWN rows (the reference has one: the normalised visit counts; engine.BatchedSelfPlay, include/aqgnn.h
# "recording completed-Q targets during self-play"): 'completed_q' records the improved policy softmax(log p + sigma(completedQ)) of every
# searched root as a float32 row, which the window takes verbatim and the .history file holds widened to Python floats (float32(float(x))
# gives the bits back).  The move is still chosen from the visit counts.  With root noise on, p is the MIXED prior.
SP_POLICY_TARGET = 'visits'  # the reference's rows
SP_POLICY_C_VISIT = 50.0
SP_POLICY_C_SCALE = 1.0
# Gumbel root search (the reference has none; engine.BatchedSelfPlay, include/aqgnn.h "Gumbel root search"): every root samples
# SP_GUMBEL_CONSIDERED actions without replacement, spends the simulations on them by sequential halving and plays the survivor.  The
# matching policy target is the completed-Q row: SP_POLICY_TARGET must be 'completed_q' (a visit row is no target under halving).
SP_GUMBEL_CONSIDERED = 0     # 0 = off: PUCT at the root and a draw from the visit counts
SP_GUMBEL_SCALE = 1.0        # factor on the Gumbel variates; 0 = a deterministic search
SP_GUMBEL_SEED = None        # None = derived from the generation's seed
# Forked self-play (the reference has none; openings.fork_table, include/aqgnn.h "start positions"): a share of every generation's games
# starts from positions the replay window already holds instead of from the opening record.  Which games, and from which row, is drawn
# per (seed, generation, game index over all ranks): every rank builds the same table from its own window, with no collective.
SP_START_FROM_WINDOW_SHARE = 0.0     # 0 = off (or an empty window): no table is built and every call is the one made today
SP_FORKED_LAST = 0                   # games of the last generation that started from a window row, over all ranks


def first_player_value(ended_state):
    """1: first player wins, -1: first player loses, 0: draw (self_play.py:22-27)."""
    if ended_state.is_lose():
        return -1 if ended_state.is_first_player() else 1
    return 0


def write_data(history):
    """Save training data to ./data/YYYYMMDDhhmmss.history (self_play.py:30-37)."""
    now = datetime.now()
    os.makedirs('./data/', exist_ok=True)
    path = './data/{:04}{:02}{:02}{:02}{:02}{:02}.history'.format(
        now.year, now.month, now.day, now.hour, now.minute, now.second)
    with open(path, mode='wb') as f:
        pickle.dump(history, f)
    return path


def _history_rows(states72, visits, z, board_size, values=None, value_blend=0.0, policy=None):
    """The rows of a .history file.  values (float32 [P], with value_blend > 0): a row's z is the blended target as a Python float --
    the float32 the replay window holds, widened -- instead of the int outcome.  policy (float32 [P, A], engine.history_policies): a
    row's policy is the recorded row widened to Python floats instead of the normalised visit counts."""
    nw = (board_size - 1) ** 2
    st, vis, zz = states72.cpu().numpy(), visits.cpu().numpy().astype(np.float64), z.cpu().numpy()
    if values is not None:
        zz = [float(x) for x in blend_targets(zz, values.cpu().numpy(), value_blend)]
    rec = None if policy is None else policy.cpu().numpy().astype(np.float64)
    out = []
    for i, (s, v, r) in enumerate(zip(st, vis, zz)):
        tot = v.sum()
        pol = rec[i].tolist() if rec is not None else (v / tot).tolist() if tot > 0 else [0.0] * v.shape[0]
        out.append([[[int(s[0]), int(s[1])], [int(s[2]), int(s[3])], [int(x) for x in s[4:4 + nw]]], pol,
                    int(r) if values is None else r])
    return out


def mirror_history(history):
    """The rows of a history followed by their left-right mirrors, in the .history schema [[player, enemy, walls], policy, z] -- on
    the host, so that write_data(mirror_history(h)) is an augmented file the reference's own train_network.py can read.  The board
    size is that of the walls list; z is unchanged and a policy is permuted, out[mirror(a)] = in[a]."""
    from .game_logic import mirror_actions, mirror_record, pack_state72
    out = list(history)
    for (player, enemy, walls), pol, z in history:
        N = int(round(len(walls) ** 0.5)) + 1
        if (N - 1) ** 2 != len(walls) or len(pol) != N * N + 2 * (N - 1) ** 2:
            raise ValueError("mirror_history: a row's walls and policy are not those of one board size")
        m = mirror_record(pack_state72(player, enemy, walls, 0, N))
        src = mirror_actions(np.arange(len(pol)), N)
        out.append([[[int(m[0]), int(player[1])], [int(m[2]), int(enemy[1])], [int(x) for x in m[4:4 + len(walls)]]],
                    [pol[a] for a in src], z])
    return out


def _resign_options():
    """(keyword arguments of the engine for this generation, the threshold they play at) -- ({}, None) when the option is off."""
    if SP_RESIGN_THRESHOLD is None:
        return {}, None
    if SP_RESIGN_THRESHOLD == "auto":
        chosen = SP_RESIGN_AUTO["threshold"]
        # collecting: nothing resigns and every game counts as played out
        thr, frac = (1.0, 1.0) if chosen is None else (chosen, SP_RESIGN_DISABLE_FRACTION)
    else:
        thr, frac = SP_RESIGN_THRESHOLD, SP_RESIGN_DISABLE_FRACTION
    return dict(resign_threshold=thr, resign_min_ply=SP_RESIGN_MIN_PLY, resign_disable_fraction=frac), thr


def _after_resign_generation(arrays, threshold, rank):
    """The statistics of one generation, already gathered: remembered in SP_RESIGN_LAST, printed on rank 0, and with 'auto' turned
    into the next generation's threshold.  Every rank holds the same arrays and therefore takes the same decision."""
    global SP_RESIGN_LAST
    stats = resign_stats_of([arrays], threshold)
    nxt = None
    if SP_RESIGN_THRESHOLD == "auto":
        parts = SP_RESIGN_AUTO["parts"]
        parts.append(arrays)
        del parts[:-SP_RESIGN_WINDOW]
        nxt = SP_RESIGN_AUTO["threshold"] = suggest_from_arrays(parts, SP_RESIGN_MAX_FALSE_POSITIVE)      # None: collect again
    SP_RESIGN_LAST = dict(threshold=threshold, stats=stats, arrays=arrays, next_threshold=nxt)
    if rank == 0:
        games = max(stats["games"], 1)
        print(f'resignation: threshold {threshold:.4f}, {stats["games_resigned"]}/{stats["games"]} games resigned, '
              f'{stats["plies"] / games:.1f} plies per game; played out: {stats["disabled_games"]} games, {stats["would_resign"]} sides '
              f'would have resigned, {stats["false_positives"]} of them did not lose (false-positive rate '
              f'{stats["false_positive_rate"]:.3f})'
              + ('' if SP_RESIGN_THRESHOLD != "auto" else
                 f'; next threshold: {"none (the next generation only collects)" if nxt is None else format(nxt, ".4f")}'))


def _gumbel_options(target):
    """The engine's keyword arguments of the Gumbel root search -- {} when it is off; refused without the completed-Q target."""
    if not SP_GUMBEL_CONSIDERED:
        return {}
    if target != "completed_q":
        raise ValueError("SP_GUMBEL_CONSIDERED needs SP_POLICY_TARGET = 'completed_q': a visit row is not a policy target under "
                         "sequential halving")
    return dict(gumbel_considered=SP_GUMBEL_CONSIDERED, gumbel_scale=SP_GUMBEL_SCALE, gumbel_seed=SP_GUMBEL_SEED)


def _value_lambda(blend):
    """SP_VALUE_LAMBDA as a float, or None when it is off; refused without a value blend, because nothing would read it."""
    if SP_VALUE_LAMBDA is None:
        return None
    lam = check_value_lambda(SP_VALUE_LAMBDA)
    if not blend > 0.0:
        raise ValueError("SP_VALUE_LAMBDA needs SP_VALUE_BLEND > 0: the lambda-return takes the place of q in (1 - L) z + L q")
    return lam


def _search_values(eng, lam):
    """The q of the blended value target, row-aligned with the engine's history: the rows' own search values, or with a lambda their
    lambda-returns (one more launch)."""
    return eng.history_values() if lam is None else eng.history_lambda_values(lam)


def play(model, device=None, uniforms=None):
    """Execute one self-play game (self_play.py:40-68) -- a generation of one game on the engine.
    Returns [[state_array, policy list[POLICY_OUTPUT_SIZE], z], ...]."""
    blend = check_value_blend(SP_VALUE_BLEND)
    lam = _value_lambda(blend)
    target, c_visit, c_scale = check_policy_record(SP_POLICY_TARGET, SP_POLICY_C_VISIT, SP_POLICY_C_SCALE)
    eng = BatchedSelfPlay(model, num_games=1, sims=pv_mcts.PV_EVALUATE_COUNT, board_size=BOARD_SIZE,
                          temperature=SP_TEMPERATURE, seed=int(np.random.randint(0, 2 ** 31 - 1)),
                          evaluator=pv_mcts.evaluator_of(model), root_noise_eps=SP_ROOT_NOISE_EPS,
                          root_noise_alpha=SP_ROOT_NOISE_ALPHA, temperature_plies=SP_TEMPERATURE_PLIES,
                          record_search_value=blend > 0.0, tree_reuse=SP_TREE_REUSE, tree_reuse_visits=SP_TREE_REUSE_VISITS,
                          policy_target=target, policy_c_visit=c_visit, policy_c_scale=c_scale, **_resign_options()[0],
                          **_gumbel_options(target))
    eng.play_generation(uniforms=uniforms, check_every=1)
    if blend > 0.0:
        return _history_rows(*eng.history_tensors(), BOARD_SIZE, _search_values(eng, lam), blend,
                             policy=eng.history_policies() if target == "completed_q" else None)
    return eng.history()


def _fresh_seed():
    """Base seed of one self_play() call.  The reference draws every move from the unseeded global numpy RNG
    (self_play.py:57), so two generations never repeat; here the engine's uniform stream is seeded per call from
    the same global RNG (or from AQG_SELFPLAY_SEED for reproducible runs).  Under torch.distributed rank 0's draw
    is broadcast, and every rank adds its rank, so the ranks' streams differ and a rerun with the same override
    reproduces the same generation."""
    import torch.distributed as dist
    env = os.environ.get("AQG_SELFPLAY_SEED")
    seed = int(env) if env is not None else int(np.random.randint(0, 2 ** 31 - 1))
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        t = torch.tensor([seed], dtype=torch.int64, device=aqd.collective_device())
        dist.broadcast(t, src=0)
        seed = int(t.item())
    return seed


def self_play(model=None, games=None, seed=None):
    """Perform self-play games and save the training data (self_play.py:71-95).  `seed` (tests) fixes the uniform
    stream; by default every call draws a fresh one, like the reference's unseeded np.random.choice."""
    import torch.distributed as dist
    if not SP_WRITE_HISTORY and SP_REPLAY is None:
        raise ValueError("SP_WRITE_HISTORY = False without a replay window (SP_REPLAY) would throw the generation away")
    reanalyse_rows = check_reanalyse_options(SP_REANALYSE_ROWS, SP_REANALYSE_SIMS, SP_REANALYSE_VALUE_BLEND, SP_REANALYSE_SLOTS,
                                             SP_REANALYSE_POLICY_TARGET, SP_REANALYSE_C_VISIT, SP_REANALYSE_C_SCALE)[0]
    if reanalyse_rows and SP_REPLAY is None:
        raise ValueError("SP_REANALYSE_ROWS > 0 needs a replay window (SP_REPLAY): there is no older row to search again")
    target, c_visit, c_scale = check_policy_record(SP_POLICY_TARGET, SP_POLICY_C_VISIT, SP_POLICY_C_SCALE)
    blend = check_value_blend(SP_VALUE_BLEND)
    lam = _value_lambda(blend)
    gumbel_kw = _gumbel_options(target)
    if model is None:
        model = load_network(PV_NETWORK_PATH + 'best.pth')       # GNNNetwork (prep_for_inference's path), or the network best.pth holds
        if isinstance(model, (GNNNetwork, CNNNetwork)) and torch.cuda.is_available():
            model.packed_weights(torch.device("cuda", torch.cuda.current_device()))
    # by the trunk alone (model.fused, whatever the policy head: a caller's model need not come from a file): 6/128/3 runs the fused evaluator; any other shape the any-shape one; the CNN its own
    evaluator = "cnn" if isinstance(model, CNNNetwork) else "gnn" if getattr(model, "fused", True) else "general"
    total = SP_GAME_COUNT if games is None else games
    distributed = dist.is_available() and dist.is_initialized()
    rank, world = (dist.get_rank(), dist.get_world_size()) if distributed else (0, 1)
    base = _fresh_seed() if seed is None else int(seed)
    mine = total // world + (1 if rank < total % world else 0)
    dev = aqd.device()                                   # this rank's GPU (LOCAL_RANK under torchrun), never a bare 'cuda'
    st = torch.zeros((0, 72), dtype=torch.uint8, device=dev)
    vis = torch.zeros((0, POLICY_OUTPUT_SIZE), dtype=torch.int16, device=dev)
    z = torch.zeros((0,), dtype=torch.int8, device=dev)
    q = torch.zeros((0,), dtype=torch.float32, device=dev) if blend > 0.0 else None       # the rows' search values, with a blend only
    pol = torch.zeros((0, POLICY_OUTPUT_SIZE), dtype=torch.float32, device=dev) if target == "completed_q" else None      # the recorded targets
    resign_kw, resign_thr = _resign_options()
    resign_arrays = None
    # forked self-play: the table of the whole generation, and this rank's slice of its index (the ranks' games are numbered through)
    global SP_FORKED_LAST
    from .openings import check_window_share, fork_table
    SP_FORKED_LAST, start_kw = 0, {}
    if check_window_share(SP_START_FROM_WINDOW_SHARE) > 0.0 and SP_REPLAY is not None:
        forked = fork_table(SP_REPLAY, total, SP_START_FROM_WINDOW_SHARE, base, SP_REPLAY.fork_updates)
        SP_REPLAY.fork_updates += 1
        if forked is not None:
            first = sum(total // world + (1 if r < total % world else 0) for r in range(rank))
            start_kw = dict(start_states=forked[0], start_index=forked[1][first:first + mine])
            SP_FORKED_LAST = int((forked[1] > 0).sum())
    slots = mine
    if SP_SLOTS is not None:
        if isinstance(SP_SLOTS, bool) or int(SP_SLOTS) != SP_SLOTS or int(SP_SLOTS) < 1:
            raise ValueError(f"SP_SLOTS must be an integer >= 1, not {SP_SLOTS!r}")
        slots = min(int(SP_SLOTS), mine)
    if mine > 0:
        # >= 256 games: independent game sets on their own streams fill the holes of each other's serial kernel chains
        eng = MultiSetSelfPlay(model, num_games=slots, quota=mine, sims=pv_mcts.PV_EVALUATE_COUNT, num_sets=None if slots >= 256 else 1,
                               board_size=BOARD_SIZE, temperature=SP_TEMPERATURE, seed=(base + rank) % (2 ** 31 - 1), device=dev,
                               evaluator=evaluator, root_noise_eps=SP_ROOT_NOISE_EPS, root_noise_alpha=SP_ROOT_NOISE_ALPHA,
                               temperature_plies=SP_TEMPERATURE_PLIES, record_search_value=blend > 0.0,
                               tree_reuse=SP_TREE_REUSE, tree_reuse_visits=SP_TREE_REUSE_VISITS,
                               policy_target=target, policy_c_visit=c_visit, policy_c_scale=c_scale, **resign_kw, **start_kw, **gumbel_kw)
        c = eng.play_generation()
        print(f'\rSelf-play (rank {rank}: {c["finished"]}/{mine} games, policy target: {target}'
              + (f', search: Gumbel root, {SP_GUMBEL_CONSIDERED} considered' if gumbel_kw else ', search: PUCT')
              + (f', value lambda: {lam:g}' if lam is not None else '')
              + (f', {SP_FORKED_LAST}/{total} games forked from the window' if start_kw else '') + ')', end='')
        st, vis, z = eng.history_tensors()
        if q is not None:
            q = _search_values(eng, lam)
        if pol is not None:
            pol = eng.history_policies()
        if resign_thr is not None:
            resign_arrays = eng.resign_arrays()
        del eng                                          # its tree pools go before a reanalyse pass builds its search engine
    if distributed and os.environ.get("AQG_DIST_LOG") == "1" and rank == 0:
        print(f'exchange step: backend={dist.get_backend()} world={world} collectives={"forced" if aqd.force_group() else "as needed"}')
    host = distributed and dist.get_backend() != 'nccl'      # gloo (CPU tests): the exchange runs on host tensors
    if host:
        st, vis, z = st.cpu(), vis.cpu(), z.cpu()
    if host and pol is not None:
        pol = pol.cpu()
    if q is not None:
        st, vis, z, q, *rest = gather_history(st, vis, z, values=q.cpu() if host else q, policies=pol)
    else:
        st, vis, z, *rest = gather_history(st, vis, z, policies=pol)
    if pol is not None:
        pol = rest[0]
    print('')
    if resign_thr is not None:
        _after_resign_generation(gather_resign_arrays(resign_arrays, device="cpu" if host or not distributed else dev), resign_thr, rank)
    if SP_REPLAY is not None:                        # every rank: the gathered rows are identical on all of them
        if pol is not None:
            SP_REPLAY.append_policy(st, pol, z, search_value=q, value_blend=blend if q is not None else 0.0)
        elif q is not None:
            SP_REPLAY.append_counts(st, vis, z, search_value=q, value_blend=blend)
        else:
            SP_REPLAY.append_counts(st, vis, z)
    if reanalyse_rows:
        # every rank searches the same rows (the seed is the call's base seed, not base + rank) and the search is deterministic: the
        # ranks' windows stay identical without a collective
        sims = pv_mcts.PV_EVALUATE_COUNT if SP_REANALYSE_SIMS is None else SP_REANALYSE_SIMS
        done = reanalyse(SP_REPLAY, model, reanalyse_rows, sims=sims, value_blend=SP_REANALYSE_VALUE_BLEND, seed=base,
                         update=SP_REPLAY.reanalyse_updates, slots=SP_REANALYSE_SLOTS, evaluator=evaluator,
                         policy_target=SP_REANALYSE_POLICY_TARGET, c_visit=SP_REANALYSE_C_VISIT, c_scale=SP_REANALYSE_C_SCALE)
        SP_REPLAY.reanalyse_updates += 1
        if rank == 0:
            print(f'reanalysed {done} of {eligible_rows(SP_REPLAY)} rows at {sims} simulations, policy target: '
                  f'{check_policy_target(SP_REANALYSE_POLICY_TARGET)[0]}')
    path = None
    if rank == 0 and SP_WRITE_HISTORY:
        path = write_data(_history_rows(st, vis, z, BOARD_SIZE, q, blend, policy=pol))
    if distributed:
        dist.barrier()          # no rank may go on to train_network.load_data() before rank 0 has finished the file
    del model
    torch.cuda.empty_cache()
    return path


def main(argv=None):
    """`python -m alphaquoridorgnn_amd.self_play` -- also the per-rank program of
    `python -m torch.distributed.run --nproc-per-node N ... -m alphaquoridorgnn_amd.self_play` (distributed.init_from_env binds
    the rank to its GPU and joins the group; one generation sharded over the ranks, one all-gather, rank 0 writes the file)."""
    import argparse
    ap = argparse.ArgumentParser(description=main.__doc__)
    ap.add_argument("--games", type=int, default=None, help="games of the generation over ALL ranks (default SP_GAME_COUNT)")
    ap.add_argument("--sims", type=int, default=None, help="simulations per move (default pv_mcts.PV_EVALUATE_COUNT)")
    ap.add_argument("--seed", type=int, default=None, help="fix the uniform streams (default: fresh per call, like the reference)")
    ap.add_argument("--root-noise-eps", type=float, default=None, help="weight of the Dirichlet noise at every root (default SP_ROOT_NOISE_EPS = 0: off)")
    ap.add_argument("--root-noise-alpha", type=float, default=None, help="Dirichlet concentration (default SP_ROOT_NOISE_ALPHA: 10 / action count)")
    args = ap.parse_args(argv)
    global SP_ROOT_NOISE_EPS, SP_ROOT_NOISE_ALPHA
    if args.root_noise_eps is not None:
        SP_ROOT_NOISE_EPS = args.root_noise_eps
    if args.root_noise_alpha is not None:
        SP_ROOT_NOISE_ALPHA = args.root_noise_alpha
    aqd.init_from_env()
    if args.sims is not None:
        pv_mcts.PV_EVALUATE_COUNT = args.sims
    try:
        path = self_play(games=args.games, seed=args.seed)
    except BaseException:
        aqd.shutdown(ok=False)
        raise
    aqd.shutdown()
    return path


if __name__ == '__main__':
    main()
