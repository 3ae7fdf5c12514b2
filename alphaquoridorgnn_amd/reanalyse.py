"""Reanalyse -- the replay window's targets refreshed by a fresh search with the newest network (MuZero's Reanalyse; neither the
reference nor AlphaZero has it).  A row's policy target is the visit row of the network that played it; with K generations in the
window most rows were labelled by networks up to K promotions old.  One pass searches R stored positions again and overwrites their
policy targets (and, with a blend, pulls their value targets towards the new search value).

Everything runs on the device: the rows' 72-byte records are gathered from the ring, searched from fresh trees G at a time
(BatchedSelfPlay.search on the engine pv_mcts keeps for searches), read out (root_visits, root_values) and written into their slots
by one aqg_replay_refresh launch per chunk (ReplayWindow.refresh_counts).  The newest generation is never touched: its targets are
the current network's already.

policy_target='completed_q' (Danihelka et al., "Policy improvement by planning with Gumbel", ICLR 2022; include/aqgnn.h, "completed-Q
policy targets"): the policy target is pi' = softmax(log p + sigma(completedQ)) of the searched root instead of its normalised visit
counts -- non-zero on unvisited actions and smooth in the values, which matters at the small simulation counts a pass runs at.  The
read-out pair becomes root_improved_policy -> ReplayWindow.refresh_policy; the search itself is the same.
"""
import torch

from . import pv_mcts
from .replay import check_value_blend, draw_reanalyse_rows
from .selfplay_options import check_policy_target


def eligible_rows(window):
    """Rows of `window` a pass may refresh: every valid row except the newest generation's -- the first eligible_rows of index()."""
    generations = window.generations
    return len(window) - generations[-1] if generations else 0


def check_reanalyse_options(rows, sims=None, value_blend=0.0, slots=None, policy_target="visits", c_visit=50.0, c_scale=1.0):
    """Validate the options of a pass as reanalyse() does: rows >= 0, sims >= 1 (None: the default), a blend in [0, 1], slots >= 1,
    policy_target 'visits' or 'completed_q' with c_visit and c_scale finite and >= 0 (selfplay_options.check_policy_target returns
    those three).  Returns (rows, sims, value_blend, slots) as ints / float."""
    check_policy_target(policy_target, c_visit, c_scale)
    for name, x, low in (("rows", rows, 0), ("sims", sims, 1), ("slots", slots, 1)):
        if x is None:
            continue
        if isinstance(x, bool) or int(x) != x or int(x) < low:
            raise ValueError(f"reanalyse: {name} must be an integer >= {low}, not {x!r}")
    return (int(rows), None if sims is None else int(sims), check_value_blend(value_blend), None if slots is None else int(slots))


def reanalyse(window, model, rows, sims=None, value_blend=0.0, seed=0, update=0, slots=2048, evaluator=None, fake_bias=0,
              policy_target="visits", c_visit=50.0, c_scale=1.0):
    """Search `rows` of the window's rows again with `model` and overwrite their targets; returns how many were refreshed.

    Eligible are the valid rows except the newest generation, index()[: len(window) - generations[-1]]; draw_reanalyse_rows(seed,
    update, eligible, rows) picks R = min(rows, eligible) of them.  Their records are searched in chunks of min(R, slots) roots at
    `sims` simulations (None: pv_mcts.PV_EVALUATE_COUNT) on one search engine -- no history, no self-play option, fresh trees; the
    last chunk is padded with copies of its first record, whose results are dropped -- and after each chunk one refresh_counts
    writes pi = visits / their sum into the rows' slots and, with value_blend L > 0, z' = (1 - L) z + L q with q the root's search
    value and z the value the ring holds now.  evaluator None: by the model, as self_play() chooses ('cnn', 'gnn', 'general');
    'fake' (tests) takes fake_bias.  policy_target 'completed_q': after each chunk root_improved_policy(c_visit, c_scale) and one
    refresh_policy write pi' = softmax(log p + sigma(completedQ)) instead; q of the blend stays root_values().  The search is
    deterministic: two windows with equal rings stay equal under equal calls.
    The engine is dropped when the pass is done, so its tree pool does not stay resident beside a self-play engine's."""
    from .pv_network_cnn import CNNNetwork
    rows, sims, value_blend, slots = check_reanalyse_options(rows, sims, value_blend, slots, policy_target, c_visit, c_scale)
    policy_target, c_visit, c_scale = check_policy_target(policy_target, c_visit, c_scale)
    sims = pv_mcts.PV_EVALUATE_COUNT if sims is None else sims
    N = window.board_size
    if evaluator is None:
        evaluator = "cnn" if isinstance(model, CNNNetwork) else "gnn" if getattr(model, "fused", True) else "general"
    if getattr(model, "board_size", N) != N:
        raise ValueError(f"reanalyse: the model is of a {model.board_size}x{model.board_size} board, the window of a {N}x{N} one")
    eligible = eligible_rows(window)
    if rows == 0 or eligible <= 0:
        return 0
    positions = draw_reanalyse_rows(seed, update, eligible, rows)
    R = int(positions.shape[0])
    chosen = window.index()[torch.from_numpy(positions).to(window.device)]      # ring slots, in age order
    records = window.tensors()[0].index_select(0, chosen)
    chunk = min(R, slots)
    eng = pv_mcts._engine_for(model, chunk, sims, N, evaluator, fake_bias)
    try:
        if eng.N != N:
            raise ValueError(f"reanalyse: the engine is of a {eng.N}x{eng.N} board, the window of a {N}x{N} one")
        records = records.to(eng.dev)
        for first in range(0, R, chunk):
            roots = records[first:first + chunk]
            m = int(roots.shape[0])
            if m < chunk:
                roots = torch.cat((roots, roots[:1].expand(chunk - m, 72)))
            visits, actions, count = eng.search(roots)
            q = eng.root_values()
            if policy_target == "completed_q":
                policy, actions, count, _ = eng.root_improved_policy(c_visit, c_scale)
                window.refresh_policy(chosen[first:first + m], policy[:m], actions[:m], count[:m], search_value=q[:m], value_blend=value_blend)
            else:
                window.refresh_counts(chosen[first:first + m], visits[:m], actions[:m], count[:m], search_value=q[:m], value_blend=value_blend)
    finally:
        pv_mcts._drop_engine(eng)
    return R
