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
from .constants import BOARD_SIZE, board_params, num_actions
from .evaluators import BINDINGS

# The engine's companions, one concern per module, importable from this path as well: the tests, README.md and include/aqgnn.h
# name them as engine.<name>.  counter_rng: the generator of csrc/counter_rng.hpp; selfplay_options: the option checks and the derived
# seeds; device_reference: numpy statements of device code; resign_calibration: the resignation statistics; two_engine_match: the
# match loop.
from .counter_rng import GOLDEN as _GOLDEN, MASK64, mix64 as _mix64_int  # noqa: F401
from .device_reference import (NODE_DTYPE, draw_resign_enabled, draw_root_noise, improved_policy_reference,  # noqa: F401
                               keep_subtree_reference, lambda_values_reference, root_improved_policy_reference, root_noise_stream_key)
from .resign_calibration import resign_false_positives, resign_stats_of, suggest_from_arrays, suggest_resign_threshold  # noqa: F401
from .gumbel import (considered_visits, draw_gumbel, gumbel_logits_reference, gumbel_winner_reference, root_score_reference)  # noqa: F401
from .selfplay_options import (ROOT_NOISE_ATTEMPTS, check_completed_q, check_gumbel, check_policy_record, check_resign, check_root_noise, check_target_options,  # noqa: F401
                               check_start_table, check_temperature, check_tree_reuse, check_value_lambda, default_gumbel_seed, default_resign_seed,
                               default_root_noise_alpha, default_root_noise_seed, set_noise_seeds, set_start_indices)
from .two_engine_match import TwoEngineMatch  # noqa: F401


class BatchedSelfPlay:
    def __init__(self, model=None, num_games=2048, sims=50, board_size=BOARD_SIZE, device=None, temperature=1.0,
                 c_puct=1.25, evaluator="gnn", fake_bias=0, seed=0, record_history=True, quota=None, eval_cache_slots=None,
                 root_noise_eps=0.0, root_noise_alpha=None, root_noise_seed=None, temperature_plies=0, record_search_value=False,
                 tree_reuse=False, tree_reuse_visits=None, resign_threshold=None, resign_min_ply=0, resign_disable_fraction=0.1,
                 resign_seed=None, policy_target="visits", policy_c_visit=50.0, policy_c_scale=1.0, start_states=None, start_index=None,
                 gumbel_considered=0, gumbel_scale=1.0, gumbel_seed=None):
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
        temperature: 1.0 samples the move from the visit counts, 0 takes their first maximum, T > 0 samples from n ** (1 / T); finite
        and >= 0, and log2(sims + tree_reuse_visits) / T <= 1016 so that no term overflows (check_temperature; ValueError otherwise).
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
        T = 1.0 never resigns and only collects.  apply_actions() and search() refuse the option.
        policy_target 'visits' (the default: move() makes the calls it makes today) or 'completed_q' (needs record_history;
        include/aqgnn.h, "recording completed-Q targets during self-play"): every searched move also records the completed-Q improved
        policy of its root, pi' = softmax(log p + sigma(completedQ)) with policy_c_visit and policy_c_scale (finite, >= 0), as a dense
        float32 row beside its visit row -- history_policies(); history() then returns it as the policy list.  One more launch per
        move, between the search and the finish-move launch.  The move is still chosen from the visit counts, under `temperature` and
        temperature_plies, and hist_visits is still written: only the recorded target changes, no game does.  Works with tree reuse
        (a kept root is valid for the read-out), with resignation (the resigning row is written like any other) and with
        evaluator='external'.  With root noise on, the root's stored priors are the MIXED ones, so the target is
        softmax(log p_mixed + sigma): the noise is not taken out again.  apply_actions() and search() refuse the option.
        start_states (None = off, the default: every call is the one made today; include/aqgnn.h, "start positions"): a uint8 [S, 72]
        tensor or array of records the games start from instead of the opening record, copied to the device once.  Game k -- the
        engine's game index, whatever slot plays it -- starts from row start_index[k] (int [quota], each in [0, S)), by default from
        row k % S.  The table goes through the checker here (game_logic.check_states_batch: one device-to-host read, in the
        constructor only) and any flagged row raises ValueError; so does an index that is short, long or out of range.  A start
        record has an even ply counter.  game_plies, the history rows, temperature_plies and resign_min_ply count the plies played in
        the game; the draw rule reads the record's own counter.  reset() and every refill start from the table; search() refuses it.
        gumbel_considered M (0 = off, the default: every call is the one made today; 1..64; include/aqgnn.h, "Gumbel root search"): the
        root samples M actions without replacement (Gumbel top-M over the stored priors), spends the sims - 1 root selections on them
        by sequential halving and move() plays the survivor with the largest g + log p + sigma(q) -- no uniform is consumed and
        `temperature` is not read.  Below the root the search is PUCT as ever.  sigma uses policy_c_visit / policy_c_scale as float32,
        the transform of policy_target='completed_q', which is the matching training target (the visit rows are still written, but a
        visit row is not a target under sequential halving).  gumbel_scale (finite, >= 0; 0 = a deterministic search) multiplies the
        variates; gumbel_seed None = derived from `seed`.  A root's variates are keyed by (seed, game index, ply) -- draw_gumbel is the
        generator in numpy -- unless move() / search() are given a table.  Needs sims >= 2; not with root noise, tree reuse,
        resignation, temperature_plies or evaluator='external' (check_gumbel).  Two launches more per move than the three-launch form;
        the fused step forms (step_heads and the options beside it) do not apply.  root_gumbel() reads the logits out."""
        self.gumbel_options = check_gumbel(gumbel_considered, gumbel_scale, sims, root_noise_eps, tree_reuse, resign_threshold,
                                           temperature_plies, evaluator)
        self.gumbel_seed = default_gumbel_seed(seed) if gumbel_seed is None else int(gumbel_seed) & MASK64
        self.policy_target, self.policy_c_visit, self.policy_c_scale = check_policy_record(policy_target, policy_c_visit, policy_c_scale,
                                                                                           record_history)
        self.resign_options = check_resign(resign_threshold, resign_min_ply, resign_disable_fraction, record_history)
        self.resign_seed = default_resign_seed(seed) if resign_seed is None else int(resign_seed) & MASK64
        self.keep_visits = check_tree_reuse(tree_reuse, tree_reuse_visits, sims, evaluator)
        self.tree_reuse = self.keep_visits is not None
        self.temperature = check_temperature(temperature, sims, self.keep_visits)
        self.temperature_plies, self.record_search_value = check_target_options(temperature_plies, record_search_value, record_history)
        self.root_noise_eps, self.root_noise_alpha = check_root_noise(
            root_noise_eps, default_root_noise_alpha(board_size) if root_noise_alpha is None else root_noise_alpha)
        self.root_noise_seed = default_root_noise_seed(seed) if root_noise_seed is None else int(root_noise_seed) & MASK64
        b = self.binding = BINDINGS[evaluator]
        b.check(model)          # before anything is allocated or launched
        self.dev = _lib.require_gpu(device)
        self.lib = _lib.load()
        self.N = board_size
        self.A = num_actions(board_size)
        self.num_walls, self.plies_for_draw = board_params(board_size)
        self.G, self.sims = int(num_games), int(sims)
        # quota > G: the slots are refilled -- a slot whose game has ended takes the next game not yet handed out (in slot
        # order, deterministic) until `quota` games have been started: the reference's loop over games (self_play.py:81-84)
        # on G concurrent slots instead of lock-step generations that idle every finished slot until the longest game ends
        self.quota = self.G if quota is None else int(quota)
        if self.quota < self.G:
            raise ValueError("quota must be >= num_games")
        start_table = check_start_table(start_states, start_index, self.N, self.quota, self.dev)      # before anything else is allocated
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
        if self.policy_target == "completed_q":
            t["hist_policy"] = z((Q, hp, self.A), torch.float32)    # rows of apply_actions are never written: they read 0
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
        e.c_puct, e.temperature = float(c_puct), self.temperature
        if self.eval_cache_slots:
            e.eval_cache_log2 = self.eval_cache_slots.bit_length() - 1
        e.root_noise_eps, e.root_noise_alpha = self.root_noise_eps, self.root_noise_alpha
        e.root_noise_seed = self.root_noise_seed if self.root_noise_eps else 0      # off: the four fields are zero
        self.reuse = None
        if self.tree_reuse:
            t["kept"] = z((G,), torch.uint8)
            t["child_index"] = torch.full((G,), -1, dtype=torch.int32, device=dev)
            t["stat_moves_kept"] = z((G,), torch.int32)
            t["stat_visits_kept"] = z((G,), torch.int32)
            self.reuse = _lib.TreeReuseStruct()
            self.reuse.keep_visits = self.keep_visits
        self.resign = None
        if self.resign_options:
            t["resign_min"] = torch.full((Q, 2), float("inf"), dtype=torch.float32, device=dev)
            t["game_resigned"] = z((Q,), torch.uint8)
            rs = self.resign = _lib.ResignStruct()
            rs.threshold, rs.min_ply, rs.disable_fraction = self.resign_options
            rs.seed = self.resign_seed
        self.policy_record = None
        if self.policy_target == "completed_q":
            pr = self.policy_record = _lib.PolicyRecordStruct()
            pr.c_visit, pr.c_scale = self.policy_c_visit, self.policy_c_scale
        self.start = None
        if start_table is not None:
            t["start_states72"], index = start_table
            st = self.start = _lib.StartTableStruct()
            st.states72, st.count = t["start_states72"].data_ptr(), t["start_states72"].shape[0]
            if index is not None:
                t["start_index"] = index
                st.index = index.data_ptr()
        self.gumbel = None
        if self.gumbel_options:
            considered, scale = self.gumbel_options
            t["gumbel_schedule"] = torch.from_numpy(considered_visits(considered, self.sims)).to(dev).contiguous()      # uploaded once
            t["gumbel_m"] = z((G,), torch.int32)
            gb = self.gumbel = _lib.GumbelStruct()
            gb.seed, gb.scale, gb.considered = self.gumbel_seed, scale, considered
            gb.c_visit, gb.c_scale = self.policy_c_visit, self.policy_c_scale          # (the struct's fields are f32)
            gb.schedule, gb.m = t["gumbel_schedule"].data_ptr(), t["gumbel_m"].data_ptr()
        # every tensor is pointed at the struct field of its name (hist_value has none: it is an argument of the move; an absent
        # tensor -- gnn_workspace, the cache's -- leaves its field NULL)
        for name, tensor in t.items():
            for struct in (e, self.reuse, self.resign, self.policy_record):
                if hasattr(struct, name):
                    setattr(struct, name, tensor.data_ptr())
        self.record_history = record_history
        self.moves_done = 0
        self.reset()

    # ------------------------------------------------------------------
    def _stream(self):
        return _lib.stream_ptr(self.dev)

    def reset(self):
        if self.start is not None:
            _lib.check(self.lib.aqg_engine_reset_start(ctypes.byref(self.e), ctypes.byref(self.start), self._stream()), "aqg_engine_reset_start")
        else:
            _lib.check(self.lib.aqg_engine_reset(ctypes.byref(self.e), self._stream()), "aqg_engine_reset")
        if self.tree_reuse:
            self._forget_kept_trees()
            self.t["stat_moves_kept"].zero_()
            self.t["stat_visits_kept"].zero_()
        if self.resign is not None:
            _lib.check(self.lib.aqg_engine_reset_resign(ctypes.byref(self.e), ctypes.byref(self.resign), self._stream()), "aqg_engine_reset_resign")
        self.moves_done = 0
        self._applied_moves = False        # no history row without a search value yet (history_lambda_values)

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

    def _set_gumbel(self, table):
        """Table mode of the Gumbel root search: the variates of this move's roots, float64 [G, MAX_LEGAL] (None = the generator).
        Copied into one buffer the engine keeps, like the root-noise table: the struct is part of the captured graph's key."""
        if self.gumbel is None:
            if table is not None:
                raise ValueError("a gumbel table needs gumbel_considered > 0")
            return
        if table is None:
            self.gumbel.table = None
            return
        table = torch.as_tensor(table, dtype=torch.float64).to(self.dev).contiguous().view(self.G, _lib.MAX_LEGAL)
        if "gumbel_table" not in self.t:
            self.t["gumbel_table"] = torch.zeros((self.G, _lib.MAX_LEGAL), dtype=torch.float64, device=self.dev)
        self.t["gumbel_table"].copy_(table)      # stream-ordered behind the previous move's reads
        self.gumbel.table = self.t["gumbel_table"].data_ptr()

    def _move_gumbel(self):
        """move() with the Gumbel root search on: one entry point, which takes every option struct that may be on beside it."""
        _lib.check(self.lib.aqg_engine_move_gumbel(ctypes.byref(self.e), None, self.temperature_plies, _lib.ptr(self.t.get("hist_value")),
                                                   None, None,
                                                   ctypes.byref(self.policy_record) if self.policy_record is not None else None,
                                                   ctypes.byref(self.start) if self.start is not None else None,
                                                   ctypes.byref(self.gumbel), self._stream()), "aqg_engine_move_gumbel")
        self.moves_done += 1

    def root_gumbel(self):
        """The Gumbel root search's state of every slot's root, read out of the tree pool (needs gumbel_considered; valid behind
        search() and in front of a finish-move): (gl f32 [G, MAX_LEGAL] -- the Gumbel logits f32(scale * g + log p) in legal_actions()
        order, -inf for an action that was not sampled and past the count --, m i32 [G] -- min(gumbel_considered, sampled actions) --,
        winner i32 [G] -- the index of the child move() would play, -1 without children).  One launch that changes nothing."""
        if self.gumbel is None:
            raise ValueError("root_gumbel needs gumbel_considered > 0")
        gl = torch.empty((self.G, _lib.MAX_LEGAL), dtype=torch.float32, device=self.dev)
        m = torch.empty((self.G,), dtype=torch.int32, device=self.dev)
        winner = torch.empty((self.G,), dtype=torch.int32, device=self.dev)
        _lib.check(self.lib.aqg_engine_root_gumbel(ctypes.byref(self.e), ctypes.byref(self.gumbel), _lib.ptr(gl), _lib.ptr(m), _lib.ptr(winner),
                                                   self._stream()), "aqg_engine_root_gumbel")
        return gl, m, winner

    def move(self, uniforms=None, root_noise=None, gumbel=None):
        """One move for every active game.  uniforms: float64 [G] in [0,1) (default: device RNG stream).  root_noise: float64
        [G, MAX_LEGAL] gamma variates of this move's roots (default: the counter-based generator; needs root_noise_eps > 0).
        gumbel: float64 [G, MAX_LEGAL] Gumbel variates of this move's roots (default: the generator; needs gumbel_considered > 0);
        with the Gumbel root search on no uniform is consumed, and giving some is a mistake (ValueError)."""
        if self.gumbel is not None and uniforms is not None:
            raise ValueError("move(uniforms=) with gumbel_considered > 0: the move is the survivor of sequential halving, no uniform is consumed")
        self._set_root_noise(root_noise)
        self._set_gumbel(gumbel)
        if self.gumbel is not None:
            return self._move_gumbel()
        if uniforms is None:
            uniforms = torch.rand((self.G,), dtype=torch.float64, device=self.dev, generator=self.gen)
        else:
            uniforms = torch.as_tensor(uniforms, dtype=torch.float64).to(self.dev).contiguous()
        self._u = uniforms  # keep alive until the stream has consumed it
        # the entry point and what follows the uniforms: the plain form while every option is off, else the first form that takes
        # all that is on -- the start table's takes the other three structs or none, the policy record's takes the other two structs or
        # none, resignation's takes a tree-reuse struct or none, tree reuse's takes the targets, and so does _targets
        external = self.evaluator == "external"                  # (check_tree_reuse: never with tree reuse)
        tail = [self.temperature_plies, _lib.ptr(self.t.get("hist_value"))]
        if self.start is not None:
            form, tail = "_start", tail + [ctypes.byref(self.reuse) if self.tree_reuse else None,
                                           ctypes.byref(self.resign) if self.resign is not None else None,
                                           ctypes.byref(self.policy_record) if self.policy_record is not None else None,
                                           ctypes.byref(self.start)]
        elif self.policy_record is not None:
            form, tail = "_policy", tail + [ctypes.byref(self.reuse) if self.tree_reuse else None,
                                            ctypes.byref(self.resign) if self.resign is not None else None,
                                            ctypes.byref(self.policy_record)]
        elif self.resign is not None:
            form, tail = "_resign", tail + [ctypes.byref(self.reuse) if self.tree_reuse else None, ctypes.byref(self.resign)]
        elif self.tree_reuse:
            form, tail = "_reuse", tail + [ctypes.byref(self.reuse)]
        elif self.temperature_plies or self.record_search_value:
            form = "_targets"
        else:
            form, tail = "", []
        name = ("aqg_engine_finish_move" if external else "aqg_engine_move") + form
        if external:
            self._external_sims()
        _lib.check(getattr(self.lib, name)(ctypes.byref(self.e), _lib.ptr(uniforms), *tail, self._stream()), name)
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
        if self.policy_record is not None:
            raise ValueError("apply_actions() plays moves nobody searched: build the engine without policy_target='completed_q'")
        actions = torch.as_tensor(actions, dtype=torch.int32).to(self.dev).contiguous().view(self.G)
        self._applied = actions  # keep alive until the stream has consumed it
        if self.start is not None:
            _lib.check(self.lib.aqg_engine_apply_actions_start(ctypes.byref(self.e), _lib.ptr(actions), ctypes.byref(self.start), self._stream()),
                       "aqg_engine_apply_actions_start")
        else:
            _lib.check(self.lib.aqg_engine_apply_actions(ctypes.byref(self.e), _lib.ptr(actions), self._stream()), "aqg_engine_apply_actions")
        if self.tree_reuse:
            self._forget_kept_trees()      # the roots changed without a search: the next move starts from fresh trees
        self._applied_moves = True
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

    def policy_beside_expansions(self):
        """Leaves expanded by the policy workgroups of a step launch, beside its step workgroups, since the last reset (aqgnn.h
        counters[7]; option "policy_beside_step").  0 wherever the step workgroup expands itself."""
        return int(self.t["counters"][7].item())

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

    def play_generation(self, uniforms=None, check_every=4, root_noise=None, gumbel=None):
        """Play the whole quota (== every slot once when quota == num_games: one self_play generation's worth of games
        on this rank).  uniforms: optional float64 [moves, G]; root_noise: optional float64 [moves, G, MAX_LEGAL] gamma variates,
        gumbel: optional float64 [moves, G, MAX_LEGAL] Gumbel variates (parity tests).  Returns the counters dict."""
        ply = 0
        limit = self.max_plies * (-(-self.quota // self.G))          # every slot plays at most ceil(quota / G) games
        while True:
            self.move(None if uniforms is None else uniforms[ply], None if root_noise is None else root_noise[ply],
                      None if gumbel is None else gumbel[ply])
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
    def search(self, root_states72, check_saturation=True, root_noise=None, gumbel=None):
        """pv_mcts_policy for G roots at once: (visits i32 [G, MAX_LEGAL], actions u8, count i32).
        root_noise: float64 [G, MAX_LEGAL] gamma variates of the roots (root_noise_eps > 0; default: the generator, keyed by slot).
        gumbel: float64 [G, MAX_LEGAL] Gumbel variates of the roots (gumbel_considered > 0; default: the generator, keyed by slot); with
        the Gumbel root search on, the visit counts are sequential halving's and root_gumbel() names the child a move would play.
        check_saturation (GNN evaluator): the fp16-range guard's word (counters[5]) is cleared before the search and read back after it
        (one 4-byte copy: the callers read the visit counts back anyway); if a launch of this search met a value outside fp16 range its
        evaluations were finite but not the network's, so the weight set is marked (model.mark_saturated), the engine switches to the
        exact f32-input kernels and the search is repeated -- the caller never receives visit counts of clamped evaluations."""
        if self.tree_reuse:
            raise ValueError("search() looks at caller-given roots from fresh trees: build the engine without tree_reuse")
        if self.resign is not None:
            raise ValueError("search() plays no game: build the engine without resign_threshold")
        if self.policy_record is not None:
            raise ValueError("search() records no history: build the engine without policy_target='completed_q' (root_improved_policy() "
                             "reads the same target out of a searched root)")
        if self.start is not None:
            raise ValueError("search() looks at caller-given roots already: build the engine without start_states")
        roots = torch.as_tensor(root_states72, dtype=torch.uint8).to(self.dev).contiguous().view(self.G, 72)
        self._roots = roots
        self._set_root_noise(root_noise)
        self._set_gumbel(gumbel)
        for attempt in range(2):
            guarded = check_saturation and self.binding.guarded and not (self.e.gnn_flags & _lib.GNN_EXACT_F32)
            if guarded:
                self.t["counters"][5] = 0          # a cached engine (pv_mcts._engines) must not inherit an earlier search's word
            if self.evaluator == "external":
                _lib.check(self.lib.aqg_engine_set_roots(ctypes.byref(self.e), _lib.ptr(roots), self._stream()), "aqg_engine_set_roots")
                self._external_sims()
            elif self.gumbel is not None:
                _lib.check(self.lib.aqg_engine_search_gumbel(ctypes.byref(self.e), _lib.ptr(roots), ctypes.byref(self.gumbel), self._stream()),
                           "aqg_engine_search_gumbel")
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

    def root_values(self):
        """The search value of every slot's root after the last search, float32 [G]: w / n of node 0 from the mover's side, the
        expression a played move records as its search value (history_values); 0 for a root without a visit."""
        value = torch.empty((self.G,), dtype=torch.float32, device=self.dev)
        _lib.check(self.lib.aqg_engine_root_values(ctypes.byref(self.e), _lib.ptr(value), self._stream()), "aqg_engine_root_values")
        return value

    def root_improved_policy(self, c_visit=50.0, c_scale=1.0):
        """The completed-Q improved policy of every slot's root, pi' = softmax(log p + sigma(completedQ)) (include/aqgnn.h,
        "completed-Q policy targets"; improved_policy_reference is the statement): (policy f32 [G, MAX_LEGAL] in legal_actions() order,
        actions u8 [G, MAX_LEGAL], count i32 [G] -- the layout of search()'s visits, 0 and 0xFF past the count -- and vmix f32 [G], the
        mixed value that completes the unvisited children).  Valid after search() and in front of a finish-move, on every evaluator and
        with tree reuse; one launch (csrc/mcts_improve.hip) that reads the tree pool and changes nothing.  c_visit and c_scale must
        be finite and >= 0 (ValueError, before any launch)."""
        c_visit, c_scale = check_completed_q(c_visit, c_scale)
        policy = torch.empty((self.G, _lib.MAX_LEGAL), dtype=torch.float32, device=self.dev)
        actions = torch.empty((self.G, _lib.MAX_LEGAL), dtype=torch.uint8, device=self.dev)
        count = torch.empty((self.G,), dtype=torch.int32, device=self.dev)
        vmix = torch.empty((self.G,), dtype=torch.float32, device=self.dev)
        _lib.check(self.lib.aqg_engine_root_improved_policy(ctypes.byref(self.e), c_visit, c_scale, _lib.ptr(policy), _lib.ptr(actions),
                                                            _lib.ptr(count), _lib.ptr(vmix), self._stream()),
                   "aqg_engine_root_improved_policy")
        return policy, actions, count, vmix

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

    def history_lambda_values(self, lam):
        """The lambda-returns of the recorded search values, float32 [P], row-aligned with history_tensors() and history_values()
        (include/aqgnn.h, "lambda-return value targets"; lambda_values_reference is the statement): row t of a finished game holds
        G_t = (1 - lam) q_t + lam (-G_{t+1}), bootstrapped into the game's outcome at its last ply -- q_t at lam = 0, z_t at lam = 1.
        One aqg_lambda_values launch into a fresh [quota, max_plies] tensor, then the mask of the finished games' rows.  lam: a
        float32 in [0, 1] (check_value_lambda).  Needs record_search_value; ValueError once apply_actions() has played a move since
        the last reset(): such a row holds no search value, and 0 in its place would be a silent wrong target."""
        lam = check_value_lambda(lam)
        if not self.record_search_value:
            raise ValueError("history_lambda_values needs record_search_value=True")
        if self._applied_moves:
            raise ValueError("history_lambda_values: apply_actions() has played moves nobody searched since the last reset(); their "
                             "rows hold no search value")
        q = self.t["hist_value"]
        out = torch.empty_like(q)                 # every float the mask below keeps is written by the launch
        _lib.check(self.lib.aqg_lambda_values(q.shape[0], q.shape[1], _lib.ptr(self.t["game_plies"]), _lib.ptr(self.t["game_result"]),
                                              _lib.ptr(self.t["game_done"]), _lib.ptr(q), lam, _lib.ptr(out), self._stream()),
                   "aqg_lambda_values")
        return out[self._history_valid()[0]]

    def history_policies(self):
        """The recorded completed-Q policy targets, float32 [P, A], row-aligned with history_tensors(): dense by action id, 0 on
        every action that was not legal at the row's root (and a zero row for a move that was applied, not searched).  Needs
        policy_target='completed_q'."""
        if self.policy_record is None:
            raise ValueError("history_policies needs policy_target='completed_q'")
        return self.t["hist_policy"][self._history_valid()[0]]

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
        (self_play.py:51-54,:63-66).  policy_i = n_i / sum(n) in float64, exactly like boltzman at T=1; with
        policy_target='completed_q' the recorded float32 row, widened to Python floats."""
        st, vis, z = (x.cpu().numpy() for x in self.history_tensors())
        rec = self.history_policies().cpu().numpy() if self.policy_record is not None else None
        nw = (self.N - 1) ** 2
        out = []
        for i, (s, v, zz) in enumerate(zip(st, vis, z)):
            v = v.astype(np.float64)
            tot = v.sum()
            pol = rec[i].astype(np.float64).tolist() if rec is not None else (v / tot).tolist() if tot > 0 else [0.0] * self.A
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
                 resign_seed=None, start_states=None, start_index=None, gumbel_seed=None, **kw):
        check_resign(kw.get("resign_threshold"), kw.get("resign_min_ply", 0), kw.get("resign_disable_fraction", 0.1),
                     kw.get("record_history", True))          # before anything is allocated
        check_policy_record(kw.get("policy_target", "visits"), kw.get("policy_c_visit", 50.0), kw.get("policy_c_scale", 1.0),
                            kw.get("record_history", True))
        check_gumbel(kw.get("gumbel_considered", 0), kw.get("gumbel_scale", 1.0), sims, kw.get("root_noise_eps", 0.0), kw.get("tree_reuse", False),
                     kw.get("resign_threshold"), kw.get("temperature_plies", 0), kw.get("evaluator", "gnn"))
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
        # ... and for the Gumbel variates: a game's do not depend on the set count
        gumbel_seeds = set_noise_seeds(seed, default_gumbel_seed(seed) if gumbel_seed is None else gumbel_seed, sizes,
                                       [max(q, g) for q, g in zip(quotas, sizes)])
        # start positions: set i plays the games [sum of the quotas before it, + its own quota) of history_tensors()' order, and is handed
        # that slice of the index -- of the caller's, or of the default k % S written out, so that a game's start never depends on the sets
        set_quotas = [max(q, g) for q, g in zip(quotas, sizes)]
        start_indices = set_start_indices(start_states, start_index, set_quotas)
        if start_states is not None:
            kw = dict(kw, start_states=start_states)
        self.sets = []
        ready = torch.cuda.current_stream(self.dev).record_event()   # e.g. the model's weight upload on the caller's stream
        for i, g in enumerate(sizes):
            with torch.cuda.stream(self.streams[i]):
                self.streams[i].wait_event(ready)
                self.sets.append(BatchedSelfPlay(model, num_games=g, sims=sims, seed=int(seed) * 64 + i, device=self.dev,
                                                 quota=max(quotas[i], g),
                                                 root_noise_seed=noise_seeds[i], resign_seed=resign_seeds[i], gumbel_seed=gumbel_seeds[i],
                                                 **(dict(kw, start_index=start_indices[i]) if start_states is not None else kw)))
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

    def _joined(self, get):
        """get(set) -- a tuple of tensors -- on every set's stream, joined in set order on the current stream."""
        parts = [get(eng) for _, eng in self._each()]
        self.sync()
        cur = torch.cuda.current_stream(self.dev)
        for st in self.streams:
            cur.wait_stream(st)
        for p in parts:
            for x in p:
                x.record_stream(cur)              # the caching allocator must not recycle them under the concatenation
        return tuple(torch.cat(col, 0) for col in zip(*parts))

    def history_tensors(self):
        return self._joined(lambda eng: eng.history_tensors())

    def history_values(self):
        """The sets' history_values() in set order: float32 [P], row-aligned with history_tensors()."""
        return self._joined(lambda eng: (eng.history_values(),))[0]

    def history_lambda_values(self, lam):
        """The sets' history_lambda_values(lam) in set order: float32 [P], row-aligned with history_tensors()."""
        lam = check_value_lambda(lam)             # before any set launches
        return self._joined(lambda eng: (eng.history_lambda_values(lam),))[0]

    def history_policies(self):
        """The sets' history_policies() in set order: float32 [P, A], row-aligned with history_tensors()."""
        return self._joined(lambda eng: (eng.history_policies(),))[0]


def gather_history(states72, visits, z, group=None, force_collective=None, values=None, policies=None):
    """The one exchange step per generation: all-gather the ragged (s, pi, z) tuples of every rank.
    Counts are gathered first, payloads are padded to the max count (RCCL needs equal sizes) and trimmed after.
    Works on any torch.distributed backend (nccl == RCCL on ROCm; gloo in the CPU tests).
    force_collective (default: AQG_DIST_FORCE_GROUP=1): run the two collectives at world size 1 as well instead of returning the
    inputs -- the RCCL code path on the one GPU a developer box has (the result is the same rows, bit for bit).
    values (float32 [P], engine.history_values): every packed row carries its four bytes as well, and a fourth tensor is returned.
    policies (float32 [P, A], engine.history_policies): every packed row carries its 4 A bytes as well, behind the value's, and one
    more tensor is returned, last.  Without these two the layout and the return value are what they always were."""
    import torch.distributed as dist
    same = (states72, visits, z) + (() if values is None else (values,)) + (() if policies is None else (policies,))
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
    vb = 0 if values is None else 4
    row = 72 + 2 * A + 1 + vb + (0 if policies is None else 4 * A)
    buf = torch.zeros((m, row), dtype=torch.uint8, device=dev)
    k = states72.shape[0]
    if k:
        buf[:k, :72] = states72
        buf[:k, 72:72 + 2 * A] = visits.contiguous().view(torch.uint8).view(k, 2 * A)
        buf[:k, 72 + 2 * A] = z.view(torch.uint8)
        if values is not None:
            buf[:k, 73 + 2 * A:73 + 2 * A + 4] = values.to(torch.float32).contiguous().view(torch.uint8).view(k, 4)
        if policies is not None:
            buf[:k, 73 + 2 * A + vb:] = policies.to(torch.float32).contiguous().view(torch.uint8).view(k, 4 * A)
    out = torch.empty((W * m, row), dtype=torch.uint8, device=dev)
    dist.all_gather_into_tensor(out, buf, group=group)
    out = out.view(W, m, row)
    parts = [out[r, :counts[r]] for r in range(W)]
    allrows = torch.cat(parts, 0)
    s = allrows[:, :72].contiguous()
    v = allrows[:, 72:72 + 2 * A].contiguous().view(torch.int16).view(-1, A)
    zz = allrows[:, 72 + 2 * A].contiguous().view(torch.int8)
    out = (s, v, zz)
    if values is not None:
        out += (allrows[:, 73 + 2 * A:73 + 2 * A + 4].contiguous().view(torch.float32).view(-1),)
    if policies is not None:
        out += (allrows[:, 73 + 2 * A + vb:].contiguous().view(torch.float32).view(-1, A),)
    return out


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
