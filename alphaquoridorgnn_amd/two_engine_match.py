"""The match loop of evaluate_network.BatchedMatch and evaluate_agents.BatchedAgentMatch: two engines, one per first mover."""
import numpy as np

from . import _lib


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
