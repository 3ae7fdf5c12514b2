"""Evaluator bindings: what the host layer knows about each evaluator the engine can run (include/aqgnn.h, `prior_mode`).

One object per evaluator name; BINDINGS, at the end, is the only place the names and their prior_mode are listed.  The library
dispatches on prior_mode once (enqueue_sims); engine.BatchedSelfPlay, the match classes and pv_mcts go through the binding instead
of a chain of `if evaluator == ...`.  A new network kind plugs in here: a subclass that says how its model is validated, what
workspace its forward needs, what the engine struct is pointed at and when cached evaluations are stale, and a line in BINDINGS.
"""


class Evaluator:
    """The base is also the whole binding of an evaluator without weights of its own."""
    network = False      # the library's kernels evaluate it: may use the evaluation cache, AQG_EVAL_CACHE_SLOTS applies, pv_mcts refreshes it
    guarded = False      # its kernels have the fp16 range guard (counters[5], GNN_EXACT_F32)
    packed = False       # model.packed_weights(device) builds what the kernels read (MultiSetSelfPlay packs before its sets start)
    width = None         # the model attribute the workspace grows with (the only one that does)

    def __init__(self, name, prior_mode):
        self.name, self.prior_mode = name, prior_mode

    def check(self, model):
        """The refusals that need no GPU: raised before anything is allocated or launched."""

    def _check_policy(self, model, board):
        if board is not None and model.policy_output_size != board[1]:
            raise ValueError(f"evaluator='{self.name}': the network's policy_output_size {model.policy_output_size} is not the "
                             f"{board[0]}x{board[0]} board's {board[1]} actions")

    def sizing_player(self, players):
        """Of a match's players, the one an engine must be built with: the one with the largest workspace."""
        return players[0] if self.width is None else max(players, key=lambda m: getattr(m, self.width))

    def workspace_floats(self, lib, model, N, A, G):
        """f32 words of `gnn_workspace` for G slots on an N x N board with A actions (0 = none)."""
        return 0

    def handle(self, model, dev, board=None):
        """What the engine struct is pointed at for `model` on `dev`; the caller keeps it alive.  board = (N, A): also refuse a
        network whose policy head is not that board's."""

    def point(self, eng, handle):
        """Write a handle into the engine (its struct, and the tensors it keeps alive)."""

    def stale(self, eng, handle):
        """refresh_weights: do the evaluations cached under eng's current handle differ from those of `handle`?"""


class _Gnn(Evaluator):
    """The default 6/128/3 network on the fused board kernels.  Handle: (packed weights, gnn_flags)."""
    network = guarded = packed = True

    def check(self, model):
        if model is not None and not getattr(model, "fused", True):
            model._require_fused("evaluator='gnn'")

    def workspace_floats(self, lib, model, N, A, G):      # smaller boards run the any-size forward, which needs a caller-owned workspace;
        # 9x9: the forward needs none -- two words per slot for the expansion jobs of option "policy_beside_step" (aqgnn.h, gnn_workspace)
        return int(lib.aqg_gcn_boards_any_workspace_floats(N, G)) if N != 9 else 2 * G

    def handle(self, model, dev, board=None):
        if model is None:
            raise ValueError("evaluator='gnn' needs a model")
        return model.packed_weights(dev), int(model.gnn_flags(dev))

    def point(self, eng, handle):
        eng.t["packed_weights"] = handle[0]
        eng.e.packed_weights = handle[0].data_ptr()
        eng.e.gnn_flags = handle[1]

    def stale(self, eng, handle):      # the SAME tensor object while no parameter has changed; the flags choose the kernel build
        return handle[0] is not eng.t["packed_weights"] or handle[1] != int(eng.e.gnn_flags)


class _General(Evaluator):
    """A GraphPolicyValueNetwork of any shape with 6 input features.  Handle: (descriptor, general_weights_key)."""
    network, width = True, "hidden_dim"

    def check(self, model):
        if model is not None and getattr(model, "num_features", 6) != 6:
            raise ValueError(f"evaluator='general': board records have 6 feature planes; this network takes "
                             f"num_features={model.num_features}")

    def workspace_floats(self, lib, model, N, A, G):
        return int(lib.aqg_gcn_boards_general_workspace_floats(N, model.hidden_dim, A, G))

    def handle(self, model, dev, board=None):
        if model is None or not hasattr(model, "general_net"):
            raise ValueError("evaluator='general' needs a GraphPolicyValueNetwork")
        net = model.general_net(dev)          # ValueError: not 6 input features, or parameters not f32 on dev
        self._check_policy(model, board)
        return net, model.general_weights_key()

    def point(self, eng, handle):
        eng.e.general_net = handle[0]

    def stale(self, eng, handle):      # (an in-place update leaves the descriptor's bytes, and the captured graph, as they were)
        return handle[1] != eng._handle[1]


class _Cnn(Evaluator):
    """The reference's residual CNNNetwork.  Handle: (packed weights, which the descriptor points into; descriptor)."""
    network, packed, width = True, True, "num_filters"

    def workspace_floats(self, lib, model, N, A, G):
        return int(lib.aqg_cnn_workspace_floats(N, model.num_filters, A, G))

    def handle(self, model, dev, board=None):
        if model is None or not hasattr(model, "cnn_net"):
            raise ValueError("evaluator='cnn' needs a CNNNetwork")
        self._check_policy(model, board)
        return model.packed_weights(dev), model.cnn_net(dev)

    def point(self, eng, handle):
        eng.e.cnn_net = handle[1]

    def stale(self, eng, handle):      # the SAME tensor while no parameter or BN statistic has changed
        return handle[0] is not eng._handle[0]


class _Fake(Evaluator):
    """The parity tests' integer-hash evaluator (oracle/mcts.py FakeModel).  Its "model" is the integer bias (None: fake_bias)."""

    def handle(self, model, dev, board=None):
        return None if model is None else int(model)

    def point(self, eng, handle):
        if handle is not None:
            eng.e.fake_bias = handle


class _External(Evaluator):
    """Any object with the reference's predict(state, device), asked from the host; the engine reads it from eng.model."""

    def handle(self, model, dev, board=None):
        if model is None or not hasattr(model, "predict"):
            raise ValueError("evaluator='external' needs a model with predict(state, device)")


BINDINGS = {b.name: b for b in (_Gnn("gnn", 0), _General("general", 3), _Cnn("cnn", 4), _Fake("fake", 1), _External("external", 2))}
