"""CPU tests (no GPU) of the evaluator bindings (alphaquoridorgnn_amd/evaluators.py): the table, and the refusals BatchedSelfPlay,
BatchedMatch and BatchedAgentMatch make for each evaluator -- which of them come before the GPU is asked for, and which after."""
import pytest
import torch


def test_binding_table():
    from alphaquoridorgnn_amd.evaluators import BINDINGS
    assert {n: b.prior_mode for n, b in BINDINGS.items()} == {"gnn": 0, "general": 3, "cnn": 4, "fake": 1, "external": 2}
    assert all(b.name == n for n, b in BINDINGS.items())
    assert {n for n, b in BINDINGS.items() if b.network} == {"gnn", "general", "cnn"}
    assert {n for n, b in BINDINGS.items() if b.guarded} == {"gnn"}


def test_sizing_player_is_the_wider_one():
    from alphaquoridorgnn_amd.evaluators import BINDINGS
    from alphaquoridorgnn_amd.pv_network_cnn import CNNNetwork
    from alphaquoridorgnn_amd.pv_network_gnn import GraphPolicyValueNetwork
    narrow, wide = GraphPolicyValueNetwork(6, 32, 2, 57, board_size=5), GraphPolicyValueNetwork(6, 64, 1, 57, board_size=5)
    assert BINDINGS["general"].sizing_player([narrow, wide]) is wide and BINDINGS["general"].sizing_player([wide, narrow]) is wide
    narrow, wide = CNNNetwork(16, 2, board_size=5), CNNNetwork(24, 1, board_size=5)
    assert BINDINGS["cnn"].sizing_player([narrow, wide]) is wide and BINDINGS["cnn"].sizing_player([wide, narrow]) is wide


def _models():
    from alphaquoridorgnn_amd.pv_network_cnn import CNNNetwork
    from alphaquoridorgnn_amd.pv_network_gnn import GNNNetwork, GraphPolicyValueNetwork
    return dict(feat8=GraphPolicyValueNetwork(8, 64, 2, 209), unfused=GraphPolicyValueNetwork(6, 64, 2, 209), none=None, obj=object(),
                gnn=GNNNetwork(), gnn5=GraphPolicyValueNetwork(6, 64, 2, 41, board_size=5), cnn5=CNNNetwork(16, 1, board_size=5))


# (evaluator, model, the refusal with a GPU, where it is made, BatchedMatch's own refusal if it is another one).  "before": a
# ValueError before the GPU is asked for, so the same on a machine without one; "after": behind require_gpu and the engine's
# allocations, so a machine without a GPU says HipLibraryError instead.  The models here sit on the CPU: with a GPU, 'general'
# refuses their parameters' device first ("float32 tensor on cuda"), an equally late ValueError.  BatchedMatch picks the sizing
# player before it builds an engine, which for a player without the width attribute is an AttributeError before anything else.
REFUSALS = [
    ("general", "feat8", "6 feature planes", "before", None),
    ("gnn", "unfused", "evaluator='external'", "before", None),
    ("gnn", "none", "evaluator='gnn' needs a model", "after", None),
    ("general", "none", "needs a GraphPolicyValueNetwork", "after", "hidden_dim"),
    ("general", "obj", "needs a GraphPolicyValueNetwork", "after", "hidden_dim"),
    ("cnn", "none", "needs a CNNNetwork", "after", "num_filters"),
    ("cnn", "gnn", "needs a CNNNetwork", "after", "num_filters"),
    ("external", "none", "evaluator='external' needs a model with predict", "after", None),
    ("external", "obj", "evaluator='external' needs a model with predict", "after", None),
    ("general", "gnn5", "policy_output_size 41 is not the 9x9 board's 209 actions|float32 tensor on cuda", "after", None),
    ("cnn", "cnn5", "policy_output_size 57 is not the 9x9 board's 209 actions", "after", None),
]


@pytest.mark.parametrize("evaluator,model,fragment,where,match_own", REFUSALS, ids=[f"{r[0]}-{r[1]}" for r in REFUSALS])
def test_refusals_before_and_after_the_gpu(evaluator, model, fragment, where, match_own):
    from alphaquoridorgnn_amd import _lib
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    from alphaquoridorgnn_amd.evaluate_agents import BatchedAgentMatch
    from alphaquoridorgnn_amd.evaluate_network import BatchedMatch
    m = _models()[model]
    if where == "before" or torch.cuda.is_available():
        expect = dict(expected_exception=ValueError, match=fragment)
    else:
        expect = dict(expected_exception=_lib.HipLibraryError, match="no MI355X visible")
    with pytest.raises(**expect):
        BatchedSelfPlay(m, num_games=2, sims=4, evaluator=evaluator)
    with pytest.raises(**expect):
        BatchedAgentMatch(m, "random", 4, sims=4, evaluator=evaluator)
    if evaluator == "external":          # (no such match: test_match_refuses_external)
        return
    if match_own is not None:
        expect = dict(expected_exception=AttributeError, match=match_own)
    with pytest.raises(**expect):
        BatchedMatch((m, m), 4, sims=4, evaluator=evaluator)


def test_match_refuses_external():
    """An engine asks ONE model, eng.model, from the host, so a match cannot point it at the mover: refused by name, up front."""
    from alphaquoridorgnn_amd.evaluate_network import BatchedMatch
    with pytest.raises(ValueError, match="BatchedMatch has no evaluator='external'"):
        BatchedMatch((object(), object()), 4, sims=4, evaluator="external")


def test_agent_match_names_come_from_the_table():
    from alphaquoridorgnn_amd.evaluate_agents import BatchedAgentMatch
    with pytest.raises(ValueError, match="evaluator must be one of gnn, general, cnn, fake, external"):
        BatchedAgentMatch(None, "random", 4, sims=4, evaluator="gcn")
