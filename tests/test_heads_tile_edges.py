"""The heads of the split network at the edges of their 16-board tile (run with -m gpu on an MI355X).

A workgroup of gcn_heads_mm_kernel (heads_body, gcn_heads_split.hpp) serves 16 boards: lane & 15 is the board of the hidden layer's
B operand, lane >> 4 picks four boards of the policy layer's accumulators, and boards past the launch's end are zero-filled, left out
of the range guard and not stored.  B = 1, 15, 16, 17 and 33 are a tile that is empty but for one board, one short, full, one over
(a second workgroup with one board) and two tiles plus one.  Every row is held to the fp64 oracle at the tolerances of
test_gpu_parity.py::test_gnn_forward_many_boards_per_workgroup, and a row must not depend on its place in a tile or on its
neighbours: the rows of the B = 17 and B = 33 launches equal the same board's row of a B = 1 launch bit for bit."""
import numpy as np
import pytest
import torch

from tests import _util as U

pytestmark = pytest.mark.gpu

SIZES = [1, 15, 16, 17, 33]
NB = max(SIZES)


@pytest.fixture(scope="module")
def dev():
    from alphaquoridorgnn_amd import _lib
    _lib.load()          # raises if the HIP library is missing: no fallback
    return _lib.require_gpu()


@pytest.fixture(scope="module")
def heads(dev):
    """The model, NB boards spread over the golden walk, their fp64 oracle and each board's own B = 1 launch: made once per module."""
    from alphaquoridorgnn_amd import _lib
    from alphaquoridorgnn_amd.pv_network_gnn import GNNNetwork
    from oracle import gnn as og
    params = og.init_params(11)
    for l in range(3):      # non-zero GCN biases, as in test_gpu_parity._walk_oracle
        params[f"gcn_layers.{l}.bias"] = (np.linspace(-0.3, 0.5, 128) * (1 + l)).astype(np.float32)
    states = U.golden("walk_9x9.npz")["states"]
    states = np.ascontiguousarray(states[np.linspace(0, states.shape[0] - 1, NB).astype(np.int64)])
    model = GNNNetwork()
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in params.items()})
    model = model.to(dev).eval()
    assert not (model.gnn_flags(dev) & _lib.GNN_EXACT_F32)          # the split network: heads_body is what runs
    recs = torch.from_numpy(states).to(dev)
    single = [[t.clone() for t in model.forward_states(recs[b:b + 1].contiguous(), want_logits=True)] for b in range(NB)]
    return dict(model=model, recs=recs, ref=og.forward_states_dense(params, states), single=single)


@pytest.mark.parametrize("B", SIZES)
def test_heads_tile_edges(dev, heads, B):
    from alphaquoridorgnn_amd import _lib
    c = heads
    ref = c["ref"]
    _lib.poison_lds(dev)
    policy, value, logits, vpre = c["model"].forward_states(c["recs"][:B].contiguous(), want_logits=True)
    assert policy.shape[0] == B and value.shape[0] == B and logits.shape[0] == B and vpre.shape[0] == B
    lg, vp = logits.cpu().numpy().astype(np.float64), vpre.cpu().numpy().astype(np.float64).reshape(B)
    np.testing.assert_allclose(lg, ref["logits"][:B], atol=1e-5, rtol=1e-4)
    np.testing.assert_allclose(vp, ref["value_pre"][:B], atol=1e-5, rtol=1e-4)
    np.testing.assert_allclose(policy.cpu().numpy(), ref["policy"][:B], atol=1e-6, rtol=1e-4)
    np.testing.assert_allclose(value.cpu().numpy().reshape(B), ref["value"][:B], atol=1e-5, rtol=1e-4)
    if B > 16:
        for b in range(B):
            for name, got, one in zip(("policy", "value", "logits", "value_pre"), (policy, value, logits, vpre), c["single"][b]):
                assert torch.equal(got[b:b + 1], one), f"{name} of board {b} in a launch of {B} differs from its own launch"
