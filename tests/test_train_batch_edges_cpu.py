"""What test_train_batch_edges.py (GPU) leans on, checked without a GPU: the target rows of _train_edges.edge_targets, the plain
numpy statement of the two losses against torch autograd in fp64, why the tiny batch sizes were chosen (the board groups of
train_final_kernel), and the ReLU-kink cap on the one draw per network that every tiny batch is sliced from."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import _train_edges as E   # noqa: E402


@pytest.mark.parametrize("N", [9, 5, 3])
def test_edge_targets_rows(N):
    A = E.policy_size(N)
    pi, z = E.edge_targets(8, A, seed=N)
    assert pi.dtype == np.float32 and z.dtype == np.float32 and pi.shape == (8, A) and z.shape == (8,)
    assert np.array_equal(z, np.array(E.EDGE_Z, dtype=np.float32))
    assert (pi >= 0).all()
    assert pi[0, A - 1] == 1.0 and np.count_nonzero(pi[0]) == 1            # the last action: lane 16 of the fourth logit on 9x9
    assert pi[1, 0] == 1.0 and np.count_nonzero(pi[1]) == 1
    assert np.array_equal(pi[2], np.full(A, np.float32(1.0 / A)))
    assert (pi[3] > 0).all() and len(np.unique(pi[3])) > A // 2
    assert not pi[6].any()
    sums = pi.astype(np.float64).sum(axis=1)
    np.testing.assert_allclose(sums, [1, 1, 1, 1, 0.5, 1.75, 0, 1], atol=1e-6)
    for b in (4, 5, 7):                                                    # sparse as the existing tests' rows: a Bernoulli(0.2) support
        assert 0 < np.count_nonzero(pi[b]) < A
    pi2, z2 = E.edge_targets(8, A, seed=N)
    assert np.array_equal(pi, pi2) and np.array_equal(z, z2)               # deterministic
    assert not np.array_equal(pi, E.edge_targets(8, A, seed=N + 1)[0])
    pi16, z16 = E.edge_targets(16, A, seed=N)                              # longer batches repeat the kinds
    assert np.array_equal(pi16[8], pi[0]) and np.array_equal(z16[8:], z)
    rn = E.renormalised(pi)
    np.testing.assert_allclose(rn.astype(np.float64).sum(axis=1), [1, 1, 1, 1, 1, 1, 0, 1], atol=1e-6)
    for b in range(8):
        assert np.array_equal(rn[b], pi[b]) == (b not in E.SCALED_ROWS)
        assert np.array_equal(rn[b] > 0, pi[b] > 0)


@pytest.mark.parametrize("N,B", [(9, 8), (5, 8), (3, 8), (9, 1), (5, 5)])
def test_numpy_loss_equals_torch_autograd_on_every_edge_row(N, B):
    """l_b = -sum_a t_a (p_a - log sum exp p), dl/dp_a = (softmax(p)_a sum(t) - t_a) / B, dv = 2 (v - z) / B against
    CrossEntropyLoss (probability targets) and MSELoss under fp64 autograd, to 1e-12, on every row kind of edge_targets."""
    A = E.policy_size(N)
    rng = np.random.RandomState(100 + N + B)
    logits = rng.randn(B, A)
    p = np.exp(logits) / np.exp(logits).sum(axis=1, keepdims=True)         # the network's own softmax: the loss softmaxes again
    v = np.tanh(rng.randn(B))
    pi, z = E.edge_targets(B, A, seed=N)
    got, want = E.loss_terms(p, v, pi, z), E.torch_loss_terms(p, v, pi, z)
    for g, w in zip(got, want):
        assert np.abs(g - w).max() <= 1e-12
    terms, dp, dv = got
    if B == 8:
        assert terms[6, 0] == 0.0                                          # the all-zero row: a term of exactly 0 ...
        np.testing.assert_array_equal(dp[6], 0.0)                          # ... and no policy gradient
        t2, dp2, dv2 = E.loss_terms(p, v, E.renormalised(pi), z)
        np.testing.assert_array_equal(dv2, dv)
        for b in range(8):
            scaled = b in E.SCALED_ROWS
            assert (np.abs(dp2[b] - dp[b]).max() > 1e-4 / B) == scaled, b  # the target-sum term moves the scaled rows' gradients only
            assert (abs(t2[b, 0] - terms[b, 0]) > 0.1) == scaled, b
        # the same softmax factor without the target sum: what a kernel that dropped `* tsum` would compute
        e = np.exp(p)
        dropped = (e / e.sum(axis=1, keepdims=True) - pi.astype(np.float64)) / B
        for b in range(8):
            assert (np.abs(dropped[b] - dp[b]).max() > 1e-4 / B) == (b in E.SCALED_ROWS or b == 6), b


def test_final_kernel_board_groups_cover_every_board_once():
    """per = ceil(B / 4), group grp = [grp per, min(B, grp per + per)): every board exactly once for B = 1 .. 130; and what the batch
    sizes of the GPU tests reach: empty groups (1, 2, 3), a last group that starts past the end (5) or at it (9)."""
    for B in range(1, 131):
        seen = np.zeros(B, dtype=int)
        for b0, b1 in E.final_groups(B):
            for b in range(b0, b1):                # range() of an empty or inverted group is empty, as the kernel's loop
                seen[b] += 1
        assert (seen == 1).all(), B
    assert all(B in E.TINY_BATCHES for B in (1, 2, 3, 5, 9))
    for B in (1, 2, 3):
        assert [b1 > b0 for b0, b1 in E.final_groups(B)] == [g < B for g in range(4)]
    assert E.final_groups(5) == [(0, 2), (2, 4), (4, 5), (6, 5)]           # per = 2: the last group starts past the end
    assert E.final_groups(9) == [(0, 3), (3, 6), (6, 9), (9, 9)]           # per = 3: it starts at the end
    past = [B for B in range(1, 131) if any(b0 > B for b0, _ in E.final_groups(B))]
    assert past == [1, 2, 5]                                                # the only batch sizes with a group past the end
    assert [B for B in range(1, 131) if any(b1 <= b0 for b0, b1 in E.final_groups(B))] == [1, 2, 3, 5, 6, 9]
    assert all(b1 - b0 == 12 for b0, b1 in E.final_groups(48))              # the existing tests: every group full


@pytest.mark.parametrize("N", [9, 5, 3])
def test_kink_cap_holds_on_the_fused_networks_draw(N):
    from tests.test_gpu_parity import KINK_DROP_BOUND
    recs, pi, z, (drawn, dropped) = E.fused_draw(N)
    print(f"{N}x{N}: kink filter dropped {dropped} of {drawn}")
    assert drawn == 2 * E.DRAW and dropped <= KINK_DROP_BOUND * drawn
    assert recs.shape == (E.DRAW, 72)
    if N == 9:
        assert dropped == 14
    from oracle import gnn as og                  # the target-edge tests' network (policy head scaled): the same margins, the same draw
    assert np.array_equal(og.relu_margins(E.fused_params(N, peaked=True), recs), og.relu_margins(E.fused_params(N), recs))


@pytest.mark.parametrize("shape,N", E.GENERAL_NETS, ids=["x".join(map(str, s)) + f"-{n}x{n}" for s, n in E.GENERAL_NETS])
def test_kink_cap_holds_on_the_any_shape_networks_draw(shape, N):
    from tests.test_gpu_parity import KINK_DROP_BOUND
    net = E.general_net(shape, N)
    recs, pi, z, (drawn, dropped) = E.general_draw(net, shape, N)
    print(f"{shape} {N}x{N}: kink filter dropped {dropped} of {drawn}")
    assert drawn == 3 * E.DRAW and dropped <= KINK_DROP_BOUND * drawn
    assert recs.shape == (E.DRAW, 72)
    assert drawn - dropped >= E.DRAW                                        # so _batch drew its 48 without replacement
    peaked = E.general_draw(E.general_net(shape, N, peaked=True), shape, N)  # the target-edge tests' network: the same draw
    assert np.array_equal(peaked[0], recs) and peaked[3] == (drawn, dropped)


EDGE_NETS = [("fused", 9), ("fused", 5), ("general", 9), ("cnn", 5)]


@pytest.mark.parametrize("kind,N", EDGE_NETS, ids=[f"{k}-{n}x{n}" for k, n in EDGE_NETS])
def test_target_edge_batch_sees_the_target_sum_term(kind, N):
    """On the networks of the GPU target-edge tests (policy head scaled: _train_edges.peaked_policy) the gradient of the loss WITHOUT
    the target-sum factor -- what `* tsum` deleted from heads_board, or `* ts` from train_general_loss_kernel, computes -- lies more
    than 10 bars from the reference's gradient in every tensor of the policy head (and leaves the value head's alone).  On the unscaled GNNs it lies within ONE bar:
    a near-uniform policy makes the second softmax constant, and no test on such a network can see the factor."""
    from tests.test_cnn import _states
    from tests.test_cnn_train import GRAD_REL, _ref_step, _rel
    from tests.test_train_general import _ref_step as general_ref_step
    pi, z = E.edge_targets(8, E.policy_size(N), seed=N)
    pi64, z64 = pi.astype(np.float64), z.astype(np.float64)

    def bars(peaked):
        if kind == "cnn":
            net, recs = E.cnn_net(16, 2, N, peaked), _states(N, 16)[:8].copy()
            ref = _ref_step(net, recs, pi, z, N)[2]
            for g, r in zip(E.cnn_step(net, recs, pi, z), ref):
                assert _rel(g, r) <= 1e-12                                  # cnn_step is the reference when nothing is dropped
            dropped = E.cnn_step(net, recs, pi, z, drop_target_sum=True)
            return {k: _rel(g, r) / GRAD_REL for (k, _), g, r in zip(net.named_parameters(), dropped, ref)}
        if kind == "fused":
            params, L, recs = E.fused_params(N, peaked), 3, E.fused_draw(N)[0][:8]
        else:
            net = E.general_net((6, 64, 2), N, peaked=peaked)
            params, L, recs = net.state_dict(), 2, E.general_draw(net, (6, 64, 2), N)[0][:8]
            for (k, _), r in zip(net._ordered_params(), general_ref_step(net, recs, pi64, z64)[0]):
                assert np.abs(E.gnn_step(params, L, recs, pi64, z64)[0][k] - r).max() <= 1e-12, k
        ref = E.gnn_step(params, L, recs, pi64, z64)[0]
        dropped = E.gnn_step(params, L, recs, pi64, z64, drop_target_sum=True)[0]
        return {k: E.grad_error(dropped[k], ref[k]) / E.GRAD_BAR for k in ref}

    seen = bars(True)
    print(f"{kind} {N}x{N}: the dropped factor moves the policy head's gradients by {min(v for k, v in seen.items() if 'policy_head' in k):.0f} bars or more")
    assert all(v > 10 for k, v in seen.items() if "policy_head" in k), seen
    assert all(v == 0 for k, v in seen.items() if "value_head" in k)
    if kind != "cnn":
        assert max(bars(False).values()) < 1


@pytest.mark.parametrize("B", [1, 5])
def test_stock_step_in_fp64_equals_both_references(B):
    """_train_edges.gnn_step, whose float32 run is the stock-fp32 yardstick of the GPU tests, is in float64 the two fp64 references:
    oracle/train.py::train_steps (6/128/3) and test_train_general._ref_step (any shape) -- at a batch of one too."""
    from oracle import gnn as og, train as ot
    from tests.test_train_general import _ref_step
    params = E.fused_params(9)
    recs, pi, z, _ = E.fused_draw(9)
    recs, pi, z = recs[:B], pi[:B].astype(np.float64), z[:B].astype(np.float64)
    ref = ot.train_steps(params, [(recs, pi, z)])[0]
    g, pl, vl = E.gnn_step(params, 3, recs, pi, z)
    assert abs(pl - ref["policy_loss"]) <= 1e-12 and abs(vl - ref["value_loss"]) <= 1e-12
    for k in og.KEYS:
        assert np.abs(g[k] - ref["grads"][k]).max() <= 1e-12, k
        assert E.grad_error(g[k], ref["grads"][k]) <= 1e-9
    one = np.ones(4)
    assert E.grad_error(one * (1 + 1.9e-5), one) <= E.GRAD_BAR < E.grad_error(one * (1 + 2.1e-5), one)       # the bar, restated
    assert E.grad_error(np.full(4, 0.9e-7), 0 * one) <= E.GRAD_BAR < E.grad_error(np.full(4, 1.1e-7), 0 * one)
    g32 = E.gnn_step(params, 3, recs, pi, z, torch.float32)[0]
    assert 0 < max(E.grad_error(g32[k], ref["grads"][k]) for k in og.KEYS) < 1e-4       # float32 is float32, and no worse
    shape, N = E.GENERAL_NETS[2]
    net = E.general_net(shape, N)
    recs, pi, z, _ = E.general_draw(net, shape, N)
    recs, pi, z = recs[:B], pi[:B].astype(np.float64), z[:B].astype(np.float64)
    g_ref, pl_ref, vl_ref = _ref_step(net, recs, pi, z)
    g, pl, vl = E.gnn_step(net.state_dict(), shape[2], recs, pi, z)
    assert abs(pl - pl_ref) <= 1e-12 and abs(vl - vl_ref) <= 1e-12
    for (k, _), r in zip(net._ordered_params(), g_ref):
        assert np.abs(g[k] - r).max() <= 1e-12, k
