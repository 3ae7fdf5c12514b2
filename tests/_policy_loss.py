"""What the loss-form tests share (test_policy_loss_cpu.py, test_policy_loss.py): the torch statement of both loss forms in fp64
(include/aqgnn.h "loss form"), fp64 autograd of the three networks under it, and the fixed row the motivation is pinned on.  No GPU,
no library call."""
import copy

import numpy as np
import torch

from tests._train_edges import (edge_targets, fused_params, general_net, cnn_net, peaked_policy, GRAD_BAR, GRAD_ABS,    # noqa: F401
                                TINY_BATCHES, policy_size)
from tests._optim_controls import assert_adam_bar, assert_visible, shadow_run                                           # noqa: F401

ROW_REL, ROW_ABS = 1e-5, 1e-7     # tests/test_train_batch_edges.py's bars of the per-position loss terms
CE, REFERENCE = 1, 0              # aqg_loss.policy_form
POLICY_KEYS_EXCLUDED = ("value_head",)    # the matrices no policy gradient reaches: the two forms agree on them, whatever the rows


def torch_loss(logits, value, target, z, form, w):
    """The torch statement: CrossEntropyLoss()(logits, t) (form 1) or, the reference's, CrossEntropyLoss()(softmax(logits), t)
    (form 0), plus w * MSELoss()(value, z).  Returns (total, policy loss, value loss)."""
    pl = torch.nn.CrossEntropyLoss()(logits if form == CE else torch.softmax(logits, dim=1), target)
    vl = torch.nn.MSELoss()(value.view(-1), z)
    return pl + w * vl, pl, vl


def torch_loss_terms(logits, vpre, pi, z, form, w):
    """(terms [B, 2], d total / d logits, d total / d pre-tanh value) from torch autograd in fp64: what loss_reference is held to."""
    x = torch.tensor(np.asarray(logits, dtype=np.float64), requires_grad=True)
    u = torch.tensor(np.asarray(vpre, dtype=np.float64), requires_grad=True)
    t, zz = torch.tensor(np.asarray(pi, dtype=np.float64)), torch.tensor(np.asarray(z, dtype=np.float64))
    v = torch.tanh(u)
    torch_loss(x, v, t, zz, form, w)[0].backward()
    with torch.no_grad():
        rows = torch.nn.CrossEntropyLoss(reduction="none")(x if form == CE else torch.softmax(x, dim=1), t)
        terms = torch.stack([rows, (v - zz) ** 2], dim=1)
    return terms.numpy(), x.grad.numpy(), u.grad.numpy(), v.detach().numpy()


def gnn_reference(params, L, recs, pi, z, form=CE, w=1.0):
    """One step of the L-layer GNN in fp64 autograd under the torch statement (tests._train_edges.gnn_step's network, the loss taken
    from the LOGITS).  Returns ({key: gradient}, logits [B, A], value [B]) as fp64 numpy."""
    from tests.test_train_general import _dense
    p = {k: torch.as_tensor(np.asarray(v.detach().cpu() if torch.is_tensor(v) else v)).double().requires_grad_(True)
         for k, v in params.items()}
    x, adj = _dense(recs)
    h = x
    for l in range(L):
        h = torch.relu(adj @ (h @ p[f"gcn_layers.{l}.lin.weight"].T) + p[f"gcn_layers.{l}.bias"])
    g = h.mean(dim=1)
    hp = torch.relu(g @ p["policy_head.0.weight"].T + p["policy_head.0.bias"])
    hv = torch.relu(g @ p["value_head.0.weight"].T + p["value_head.0.bias"])
    logits = hp @ p["policy_head.2.weight"].T + p["policy_head.2.bias"]
    value = torch.tanh(hv @ p["value_head.2.weight"].T + p["value_head.2.bias"]).view(-1)
    total = torch_loss(logits, value, torch.as_tensor(np.asarray(pi)).double(), torch.as_tensor(np.asarray(z)).double(), form, w)[0]
    total.backward()
    return {k: v.grad.numpy() for k, v in p.items()}, logits.detach().numpy(), value.detach().numpy()


def cnn_reference(net, recs, pi, z, form=CE, w=1.0):
    """The same for the residual CNN: a fp64 copy in train mode (BatchNorm on the batch statistics, as the HIP step).  Returns
    ([gradient per parameter], logits, value, the stepped copy)."""
    from tests.test_cnn_cpu import _triples
    m = copy.deepcopy(net).cpu().double().train()
    x = torch.from_numpy(m.preprocess_input(_triples(recs, net.board_size))).double()
    x = m.global_avg_pool(m.residual_blocks(torch.relu(m.conv(x))))
    logits = m.policy_head[1](m.policy_head[0](x))
    value = m.value_head(x).view(-1)
    total = torch_loss(logits, value, torch.from_numpy(np.asarray(pi)).double(), torch.from_numpy(np.asarray(z)).double(), form, w)[0]
    total.backward()
    return [q.grad.numpy() for q in m.parameters()], logits.detach().numpy(), value.detach().numpy(), m


def grad_bar(ref):
    """The project's gradient bar of one tensor: GRAD_BAR max|ref| + GRAD_ABS."""
    return GRAD_BAR * float(np.abs(ref).max()) + GRAD_ABS


def assert_rows(got, ref, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), (what, got)
    assert (np.abs(got - ref) <= ROW_REL * np.abs(ref) + ROW_ABS).all(), (what, np.abs(got - ref).max(), got, ref)


def assert_grads(keys, got, ref, what):
    """Every tensor within GRAD_BAR max|ref| + GRAD_ABS; prints the worst error in the bar's unit before it asserts."""
    errs = {}
    for k, g, r in zip(keys, got, ref):
        g, r = np.asarray(g, dtype=np.float64), np.asarray(r, dtype=np.float64)
        assert np.isfinite(g).all(), (what, k)
        errs[k] = np.abs(g - r).max() / grad_bar(r)
    worst = max(errs, key=errs.get)
    print(f"{what}: worst gradient error {errs[worst]:.3g} of the bar at {worst}")
    assert errs[worst] <= 1.0, (what, worst, errs[worst])


def assert_forms_differ(keys, ref_ce, ref_reference, what):
    """The visibility guard of the one-step comparisons, on the fp64 references alone: a kernel that ignored the option would return
    the reference form's gradients, and the comparison must then fail by a wide margin on EVERY weight matrix the policy gradient
    reaches -- max|g_ce - g_reference| > 100 x the bar of that matrix.  (The value head's matrices are left out: both forms share the
    value term, so the two gradients agree there exactly.  Stated as a share of the elements the guard cannot hold for any correct
    step: 9 % to 60 % of a matrix's gradient elements are exactly zero in both forms -- ReLU units dead on the batch, feature
    columns that are zero -- and on the 9x9 board fewer than half of the rest reach 2e-3 max|g| at all, in either form.  The share
    is printed; measured over the cases of test_policy_loss.py: 8 % to 99 % of a matrix, the fused 9x9 network lowest.)"""
    shares = []
    for k, a, b in zip(keys, ref_ce, ref_reference):
        a, b = np.asarray(a), np.asarray(b)
        if a.ndim < 2 or k.startswith(POLICY_KEYS_EXCLUDED):
            continue
        d = np.abs(a - b)
        shares.append(float((d > 100 * grad_bar(a)).mean()))
        assert d.max() > 100 * grad_bar(a), (what, k, d.max() / grad_bar(a))
    print(f"{what}: share of each matrix where the forms differ by > 100 x the bar: {min(shares):.2f} .. {max(shares):.2f}")


# The fixed row of the motivation (A = 17, the 3x3 board's policy size): a soft target whose largest entry leads the second by 0.15.
# The reference's loss over the simplex, lse(p) - t . p, has its minimum at the vertex e_k exactly when t_k - t_j >=
# (e - 1) / (A - 1 + e) = 0.092 for every j (the gradient softmax(p) - t at e_k, compared across coordinates), which this row meets.
MOTIVATION_A = 17
MOTIVATION_ROW = np.full(MOTIVATION_A, 0.35 / 15)
MOTIVATION_ROW[3], MOTIVATION_ROW[11] = 0.40, 0.25


def descend(form, lr, steps, seed=0):
    """fp64 gradient descent on the logits of the fixed row under loss_reference's gradient; returns softmax(logits) at the end."""
    from alphaquoridorgnn_amd.train_reference import loss_reference
    x = np.random.RandomState(seed).randn(1, MOTIVATION_A) * 0.1
    for _ in range(steps):
        x -= lr * loss_reference(x, np.zeros(1), MOTIVATION_ROW[None], np.zeros(1), policy_form=form)[1]
    p = np.exp(x - x.max())
    return (p / p.sum())[0]


# ---------------------------------------------------------------- the fused trainer's networks and draws, one per board size
FUSED_BOARDS = (3, 5, 7, 9)       # A = 17 / 57 / 121 / 209: one, one, two and four lane rounds of wave 0's softmax section
FUSED_7 = (4, 2)                  # (og.init_params seed, _train_batch seed) of the 7x7 network, which _train_edges does not draw


def fused_net_params(N, peaked=False):
    from tests import _train_edges as E
    if N in E.FUSED_NETS:
        return fused_params(N, peaked)
    from oracle import gnn as og
    params = og.init_params(FUSED_7[0], N=N)
    if peaked:
        peaked_policy(params["policy_head.2.weight"], params["policy_head.2.bias"])
    return params


def fused_draw(N):
    """recs [48, 72] of the fused trainer's network on the N x N board, kink-filtered (test_gpu_parity._train_batch)."""
    from tests import _train_edges as E
    if N in E.FUSED_NETS:
        return E.fused_draw(N)[0]
    from tests.test_gpu_parity import _train_batch
    return np.ascontiguousarray(_train_batch(E.DRAW, FUSED_7[1], N=N, params=fused_net_params(N))[0])
