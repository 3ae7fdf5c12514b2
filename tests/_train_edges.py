"""What the training steps' edge tests (test_train_batch_edges.py, on the GPU) lean on, stated without a GPU: the batch sizes and why
they were chosen (the board groups of train_final_kernel), the policy / value targets at their edges, the loss both references
compute in plain numpy fp64, and the one kink-filtered draw per network that every tiny batch is a slice of."""
import numpy as np
import torch

FINAL_GROUPS = 4                 # csrc/gcn_train_final.hip
TINY_BATCHES = (1, 2, 3, 5, 9)   # 1, 2, 3: groups 1 .. 3 empty; 5 (per = 2): the last group starts past the end; 9 (per = 3): at it
DRAW = 48                        # the size at which the existing helpers draw (and at which KINK_DROP_BOUND means something)
EDGE_Z = (0.37, -0.93, 1.0, -1.0, 0.0, 0.999, -0.5, 0.125)
EDGE_ROWS = len(EDGE_Z)
SCALED_ROWS = {4: 0.5, 5: 1.75}  # row -> the sum of its policy target


def policy_size(N):
    return N * N + 2 * (N - 1) ** 2


def final_groups(B):
    """The board ranges [b0, b1) train_final_kernel's FINAL_GROUPS groups sum at batch B (an empty group: b1 <= b0)."""
    per = (B + FINAL_GROUPS - 1) // FINAL_GROUPS
    return [(grp * per, min(B, grp * per + per)) for grp in range(FINAL_GROUPS)]


def _sparse_row(rng, A):
    """A row as the existing tests draw it: about 20 % of the actions, normalised."""
    row = rng.rand(A) * (rng.rand(A) < 0.2)
    row[0] += 1e-3
    return row / row.sum()


def edge_targets(B, A, seed):
    """(pi float32 [B, A], z float32 [B]): row b is of kind b % 8 --
    0 all mass on action A - 1, 1 all mass on action 0, 2 dense uniform, 3 dense random (every entry > 0, normalised),
    4 a sparse row scaled to sum 0.5, 5 a sparse row scaled to sum 1.75, 6 all zeros, 7 an ordinary normalised sparse row --
    and z[b] = EDGE_Z[b % 8].  Nothing is renormalised: the losses are torch's CrossEntropyLoss with probability targets and MSELoss
    on whatever rows they are given."""
    rng = np.random.RandomState(seed)
    pi = np.zeros((B, A), dtype=np.float64)
    for b in range(B):
        kind = b % EDGE_ROWS
        if kind == 0:
            pi[b, A - 1] = 1.0
        elif kind == 1:
            pi[b, 0] = 1.0
        elif kind == 2:
            pi[b] = 1.0 / A
        elif kind == 3:
            row = rng.rand(A) + 0.05
            pi[b] = row / row.sum()
        elif kind in SCALED_ROWS:
            pi[b] = _sparse_row(rng, A) * SCALED_ROWS[kind]
        elif kind == 7:
            pi[b] = _sparse_row(rng, A)
    z = np.array([EDGE_Z[b % EDGE_ROWS] for b in range(B)])
    return pi.astype(np.float32), z.astype(np.float32)


def renormalised(pi):
    """`pi` with its scaled rows (kinds 4 and 5) divided by their sums; every other row as it is."""
    out = pi.astype(np.float64)
    for b in range(out.shape[0]):
        if b % EDGE_ROWS in SCALED_ROWS:
            out[b] /= out[b].sum()
    return out.astype(np.float32)


def loss_terms(p, v, pi, z):
    """The reference's losses on an (already softmaxed) policy p [B, A] and a tanh value v [B], in plain numpy fp64:
        l_b = -sum_a t_a (p_a - log sum_a' exp p_a'),   dl/dp_a = (softmax(p)_a sum(t) - t_a) / B,   dv = 2 (v - z) / B
    Returns (terms [B, 2] = (l_b, (v_b - z_b)^2), d mean(l) / dp [B, A], d mean((v - z)^2) / dv [B])."""
    p, v, pi, z = (np.asarray(x, dtype=np.float64) for x in (p, v, pi, z))
    B = p.shape[0]
    e = np.exp(p)
    s = e.sum(axis=1, keepdims=True)
    terms = np.stack([-(pi * (p - np.log(s))).sum(axis=1), (v - z) ** 2], axis=1)
    dp = ((e / s) * pi.sum(axis=1, keepdims=True) - pi) / B
    return terms, dp, 2.0 * (v - z) / B


def torch_loss_terms(p, v, pi, z):
    """The same three from torch: CrossEntropyLoss and MSELoss with autograd in fp64 (per-row terms by reduction='none')."""
    p = torch.tensor(np.asarray(p, dtype=np.float64), requires_grad=True)
    v = torch.tensor(np.asarray(v, dtype=np.float64), requires_grad=True)
    t, zz = torch.tensor(np.asarray(pi, dtype=np.float64)), torch.tensor(np.asarray(z, dtype=np.float64))
    (torch.nn.CrossEntropyLoss()(p, t) + torch.nn.MSELoss()(v, zz)).backward()
    with torch.no_grad():
        terms = torch.stack([torch.nn.CrossEntropyLoss(reduction="none")(p, t), torch.nn.MSELoss(reduction="none")(v, zz)], dim=1)
    return terms.numpy(), p.grad.numpy(), v.grad.numpy()


# ---------------------------------------------------------------- the networks the GPU tests draw from, and their one draw each
FUSED_NETS = {9: (2, 0), 5: (4, 2), 3: (4, 2)}                       # N -> (og.init_params seed, _train_batch seed)
GENERAL_NETS = [((6, 128, 3), 9), ((6, 64, 2), 9), ((6, 64, 2), 5)]  # (shape, N)


def fused_params(N, peaked=False):
    from oracle import gnn as og
    params = og.init_params(FUSED_NETS[N][0], N=N)
    if peaked:
        peaked_policy(params["policy_head.2.weight"], params["policy_head.2.bias"])
    return params


def fused_draw(N):
    """(recs [48, 72], pi, z, (drawn, dropped)) of the fused trainer's network on the N x N board: test_gpu_parity._train_batch at
    48, which asserts KINK_DROP_BOUND on the 96 positions it draws."""
    from tests.test_gpu_parity import _kink_dropped, _train_batch
    seed = FUSED_NETS[N][1]
    recs, pi, z = _train_batch(DRAW, seed, N=N, params=fused_params(N))
    return np.ascontiguousarray(recs), pi, z, _kink_dropped[(DRAW, seed, N)]


def general_net(shape, N, device="cpu", peaked=False):
    """test_train_general._net (test_gnn_any_shape._make_net with its GCN biases moved off zero), built on the CPU so that the draw
    can be judged without a GPU: the same weights, torch's CPU generator seeds both."""
    from alphaquoridorgnn_amd.pv_network_gnn import GraphPolicyValueNetwork
    torch.manual_seed(7 * sum(shape) + N)
    net = GraphPolicyValueNetwork(*shape, policy_size(N), board_size=N)
    with torch.no_grad():
        for l, layer in enumerate(net.gcn_layers):
            layer.bias.copy_(torch.linspace(-0.3, 0.5, layer.out_channels) * (1 + 0.5 * l))
            layer.bias.add_(0.00317)
        if peaked:
            peaked_policy(net.policy_head[2].weight, net.policy_head[2].bias)
    return net.to(device).eval()


def general_seed(shape, N):
    return N + shape[1]


def general_draw(net, shape, N):
    """(recs [48, 72], pi, z, (drawn, dropped)) of an any-shape network: test_train_general._batch at 48, and the share of its
    candidates the kink filter dropped (restated here: _batch keeps no record of it)."""
    from tests.test_gpu_parity import KINK_MARGIN, _walk_states
    from tests.test_train_general import _batch, _params64, _ref_forward
    seed = general_seed(shape, N)
    recs, pi, z = _batch(net, N, DRAW, seed)
    rng = np.random.RandomState(seed)
    pool = _walk_states(N, 4 * DRAW, seed + 100)
    cand = pool[rng.choice(pool.shape[0], min(3 * DRAW, pool.shape[0]), replace=False)]
    with torch.no_grad():
        margin = _ref_forward(_params64(net), net.num_gcn_layers, cand)[2]
    return recs, pi, z, (cand.shape[0], int((margin < KINK_MARGIN).sum()))


GNN_POLICY_SCALE = 32.0      # the last policy layer of the networks of the target-edge tests is scaled by these (peaked_policy):
CNN_POLICY_SCALE = 6.0       # a GNN's logits at initialisation spread by ~0.1, the CNN's (BatchNorm in front) by ~0.5


def peaked_policy(weight, bias, scale=GNN_POLICY_SCALE):
    """Scale the policy head's last linear layer in place, so that the network's policy is peaked (largest entries 0.1 .. 0.5 instead
    of ~1 / A everywhere).  The reference's loss softmaxes the softmaxed policy again: under a near-uniform policy that second softmax
    is constant to ~1e-5, the first softmax's backward removes constants, and the target-sum factor of d loss / d policy -- the very
    term the target-edge tests exist for -- moves no gradient by more than a tenth of the bar.  No ReLU follows this layer: the kink
    filter's verdict on a position does not change."""
    for t in (weight, bias):
        t *= scale


def policy_loss(policy, target, drop_target_sum=False):
    """CrossEntropyLoss()(policy, target) for probability targets, written out: mean_b (-sum_a t_a p_a + sum(t) logsumexp(p)).  With
    drop_target_sum the sum(t) is left out: the loss whose gradient a kernel computes that forgot the factor."""
    lse = torch.logsumexp(policy, dim=1)
    return (-(target * policy).sum(dim=1) + (lse if drop_target_sum else target.sum(dim=1) * lse)).mean()


def gnn_step(params, L, recs, pi, z, dtype=torch.float64, drop_target_sum=False):
    """One step of the L-layer GNN in stock torch on the CPU in `dtype` (the statement of oracle/train.py and
    test_train_general._ref_step, which are fp64 only): ({key: gradient as fp64 numpy}, policy_loss, value_loss).  In float32 it
    is the stock step whose error against fp64 the gradient bar may fall back on; in float64 it equals both references."""
    from tests.test_train_general import _dense
    p = {k: torch.as_tensor(np.asarray(v.detach().cpu() if torch.is_tensor(v) else v)).to(dtype).requires_grad_(True)
         for k, v in params.items()}
    x, adj = (t.to(dtype) for t in _dense(recs))
    h = x
    for l in range(L):
        h = torch.relu(adj @ (h @ p[f"gcn_layers.{l}.lin.weight"].T) + p[f"gcn_layers.{l}.bias"])
    g = h.mean(dim=1)
    hp = torch.relu(g @ p["policy_head.0.weight"].T + p["policy_head.0.bias"])
    hv = torch.relu(g @ p["value_head.0.weight"].T + p["value_head.0.bias"])
    policy = torch.softmax(hp @ p["policy_head.2.weight"].T + p["policy_head.2.bias"], dim=1)
    value = torch.tanh(hv @ p["value_head.2.weight"].T + p["value_head.2.bias"])
    target = torch.as_tensor(np.asarray(pi)).to(dtype)
    pl = policy_loss(policy, target, True) if drop_target_sum else torch.nn.CrossEntropyLoss()(policy, target)
    vl = torch.nn.MSELoss()(value.view(-1), torch.as_tensor(np.asarray(z)).to(dtype))
    (pl + vl).backward()
    return {k: v.grad.double().numpy() for k, v in p.items()}, float(pl.detach()), float(vl.detach())


GRAD_BAR = 2e-5        # every gradient tensor within GRAD_BAR * max|g_ref| + GRAD_ABS of fp64 autograd (the GNN trainers' bar)
GRAD_ABS = 1e-7


def grad_error(g, r):
    """max|g - r| of one tensor in the unit of the bar: <= GRAD_BAR exactly when max|g - r| <= GRAD_BAR max|r| + GRAD_ABS."""
    g, r = np.asarray(g, dtype=np.float64), np.asarray(r, dtype=np.float64)
    return GRAD_BAR * np.abs(g - r).max() / (GRAD_BAR * np.abs(r).max() + GRAD_ABS)


def cnn_net(F, L, N, peaked=False):
    """test_cnn._make_net (on the CPU, eval mode) as the edge tests seed it; peaked: its policy head's linear layer scaled."""
    from tests.test_cnn import _make_net
    net = _make_net(F, L, N, seed=F * 10 + L + N)
    if peaked:
        with torch.no_grad():
            peaked_policy(net.policy_head[1].weight, net.policy_head[1].bias, CNN_POLICY_SCALE)
    return net


def cnn_step(net, recs, pi, z, drop_target_sum=False):
    """test_cnn_train._ref_step's gradients (fp64, train mode, CPU), with the policy loss written out so that the target-sum factor
    can be dropped."""
    import copy
    from tests.test_cnn_cpu import _triples
    m = copy.deepcopy(net).cpu().double().train()
    policy, value = m._forward_stock(torch.from_numpy(m.preprocess_input(_triples(recs, net.board_size))).double())
    pl = policy_loss(policy, torch.from_numpy(np.asarray(pi)).double(), drop_target_sum)
    (pl + torch.nn.MSELoss()(value.view(-1), torch.from_numpy(np.asarray(z)).double())).backward()
    return [p.grad.numpy() for p in m.parameters()]
