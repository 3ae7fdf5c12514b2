"""The three training steps -- the fused 6/128/3 step (GNNTrainer), the any-shape GNN step (GeneralTrainer) and the residual CNN's
(CNNTrainer) -- where the pipeline takes them and the other tests do not: batches of 1, 2, 3, 5 and 9 (train_final_kernel's board
groups empty, or starting at or past the end: tests/_train_edges.py), a small step in a workspace a large one has dirtied, an epoch
whose last batch is one row, and policy / value targets at their edges (mass on the last action, dense rows, rows that do not sum
to 1, an all-zero row, fractional z).  References and bars are the project's: fp64 torch autograd of the same module on the CPU
(oracle/train.py, test_train_general._ref_step, test_cnn_train._ref_step).  Every tiny GNN batch is a prefix of ONE kink-filtered
draw of 48 per network (test_train_batch_edges_cpu.py judges the filter's cap on that draw).  Each case prints its worst gradient
error ("worst") beside the bar and the error of the stock fp32 CPU step of the same batch."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import _train_edges as E   # noqa: E402
from tests.test_cnn import BAR, _make_net as _make_cnn, _states   # noqa: E402  (_make_cnn: sections B and C)
from tests.test_cnn_train import GRAD_REL, _ref_step as _cnn_ref_step, _rel, _targets   # noqa: E402
from tests.test_gpu_parity import TRAIN_FUSED_DEFAULT, _train_batch   # noqa: E402
from tests.test_train_general import _net, _params64, _ref_forward, _ref_step as _general_ref_step   # noqa: E402

pytestmark = pytest.mark.gpu

ROW_REL, ROW_ABS = 1e-5, 1e-7        # per-position loss terms: the absolute part is what an all-zero target row (term 0) needs


@pytest.fixture(scope="module")
def dev():
    from alphaquoridorgnn_amd import _lib
    _lib.load()
    return _lib.require_gpu()


class _fused_form:
    """`with _fused_form(f):` -- the train_fused option set to f, and back at the default afterwards."""

    def __init__(self, form):
        self.form = form

    def __enter__(self):
        from alphaquoridorgnn_amd import _lib
        _lib.set_option("train_fused", self.form)

    def __exit__(self, *exc):
        from alphaquoridorgnn_amd import _lib
        _lib.set_option("train_fused", TRAIN_FUSED_DEFAULT)


def _poison(tr, dev, everything=False):
    """NaN in LDS and in the trainer's workspace (the fused trainer: every ws tensor; the other two: the workspace buffer, and with
    `everything` their output tensors too), so that a read of something this call did not write shows."""
    from alphaquoridorgnn_amd import _lib
    _lib.poison_lds(dev)
    for k, x in tr.ws.items():
        if "workspace" not in tr.ws or k == "workspace" or (everything and k != "loss_mean"):
            x.fill_(float("nan"))


def _dev(dev, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


# ---------------------------------------------------------------- the networks, each with its one draw (module-wide, never changed)
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _fused_model(N, dev, peaked=False):
    from alphaquoridorgnn_amd.pv_network_gnn import GNNNetwork, GraphPolicyValueNetwork
    params = E.fused_params(N, peaked)
    model = GNNNetwork() if N == 9 else GraphPolicyValueNetwork(policy_output_size=E.policy_size(N), board_size=N)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in params.items()})
    return model.to(dev).eval(), params


def _fused_case(N, form, dev, peaked=False):
    """(model, params, trainer with max_batch 16, the draw) of one form of the fused trainer on the N x N board; peaked: the
    network of the target-edge tests (_train_edges.peaked_policy: the same kink margins, so the same draw)."""
    from alphaquoridorgnn_amd.train_network import GNNTrainer

    def make():
        model, params = _fused_model(N, dev, peaked)
        with _fused_form(form):
            tr = GNNTrainer(model, max_batch=16)
        return model, params, tr, _cached(("fused draw", N), lambda: E.fused_draw(N))
    return _cached(("fused", N, form, peaked), make)


def _general_case(shape, N, dev, peaked=False):
    from alphaquoridorgnn_amd.train_network import GeneralTrainer

    def make():
        net = _net(shape, E.policy_size(N), seed=7 * sum(shape) + N, N=N)
        if peaked:
            with torch.no_grad():
                E.peaked_policy(net.policy_head[2].weight, net.policy_head[2].bias)
        cpu = E.general_net(shape, N, peaked=peaked)      # the network whose draw the CPU test judged: the same weights
        for (k, a), (_, b) in zip(net.state_dict().items(), cpu.state_dict().items()):
            assert torch.equal(a.cpu(), b), k
        return net, GeneralTrainer(net, max_batch=16), E.general_draw(net, shape, N)
    return _cached(("general", shape, N, peaked), make)


def _cnn_case(F, L, N, dev, peaked=False):
    from alphaquoridorgnn_amd.train_network import CNNTrainer

    def make():
        net = E.cnn_net(F, L, N, peaked).to(dev)
        return net, CNNTrainer(net, max_batch=16), _states(N, 16)
    return _cached(("cnn", F, L, N, peaked), make)


# ---------------------------------------------------------------- one step against fp64
def _check_rows(tr, B, policy_ref, value_ref, pi, z, what):
    """ws['loss'][:B] = (l_b, (v_b - z_b)^2) of every position against the numpy statement on the fp64 reference's outputs."""
    terms = E.loss_terms(policy_ref, value_ref, pi, z)[0]
    got = tr.ws["loss"][:B].double().cpu().numpy()
    assert got.shape == terms.shape
    assert (np.abs(got - terms) <= ROW_REL * np.abs(terms) + ROW_ABS).all(), (what, got, terms)


def _check_gnn_grads(keys, grads, g_ref, g_stock, what):
    """Every gradient tensor within GRAD_BAR max|g_ref| + GRAD_ABS -- or, where the stock fp32 CPU step of the same batch is itself
    further from fp64 than a quarter of that, within 4 x its error.  Prints the worst error in the bar's unit."""
    stock = max(E.grad_error(g_stock[k], r) for k, r in zip(keys, g_ref))
    bar = max(E.GRAD_BAR, 4 * stock)
    errs = {k: E.grad_error(g.cpu().numpy(), r) for k, g, r in zip(keys, grads, g_ref)}
    worst = max(errs, key=errs.get)
    print(f"{what}: worst {errs[worst]:.3g} at {worst} (bar {bar:.3g}, stock fp32 {stock:.3g})")
    assert all(np.isfinite(g.cpu().numpy()).all() for g in grads), what
    assert errs[worst] <= bar, (what, worst, errs[worst], stock)


def _step_fused(model, params, tr, form, recs, pi, z, dev, what, fallbacks=True):
    """One update=False step of the fused trainer (workspace and LDS poisoned) against oracle/train.py at the project's bars.
    Returns the gradients (fp64 numpy) and the reference's."""
    from alphaquoridorgnn_amd import _lib
    from oracle import gnn as og, train as ot
    lib, B = _lib.load(), recs.shape[0]
    _poison(tr, dev)
    with _fused_form(form):
        lib.aqg_gcn_train_fallbacks(1)
        pl, vl = tr.step(*_dev(dev, recs, pi, z), update=False)
        redone = lib.aqg_gcn_train_fallbacks(1)
    if fallbacks:
        assert redone == (B if form == 3 else 0), (what, redone)
    pi64, z64 = pi.astype(np.float64), z.astype(np.float64)
    ref = ot.train_steps(params, [(recs, pi64, z64)])[0]
    pol, val = tr.outputs(B)
    np.testing.assert_allclose(pol.cpu().numpy(), ref["policy"], atol=1e-6, rtol=1e-4, err_msg=what)
    np.testing.assert_allclose(val.cpu().numpy(), ref["value"], atol=1e-5, rtol=1e-4, err_msg=what)
    assert abs(float(pl) - ref["policy_loss"]) <= 1e-5 * abs(ref["policy_loss"]), (what, float(pl), ref["policy_loss"])
    assert abs(float(vl) - ref["value_loss"]) <= 1e-5 * abs(ref["value_loss"]) + 1e-7, (what, float(vl), ref["value_loss"])
    _check_rows(tr, B, ref["policy"], ref["value"], pi64, z64, what)
    g_ref = [ref["grads"][k] for k in og.KEYS]
    _check_gnn_grads(og.KEYS, tr.grads, g_ref, E.gnn_step(params, 3, recs, pi64, z64, torch.float32)[0], what)
    return [g.double().cpu().numpy() for g in tr.grads], g_ref


def _step_general(net, tr, recs, pi, z, dev, what):
    """The same for GeneralTrainer against test_train_general._ref_step; policy and value bit-identical to the any-shape forward."""
    B = recs.shape[0]
    S, P, Z = _dev(dev, recs, pi, z)
    _poison(tr, dev)
    pl, vl = tr.step(S, P, Z, update=False)
    pi64, z64 = pi.astype(np.float64), z.astype(np.float64)
    g_ref, pl_ref, vl_ref = _general_ref_step(net, recs, pi64, z64)
    assert abs(float(pl) - pl_ref) <= 1e-5 * abs(pl_ref), (what, float(pl), pl_ref)
    assert abs(float(vl) - vl_ref) <= 1e-5 * abs(vl_ref) + 1e-7, (what, float(vl), vl_ref)
    with torch.no_grad():
        policy_ref, value_ref, _ = _ref_forward(_params64(net), net.num_gcn_layers, recs)
    pol, val = tr.outputs(B)
    np.testing.assert_allclose(pol.cpu().numpy(), policy_ref.numpy(), atol=1e-6, rtol=1e-4, err_msg=what)
    np.testing.assert_allclose(val.cpu().numpy(), value_ref.numpy()[:, 0], atol=1e-5, rtol=1e-4, err_msg=what)
    pol, val = pol.clone(), val.clone()
    if net.fused:            # forward_states of the default shape takes the fused kernels: the any-shape forward is the identical one
        fpol, fval = net._forward_states_general(S, False, 0)
    else:
        fpol, fval = net.forward_states(S)
    assert torch.equal(pol, fpol) and torch.equal(val, fval[:, 0]), what
    _check_rows(tr, B, policy_ref.numpy(), value_ref.numpy()[:, 0], pi64, z64, what)
    keys = [k for k, _ in net._ordered_params()]
    _check_gnn_grads(keys, tr.grads, g_ref, E.gnn_step(net.state_dict(), net.num_gcn_layers, recs, pi64, z64, torch.float32)[0], what)
    return [g.double().cpu().numpy() for g in tr.grads], g_ref


def _step_cnn(net, tr, recs, pi, z, dev, what):
    """test_cnn_train._check_step on given targets, with the per-position loss terms: outputs and running statistics at BAR, the
    gradients at max(GRAD_REL, 4 x the stock fp32 CPU step's error)."""
    N, B = net.board_size, recs.shape[0]
    outs, losses, g_ref, m64 = _cnn_ref_step(net, recs, pi, z, N)
    stock = max(_rel(g, r) for g, r in zip(_cnn_ref_step(net, recs, pi, z, N, torch.float32)[2], g_ref))
    nbt = [int(bn.num_batches_tracked) for bn in tr.bns]
    _poison(tr, dev)
    pl, vl = tr.step(*_dev(dev, recs, pi, z), update=False)
    assert abs(float(pl) - losses[0]) <= 1e-5 * abs(losses[0]), (what, float(pl), losses[0])
    assert abs(float(vl) - losses[1]) <= 1e-5 * abs(losses[1]) + 1e-7, (what, float(vl), losses[1])
    pol, val = tr.outputs(B)
    np.testing.assert_allclose(pol.cpu().numpy(), outs[0], **BAR, err_msg=what)
    np.testing.assert_allclose(val.cpu().numpy(), outs[1], **BAR, err_msg=what)
    _check_rows(tr, B, outs[0], outs[1], pi, z, what)
    bar = max(GRAD_REL, 4 * stock)
    errs = {k: _rel(g.cpu().numpy(), r) for (k, _), g, r in zip(net.named_parameters(), tr.grads, g_ref)}
    worst = max(errs, key=errs.get)
    print(f"{what}: worst {errs[worst]:.3g} at {worst} (bar {bar:.3g}, stock fp32 {stock:.3g})")
    assert errs[worst] <= bar, (what, worst, errs[worst], stock)
    for bn, bn64, n0 in zip(tr.bns, [cb.bn for cb in m64._convs()], nbt):
        np.testing.assert_allclose(bn.running_mean.cpu().numpy(), bn64.running_mean.numpy(), **BAR, err_msg=what)
        np.testing.assert_allclose(bn.running_var.cpu().numpy(), bn64.running_var.numpy(), **BAR, err_msg=what)
        assert int(bn.num_batches_tracked) == n0 + 1 == int(bn64.num_batches_tracked), what
    return [g.double().cpu().numpy() for g in tr.grads], g_ref


# ---------------------------------------------------------------- A. tiny batches against fp64
FUSED_TINY = ([(9, form, B) for form in (2, 1, 3) for B in E.TINY_BATCHES]
              + [(N, 1, B) for N in (5, 3) for B in (1, 5)])


@pytest.mark.parametrize("N,form,B", FUSED_TINY, ids=[f"{N}x{N}-form{f}-B{B}" for N, f, B in FUSED_TINY])
def test_fused_step_tiny_batch_vs_fp64(dev, N, form, B):
    """One trainer per form (max_batch 16), batches ascending; train_final_kernel's groups 1 .. 3 are empty (B < 4), its last group
    starts past the end (5) or at it (9).  Form 3 redoes exactly B positions in f32, form 2 none."""
    model, params, tr, (recs, pi, z, _) = _fused_case(N, form, dev)
    _step_fused(model, params, tr, form, recs[:B], pi[:B], z[:B], dev, f"fused {N}x{N} form {form} B{B}")


GENERAL_TINY = [(s, N, B) for s, N in E.GENERAL_NETS for B in E.TINY_BATCHES]


@pytest.mark.parametrize("shape,N,B", GENERAL_TINY, ids=["x".join(map(str, s)) + f"-{N}x{N}-B{B}" for s, N, B in GENERAL_TINY])
def test_general_step_tiny_batch_vs_fp64(dev, shape, N, B):
    """The width-generic primitives composed at M = 1 head GEMMs and M = V trunk GEMMs (B = 1) and just above."""
    net, tr, (recs, pi, z, _) = _general_case(shape, N, dev)
    _step_general(net, tr, recs[:B], pi[:B], z[:B], dev, f"general {shape} {N}x{N} B{B}")


CNN_TINY = [(16, 2, 3, B) for B in (1, 2, 3, 5)] + [(7, 1, 5, B) for B in (2, 3)]


@pytest.mark.parametrize("F,L,N,B", CNN_TINY, ids=[f"{F}x{L}-{N}x{N}-B{B}" for F, L, N, B in CNN_TINY])
def test_cnn_step_tiny_batch_vs_fp64(dev, F, L, N, B):
    """At B = 1 on 3x3 a BatchNorm channel has 9 values in all: the unbiased variance of the running statistics divides by 8."""
    net, tr, recs = _cnn_case(F, L, N, dev)
    pi, z = _targets(B, E.policy_size(N), seed=B)
    _step_cnn(net, tr, recs[:B].copy(), pi, z, dev, f"cnn {F}x{L} {N}x{N} B{B}")


# ---------------------------------------------------------------- B. a small step after a large one reads nothing stale
class _Kind:
    """One trainer kind of sections B and C: identical fresh networks, a trainer on one, data, and the tensors a step leaves."""

    def __init__(self, name, N, dev):
        self.name, self.N, self.dev = name, N, dev
        self.form = int(name[-1]) if name.startswith("fused") else None

    def net(self):
        if self.form is not None:
            return _fused_model(self.N, self.dev)[0]
        if self.name == "general":
            return _net((6, 64, 2), E.policy_size(self.N), seed=77, N=self.N)
        return _make_cnn(16, 2, self.N, seed=33).to(self.dev)

    def trainer(self, net, max_batch):
        from alphaquoridorgnn_amd.train_network import CNNTrainer, GeneralTrainer, GNNTrainer
        cls = GNNTrainer if self.form is not None else GeneralTrainer if self.name == "general" else CNNTrainer
        return cls(net, max_batch=max_batch)

    def data(self, n, seed):
        if self.name == "cnn":
            return _dev(self.dev, _states(self.N, n), *_targets(n, E.policy_size(self.N), seed))
        return _dev(self.dev, *_train_batch(n, seed, N=self.N))       # bit-identity needs no reference: no kink filter

    def step(self, tr, S, P, Z, **kw):
        if self.form is None:
            return tr.step(S, P, Z, **kw)
        with _fused_form(self.form):
            return tr.step(S, P, Z, **kw)

    def run_epoch(self, tr, *a, **kw):
        if self.form is None:
            return tr.run_epoch(*a, **kw)
        with _fused_form(self.form):
            return tr.run_epoch(*a, **kw)

    @staticmethod
    def left(tr, B, losses):
        """Everything an update=False step leaves: losses, per-position terms, outputs, every gradient, running statistics."""
        pol, val = tr.outputs(B)
        return [x.detach().clone() for x in (*losses, tr.ws["loss"][:B], pol, val, tr.flat_grads, *tr.buffers)]

    @staticmethod
    def state(tr):
        return [x.detach().clone() for x in (*tr.params, *tr.adam_m, *tr.adam_v, *tr.buffers)]


def _same(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), (what, i, float((x.double() - y.double()).abs().max()))


STALE = [("fused2", 9), ("fused1", 9), ("general", 9), ("cnn", 5)]


@pytest.mark.parametrize("name,N", STALE, ids=[n for n, _ in STALE])
def test_small_step_after_large_reads_nothing_stale(dev, name, N):
    """A trainer with max_batch 64 steps at 64, then at 1 and at 5: bit for bit what fresh trainers with max_batch = B give on
    identical networks (losses, loss terms, outputs, gradients, running statistics); the step at 5 again with every workspace tensor
    NaN: the same bits; an updating step at 5: parameters and Adam moments bit-identical to the fresh trainer's."""
    kind = _Kind(name, N, dev)
    S, P, Z = kind.data(64, seed=5)
    net = kind.net()
    T = kind.trainer(net, 64)
    stats0 = [b.detach().clone() for b in T.buffers]

    def from_start(tr):                   # the CNN's running statistics move with every forward: each step starts from the same ones
        for b, s in zip(tr.buffers, stats0):
            b.copy_(s)

    _same(stats0, [b.detach().clone() for b in kind.trainer(kind.net(), 1).buffers], "identical networks")
    kind.step(T, S, P, Z, update=False)
    assert all(torch.isfinite(g).all() for g in T.grads)
    fresh = {}
    for B in (1, 5):
        s, p, z = S[7:7 + B].contiguous(), P[7:7 + B].contiguous(), Z[7:7 + B].contiguous()
        from_start(T)
        after_large = kind.left(T, B, kind.step(T, s, p, z, update=False))
        fresh[B] = kind.trainer(kind.net(), B)
        alone = kind.left(fresh[B], B, kind.step(fresh[B], s, p, z, update=False))
        assert all(torch.isfinite(x).all() for x in alone)
        _same(after_large, alone, f"{name} B{B} after B64 against a fresh trainer")
    _poison(T, dev, everything=True)
    from_start(T)
    _same(kind.left(T, 5, kind.step(T, s, p, z, update=False)), after_large, f"{name} B5 in a NaN workspace")
    from_start(T)
    from_start(fresh[5])
    before = [x.detach().clone() for x in T.params]
    kind.step(T, s, p, z, lr=1e-3)
    kind.step(fresh[5], s, p, z, lr=1e-3)
    assert T.step_count == fresh[5].step_count == 1
    assert any(not torch.equal(a, b) for a, b in zip(T.params, before))            # the step did update
    _same(kind.state(T), kind.state(fresh[5]), f"{name} updating step at B5")


# ---------------------------------------------------------------- C. an epoch whose last batch is one row
EPOCHS = [("fused2", 5, 32), ("fused2", 9, 16), ("general", 5, 32), ("cnn", 5, 32)]
EPOCH_CASES = [(name, N, batch, rows, pre) for name, N, batch in EPOCHS for rows in ("2b+1", "b", "1") for pre in (True, False)]
EPOCH_RTOL = {"fused2": 1e-5, "general": 1e-5, "cnn": 1e-6}      # the bars of the three existing epoch tests


@pytest.mark.parametrize("name,N,batch,rows,pre_shuffle", EPOCH_CASES,
                         ids=[f"{n}-{N}x{N}-b{b}-n{r}-{'shuffled' if p else 'order'}" for n, N, b, r, p in EPOCH_CASES])
def test_epoch_with_a_one_row_last_batch_equals_single_steps(dev, name, N, batch, rows, pre_shuffle):
    """run_epoch over n = 2 batch + 1 rows (the last batch is one row), n = batch (no short batch) and n = 1, in both order forms:
    parameters, Adam moments and running statistics bit-identical to step() on the same batches, the returned sums within the
    existing rtol of the summed step losses, step_count advanced by the number of batches."""
    kind = _Kind(name, N, dev)
    n = {"2b+1": 2 * batch + 1, "b": batch, "1": 1}[rows]
    S, P, Z = kind.data(n, seed=21)
    order = torch.from_numpy(np.random.RandomState(3).permutation(n))
    ma, mb = kind.net(), kind.net()
    ta, tb = kind.trainer(ma, batch), kind.trainer(mb, batch)
    sums = kind.run_epoch(ta, S, P, Z, order, lr=7e-4, pre_shuffle=pre_shuffle)
    ref = torch.zeros(2, device=dev)
    od = order.to(dev)
    for i in range(0, n, batch):
        idx = od[i:i + batch]
        pl, vl = kind.step(tb, S[idx], P[idx], Z[idx], lr=7e-4)
        ref += torch.stack([pl, vl])
    steps = (n + batch - 1) // batch
    assert steps == {"2b+1": 3, "b": 1, "1": 1}[rows] and ta.step_count == tb.step_count == steps
    _same(kind.state(ta), kind.state(tb), f"{name} {N}x{N} n={n}")
    assert all(torch.isfinite(x).all() for x in kind.state(ta))
    np.testing.assert_allclose(sums.cpu().numpy(), ref.cpu().numpy(), rtol=EPOCH_RTOL[name])
    if name == "cnn":
        assert all(int(bn.num_batches_tracked) == steps for bn in ta.bns + tb.bns)


# ---------------------------------------------------------------- D. target edges against fp64
EDGES = [("fused2", 9), ("fused1", 9), ("fused3", 9), ("fused1", 5), ("general", 9), ("cnn", 5)]


def _moved(g, r, rel):
    """How far gradient tensor g lies from r, in the unit of its trainer's bar (GRAD_BAR for the GNNs, GRAD_REL for the CNN)."""
    return _rel(g, r) if rel else E.grad_error(g, r)


@pytest.mark.parametrize("name,N", EDGES, ids=[f"{n}-{N}x{N}" for n, N in EDGES])
def test_target_edges_vs_fp64(dev, name, N):
    """A batch of the eight rows of _train_edges.edge_targets (B = 8) at the usual bars: all mass on action A - 1 (on 9x9 lane 16 of
    the fourth logit of a lane, and the tail of the 256-thread stride), on action 0, dense rows, rows summing to 0.5 and 1.75 (the
    target-sum factor of the double-softmax gradient), an all-zero row (loss term exactly 0) and fractional z -- on networks whose
    last policy layer is scaled (_train_edges.peaked_policy): under the near-uniform policy of fresh weights that factor moves no
    gradient by a tenth of the bar, and its loss would go unseen (test_train_batch_edges_cpu.py shows both).  Then the same batch
    with the two scaled rows renormalised: the gradients move by more than the bar -- in the reference first, then in the kernels --
    so this test sees the target-sum term."""
    A = E.policy_size(N)
    pi, z = E.edge_targets(8, A, seed=N)
    if name == "cnn":
        net, tr, recs = _cnn_case(16, 2, N, dev, peaked=True)
        run = lambda t, what: _step_cnn(net, tr, recs[:8].copy(), t, z, dev, what)                      # noqa: E731
    elif name == "general":
        net, tr, (recs, _, _, _) = _general_case((6, 64, 2), N, dev, peaked=True)
        run = lambda t, what: _step_general(net, tr, recs[:8], t, z, dev, what)                         # noqa: E731
    else:
        form = int(name[-1])
        model, params, tr, (recs, _, _, _) = _fused_case(N, form, dev, peaked=True)
        run = lambda t, what: _step_fused(model, params, tr, form, recs[:8], t, z, dev, what)           # noqa: E731
    g, g_ref = run(pi, f"edges {name} {N}x{N}")
    assert float(tr.ws["loss"][6, 0]) == 0.0                                       # the all-zero row
    g2, g2_ref = run(E.renormalised(pi), f"edges {name} {N}x{N}, rows 4 and 5 renormalised")
    rel = name == "cnn"
    bar = GRAD_REL if rel else E.GRAD_BAR
    moved = [i for i, (a, b) in enumerate(zip(g2_ref, g_ref)) if _moved(a, b, rel) > 10 * bar]
    assert moved, "the reference's gradients do not depend on the target sums: the inputs are wrong"
    for i in moved:
        assert _moved(g2[i], g[i], rel) > bar, (name, i)
