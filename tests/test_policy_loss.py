"""The loss form (include/aqgnn.h "loss form") on the GPU: the cross-entropy kernel alone inside NaN margins, one gradient step of
each trainer against fp64 autograd of the same network under torch's statement, three Adam steps with a value weight against torch's
Adam fed the fp64 gradients, the identities with the option off, the loop end to end, and the refusals."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import _policy_loss as PL   # noqa: E402
from tests import _train_edges as E    # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from alphaquoridorgnn_amd import _lib
    _lib.load()
    return _lib.require_gpu()


def _host(tensors):
    return [x.detach().cpu().numpy().copy() for x in tensors]


def _state(tr):
    return [x.detach().clone() for x in tr.params + tr.adam_m + tr.adam_v + getattr(tr, "buffers", [])]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------- 1. the kernel alone
MARGIN = 64
SIZES = (1, 17, 63, 64, 65, 209, 255, 256, 257, 1025)
# the target table: row kinds of edge_targets in this order, with the underflow row U in third place
TABLE_KINDS = (7, 6, "U", 3, 4, 5, 2, 0, 1)
ORDER = (8, 2, 1, 3, 7, 5)            # with an order and first = 1: U, the all-zero row, dense, one-hot last, sum 1.75


def _target_table(A, seed):
    pi8, z8 = E.edge_targets(8, A, seed)
    pi = np.zeros((len(TABLE_KINDS), A), np.float32)
    z = np.zeros(len(TABLE_KINDS), np.float32)
    for r, kind in enumerate(TABLE_KINDS):
        if kind == "U":
            pi[r, 0] = 1.0                 # all its mass on action 0, which the logits of its position put 110 below the maximum
            z[r] = -0.25
        else:
            pi[r], z[r] = pi8[kind], z8[kind]
    return pi, z


@pytest.mark.parametrize("ordered", [False, True], ids=["rows", "order"])
@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("A", SIZES)
def test_kernel_alone_inside_nan_margins(dev, A, B, ordered):
    """aqg_policy_value_loss at every A around the workgroup's 256 threads and B = 1, 3, 5, the rows taken in place (first = 1) and
    through an order, with NaN margins around all three outputs: terms, d loss / d logits and d loss / d pre-tanh value against
    loss_reference on the same f32 inputs at the project's bars; the all-zero row exactly zero; a row whose target sits 110 logit
    units below the maximum (its p underflows in f32) finite and within the bar; nothing written outside the outputs."""
    from alphaquoridorgnn_amd import _lib
    from alphaquoridorgnn_amd.train_reference import loss_reference
    lib = _lib.load()
    w = 0.25
    pi, z = _target_table(A, seed=A)
    rows = [ORDER[1 + b] for b in range(B)] if ordered else [1 + b for b in range(B)]
    rng = np.random.RandomState(1000 * A + 10 * B + ordered)
    logits = (rng.randn(B, A) * 3.0).astype(np.float32)
    value = np.tanh(rng.randn(B)).astype(np.float32)
    for b, r in enumerate(rows):
        if TABLE_KINDS[r] == "U" and A > 1:
            logits[b, 0], logits[b, A - 1] = -50.0, 60.0
    ref = loss_reference(logits, value, pi[rows], z[rows], policy_form=1, value_weight=w)
    if A > 1 and "U" in [TABLE_KINDS[r] for r in rows]:
        b = [TABLE_KINDS[r] for r in rows].index("U")
        assert ref[0][b, 0] >= 104.0 and np.exp(np.float32(-110.0)) * 1.0 < np.finfo(np.float32).tiny
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)      # noqa: E731
    L, VAL, PI, Z = d(logits), d(value), d(pi), d(z)
    order = d(np.array(ORDER, np.int64)) if ordered else None
    sizes = (2 * B, B * A, B)
    buf = torch.full((sum(sizes) + 4 * MARGIN,), float("nan"), dtype=torch.float32, device=dev)
    outs, off = [], MARGIN
    for n in sizes:
        outs.append(buf[off:off + n])
        off += n + MARGIN
    form = _lib.LossStruct(1, w)
    _lib.check(lib.aqg_policy_value_loss(B, A, _lib.ptr(L), _lib.ptr(VAL), _lib.ptr(PI), _lib.ptr(Z), _lib.ptr(order), 1,
                                         ctypes.byref(form), *[_lib.ptr(o) for o in outs], _lib.stream_ptr(dev)),
               "aqg_policy_value_loss")
    host = buf.cpu().numpy()
    inside = np.zeros(host.shape, bool)
    off = MARGIN
    for n in sizes:
        inside[off:off + n] = True
        off += n + MARGIN
    assert np.isnan(host[~inside]).all() and np.isfinite(host[inside]).all()
    loss, dlogits, dvpre = (o.cpu().numpy().astype(np.float64) for o in outs)
    PL.assert_rows(loss.reshape(B, 2), ref[0], (A, B, ordered))
    for name, got, want in (("dlogits", dlogits.reshape(B, A), ref[1]), ("dvpre", dvpre, ref[2])):
        err = np.abs(got - want).max()
        assert err <= PL.grad_bar(want), (name, A, B, ordered, err, PL.grad_bar(want))
    for b, r in enumerate(rows):
        if TABLE_KINDS[r] == 6:
            assert loss[2 * b] == 0.0 and (dlogits.reshape(B, A)[b] == 0.0).all(), (A, B, ordered)


# ---------------------------------------------------------------------------------------------- 2. one gradient step per trainer
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _dev(dev, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _fused_case(N, peaked, dev):
    from alphaquoridorgnn_amd.pv_network_gnn import GNNNetwork, GraphPolicyValueNetwork
    from alphaquoridorgnn_amd.train_network import GNNTrainer

    def make():
        params = PL.fused_net_params(N, peaked)
        model = GNNNetwork() if N == 9 else GraphPolicyValueNetwork(policy_output_size=E.policy_size(N), board_size=N)
        model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in params.items()})
        tr = GNNTrainer(model.to(dev).eval(), max_batch=48, policy_loss="cross_entropy")
        return params, tr, _cached(("fused draw", N), lambda: PL.fused_draw(N))
    return _cached(("fused", N, peaked), make)


def _check_step(tr, keys, recs, pi, z, refs, dev, what):
    """One update=False step of `tr` under the cross-entropy against the fp64 references (grads, logits, value) of both forms."""
    from alphaquoridorgnn_amd import _lib
    from alphaquoridorgnn_amd.train_reference import loss_reference
    (g_ce, logits, value), (g_ref0, _, _) = refs
    B = recs.shape[0]
    PL.assert_forms_differ(keys, g_ce, g_ref0, what)
    _lib.poison_lds(dev)
    pl, vl = tr.step(*_dev(dev, recs, pi, z), update=False)
    terms = loss_reference(logits, value, pi, z, policy_form=1)[0]
    PL.assert_rows(tr.ws["loss"][:B].double().cpu().numpy(), terms, what)
    assert abs(float(pl) - terms[:, 0].mean()) <= 1e-5 * abs(terms[:, 0].mean()) + 1e-7, (what, float(pl))
    assert abs(float(vl) - terms[:, 1].mean()) <= 1e-5 * abs(terms[:, 1].mean()) + 1e-7, (what, float(vl))
    PL.assert_grads(keys, _host(tr.grads), g_ce, what)


FUSED = [(N, B, peaked) for N in PL.FUSED_BOARDS for B in PL.TINY_BATCHES + (48,) for peaked in (False, True)]


@pytest.mark.parametrize("N,B,peaked", FUSED, ids=[f"{N}x{N}-B{B}-{'peaked' if p else 'plain'}" for N, B, p in FUSED])
def test_fused_step_cross_entropy_vs_fp64(dev, N, B, peaked):
    """GNNTrainer(policy_loss='cross_entropy') on the four boards (A = 17 / 57 / 121 / 209), every tiny batch and 48, the rows of
    edge_targets, plain and peaked weights: per-row terms at ROW_REL / ROW_ABS, all 14 gradients at GRAD_BAR / GRAD_ABS of fp64
    autograd of torch.nn.CrossEntropyLoss()(logits, t) + MSELoss; the default form of each board (split precision on 9x9)."""
    from oracle import gnn as og
    params, tr, draw = _fused_case(N, peaked, dev)
    recs = draw[:B]
    pi, z = E.edge_targets(B, E.policy_size(N), seed=N)
    refs = [PL.gnn_reference(params, 3, recs, pi, z, form) for form in (PL.CE, PL.REFERENCE)]
    refs = [([g[k] for k in og.KEYS], lg, v) for g, lg, v in refs]
    _check_step(tr, og.KEYS, recs, pi, z, refs, dev, ("fused", N, B, peaked))


@pytest.mark.parametrize("form", [1, 3])
def test_fused_step_cross_entropy_other_bodies_9x9(dev, form):
    """The same on 9x9 through the exact-f32 board kernel (train_fused 1) and with every board sent through the split kernel's
    f32 fallback (3): each is an instantiation of its own."""
    from alphaquoridorgnn_amd import _lib
    from oracle import gnn as og
    from tests.test_gpu_parity import TRAIN_FUSED_DEFAULT
    params, tr, draw = _fused_case(9, True, dev)
    B = 5
    recs = draw[:B]
    pi, z = E.edge_targets(B, E.policy_size(9), seed=9)
    refs = [PL.gnn_reference(params, 3, recs, pi, z, f) for f in (PL.CE, PL.REFERENCE)]
    refs = [([g[k] for k in og.KEYS], lg, v) for g, lg, v in refs]
    _lib.set_option("train_fused", form)
    try:
        _check_step(tr, og.KEYS, recs, pi, z, refs, dev, ("fused body", form))
    finally:
        _lib.set_option("train_fused", TRAIN_FUSED_DEFAULT)


@pytest.mark.parametrize("N", [5, 9])
@pytest.mark.parametrize("peaked", [False, True], ids=["plain", "peaked"])
def test_general_step_cross_entropy_vs_fp64(dev, N, peaked):
    from alphaquoridorgnn_amd.train_network import GeneralTrainer
    shape, B = (6, 64, 2), 9
    net = E.general_net(shape, N, device=dev, peaked=peaked)
    recs = _cached(("general draw", N), lambda: E.general_draw(E.general_net(shape, N), shape, N)[0])[:B]
    tr = GeneralTrainer(net, max_batch=16, policy_loss="cross_entropy")
    pi, z = E.edge_targets(B, E.policy_size(N), seed=N)
    keys = [k for k, _ in net._ordered_params()]
    refs = [PL.gnn_reference(net.state_dict(), 2, recs, pi, z, form) for form in (PL.CE, PL.REFERENCE)]
    refs = [([g[k] for k in keys], lg, v) for g, lg, v in refs]
    _check_step(tr, keys, recs, pi, z, refs, dev, ("general", N, peaked))


@pytest.mark.parametrize("peaked", [False, True], ids=["plain", "peaked"])
def test_cnn_step_cross_entropy_vs_fp64(dev, peaked):
    """8 filters x 1 block at 5x5, BatchNorm on the batch statistics as in tests/test_cnn_train.py."""
    from alphaquoridorgnn_amd.train_network import CNNTrainer
    from tests.test_cnn import _states
    N, B = 5, 9
    net = E.cnn_net(8, 1, N, peaked).to(dev)
    recs = _states(N, 16)[:B]
    pi, z = E.edge_targets(B, E.policy_size(N), seed=N)
    refs = [PL.cnn_reference(net, recs, pi, z, form)[:3] for form in (PL.CE, PL.REFERENCE)]
    keys = [k for k, _ in net.named_parameters()]
    tr = CNNTrainer(net, max_batch=16, policy_loss="cross_entropy")
    _check_step(tr, keys, recs, pi, z, refs, dev, ("cnn", peaked))


# ---------------------------------------------------------------------------------------------- 2b. one step with a value weight
def _check_weighted(tr, keys, reference, recs, pi, z, form, dev, what):
    """One update=False step of `tr` with value_loss_weight = W under `form` (the reference's form with a weight has kernels of its
    own: the fused step's third instantiation, the scaling launch of the other two) against reference(form, w) = fp64 autograd's
    (grads, logits, value): per-row terms (the value term unweighted) at ROW_REL / ROW_ABS, every gradient at GRAD_BAR / GRAD_ABS.
    Guard, on the fp64 side: on each of the value head's matrices the gradients at w = W and w = 1 differ by more than 100 x the
    bar -- a step that ignored the weight would fail there by that margin."""
    from alphaquoridorgnn_amd import _lib
    from alphaquoridorgnn_amd.train_reference import loss_reference
    g_w, logits, value = reference(form, W)
    g_1 = reference(form, 1.0)[0]
    guarded = 0
    for k, a, b in zip(keys, g_w, g_1):
        if k.startswith("value_head") and np.asarray(a).ndim >= 2:
            assert np.abs(a - b).max() > 100 * PL.grad_bar(b), (what, k)
            guarded += 1
    assert guarded >= 1, what
    B = recs.shape[0]
    old = tr.policy_loss, tr.value_loss_weight
    tr.policy_loss, tr.value_loss_weight = ("cross_entropy" if form == PL.CE else "reference"), W
    try:
        _lib.poison_lds(dev)
        pl, vl = tr.step(*_dev(dev, recs, pi, z), update=False)
    finally:
        tr.policy_loss, tr.value_loss_weight = old
    terms = loss_reference(logits, value, pi, z, policy_form=form)[0]
    PL.assert_rows(tr.ws["loss"][:B].double().cpu().numpy(), terms, what)
    assert abs(float(vl) - terms[:, 1].mean()) <= 1e-5 * abs(terms[:, 1].mean()) + 1e-7, (what, float(vl))      # unweighted
    PL.assert_grads(keys, _host(tr.grads), g_w, what)


FORMS = [PL.REFERENCE, PL.CE]
FORM_IDS = ["reference", "cross_entropy"]
FUSED_WEIGHTED = [(9, 2), (9, 1), (9, 3), (5, 1), (3, 1)]        # (board, train_fused): split, exact, fallback; two smaller boards


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("N,fused", FUSED_WEIGHTED, ids=[f"{N}x{N}-fused{f}" for N, f in FUSED_WEIGHTED])
def test_fused_step_with_a_value_weight_vs_fp64(dev, N, fused, form):
    from alphaquoridorgnn_amd import _lib
    from oracle import gnn as og
    from tests.test_gpu_parity import TRAIN_FUSED_DEFAULT
    params, tr, draw = _fused_case(N, True, dev)
    B = 9
    recs = draw[:B]
    pi, z = E.edge_targets(B, E.policy_size(N), seed=N)

    def reference(f, w):
        g, lg, v = PL.gnn_reference(params, 3, recs, pi, z, f, w)
        return [g[k] for k in og.KEYS], lg, v
    _lib.set_option("train_fused", fused)
    try:
        _check_weighted(tr, og.KEYS, reference, recs, pi, z, form, dev, ("fused weighted", N, fused, form))
    finally:
        _lib.set_option("train_fused", TRAIN_FUSED_DEFAULT)


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("N", [5, 9])
def test_general_step_with_a_value_weight_vs_fp64(dev, N, form):
    from alphaquoridorgnn_amd.train_network import GeneralTrainer
    shape, B = (6, 64, 2), 9
    net = E.general_net(shape, N, device=dev, peaked=True)
    recs = _cached(("general draw", N), lambda: E.general_draw(E.general_net(shape, N), shape, N)[0])[:B]
    pi, z = E.edge_targets(B, E.policy_size(N), seed=N)
    keys = [k for k, _ in net._ordered_params()]

    def reference(f, w):
        g, lg, v = PL.gnn_reference(net.state_dict(), 2, recs, pi, z, f, w)
        return [g[k] for k in keys], lg, v
    _check_weighted(GeneralTrainer(net, max_batch=16), keys, reference, recs, pi, z, form, dev, ("general weighted", N, form))


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_cnn_step_with_a_value_weight_vs_fp64(dev, form):
    from alphaquoridorgnn_amd.train_network import CNNTrainer
    from tests.test_cnn import _states
    N, B = 5, 9
    net = E.cnn_net(8, 1, N, True).to(dev)
    recs = _states(N, 16)[:B]
    pi, z = E.edge_targets(B, E.policy_size(N), seed=N)
    keys = [k for k, _ in net.named_parameters()]
    _check_weighted(CNNTrainer(net, max_batch=16), keys, lambda f, w: PL.cnn_reference(net, recs, pi, z, f, w)[:3], recs, pi, z, form,
                    dev, ("cnn weighted", form))


# ---------------------------------------------------------------------------------------------- 3. three Adam steps, w = 0.25
KINDS =["general-5x5", "gnn-5x5", "gnn-9x9", "cnn-5x5"]
W = 0.25


def _reference_grads(tr, kind, S, P, Z, w):
    """fp64 gradients of `tr`'s network as it stands, under the cross-entropy with value weight w, in the trainer's tensor order."""
    recs, pi, z = (x.cpu().numpy() for x in (S, P, Z))
    if kind.startswith("cnn"):
        return PL.cnn_reference(tr.model, recs, pi, z, PL.CE, w)[0]
    if kind.startswith("gnn"):
        from alphaquoridorgnn_amd.pv_network_gnn import STATE_DICT_KEYS as keys
        L = 3
    else:
        keys, L = [k for k, _ in tr.model._ordered_params()], tr.model.num_gcn_layers
    g = PL.gnn_reference({k: v for k, v in tr.model.state_dict().items()}, L, recs, pi, z, PL.CE, w)[0]
    return [g[k] for k in keys]


@pytest.mark.parametrize("kind", KINDS)
def test_three_adam_steps_with_a_value_weight(dev, kind):
    """Three steps under policy_loss='cross_entropy', value_loss_weight=0.25 on the networks and batches of
    tests/test_optim_controls.py, against torch.optim.Adam on the CPU fed the fp64 gradients of the trainer's parameters at every
    step, at the project's Adam bar.  The weight is visible on the trunk's Adam path (assert_visible against the same run at w = 1:
    the trunk's gradient is a mix of both terms).  On the value head's own matrices it cannot show on an Adam path -- their gradient
    is the value term alone, w scales it uniformly, and Adam's update is invariant to the scale of a tensor's gradient (measured:
    under 1 % of their elements move by 1e-3) -- so there it is held on the gradients themselves: |g(0.25) - g(1)| = 0.75 |g(1)|
    exceeds 100 x the gradient bar on at least half of each matrix (fp64 alone; the GPU's gradients under a weight are held to
    fp64 directly by the *_step_with_a_value_weight_vs_fp64 tests above)."""
    from tests import _optim_controls as OC
    from tests.test_optim_controls import _batch, _make
    tr, N = _make(kind, dev, policy_loss="cross_entropy", value_loss_weight=W)
    names = [k for k, _ in tr.model.named_parameters()] if kind.startswith("cnn") else None
    if names is None:
        from alphaquoridorgnn_amd.pv_network_gnn import STATE_DICT_KEYS
        names = list(STATE_DICT_KEYS) if kind.startswith("gnn") else [k for k, _ in tr.model._ordered_params()]
    params0 = _host(tr.params)
    grads, grads_w1, got = [], [], []
    for i in range(3):
        S, P, Z = _batch(N, dev, i)
        grads.append(_reference_grads(tr, kind, S, P, Z, W))
        grads_w1.append(_reference_grads(tr, kind, S, P, Z, 1.0))
        tr.step(S, P, Z, lr=OC.LRS[i])
        got.append(_host(tr.params))
    ref = OC.shadow_run(params0, grads, list(OC.LRS))
    for i in range(3):
        OC.assert_adam_bar(got[i], ref[i], grads[i], OC.LRS[i], (kind, i))
    other = OC.shadow_run(params0, grads_w1, list(OC.LRS))
    trunk = [j for j, k in enumerate(names) if not k.startswith(("policy_head", "value_head"))]
    OC.assert_visible([ref[-1][j] for j in trunk], [other[-1][j] for j in trunk], [params0[j] for j in trunk], kind)
    for j, k in enumerate(names):
        if k.startswith("value_head") and params0[j].ndim >= 2:
            far = np.abs(grads[0][j] - grads_w1[0][j]) > 100 * PL.grad_bar(grads_w1[0][j])
            assert far.mean() >= 0.5, (kind, k, far.mean())


# ---------------------------------------------------------------------------------------------- 4. identities
@pytest.mark.parametrize("kind", KINDS)
def test_default_form_through_the_loss_entry_points_is_the_plain_call(dev, kind):
    """policy_loss='reference', value_loss_weight=1.0 handed to the _loss entry points as an explicit struct: parameters, moments,
    loss terms and epoch sums of the plain calls, bit for bit, after three steps and an epoch."""
    from alphaquoridorgnn_amd import _lib
    from tests.test_optim_controls import _batch, _data, _make
    plain, N = _make(kind, dev)
    forced, _ = _make(kind, dev)
    forced._loss = lambda: _lib.LossStruct(0, 1.0)
    called = []
    real = forced.lib

    class Spy:
        def __getattr__(self, name):
            called.append(name)
            return getattr(real, name)
    forced.lib = Spy()
    for i in range(3):
        S, P, Z = _batch(N, dev, i)
        a, b = plain.step(S, P, Z), forced.step(S, P, Z)
        assert torch.equal(torch.stack(a), torch.stack(b))
        assert torch.equal(plain.ws["loss"][:S.shape[0]], forced.ws["loss"][:S.shape[0]])
    S, P, Z = _data(N, dev)
    order = torch.from_numpy(np.random.RandomState(5).permutation(20)).to(dev)
    assert torch.equal(plain.run_epoch(S, P, Z, order, batch=8), forced.run_epoch(S, P, Z, order, batch=8))
    assert _same(_state(plain), _state(forced))
    assert [n for n in called if n.endswith("_loss")] == [forced._STEP + "_loss"] * 3 + [forced._STEPS + "_loss"]


@pytest.mark.parametrize("kind", KINDS)
def test_run_epoch_under_cross_entropy_equals_single_steps(dev, kind):
    from tests.test_optim_controls import _data, _make
    controls = dict(policy_loss="cross_entropy", value_loss_weight=W)
    ta, N = _make(kind, dev, **controls)
    tb, _ = _make(kind, dev, **controls)
    off, _ = _make(kind, dev)
    S, P, Z = _data(N, dev)
    n, lr, B = 20, 7e-4, 8
    order = torch.from_numpy(np.random.RandomState(3).permutation(n)).to(dev)
    for pre_shuffle in (True, False):
        sums = ta.run_epoch(S, P, Z, order, lr=lr, batch=B, pre_shuffle=pre_shuffle)
        ref = torch.zeros(2, device=dev)
        for i in range(0, n, B):
            idx = order[i:i + B]
            ref += torch.stack(tb.step(S[idx], P[idx], Z[idx], lr=lr))
        assert _same(_state(ta), _state(tb)), pre_shuffle
        np.testing.assert_allclose(sums.cpu().numpy(), ref.cpu().numpy(), rtol=1e-5)
    off.run_epoch(S, P, Z, order, lr=lr, batch=B)
    assert not _same(_state(off)[:len(off.params)], _state(ta)[:len(ta.params)])


@pytest.mark.parametrize("kind", KINDS)
def test_cross_entropy_composes_with_the_other_options(dev, kind):
    """weight_decay + max_grad_norm + an attached weight average under the cross-entropy: one step equals adam_reference (with
    clip_coefficient's factor) and weight_average_reference applied to the form-1 gradients a mode-0 call leaves, at the Adam bar."""
    from alphaquoridorgnn_amd.train_network import (WeightAverage, adam_reference, clip_coefficient, default_decay_mask,
                                                    weight_average_reference)
    from tests import _optim_controls as OC
    from tests.test_optim_controls import _batch, _make
    wd, lr, decay = 0.1, 1e-3, 0.9
    tr, N = _make(kind, dev, policy_loss="cross_entropy", value_loss_weight=W, weight_decay=wd, decoupled=True, max_grad_norm=1.0)
    plain, _ = _make(kind, dev, policy_loss="cross_entropy", value_loss_weight=W)
    S, P, Z = _batch(N, dev, 0)
    tr.step(S, P, Z, update=False)
    plain.step(S, P, Z, update=False)
    assert torch.equal(tr.flat_grads, plain.flat_grads)                     # mode 0: the form-1 gradients, never scaled
    norm = float(tr.last_grad_norm)
    g = _host(tr.grads)
    assert abs(norm - OC.global_norm64(g)) <= 1e-5 * norm
    tr.max_grad_norm = 0.5 * norm
    avg = WeightAverage(tr, decay=decay, every=1)
    p0 = _host(tr.params)
    tr.step(S, P, Z, lr=lr)
    coef = clip_coefficient(np.float32(norm), np.float32(0.5 * norm))
    mask = default_decay_mask(tr.params)
    want = [adam_reference(p, gi, np.zeros_like(p), np.zeros_like(p), 1, lr=lr, weight_decay=wd if d else 0.0, decoupled=True,
                           coef=coef)[0] for p, gi, d in zip(p0, g, mask)]
    eff = [coef * gi for gi in g]
    OC.assert_adam_bar(_host(tr.params), want, eff, lr, (kind, "params"))
    shadows = _host(avg.shadows)[:len(want)]
    OC.assert_adam_bar(shadows, [weight_average_reference(a, b, decay) for a, b in zip(p0, want)], eff, lr, (kind, "average"))
    assert any(not np.array_equal(a, b) for a, b in zip(shadows, _host(tr.params)))


# ---------------------------------------------------------------------------------------------- 5. end to end
LOOP_N, LOOP_ROWS, LOOP_BATCH = 5, 40, 8


def _loop_run(tn, path):
    """train_network() under the seed of the epochs' shuffles: (latest.pth's bytes, what it printed)."""
    import contextlib
    import io
    torch.manual_seed(21)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        tn.train_network()
    with open(path + "latest.pth", "rb") as f:
        return f.read(), out.getvalue()


def _loop_child(tmp):
    """The body of test_loop_under_cross_entropy, in a process of its own: the board size is read when the package is imported."""
    from alphaquoridorgnn_amd import _lib, constants, train_network as tn
    from alphaquoridorgnn_amd.pv_network_gnn import GraphPolicyValueNetwork, load_network
    from alphaquoridorgnn_amd.replay import ReplayWindow
    from tests.test_cnn import _states
    assert constants.BOARD_SIZE == LOOP_N
    dev = _lib.require_gpu()
    N, rows, A = LOOP_N, LOOP_ROWS, E.policy_size(LOOP_N)
    path = str(tmp) + "/"
    os.chdir(path)
    tn.PV_NETWORK_PATH, tn.NUM_EPOCH, tn.BATCH_SIZE = path, 2, LOOP_BATCH
    torch.manual_seed(3)
    torch.save(GraphPolicyValueNetwork(6, 16, 2, A, board_size=N).state_dict(), path + "best.pth")
    rng = np.random.RandomState(N)
    pi = rng.rand(rows, A) * (rng.rand(rows, A) < 0.3)
    pi[:, 0] += 1e-3
    pi = (pi / pi.sum(1, keepdims=True)).astype(np.float32)
    z = rng.choice([-1.0, 0.0, 1.0], rows).astype(np.float32)
    window = ReplayWindow(N, max_generations=1, device=dev)
    window.append_rows(*(torch.from_numpy(x).to(dev) for x in (_states(N, rows), pi, z)))
    tn.TRAIN_WINDOW = window
    off, out = _loop_run(tn, path)
    assert "(CE)" not in out and "| Policy Loss: " in out
    tn.TRAIN_POLICY_LOSS, tn.TRAIN_VALUE_LOSS_WEIGHT = "cross_entropy", W
    on, out = _loop_run(tn, path)
    assert on != off
    assert "| Policy Loss (CE): " in out
    # the trainer driven by hand with the keyword, under the same seed
    torch.manual_seed(21)
    model = load_network(path + "best.pth", dev)
    tr = tn.GeneralTrainer(model, max_batch=LOOP_BATCH, policy_loss="cross_entropy", value_loss_weight=W)
    S, P, Z = window.tensors()
    index = window.index()
    for epoch in range(2):
        order = index[torch.randperm(rows, device=dev)]
        tr.run_epoch(S, P, Z, order, lr=tn.LEARNING_RATE * tn.lr_lambda(epoch))
    os.makedirs(path + "twin")
    torch.save(model.state_dict(), path + "twin/latest.pth")
    with open(path + "twin/latest.pth", "rb") as f:
        assert on == f.read()
    # with a hold-out
    tn.TRAIN_HOLDOUT_SHARE, tn.TRAIN_HOLDOUT_KEEP_BEST, tn.TRAIN_HOLDOUT_LOG = 0.3, True, path + "val.jsonl"
    _, out = _loop_run(tn, path)
    with open(path + "val.jsonl") as f:
        record = json.loads(f.readlines()[-1])
    assert record["options"]["policy_loss"] == "cross_entropy" and record["options"]["value_loss_weight"] == W
    shown = re.findall(r"Val Loss: ([0-9.]+) / ([0-9.]+)", out)
    assert len(shown) == len(record["curve"]) == 2, (shown, record["curve"])
    for (ce, mse), point in zip(shown, record["curve"]):
        assert ce == f"{point['policy_ce']:.4f}" and mse == f"{point['value_mse']:.4f}", (ce, mse, point)
        assert point["score"] == point["policy_ce"] + W * point["value_mse"], point
        assert abs(point["policy_ce"] - point["policy_loss"]) > 1e-3               # the column is not the reference form's number
    best = min(record["curve"], key=lambda c: c["score"])
    assert f"kept epoch {best['epoch']}/2: held-out policy CE + 0.25 x value MSE = {best['score']:.4f}" in out, out
    print("loop ok")


def test_loop_under_cross_entropy(dev, tmp_path):
    """train_network() on a 40-row 5x5 window (a 6/16/2 best.pth), two epochs at batch 8, in one child process started on the 5x5
    board: TRAIN_POLICY_LOSS = 'cross_entropy' writes another latest.pth than the option off, and byte for byte the file of a trainer
    built with the keyword and driven by hand under the same seed; the progress line names the loss.  With a hold-out, the Val Loss
    column is the table's ce and the keep-best score ce + w mse."""
    import subprocess
    code = f"import sys; sys.path.insert(0, {REPO!r}); import tests.test_policy_loss as T; T._loop_child({str(tmp_path)!r})"
    run = subprocess.run([sys.executable, "-c", code], cwd=REPO, env=dict(os.environ, AQG_BOARD_SIZE=str(LOOP_N)),
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.strip().endswith("loop ok"), run.stdout[-2000:] + run.stderr[-4000:]


# ---------------------------------------------------------------------------------------------- 6. refusals
@pytest.mark.parametrize("kind", KINDS)
def test_refusals(dev, kind):
    """A form other than the two and a negative or non-finite weight reach Python as ValueError before any launch (parameters,
    moments and gradients keep their bits), from the constructor and from the attributes read at every call; the library itself
    refuses the same structs with -1."""
    from alphaquoridorgnn_amd import _lib
    from tests.test_optim_controls import _batch, _make
    tr, N = _make(kind, dev)
    S, P, Z = _batch(N, dev, 0)
    tr.step(S, P, Z)
    torch.cuda.synchronize()
    kept = _state(tr) + [tr.flat_grads.clone()]
    for attrs in (dict(policy_loss=2), dict(policy_loss="kl"), dict(value_loss_weight=-1.0), dict(value_loss_weight=float("nan")),
                  dict(value_loss_weight=float("inf"))):
        with pytest.raises(ValueError, match="policy_form must be 0|value_weight must be finite"):
            _make(kind, dev, **attrs)
        old = {k: getattr(tr, k) for k in attrs}
        for k, v in attrs.items():
            setattr(tr, k, v)
        try:
            for update in (True, False):
                with pytest.raises(ValueError, match="policy_form must be 0|value_weight must be finite"):
                    tr.step(S, P, Z, update=update)
            with pytest.raises(ValueError):
                tr.run_epoch(S, P, Z, torch.arange(8, device=dev), batch=8)
        finally:
            for k, v in old.items():
                setattr(tr, k, v)
    # the library's own refusals, in its words
    tr.t.batch, tr.t.step = 8, 2
    for form, w, words in ((2, 1.0, "policy_form must be 0"), (1, -1.0, "value_weight must be finite"),
                           (0, float("nan"), "value_weight must be finite")):
        bad = _lib.LossStruct(form, w)
        rc = getattr(tr.lib, tr._STEP + "_loss")(ctypes.byref(tr.t), _lib.ptr(S), _lib.ptr(P), _lib.ptr(Z), 1, None, None,
                                                 ctypes.byref(bad), _lib.stream_ptr(dev))
        assert rc == -1 and words in tr.lib.aqg_last_error().decode()
    torch.cuda.synchronize()
    assert _same(kept, _state(tr) + [tr.flat_grads])
