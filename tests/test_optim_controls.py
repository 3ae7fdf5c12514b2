"""Weight decay and global-norm gradient clipping inside the HIP training steps (include/aqgnn.h "optimiser controls",
csrc/train_adam.hpp, csrc/grad_norm.hip): the norm kernels alone, and for each trainer the norm, the clip, both decays, the
identities against the trainer with the options off, the epoch call and the refusals.  The torch side lives in
tests/_optim_controls.py, shared with test_optim_controls_cpu.py."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import _optim_controls as OC   # noqa: E402
from tests.test_cnn import _make_net as _make_cnn, _states   # noqa: E402
from tests.test_gnn_graph_autograd import _sync_count   # noqa: E402

pytestmark = pytest.mark.gpu

C = 8192                                   # stage 1's chunk (csrc/grad_norm.hip GN_CHUNK)
KINDS = ["general-5x5", "gnn-5x5", "gnn-9x9", "cnn-5x5"]
B = 8


@pytest.fixture(scope="module")
def dev():
    from alphaquoridorgnn_amd import _lib
    _lib.load()
    return _lib.require_gpu()


def _A(N):
    return N * N + 2 * (N - 1) ** 2


GCN_BIAS, HEAD_BIAS = 0.3, 0.3


def _make(kind, dev, **controls):
    """(trainer, N) on a freshly seeded network of `kind`: two calls give bit-identical parameters."""
    from alphaquoridorgnn_amd.pv_network_gnn import GraphPolicyValueNetwork
    from alphaquoridorgnn_amd.train_network import CNNTrainer, GeneralTrainer, GNNTrainer
    N = int(kind[-1])
    torch.manual_seed(11)
    if kind.startswith("cnn"):
        return CNNTrainer(_make_cnn(8, 1, N, seed=11).to(dev), max_batch=B, **controls), N
    fused = kind.startswith("gnn")
    net = GraphPolicyValueNetwork(6, 128 if fused else 32, 3 if fused else 2, _A(N), board_size=N)
    # Every ReLU unit alive on a batch of 8: a unit that is dead on all of them has a zero gradient row, which no clip level can
    # make visible (assert_visible asks for half of EVERY weight matrix).  It also gives the GCN biases non-zero values to decay.
    with torch.no_grad():
        for layer in net.gcn_layers:
            layer.bias.add_(GCN_BIAS)
        net.policy_head[0].bias.add_(HEAD_BIAS)
        net.value_head[0].bias.add_(HEAD_BIAS)
    return (GNNTrainer if fused else GeneralTrainer)(net.to(dev), max_batch=B, **controls), N


_DATA = {}


def _data(N, dev):
    """Three batches of B positions with random probability and value targets, made once per board size."""
    if N not in _DATA:
        rng = np.random.RandomState(N)
        A = _A(N)
        pi = rng.rand(3 * B, A) * (rng.rand(3 * B, A) < 0.2)
        pi[:, 0] += 1e-3
        pi = (pi / pi.sum(1, keepdims=True)).astype(np.float32)
        z = rng.choice([-1.0, 0.0, 1.0], 3 * B).astype(np.float32)
        _DATA[N] = tuple(torch.from_numpy(x).to(dev) for x in (_states(N, 3 * B), pi, z))
    return _DATA[N]


def _batch(N, dev, i):
    return tuple(x[B * i:B * (i + 1)] for x in _data(N, dev))


def _host(tensors):
    return [x.detach().cpu().numpy().copy() for x in tensors]


def _state(tr):
    return [x.detach().clone() for x in tr.params + tr.adam_m + tr.adam_v]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------- the norm kernels alone
def _exact_case(dev, rng, n, off):
    from alphaquoridorgnn_amd.train_network import grad_norm
    vals = rng.randint(-2, 3, n).astype(np.float32)
    buf = np.full(off + n + 5, np.nan, np.float32)                      # everything outside [off, off + n) is NaN
    buf[off:off + n] = vals
    d = torch.from_numpy(buf).to(dev)
    got = float(grad_norm(d[off:off + n]))
    want = np.float32(np.sqrt(float((vals.astype(np.float64) ** 2).sum())))     # the sum of squares is an exact integer < 2^24
    assert np.isfinite(got), (n, off)
    assert abs(np.float64(got) - np.float64(want)) <= np.spacing(want), (n, off, got, want)


def test_norm_exact_small_sizes_and_offsets(dev):
    """Values in {-2 .. 2}: every partial sum is an integer below 2^24, so any summation order is exact and the result is
    float32(sqrt(sum)) to the last bit or its neighbour (the device's sqrt against numpy's).  Every size around the 16-byte word, the
    wave, the workgroup and the chunk, at every offset of the base inside 16 bytes, in a buffer that is NaN everywhere else: one
    element read outside the range makes the result NaN."""
    rng = np.random.RandomState(0)
    for n in (1, 3, 4, 5, 255, 256, 257, C - 1, C, C + 1, 2 * C + 1):
        for off in range(4):
            _exact_case(dev, rng, n, off)


def test_norm_exact_second_combining_level(dev):
    """More than 256 partials: a slot of the combine adds two of them (n <= 4 x 2,105,345 keeps the integer sum below 2^24)."""
    rng = np.random.RandomState(1)
    for off in range(4):
        _exact_case(dev, rng, 257 * C + 1, off)


def test_norm_random_and_deterministic(dev):
    """100,003 normal values against the float64 norm at rtol 1e-5: at most 90 additions lie between a term and the total, so the
    sum of squares is within 91 u / (1 - 91 u) < 5.5e-6 of exact and the norm within half of that plus the sqrt's rounding."""
    from alphaquoridorgnn_amd.train_network import grad_norm
    x = np.random.RandomState(2).randn(100003).astype(np.float32)
    d = torch.from_numpy(x).to(dev)
    a, b = grad_norm(d), grad_norm(d)
    assert a.dim() == 0 and a.device == d.device and a.dtype == torch.float32
    want = np.linalg.norm(x.astype(np.float64))
    assert abs(float(a) - want) <= 1e-5 * want, (float(a), want)
    assert torch.equal(a, b)
    with pytest.raises(ValueError):
        grad_norm(d[::2])
    with pytest.raises(ValueError):
        grad_norm(d.double())


# ---------------------------------------------------------------------------------------------- per trainer
@pytest.mark.parametrize("kind", KINDS)
def test_norm_clip_and_moments_after_one_step(dev, kind):
    from alphaquoridorgnn_amd.train_network import clip_coefficient
    tr, N = _make(kind, dev, max_grad_norm=1.0)
    plain, _ = _make(kind, dev)
    S, P, Z = _batch(N, dev, 0)
    tr.step(S, P, Z, update=False)                                     # mode 0: the norm is reported, nothing is scaled
    plain.step(S, P, Z, update=False)
    assert torch.equal(tr.flat_grads, plain.flat_grads)
    norm = tr.last_grad_norm
    assert norm.dim() == 0 and norm.device == tr.dev and norm.dtype == torch.float32
    g = _host(tr.grads)
    want = OC.global_norm64(g)
    assert abs(float(norm) - want) <= 1e-5 * want, (float(norm), want)
    before = tr.flat_grads.clone()
    tr.max_grad_norm = 0.5 * float(norm)
    tr.step(S, P, Z)
    assert torch.equal(tr.last_grad_norm, norm)                        # the same gradient, the same bits
    coef = float(clip_coefficient(np.float32(float(norm)), np.float32(0.5 * float(norm))))
    if kind.startswith("gnn"):                                         # the fused step leaves the clipped gradient, as torch does
        assert torch.equal(tr.flat_grads, before * torch.tensor(coef, dtype=torch.float32, device=dev))
    else:                                                              # the other two leave the gradients as computed
        assert torch.equal(tr.flat_grads, before)
    assert 0.49 < coef < 0.5
    b1, b2 = float(np.float32(0.9)), float(np.float32(0.999))
    # atol: (coef g)^2 below 1e-30 nears float32's subnormals (1.2e-38 / (1 - beta2)), where no relative bound holds
    for gi, m, v in zip(g, _host(tr.adam_m), _host(tr.adam_v)):
        cg = coef * gi.astype(np.float64)
        np.testing.assert_allclose(m, (1 - b1) * cg, rtol=2e-5, atol=1e-30)
        np.testing.assert_allclose(v, (1 - b2) * cg * cg, rtol=4e-5, atol=1e-30)


@pytest.mark.parametrize("config", ["clip", "coupled+clip", "decoupled+clip"])
@pytest.mark.parametrize("kind", KINDS)
def test_three_steps_against_torch(dev, kind, config):
    """Three steps on three batches, step i clipped at CLIP_FACTORS[i] x its own unclipped norm, against CPU torch
    (clip_grad_norm_, then Adam(weight_decay=) or AdamW with the decay on the default mask) fed the trainer's raw gradients, at the
    project's Adam bar.  The bar's conditioning clause, |g| >= 1e-3 max|g|, is about the gradient Adam consumes: with coupled decay
    that is coef g + wd p.  assert_visible keeps the comparison from passing with the options ignored, and explains the rates
    (OC.LRS: a small first step, then 2e-2 twice), the same for every network and configuration.  Share of the worst weight matrix
    that the options move by more than 1e-3, torch side, on an MI355X's gradients: clip alone 68 % on the fused network (5x5 and
    9x9; about a quarter of its weight gradients are exactly zero), 80 % general, 90 % CNN; with a decay 86 to 99 %."""
    from alphaquoridorgnn_amd.train_network import default_decay_mask
    wd = 0.0 if config == "clip" else OC.DECAY
    decoupled = config != "coupled+clip"
    tr, N = _make(kind, dev, weight_decay=wd, decoupled=decoupled, max_grad_norm=1.0)
    mask = default_decay_mask(tr.params)
    params0 = _host(tr.params)
    grads, eff, max_norms, got = [], [], [], []
    for i, factor in enumerate(OC.CLIP_FACTORS):
        S, P, Z = _batch(N, dev, i)
        tr.step(S, P, Z, update=False)
        norm = float(tr.last_grad_norm)
        grads.append(_host(tr.grads))                                  # raw: the fused step's update leaves them clipped
        tr.max_grad_norm = factor * norm
        before = _host(tr.params)
        tr.step(S, P, Z, lr=OC.LRS[i])
        assert float(tr.last_grad_norm) == norm
        max_norms.append(factor * norm)
        eff.append([factor * g + (wd * p if (d and not decoupled) else 0.0) for g, p, d in zip(grads[-1], before, mask)])
        got.append(_host(tr.params))
    ref = OC.shadow_run(params0, grads, list(OC.LRS), wd, decoupled, mask, max_norms)
    for i in range(3):
        OC.assert_adam_bar(got[i], ref[i], eff[i], OC.LRS[i], (kind, config, i))
    OC.assert_visible(ref[-1], OC.shadow_run(params0, grads, list(OC.LRS))[-1], params0, (kind, config))


@pytest.mark.parametrize("kind", KINDS)
def test_identities_against_options_off(dev, kind):
    off, N = _make(kind, dev)
    huge, _ = _make(kind, dev, max_grad_norm=1e30, weight_decay=0.0)                 # the clipped path with coef exactly 1
    coupled, _ = _make(kind, dev, weight_decay=OC.DECAY, decoupled=False)              # biases / BatchNorm must not decay
    both, _ = _make(kind, dev, weight_decay=OC.DECAY, decoupled=False, decay_all=True)
    dec, _ = _make(kind, dev, weight_decay=OC.DECAY, decoupled=True)
    for i in range(2):
        S, P, Z = _batch(N, dev, i)
        for t in (off, huge):
            t.step(S, P, Z)
        if i == 0:
            for t in (coupled, both, dec):
                t.step(S, P, Z)
    assert _same(_state(off), _state(huge))
    assert huge.last_grad_norm.dim() == 0 and float(huge.last_grad_norm) > 0
    # one step from the same parameters on the same batch: the gradients agree, so an undecayed tensor takes the plain step's bits
    first, _ = _make(kind, dev)
    first.step(*_batch(N, dev, 0))
    assert torch.equal(first.flat_grads, coupled.flat_grads) and torch.equal(first.flat_grads, both.flat_grads)
    for j, (p, a, c) in enumerate(zip(first.params, coupled.params, dec.params)):
        if p.dim() >= 2:                                                       # a weight decays, either way: decoupled in the
            assert not torch.equal(p, c), j                                    # parameter itself; coupled in the gradient Adam
            assert not torch.equal(first.adam_m[j], coupled.adam_m[j]), j      # takes (a first step moves by lr sign(g) alone)
        else:
            assert torch.equal(p, a) and torch.equal(p, c), j                  # a bias / BatchNorm tensor does not ...
            assert torch.equal(first.adam_m[j], coupled.adam_m[j]) and torch.equal(first.adam_v[j], coupled.adam_v[j]), j
            if bool((p != 0).any()) and bool((first.adam_m[j] != 0).any()):
                assert not torch.equal(first.adam_m[j], both.adam_m[j]), j     # ... unless decay_all says so


@pytest.mark.parametrize("kind", KINDS)
def test_run_epoch_with_options(dev, kind):
    """run_epoch with decay and clipping on takes bit-identically the steps step() takes (the short last batch included), in both
    order forms; grad_norms holds each step's last_grad_norm bit for bit; two runs agree; no call reads the device."""
    probe, N = _make(kind, dev, max_grad_norm=1.0)
    S, P, Z = _data(N, dev)
    n, lr = 20, 7e-4
    S, P, Z = S[:n], P[:n], Z[:n]
    probe.step(S[:B], P[:B], Z[:B], update=False)
    controls = dict(weight_decay=0.1, decoupled=True, max_grad_norm=0.3 * float(probe.last_grad_norm))
    order = torch.from_numpy(np.random.RandomState(3).permutation(n)).to(dev)
    finals = []
    for pre_shuffle in (True, False, True):
        ta, tb = _make(kind, dev, **controls)[0], _make(kind, dev, **controls)[0]
        sums = ta.run_epoch(S, P, Z, order, lr=lr, batch=B, pre_shuffle=pre_shuffle)
        norms, ref = [], torch.zeros(2, device=dev)
        for i in range(0, n, B):
            idx = order[i:i + B]
            pl, vl = tb.step(S[idx], P[idx], Z[idx], lr=lr)
            ref += torch.stack([pl, vl])
            norms.append(tb.last_grad_norm.clone())
        assert _same(_state(ta), _state(tb)), pre_shuffle
        assert ta.grad_norms.shape == (3,) and torch.equal(ta.grad_norms, torch.stack(norms)), pre_shuffle
        assert torch.equal(ta.last_grad_norm, norms[-1])
        assert bool((ta.grad_norms > controls["max_grad_norm"]).any())          # at least one step was clipped
        np.testing.assert_allclose(sums.cpu().numpy(), ref.cpu().numpy(), rtol=1e-5)
        finals.append((_state(ta), ta.grad_norms.clone()))
    assert _same(finals[0][0], finals[2][0]) and torch.equal(finals[0][1], finals[2][1])
    assert _same(finals[0][0], finals[1][0]) and torch.equal(finals[0][1], finals[1][1])
    ta = _make(kind, dev, **controls)[0]
    ta.step(S[:B], P[:B], Z[:B])                                                 # buffers allocated
    torch.cuda.synchronize()
    assert _sync_count(lambda: ta.step(S[:B], P[:B], Z[:B])) == 0
    assert _sync_count(lambda: ta.run_epoch(S, P, Z, order, lr=lr, batch=B)) == 0


@pytest.mark.parametrize("kind", KINDS)
def test_refusals(dev, kind):
    """Every refusal of the section, through the trainer on real device memory: each is raised before any launch, so parameters,
    moments and gradients keep their bits."""
    from alphaquoridorgnn_amd._lib import HipLibraryError
    tr, N = _make(kind, dev)
    S, P, Z = _batch(N, dev, 0)
    tr.step(S, P, Z)
    torch.cuda.synchronize()
    kept = _state(tr) + [tr.flat_grads.clone()]

    def refused(match, update=True, **attrs):
        old = {k: getattr(tr, k) for k in attrs}
        for k, v in attrs.items():
            setattr(tr, k, v)
        try:
            with pytest.raises(HipLibraryError, match=match):
                tr.step(S, P, Z, update=update)
        finally:
            for k, v in old.items():
                setattr(tr, k, v)
        torch.cuda.synchronize()
        assert _same(_state(tr) + [tr.flat_grads], kept), attrs

    for update in (True, False):
        refused("weight decay", update, weight_decay=-1e-4)
        refused("weight decay", update, weight_decay=float("inf"))
        refused("weight decay", update, weight_decay=float("nan"))
        refused("max_grad_norm", update, max_grad_norm=-1.0)
        refused("max_grad_norm", update, max_grad_norm=float("inf"))
        refused("max_grad_norm", update, max_grad_norm=float("nan"))
        refused("workspace too small", update, max_grad_norm=1.0, _optim_ws=torch.empty((0,), dtype=torch.float32, device=dev))
    other = torch.zeros_like(tr.grads[3])
    was = tr.t.grads[3]
    tr.t.grads[3] = other.data_ptr()                                   # a gradient tensor outside the flat buffer
    try:
        refused("consecutive", max_grad_norm=1.0)
        tr.max_grad_norm = 1.0
        with pytest.raises(HipLibraryError, match="consecutive"):
            tr.run_epoch(S, P, Z, torch.arange(B, device=dev), batch=B)
    finally:
        tr.t.grads[3], tr.max_grad_norm = was, None
    # the epoch call refuses the same
    tr.weight_decay = -1.0
    with pytest.raises(HipLibraryError, match="weight decay"):
        tr.run_epoch(S, P, Z, torch.arange(B, device=dev), batch=B)
    tr.weight_decay = 0.0
    torch.cuda.synchronize()
    assert _same(_state(tr) + [tr.flat_grads], kept)
    # and the stand-alone norm: a workspace one float short
    lib, x, out = tr.lib, torch.ones(C + 1, device=dev), torch.zeros(1, device=dev)
    ws = torch.zeros(1, device=dev)
    assert lib.aqg_optim_workspace_floats(C + 1) == 2
    assert lib.aqg_grad_norm(ctypes.c_void_p(x.data_ptr()), C + 1, ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(ws.data_ptr()), 1,
                             None) < 0
    assert "workspace too small" in lib.aqg_last_error().decode()
