"""Weight averaging (include/aqgnn.h "weight averaging"), the part that needs no GPU: the numpy statement against torch's EMA function
and against the float64 closed form, the `every` rule, the Python-side refusals, train_cycle's options, and the host backend of
WeightAverage.for_module on a CPU network."""
import os
import sys
import types

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

DECAYS = (0.0, 0.5, 0.9, 0.999, 0.9999, 1.0 - 2.0 ** -24)


def _net(seed=0):
    from alphaquoridorgnn_amd.pv_network_gnn import GraphPolicyValueNetwork
    torch.manual_seed(seed)
    return GraphPolicyValueNetwork(6, 16, 2, 17, board_size=3)


@pytest.mark.parametrize("decay", DECAYS)
def test_reference_is_torchs_ema_function_bit_for_bit(decay):
    """weight_average_reference against torch.optim.swa_utils.get_ema_avg_fn(float(d)), what AveragedModel applies, on 100,000 random
    floats of mixed scale, three updates in a row."""
    from torch.optim.swa_utils import get_ema_avg_fn
    from alphaquoridorgnn_amd.train_network import weight_average_reference
    d = np.float32(decay)
    assert 0 <= d < 1
    fn = get_ema_avg_fn(float(d))
    rng = np.random.RandomState(3)
    e = (rng.randn(100000) * 10.0 ** rng.randint(-6, 3, 100000)).astype(np.float32)
    te = torch.from_numpy(e.copy())
    for k in range(3):
        p = (rng.randn(100000) * 10.0 ** rng.randint(-6, 3, 100000)).astype(np.float32)
        e = weight_average_reference(e, p, decay)
        te = fn(te, torch.from_numpy(p), k)
        assert e.dtype == np.float32
        assert np.array_equal(e.view(np.uint32), te.numpy().view(np.uint32)), (decay, k)


@pytest.mark.parametrize("decay", DECAYS)
@pytest.mark.parametrize("n", (1, 7, 200))
def test_reference_against_the_closed_form(decay, n):
    """e_n = d^n e_0 + w sum_k d^(n-1-k) p_k in float64, with the float32 values of d and w as doubles.  The bar is derived: an update
    rounds three times, each by at most 2^-24 M (M = the largest magnitude involved), and carries the inherited error on with weight
    d: 3 * 2^-24 * M * (1 + d + d^2 + ...) <= 3 * 2^-24 * M * min(n, 1 / (1 - d))."""
    from alphaquoridorgnn_amd.train_network import weight_average_reference
    d32 = np.float32(decay)
    w32 = np.float32(1.0 - float(d32))
    d, w = float(d32), float(w32)
    rng = np.random.RandomState(n)
    e0 = rng.randn(4096).astype(np.float32)
    ps = [rng.randn(4096).astype(np.float32) for _ in range(n)]
    e = e0
    for p in ps:
        e = weight_average_reference(e, p, decay)
    exact = d ** n * e0.astype(np.float64)
    for k, p in enumerate(ps):
        exact += w * d ** (n - 1 - k) * p.astype(np.float64)
    M = max(np.abs(e0).max(), max(np.abs(p).max() for p in ps))
    bar = 3 * 2.0 ** -24 * float(M) * min(n, 1.0 / (1.0 - d))
    assert np.abs(e.astype(np.float64) - exact).max() <= bar, (decay, n, np.abs(e - exact).max(), bar)


def test_decay_zero_gives_the_source_back():
    from alphaquoridorgnn_amd.train_network import weight_average_reference
    rng = np.random.RandomState(5)
    e, p = rng.randn(1000).astype(np.float32), rng.randn(1000).astype(np.float32)
    p[:4] = (0.0, 1e-45, -1e-45, 3e38)
    assert np.array_equal(weight_average_reference(e, p, 0.0), p)


@pytest.mark.parametrize("every", (1, 2, 3, 5))
def test_every_rule_on_step_numbers(every):
    """Updates fall on the multiples of K among the step numbers 1 .. 13, and the count a WeightAverage keeps over library calls of
    any length is the number of those multiples, wherever the calls end."""
    from alphaquoridorgnn_amd.train_network import WeightAverage, weight_average_due
    due = [s for s in range(1, 14) if weight_average_due(s, every)]
    assert due == list(range(every, 14, every))
    for call in (1, 3, 4, 13):
        avg = WeightAverage.for_module(_net(), 0.9, every)
        for first in range(1, 14, call):
            avg._stepped(first, min(call, 14 - first), every)
        assert avg.updates == len(due), (every, call)


def _fake_trainer(model, params=None):
    return types.SimpleNamespace(model=model, params=list(model.parameters()) if params is None else params, buffers=[], average=None)


@pytest.mark.parametrize("decay", (-0.1, 1.0, 1.5, float("nan"), 1.0 - 2.0 ** -26, float("inf"), "much", None))
def test_bad_decay_is_refused(decay):
    from alphaquoridorgnn_amd.train_network import WeightAverage
    with pytest.raises(ValueError):
        WeightAverage.for_module(_net(), decay)
    with pytest.raises(ValueError):
        WeightAverage(_fake_trainer(_net()), decay=decay)
    avg = WeightAverage.for_module(_net(), 0.5)
    before = [x.clone() for x in avg.tensors()]
    avg.decay = decay                                   # read at every call: refused at the call, the average untouched
    with pytest.raises(ValueError):
        avg.update()
    assert avg.updates == 0 and all(torch.equal(a, b) for a, b in zip(before, avg.tensors()))


@pytest.mark.parametrize("every", (0, -1, 2.5, True, None, "2"))
def test_bad_every_is_refused(every):
    from alphaquoridorgnn_amd.train_network import WeightAverage
    with pytest.raises(ValueError):
        WeightAverage.for_module(_net(), 0.9, every)
    avg = WeightAverage.for_module(_net(), 0.9)
    avg.every = every
    with pytest.raises(ValueError):
        avg.update()


def test_other_python_side_refusals():
    from alphaquoridorgnn_amd import _lib
    from alphaquoridorgnn_amd.train_network import WeightAverage
    net = _net()
    tr = _fake_trainer(net)
    first = WeightAverage(tr, decay=0.9)
    assert tr.average is first
    with pytest.raises(ValueError, match="already"):
        WeightAverage(tr, decay=0.9)
    with pytest.raises(ValueError, match="no float32"):
        WeightAverage.for_module(torch.nn.Linear(3, 2).double())
    with pytest.raises(ValueError, match="contiguous"):                          # a strided view
        WeightAverage(_fake_trainer(net, [net.policy_head[0].weight.detach().t()]))
    with pytest.raises(ValueError, match="contiguous"):                          # not float32
        WeightAverage(_fake_trainer(net, [torch.zeros(3, dtype=torch.float64)]))
    with pytest.raises(ValueError, match="contiguous"):                          # fewer than 1 element
        WeightAverage(_fake_trainer(net, [torch.zeros(0)]))
    with pytest.raises(ValueError, match="state_dict"):                          # a tensor that is not the model's
        WeightAverage(_fake_trainer(net, [torch.zeros(3)]))
    with pytest.raises(ValueError, match="state_dict"):                          # one tensor twice
        WeightAverage(_fake_trainer(net, [net.policy_head[0].bias.detach()] * 2))
    with pytest.raises(ValueError, match="tensors"):
        WeightAverage(_fake_trainer(net, []))
    with pytest.raises(ValueError, match="tensors"):
        WeightAverage(_fake_trainer(net, [torch.zeros(1)] * (_lib.WEIGHT_AVERAGE_MAX_TENSORS + 1)))
    from alphaquoridorgnn_amd.pv_network_gnn import GraphPolicyValueNetwork
    with pytest.raises(ValueError, match="copy_to"):
        first.copy_to(GraphPolicyValueNetwork(6, 32, 2, 17, board_size=3))      # another width
    with pytest.raises(ValueError, match="copy_to"):
        first.copy_to(torch.nn.Linear(3, 2))


def test_train_cycle_options(monkeypatch):
    from alphaquoridorgnn_amd import train_cycle as tc, train_network as tn
    for k in ("TRAIN_EMA_DECAY", "TRAIN_EMA_EVERY"):
        monkeypatch.setattr(tn, k, getattr(tn, k))
    assert (tn.TRAIN_EMA_DECAY, tn.TRAIN_EMA_EVERY) == (None, 1)
    tc._set_average_options(tc._parser().parse_args([]))
    assert (tn.TRAIN_EMA_DECAY, tn.TRAIN_EMA_EVERY) == (None, 1)
    for bad in (["--ema-every", "2"], ["--ema-decay", "1"], ["--ema-decay", "-0.1"], ["--ema-decay", "nan"],
                ["--ema-decay", "0.99999999"], ["--ema-decay", "0.9", "--ema-every", "0"], ["--ema-decay", "0.9", "--ema-every", "-3"]):
        with pytest.raises(ValueError):
            tc._check_average_args(tc._parser().parse_args(bad))
        with pytest.raises(ValueError):                  # refused by main() in front of anything that touches a device
            tc.main(bad)
        assert (tn.TRAIN_EMA_DECAY, tn.TRAIN_EMA_EVERY) == (None, 1)
    tc._set_average_options(tc._parser().parse_args(["--ema-decay", "0.99", "--ema-every", "4"]))
    assert (tn.TRAIN_EMA_DECAY, tn.TRAIN_EMA_EVERY) == (0.99, 4)
    tc._set_average_options(tc._parser().parse_args(["--ema-decay", "0"]))
    assert tn.TRAIN_EMA_DECAY == 0.0


def test_for_module_on_a_cpu_network():
    """The host backend: state_dict() has the module's keys, order and dtypes; three updates equal the numpy statement and torch's
    AveragedModel under get_ema_avg_fn; copy_to writes the average into a module of the same shape and advances version counters."""
    from torch.optim.swa_utils import AveragedModel, get_ema_avg_fn
    from alphaquoridorgnn_amd.train_network import WeightAverage, weight_average_reference
    d = 0.9
    net = _net(1)
    avg = WeightAverage.for_module(net, d)
    assert avg.host and avg.updates == 0
    torchs = AveragedModel(net, avg_fn=get_ema_avg_fn(float(np.float32(d))))
    torchs.update_parameters(net)                        # its first call copies: our average starts as that copy
    want = [p.detach().numpy().copy() for p in net.parameters()]
    assert all(np.array_equal(e.numpy(), w) for e, w in zip(avg.tensors(), want))
    for k in range(3):
        with torch.no_grad():
            for p in net.parameters():
                p.add_(torch.randn_like(p) * 0.1)
        avg.update()
        torchs.update_parameters(net)
        want = [weight_average_reference(w, p.detach().numpy(), d) for w, p in zip(want, net.parameters())]
    assert avg.updates == 3
    for e, w, t in zip(avg.tensors(), want, torchs.module.parameters()):
        assert np.array_equal(e.numpy(), w) and torch.equal(e, t.detach())
    sd, ref = avg.state_dict(), net.state_dict()
    assert list(sd.keys()) == list(ref.keys())
    assert all(sd[k].dtype == ref[k].dtype and sd[k].shape == ref[k].shape for k in ref)
    assert all(np.array_equal(sd[k].numpy(), w) for k, w in zip(avg.keys, want))
    assert not any(torch.equal(sd[k], ref[k]) for k in avg.keys if ref[k].dim() >= 2)
    other = _net(2)
    versions = [p._version for p in other.parameters()]
    avg.copy_to(other)
    assert all(torch.equal(a, b) for a, b in zip(other.state_dict().values(), sd.values()))
    assert all(p._version > v for p, v in zip(other.parameters(), versions))
    other.load_state_dict(sd)                            # a state_dict consumer loads it
