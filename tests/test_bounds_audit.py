"""Bounds audit on the GPU: every workload runs three times -- plain, and with every allocation of the package's modules (and the
test's own inputs, weights and workspaces) served from the middle of a poisoned buffer by tests/_guard_bands.py, once per pattern.

    1. after each guarded run (and a device synchronise) every pad still holds its pattern: nothing was written out of bounds;
    2. the two guarded runs agree byte for byte: nothing read from a pad -- or from memory nobody wrote, which holds the pattern
       too -- reached a result;
    3. the guarded runs agree with the plain run byte for byte: every path here is documented as deterministic.

What this cannot see: an out-of-bounds READ whose value is masked before it reaches a result leaves no trace (pads intact, results
equal); a write further away than the pads (64 KiB, or two leading rows of the tensor) is not contained by them; tensors that do
not come from zeros / empty / full / ones(_like) of a wrapped module -- .to(device) copies, torch.rand, index_select results, the
functions test_bounds_audit_cpu.BLIND_SPOTS lists -- are not guarded unless the workload places them itself.
The results compared are what a caller may read: rows a call leaves unwritten by contract (an inactive row, entries past a count)
are cut away first, they hold the pattern.  The exact-size refusals at the end run on guarded buffers as well: "untouched" is
checked."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import _guard_bands as GB   # noqa: E402
from tests import _train_edges as E   # noqa: E402
from tests import _util as U   # noqa: E402
from tests import witness_cases as W   # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from alphaquoridorgnn_amd import _lib
    _lib.load()
    return _lib.require_gpu()


_MODULES = None


def wrapped_modules():
    """The package modules the audit wraps: derived by the scan of test_bounds_audit_cpu, not written down."""
    global _MODULES
    if _MODULES is None:
        from tests.test_bounds_audit_cpu import scan_package
        _MODULES = [importlib.import_module("alphaquoridorgnn_amd." + name) for name in scan_package()[0]]
    return _MODULES


class Env:
    """What a workload gets: the device, `t` -- torch, or in a guarded run its stand-in for the workload's own allocations --
    and place() for inputs it made elsewhere."""

    def __init__(self, dev, bands):
        self.dev, self.bands = dev, bands
        self.t = torch if bands is None else bands.proxy("test")

    def place(self, x):
        x = x.to(self.dev).contiguous()
        return x.clone() if self.bands is None else self.bands.place(x)

    def from_numpy(self, a):
        return self.place(torch.from_numpy(np.ascontiguousarray(a)))

    def guard_module(self, net):
        """Move every parameter and buffer of a module (already on the device) into guarded memory."""
        with torch.no_grad():
            for p in net.parameters():
                p.data = self.place(p.data)
            for m in net.modules():
                for k, b in list(m._buffers.items()):
                    if b is not None:
                        m._buffers[k] = self.place(b)
        return net

    def packed(self, net):
        """The fused network's packed weights, built and moved into guarded memory (they reach the device by a copy)."""
        net.packed_weights(self.dev)
        net._packed = self.place(net._packed)
        return net


def _bytes(results):
    out = {}
    for k, v in results.items():
        if v is None:
            continue
        if not torch.is_tensor(v):
            v = torch.as_tensor(np.asarray(v))
        out[k] = v.detach().cpu().contiguous().numpy().tobytes()
    return out


def _run(workload, dev, bands, modules):
    env = Env(dev, bands)
    if bands is None:
        res = _bytes(workload(env))
        torch.cuda.synchronize()
        return res
    with pytest.MonkeyPatch.context() as mp:
        bands.install(mp, modules)
        res = workload(env)
        torch.cuda.synchronize()
        broken = bands.intact()
        res = _bytes(res)
    assert broken == [], f"pattern {bands.pattern}: pads written: {broken}"
    assert len(bands.buffers) > 0
    return res


def audit(workload, modules=None, dev=None):
    """Run `workload` plain, under GuardBands(0) and under GuardBands(1); the three assertions of the module docstring."""
    modules = wrapped_modules() if modules is None else modules
    dev = torch.device("cuda", torch.cuda.current_device()) if dev is None else dev
    plain = _run(workload, dev, None, modules)
    guarded = [_run(workload, dev, GB.GuardBands(p), modules) for p in (0, 1)]
    assert plain.keys() == guarded[0].keys() == guarded[1].keys() and len(plain) > 0
    for k in plain:
        assert guarded[0][k] == guarded[1][k], f"{k}: the guarded runs differ -- something read outside its tensor reached it"
    for k in plain:
        assert plain[k] == guarded[0][k], f"{k}: the guarded runs differ from the plain run"
    return plain


def _A(N):
    return N * N + 2 * (N - 1) ** 2


def _small(N, B, step=None):
    from tests.test_gpu_parity import _small_board_states
    pool = U.golden("walk_9x9.npz")["states"] if N == 9 else _small_board_states(N)
    idx = (np.arange(B) * (step or max(1, pool.shape[0] // max(B, 1)))) % pool.shape[0]
    return np.ascontiguousarray(pool[idx])


def _cut(rows, count):
    """Rows [B, n] with everything past count[b] zeroed: what lies past a count is nobody's."""
    keep = torch.arange(rows.shape[1], device=rows.device).unsqueeze(0) < count.unsqueeze(1).long()
    return torch.where(keep, rows, torch.zeros_like(rows))


# ---------------------------------------------------------------------- the instrument can fail
def test_a_planted_write_is_reported(dev):
    """A real workload, then ONE byte written by torch indexing into the slack right behind one recorded tensor: intact() names it."""
    from alphaquoridorgnn_amd import game_logic as gl
    bands = GB.GuardBands(0)
    with pytest.MonkeyPatch.context() as mp:
        bands.install(mp, [gl])
        recs = bands.place(torch.from_numpy(_small(5, 7)).to(dev))
        mask, order, count = gl.legal_actions_batch(recs, 5)
        torch.cuda.synchronize()
        assert bands.intact() == []
        assert [r.module for r in bands.buffers] == ["test", "game_logic", "game_logic", "game_logic"]
        r, at = bands.rear_slack(count)                 # int32 [7]: 28 bytes, 484 bytes of slack behind them
        assert r.nbytes == 28 and at == r.start + 28
        r.buf[at] = 0x5A
        torch.cuda.synchronize()
        assert bands.intact() == [("game_logic", (7,), torch.int32, "rear")]
        r.buf[at] = 0
        assert bands.intact() == []
        r, _ = bands.rear_slack(order)
        r.buf[r.start - 1] = 0x5A
        assert bands.intact() == [("game_logic", (7, 136), torch.uint8, "front")]


# ---------------------------------------------------------------------- rules
_CROWDED = {}


def _rule_records(N, B, last="most"):
    """B records whose LAST one is the most crowded the board has here: the 63-task layout runs against the end of every array."""
    recs = _small(N, B, step=37)
    if N == 9:
        if "crowded" not in _CROWDED:
            _CROWDED["crowded"] = W.crowded(9, 32, 3)
        recs[-1] = W.most_crowded() if last == "most" else _CROWDED["crowded"]
    elif N == 5:
        recs[-1] = W.plugged_corridor(5)
    return recs


@pytest.mark.parametrize("N", [3, 5, 7, 9])
def test_rules(dev, N):
    from alphaquoridorgnn_amd import game_logic as gl
    from alphaquoridorgnn_amd.constants import board_params
    batches = [(f"{B}{last[0]}", _rule_records(N, B, last)) for B in (1, 63, 65) for last in (("most", "crowded") if N == 9 else ("most",))]

    def workload(env):
        out = {}
        for tag, h in batches:
            recs = env.from_numpy(h)
            mask, order, count = gl.legal_actions_batch(recs, N)
            first = torch.where(count > 0, order[:, 0].to(torch.int32), torch.zeros_like(count))      # a legal action of every row that has one
            nxt = gl.next_batch(recs, env.place(first), N)
            out.update({f"mask{tag}": mask, f"order{tag}": order, f"count{tag}": count, f"next{tag}": nxt[count > 0],
                        f"status{tag}": gl.status_batch(recs, N, board_params(N)[1]), f"check{tag}": gl.check_states_batch(recs, N)})
            _, o2, c2 = gl.legal_actions_batch(recs, N, want_mask=False)
            out.update({f"order_nomask{tag}": o2, f"count_nomask{tag}": c2})
        return out

    audit(workload)


# ---------------------------------------------------------------------- 9x9 trunk and heads
def _gnn9(seed=0, scale=1.0):
    from tests.test_gpu_parity import _model
    model, params = _model(seed)
    if scale != 1.0:
        big = {k: (v * (scale if "gcn" in k and "weight" in k else 1.0)).astype(np.float32) for k, v in params.items()}
        big["gcn_layers.0.bias"] = np.linspace(-0.2, 0.4, 128).astype(np.float32)
        model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in big.items()})
    return model


@pytest.mark.parametrize("variant", [3, 1, 6])
def test_trunk_and_heads_9x9(dev, variant):
    from alphaquoridorgnn_amd import _lib
    from tests.test_engine_general import _pack24
    host = {B: _small(9, B, step=29) for B in (1, 17, 513)}
    host24 = {B: _pack24(host[B], 9) for B in (1, 17, 513)}

    def workload(env):
        model = env.packed(env.guard_module(_gnn9(0)))
        assert not (model.gnn_flags(env.dev) & _lib.GNN_EXACT_F32)
        out = {}
        for B, h in host.items():
            p, v, lg, vp = model.forward_states(env.from_numpy(h), want_logits=True)
            out.update({f"policy{B}": p, f"value{B}": v, f"logits{B}": lg, f"vpre{B}": vp})
            p, v = model.forward_states(env.from_numpy(h))
            out.update({f"policy_only{B}": p, f"value_only{B}": v})
        for B, h in host24.items():
            p, v = model.forward_states(env.from_numpy(h), state_fmt=1)
            out.update({f"policy24_{B}": p, f"value24_{B}": v})
        return out

    _lib.set_option("trunk_variant", variant)
    try:
        audit(workload)
    finally:
        _lib.set_option("trunk_variant", 3)


def test_exact_f32_kernels_9x9(dev):
    """The range guard's fallback set (trunk weights x300, test_gnn_fp16_range_guard): served by the exact f32-input kernels."""
    from alphaquoridorgnn_amd import _lib
    host = {B: _small(9, B, step=31) for B in (1, 17, 513)}

    def workload(env):
        model = env.packed(env.guard_module(_gnn9(3, 300.0)))
        assert model.gnn_flags(env.dev) == _lib.GNN_EXACT_F32
        out = {}
        for B, h in host.items():
            p, v, lg, vp = model.forward_states(env.from_numpy(h), want_logits=True)
            out.update({f"policy{B}": p, f"value{B}": v, f"logits{B}": lg, f"vpre{B}": vp})
        return out

    audit(workload)


# ---------------------------------------------------------------------- small boards, any shape
def _fixed_net(N, seed=4):
    from alphaquoridorgnn_amd.pv_network_gnn import GraphPolicyValueNetwork
    from oracle import gnn as og
    params = og.init_params(seed, N=N)
    net = GraphPolicyValueNetwork(6, 128, 3, _A(N), board_size=N)
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in params.items()})
    return net.to("cuda").eval()


@pytest.mark.parametrize("N", [3, 5, 7])
def test_fixed_network_small_boards(dev, N):
    def workload(env):
        model = env.packed(env.guard_module(_fixed_net(N)))
        out = {}
        for B in (1, 65):
            p, v, lg, vp = model.forward_states(env.from_numpy(_small(N, B)), want_logits=True)     # the workspace: exactly ..._any_workspace_floats
            out.update({f"policy{B}": p, f"value{B}": v, f"logits{B}": lg, f"vpre{B}": vp})
        return out

    audit(workload)


@pytest.mark.parametrize("A", [1, 300])
@pytest.mark.parametrize("shape", [(6, 8, 1), (6, 130, 2)], ids=lambda s: "x".join(map(str, s)))
def test_any_shape_networks(dev, shape, A):
    """forward_states of a non-default shape (the featuriser and the width-generic layers) on 5x5 boards, and the fused any-shape
    forward (aqg_gcn_forward_boards_general) with its workspace at exactly the size the library states, when the head is the board's."""
    from alphaquoridorgnn_amd import _lib
    from tests.test_gnn_any_shape import _make_net
    N = 5
    lib = _lib.load()

    def workload(env):
        net = env.guard_module(_make_net(shape, A, seed=sum(shape) + A, N=N))
        out = {}
        with torch.no_grad():
            for B in (1, 65):
                p, v, lg, vp = net.forward_states(env.from_numpy(_small(N, B)), want_logits=True)
                out.update({f"policy{B}": p, f"value{B}": v, f"logits{B}": lg, f"vpre{B}": vp})
            for B in (1, 65):
                recs = env.from_numpy(_small(N, B))
                nws = int(lib.aqg_gcn_boards_general_workspace_floats(N, shape[1], A, B))
                assert nws > 0
                f32 = dict(dtype=torch.float32, device=env.dev)
                ws = env.t.empty((nws,), **f32)
                pooled, logits, policy = env.t.empty((B, shape[1]), **f32), env.t.empty((B, A), **f32), env.t.empty((B, A), **f32)
                vpre, value = env.t.empty((B,), **f32), env.t.empty((B,), **f32)
                active = env.place(torch.from_numpy((np.arange(B) % 3 != 1).astype(np.uint8)))
                d = net.general_net(env.dev)
                _lib.check(lib.aqg_gcn_forward_boards_general(N, _lib.ptr(recs), 0, B, ctypes.byref(d), _lib.ptr(active), _lib.ptr(ws), nws,
                                                              _lib.ptr(pooled), _lib.ptr(logits), _lib.ptr(policy), _lib.ptr(vpre),
                                                              _lib.ptr(value), _lib.stream_ptr(env.dev)), "aqg_gcn_forward_boards_general")
                on = active == 1
                out.update({f"f_policy{B}": policy[on], f"f_value{B}": value[on], f"f_logits{B}": logits[on], f"f_vpre{B}": vpre[on],
                            f"f_pooled{B}": pooled[on]})
        return out

    audit(workload)


# ---------------------------------------------------------------------- CNN forward
@pytest.mark.parametrize("F_,L,N", [(1, 0, 3), (65, 1, 5), (130, 1, 9)])
def test_cnn_forward(dev, F_, L, N):
    from tests.test_cnn import _make_net
    from tests.test_cnn_cpu import _triples

    def workload(env):
        net = env.guard_module(_make_net(F_, L, N, seed=F_ + L + N).to(env.dev))
        out = {}
        with torch.no_grad():
            for B in (1, 5):
                h = _small(N, B)
                recs = env.from_numpy(h)
                p, v, lg, vp, pooled = net.forward_states(recs, want_logits=True, want_pooled=True)
                out.update({f"policy{B}": p, f"value{B}": v, f"logits{B}": lg, f"vpre{B}": vp, f"pooled{B}": pooled})
                active = env.place(torch.from_numpy((np.arange(B) % 2 == 0).astype(np.uint8)))
                p, v = net.forward_states(recs, active=active)
                out.update({f"masked_policy{B}": p[active == 1], f"masked_value{B}": v[active == 1]})
                planes = env.from_numpy(net.preprocess_input(_triples(h, N)))
                p, v = net(planes)                                        # the planes entry
                out.update({f"planes_policy{B}": p, f"planes_value{B}": v})
        return out

    audit(workload)


# ---------------------------------------------------------------------- the engine
def _engine_results(eng, counters):
    out = {"counters": np.asarray([counters[k] for k in sorted(counters)], dtype=np.int64)}
    st, vis, z = eng.history_tensors()
    out.update(states=st, visits=vis, z=z)
    one = eng if hasattr(eng, "t") else None
    if (one.record_search_value if one else eng.sets[0].record_search_value):
        out["values"] = eng.history_values()
        out["lambda"] = eng.history_lambda_values(0.7)
    if (one.policy_record if one else eng.sets[0].policy_record) is not None:
        out["policies"] = eng.history_policies()
    for i, e in enumerate([one] if one else eng.sets):
        for k in ("stat_leaf_evals", "stat_terminal_sims", "stat_cache_hits", "stat_moves_kept", "stat_visits_kept", "game_plies",
                  "game_result", "game_done", "resign_min", "game_resigned", "counters"):
            if k in e.t:
                out[f"{k}.{i}"] = e.t[k]
    return out


ALL_ON = dict(root_noise_eps=0.25, temperature_plies=4, record_search_value=True, tree_reuse=True, resign_threshold=0.25,
              resign_disable_fraction=0.5, policy_target="completed_q")


def _start_table(N, quota):
    rows = np.ascontiguousarray(_small(N, 40, step=11))
    from alphaquoridorgnn_amd.game_logic import check_state_host
    rows = np.stack([r for r in rows if check_state_host(r, N) == 0 and (int(r[68]) | (int(r[69]) << 8)) % 2 == 0][:3])
    return rows, (np.arange(quota) * 2 % rows.shape[0]).astype(np.int32)


@pytest.mark.parametrize("options", ["all", "none"])
@pytest.mark.parametrize("G", [1, 5])
@pytest.mark.parametrize("N", [3, 5])
def test_engine_fake_evaluator(dev, N, G, options):
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    quota = 7
    kw = {}
    if options == "all":
        rows, index = _start_table(N, quota)
        kw = dict(ALL_ON, start_states=rows, start_index=index)

    def workload(env):
        eng = BatchedSelfPlay(None, num_games=G, sims=8, board_size=N, evaluator="fake", fake_bias=2, seed=5, quota=quota, **kw)
        c = eng.play_generation()
        assert c["finished"] == quota and c["active"] == 0
        return _engine_results(eng, c)

    audit(workload)


def _net_of(kind, N, env):
    if kind == "general":
        from tests.test_gnn_any_shape import _make_net
        return env.guard_module(_make_net((6, 16, 2), _A(N), seed=11, N=N))
    if kind == "cnn":
        from tests.test_cnn import _make_net
        return env.guard_module(_make_net(8, 1, N, seed=12).to(env.dev))
    return env.packed(env.guard_module(_gnn9(2)))


@pytest.mark.parametrize("kind,N,slots,beside", [("gnn", 9, 0, 1), ("gnn", 9, 64, 1), ("gnn", 9, 0, 0), ("general", 5, 0, 1), ("cnn", 5, 64, 1)])
def test_engine_network_evaluators(dev, kind, N, slots, beside):
    from alphaquoridorgnn_amd import _lib
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay

    def workload(env):
        net = _net_of(kind, N, env)
        eng = BatchedSelfPlay(net, num_games=5, sims=4, board_size=N, evaluator=kind, seed=3, eval_cache_slots=slots,
                              record_search_value=True)
        c = eng.play_generation()
        assert c["finished"] == 5 and c["gnn_saturated"] == 0
        return _engine_results(eng, c)

    _lib.set_option("legal_beside_trunk", beside)
    try:
        audit(workload)
    finally:
        _lib.set_option("legal_beside_trunk", 1)


def test_engine_two_sets(dev):
    from alphaquoridorgnn_amd.engine import MultiSetSelfPlay

    def workload(env):
        eng = MultiSetSelfPlay(None, num_games=5, sims=8, num_sets=2, seed=7, quota=7, board_size=5, evaluator="fake", fake_bias=2,
                               record_search_value=True, tree_reuse=True)
        c = eng.play_generation()
        eng.sync()
        assert c["finished"] == 7
        return _engine_results(eng, c)

    audit(workload)


# ---------------------------------------------------------------------- the trainers
def _trainer_results(tr, avg, losses, outs):
    out = {f"loss{i}": torch.stack(list(l)) if isinstance(l, tuple) else l for i, l in enumerate(losses)}
    out.update({f"out{i}": o for i, o in enumerate(outs)})
    out["flat_grads"] = tr.flat_grads
    for i, (p, m, v) in enumerate(zip(tr.params, tr.adam_m, tr.adam_v)):
        out.update({f"param{i}": p, f"m{i}": m, f"v{i}": v})
    for i, b in enumerate(tr.buffers):
        out[f"buffer{i}"] = b
    for i, s in enumerate(avg.shadows):
        out[f"average{i}"] = s
    out["grad_norm"], out["grad_norms"] = tr.last_grad_norm, tr.grad_norms
    return out


def _train_workload(make_net, make_trainer, N, max_batch, batches):
    from alphaquoridorgnn_amd.train_network import WeightAverage, weight_average_table
    A = _A(N)
    rows = 2 * max_batch + 1
    host = _small(N, rows, step=13)
    pi, z = E.edge_targets(rows, A, seed=N)

    def workload(env):
        net = env.guard_module(make_net())
        tr = make_trainer(net, max_batch=max_batch, weight_decay=0.01, max_grad_norm=0.5)
        avg = WeightAverage(tr, decay=0.9)
        avg.shadows = [env.place(s) for s in avg.shadows]                      # clones: moved into guarded memory, the table rebuilt
        avg._host_table, avg.table, avg.total_chunks = weight_average_table(avg.shadows, avg.sources)
        s72, p, zz = env.from_numpy(host), env.from_numpy(pi), env.from_numpy(z)
        losses, outs = [], []
        for B in batches:
            sb, pb, zb = (env.place(x[:B]) for x in (s72, p, zz))
            losses.append(tr.step(sb, pb, zb, update=False))
            outs += [x.clone() for x in tr.outputs(B)]
            losses.append(tr.step(sb, pb, zb, update=True))
            outs += [x.clone() for x in tr.outputs(B)]
        order = env.place(torch.from_numpy(np.random.RandomState(1).permutation(rows)))
        losses.append(tr.run_epoch(s72, p, zz, order, mirror=(17, 0)))
        return _trainer_results(tr, avg, losses, outs)

    return workload


@pytest.mark.parametrize("N,fused", [(9, 1), (9, 2), (9, 3), (5, None)])
def test_gnn_trainer(dev, N, fused):
    from alphaquoridorgnn_amd import _lib
    from alphaquoridorgnn_amd.train_network import GNNTrainer
    from tests.test_gpu_parity import TRAIN_FUSED_DEFAULT
    make = (lambda: _gnn9(2)) if N == 9 else (lambda: _fixed_net(5))
    if fused is not None:
        _lib.set_option("train_fused", fused)
    try:
        audit(_train_workload(make, GNNTrainer, N, 16 if N == 9 else 8, (16 if N == 9 else 8, 1)))
    finally:
        _lib.set_option("train_fused", TRAIN_FUSED_DEFAULT)


@pytest.mark.parametrize("shape,N", [((6, 8, 1), 3), ((6, 130, 2), 5)], ids=["6x8x1-3", "6x130x2-5"])
def test_general_trainer(dev, shape, N):
    from alphaquoridorgnn_amd.train_network import GeneralTrainer
    from tests.test_gnn_any_shape import _make_net
    audit(_train_workload(lambda: _make_net(shape, _A(N), seed=sum(shape), N=N), GeneralTrainer, N, 8, (8, 1)))


@pytest.mark.parametrize("F_,L,N", [(1, 0, 3), (65, 1, 5)])
def test_cnn_trainer(dev, F_, L, N):
    from alphaquoridorgnn_amd.train_network import CNNTrainer
    from tests.test_cnn import _make_net
    audit(_train_workload(lambda: _make_net(F_, L, N, seed=F_ + N).to("cuda"), CNNTrainer, N, 8, (8, 1)))


# ---------------------------------------------------------------------- the batched agents
@pytest.mark.parametrize("B", [1, 65])
@pytest.mark.parametrize("N", [5, 9])
def test_agents(dev, N, B):
    from alphaquoridorgnn_amd import agents as ag

    def workload(env):
        recs = env.from_numpy(_rule_records(N, B))
        out = {"random": ag.random_action_device(recs, N, seed=3)}
        action, visits, actions, count, draws = ag.mcts_action_device(recs, N, evaluations=100, seed=4)       # workspace: exactly ..._workspace_bytes
        out.update(mcts_action=action, mcts_visits=_cut(visits, count), mcts_actions=_cut(actions, count), mcts_count=count, mcts_draws=draws)
        active = env.place(torch.from_numpy((np.arange(B) % 4 != 2).astype(np.uint8)))
        ab, nodes = ag.alpha_beta_action_device(recs, N, max_depth=2, active=active, return_nodes=True)
        out.update(alpha_beta=ab, alpha_beta_nodes=nodes[active == 1])
        value, plies, ndraws, final = ag.playout_batch(recs, seed=5, return_final=True)
        out.update(playout_value=value, playout_plies=plies, playout_draws=ndraws, playout_final=final)
        out["paths"] = ag.shortest_paths_batch(recs)
        return out

    audit(workload)


# ---------------------------------------------------------------------- the replay window
def _generation(N, n, seed):
    rng = np.random.RandomState(seed)
    A = _A(N)
    s = _small(N, n, step=7 + seed)
    visits = (rng.randint(0, 40, size=(n, A)) * (rng.rand(n, A) < 0.3)).astype(np.int16)
    visits[:, 0] += 1
    z = rng.randint(-1, 2, size=n).astype(np.int8)
    q = rng.uniform(-1, 1, size=n).astype(np.float32)
    pi = (visits / np.maximum(visits.sum(1, keepdims=True), 1)).astype(np.float32)
    return s, visits, z, q, pi


@pytest.mark.parametrize("n", [17, 20])
@pytest.mark.parametrize("form", ["counts", "rows", "policy", "blend"])
def test_replay_window(dev, form, n):
    from alphaquoridorgnn_amd import _lib
    from alphaquoridorgnn_amd.replay import ReplayWindow
    N, cap = 5, 20
    A = _A(N)
    first, gen = _generation(N, 11, 1), _generation(N, n, 2)

    def workload(env):
        def append(w, g):
            s, v, z, q, pi = (env.from_numpy(x) for x in g)
            if form == "counts":
                w.append_counts(s, v, z)
            elif form == "rows":
                w.append_rows(s, pi, env.place(z.float()))
            elif form == "policy":
                w.append_policy(s, pi, z, q, 0.25)
            else:
                w.append_counts(s, v, z, q, 0.5)

        w = ReplayWindow(N, max_generations=2, capacity_rows=cap, device=env.dev)
        append(w, first)                                  # 11 rows: the next generation is written from slot 11 and wraps the ring
        append(w, gen)
        assert len(w) == n and (n == cap or int(w.index()[0]) == 11)
        out = dict(zip(("ring72", "ring_pi", "ring_z"), (x.clone() for x in w.tensors())), index=w.index())
        # refresh, both forms, on every other valid slot
        slots = env.place(w.index()[::2])
        k = int(slots.numel())
        rng = np.random.RandomState(9)
        count = rng.randint(0, 6, size=k).astype(np.int32)
        count[0] = _lib.MAX_LEGAL if N == 9 else min(_lib.MAX_LEGAL, A)
        actions = np.stack([rng.permutation(A)[:_lib.MAX_LEGAL] if A >= _lib.MAX_LEGAL else np.resize(rng.permutation(A), _lib.MAX_LEGAL)
                            for _ in range(k)]).astype(np.uint8)
        visits = rng.randint(0, 9, size=(k, _lib.MAX_LEGAL)).astype(np.int32)
        q = rng.uniform(-1, 1, size=k).astype(np.float32)
        w.refresh_counts(slots, env.from_numpy(visits), env.from_numpy(actions), env.from_numpy(count), env.from_numpy(q), 0.5)
        out.update(refreshed_pi=w.tensors()[1].clone(), refreshed_z=w.tensors()[2].clone())
        w.refresh_policy(slots, env.from_numpy(visits.astype(np.float32) / 9), env.from_numpy(actions), env.from_numpy(count))
        out.update(refreshed2_pi=w.tensors()[1].clone(), refreshed2_z=w.tensors()[2].clone())
        out.update(zip(("m72", "m_pi", "m_z", "m_count"), w.merged()))
        train, held = w.holdout_split(0.3, seed=2)
        out.update(train=train, held=held)
        return out

    audit(workload)


def test_replay_merge_surprise_metrics(dev):
    """Merge runs at the exact merge workspace (n - u >= 64 makes it non-empty), surprise rows and counts, row metrics and its
    reduction, over a ring with stale slots and an index."""
    from alphaquoridorgnn_amd import _lib
    from alphaquoridorgnn_amd.replay_merge import merge_positions
    from alphaquoridorgnn_amd.replay_surprise import surprise_index
    from alphaquoridorgnn_amd.validation import holdout_split, row_metrics
    N, rows = 5, 203
    A = _A(N)
    s, visits, z, q, pi = _generation(N, rows, 4)
    s[:] = s[np.arange(rows) % 37]                                     # 37 distinct positions: runs of 5 and 6
    index = np.random.RandomState(3).permutation(rows)[:197].astype(np.int64)
    assert int(_lib.load().aqg_replay_merge_workspace_floats(N, 197, 37)) > 0

    def workload(env):
        net = env.packed(env.guard_module(_fixed_net(N)))
        d72, dpi, dz, didx = env.from_numpy(s), env.from_numpy(pi), env.from_numpy(z.astype(np.float32)), env.from_numpy(index)
        out = dict(zip(("m72", "m_pi", "m_z", "m_count"), merge_positions(d72, dpi, dz, didx, N)))
        out.update(zip(("a72", "a_pi", "a_z", "a_count"), merge_positions(d72, dpi, dz, None, N)))
        stats = {}
        expanded, k, count = surprise_index(net, d72, dpi, didx, seed=5, update=2, chunk_rows=64, stats=stats)
        out.update(expanded=expanded, k=k, count=count)
        m = row_metrics(net, d72, dpi, dz, didx, bucket_plies=2, buckets=5, chunk_rows=64)
        out["metrics_sums"], out["metrics_counts"] = np.asarray(m.sums, dtype=np.float64), np.asarray(m.counts, dtype=np.int64)
        train, held = holdout_split(d72, didx, 0.25, 7, N)
        out.update(train=train, held=held)
        return out

    audit(workload)


# ---------------------------------------------------------------------- exact-size refusals
def _untouched(bands, *views):
    """Every view still holds the pattern it was allocated with (`empty` under the bands), and every pad is intact."""
    torch.cuda.synchronize()
    assert bands.intact() == []
    for v in views:
        want = GB.pad_value(torch, v.dtype, bands.pattern)
        same = torch.isnan(v) if (v.dtype.is_floating_point and want != want) else (v == want)
        assert bool(same.all())


def _last_error():
    from alphaquoridorgnn_amd import _lib
    return _lib.load().aqg_last_error().decode(errors="replace")


@pytest.mark.parametrize("pattern", [0, 1])
def test_one_short_workspace_is_refused(dev, pattern):
    """One float (byte) fewer than the size function returns: a non-zero return, a message, and nothing written -- outputs and
    workspace were allocated with `empty` under the bands, so they must still hold the pattern."""
    from alphaquoridorgnn_amd import _lib
    from alphaquoridorgnn_amd import agents as ag
    from alphaquoridorgnn_amd.constants import board_params
    from tests.test_cnn import _make_net as cnn_net
    from tests.test_gnn_any_shape import _make_net as gnn_net
    lib = _lib.load()
    bands = GB.GuardBands(pattern)
    t = bands.proxy("test")
    f32 = dict(dtype=torch.float32, device=dev)
    st = _lib.stream_ptr(dev)
    N, B = 5, 5
    A = _A(N)
    recs = bands.place(torch.from_numpy(_small(N, B)).to(dev))

    def outputs(width):
        return [t.empty((B, width), **f32), t.empty((B, A), **f32), t.empty((B, A), **f32), t.empty((B,), **f32), t.empty((B,), **f32)]

    # the CNN forward, boards and planes
    net = cnn_net(8, 1, N, seed=1).to(dev)
    nws = int(lib.aqg_cnn_workspace_floats(N, 8, A, B))
    ws, outs, d = t.empty((nws - 1,), **f32), outputs(8), net.cnn_net(dev)
    rc = lib.aqg_cnn_forward_boards(N, _lib.ptr(recs), 0, B, ctypes.byref(d), None, _lib.ptr(ws), nws - 1, *(_lib.ptr(o) for o in outs), st)
    assert rc != 0 and "workspace" in _last_error()
    planes = bands.place(torch.zeros((B, 6, N, N), **f32))
    rc = lib.aqg_cnn_forward_planes(N, _lib.ptr(planes), B, ctypes.byref(d), None, _lib.ptr(ws), nws - 1, *(_lib.ptr(o) for o in outs), st)
    assert rc != 0 and "workspace" in _last_error()
    _untouched(bands, ws, *outs)

    # the fixed network on a small board
    fixed = _fixed_net(N)
    nws = int(lib.aqg_gcn_boards_any_workspace_floats(N, B))
    ws, outs = t.empty((nws - 1,), **f32), outputs(128)
    rc = lib.aqg_gcn_forward_boards_any(N, _lib.ptr(recs), 0, B, _lib.ptr(fixed.packed_weights(dev)), _lib.ptr(ws), nws - 1,
                                        *(_lib.ptr(o) for o in outs), 0, st)
    assert rc != 0 and "workspace" in _last_error()
    _untouched(bands, ws, *outs)

    # the fused any-shape forward
    gen = gnn_net((6, 16, 2), A, seed=2, N=N)
    nws = int(lib.aqg_gcn_boards_general_workspace_floats(N, 16, A, B))
    ws, outs, d = t.empty((nws - 1,), **f32), outputs(16), gen.general_net(dev)
    rc = lib.aqg_gcn_forward_boards_general(N, _lib.ptr(recs), 0, B, ctypes.byref(d), None, _lib.ptr(ws), nws - 1,
                                            *(_lib.ptr(o) for o in outs), st)
    assert rc != 0 and "workspace" in _last_error()
    _untouched(bands, ws, *outs)

    # the gradient norm
    n = 70000
    x = bands.place(torch.ones((n,), **f32))
    nws = int(lib.aqg_optim_workspace_floats(n))
    ws, out = t.empty((nws - 1,), **f32), t.empty((1,), **f32)
    rc = lib.aqg_grad_norm(_lib.ptr(x), n, _lib.ptr(out), _lib.ptr(ws), nws - 1, st)
    assert rc != 0 and "workspace too small" in _last_error()
    _untouched(bands, ws, out)

    # the two agents
    walls, draw = board_params(N)
    E_ = 20
    explore = torch.from_numpy(ag.explore_table(E_)).to(dev)
    nb = int(lib.aqg_agent_mcts_workspace_bytes(N, B, E_))
    ws = t.empty((nb - 1,), dtype=torch.uint8, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    outs = [t.empty((B,), **i32), t.empty((B, _lib.MAX_LEGAL), **i32), t.empty((B, _lib.MAX_LEGAL), dtype=torch.uint8, device=dev),
            t.empty((B,), **i32), t.empty((B,), **i32)]
    rc = lib.aqg_agent_mcts(N, _lib.ptr(recs), B, E_, draw, _lib.ptr(explore), None, 0, 1, _lib.ptr(ws), nb - 1, *(_lib.ptr(o) for o in outs), st)
    assert rc != 0 and "workspace" in _last_error()
    _untouched(bands, ws, *outs)
    nb = int(lib.aqg_agent_alpha_beta_workspace_bytes(N, B, 2))
    ws, action, nodes = t.empty((nb - 1,), dtype=torch.uint8, device=dev), t.empty((B,), **i32), t.empty((B,), dtype=torch.int64, device=dev)
    rc = lib.aqg_agent_alpha_beta(N, _lib.ptr(recs), B, None, draw, draw // 2 - walls, 2, _lib.ptr(ws), nb - 1, _lib.ptr(action), _lib.ptr(nodes), st)
    assert rc != 0 and "workspace" in _last_error()
    _untouched(bands, ws, action, nodes)


@pytest.mark.parametrize("kind", ["general", "cnn"])
def test_one_short_trainer_workspace_is_refused(dev, kind):
    """The two workspace trainers with workspace_floats one below aqg_*_train_workspace_floats: the step is refused, and parameters,
    moments, gradients, outputs and the workspace are what they were."""
    from alphaquoridorgnn_amd import _lib
    from alphaquoridorgnn_amd import train_network as tn
    N, B = 5, 4
    A = _A(N)
    bands = GB.GuardBands(1)
    with pytest.MonkeyPatch.context() as mp:
        bands.install(mp, [tn])
        env = Env(dev, bands)
        if kind == "general":
            from tests.test_gnn_any_shape import _make_net
            tr = tn.GeneralTrainer(env.guard_module(_make_net((6, 16, 2), A, seed=3, N=N)), max_batch=B)
        else:
            from tests.test_cnn import _make_net
            tr = tn.CNNTrainer(env.guard_module(_make_net(8, 1, N, seed=3).to(dev)), max_batch=B)
        pi, z = E.edge_targets(B, A, seed=1)
        s72, p, zz = env.from_numpy(_small(N, B)), env.from_numpy(pi), env.from_numpy(z)
        tr.t.workspace_floats = tr.ws["workspace"].numel() - 1
        watched = tr.params + tr.buffers + tr.adam_m + tr.adam_v + [tr.flat_grads] + [tr.ws[k] for k in ("workspace", "pol", "val", "loss")]
        torch.cuda.synchronize()
        before = [x.detach().cpu().numpy().tobytes() for x in watched]
        for update in (False, True):
            with pytest.raises(_lib.HipLibraryError, match="workspace too small"):
                tr.step(s72, p, zz, update=update)
        with pytest.raises(_lib.HipLibraryError, match="workspace too small"):
            tr.run_epoch(s72, p, zz, torch.arange(B, device=dev))
        torch.cuda.synchronize()
        assert bands.intact() == []
        assert [x.detach().cpu().numpy().tobytes() for x in watched] == before
