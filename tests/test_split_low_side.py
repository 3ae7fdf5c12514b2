"""The fp16-split kernels on the LOW side of fp16 range (gpu).

The default 9x9 hot path carries every f32 operand as hi = f16(x), lo = f16(x - hi): fp32-equivalent only while lo is a normal
fp16 number.  Below |x| ~ 2^-3 lo is subnormal and the pair's absolute error stops shrinking at ~2^-25; below 2^-14 hi is
subnormal too.  The networks here are ONE function in many scalings (tests/_low_side.py: a layer's weight and bias times 2^-k, the
next layer's weight times 2^k -- exact multiples in f32, the same fp64 oracle to 1e-9), which the reference's fp32 serves without
blinking; every path that can meet them -- the module's forward, the raw C entry, the engine, the split training step -- is held
to the bars the suite already states for it, against the fp64 oracle of the BASE set.

Every test prints, per (site, k), the worst observed error as a multiple of its bar (lines starting LOWSIDE), all cells before it
asserts any."""
import numpy as np
import pytest
import torch

from tests import _low_side as L
from tests import _util as U
from tests.test_gpu_parity import TRAIN_FUSED_DEFAULT, _root_children, _train_batch   # noqa: E402

pytestmark = pytest.mark.gpu

SITES = list(L.SITES)


@pytest.fixture(scope="module")
def dev():
    from alphaquoridorgnn_amd import _lib
    _lib.load()          # raises if the HIP library is missing: no fallback
    return _lib.require_gpu()


@pytest.fixture(scope="module")
def world():
    """48 reference-walk states, the base weights, their fp64 oracle -- and, once, the condition everything here rests on: the
    oracle of every rescaled set equals the base set's to 1e-9 relative (the reference alone stays within every bar)."""
    from oracle import gnn as og
    states = U.golden("walk_9x9.npz")["states"]
    recs = states[np.linspace(0, states.shape[0] - 1, 48).astype(int)]
    base = L.base_params(3)
    for site in SITES:
        for k in L.KS:
            L.assert_same_function(base, L.rescale(base, site, k)[0], recs)
    return recs, base, og.forward_states_dense(base, recs)


def _load(params, dev):
    from alphaquoridorgnn_amd.pv_network_gnn import GNNNetwork
    m = GNNNetwork()
    m.load_state_dict({k: torch.from_numpy(np.asarray(v).copy()) for k, v in params.items()})
    return m.to(dev).eval()


def _forward_ratio(ref, logits, vpre, policy):
    """Worst error as a multiple of the forward bars: logits and value_pre atol 1e-5 rtol 1e-4, policy 1e-6 / 1e-4."""
    return max(L.bar_ratio(logits, ref["logits"], 1e-5, 1e-4), L.bar_ratio(vpre, ref["value_pre"], 1e-5, 1e-4),
               L.bar_ratio(policy, ref["policy"], 1e-6, 1e-4))


# ------------------------------------------------------------------ forward through the module
@pytest.mark.parametrize("site", SITES)
def test_forward_states_on_rescaled_networks(dev, world, site):
    """model.forward_states on every rescaling of `site`, trunk_variant 3 and 6, LDS poisoned first: logits, value_pre and policy
    within the forward bars of the base set's fp64 oracle, whichever kernel family the module chose -- except that k = 0 is
    GNN_RANGE_PROVEN as ever and k = 4 is still on the split kernels (correctness is not to be bought by sending ordinary
    networks to the slow ones)."""
    from alphaquoridorgnn_amd import _lib
    recs, base, ref = world
    d = torch.from_numpy(recs).to(dev)
    bad = []
    try:
        for variant in (3, 6):
            _lib.set_option("trunk_variant", variant)
            for k in L.KS:
                model = _load(L.rescale(base, site, k)[0], dev)
                flags = model.gnn_flags(dev)
                _lib.poison_lds(dev)
                policy, _, logits, vpre = model.forward_states(d, want_logits=True)
                r = _forward_ratio(ref, logits.cpu().numpy(), vpre.cpu().numpy(), policy.cpu().numpy())
                print(f"LOWSIDE forward_states site={site} k={k} variant={variant} flags={flags}->{model.gnn_flags(dev)} ratio={r:.3g}")
                if not r <= 1.0:
                    bad.append((variant, k, "bar", r))
                if k == 0 and flags != _lib.GNN_RANGE_PROVEN:
                    bad.append((variant, k, "flags", flags))
                if k == 4 and (flags & _lib.GNN_EXACT_F32 or model.gnn_flags(dev) & _lib.GNN_EXACT_F32):
                    bad.append((variant, k, "flags", flags))
    finally:
        _lib.set_option("trunk_variant", 3)
    assert not bad, bad


def test_calibration_catches_what_the_packing_admits(dev, world):
    """The packing's test looks at a matrix's largest entry only.  gcn_layers.1 scaled down by 2^-10 (gcn_layers.2 up) with ONE entry
    put back at 2^-8 passes it -- positive GUARD thresholds, no `saturated` word -- yet is the k = 10 network to the split kernels: 6 x
    the forward bar.  It is the calibration that has to refuse this set, and only at the bar stated for the split kernels does it:
    at ten times that bar (1e-4 + 1e-3 |x|) the k = 10 rescalings passed.  gnn_flags is GNN_EXACT_F32, and the module's outputs
    are within the forward bars of this set's own fp64 oracle."""
    from alphaquoridorgnn_amd import _lib
    from oracle import gnn as og
    lib = _lib.load()
    recs, base, _ = world
    p, _ = L.rescale(base, "gcn1/gcn2", 10)
    p["gcn_layers.1.lin.weight"][0, 0] = np.float32(2.0 ** -8)
    ref = og.forward_states_dense(p, recs)
    model = _load(p, dev)
    pk = model.packed_weights(dev)
    assert pk[-4:].cpu().tolist()[:2] == pytest.approx([(65504.0 - L.CQ * 5.0 ** 0.5 * 1.0 * 2.0 ** -10) / 2.07, 65504.0], abs=1e-2)   # admitted
    d = torch.from_numpy(recs).to(dev)
    B, A = recs.shape[0], 209
    word = torch.zeros((1,), dtype=torch.int32, device=dev)
    pooled, logits, vpre = torch.empty((B, 128), device=dev), torch.empty((B, A), device=dev), torch.empty((B,), device=dev)
    policy = torch.empty((B, A), device=dev)
    _lib.check(lib.aqg_gcn_forward_boards_guarded(9, _lib.ptr(d), 0, B, _lib.ptr(pk), _lib.ptr(pooled), _lib.ptr(logits), _lib.ptr(policy),
                                                  _lib.ptr(vpre), None, 0, _lib.ptr(word), _lib.stream_ptr(dev)), "guarded")
    r_split = _forward_ratio(ref, logits.cpu().numpy(), vpre.cpu().numpy(), policy.cpu().numpy())
    flags = model.gnn_flags(dev)
    _lib.poison_lds(dev)
    policy, _, logits, vpre = model.forward_states(d, want_logits=True)
    r = _forward_ratio(ref, logits.cpu().numpy(), vpre.cpu().numpy(), policy.cpu().numpy())
    print(f"LOWSIDE calibration site=gcn1/gcn2 k=10 one_entry=2^-8 saturated={int(word.item())} split_ratio={r_split:.3g} flags={flags} ratio={r:.3g}")
    assert int(word.item()) == 0 and r_split > 1.0            # the case is what it claims to be: no signal, outside the bar
    assert flags == _lib.GNN_EXACT_F32
    assert r <= 1.0


# ------------------------------------------------------------------ the raw C entry
@pytest.mark.parametrize("site", SITES)
def test_guarded_entry_is_inside_the_bar_or_says_so(dev, world, site):
    """aqg_gcn_forward_boards_guarded with flags 0 -- the split kernels, none of the module's calibration: for every rescaled set
    either ALL outputs are inside the forward bars or the `saturated` word is raised ("or could not rule one out", include/aqgnn.h,
    on the low side too).  The ordinary sets (k = 0, k = 4) leave the word alone and are inside the bar."""
    from alphaquoridorgnn_amd import _lib
    lib = _lib.load()
    recs, base, ref = world
    d = torch.from_numpy(recs).to(dev)
    B, A = recs.shape[0], 209
    bad = []
    for k in L.KS:
        pk = _load(L.rescale(base, site, k)[0], dev).packed_weights(dev)
        word = torch.zeros((1,), dtype=torch.int32, device=dev)
        pooled = torch.empty((B, 128), device=dev)
        logits, policy = torch.empty((B, A), device=dev), torch.empty((B, A), device=dev)
        vpre, value = torch.empty((B,), device=dev), torch.empty((B,), device=dev)
        _lib.poison_lds(dev)
        _lib.check(lib.aqg_gcn_forward_boards_guarded(9, _lib.ptr(d), 0, B, _lib.ptr(pk), _lib.ptr(pooled), _lib.ptr(logits), _lib.ptr(policy),
                                                      _lib.ptr(vpre), _lib.ptr(value), 0, _lib.ptr(word), _lib.stream_ptr(dev)), "guarded")
        raised = int(word.item())
        r = _forward_ratio(ref, logits.cpu().numpy(), vpre.cpu().numpy(), policy.cpu().numpy())
        print(f"LOWSIDE guarded_entry site={site} k={k} saturated={raised} ratio={r:.3g}")
        if not (r <= 1.0 or raised):
            bad.append((k, "outside the bar, word not raised", r))
        if k in (0, 4) and (raised or not r <= 1.0):
            bad.append((k, "ordinary set", raised, r))
    assert not bad, bad


# ------------------------------------------------------------------ engine
_ENGINE_REF = {}


def _engine_reference(base):
    """Roots, oracle priors and oracle visit counts of test_engine_priors_and_visits_vs_oracle_gnn, for the base set (once)."""
    from oracle import gnn as og, mcts as om, quoridor as oq
    if not _ENGINE_REF:
        g = U.golden("walk_9x9.npz")
        recs = np.stack([g["states"][i] for i in [0, 5, 40, 333, 1200, 2600, 5000, 9000]])
        recs = recs[[not (oq.State(r).is_done()) for r in recs]]
        oracle = og.OracleModel(base)
        want = []
        for rec in recs:
            st = oq.State(rec)
            want.append((st.legal_actions(), oracle.predict(st)[0], [c.n for c in om.search(oracle, st, 10).children]))
        _ENGINE_REF["v"] = (recs, want)
    return _ENGINE_REF["v"]


@pytest.mark.parametrize("step_heads", [1, 0])
@pytest.mark.parametrize("site", ["gcn1/gcn2", "gcn0/gcn1"])
def test_engine_search_on_rescaled_networks(dev, world, site, step_heads):
    """BatchedSelfPlay.search, 10 simulations from the eight roots of test_engine_priors_and_visits_vs_oracle_gnn, with the k = 10
    rescaling of `site`: root priors within that test's bar (1e-6 / 1e-5) of OracleModel.predict, child i = legal action i, visit
    counts equal to oracle.mcts.search; with the heads inside the step kernel and without."""
    from alphaquoridorgnn_amd import _lib
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    _, base, _ = world
    recs, want = _engine_reference(base)
    model = _load(L.rescale(base, site, 10)[0], dev)
    _lib.set_option("step_heads", step_heads)
    try:
        eng = BatchedSelfPlay(model, num_games=recs.shape[0], sims=10, record_history=False)
        eng.search(recs)
        torch.cuda.synchronize()
        got = _root_children(eng)
    finally:
        _lib.set_option("step_heads", 1)
    worst, bad = 0.0, []
    for i, ((pri, vis, act), (legal, prior, visits)) in enumerate(zip(got, want)):
        assert [int(a) for a in act] == [int(a) for a in legal]
        r = L.bar_ratio(pri, prior, 1e-6, 1e-5)
        worst = max(worst, r)
        if not r <= 1.0:
            bad.append((i, "priors", r))
        if [int(v) for v in vis] != visits:
            bad.append((i, "visits", [int(v) for v in vis], visits))
    print(f"LOWSIDE engine_search site={site} k=10 step_heads={step_heads} flags={model.gnn_flags(dev)} ratio={worst:.3g}")
    assert not bad, bad


# ------------------------------------------------------------------ training step
_TRAIN_REF = {}


def _train_reference(base):
    """Batch of 48 (kink filter on the BASE set: the pre-activations of a rescaled set are exact multiples of its), and the fp64
    autograd step of oracle/train.py on the base set (once)."""
    from oracle import train as ot
    if not _TRAIN_REF:
        recs, pi, z = _train_batch(48, 7, params=base)
        _TRAIN_REF["v"] = (recs, pi, z, ot.train_steps(base, [(recs, pi.astype(np.float64), z.astype(np.float64))])[0])
    return _TRAIN_REF["v"]


def _train_step_ratios(dev, params, gfac, fused, batch_ref):
    """One update=False step: (loss ratio to 1e-5 relative, worst gradient ratio to 2e-5 max|g| + 1e-7 after undoing the scaling and
    the tensor it is at, fallbacks counted)."""
    from alphaquoridorgnn_amd import _lib
    from alphaquoridorgnn_amd.train_network import GNNTrainer
    from oracle import gnn as og
    lib = _lib.load()
    recs, pi, z, ref = batch_ref
    model = _load(params, dev)
    _lib.set_option("train_fused", fused)
    try:
        tr = GNNTrainer(model, max_batch=64)
        _lib.poison_lds(dev)
        lib.aqg_gcn_train_fallbacks(1)
        pl, vl = tr.step(torch.from_numpy(recs), torch.from_numpy(pi), torch.from_numpy(z), update=False)
        fallbacks = int(lib.aqg_gcn_train_fallbacks(1))
    finally:
        _lib.set_option("train_fused", TRAIN_FUSED_DEFAULT)
    loss_r = max(abs(float(pl) - ref["policy_loss"]) / (1e-5 * abs(ref["policy_loss"])),
                 abs(float(vl) - ref["value_loss"]) / (1e-5 * abs(ref["value_loss"])))
    grad_r, at = 0.0, None
    for key, gt in zip(og.KEYS, tr.grads):
        r = ref["grads"][key]
        g = gt.cpu().numpy().astype(np.float64) / gfac[key]             # the exact power of two the rescaling put on this gradient
        e = np.abs(g - r)
        q = float(np.where(np.isfinite(e), e, np.inf).max()) / (2e-5 * np.abs(r).max() + 1e-7)
        if q > grad_r:
            grad_r, at = q, key
    return (loss_r if np.isfinite(loss_r) else float("inf")), grad_r, at, fallbacks


@pytest.mark.parametrize("site", SITES)
def test_split_training_step_on_rescaled_networks(dev, world, site):
    """train_fused 2 (the split step), batch 48, update=False, k in {0, 3, 4, 8, 12, 16}: both losses within 1e-5 relative of
    oracle/train.py, every gradient -- multiplied back by the exact factor of its tensor, so that the absolute term does not
    swallow a down-scaled one -- within 2e-5 max|g| + 1e-7 of the BASE set's fp64 gradient: the bar of
    test_train_step_gradients_vs_autograd.  The fallback count is printed; it must be 0 at k = 0 and at k = 3, the last k the split
    form is meant to serve (0.08 of the bar or less there: ordinary networks are not to pay for both bodies).  (k = 4 is where the split form
    was last inside the bar before it learned to hand such steps to its f32 body: 0.1 to 0.9 of it, then 50 x at k = 5 -- the ReLU
    masks of a layer scaled down that far are decided by the split's absolute error.)"""
    _, base, _ = world
    batch_ref = _train_reference(base)
    bad = []
    for k in (0, 3, 4, 8, 12, 16):
        p, gfac = L.rescale(base, site, k)
        loss_r, grad_r, at, fb = _train_step_ratios(dev, p, gfac, 2, batch_ref)
        print(f"LOWSIDE train_step site={site} k={k} train_fused=2 fallbacks={fb} loss_ratio={loss_r:.3g} grad_ratio={grad_r:.3g} at={at}")
        if not loss_r <= 1.0:
            bad.append((k, "loss", loss_r))
        if not grad_r <= 1.0:
            bad.append((k, "gradient", at, grad_r))
        if k in (0, 3) and fb != 0:
            bad.append((k, "fallbacks", fb))
    assert not bad, bad


def test_f32_training_step_on_rescaled_networks(dev, world):
    """The f32-input form of the step (train_fused 1) at k = 16, every site: the same bar -- the reference path stays inside it, so
    the bar is one an fp32 implementation meets."""
    _, base, _ = world
    batch_ref = _train_reference(base)
    bad = []
    for site in SITES:
        p, gfac = L.rescale(base, site, 16)
        loss_r, grad_r, at, fb = _train_step_ratios(dev, p, gfac, 1, batch_ref)
        print(f"LOWSIDE train_step site={site} k=16 train_fused=1 fallbacks={fb} loss_ratio={loss_r:.3g} grad_ratio={grad_r:.3g} at={at}")
        if not (loss_r <= 1.0 and grad_r <= 1.0):
            bad.append((site, loss_r, grad_r, at))
    assert not bad, bad
