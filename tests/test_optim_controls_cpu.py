"""The optimiser controls without a GPU: train_network's numpy statements (adam_reference, clip_coefficient) against CPU torch
(Adam(weight_decay=), AdamW, clip_grad_norm_), the guard that the chosen decays and clip levels are visible at the Adam bar, the
aqg_optim layout against a C++ compile of the header, every host-side refusal of the new entry points, the default decay mask
of the three network kinds, and train_cycle's options."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import _optim_controls as OC   # noqa: E402

SHAPES = [(24, 16), (24,), (12, 24), (12,), (1, 12), (1,)]
MASK = [len(s) >= 2 for s in SHAPES]
# (weight_decay, decoupled, clipped)
CONFIGS = {"plain": (0.0, True, False), "clip": (0.0, True, True), "coupled+clip": (OC.DECAY, False, True),
           "decoupled+clip": (OC.DECAY, True, True), "decoupled": (OC.DECAY, True, False), "coupled": (OC.DECAY, False, False)}


def _problem(seed=0):
    """Parameters at initialisation scale and three steps of gradients as consecutive batches give them: a direction per tensor
    that persists under 60 % batch noise, at a scale that differs per tensor."""
    rng = np.random.RandomState(seed)
    params = [rng.uniform(-0.2, 0.2, s).astype(np.float32) for s in SHAPES]
    base = [rng.randn(*s) * 10.0 ** rng.uniform(-3, 0) for s in SHAPES]
    grads = [[(b * (1.0 + 0.6 * rng.randn(*b.shape))).astype(np.float32) for b in base] for _ in range(3)]
    return params, grads


def _max_norms(grads, clipped):
    return [f * OC.global_norm64(g) if clipped else None for f, g in zip(OC.CLIP_FACTORS, grads)]


def _numpy_run(params, grads, wd, decoupled, max_norms):
    from alphaquoridorgnn_amd.train_network import adam_reference, clip_coefficient
    p = [x.copy() for x in params]
    m = [np.zeros_like(x) for x in params]
    v = [np.zeros_like(x) for x in params]
    out = []
    for step, (g, mx) in enumerate(zip(grads, max_norms), start=1):
        norm = np.float32(np.sqrt(np.float32(sum(np.float32((x.astype(np.float32) ** 2).sum()) for x in g))))
        coef = 1.0 if mx is None else clip_coefficient(norm, mx)
        for i in range(len(p)):
            p[i], m[i], v[i] = adam_reference(p[i], g[i], m[i], v[i], step, lr=OC.LRS[step - 1], weight_decay=wd if MASK[i] else 0.0,
                                              decoupled=decoupled, coef=coef)
            assert p[i].dtype == m[i].dtype == v[i].dtype == np.float32
        out.append([x.copy() for x in p])
    return out


@pytest.mark.parametrize("name", list(CONFIGS))
def test_numpy_statements_against_torch(name):
    wd, decoupled, clipped = CONFIGS[name]
    params, grads = _problem()
    mx = _max_norms(grads, clipped)
    ref = OC.shadow_run(params, grads, list(OC.LRS), wd, decoupled, MASK, mx)
    got = _numpy_run(params, grads, wd, decoupled, mx)
    for i in range(3):
        OC.assert_adam_bar(got[i], ref[i], grads[i], OC.LRS[i], (name, i))


def test_clip_coefficient_against_torch():
    from alphaquoridorgnn_amd.train_network import clip_coefficient
    rng = np.random.RandomState(1)
    g = rng.randn(1000).astype(np.float32)
    norm = np.float32(np.linalg.norm(g.astype(np.float64)))
    for factor in (0.1, 0.5, 0.999999, 1.0, 1.5, 1e30 / float(norm)):
        t = torch.nn.Parameter(torch.zeros(1000))
        t.grad = torch.from_numpy(g.copy())
        torch.nn.utils.clip_grad_norm_([t], factor * float(norm))
        coef = clip_coefficient(norm, factor * float(norm))
        assert coef.dtype == np.float32
        np.testing.assert_allclose(t.grad.numpy(), coef * g, rtol=3e-7)
    assert clip_coefficient(norm, 2.0 * float(norm)) == np.float32(1.0)             # nothing clipped: exactly one
    assert clip_coefficient(norm, 1e30) == np.float32(1.0)
    assert np.isnan(clip_coefficient(np.float32("nan"), 1.0))                         # torch.clamp keeps a NaN
    assert clip_coefficient(np.float32("inf"), 1.0) == 0.0


@pytest.mark.parametrize("name", [n for n in CONFIGS if n != "plain"])
def test_chosen_options_are_visible(name):
    """The guard of tests/_optim_controls.assert_visible on this file's problem: without it a comparison at the Adam bar could pass
    with the option ignored."""
    wd, decoupled, clipped = CONFIGS[name]
    params, grads = _problem()
    with_option = OC.shadow_run(params, grads, list(OC.LRS), wd, decoupled, MASK, _max_norms(grads, clipped))
    without = OC.shadow_run(params, grads, list(OC.LRS))
    OC.assert_visible(with_option[-1], without[-1], params, name)


def test_coupled_and_decoupled_differ():
    params, grads = _problem()
    a = OC.shadow_run(params, grads, list(OC.LRS), OC.DECAY, True, MASK)[-1]
    b = OC.shadow_run(params, grads, list(OC.LRS), OC.DECAY, False, MASK)[-1]
    OC.assert_visible(a, b, params, "decoupled against coupled")


# ---------------------------------------------------------------------------------------------- the C ABI on the host
def _lib_or_fail():
    from alphaquoridorgnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} missing: build first")
    return _lib, _lib.load()


def test_optim_layout_matches_header(tmp_path):
    from alphaquoridorgnn_amd import _lib
    fields = ["decoupled", "num_tensors", "weight_decay", "max_grad_norm", "grad_norm", "workspace", "workspace_floats"]
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "aqgnn.h"\nint main() { std::printf("%zu'
                   + " %zu" * len(fields) + '\\n", sizeof(aqg_optim)' + "".join(f", offsetof(aqg_optim, {f})" for f in fields)
                   + "); }\n")
    exe = tmp_path / "layout"
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    T = _lib.OptimStruct
    assert got == [ctypes.sizeof(T)] + [getattr(T, f).offset for f in fields]


def test_abi_number_unchanged():
    _, lib = _lib_or_fail()
    assert lib.aqg_abi_version() == 15


def _flat(arr, numel, base=1 << 20):
    """Fill a struct's pointer array with consecutive views of one (never dereferenced) flat buffer."""
    off = base
    for i, n in enumerate(numel):
        arr[i] = off
        off += 4 * n


def _fused(_lib, N=5):
    A = N * N + 2 * (N - 1) ** 2
    t = _lib.TrainStruct()
    t.board_size, t.batch, t.policy_size, t.step = N, 4, A, 1
    t.lr, t.beta1, t.beta2, t.eps = 1e-3, 0.9, 0.999, 1e-8
    numel = [128 * 6, 128, 128 * 128, 128, 128 * 128, 128, 64 * 128, 64, A * 64, A, 64 * 128, 64, 64, 1]
    for name in ("params", "adam_m", "adam_v"):
        for i in range(14):
            getattr(t, name)[i] = 4096
    _flat(t.grads, numel)
    return t, numel


def _general(_lib, N=5, hidden=32, layers=2):
    A = N * N + 2 * (N - 1) ** 2
    t = _lib.TrainGeneralStruct()
    t.board_size, t.num_features, t.hidden, t.num_layers, t.policy_size, t.batch, t.step = N, 6, hidden, layers, A, 4, 1
    t.lr, t.beta1, t.beta2, t.eps = 1e-3, 0.9, 0.999, 1e-8
    h = hidden // 2
    numel = [x for l in range(layers) for x in (hidden * (6 if l == 0 else hidden), hidden)] + [h * hidden, h, A * h, A, h * hidden, h, h, 1]
    for name in ("params", "adam_m", "adam_v"):
        for i in range(len(numel)):
            getattr(t, name)[i] = 4096
    _flat(t.grads, numel)
    t.workspace, t.workspace_floats = 4096, 1
    return t, numel


def _cnn(_lib, N=5, F=8, L=1):
    A = N * N + 2 * (N - 1) ** 2
    t = _lib.CnnTrainStruct()
    t.board_size, t.num_filters, t.num_blocks, t.policy_size, t.batch, t.step = N, F, L, A, 4, 1
    t.lr, t.beta1, t.beta2, t.eps = 1e-3, 0.9, 0.999, 1e-8
    C = 2 * L + 1
    numel = [x for l in range(C) for x in ((54 if l == 0 else 9 * F) * F, F, F)] + [A * F, A, F, 1]
    for l in range(C):
        t.bn_eps[l], t.bn_momentum[l] = 1e-5, 0.1
        t.running_mean[l] = t.running_var[l] = 4096
    for i in range(len(numel)):
        t.params[i] = 4096
    _flat(t.grads, numel)
    t.adam_table = 4096
    t.workspace, t.workspace_floats = 4096, 1
    return t, numel


ENTRY = {"fused": ("aqg_gcn_train_step_optim", "aqg_gcn_train_steps_optim", _fused),
         "general": ("aqg_gcn_train_step_general_optim", "aqg_gcn_train_steps_general_optim", _general),
         "cnn": ("aqg_cnn_train_step_optim", "aqg_cnn_train_steps_optim", _cnn)}


def _optim(_lib, tensors, wd=None, max_norm=0.0, norm_ptr=None, ws=4096, ws_floats=1 << 20, num_tensors=None):
    o = _lib.OptimStruct()
    o.decoupled = 1
    if wd is not None:
        o._wd = (ctypes.c_float * tensors)(*([wd] * tensors if not isinstance(wd, list) else wd))
        o.weight_decay = ctypes.cast(o._wd, ctypes.POINTER(ctypes.c_float))
        o.num_tensors = tensors if num_tensors is None else num_tensors
    o.max_grad_norm = max_norm
    o.grad_norm = norm_ptr
    o.workspace, o.workspace_floats = ws, ws_floats
    return o


@pytest.mark.parametrize("kind", list(ENTRY))
def test_optim_entry_points_refuse_on_the_host(kind):
    """Everything section "optimiser controls" of include/aqgnn.h says is refused, on never-dereferenced pointers: each refusal
    happens before any launch, so none of these calls touches a device."""
    _lib, lib = _lib_or_fail()
    step_name, steps_name, make = ENTRY[kind]
    step, steps = getattr(lib, step_name), getattr(lib, steps_name)
    dummy = ctypes.c_void_p(4096)
    t, numel = make(_lib)
    T = len(numel)
    need = lib.aqg_optim_workspace_floats(sum(numel))
    assert need >= 1

    def refused(o, msg, struct=t, modes=(0, 1, 2)):
        for mode in modes:
            assert step(ctypes.byref(struct), dummy, dummy, dummy, mode, ctypes.byref(o), None) < 0, (msg, mode)
            assert msg in lib.aqg_last_error().decode(), (msg, mode, lib.aqg_last_error().decode())
        assert steps(ctypes.byref(struct), dummy, dummy, dummy, None, 8, None, ctypes.byref(o), None) < 0, msg
        assert msg in lib.aqg_last_error().decode(), (msg, lib.aqg_last_error().decode())

    refused(_optim(_lib, T, wd=-1e-3), "weight decay")
    refused(_optim(_lib, T, wd=[0.0] * (T - 1) + [float("nan")]), "weight decay")
    refused(_optim(_lib, T, wd=float("inf")), "weight decay")
    refused(_optim(_lib, T, wd=1e-3, num_tensors=T - 1), "num_tensors")
    refused(_optim(_lib, T, max_norm=-1.0), "max_grad_norm")
    refused(_optim(_lib, T, max_norm=float("inf")), "max_grad_norm")
    refused(_optim(_lib, T, max_norm=float("nan")), "max_grad_norm")
    refused(_optim(_lib, T, max_norm=1.0, ws_floats=need - 1), "workspace too small")
    refused(_optim(_lib, T, max_norm=1.0, ws=None), "workspace too small")
    refused(_optim(_lib, T, norm_ptr=4096, ws_floats=need - 1), "workspace too small")      # the norm alone needs it too
    t2, _ = make(_lib)
    t2.grads[3] += 4                                                                         # one tensor off the flat buffer
    refused(_optim(_lib, T, max_norm=1.0), "consecutive", struct=t2)
    refused(_optim(_lib, T, norm_ptr=4096), "consecutive", struct=t2)
    # the plain call's own refusals come first and keep their texts
    assert step(None, dummy, dummy, dummy, 1, ctypes.byref(_optim(_lib, T, max_norm=1.0)), None) < 0
    assert step(ctypes.byref(t), dummy, dummy, dummy, 3, ctypes.byref(_optim(_lib, T, max_norm=1.0)), None) < 0
    assert "bad argument" in lib.aqg_last_error().decode()
    t3, _ = make(_lib)
    t3.step = 0
    assert step(ctypes.byref(t3), dummy, dummy, dummy, 1, ctypes.byref(_optim(_lib, T, max_norm=1.0)), None) < 0
    assert "step must be >= 1" in lib.aqg_last_error().decode()


def _set(**fields):
    def change(t):
        for k, v in fields.items():
            setattr(t, k, v)
    return change


def _no_tensors(t):
    for i in range(len(t.params)):
        t.params[i] = None


def _index(name, i, value):
    def change(t):
        getattr(t, name)[i] = value
    return change


# (change to a good struct, mode, states72 given, message): what the plain step entry refuses on the host in
# test_train_general_cpu / test_cnn_train_cpu (test_entry_points_check_arguments_on_the_host), and the fused kind's own three
_BAD_MODE, _NO_STATES = (_set(), 3, True, "bad argument"), (_set(), 1, False, "null argument")
STEP_REFUSALS = {
    "fused": [_BAD_MODE, _NO_STATES, (_no_tensors, 1, True, "null parameter tensor"), (_set(step=0), 1, True, "step must be >= 1")],
    "general": [_BAD_MODE, _NO_STATES, (_set(board_size=4), 1, True, "board_size"), (_set(hidden=1), 1, True, "hidden"),
                (_set(hidden=2048), 1, True, "hidden"), (_set(num_layers=0), 1, True, "num_layers"),
                (_set(num_layers=33), 1, True, "num_layers"), (_set(policy_size=0), 1, True, "policy_size"),
                (_set(policy_size=5000), 1, True, "policy_size"), (_set(step=0), 1, True, "step"),
                (_no_tensors, 1, True, "null parameter"), (_set(num_features=8), 1, True, "num_features"),
                (_set(batch=-1), 0, True, "negative batch"), (_set(), 1, True, "workspace too small")],
    "cnn": [_BAD_MODE, _NO_STATES, (_set(board_size=4), 1, True, "board_size"), (_set(num_filters=0), 1, True, "num_filters"),
            (_set(num_filters=513), 1, True, "num_filters"), (_set(num_blocks=41), 1, True, "num_blocks"),
            (_set(num_blocks=-1), 1, True, "num_blocks"), (_set(policy_size=40), 1, True, "policy_size"),
            (_no_tensors, 1, True, "null parameter"), (_index("running_var", 2, None), 1, True, "running statistics"),
            (_index("bn_momentum", 0, 1.5), 1, True, "bn_momentum"), (_index("bn_eps", 2, 0.0), 1, True, "bn_eps"),
            (_set(adam_table=None), 1, True, "adam_table"), (_set(step=0), 1, True, "step"),
            (_set(), 1, True, "workspace too small"), (_set(batch=-1), 0, True, "negative batch")],
}
# (change, positions, states72 given, message) of the steps entry
STEPS_REFUSALS = {
    "fused": [(_set(), -1, True, "bad argument"), (_set(), 8, False, "bad argument"), (_no_tensors, 8, True, "null parameter tensor"),
              (_set(step=0), 8, True, "step must be >= 1")],
    "general": [(_set(), 10, True, "workspace too small"), (_set(batch=0), 10, True, "batch"), (_set(), -1, True, "bad argument"),
                (_set(), 10, False, "bad argument")],
    "cnn": [(_set(), -1, True, "bad argument"), (_set(), 4, False, "bad argument"), (_set(batch=0), 4, True, "batch"),
            (_set(), 4, True, "workspace too small"), (_no_tensors, 4, True, "null parameter")],
}


@pytest.mark.parametrize("kind", list(ENTRY))
def test_optim_forms_make_the_plain_calls_refusals(kind):
    """Every host-side refusal of a plain step / steps entry comes out of its _optim form too, with an all-off (zeroed) aqg_optim:
    the same sign and the same words.  Never-dereferenced pointers: each call returns on the host before any launch."""
    _lib, lib = _lib_or_fail()
    step_name, steps_name, make = ENTRY[kind]
    dummy, off = ctypes.c_void_p(4096), _lib.OptimStruct()

    def both(name, change, args, msg):
        t, _ = make(_lib)
        change(t)
        plain = getattr(lib, name[:-len("_optim")])(ctypes.byref(t), *args, None)
        plain_said = lib.aqg_last_error().decode()
        optim = getattr(lib, name)(ctypes.byref(t), *args, ctypes.byref(off), None)
        optim_said = lib.aqg_last_error().decode()
        if msg is None:
            assert plain == 0 and optim == 0, (name, plain, optim)
        else:
            assert plain < 0 and optim < 0, (name, msg, plain, optim)
            assert msg in plain_said and msg in optim_said, (name, msg, plain_said, optim_said)

    for change, mode, states, msg in STEP_REFUSALS[kind]:
        both(step_name, change, (dummy if states else None, dummy, dummy, mode), msg)
    for change, positions, states, msg in STEPS_REFUSALS[kind]:
        both(steps_name, change, (dummy if states else None, dummy, dummy, None, positions, None), msg)
    for name in (step_name, steps_name):                       # a null struct, through both forms
        args = (dummy, dummy, dummy, 1) if name == step_name else (dummy, dummy, dummy, None, 8, None)
        assert getattr(lib, name[:-len("_optim")])(None, *args, None) < 0 and getattr(lib, name)(None, *args, ctypes.byref(off), None) < 0
    if kind == "cnn":                                          # batch 0, mode 0: nothing to do, nothing launched
        both(step_name, _set(batch=0), (dummy, dummy, dummy, 0), None)
        both(step_name, _set(batch=0), (None, dummy, dummy, 0), None)


def test_grad_norm_refusals_and_workspace():
    _lib, lib = _lib_or_fail()
    f = lib.aqg_optim_workspace_floats
    assert f(0) == 0 and f(1) == 1 and f(8192 - 3) == 1 and f(8192 - 2) == 2 and f(8192) == 2 and f(4760000) == 582
    top = 64 * 256 * 8192 - 3
    assert f(top) == 64 * 256 and f(top + 1) == 0
    gn = lib.aqg_grad_norm
    assert gn(None, 4, 4096, 4096, 1, None) < 0 and "null" in lib.aqg_last_error().decode()
    assert gn(4096, 4, None, 4096, 1, None) < 0 and gn(4096, 4, 4096, None, 1, None) < 0
    assert gn(4098, 4, 4096, 4096, 1, None) < 0 and "aligned" in lib.aqg_last_error().decode()
    assert gn(4096, 0, 4096, 4096, 1, None) < 0
    assert gn(4096, 8192, 4096, 4096, 1, None) < 0 and "workspace too small" in lib.aqg_last_error().decode()


# ---------------------------------------------------------------------------------------------- Python
def test_default_decay_mask():
    from alphaquoridorgnn_amd.pv_network_cnn import CNNNetwork
    from alphaquoridorgnn_amd.pv_network_gnn import GNNNetwork, GraphPolicyValueNetwork
    from alphaquoridorgnn_amd.train_network import default_decay_mask
    gnn = GNNNetwork()
    params = [p for _, p in gnn._ordered_params()]
    assert default_decay_mask(params) == [True, False] * 7                         # weight, bias of the 3 layers and 4 head layers
    net = GraphPolicyValueNetwork(6, 32, 2, 41, board_size=5)
    assert default_decay_mask([p for _, p in net._ordered_params()]) == [True, False] * 6
    cnn = CNNNetwork(8, 1, board_size=5)
    names = [k for k, _ in cnn.named_parameters()]
    mask = default_decay_mask(list(cnn.parameters()))
    assert mask == [True, False, False] * 3 + [True, False, True, False]           # conv kernel, BN weight, BN bias; the two heads
    for k, d in zip(names, mask):
        assert d == (k.endswith("weight") and "bn" not in k.lower().split(".")[-2]), k
    assert default_decay_mask(list(cnn.parameters()), decay_all=True) == [True] * len(names)


def test_train_cycle_options(monkeypatch):
    from alphaquoridorgnn_amd import train_cycle as tc, train_network as tn
    for k in ("TRAIN_WEIGHT_DECAY", "TRAIN_DECOUPLED", "TRAIN_MAX_GRAD_NORM"):
        monkeypatch.setattr(tn, k, getattr(tn, k))
    assert (tn.TRAIN_WEIGHT_DECAY, tn.TRAIN_DECOUPLED, tn.TRAIN_MAX_GRAD_NORM) == (0.0, True, None)
    tc._set_optimiser_options(tc._parser().parse_args([]))
    assert (tn.TRAIN_WEIGHT_DECAY, tn.TRAIN_DECOUPLED, tn.TRAIN_MAX_GRAD_NORM) == (0.0, True, None)
    tc._set_optimiser_options(tc._parser().parse_args(["--weight-decay", "1e-4", "--max-grad-norm", "2.5"]))
    assert (tn.TRAIN_WEIGHT_DECAY, tn.TRAIN_DECOUPLED, tn.TRAIN_MAX_GRAD_NORM) == (1e-4, True, 2.5)
    assert tn._configured_controls() == dict(weight_decay=1e-4, decoupled=True, max_grad_norm=2.5)
    tc._set_optimiser_options(tc._parser().parse_args(["--weight-decay", "1e-4", "--coupled-weight-decay"]))
    assert tn.TRAIN_DECOUPLED is False
    for bad in (["--coupled-weight-decay"], ["--weight-decay", "-1"], ["--weight-decay", "nan"], ["--max-grad-norm", "0"],
                ["--max-grad-norm", "inf"]):
        with pytest.raises(ValueError):
            tc._set_optimiser_options(tc._parser().parse_args(bad))
