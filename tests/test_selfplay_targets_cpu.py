"""Self-play targets without a GPU: the blend's numpy statement against an independent float64 statement, append_reference and a host
ReplayWindow with a blend, the .history row writer and gather_history with search values (two gloo ranks), the options of
self_play / train_cycle and their refusals, and the ABI -- three new exports, no new field in the engine struct."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests.test_replay_window_cpu import _A, _bits, counts_rows   # noqa: E402

SPECIAL = np.asarray([1.0, -1.0, 0.0, -0.0], dtype=np.float32)


def search_values(n, seed):
    """Random f32 in [-1, 1] with +1, -1, 0 and -0.0 in front (as many of them as fit)."""
    v = np.random.RandomState(seed).uniform(-1.0, 1.0, n).astype(np.float32)
    v[:min(n, 4)] = SPECIAL[:min(n, 4)]
    return v


# ------------------------------------------------------------------ 1. the numpy statements
@pytest.mark.parametrize("blend", [0.0, 0.25, 0.5, 1.0])
def test_blend_targets_against_float64(blend):
    """Where nothing is rounded twice: v a multiple of 2^-10 in [-1, 1] and a dyadic blend make keep * z, blend * v and their sum
    exact in float64 AND representable in float32, so the f32 statement must give exactly float32 of the float64 expression."""
    from alphaquoridorgnn_amd.replay import blend_targets
    rng = np.random.RandomState(1)
    z = rng.choice([-1, 0, 1], 4096).astype(np.int8)
    v = (rng.randint(-1024, 1025, 4096) / 1024.0).astype(np.float32)
    want64 = (1.0 - blend) * z.astype(np.float64) + blend * v.astype(np.float64)
    assert np.array_equal(want64.astype(np.float32).astype(np.float64), want64)          # no rounding anywhere
    got = blend_targets(z, v, blend)
    assert got.dtype == np.float32 and np.array_equal(got, want64.astype(np.float32))


def test_blend_targets_is_three_rounded_f32_operations():
    """A blend that is not dyadic: each product and the sum rounded to f32 on its own -- not the fused form, not the float64 one."""
    from alphaquoridorgnn_amd.replay import blend_targets
    b = np.float32(0.3)
    keep = np.float32(np.float32(1.0) - b)
    z = np.asarray([1, -1, 0, 1, -1], dtype=np.int8)
    v = np.asarray([0.1234567, 0.7654321, -0.3333333, -1.0, 1.0], dtype=np.float32)
    want = np.asarray([np.float32(np.float32(keep * np.float32(zz)) + np.float32(b * vv)) for zz, vv in zip(z, v)], dtype=np.float32)
    assert np.array_equal(_bits(blend_targets(z, v, 0.3)), _bits(want))
    assert np.array_equal(blend_targets(z, v, 0.0), z.astype(np.float32))                # blend 0: z
    assert np.array_equal(blend_targets(z, v, 1.0), v)                                   # blend 1: v
    for bad in (-0.01, 1.01, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="value_blend"):
            blend_targets(z, v, bad)
    with pytest.raises(ValueError, match="search_value"):
        blend_targets(z, v.astype(np.float64), 0.5)
    with pytest.raises(ValueError, match="search_value"):
        blend_targets(z, v[:3], 0.5)


@pytest.mark.parametrize("N", (3, 9))
def test_append_reference_with_a_blend(N):
    from alphaquoridorgnn_amd.replay import append_reference, blend_targets
    A, n, capacity, head = _A(N), 21, 30, 25
    S, V, Z = counts_rows(N, n, seed=N)
    q = search_values(n, seed=N)
    fill = lambda: (np.full((capacity, 72), 0xA5, np.uint8), np.full((capacity, A), -7.25, np.float32),    # noqa: E731
                    np.full((capacity,), -7.25, np.float32))
    plain, blended, zero = fill(), fill(), fill()
    append_reference(N, S, V, Z, None, None, head, *plain)
    append_reference(N, S, V, Z, None, None, head, *blended, search_value=q, value_blend=0.25)
    append_reference(N, S, V, Z, None, None, head, *zero, search_value=q, value_blend=0.0)
    slots = (head + np.arange(n)) % capacity
    rest = np.setdiff1d(np.arange(capacity), slots)
    assert np.array_equal(blended[0], plain[0]) and np.array_equal(_bits(blended[1]), _bits(plain[1]))
    assert np.array_equal(_bits(blended[2][slots]), _bits(blend_targets(Z, q, 0.25)))
    assert (blended[2][rest] == np.float32(-7.25)).all()
    assert not np.array_equal(blended[2], plain[2])
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(zero, plain))           # blend 0 is the plain append
    rings = fill()
    with pytest.raises(ValueError, match="value_blend"):
        append_reference(N, S, V, Z, None, None, head, *rings, search_value=q, value_blend=1.5)
    with pytest.raises(ValueError, match="value_blend"):
        append_reference(N, S, V, Z, None, None, head, *rings, search_value=q, value_blend=float("nan"))
    with pytest.raises(ValueError, match="search_value"):
        append_reference(N, S, V, Z, None, None, head, *rings, value_blend=0.5)          # a blend without values
    with pytest.raises(ValueError, match="search_value"):
        append_reference(N, S, V, Z, None, None, head, *rings, search_value=q[:-1], value_blend=0.5)
    with pytest.raises(ValueError, match="search_value"):
        append_reference(N, S, V, Z, None, None, head, *rings, search_value=q.astype(np.float64), value_blend=0.5)
    with pytest.raises(ValueError, match="counts form"):
        append_reference(N, S, None, None, plain[1][:n].copy(), Z.astype(np.float32), head, *rings, search_value=q, value_blend=0.5)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(rings, fill()))         # a refusal writes nothing


def test_host_window_with_a_blend():
    from alphaquoridorgnn_amd.replay import ReplayWindow, blend_targets
    N = 5
    w, plain = ReplayWindow(N, max_generations=2, capacity_rows=40), ReplayWindow(N, max_generations=2, capacity_rows=40)
    want = []
    for k, m in enumerate((17, 30, 11)):                    # the second append evicts nothing, the third wraps
        S, V, Z = counts_rows(N, m, seed=k)
        q = search_values(m, seed=10 + k)
        args = (torch.from_numpy(S), torch.from_numpy(V.view(np.int16)), torch.from_numpy(Z))
        w.append_counts(*args, search_value=torch.from_numpy(q), value_blend=0.5)
        plain.append_counts(*args)
        want.append(blend_targets(Z, q, 0.5))
        assert w.generations == plain.generations and torch.equal(w.index(), plain.index())
    held = np.concatenate(want[-len(w.generations):])
    assert np.array_equal(_bits(w.rows()[2].numpy()), _bits(held))
    assert torch.equal(w.rows()[0], plain.rows()[0]) and torch.equal(w.rows()[1], plain.rows()[1])
    S, V, Z = counts_rows(N, 5, seed=9)
    args = (torch.from_numpy(S), torch.from_numpy(V.view(np.int16)), torch.from_numpy(Z))
    before = [x.clone() for x in w.tensors()]
    for kw, word in ((dict(value_blend=0.5), "search_value"), (dict(search_value=torch.zeros(4), value_blend=0.5), "search_value"),
                     (dict(search_value=torch.zeros(5, dtype=torch.float64), value_blend=0.5), "search_value"),
                     (dict(search_value=torch.zeros(5), value_blend=-0.5), "value_blend"),
                     (dict(search_value=torch.zeros(5), value_blend=float("nan")), "value_blend")):
        with pytest.raises(ValueError, match=word):
            w.append_counts(*args, **kw)
    assert all(torch.equal(a, b) for a, b in zip(before, w.tensors())) and w.generations == plain.generations


# ------------------------------------------------------------------ 2. the file and the gather routes
def test_history_rows_with_values():
    """The .history writer: with values a row's z is the blended float32 target widened to a Python float -- so that the trainers'
    float32 conversion gives back the window's bits -- and without them the int it always was."""
    from alphaquoridorgnn_amd.replay import blend_targets
    from alphaquoridorgnn_amd.self_play import _history_rows
    N, n = 5, 12
    S, V, Z = counts_rows(N, n, seed=3)
    q = search_values(n, seed=4)
    t = (torch.from_numpy(S), torch.from_numpy(V.view(np.int16)), torch.from_numpy(Z))
    plain = _history_rows(*t, N)
    rows = _history_rows(*t, N, torch.from_numpy(q), 0.5)
    assert all(type(r[2]) is int for r in plain) and [r[2] for r in plain] == Z.tolist()
    assert all(type(r[2]) is float for r in rows)
    assert [r[:2] for r in rows] == [r[:2] for r in plain]
    back = torch.tensor(np.array([r[2] for r in rows]), dtype=torch.float32).numpy()     # the conversion of the trainers
    assert np.array_equal(_bits(back), _bits(blend_targets(Z, q, 0.5)))
    assert _history_rows(*t, N, None, 0.0) == plain


_GLOO_WORKER = r'''
import os, sys
sys.path.insert(0, os.environ["AQG_REPO"])
import numpy as np
import torch, torch.distributed as dist
from alphaquoridorgnn_amd.engine import gather_history
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:" + os.environ["AQG_PORT"], rank=int(os.environ["RANK"]), world_size=2)
r = dist.get_rank()
n = 5 if r == 0 else 3                      # ragged: ranks hold different numbers of positions


def shard(rank, n):
    st = torch.full((n, 72), 10 + rank, dtype=torch.uint8)
    vis = (torch.arange(n * 57).view(n, 57) % 199 + 1000 * rank).to(torch.int16)
    z = torch.tensor([(-1) ** i for i in range(n)], dtype=torch.int8) * (1 if rank == 0 else -1)
    q = torch.from_numpy(np.asarray([-0.0, 1.0, -1.0, 0.3, 1e-30][:n], dtype=np.float32)) * (1 if rank == 0 else -3)
    return st, vis, z, q


st, vis, z, q = shard(r, n)
want = [torch.cat([a, b]) for a, b in zip(shard(0, 5), shard(1, 3))]
got = gather_history(st, vis, z, values=q)
assert len(got) == 4 and got[3].dtype == torch.float32 and got[3].shape == (8,)
assert all(torch.equal(a, b) for a, b in zip(got[:3], want[:3]))
assert torch.equal(got[3].view(torch.int32), want[3].view(torch.int32))          # bit for bit, -0.0 and the tiny one included
three = gather_history(st, vis, z)                                               # the 3-tuple form, as it always was
assert len(three) == 3 and all(torch.equal(a, b) for a, b in zip(three, want[:3]))
got = gather_history(*(x[:0] if r == 1 else x for x in (st, vis, z)), values=q[:0] if r == 1 else q)      # an empty shard
assert got[3].shape == (5,) and torch.equal(got[3].view(torch.int32), shard(0, 5)[3].view(torch.int32))
dist.destroy_process_group()
print("ok", r)
'''


def test_gather_history_with_values_world_size_2_gloo(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(_GLOO_WORKER)
    port = str(31500 + os.getpid() % 2000)
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), AQG_REPO=REPO, AQG_PORT=port, MASTER_ADDR="127.0.0.1")
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = [p.communicate(timeout=120)[0].decode() for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o
        assert "ok" in o


def test_gather_history_without_a_group_returns_its_inputs():
    from alphaquoridorgnn_amd.engine import gather_history
    st, vis, z, q = torch.zeros((2, 72), dtype=torch.uint8), torch.zeros((2, 57), dtype=torch.int16), torch.zeros(2, dtype=torch.int8), torch.ones(2)
    got = gather_history(st, vis, z)
    assert len(got) == 3 and all(a is b for a, b in zip(got, (st, vis, z)))
    got = gather_history(st, vis, z, values=q)
    assert len(got) == 4 and all(a is b for a, b in zip(got, (st, vis, z, q)))


# ------------------------------------------------------------------ 3. options
def test_defaults_and_train_cycle_options():
    from alphaquoridorgnn_amd import self_play as sp, train_cycle as tc
    assert sp.SP_TEMPERATURE_PLIES == 0 and sp.SP_VALUE_BLEND == 0.0
    args = tc._parser().parse_args([])
    assert args.temperature_plies is None and args.value_blend is None
    tc._set_target_options(args)
    assert sp.SP_TEMPERATURE_PLIES == 0 and sp.SP_VALUE_BLEND == 0.0
    args = tc._parser().parse_args(["--temperature-plies", "12", "--value-blend", "0.5"])
    assert (args.temperature_plies, args.value_blend) == (12, 0.5)
    try:
        tc._set_target_options(args)
        assert sp.SP_TEMPERATURE_PLIES == 12 and sp.SP_VALUE_BLEND == 0.5
        for argv, word in ((["--temperature-plies", "-1"], "temperature_plies"), (["--value-blend", "1.5"], "value_blend"),
                           (["--value-blend", "-0.1"], "value_blend"), (["--value-blend", "nan"], "value_blend")):
            with pytest.raises(ValueError, match=word):
                tc._set_target_options(tc._parser().parse_args(argv))
            assert sp.SP_TEMPERATURE_PLIES == 12 and sp.SP_VALUE_BLEND == 0.5            # a refused option sets nothing
    finally:
        sp.SP_TEMPERATURE_PLIES, sp.SP_VALUE_BLEND = 0, 0.0
    with pytest.raises(SystemExit):
        tc._parser().parse_args(["--temperature-plies", "1.5"])


@pytest.mark.parametrize("kw,word", [(dict(temperature_plies=-1), "temperature_plies"), (dict(temperature_plies=1.5), "temperature_plies"),
                                     (dict(temperature_plies=True), "temperature_plies"),
                                     (dict(record_search_value=True, record_history=False), "record_history")])
def test_engine_refuses_bad_target_options(kw, word):
    """Before a GPU is asked for."""
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    with pytest.raises(ValueError, match=word):
        BatchedSelfPlay(None, num_games=2, sims=4, board_size=5, evaluator="fake", **kw)


@pytest.mark.parametrize("opt", [dict(temperature_plies=3), dict(record_search_value=True)])
def test_evaluation_paths_do_not_take_the_options(opt):
    from alphaquoridorgnn_amd import evaluate_agents, evaluate_network, pv_mcts
    with pytest.raises(TypeError):
        evaluate_network.BatchedMatch((0, 1), 2, sims=4, board_size=5, evaluator="fake", **opt)
    with pytest.raises(TypeError):
        evaluate_agents.BatchedAgentMatch(0, "random", 2, sims=4, board_size=5, evaluator="fake", **opt)
    with pytest.raises(TypeError):
        pv_mcts.pv_mcts_action(None, **opt)


# ------------------------------------------------------------------ 4. ABI
def test_abi_three_exports_and_no_new_field(tmp_path):
    from alphaquoridorgnn_amd import _lib
    header = open(os.path.join(REPO, "include", "aqgnn.h")).read()
    assert re.search(r"#define\s+AQG_ABI_VERSION\s+15\b", header) and _lib.ABI_VERSION == 15
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (("aqg_engine_move_targets", 5), ("aqg_engine_finish_move_targets", 5), ("aqg_replay_append_blend", 14)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name                     # declared
        assert hasattr(lib, name), name                                                    # exported
        res, args = _lib.SIGNATURES[name]                                                  # bound
        assert res is _lib._c.c_int and len(args) == nargs, name
    assert _lib.SIGNATURES["aqg_replay_append_blend"][1][6] is _lib._c.c_float
    assert _lib.SIGNATURES["aqg_engine_move_targets"][1][2] is _lib._c.c_int32
    # the struct is the one of the root-noise change: root_noise is its last field, and C and ctypes agree on its size
    src = tmp_path / "size.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "aqgnn.h"\n'
                   'int main() { std::printf("%zu %zu\\n", sizeof(aqg_engine), offsetof(aqg_engine, root_noise)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    size, last = (int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert ctypes.sizeof(_lib.EngineStructGeneral) == size and _lib.EngineStructGeneral.root_noise.offset == last
    assert last + 8 == size and _lib.EngineStructGeneral._fields_[-1][0] == "root_noise"
    for word in ("temperature_plies", "hist_value"):
        assert not hasattr(_lib.EngineStructGeneral, word)


def test_library_refuses_bad_target_arguments():
    """On the host, before anything is launched: a negative K, and a value buffer on an engine without a history.  (The engine is as
    incomplete as one can be without a GPU: the target checks run behind the engine's own, so it is made to pass those.)"""
    from alphaquoridorgnn_amd import _lib
    lib = _lib.load()
    e = _lib.EngineStructGeneral()
    e.board_size, e.num_games, e.quota, e.sims, e.node_cap, e.prior_mode = 5, 2, 2, 4, 1 + 4 * _lib.MAX_LEGAL, 1
    dummy = (ctypes.c_double * 8)()
    for name in ("slot_game", "game_done", "game_slot", "game_first_move"):
        setattr(e, name, ctypes.addressof(dummy))
    for fn in (lib.aqg_engine_move_targets, lib.aqg_engine_finish_move_targets):
        assert fn(ctypes.byref(e), ctypes.addressof(dummy), -1, None, None) != 0
        assert "temperature_plies" in lib.aqg_last_error().decode()
        assert fn(ctypes.byref(e), ctypes.addressof(dummy), 0, ctypes.addressof(dummy), None) != 0      # max_plies == 0
        assert "hist_value" in lib.aqg_last_error().decode()
        assert fn(ctypes.byref(e), None, 0, None, None) != 0 and "null" in lib.aqg_last_error().decode()
    for blend, word in ((-0.5, "blend"), (1.5, "blend"), (float("nan"), "blend")):
        assert lib.aqg_replay_append_blend(5, 57, None, None, None, None, blend, 0, 8, 0, None, None, None, None) != 0
        assert word in lib.aqg_last_error().decode()
    assert lib.aqg_replay_append_blend(5, 57, None, None, None, None, 0.5, 0, 8, 0, None, None, None, None) == 0      # n == 0
