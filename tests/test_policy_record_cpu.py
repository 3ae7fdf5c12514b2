"""Recording completed-Q targets during self-play, without a GPU (include/aqgnn.h "recording completed-Q targets during self-play"):
replay.append_reference(policy=) against the .history route bit for bit, its blend against replay.blend_targets, a host ReplayWindow's
append_policy beside append_counts, gather_history(policies=) over two gloo ranks, the option checks and train_cycle's parse refusals,
the ABI, and the host statement of a recorded row on the oracle's trees."""
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

from tests._improved_policy import pi_close   # noqa: E402
from tests._policy_record import policy_file_route, policy_size, recorded_rows, root_row, statement_rows   # noqa: E402
from tests.test_replay_window_cpu import _bits, counts_rows   # noqa: E402
from tests.test_selfplay_targets_cpu import search_values   # noqa: E402


def _fill(capacity, A):
    return (np.full((capacity, 72), 0xA5, np.uint8), np.full((capacity, A), -7.25, np.float32), np.full((capacity,), -7.25, np.float32))


# ------------------------------------------------------------------ 1. the numpy statement
@pytest.mark.parametrize("blend", [None, 0.25])
@pytest.mark.parametrize("N", (3, 5, 7, 9))
def test_append_reference_policy_equals_the_file_route(N, blend, tmp_path):
    from alphaquoridorgnn_amd.replay import append_reference
    n, A = 23, policy_size(N)
    S, V, Z = counts_rows(N, n, seed=N)
    P = recorded_rows(N, n, seed=40 + N)
    q = None if blend is None else search_values(n, seed=N)
    r72, rpi, rz = _fill(n, A)
    append_reference(N, S, None, Z, None, None, 0, r72, rpi, rz, search_value=q, value_blend=blend or 0.0, policy=P)
    s, p, v = policy_file_route(S, V, Z, P, N, tmp_path, q, blend or 0.0)
    assert p.dtype == np.float32 and np.array_equal(_bits(rpi), _bits(p)) and np.array_equal(_bits(rz), _bits(v))
    assert np.array_equal(_bits(rpi), _bits(P))                      # verbatim: the denormal and the -0.0 included
    assert _bits(P)[1, 1] == np.int32(-2 ** 31) and 0 < P[0, 0] < np.float32(1.2e-38)
    keep = np.ones(72, bool)
    keep[68:70] = False                                              # the ply counter: to_array() drops it
    assert np.array_equal(r72[:, keep], s[:, keep]) and np.array_equal(r72, S)


def test_append_reference_policy_blend_wrap_and_refusals():
    from alphaquoridorgnn_amd.replay import append_reference, blend_targets
    N, n, capacity, head = 5, 21, 30, 25
    A = policy_size(N)
    S, V, Z = counts_rows(N, n, seed=1)
    P, q = recorded_rows(N, n, seed=2), search_values(n, seed=3)
    plain, blended, zero, counts = _fill(capacity, A), _fill(capacity, A), _fill(capacity, A), _fill(capacity, A)
    append_reference(N, S, None, Z, None, None, head, *plain, policy=P)
    append_reference(N, S, None, Z, None, None, head, *blended, search_value=q, value_blend=0.25, policy=P)
    append_reference(N, S, None, Z, None, None, head, *zero, search_value=q, value_blend=0.0, policy=P)
    append_reference(N, S, V, Z, None, None, head, *counts, search_value=q, value_blend=0.25)
    slots = (head + np.arange(n)) % capacity
    rest = np.setdiff1d(np.arange(capacity), slots)
    assert np.array_equal(_bits(plain[1][slots]), _bits(P)) and np.array_equal(plain[2][slots], Z.astype(np.float32))
    assert np.array_equal(_bits(blended[2][slots]), _bits(blend_targets(Z, q, 0.25)))
    assert np.array_equal(_bits(blended[2]), _bits(counts[2])) and np.array_equal(blended[0], counts[0])      # z and records: the counts form's
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(zero, plain))                               # blend 0 is the plain append
    for ring in plain:
        assert (ring[rest] == ring.dtype.type(0xA5 if ring.dtype == np.uint8 else -7.25)).all()
    rings = _fill(capacity, A)
    bad = [(dict(policy=P, value_blend=0.5), "search_value"), (dict(policy=P, search_value=q, value_blend=1.5), "value_blend"),
           (dict(policy=P, search_value=q, value_blend=float("nan")), "value_blend"), (dict(policy=P[:-1]), "policy"),
           (dict(policy=P.astype(np.float64)), "policy"), (dict(policy=P[:, :-1]), "policy"),
           (dict(policy=P, search_value=q[:-1], value_blend=0.5), "search_value")]
    for kw, word in bad:
        with pytest.raises(ValueError, match=word):
            append_reference(N, S, None, Z, None, None, head, *rings, **kw)
    with pytest.raises(ValueError, match="policy goes with z_i8"):
        append_reference(N, S, V, Z, None, None, head, *rings, policy=P)
    with pytest.raises(ValueError, match="policy goes with z_i8"):
        append_reference(N, S, None, None, None, Z.astype(np.float32), head, *rings, policy=P)
    with pytest.raises(ValueError, match="counts form"):                                  # without policy= the old sentence
        append_reference(N, S, None, Z, P, None, head, *rings)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(rings, _fill(capacity, A)))      # a refusal writes nothing


# ------------------------------------------------------------------ 2. the host window
def test_host_window_append_policy_beside_append_counts():
    from alphaquoridorgnn_amd.replay import ReplayWindow, blend_targets
    N = 5
    w, c = ReplayWindow(N, max_generations=2, capacity_rows=40), ReplayWindow(N, max_generations=2, capacity_rows=40)
    held = []
    for k, m in enumerate((17, 30, 11, 45)):                 # nothing evicted, an eviction, a wrap, a generation larger than the ring
        S, V, Z = counts_rows(N, m, seed=k)
        P, q = recorded_rows(N, m, seed=20 + k), search_values(m, seed=10 + k)
        blend = dict(search_value=torch.from_numpy(q), value_blend=0.5) if k % 2 else {}
        w.append_policy(torch.from_numpy(S), torch.from_numpy(P), torch.from_numpy(Z), **blend)
        c.append_counts(torch.from_numpy(S), torch.from_numpy(V.view(np.int16)), torch.from_numpy(Z), **blend)
        assert w.generations == c.generations and torch.equal(w.index(), c.index()) and len(w) == len(c)
        assert torch.equal(w.tensors()[0], c.tensors()[0])
        assert torch.equal(w.tensors()[2].view(torch.int32), c.tensors()[2].view(torch.int32))
        held.append((P, blend_targets(Z, q, 0.5) if k % 2 else Z.astype(np.float32)))
    assert w.generations == [40]                             # the last generation alone, its newest 40 rows
    assert np.array_equal(_bits(w.rows()[1].numpy()), _bits(held[-1][0][-40:]))
    assert np.array_equal(_bits(w.rows()[2].numpy()), _bits(held[-1][1][-40:]))
    S, V, Z = counts_rows(N, 5, seed=9)
    P = recorded_rows(N, 5, seed=9)
    before = [x.clone() for x in w.tensors()]
    s, p, z = torch.from_numpy(S), torch.from_numpy(P), torch.from_numpy(Z)
    for args, kw, word in (((s, p, z), dict(value_blend=0.5), "search_value"), ((s, p, z), dict(search_value=torch.zeros(4), value_blend=0.5), "search_value"),
                           ((s, p, z), dict(search_value=torch.zeros(5), value_blend=-0.5), "value_blend"),
                           ((s, p.double(), z), {}, "policy"), ((s, p[:, :-1], z), {}, "policy"), ((s, p[:-1], z), {}, "policy"),
                           ((s, p, z.float()), {}, "z"), ((s, torch.from_numpy(V.view(np.int16)), z), {}, "policy")):
        with pytest.raises(ValueError, match=word):
            w.append_policy(*args, **kw)
    assert all(torch.equal(a, b) for a, b in zip(before, w.tensors())) and w.generations == [40]


# ------------------------------------------------------------------ 3. the file rows and the exchange
def test_history_rows_with_policy():
    from alphaquoridorgnn_amd.self_play import _history_rows
    N, n = 5, 12
    S, V, Z = counts_rows(N, n, seed=3)
    P = recorded_rows(N, n, seed=4)
    t = (torch.from_numpy(S), torch.from_numpy(V.view(np.int16)), torch.from_numpy(Z))
    plain = _history_rows(*t, N)
    rows = _history_rows(*t, N, policy=torch.from_numpy(P))
    assert [(r[0], r[2]) for r in rows] == [(r[0], r[2]) for r in plain] and all(type(r[2]) is int for r in rows)
    assert all(type(x) is float for r in rows for x in r[1]) and all(len(r[1]) == policy_size(N) for r in rows)
    assert np.array_equal(_bits(np.array([r[1] for r in rows]).astype(np.float32)), _bits(P))      # float32(float(x)) gives the bits back
    assert _history_rows(*t, N, None, 0.0, policy=None) == plain


_GLOO_WORKER = r'''
import os, sys
sys.path.insert(0, os.environ["AQG_REPO"])
import numpy as np
import torch, torch.distributed as dist
from alphaquoridorgnn_amd.engine import gather_history
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:" + os.environ["AQG_PORT"], rank=int(os.environ["RANK"]), world_size=2)
r = dist.get_rank()
n, A = (5 if r == 0 else 3), 57                  # ragged: the ranks hold different numbers of positions


def shard(rank, n):
    st = torch.full((n, 72), 10 + rank, dtype=torch.uint8)
    vis = (torch.arange(n * A).view(n, A) % 199 + 1000 * rank).to(torch.int16)
    z = torch.tensor([(-1) ** i for i in range(n)], dtype=torch.int8) * (1 if rank == 0 else -1)
    q = torch.from_numpy(np.asarray([-0.0, 1.0, -1.0, 0.3, 1e-30][:n], dtype=np.float32)) * (1 if rank == 0 else -3)
    pol = torch.from_numpy(np.random.RandomState(rank).randint(0, 2 ** 32, (n, A), dtype=np.uint64).astype(np.uint32).view(np.float32).copy())
    if n:
        pol[0, :3] = torch.tensor([-0.0, 1e-42, 1.0])
    return st, vis, z, q, pol


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


st, vis, z, q, pol = shard(r, n)
want = [torch.cat([a, b]) for a, b in zip(shard(0, 5), shard(1, 3))]
got = gather_history(st, vis, z, policies=pol)                                   # the policies alone: a fourth tensor
assert len(got) == 4 and got[3].dtype == torch.float32 and got[3].shape == (8, A)
assert all(same(a, b) for a, b in zip(got, want[:3] + [want[4]]))                # rank order, bit for bit (random bit patterns, NaNs included)
got = gather_history(st, vis, z, values=q, policies=pol)                         # with the values: the policies come last
assert len(got) == 5 and all(same(a, b) for a, b in zip(got, want))
three = gather_history(st, vis, z)                                               # without the argument: what it always was
assert len(three) == 3 and all(same(a, b) for a, b in zip(three, want[:3]))
four = gather_history(st, vis, z, values=q)
assert len(four) == 4 and all(same(a, b) for a, b in zip(four, want[:4]))
cut = lambda x: x[:0] if r == 1 else x                                           # rank 1 holds no row at all
got = gather_history(cut(st), cut(vis), cut(z), policies=cut(pol))
assert all(same(a, b) for a, b in zip(got, [x for i, x in enumerate(shard(0, 5)) if i != 3]))
dist.destroy_process_group()
print("ok", r)
'''


def test_gather_history_with_policies_world_size_2_gloo(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(_GLOO_WORKER)
    port = str(33500 + os.getpid() % 2000)
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
    st, vis, z = torch.zeros((2, 72), dtype=torch.uint8), torch.zeros((2, 57), dtype=torch.int16), torch.zeros(2, dtype=torch.int8)
    q, pol = torch.ones(2), torch.ones((2, 57))
    got = gather_history(st, vis, z, policies=pol)
    assert len(got) == 4 and all(a is b for a, b in zip(got, (st, vis, z, pol)))
    got = gather_history(st, vis, z, values=q, policies=pol)
    assert len(got) == 5 and all(a is b for a, b in zip(got, (st, vis, z, q, pol)))
    assert len(gather_history(st, vis, z)) == 3 and len(gather_history(st, vis, z, values=q)) == 4


# ------------------------------------------------------------------ 4. options, flags, ABI
def test_option_checks():
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay, MultiSetSelfPlay
    from alphaquoridorgnn_amd.selfplay_options import check_policy_record
    assert check_policy_record() == ("visits", 50.0, 1.0)
    assert check_policy_record("completed_q", 0, 0.5) == ("completed_q", 0.0, 0.5)
    assert check_policy_record("completed-q") == ("completed_q", 50.0, 1.0)          # as the command line spells it
    assert check_policy_record("visits", record_history=False) == ("visits", 50.0, 1.0)
    with pytest.raises(ValueError, match="record_history"):
        check_policy_record("completed_q", record_history=False)
    bad = (dict(policy_target="q"), dict(policy_target=None), dict(policy_c_visit=-1e-9), dict(policy_c_scale=-1.0),
           dict(policy_c_visit=float("nan")), dict(policy_c_scale=float("inf")), dict(policy_c_visit="50"), dict(policy_c_scale=None),
           dict(policy_c_visit=True))
    for kw in bad:
        with pytest.raises(ValueError):
            check_policy_record(**kw)
    # the constructors refuse before anything is allocated or a GPU is asked for: the same error on a machine without one
    for kw in bad + (dict(policy_target="completed_q", record_history=False),):
        with pytest.raises(ValueError, match="policy_target|c_visit|c_scale|record_history"):
            BatchedSelfPlay(None, num_games=2, sims=2, board_size=3, evaluator="fake", **kw)
        with pytest.raises(ValueError, match="policy_target|c_visit|c_scale|record_history"):
            MultiSetSelfPlay(None, num_games=2, sims=2, board_size=3, evaluator="fake", **kw)


def test_defaults_and_train_cycle_flags(monkeypatch):
    from alphaquoridorgnn_amd import self_play as sp, train_cycle as tc
    assert (sp.SP_POLICY_TARGET, sp.SP_POLICY_C_VISIT, sp.SP_POLICY_C_SCALE) == ("visits", 50.0, 1.0)
    for name in ("SP_POLICY_TARGET", "SP_POLICY_C_VISIT", "SP_POLICY_C_SCALE"):
        monkeypatch.setattr(sp, name, getattr(sp, name))        # restored after the test
    args = tc._parser().parse_args([])
    assert (args.policy_target, args.policy_c_visit, args.policy_c_scale) == (None, None, None) and tc._check_policy_args(args) is None
    tc._set_policy_options(args)
    assert (sp.SP_POLICY_TARGET, sp.SP_POLICY_C_VISIT, sp.SP_POLICY_C_SCALE) == ("visits", 50.0, 1.0)
    assert tc._check_policy_args(tc._parser().parse_args(["--policy-target", "visits"])) == ("visits", 50.0, 1.0)
    for flags in (["--policy-c-visit", "3"], ["--policy-c-scale", "0.5"], ["--policy-target", "visits", "--policy-c-visit", "3"],
                  ["--policy-target", "completed-q", "--policy-c-visit", "-1"], ["--policy-target", "completed-q", "--policy-c-scale", "nan"],
                  ["--policy-target", "completed-q", "--policy-c-visit", "inf"]):
        with pytest.raises(ValueError, match="--policy-"):
            tc._check_policy_args(tc._parser().parse_args(flags))
        with pytest.raises(ValueError, match="--policy-"):      # main() refuses at parse time, before a device or the process group
            tc.main(flags)
    with pytest.raises(SystemExit):
        tc._parser().parse_args(["--policy-target", "q"])
    tc._set_policy_options(tc._parser().parse_args(["--policy-target", "completed-q", "--policy-c-visit", "20", "--policy-c-scale", "0.5"]))
    assert (sp.SP_POLICY_TARGET, sp.SP_POLICY_C_VISIT, sp.SP_POLICY_C_SCALE) == ("completed_q", 20.0, 0.5)
    monkeypatch.setattr(sp, "SP_POLICY_C_SCALE", -1.0)
    with pytest.raises(ValueError, match="c_scale"):            # self_play() and play() check the switches before anything else
        sp.self_play(model=object(), games=1)
    with pytest.raises(ValueError, match="c_scale"):
        sp.play(object())


def test_abi_binding_and_build_list(tmp_path):
    from alphaquoridorgnn_amd import _lib
    header = open(os.path.join(REPO, "include", "aqgnn.h")).read()
    assert re.search(r"#define\s+AQG_ABI_VERSION\s+15\b", header) and _lib.ABI_VERSION == 15
    for name in ("aqg_engine_move_policy", "aqg_engine_finish_move_policy", "aqg_engine_record_improved_policy", "aqg_replay_append_policy"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header) and name in _lib.SIGNATURES
    assert _lib.SIGNATURES["aqg_engine_move_policy"][1][:6] == _lib.SIGNATURES["aqg_engine_move_resign"][1][:6]
    assert _lib.SIGNATURES["aqg_engine_finish_move_policy"][1] == _lib.SIGNATURES["aqg_engine_move_policy"][1]
    assert _lib.SIGNATURES["aqg_replay_append_policy"][1] == _lib.SIGNATURES["aqg_replay_append_blend"][1]
    assert not hasattr(_lib.EngineStructGeneral, "hist_policy")          # the option is a struct beside the engine's, not a field of it
    src = tmp_path / "size.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "aqgnn.h"\n'
                   'int main() { std::printf("%zu %zu %zu %zu %zu\\n", sizeof(aqg_policy_record), offsetof(aqg_policy_record, c_visit), '
                   'offsetof(aqg_policy_record, c_scale), offsetof(aqg_policy_record, hist_policy), sizeof(aqg_engine)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    size, a, b, c, engine = (int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    P = _lib.PolicyRecordStruct
    assert (ctypes.sizeof(P), P.c_visit.offset, P.c_scale.offset, P.hist_policy.offset) == (size, a, b, c) == (24, 0, 8, 16)
    assert ctypes.sizeof(_lib.EngineStructGeneral) == engine
    build = open(os.path.join(REPO, "alphaquoridorgnn_amd", "csrc", "build.sh")).read()
    assert re.search(r"\bmcts_record\b", build)
    csrc = os.path.join(REPO, "alphaquoridorgnn_amd", "csrc")
    code = {f: re.sub(r"//[^\n]*", "", open(os.path.join(csrc, f)).read()) for f in ("mcts_improve.hip", "mcts_record.hip", "mcts_improve_row.hpp")}
    # the arithmetic exists once, in the header both units include; it is never built with contraction or fast-math
    assert "exp(" in code["mcts_improve_row.hpp"] and "log(" in code["mcts_improve_row.hpp"]
    assert "#pragma clang fp contract(off)" in code["mcts_improve_row.hpp"] and "__FAST_MATH__" in code["mcts_improve_row.hpp"]
    for unit in ("mcts_improve.hip", "mcts_record.hip"):
        assert '#include "mcts_improve_row.hpp"' in code[unit] and "improved_policy_row(" in code[unit]
        assert "exp(" not in code[unit] and "log(" not in code[unit]
    assert "__syncthreads" not in code["mcts_record.hip"] and "atomic" not in code["mcts_record.hip"]      # wave-scope fences only


# ------------------------------------------------------------------ 5. the host statement
def test_host_statement_on_a_3x3_game():
    """One 3x3 game of the oracle's self-play, 8 simulations per move: every row of the statement sums to 1 within A ulps (A roundings of at
    most half an ulp of an entry <= 1 each), is 0 on every illegal action, and with c_scale = 0 -- sigma = 0 -- is the root's priors
    scattered (softmax(log p) is p / sum p, and the priors sum to 1 up to their own f32 rounding: held to one f32 ulp of that
    quotient, tests/_improved_policy.pi_close, and above 0 exactly where p is)."""
    from oracle import mcts as om, quoridor as oq
    N, sims, bias = 3, 8, 2
    A = policy_size(N)
    u = np.random.RandomState(5).random_sample(64)
    state, recs, actions = oq.State(N=N), [], []
    while not state.is_done():                               # oracle.mcts.play's loop, keeping the records and the moves
        visits = [c.n for c in om.search(om.FakeModel(bias), state, sims).children]
        legal = list(state.legal_actions())
        recs.append(np.asarray(state.rec, dtype=np.uint8).copy())
        actions.append(legal[om.choice_index(om.boltzman(visits, 1.0), u[len(recs) - 1])])
        state = state.next(actions[-1])
    history = recs
    recs, actions = np.stack(recs), np.asarray(actions, dtype=np.uint8)
    assert len(history) >= 2                                 # (a 3x3 game is over in a few plies)
    rows = statement_rows(N, sims, bias, recs, actions)
    priors = statement_rows(N, sims, bias, recs, actions, c_scale=0.0)
    assert rows.dtype == np.float32 and rows.shape == (len(history), A)
    for ply in range(len(history)):
        st = oq.State(recs[ply])
        legal = np.zeros(A, dtype=bool)
        legal[list(st.legal_actions())] = True
        assert abs(float(rows[ply].astype(np.float64).sum()) - 1.0) <= A * 2.0 ** -23
        assert (rows[ply][~legal] == 0).all() and (rows[ply][legal] > 0).all()
        root = om.search(om.FakeModel(bias), st, sims)
        assert np.array_equal(_bits(rows[ply]), _bits(root_row(root, N)))
        p = np.zeros(A, dtype=np.float32)
        p[list(st.legal_actions())] = [np.float32(c.p) for c in root.children]
        assert pi_close(priors[ply], p.astype(np.float64) / p.astype(np.float64).sum())     # softmax(log p) IS p / sum p
        assert np.array_equal(priors[ply] > 0, p > 0)
        assert not np.array_equal(rows[ply], priors[ply])           # ... and the values do move the target
    kept = statement_rows(N, sims, bias, recs, actions, keep_visits=sims)      # a kept root has more visits: other rows behind ply 0
    assert np.array_equal(kept[0], rows[0]) and not np.array_equal(kept[1:], rows[1:])
