"""CPU tests around the batched alpha-beta agent: the native host search against the reference's recordings on positions with
walls in hand (tests/golden/ab_walls_*.npz, tools/gen_golden_alpha_beta.py), and the parts of the device path that need no GPU
-- the binding, the workspace size, the `backend` argument."""

import numpy as np
import pytest

from tests import _util as U

FILES = ["ab_walls_5x5.npz", "ab_walls_9x9.npz"]


@pytest.mark.parametrize("name", FILES)
def test_recordings_hold_what_they_promise(name):
    g = U.golden(name)
    states = g["states"]
    assert ((states[:, 1] > 0) | (states[:, 3] > 0)).all()                    # a wall in hand in every state
    assert np.array_equal(g["both_walls"], (states[:, 1] > 0) & (states[:, 3] > 0))
    assert int(g["ab2_count"][0]) == len(g["ab2_index"]) == len(g["ab2"])
    if name == "ab_walls_5x5.npz":
        assert len(states) == 24 and len(g["ab2"]) == 24
        assert g["both_walls"].sum() >= 8 and g["adjacent"].sum() >= 4 and (g["adjacent"] & g["diagonal"]).sum() >= 1
    else:
        deep = g["ab2_index"]
        assert len(states) - len(deep) == 12 and len(deep) >= 4
        assert (states[deep, 1] <= 3).all() and (states[deep, 3] <= 3).all()


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("name", FILES)
def test_host_search_equals_recordings(name, threads):
    from alphaquoridorgnn_amd import agents
    g = U.golden(name)
    states = g["states"]
    assert np.array_equal(agents.alpha_beta_action_batch(states, max_depth=1, threads=threads), g["ab1"].astype(np.int32))
    deep = g["ab2_index"]
    assert np.array_equal(agents.alpha_beta_action_batch(states[deep], max_depth=2, threads=threads), g["ab2"].astype(np.int32))


@pytest.mark.parametrize("name", FILES)
def test_host_heuristic_and_paths_equal_recordings(name):
    from alphaquoridorgnn_amd import agents
    g = U.golden(name)
    for i, rec in enumerate(g["states"]):
        assert agents.heuristic_eval(rec) == float(g["heuristic"][i]), i
        assert agents.shortest_path(rec) == int(g["paths"][i, 0]), i
        assert float(g["heuristic"][i]) == (int(g["paths"][i, 1]) - int(g["paths"][i, 0])) / int(g["max_dist"][0])


def test_lib_binds_the_new_symbols():
    from alphaquoridorgnn_amd import _lib
    lib = _lib.load()
    for name in ("aqg_agent_shortest_paths", "aqg_agent_alpha_beta_workspace_bytes", "aqg_agent_alpha_beta"):
        assert name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]


def test_abi_stays_15():
    from alphaquoridorgnn_amd import _lib
    assert _lib.ABI_VERSION == 15 and _lib.load().aqg_abi_version() == 15


def test_workspace_bytes():
    from alphaquoridorgnn_amd import _lib, agents
    f = _lib.load().aqg_agent_alpha_beta_workspace_bytes
    for N in (3, 5, 7, 9):
        for depth in range(agents.AB_MAX_DEPTH + 1):
            assert f(N, 1, depth) > 0
            assert f(N, 70, depth) >= 70 * f(N, 1, depth) // 2
    assert f(4, 8, 2) == 0 and f(11, 8, 2) == 0 and f(0, 8, 2) == 0           # board_size
    assert f(9, 0, 2) == 0 and f(9, -3, 2) == 0                               # B
    assert f(9, 8, -1) == 0 and f(9, 8, agents.AB_MAX_DEPTH + 1) == 0         # depth


def test_backend_argument():
    from alphaquoridorgnn_amd import agents
    states = U.golden("ab_walls_5x5.npz")["states"][:6]
    plain = agents.alpha_beta_action_batch(states, max_depth=2)
    assert np.array_equal(agents.alpha_beta_action_batch(states, max_depth=2, backend="host"), plain)
    assert np.array_equal(agents.alpha_beta_action_batch(states, max_depth=2, threads=2, backend="host"), plain)
    with pytest.raises(ValueError, match="backend"):
        agents.alpha_beta_action_batch(states, backend="cuda")
    with pytest.raises(ValueError, match="max_depth"):
        agents.alpha_beta_action_batch(states, max_depth=agents.AB_MAX_DEPTH + 1, backend="hip")
    assert isinstance(agents.ALPHA_BETA_DEVICE_MIN_STATES, int) and agents.ALPHA_BETA_DEVICE_MIN_STATES >= 1


def test_match_rejects_an_unknown_backend():
    from alphaquoridorgnn_amd.evaluate_agents import BatchedAgentMatch
    with pytest.raises(ValueError, match="backend"):
        BatchedAgentMatch(7, "alpha_beta", 0, sims=4, board_size=5, evaluator="fake", agent_kwargs={"backend": "gpu"})
