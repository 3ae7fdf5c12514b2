"""CPU tests of the strength-tracking workload (evaluate_agents.py): the reference's call surface, the threaded alpha-beta batch
against the reference-pinned goldens, the counter-based generator's numpy mirror, the host match loops, and the train_cycle flag.
The kernels behind the random / rollout agents are tested on the GPU (tests/test_agent_match.py)."""
import numpy as np
import pytest

from tests import _util as U


def test_evaluate_agents_exposes_the_reference_surface():
    from alphaquoridorgnn_amd import evaluate_agents as ea
    from alphaquoridorgnn_amd.dropin import evaluate_agents as d
    for mod in (ea, d):
        for name in ("EP_GAME_COUNT", "first_player_point", "play", "evaluate_algorithm_of", "evaluate_best_player"):
            assert hasattr(mod, name), name
        assert mod.EP_GAME_COUNT == 10
    assert d.play is ea.play and d.evaluate_best_player is ea.evaluate_best_player


@pytest.mark.parametrize("N", [3, 5, 9])
@pytest.mark.parametrize("threads", [1, 4])
def test_alpha_beta_batch_equals_goldens(N, threads):
    """Every state of agents_NxN.npz, depth 2 and depth 1, in input order."""
    from alphaquoridorgnn_amd import agents
    g = U.golden(f"agents_{N}x{N}.npz")
    for depth, key in ((2, "ab2"), (1, "ab1")):
        got = agents.alpha_beta_action_batch(g["states"], max_depth=depth, threads=threads)
        assert got.dtype == np.int32 and np.array_equal(got, g[key].astype(np.int32)), (N, depth, threads)
    one = agents.alpha_beta_action_batch([g["states"][3]], max_depth=2, threads=threads)
    assert int(one[0]) == int(g["ab2"][3])


def test_default_pool_is_at_most_16_threads():
    from alphaquoridorgnn_amd import agents
    assert 1 <= agents.default_threads() <= 16


def _mix(z):
    M = (1 << 64) - 1
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    return z ^ (z >> 31)


def _f(seed, b, i):
    """The generator as include/aqgnn.h states it, in Python integers."""
    M, G = (1 << 64) - 1, 0x9E3779B97F4A7C15
    key = _mix((seed + G * (b + 1)) & M)
    return (_mix((key + G * (i + 1)) & M) >> 11) * 2.0 ** -53


def test_draw_uniforms_is_the_documented_generator():
    from alphaquoridorgnn_amd import agents
    known = {(0, 0): ['0x1.4e0dba5e9a32fp-1', '0x1.6705460be8829p-1', '0x1.8c6a4553eeafcp-2'],
             (1, 2): ['0x1.4d8e311c0aa22p-1', '0x1.b5405a1e65cd8p-2', '0x1.54fd0892c3e92p-1'],
             (12345, 37): ['0x1.bd428228de314p-2', '0x1.b843834cd0d1cp-1', '0x1.7815bc128bea0p-6'],
             (2 ** 63 + 5, 1000): ['0x1.1f19927f1fb38p-1', '0x1.0844f5c0d3239p-1', '0x1.a85735a7c5a2cp-1']}
    for (seed, b), want in known.items():
        u = agents.draw_uniforms(seed, b, 3)
        assert u.dtype == np.float64 and [float(x).hex() for x in u] == want
    for seed, b in ((7, 0), (7, 63), (2 ** 64 - 1, 5)):
        u = agents.draw_uniforms(seed, b, 4096)
        assert u.shape == (4096,) and (u >= 0).all() and (u < 1).all()
        assert [float(x) for x in u[:50]] == [_f(seed, b, i) for i in range(50)]
        assert np.array_equal(u[:100], agents.draw_uniforms(seed, b, 100))          # a pure function of (seed, b, i)
        assert 0.45 < u.mean() < 0.55
    a = agents.draw_uniforms(7, 0, 64)
    assert not np.array_equal(a, agents.draw_uniforms(7, 1, 64)) and not np.array_equal(a, agents.draw_uniforms(8, 0, 64))
    assert agents.draw_uniforms(3, 3, 0).shape == (0,)


def test_explore_table_is_the_reference_expression():
    import math
    from alphaquoridorgnn_amd import agents
    t = agents.explore_table(40)
    assert t.shape == (41, 41) and t.dtype == np.float64
    for tt in range(1, 41):
        for n in range(1, tt + 1):
            assert t[tt, n] == 2 * (2 * math.log(tt) / n) ** 0.5


@pytest.mark.parametrize("N", [3, 5])
def test_host_play_points_and_colours(N, capsys):
    """play() / evaluate_algorithm_of() with two host agents: points in {0, 0.5, 1}, and the first agent moves first in the even
    games only."""
    import random
    from alphaquoridorgnn_amd import agents, evaluate_agents as ea
    random.seed(5)
    seen = []

    def a0(state):
        seen.append((0, state.is_first_player()))
        return agents.random_action(state)

    def a1(state):
        seen.append((1, state.is_first_player()))
        return agents.alpha_beta_action(state, 1)

    p = ea.play((a0, a1), board_size=N)
    assert p in (0, 0.5, 1)
    assert all(first == (who == 0) for who, first in seen)
    games = []
    plain_play = ea.play

    def recording_play(next_actions, board_size=None):
        del seen[:]
        out = plain_play(next_actions, board_size)
        games.append((seen[0], out))
        return out
    ea.play = recording_play
    try:
        avg = ea.evaluate_algorithm_of("VS_Test", (a0, a1), games=4, board_size=N)
    finally:
        ea.play = plain_play
    assert [g[0] for g in games] == [(0, True), (1, True), (0, True), (1, True)]      # who makes the first move of game i
    assert all(g[1] in (0, 0.5, 1) for g in games)
    want = sum(pt if i % 2 == 0 else 1 - pt for i, (_, pt) in enumerate(games)) / 4
    assert avg == want and 0 <= avg <= 1
    assert "VS_Test" in capsys.readouterr().out


def test_train_cycle_baseline_games_flag():
    from alphaquoridorgnn_amd import train_cycle
    ap = train_cycle._parser()
    assert ap.parse_args([]).baseline_games == 0
    assert ap.parse_args(["--baseline-games", "6"]).baseline_games == 6
    assert "--baseline-games" in ap.format_help()
    with pytest.raises(SystemExit):
        train_cycle.main(["--help"])
    assert [t for t, _ in train_cycle._STAGES] == ["self-play", "parameter update", "evaluation of the new parameters"]
