"""CPU tests (no GPU) of the root exploration noise: the numpy mirror of the device's gamma generator (engine.draw_root_noise) and its
moments against the analytic Dirichlet, the C ABI's four appended fields, the option checks -- and the pure-numpy statement of the
mix that tests/test_root_noise.py holds the kernel to."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import _util as U

REPO = U.REPO
MAX_LEGAL = 136


# ------------------------------------------------------------------ the mix, stated in numpy (imported by the GPU tests)
def wave_sum_f32(vals):
    """The f32 sum as a 64-lane wavefront forms it (csrc/mcts_tree.hpp wave_sum_f behind the lanes' own partial sums): lane l adds its
    entries l, l + 64, l + 128 in that order, then the xor butterfly from distance 32 down to 1."""
    v = np.zeros(192, dtype=np.float32)
    v[:len(vals)] = np.asarray(vals, dtype=np.float32)
    lane = np.float32(0.0) + v[:64]
    lane = (lane + v[64:128]).astype(np.float32)
    lane = (lane + v[128:192]).astype(np.float32)
    idx = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        lane = (lane + lane[idx ^ off]).astype(np.float32)
    return np.float32(lane[0])


def gather_priors(dense_row, legal):
    """The root's priors of a network evaluator: the dense row at the legal actions, divided by the sum unless it is 0."""
    p = np.asarray(dense_row, dtype=np.float32)[np.asarray(legal, dtype=np.int64)]
    s = wave_sum_f32(p)
    return (p / (s if s != 0 else np.float32(1.0))).astype(np.float32)


def noise_eta(gammas):
    """eta_i = f32(g_i / S), S the float64 sum; an entry that is not > 0 and finite counts as 0.  None: no usable noise."""
    g = np.asarray(gammas, dtype=np.float64)
    g = np.where((g > 0) & np.isfinite(g), g, 0.0)
    S = g.sum()
    if not (S > 0 and np.isfinite(S)):
        return None
    return (g / S).astype(np.float32)


def mix_statement(priors, gammas, eps):
    """p'_i = (1 - eps) p_i + eps eta_i in f32: one subtraction, two products, one sum, each rounded.  `priors`: f32 over the legal
    actions in order (gather_priors for a dense row); `gammas`: the float64 variates g_0 .. g_{cnt-1}."""
    p = np.asarray(priors, dtype=np.float32)
    eta = noise_eta(np.asarray(gammas)[:len(p)])
    if eta is None or len(p) == 0:
        return p.copy()
    eps = np.float32(eps)
    keep = np.float32(np.float32(1.0) - eps)
    x = (keep * p).astype(np.float32)
    y = (eps * eta).astype(np.float32)
    return (x + y).astype(np.float32)


def test_mix_statement_edges():
    p = np.asarray([0.5, 0.25, 0.25], dtype=np.float32)
    assert np.array_equal(mix_statement(p, [0.0, 0.0, 0.0], 0.25), p)                  # no usable noise: untouched
    assert np.array_equal(mix_statement(p, [np.nan, -1.0, np.inf], 0.25), p)
    one = mix_statement(np.ones(1, np.float32), [7.0], 0.25)                             # cnt = 1: (1 - eps) 1 + eps 1
    assert one[0] == np.float32(np.float32(0.75) * np.float32(1.0) + np.float32(0.25) * np.float32(1.0))
    got = mix_statement(p, [1.0, 2.0, 1.0], 0.5)
    assert np.array_equal(got, np.asarray([0.375, 0.375, 0.25], dtype=np.float32))
    assert mix_statement(p, [1.0, np.nan, 1.0], 0.5)[1] == np.float32(0.125)              # a bad entry gets no noise mass
    dense = np.zeros(57, dtype=np.float32)
    dense[[3, 9, 40]] = [0.2, 0.2, 0.4]
    g = gather_priors(dense, [3, 9, 40])
    assert np.array_equal(g, (np.asarray([0.2, 0.2, 0.4], np.float32) / wave_sum_f32([0.2, 0.2, 0.4])).astype(np.float32))
    assert np.array_equal(gather_priors(np.zeros(57, np.float32), [1, 2]), np.zeros(2, np.float32))     # sum 0: not divided


# ------------------------------------------------------------------ the generator's mirror
def test_draw_root_noise_deterministic_positive_and_prefix_stable():
    from alphaquoridorgnn_amd.engine import draw_root_noise
    for alpha in (0.03, 0.3, 1.0, 3.0):
        a = draw_root_noise(12345, 7, 3, 131, alpha)
        assert a.shape == (131,) and a.dtype == np.float64
        assert np.array_equal(a, draw_root_noise(12345, 7, 3, 131, alpha))
        assert np.isfinite(a).all() and (a > 0).all()
        for c in (1, 5, 35):           # component i has its own sub-stream: the first c components do not depend on count
            assert np.array_equal(draw_root_noise(12345, 7, 3, c, alpha), a[:c])
        # the stream is keyed by (seed, game, ply): each of the three changes it
        for other in ((12346, 7, 3), (12345, 8, 3), (12345, 7, 4)):
            assert not np.array_equal(draw_root_noise(*other, 131, alpha), a)
        many = draw_root_noise(12345, np.arange(5, 9), 3, 131, alpha)           # a batch of games is the same function
        assert many.shape == (4, 131) and np.array_equal(many[2], a)
    tiny = draw_root_noise(1, np.arange(4000), 0, 131, 0.03)                     # u ** (1 / 0.03) underflows now and then: never 0
    assert (tiny > 0).all() and np.isfinite(tiny).all()


def _beta_raw_moments(a, b):
    """E[x^r], r = 1..4, of Beta(a, b)."""
    out, m = [], 1.0
    for r in range(4):
        m *= (a + r) / (a + b + r)
        out.append(m)
    return out


@pytest.mark.parametrize("alpha", [0.03, 0.3, 1.0, 3.0])
@pytest.mark.parametrize("count", [1, 5, 35, 131])
def test_draw_root_noise_moments_match_dirichlet(alpha, count):
    """eta = g / sum(g) over 20,000 streams against Dir(alpha): every component's mean against 1/n and variance against
    (1/n)(1 - 1/n) / (n alpha + 1), each within 6 standard errors of its estimator.  The standard errors come from the analytic
    moments of the marginal Beta(alpha, (n - 1) alpha): Var(mean) = s2 / M, Var(sample variance) = (mu4 - s2^2 (M - 3) / (M - 1)) / M."""
    from alphaquoridorgnn_amd.engine import draw_root_noise
    M, n = 20000, count
    g, exhausted = draw_root_noise(20261017, np.arange(M), 2, n, alpha, return_exhausted=True)
    assert exhausted == 0
    assert g.shape == (M, n) and (g > 0).all() and np.isfinite(g).all()
    eta = g / g.sum(axis=1, keepdims=True)
    mean, var = eta.mean(axis=0), eta.var(axis=0, ddof=1)
    a32 = float(np.float32(alpha))
    want_mean = 1.0 / n
    want_var = want_mean * (1.0 - want_mean) / (n * a32 + 1.0)
    if n == 1:
        assert np.array_equal(eta, np.ones((M, 1))) and want_var == 0.0
        return
    m1, m2, m3, m4 = _beta_raw_moments(a32, (n - 1) * a32)
    s2 = m2 - m1 * m1
    mu4 = m4 - 4 * m1 * m3 + 6 * m1 * m1 * m2 - 3 * m1 ** 4
    assert abs(m1 - want_mean) < 1e-15 and abs(s2 - want_var) < 1e-12 * want_var + 1e-18
    se_mean = np.sqrt(s2 / M)
    se_var = np.sqrt((mu4 - s2 * s2 * (M - 3) / (M - 1)) / M)
    dm, dv = np.abs(mean - want_mean).max(), np.abs(var - want_var).max()
    print(f"alpha {alpha} n {n}: mean off by {dm / se_mean:.2f} SE, variance off by {dv / se_var:.2f} SE (worst component)")
    assert dm <= 6 * se_mean
    assert dv <= 6 * se_var


def _stream_keys(noise_seed, games, plies):
    from alphaquoridorgnn_amd.engine import root_noise_stream_key
    return {root_noise_stream_key(noise_seed, k, ply) for k in range(games) for ply in range(plies)}


def test_stream_key_is_the_generators():
    """root_noise_stream_key is the key draw_root_noise draws under, in the agents' keying K(s, b) = mix(s + G (b + 1)) -- so a game
    index is a shift of the seed by G, which is why a default noise seed must not be linear in the engine's seed."""
    from alphaquoridorgnn_amd.agents import draw_uniforms
    from alphaquoridorgnn_amd.engine import _mix64_int, _GOLDEN, draw_root_noise, root_noise_stream_key
    assert draw_uniforms(99, 4, 1)[0] == (_mix64_int(_mix64_int(99 + _GOLDEN * 5) + _GOLDEN) >> 11) * 2.0 ** -53
    assert root_noise_stream_key(99, 4, 7) == _mix64_int(_mix64_int(99 + _GOLDEN * 5) + _GOLDEN * 8)
    assert root_noise_stream_key(99 + _GOLDEN, 4, 7) == root_noise_stream_key(99, 5, 7)
    assert np.array_equal(draw_root_noise(99 + _GOLDEN, 4, 7, 35, 0.3), draw_root_noise(99, 5, 7, 35, 0.3))
    assert not np.array_equal(draw_root_noise(100, 4, 7, 35, 0.3), draw_root_noise(99, 5, 7, 35, 0.3))


@pytest.mark.parametrize("seed", [0, 7, 2 ** 31 - 3])
def test_engines_with_consecutive_seeds_share_no_stream(seed):
    """self_play() gives rank r the engine seed base + r: the default noise seeds of consecutive engine seeds must not put any
    (game, ply) of one engine on a stream of the next -- for single engines and for MultiSetSelfPlay's sets alike."""
    from alphaquoridorgnn_amd.engine import default_root_noise_seed, set_noise_seeds
    quota, plies = 300, 116
    a = _stream_keys(default_root_noise_seed(seed), quota, plies)
    b = _stream_keys(default_root_noise_seed(seed + 1), quota, plies)
    assert len(a) == len(b) == quota * plies and not (a & b)
    sizes, quotas = [8, 8, 7, 7], [75, 75, 75, 75]
    per_engine = []
    for s in (seed, seed + 1):
        seeds = set_noise_seeds(s, None, sizes, quotas)
        assert len(set(seeds)) == 4
        keys = [_stream_keys(ns, q, plies) for ns, q in zip(seeds, quotas)]
        union = set().union(*keys)
        assert len(union) == sum(quotas) * plies                 # no two games of one engine share a stream
        per_engine.append(union)
    assert not (per_engine[0] & per_engine[1])                   # ... nor do games of the two engines
    # the sets' games are numbered through: set i's game k is game first_i + k under the base seed
    seeds = set_noise_seeds(seed, 1234, sizes, quotas)
    assert _stream_keys(seeds[2], 75, 2) == {k2 for k2 in _stream_keys(1234, 225, 2)} - _stream_keys(1234, 150, 2)


# ------------------------------------------------------------------ C ABI
def test_root_noise_fields_sit_behind_cnn_net(tmp_path):
    from alphaquoridorgnn_amd import _lib
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "aqgnn.h"\n'
                   "int main() { std::printf(\"%zu %zu %zu %zu %zu %zu %zu %d\\n\", sizeof(aqg_engine), offsetof(aqg_engine, cnn_net),"
                   " sizeof(aqg_cnn_net), offsetof(aqg_engine, root_noise_eps), offsetof(aqg_engine, root_noise_alpha),"
                   " offsetof(aqg_engine, root_noise_seed), offsetof(aqg_engine, root_noise), AQG_ABI_VERSION); }\n")
    exe = tmp_path / "layout"
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    E = _lib.EngineStructGeneral
    assert got == [ctypes.sizeof(E), E.cnn_net.offset, ctypes.sizeof(_lib.CnnNetStruct), E.root_noise_eps.offset,
                   E.root_noise_alpha.offset, E.root_noise_seed.offset, E.root_noise.offset, 15]
    end = E.cnn_net.offset + ctypes.sizeof(_lib.CnnNetStruct)
    assert [E.root_noise_eps.offset, E.root_noise_alpha.offset, E.root_noise_seed.offset, E.root_noise.offset] == \
        [end, end + 4, end + 8, end + 16]                       # appended without padding: the struct's bytes are the graph key
    assert ctypes.sizeof(E) == end + 24
    z = E()
    assert (z.root_noise_eps, z.root_noise_alpha, z.root_noise_seed, z.root_noise) == (0.0, 0.0, 0, None)      # zero = off


def _engine_struct(eps, alpha):
    """An engine struct that passes every host-side check but the noise options' (dummy pointers: nothing is launched)."""
    from alphaquoridorgnn_amd import _lib
    e = _lib.EngineStructGeneral()
    e.board_size, e.num_games, e.quota, e.sims, e.node_cap, e.prior_mode = 5, 4, 4, 8, 1 + 8 * 136, 1
    for name in ("slot_game", "game_done", "game_slot", "game_first_move"):
        setattr(e, name, 0x1000)
    e.root_noise_eps, e.root_noise_alpha = eps, alpha
    return e


@pytest.mark.parametrize("eps,alpha,word", [(-0.1, 0.3, "eps"), (1.0, 0.3, "eps"), (1.5, 0.3, "eps"), (float("nan"), 0.3, "eps"),
                                            (0.25, 0.0, "alpha"), (0.25, -1.0, "alpha"), (0.25, 100.5, "alpha"),
                                            (0.25, float("nan"), "alpha")])
def test_library_refuses_bad_noise_options(eps, alpha, word):
    from alphaquoridorgnn_amd import _lib
    lib = _lib.load()
    for fn in (lib.aqg_engine_root_noise, lib.aqg_engine_begin_move):
        rc = fn(ctypes.byref(_engine_struct(eps, alpha)), None)
        assert rc != 0 and f"root_noise_{word}" in lib.aqg_last_error().decode()


def test_library_noise_off_launches_nothing():
    """eps == 0: aqg_engine_root_noise returns 0 before it touches the device (alpha is not looked at)."""
    from alphaquoridorgnn_amd import _lib
    lib = _lib.load()
    assert lib.aqg_engine_root_noise(ctypes.byref(_engine_struct(0.0, 0.0)), None) == 0
    assert lib.aqg_engine_root_noise(ctypes.byref(_engine_struct(0.0, 500.0)), None) == 0
    assert lib.aqg_engine_root_noise(None, None) != 0


# ------------------------------------------------------------------ Python options
@pytest.mark.parametrize("kw", [dict(root_noise_eps=-0.01), dict(root_noise_eps=1.0), dict(root_noise_eps=2.0),
                                dict(root_noise_eps=0.99999999),          # 1.0 as the float32 the library sees
                                dict(root_noise_eps=0.25, root_noise_alpha=1e-60),
                                dict(root_noise_eps=0.25, root_noise_alpha=0.0), dict(root_noise_eps=0.25, root_noise_alpha=-3.0),
                                dict(root_noise_eps=0.25, root_noise_alpha=100.01)])
def test_self_play_engine_refuses_bad_noise_options(kw):
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay, check_root_noise
    with pytest.raises(ValueError, match="root_noise"):
        BatchedSelfPlay(None, num_games=2, sims=4, board_size=5, evaluator="fake", **kw)
    with pytest.raises(ValueError, match="root_noise"):
        check_root_noise(kw["root_noise_eps"], kw.get("root_noise_alpha", 0.3))


def test_noise_option_defaults():
    from alphaquoridorgnn_amd import self_play as sp
    from alphaquoridorgnn_amd.engine import check_root_noise, default_root_noise_alpha
    assert sp.SP_ROOT_NOISE_EPS == 0.0 and sp.SP_ROOT_NOISE_ALPHA is None
    assert default_root_noise_alpha(9) == 10.0 / 209 and default_root_noise_alpha(3) == 10.0 / 17
    assert check_root_noise(0.0, None) == (0.0, 0.0)                   # off: alpha is not looked at
    assert check_root_noise(0.25, 100.0) == (0.25, 100.0)
    from alphaquoridorgnn_amd.dropin import self_play as shim
    assert shim.SP_ROOT_NOISE_EPS == 0.0 and shim.SP_ROOT_NOISE_ALPHA is None
    from alphaquoridorgnn_amd.train_cycle import _parser
    args = _parser().parse_args(["--root-noise-eps", "0.25", "--root-noise-alpha", "0.05"])
    assert (args.root_noise_eps, args.root_noise_alpha) == (0.25, 0.05)
    assert _parser().parse_args([]).root_noise_eps is None


@pytest.mark.parametrize("opt", [dict(root_noise_eps=0.25), dict(root_noise_alpha=0.3), dict(root_noise_seed=1),
                                 dict(root_noise_eps=0.0)])
def test_evaluation_paths_refuse_noise_options(opt):
    from alphaquoridorgnn_amd import evaluate_agents, evaluate_network, pv_mcts
    with pytest.raises(ValueError, match="root exploration noise"):
        evaluate_network.BatchedMatch((0, 1), 2, sims=4, board_size=5, evaluator="fake", **opt)
    with pytest.raises(ValueError, match="root exploration noise"):
        evaluate_agents.BatchedAgentMatch(0, "random", 2, sims=4, board_size=5, evaluator="fake", **opt)
    with pytest.raises(ValueError, match="root exploration noise"):
        pv_mcts.pv_mcts_action(None, **opt)
    with pytest.raises(ValueError, match="root exploration noise"):
        evaluate_network.evaluate_network(**opt)
    with pytest.raises(ValueError, match="root exploration noise"):
        evaluate_agents.evaluate_best_player(**opt)
