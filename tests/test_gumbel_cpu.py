"""The Gumbel root search on the host (alphaquoridorgnn_amd/gumbel.py, include/aqgnn.h "Gumbel root search"): the visit schedule
against a transcription of the paper's, the reference search (tests/_gumbel.py) against what the schedule implies, rule 3 at scale 0,
the refusals of check_gumbel and of the train_cycle parser, and the variates at the ends of the uniform's range."""
import math

import numpy as np
import pytest

from alphaquoridorgnn_amd import gumbel as G
from alphaquoridorgnn_amd.selfplay_options import check_gumbel
from tests import _gumbel as TG

MS = (1, 2, 3, 4, 5, 16, 64)
BUDGETS = (1, 2, 7, 16, 50, 199)


def _paper_sequence(m, budget):
    """Sequential halving's considered visit counts as the paper's appendix writes the procedure, phase by phase: each phase gives
    every surviving action the same number of extra visits, one round of visits at a time, then halves the survivors (never below
    two); the first `budget` entries."""
    if m <= 1:
        return list(range(budget))
    phases = int(math.ceil(math.log2(m)))
    counts = [0] * m
    alive = m
    out = []
    while len(out) < budget:
        extra = max(1, budget // (phases * alive))
        for _ in range(extra):
            for i in range(alive):
                out.append(counts[i])
            for i in range(alive):
                counts[i] += 1
        alive = max(2, alive // 2)
    return out[:budget]


@pytest.mark.parametrize("budget", BUDGETS)
def test_considered_visits_against_the_papers_schedule(budget):
    sims = budget + 1
    for M in MS:
        T = G.considered_visits(M, sims)
        assert T.shape == (M + 1, budget) and T.dtype == np.int32
        for m in range(M + 1):
            row = [int(x) for x in T[m]]
            assert row == _paper_sequence(m, budget), (M, m)
            assert len(row) == budget
            lead = min(max(m, 1), budget)
            assert row[:lead] == ([0] * lead if m > 1 else list(range(lead))), (M, m)      # the first m' entries sample m' actions
            tail = row[min(m, budget):]
            assert all(a <= b for a, b in zip(tail, tail[1:])), (M, m, row)                 # non-decreasing behind them


def test_considered_visits_rows_worked_by_hand():
    T = G.considered_visits(4, 8)
    assert [int(x) for x in T[4]] == [0, 0, 0, 0, 1, 1, 2]
    assert [int(x) for x in T[3]] == [0, 0, 0, 1, 1, 2, 2]
    assert [int(x) for x in T[2]] == [0, 0, 1, 1, 2, 2, 3]
    assert [int(x) for x in T[1]] == [int(x) for x in T[0]] == [0, 1, 2, 3, 4, 5, 6]
    assert [int(x) for x in G.considered_visits(16, 17)[16]] == [0] * 16
    # M = 5, 16 selections: 3 phases; 5 actions once, then two actions 2 + 2 + 2 visits per phase (never fewer than two survive)
    assert [int(x) for x in G.considered_visits(5, 17)[5]] == [0, 0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6]
    # M = 16, 50 selections: 4 phases of 50 // (4 k) rounds: 16 actions once, 8 once, 4 three times, 2 six times, then the rest
    assert [int(x) for x in G.considered_visits(16, 51)[16]] == ([0] * 16 + [1] * 8 + [2] * 4 + [3] * 4 + [4] * 4
                                                                  + [5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10] + [11, 11])
    # M = 64, 199 selections: 6 phases; 64 once (199 // 384 -> 1), 32 once (199 // 192), 16 twice (199 // 96), 8 four times (199 // 48), ...
    row = [int(x) for x in G.considered_visits(64, 200)[64]]
    assert row[:64 + 32 + 32 + 32] == [0] * 64 + [1] * 32 + [2] * 16 + [3] * 16 + [4] * 8 + [5] * 8 + [6] * 8 + [7] * 8
    assert row[160:160 + 32] == [v for v in range(8, 16) for _ in range(4)] and row[192:] == [16, 16, 17, 17, 18, 18, 19]
    # a smaller m' inside a larger table is the schedule of m' itself
    assert [int(x) for x in G.considered_visits(64, 17)[5]] == [int(x) for x in G.considered_visits(5, 17)[5]]
    with pytest.raises(ValueError):
        G.considered_visits(0, 8)
    with pytest.raises(ValueError):
        G.considered_visits(65, 8)
    with pytest.raises(ValueError):
        G.considered_visits(4, 1)


@pytest.mark.parametrize("N,sims,M", [(3, 9, 2), (3, 17, 4), (3, 50, 16), (5, 17, 4), (5, 50, 16), (5, 9, 16), (5, 2, 4), (5, 3, 1)])
def test_reference_search_visits_are_the_schedules(N, sims, M):
    """Every considered action ends with the visit count the schedule implies, every other child with 0 (M above the legal count on
    3x3 included: m_g is then the legal count)."""
    from oracle import mcts as om, quoridor as oq
    state = oq.State(TG.opening(N))
    cnt = len(state.legal_actions())
    g = G.draw_gumbel(7, 0, 0, cnt)
    seen = {}

    def logits(p):
        seen["gl"] = G.gumbel_logits_reference(p, g, 1.0)
        return seen["gl"]
    chosen = []
    root = TG.search(om.FakeModel(3), state, sims, logits, M, chosen=chosen)
    gl, n = seen["gl"], np.array([c.n for c in root.children])
    assert root.n == sims and n.sum() == sims - 1 and len(chosen) == sims - 1
    m_g = G.considered_count(gl, M)
    assert m_g == min(M, cnt) and root.m == m_g
    top = np.argsort(-gl.astype(np.float64), kind="stable")[:m_g]          # the sampled actions: the m_g largest logits
    assert sorted(n[top], reverse=True) == TG.implied_visits(gl, M, sims)
    rest = np.setdiff1d(np.arange(cnt), top)
    assert not n[rest].any()
    # the survivor is one of the most visited, and rule 4 names it
    w = TG.winner(root)
    assert n[w] == n.max() and w in top


def test_scale_zero_with_equal_q_is_the_argmax_of_the_priors():
    rng = np.random.RandomState(3)
    for cnt in (1, 5, 64, 65, 131):
        p = rng.dirichlet(np.ones(cnt)).astype(np.float32)
        gl = G.gumbel_logits_reference(p, rng.standard_normal(cnt) * 100, 0.0)
        assert gl.tobytes() == np.log(p.astype(np.float64)).astype(np.float32).tobytes()
        for n_all, q_all in ((0, 0.0), (3, 0.25), (3, -1.0)):
            n = np.full(cnt, n_all)
            q = np.full(cnt, q_all, np.float32)
            s = G.root_score_reference(gl, n, q, 50.0, 1.0, n_all)
            assert G.first_argmax(s) == int(np.argmax(p))
            assert G.gumbel_winner_reference(gl, n, q, 50.0, 1.0) == int(np.argmax(p))
    # ... and only the considered count takes part
    gl = np.array([0.0, 5.0, 1.0], np.float32)
    s = G.root_score_reference(gl, [1, 0, 1], [0.0, 0.0, 0.5], 50.0, 1.0, 1)
    assert s[1] == -np.inf and G.first_argmax(s) == 2
    assert s[0] == np.float32(np.float32(51.0) * np.float32(0.5)) and s[2] == np.float32(np.float32(1.0) + np.float32(51.0) * np.float32(0.75))
    # nothing sampled: child 0, as the PUCT arg-max does
    assert G.first_argmax(G.root_score_reference(np.full(3, -np.inf, np.float32), [0, 0, 0], [0, 0, 0], 50.0, 1.0, 0)) == 0
    assert G.gumbel_winner_reference(np.zeros(0, np.float32), [], [], 50.0, 1.0) == -1


def test_logits_exclude_what_has_no_prior():
    p = np.array([0.5, 0.0, -0.25, np.nan, 0.25], np.float32)
    g = np.array([1.0, 2.0, 3.0, 4.0, np.inf])
    gl = G.gumbel_logits_reference(p, g, 2.0)
    assert list(np.isneginf(gl)) == [False, True, True, True, False]
    assert gl[0] == np.float32(2.0 * 1.0 + math.log(0.5)) and gl[4] == np.float32(math.log(0.25))      # a non-finite variate reads 0
    assert G.considered_count(gl, 16) == 2 and G.considered_count(gl, 1) == 1


def test_draw_gumbel_is_finite_at_the_ends_of_the_uniforms_range():
    below_one = 1.0 - 2.0 ** -53                         # the largest draw of the counter generator is (2^53 - 1) 2^-53
    g = G.draw_gumbel(uniforms=[0.0, 2.0 ** -53, 0.5, below_one])
    assert np.isfinite(g).all()
    assert g[0] == -math.log(G.DBL_MIN) and g[3] == -math.log(-math.log(2.0 ** -53))
    assert g[0] > g[1] > g[2] > g[3]
    # the generator: a component's variate does not depend on the count, a game's row not on anything but (seed, game, ply)
    a, b = G.draw_gumbel(11, 5, 2, 136), G.draw_gumbel(11, 5, 2, 40)
    assert np.isfinite(a).all() and a[:40].tobytes() == b.tobytes()
    assert not np.array_equal(a[:40], G.draw_gumbel(11, 6, 2, 40)) and not np.array_equal(a[:40], G.draw_gumbel(11, 5, 3, 40))
    assert abs(float(G.draw_gumbel(1, 0, 0, 136).mean()) - 0.5772) < 0.35      # Euler's constant, 136 draws (sd 1.28 / sqrt(136) = 0.11)


# ------------------------------------------------------------------ refusals
def test_check_gumbel_refuses_in_the_librarys_order():
    assert check_gumbel() is None and check_gumbel(0, float("nan"), 1, 0.25, True, 0.9, 3, "external") is None      # off: nothing is read
    assert check_gumbel(16, 1.0, 2) == (16, 1.0) and check_gumbel(64, 0, 200) == (64, 0.0) and check_gumbel(1, 2.5, 9) == (1, 2.5)
    for bad, word in ((dict(sims=1), "sims >= 2"), (dict(gumbel_considered=65), "1..64"), (dict(gumbel_considered=-1), "1..64"),
                      (dict(gumbel_scale=-0.5), "gumbel_scale"), (dict(gumbel_scale=float("nan")), "gumbel_scale"),
                      (dict(gumbel_scale=float("inf")), "gumbel_scale"), (dict(gumbel_scale="1"), "gumbel_scale"),
                      (dict(root_noise_eps=0.25), "root noise"), (dict(tree_reuse=True), "tree_reuse"),
                      (dict(resign_threshold=0.9), "resignation"), (dict(temperature_plies=4), "temperature_plies"),
                      (dict(evaluator="external"), "external"), (dict(gumbel_considered=True), "integer"),
                      (dict(gumbel_considered=4.0), "integer")):
        kw = dict(gumbel_considered=16, gumbel_scale=1.0, sims=50)
        kw.update(bad)
        with pytest.raises(ValueError, match=word):
            check_gumbel(**kw)
    # the order: the first failing check names the error
    with pytest.raises(ValueError, match="sims >= 2"):
        check_gumbel(65, -1.0, 1, 0.25, True, 0.9, 3, "external")
    with pytest.raises(ValueError, match="1..64"):
        check_gumbel(65, -1.0, 2, 0.25, True, 0.9, 3, "external")
    with pytest.raises(ValueError, match="gumbel_scale"):
        check_gumbel(4, -1.0, 2, 0.25, True, 0.9, 3, "external")
    with pytest.raises(ValueError, match="root noise"):
        check_gumbel(4, 1.0, 2, 0.25, True, 0.9, 3, "external")
    with pytest.raises(ValueError, match="tree_reuse"):
        check_gumbel(4, 1.0, 2, 0.0, True, 0.9, 3, "external")
    with pytest.raises(ValueError, match="resignation"):
        check_gumbel(4, 1.0, 2, 0.0, False, 0.9, 3, "external")
    with pytest.raises(ValueError, match="temperature_plies"):
        check_gumbel(4, 1.0, 2, 0.0, False, None, 3, "external")


def _parse(*argv):
    from alphaquoridorgnn_amd import train_cycle_options as tco
    args = tco._parser().parse_args(list(argv))
    tco.check_args(args)
    return tco._check_gumbel_args(args)


def test_train_cycle_parser_refuses_at_parse_time():
    assert _parse() is None
    assert _parse("--policy-target", "completed-q", "--gumbel-considered", "16") == (16, 1.0, None)
    assert _parse("--policy-target", "completed-q", "--gumbel-considered", "4", "--gumbel-scale", "0", "--gumbel-seed", "9", "--sims", "32") == (4, 0.0, 9)
    ok = ("--policy-target", "completed-q", "--gumbel-considered", "16")
    for argv, word in ((("--gumbel-considered", "16"), "completed-q"),
                       (("--policy-target", "visits", "--gumbel-considered", "16"), "completed-q"),
                       (("--gumbel-scale", "1.0"), "need --gumbel-considered"), (("--gumbel-seed", "3"), "need --gumbel-considered"),
                       (("--policy-target", "completed-q", "--gumbel-considered", "0"), "1..64"),
                       (("--policy-target", "completed-q", "--gumbel-considered", "65"), "1..64"),
                       (ok + ("--gumbel-scale", "-1"), "gumbel_scale"), (ok + ("--gumbel-scale", "nan"), "gumbel_scale"),
                       (ok + ("--sims", "1"), "sims >= 2"), (ok + ("--root-noise-eps", "0.25"), "root noise"),
                       (ok + ("--tree-reuse",), "tree_reuse"), (ok + ("--resign-threshold", "0.9"), "resignation"),
                       (ok + ("--resign-threshold", "auto"), "resignation"), (ok + ("--temperature-plies", "6"), "temperature_plies")):
        with pytest.raises(ValueError, match=word):
            _parse(*argv)


def test_evaluation_paths_refuse_the_option():
    from alphaquoridorgnn_amd import evaluate_agents as ea, evaluate_network as en
    for call in (lambda: en.BatchedMatch([0, 1], 2, evaluator="fake", gumbel_considered=4), lambda: en.evaluate_network(gumbel_scale=1.0),
                 lambda: ea.evaluate_best_player(gumbel_seed=1), lambda: ea.BatchedAgentMatch(None, "random", 2, gumbel_considered=0)):
        with pytest.raises(ValueError, match="Gumbel root search"):
            call()


def test_self_play_needs_the_completed_q_target():
    from alphaquoridorgnn_amd import self_play as sp
    assert sp._gumbel_options("visits") == {} and sp.SP_GUMBEL_CONSIDERED == 0
    old = sp.SP_GUMBEL_CONSIDERED
    try:
        sp.SP_GUMBEL_CONSIDERED = 8
        assert sp._gumbel_options("completed_q") == dict(gumbel_considered=8, gumbel_scale=1.0, gumbel_seed=None)
        with pytest.raises(ValueError, match="completed_q"):
            sp._gumbel_options("visits")
    finally:
        sp.SP_GUMBEL_CONSIDERED = old
