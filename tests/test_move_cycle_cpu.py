"""The host statements of tests/_move_cycle.py without a GPU: finish_move_reference against oracle.mcts.choice_index and
oracle.mcts.pv_mcts_policy on the oracle's searches, the input builders against what they claim (counts, boundaries, margins), and
refill_reference against a hand-written script and the chain statements tests/test_gpu_parity.py::
test_slot_refill_games_equal_standalone_games makes about the recorded arrays; every refill script against the property it is named
after."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import _move_cycle as MC   # noqa: E402


# ---------------------------------------------------------------------------------------------- A. the choice of a move
def test_boltzman_is_the_package_s_and_the_oracle_s():
    from alphaquoridorgnn_amd import pv_mcts
    from oracle import mcts as om
    for n in ([3, 0, 1, 7], [1] * 136, [32767, 1, 1]):
        for T in (1.0, 0.5, 2.0, 0.25):
            assert MC.boltzman(n, T) == pv_mcts.boltzman(n, T) == om.boltzman(n, T)


@pytest.mark.parametrize("N,sims", [(3, 12), (5, 30), (9, 40)])
def test_statement_equals_the_oracle_on_its_own_searches(N, sims):
    from oracle import mcts as om, quoridor as oq
    rng = np.random.RandomState(N)
    for rec in MC.real_roots(N)["walk"][:3] + [MC.real_roots(N)["opening"]]:
        state = oq.State(rec)
        root = om.search(om.FakeModel(2), state, sims)
        n, legal = [c.n for c in root.children], state.legal_actions()
        for T in (0, 1.0, 0.5, 2.0):
            policy = om.pv_mcts_policy(om.FakeModel(2), state, T, sims)
            for u in [0.0, MC.U_TOP] + rng.random_sample(6).tolist():
                idx, action, value = MC.finish_move_reference(n, legal, root.w, root.n, T, 0, state.plies_played, u)
                assert idx == om.choice_index(policy, u) and action == legal[idx] and n[idx] > 0
                assert value.dtype == np.float32 and value == np.float32(root.w / root.n)
        # the schedule: from ply K on the first maximum, whatever the uniform
        first = int(np.argmax(n))
        for K in (1, state.plies_played, state.plies_played + 1):
            late = K > 0 and state.plies_played >= K
            idx = MC.finish_move_reference(n, legal, root.w, root.n, 1.0, K, state.plies_played, MC.U_TOP)[0]
            assert idx == (first if late else om.choice_index(om.boltzman(n, 1.0), MC.U_TOP))
    assert MC.finish_move_reference([0, 0], [4, 5], 0.0, 0, 0, 0, 0, 0.5) == (0, 4, np.float32(0))


def _picked(c, u, T=1.0, K=0):
    from oracle import quoridor as oq
    return MC.finish_move_reference(c["n"], list(range(c["cnt"])), c["w_root"], c["n_root"], T, K, oq.State(c["root"]).plies_played, u)[0]


def test_sampling_cases_do_what_they_claim():
    cases = MC.sampling_cases()
    counts = sorted({c["cnt"] for c in cases})
    assert counts == [1, 2, 63, 64, 65, 127, 128, 129, 131]
    names = {c["name"].split("/")[0] for c in cases}
    assert {"single0", "separated", "big", "random"} <= names
    equalities = 0
    for c in cases:
        n, kind = c["n"], c["name"].split("/")[0]
        assert n.sum() > 0 and len(n) == c["cnt"] <= MC.legal_count(c["root"]) and all(0.0 <= u < 1.0 for u in c["us"])
        visited = np.flatnonzero(n > 0)
        if kind.startswith("single"):
            assert len(visited) == 1 and c["us"] == [0.0, 0.5, MC.U_TOP] and all(_picked(c, u) == visited[0] for u in c["us"])
        if kind == "separated":
            assert n[0] == 0 and n[-1] == 0 and (np.diff(visited) > 1).any()
            assert {63, 64, 127, 128} & set(range(1, c["cnt"] - 1)) <= set(visited.tolist())
        if kind == "big":
            assert n.max() == 32767 and (np.delete(n, c["cnt"] // 2) == 1).all()
        if kind == "random":
            assert abs((n == 0).mean() - 0.5) <= 0.2 or c["cnt"] <= 2
        if kind in ("separated", "big", "random"):
            cdf = MC.cdf_values(n, 1.0)
            for u in c["us"]:
                at = np.flatnonzero(cdf == u)
                if len(at):                                    # u = c: the visited child behind the one whose interval ends at c
                    equalities += 1
                    below = visited[visited <= at[-1]]
                    assert _picked(c, u) == visited[len(below)] and n[_picked(c, u)] > 0
                elif (cdf == np.nextafter(u, 1.0)).any():      # u = nextafter(c, 0): the child whose interval ends at c
                    at = np.flatnonzero(cdf == np.nextafter(u, 1.0))
                    assert _picked(c, u) == at[0] and n[at[0]] > 0
                assert n[_picked(c, u)] > 0
        if kind == "separated":                                # every distinct cdf value is there, both ways
            values = np.unique(MC.cdf_values(n, 1.0))
            assert set(values[values < 1.0].tolist()) <= set(c["us"]) and {float(np.nextafter(v, 0.0)) for v in values if v > 0} <= set(c["us"])
    assert equalities >= 60


def test_real_root_cases_do_what_they_claim():
    from oracle import quoridor as oq
    for N in (3, 5, 9):
        cases = MC.real_root_cases(N)
        for c in cases:
            assert c["cnt"] == MC.legal_count(c["root"]) and oq.State(c["root"]).N == N and not oq.State(c["root"]).is_done()
            assert all(c["n"][_picked(c, u)] > 0 for u in c["us"])
    roots = MC.real_roots(3)
    assert roots["no_walls"][1] == 0 and all(a < 9 for a in oq.legal_actions(roots["no_walls"]))
    legal = oq.legal_actions(roots["one_step"])
    assert oq.State(roots["one_step"]).next(legal[roots["one_step_child"]]).is_lose()
    one = [c for c in MC.real_root_cases(3) if c["name"] == "one_step"][0]
    assert all(_picked(one, u) == roots["one_step_child"] for u in one["us"])
    rec, done, z = MC.transition_reference(roots["one_step"], legal[roots["one_step_child"]])
    assert done == 1 and z == (-1 if oq.State(rec).plies_played % 2 == 0 else 1)


def test_first_maximum_cases_do_what_they_claim():
    from oracle import quoridor as oq
    cases = MC.first_maximum_cases()
    plies = {c["name"].split("/")[0]: oq.State(c["root"]).plies_played for c in cases}
    assert plies["opening"] == 0 and plies["later"] >= 1
    assert MC.legal_count(MC.real_roots(9)["later"]) >= 129
    for c in cases:
        n, kind = c["n"], c["name"].split("/")[1]
        top = np.flatnonzero(n == n.max())
        if kind == "tie":
            assert len(top) == 3 and (top[0] > 0 or c["cnt"] == 3)
        else:
            assert top.tolist() == [c["cnt"] - 1]
        late = plies[c["name"].split("/")[0]] >= 1
        for u in c["us"]:
            assert _picked(c, u, T=0) == top[0]
            assert (_picked(c, u, T=1.0, K=1) == top[0]) == (late or _picked(c, u, T=1.0) == top[0])
        last_visited = np.flatnonzero(n > 0)[-1]
        assert _picked(c, MC.U_TOP, T=1.0, K=1) == (top[0] if late else last_visited)
    assert {c["cnt"] for c in cases if "tie" in c["name"]} >= {63, 64, 65, 127, 128, 129}


@pytest.mark.parametrize("T,nmax,big", [(0.5, 30, True), (2.0, 30, True), (0.25, 30, True), (float(np.float32(0.02)), 200, False)])
def test_temperature_cases_keep_their_margin(T, nmax, big):
    cases = MC.temperature_cases(T, nmax=nmax, big=big)
    assert sorted({c["cnt"] for c in cases}) == [1, 2, 63, 64, 65, 127, 128, 129, 131]
    for c in cases:
        cdf = MC.cdf_values(c["n"], T)
        assert np.isfinite(cdf).all() and c["n"].max() <= (32767 if "big" in c["name"] else nmax)
        visited = np.flatnonzero(c["n"] > 0)
        assert 1 <= len(c["us"]) <= len(visited)
        for u in c["us"]:
            assert np.abs(cdf - u).min() >= MC.MARGIN and c["n"][_picked(c, u, T=T)] > 0
        if "random" in c["name"] and T >= 0.25:               # every visited child's midpoint is usable
            assert len(c["us"]) == len(visited) and sorted({_picked(c, u, T=T) for u in c["us"]}) == visited.tolist()
        if "big" in c["name"]:
            assert c["cnt"] // 2 in {_picked(c, u, T=T) for u in c["us"]}
            if T == 2.0:
                assert len(c["us"]) == c["cnt"]


# ---------------------------------------------------------------------------------------------- B. the slot refill
def test_refill_statement_on_a_hand_written_script():
    """G = 6, Q = 11.  Move 1 ends slots 1 and 4 (games 6, 7); move 2 ends 0, 4 and 5 (games 8, 9, 10: the quota is handed out); move
    3 ends 1 and 2 -- retired; move 4 names a retired and an active slot."""
    G, Q = 6, 11
    steps = MC.refill_reference(G, Q, [[1, 4], [0, 4, 5], [1, 2], [2, 3]])
    assert steps[0]["slot_game"].tolist() == [0, 6, 2, 3, 7, 5] and steps[0]["counters"] == (6, 2, 2, 8, 1)
    assert steps[1]["slot_game"].tolist() == [8, 6, 2, 3, 9, 10] and steps[1]["counters"] == (6, 5, 5, 11, 2)
    assert steps[2]["slot_game"].tolist() == [8, -1, -1, 3, 9, 10] and steps[2]["counters"] == (4, 7, 7, 11, 3)
    assert steps[2]["game_active"].tolist() == [1, 0, 0, 1, 1, 1] and not steps[2]["refilled"].any()
    assert steps[3]["slot_game"].tolist() == [8, -1, -1, -1, 9, 10] and steps[3]["counters"] == (3, 8, 8, 11, 4)
    last = steps[3]
    assert last["game_slot"].tolist() == [0, 1, 2, 3, 4, 5, 1, 4, 0, 4, 5]
    assert last["game_first_move"].tolist() == [0, 0, 0, 0, 0, 0, 1, 1, 2, 2, 2]
    assert last["game_done"].tolist() == [1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0]
    assert steps[1]["refilled"].tolist() == [True, False, False, False, True, True]
    # Q == G: no refill launch, so no slot is retired and the move counter stays
    one = MC.refill_reference(3, 3, [[1], [1, 2]])
    assert one[1]["slot_game"].tolist() == [0, 1, 2] and one[1]["game_active"].tolist() == [1, 0, 0] and one[1]["counters"] == (1, 2, 2, 3, 0)


def test_refill_statement_keeps_the_chains_of_a_generation():
    """What test_slot_refill_games_equal_standalone_games asserts of the recorded arrays, on the statement driven by game lengths."""
    G, Q = 6, 23
    lengths = np.random.RandomState(5).randint(2, 15, Q)
    sets = MC.end_sets_from_lengths(G, Q, lengths)
    last = MC.refill_reference(G, Q, sets)[-1]
    slot, first = last["game_slot"], last["game_first_move"]
    assert last["game_done"].all() and (slot >= 0).all() and sorted(slot[:G].tolist()) == list(range(G)) and (first[:G] == 0).all()
    for g in range(G):
        ks = [k for k in range(Q) if slot[k] == g]
        assert all(first[b] == first[a] + lengths[a] for a, b in zip(ks, ks[1:]))
    assert last["counters"] == (0, Q, Q, Q, max(sum(lengths[k] for k in range(Q) if slot[k] == g) for g in range(G)))
    assert (last["slot_game"] == -1).all()
    # games are handed out in the order in which slots fall idle, ties in slot order
    order = sorted(range(G, Q), key=lambda k: (first[k], slot[k]))
    assert order == list(range(G, Q))


@pytest.mark.parametrize("G", MC.REFILL_SLOTS)
def test_refill_scripts_do_what_they_are_named_after(G):
    Q = MC.plain_quota(G)
    for name, sets in MC.plain_scripts(G):
        steps = MC.refill_reference(G, Q, sets)
        assert all((s["slot_game"] >= 0).all() and s["counters"][0] == G for s in steps), name      # the quota is never met
        assert steps[-1]["counters"][3] == G + sum(len(s) for s in sets) <= Q
        assert all(s["refilled"].sum() == len(e) for s, e in zip(steps, sets))
    named = dict(MC.plain_scripts(G))
    assert named["all_twice"] == [list(range(G))] * 2 and named["last_slot"] == [[G - 1]]
    a, b = named["lane63_then_lane0"]
    assert all(s % 64 == 63 for s in a) and all(s % 64 == 0 for s in b) and len(a) == G // 64 and len(b) == (G + 63) // 64
    half, few = named["random_half_then_1pct"]
    assert len(half) - (G + 1) // 2 in (0, 1) and len(few) == max(1, G // 100)
    assert ("1023_and_1024" in named) == (G >= 1025)
    if G >= 65:                                                # idle slots in every wave
        assert {s // 64 for s in half} == set(range((G + 63) // 64))
    cuts = {name: (q, sets, retired) for name, q, sets, retired in MC.cut_scripts(G)}
    assert ("cut_inside_a_wave" in cuts) == (G >= 63) and ("cut_at_a_wave_boundary" in cuts) == (G >= 65)
    assert ("cut_inside_the_second_chunk" in cuts) == (G >= 1025) and "cut_with_no_game_left" in cuts
    for name, (q, sets, retired) in cuts.items():
        assert q > G
        steps = MC.refill_reference(G, q, sets)
        idle = [s for s in sets[1]]
        left = q - steps[0]["counters"][3]
        assert steps[0]["counters"][0] == G and 0 <= left < len(idle), name                  # fewer games left than idle slots
        assert steps[1]["counters"][3] == q and steps[1]["counters"][0] == G - (len(idle) - left)
        gone = np.flatnonzero(steps[1]["slot_game"] == -1).tolist()
        assert gone == idle[left:] and gone[0] == retired, name
        if name == "cut_inside_a_wave":
            assert retired % 64 not in (0, 63) and idle[left - 1] // 64 == retired // 64 and (G < 128 or retired >= 64)
        if name == "cut_at_a_wave_boundary":
            assert idle[left - 1] // 64 < retired // 64 == [s for s in idle if s // 64 == retired // 64][0] // 64 and retired < 1024
            assert retired == min(s for s in idle if s // 64 == retired // 64)
        if name == "cut_inside_the_second_chunk":
            assert retired >= 1024 and (G == 1025 or idle[left - 1] >= 1024)
        if name == "cut_with_no_game_left":
            assert left == 0 and not steps[1]["refilled"].any()
        # the move after the cut: some active slots and some retired ones are named
        after = sets[2]
        ended = [s for s in after if steps[1]["game_active"][s]]
        assert (ended or G == 1) and any(steps[1]["slot_game"][s] == -1 for s in after)
        assert steps[2]["counters"][0] == steps[1]["counters"][0] - len(ended) and steps[2]["counters"][3] == q
        assert not steps[2]["refilled"].any() and set(np.flatnonzero(steps[2]["slot_game"] == -1)) == set(gone) | set(ended)
