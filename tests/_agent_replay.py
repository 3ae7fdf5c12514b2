"""Host replays of the batched baseline agents (test infrastructure): a random playout and the rollout MCTS by the reference-pinned
rules (agents._legal + State.next, agents._Tree), driven by the same tables of uniforms as the kernels of csrc/agents.hip, and the
comparisons of the kernels' answers with them.  Shared by tests/test_agent_match.py and tests/test_jump_cases.py."""
import numpy as np


def _State():
    from alphaquoridorgnn_amd.game_logic import State
    return State


def _pick(la, u):
    c = len(la)
    return la[min(c - 1, int(u * c))]


def _host_playout(rec, table):
    from alphaquoridorgnn_amd import agents
    s, sign, i, plies = _State().from_record(rec), 1, 0, 0
    while True:
        if s.is_lose():
            value = -sign
            break
        if s.is_draw():
            value = 0
            break
        la = agents._legal(s)
        if not la:
            value = 0
            break
        s = s.next(_pick(la, table[i]))
        i += 1
        sign = -sign
        plies += 1
    return value, plies, i, s.record()


def _check_playouts(N, states, tables, got):
    value, plies, draws, final = got
    for b in range(len(states)):
        v, p, d, f = _host_playout(states[b], tables[b])
        assert (int(value[b]), int(plies[b]), int(draws[b])) == (v, p, d), (N, b)
        assert np.array_equal(final[b], f), (N, b)


class _TableDraw:
    """agents.random_action drawing from a table in consumption order."""

    def __init__(self, table):
        self.table, self.i = table, 0

    def __call__(self, state):
        from alphaquoridorgnn_amd import agents
        a = _pick(agents._legal(state), self.table[self.i])
        self.i += 1
        return a


def _host_tree(monkeypatch, rec, table, evaluations):
    from alphaquoridorgnn_amd import agents
    draw = _TableDraw(table)
    monkeypatch.setattr(agents, "random_action", draw)
    state = _State().from_record(rec)
    tree = agents._Tree(state)
    for _ in range(evaluations):
        tree.simulate()
    visits = tree.n[tree.first[0]:tree.first[0] + tree.count[0]]
    la = agents._legal(state)
    action = la[agents.argmax(visits)] if la else -1
    expanded = sum(1 for c in tree.count[1:] if c > 0)
    return visits, la, action, draw.i, expanded


def _check_mcts(monkeypatch, N, states, tables, E, got, need_expansion):
    action, visits, actions, count = got
    expanded_somewhere = False
    for b in range(len(states)):
        v, la, a, used, expanded = _host_tree(monkeypatch, states[b], tables[b], E)
        expanded_somewhere |= expanded > 0
        c = int(count[b])
        assert c == len(la) and [int(x) for x in actions[b, :c]] == la, (N, E, b)
        assert [int(x) for x in visits[b, :c]] == v, (N, E, b)
        assert (visits[b, c:] == 0).all() and (actions[b, c:] == 0xFF).all()
        assert int(action[b]) == a, (N, E, b)
    if need_expansion:
        assert expanded_somewhere, "no host tree expanded a node below the root: the tenth-visit path was not exercised"
