"""Host statement of self-play with tree reuse (include/aqgnn.h, "tree reuse") -- shared by test_tree_reuse_cpu.py and
test_tree_reuse.py.  Built from the oracle's PV-MCTS pieces: `search_from` is the loop of oracle.mcts.search started from a given
root node (which may be expanded already), `play_game` is oracle.mcts.play's loop with the rule of the option, and `serialise` /
`decode` move a pointer tree into a pool of the engine's node records and back, in the engine's expansion order."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from oracle import mcts as om, quoridor as oq   # noqa: E402


def action_count(N):
    return N * N + 2 * (N - 1) ** 2


class Node(om._Node):
    """oracle.mcts._Node with the action that led to it and the number of its expansion: the engine allocates a node's child block
    when the node is expanded, so blocks sit in the pool in expansion order."""
    __slots__ = ("action", "seq")

    def __init__(self, state, p, action=0xFF):
        super().__init__(state, p)
        self.action, self.seq = action, -1


class Clock:
    """Expansion numbers that go on across the moves of a game (a kept subtree keeps its blocks' order)."""

    def __init__(self):
        self.t = 0

    def tick(self):
        self.t += 1
        return self.t


def search_from(model, root, sims, clock=None, first_priors=None):
    """oracle.mcts.search's loop, `sims` simulations, from `root` as it stands.  first_priors: a function of the priors, applied to
    the FIRST prediction if that is the root's (root noise of a fresh root)."""
    clock = clock or Clock()
    for sim in range(sims):
        path, node = [root], root
        while True:
            if node.state.is_done():
                value = -1 if node.state.is_lose() else 0
                break
            if not node.children:
                prior, value = model.predict(node.state)
                if node is root and first_priors is not None:
                    prior = first_priors(prior)
                legal = node.state.legal_actions()
                node.children = [Node(node.state.next(a), p, int(a)) for a, p in zip(legal, prior)]
                node.seq = clock.tick()
                break
            node = om._select(node)
            path.append(node)
        v = value
        for nd in reversed(path):
            nd.w += v
            nd.n += 1
            v = -v
    return root


def keeps(child, ended, keep_visits):
    """The rule: the game goes on, the child is expanded, child.n <= keep_visits."""
    return (not ended) and bool(child.children) and child.n <= keep_visits


def reroot(child):
    """The chosen child as the next root: its statistics and subtree as they stand, a fresh root's action and prior."""
    child.action, child.p = 0xFF, 0
    return child


def play_game(N, sims, keep_visits, uniforms, bias=2, temperature_plies=0, noise=None, eps=None):
    """One game with tree reuse (keep_visits None = off: oracle.mcts.play's loop).  noise: per ply the float64 gamma variates of
    that root (table mode), mixed with weight `eps` -- into the root's prediction when the root is fresh, into its children's stored
    priors when it was kept.  Returns (rows, z): per ply dict(rec, visits dense int16 [A], action, value float32 = root.w / root.n,
    kept = the move started from a kept subtree, kept_visits)."""
    from tests.test_root_noise_cpu import mix_statement
    model, state, rows, clock = om.FakeModel(bias), oq.State(N=N), [], Clock()
    root, kept = Node(state, 0), False
    A = action_count(N)
    while not state.is_done():
        ply = state.plies_played
        kept_visits = root.n if kept else 0
        first_priors = None
        if noise is not None:
            if kept:
                mixed = mix_statement(np.asarray([c.p for c in root.children], dtype=np.float32), noise[ply], eps)
                for c, p in zip(root.children, mixed):
                    c.p = p
            else:
                first_priors = lambda p, ply=ply: mix_statement(p, noise[ply], eps)      # noqa: E731
        search_from(model, root, sims, clock, first_priors)
        visits = [c.n for c in root.children]
        legal = state.legal_actions()
        draw = om.choice_index(om.boltzman(visits, 1.0), uniforms[ply])
        idx = draw if not (temperature_plies and ply >= temperature_plies) else int(np.argmax(visits))
        dense = np.zeros(A, dtype=np.int16)
        dense[list(legal)] = visits
        rows.append(dict(rec=state.rec.copy(), visits=dense, action=int(legal[idx]), value=np.float32(root.w / root.n), kept=kept,
                         kept_visits=kept_visits))
        child = root.children[idx]
        state = child.state
        kept = keep_visits is not None and keeps(child, state.is_done(), keep_visits)
        root = reroot(child) if kept else Node(state, 0)
    return rows, om.first_player_value(state)


# ------------------------------------------------------------------ pointer tree <-> pool of node records
def _record(node, kids):
    from alphaquoridorgnn_amd.engine import NODE_DTYPE
    r = np.zeros((), dtype=NODE_DTYPE)
    p = np.float32(node.p)
    r["w"], r["p"], r["action"], r["n"], r["kids"] = float(node.w), p, node.action, node.n, kids
    r["q"] = np.float32(-node.w / node.n) if node.n else np.float32(0.0)
    r["cp"] = np.float32(om.C_PUCT) * p
    return r


def serialise(root, cap=None):
    """The tree as the engine's pool: the root at 0, then every expanded node's child block in expansion order (Node.seq)."""
    from alphaquoridorgnn_amd.engine import NODE_DTYPE
    expanded, stack = [], [root]
    while stack:
        nd = stack.pop()
        if nd.children:
            expanded.append(nd)
            stack.extend(nd.children)
    expanded.sort(key=lambda nd: nd.seq)
    first, nxt = {}, 1
    for nd in expanded:
        first[id(nd)] = nxt
        nxt += len(nd.children)
    pool = np.zeros(max(nxt, cap or 0), dtype=NODE_DTYPE)
    kids = lambda nd: (first[id(nd)] | (len(nd.children) << 24)) if nd.children else 0      # noqa: E731
    pool[0] = _record(root, kids(root))
    pool[0]["p"], pool[0]["cp"] = 0, 0
    for nd in expanded:
        for i, c in enumerate(nd.children):
            pool[first[id(nd)] + i] = _record(c, kids(c))
    return pool, nxt


def decode(pool, count, root_state):
    """The pointer tree of a pool (states by replaying the actions from root_state); expansion numbers = the blocks' positions."""
    def build(i, state, is_root):
        r = pool[i]
        nd = Node(state, 0 if is_root else np.float32(r["p"]), int(r["action"]))
        nd.w, nd.n = float(r["w"]), int(r["n"])
        cnt, first = int(r["kids"]) >> 24, int(r["kids"]) & 0xFFFFFF
        if cnt:
            assert first + cnt <= count
            nd.seq = first
            nd.children = [build(first + j, state.next(int(pool[first + j]["action"])), False) for j in range(cnt)]
        return nd
    return build(0, root_state, True)


def same_tree(a, b):
    """Two pointer trees agree in every node's statistics, prior, action and child order."""
    stack = [(a, b)]
    while stack:
        x, y = stack.pop()
        if (float(x.w), x.n, x.action) != (float(y.w), y.n, y.action) or np.float32(x.p).tobytes() != np.float32(y.p).tobytes():
            return False
        if len(x.children or []) != len(y.children or []):
            return False
        stack.extend(zip(x.children or [], y.children or []))
    return True


def block_starts(pool, count):
    """(old first index of every child block in the used pool, ascending) -- by walking the tree from the root."""
    out, stack = [], [0]
    while stack:
        i = stack.pop()
        cnt, first = int(pool[i]["kids"]) >> 24, int(pool[i]["kids"]) & 0xFFFFFF
        if cnt:
            out.append((first, cnt))
            stack.extend(range(first, first + cnt))
    return sorted(out)


# ------------------------------------------------------------------ synthetic trees (no game behind them)
class NoState:
    """Stands in for a position where only the tree's shape matters."""

    def next(self, action):
        return self


def synthetic_tree(seed, expansions, shape="random", max_children=136):
    """A tree of `expansions` expanded nodes with consistent counts (an expanded node's n is 1 + its children's, an unexpanded one's
    0), random w / p / action.  shape 'random': every expansion picks an unexpanded node anywhere and gives it 1 .. max_children
    children; 'chain': the root has two children, every node below the first has one -- the first child's subtree is `expansions - 1`
    deep with one-record blocks back to back; 'interleaved': the root has three children whose subtrees are expanded in turn, so the
    blocks of any one of them alternate with the others' in the pool."""
    rng = np.random.RandomState(seed)
    clock = Clock()

    def expand(nd, cnt):
        nd.children = [Node(NoState(), np.float32(rng.random_sample()), int(rng.randint(0, 200))) for _ in range(cnt)]
        nd.seq = clock.tick()
        return nd.children

    root = Node(NoState(), 0)
    if shape == "chain":
        nd = expand(root, 2)[0]
        for _ in range(expansions - 1):
            nd = expand(nd, 1)[0]
    elif shape == "interleaved":
        open_ = [[c] for c in expand(root, 3)]
        for e in range(expansions - 1):
            mine = open_[e % 3]
            nd = mine.pop(rng.randint(len(mine)))
            mine.extend(expand(nd, int(rng.randint(1, max_children + 1))))
    else:
        open_ = [root]
        for _ in range(expansions):
            nd = open_.pop(rng.randint(len(open_)))
            open_.extend(expand(nd, int(rng.randint(1, max_children + 1))))
    order, stack = [], [root]
    while stack:
        nd = stack.pop()
        order.append(nd)
        stack.extend(nd.children or [])
    for nd in reversed(order):                      # children before parents
        nd.n = 1 + sum(c.n for c in nd.children) if nd.children else 0
        nd.w = float(np.round(rng.standard_normal() * nd.n, 3))
    return root
