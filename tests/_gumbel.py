"""The reference Gumbel root search -- shared by test_gumbel_cpu.py and test_gumbel.py.

It is oracle.mcts.search with its root `_select` replaced by rule 3 of include/aqgnn.h ("Gumbel root search") from a GIVEN row of
Gumbel logits: oracle.mcts._select, the expansion and the backup below the root are reused as they are.  The GPU tests feed it the
device's own gl rows (root_gumbel()) and the evaluations recovered from the device's tree (tests/_tree_parity.py TreeFed), so no
decision of either side depends on a transcendental, and hold every node's n and w to it bit for bit."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from oracle import mcts as om, quoridor as oq   # noqa: E402
from alphaquoridorgnn_amd import gumbel as G   # noqa: E402
from alphaquoridorgnn_amd.constants import MAX_LEGAL   # noqa: E402

C_VISIT, C_SCALE = 50.0, 1.0      # the engine's defaults (policy_c_visit, policy_c_scale)


def child_q(c):
    """The child's stored q (csrc/mcts_tree.hpp q_of): f32(-w / n), 0 while n == 0."""
    return np.float32(-c.w / c.n) if c.n else np.float32(0.0)


class _Root(om._Node):
    """The root of a Gumbel search: an oracle node that also carries its logits row `gl` and m_g `m`."""


def select_root(root, gl, v, c_visit=C_VISIT, c_scale=C_SCALE):
    """Rule 3: the first index of the maximum of S over the root's children, for the considered visit count v."""
    n = [c.n for c in root.children]
    q = [child_q(c) for c in root.children]
    return G.first_argmax(G.root_score_reference(gl, n, q, c_visit, c_scale, v))


def search(model, state, sims, gl, considered, c_visit=C_VISIT, c_scale=C_SCALE, device=None, chosen=None):
    """oracle.mcts.search (pv_mcts.py:81-85, :33-66) with the root selected by rule 3.  gl: float32 [>= the root's children], a
    callable(priors) -> gl (it is asked once, when the root is expanded), or None for an already decided row.  chosen: a list that
    receives the root child index of every simulation that selected at the root."""
    root = _Root(state, 0)
    T = G.considered_visits(considered, sims)
    row, m_g = None, 0
    for s in range(sims):
        path = [root]
        node = root
        while True:
            if node.state.is_done():
                value = -1 if node.state.is_lose() else 0
                break
            if not node.children:
                prior, value = model.predict(node.state, device)
                legal = node.state.legal_actions()
                node.children = [om._Node(node.state.next(a), p) for a, p in zip(legal, prior)]
                if node is root and row is None and legal:
                    row = np.asarray(gl(np.asarray(prior, np.float32)) if callable(gl) else gl, dtype=np.float32)[:len(legal)]
                    m_g = G.considered_count(row, considered)
                break
            if node is root:
                assert s >= 1
                i = select_root(root, row, int(T[m_g][s - 1]), c_visit, c_scale)
                if chosen is not None:
                    chosen.append(i)
                node = root.children[i]
            else:
                node = om._select(node)
            path.append(node)
        v = value
        for nd in reversed(path):
            nd.w += v
            nd.n += 1
            v = -v
    root.gl, root.m = row, m_g
    return root


def winner(root, c_visit=C_VISIT, c_scale=C_SCALE):
    """Rule 4 on a searched root: the child index that is played (-1 without children)."""
    if not root.children:
        return -1
    return G.gumbel_winner_reference(root.gl, [c.n for c in root.children], [child_q(c) for c in root.children], c_visit, c_scale)


def implied_visits(gl, considered, sims):
    """What the schedule implies for the final visit counts when no simulation ends early at the root: replay T[m_g] on counters --
    every entry promotes one child with that count, so only the multiset of counts is implied: sorted, descending."""
    m_g = G.considered_count(gl, considered)
    counts = [0] * max(m_g, 1)
    for v in G.considered_visits(considered, sims)[m_g]:
        counts[counts.index(int(v))] += 1
    return sorted(counts, reverse=True)


# ------------------------------------------------------------------ a device tree against the reference search (GPU tests)
def check_tree(pool, count, root_rec, sims, gl, considered, c_visit=C_VISIT, c_scale=C_SCALE):
    """tests/_tree_parity.py check_exact with the Gumbel reference search: every node's n and w (f64 bits) of the device's pool
    against search() under the evaluations recovered from that pool and the device's own gl row.  Returns the reference root."""
    from tests import _tree_parity as TP
    fed = TP.TreeFed(pool, count, root_rec)
    assert int(pool[0]["n"]) == sims, (int(pool[0]["n"]), sims)
    root = search(fed, fed.root, sims, gl, considered, c_visit, c_scale)
    stack = [(root, 0, 0)]
    while stack:
        node, i, depth = stack.pop()
        rec = pool[i]
        where = f"node {i} at depth {depth}"
        assert node.n == int(rec["n"]), f"{where}: n {int(rec['n'])}, the reference search {node.n}"
        assert TP._bits(node.w) == TP._bits(rec["w"]), f"{where}: w {float(rec['w'])!r}, the reference search {float(node.w)!r}"
        first, cnt = TP.kids_of(rec)
        if node.children:
            assert cnt == len(node.children), where
            stack.extend((c, first + j, depth + 1) for j, c in enumerate(node.children))
        else:
            assert cnt == 0, f"{where}: expanded in the tree, never in the reference search"
    return root


def opening(N):
    return oq.init_record(N)


def table_with_peak(G_slots, peak, seed=0, spread=4.0):
    """A variate table float64 [G, MAX_LEGAL] of integer-valued entries in [-spread, spread] with a clear largest one (+64) at
    child `peak` of every row: that child has the largest gl whatever the priors are (log p spans far less)."""
    t = np.random.RandomState(seed).randint(-int(spread), int(spread) + 1, size=(G_slots, MAX_LEGAL)).astype(np.float64)
    t[:, peak] = 64.0
    return t
