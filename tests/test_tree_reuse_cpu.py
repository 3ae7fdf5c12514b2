"""Tree reuse without a GPU (include/aqgnn.h "tree reuse"): engine.keep_subtree_reference -- the numpy statement of the keep launch --
against the oracle's pointer trees, the rule's edges, every refusal, and the C ABI (additive: ABI 15, struct aqg_engine unchanged)."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import _tree_reuse as T   # noqa: E402

BIG = 1 << 20      # a keep_visits that keeps every expanded child


def _searched_root(N, sims, bias=2):
    from oracle import mcts as om, quoridor as oq
    return T.search_from(om.FakeModel(bias), T.Node(oq.State(N=N), 0), sims)


@functools.lru_cache(maxsize=None)
def _pool(N, sims):
    return T.serialise(_searched_root(N, sims))


# ------------------------------------------------------------------ the reference against the pointer tree
@pytest.mark.parametrize("N,sims", [(3, 8), (3, 24), (5, 8), (5, 24)])
def test_reference_rerooting_is_the_childs_subtree(N, sims):
    from alphaquoridorgnn_amd.engine import keep_subtree_reference
    from oracle import mcts as om
    pool, count = _pool(N, sims)
    root = _searched_root(N, sims)
    assert T.same_tree(T.decode(pool, count, root.state), root)                 # the serialisation round-trips
    assert (int(pool[0]["kids"]) & 0xFFFFFF) == 1 and pool[0]["n"] == sims
    kept_some = dropped_some = False
    for idx, child in enumerate(root.children):
        out, cnt, kept = keep_subtree_reference(pool, count, idx, BIG)
        assert kept == bool(child.children)
        if not kept:
            assert cnt == count and out.tobytes() == pool.tobytes()
            dropped_some = True
            continue
        kept_some = True
        # exactly the child's subtree, as a tree and as the pool the engine's expansion order gives
        want = T.reroot(_searched_root(N, sims).children[idx])
        assert T.same_tree(T.decode(out, cnt, child.state), want)
        wpool, wcount = T.serialise(want)
        assert cnt == wcount and out[:cnt].tobytes() == wpool[:wcount].tobytes()
        # layout: root at 0 with a fresh root's action / p / cp, its children at 1 .. cnt, blocks contiguous and in the old order
        r = out[0]
        assert (r["action"], r["p"], r["cp"]) == (0xFF, 0, 0) and (r["w"], r["n"], r["q"]) == (float(child.w), child.n, np.float32(-child.w / child.n))
        assert (int(r["kids"]) & 0xFFFFFF) == 1 and (int(r["kids"]) >> 24) == len(child.children)
        blocks = T.block_starts(out, cnt)
        assert blocks[0][0] == 1 and all(a + c == b for (a, c), (b, _) in zip(blocks, blocks[1:])) and blocks[-1][0] + blocks[-1][1] == cnt
        assert int(r["n"]) == 1 + int(out[1:1 + len(child.children)]["n"].sum())
        assert not (out[:cnt]["action"] >> 8).any()
        # a search continued on the decoded pool equals one continued on the tree
        a = T.search_from(om.FakeModel(2), T.decode(out, cnt, child.state), 8)
        b = T.search_from(om.FakeModel(2), want, 8)
        assert T.same_tree(a, b) and a.n == child.n + 8
    assert kept_some and (dropped_some or sims >= 24)


def test_reference_keeps_old_block_order():
    """Kept blocks interleaved with dropped ones keep their relative order, and every new index is <= the old one."""
    from alphaquoridorgnn_amd.engine import keep_subtree_reference
    pool, count = _pool(5, 24)
    root_first, root_cnt = int(pool[0]["kids"]) & 0xFFFFFF, int(pool[0]["kids"]) >> 24
    idx = int(np.argmax(pool[root_first:root_first + root_cnt]["n"]))
    out, cnt, kept = keep_subtree_reference(pool, count, idx, BIG)
    assert kept and cnt < count
    # every kept record, found again by (w, p, action, n): old positions ascend with the new ones and never lie before them
    key = lambda r: (float(r["w"]), float(r["p"]), int(r["action"]), int(r["n"]), int(r["kids"]) >> 24)      # noqa: E731
    pos, last = 0, 0
    for i in range(1, cnt):
        want = key(out[i])
        pos = next(j for j in range(max(pos + 1, i), count) if key(pool[j]) == want)
        assert pos >= i and pos > last
        last = pos


# ------------------------------------------------------------------ the rule's edges
def test_rule_edges():
    from alphaquoridorgnn_amd.engine import keep_subtree_reference
    pool, count = _pool(5, 24)
    first, rcnt = int(pool[0]["kids"]) & 0xFFFFFF, int(pool[0]["kids"]) >> 24
    kids = pool[first:first + rcnt]
    expanded = [i for i in range(rcnt) if int(kids[i]["kids"]) >> 24]
    bare = [i for i in range(rcnt) if not int(kids[i]["kids"]) >> 24]
    assert expanded and bare
    i = expanded[0]
    n = int(kids[i]["n"])
    assert n >= 1
    assert keep_subtree_reference(pool, count, i, n)[2] is True                      # c.n == keep is kept
    assert keep_subtree_reference(pool, count, i, n - 1)[2] is False                 # c.n == keep + 1 is not
    assert keep_subtree_reference(pool, count, bare[0], BIG)[2] is False             # an unexpanded child is not kept
    for j in range(rcnt):                                                            # keep_visits 0 never keeps
        assert keep_subtree_reference(pool, count, j, 0)[2] is False
    for bad in (-1, -7, rcnt, rcnt + 5):                                             # no child named
        out, cnt, kept = keep_subtree_reference(pool, count, bad, BIG)
        assert not kept and cnt == count and out.tobytes() == pool.tobytes()
    # a game that ended is not kept, whatever the child holds
    child = _searched_root(5, 24).children[i]
    assert T.keeps(child, False, n) and not T.keeps(child, True, BIG) and not T.keeps(child, False, n - 1)
    # float64 [cap, 4] -- the engine's tensor -- is taken as it is
    assert keep_subtree_reference(pool.view(np.float64).reshape(-1, 4), count, i, n)[0].tobytes() == keep_subtree_reference(pool, count, i, n)[0].tobytes()


def test_statement_game_keeps_on_some_moves_and_not_on_others():
    from oracle import mcts as om
    u = np.random.RandomState(5).random_sample(64)
    rows, z = T.play_game(5, 16, 6, u)
    flags = [r["kept"] for r in rows]
    assert any(flags) and not all(flags[1:]) and not flags[0]
    for r in rows:
        assert int(r["visits"].sum()) == r["kept_visits"] + 16 - 1 and (r["kept_visits"] > 0) == r["kept"]      # root.n == 1 + the children's
        assert r["kept_visits"] <= 6
    # off: the oracle's own game
    plain, z0 = T.play_game(5, 16, None, u)
    ref = om.play(om.FakeModel(2), 16, N=5, uniforms=list(u))
    assert len(plain) == len(ref) and z0 == ref[0][2]
    assert all(np.allclose(r["visits"] / r["visits"].sum(), pol, rtol=0, atol=1e-15) for r, (_, pol, _) in zip(plain, ref))
    # keep_visits 0: on, never keeps -- the same game
    zero, z1 = T.play_game(5, 16, 0, u)
    assert z1 == z0 and all(a["visits"].tobytes() == b["visits"].tobytes() and a["action"] == b["action"] for a, b in zip(zero, plain))


# ------------------------------------------------------------------ refusals
def test_self_play_engine_refuses():
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay, check_tree_reuse
    for kw in (dict(tree_reuse=True, tree_reuse_visits=-1), dict(tree_reuse=True, tree_reuse_visits=1.5),
               dict(tree_reuse=True, tree_reuse_visits=32767 - 7), dict(tree_reuse=False, tree_reuse_visits=4),
               dict(tree_reuse=True, evaluator="external")):
        with pytest.raises(ValueError, match="tree_reuse"):
            BatchedSelfPlay(None, num_games=2, sims=8, board_size=5, **{"evaluator": "fake", **kw})
    assert check_tree_reuse(False, None, 8) is None
    assert check_tree_reuse(True, None, 8) == 8 and check_tree_reuse(True, 0, 8) == 0 and check_tree_reuse(True, 32759, 8) == 32759
    eng = BatchedSelfPlay.__new__(BatchedSelfPlay)      # search() refuses before it touches anything
    eng.tree_reuse = True
    with pytest.raises(ValueError, match="tree_reuse"):
        eng.search(np.zeros((1, 72), np.uint8))
    with pytest.raises(ValueError, match="tree_reuse"):
        BatchedSelfPlay.tree_reuse_stats(type("E", (), {"tree_reuse": False})())


@pytest.mark.parametrize("opt", [dict(tree_reuse=True), dict(tree_reuse_visits=8), dict(tree_reuse=False)])
def test_matches_and_evaluation_paths_refuse(opt):
    from alphaquoridorgnn_amd import evaluate_agents, evaluate_network, pv_mcts
    word = "never keeps a subtree"
    with pytest.raises(ValueError, match=word):
        evaluate_network.BatchedMatch((0, 1), 2, sims=4, board_size=5, evaluator="fake", **opt)
    with pytest.raises(ValueError, match=word):
        evaluate_agents.BatchedAgentMatch(0, "random", 2, sims=4, board_size=5, evaluator="fake", **opt)
    with pytest.raises(ValueError, match=word):
        pv_mcts.pv_mcts_policy_batch(None, np.zeros((1, 72), np.uint8), 1.0, evaluator="fake", **opt)
    with pytest.raises(ValueError, match=word):
        pv_mcts.pv_mcts_action(None, **opt)
    with pytest.raises(ValueError, match=word):
        evaluate_network.evaluate_network(**opt)
    with pytest.raises(ValueError, match=word):
        evaluate_agents.evaluate_best_player(**opt)


def test_option_defaults_and_flags():
    from alphaquoridorgnn_amd import self_play as sp
    from alphaquoridorgnn_amd.train_cycle import _parser
    assert sp.SP_TREE_REUSE is False and sp.SP_TREE_REUSE_VISITS is None
    args = _parser().parse_args(["--tree-reuse", "--tree-reuse-visits", "40"])
    assert args.tree_reuse is True and args.tree_reuse_visits == 40
    args = _parser().parse_args([])
    assert args.tree_reuse is False and args.tree_reuse_visits is None


# ------------------------------------------------------------------ C ABI
def _structs(sims=8, keep=8, node_cap=None, prior_mode=1):
    from alphaquoridorgnn_amd import _lib
    e = _lib.EngineStructGeneral()
    e.board_size, e.num_games, e.quota, e.sims, e.prior_mode = 5, 4, 4, sims, prior_mode
    e.node_cap = 1 + (sims + max(keep, 0)) * 136 if node_cap is None else node_cap
    for name in ("slot_game", "game_done", "game_slot", "game_first_move"):
        setattr(e, name, 0x1000)
    ru = _lib.TreeReuseStruct()
    ru.keep_visits = keep
    for name in ("kept", "child_index", "stat_moves_kept", "stat_visits_kept"):
        setattr(ru, name, 0x1000)
    return e, ru


def test_abi_is_additive(tmp_path):
    from alphaquoridorgnn_amd import _lib
    assert _lib.ABI_VERSION == 15
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "aqgnn.h"\n'
                   "int main() { std::printf(\"%zu %zu %zu %zu %zu %zu %zu %zu %d\\n\", sizeof(aqg_engine), offsetof(aqg_engine, root_noise),"
                   " sizeof(aqg_tree_reuse), offsetof(aqg_tree_reuse, keep_visits), offsetof(aqg_tree_reuse, kept),"
                   " offsetof(aqg_tree_reuse, child_index), offsetof(aqg_tree_reuse, stat_moves_kept),"
                   " offsetof(aqg_tree_reuse, stat_visits_kept), AQG_ABI_VERSION); }\n")
    exe = tmp_path / "layout"
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    E, R = _lib.EngineStructGeneral, _lib.TreeReuseStruct
    assert got == [ctypes.sizeof(E), E.root_noise.offset, ctypes.sizeof(R), R.keep_visits.offset, R.kept.offset, R.child_index.offset,
                   R.stat_moves_kept.offset, R.stat_visits_kept.offset, 15]
    assert ctypes.sizeof(E) == E.root_noise.offset + 8                 # root_noise is still the struct's last field
    header = open(os.path.join(REPO, "include", "aqgnn.h")).read()
    assert "tree reuse (additive to ABI 15" in header
    for name in ("aqg_engine_move_reuse", "aqg_engine_finish_move_reuse", "aqg_engine_keep_subtrees", "aqg_engine_reset_reuse"):
        assert name in _lib.SIGNATURES and f"int {name}(" in header
    for old in ("aqg_engine_move", "aqg_engine_move_targets", "aqg_engine_finish_move", "aqg_engine_finish_move_targets"):
        assert old in _lib.SIGNATURES and f"int {old}(" in header


@pytest.mark.parametrize("kw,word", [(dict(keep=-1), "keep_visits must be >= 0"), (dict(sims=8, keep=32760), "32767"),
                                     (dict(node_cap=1 + 16 * 136 - 1), "node_cap"), (dict(prior_mode=2), "prior_mode 2")])
def test_library_refuses_before_any_launch(kw, word):
    from alphaquoridorgnn_amd import _lib
    lib = _lib.load()
    u = ctypes.c_void_p(0x1000)
    e, ru = _structs(**kw)
    calls = (lambda: lib.aqg_engine_move_reuse(ctypes.byref(e), u, 0, None, ctypes.byref(ru), None),
             lambda: lib.aqg_engine_finish_move_reuse(ctypes.byref(e), u, 0, None, ctypes.byref(ru), None),
             lambda: lib.aqg_engine_keep_subtrees(ctypes.byref(e), ctypes.byref(ru), u, None),
             lambda: lib.aqg_engine_reset_reuse(ctypes.byref(e), ctypes.byref(ru), None))
    for call in calls:
        assert call() != 0 and word in lib.aqg_last_error().decode()
    e, ru = _structs()
    ru.kept = None
    assert lib.aqg_engine_keep_subtrees(ctypes.byref(e), ctypes.byref(ru), u, None) != 0 and "required" in lib.aqg_last_error().decode()
    assert lib.aqg_engine_move_reuse(ctypes.byref(e), u, 0, None, None, None) != 0
