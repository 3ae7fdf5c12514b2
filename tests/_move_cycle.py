"""Shared by tests/test_move_cycle_cpu.py and tests/test_move_cycle.py: host statements of the two kernels that end every self-play
move (csrc/mcts_move.hip engine_finish_move_kernel and engine_refill_kernel) and the inputs that put them at their edges.  No torch.

finish_move_reference is the move's choice as the reference makes it: the first maximum of the visit counts, or np.random.choice over
boltzman(n, T) for one uniform.  At T == 1 the device's arithmetic is the statement's -- the same IEEE additions and divisions in the
same order -- so a uniform that EQUALS a cdf value is a meaningful input there; at any other T the two evaluate pow with different
libraries, and every uniform is kept MARGIN away from every cdf value (two correct pows differ by a few ulp, over 136 terms far below
1e-13).  Where a child's cdf interval is too narrow for that (n = 1 beside n = 32767 at T = 0.5: 9.3e-10 wide) its midpoint is not
used; the builders assert the margin of every uniform they emit.

refill_reference is the slot refill as the kernel's header comment states it: after every move the idle slots take the next game
indices in slot order while they are below the quota, the rest are retired."""
import numpy as np

from tests._improved_policy import walked_records

MAX_LEGAL = 136
U_TOP = 1.0 - 2.0 ** -53          # the largest double below 1
MARGIN = 1e-9
COUNTS = (1, 2, 63, 64, 65, 127, 128, 129, None)      # root child counts: the lane-round edges, None = the whole legal list
TEMPERATURES = (0.5, 2.0, 0.25)


# ---------------------------------------------------------------------------------------------- A. the choice of a move
def boltzman(xs, temperature):
    """pv_mcts.py:106-109, as written there."""
    xs = [x ** (1 / temperature) for x in xs]
    return [x / sum(xs) for x in xs]


def cdf_values(n, temperature):
    """The cdf np.random.choice searches: cumsum(p), divided by its last entry."""
    cdf = np.cumsum(np.asarray(boltzman([int(x) for x in n], temperature), dtype=np.float64))
    cdf /= cdf[-1]
    return cdf


def finish_move_reference(n, actions, w_root, n_root, temperature, temperature_plies, plies_played, u):
    """(index, action, f32 search value) of one searched move: n the root's child visit counts in legal order, actions their action
    ids, w_root / n_root the root's own sums.  temperature is the value the engine holds (a float32, widened)."""
    from oracle.mcts import choice_index
    n = [int(x) for x in n]
    late = temperature_plies > 0 and plies_played >= temperature_plies
    if temperature == 0 or late:
        idx = 0
        for i, x in enumerate(n):
            if x > n[idx]:
                idx = i
    else:
        idx = choice_index(boltzman(n, temperature), u)
        assert idx < len(n), "u must be below 1"
    value = np.float32(float(w_root) / int(n_root)) if n_root else np.float32(0.0)
    return idx, int(actions[idx]), value


def transition_reference(rec, action):
    """What engine_transition leaves behind a legal move: (next record, done, z of ply 0)."""
    from oracle import quoridor as oq
    t = oq.State(oq.next_record(rec, int(action)))
    if t.is_lose():
        return t.rec, 1, (-1 if t.plies_played % 2 == 0 else 1)
    return t.rec, int(t.is_draw()), 0


def single(cnt, pos, visits=7):
    n = np.zeros(cnt, dtype=np.int32)
    n[pos] = visits
    return n


def separated(cnt, seed):
    """Visited children -- single ones and a run of two -- between runs of unvisited ones, child 0 and the last child unvisited, with a
    visited child at every lane-round edge the count has."""
    assert cnt >= 3
    rng = np.random.RandomState(seed)
    at = sorted({i for i in (1, 2, 5, 62, 63, 64, 65, 100, 126, 127, 128, cnt - 2) if 0 < i < cnt - 1})
    n = np.zeros(cnt, dtype=np.int32)
    n[at] = rng.randint(1, 10, len(at))
    return n


def tie_of_three(cnt, seed):
    """The maximum 9 in three children, the first of them not child 0 where the count allows it; half of the others unvisited."""
    assert cnt >= 3
    rng = np.random.RandomState(seed)
    n = rng.randint(0, 6, cnt).astype(np.int32)
    n[rng.rand(cnt) < 0.5] = 0
    at = (0, 1, 2) if cnt == 3 else (max(1, cnt // 3), cnt // 2 + 1, cnt - 1)
    assert len(set(at)) == 3
    n[list(at)] = 9
    return n, at[0]


def maximum_last(cnt, seed):
    rng = np.random.RandomState(seed)
    n = rng.randint(0, 6, cnt).astype(np.int32)
    n[cnt - 1] = 9
    return n


def big_beside_ones(cnt):
    assert cnt >= 2
    n = np.ones(cnt, dtype=np.int32)
    n[cnt // 2] = 32767
    return n


def random_half_zero(cnt, seed, nmax=30):
    rng = np.random.RandomState(seed)
    n = rng.randint(1, nmax + 1, cnt).astype(np.int32)
    n[rng.rand(cnt) < 0.5] = 0
    if not n.any():
        n[rng.randint(cnt)] = nmax
    return n


def boundary_uniforms(n, limit=None, seed=0):
    """T == 1: for every distinct cdf value c (at most `limit` of them, drawn) u = c and u = nextafter(c, 0) -- c = 0 (unvisited children
    in front) only as u = 0, c = 1 only as the largest double below it."""
    cdf = cdf_values(n, 1.0)
    values = np.unique(cdf)
    if limit is not None and len(values) > limit:
        keep = np.random.RandomState(seed).choice(len(values) - 2, limit - 2, replace=False) + 1
        values = np.concatenate([values[:1], values[np.sort(keep)], values[-1:]])
    us = []
    for c in values:
        if c < 1.0:
            us.append(float(c))
        if c > 0.0:
            us.append(float(np.nextafter(c, 0.0)))
    return us


def midpoint_uniforms(n, temperature):
    """The midpoint of every visited child's cdf interval that lies MARGIN away from every cdf value."""
    cdf = cdf_values(n, temperature)
    us = []
    for i in np.flatnonzero(np.asarray(n) > 0):
        u = 0.5 * ((cdf[i - 1] if i else 0.0) + cdf[i])
        if np.abs(cdf - u).min() >= MARGIN:
            us.append(float(u))
    assert us and all(0.0 <= u < 1.0 and np.abs(cdf - u).min() >= MARGIN for u in us)
    return us


def legal_count(rec):
    from oracle import quoridor as oq
    return len(oq.legal_actions(rec))


_ROOTS = {}


def real_roots(N):
    """Named real positions of one board: the opening, a short walk from it, and the special ones the patterns need."""
    from oracle import quoridor as oq
    if N in _ROOTS:
        return _ROOTS[N]
    walk = walked_records(N, 24, seed=40 + N)
    roots = {"opening": oq.init_record(N)}
    step = min(a for a in oq.legal_actions(roots["opening"]) if a < N * N)
    roots["later"] = oq.next_record(roots["opening"], step)               # plies_played 1 behind a pawn step: every wall is still legal
    roots["walk"] = [r for r in walk[1:6]]
    if N == 3:
        roots["no_walls"] = next(r for r in walk if r[1] == 0 and oq.State(r).plies_played >= 1)
        assert all(a < N * N for a in oq.legal_actions(roots["no_walls"]))
        roots["one_step"], roots["one_step_child"] = one_step_from_goal(N)
    _ROOTS[N] = roots
    return roots


def one_step_from_goal(N):
    """(record, child index) of a position whose mover reaches the goal row with that child: the first one a seeded walk meets."""
    from oracle import quoridor as oq
    rng = np.random.RandomState(7)
    for _ in range(200):
        state = oq.State(N=N)
        while not state.is_done():
            legal = state.legal_actions()
            for i, a in enumerate(legal):
                if state.next(a).is_lose():
                    return state.rec.copy(), i
            state = state.next(int(legal[rng.randint(len(legal))]))
    raise AssertionError("no position one step from the goal")


def case(name, root, cnt, n, us, seed=0):
    """One root for one slot: its record, the child count to narrow to (<= the real one), the visit counts, consistent sums, and the
    uniforms to launch with in turn."""
    real = legal_count(root)
    cnt = real if cnt is None else cnt
    n = np.asarray(n, dtype=np.int32)
    assert 1 <= cnt <= real and n.shape == (cnt,) and (n >= 0).all() and (n <= 32767).all()
    rng = np.random.RandomState(1000 + seed)
    value = rng.uniform(-1, 1, cnt)
    w = np.where(n > 0, -value * n, 0.0)
    q = np.where(n > 0, -w / np.maximum(n, 1), 0.0).astype(np.float32)
    n_root = 1 + int(n.astype(np.int64).sum())
    return dict(name=name, root=np.asarray(root, dtype=np.uint8), cnt=cnt, n=n, w=w, q=q, n_root=n_root,
                w_root=float(rng.uniform(-1, 1)) * n_root, us=[float(u) for u in us])


def _counts(root, least=1):
    real = legal_count(root)
    return [c for c in COUNTS if (c is None and real >= least) or (c is not None and least <= c <= real)]


def sampling_cases():
    """T == 1 on the 9x9 opening root's prefixes and on real roots: what decides acc / last <= u at equality."""
    root = real_roots(9)["opening"]
    assert legal_count(root) == 131
    out = []
    for k, cnt in enumerate(_counts(root)):
        c = legal_count(root) if cnt is None else cnt
        for pos in sorted({0, c // 2, c - 1}):
            out.append(case(f"single{pos}/{c}", root, cnt, single(c, pos), (0.0, 0.5, U_TOP), seed=k))
        if c >= 3:
            n = separated(c, seed=k)
            out.append(case(f"separated/{c}", root, cnt, n, boundary_uniforms(n), seed=k))
        if c >= 2:
            n = big_beside_ones(c)
            cdf = cdf_values(n, 1.0)
            around = [cdf[c // 2 - 1], cdf[c // 2]] if c // 2 else [cdf[0]]
            us = [0.0, U_TOP] + [float(x) for v in around for x in (v, np.nextafter(v, 0.0)) if x < 1.0]
            out.append(case(f"big/{c}", root, cnt, n, us, seed=k))
        n = random_half_zero(c, seed=k)
        out.append(case(f"random/{c}", root, cnt, n, boundary_uniforms(n, limit=8, seed=k) + midpoint_uniforms(n, 1.0)[:4], seed=k))
    return out


def real_root_cases(N):
    """T == 1 on real positions of one board at their own child counts."""
    roots = real_roots(N)
    named = [("later", roots["later"])] + [(f"walk{i}", r) for i, r in enumerate(roots["walk"])]
    if N == 3:
        named.append(("no_walls", roots["no_walls"]))
    out = []
    for k, (name, root) in enumerate(named):
        c = legal_count(root)
        n = random_half_zero(c, seed=50 + k)
        out.append(case(f"{name}/random", root, None, n, boundary_uniforms(n, limit=8, seed=k), seed=k))
        out.append(case(f"{name}/last", root, None, single(c, c - 1), (0.0, 0.5, U_TOP), seed=k))
    if N == 3:
        c = legal_count(roots["one_step"])
        out.append(case("one_step", roots["one_step"], None, single(c, roots["one_step_child"]), (0.0, 0.5, U_TOP)))
    return out


def first_maximum_cases():
    """A tied maximum and a maximum in the last child, on a root at ply 0 and on one at ply >= 1: for an engine at T = 0 (both take the
    first maximum) and for one at T = 1 with temperature_plies = 1 (ply 0 samples -- U_TOP then picks the last visited child)."""
    roots = real_roots(9)
    out = []
    for name in ("opening", "later"):
        root = roots[name]
        for k, cnt in enumerate(_counts(root, least=2)):
            c = legal_count(root) if cnt is None else cnt
            if c >= 3:
                out.append(case(f"{name}/tie/{c}", root, cnt, tie_of_three(c, seed=k)[0], (0.0, 0.3, U_TOP), seed=k))
            out.append(case(f"{name}/last/{c}", root, cnt, maximum_last(c, seed=k), (0.0, 0.3, U_TOP), seed=k))
    return out


def temperature_cases(temperature, nmax=30, big=True):
    """T != 1 on the 9x9 opening root's prefixes: the random and the 32767 patterns with every usable midpoint."""
    root = real_roots(9)["opening"]
    out = []
    for k, cnt in enumerate(_counts(root)):
        c = legal_count(root) if cnt is None else cnt
        n = random_half_zero(c, seed=70 + k, nmax=nmax)
        out.append(case(f"random/{c}", root, cnt, n, midpoint_uniforms(n, temperature), seed=k))
        if big and c >= 2:
            n = big_beside_ones(c)
            out.append(case(f"big/{c}", root, cnt, n, midpoint_uniforms(n, temperature), seed=k))
    return out


# ---------------------------------------------------------------------------------------------- B. the slot refill
class RefillState:
    """The engine's slot and game tables on the host.  move(ended) ends the game of every ACTIVE slot in `ended` as a dead-end draw and
    then refills, as aqg_engine_apply_actions does with action -1 in those slots and an action >= A everywhere else."""

    def __init__(self, G, Q):
        assert Q >= G >= 1
        self.G, self.Q = G, Q
        self.slot_game = np.arange(G, dtype=np.int32)
        self.game_active = np.ones(G, dtype=np.uint8)
        self.game_slot = np.where(np.arange(Q) < G, np.arange(Q), -1).astype(np.int32)
        self.game_first_move = np.zeros(Q, dtype=np.int32)
        self.game_done = np.zeros(Q, dtype=np.uint8)
        self.active, self.finished, self.dead_ends, self.started, self.moves = G, 0, 0, G, 0
        self.refilled = np.zeros(G, dtype=bool)

    def move(self, ended):
        ended = [int(s) for s in sorted(set(int(s) for s in ended)) if self.game_active[int(s)]]
        for s in ended:
            self.game_done[self.slot_game[s]] = 1
            self.game_active[s] = 0
        self.active -= len(ended)
        self.finished += len(ended)
        self.dead_ends += len(ended)
        self.refilled = np.zeros(self.G, dtype=bool)
        if self.Q > self.G:                                   # the refill launch
            self.moves += 1
            idle = [s for s in range(self.G) if not self.game_active[s] and self.slot_game[s] >= 0]
            for i, s in enumerate(idle):                      # in slot order
                k = self.started + i
                if k < self.Q:
                    self.slot_game[s], self.game_slot[k], self.game_first_move[k] = k, s, self.moves
                    self.game_active[s], self.refilled[s] = 1, True
                    self.active += 1
                else:
                    self.slot_game[s] = -1                    # retired
            self.started = min(self.started + len(idle), self.Q)
        return self.snapshot()

    def snapshot(self):
        return dict(slot_game=self.slot_game.copy(), game_active=self.game_active.copy(), game_slot=self.game_slot.copy(),
                    game_first_move=self.game_first_move.copy(), game_done=self.game_done.copy(), refilled=self.refilled.copy(),
                    counters=(self.active, self.finished, self.dead_ends, self.started, self.moves))


def refill_reference(G, Q, end_sets):
    """The tables and counters after every move of the script: a list of snapshots."""
    state = RefillState(G, Q)
    return [state.move(ended) for ended in end_sets]


def end_sets_from_lengths(G, Q, lengths):
    """The script a generation of searched games plays: game k ends `lengths[k]` moves after its first."""
    state, out = RefillState(G, Q), []
    while state.active:
        ended = [s for s in range(G) if state.game_active[s]
                 and state.moves + 1 - state.game_first_move[state.slot_game[s]] == lengths[state.slot_game[s]]]
        out.append(ended)
        state.move(ended)
        assert len(out) <= int(np.sum(lengths))
    return out


REFILL_SLOTS = (1, 63, 64, 65, 1024, 1025, 2300)


def plain_scripts(G):
    """(name, end sets) of the scripts that never meet the quota; plain_quota(G) games are enough for each."""
    rng = np.random.RandomState(G)
    every = list(range(G))
    half = sorted(set(rng.choice(G, (G + 1) // 2, replace=False).tolist()) | {G - 1})        # (the last wave may hold the last slot alone)
    out = [("all_twice", [every, every]),
           ("lane63_then_lane0", [[s for s in every if s % 64 == 63], [s for s in every if s % 64 == 0]]),
           ("last_slot", [[G - 1]]),
           ("random_half_then_1pct", [half, sorted(rng.choice(G, max(1, G // 100), replace=False).tolist())])]
    if G >= 1025:
        out.append(("1023_and_1024", [[1023, 1024]]))
    return out


def plain_quota(G):
    return 3 * G + 5


def cut_scripts(G):
    """(name, Q, end sets, first retired slot or None) of the quota cuts: a first move ends 1 % of the slots (all of them are
    refilled), the second ends a random half, of which only the first r find a game left; Q = G + |first| + r.  A third move ends a
    few active and a few retired slots."""
    rng = np.random.RandomState(100 + G)
    first = sorted(rng.choice(G, max(1, G // 100), replace=False).tolist())
    half = np.sort(rng.choice(G, (G + 1) // 2, replace=False))
    for s in (G - 1, 1024) if G > 1024 else (G - 1,):                            # the last slot and the second chunk's first one are idle
        half = np.union1d(half, [s])
    half = half.astype(int).tolist()
    out = []

    def add(name, r):
        busy = [s for s in range(G) if s not in set(half)]                       # active whatever the cut
        after = sorted(set(rng.choice(G, max(1, G // 50), replace=False).tolist()) | set(half[r:r + 3]) | set(half[:2]) | set(busy[-2:]))
        out.append((name, G + len(first) + r, [first, half, after], half[r] if r < len(half) else None))

    inside = [r for r in range(1, len(half)) if half[r] % 64 not in (0, 63) and half[r] // 64 == half[r - 1] // 64
              and (G < 128 or half[r] >= 64) and half[r] < 1024]
    if inside:
        add("cut_inside_a_wave", inside[len(inside) // 2])
    edge = [r for r in range(1, len(half)) if half[r] // 64 > half[r - 1] // 64 and half[r] < 1024]
    if edge:
        add("cut_at_a_wave_boundary", edge[len(edge) // 2])
    if G >= 1025:
        second = [r for r in range(1, len(half)) if half[r] >= 1024 and (half[r - 1] >= 1024 or G == 1025)]
        add("cut_inside_the_second_chunk", second[len(second) // 2])
    add("cut_with_no_game_left", 0)
    return out
