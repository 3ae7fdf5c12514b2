"""Shared by tests/test_improved_policy_cpu.py and tests/test_improved_policy.py: the completed-Q improved policy written out in plain
python floats (independently of engine.improved_policy_reference), the tolerances of include/aqgnn.h "completed-Q policy targets",
synthetic tree pools with every edge the read-out names, and policy rows with every edge the refresh form names.

The tolerances are derived, not measured.  Every float64 intermediate of the definition is good to far better than 2^-40 relative
(a handful of roundings of 2^-53 each, times at most MAX_LEGAL terms, times the transform's scale: well below 2^-23 even at
nmax = 32767), so two evaluations can differ in an f32 OUTPUT only by landing on either side of a rounding boundary:
    pi':   |a - b| <= 2^-23 |b|                                            (one f32 ulp)
    vmix:  |a - b| <= 2^-23 |b| + (cnt + 1) (Nsum + 1) 2^-53
The second term is the absolute floor for the cancellation in vhat = root.w + sum w_i: |w_i| <= n_i and |root.w| <= Nsum + 1, so
every partial sum is at most 2 Nsum + 1 and each of the at most min(cnt, Nsum) inexact additions errs by at most 2^-53 (2 Nsum + 1);
two evaluation orders differ by at most twice that, and vmix divides vhat by 1 + Nsum: 4 min(cnt, Nsum) 2^-53 <= (cnt + 1)(Nsum + 1)
2^-53."""
import math

import numpy as np

from tests._reanalyse import MAX_LEGAL, policy_size, search_rows

ULP = 2.0 ** -23


def paper_policy(p, n, q, w, root_w, c_visit=50.0, c_scale=1.0):
    """Danihelka et al. (ICLR 2022), section 4 and appendix D, in python floats, one child at a time: (pi' list[float], vmix float)."""
    cnt = len(p)
    p, q, w = [float(x) for x in p], [float(x) for x in q], [float(x) for x in w]
    n = [int(x) for x in n]
    nsum, nmax = 0, 0
    for x in n:
        nsum += x
        nmax = max(nmax, x)
    vhat = float(root_w)
    for x in w:
        vhat += x
    pv = qv = 0.0
    for i in range(cnt):
        if n[i] > 0:
            pv += p[i]
            qv += p[i] * q[i]
    vmix = (vhat + nsum * (qv / pv)) / (1 + nsum) if pv > 0 else vhat
    logits = []
    for i in range(cnt):
        completed = q[i] if n[i] > 0 else vmix
        sigma = (c_visit + nmax) * c_scale * ((completed + 1.0) / 2.0)
        logits.append(math.log(p[i]) + sigma if p[i] > 0 else None)
    live = [x for x in logits if x is not None]
    if not live:
        return [0.0] * cnt, vmix
    top = max(live)
    e = [0.0 if x is None else math.exp(x - top) for x in logits]
    total = 0.0
    for x in e:
        total += x
    return [x / total for x in e], vmix


def pi_close(got, want):
    """|got - want| <= one f32 ulp of want, entry by entry (both as float64)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return bool((np.abs(got - want) <= ULP * np.abs(want)).all())


def vmix_bound(want, cnt, nsum):
    return ULP * abs(float(want)) + (int(cnt) + 1) * (int(nsum) + 1) * 2.0 ** -53


def vmix_close(got, want, cnt, nsum):
    return abs(float(got) - float(want)) <= vmix_bound(want, cnt, nsum)


def oracle_children(root):
    """(p f32, n i32, q f32, w f64, root_w) of an oracle search tree's root, as the engine's records hold them."""
    kids = root.children or []
    p = np.array([np.float32(c.p) for c in kids], dtype=np.float32)
    n = np.array([c.n for c in kids], dtype=np.int32)
    w = np.array([float(c.w) for c in kids], dtype=np.float64)
    q = np.array([np.float32(-c.w / c.n) if c.n else np.float32(0.0) for c in kids], dtype=np.float32)
    return p, n, q, w, float(root.w)


# ---- synthetic pools (GPU test (a)): one root and its child block, with the patterns the issue names
COUNTS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 136)          # the lane-round edges
PATTERNS = ("none_visited", "all_visited", "zero_prior_visited", "tiny_priors", "q_extremes", "big_n", "mixed")


def synthetic_pool(node_dtype, cap, cnt, pattern, seed, first=None):
    """A pool of `cap` records: random bytes everywhere, then node 0 and its `cnt` children at `first` (default: somewhere inside).
    Returns the pool; the children's fields are consistent with a search (q = f32(-w / n), |w| <= n) except where a pattern says."""
    rng = np.random.RandomState(seed)
    pool = np.frombuffer(rng.bytes(32 * cap), dtype=node_dtype).copy()
    pool["w"] = rng.uniform(-3, 3, cap)                        # no NaN among the bytes a guard failure would show
    if first is None:
        first = 1 + int(rng.randint(0, cap - cnt))             # first + cnt <= cap
    p = rng.dirichlet(np.full(max(cnt, 1), 0.3))[:cnt].astype(np.float32) if cnt else np.zeros(0, np.float32)
    n = rng.randint(0, 6, cnt).astype(np.int32)
    n[rng.rand(cnt) < 0.5] = 0
    if pattern == "none_visited":
        n[:] = 0
    elif pattern == "all_visited":
        n = np.maximum(n, 1)
    elif pattern == "zero_prior_visited":                      # PV == 0: only children without a prior are visited
        zero = rng.rand(cnt) < 0.4
        if cnt:
            zero[0] = True
        p[zero] = 0
        n = np.where(zero, np.maximum(n, 1), 0).astype(np.int32)
    elif pattern == "tiny_priors":
        p[rng.rand(cnt) < 0.3] = 0
        p[rng.rand(cnt) < 0.3] = np.float32(1e-38)
    elif pattern == "big_n":                                   # the transform's scale is 32817: every other entry underflows to 0
        if cnt:
            n[int(rng.randint(cnt))] = 32767
    value = rng.uniform(-1, 1, cnt)
    if pattern == "q_extremes":
        n = np.maximum(n, (rng.rand(cnt) < 0.7).astype(np.int32))
        value = rng.choice([-1.0, 1.0], cnt)
    if pattern == "big_n" and cnt:
        value[n == 32767] = 1.0
    w = np.where(n > 0, -value * n, 0.0)
    q = np.where(n > 0, (-w / np.maximum(n, 1)).astype(np.float32), np.float32(0)).astype(np.float32)
    pool["kids"][0] = np.uint32((first & 0xFFFFFF) | (cnt << 24))
    pool["n"][0] = 1 + int(n.sum())
    pool["w"][0] = float(rng.uniform(-1, 1)) - float(w.sum())   # vhat in [-1, 1]
    stop = min(first + cnt, cap)                               # (a range past the pool: the records that exist)
    k = stop - first
    if k > 0:
        blk = pool[first:stop]
        blk["p"], blk["n"], blk["q"], blk["w"] = p[:k], n[:k], q[:k], w[:k]
        blk["action"] = rng.permutation(209)[:cnt][:k].astype(np.uint32)
        blk["kids"] = 0
    return pool


# ---- policy rows (the refresh form): search_rows' layout with f32 entries, and the special rows of both
POLICY_SPECIAL = ("count0", "count1", "count136", "zero_row", "big_action", "slot_above", "slot_below", "count_negative", "count137",
                  "nan_entry", "inf_entry", "negative_entry")


def policy_rows(N, n, seed, capacity):
    """(policy f32 [n,136], actions u8, count i32, search_value f32, slots i64, kinds): improved-policy-like rows in legal order -- zeros,
    denormals and a -0.0 among the entries -- with garbage bits behind the count, and every row of POLICY_SPECIAL behind row 0 when
    n is large enough."""
    visits, actions, count, q, slots, _ = search_rows(N, n, seed, capacity)
    rng = np.random.RandomState(seed + 1)
    kinds = ["plain"] * n
    if n > len(POLICY_SPECIAL):
        kinds[1:1 + len(POLICY_SPECIAL)] = POLICY_SPECIAL
    A = policy_size(N)
    policy = rng.randint(0, 2 ** 32, (n, MAX_LEGAL), dtype=np.uint64).astype(np.uint32).view(np.float32).copy()     # garbage everywhere
    for i, kind in enumerate(kinds):
        c = {"count0": 0, "count1": 1, "count136": MAX_LEGAL, "count_negative": -3, "count137": MAX_LEGAL + 1}.get(
            kind, int(rng.randint(2, min(A, MAX_LEGAL) + 1)))
        count[i] = c
        k = max(0, min(c, MAX_LEGAL))
        actions[i, :k] = rng.permutation(max(A, k))[:k]
        row = rng.dirichlet(np.full(max(k, 1), 0.2))[:k].astype(np.float32)
        row[rng.rand(k) < 0.3] = 0
        if k:
            row[rng.randint(k)] = np.float32(0.25)             # an ordinary row has an entry above 0
        if k > 3:
            row[1], row[2] = np.float32(1e-42), np.float32(-0.0)          # a denormal and a negative zero are copied as they are
        if kind == "zero_row":
            row[:] = 0
        if kind == "big_action":
            actions[i, rng.randint(k)] = A if A < 256 else 255
            actions[i, (rng.randint(k - 1) + 1) % k] = 255
        if kind == "slot_above":
            slots[i] = capacity + 3
        if kind == "slot_below":
            slots[i] = -1
        if kind in ("nan_entry", "inf_entry", "negative_entry"):
            row[rng.randint(k)] = {"nan_entry": np.float32("nan"), "inf_entry": np.float32("inf"), "negative_entry": np.float32(-1e-30)}[kind]
        policy[i, :k] = row
    return policy, actions, count, q, slots, kinds


def policy_written_rows(policy, count, slots, capacity):
    """Source rows the refresh form writes, from the issue's statement."""
    out = np.zeros(len(count), dtype=bool)
    for i, c in enumerate(count):
        if not 1 <= c <= MAX_LEGAL or not 0 <= slots[i] < capacity:
            continue
        ok, some = True, False
        for x in policy[i, :c]:
            x = float(x)
            ok = ok and math.isfinite(x) and x >= 0
            some = some or x > 0
        out[i] = ok and some
    return out


def expected_refresh_policy(N, policy, actions, count, q, blend, slots, rings):
    """The rings after the launch, written out entry by entry: new arrays."""
    from alphaquoridorgnn_amd.replay import blend_targets
    A = policy_size(N)
    r72, rpi, rz = (x.copy() for x in rings)
    for i in np.flatnonzero(policy_written_rows(policy, count, slots, rpi.shape[0])):
        row = np.zeros((A,), dtype=np.float32)
        for j in range(int(count[i])):
            if actions[i, j] < A:
                row[actions[i, j]] = policy[i, j]
        rpi[slots[i]] = row
        if q is not None and blend != 0.0:
            rz[slots[i]] = blend_targets(rz[slots[i]:slots[i] + 1], q[i:i + 1], blend)[0]
    return r72, rpi, rz


class OracleEngine:
    """What reanalyse() asks of a search engine, on the host: the oracle's PV-MCTS with FakeModel per root, read out through the
    package's references -- the stage's chunking, padding and slot mapping can then be held to a host statement without a GPU."""

    def __init__(self, N, G, sims, bias):
        import torch
        self.N, self.G, self.sims, self.bias, self.dev = N, G, sims, bias, torch.device("cpu")
        self.searches = 0

    def search(self, roots):
        import torch
        from oracle import mcts as om, quoridor as oq
        assert tuple(roots.shape) == (self.G, 72)
        self.searches += 1
        self.roots = [om.search(om.FakeModel(self.bias), oq.State(rec), self.sims) for rec in roots.numpy()]
        visits = np.zeros((self.G, MAX_LEGAL), dtype=np.int32)
        self.actions = np.full((self.G, MAX_LEGAL), 0xFF, dtype=np.uint8)
        self.count = np.zeros((self.G,), dtype=np.int32)
        for g, root in enumerate(self.roots):
            legal = list(root.state.legal_actions())
            self.count[g] = len(legal)
            visits[g, :len(legal)], self.actions[g, :len(legal)] = [c.n for c in root.children], legal
        return torch.from_numpy(visits), torch.from_numpy(self.actions.copy()), torch.from_numpy(self.count.copy())

    def root_values(self):
        import torch
        return torch.from_numpy(np.array([np.float32(r.w / r.n) for r in self.roots], dtype=np.float32))

    def root_improved_policy(self, c_visit=50.0, c_scale=1.0):
        import torch
        from alphaquoridorgnn_amd.engine import improved_policy_reference
        policy, vmix = np.zeros((self.G, MAX_LEGAL), dtype=np.float32), np.zeros((self.G,), dtype=np.float32)
        for g, root in enumerate(self.roots):
            policy[g, :self.count[g]], vmix[g] = improved_policy_reference(*oracle_children(root), c_visit, c_scale)
        return torch.from_numpy(policy), torch.from_numpy(self.actions.copy()), torch.from_numpy(self.count.copy()), torch.from_numpy(vmix)


def walked_records(N, n, seed):
    """n records of real positions: random walks from the initial position with the oracle's rules (no finished position)."""
    from oracle import quoridor as oq
    rng = np.random.RandomState(seed)
    out, state = [], oq.State(N=N)
    while len(out) < n:
        if state.is_done() or state.plies_played >= 12:
            state = oq.State(N=N)
        out.append(np.array(state.rec, dtype=np.uint8).copy())
        legal = state.legal_actions()
        state = state.next(int(legal[rng.randint(len(legal))]))
    return np.stack(out)
