"""Shared by tests/test_reanalyse_cpu.py and tests/test_reanalyse.py: searched roots as engine.search returns them with every edge
the refresh launch names, rings pre-filled with random bits, and the expectation of a refresh written out independently of
replay.refresh_reference."""
import numpy as np

MAX_LEGAL = 136
# the special rows, placed at source rows 1 .. len(SPECIAL) of a set that is large enough (row 0 stays an ordinary row)
SPECIAL = ("count0", "count1", "count136", "zero_visits", "big_action", "slot_above", "slot_below", "count_negative", "count137")


def policy_size(N):
    return N * N + 2 * (N - 1) ** 2


def bits(x):
    return x.view(np.int32) if x.dtype == np.float32 else x


def kinds_of(n):
    """The kind of every source row of a set of n rows: all of SPECIAL when they fit behind row 0, else ordinary rows only."""
    kinds = ["plain"] * n
    if n > len(SPECIAL):
        kinds[1:1 + len(SPECIAL)] = SPECIAL
    return kinds


def search_rows(N, n, seed, capacity, top=60000):
    """(visits i32 [n,136], actions u8 [n,136], count i32 [n], search_value f32 [n], slots i64 [n], kinds): legal-order counts with
    distinct action ids, garbage behind the count (the launch must mask by the count, not by what lies there), slots scattered over
    the ring with slot 0 and slot capacity - 1 named (n >= 2), and the rows of SPECIAL.  Totals stay below 2^24."""
    assert top * MAX_LEGAL < 2 ** 24 and capacity >= n
    rng = np.random.RandomState(seed)
    A = policy_size(N)
    kinds = kinds_of(n)
    visits = rng.randint(0, top + 1, (n, MAX_LEGAL)).astype(np.int32)
    actions = rng.randint(0, 256, (n, MAX_LEGAL)).astype(np.uint8)
    count = np.zeros((n,), dtype=np.int32)
    slots = rng.permutation(capacity)[:n].astype(np.int64)
    if n >= 2:                                                  # slot 0 and the last slot are named, by ordinary rows where possible
        for want, i in ((0, 0), (capacity - 1, n - 1)):
            if want in slots:
                slots[np.flatnonzero(slots == want)[0]] = slots[i]
            slots[i] = want
    for i, kind in enumerate(kinds):
        c = {"count0": 0, "count1": 1, "count136": MAX_LEGAL, "count_negative": -3, "count137": MAX_LEGAL + 1}.get(
            kind, int(rng.randint(2, min(A, MAX_LEGAL) + 1)))
        count[i] = c
        k = max(0, min(c, MAX_LEGAL))
        # distinct ids: of the board where they fit, else (136 ids on a board with fewer actions) bytes of which some are >= A
        actions[i, :k] = rng.permutation(max(A, k))[:k]
        if rng.rand() < 0.5:
            visits[i, :k] = np.minimum(visits[i, :k], rng.randint(1, 40))              # the sums a real search gives, too
        visits[i, :k][rng.rand(k) < 0.3] = 0
        if k:
            visits[i, rng.randint(k)] = max(1, visits[i, 0])                          # an ordinary row has a visit
        if kind == "zero_visits":
            visits[i, :k] = 0
        if kind == "big_action":
            actions[i, rng.randint(k)] = A if A < 256 else 255                        # A <= 209: a byte >= policy_size
            actions[i, (rng.randint(k - 1) + 1) % k] = 255
        if kind == "slot_above":
            slots[i] = capacity + 3
        if kind == "slot_below":
            slots[i] = -1
    q = (rng.randint(-32768, 32768, n) / 32768.0).astype(np.float32)
    return visits, actions, count, q, slots, kinds


def random_rings(N, capacity, seed):
    """(ring72, ring_pi, ring_z) of random bits -- NaNs and infinities among the policy floats; the value ring finite, since a blend
    computes with what it holds."""
    rng = np.random.RandomState(seed)
    r72 = rng.randint(0, 256, (capacity, 72)).astype(np.uint8)
    rpi = rng.randint(0, 2 ** 32, (capacity, policy_size(N)), dtype=np.uint64).astype(np.uint32).view(np.float32)
    rz = rng.randint(0, 2 ** 32, (capacity,), dtype=np.uint64).astype(np.uint32)
    rz[(rz & 0x7F800000) == 0x7F800000] &= np.uint32(0xBFFFFFFF)          # exponent all ones -> finite
    return r72, rpi, rz.view(np.float32)


def written_rows(N, visits, count, slots, capacity):
    """Source rows the launch writes: 1 <= count <= 136, a visit among the first `count`, a slot of the ring."""
    tot = np.array([int(visits[i, :max(0, min(int(c), MAX_LEGAL))].astype(np.int64).sum()) for i, c in enumerate(count)])
    return (count >= 1) & (count <= MAX_LEGAL) & (tot > 0) & (slots >= 0) & (slots < capacity)


def expected_refresh(N, visits, actions, count, q, blend, slots, rings):
    """The rings after the launch, written out from the issue's statement: float32(float64(v) / float64(tot)) scattered by action over
    a zero row; the blend as replay.blend_targets computes it, on the ring's own value.  Returns new arrays."""
    from alphaquoridorgnn_amd.replay import blend_targets
    A = policy_size(N)
    r72, rpi, rz = (x.copy() for x in rings)
    capacity = rpi.shape[0]
    for i in np.flatnonzero(written_rows(N, visits, count, slots, capacity)):
        c = int(count[i])
        v = visits[i, :c]
        tot = int(v.astype(np.int64).sum())
        row = np.zeros((A,), dtype=np.float32)
        for j in range(c):
            if actions[i, j] < A:
                row[actions[i, j]] = np.float32(np.float64(v[j]) / np.float64(tot))
        rpi[slots[i]] = row
        if q is not None and blend != 0.0:
            rz[slots[i]] = blend_targets(rz[slots[i]:slots[i] + 1], q[i:i + 1], blend)[0]
    return r72, rpi, rz
