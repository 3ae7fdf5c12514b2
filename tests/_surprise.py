"""Builders and the bound on k for the surprise-weighting tests (tests/test_surprise_weighting_cpu.py, tests/test_surprise_weighting.py).

THE BOUND ON k (derived, not measured).  The kernel and replay.surprise_reference run the same float64 operations in the same order;
what differs is the library that evaluates ln.  Accuracies, as documented: the device library's table is not shipped with the
toolchain this suite builds with, so the device side is taken at OpenCL's full-profile requirement for double log, 3 ulp; numpy calls
the C library's log, which glibc documents at 1 ulp.  Every logarithm taken here has |ln| < 88 (f32 arguments no smaller than 2^-126),
and the ulp of a float64 below 128 is at most 2^-46.  A row's sum is sum_a t_a (ln t_a - ln p_a), so before the final rounding the
two routes differ by at most sum_a t_a (ULP_DEVICE + ULP_NUMPY) 2^-46; rounding to f32 can then separate them by one f32 ulp of the
reference's k.  The bar is the sum of the two.  Everything after k -- q, S, f, the draws, the counts, the index -- is integer or
exact-order float64 and is held bit for bit."""
import numpy as np

ULP_DEVICE, ULP_NUMPY = 3.0, 1.0
LN_ULP = 2.0 ** -46
BOARDS = (3, 5, 7, 9)
# the rows kernel: SPR_GROUP = 4 rows per wavefront, SPR_ROWS = 16 per workgroup; the counts kernel: SPR_LANES = 256 rows per workgroup
SIZES = (1, 3, 4, 5, 15, 16, 17, 63, 64, 65)


def policy_size(N):
    return N * N + 2 * (N - 1) * (N - 1)


def k_bar(k_ref, targets):
    """The bar on |k - k_ref| per row, float64 [m]: one f32 ulp of k_ref plus sum_a t_a (3 + 1) 2^-46 over the row's positive target
    entries (targets float32 [m,A], the rows k_ref was computed for)."""
    k_ref = np.asarray(k_ref, dtype=np.float32)
    t = np.where(np.asarray(targets) > 0, targets, 0).astype(np.float64)
    return np.spacing(k_ref).astype(np.float64) + t.sum(axis=1) * (ULP_DEVICE + ULP_NUMPY) * LN_ULP


def within_bar(k, k_ref, targets):
    return np.abs(np.asarray(k, np.float64) - np.asarray(k_ref, np.float64)) <= k_bar(k_ref, targets)


def target_rows(rng, rows, A):
    """Policy targets as the loop makes them, float32 [rows,A]: a distribution over a random subset of 1 .. A actions (visit counts over
    their sum), zero elsewhere; every fourth row a dense softmax (a completed-Q target)."""
    out = np.zeros((rows, A), dtype=np.float32)
    for i in range(rows):
        if i % 4 == 3:
            x = rng.standard_normal(A) * 3
            e = np.exp(x - x.max())
            out[i] = (e / e.sum()).astype(np.float32)
        else:
            legal = rng.permutation(A)[:rng.randint(1, A + 1)]
            v = rng.randint(0, 40, legal.shape[0]).astype(np.float64)
            v[rng.randint(legal.shape[0])] += 1
            out[i, legal] = (v / v.sum()).astype(np.float32)
    return out


def network_rows(rng, m, A):
    """Softmaxed network policies, float32 [m,A]: sharp and flat rows, and in every third row some entries that underflowed to exactly 0
    or to a subnormal -- below the 2^-126 a logarithm is taken of."""
    x = rng.standard_normal((m, A)) * rng.choice([0.5, 4.0, 30.0], size=(m, 1))
    e = np.exp(x - x.max(axis=1, keepdims=True))
    p = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
    for i in range(0, m, 3):
        p[i, rng.permutation(A)[:3]] = (0.0, 1e-41, 2.0 ** -126)
    return p


SPECIAL = ("nan_target", "inf_target", "negative_target", "no_positive_target", "nan_policy", "inf_policy", "neg_inf_policy")


def special_rows(rng, A):
    """(pi, net) of len(SPECIAL) rows, one of each kind: every one reads k = 0, q = 0.  The entry that makes a row special sits at a
    place of its own -- the first lane, the last action, a lane of the last pass."""
    pi, net = target_rows(rng, len(SPECIAL), A), network_rows(rng, len(SPECIAL), A)
    at = [0, A - 1, A // 2, 0, A - 1, (A - 1) // 64 * 64, 1 % A]
    pi[0, at[0]] = np.nan
    pi[1, at[1]] = np.inf
    pi[2, at[2]] = -0.125
    pi[3] = 0.0
    pi[3, 1 % A] = -0.0                                  # not a negative entry, and not a positive one
    net[4, at[4]] = np.nan
    net[5, at[5]] = np.inf
    net[6, at[6]] = -np.inf
    return pi, net


EXACT = ("target_is_policy", "one_hot_on_one", "zero_policy_under_one_hot", "zero_policy_under_half")


def exact_rows(rng, A):
    """(pi, net, want) of len(EXACT) rows whose k is known in closed form: t == p bitwise -> 0; a one-hot target on p = 1 -> 0; p = 0
    under a one-hot target -> f32(126 ln 2) (ln 1 = 0 exactly, and the reference's ln 2^-126); p = 0 under t = 1/2 there and t = p =
    1/2 elsewhere -> f32(0.5 (ln 0.5 + 126 ln 2)).  want holds None where the value is the reference's own (it is then only compared
    within the bar)."""
    pi, net = np.zeros((len(EXACT), A), np.float32), np.zeros((len(EXACT), A), np.float32)
    net[0] = network_rows(rng, 1, A)[0]
    pi[0] = net[0]
    hot = A - 1
    pi[1, hot], net[1, hot] = 1.0, 1.0
    pi[2, hot] = 1.0
    net[2, 0] = 1.0
    pi[3, hot], pi[3, 0] = 0.5, 0.5
    net[3, 0] = 0.5
    tiny = np.log(np.float64(2.0 ** -126))
    want = [np.float32(0), np.float32(0), np.float32(0.0 - tiny), np.float32(0.5 * (np.log(0.5) - tiny) + 0.5 * 0.0)]
    return pi, net, want


def plain_kl(t, p):
    """The definition without the order: float64 [m], sum over t_a > 0 of t_a (ln t_a - ln max(p_a, 2^-126)) by numpy's own sum, and the
    sum of the terms' magnitudes beside it (what a reordering can move the result by, times A 2^-53)."""
    t, p = np.asarray(t, np.float64), np.maximum(np.asarray(p, np.float64), 2.0 ** -126)
    pos = t > 0
    with np.errstate(all="ignore"):
        term = np.where(pos, np.where(pos, t, 1.0) * (np.log(np.where(pos, t, 1.0)) - np.log(p)), 0.0)
    return term.sum(axis=1), np.abs(term).sum(axis=1)
