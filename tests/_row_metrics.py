"""Builders and the derived bars of the row-metrics tests (tests/test_row_metrics_cpu.py, tests/test_row_metrics.py,
tests/test_validation_loop.py).

THE BARS (derived, not measured).  Two routes to a row's ce, ent and lp are compared: replay.row_metrics_reference against a plain
float64 torch composition on the CPU, and the kernel against replay.row_metrics_reference on the GPU.  Both routes start from the same
f32 inputs and differ in (a) the library that evaluates ln and exp and (b) the order of the additions.  As tests/_surprise.py does:
glibc documents its double log and exp at 1 ulp (numpy and torch's CPU kernels are held to the same), and the device library is taken
at OpenCL's full-profile requirement for double log and exp, 3 ulp.  With u = 2^-53:

  ce, ent   Every logarithm taken has |ln| < 88 < 128 (f32 arguments no smaller than 2^-126 and, in these tests, no larger than 1), so
            one ulp of it is at most 2^-46.  A term is t * ln x: the two routes' terms differ by at most t (U_A + U_B) 2^-46, plus one
            rounding of the product each (2 u |term|).  A sum of K terms in ANY order is within (K - 1) u sum|term| of the exact sum
            to first order, so two orders differ by at most 2 (K - 1) u sum|term|; K <= A.  Bar:
                sum_a t_a (U_A + U_B) 2^-46 + 2 (A + 1) u sum|term|, times (1 + 2^-20) for the second-order terms.
  lp        = S_t ln(S_e) - S_tp with S_e = sum exp(p).  The tests' p lie in [0, 1]: exp(p) in [1, e], and a relative error of U ulp
            is at most U 2^-52.  All terms of S_e are positive, so its relative error is at most U 2^-52 + (A - 1) u per route.  The
            torch route (logsumexp / CrossEntropyLoss) subtracts the row maximum first: one more rounding of an argument of magnitude
            <= 1 (u absolute, so u relative in exp) and one more addition: 2 u more.  d ln(S_e) = dS_e / S_e, plus the logarithm's own
            error: ln(S_e) <= ln(209 e) < 8, one ulp <= 2^-50.  So per route d_lse <= U 2^-52 + (A + 1) u + U 2^-50, and
                |d lp| <= S_t (d_lse_A + d_lse_B) + 2 (A + 2) u (S_t lse + sum t |p|)
            where the second part covers S_t's and S_tp's own sums, the products' roundings, the final difference and the other
            route's form sum_a t_a (lse - p_a); times (1 + 2^-20) again.
  se        exact up to one rounding, the same in both routes: bit for bit.  tag and the rejections: bit for bit.

THE REDUCTION'S BAR.  Against np.add.at in float64: both sum the same float64 terms, so they differ by at most (depth_A + depth_B) u
sum|x| per bucket: the kernel's depth is 16 additions in a lane, 6 across the wave, 3 across the waves, then ceil(chunks / 64) and 6
more; np.add.at adds a bucket's rows one by one, at most m - 1 additions.  On dyadic data (every partial sum exact) the two are equal
bit for bit."""
import numpy as np

from tests._surprise import network_rows, policy_size, target_rows  # noqa: F401

ULP_DEVICE, ULP_HOST = 3.0, 1.0
U = 2.0 ** -53
LN_ULP = 2.0 ** -46
BOARDS = (3, 5, 7, 9)
SECOND_ORDER = 1.0 + 2.0 ** -20
OFFSETS = (0, 1, 15, 16, 17)


def bars(t, p, ulp_a, ulp_b):
    """(bar_ce, bar_ent, bar_lp) per row, float64 [m] each, for targets t and network policies p (float32 [m,A]; p in [0, 1]) whose
    two routes evaluate ln and exp within ulp_a and ulp_b ulp.  Non-finite and negative entries count as zero (such rows are rejected
    and held bit for bit)."""
    t = np.nan_to_num(np.asarray(t, np.float64), nan=0.0, posinf=0.0, neginf=0.0)
    p = np.nan_to_num(np.asarray(p, np.float64), nan=0.0, posinf=0.0, neginf=0.0)
    t = np.where(t > 0, t, 0.0)
    A = t.shape[1]
    ulps = ulp_a + ulp_b
    pos = t > 0
    with np.errstate(all="ignore"):
        ln_p = np.where(pos, np.abs(np.log(np.maximum(p, 2.0 ** -126))), 0.0)
        ln_t = np.where(pos, np.abs(np.log(np.where(pos, t, 1.0))), 0.0)
    s_t = t.sum(axis=1)
    bar_ce = (s_t * ulps * LN_ULP + 2 * (A + 1) * U * (t * ln_p).sum(axis=1)) * SECOND_ORDER
    bar_ent = (s_t * ulps * LN_ULP + 2 * (A + 1) * U * (t * ln_t).sum(axis=1)) * SECOND_ORDER
    lse = np.log(np.exp(p).sum(axis=1))
    d_lse = ulps * 2.0 ** -52 + 2 * (A + 1) * U + ulps * 2.0 ** -50
    bar_lp = (s_t * d_lse + 2 * (A + 2) * U * (s_t * lse + (t * np.abs(p)).sum(axis=1))) * SECOND_ORDER
    return bar_ce, bar_ent, bar_lp


def within_bars(vals, vals_ref, t, p, ulp_a, ulp_b):
    """Per row: ce, ent and lp within their bars, se bit for bit.  bool [m]."""
    vals, vals_ref = np.asarray(vals, np.float64), np.asarray(vals_ref, np.float64)
    ok = vals[:, 3].tobytes() == vals_ref[:, 3].tobytes()
    out = np.full((vals.shape[0],), ok)
    for col, bar in enumerate(bars(t, p, ulp_a, ulp_b)):
        out &= np.abs(vals[:, col] - vals_ref[:, col]) <= bar
    return out


def reduce_depth(m):
    """The additions between a term and its bucket's total: the kernel's plus np.add.at's."""
    chunks = -(-m // 4096)
    return (16 + 6 + 3 + -(-chunks // 64) + 6) + max(m - 1, 0)


def records(rng, rows, plies=None):
    """uint8 [rows,72] records of random bytes with the ply counter (bytes 68-69, little endian) set to `plies` (default: random 0..199)."""
    s = rng.randint(0, 256, (rows, 72)).astype(np.uint8)
    plies = rng.randint(0, 200, rows) if plies is None else np.asarray(plies)
    s[:, 68], s[:, 69] = plies & 255, plies >> 8
    return s


def value_rows(rng, m):
    """(v float32 [m] in (-1, 1), z float32 [rows]): tanh values and targets among -1, 0, 1 and blended values."""
    v = np.tanh(rng.standard_normal(m)).astype(np.float32)
    z = rng.choice(np.array([-1.0, 0.0, 1.0, 0.25, -0.5], np.float32), m).astype(np.float32)
    return v, z


def case(rng, N, rows, m):
    """One ordinary case: (states72 [rows,72], pi [rows,A], z [rows], net_policy [m,A], net_value [m])."""
    A = policy_size(N)
    v, _ = value_rows(rng, m)
    _, z = value_rows(rng, rows)
    return records(rng, rows), target_rows(rng, rows, A), z, network_rows(rng, m, A), v


SPECIAL = ("nan_target", "inf_target", "negative_target", "no_positive_target", "nan_policy", "inf_policy", "neg_inf_policy",
           "nan_value", "inf_value", "nan_z", "neg_inf_z")


def special_rows(rng, N):
    """A case of len(SPECIAL) rows, one of each kind: every one is rejected.  The entry that makes a row special sits at a place of its
    own -- the first lane, the last action, a lane of the last pass."""
    A, n = policy_size(N), len(SPECIAL)
    s72, pi, z, net, v = case(rng, N, n, n)
    pi[0, 0] = np.nan
    pi[1, A - 1] = np.inf
    pi[2, A // 2] = -0.125
    pi[3] = 0.0
    pi[3, 1 % A] = -0.0                                  # not a negative entry, and not a positive one
    net[4, A - 1] = np.nan
    net[5, (A - 1) // 64 * 64] = np.inf
    net[6, 1 % A] = -np.inf
    v[7], v[8] = np.nan, np.inf
    z[9], z[10] = np.nan, -np.inf
    return s72, pi, z, net, v


def torch_composition(t, p, v, z):
    """The definition as a plain float64 torch composition, without the kernel's order: (ce, ent, lp, se, hit, counted, agrees) per row
    as numpy arrays -- xlogy for ent, xlogy on the clamped p for ce, logsumexp is inside CrossEntropyLoss()(p64, t64), called a row at
    a time (its default reduction is the batch mean), for lp."""
    import torch
    t64, p64 = torch.from_numpy(np.asarray(t)).double(), torch.from_numpy(np.asarray(p)).double()
    v64, z64 = torch.from_numpy(np.asarray(v)).double(), torch.from_numpy(np.asarray(z)).double()
    ce = -torch.xlogy(t64, p64.clamp(min=2.0 ** -126)).sum(dim=1)
    ent = -torch.xlogy(t64, t64).sum(dim=1)
    loss = torch.nn.CrossEntropyLoss()
    lp = torch.stack([loss(p64[i:i + 1], t64[i:i + 1]) for i in range(t64.shape[0])]) if t64.shape[0] else torch.zeros(0).double()
    lp_lse = t64.sum(dim=1) * torch.logsumexp(p64, dim=1) - (t64 * p64).sum(dim=1)
    se = (v64 - z64) ** 2
    first = p64.argmax(dim=1)
    hit = t64.gather(1, first[:, None])[:, 0] == t64.max(dim=1).values
    counted = z64 != 0
    agrees = counted & (v64 * z64 > 0)
    return tuple(x.numpy() for x in (ce, ent, lp, se, hit, counted, agrees)) + (lp_lse.numpy(),)


class StubModel:
    """A host network for the loop's CPU tests: a softmax over a linear map of the record bytes and a tanh value, with one weight
    tensor `w` that a stub trainer moves.  The surface row_metrics and the loop use: board_size, policy_output_size, forward_states,
    eval / train, state_dict."""

    def __init__(self, N=5, seed=0):
        import torch
        self.board_size, self.policy_output_size, self.training = N, policy_size(N), False
        g = torch.Generator().manual_seed(seed)
        self.w = torch.randn((72, self.policy_output_size + 1), generator=g) * 0.02
        self.forwards = 0

    def eval(self):
        self.training = False
        return self

    def train(self, mode=True):
        self.training = bool(mode)
        return self

    def state_dict(self):
        from collections import OrderedDict
        return OrderedDict(w=self.w)

    def forward_states(self, states72):
        import torch
        assert not self.training
        self.forwards += 1
        out = states72.float() @ self.w
        return torch.softmax(out[:, :-1], dim=1), torch.tanh(out[:, -1:] * 0.1)
