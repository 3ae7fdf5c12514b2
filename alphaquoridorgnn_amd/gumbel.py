"""The Gumbel root search (include/aqgnn.h, "Gumbel root search"; Danihelka et al., ICLR 2022) on the host, in numpy: the statements
the kernels are held to.  Same arithmetic, float32 where the kernel is float32 and float64 where it is float64.

    considered_visits        the visit schedule T of sequential halving (built here, uploaded once by the engine)
    draw_gumbel              the generator's Gumbel(0, 1) variates of one root (csrc/mcts_gumbel.hip gumbel_variate)
    gumbel_logits_reference  rule 1: gl_i = f32(scale * g_i + log p_i), -inf where p_i is not > 0
    root_score_reference     rule 3: S_i, -inf where n_i is not the considered count
    gumbel_winner_reference  rule 4: the child that is played
"""
import math

import numpy as np

from .constants import MAX_LEGAL
from .counter_rng import counter_uniform, stream_key

DBL_MIN = float(np.finfo(np.float64).tiny)
MAX_CONSIDERED = 64


def considered_visits(considered, sims):
    """T[m'][0 .. sims - 2] for m' = 0 .. considered, int32 [considered + 1, sims - 1]: the sequence of considered visit counts of
    sequential halving over m' actions with sims - 1 simulations (simulation 0 evaluates the root)."""
    considered, sims = int(considered), int(sims)
    if not 1 <= considered <= MAX_CONSIDERED:
        raise ValueError(f"gumbel_considered must be in 1..{MAX_CONSIDERED}, not {considered}")
    if sims < 2:
        raise ValueError("the Gumbel root search needs sims >= 2: simulation 0 evaluates the root")
    budget = sims - 1
    table = np.zeros((considered + 1, budget), dtype=np.int32)
    for m in range(considered + 1):
        if m <= 1:
            table[m] = np.arange(budget)
            continue
        L = math.ceil(math.log2(m))
        visits, k, seq = [0] * m, m, []
        while len(seq) < budget:
            x = max(1, budget // (L * k))
            for _ in range(x):
                seq.extend(visits[:k])
                for i in range(k):
                    visits[i] += 1
            k = max(2, k // 2)
        table[m] = seq[:budget]
    return table


def draw_gumbel(seed=0, game=0, plies=0, count=MAX_LEGAL, uniforms=None):
    """The Gumbel(0, 1) variates g_0 .. g_{count-1} of the root of game `game` (the slot in search()) at ply `plies`, float64 [count]:
    u = draw 0 of the stream K(K(K(seed, game), plies), i), e = -log(1 - u), e = DBL_MIN if that is 0, g = -log(e).  uniforms: the
    transform alone, of caller-given u in [0, 1)."""
    if uniforms is None:
        key = stream_key(stream_key(stream_key(int(seed), int(game)), int(plies)), np.arange(int(count)))
        u = counter_uniform(key, 0)
    else:
        u = np.asarray(uniforms, dtype=np.float64)
    e = -np.log(1.0 - u)
    e = np.where(e == 0.0, DBL_MIN, e)
    return -np.log(e)


def gumbel_logits_reference(priors, g, scale=1.0):
    """Rule 1 for one root: priors float32 [cnt] (the children's stored p), g float64 [>= cnt] variates (a non-finite entry reads 0).
    Returns gl float32 [cnt]: f32(scale * g_i + log(p_i)) formed in float64 and rounded once; -inf where p_i is not > 0 (NaN too)."""
    p = np.asarray(priors, dtype=np.float32).reshape(-1)
    gv = np.asarray(g, dtype=np.float64).reshape(-1)[:p.shape[0]]
    gv = np.where(np.isfinite(gv), gv, 0.0)
    ok = p > 0                                          # False for NaN
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        x = np.float64(scale) * gv + np.log(np.where(ok, p, np.float32(1)).astype(np.float64))
        gl = x.astype(np.float32)
    return np.where(ok, gl, np.float32(-np.inf)).astype(np.float32)


def considered_count(gl, considered):
    """m_g = min(considered, number of children with gl_i > -inf)."""
    return min(int(considered), int((np.asarray(gl) > -np.inf).sum()))


def root_score_reference(gl, n, q, c_visit, c_scale, v):
    """Rule 3 for one root: S float32 [cnt] from gl float32, n int, q float32 (the children's stored q) and the considered visit count
    v.  Float32, left to right: gl_i + (n_i > 0 ? ((c_visit + float(nmax)) * c_scale) * ((q_i + 1) * 0.5) : 0); -inf where n_i != v
    or gl_i is -inf."""
    gl, q = np.asarray(gl, dtype=np.float32).reshape(-1), np.asarray(q, dtype=np.float32).reshape(-1)
    n = np.asarray(n, dtype=np.int64).reshape(-1)
    f = np.float32
    nmax = f(int(n.max())) if n.shape[0] else f(0)
    with np.errstate(invalid="ignore", over="ignore"):
        scale = f(f(f(c_visit) + nmax) * f(c_scale))
        sigma = np.where(n > 0, (scale * ((q + f(1.0)) * f(0.5)).astype(np.float32)).astype(np.float32), f(0.0)).astype(np.float32)
        s = (gl + sigma).astype(np.float32)
    return np.where((n == int(v)) & (gl > -np.inf), s, f(-np.inf)).astype(np.float32)


def first_argmax(scores):
    """The first index of the maximum, ignoring NaN; 0 if nothing equals it (the step kernel's arg-max)."""
    best, idx = np.float32(-np.inf), 0
    for i, s in enumerate(np.asarray(scores, dtype=np.float32)):
        if s > best:
            best, idx = s, i
    return idx


def gumbel_winner_reference(gl, n, q, c_visit, c_scale):
    """Rule 4 for one root: the index of the child that is played -- the first arg-max of S with v = the largest visit count among
    the children with gl > -inf; -1 without children."""
    gl = np.asarray(gl, dtype=np.float32).reshape(-1)
    n = np.asarray(n, dtype=np.int64).reshape(-1)
    if gl.shape[0] == 0:
        return -1
    sampled = gl > -np.inf
    v = int(n[sampled].max()) if sampled.any() else -1
    return first_argmax(root_score_reference(gl, n, q, c_visit, c_scale, v))
