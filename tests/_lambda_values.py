"""Shared by the lambda-return tests (include/aqgnn.h, "lambda-return value targets"): seeded input builders in the engine's layout
and the recurrence stated in float64, once as the recurrence and once as its closed form."""
import numpy as np

# the lambdas of the GPU cases: the ends, the last float32 below 1 and the smallest power of two that still moves 1 - lambda
LAMBDAS = (0.0, 2.0 ** -24, 0.5, 0.95, 1.0 - 2.0 ** -24, 1.0)


def games(quota, hp, seed, special_q=False):
    """Synthetic arrays of one launch, as the engine lays them out: game_plies int32 [quota], game_result int8 [quota], game_done
    uint8 [quota], hist_value float32 [quota, hp].  The plies cycle through 1, 63, 64, 65 and hp -- and through 0, hp + 1 and a
    negative count, which the kernel must skip -- the results through -1, 0, 1; every fifth game is not done, between done ones, and
    done is a byte other than 1 now and then.  q is uniform in [-1, 1] on EVERY entry, the ones past a game's end included (the kernel
    must not read them into the result); special_q draws from +-1 and +-0 only."""
    rng = np.random.RandomState(seed)
    cycle = [1, 63, 64, 65, hp, 0, hp + 1, -3, max(hp - 1, 1), (hp + 1) // 2]
    plies = np.array([cycle[(k + seed) % len(cycle)] for k in range(quota)], dtype=np.int32)
    inside = (plies >= 1) & (plies <= hp)
    plies[~inside & (plies > hp + 1)] = hp                      # 63 / 64 / 65 above a short hp: the whole row instead
    result = np.array([(-1, 0, 1)[(k // 2 + seed) % 3] for k in range(quota)], dtype=np.int8)
    done = np.array([0 if (k + seed) % 5 == 3 else (1, 1, 255, 2)[k % 4] for k in range(quota)], dtype=np.uint8)
    if special_q:
        q = np.array([1.0, -1.0, 0.0, -0.0], dtype=np.float32)[rng.randint(0, 4, size=(quota, hp))]
    else:
        q = rng.uniform(-1.0, 1.0, size=(quota, hp)).astype(np.float32)
    return plies, result, done, np.ascontiguousarray(q)


def processed(plies, done, hp):
    """Which games a launch processes, and the mask [quota, hp] of the floats it writes."""
    live = (done != 0) & (plies >= 1) & (plies <= hp)
    return live, live[:, None] & (np.arange(hp)[None, :] < plies[:, None])


def z_of(result, t):
    """z_t as float32: the result from the mover's side at ply t (-0.0 for a draw at an odd ply)."""
    r = np.float32(result)
    return r if t % 2 == 0 else -r


def recurrence_f64(q_row, T, result, lam):
    """G_0 .. G_{T-1} of one game in float64, with the float32 lambda the kernel is given."""
    lam = float(np.float32(lam))
    a = 1.0 - lam
    q = np.asarray(q_row[:T], dtype=np.float64)
    G = np.empty(T, dtype=np.float64)
    G[T - 1] = a * q[T - 1] + lam * float(z_of(result, T - 1))
    for t in range(T - 2, -1, -1):
        G[t] = a * q[t] + lam * -G[t + 1]
    return G


def closed_form_f64(q_row, T, result, lam):
    """G_t = sum_k (-lam)^k (1 - lam) q_{t+k} + (-lam)^(T-1-t) lam z_{T-1}, in float64."""
    lam = float(np.float32(lam))
    q = np.asarray(q_row[:T], dtype=np.float64)
    zl = float(z_of(result, T - 1))
    G = np.empty(T, dtype=np.float64)
    for t in range(T):
        k = np.arange(T - t)
        G[t] = np.sum((-lam) ** k * (1.0 - lam) * q[t:]) + (-lam) ** (T - 1 - t) * lam * zl
    return G


def bits(x):
    return np.ascontiguousarray(x).view(np.int32)
