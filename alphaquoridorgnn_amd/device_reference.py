"""The device code of the self-play options in numpy: the references the GPU tests hold the kernels to."""
import numpy as np

from .counter_rng import counter_uniform, stream_key
from .selfplay_options import ROOT_NOISE_ATTEMPTS, check_completed_q, check_value_lambda


def draw_resign_enabled(seed, k, disable_fraction=0.1):
    """Whether game k may resign under the resignation seed `seed`: counter_uniform(stream_key(seed, k), 0) >= disable_fraction --
    the draw of engine_finish_move_kernel in numpy (include/aqgnn.h, "resignation").  k may be an array of game indices."""
    out = counter_uniform(stream_key(int(seed), np.asarray(k, dtype=np.int64)), 0) >= float(disable_fraction)
    return bool(out) if np.ndim(k) == 0 else out


def lambda_values_reference(game_plies, game_result, game_done, hist_value, lam, out):
    """aqg_lambda_values in numpy, on host arrays, in place (include/aqgnn.h, "lambda-return value targets"): game_plies int [quota],
    game_result int [quota] (-1 / 0 / 1 from the side of ply 0), game_done [quota], hist_value float32 [quota, hp], out float32
    [quota, hp].  Game k is processed iff game_done[k] != 0 and 1 <= game_plies[k] <= hp; out[k, t] is then written for
    t < game_plies[k] and nothing else is.  With a = float32(1) - lam, from the last ply T - 1 down,
    G_t = a * q_t + lam * (-G_{t+1}), and lam * z_{T-1} at the top -- two f32 products and one f32 sum per ply, each rounded, no
    fused multiply-add; z_t is float32(r) at an even ply and -float32(r) at an odd one.  Returns out."""
    lam = np.float32(check_value_lambda(lam))
    a = np.float32(1.0) - lam
    q, plies = np.asarray(hist_value), np.asarray(game_plies).astype(np.int64)
    if q.dtype != np.float32 or q.ndim != 2 or q.shape[1] < 1:
        raise ValueError("lambda_values_reference: hist_value must be float32 [quota, hp] with hp >= 1")
    quota, hp = q.shape
    if not isinstance(out, np.ndarray) or out.dtype != np.float32 or out.shape != q.shape:
        raise ValueError("lambda_values_reference: out must be a float32 array of hist_value's shape")
    if any(np.asarray(x).shape != (quota,) for x in (game_plies, game_result, game_done)):
        raise ValueError("lambda_values_reference: game_plies, game_result and game_done must hold one entry per row of hist_value")
    live = np.nonzero((np.asarray(game_done) != 0) & (plies >= 1) & (plies <= hp))[0]
    if live.size == 0:
        return out
    T = plies[live]
    r = np.asarray(game_result)[live].astype(np.float32)
    z_last = np.where((T - 1) % 2 == 0, r, -r).astype(np.float32)          # -float32(0) is -0.0, as on the device
    after = np.zeros(live.shape, dtype=np.float32)                          # -G_{t+1}, or z_{T-1} at a game's last ply
    with np.errstate(all="ignore"):         # a shorter game's columns past its end are computed and dropped, whatever they hold
        for t in range(int(T.max()) - 1, -1, -1):
            after = np.where(T - 1 == t, z_last, after)
            x = (a * q[live, t]).astype(np.float32)
            y = (lam * after).astype(np.float32)
            g = (x + y).astype(np.float32)
            on = t < T
            out[live[on], t] = g[on]
            after = -g
    return out


def root_noise_stream_key(seed, k, ply):
    """The 64-bit key of the noise stream of game k's root at `ply` under the noise seed `seed` (include/aqgnn.h: K(K(seed, k), ply))."""
    return int(stream_key(stream_key(int(seed), int(k)), int(ply)))


def draw_root_noise(seed, k, ply, count, alpha, return_exhausted=False):
    """The gamma variates g_0 .. g_{count-1} of the root of game k at ply `ply`, float64 [count] -- the generator of
    engine_root_noise_kernel in numpy (the recipe is in include/aqgnn.h, "root exploration noise").  k may be an array of game
    indices: the result is then [len(k), count].  Component i draws from its own sub-stream, so the first c components do not
    depend on count.  return_exhausted: also return how many variates took the fallback of the capped rejection loop."""
    scalar = np.ndim(k) == 0
    root = stream_key(stream_key(int(seed), np.atleast_1d(np.asarray(k, dtype=np.int64))), int(ply))
    key = stream_key(root[:, None], np.arange(int(count))[None, :])
    alpha = float(np.float32(alpha))          # the struct field is f32
    boost = alpha < 1.0
    a = alpha + 1.0 if boost else alpha
    d = a - 1.0 / 3.0
    c = 1.0 / np.sqrt(9.0 * d)
    val = np.full(key.shape, d, dtype=np.float64)
    todo = np.ones(key.shape, dtype=bool)
    for t in range(ROOT_NOISE_ATTEMPTS):
        if not todo.any():
            break
        kt = key[todo]
        u1, u2, u3 = (counter_uniform(kt, j + 3 * t) for j in (1, 2, 3))
        x = np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos(2.0 * np.pi * u2)
        v1 = 1.0 + c * x
        ok = v1 > 0.0
        v = np.where(ok, v1 * v1 * v1, 1.0)
        ok &= np.log(1.0 - u3) < 0.5 * x * x + d - d * v + d * np.log(v)
        idx = np.flatnonzero(todo.ravel())
        val.ravel()[idx[ok]] = d * v[ok]
        todo.ravel()[idx[ok]] = False
    exhausted = int(todo.sum())
    if boost:
        val = val * np.power(1.0 - counter_uniform(key, 0), 1.0 / alpha)
    val = np.maximum(val, np.finfo(np.float64).tiny)
    if scalar:
        val = val[0]
    return (val, exhausted) if return_exhausted else val


NODE_DTYPE = np.dtype([("w", "<f8"), ("p", "<f4"), ("action", "<u4"), ("n", "<i4"), ("kids", "<u4"), ("q", "<f4"), ("cp", "<f4")])
assert NODE_DTYPE.itemsize == 32      # csrc/mcts_tree.hpp NodeRec


def improved_policy_reference(p, n, q, w, root_w, c_visit=50.0, c_scale=1.0):
    """The completed-Q improved policy of ONE root in numpy (include/aqgnn.h, "completed-Q policy targets"; Danihelka et al., ICLR 2022,
    section 4 and appendix D) -- the statement csrc/mcts_improve.hip is held to.  Of the root's cnt children in legal_actions() order, as
    their records hold them: p float32 [cnt] priors, n int32 [cnt] visits, q float32 [cnt] = f32(-w_i / n_i) (0 while n_i == 0), w
    float64 [cnt]; root_w the root's own w.  All arithmetic is float64:
        vhat = root_w + sum w;  vmix = (vhat + Nsum * (QV / PV)) / (1 + Nsum) over the visited children (vhat when PV is not > 0)
        c_i = q_i if n_i > 0 else vmix;  sigma_i = (c_visit + max n) * c_scale * ((c_i + 1) / 2)
        pi' = softmax(log p + sigma) over the entries with p_i > 0, 0 elsewhere
    Returns (pi' float32 [cnt], vmix float32); a root without a prior above 0 (cnt == 0 included) gets zeros."""
    c_visit, c_scale = check_completed_q(c_visit, c_scale)
    p, q = np.asarray(p, dtype=np.float32).reshape(-1), np.asarray(q, dtype=np.float32).reshape(-1)
    n, w = np.asarray(n, dtype=np.int64).reshape(-1), np.asarray(w, dtype=np.float64).reshape(-1)
    cnt = p.shape[0]
    if not n.shape[0] == q.shape[0] == w.shape[0] == cnt:
        raise ValueError("improved_policy_reference: p, n, q and w must have one entry per child")
    p64, q64 = p.astype(np.float64), q.astype(np.float64)
    nsum = int(n.sum())
    nmax = int(n.max()) if cnt else 0
    nmax = max(nmax, 0)
    vhat = np.float64(root_w) + np.float64(w.sum())
    visited = n > 0
    pv, qv = np.float64(p64[visited].sum()), np.float64((p64[visited] * q64[visited]).sum())
    vmix = (vhat + np.float64(nsum) * (qv / pv)) / (np.float64(1.0) + np.float64(nsum)) if pv > 0 else vhat
    pi = np.zeros((cnt,), dtype=np.float32)
    live = p > 0                                               # p <= 0 or NaN: excluded
    if live.any():
        c = np.where(visited, q64, vmix)
        sigma = ((np.float64(c_visit) + np.float64(nmax)) * np.float64(c_scale)) * ((c + 1.0) / 2.0)
        x = np.log(p64[live]) + sigma[live]
        e = np.exp(x - x.max())
        pi[live] = (e / e.sum()).astype(np.float32)
    return pi, np.float32(vmix)


def root_improved_policy_reference(pool_records, c_visit=50.0, c_scale=1.0):
    """The row aqg_engine_root_improved_policy writes for one slot, from its pool (NODE_DTYPE [node_cap], or anything of 32 bytes per
    record): (policy float32 [MAX_LEGAL], actions uint8 [MAX_LEGAL], count, vmix float32) -- improved_policy_reference on the root's
    child block, 0 and 0xFF past the count.  A count above MAX_LEGAL or a child range that leaves the pool gives the zero row: count
    0, vmix 0."""
    from ._lib import MAX_LEGAL
    src = np.ascontiguousarray(pool_records).view(NODE_DTYPE).reshape(-1)
    policy, actions = np.zeros((MAX_LEGAL,), dtype=np.float32), np.full((MAX_LEGAL,), 0xFF, dtype=np.uint8)
    cnt, first = int(src["kids"][0]) >> 24, int(src["kids"][0]) & 0xFFFFFF
    if cnt > MAX_LEGAL or first + cnt > src.shape[0]:
        check_completed_q(c_visit, c_scale)
        return policy, actions, 0, np.float32(0.0)
    kids = src[first:first + cnt]
    policy[:cnt], vmix = improved_policy_reference(kids["p"], kids["n"], kids["q"], kids["w"], src["w"][0], c_visit, c_scale)
    actions[:cnt] = kids["action"].astype(np.uint8)
    return policy, actions, cnt, vmix


def keep_subtree_reference(pool_records, node_count, child_index, keep_visits):
    """The keep launch (csrc/mcts_reuse.hip) for one slot, in numpy.  pool_records: the slot's pool, NODE_DTYPE [cap] (or anything
    of 32 bytes per record, e.g. float64 [cap, 4]); node_count: its used records; child_index: index of the chosen child in the root's
    child block, < 0 = do not keep.  Returns (records, count, kept): kept is True iff the index names a child that is expanded with
    n <= keep_visits; then records[:count] is the child's subtree re-rooted -- the child at 0 with a fresh root's action / p / cp, every
    kept child block behind it in ascending order of its old first index, child ranges renamed -- and records[count:] is unspecified
    (here: the input's).  Not kept: the input's records and count."""
    src = np.ascontiguousarray(pool_records).view(NODE_DTYPE).reshape(-1)
    out = src.copy()
    count = min(int(node_count), src.shape[0])
    idx = int(child_index)
    if idx < 0 or count <= 1:
        return out, int(node_count), False
    rcnt, rfirst = int(src["kids"][0]) >> 24, int(src["kids"][0]) & 0xFFFFFF
    if idx >= rcnt or rfirst < 1 or rfirst + rcnt > count:
        return out, int(node_count), False
    c = src[rfirst + idx]
    ccnt, cfirst = int(c["kids"]) >> 24, int(c["kids"]) & 0xFFFFFF
    if ccnt == 0 or int(c["n"]) > int(keep_visits) or cfirst < rfirst + rcnt or cfirst + ccnt > count:
        return out, int(node_count), False
    keep = np.zeros(count, dtype=bool)
    keep[cfirst:cfirst + ccnt] = True
    kids = src["kids"][:count].astype(np.int64)
    for i in range(cfirst, count):            # a node's child block lies behind the node: one ascending pass decides every record
        if keep[i] and kids[i] >> 24:
            first, cnt = int(kids[i] & 0xFFFFFF), int(kids[i] >> 24)
            assert first > i, "a child block lies behind its parent"
            keep[first:min(first + cnt, count)] = True
    new_index = np.cumsum(keep)               # 1-based among the kept records == the new index (0 is the new root)
    old = np.nonzero(keep)[0]
    moved = src[old].copy()
    exp = (moved["kids"] >> 24) != 0
    firsts = (moved["kids"][exp] & 0xFFFFFF).astype(np.int64)
    moved["kids"][exp] = (new_index[firsts].astype(np.uint32) & 0xFFFFFF) | (moved["kids"][exp] & np.uint32(0xFF000000))
    total = 1 + old.shape[0]
    out[1:total] = moved
    root = np.zeros((), dtype=NODE_DTYPE)
    root["w"], root["n"], root["q"] = c["w"], c["n"], c["q"]
    root["action"], root["kids"] = 0xFF, 1 | (ccnt << 24)
    out[0] = root
    return out, total, True
