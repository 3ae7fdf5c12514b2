"""Shared by test_split_low_side.py (gpu) and test_split_low_side_cpu.py: function-preserving rescalings of the GNN's weights,
and a numpy statement of the fp16 hi/lo split the default 9x9 kernels compute with (test infrastructure).

A ReLU network is positively homogeneous: layer a's weight and bias times s and the next layer's weight times 1/s is the same
function.  With s = 2^-k every f32 parameter of the rescaled set is an EXACT multiple, so fp32 -- the reference's, and the exact
kernels' -- computes the same numbers shifted in the exponent.  The split kernels do not: hi = f16(x), lo = f16(x - hi) is an
fp32-equivalent pair only while lo is a normal fp16 number, i.e. |x| >= 2^-3; below that the pair's absolute error stops
shrinking at about 2^-25."""
import numpy as np

from oracle import gnn as og

CQ = 15.0 / 16.0          # csrc/gcn_packed.hpp: the scale of the split trunk's activation image
KS = (0, 4, 8, 10, 12, 14, 16)

# site -> (tensors scaled DOWN by s = 2^-k: the layer's weight and bias;  tensors scaled UP by 1/s: the next layer's weight(s))
SITES = {
    "gcn0/gcn1": (("gcn_layers.0.lin.weight", "gcn_layers.0.bias"), ("gcn_layers.1.lin.weight",)),
    "gcn1/gcn2": (("gcn_layers.1.lin.weight", "gcn_layers.1.bias"), ("gcn_layers.2.lin.weight",)),
    "gcn2/heads": (("gcn_layers.2.lin.weight", "gcn_layers.2.bias"), ("policy_head.0.weight", "value_head.0.weight")),
    "policy0/policy2": (("policy_head.0.weight", "policy_head.0.bias"), ("policy_head.2.weight",)),
    "value0/value2": (("value_head.0.weight", "value_head.0.bias"), ("value_head.2.weight",)),
}


def base_params(seed=3):
    """oracle/gnn.py initialisation with non-zero GCN biases (PyG's zero biases would leave the bias path out)."""
    p = og.init_params(seed)
    for l in range(3):
        p[f"gcn_layers.{l}.bias"] = (np.linspace(-0.3, 0.5, 128) * (1 + l)).astype(np.float32)
    return p


def rescale(params, site, k):
    """(rescaled parameter set, {key: f}) with s = 2^-k at `site`: the same function; the gradient with respect to tensor `key` of
    the rescaled set is EXACTLY f times that of the base set (1/s for the tensors scaled down, s for those scaled up, 1 elsewhere).
    Biases behind the scaled layer stay untouched."""
    down, up = SITES[site]
    s = np.float32(2.0 ** -k)
    out = {key: np.asarray(v, dtype=np.float32).copy() for key, v in params.items()}
    gfac = {key: 1.0 for key in params}
    for key in down:
        out[key] = out[key] * s
        gfac[key] = float(2.0 ** k)
    for key in up:
        out[key] = out[key] / s
        gfac[key] = float(2.0 ** -k)
    for key in down + up:                                   # exact multiples: nothing was rounded, nothing left f32's normal range
        assert np.array_equal(out[key].astype(np.float64), np.asarray(params[key], dtype=np.float64) * (2.0 ** (-k if key in down else k))), key
        assert np.abs(out[key]).max() < 65504.0 * CQ
    return out, gfac


def assert_same_function(base, rescaled, recs):
    """The fp64 oracle of the rescaled set equals that of the base set to 1e-9 relative: the reference alone stays within any bar."""
    a, b = og.forward_states_dense(base, recs), og.forward_states_dense(rescaled, recs)
    for key in ("logits", "value_pre", "policy"):
        assert np.abs(a[key] - b[key]).max() <= 1e-9 * max(np.abs(a[key]).max(), 1e-300), key


# ------------------------------------------------------------------ the split in numpy
def f16(x, flush):
    """RNE to fp16 and back, as float64; flush: results below fp16's smallest normal become zero (subnormals not kept)."""
    with np.errstate(over="ignore"):
        h = np.asarray(x, dtype=np.float64).astype(np.float16).astype(np.float64)
    if flush:
        h = np.where(np.abs(h) < 2.0 ** -14, 0.0, h)
    return h


def split(x, flush):
    """hi = f16(x), lo = f16(x - hi)."""
    x = np.asarray(x, dtype=np.float64)
    hi = f16(x, flush)
    return hi, f16(x - hi, flush)


def mm3(a, b, flush):
    """a @ b with both operands as fp16 pairs: hi hi + hi lo + lo hi, formed and summed in f64."""
    ah, al = split(a, flush)
    bh, bl = split(b, flush)
    return ah @ bh + ah @ bl + al @ bh


def _board(rec):
    """(A + I) as a dense 0/1 matrix and the closed degrees of one board graph."""
    V = int(rec[70]) ** 2
    e = og.board_edges(rec)
    A = np.zeros((V, V))
    A[e[1], e[0]] = 1.0
    A[np.arange(V), np.arange(V)] = 1.0
    return A, A.sum(1)


def forward_split(params, recs, flush=False):
    """The default 9x9 forward as the split kernels arrange it (csrc/gcn_trunk_body.hpp, gcn_heads_split.hpp), operand by operand:
      layer 1, aggregate first   G' = (A + I) D^-1/2 X as a pair;  Q1 = relu(G' (c W1)^T + c sqrt(deg) b1)      [c = CQ]
      layers 2, 3                U = Q (W / c)^T with both operands as pairs;  V = (A + I) diag(c / deg) U + c sqrt(deg) b with U
                                 as a pair and c / deg exact in fp16;  Q = relu(V), the image c sqrt(deg) H of the activations
      pool                       mean of D^-1/2 Q3 / c, in f32
      heads                      pooled and both hidden layers as pairs against the pairs of policy_head.0 / value_head.0 /
                                 policy_head.2;  value_head.2 in f32.
    Everything between two splits is f64: what is stated is the split alone, not the kernels' f32 accumulation (which costs the
    same few 1e-8 at every scale)."""
    f32 = lambda a: np.asarray(a, dtype=np.float64)
    p = {k: np.asarray(v, dtype=np.float64) for k, v in params.items()}
    W1c = CQ * p["gcn_layers.0.lin.weight"]
    Wc = [None, p["gcn_layers.1.lin.weight"] / CQ, p["gcn_layers.2.lin.weight"] / CQ]
    pooled = []
    for rec in np.asarray(recs, dtype=np.uint8).reshape(-1, 72):
        A, deg = _board(rec)
        sq = np.sqrt(deg)
        tb = lambda l: CQ * p[f"gcn_layers.{l}.bias"][None, :] * sq[:, None]
        G = (A @ (og.node_features(rec) / sq[:, None]))
        Q = (np.maximum(mm3(G, W1c.T, flush) + tb(0), 0.0))
        for l in (1, 2):
            U = (mm3(Q, Wc[l].T, flush))
            uh, ul = split(U, flush)
            Ac = A * (CQ / deg)[None, :]                    # exact in fp16: 0.9375, 0.46875, 0.3125, 0.234375, 0.1875
            Q = (np.maximum(Ac @ uh + Ac @ ul + tb(l), 0.0))
        pooled.append((Q / (CQ * sq)[:, None]).mean(0))
    g = np.stack(pooled)
    hp = (np.maximum(mm3(g, p["policy_head.0.weight"].T, flush) + p["policy_head.0.bias"], 0.0))
    logits = mm3(hp, p["policy_head.2.weight"].T, flush) + p["policy_head.2.bias"]
    hv = (np.maximum(mm3(g, p["value_head.0.weight"].T, flush) + p["value_head.0.bias"], 0.0))
    vpre = hv @ p["value_head.2.weight"].T + p["value_head.2.bias"]
    return dict(logits=logits, value_pre=vpre[:, 0])


def bar_ratio(got, ref, atol, rtol):
    """Worst |got - ref| as a multiple of the bar atol + rtol |ref| (NaN counts as infinitely far)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    r = np.abs(got - ref) / (atol + rtol * np.abs(ref))
    return float(np.where(np.isfinite(r), r, np.inf).max()) if r.size else 0.0
