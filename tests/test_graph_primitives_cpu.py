"""CPU half (no GPU) of the width-generic graph primitives' contract test (include/aqgnn.h, "width-generic graph primitives";
tests/test_graph_primitives.py is the GPU half and imports everything below).

Here live the case lists, the input generators, the plain numpy references in float64, and the host statement of "a k-ordered
fmaf chain" (tests/hostcheck/fmaf_chain.cpp).  The tests in this file check the references against an independent statement
(torch float64: nn.functional.linear, index_add_, softmax, autograd), check that every exact-input case stays below 2^24, and
check aqg_graph_linear_grad_workspace_floats, which is host arithmetic.

Two kinds of input:
  exact  every operand is an integer in [-3, 3] stored as f32.  Every partial sum is then an integer below 2^24, so the f32 result
         is exact in ANY summation order and must equal the float64 reference (itself exact: integers below 2^53) bit for bit.
  real   standard-normal operands, compared element-wise with float64 under |got - ref| <= (n + 3) 2^-24 S: n the number of
         terms, S the same expression on absolute values.  An n-term f32 dot product in any order (with or without fused
         multiply-adds) errs by at most n u S (Jeannerod & Rump 2013, no higher-order term); the bias, the accumulate and a division
         add one rounding each.  ReLU and the mask are exact and 1-Lipschitz, so the bound survives them."""
import ctypes
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
if REPO not in sys.path:
    sys.path.insert(0, REPO)

U32 = 2.0 ** -24                 # unit roundoff of f32
EXACT_LIMIT = 2 ** 24            # integers up to here are f32
RELU, W_KN, ACC = 1, 2, 4        # AQG_LIN_* (include/aqgnn.h)

# ---------------------------------------------------------------------------------------------------------------- case lists
# aqg_graph_linear, (M, K, N): the 64x64 output tile's row and column tails, the K slab of 32 and its contraction in 4s
LIN_EDGE_M = [1, 63, 64, 65, 129]
LIN_EDGE_N = [1, 15, 16, 17, 63, 64, 65, 130]
LIN_EDGE_K = [0, 1, 3, 4, 5, 31, 32, 33, 64, 100]
LIN_EDGE = [(m, k, n) for m in LIN_EDGE_M for k in LIN_EDGE_K for n in LIN_EDGE_N]
LIN_FLAG_SHAPES = [(65, 33, 65), (129, 100, 17)]
LIN_FLAG_CASES = [(s, f, b, m) for s in LIN_FLAG_SHAPES for f in range(8) for b in (True, False) for m in (True, False)]
LIN_LARGE = [((10368, 54, 128), 0), ((10368, 1152, 128), 0), ((648, 4608, 512), 0), ((128, 512, 4096), 0), ((128, 128, 1), 0),
             ((331776, 6, 64), 0), ((10368, 128, 1152), W_KN), ((648, 512, 4608), W_KN), ((128, 4096, 512), W_KN),
             ((128, 1, 512), W_KN | ACC)]
LIN_FMAF = [(65, 100, 65), (648, 4608, 64)]
# aqg_graph_linear_grad, (M, K, N)
GRAD_EDGE_NK = [1, 63, 64, 65, 130]
GRAD_EDGE_M = [1, 31, 32, 33, 100]
GRAD_EDGE = [(m, k, n) for m in GRAD_EDGE_M for k in GRAD_EDGE_NK for n in GRAD_EDGE_NK]
GRAD_CHUNK_BASES = [(1000, 7, 5), (17000, 7, 5)]      # (M the chunking is derived at, K, N): 32 and 64 rows per chunk
GRAD_LARGE = [(10368, 1152, 128), (648, 4608, 512), (128, 512, 4096), (331776, 6, 64)]
GRAD_NULL_SHAPE = (100, 65, 63)
# aqg_graph_aggregate / mean pool / heads
AGG_N = [1, 2, 3, 4, 6, 63, 64, 65, 255, 256, 257, 260, 1024]
AGG_ALIGN_N = [64, 6, 65]                              # a multiple of 4, of 2 only, odd: the 4 / 2 / 1-wide kernels
POOL_N = [1, 255, 256, 257, 1024]
POOL_COUNTS = [0, 1, 2, 0, 0, 2100, 5, 0]              # empty graphs first, last and twice in a row; 1, 2 and 2,100 nodes
HEADS_A = [1, 2, 63, 64, 255, 256, 257, 1000, 4096]
HUB = 2100


def flags_id(f):
    return "+".join(n for b, n in ((RELU, "relu"), (W_KN, "wkn"), (ACC, "acc")) if f & b) or "plain"


def mkn_id(s):
    return "M%d-K%d-N%d" % tuple(s)


# ---------------------------------------------------------------------------------------------------------------- inputs
def ints(rng, shape):
    """Exact inputs: integers in [-3, 3] as f32."""
    return rng.integers(-3, 4, size=shape).astype(np.float32)


def reals(rng, shape):
    return rng.standard_normal(shape).astype(np.float32)


def draw(rng, shape, exact):
    return ints(rng, shape) if exact else reals(rng, shape)


def make_mask(rng, shape):
    """A ReLU-backward mask whose entries include 0, -0.0, negatives and NaN (all of them "not > 0") beside positives."""
    vals = np.array([1.0, 0.5, 3.0, 0.0, -0.0, -1.0, -0.25, np.nan], dtype=np.float32)
    m = vals[rng.integers(0, len(vals), size=shape)]
    flat = m.reshape(-1)
    flat[:min(len(vals), flat.size)] = vals[:flat.size]        # every kind is present whatever the draw
    return m


def flag_inputs(shape, flags, has_bias, has_mask, exact, seed=0):
    """Inputs of one flag case.  The initial Y is large against acc + bias in a good share of elements, so that the documented
    order (accumulate, then ReLU, then mask) is observable: X is sparse in the exact variant (Y0 is confined to [-3, 3]) and Y0 is
    scaled to the sum's spread in the real one."""
    M, K, N = shape
    rng = np.random.default_rng(1000 * seed + 8 * (M + K + N) + flags)
    X = draw(rng, (M, K), exact)
    if exact:
        X = X * (rng.random((M, K)) < 2.0 / max(K, 1)).astype(np.float32)
    W = draw(rng, (K, N) if flags & W_KN else (N, K), exact)
    bias = draw(rng, (N,), exact) if has_bias else None
    Y0 = draw(rng, (M, N), exact)
    if not exact:
        Y0 = (Y0 * np.float32(np.sqrt(K))).astype(np.float32)
    mask = make_mask(rng, (M, N)) if has_mask else None
    return X, W, bias, mask, Y0


def make_csr(rng, exact, n=41):
    """A CSR over n nodes with rows of 0, 1 and 5 entries and one 2,100-entry hub, repeated sources, and csr_src = -1 entries at the
    start, in the middle and at the end of a row.  The -1 entries carry weights like any other (NaN and inf among them in the real
    variant): they are skipped whatever their weight."""
    kinds = ["empty", "one", "five", "skip_first", "skip_mid", "skip_last", "hub", "skip_all"]
    ptr, src = [0], []
    for i in range(n):
        kind = kinds[i % len(kinds)]
        if kind == "hub" and i != 6:                            # one hub only
            kind = "five"
        cnt = {"empty": 0, "one": 1, "hub": HUB}.get(kind, 5)
        s = rng.integers(0, n, size=cnt)
        if cnt == 5:
            s[1] = s[3]                                         # a repeated source
        neg = {"skip_first": [0], "skip_mid": [2], "skip_last": [4], "skip_all": [0, 1, 2, 3, 4],
               "hub": [0, 7, 1000, 1001, HUB - 1]}.get(kind, [])
        s[neg] = -1
        src.extend(s.tolist())
        ptr.append(len(src))
    src = np.asarray(src, dtype=np.int32)
    w = draw(rng, (len(src),), exact)
    if exact:
        w[src < 0] = 3.0
    else:
        w[src < 0] = np.resize(np.array([np.nan, np.inf, -np.inf, 1e30], dtype=np.float32), int((src < 0).sum()))
    return np.asarray(ptr, dtype=np.int32), src, w


def graph_ptr_of(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def heads_inputs(rng, A, G=9):
    """Logit rows that break a naive softmax: plain rows, rows shifted by +-90 (expf overflows / underflows without the max
    subtraction), a row with one dominant logit (the others underflow to exactly 0), a constant row; value_pre incl. 0 and
    saturating values.  Apart from those exact zeros every probability stays a normal f32 (a row spans well under 87 = ln 2^126):
    the derived bound of the backward models rounding, not underflow, and a subnormal probability would carry an absolute error
    the bound does not describe."""
    L = reals(rng, (G, A)) * np.float32(2.0)
    L[1] += np.float32(90.0)
    L[2] -= np.float32(90.0)
    L[3] = 0.0
    L[3, A // 2] = 120.0
    L[4] = np.float32(-1.5)
    L[5] = L[5] * np.float32(2.0) + np.float32(90.0)
    vpre = (reals(rng, (G,)) * np.float32(2.0))
    vpre[0], vpre[1], vpre[2] = 0.0, 20.0, -20.0
    return L, vpre


# ---------------------------------------------------------------------------------------------------------------- references
def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def ref_linear(X, W, bias=None, mask=None, flags=0, Y0=None):
    """aqg_graph_linear in float64 -> (Y, S, n): S the same expression on absolute values (before ReLU / mask), n = K."""
    X, W, bias, Y0 = _f64(X), _f64(W), _f64(bias), _f64(Y0)
    Wt = W if flags & W_KN else W.T
    v, S = X @ Wt, np.abs(X) @ np.abs(Wt)
    if bias is not None:
        v, S = v + bias, S + np.abs(bias)
    if flags & ACC:
        v, S = Y0 + v, S + np.abs(Y0)
    if flags & RELU:
        v = np.maximum(v, 0.0)
    if mask is not None:
        with np.errstate(invalid="ignore"):
            v = np.where(np.asarray(mask) > 0, v, 0.0)
    return v, S, X.shape[1]


def ref_linear_grad(dY, X, dYb=None):
    """aqg_graph_linear_grad in float64 -> (dW, db, S_dW, S_db, n = M)."""
    dY, X = _f64(dY), _f64(X)
    dYb = dY if dYb is None else _f64(dYb)
    return dY.T @ X, dYb.sum(0), np.abs(dY).T @ np.abs(X), np.abs(dYb).sum(0), dY.shape[0]


def ref_aggregate(Y, ptr, src, w, bias=None, relu=False):
    """aqg_graph_aggregate in float64 -> (out, S, n [rows]): entries with src < 0 are skipped, whatever their weight."""
    Y, bias = _f64(Y), _f64(bias)
    n_nodes, N = Y.shape
    out, S, terms = np.zeros((n_nodes, N)), np.zeros((n_nodes, N)), np.zeros(n_nodes)
    for i in range(n_nodes):
        for e in range(int(ptr[i]), int(ptr[i + 1])):
            if src[e] < 0:
                continue
            out[i] += float(w[e]) * Y[src[e]]
            S[i] += abs(float(w[e])) * np.abs(Y[src[e]])
            terms[i] += 1
    if bias is not None:
        out, S = out + bias, S + np.abs(bias)
    if relu:
        out = np.maximum(out, 0.0)
    return out, S, terms


def ref_mean_pool(H, gptr):
    """aqg_graph_mean_pool -> (sums float64 [G,N], counts int64 [G], S = sums of |H|); the mean is sums / counts, 0 when empty."""
    H = _f64(H)
    G = len(gptr) - 1
    sums, S = np.zeros((G, H.shape[1])), np.zeros((G, H.shape[1]))
    for g in range(G):
        sums[g] = H[gptr[g]:gptr[g + 1]].sum(0)
        S[g] = np.abs(H[gptr[g]:gptr[g + 1]]).sum(0)
    return sums, np.diff(np.asarray(gptr, dtype=np.int64)), S


def pool_expected_f32(sums, counts):
    """What the kernel must give when the sum is exact: one correctly rounded f32 division (0 for an empty graph)."""
    c = np.maximum(counts, 1).astype(np.float32)[:, None]
    return np.where(counts[:, None] > 0, sums.astype(np.float32) / c, np.float32(0.0)).astype(np.float32)


def ref_mean_pool_backward(dpooled, gptr, mask=None):
    """aqg_graph_mean_pool_backward as f32: dH[i] = dpooled[g(i)] / |g(i)| -- one correctly rounded f32 division per element, so
    the expected value is exact -- zeroed where the mask is not > 0."""
    counts = np.diff(np.asarray(gptr, dtype=np.int64))
    g = np.repeat(np.arange(len(counts)), counts)               # node -> graph, across the empty ones
    d = (np.asarray(dpooled, dtype=np.float32)[g] / counts[g].astype(np.float32)[:, None]).astype(np.float32)
    if mask is not None:
        with np.errstate(invalid="ignore"):
            d = np.where(np.asarray(mask) > 0, d, np.float32(0.0)).astype(np.float32)
    return d


def ref_heads(logits, vpre=None):
    L = _f64(logits)
    e = np.exp(L - L.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True), (None if vpre is None else np.tanh(_f64(vpre)))


def ref_heads_backward(policy, dpolicy, value, dvalue):
    """-> (dlogits, S_dlogits, dvpre, S_dvpre) in float64 from the given policy / value."""
    p, dp, v, dv = _f64(policy), _f64(dpolicy), _f64(value), _f64(dvalue)
    s = (dp * p).sum(1, keepdims=True)
    sa = (np.abs(dp) * np.abs(p)).sum(1, keepdims=True)
    return p * (dp - s), np.abs(p) * (np.abs(dp) + sa), dv * (1.0 - v * v), np.abs(dv) * (1.0 + v * v)


def bound(n, S):
    """The derived element-wise tolerance (n + 3) 2^-24 S."""
    return (np.asarray(n, dtype=np.float64) + 3.0) * U32 * S


def worst_ratio(got, ref, n, S):
    """max |got - ref| / bound over the elements (0 / 0 counts as 0; a non-zero error at a zero bound is inf)."""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    b = np.broadcast_to(bound(n, S), err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / b)
    return float(r.max()) if r.size else 0.0


# the largest |partial sum| an exact-input case can reach: 9 per term, 3 for the bias, 3 for the initial Y
def exact_bound_linear(K):
    return 9 * K + 6


def exact_bound_grad(M):
    return 9 * M


# ---------------------------------------------------------------------------------------------------------------- fmaf chain
_fc = None


def fmaf_chain():
    """tests/hostcheck/fmaf_chain.cpp, built the way tests/_util.hostcheck() builds its library."""
    global _fc
    if _fc is None:
        src = os.path.join(HERE, "hostcheck", "fmaf_chain.cpp")
        so = os.path.join(HERE, "hostcheck", "libfmafchain.so")
        if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, src])
        _fc = ctypes.CDLL(so)
    return _fc


def fmaf_linear(X, W, bias=None, w_kn=False):
    """Y = X W^T (+ bias) as a k-ordered std::fmaf chain in f32 on the host."""
    X, W = np.ascontiguousarray(X, dtype=np.float32), np.ascontiguousarray(W, dtype=np.float32)
    M, K = X.shape
    N = W.shape[1] if w_kn else W.shape[0]
    Y = np.empty((M, N), dtype=np.float32)
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    b = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
    fn = fmaf_chain().fc_linear
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 3 + [ctypes.c_int, ctypes.c_void_p]
    assert fn(M, K, N, p(X), p(W), p(b), int(w_kn), p(Y)) == 0
    return Y


# ================================================================================================================ the tests
def _t(a):
    return None if a is None else torch.from_numpy(np.asarray(a, dtype=np.float64))


@pytest.mark.parametrize("flags", range(8), ids=flags_id)
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "real"])
def test_ref_linear_against_torch(flags, exact):
    """ref_linear against torch float64: nn.functional.linear, then add / relu / where in the documented order."""
    for shape in [(5, 0, 3), (7, 9, 4)] + LIN_FLAG_SHAPES:
        X, W, bias, mask, Y0 = flag_inputs(shape, flags, True, True, exact)
        got, S, n = ref_linear(X, W, bias, mask, flags, Y0)
        v = F.linear(_t(X), _t(W).T if flags & W_KN else _t(W), _t(bias))
        if flags & ACC:
            v = _t(Y0) + v
        if flags & RELU:
            v = torch.relu(v)
        v = torch.where(torch.from_numpy(mask) > 0, v, torch.zeros_like(v))
        np.testing.assert_allclose(got, v.numpy(), rtol=1e-13, atol=1e-13)
        assert n == shape[1] and S.shape == got.shape and (S >= np.abs(got) - 1e-9).all()
        if exact:
            assert np.array_equal(got, np.rint(got))


@pytest.mark.parametrize("case", LIN_FLAG_CASES, ids=lambda c: f"{mkn_id(c[0])}-{flags_id(c[1])}-{'b' if c[2] else 'nob'}-{'m' if c[3] else 'nom'}")
def test_flag_inputs_make_the_order_observable(case):
    """The flag cases' inputs: in a good share of elements Y0 + acc + b changes sign against acc + b, ReLU-then-accumulate differs
    from accumulate-then-ReLU, and a mask laid before the ReLU / accumulate would differ from one laid after."""
    shape, flags, has_bias, has_mask = case
    for exact in (True, False):
        X, W, bias, mask, Y0 = flag_inputs(shape, flags, has_bias, has_mask, exact)
        pre, _, _ = ref_linear(X, W, bias, None, flags & W_KN)
        flips = np.mean(np.sign(Y0 + pre) != np.sign(pre))
        wrong_order = np.mean(np.maximum(pre, 0.0) + Y0 != np.maximum(Y0 + pre, 0.0))
        assert flips >= 0.1 and wrong_order >= 0.3, (flips, wrong_order)
        if has_mask:
            with np.errstate(invalid="ignore"):
                dead = ~(mask > 0)
            assert np.isnan(mask).any() and (mask < 0).any() and (mask == 0).any() and np.signbit(mask[mask == 0]).any()
            assert 0.3 <= dead.mean() <= 0.8 and np.mean(dead & (Y0 != 0)) >= 0.2      # mask-then-accumulate would leave Y0 there


def test_ref_linear_grad_against_autograd():
    """ref_linear_grad against autograd through nn.functional.linear in float64 (dYb = dY), and db from a separate dYb."""
    rng = np.random.default_rng(1)
    for (M, K, N), exact in itertools.product([(1, 1, 1), (33, 5, 7), (100, 65, 63)], (True, False)):
        dY, X, dYb = draw(rng, (M, N), exact), draw(rng, (M, K), exact), draw(rng, (M, N), exact)
        W = torch.zeros((N, K), dtype=torch.float64, requires_grad=True)
        b = torch.zeros((N,), dtype=torch.float64, requires_grad=True)
        F.linear(_t(X), W, b).backward(_t(dY))
        dW, db, SW, Sb, n = ref_linear_grad(dY, X)
        np.testing.assert_allclose(dW, W.grad.numpy(), rtol=1e-13, atol=1e-13)
        np.testing.assert_allclose(db, b.grad.numpy(), rtol=1e-13, atol=1e-13)
        assert n == M and (SW >= np.abs(dW) - 1e-9).all() and (Sb >= np.abs(db) - 1e-9).all()
        dW2, db2, _, _, _ = ref_linear_grad(dY, X, dYb)
        assert np.array_equal(dW2, dW)
        np.testing.assert_allclose(db2, _t(dYb).sum(0).numpy(), rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "real"])
def test_ref_aggregate_against_index_add(exact):
    """ref_aggregate against torch float64 index_add_ over the kept entries; the CSR has the rows the contract names."""
    rng = np.random.default_rng(2)
    ptr, src, w = make_csr(rng, exact)
    n = len(ptr) - 1
    lens = np.diff(ptr)
    assert {0, 1, 5, HUB} <= set(lens.tolist()) and (src < 0).sum() >= 10
    # -1 at the start, in the middle and at the end of some row
    firsts = [src[ptr[i]] < 0 for i in range(n) if lens[i] == 5]
    lasts = [src[ptr[i + 1] - 1] < 0 for i in range(n) if lens[i] == 5]
    mids = [src[ptr[i] + 2] < 0 and src[ptr[i]] >= 0 for i in range(n) if lens[i] == 5]
    assert any(firsts) and any(lasts) and any(mids)
    hub = int(np.flatnonzero(lens == HUB)[0])
    hs = src[ptr[hub]:ptr[hub + 1]]
    assert hs[0] < 0 and hs[-1] < 0 and hs[1000] < 0 and len(np.unique(hs[hs >= 0])) < (hs >= 0).sum()    # repeated sources
    if not exact:
        assert np.isnan(w[src < 0]).any() and np.isinf(w[src < 0]).any()
    for N in (1, 6, 65):
        Y, bias = draw(rng, (n, N), exact), draw(rng, (N,), exact)
        dst = np.repeat(np.arange(n), lens)
        keep = src >= 0
        t = torch.zeros((n, N), dtype=torch.float64).index_add_(
            0, torch.from_numpy(dst[keep]), _t(w[keep])[:, None] * _t(Y)[torch.from_numpy(src[keep].astype(np.int64))])
        cnt = np.bincount(dst[keep], minlength=n)
        out, S, terms = ref_aggregate(Y, ptr, src, w, bias, relu=True)
        np.testing.assert_allclose(out, torch.relu(t + _t(bias)).numpy(), rtol=1e-12, atol=1e-12)
        assert np.array_equal(terms, cnt) and np.isfinite(out).all() and np.isfinite(S).all()
        out2, _, _ = ref_aggregate(Y, ptr, src, w)
        np.testing.assert_allclose(out2, t.numpy(), rtol=1e-12, atol=1e-12)
        if exact:
            assert S.max() + 3 < EXACT_LIMIT and np.array_equal(out, np.rint(out))


def test_ref_mean_pool_against_index_add_and_autograd():
    """ref_mean_pool against index_add_ / counts, and ref_mean_pool_backward against autograd through that mean (to f32
    rounding: the reference is the single f32 division the kernel performs)."""
    rng = np.random.default_rng(3)
    gptr = graph_ptr_of(POOL_COUNTS)
    n, G = int(gptr[-1]), len(POOL_COUNTS)
    assert POOL_COUNTS[0] == 0 and POOL_COUNTS[-1] == 0 and (0, 0) in zip(POOL_COUNTS, POOL_COUNTS[1:]) and HUB in POOL_COUNTS
    batch = torch.from_numpy(np.repeat(np.arange(G), POOL_COUNTS))
    for exact in (True, False):
        H = draw(rng, (n, 5), exact)
        Ht = _t(H).requires_grad_()
        cnt = torch.zeros(G, dtype=torch.float64).index_add_(0, batch, torch.ones(n, dtype=torch.float64))
        pooled = torch.zeros((G, 5), dtype=torch.float64).index_add_(0, batch, Ht) / cnt.clamp(min=1.0)[:, None]
        sums, counts, S = ref_mean_pool(H, gptr)
        assert np.array_equal(counts, cnt.numpy().astype(np.int64))
        np.testing.assert_allclose(sums / np.maximum(counts, 1)[:, None], pooled.detach().numpy(), rtol=1e-13, atol=1e-13)
        exp = pool_expected_f32(sums, counts)
        assert exp.dtype == np.float32 and (exp[np.asarray(POOL_COUNTS) == 0] == 0).all()
        if exact:
            assert S.max() < EXACT_LIMIT and np.array_equal(sums, np.rint(sums))
        dpooled = draw(rng, (G, 5), exact)
        pooled.backward(_t(dpooled))
        dH = ref_mean_pool_backward(dpooled, gptr)
        assert dH.dtype == np.float32 and dH.shape == (n, 5)
        np.testing.assert_allclose(dH, Ht.grad.numpy(), rtol=2 * U32, atol=0)
        mask = make_mask(rng, (n, 5))
        with np.errstate(invalid="ignore"):
            keep = mask > 0
        dHm = ref_mean_pool_backward(dpooled, gptr, mask)
        assert np.array_equal(dHm[keep], dH[keep]) and (dHm[~keep] == 0).all()


def test_ref_heads_against_softmax_and_autograd():
    """ref_heads against torch float64 softmax / tanh on the rows that break a naive softmax, and ref_heads_backward against
    autograd through them."""
    rng = np.random.default_rng(4)
    for A in (1, 2, 63, 257):
        L, vpre = heads_inputs(rng, A)
        p, v = ref_heads(L, vpre)
        Lt, vt = _t(L).requires_grad_(), _t(vpre).requires_grad_()
        pt, vv = torch.softmax(Lt, 1), torch.tanh(vt)
        np.testing.assert_allclose(p, pt.detach().numpy(), rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(v, vv.detach().numpy(), rtol=1e-13, atol=0)
        assert np.isfinite(p).all() and np.allclose(p.sum(1), 1.0, atol=1e-12)
        if A > 1:
            assert p[3, A // 2] == 1.0 and np.float32(np.exp(-120.0)) == 0.0     # the others underflow in f32
        assert np.allclose(p[4], 1.0 / A)
        assert (np.ptp(np.delete(L, 3, 0), axis=1) < 60).all()                   # no subnormal probability (see heads_inputs)
        dp, dv = reals(rng, (L.shape[0], A)), reals(rng, (L.shape[0],))
        (pt * _t(dp)).sum().backward()
        (vv * _t(dv)).sum().backward()
        dl, Sl, dvp, Sv = ref_heads_backward(p, dp, v, dv)
        np.testing.assert_allclose(dl, Lt.grad.numpy(), rtol=1e-9, atol=1e-15)
        np.testing.assert_allclose(dvp, vt.grad.numpy(), rtol=1e-9, atol=1e-15)
        assert (Sl >= np.abs(dl) - 1e-12).all() and (Sv >= np.abs(dvp) - 1e-12).all()


def test_every_exact_case_stays_below_2_pow_24():
    """Every exact-input case of the GPU file: the largest |partial sum| it can reach is below 2^24, so f32 holds every partial
    sum exactly in any order."""
    for (M, K, N) in LIN_EDGE + LIN_FLAG_SHAPES + [s for s, _ in LIN_LARGE]:
        assert exact_bound_linear(K) < EXACT_LIMIT, (M, K, N)
    assert max(exact_bound_linear(K) for (_, K, _), _ in LIN_LARGE) == 9 * 4608 + 6
    grad_ms = [M for M, _, _ in GRAD_EDGE + GRAD_LARGE] + [M + 64 for M, _, _ in GRAD_CHUNK_BASES] + [GRAD_NULL_SHAPE[0]]
    for M in grad_ms:
        assert exact_bound_grad(M) < EXACT_LIMIT, M
    assert max(grad_ms) == 331776 and exact_bound_grad(331776) == 2985984
    assert 9 * HUB + 3 < EXACT_LIMIT and 3 * max(POOL_COUNTS) < EXACT_LIMIT         # aggregate's hub row, the largest pooled graph
    # and the data obeys the premise: integers in [-3, 3]
    a = ints(np.random.default_rng(0), (1000,))
    assert a.dtype == np.float32 and set(a.tolist()) == {-3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 3.0}


def test_case_lists_are_the_issue_s():
    assert len(LIN_EDGE) == 5 * 10 * 8 and len(set(LIN_EDGE)) == 400
    assert len(LIN_FLAG_CASES) == 64 and len(GRAD_EDGE) == 125 and len(LIN_LARGE) == 10


def _rows_per_chunk(M, chunks):
    return -(-(-(-M // chunks)) // 32) * 32


def test_linear_grad_workspace_floats_is_whole_chunks():
    """aqg_graph_linear_grad_workspace_floats is host arithmetic: a whole number of [N K + N] partial tiles, between 1 and 512 of
    them and never more than ceil(M / 32); 0 when any size is 0; and rows per chunk x chunks covers M."""
    from alphaquoridorgnn_amd import _lib
    fn = _lib.load().aqg_graph_linear_grad_workspace_floats
    Ms = [0, 1, 31, 32, 33, 100, 1000, 1023, 1024, 1025, 16384, 16385, 17000, 100000, 331776]
    Ns = [0, 1, 5, 63, 64, 65, 130, 512, 4096]
    Ks = [0, 1, 6, 7, 64, 65, 1152, 4608]
    seen = set()
    for M, N, K in itertools.product(Ms, Ns, Ks):
        ws = int(fn(M, N, K))
        if M == 0 or N == 0 or K == 0:
            assert ws == 0, (M, N, K)
            continue
        part = N * K + N
        assert ws % part == 0, (M, N, K, ws)
        chunks = ws // part
        assert 1 <= chunks <= 512 and chunks <= -(-M // 32), (M, N, K, chunks)
        rows = _rows_per_chunk(M, chunks)
        assert rows % 32 == 0 and rows * chunks >= M and rows * (chunks - 1) < M, (M, N, K, chunks, rows)
        seen.add(chunks)
    assert 1 in seen and 512 in seen and len(seen) > 10
    assert int(fn(331776, 4096, 4608)) == 4096 * 4608 + 4096            # one tile larger than the partial budget: one chunk
    for M, K, N in GRAD_CHUNK_BASES:                                     # the chunk-edge cases of the GPU file have several chunks
        assert int(fn(M, N, K)) // (N * K + N) > 1


def test_fmaf_chain_helper_is_exact_on_integers():
    """The host fmaf chain on exact inputs equals the float64 reference bit for bit, in both weight layouts, with and without bias,
    at K = 0 too; and on real inputs it stays within the derived bound of float64."""
    rng = np.random.default_rng(5)
    for (M, K, N), w_kn, has_bias in itertools.product([(3, 0, 4), (5, 1, 3), (17, 100, 9), (4, 4608, 5)], (False, True), (False, True)):
        X, W = ints(rng, (M, K)), ints(rng, (K, N) if w_kn else (N, K))
        bias = ints(rng, (N,)) if has_bias else None
        ref, _, _ = ref_linear(X, W, bias, None, W_KN if w_kn else 0)
        got = fmaf_linear(X, W, bias, w_kn)
        assert got.dtype == np.float32 and np.array_equal(got, ref), (M, K, N, w_kn, has_bias)
        X, W = reals(rng, (M, K)), reals(rng, (K, N) if w_kn else (N, K))
        ref, S, n = ref_linear(X, W, bias, None, W_KN if w_kn else 0)
        assert worst_ratio(fmaf_linear(X, W, bias, w_kn), ref, n, S) <= 1.0
    # a chain, not a sum of rounded products: 1 + 2^-12 squared keeps its 2^-24 term only under fmaf
    x = np.array([[1.0, 1 + 2.0 ** -12]], dtype=np.float32)
    w = np.array([[-1.0, 1 + 2.0 ** -12]], dtype=np.float32)
    assert fmaf_linear(x, w)[0, 0] == np.float32(2.0 ** -11 + 2.0 ** -24)
