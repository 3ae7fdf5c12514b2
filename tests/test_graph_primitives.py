"""The width-generic graph primitives (csrc/gcn_general.hip; include/aqgnn.h, "width-generic graph primitives"), each called
alone and compared with the plain float64 numpy references of tests/test_graph_primitives_cpu.py: at the tile, slab and chunk
edges, in every flag / NULL form, at the project's own large shapes, with sentinel-guarded outputs.

Every contraction and sum runs on two kinds of input (see the CPU file's docstring): exact integer inputs that must match bit for
bit in any summation order, and standard-normal inputs under the derived bound (n + 3) 2^-24 S.  Each test prints the worst
observed ratio to that bound ("worst")."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import _util as U                                                                          # noqa: E402
from tests.test_graph_primitives_cpu import (ACC, AGG_ALIGN_N, AGG_N, EXACT_LIMIT, GRAD_CHUNK_BASES, GRAD_EDGE,   # noqa: E402
                                             GRAD_LARGE, GRAD_NULL_SHAPE, HEADS_A, HUB, LIN_EDGE, LIN_FLAG_CASES, LIN_FMAF,
                                             LIN_LARGE, POOL_COUNTS, POOL_N, RELU, W_KN, _rows_per_chunk, draw,
                                             exact_bound_grad, exact_bound_linear, flag_inputs, flags_id, fmaf_linear,
                                             graph_ptr_of, heads_inputs, ints, make_csr, make_mask, mkn_id, pool_expected_f32,
                                             reals, ref_aggregate, ref_heads, ref_heads_backward, ref_linear, ref_linear_grad,
                                             ref_mean_pool, ref_mean_pool_backward, worst_ratio)

pytestmark = pytest.mark.gpu

BAR = dict(atol=1e-5, rtol=1e-4)       # the project's forward bar (test_predict_contract)
PAD = 300                              # guard floats on either side of an output (a multiple of 4: the view stays 16-byte aligned)
SENT = -7777.0
KINDS = [True, False]
KIND_IDS = ["exact", "real"]


@pytest.fixture(scope="module")
def dev():
    from alphaquoridorgnn_amd import _lib
    _lib.load()
    return _lib.require_gpu()


@pytest.fixture(scope="module")
def lib():
    from alphaquoridorgnn_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------- helpers
class Guarded:
    """An output of `shape` as a view into the middle of a larger buffer filled with a sentinel (the view too, unless `fill` is
    given), `off` floats past a 16-byte boundary.  intact() says whether every float around the view still holds the sentinel."""

    def __init__(self, dev, shape, fill=None, off=0):
        n = int(np.prod(shape))
        self.buf = torch.full((PAD + off + n + PAD,), SENT, dtype=torch.float32, device=dev)
        self.lo, self.hi = PAD + off, PAD + off + n
        self.view = self.buf[self.lo:self.hi].view(*shape)
        if fill is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(fill, dtype=np.float32)))
        assert self.view.data_ptr() % 16 == (4 * off) % 16

    def intact(self):
        return bool((self.buf[:self.lo] == SENT).all()) and bool((self.buf[self.hi:] == SENT).all())

    def untouched(self):
        return bool((self.buf == SENT).all())

    def host(self):
        return self.view.cpu().numpy()


def to_dev(dev, a, off=0, dtype=None):
    """numpy -> a contiguous device tensor (None stays None), `off` floats into its storage when off > 0."""
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype=dtype)))
    if off == 0:
        return t.to(dev)
    buf = torch.empty((off + t.numel() + 4,), dtype=t.dtype, device=dev)
    v = buf[off:off + t.numel()].view(*t.shape)
    v.copy_(t)
    return v


def _ptr(t):
    from alphaquoridorgnn_amd import _lib
    return _lib.ptr(t)


def _stream(dev):
    from alphaquoridorgnn_amd import _lib
    return _lib.stream_ptr(dev)


def last_error(lib):
    return lib.aqg_last_error().decode(errors="replace")


def assert_exact(got, ref, what):
    assert np.abs(ref).max(initial=0.0) < EXACT_LIMIT
    assert got.dtype == np.float32 and got.shape == ref.shape
    bad = np.flatnonzero(got.astype(np.float64).reshape(-1) != ref.reshape(-1))
    assert bad.size == 0, f"{what}: {bad.size} of {ref.size} elements differ from the exact result, first at flat index {bad[0]}: " \
                          f"{got.reshape(-1)[bad[0]]} vs {ref.reshape(-1)[bad[0]]}"


def assert_bound(got, ref, n, S, what):
    """|got - ref| <= (n + 3) 2^-24 S element-wise; returns the worst observed ratio."""
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    r = worst_ratio(got, ref, n, S)
    assert r <= 1.0, f"{what}: worst error is {r:.3g} x the derived bound"
    return r


def run_linear(lib, dev, X, W, bias=None, mask=None, flags=0, Y0=None, off=0):
    """aqg_graph_linear through the package's wrapper into a guarded Y -> the result on the host."""
    from alphaquoridorgnn_amd.pv_network_gnn import _linear
    M = X.shape[0]
    N = W.shape[1] if flags & W_KN else W.shape[0]
    g = Guarded(dev, (M, N), fill=Y0 if flags & ACC else None, off=off)
    _linear(lib, dev, to_dev(dev, X), to_dev(dev, W), to_dev(dev, bias), relu=bool(flags & RELU), mask=to_dev(dev, mask),
            w_kn=bool(flags & W_KN), out=g.view, accumulate=bool(flags & ACC))
    torch.cuda.synchronize()
    assert g.intact(), "aqg_graph_linear wrote outside Y[M, N]"
    return g.host()


def check_linear(lib, dev, X, W, bias, mask, flags, Y0, exact, what):
    got = run_linear(lib, dev, X, W, bias, mask, flags, Y0)
    ref, S, n = ref_linear(X, W, bias, mask, flags, Y0)
    if exact:
        assert exact_bound_linear(X.shape[1]) < EXACT_LIMIT
        assert_exact(got, ref, what)
        return 0.0
    return assert_bound(got, ref, n, S, what)


def run_linear_grad(lib, dev, dY, X, dYb=None, want_db=True, ws_short=0):
    """aqg_graph_linear_grad called directly into guarded dW / db -> (rc, dW, db, guards)."""
    M, N = dY.shape
    K = X.shape[1]
    nws = int(lib.aqg_graph_linear_grad_workspace_floats(M, N, K))
    ws = torch.empty((max(nws, 1),), dtype=torch.float32, device=dev)
    gW, gb = Guarded(dev, (N, K)), Guarded(dev, (N,))
    dYd, Xd, dYbd = to_dev(dev, dY), to_dev(dev, X), to_dev(dev, dYb)       # held until the synchronize below
    rc = lib.aqg_graph_linear_grad(M, K, N, _ptr(dYd), _ptr(Xd), _ptr(dYbd), _ptr(ws), nws - ws_short, _ptr(gW.view),
                                   _ptr(gb.view) if want_db else None, _stream(dev))
    torch.cuda.synchronize()
    return rc, gW.host(), gb.host(), (gW, gb)


def check_linear_grad(lib, dev, M, K, N, exact, what, seed=0, sep_b=False):
    rng = np.random.default_rng(seed)
    dY, X = draw(rng, (M, N), exact), draw(rng, (M, K), exact)
    dYb = draw(rng, (M, N), exact) if sep_b else None
    rc, dW, db, (gW, gb) = run_linear_grad(lib, dev, dY, X, dYb)
    assert rc == 0, last_error(lib)
    assert gW.intact() and gb.intact(), "aqg_graph_linear_grad wrote outside dW[N, K] / db[N]"
    rW, rb, SW, Sb, n = ref_linear_grad(dY, X, dYb)
    if exact:
        assert exact_bound_grad(M) < EXACT_LIMIT
        assert_exact(dW, rW, what + " dW")
        assert_exact(db, rb, what + " db")
        return 0.0
    return max(assert_bound(dW, rW, n, SW, what + " dW"), assert_bound(db, rb, n, Sb, what + " db"))


# ================================================================================================================ linear
@pytest.mark.parametrize("shape", LIN_EDGE, ids=mkn_id)
def test_linear_tile_and_slab_edges(dev, lib, shape):
    """The full cross of M, K, N over the 64x64 tile's tails and the K slab's edges: exact inputs with bias and, in the [K, N]
    layout, without (K = 0 gives the bias alone, or zero), and real inputs under the derived bound."""
    M, K, N = shape
    rng = np.random.default_rng(M * 1000003 + K * 1009 + N)
    X = ints(rng, (M, K))
    check_linear(lib, dev, X, ints(rng, (N, K)), ints(rng, (N,)), None, 0, None, True, "exact [N,K] + bias")
    check_linear(lib, dev, X, ints(rng, (K, N)), None, None, W_KN, None, True, "exact [K,N]")
    worst = check_linear(lib, dev, reals(rng, (M, K)), reals(rng, (N, K)), reals(rng, (N,)), None, 0, None, False, "real [N,K] + bias")
    print(f"linear {mkn_id(shape)}: worst {worst:.3g} of the bound")


@pytest.mark.parametrize("exact", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("case", LIN_FLAG_CASES,
                         ids=lambda c: f"{mkn_id(c[0])}-{flags_id(c[1])}-{'bias' if c[2] else 'nobias'}-{'mask' if c[3] else 'nomask'}")
def test_linear_flags(dev, lib, case, exact):
    """All 8 combinations of the AQG_LIN_* flags, with bias / NULL and mask / NULL.  The documented order -- accumulate, then
    ReLU, then mask -- is observable in these inputs (the CPU file checks that); mask entries 0, -0.0, negatives and NaN all zero
    the output."""
    shape, flags, has_bias, has_mask = case
    X, W, bias, mask, Y0 = flag_inputs(shape, flags, has_bias, has_mask, exact)
    worst = check_linear(lib, dev, X, W, bias, mask, flags, Y0, exact, f"{mkn_id(shape)} {flags_id(flags)}")
    if has_mask:
        got = run_linear(lib, dev, X, W, bias, mask, flags, Y0)
        with np.errstate(invalid="ignore"):
            assert (got[~(mask > 0)] == 0).all()
    print(f"linear flags {flags_id(flags)}: worst {worst:.3g} of the bound")


@pytest.mark.parametrize("exact", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("case", LIN_LARGE, ids=lambda c: f"{mkn_id(c[0])}-{flags_id(c[1])}")
def test_linear_project_shapes(dev, lib, case, exact):
    """The shapes the project itself runs: the CNN trainer's im2col GEMMs (forward, and dX in the [K, N] layout), the CNN's and
    the networks' heads, and the value head's dX accumulated into an existing gradient."""
    (M, K, N), flags = case
    rng = np.random.default_rng(M + 7 * K + 13 * N)
    X, W = draw(rng, (M, K), exact), draw(rng, (K, N) if flags & W_KN else (N, K), exact)
    bias = None if flags & W_KN else draw(rng, (N,), exact)
    Y0 = draw(rng, (M, N), exact) if flags & ACC else None
    worst = check_linear(lib, dev, X, W, bias, None, flags, Y0, exact, mkn_id((M, K, N)))
    print(f"linear {mkn_id((M, K, N))} {flags_id(flags)}: worst {worst:.3g} of the bound")


@pytest.mark.parametrize("flags", [0, W_KN], ids=flags_id)
def test_linear_rows_are_independent(dev, lib, flags):
    """Rows [a, b) of a call at M equal, bit for bit, the call on X[a:b] alone, for (a, b) off the tile boundaries: what the CNN's
    "bit-identical at any B" rests on."""
    from alphaquoridorgnn_amd.pv_network_gnn import _linear
    M, K, N = 200, 100, 65
    rng = np.random.default_rng(11)
    X, bias = to_dev(dev, reals(rng, (M, K))), to_dev(dev, reals(rng, (N,)))
    W = to_dev(dev, reals(rng, (K, N) if flags & W_KN else (N, K)))
    full = _linear(lib, dev, X, W, bias, relu=True, w_kn=bool(flags & W_KN))
    for a, b in [(0, 1), (1, 2), (3, 70), (63, 130), (65, 200), (100, 101), (199, 200)]:
        part = _linear(lib, dev, X[a:b].contiguous(), W, bias, relu=True, w_kn=bool(flags & W_KN))
        assert torch.equal(part, full[a:b]), (a, b)
    ref, S, n = ref_linear(X.cpu().numpy(), W.cpu().numpy(), bias.cpu().numpy(), None, flags | RELU)
    assert_bound(full.cpu().numpy(), ref, n, S, "full call")


@pytest.mark.parametrize("flags", [RELU, W_KN | ACC], ids=flags_id)
def test_linear_offset_pointers(dev, lib, flags):
    """X, W, bias, mask and Y as views one float into their storage (4-byte aligned only) give the aligned call's bits."""
    from alphaquoridorgnn_amd.pv_network_gnn import _linear
    shape = (65, 33, 65)
    X, W, bias, mask, Y0 = flag_inputs(shape, flags, True, True, False)
    base = run_linear(lib, dev, X, W, bias, mask, flags, Y0)
    g = Guarded(dev, (shape[0], shape[2]), fill=Y0 if flags & ACC else None, off=1)
    args = [to_dev(dev, a, off=1) for a in (X, W, bias, mask)]
    assert all(a.data_ptr() % 8 == 4 for a in args) and g.view.data_ptr() % 8 == 4
    _linear(lib, dev, args[0], args[1], args[2], relu=bool(flags & RELU), mask=args[3], w_kn=bool(flags & W_KN), out=g.view,
            accumulate=bool(flags & ACC))
    torch.cuda.synchronize()
    assert g.intact() and np.array_equal(g.host(), base)


@pytest.mark.parametrize("shape", LIN_FMAF, ids=mkn_id)
def test_linear_is_a_k_ordered_fmaf_chain(dev, lib, shape):
    """include/aqgnn.h: every contraction "runs on the f32-input MFMA (a k-ordered fmaf chain)".  As stated: the result equals
    acc = fmaf(x[k], w[k], acc) over k from 0 in f32 (std::fmaf on the host), then + bias, bit for bit.  The derived bound against
    float64 is asserted beside it and does not depend on the order.  (On an MI355X the sentence holds: 0 of 4,225 and 0 of 41,472
    elements differ, in either weight layout.)"""
    M, K, N = shape
    rng = np.random.default_rng(K)
    X, W, bias = reals(rng, (M, K)), reals(rng, (N, K)), reals(rng, (N,))
    got = run_linear(lib, dev, X, W, bias)
    ref, S, n = ref_linear(X, W, bias)
    worst = assert_bound(got, ref, n, S, mkn_id(shape))
    chain = fmaf_linear(X, W, bias)
    diff = got != chain
    ulps = np.abs(got.view(np.int32).astype(np.int64) - chain.view(np.int32).astype(np.int64))
    print(f"linear {mkn_id(shape)} against the host fmaf chain: {int(diff.sum())} of {diff.size} elements differ, "
          f"largest distance {int(ulps.max())} ulp; worst {worst:.3g} of the bound against float64")
    assert not diff.any()
    got_kn = run_linear(lib, dev, X, np.ascontiguousarray(W.T), None, None, W_KN)
    assert np.array_equal(got_kn, fmaf_linear(X, W)), "[K, N] layout"


# ================================================================================================================ linear_grad
@pytest.mark.parametrize("exact", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("shape", GRAD_EDGE, ids=mkn_id)
def test_linear_grad_tile_and_row_edges(dev, lib, shape, exact):
    """N and K over the 64-wide tiles' tails, M over the 32-row staging's edges."""
    M, K, N = shape
    worst = check_linear_grad(lib, dev, M, K, N, exact, mkn_id(shape), seed=M * 100003 + K * 1009 + N)
    print(f"linear_grad {mkn_id(shape)}: worst {worst:.3g} of the bound")


@pytest.mark.parametrize("exact", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("delta", [-1, 0, 1], ids=["edge-1", "edge", "edge+1"])
@pytest.mark.parametrize("base", GRAD_CHUNK_BASES, ids=mkn_id)
def test_linear_grad_chunk_edges(dev, lib, base, delta, exact):
    """M around a chunk edge: the chunk count and the rows per chunk derived from aqg_graph_linear_grad_workspace_floats at the
    base shape, then M = rows x chunks - 1, that product and + 1."""
    M0, K, N = base
    chunks = int(lib.aqg_graph_linear_grad_workspace_floats(M0, N, K)) // (N * K + N)
    rows = _rows_per_chunk(M0, chunks)
    assert chunks > 1 and rows % 32 == 0 and rows * (chunks - 1) < M0 <= rows * chunks
    M = rows * chunks + delta
    worst = check_linear_grad(lib, dev, M, K, N, exact, f"M{M} ({chunks} chunks of {rows} rows at M{M0})", seed=M)
    print(f"linear_grad chunk edge M{M}: worst {worst:.3g} of the bound")


@pytest.mark.parametrize("exact", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("shape", GRAD_LARGE, ids=mkn_id)
def test_linear_grad_project_shapes(dev, lib, shape, exact):
    """The CNN trainer's dW GEMMs (few chunks at 512 x 4,608, the maximum at M = 331,776) and the policy head's."""
    M, K, N = shape
    worst = check_linear_grad(lib, dev, M, K, N, exact, mkn_id(shape), seed=M + K)
    print(f"linear_grad {mkn_id(shape)}: worst {worst:.3g} of the bound")


@pytest.mark.parametrize("exact", KINDS, ids=KIND_IDS)
def test_linear_grad_null_forms(dev, lib, exact):
    """dYb NULL (db from dY); dYb another tensor (db from dYb, dW still from dY); db NULL (dW alone, nothing written at db)."""
    M, K, N = GRAD_NULL_SHAPE
    worst = check_linear_grad(lib, dev, M, K, N, exact, "dYb NULL", seed=1)
    worst = max(worst, check_linear_grad(lib, dev, M, K, N, exact, "dYb separate", seed=2, sep_b=True))
    rng = np.random.default_rng(3)
    dY, X, dYb = draw(rng, (M, N), exact), draw(rng, (M, K), exact), draw(rng, (M, N), exact)
    for b in (None, dYb):
        rc, dW, _, (gW, gb) = run_linear_grad(lib, dev, dY, X, b, want_db=False)
        assert rc == 0 and gW.intact() and gb.untouched()
        rW, _, SW, _, n = ref_linear_grad(dY, X, b)
        if exact:
            assert_exact(dW, rW, "db NULL")
        else:
            worst = max(worst, assert_bound(dW, rW, n, SW, "db NULL"))
    print(f"linear_grad NULL forms: worst {worst:.3g} of the bound")


def test_linear_grad_empty_short_workspace_and_k0(dev, lib):
    """M = 0 overwrites dW and db with zeros; a workspace one float short is refused with "workspace too small" and leaves dW
    untouched; K = 0 is refused."""
    rng = np.random.default_rng(4)
    N, K = 63, 65
    rc, dW, db, (gW, gb) = run_linear_grad(lib, dev, np.zeros((0, N), np.float32), np.zeros((0, K), np.float32))
    assert rc == 0 and gW.intact() and gb.intact() and (dW == 0).all() and (db == 0).all()
    rc, dW, db, (gW, gb) = run_linear_grad(lib, dev, reals(rng, (100, N)), reals(rng, (100, K)), ws_short=1)
    assert rc != 0 and "workspace too small" in last_error(lib)
    assert gW.untouched() and gb.untouched()
    gW = Guarded(dev, (N, 1))
    ws = torch.empty((1024,), dtype=torch.float32, device=dev)
    dY = to_dev(dev, reals(rng, (100, N)))
    rc = lib.aqg_graph_linear_grad(100, 0, N, _ptr(dY), _ptr(dY), None, _ptr(ws), 1024, _ptr(gW.view), None, _stream(dev))
    torch.cuda.synchronize()
    assert rc != 0 and "K must be" in last_error(lib) and gW.untouched()


@pytest.mark.parametrize("shape", [(1025, 7, 5), (100, 65, 63), (10368, 1152, 128)], ids=mkn_id)
def test_linear_grad_is_deterministic(dev, lib, shape):
    """Two identical calls give identical bits (no atomics: partial tiles, then a fixed-order reduce)."""
    from alphaquoridorgnn_amd.pv_network_gnn import _linear_grad
    M, K, N = shape
    rng = np.random.default_rng(5)
    dY, X = to_dev(dev, reals(rng, (M, N))), to_dev(dev, reals(rng, (M, K)))
    dW1, db1 = _linear_grad(lib, dev, dY, X)
    dW2, db2 = _linear_grad(lib, dev, dY, X)
    assert torch.equal(dW1, dW2) and torch.equal(db1, db2)
    rW, rb, SW, Sb, n = ref_linear_grad(dY.cpu().numpy(), X.cpu().numpy())
    assert_bound(dW1.cpu().numpy(), rW, n, SW, "dW")
    assert_bound(db1.cpu().numpy(), rb, n, Sb, "db")


# ================================================================================================================ aggregate
def run_aggregate(lib, dev, Y, csr, bias=None, relu=0, off=0):
    """aqg_graph_aggregate called directly: Y `off` floats past a 16-byte boundary, out guarded -> out on the host."""
    ptr, src, w = csr
    n, N = Y.shape
    gY = Guarded(dev, (n, N), fill=Y, off=off)
    g = Guarded(dev, (n, N))
    ptrd, srcd, wd, biasd = to_dev(dev, ptr), to_dev(dev, src), to_dev(dev, w), to_dev(dev, bias)   # held until the synchronize
    rc = lib.aqg_graph_aggregate(n, N, _ptr(gY.view), _ptr(ptrd), _ptr(srcd), _ptr(wd), _ptr(biasd), int(relu), _ptr(g.view),
                                 _stream(dev))
    torch.cuda.synchronize()
    assert rc == 0, last_error(lib)
    assert g.intact(), "aqg_graph_aggregate wrote outside out[num_nodes, N]"
    return g.host()


@pytest.mark.parametrize("exact", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("relu", [0, 1], ids=["norelu", "relu"])
@pytest.mark.parametrize("has_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("N", AGG_N, ids=lambda n: f"N{n}")
def test_aggregate_widths_and_rows(dev, lib, N, has_bias, relu, exact):
    """Rows of 0, 1, 5 and 2,100 entries, repeated sources, csr_src = -1 entries at the start, middle and end of a row (skipped
    whatever their weight: NaN and inf in the real variant), at widths across the 4 / 2 / 1-wide kernels and the 64-lane stride."""
    rng = np.random.default_rng(N)
    csr = make_csr(rng, exact)
    n = len(csr[0]) - 1
    Y, bias = draw(rng, (n, N), exact), (draw(rng, (N,), exact) if has_bias else None)
    got = run_aggregate(lib, dev, Y, csr, bias, relu)
    ref, S, terms = ref_aggregate(Y, *csr, bias, relu)
    if exact:
        assert 9 * HUB + 3 < EXACT_LIMIT
        assert_exact(got, ref, f"N{N}")
        worst = 0.0
    else:
        worst = assert_bound(got, ref, terms[:, None], S, f"N{N}")
    print(f"aggregate N{N}: worst {worst:.3g} of the bound")


@pytest.mark.parametrize("off", [1, 2, 3])
@pytest.mark.parametrize("N", AGG_ALIGN_N, ids=lambda n: f"N{n}")
def test_aggregate_unaligned_y(dev, lib, N, off):
    """Y 1, 2 and 3 floats past a 16-byte boundary, for an N divisible by 4, by 2 only and odd: the alignment selects the 4 / 2 /
    1-wide kernel, and every one of them gives the aligned call's bits (and the exact result on exact inputs)."""
    for exact in KINDS:
        rng = np.random.default_rng(100 * N + off)
        csr = make_csr(rng, exact)
        n = len(csr[0]) - 1
        Y, bias = draw(rng, (n, N), exact), draw(rng, (N,), exact)
        base = run_aggregate(lib, dev, Y, csr, bias, 1)
        got = run_aggregate(lib, dev, Y, csr, bias, 1, off=off)
        assert np.array_equal(got, base)
        ref, S, terms = ref_aggregate(Y, *csr, bias, 1)
        if exact:
            assert_exact(got, ref, f"N{N} off {off}")
        else:
            assert_bound(got, ref, terms[:, None], S, f"N{N} off {off}")


def _boards(N):
    """A few board records: reference-walk states at 5x5, random legal play at 9x9."""
    if N == 5:
        return np.ascontiguousarray(U.golden("walk_5x5.npz")["states"][::600])
    from oracle import quoridor as oq
    rng = np.random.RandomState(3)
    recs, s = [oq.init_record(9)], oq.State()
    for _ in range(30):
        la = s.legal_actions()
        s = s.next(la[rng.randint(len(la))])
        if s.is_done():
            break
        recs.append(s.rec.copy())
    return np.stack(recs)[::5]


@pytest.mark.parametrize("N", [5, 9], ids=lambda n: f"{n}x{n}")
def test_aggregate_on_board_ell_rows(dev, lib, N):
    """The ELL rows of aqg_gcn_boards_graph as csr_ptr = 5 i: closed sides are index -1 and are skipped."""
    recs = _boards(N)
    B, R = recs.shape[0], recs.shape[0] * N * N
    assert B >= 3
    x = torch.empty((R, 6), dtype=torch.float32, device=dev)
    idx = torch.empty((R * 5,), dtype=torch.int32, device=dev)
    w = torch.empty((R * 5,), dtype=torch.float32, device=dev)
    d72 = to_dev(dev, recs)
    assert lib.aqg_gcn_boards_graph(N, _ptr(d72), B, _ptr(x), _ptr(idx), _ptr(w), _stream(dev)) == 0, last_error(lib)
    torch.cuda.synchronize()
    csr = (np.arange(0, 5 * R + 1, 5, dtype=np.int32), idx.cpu().numpy(), w.cpu().numpy())
    assert (csr[1] < 0).any() and csr[1].max() < R
    rng = np.random.default_rng(N)
    worst = 0.0
    for width in (6, 64, 65):
        Y, bias = reals(rng, (R, width)), reals(rng, (width,))
        got = run_aggregate(lib, dev, Y, csr, bias, 1)
        ref, S, terms = ref_aggregate(Y, *csr, bias, 1)
        worst = max(worst, assert_bound(got, ref, terms[:, None], S, f"{N}x{N} width {width}"))
    print(f"aggregate on {N}x{N} board rows: worst {worst:.3g} of the bound")


# ================================================================================================================ mean pool
def run_mean_pool(lib, dev, H, gptr):
    n, N = H.shape
    G = len(gptr) - 1
    g = Guarded(dev, (G, N))
    Hd, gptrd = to_dev(dev, H), to_dev(dev, gptr)                           # held until the synchronize below
    rc = lib.aqg_graph_mean_pool(n, N, _ptr(Hd), _ptr(gptrd), G, _ptr(g.view), _stream(dev))
    torch.cuda.synchronize()
    assert rc == 0, last_error(lib)
    assert g.intact(), "aqg_graph_mean_pool wrote outside pooled[num_graphs, N]"
    return g.host()


@pytest.mark.parametrize("exact", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("N", POOL_N, ids=lambda n: f"N{n}")
def test_mean_pool(dev, lib, N, exact):
    """Empty graphs first, last and twice in a row pool to zero; graphs of 1, 2 and 2,100 nodes.  With an exact sum the kernel's
    single division is the correctly rounded f32 quotient, so exact inputs are compared bit for bit."""
    gptr = graph_ptr_of(POOL_COUNTS)
    rng = np.random.default_rng(N)
    H = draw(rng, (int(gptr[-1]), N), exact)
    got = run_mean_pool(lib, dev, H, gptr)
    sums, counts, S = ref_mean_pool(H, gptr)
    assert (got[counts == 0] == 0).all()
    worst = 0.0
    if exact:
        assert S.max() < EXACT_LIMIT
        exp = pool_expected_f32(sums, counts)
        assert np.array_equal(got, exp), f"{int((got != exp).sum())} elements differ from float32(sum) / float32(count)"
    else:
        c = np.maximum(counts, 1)[:, None]
        worst = assert_bound(got, sums / c, counts[:, None], S / c, f"N{N}")
    print(f"mean_pool N{N}: worst {worst:.3g} of the bound")


@pytest.mark.parametrize("N", POOL_N, ids=lambda n: f"N{n}")
def test_mean_pool_all_graphs_empty(dev, lib, N):
    """num_nodes = 0 with H NULL: every graph is empty and pools to zero, over a sentinel-filled output."""
    got = run_mean_pool(lib, dev, np.zeros((0, N), np.float32), np.zeros(5, np.int32))
    assert got.shape == (4, N) and (got == 0).all()


@pytest.mark.parametrize("exact", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("has_mask", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("N", POOL_N, ids=lambda n: f"N{n}")
def test_mean_pool_backward(dev, lib, N, has_mask, exact):
    """dH[i] = dpooled[g(i)] / |g(i)|: every node lands in the right graph across the empty ones (the binary search), and the
    quotient is one correctly rounded f32 division -- compared bit for bit.  Mask entries 0, -0.0, negatives and NaN zero dH."""
    gptr = graph_ptr_of(POOL_COUNTS)
    n, G = int(gptr[-1]), len(POOL_COUNTS)
    rng = np.random.default_rng(N + 7)
    dpooled = draw(rng, (G, N), exact)
    mask = make_mask(rng, (n, N)) if has_mask else None
    g = Guarded(dev, (n, N))
    dpd, gptrd, maskd = to_dev(dev, dpooled), to_dev(dev, gptr), to_dev(dev, mask)
    rc = lib.aqg_graph_mean_pool_backward(n, N, _ptr(dpd), _ptr(gptrd), G, _ptr(maskd), _ptr(g.view), _stream(dev))
    torch.cuda.synchronize()
    assert rc == 0, last_error(lib)
    assert g.intact(), "aqg_graph_mean_pool_backward wrote outside dH[num_nodes, N]"
    got, exp = g.host(), ref_mean_pool_backward(dpooled, gptr, mask)
    assert np.array_equal(got, exp), f"{int((got != exp).sum())} of {exp.size} elements differ"
    # the same through the package's wrapper
    from alphaquoridorgnn_amd.pv_network_gnn import _mean_pool_backward
    via = _mean_pool_backward(lib, dev, dpd, gptrd, G, n, mask=maskd)
    assert np.array_equal(via.cpu().numpy(), exp)


# ================================================================================================================ heads
def run_heads(lib, dev, L, vpre, want_value=True):
    G, A = L.shape
    gp, gv = Guarded(dev, (G, A)), Guarded(dev, (G,))
    Ld, vd = to_dev(dev, L), to_dev(dev, vpre)                               # held until the synchronize below
    rc = lib.aqg_graph_heads(G, A, _ptr(Ld), _ptr(vd) if want_value else None, _ptr(gp.view),
                             _ptr(gv.view) if want_value else None, _stream(dev))
    torch.cuda.synchronize()
    assert rc == 0, last_error(lib)
    assert gp.intact() and gv.intact(), "aqg_graph_heads wrote outside policy[num_graphs, A] / value[num_graphs]"
    return gp.host(), gv


@pytest.mark.parametrize("A", HEADS_A, ids=lambda a: f"A{a}")
def test_heads_forward(dev, lib, A):
    """Softmax rows shifted by +-90 (expf overflows without the max subtraction), a dominant logit (the others underflow), a
    constant row; against float64 at the project's bar, row sums within 1e-5.  value_pre and value both NULL leaves value alone;
    exactly one of them NULL is refused."""
    rng = np.random.default_rng(A)
    L, vpre = heads_inputs(rng, A)
    policy, gv = run_heads(lib, dev, L, vpre)
    rp, rv = ref_heads(L, vpre)
    value = gv.host()
    print(f"heads A{A}: worst |policy - ref| {np.abs(policy - rp).max():.3g}, |value - ref| {np.abs(value - rv).max():.3g}, "
          f"|row sum - 1| {np.abs(policy.astype(np.float64).sum(1) - 1).max():.3g}")
    assert np.isfinite(policy).all() and (policy >= 0).all()
    np.testing.assert_allclose(policy, rp, **BAR)
    np.testing.assert_allclose(value, rv, **BAR)
    assert np.abs(policy.astype(np.float64).sum(1) - 1.0).max() <= 1e-5
    p2, gv2 = run_heads(lib, dev, L, None, want_value=False)
    assert np.array_equal(p2, policy) and gv2.untouched()
    Ld, vd = to_dev(dev, L), to_dev(dev, vpre)
    for vp_arg, v_arg in ((vd, False), (None, True)):
        gp, gv3 = Guarded(dev, L.shape), Guarded(dev, (L.shape[0],))
        rc = lib.aqg_graph_heads(L.shape[0], A, _ptr(Ld), _ptr(vp_arg), _ptr(gp.view), _ptr(gv3.view) if v_arg else None, _stream(dev))
        torch.cuda.synchronize()
        assert rc != 0 and "null argument" in last_error(lib) and gp.untouched() and gv3.untouched()


@pytest.mark.parametrize("A", HEADS_A, ids=lambda a: f"A{a}")
def test_heads_backward(dev, lib, A):
    """dlogits = p (dp - <dp, p>) and dvalue_pre = dv (1 - v^2) against the float64 formula on the kernel's own f32 policy /
    value, under the derived bound (n = A for dlogits; three roundings for dvalue_pre).  dpolicy NULL and dvalue NULL give zeros;
    dlogits NULL is accepted."""
    rng = np.random.default_rng(A + 1)
    L, vpre = heads_inputs(rng, A)
    G = L.shape[0]
    policy, gv = run_heads(lib, dev, L, vpre)
    value = gv.host()
    assert ((policy == 0) | (policy >= np.finfo(np.float32).tiny)).all()     # no subnormal probability: see heads_inputs
    dp, dv = reals(rng, (G, A)), reals(rng, (G,))
    pd, vd, dpd, dvd = (to_dev(dev, a) for a in (policy, value, dp, dv))

    def call(dpolicy, dvalue, want_dlogits=True):
        gl, gd = Guarded(dev, (G, A)), Guarded(dev, (G,))
        rc = lib.aqg_graph_heads_backward(G, A, _ptr(pd), _ptr(dpolicy), _ptr(vd), _ptr(dvalue), _ptr(gl.view) if want_dlogits else None,
                                          _ptr(gd.view), _stream(dev))
        torch.cuda.synchronize()
        assert rc == 0, last_error(lib)
        assert gl.intact() and gd.intact(), "aqg_graph_heads_backward wrote outside dlogits / dvalue_pre"
        return gl, gd

    gl, gd = call(dpd, dvd)
    rl, Sl, rd, Sd = ref_heads_backward(policy, dp, value, dv)
    worst_l = assert_bound(gl.host(), rl, A, Sl, f"A{A} dlogits")
    worst_v = assert_bound(gd.host(), rd, 1, Sd, f"A{A} dvalue_pre")
    print(f"heads_backward A{A}: worst {worst_l:.3g} (dlogits), {worst_v:.3g} (dvalue_pre) of the bound")
    gl0, gd0 = call(None, dvd)
    assert (gl0.host() == 0).all() and np.array_equal(gd0.host(), gd.host())
    gl1, gd1 = call(dpd, None)
    assert np.array_equal(gl1.host(), gl.host()) and (gd1.host() == 0).all()
    gl2, gd2 = call(dpd, dvd, want_dlogits=False)
    assert gl2.untouched() and np.array_equal(gd2.host(), gd.host())


# ================================================================================================================ arguments
def test_argument_checks_write_nothing(dev, lib):
    """A negative size and an unknown flag bit return non-zero and write nothing; a call with no rows or no columns returns 0 and
    launches nothing (a sentinel-filled output stays as it was)."""
    rng = np.random.default_rng(9)
    M, K, N = 5, 7, 3
    X, W, b = to_dev(dev, reals(rng, (M, K))), to_dev(dev, reals(rng, (N, K))), to_dev(dev, reals(rng, (N,)))
    st = _stream(dev)
    g = Guarded(dev, (M, N))
    y = _ptr(g.view)
    i32 = to_dev(dev, np.zeros(8, np.int32))

    def refused(rc, text):
        torch.cuda.synchronize()
        assert rc != 0 and text in last_error(lib) and g.untouched(), (rc, last_error(lib))

    def nothing(rc):
        torch.cuda.synchronize()
        assert rc == 0 and g.untouched(), (rc, last_error(lib))

    for m, k, n in ((-1, K, N), (M, -1, N), (M, K, -1)):
        refused(lib.aqg_graph_linear(m, k, n, _ptr(X), _ptr(W), _ptr(b), None, 0, y, st), "negative size")
        refused(lib.aqg_graph_linear_grad(m, k, n, _ptr(X), _ptr(X), None, _ptr(X), 1, y, None, st), "negative size")
    for flags in (8, 16, 8 | RELU, -1):
        refused(lib.aqg_graph_linear(M, K, N, _ptr(X), _ptr(W), _ptr(b), None, flags, y, st), "unknown flag")
    refused(lib.aqg_graph_aggregate(-1, N, _ptr(X), _ptr(i32), _ptr(i32), _ptr(X), None, 0, y, st), "negative size")
    refused(lib.aqg_graph_aggregate(M, -1, _ptr(X), _ptr(i32), _ptr(i32), _ptr(X), None, 0, y, st), "negative size")
    refused(lib.aqg_graph_mean_pool(M, N, _ptr(X), _ptr(i32), -1, y, st), "negative size")
    refused(lib.aqg_graph_mean_pool(-1, N, _ptr(X), _ptr(i32), 1, y, st), "negative size")
    refused(lib.aqg_graph_mean_pool_backward(M, -1, _ptr(X), _ptr(i32), 1, None, y, st), "negative size")
    refused(lib.aqg_graph_mean_pool_backward(M, N, _ptr(X), _ptr(i32), 0, None, y, st), "nodes without graphs")
    refused(lib.aqg_graph_heads(-1, N, _ptr(X), None, y, None, st), "bad size")
    refused(lib.aqg_graph_heads(M, 0, _ptr(X), None, y, None, st), "bad size")
    refused(lib.aqg_graph_heads_backward(-1, N, _ptr(X), _ptr(X), None, None, y, None, st), "bad size")
    # no rows / no columns: returns 0, launches nothing
    nothing(lib.aqg_graph_linear(0, K, N, _ptr(X), _ptr(W), _ptr(b), None, 0, y, st))
    nothing(lib.aqg_graph_linear(M, K, 0, _ptr(X), _ptr(W), _ptr(b), None, 0, y, st))
    nothing(lib.aqg_graph_linear_grad(M, K, 0, _ptr(X), _ptr(X), None, _ptr(X), 1, y, None, st))
    nothing(lib.aqg_graph_aggregate(0, N, _ptr(X), _ptr(i32), _ptr(i32), _ptr(X), None, 0, y, st))
    nothing(lib.aqg_graph_aggregate(M, 0, _ptr(X), _ptr(i32), _ptr(i32), _ptr(X), None, 0, y, st))
    nothing(lib.aqg_graph_mean_pool(0, N, None, _ptr(i32), 0, y, st))
    nothing(lib.aqg_graph_mean_pool(M, 0, _ptr(X), _ptr(i32), 1, y, st))
    nothing(lib.aqg_graph_mean_pool_backward(0, N, _ptr(X), _ptr(i32), 1, None, y, st))
    nothing(lib.aqg_graph_heads(0, N, _ptr(X), None, y, None, st))
    nothing(lib.aqg_graph_heads_backward(0, N, _ptr(X), _ptr(X), None, None, y, None, st))
