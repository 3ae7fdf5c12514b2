"""The CNN forward's conv kernel and its packing (csrc/cnn_forward.hip: cnn_conv_kernel in both its scalar and its vector form,
cnn_pack_conv_kernel, cnn_pack_bn_kernel), reached through the public surface alone -- a CNNNetwork in eval mode on arbitrary
[B,6,N,N] planes -- and compared with the float64 references of tests/test_cnn_conv_edges_cpu.py (its docstring has the method):
exact integer cases whose pool must match bit for bit over the whole shape cross, position probes, a BatchNorm fold under a
derived bound, real-valued networks at the project's forward bar, and the mask / batch independence at an edge shape."""
import copy
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests.test_cnn import BAR                                                                          # noqa: E402
from tests.test_cnn_conv_edges_cpu import (B_CROSS, BN_FOLD, CROSS, CROSS_REAL, KS, MASK_CASE, PROBE_N, TILE, bn_fold_case,   # noqa: E402
                                           exact_case, fnl_id, fold_bn, module_fp64, packed_conv, policy_size, probe_case,
                                           real_net, real_planes)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from alphaquoridorgnn_amd import _lib
    _lib.load()
    return _lib.require_gpu()


def hip_forward(net, dev, planes):
    """A copy of `net` on the device, through forward's HIP path -> dict of host arrays."""
    m = copy.deepcopy(net).to(dev).eval()
    with torch.no_grad():
        policy, value, logits, _, pooled = m._forward_planes(torch.from_numpy(np.array(planes)).to(dev), want_logits=True,
                                                                want_pooled=True)
    torch.cuda.synchronize()
    return dict(policy=policy.cpu().numpy(), value=value.cpu().numpy()[:, 0], logits=logits.cpu().numpy(),
                pooled=pooled.cpu().numpy())


def assert_bits(got, exp, what):
    assert got.dtype == np.float32 and got.shape == exp.shape, what
    bad = np.argwhere(got.view(np.uint32) != exp.view(np.uint32))
    assert bad.size == 0, f"{what}: {len(bad)} of {exp.size} pooled elements differ from the exact result, first at [board, channel] " \
                          f"{bad[0].tolist()}: {got[tuple(bad[0])]!r} vs {exp[tuple(bad[0])]!r}; channels {sorted(set(bad[:, 1].tolist()))[:12]}"


@pytest.mark.parametrize("case", CROSS, ids=fnl_id)
def test_exact_pool_bit_for_bit(dev, case):
    """Integer planes, sparse ternary weights, BatchNorm an integer shift: every f32 sum is exact in any order, so pooled must equal
    float32(sum / V) of the float64 network in every bit.  L = 0 is the stem (Cin = 6, the scalar path) and the pool; L >= 1 adds
    the Cin = F convs, the in-place residual and xa -> xt -> xa, where a tile's place feeds the next conv."""
    net, planes, exp, _ = exact_case(*case)
    got = hip_forward(net, dev, planes)
    assert_bits(got["pooled"], exp, fnl_id(case))
    assert np.isfinite(got["policy"]).all() and np.isfinite(got["value"]).all()


@pytest.mark.parametrize("tap", range(9))
@pytest.mark.parametrize("where", ["stem", "block"])
@pytest.mark.parametrize("N", PROBE_N)
def test_position_probes(dev, N, where, tap):
    """One nonzero weight at one tap, one probe element per board at each corner, each edge midpoint and the centre: the halo and
    the tap's orientation one at a time, in the stem and in the second K slab of the scalar path."""
    net, planes, exp, _ = probe_case(N, tap, where)
    assert_bits(hip_forward(net, dev, planes)["pooled"], exp, f"{where} tap {tap} at {N}x{N}")


def test_batchnorm_fold(dev):
    """cnn_pack_bn_kernel through real gamma, beta, mean, var and the default eps on exact integer conv sums (F = 65, N = 5, L = 0):
    pooled against the float64 mean of relu(fmaf(sum, scale, shift)) under (V + 1) 2^-24 sum |terms| / V (derived in bn_fold_case),
    and the packed scale / shift themselves against the header's statement (float64, rounded once)."""
    net, planes, ref, bound = bn_fold_case()
    got = hip_forward(net, dev, planes)["pooled"].astype(np.float64)
    err = np.abs(got - ref["pooled"])
    ratio = float((err[bound > 0] / bound[bound > 0]).max())
    print(f"BatchNorm fold {fnl_id(BN_FOLD)}: worst {ratio:.3g} of the bound")
    assert (err <= bound).all(), f"worst error is {ratio:.3g} x the derived bound"
    F_ = BN_FOLD[0]
    pk = copy.deepcopy(net).to(dev).packed_weights(dev).cpu().numpy()
    nt = (F_ + TILE - 1) // TILE
    off = nt * 1 * 9 * (KS // 4) * TILE * 4                      # the stem's one weight slab per tile, then scale [Fp], shift [Fp]
    sc, sh = fold_bn(net.conv.bn)
    scale, shift = pk[off:off + nt * TILE], pk[off + nt * TILE:off + 2 * nt * TILE]
    assert np.array_equal(scale[:F_], sc.astype(np.float32)) and (scale[F_:] == 0).all()
    assert (shift[F_:] == 0).all()
    # shift = beta - mean * sc in float64, rounded once; a contracted multiply-add may move the float64 value by an ulp of it,
    # which moves the f32 rounding only at a tie: allow one f32 ulp, and say how many elements needed it
    ulp = np.abs(shift[:F_].view(np.int32).astype(np.int64) - sh.astype(np.float32).view(np.int32).astype(np.int64))
    print(f"packed shift: {int((ulp != 0).sum())} of {F_} elements off the two-step float64 value")
    assert ulp.max() <= 1


@pytest.mark.parametrize("F_,L", [(33, 1), (66, 1), (5, 0)], ids=lambda v: str(v))
def test_packed_conv_weights(dev, F_, L):
    """cnn_pack_conv_kernel alone: the packed buffer's conv regions are the weights in [nt][ks][tap][k/4][n][k%4], zero past Cout /
    Cin, bit for bit (random normal weights: a misplaced element cannot hide)."""
    net = real_net(F_, L, 3, seed=F_).to(dev)
    pk = net.packed_weights(dev).cpu().numpy()
    nt, off = (F_ + TILE - 1) // TILE, 0
    for cb in net._convs():
        want = packed_conv(cb.conv.weight.detach().cpu().numpy(), F_).reshape(-1)
        got = pk[off:off + want.size]
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"conv at float {off}"
        off += want.size + 2 * nt * TILE


@pytest.mark.parametrize("case", CROSS_REAL, ids=fnl_id)
def test_real_weights_vs_fp64_module(dev, case):
    """Normal planes, default-initialised weights and non-trivial BatchNorm statistics against the same module in float64, at the
    forward bar of tests/test_cnn.py."""
    F_, N, L = case
    net, planes = real_net(F_, L, N, seed=1000 + CROSS_REAL.index(case)), real_planes(F_, N, L)
    want = module_fp64(net, planes)
    got = hip_forward(net, dev, planes)
    for k in ("pooled", "logits", "policy", "value"):
        np.testing.assert_allclose(got[k], want[k], err_msg=f"{fnl_id(case)} {k}", **BAR)


def test_mask_and_batch_independence_at_an_edge_shape(dev):
    """F = 33 (scalar path, two slabs, one 33-column tile), L = 1, N = 7 (49 tiles in 64 rows), B = 5 with active = {1, 0, 2, 1, 1}:
    skipped rows keep their poison, active rows equal the unmasked call and board 3 alone equals board 3 in the batch, bit for bit."""
    from alphaquoridorgnn_amd import _lib
    lib = _lib.load()
    F_, L, N, act = MASK_CASE["F"], MASK_CASE["L"], MASK_CASE["N"], MASK_CASE["active"]
    B, A = len(act), policy_size(N)
    net = real_net(F_, L, N, seed=77).to(dev)
    planes = torch.from_numpy(real_planes(F_, N, L, B=B)).to(dev)
    with torch.no_grad():
        full = net._forward_planes(planes, want_logits=True, want_pooled=True)
        one = net._forward_planes(planes[3:4].contiguous(), want_logits=True, want_pooled=True)
    for a, b in zip(one, full):
        assert torch.equal(a[0], b[3])
    POISON = -7.0
    active = torch.tensor(act, dtype=torch.uint8, device=dev)
    policy = torch.full((B, A), POISON, device=dev)
    value = torch.full((B,), POISON, device=dev)
    nws = int(lib.aqg_cnn_workspace_floats(N, F_, A, B))
    ws = torch.empty((nws,), device=dev)
    d = net.cnn_net(dev)
    _lib.check(lib.aqg_cnn_forward_planes(N, _lib.ptr(planes), B, ctypes.byref(d), _lib.ptr(active), _lib.ptr(ws), nws, None, None,
                                          _lib.ptr(policy), None, _lib.ptr(value), _lib.stream_ptr(dev)), "aqg_cnn_forward_planes")
    torch.cuda.synchronize()
    on = active == 1
    assert on.tolist() == [True, False, False, True, True]
    assert torch.equal(policy[on], full[0][on]) and torch.equal(value[on], full[1][:, 0][on])
    assert bool((policy[~on] == POISON).all()) and bool((value[~on] == POISON).all())
    assert B_CROSS < B
