"""The low side of fp16 range, without a GPU: what the fp16 hi/lo split of the default 9x9 kernels does to a network whose layers
are rescaled (tests/_low_side.py), stated in numpy; and the criterion the packing applies against it, through the host function.

Every figure asserted here is derived by this file from the arithmetic of the split, under a stated assumption about fp16
subnormals; none is a hardware number.  tests/test_split_low_side.py holds the kernels themselves to the project's bars."""
import ctypes
import math

import numpy as np
import pytest

from tests import _low_side as L
from tests import _util as U
from oracle import gnn as og

TABLE_KS = (0, 6, 8, 10, 12, 14, 16)
# Worst logit error of the kept-subnormal split as a multiple of the forward bar (atol 1e-5, rtol 1e-4) and of the calibration's
# former bar (1e-4, 1e-3), as listed in the issue that asked for these tests (seed-3 weights with non-zero biases, 12 walk_9x9
# states); per site, one figure per k of TABLE_KS.  Every cell is asserted within a factor 2 of its figure, with two exceptions.
#   k = 0, forward bar: the issue lists 0.01.  THIS file derives 0.029 for both sites (0.028 .. 0.033 over three choices of the 12
#     states, with and without the split of U before the aggregation, either order of layer 1), which a factor 2 around 0.01 does
#     not admit.  The discrepancy is not explained -- the issue's own emulation is not available -- and the hardware sides with this
#     file (0.0294 on 48 states, profiles/split_low_side.log).  The cell is asserted around the derived 0.029.
#   k = 0, calibration bar: listed as 0.00, around which a factor 2 is empty; asserted to be at most 0.005.
DERIVED_K0_FORWARD = 0.029
TABLE = {
    ("gcn1/gcn2", "forward"): (DERIVED_K0_FORWARD, 0.23, 1.15, 6.3, 19, 123, 452),
    ("gcn0/gcn1", "forward"): (DERIVED_K0_FORWARD, 0.31, 1.13, 4.0, 17, 73, 214),
    ("gcn1/gcn2", "calibration"): (None, 0.02, 0.12, 0.63, 1.9, 12, 45),
    ("gcn0/gcn1", "calibration"): (None, 0.03, 0.11, 0.40, 1.7, 7.3, 21),
}
K0_CALIBRATION_AT_MOST = 0.005
BARS = {"forward": (1e-5, 1e-4), "calibration": (1e-4, 1e-3)}
FLUSHED_AT_S1 = 12.0          # the same split with subnormals flushed, k = 0, forward bar


@pytest.fixture(scope="module")
def world():
    states = U.golden("walk_9x9.npz")["states"]
    recs = states[np.linspace(0, states.shape[0] - 1, 12).astype(int)]
    base = L.base_params(3)
    return recs, base, og.forward_states_dense(base, recs)


def test_rescalings_preserve_the_function(world):
    """Every site, every k: exact multiples, and the fp64 oracle of the rescaled set equals the base set's to 1e-9 relative."""
    recs, base, _ = world
    for site in L.SITES:
        for k in L.KS:
            p, gfac = L.rescale(base, site, k)
            L.assert_same_function(base, p, recs)
            down, up = L.SITES[site]
            assert all(gfac[key] == 2.0 ** k for key in down) and all(gfac[key] == 2.0 ** -k for key in up)
            assert sum(1 for f in gfac.values() if f != 1.0) == (0 if k == 0 else len(down) + len(up))


def test_split_pair_error_floor():
    """The pair hi + lo carries x to ~2^-22 |x| while lo is normal (|x| >= 2^-3), to a fixed 2^-25 below that (lo's subnormal
    spacing is 2^-24), to nothing below 2^-25; with subnormals flushed the floor is hi's own rounding from 2^-3 down."""
    rng = np.random.RandomState(0)
    for e in range(2, -27, -1):
        x = rng.uniform(1.0, 2.0, 4096) * 2.0 ** e
        hi, lo = L.split(x, False)
        err = np.abs(hi + lo - x).max()
        if e >= -3:
            assert err <= 2.0 ** -22 * 2.0 ** (e + 1)
        else:
            assert err <= 2.0 ** -25
        if e == -10:
            assert err >= 2.0 ** -27                    # the floor is really there: 2^-15 relative at this scale
        hf, lf = L.split(x, True)
        if -14 <= e < -3 - 11:
            assert not lf.any()                          # |lo| <= 2^-11 |x| < 2^-14: flushed, the pair is hi alone
    z, zl = L.split(np.array([2.0 ** -26, -2.0 ** -26]), False)
    assert not z.any() and not zl.any()


def test_table_of_the_kept_subnormal_split(world):
    """The split with fp16 subnormals KEPT, on the two trunk sites: the worst logit error against the fp64 oracle of the base set, as a
    multiple of the forward bar and of the bar the calibration used to apply, within a factor 2 of the listed figures (TABLE, with
    its two stated exceptions at k = 0).  Prints every cell."""
    recs, base, ref = world
    for site in ("gcn1/gcn2", "gcn0/gcn1"):
        outs = [L.forward_split(L.rescale(base, site, k)[0], recs)["logits"] for k in TABLE_KS]
        for which, (atol, rtol) in BARS.items():
            got = [L.bar_ratio(o, ref["logits"], atol, rtol) for o in outs]
            print(f"kept, {site}, x {which} bar: " + "  ".join(f"k={k}: {r:.3g}" for k, r in zip(TABLE_KS, got)))
            for k, r, listed in zip(TABLE_KS, got, TABLE[(site, which)]):
                if listed is None:
                    assert r <= K0_CALIBRATION_AT_MOST, (site, which, k, r)
                else:
                    assert listed / 2.0 <= r <= listed * 2.0, (site, which, k, r, listed)


def test_flushed_split_misses_the_bar_at_ordinary_scale(world):
    """The same arithmetic with subnormals FLUSHED misses the forward bar already at k = 0, about 12-fold (factor-2 band): kernels
    that pass the existing forward tests at initialisation scale keep their subnormals -- if test_split_low_side.py's k = 0 and
    k = 4 cells sit near the kept column, that is settled."""
    recs, base, ref = world
    r = L.bar_ratio(L.forward_split(base, recs, flush=True)["logits"], ref["logits"], 1e-5, 1e-4)
    print(f"flushed, k=0, x forward bar: {r:.3g}")
    assert FLUSHED_AT_S1 / 2.0 <= r <= FLUSHED_AT_S1 * 2.0


# ------------------------------------------------------------------ the criterion at pack time
MIN_PLANE_SCALE = 2.0 ** -8     # csrc/split_mfma.hpp SPLIT_MIN_PLANE_SCALE
SPLIT_MATRICES = ("gcn_layers.0.lin.weight", "gcn_layers.1.lin.weight", "gcn_layers.2.lin.weight", "policy_head.0.weight",
                  "value_head.0.weight", "policy_head.2.weight")        # what the split kernels carry as hi / lo planes


def _guard(params):
    from alphaquoridorgnn_amd import _lib
    lib = _lib.load()
    host = [np.ascontiguousarray(params[k], dtype=np.float32) for k in og.KEYS]
    arr = (ctypes.c_void_p * 14)(*[h.ctypes.data_as(ctypes.c_void_p) for h in host])
    n = lib.aqg_gcn_packed_floats(9)
    out = np.zeros(n, dtype=np.float32)
    assert lib.aqg_gcn_pack_weights_host(9, arr, out.ctypes.data_as(ctypes.c_void_p)) == 0
    return out[n - 4:]


def _refused(params):
    """The documented criterion (include/aqgnn.h, GUARD): a split matrix that is not all zero and has no entry of 2^-8 or more."""
    return any(0.0 < float(np.abs(params[k]).max()) < MIN_PLANE_SCALE for k in SPLIT_MATRICES)


def test_pack_refuses_matrices_below_the_splits_scale(world):
    """aqg_gcn_pack_weights_host on every rescaled set: the GUARD floats read as before where no split matrix is below the scale
    (k = 0 and k = 4 at every site: ordinary networks keep the fast kernels), and are (-1, -1, 0, 0) where one is -- every board of
    such a set raises the `saturated` word, the routes to the exact kernels that exist for the high side."""
    _, base, _ = world
    tb2 = L.CQ * math.sqrt(5.0) * float(np.abs(base["gcn_layers.1.bias"].astype(np.float64)).max())
    for site in L.SITES:
        for k in L.KS:
            p, _ = L.rescale(base, site, k)
            g = _guard(p)
            bites = _refused(p)
            assert bites == (k >= 8), (site, k)         # initialisation-scale matrices have maxima of 2^-3.5 .. 2^-2.3: k = 4 stays above 2^-8
            if bites:
                assert list(g) == [-1.0, -1.0, 0.0, 0.0], (site, k, g)
            else:
                t = tb2 * (2.0 ** -k if site == "gcn1/gcn2" else 1.0)       # layer 2's own bias rows are scaled with it there
                assert abs(g[0] - (65504.0 - t) / 2.07) <= 1e-2 and list(g[1:]) == [65504.0, 0.0, 0.0], (site, k, g)


def test_pack_criterion_edges(world):
    """Exactly at the scale is served, one ulp below is not; an all-zero matrix is exact in any split and is served; a matrix that is
    no split operand is not looked at; the high-side refusal reads the same (-1, -1)."""
    _, base, _ = world
    for key in SPLIT_MATRICES:
        p = {k: v.copy() for k, v in base.items()}
        p[key] = p[key] * np.float32(MIN_PLANE_SCALE / np.abs(p[key]).max() / 2.0)
        p[key].flat[0] = np.float32(MIN_PLANE_SCALE)
        assert list(_guard(p)[1:]) == [65504.0, 0.0, 0.0], key
        p[key].flat[0] = np.nextafter(np.float32(MIN_PLANE_SCALE), np.float32(0.0))
        assert list(_guard(p)) == [-1.0, -1.0, 0.0, 0.0], key
        p[key][:] = 0.0
        assert list(_guard(p)[1:]) == [65504.0, 0.0, 0.0], key
    p = {k: v.copy() for k, v in base.items()}
    p["value_head.2.weight"] = p["value_head.2.weight"] * np.float32(2.0 ** -20)    # not a split matrix: f32 in every kernel
    assert list(_guard(p)[1:]) == [65504.0, 0.0, 0.0]
    p = {k: v.copy() for k, v in base.items()}
    p["gcn_layers.1.lin.weight"][3, 7] = 7e4
    assert list(_guard(p)) == [-1.0, -1.0, 0.0, 0.0]


def test_criterion_leaves_the_split_a_margin(world):
    """Why 2^-8.  By the kept-subnormal arithmetic above, the smallest power-of-two rescaling of each site that still passes the
    criterion (the scaled matrix's largest entry in [2^-8, 2^-7)) leaves the split within a THIRD of the forward bar on logits and
    pre-tanh value -- the rest is for what this statement leaves out, the kernels' f32 accumulation -- while the first k the
    arithmetic puts past the bar is 8 (the table above): what is refused between the two is a weight matrix whose largest entry is
    below 0.004, and k = 4 is served at every site."""
    recs, base, ref = world
    for site, (down, _) in L.SITES.items():
        m = float(np.abs(base[down[0]]).max())
        k_last = int(math.floor(math.log2(m / MIN_PLANE_SCALE)))
        assert 4 <= k_last < 8
        p, _ = L.rescale(base, site, k_last)
        assert not _refused(p) and _refused(L.rescale(base, site, k_last + 1)[0])
        out = L.forward_split(p, recs)
        r = max(L.bar_ratio(out["logits"], ref["logits"], 1e-5, 1e-4), L.bar_ratio(out["value_pre"], ref["value_pre"], 1e-5, 1e-4))
        print(f"{site}: last k served by the split = {k_last}, {r:.3g} of the forward bar")
        assert r <= 1.0 / 3.0, (site, k_last, r)
