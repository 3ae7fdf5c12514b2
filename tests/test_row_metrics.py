"""Row metrics on the GPU (csrc/row_metrics.hip): the rows kernel against replay.row_metrics_reference -- se, tag and the rejections bit
for bit, ce, ent and lp within the derived bars of tests/_row_metrics.py (the device's 3-ulp log / exp in place of glibc's 1) -- on all
four boards, at m = 1 .. 65, with and without an index, across chunk seams, inside NaN- and sentinel-filled buffers; the reduction
bit for bit on general float64 data; the hold-out mask bit for bit; every refusal of the three entries with its outputs untouched."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests._row_metrics import (BOARDS, OFFSETS, SPECIAL, ULP_DEVICE, ULP_HOST, case, policy_size, records, special_rows,  # noqa: E402
                                within_bars)

pytestmark = pytest.mark.gpu

FILL_I32, MARGIN = np.int32(-77), 3


@pytest.fixture(scope="module")
def dev():
    from alphaquoridorgnn_amd import _lib
    _lib.load()
    return _lib.require_gpu()


def _t(dev, x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _at(t, items):
    return ctypes.c_void_p(t.data_ptr() + items * t.element_size())


# ------------------------------------------------------------------ the rows kernel
def _rows_launch(dev, N, s72, pi, z, net, v, index=None, chunks=None, bucket_plies=8, buckets=16):
    """aqg_replay_row_metrics over device copies, one launch per (offset, n) of `chunks` (default: one launch of all m rows), each fed
    its own slice of net and v; vals sits in a NaN-filled buffer and tag in a sentinel-filled one, MARGIN rows in front and behind,
    checked here.  Returns (vals [m,4], tag [m]) as numpy arrays -- rows no launch named still hold the fill."""
    from alphaquoridorgnn_amd import _lib
    lib = _lib.load()
    A, m = policy_size(N), net.shape[0]
    d72, d_pi, d_z, d_index = _t(dev, s72), _t(dev, pi), _t(dev, z), _t(dev, index)
    vals = torch.full((m + 2 * MARGIN, 4), float("nan"), dtype=torch.float64, device=dev)
    tag = torch.full((m + 2 * MARGIN,), int(FILL_I32), dtype=torch.int32, device=dev)
    for off, n in chunks or ((0, m),):
        d_net, d_v = _t(dev, net[off:off + n]), _t(dev, v[off:off + n])
        rc = lib.aqg_replay_row_metrics(N, A, _lib.ptr(d_net), _lib.ptr(d_v), _lib.ptr(d72), _lib.ptr(d_pi), _lib.ptr(d_z), _lib.ptr(d_index),
                                        pi.shape[0], m, off, n, bucket_plies, buckets, _at(vals, 4 * MARGIN), _at(tag, MARGIN),
                                        _lib.stream_ptr(dev))
        assert rc == 0, lib.aqg_last_error()
        torch.cuda.synchronize()
        assert d_net.cpu().numpy().tobytes() == np.ascontiguousarray(net[off:off + n]).tobytes()
    assert d_pi.cpu().numpy().tobytes() == pi.tobytes() and d72.cpu().numpy().tobytes() == s72.tobytes()
    hv, ht = vals.cpu().numpy(), tag.cpu().numpy()
    assert np.isnan(hv[:MARGIN]).all() and np.isnan(hv[m + MARGIN:]).all()
    assert np.all(ht[:MARGIN] == FILL_I32) and np.all(ht[m + MARGIN:] == FILL_I32)
    return hv[MARGIN:m + MARGIN], ht[MARGIN:m + MARGIN]


def _gathered(pi, m, index):
    rows = np.arange(m) if index is None else np.asarray(index)
    inside = (rows >= 0) & (rows < pi.shape[0])
    t = np.zeros((m, pi.shape[1]), np.float32)
    t[inside] = pi[rows[inside]]
    return t


def _check_rows(dev, N, s72, pi, z, net, v, index=None, chunks=None, **options):
    from alphaquoridorgnn_amd.replay import row_metrics_reference
    vals, tag = _rows_launch(dev, N, s72, pi, z, net, v, index, chunks, **options)
    vals_ref, tag_ref = row_metrics_reference(s72, pi, z, net, v, index, **options)
    named = np.zeros((net.shape[0],), bool)
    for off, n in chunks or ((0, net.shape[0]),):
        named[off:off + n] = True
    assert np.isnan(vals[~named]).all() and np.all(tag[~named] == FILL_I32)                 # every unnamed element untouched
    assert np.array_equal(tag[named], tag_ref[named])                                       # tag and the rejections: bit for bit
    ok = within_bars(vals[named], vals_ref[named], _gathered(pi, net.shape[0], index)[named], net[named], ULP_DEVICE, ULP_HOST)
    diff = np.abs(vals[named][:, :3] - vals_ref[named][:, :3]).max() if named.any() else 0.0
    print(f"rows kernel {N}x{N} m={net.shape[0]}: max |ce, ent, lp - reference| = {diff:.3e}")
    assert np.all(ok), (np.flatnonzero(~ok), vals[named][~ok], vals_ref[named][~ok])
    rejected = (tag_ref & 255) == options.get("buckets", 16)
    assert vals[named & rejected].tobytes() == np.zeros((int((named & rejected).sum()), 4)).tobytes()
    return vals, tag


@pytest.mark.parametrize("N", BOARDS)
def test_rows_kernel_against_the_statement(dev, N):
    """m = 1 .. 65 (every count of rows in a wavefront's group, a workgroup, and one past four workgroups): all rows in order, and an
    index in an order of its own that skips ring rows filled with NaN."""
    for m in range(1, 66):
        rng = np.random.RandomState(100 * N + m)
        s72, pi, z, net, v = case(rng, N, m + 9, m)
        _check_rows(dev, N, s72, pi, z, net, v)
        if m % 4 == 1 or m >= 60:
            index = rng.permutation(m + 9)[:m].astype(np.int64)
            pi[np.setdiff1d(np.arange(m + 9), index)] = np.nan
            z[np.setdiff1d(np.arange(m + 9), index)] = np.nan
            vals, tag = _check_rows(dev, N, s72, pi, z, net, v, index)
            assert np.all((tag & 255) < 16)


@pytest.mark.parametrize("N", BOARDS)
def test_rows_kernel_across_chunk_seams(dev, N):
    """50 rows cut at the offsets 0, 1, 15, 16, 17 (and 33): each launch with its own network buffers; the bits of the single launch.
    A launch of one chunk alone writes its own rows and no other."""
    rng = np.random.RandomState(200 + N)
    s72, pi, z, net, v = case(rng, N, 70, 50)
    index = rng.permutation(70)[:50].astype(np.int64)
    cuts = list(OFFSETS) + [33, 50]
    seams = tuple((a, b - a) for a, b in zip(cuts[:-1], cuts[1:]) if b > a)
    for idx in (None, index):
        whole = _check_rows(dev, N, s72, pi, z, net, v, idx)
        parts = _check_rows(dev, N, s72, pi, z, net, v, idx, chunks=seams)
        assert whole[0].tobytes() == parts[0].tobytes() and np.array_equal(whole[1], parts[1])
        for off in OFFSETS:
            alone = _check_rows(dev, N, s72, pi, z, net, v, idx, chunks=((off, 17),))
            assert alone[0][off:off + 17].tobytes() == whole[0][off:off + 17].tobytes()


@pytest.mark.parametrize("N", BOARDS)
def test_rows_kernel_special_rows(dev, N):
    """Every special row is rejected bit for bit, alone in its group and beside ordinary rows; an index of -1, of `rows` and of 2^40
    are three more; p = 0 under a positive target is the statement's value within the bar; plies on both sides of every bucket edge
    and a ply of 65,535 land in the statement's buckets, at three bucket shapes."""
    A, rng = policy_size(N), np.random.RandomState(300 + N)
    s72, pi, z, net, v = special_rows(rng, N)
    n = len(SPECIAL)
    vals, tag = _check_rows(dev, N, s72, pi, z, net, v)
    assert tag.tolist() == [16] * n, dict(zip(SPECIAL, tag))
    more = case(rng, N, 6, 6)
    order = rng.permutation(n + 6)
    mixed = [np.concatenate([a, b])[order] for a, b in zip((s72, pi, z, net, v), more)]
    vals, tag = _check_rows(dev, N, *mixed)
    assert np.all(tag[order < n] == 16) and np.all((tag[order >= n] & 255) < 16) and np.all(vals[order >= n, 0] > 0)
    vals, tag = _check_rows(dev, N, *more[:3], more[3], more[4], index=np.array([0, 6, 2, -1, 4, 2 ** 40], np.int64))
    assert tag[[1, 3, 5]].tolist() == [16] * 3 and np.all((tag[[0, 2, 4]] & 255) < 16)
    hot = np.zeros_like(more[1])
    hot[:, A - 1] = 1.0
    zero = more[3].copy()
    zero[:, A - 1] = 0.0
    vals, tag = _check_rows(dev, N, more[0], hot, more[2], zero, more[4])
    assert np.all((tag & 255) < 16) and np.all(np.abs(vals[:, 0] - 126 * np.log(2.0)) < 1e-12) and not vals[:, 1].any()
    for bucket_plies, buckets in ((8, 16), (1, 64), (300, 3), (8, 1)):
        edges = [b * bucket_plies + d for b in range(min(buckets + 1, 18)) for d in (-1, 0)]
        plies = np.array([x for x in edges if 0 <= x <= 65535] + [65535, 0, 255, 256])
        m = len(plies)
        c = case(rng, N, m, m)
        vals, tag = _check_rows(dev, N, records(rng, m, plies=plies), *c[1:], bucket_plies=bucket_plies, buckets=buckets)
        assert np.array_equal(tag & 255, np.minimum(plies // bucket_plies, buckets - 1))


# ------------------------------------------------------------------ the reduction
def _reduce_launch(dev, vals, tag, buckets):
    from alphaquoridorgnn_amd import _lib
    lib = _lib.load()
    m = vals.shape[0]
    d_vals, d_tag = _t(dev, vals), _t(dev, tag)
    words = int(lib.aqg_row_metrics_workspace_doubles(m, buckets))
    partial = torch.full((words + 2,), float("nan"), dtype=torch.float64, device=dev)
    sums = torch.full((buckets + 1 + 2, 4), float("nan"), dtype=torch.float64, device=dev)
    counts = torch.full((buckets + 1 + 2, 4), -77, dtype=torch.int64, device=dev)
    rc = lib.aqg_row_metrics_reduce(_lib.ptr(d_vals) if m else None, _lib.ptr(d_tag) if m else None, m, buckets, _at(partial, 1) if m else None,
                                    _at(sums, 4), _at(counts, 4), _lib.stream_ptr(dev))
    assert rc == 0, lib.aqg_last_error()
    torch.cuda.synchronize()
    hs, hc, hp = sums.cpu().numpy(), counts.cpu().numpy(), partial.cpu().numpy()
    assert np.isnan(hs[0]).all() and np.isnan(hs[-1]).all() and np.all(hc[0] == -77) and np.all(hc[-1] == -77)
    assert np.isnan(hp[0]) and np.isnan(hp[-1])
    if m:
        assert d_vals.cpu().numpy().tobytes() == vals.tobytes() and np.array_equal(d_tag.cpu().numpy(), tag)
    return hs[1:-1], hc[1:-1]


@pytest.mark.parametrize("m", (0, 1, 255, 256, 257, 4095, 4096, 4097, 8193))
def test_reduce_equals_the_statement_bit_for_bit(dev, m):
    """General float64 data at every size around a lane round, a chunk and two chunks, at buckets = 1, 2, 16, 64; empty buckets, and
    every row in one bucket; a bucket field above `buckets` belongs to no bucket."""
    from alphaquoridorgnn_amd.replay import row_metrics_reduce_reference
    rng = np.random.RandomState(m)
    for buckets in (1, 2, 16, 64):
        general = rng.standard_normal((m, 4)) * np.exp(rng.standard_normal((m, 1)) * 3)
        tags = [(rng.randint(0, buckets + 1, m) | rng.randint(0, 8, m) << 8).astype(np.int32),
                np.full((m,), (buckets - 1) | 5 << 8, np.int32)]                            # every row in one bucket
        if buckets == 16:
            tags.append((rng.choice([3, 9, 200], m) | rng.randint(0, 8, m) << 8).astype(np.int32))      # empty buckets, and no bucket
        for tag in tags:
            sums, counts = _reduce_launch(dev, general, tag, buckets)
            want, want_counts = row_metrics_reduce_reference(general, tag, buckets)
            assert sums.tobytes() == want.tobytes() and np.array_equal(counts, want_counts), (m, buckets)


# ------------------------------------------------------------------ the mask
def _mask_launch(dev, keys, seed, share):
    from alphaquoridorgnn_amd import _lib
    lib = _lib.load()
    n = keys.shape[0]
    d_keys = _t(dev, keys)
    mask = torch.full((n + 2 * MARGIN,), 99, dtype=torch.uint8, device=dev)
    rc = lib.aqg_replay_holdout_mask(_lib.ptr(d_keys), n, seed, share, _at(mask, MARGIN), _lib.stream_ptr(dev))
    assert rc == 0, lib.aqg_last_error()
    torch.cuda.synchronize()
    h = mask.cpu().numpy()
    assert np.all(h[:MARGIN] == 99) and np.all(h[n + MARGIN:] == 99) and np.array_equal(d_keys.cpu().numpy(), keys)
    return h[MARGIN:n + MARGIN]


def test_mask_equals_the_statement_bit_for_bit(dev):
    """n = 1 .. 257 at the shares 2^-53, 0.5 and 1 - 2^-53, under a small and a 64-bit seed; keys of both signs."""
    from alphaquoridorgnn_amd.replay import holdout_reference
    rng = np.random.RandomState(1)
    big = (1 << 64) - 3
    for n in range(1, 258):
        keys = rng.randint(-2 ** 63, 2 ** 63, n, dtype=np.int64)
        for share in (2.0 ** -53, 0.5, 1 - 2.0 ** -53):
            seed = (7, big)[n % 2]
            assert np.array_equal(_mask_launch(dev, keys, seed, share), holdout_reference(keys, seed, share)), (n, share)
    keys = rng.randint(-2 ** 63, 2 ** 63, 4096, dtype=np.int64)
    got = _mask_launch(dev, keys, 0, 0.25)
    assert np.array_equal(got, holdout_reference(keys, 0, 0.25)) and abs(int(got.sum()) - 1024) <= 5 * np.sqrt(4096 * 0.25 * 0.75)


def test_holdout_split_on_the_device(dev):
    """holdout_split and ReplayWindow.holdout_split on the GPU: the numpy statement's two sides, in input order."""
    from alphaquoridorgnn_amd.replay import ReplayWindow, holdout_split, holdout_split_reference
    rng = np.random.RandomState(2)
    s72 = records(rng, 40)[rng.randint(0, 40, 300)]
    s72[:, 68] = rng.randint(0, 256, 300)
    index = rng.permutation(300)[:211].astype(np.int64)
    for idx in (None, index):
        train, held = holdout_split(_t(dev, s72), _t(dev, idx), 0.3, 11, 5)
        want = holdout_split_reference(s72, idx, 0.3, 11)
        assert train.dtype == torch.int64 and train.device == dev and held.device == dev
        assert np.array_equal(train.cpu().numpy(), want[0]) and np.array_equal(held.cpu().numpy(), want[1]) and 0 < len(want[1]) < 211
    with pytest.raises(ValueError, match="share"):
        holdout_split(_t(dev, s72), None, 1.0, 0, 5)
    with pytest.raises(ValueError, match="index"):
        holdout_split(_t(dev, s72), _t(dev, np.array([0, 300], np.int64)), 0.5, 0, 5)
    empty = holdout_split(_t(dev, s72[:0]), None, 0.5, 0, 5)
    assert empty[0].numel() == 0 and empty[1].numel() == 0
    w = ReplayWindow(5, max_generations=2, capacity_rows=200, device=dev)
    pi, z = torch.rand((150, 57)), torch.zeros((150,))
    w.append_rows(torch.from_numpy(s72[:150]), pi, z)
    w.append_rows(torch.from_numpy(s72[150:]), pi, z)               # the ring wraps: the valid slots start past 0
    train, held = w.holdout_split(0.4, seed=5)
    want = holdout_split_reference(w.tensors()[0].cpu().numpy(), w.index().cpu().numpy(), 0.4, 5)
    assert np.array_equal(train.cpu().numpy(), want[0]) and np.array_equal(held.cpu().numpy(), want[1])


# ------------------------------------------------------------------ refusals
def test_the_c_entries_refuse_on_the_host(dev):
    """Every refusal of the three entries, made before any launch: -1 with a message, outputs and sources as they were."""
    from alphaquoridorgnn_amd import _lib
    lib = _lib.load()
    N, A, rows, m = 5, policy_size(5), 30, 20
    rng = np.random.RandomState(0)
    s72, pi, z, net, v = case(rng, N, rows, m)
    host = [net, v, s72, pi, z, rng.permutation(rows)[:m].astype(np.int64)]
    d_net, d_v, d72, d_pi, d_z, index = [_t(dev, x) for x in host]
    vals = torch.full((m, 4), float("nan"), dtype=torch.float64, device=dev)
    tag = torch.full((m,), int(FILL_I32), dtype=torch.int32, device=dev)
    st, p = _lib.stream_ptr(dev), _lib.ptr

    def refused(rc, word):
        assert rc == -1 and word in lib.aqg_last_error().decode(), (rc, lib.aqg_last_error())

    def rows_call(board=N, policy=A, net_=p(d_net), v_=p(d_v), s72_=p(d72), pi_=p(d_pi), z_=p(d_z), index_=p(index), ring=rows,
                  total_rows=m, offset=0, n=m, bucket_plies=8, buckets=16, vals_=p(vals), tag_=p(tag)):
        return lib.aqg_replay_row_metrics(board, policy, net_, v_, s72_, pi_, z_, index_, ring, total_rows, offset, n, bucket_plies, buckets,
                                          vals_, tag_, st)

    for board in (4, 11, 0):
        refused(rows_call(board=board), "board_size")
    refused(rows_call(policy=A + 1), "policy_size")
    refused(rows_call(total_rows=-1), "m out of range")
    refused(rows_call(total_rows=(1 << 24) + 1), "m out of range")
    refused(rows_call(index_=None, total_rows=rows + 1, n=1), "m out of range")
    refused(rows_call(ring=-1), "negative")
    for chunk in (dict(offset=-1), dict(n=-1), dict(offset=1), dict(offset=m, n=1)):
        refused(rows_call(**chunk), "chunk")
    for buckets in (0, -1, 65):
        refused(rows_call(buckets=buckets), "buckets")
    for bucket_plies in (0, -8):
        refused(rows_call(bucket_plies=bucket_plies), "bucket_plies")
    for name in ("net_", "v_", "s72_", "pi_", "z_", "vals_", "tag_"):
        refused(rows_call(**{name: None}), "must be given")
    refused(rows_call(vals_=_at(d_net, m * A - 1)), "overlaps a source")
    refused(rows_call(tag_=_at(d_v, m - 1)), "overlaps a source")
    refused(rows_call(tag_=_at(d_pi, A - 1)), "overlaps a source")              # inside the one certain row of a gathered ring
    refused(rows_call(tag_=_at(d72, 68)), "overlaps a source")
    refused(rows_call(tag_=_at(d_z, 0)), "overlaps a source")
    refused(rows_call(vals_=ctypes.c_void_p(index.data_ptr() + 8 * m - 4)), "overlaps a source")
    refused(rows_call(tag_=ctypes.c_void_p(vals.data_ptr() + 32 * m - 4)), "vals overlaps tag")
    assert rows_call(n=0, net_=None, v_=None, s72_=None, pi_=None, z_=None, index_=None, vals_=None, tag_=None) == 0
    assert rows_call(total_rows=0, n=0, net_=None, v_=None, s72_=None, pi_=None, z_=None, index_=None, vals_=None, tag_=None) == 0

    r_vals, r_tag = _t(dev, rng.standard_normal((m, 4))), _t(dev, rng.randint(0, 17, m).astype(np.int32))
    words = int(lib.aqg_row_metrics_workspace_doubles(m, 16))
    assert words == 17 * 8 and lib.aqg_row_metrics_workspace_doubles(0, 16) == 0 and lib.aqg_row_metrics_workspace_doubles(m, 0) == 0
    assert lib.aqg_row_metrics_workspace_doubles(m, 65) == 0 and lib.aqg_row_metrics_workspace_doubles((1 << 24) + 1, 16) == 0
    partial = torch.full((words,), float("nan"), dtype=torch.float64, device=dev)
    sums = torch.full((17, 4), float("nan"), dtype=torch.float64, device=dev)
    counts = torch.full((17, 4), -77, dtype=torch.int64, device=dev)

    def reduce_call(vals_=p(r_vals), tag_=p(r_tag), n=m, buckets=16, partial_=p(partial), sums_=p(sums), counts_=p(counts)):
        return lib.aqg_row_metrics_reduce(vals_, tag_, n, buckets, partial_, sums_, counts_, st)

    refused(reduce_call(n=-1), "m out of range")
    refused(reduce_call(n=(1 << 24) + 1), "m out of range")
    for buckets in (0, 65):
        refused(reduce_call(buckets=buckets), "buckets")
    for name in ("vals_", "tag_", "partial_", "sums_", "counts_"):
        refused(reduce_call(**{name: None}), "must be given")
    refused(reduce_call(sums_=_at(r_vals, 4 * m - 1)), "overlaps a source")
    refused(reduce_call(counts_=_at(r_tag, m - 1)), "overlaps a source")
    refused(reduce_call(partial_=_at(r_vals, 0)), "overlaps a source")
    refused(reduce_call(counts_=_at(sums, 67)), "outputs overlap")
    refused(reduce_call(partial_=_at(counts, 67)), "outputs overlap")

    keys = _t(dev, rng.randint(-2 ** 63, 2 ** 63, m, dtype=np.int64))
    mask = torch.full((m,), 99, dtype=torch.uint8, device=dev)

    def mask_call(keys_=p(keys), n=m, share=0.5, mask_=p(mask)):
        return lib.aqg_replay_holdout_mask(keys_, n, 3, share, mask_, st)

    refused(mask_call(n=-1), "negative")
    for share in (0.0, 1.0, -0.25, 1.5, float("nan"), float("inf")):
        refused(mask_call(share=share), "share")
    for name in ("keys_", "mask_"):
        refused(mask_call(**{name: None}), "must be given")
    refused(mask_call(mask_=ctypes.c_void_p(keys.data_ptr() + 8 * m - 1)), "overlaps")
    assert mask_call(n=0, keys_=None, mask_=None) == 0
    torch.cuda.synchronize()
    for x, hx in zip((d_net, d_v, d72, d_pi, d_z, index), host):
        assert x.cpu().numpy().tobytes() == hx.tobytes()
    assert bool(vals.isnan().all()) and bool((tag == int(FILL_I32)).all()) and bool(partial.isnan().all()) and bool(sums.isnan().all())
    assert bool((counts == -77).all()) and bool((mask == 99).all())
    assert rows_call() == 0 and reduce_call() == 0 and mask_call() == 0          # and the calls they were variations of are good ones
    torch.cuda.synchronize()
