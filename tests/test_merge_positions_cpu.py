"""The position merge without a GPU: the hash's properties (replay.position_keys), replay.merge_reference against a plain float64
statement of "one row per distinct position with the mean targets", the bookkeeping of ReplayWindow.merged() on a host window, and
the ABI, the defaults and the command line."""
import os
import re
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from alphaquoridorgnn_amd import replay   # noqa: E402
from alphaquoridorgnn_amd.replay import KEY_BYTES, ReplayWindow, merge_depth, merge_reference, position_keys   # noqa: E402

OTHER_BYTES = (68, 69, 71)


def _A(N):
    return N * N + 2 * (N - 1) ** 2


def _bits(x):
    return x.view(np.int32) if x.dtype == np.float32 else x


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def mixed(rng, *shape):
    """f32 values of mixed magnitude and sign: a sum in another order has other bits."""
    return (rng.standard_normal(shape) * 10.0 ** rng.randint(-4, 3, shape)).astype(np.float32)


def repeated_rows(N, n, distinct, seed, lengths=None):
    """n rows over `distinct` random positions, scattered (or with the run lengths given, then shuffled); bytes 68, 69 and 71 differ
    from row to row; pi and z of mixed magnitude."""
    rng = np.random.RandomState(seed)
    base = rng.randint(0, 256, (distinct if lengths is None else len(lengths), 72)).astype(np.uint8)
    which = rng.randint(0, distinct, n) if lengths is None else rng.permutation(np.repeat(np.arange(len(lengths)), lengths))
    S = base[which].copy()
    for b in OTHER_BYTES:
        S[:, b] = rng.randint(0, 256, S.shape[0])
    return S, mixed(rng, S.shape[0], _A(N)), mixed(rng, S.shape[0])


def float64_statement(S, P, Z, index=None):
    """One row per distinct position (np.unique on the key bytes), in first-occurrence order, with the float64 mean of the targets and of
    their magnitudes: (records, mean pi, mean z, count, mean |pi|, mean |z|)."""
    rows = np.arange(S.shape[0]) if index is None else np.asarray(index)
    s, p, z = S[rows], P[rows].astype(np.float64), Z[rows].astype(np.float64)
    _, first, inverse, count = np.unique(s[:, KEY_BYTES], axis=0, return_index=True, return_inverse=True, return_counts=True)
    inverse = inverse.reshape(-1)
    order = np.argsort(first, kind="stable")
    groups = [np.flatnonzero(inverse == g) for g in order]
    return (s[first[order]], np.stack([p[g].mean(axis=0) for g in groups]), np.array([z[g].mean() for g in groups]),
            count[order], np.stack([np.abs(p[g]).mean(axis=0) for g in groups]), np.array([np.abs(z[g]).mean() for g in groups]))


def check_against_float64(got, S, P, Z, index=None):
    """u, the records, the order and the counts exact; each target within (d + 2) 2^-24 mean|x| of the float64 mean, d = merge_depth."""
    out72, out_pi, out_z, count = got
    want72, want_pi, want_z, want_count, mag_pi, mag_z = float64_statement(S, P, Z, index)
    assert out72.shape == want72.shape and np.array_equal(out72, want72)            # u, the records verbatim, first-occurrence order
    assert count.dtype == np.int32 and np.array_equal(count, want_count)
    assert int(count.sum()) == (S.shape[0] if index is None else len(index))
    bound = (np.array([merge_depth(c) for c in count]) + 2) * 2.0 ** -24
    assert np.all(np.abs(out_pi.astype(np.float64) - want_pi) <= bound[:, None] * mag_pi)
    assert np.all(np.abs(out_z.astype(np.float64) - want_z) <= bound * mag_z)


# ------------------------------------------------------------------ the hash
def test_key_ignores_the_ply_counter_and_the_spare_byte_and_nothing_else():
    rng = np.random.RandomState(1)
    rec = rng.randint(0, 256, (1, 72)).astype(np.uint8)
    key = position_keys(rec)
    assert key.dtype == np.int64 and key.shape == (1,)
    variants = [rec]
    for k in range(72):
        for b in range(256):
            if b == rec[0, k]:
                continue
            other = rec.copy()
            other[0, k] = b
            if k in OTHER_BYTES:
                assert position_keys(other)[0] == key[0]
            else:
                variants.append(other)
    keys = position_keys(np.concatenate(variants))
    assert len(variants) == 1 + 69 * 255 and keys[0] == key[0]
    assert len(set(keys.tolist())) == len(variants)          # every single-byte variant changes the key, and no two agree


def test_keys_of_an_index_are_the_keys_of_the_rows():
    rng = np.random.RandomState(2)
    S = rng.randint(0, 256, (50, 72)).astype(np.uint8)
    index = rng.permutation(50)[:31]
    assert np.array_equal(position_keys(S, index), position_keys(S)[index])
    assert position_keys(S[:0]).shape == (0,)


def test_merge_depth():
    assert [merge_depth(L) for L in (1, 2, 63, 64, 65, 128, 129, 20000)] == [0, 1, 62, 63, 64, 64, 65, 63 + 312]


# ------------------------------------------------------------------ merge_reference
def test_merge_reference_against_the_float64_statement():
    for N, n, distinct, lengths in ((3, 200, 30, None), (5, 300, 7, None), (9, 64, 64, None),
                                    (5, 0, 0, (1, 2, 3, 63, 64, 65, 127, 128, 129, 200, 1, 1))):
        S, P, Z = repeated_rows(N, n, distinct, seed=10 * N + distinct, lengths=lengths)
        check_against_float64(merge_reference(S, P, Z), S, P, Z)
    S, P, Z = repeated_rows(5, 120, 9, seed=77)
    index = np.random.RandomState(3).permutation(120)[:70]              # a gathered input, in an order of its own
    got = merge_reference(S, P, Z, index=index)
    check_against_float64(got, S, P, Z, index)
    assert all(same(a, b) for a, b in zip(got, merge_reference(S[index], P[index], Z[index])))


def test_a_hash_collision_splits_a_run_and_never_merges():
    """perm is all merge_reference takes from the keys: a perm that puts another position between two equal ones gives three rows."""
    S, P, Z = repeated_rows(3, 3, 2, seed=5, lengths=(1, 1))
    S = S[[0, 1, 0]]
    P, Z = np.concatenate([P, P[:1] * 3]), np.concatenate([Z, Z[:1] * 3])
    out72, _, _, count = merge_reference(S, P, Z, perm=np.arange(3))
    assert count.tolist() == [1, 1, 1] and np.array_equal(out72, S)
    out72, out_pi, _, count = merge_reference(S, P, Z)
    assert count.tolist() == [2, 1] and np.array_equal(out72, S[:2]) and same(out_pi[0], (P[0] + P[2]) / np.float32(2))


def test_all_rows_distinct_is_the_input_bit_for_bit():
    rng = np.random.RandomState(8)
    S = rng.randint(0, 256, (90, 72)).astype(np.uint8)
    P, Z = mixed(rng, 90, _A(7)), mixed(rng, 90)
    P[3, 5], Z[4] = np.float32(np.nan), np.float32(-0.0)
    out72, out_pi, out_z, count = merge_reference(S, P, Z)
    assert same(out72, S) and same(out_pi, P) and same(out_z, Z) and np.array_equal(count, np.ones(90, np.int32))


def test_the_summation_order_is_the_documented_one():
    """A run of 130 rows: chunks of 64, 64 and 2, each from its first row on, then the three chunk sums from the first on."""
    S, P, Z = repeated_rows(3, 130, 1, seed=9)
    f = np.float32
    chunks = []
    for c in (0, 64, 128):
        acc = Z[c]
        for k in range(c + 1, min(c + 64, 130)):
            acc = f(acc + Z[k])
        chunks.append(acc)
    want = f(f(f(chunks[0] + chunks[1]) + chunks[2]) / f(130))
    assert _bits(merge_reference(S, P, Z)[2])[0] == _bits(np.array([want]))[0]


# ------------------------------------------------------------------ the window
def test_merged_of_a_host_window_reads_no_stale_slot():
    """Three generations into a ring of 40 slots that keeps two: the third wraps and evicts the first.  The stale slots get the key bytes
    of a valid row and NaN targets: no NaN may come out, and merged() is merge_reference over rows()."""
    N = 5
    w = ReplayWindow(N, max_generations=2, capacity_rows=40)
    six = np.random.RandomState(4).randint(0, 256, (6, 72)).astype(np.uint8)
    for S, P, Z in [repeated_rows(N, m, 6, seed=40 + m) for m in (14, 16, 15)]:
        S[:, KEY_BYTES] = six[np.arange(S.shape[0]) % 6][:, KEY_BYTES]              # the same six positions in every generation
        w.append_rows(torch.from_numpy(S), torch.from_numpy(P), torch.from_numpy(Z))
    assert w.generations == [16, 15] and len(w) == 31
    index = w.index().numpy()
    assert index[0] == 14 and index[-1] == (14 + 31 - 1) % 40 and index.max() == 39 and index.min() == 0     # wrapped
    stale = np.setdiff1d(np.arange(40), index)
    assert len(stale) == 9
    r72, rpi, rz = (x.numpy() for x in w.tensors())
    r72[stale] = r72[index[0]]
    rpi[stale], rz[stale] = np.nan, np.nan
    before = [x.copy() for x in (r72, rpi, rz)]
    rows = [x.numpy().copy() for x in w.rows()]
    out = [x.numpy() for x in w.merged()]
    assert not np.isnan(out[1]).any() and not np.isnan(out[2]).any()
    assert all(same(a, b) for a, b in zip(out, merge_reference(*rows)))
    assert out[0].shape[0] == 6 and int(out[3].sum()) == 31
    check_against_float64(out, *rows)
    assert all(same(a, b) for a, b in zip(before, (x.numpy() for x in w.tensors())))            # the ring as it was
    assert all(same(a, b) for a, b in zip(rows, (x.numpy() for x in w.rows()))) and w.generations == [16, 15]
    empty = ReplayWindow(N, max_generations=2).merged()
    assert [tuple(x.shape) for x in empty] == [(0, 72), (0, _A(N)), (0,), (0,)] and empty[3].dtype == torch.int32


# ------------------------------------------------------------------ ABI and defaults
def test_abi_defaults_and_the_command_line():
    from alphaquoridorgnn_amd import _lib, train_cycle as tc, train_network as tn
    header = open(os.path.join(REPO, "include", "aqgnn.h")).read()
    assert re.search(r"#define\s+AQG_ABI_VERSION\s+15\b", header) and _lib.ABI_VERSION == 15
    for name in ("aqg_replay_position_keys", "aqg_replay_run_heads", "aqg_replay_merge_runs", "aqg_replay_merge_workspace_floats"):
        assert name in _lib.SIGNATURES and re.search(r"\b%s\(" % name, header)
    assert tn.TRAIN_MERGE_POSITIONS is False
    assert tc._parser().parse_args([]).merge_positions is False
    assert tc._set_replay_options(tc._parser().parse_args([])) is None and tn.TRAIN_MERGE_POSITIONS is False
    assert tc._parser().parse_args(["--merge-positions"]).merge_positions is True
    assert replay.MERGE_CHUNK == 64
