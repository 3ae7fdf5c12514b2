"""Row metrics and the hold-out split without a GPU: the numpy statements (replay.row_metrics_reference, row_metrics_reduce_reference,
holdout_reference) against a plain float64 torch composition within the derived bars of tests/_row_metrics.py, their invariants,
the split's properties, the option checks, the command line's refusals, and the whole loop on a host window with a stub model."""
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests._row_metrics import (BOARDS, SPECIAL, ULP_HOST, U, StubModel, case, policy_size, records, reduce_depth, special_rows,  # noqa: E402
                                torch_composition, value_rows, within_bars)
from tests._surprise import network_rows, target_rows  # noqa: E402

HOLDOUT_SEED_CHECKED = 0        # the seed of test_split_share: 4,096 distinct keys at share 0.25 hold out 1,046 under it (checked on the CPU)


# ------------------------------------------------------------------ the rows statement
@pytest.mark.parametrize("N", BOARDS)
def test_statement_against_the_torch_composition(N):
    from alphaquoridorgnn_amd.replay import TAG_HIT, TAG_SIGN_AGREES, TAG_SIGN_COUNTED, row_metrics_reference
    rng = np.random.RandomState(10 + N)
    m, rows = 41, 50
    s72, pi, z, net, v = case(rng, N, rows, m)
    net = np.where(net < 2.0 ** -126, np.float32(0), net)           # (subnormal entries are clamped alike; keep p in [0, 1])
    index = rng.permutation(rows)[:m].astype(np.int64)
    recorded = pi
    for idx in (None, index):
        where = np.arange(m) if idx is None else idx
        pi = recorded.copy()
        pi[where[::3]] = 0.0
        pi[where[::3], net[::3].argmax(axis=1)] = 1.0               # every third row: a one-hot target on the network's choice
        vals, tag = row_metrics_reference(s72, pi, z, net, v, idx, bucket_plies=8, buckets=16)
        ce, ent, lp, se, hit, counted, agrees, lp_lse = torch_composition(pi[where], net, v, z[where])
        want = np.stack((ce, ent, lp, se), axis=1)
        ok = within_bars(vals, want, pi[where], net, ULP_HOST, ULP_HOST)
        assert np.all(ok), (np.flatnonzero(~ok), vals[~ok], want[~ok])
        assert np.all(within_bars(vals, np.stack((ce, ent, lp_lse, se), axis=1), pi[where], net, ULP_HOST, ULP_HOST))
        ply = s72[where, 68].astype(int) | s72[where, 69].astype(int) << 8
        assert np.array_equal(tag & 255, np.minimum(ply // 8, 15))
        assert np.array_equal((tag & TAG_HIT) != 0, hit) and np.array_equal((tag & TAG_SIGN_COUNTED) != 0, counted)
        assert np.array_equal((tag & TAG_SIGN_AGREES) != 0, agrees)
        assert vals.dtype == np.float64 and tag.dtype == np.int32 and 0 < hit.sum() < m and 0 < agrees.sum() < counted.sum() < m


@pytest.mark.parametrize("N", BOARDS)
def test_invariants(N):
    from alphaquoridorgnn_amd.replay import TAG_HIT, TAG_SIGN_AGREES, TAG_SIGN_COUNTED, row_metrics_reference
    A, rng = policy_size(N), np.random.RandomState(20 + N)
    m = 12
    s72 = records(rng, m, plies=np.arange(m))
    net = network_rows(rng, m, A)
    net = np.where(net < 2.0 ** -126, np.float32(2.0 ** -126), net)
    v, z = value_rows(rng, m)
    # p == t: KL = ce - ent = 0 within the bars (the same logarithms of the same arguments: it is exactly 0 here)
    vals, tag = row_metrics_reference(s72, net, z, net, v)
    assert np.all(vals[:, 0] - vals[:, 1] == 0.0) and np.all(vals[:, 0] > 0) and np.all((tag & TAG_HIT) != 0)
    # a one-hot target on p's maximum hits, one anywhere else does not; ent = +0.0 exactly
    best = net.argmax(axis=1)
    hot = np.zeros((m, A), np.float32)
    hot[np.arange(m), best] = 1.0
    vals, tag = row_metrics_reference(s72, hot, z, net, v)
    assert np.all((tag & TAG_HIT) != 0) and vals[:, 1].tobytes() == np.zeros(m).tobytes()
    miss = np.zeros((m, A), np.float32)
    miss[np.arange(m), (best + 1) % A] = 1.0
    assert not np.any(row_metrics_reference(s72, miss, z, net, v)[1] & TAG_HIT) or A == 1
    # tied targets: the row hits whichever of the tied entries p prefers, and whichever comes first in t
    tied = np.zeros((m, A), np.float32)
    other = (best + 3) % A
    tied[np.arange(m), best], tied[np.arange(m), other] = 0.5, 0.5
    assert np.all((row_metrics_reference(s72, tied, z, net, v)[1] & TAG_HIT) != 0)
    flat = np.full((m, A), np.float32(1.0 / A))                    # p flat: its first maximum is entry 0, which shares t's maximum
    assert np.all((row_metrics_reference(s72, tied[:, ::-1].copy(), z, flat, v)[1] & TAG_HIT) == ((tied[:, ::-1][:, 0] == 0.5) << 8))
    assert np.all((row_metrics_reference(s72, flat, z, flat, v)[1] & TAG_HIT) != 0)
    # z == 0 is not counted; the sign agrees iff v z > 0; v == 0 never agrees
    z3 = np.array([0.0, -0.0, 1.0, -1.0, 0.5, -0.25] * 2, np.float32)
    v3 = np.array([0.5, 0.5, 0.5, 0.5, -0.5, -0.5] * 2, np.float32)
    v3[8:] = 0.0
    tag = row_metrics_reference(s72, net, z3, net, v3)[1]
    assert ((tag & TAG_SIGN_COUNTED) != 0).tolist() == [False, False, True, True, True, True] * 2
    assert ((tag & TAG_SIGN_AGREES) != 0).tolist() == [False, False, True, False, False, True, False, False] + [False] * 4
    # se is the float64 square of the float64 difference
    vals = row_metrics_reference(s72, net, z3, net, v3)[0]
    assert vals[:, 3].tobytes() == ((v3.astype(np.float64) - z3.astype(np.float64)) ** 2).tobytes()


@pytest.mark.parametrize("N", (3, 9))
def test_every_rejection(N):
    from alphaquoridorgnn_amd.replay import row_metrics_reference
    rng = np.random.RandomState(30 + N)
    s72, pi, z, net, v = special_rows(rng, N)
    n = len(SPECIAL)
    for buckets in (1, 16, 64):
        vals, tag = row_metrics_reference(s72, pi, z, net, v, buckets=buckets)
        assert tag.tolist() == [buckets] * n and vals.tobytes() == np.zeros((n, 4)).tobytes(), dict(zip(SPECIAL, tag))
    good = case(rng, N, 6, 6)
    vals, tag = row_metrics_reference(*good[:3], good[3], good[4], index=np.array([0, 6, 2, -1, 4, 2 ** 40], np.int64))
    assert tag[[1, 3, 5]].tolist() == [16] * 3 and not vals[[1, 3, 5]].any() and np.all((tag[[0, 2, 4]] & 255) < 16) and np.all(vals[[0, 2, 4], 0] > 0)
    # p == 0 under a positive target is not a rejection: ln 2^-126
    hot = np.zeros_like(good[1])
    hot[:, 0] = 1.0
    net = good[3].copy()
    net[:, 0] = 0.0
    vals, tag = row_metrics_reference(good[0], hot, good[2], net, good[4])
    assert np.all((tag & 255) < 16) and np.allclose(vals[:, 0], 126 * np.log(2.0), rtol=0, atol=1e-12)


def test_buckets_and_their_edges():
    from alphaquoridorgnn_amd.replay import row_metrics_reference
    rng = np.random.RandomState(4)
    for bucket_plies, buckets in ((8, 16), (1, 64), (5, 3), (70000, 2), (8, 1)):
        edges = [b * bucket_plies + d for b in range(min(buckets + 1, 20)) for d in (-1, 0)]
        plies = np.array([x for x in edges if 0 <= x <= 65535] + [65535, 0])
        m = len(plies)
        s72, pi, z, net, v = case(rng, 5, m, m)
        s72 = records(rng, m, plies=plies)
        tag = row_metrics_reference(s72, pi, z, net, v, bucket_plies=bucket_plies, buckets=buckets)[1]
        assert np.array_equal(tag & 255, np.minimum(plies // bucket_plies, buckets - 1))


def test_the_statements_refuse():
    from alphaquoridorgnn_amd.replay import (check_holdout_options, check_row_metrics_options, holdout_reference, row_metrics_reduce_reference,
                                             row_metrics_reference)
    rng = np.random.RandomState(5)
    s72, pi, z, net, v = case(rng, 5, 8, 8)
    for bad in (dict(buckets=0), dict(buckets=65), dict(bucket_plies=0), dict(bucket_plies=1.5), dict(buckets=2.5)):
        with pytest.raises(ValueError):
            row_metrics_reference(s72, pi, z, net, v, **bad)
    for args in ((s72[:, :71], pi, z, net, v), (s72, pi.astype(np.float64), z, net, v), (s72, pi, z[:7], net, v), (s72, pi, z, net[:, :56], v),
                 (s72, pi, z, net, v[:7]), (s72[:7], pi[:7], z[:7], net, v)):
        with pytest.raises(ValueError):
            row_metrics_reference(*args)
    assert check_row_metrics_options(8, 16) == (8, 16)
    with pytest.raises(ValueError):
        row_metrics_reduce_reference(np.zeros((3, 4)), np.zeros(3, np.int64))
    with pytest.raises(ValueError):
        row_metrics_reduce_reference(np.zeros((3, 3)), np.zeros(3, np.int32))
    for share in (0.0, 1.0, -0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="share"):
            check_holdout_options(share)
        with pytest.raises(ValueError, match="share"):
            holdout_reference(np.zeros(3, np.int64), 0, share)
    for every in (0, -1, 1.5):
        with pytest.raises(ValueError, match="every"):
            check_holdout_options(0.5, 0, every)
    with pytest.raises(ValueError, match="seed"):
        check_holdout_options(0.5, 0.5)
    assert check_holdout_options(0.25, -1, 3) == (0.25, (1 << 64) - 1, 3)
    with pytest.raises(ValueError):
        holdout_reference(np.zeros(3, np.int32), 0, 0.5)


# ------------------------------------------------------------------ the reduce statement
def _add_at(vals, tag, buckets):
    sums = np.zeros((buckets + 1, 4))
    field = tag & 255
    keep = field <= buckets
    np.add.at(sums, field[keep], vals[keep])
    counts = np.zeros((buckets + 1, 4), np.int64)
    flags = np.stack((np.ones_like(tag), (tag >> 8) & 1, (tag >> 9) & 1, (tag >> 10) & 1), axis=1).astype(np.int64)
    np.add.at(counts, field[keep], flags[keep])
    return sums, counts


@pytest.mark.parametrize("m", (0, 1, 255, 257, 4096, 4097, 8193))
def test_reduce_statement_against_add_at(m):
    from alphaquoridorgnn_amd.replay import row_metrics_reduce_reference, row_metrics_workspace_doubles
    rng = np.random.RandomState(m)
    for buckets in (1, 2, 16, 64):
        tag = (rng.randint(0, buckets + 1, m) | rng.randint(0, 8, m) << 8).astype(np.int32)
        if buckets == 16:
            tag = (rng.choice([3, 9], m) | rng.randint(0, 8, m) << 8).astype(np.int32)       # empty buckets
        if buckets == 2:
            tag = np.full((m,), 1 | 5 << 8, np.int32)                                          # every row in one bucket
        dyadic = rng.randint(-2 ** 20, 2 ** 20, (m, 4)).astype(np.float64) / 2 ** 10
        sums, counts = row_metrics_reduce_reference(dyadic, tag, buckets)
        want, want_counts = _add_at(dyadic, tag, buckets)
        assert sums.tobytes() == want.tobytes() and np.array_equal(counts, want_counts)
        general = rng.standard_normal((m, 4)) * np.exp(rng.standard_normal((m, 1)) * 3)
        sums, counts = row_metrics_reduce_reference(general, tag, buckets)
        want, _ = _add_at(general, tag, buckets)
        mass = np.zeros((buckets + 1, 4))
        np.add.at(mass, tag & 255, np.abs(general))
        assert np.all(np.abs(sums - want) <= reduce_depth(m) * U * mass) and np.array_equal(counts, want_counts)
        assert row_metrics_workspace_doubles(m, buckets) == -(-m // 4096) * (buckets + 1) * 8
    assert row_metrics_workspace_doubles(5, 65) == 0 and row_metrics_workspace_doubles((1 << 24) + 1, 4) == 0


def test_reduce_ignores_a_bucket_field_above_buckets():
    from alphaquoridorgnn_amd.replay import row_metrics_reduce_reference
    vals = np.ones((5, 4))
    sums, counts = row_metrics_reduce_reference(vals, np.array([0, 1, 2, 3, 200], np.int32), 2)
    assert sums[:, 0].tolist() == [1.0, 1.0, 1.0] and counts[:, 0].tolist() == [1, 1, 1]


# ------------------------------------------------------------------ the split
def test_split_goes_by_key_bytes_alone():
    from alphaquoridorgnn_amd.replay import KEY_BYTES, holdout_reference, holdout_split_reference, position_keys
    rng = np.random.RandomState(6)
    base = records(rng, 300)
    again = base.copy()
    again[:, 68], again[:, 69], again[:, 71] = rng.randint(0, 256, 300), rng.randint(0, 256, 300), rng.randint(0, 256, 300)
    both = np.concatenate([base, again])
    assert np.array_equal(both[:300][:, KEY_BYTES], both[300:][:, KEY_BYTES])
    for seed in (0, 1, (1 << 64) - 1):
        mask = holdout_reference(position_keys(both), seed, 0.5)
        assert mask.dtype == np.uint8 and np.array_equal(mask[:300], mask[300:]) and 100 < mask[:300].sum() < 200
        train, held = holdout_split_reference(both, None, 0.5, seed)
        assert np.array_equal(np.sort(np.concatenate([train, held])), np.arange(600)) and np.all(np.diff(train) > 0) and np.all(np.diff(held) > 0)
        assert np.array_equal(held, np.flatnonzero(mask))
    assert not np.array_equal(holdout_reference(position_keys(both), 0, 0.5), holdout_reference(position_keys(both), 1, 0.5))
    # an index in an order of its own: both sides keep that order
    index = rng.permutation(600)[:200].astype(np.int64)
    train, held = holdout_split_reference(both, index, 0.3, 7)
    mask = holdout_reference(position_keys(both, index), 7, 0.3).astype(bool)
    assert np.array_equal(train, index[~mask]) and np.array_equal(held, index[mask])
    # a larger share holds out a superset
    small, large = (set(holdout_split_reference(both, None, s, 3)[1].tolist()) for s in (0.2, 0.6))
    assert small < large


def test_a_position_and_its_mirror_are_drawn_separately():
    """The mirror of a record (game_logic.mirror_record) is another position with another key: over the rows of the golden 5x5 set
    that are not their own mirror image, the mirrored copies' sides are not the originals'."""
    from alphaquoridorgnn_amd.game_logic import mirror_record
    from alphaquoridorgnn_amd.pv_network_gnn import pack_states
    from alphaquoridorgnn_amd.replay import KEY_BYTES, holdout_reference, position_keys
    g = np.load(os.path.join(REPO, "tests", "golden", "cnn_train_5x5.npz"))
    s = pack_states([[[int(r[0]), int(r[1])], [int(r[2]), int(r[3])], [int(x) for x in r[4:20]]] for r in g["states"]], 5)
    mirrored = mirror_record(s)
    differ = (mirrored[:, KEY_BYTES] != s[:, KEY_BYTES]).any(axis=1)
    assert differ.sum() >= 10
    a = holdout_reference(position_keys(s[differ]), 0, 0.5)
    b = holdout_reference(position_keys(mirrored[differ]), 0, 0.5)
    assert np.all(position_keys(s[differ]) != position_keys(mirrored[differ])) and not np.array_equal(a, b)


def test_split_of_the_merge_is_the_merge_of_the_split():
    from alphaquoridorgnn_amd.replay import holdout_split_reference, merge_reference
    rng = np.random.RandomState(8)
    base = records(rng, 40)
    rows = base[rng.randint(0, 40, 200)]
    rows[:, 68] = rng.randint(0, 256, 200)                          # repeated positions at other plies
    pi, z = target_rows(rng, 200, 57), value_rows(rng, 200)[1]
    m72, mpi, mz, _ = merge_reference(rows, pi, z)
    train_m, held_m = holdout_split_reference(m72, None, 0.4, 2)
    train, held = holdout_split_reference(rows, None, 0.4, 2)
    for side_m, side in ((train_m, train), (held_m, held)):
        s72, spi, sz, _ = merge_reference(rows, pi, z, index=side)
        assert s72.tobytes() == m72[side_m].tobytes() and spi.tobytes() == mpi[side_m].tobytes() and sz.tobytes() == mz[side_m].tobytes()
    assert 0 < len(held_m) < len(m72)


def test_split_share():
    """4,096 distinct keys at share 0.25 under HOLDOUT_SEED_CHECKED: the held-out count within five binomial standard deviations of
    1,024 (sd = sqrt(4096 * 0.25 * 0.75) = 27.7)."""
    from alphaquoridorgnn_amd.replay import holdout_reference, position_keys
    s = np.zeros((4096, 72), np.uint8)
    s[:, 0], s[:, 1] = np.arange(4096) & 255, np.arange(4096) >> 8
    keys = position_keys(s)
    assert len(set(keys.tolist())) == 4096
    held = int(holdout_reference(keys, HOLDOUT_SEED_CHECKED, 0.25).sum())
    print("held out", held)
    assert abs(held - 1024) <= 5 * np.sqrt(4096 * 0.25 * 0.75)
    # the extreme shares of the device test: 2^-53 holds out a draw of exactly 0 alone, 1 - 2^-53 everything else
    assert holdout_reference(keys, 0, 2.0 ** -53).sum() == 0 and holdout_reference(keys, 0, 1 - 2.0 ** -53).sum() == 4096


# ------------------------------------------------------------------ the surface
def test_defaults_names_and_the_binding():
    from alphaquoridorgnn_amd import _lib, replay, train_network as tn, validation
    assert tn.TRAIN_HOLDOUT_SHARE is None and tn.TRAIN_HOLDOUT_SEED == 0 and tn.TRAIN_HOLDOUT_EVERY == 1
    assert tn.TRAIN_HOLDOUT_KEEP_BEST is False and tn.TRAIN_HOLDOUT_LOG is None
    for name in ("row_metrics_reference", "row_metrics_reduce_reference", "holdout_reference", "check_holdout_options", "row_metrics",
                 "holdout_split", "HOLDOUT_STREAM"):
        assert hasattr(replay, name)
    with open(os.path.join(REPO, "include", "aqgnn.h")) as f:
        header = f.read()
    assert re.search(r"#define\s+AQG_ABI_VERSION\s+15\b", header) and _lib.ABI_VERSION == 15
    assert re.search(r"#define\s+AQG_HOLDOUT_STREAM\s+0x%Xull" % replay.HOLDOUT_STREAM, header)
    for name in ("aqg_replay_row_metrics", "aqg_row_metrics_reduce", "aqg_replay_holdout_mask", "aqg_row_metrics_workspace_doubles"):
        assert name in _lib.SIGNATURES and re.search(r"\b(int|size_t) " + name + r"\(", header)
    src = open(os.path.join(REPO, "alphaquoridorgnn_amd", "csrc", "row_metrics.hip")).read()
    for text in ("RM_GROUP = 4;", "RM_WAVES = 4;", "RM_MAX_ROWS = 1 << 24;", "RM_TINY = 0x1.0p-126f;", "RMR_CHUNK = 4096;", "RMR_LANES = 256;",
                 "#pragma clang fp contract(off)"):
        assert text in src
    assert "atomic" not in src.split("#include", 1)[1].lower()
    build = open(os.path.join(REPO, "alphaquoridorgnn_amd", "csrc", "build.sh")).read()
    assert "expected seven row-metrics kernels" in build and "aqg_row_metrics.remarks" in build
    import inspect
    sig = inspect.signature(validation.row_metrics)
    for name, default in (("index", None), ("bucket_plies", 8), ("buckets", 16), ("chunk_rows", 16384)):
        assert sig.parameters[name].default == default
    assert sig.parameters["bucket_plies"].kind is inspect.Parameter.KEYWORD_ONLY


def test_command_line_refusals():
    from alphaquoridorgnn_amd import train_cycle as tc, train_network as tn
    parse = tc._parser().parse_args
    assert tc._check_holdout_args(parse([])) is None
    assert tc._check_holdout_args(parse(["--holdout-share", "0.25"])) == (0.25, 0, 1)
    assert tc._check_holdout_args(parse(["--holdout-share", "0.1", "--holdout-seed", "9", "--holdout-every", "5", "--keep-best-epoch",
                                         "--holdout-log", "x.jsonl"])) == (0.1, 9, 5)
    for flags in (["--holdout-seed", "1"], ["--holdout-every", "2"], ["--keep-best-epoch"], ["--holdout-log", "x"]):
        with pytest.raises(ValueError, match="need --holdout-share"):
            tc._check_holdout_args(parse(flags))
        with pytest.raises(ValueError, match="holdout"):
            tc.main(["--cycles", "1"] + flags)                      # at parse time: no device, no process group
    for flags in (["--holdout-share", "0"], ["--holdout-share", "1"], ["--holdout-share", "-0.5"], ["--holdout-share", "nan"],
                  ["--holdout-share", "0.5", "--holdout-every", "0"], ["--holdout-share", "0.5", "--holdout-every", "-3"]):
        with pytest.raises(ValueError, match="holdout"):
            tc._check_holdout_args(parse(flags))
        with pytest.raises(ValueError, match="holdout"):
            tc.main(["--cycles", "1"] + flags)
    assert tn.TRAIN_HOLDOUT_SHARE is None                           # checking sets nothing


# ------------------------------------------------------------------ row_metrics and the loop on host rows
def _host_window(rng, N=5, rows=120, distinct=60):
    from alphaquoridorgnn_amd.replay import ReplayWindow
    base = records(rng, distinct, plies=rng.randint(0, 40, distinct))
    s = base[rng.randint(0, distinct, rows)]
    w = ReplayWindow(N, max_generations=2, capacity_rows=rows + 30)
    w.append_rows(torch.from_numpy(s[:70]), torch.from_numpy(target_rows(rng, 70, policy_size(N))), torch.from_numpy(value_rows(rng, 70)[1]))
    w.append_rows(torch.from_numpy(s[70:]), torch.from_numpy(target_rows(rng, rows - 70, policy_size(N))),
                  torch.from_numpy(value_rows(rng, rows - 70)[1]))
    return w


def test_row_metrics_on_host_rows():
    """Rows in host memory go through the numpy statements: the Metrics object's tables, totals and table(); the model's mode is left
    as it was; chunk_rows cuts the forward into chunks."""
    from alphaquoridorgnn_amd.replay import row_metrics_reduce_reference, row_metrics_reference
    from alphaquoridorgnn_amd.validation import Metrics, row_metrics
    rng = np.random.RandomState(9)
    w = _host_window(rng)
    model = StubModel().train()
    s72, pi, z = w.tensors()
    got = w.row_metrics(model)
    assert model.training and isinstance(got, Metrics) and got.rows == len(w) == 120 and got.rejected == 0
    model.eval()
    net, v = model.forward_states(s72.index_select(0, w.index()))
    vals, tag = row_metrics_reference(s72.numpy(), pi.numpy(), z.numpy(), net.numpy(), v[:, 0].numpy(), w.index().numpy())
    sums, counts = row_metrics_reduce_reference(vals, tag)
    assert got.sums.tobytes() == sums.tobytes() and np.array_equal(got.counts, counts)
    assert abs(got.policy_ce - vals[:, 0].mean()) < 1e-12 and abs(got.policy_loss - vals[:, 2].mean()) < 1e-12
    assert abs(got.kl - (vals[:, 0] - vals[:, 1]).mean()) < 1e-12 and abs(got.value_mse - vals[:, 3].mean()) < 1e-12
    assert got.top1 == ((tag >> 8) & 1).mean() and got.value_sign == ((tag >> 10) & 1).sum() / ((tag >> 9) & 1).sum()
    chunked = row_metrics(model, s72, pi, z, w.index(), chunk_rows=7)
    assert model.forwards == 1 + 1 + 18 and np.array_equal(chunked.counts[:, 0], got.counts[:, 0])
    assert np.allclose(chunked.sums, got.sums, rtol=1e-5, atol=0)   # (the stub's host matmul rounds by batch size; the statements do not)
    lines = got.table().splitlines()
    assert lines[0].split() == ["plies", "rows", "CE", "H(t)", "KL", "P", "loss", "V", "MSE", "top-1", "sign"]
    assert [x.split()[0] for x in lines[1:]] == ["0-7", "8-15", "16-23", "24-31", "32-39", "all"] and lines[-1].split()[1] == "120"
    other = row_metrics(model, s72, pi, z, w.index(), bucket_plies=16, buckets=2)
    assert other.counts[:, 0].tolist() == [int(counts[:2, 0].sum()), int(counts[2:, 0].sum()), 0] and abs(other.kl - got.kl) < 1e-12
    json.dumps(got.as_dict())
    empty = row_metrics(model, s72[:0], pi[:0], z[:0])
    assert empty.rows == 0 and np.isnan(empty.kl)
    for bad in (dict(buckets=0), dict(bucket_plies=0), dict(chunk_rows=0)):
        with pytest.raises(ValueError):
            row_metrics(model, s72, pi, z, **bad)
    with pytest.raises(ValueError):
        row_metrics(model, s72, pi.double(), z)
    with pytest.raises(ValueError):
        row_metrics(model, s72, pi, z, w.index().int())


def test_window_holdout_split_on_host_rows():
    from alphaquoridorgnn_amd.replay import ReplayWindow, holdout_split_reference
    rng = np.random.RandomState(11)
    w = _host_window(rng)
    train, held = w.holdout_split(0.25, seed=3)
    want = holdout_split_reference(w.tensors()[0].numpy(), w.index().numpy(), 0.25, 3)
    assert train.dtype == torch.int64 and np.array_equal(train.numpy(), want[0]) and np.array_equal(held.numpy(), want[1])
    assert 0 < len(held) < 120
    with pytest.raises(ValueError, match="share"):
        w.holdout_split(1.0)
    empty = ReplayWindow(5).holdout_split(0.5)
    assert empty[0].numel() == 0 and empty[1].numel() == 0


class _StubTrainer:
    """Records every epoch's order and moves the model's weights, the same way whatever the rows: epoch k leaves the first weights
    scaled by SCALES[k] -- towards a flat policy and past it, so the held-out loss falls and rises again."""

    max_grad_norm = None
    average = None
    SCALES = (0.8, 0.4, 0.1, -0.3, -0.7, -1.1)

    def __init__(self, model):
        self.model, self.orders, self.first = model, [], model.w.clone()

    def run_epoch(self, s, p, v, order, lr=0.001, mirror=None):
        self.orders.append(order.clone())
        self.model.w = self.first * self.SCALES[len(self.orders) - 1]
        return torch.tensor([1.0, 0.5])


def _run_loop(monkeypatch, tmp_path, window, **settings):
    from alphaquoridorgnn_amd import constants, distributed as aqd, train_network as tn
    monkeypatch.chdir(tmp_path)
    os.makedirs(constants.PV_NETWORK_PATH, exist_ok=True)
    monkeypatch.setattr(aqd, "device", lambda: torch.device("cpu"))
    monkeypatch.setattr(tn, "NUM_EPOCH", 6)
    monkeypatch.setattr(tn, "TRAIN_WINDOW", window)
    for name, value in settings.items():
        monkeypatch.setattr(tn, name, value)
    made = []

    def make_trainer(model, max_batch):
        made.append(_StubTrainer(model))
        return made[-1]

    torch.manual_seed(3)
    tn._train_loop(lambda path, dev: StubModel(), make_trainer, 0, 1)
    return made[0], torch.load(constants.PV_NETWORK_PATH + "latest.pth", weights_only=True)


def test_the_loop_on_a_host_window(monkeypatch, tmp_path, capsys):
    """_train_loop with a stub model and trainer on a host window: the option off trains on every row and prints no validation; with
    share 0.25 no held-out slot appears in any epoch's order, the training side is the host-built one, every TRAIN_HOLDOUT_EVERY-th
    epoch and the last are validated, the curve is row_metrics of the model as it then was, the log line parses and holds the printed
    numbers, and TRAIN_HOLDOUT_KEEP_BEST saves the snapshot of the first minimum."""
    from alphaquoridorgnn_amd import train_network as tn
    from alphaquoridorgnn_amd.replay import holdout_split_reference
    rng = np.random.RandomState(12)
    w = _host_window(rng)
    trainer, off = _run_loop(monkeypatch, tmp_path, w)
    out = capsys.readouterr().out
    assert "Val Loss" not in out and "held out" not in out and len(trainer.orders) == 6
    assert all(sorted(o.tolist()) == sorted(w.index().tolist()) for o in trainer.orders)
    want_train, want_held = holdout_split_reference(w.tensors()[0].numpy(), w.index().numpy(), 0.25, 5)
    log = tmp_path / "val.jsonl"
    trainer, on = _run_loop(monkeypatch, tmp_path, w, TRAIN_HOLDOUT_SHARE=0.25, TRAIN_HOLDOUT_SEED=5, TRAIN_HOLDOUT_EVERY=4,
                            TRAIN_HOLDOUT_LOG=str(log))
    out = capsys.readouterr().out
    distinct = len({bytes(r) for r in w.tensors()[0].numpy()[want_held][:, [k for k in range(72) if k not in (68, 69, 71)]]})
    assert f"held out: {len(want_held)} of 120 rows ({distinct} distinct positions)" in out
    assert all(sorted(o.tolist()) == sorted(want_train.tolist()) for o in trainer.orders) and not set(want_held) & set(want_train)
    assert torch.equal(on["w"], off["w"])                           # the stub's update does not depend on the rows: the last iterate
    assert torch.equal(on["w"], StubModel().w * _StubTrainer.SCALES[-1])
    lines = [x for x in out.replace("\r", "\n").splitlines() if x.startswith("Epoch")]
    assert [("Val Loss" in x) for x in lines] == [False, False, False, True, False, True]
    record = json.loads(log.read_text().splitlines()[-1])
    assert [c["epoch"] for c in record["curve"]] == [4, 6] and record["saved_epoch"] == 6
    assert record["split"] == dict(rows=120, held=len(want_held), train=len(want_train), distinct=distinct)
    assert record["options"]["share"] == 0.25 and record["options"]["seed"] == 5 and record["options"]["every"] == 4
    last = record["curve"][-1]
    assert f"| Val Loss: {last['policy_loss']:.4f} / {last['value_mse']:.4f} | Val KL: {last['kl']:.4f} | Top-1: {last['top1']:.3f}" in lines[-1]
    assert record["table"]["totals"]["rows"] == len(want_held) and record["table"]["totals"]["rejected"] == 0
    # the curve is the validation of the model as it was after each epoch: a hand-run twin
    twin = _StubTrainer(StubModel())
    curve, states = [], []
    for epoch in range(6):
        twin.run_epoch(None, None, None, torch.zeros(1), lr=tn.LEARNING_RATE * tn.lr_lambda(epoch))
        metrics = w.row_metrics(twin.model, torch.from_numpy(want_held))
        curve.append(metrics.policy_loss + metrics.value_mse)
        states.append(twin.model.w.clone())
    assert abs(record["curve"][0]["score"] - curve[3]) < 1e-12 and abs(record["curve"][1]["score"] - curve[5]) < 1e-12
    # keep best: the snapshot of the first minimum of the validated curve
    trainer, kept = _run_loop(monkeypatch, tmp_path, w, TRAIN_HOLDOUT_SHARE=0.25, TRAIN_HOLDOUT_SEED=5, TRAIN_HOLDOUT_EVERY=1,
                              TRAIN_HOLDOUT_KEEP_BEST=True, TRAIN_HOLDOUT_LOG=str(log))
    out = capsys.readouterr().out
    best = int(np.argmin(curve))
    assert 0 < best < 5 and f"kept epoch {best + 1}/6" in out and torch.equal(kept["w"], states[best]) and not torch.equal(kept["w"], on["w"])
    record = json.loads(log.read_text().splitlines()[-1])
    assert record["saved_epoch"] == best + 1 and len(record["curve"]) == 6 and len(log.read_text().splitlines()) == 2
    assert abs(record["table"]["totals"]["policy_loss"] + record["table"]["totals"]["value_mse"] - curve[best]) < 1e-12
    # an empty side names the share
    tiny = _host_window(np.random.RandomState(1), rows=71, distinct=1)
    with pytest.raises(ValueError, match="TRAIN_HOLDOUT_SHARE = 0.25"):
        _run_loop(monkeypatch, tmp_path, tiny, TRAIN_HOLDOUT_SHARE=0.25)
