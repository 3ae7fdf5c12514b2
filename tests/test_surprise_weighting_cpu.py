"""Policy surprise weighting without a GPU: the numpy statements of replay.py (surprise_reference, surprise_weights,
surprise_counts_reference, expand_rows) against the definition of include/aqgnn.h, the defaults, and the command-line refusals."""
import os
import re
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests._surprise import (BOARDS, EXACT, SPECIAL, exact_rows, k_bar, network_rows, plain_kl, policy_size, special_rows,   # noqa: E402
                             target_rows, within_bar)


# ------------------------------------------------------------------ steps 1 and 2
@pytest.mark.parametrize("N", BOARDS)
def test_reference_against_the_plain_formula(N):
    """k of the ordered statement against numpy's own float64 sum of the same terms: one f32 ulp plus what reordering A terms can move
    a float64 sum by (A 2^-53 times the sum of the terms' magnitudes).  With and without an index that reorders and skips rows."""
    from alphaquoridorgnn_amd.replay import surprise_reference, surprise_weights
    A, rng = policy_size(N), np.random.RandomState(10 + N)
    pi = target_rows(rng, 90, A)
    for index in (None, rng.permutation(90)[:70].astype(np.int64)):
        m = 90 if index is None else 70
        net = network_rows(rng, m, A)
        k, q = surprise_reference(pi, net, index)
        t = pi if index is None else pi[index]
        kl, mag = plain_kl(t, net)
        assert k.dtype == np.float32 and q.dtype == np.int32 and k.shape == q.shape == (m,)
        assert np.all(np.abs(k.astype(np.float64) - np.maximum(kl, 0)) <= np.spacing(k).astype(np.float64) + A * 2.0 ** -53 * mag)
        assert np.all(k >= 0) and np.all(k <= 126 * np.log(2)) and k.max() > 1.0
        assert np.array_equal(q, surprise_weights(k)) and np.all(q >= 0) and np.all(q < 2 ** 27)
        assert np.all(within_bar(k, k, t)) and np.all(k_bar(k, t) < 2e-5)


@pytest.mark.parametrize("N", BOARDS)
def test_exact_cases(N):
    from alphaquoridorgnn_amd.replay import surprise_reference
    A = policy_size(N)
    pi, net, want = exact_rows(np.random.RandomState(N), A)
    k, q = surprise_reference(pi, net)
    assert len(want) == len(EXACT)
    for i, w in enumerate(want):
        assert k[i].tobytes() == w.tobytes(), (EXACT[i], k[i], w)
    assert q[0] == 0 and q[1] == 0
    assert k[2] == np.float32(126 * np.log(2)) and abs(float(k[3]) - 0.5 * (126 - 1) * np.log(2)) < 1e-5


@pytest.mark.parametrize("N", BOARDS)
def test_every_special_row_reads_zero(N):
    from alphaquoridorgnn_amd.replay import surprise_reference
    A, rng = policy_size(N), np.random.RandomState(20 + N)
    pi, net = special_rows(rng, A)
    k, q = surprise_reference(pi, net)
    assert len(k) == len(SPECIAL) and not k.any() and not q.any(), dict(zip(SPECIAL, k))
    # beside ordinary rows they change nothing, and an index entry outside the arrays is one more such row
    more_pi, more_net = target_rows(rng, 5, A), network_rows(rng, 5, A)
    both_k, _ = surprise_reference(np.concatenate([pi, more_pi]), np.concatenate([net, more_net]))
    assert not both_k[:len(SPECIAL)].any() and np.array_equal(both_k[len(SPECIAL):], surprise_reference(more_pi, more_net)[0])
    out_k, out_q = surprise_reference(more_pi, more_net, index=np.array([0, 5, 2, -1, 4], np.int64))
    assert out_k[1] == 0 and out_k[3] == 0 and out_q[1] == 0 and out_k[0] > 0 and out_k[2] > 0


def test_weights_at_the_steps_of_q():
    """q = floor(k 2^20): at k = i 2^-20 it is i, one f32 ulp under it i - 1."""
    from alphaquoridorgnn_amd.replay import surprise_weights
    i = np.array([1, 2, 3, 1000, 2 ** 20, 2 ** 20 + 1, 5 * 2 ** 20 + 77, 87 * 2 ** 20 + 12344, 2 ** 26 + 8], dtype=np.int64)
    k = (i.astype(np.float64) * 2.0 ** -20).astype(np.float32)
    assert np.array_equal(k.astype(np.float64) * 2.0 ** 20, i)                    # every one a float32
    assert np.array_equal(surprise_weights(k), i)
    under = np.nextafter(k, np.float32(0))
    step = np.maximum((np.spacing(under).astype(np.float64) * 2.0 ** 20).astype(np.int64), 1)      # an f32 ulp is 2, 4, 8 steps of q from k = 16 on
    assert step.tolist() == [1, 1, 1, 1, 1, 1, 1, 8, 8]
    assert np.array_equal(surprise_weights(under), i - step)
    assert surprise_weights(np.zeros(3, np.float32)).tolist() == [0, 0, 0]
    assert int(surprise_weights(np.array([88.0], np.float32))[0]) == 88 * 2 ** 20 < 2 ** 27
    with pytest.raises(ValueError):
        surprise_weights(np.zeros(3, np.float64))


# ------------------------------------------------------------------ steps 3 and 4
def _f(q, E, U):
    q = np.asarray(q, np.float64)
    m, S = len(q), q.sum()
    return (E * U) / m + ((E * (1 - U)) * q) / S if S > 0 else np.full(m, E / m)


@pytest.mark.parametrize("m", (1, 5, 49, 256, 1000))
def test_counts_follow_the_expected_copies(m):
    from alphaquoridorgnn_amd.replay import surprise_counts_reference
    rng = np.random.RandomState(m)
    q = (rng.exponential(0.3, m) * 2 ** 20).astype(np.int32)
    q[rng.permutation(m)[:m // 4]] = 0
    slots = rng.permutation(4 * m)[:m].astype(np.int64)
    for E, U, C in ((m, 0.5, 8), (3 * m + 1, 0.25, 255), (max(m // 2, 1), 0.0, 2), (m, 0.5, 1)):
        f = _f(q, np.float64(E), np.float64(U))
        assert abs(f.sum() - E) <= m * 2.0 ** -52 * E
        c = surprise_counts_reference(q, slots, 7, 3, E, U, C)
        lo = np.floor(f)
        assert c.dtype == np.int32 and np.all((c == np.minimum(lo, C)) | (c == np.minimum(lo + 1, C)))
        assert np.array_equal(c[f == lo], np.minimum(lo, C)[f == lo].astype(np.int32))      # a whole f is never rounded up
        if C == 255 and m >= 256:
            assert abs(int(c.sum()) - E) < 6 * np.sqrt(m) + 1 and len(set(c.tolist())) > 2
        if C == 1:
            assert set(c.tolist()) <= {0, 1}


@pytest.mark.parametrize("m", (1, 7, 49, 64, 1000))
def test_uniform_share_one_is_every_row_c_times(m):
    """U = 1, E = c m: f = c exactly, so every count is c -- at m = 49, where 1 / 49 is no float64, too; and S = 0 is uniform."""
    from alphaquoridorgnn_amd.replay import surprise_counts_reference
    q = np.random.RandomState(m).randint(0, 2 ** 26, m).astype(np.int32)
    assert surprise_counts_reference(q, None, 1, 2, m, 1.0, 8).tolist() == [1] * m
    assert surprise_counts_reference(q, None, 1, 2, 2 * m, 1.0, 8).tolist() == [2] * m
    assert surprise_counts_reference(q, None, 1, 2, 9 * m, 1.0, 8).tolist() == [8] * m               # capped
    zero = np.zeros(m, np.int32)
    assert surprise_counts_reference(zero, None, 1, 2, m, 0.5, 8).tolist() == [1] * m
    assert surprise_counts_reference(zero, None, 1, 2, 3 * m, 0.0, 8).tolist() == [3] * m
    if m > 1:
        half = surprise_counts_reference(zero, None, 1, 2, m // 2, 0.5, 8)
        assert set(half.tolist()) <= {0, 1} and half.sum() < m


def test_a_rows_draw_is_its_own():
    """u is keyed by (seed, update, slot): dropping other rows, or reordering them, leaves a row's draw -- so with f held fixed its
    count -- unchanged; another update or seed draws afresh."""
    from alphaquoridorgnn_amd.counter_rng import counter_uniform, stream_key
    from alphaquoridorgnn_amd.replay import surprise_counts_reference
    m = 400
    slots = np.random.RandomState(1).permutation(5000)[:m].astype(np.int64)
    zero = np.zeros(m, np.int32)                                 # S = 0: f = E / m for every row, whatever the others are
    E = m // 2                                                   # f = 0.5
    whole = surprise_counts_reference(zero, slots, 11, 4, E, 0.5, 8)
    u = counter_uniform(stream_key(11, 4), slots.astype(np.uint64))
    assert np.array_equal(whole, (u < 0.5).astype(np.int32)) and 120 < whole.sum() < 280
    keep = np.random.RandomState(2).permutation(m)[:100]
    part = surprise_counts_reference(zero[keep], slots[keep], 11, 4, 50, 0.5, 8)
    assert np.array_equal(part, whole[keep])
    assert not np.array_equal(surprise_counts_reference(zero, slots, 11, 5, E, 0.5, 8), whole)
    assert not np.array_equal(surprise_counts_reference(zero, slots, 12, 4, E, 0.5, 8), whole)
    assert np.array_equal(surprise_counts_reference(zero, None, 11, 4, E, 0.5, 8),
                          surprise_counts_reference(zero, np.arange(m), 11, 4, E, 0.5, 8))


def test_crafted_weights():
    """One dominant row hits C; f with a fraction of exactly 0 stays, of exactly 0.5 follows the draw."""
    from alphaquoridorgnn_amd.counter_rng import counter_uniform, stream_key
    from alphaquoridorgnn_amd.replay import surprise_counts_reference
    q = np.zeros(64, np.int32)
    q[5] = 80 * 2 ** 20
    c = surprise_counts_reference(q, None, 0, 0, 64, 0.5, 8)              # f = 0.5 everywhere, 32.5 at row 5
    u = counter_uniform(stream_key(0, 0), np.arange(64, dtype=np.uint64))
    want = (u < 0.5).astype(np.int32)
    want[5] = 8
    assert np.array_equal(c, want)
    q = np.array([1, 1, 2, 4], np.int32)                                  # S = 8, E = 16, U = 0.5: f = 2 + q = 3, 3, 4, 6
    assert surprise_counts_reference(q, None, 3, 9, 16, 0.5, 5).tolist() == [3, 3, 4, 5]
    q = np.array([1, 3], np.int32)                                        # S = 4, E = 4, U = 0.5: f = 1 + 0.5, 1 + 1.5
    u = counter_uniform(stream_key(3, 9), np.arange(2, dtype=np.uint64))
    assert surprise_counts_reference(q, None, 3, 9, 4, 0.5, 8).tolist() == [1 + int(u[0] < 0.5), 2 + int(u[1] < 0.5)]


def test_the_statements_refuse_what_the_library_refuses():
    from alphaquoridorgnn_amd.replay import check_surprise_options, surprise_counts_reference, surprise_reference
    q = np.ones(4, np.int32)
    for bad in (dict(uniform_share=-0.1), dict(uniform_share=1.5), dict(uniform_share=float("nan")), dict(max_copies=0),
                dict(max_copies=256), dict(max_copies=2.5), dict(expected_rows=0), dict(expected_rows=-3), dict(expected_rows=None)):
        kw = dict(expected_rows=4, uniform_share=0.5, max_copies=8)
        kw.update(bad)
        with pytest.raises(ValueError):
            surprise_counts_reference(q, None, 0, 0, **kw)
    with pytest.raises(ValueError):
        surprise_counts_reference(q.astype(np.int64), None, 0, 0, 4, 0.5, 8)
    with pytest.raises(ValueError):
        surprise_counts_reference(q, np.arange(3), 0, 0, 4, 0.5, 8)
    assert check_surprise_options(None, 1, 255) == (None, 1.0, 255) and check_surprise_options(7, 0, 1) == (7, 0.0, 1)
    assert surprise_counts_reference(q[:0], None, 0, 0, 4, 0.5, 8).shape == (0,)
    pi = np.zeros((4, 17), np.float32)
    with pytest.raises(ValueError):
        surprise_reference(pi, np.zeros((5, 17), np.float32))                       # more policies than rows, no index
    with pytest.raises(ValueError):
        surprise_reference(pi, np.zeros((4, 57), np.float32))
    with pytest.raises(ValueError):
        surprise_reference(pi.astype(np.float64), np.zeros((4, 17), np.float32))
    with pytest.raises(ValueError):
        surprise_reference(pi, np.zeros((4, 17), np.float32), index=np.arange(3))


# ------------------------------------------------------------------ step 5
def test_the_expansion_is_numpys_repeat():
    from alphaquoridorgnn_amd.replay import expand_rows
    rng = np.random.RandomState(5)
    for m in (1, 16, 257):
        base = rng.permutation(3 * m)[:m].astype(np.int64)
        count = rng.randint(0, 9, m).astype(np.int32)
        want = np.repeat(base, count)
        for total in (None, int(count.sum())):
            got = expand_rows(torch.from_numpy(base), torch.from_numpy(count), total)
            assert got.dtype == torch.int64 and np.array_equal(got.numpy(), want)
    assert expand_rows(torch.arange(4), torch.zeros(4, dtype=torch.int32), 0).numel() == 0


# ------------------------------------------------------------------ the surface
def test_defaults_and_the_binding():
    from alphaquoridorgnn_amd import _lib, replay, train_network as tn
    assert tn.TRAIN_SURPRISE_WEIGHTING is False and tn.TRAIN_SURPRISE_UNIFORM_SHARE == 0.5
    assert tn.TRAIN_SURPRISE_MAX_COPIES == 8 and tn.TRAIN_SURPRISE_SEED == 0
    import inspect
    sig = inspect.signature(tn._training_rows)
    assert list(sig.parameters) == ["dev", "board_size", "model"] and sig.parameters["model"].default is None
    sig = inspect.signature(replay.surprise_index)
    for name, default in (("index", None), ("expected_rows", None), ("uniform_share", 0.5), ("max_copies", 8), ("chunk_rows", 16384)):
        assert sig.parameters[name].default == default
    assert sig.parameters["seed"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["seed"].default is inspect.Parameter.empty
    assert replay.ReplayWindow(5).surprise_updates == 0
    with pytest.raises(ValueError):
        replay.ReplayWindow(5).surprise_index(None, seed=0)                       # a host window
    with open(os.path.join(REPO, "include", "aqgnn.h")) as f:
        header = f.read()
    assert re.search(r"#define\s+AQG_ABI_VERSION\s+15\b", header) and _lib.ABI_VERSION == 15
    for name in ("aqg_replay_surprise_rows", "aqg_replay_surprise_counts"):
        assert name in _lib.SIGNATURES and re.search(r"\bint " + name + r"\(", header)
    src = open(os.path.join(REPO, "alphaquoridorgnn_amd", "csrc", "replay_surprise.hip")).read()
    for text in ("SPR_GROUP = 4;", "SPR_WAVES = 4;", "SPR_LANES = 256;", "SPR_MAX_ROWS = 1 << 24;", "SPR_TINY = 0x1.0p-126f;",
                 "SPR_K_MAX = 88.0;", "SPR_Q_SCALE = 0x1.0p20;", "#pragma clang fp contract(off)"):
        assert text in src
    assert replay.SURPRISE_MAX_ROWS == 1 << 24 and replay.SURPRISE_K_MAX == 88.0 and replay.SURPRISE_Q_SCALE == 2.0 ** 20


def test_training_rows_needs_the_model(monkeypatch):
    from alphaquoridorgnn_amd import train_network as tn
    rows = (torch.zeros((3, 72), dtype=torch.uint8), torch.zeros((3, 57)), torch.zeros(3), None)
    monkeypatch.setattr(tn, "_recorded_rows", lambda dev, board_size: rows)
    assert tn._training_rows("cpu", 5) is not None and tn._training_rows("cpu", 5)[3] is None     # off: the rows as they are
    monkeypatch.setattr(tn, "TRAIN_SURPRISE_WEIGHTING", True)
    with pytest.raises(ValueError, match="model"):
        tn._training_rows("cpu", 5)


def test_command_line_refusals():
    from alphaquoridorgnn_amd import train_cycle as tc, train_network as tn
    parse = tc._parser().parse_args
    assert tc._check_surprise_args(parse([])) is None
    assert tc._check_surprise_args(parse(["--surprise-weighting"])) == (0.5, 8, 0)
    assert tc._check_surprise_args(parse(["--surprise-weighting", "--surprise-uniform-share", "0.25", "--surprise-max-copies", "3",
                                          "--surprise-seed", "9"])) == (0.25, 3, 9)
    for flags in (["--surprise-uniform-share", "0.5"], ["--surprise-max-copies", "4"], ["--surprise-seed", "1"]):
        with pytest.raises(ValueError, match="need --surprise-weighting"):
            tc._check_surprise_args(parse(flags))
    for flags in (["--surprise-uniform-share", "1.5"], ["--surprise-uniform-share", "-0.5"], ["--surprise-uniform-share", "nan"],
                  ["--surprise-max-copies", "0"], ["--surprise-max-copies", "256"]):
        with pytest.raises(ValueError):
            tc._check_surprise_args(parse(["--surprise-weighting"] + flags))
    assert tn.TRAIN_SURPRISE_WEIGHTING is False                  # checking sets nothing


def test_main_refuses_before_anything_else():
    """The coefficient flags without --surprise-weighting, and bad values with it, end main() at parse time: no device, no process group."""
    from alphaquoridorgnn_amd import train_cycle as tc
    for bad in (["--surprise-uniform-share", "0.5"], ["--surprise-max-copies", "2"], ["--surprise-seed", "3"],
                ["--surprise-weighting", "--surprise-uniform-share", "2"], ["--surprise-weighting", "--surprise-max-copies", "300"]):
        with pytest.raises(ValueError, match="surprise"):
            tc.main(["--cycles", "1"] + bad)
