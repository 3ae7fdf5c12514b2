"""CPU tests (no GPU) of the mirror-symmetry augmentation: the host statements of the mirror (game_logic.mirror_action(s),
mirror_record, State.mirror), that the mirror is a symmetry of the rules (the host build of the rule header the kernels compile), the
seeded draw in numpy (train_network.draw_mirror_flips), self_play.mirror_history and the options -- and the numpy statement of
aqg_augment_gather that tests/test_mirror_augment.py holds the kernel to."""
import ctypes
import json
import os

import numpy as np
import pytest

from tests import _util as U

SIZES = (3, 5, 7, 9)
_MASK64 = (1 << 64) - 1
_GOLDEN = 0x9E3779B97F4A7C15


# ------------------------------------------------------------------ aqg_augment_gather, stated in numpy (imported by the GPU tests)
def augment_reference(board_size, states72=None, pi=None, z=None, order=None, flips=None):
    """(out72, out_pi, out_z) of aqg_augment_gather in table mode; flips None = a plain gather.  pi moves as int32 bit patterns."""
    from alphaquoridorgnn_amd.game_logic import mirror_actions, mirror_record
    rows = next(x for x in (states72, pi, z) if x is not None).shape[0]
    order = np.arange(rows) if order is None else np.asarray(order, dtype=np.int64)
    flip = np.zeros(rows, dtype=bool) if flips is None else np.asarray(flips) != 0
    f = flip[order]
    out72 = out_pi = out_z = None
    if states72 is not None:
        out72 = states72[order].copy()
        if f.any():
            out72[f] = mirror_record(out72[f])
    if pi is not None:
        bits = pi.view(np.int32)[order].copy()
        src = mirror_actions(np.arange(pi.shape[1]), board_size)          # an involution: out[mirror(a)] = in[a] is out = in[:, src]
        bits[f] = bits[f][:, src]
        out_pi = bits.view(np.float32)
    if z is not None:
        out_z = z[order].copy()
    return out72, out_pi, out_z


def walk_records(board_size):
    """The walk fixture's records: all of 3x3 and 5x5, every 28th of 9x9 (500 records over the whole walk)."""
    states = U.golden(f"walk_{board_size}x{board_size}.npz")["states"]
    return states if board_size < 9 else states[::28]


# ------------------------------------------------------------------ the maps
@pytest.mark.parametrize("N", SIZES)
def test_mirror_action_is_an_involution_inside_each_block(N):
    from alphaquoridorgnn_amd.game_logic import mirror_action, mirror_actions, num_actions
    V, NW, A = N * N, (N - 1) ** 2, num_actions(N)
    a = np.arange(A)
    m = mirror_actions(a, N)
    assert m.dtype == np.int64 and sorted(m.tolist()) == a.tolist()                  # a bijection
    assert np.array_equal(mirror_actions(m, N), a)                                    # an involution
    block = lambda x: (x >= V).astype(int) + (x >= V + NW).astype(int)
    assert np.array_equal(block(m), block(a))
    assert [mirror_action(int(x), N) for x in a] == m.tolist()
    # the formulas of the issue, spelled out
    W = N - 1
    for x in range(A):
        if x < V:
            want = (x // N) * N + (N - 1 - x % N)
        else:
            base = V if x < V + NW else V + NW
            i = x - base
            want = base + (i // W) * W + (W - 1 - i % W)
        assert m[x] == want
    assert mirror_action(N // 2, N) == N // 2 and mirror_action(0, N) == N - 1         # the centre column is fixed
    for bad in (-1, A):
        with pytest.raises(ValueError):
            mirror_action(bad, N)
    with pytest.raises(ValueError):
        mirror_actions([0], 4)


@pytest.mark.parametrize("N", (3, 5, 9))
def test_mirror_record_twice_is_the_identity(N):
    from alphaquoridorgnn_amd.game_logic import State, mirror_record
    recs = walk_records(N)
    m = mirror_record(recs)
    assert m.dtype == np.uint8 and m.shape == recs.shape
    assert np.array_equal(mirror_record(m), recs)
    assert not np.array_equal(m, recs)
    for k in (1, 3, 68, 69, 70, 71):
        assert np.array_equal(m[:, k], recs[:, k])
    nw = (N - 1) ** 2
    assert np.array_equal(m[:, 4 + nw:68], recs[:, 4 + nw:68])
    assert np.array_equal(np.sort(m[:, 4:4 + nw], axis=1), np.sort(recs[:, 4:4 + nw], axis=1))       # values kept, slots moved
    W = N - 1
    for i in range(nw):                                      # the slot formula of the issue, directly
        assert np.array_equal(m[:, 4 + (i // W) * W + (W - 1 - i % W)], recs[:, 4 + i])
    for k in (0, 2):                                         # ... and the position formula
        assert np.array_equal(m[:, k], (recs[:, k] // N) * N + (N - 1 - recs[:, k] % N))
    assert np.array_equal(m[:, 0] // N, recs[:, 0] // N) and np.array_equal(m[:, 0] % N, N - 1 - recs[:, 0] % N)
    assert np.array_equal(mirror_record(recs[7]), m[7])                                 # one record is the batch's row
    s = State.from_record(recs[7]).mirror()
    assert np.array_equal(s.record(), m[7]) and np.array_equal(s.mirror().record(), recs[7])
    off = recs[:3].copy()
    off[:, 0], off[:, 2] = N * N, 255                                                 # no tile of the board: copied through
    mo = mirror_record(off)
    assert np.array_equal(mo[:, 0], off[:, 0]) and np.array_equal(mo[:, 2], off[:, 2])
    with pytest.raises(ValueError):
        mirror_record(np.zeros(71, np.uint8))


def _host_legal(lib, N, rec):
    out = np.empty(U.MAX_LEGAL, dtype=np.uint8)
    c = lib.aqg_host_legal_actions(N, rec.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p))
    assert 0 <= c <= U.MAX_LEGAL
    return out[:c].astype(np.int64)


def _host_next(lib, N, rec, a):
    out = np.empty(72, dtype=np.uint8)
    assert lib.aqg_host_next(N, rec.ctypes.data_as(ctypes.c_void_p), int(a), out.ctypes.data_as(ctypes.c_void_p)) == 0
    return out


@pytest.mark.parametrize("N", (3, 5, 9))
def test_the_rules_commute_with_the_mirror(N):
    """legal(mirror(s)) == mirror(legal(s)) as SETS (the list order changes), and mirror(next(s, a)) == next(mirror(s), mirror(a)):
    for every legal action at 3x3, for one sampled action per record elsewhere."""
    from alphaquoridorgnn_amd import _lib
    from alphaquoridorgnn_amd.game_logic import mirror_actions, mirror_record
    lib = _lib.load()
    recs = np.ascontiguousarray(walk_records(N))
    mirrored = np.ascontiguousarray(mirror_record(recs))
    rng = np.random.RandomState(20261018 + N)
    reordered = checked = 0
    for rec, mrec in zip(recs, mirrored):
        legal = _host_legal(lib, N, rec)
        want = mirror_actions(legal, N)
        got = _host_legal(lib, N, mrec)
        assert sorted(got.tolist()) == sorted(want.tolist())
        reordered += int(not np.array_equal(got, want))
        if len(legal) == 0:
            continue
        for a in (legal if N == 3 else [legal[rng.randint(len(legal))]]):
            ma = int(mirror_actions(a, N))
            assert np.array_equal(mirror_record(_host_next(lib, N, rec, a)), _host_next(lib, N, mrec, ma))
            checked += 1
    assert checked >= len(recs) // 2
    assert reordered > 0                    # why sets are compared, not lists


# ------------------------------------------------------------------ the seeded draw
def _mix(z):
    z &= _MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK64
    return z ^ (z >> 31)


def _flip_int(seed, epoch, r):
    """counter_rng.hpp in Python integers: counter_uniform(stream_key(seed, epoch), r) < 0.5."""
    key = _mix(seed + _GOLDEN * (epoch + 1))
    return int((_mix(key + _GOLDEN * (r + 1)) >> 11) * 2.0 ** -53 < 0.5)


# the formula above evaluated by hand (Python integers) for rows 0..15 of (seed 0, epoch 0) and of (seed 20261018, epoch 1)
FLIPS_0_0 = [0, 0, 1, 0, 0, 1, 0, 1, 1, 0, 1, 1, 1, 0, 0, 1]
FLIPS_20261018_1 = [0, 1, 0, 1, 1, 0, 1, 0, 1, 0, 0, 1, 1, 0, 1, 1]


def test_draw_mirror_flips():
    from alphaquoridorgnn_amd.train_network import draw_mirror_flips
    a = draw_mirror_flips(7, 3, 1000)
    assert a.dtype == np.uint8 and a.shape == (1000,) and set(a.tolist()) == {0, 1}
    assert np.array_equal(a, draw_mirror_flips(7, 3, 1000))
    for n in (0, 1, 37, 64, 999):                    # a function of (seed, epoch, index) alone
        assert np.array_equal(draw_mirror_flips(7, 3, n), a[:n])
    assert not np.array_equal(draw_mirror_flips(8, 3, 1000), a)
    assert not np.array_equal(draw_mirror_flips(7, 4, 1000), a)
    assert 400 < int(a.sum()) < 600                  # a fair coin: 500 +- 6.3 standard deviations of 15.8
    for seed, epoch in ((7, 3), (0, 0), (2 ** 64 - 1, 99), (123456789, 0)):
        got = draw_mirror_flips(seed, epoch, 70)
        assert got.tolist() == [_flip_int(seed, epoch, r) for r in range(70)]
    assert [_flip_int(0, 0, r) for r in range(16)] == FLIPS_0_0
    assert draw_mirror_flips(0, 0, 16).tolist() == FLIPS_0_0
    assert draw_mirror_flips(20261018, 1, 16).tolist() == FLIPS_20261018_1


# ------------------------------------------------------------------ the history file
def test_mirror_history_doubles_the_golden_history():
    from alphaquoridorgnn_amd.self_play import mirror_history
    with open(os.path.join(U.GOLDEN, "history_9x9.json")) as f:
        history = json.load(f)["history"]
    n = len(history)
    both = mirror_history(history)
    assert len(both) == 2 * n and both[:n] == history
    for row, m in zip(history, both[n:]):
        (player, enemy, walls), pol, z = m
        assert isinstance(m, list) and len(m) == 3 and len(player) == 2 and len(enemy) == 2 and len(walls) == 64 and len(pol) == 209
        assert all(type(x) is int for x in player + enemy + walls)
        assert z == row[2] and type(z) is type(row[2])
        assert player[1] == row[0][0][1] and enemy[1] == row[0][1][1]
        assert sum(pol) == pytest.approx(sum(row[1]), abs=1e-12) and sorted(pol) == sorted(row[1])
    assert any(m != row for row, m in zip(history, both[n:]))
    again = mirror_history(both[n:])
    assert again[n:] == history                         # mirroring the second half gives back the first
    with pytest.raises(ValueError):
        mirror_history([[[[76, 10], [76, 10], [0] * 64], [0.0] * 57, 1]])


# ------------------------------------------------------------------ options and ABI
def test_options_and_abi():
    from alphaquoridorgnn_amd import _lib, train_network as tn
    from alphaquoridorgnn_amd.train_cycle import _parser, _set_mirror_options
    assert tn.TRAIN_MIRROR is False and tn.TRAIN_MIRROR_SEED == 0
    saved = tn.TRAIN_MIRROR, tn.TRAIN_MIRROR_SEED
    try:
        _set_mirror_options(_parser().parse_args([]))
        assert (tn.TRAIN_MIRROR, tn.TRAIN_MIRROR_SEED) == (False, 0)
        _set_mirror_options(_parser().parse_args(["--mirror-augment", "--mirror-seed", "41"]))
        assert (tn.TRAIN_MIRROR, tn.TRAIN_MIRROR_SEED) == (True, 41)
    finally:
        tn.TRAIN_MIRROR, tn.TRAIN_MIRROR_SEED = saved
    assert _lib.ABI_VERSION == 15 and _lib.load().aqg_abi_version() == 15
    with open(os.path.join(U.REPO, "include", "aqgnn.h")) as f:
        assert "#define AQG_ABI_VERSION 15\n" in f.read()


@pytest.mark.parametrize("kw,word", [(dict(board_size=4), "board_size"), (dict(policy_size=208), "policy_size"), (dict(n=-1), "negative"),
                                     (dict(out72=None), "both"), (dict(alias=True), "overlaps"),
                                     (dict(out72=0x100000, order=0x300000), "overlaps")])
def test_library_refuses_before_it_launches(kw, word):
    """The argument errors of aqg_augment_gather come back before anything touches a device (dummy pointers)."""
    from alphaquoridorgnn_amd import _lib
    lib = _lib.load()
    a = dict(board_size=9, policy_size=209, n=8, states72=0x100000, out72=0x200000)
    alias = kw.pop("alias", False)
    a.update(kw)
    if alias:
        a["out72"] = a["states72"] + 72 * 7            # the last source row
    rc = lib.aqg_augment_gather(a["board_size"], a["policy_size"], a["states72"], None, None, a.get("order"), None, 0, 0, 0, a["n"],
                                a["out72"], None, None, None)
    assert rc != 0 and word in lib.aqg_last_error().decode()


def test_library_takes_zero_rows_whatever_the_pointers():
    """n == 0 writes nothing and returns 0 without looking at the pointers: an empty output array's pointer may be NULL next to a
    non-empty source (a rank without a position of a ragged last batch gathers zero rows from the whole history)."""
    from alphaquoridorgnn_amd import _lib
    lib = _lib.load()
    for s72, pi, z, o72, opi, oz in ((0x100000, 0x200000, 0x300000, None, None, None), (None, None, None, None, None, None),
                                     (0x100000, None, None, 0x100000, None, None)):
        assert lib.aqg_augment_gather(9, 209, s72, pi, z, 0x400000, None, 1, 5, 2, 0, o72, opi, oz, None) == 0
    assert lib.aqg_augment_gather(9, 208, 0x100000, None, None, None, None, 0, 0, 0, 0, None, None, None, None) != 0      # still an error
