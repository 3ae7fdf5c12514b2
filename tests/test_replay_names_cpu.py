"""The replay family's surface without a GPU or the library: every public name stays importable from alphaquoridorgnn_amd.replay
wherever it lives, the numpy statements import without torch, and the two refresh statements refuse alike."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

# what could be imported from alphaquoridorgnn_amd.replay when it was one module
PUBLIC_NAMES = (
    "ReplayWindow", "policy_size", "merge_positions", "surprise_index", "expand_rows",
    "check_value_blend", "blend_targets", "append_reference", "refresh_reference", "refresh_policy_reference", "draw_reanalyse_rows",
    "KEY_BYTES", "MERGE_CHUNK", "position_keys", "merge_depth", "merge_reference", "merge_runs_reference",
    "SURPRISE_MAX_ROWS", "SURPRISE_TINY", "SURPRISE_K_MAX", "SURPRISE_Q_SCALE", "check_surprise_options", "surprise_reference",
    "surprise_weights", "surprise_counts_reference")


@pytest.mark.parametrize("name", PUBLIC_NAMES)
def test_name_is_importable_from_replay(name):
    assert hasattr(importlib.import_module("alphaquoridorgnn_amd.replay"), name)


def test_replay_reference_imports_without_torch():
    code = ("import sys; import alphaquoridorgnn_amd.replay_reference as r; "
            "bad = [m for m in ('torch', 'alphaquoridorgnn_amd._lib') if m in sys.modules]; "
            "assert not bad, bad; assert r.MAX_LEGAL == 136; print('ok')")
    run = subprocess.run([sys.executable, "-c", code], cwd=REPO, capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stderr


def _message(call):
    with pytest.raises(ValueError) as err:
        call()
    return str(err.value)


def test_both_refresh_statements_refuse_alike():
    """The same bad arguments give both entries the same message, up to the entry's own name and how it names its source rows
    ("visits must be int32" / "policy must be float32")."""
    from alphaquoridorgnn_amd.replay import refresh_policy_reference, refresh_reference
    N, n, capacity, L = 5, 6, 10, 136
    A = N * N + 2 * (N - 1) ** 2
    actions = np.zeros((n, L), dtype=np.uint8)
    count = np.ones((n,), dtype=np.int32)
    q = np.zeros((n,), dtype=np.float32)
    slots = np.arange(n, dtype=np.int64)
    rpi, rz = np.zeros((capacity, A), dtype=np.float32), np.zeros((capacity,), dtype=np.float32)
    entries = ((refresh_reference, "refresh_reference", "visits must be int32", np.ones((n, L), dtype=np.int32)),
               (refresh_policy_reference, "refresh_policy_reference", "policy must be float32", np.ones((n, L), dtype=np.float32)))
    messages = []
    for entry, name, source_words, src in entries:
        bad = [lambda: entry(4, src, actions, count, None, 0.0, slots, rpi, rz),                    # no such board
               lambda: entry(N, src, actions, count, None, 0.5, slots, rpi, rz),                    # a blend without search_value
               lambda: entry(N, src, actions, count, q, 1.5, slots, rpi, rz),                       # a blend outside [0, 1]
               lambda: entry(N, src, actions, count, q, float("nan"), slots, rpi, rz),
               lambda: entry(N, src, actions, count, q, 0.5, slots, rpi[:0], rz),                   # no capacity
               lambda: entry(N, src, actions, count, q, 0.5, slots, rpi, None),                     # a blend without ring_z
               lambda: entry(N, src.astype(np.int64), actions, count, q, 0.5, slots, rpi, rz),      # the source: dtype, then shape
               lambda: entry(N, src[:, :100], actions, count, q, 0.5, slots, rpi, rz),
               lambda: entry(N, src, actions.astype(np.int8), count, q, 0.5, slots, rpi, rz),
               lambda: entry(N, src, actions, count[:5], q, 0.5, slots, rpi, rz),
               lambda: entry(N, src, actions, count, q.astype(np.float64), 0.5, slots, rpi, rz),
               lambda: entry(N, src, actions, count, q, 0.5, slots.astype(np.int32), rpi, rz),
               lambda: entry(9, src, actions, count, q, 0.5, slots, rpi, rz),                       # another board's policy rows
               lambda: entry(N, src, actions, count, q, 0.5, slots, rpi, rz[:5])]
        got = [_message(call) for call in bad]
        assert all(m.startswith(name + ": ") or m.startswith("value_blend must be") for m in got), got
        messages.append([m.replace(name + ": ", "ENTRY: ").replace(source_words, "SOURCE") for m in got])
    assert messages[0] == messages[1]
    assert sum("SOURCE" in m for m in messages[0]) == 2 and len(set(messages[0])) >= 11
