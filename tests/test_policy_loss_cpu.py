"""The loss form (include/aqgnn.h "loss form"), the part that needs no GPU: the numpy statement against torch in fp64, the
motivation pinned on a fixed row, the command-line flags, and the struct mirror against the header."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import _policy_loss as PL   # noqa: E402
from alphaquoridorgnn_amd.train_reference import check_loss_controls, loss_reference   # noqa: E402


# ---------------------------------------------------------------------------------------------- loss_reference against torch
@pytest.mark.parametrize("form", [PL.CE, PL.REFERENCE], ids=["cross_entropy", "reference"])
@pytest.mark.parametrize("w", [1.0, 0.25, 0.0])
@pytest.mark.parametrize("A", [17, 209])
def test_loss_reference_equals_torch(form, w, A):
    """Every row kind of edge_targets (one-hot last, one-hot first, uniform, dense, sums 0.5 and 1.75, all-zero, sparse; two of
    each), logits of spread 3: terms and both gradients within 1e-12 of fp64 CrossEntropyLoss + w MSELoss under autograd."""
    B = 16
    pi, z = PL.edge_targets(B, A, seed=A)
    rng = np.random.RandomState(A + 1)
    logits, vpre = rng.randn(B, A) * 3.0, rng.randn(B)
    terms, dlogits, dvpre, v = PL.torch_loss_terms(logits, vpre, pi, z, form, w)
    got = loss_reference(logits, v, pi, z, policy_form=form, value_weight=w)
    for name, a, b in zip(("terms", "dlogits", "dvpre"), got, (terms, dlogits, dvpre)):
        assert a.shape == b.shape, name
        assert np.abs(a - b).max() <= 1e-12, (name, np.abs(a - b).max())
    zero = [b for b in range(B) if b % 8 == 6]
    assert (got[0][zero, 0] == 0).all() and (got[1][zero] == 0).all()          # the all-zero rows: no term, no policy gradient


def test_cross_entropy_is_finite_where_the_policy_underflows():
    """All target mass on an action 800 logit units below the maximum (exp underflows even in fp64): the term is the gap itself."""
    x = np.zeros((1, 5))
    x[0, 2] = -800.0
    t = np.zeros((1, 5))
    t[0, 2] = 1.0
    terms = loss_reference(x, np.zeros(1), t, np.zeros(1))[0]
    assert np.isfinite(terms).all() and abs(terms[0, 0] - (800.0 + np.log(4.0))) <= 1e-9


# ---------------------------------------------------------------------------------------------- the motivation, pinned
def test_cross_entropy_learns_the_target_and_the_reference_form_a_one_hot():
    """fp64 gradient descent on the logits of one fixed soft row (_policy_loss.MOTIVATION_ROW): under the cross-entropy the policy
    converges to the target itself; under the reference's form to the one-hot at the target's maximum, whatever the rest of the row
    says -- why better-shaped targets cannot be learned through it."""
    t = PL.MOTIVATION_ROW
    assert abs(t.sum() - 1.0) < 1e-12 and np.sort(t)[-1] - np.sort(t)[-2] >= (np.e - 1) / (PL.MOTIVATION_A - 1 + np.e)
    p = PL.descend(PL.CE, lr=1.0, steps=3000)
    assert np.abs(p - t).max() <= 1e-9, np.abs(p - t).max()
    q = PL.descend(PL.REFERENCE, lr=200.0, steps=20000)
    assert int(q.argmax()) == int(t.argmax()) and q.max() >= 0.9999, q
    assert np.abs(q - t).max() >= 0.59                                         # nowhere near the target


# ---------------------------------------------------------------------------------------------- controls and flags
def test_check_loss_controls():
    assert check_loss_controls("reference", 1.0) == (0, 1.0)
    assert check_loss_controls("cross_entropy", 0.25) == (1, 0.25)
    assert check_loss_controls("cross_entropy", 0) == (1, 0.0)
    for bad in (("cross-entropy", 1.0), ("kl", 1.0), (2, 1.0), (None, 1.0), ("reference", -1.0), ("reference", float("nan")),
                ("reference", float("inf")), ("reference", "much")):
        with pytest.raises(ValueError):
            check_loss_controls(*bad)


def test_train_cycle_flags(monkeypatch, capsys):
    from alphaquoridorgnn_amd import train_cycle_options as tco, train_network as tn
    for k in ("TRAIN_POLICY_LOSS", "TRAIN_VALUE_LOSS_WEIGHT"):
        monkeypatch.setattr(tn, k, getattr(tn, k))
    assert (tn.TRAIN_POLICY_LOSS, tn.TRAIN_VALUE_LOSS_WEIGHT) == ("reference", 1.0)
    tco._set_loss_options(tco._parser().parse_args([]))
    assert (tn.TRAIN_POLICY_LOSS, tn.TRAIN_VALUE_LOSS_WEIGHT) == ("reference", 1.0)          # a default parse leaves both alone
    assert tn._configured_loss() == dict(policy_loss="reference", value_loss_weight=1.0)
    tco._set_loss_options(tco._parser().parse_args(["--policy-loss", "cross-entropy", "--value-loss-weight", "0.25"]))
    assert (tn.TRAIN_POLICY_LOSS, tn.TRAIN_VALUE_LOSS_WEIGHT) == ("cross_entropy", 0.25)
    assert tn._configured_loss() == dict(policy_loss="cross_entropy", value_loss_weight=0.25)
    tco._set_loss_options(tco._parser().parse_args(["--policy-loss", "reference"]))
    assert (tn.TRAIN_POLICY_LOSS, tn.TRAIN_VALUE_LOSS_WEIGHT) == ("reference", 0.25)
    for bad in (["--policy-loss", "kl"], ["--policy-loss", "cross_entropy"], ["--value-loss-weight", "-1"],
                ["--value-loss-weight", "nan"], ["--value-loss-weight", "inf"], ["--value-loss-weight", "much"]):
        with pytest.raises(SystemExit):                                                      # refused at parse time
            tco._parser().parse_args(bad)
    capsys.readouterr()


def test_apply_args_sets_the_loss_form(monkeypatch):
    """Through the command line's own path: check_args, then apply_args onto the module constants."""
    from alphaquoridorgnn_amd import train_cycle_options as tco, train_network as tn
    for k in ("TRAIN_POLICY_LOSS", "TRAIN_VALUE_LOSS_WEIGHT"):
        monkeypatch.setattr(tn, k, getattr(tn, k))
    args = tco._parser().parse_args(["--policy-loss", "cross-entropy", "--value-loss-weight", "0.5"])
    tco.check_args(args)
    tco.apply_args(args)
    assert (tn.TRAIN_POLICY_LOSS, tn.TRAIN_VALUE_LOSS_WEIGHT) == ("cross_entropy", 0.5)


def test_progress_line_and_validation_follow_the_option():
    """The progress line names the cross-entropy; the Val Loss column and the keep-best score are the table's ce and ce + w mse under
    it, and what they always were with the option off (a trainer that does not know the option included)."""
    from alphaquoridorgnn_amd import train_network as tn
    from alphaquoridorgnn_amd.validation import Metrics
    import torch

    class Tr:
        max_grad_norm, grad_norms = None, torch.zeros((0,))

    sums = np.zeros((2, 4))
    sums[0] = (30.0, 10.0, 50.0, 4.0)                     # ce, ent, lp, se over 10 rows
    counts = np.zeros((2, 4), dtype=np.int64)
    counts[0] = (10, 5, 8, 6)
    m = Metrics(sums, counts, 8, 1)
    off = Tr()
    assert tn._validation_loss(m, off) == (5.0, 5.0 + 0.4)
    assert tn._validation_loss(m, None) == (5.0, 5.0 + 0.4)
    line = tn._progress_line(0, 1.0, 2.0, off, m)
    assert "| Policy Loss: 1.0000 |" in line and "Val Loss: 5.0000 / 0.4000" in line and "(CE)" not in line
    on = Tr()
    on.policy_loss, on.value_loss_weight = "cross_entropy", 0.25
    assert tn._validation_loss(m, on) == (3.0, 3.0 + 0.25 * 0.4)
    line = tn._progress_line(0, 1.0, 2.0, on, m)
    assert "| Policy Loss (CE): 1.0000 |" in line and "Val Loss: 3.0000 / 0.4000" in line
    weighted = Tr()
    weighted.policy_loss, weighted.value_loss_weight = "reference", 2.0
    assert tn._validation_loss(m, weighted) == (5.0, 5.0 + 2.0 * 0.4)


# ---------------------------------------------------------------------------------------------- the C ABI on the host
def test_loss_layout_matches_header(tmp_path):
    from alphaquoridorgnn_amd import _lib
    fields = ["policy_form", "value_weight"]
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "aqgnn.h"\nint main() { std::printf("%zu'
                   + " %zu" * len(fields) + '\\n", sizeof(aqg_loss)' + "".join(f", offsetof(aqg_loss, {f})" for f in fields)
                   + "); }\n")
    exe = tmp_path / "layout"
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    T = _lib.LossStruct
    assert got == [ctypes.sizeof(T)] + [getattr(T, f).offset for f in fields] == [8, 0, 4]


def test_entry_points_are_declared_and_exported():
    """The six _loss entry points and the stand-alone call: in the header, in the binding's signatures (one more pointer than the
    _avg form, in front of the stream) and in the built library; the ABI number is what it was."""
    from alphaquoridorgnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} missing: build first")
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "aqgnn.h")).read()
    stems = ["aqg_gcn_train_step", "aqg_gcn_train_steps", "aqg_gcn_train_step_general", "aqg_gcn_train_steps_general",
             "aqg_cnn_train_step", "aqg_cnn_train_steps"]
    for stem in stems:
        avg, loss = _lib.SIGNATURES[stem + "_avg"], _lib.SIGNATURES[stem + "_loss"]
        assert loss[0] is avg[0] and len(loss[1]) == len(avg[1]) + 1
        assert loss[1][:-2] == avg[1][:-1] and loss[1][-1] is avg[1][-1], stem
        assert loss[1][-2]._type_ is _lib.LossStruct, stem
        assert f"int {stem}_loss(" in header and hasattr(lib, stem + "_loss"), stem
    assert "int aqg_policy_value_loss(" in header and hasattr(lib, "aqg_policy_value_loss")
    assert lib.aqg_abi_version() == 15
