"""The training modules' surface without a GPU or the library: every name that could be imported from train_network and train_cycle
when each was one file still can be, a name that moved is one object in both places, the numpy statements import without torch, and
the drop-in shim shows what the module shows."""
import importlib
import importlib.util
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

PKG = "alphaquoridorgnn_amd."

# what was defined in alphaquoridorgnn_amd.train_network when it was one module, private names included: tests and tools use them
TRAIN_NETWORK_NAMES = """
    BATCH_SIZE BOARD_SIZE CNNTrainer CNN_TRAINING_NOT_BUILT GNNTrainer GeneralTrainer HIDDEN_DIM LEARNING_RATE NUM_EPOCH NUM_FEATURES
    PV_NETWORK_PATH STATE_DICT_KEYS TRAIN_DECOUPLED TRAIN_EMA_DECAY TRAIN_EMA_EVERY TRAIN_EPOCH_ROWS TRAIN_GENERATIONS
    TRAIN_HOLDOUT_EVERY TRAIN_HOLDOUT_KEEP_BEST TRAIN_HOLDOUT_LOG TRAIN_HOLDOUT_SEED TRAIN_HOLDOUT_SHARE TRAIN_MAX_GRAD_NORM
    TRAIN_MERGE_POSITIONS TRAIN_MIRROR TRAIN_MIRROR_SEED TRAIN_SURPRISE_MAX_COPIES TRAIN_SURPRISE_SEED TRAIN_SURPRISE_UNIFORM_SHARE
    TRAIN_SURPRISE_WEIGHTING TRAIN_WEIGHT_DECAY TRAIN_WINDOW WeightAverage _Holdout _Trainer _augment_launch _checked_average_controls
    _configured_controls _epoch_order _finite_or_none _held_out_rows _merged_and_drawn _mirror_arguments _progress_line _recorded_rows
    _surprise_rows _surprise_updates _train _train_loop _training_rows _update_rows adam_reference augment_gather clip_coefficient
    default_decay_mask draw_mirror_flips grad_norm load_data lr_lambda train_cnn_network train_network trainer_for weight_average_due
    weight_average_reference weight_average_table""".split()

# what the tests and tools reach for as train_cycle.<name>
TRAIN_CYCLE_NAMES = """
    NUM_TRAIN_CYCLE _STAGES main parameter_update self_play train_cycle train_network _parser
    _check_average_args _check_holdout_args _check_policy_args _check_reanalyse_args _check_reanalyse_policy_args _check_start_args
    _check_surprise_args _check_value_lambda_args _set_average_options _set_optimiser_options _set_policy_options
    _set_reanalyse_options _set_replay_options _set_resign_options _set_target_options""".split()

# where a name lives now, and from where it is imported back
MOVED = {
    "train_reference": ("train_network", """clip_coefficient adam_reference weight_average_reference weight_average_due
                                            check_average_controls _checked_average_controls LEARNING_RATE""".split()),
    "train_augment": ("train_network", "draw_mirror_flips _mirror_arguments _augment_launch augment_gather".split()),
    "trainers": ("train_network", "BATCH_SIZE default_decay_mask grad_norm _Trainer GNNTrainer GeneralTrainer CNNTrainer".split()),
    "weight_average": ("train_network", "weight_average_table WeightAverage".split()),
    "train_cycle_options": ("train_cycle", [n for n in TRAIN_CYCLE_NAMES if n.startswith(("_parser", "_check_", "_set_"))]
                            + ["_set_mirror_options", "_set_tree_reuse_options", "_set_start_options", "_set_surprise_options",
                               "_set_holdout_options", "check_args", "apply_args"]),
}


def test_the_name_lists_are_whole():
    assert len(TRAIN_NETWORK_NAMES) == len(set(TRAIN_NETWORK_NAMES)) == 65
    assert sum(n.startswith(("_check_", "_set_")) for n in TRAIN_CYCLE_NAMES) == 15


@pytest.mark.parametrize("name", TRAIN_NETWORK_NAMES)
def test_name_is_importable_from_train_network(name):
    assert hasattr(importlib.import_module(PKG + "train_network"), name)


@pytest.mark.parametrize("name", TRAIN_CYCLE_NAMES)
def test_name_is_importable_from_train_cycle(name):
    assert hasattr(importlib.import_module(PKG + "train_cycle"), name)


@pytest.mark.parametrize("home", sorted(MOVED))
def test_a_moved_name_is_one_object(home):
    surface, names = MOVED[home]
    there, here = importlib.import_module(PKG + home), importlib.import_module(PKG + surface)
    for name in names:
        assert getattr(here, name) is getattr(there, name), name
    # a class or function says where it lives
    assert all(getattr(there, n).__module__ == PKG + home for n in names if hasattr(getattr(there, n), "__module__"))


def test_the_old_name_of_the_average_check_is_an_alias():
    tn = importlib.import_module(PKG + "train_network")
    assert tn._checked_average_controls is tn.check_average_controls
    assert tn.check_average_controls(0.5, 2) == (0.5, 2)
    for bad in ((1.0, 1), (float("nan"), 1), (0.5, 0), (0.5, True), (0.5, 1.5), ("x", 1)):
        with pytest.raises(ValueError, match="weight average"):
            tn.check_average_controls(*bad)


def test_train_reference_imports_without_torch():
    code = ("import sys; import alphaquoridorgnn_amd.train_reference as r; "
            "bad = [m for m in ('torch', 'alphaquoridorgnn_amd._lib') if m in sys.modules]; "
            "assert not bad, bad; assert r.weight_average_due(4, 2) and float(r.clip_coefficient(4.0, 1.0)) < 0.25; print('ok')")
    run = subprocess.run([sys.executable, "-c", code], cwd=REPO, capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stderr


@pytest.mark.parametrize("module", ["train_network", "train_cycle"])
def test_dropin_shim_shows_what_the_module_shows(module):
    """The shim's file is loaded under a private name: `import train_network` itself is left to whoever puts the directory on the path."""
    impl = importlib.import_module(PKG + module)
    spec = importlib.util.spec_from_file_location("_dropin_" + module, os.path.join(REPO, "alphaquoridorgnn_amd", "dropin", module + ".py"))
    shim = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(shim)
    public = [k for k in vars(impl) if not k.startswith("_")]
    assert public and all(getattr(shim, k) is getattr(impl, k) for k in public)
    listed = TRAIN_NETWORK_NAMES if module == "train_network" else TRAIN_CYCLE_NAMES
    assert all(getattr(shim, k) is getattr(impl, k) for k in listed)
