"""Held-out validation in the loop, on the GPU: validation.row_metrics end to end for every network kind against the numpy statements
fed the same forward_states outputs; its policy_loss and value_mse against the trainers' own losses; the network a validation sees is
the one the trainer just updated; train_network() / train_cnn_network() with the option unset and set, byte for byte against the
plain loop and against the option off on the host-built training index; keep-best; two data-parallel ranks; the log."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests._row_metrics import ULP_DEVICE, ULP_HOST, U, bars, policy_size, reduce_depth  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from alphaquoridorgnn_amd import _lib
    _lib.load()
    return _lib.require_gpu()


@pytest.fixture(scope="module")
def played(dev):
    """Two seeded 5x5 self-play generations in a window on the GPU, shared by the tests below and left unchanged."""
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    from alphaquoridorgnn_amd.replay import ReplayWindow
    w = ReplayWindow(5, max_generations=2, device=dev)
    for g in range(2):
        eng = BatchedSelfPlay(None, num_games=8, sims=8, board_size=5, evaluator="fake", fake_bias=0, seed=70 + g)
        eng.play_generation()
        w.append_counts(*eng.history_tensors())
    return w


def _network(kind, N, dev):
    from alphaquoridorgnn_amd.pv_network_cnn import CNNNetwork
    from alphaquoridorgnn_amd.pv_network_gnn import GraphPolicyValueNetwork
    torch.manual_seed(40 + N)
    if kind == "cnn":
        net = CNNNetwork(4, 1, board_size=N)
        with torch.no_grad():
            for mod in net.modules():
                if isinstance(mod, torch.nn.BatchNorm2d):
                    mod.running_mean.uniform_(-0.3, 0.3)
                    mod.running_var.uniform_(0.5, 2.0)
        return net.to(dev)
    return GraphPolicyValueNetwork(6, kind[0], kind[1], policy_size(N), board_size=N).to(dev)


@pytest.mark.parametrize("kind", [(128, 3), (64, 2), "cnn"], ids=["6-128-3", "6-64-2", "cnn-4x1"])
def test_row_metrics_end_to_end(dev, played, kind):
    """On the rows of the self-play generations: counts and the se column bit for bit, the other sums within the rows' bars added up
    per bucket (plus the reduction's own rounding), no row rejected; in chunks of 16 rows the same bits; the module's mode, parameters
    and running statistics as they were."""
    from alphaquoridorgnn_amd.replay import row_metrics_reduce_reference, row_metrics_reference
    w, m = played, len(played)
    assert m > 40
    model = _network(kind, 5, dev).train()
    state = {name: x.detach().clone() for name, x in model.state_dict().items()}
    got = w.row_metrics(model)
    assert model.training and all(torch.equal(x, state[name]) for name, x in model.state_dict().items())
    assert got.rejected == 0 and got.rows == m
    s72, pi, z = w.tensors()
    slots = w.index()
    model.eval()
    with torch.no_grad():
        net, v = model.forward_states(s72.index_select(0, slots).contiguous())
    h72, h_pi, h_z, h_slots = s72.cpu().numpy(), pi.cpu().numpy(), z.cpu().numpy(), slots.cpu().numpy()
    net, v = net.cpu().numpy(), v[:, 0].contiguous().cpu().numpy()
    vals, tag = row_metrics_reference(h72, h_pi, h_z, net, v, h_slots)
    sums, counts = row_metrics_reduce_reference(vals, tag)
    assert np.array_equal(got.counts, counts) and got.sums[:, 3].tobytes() == sums[:, 3].tobytes()
    bucket = tag & 255
    for col, bar in enumerate(bars(h_pi[h_slots], net, ULP_DEVICE, ULP_HOST)):
        per_bucket, mass = np.zeros(17), np.zeros(17)
        np.add.at(per_bucket, bucket, bar)
        np.add.at(mass, bucket, np.abs(vals[:, col]))
        print(f"{kind} column {col}: max |sum - reference| = {np.abs(got.sums[:, col] - sums[:, col]).max():.3e}")
        assert np.all(np.abs(got.sums[:, col] - sums[:, col]) <= per_bucket + reduce_depth(m) * U * mass)
    assert got.policy_ce > got.target_entropy > 0 and got.kl > 0 and 0 <= got.top1 <= 1 and got.policy_loss > 0 and got.value_mse > 0
    assert (counts[:16, 0] > 0).sum() >= 2 and len(got.table().splitlines()) >= 4
    chunked = w.row_metrics(model, chunk_rows=16)
    assert chunked.sums.tobytes() == got.sums.tobytes() and np.array_equal(chunked.counts, got.counts) and not model.training
    some = slots[torch.arange(0, m, 3, device=dev)]
    part = w.row_metrics(model, some, bucket_plies=4, buckets=3)
    assert part.rows == some.numel() and part.sums.shape == (4, 4) and part.rejected == 0
    empty = w.row_metrics(model, slots[:0])
    assert empty.rows == 0 and not empty.sums.any() and not empty.counts.any()
    with pytest.raises(ValueError):
        w.row_metrics(model, buckets=65)


@pytest.mark.parametrize("shape", [(128, 3), (16, 2)], ids=["fused", "general"])
def test_policy_loss_and_value_mse_are_the_trainers(dev, played, shape):
    """row_metrics' policy_loss and value_mse on a batch of at most 128 rows against trainer.step(update=False) on the same rows, for GNNTrainer
    and GeneralTrainer -- at the tolerance tests/test_train_general.py::_check_step holds the trainers' losses to their fp64 statement:
    1e-5 relative on the policy loss, 1e-5 relative + 1e-7 on the value loss."""
    from alphaquoridorgnn_amd.train_network import trainer_for
    from alphaquoridorgnn_amd.validation import row_metrics
    model = _network(shape, 5, dev)
    s72, pi, z = (x[:128].contiguous() for x in played.rows())
    assert 40 < s72.shape[0] <= 128
    trainer = trainer_for(model, max_batch=128)
    assert type(trainer).__name__ == ("GNNTrainer" if shape == (128, 3) else "GeneralTrainer")
    pl, vl = trainer.step(s72, pi, z, update=False)
    got = row_metrics(model, s72, pi, z)
    print(f"{shape}: policy loss {float(pl):.8f} / {got.policy_loss:.8f}, value loss {float(vl):.8f} / {got.value_mse:.8f}")
    assert abs(got.policy_loss - float(pl)) <= 1e-5 * abs(float(pl))
    assert abs(got.value_mse - float(vl)) <= 1e-5 * abs(float(vl)) + 1e-7


def _trainer(kind, model):
    from alphaquoridorgnn_amd import train_network as tn
    return tn.CNNTrainer(model, max_batch=32) if kind == "cnn" else tn.trainer_for(model, max_batch=32)


@pytest.mark.parametrize("kind", [(128, 3), (16, 2), "cnn"], ids=["fused", "general", "cnn"])
def test_validation_sees_the_trainers_update(dev, played, kind, tmp_path):
    """forward_states sees the in-place update: the validation after three steps, and after one epoch more, equals the validation of a
    freshly loaded copy of the saved state_dict, bit for bit -- and differs from the validation before the steps."""
    from alphaquoridorgnn_amd.validation import row_metrics
    model = _network(kind, 5, dev)
    trainer = _trainer(kind, model)
    s72, pi, z = (x.contiguous() for x in played.rows())
    held = torch.arange(0, s72.shape[0], 4, device=dev)
    before = row_metrics(model, s72, pi, z, held)
    assert s72.shape[0] >= 48
    for i in range(3):
        trainer.step(s72[16 * i:16 * i + 16], pi[16 * i:16 * i + 16], z[16 * i:16 * i + 16])
    for stage in ("steps", "epoch"):
        if stage == "epoch":
            trainer.run_epoch(s72, pi, z, torch.arange(48, device=dev))
        after = row_metrics(model, s72, pi, z, held)
        torch.save(model.state_dict(), tmp_path / "saved.pth")
        copy = _network(kind, 5, dev)                               # (load_network would take the process's board size)
        copy.load_state_dict(torch.load(tmp_path / "saved.pth", map_location=dev, weights_only=True))
        fresh = row_metrics(copy.eval(), s72, pi, z, held)
        assert after.sums.tobytes() == fresh.sums.tobytes() and np.array_equal(after.counts, fresh.counts), stage
        assert after.sums.tobytes() != before.sums.tobytes()
        before = after


# ------------------------------------------------------------------ the loop end to end
_LOOP = r'''
import json, os, pickle, sys
sys.path.insert(0, os.environ["AQG_REPO"])
import numpy as np
import torch
from alphaquoridorgnn_amd import constants, distributed as aqd, train_network as tn
from alphaquoridorgnn_amd.pv_network_cnn import CNNNetwork, load_network as load_cnn
from alphaquoridorgnn_amd.pv_network_gnn import GraphPolicyValueNetwork, load_network, pack_states
from alphaquoridorgnn_amd.replay import KEY_BYTES, ReplayWindow, holdout_split_reference
from alphaquoridorgnn_amd.validation import row_metrics

g = np.load(os.path.join(os.environ["AQG_REPO"], "tests", "golden", "cnn_train_5x5.npz"))
rows = [[[[int(s[0]), int(s[1])], [int(s[2]), int(s[3])], [int(x) for x in s[4:20]]], p.tolist(), int(z)]
        for s, p, z in zip(g["states"], g["pi"], g["z"])]
_, first = np.unique(pack_states([r[0] for r in rows], 5)[:, KEY_BYTES], axis=0, return_index=True)
rows = [rows[i] for i in sorted(first)]                       # the golden rows repeat positions: each one once
assert len(rows) == 25 and constants.BOARD_SIZE == 5
older = [[s, [0.25 * x + 0.75 / 57 for x in p], -z] for s, p, z in rows[:15]]      # the first 15 positions again, other targets
os.makedirs("data")
with open("data/20260101000001.history", "wb") as f:
    pickle.dump(rows, f)
os.makedirs(constants.PV_NETWORK_PATH)
BEST, LATEST = constants.PV_NETWORK_PATH + "best.pth", constants.PV_NETWORK_PATH + "latest.pth"
SEED = 4
tn.NUM_EPOCH, tn.TRAIN_HOLDOUT_SEED = 3, SEED
dev = aqd.device()
train, load, make = tn.train_network, load_network, tn.trainer_for
orders = []
plain_epoch = tn._Trainer.run_epoch


def recording_epoch(self, s, p, v, order, **kw):
    orders.append(order.cpu().numpy().copy())
    return plain_epoch(self, s, p, v, order, **kw)


tn._Trainer.run_epoch = recording_epoch


def run():
    torch.manual_seed(11)               # the epochs' shuffles
    del orders[:]
    train()
    with open(LATEST, "rb") as f:
        return f.read()


def window(histories, generations=2):
    w = ReplayWindow(5, max_generations=generations, device=dev)
    for h in histories:
        w.append_history(h)
    return w


def on_the_index(w, index):
    """The hold-out off on a window whose index() is `index`."""
    keep, w._index = w._index, torch.from_numpy(index).to(dev)
    share, tn.TRAIN_HOLDOUT_SHARE, w.surprise_updates = tn.TRAIN_HOLDOUT_SHARE, None, 0
    try:
        return run()
    finally:
        w._index, tn.TRAIN_HOLDOUT_SHARE = keep, share


def hand_loop(w, index, held=None, ema=None):
    """The loop by hand on the trainer's own surface: (bytes of the last iterate's file, [(score, state)] per epoch)."""
    torch.manual_seed(11)
    model = load(BEST, dev)
    s, p, v = w.tensors()
    index = torch.from_numpy(index).to(dev)
    trainer = make(model, max_batch=tn.BATCH_SIZE)
    average = None if ema is None else tn.WeightAverage(trainer, decay=ema, every=1)
    twin = None if ema is None else load(BEST, dev)
    curve = []
    for epoch in range(tn.NUM_EPOCH):
        perm = torch.randperm(index.shape[0], device=dev)
        trainer.run_epoch(s, p, v, index[perm], lr=tn.LEARNING_RATE * tn.lr_lambda(epoch))
        if held is not None:
            target = model
            if average is not None:
                average.copy_to(twin)
                target = twin
            metrics = row_metrics(target, s, p, v, torch.from_numpy(held).to(dev))
            state = model.state_dict() if average is None else average.state_dict()
            curve.append((metrics.policy_loss + metrics.value_mse, {k: x.detach().clone() for k, x in state.items()}, metrics))
    os.makedirs("hand", exist_ok=True)                              # (the archive holds the file's name: the same name elsewhere)
    torch.save(model.state_dict() if average is None else average.state_dict(), "hand/latest.pth")
    with open("hand/latest.pth", "rb") as f:
        return f.read(), curve


def same_state(path, state):
    got = torch.load(path, map_location=dev, weights_only=True)
    return list(got) == list(state) and all(torch.equal(got[k], state[k]) for k in state)


def suite(tag):
    two = window([older, rows])
    tn.TRAIN_WINDOW = two
    h72, h_index = two.tensors()[0].cpu().numpy(), two.index().cpu().numpy()
    want_train, want_held = holdout_split_reference(h72, h_index, 0.25, SEED)
    off = run()
    whole = len(orders) == 3 and all(len(o) == 40 for o in orders)
    print(tag, "UNSET_IS_THE_PLAIN_LOOP", off == hand_loop(two, h_index)[0], whole)
    tn.TRAIN_HOLDOUT_SHARE = 0.25
    on = run()
    seen = set(np.concatenate(orders).tolist())
    print(tag, "SPLIT_IS_THE_HOST_INDEX", on == on_the_index(two, want_train), on != off, seen == set(want_train.tolist()),
          not seen & set(want_held.tolist()), 0 < len(want_held) < 40)
    tn.TRAIN_MERGE_POSITIONS = True
    merged = run()
    print(tag, "BEHIND_THE_MERGE", merged == on_the_index(two, want_train), merged != on)
    tn.TRAIN_MERGE_POSITIONS, tn.TRAIN_SURPRISE_WEIGHTING, tn.TRAIN_MIRROR, two.surprise_updates = False, True, True, 0
    drawn = run()
    seen = set(np.concatenate(orders).tolist())
    print(tag, "SURPRISE_AND_MIRROR", drawn == on_the_index(two, want_train), drawn != on, not seen & set(want_held.tolist()))
    tn.TRAIN_SURPRISE_WEIGHTING, tn.TRAIN_MIRROR = False, False
    # keep best: the snapshot of the first minimum of a hand-run loop's own validated curve; with a weight average, the average's
    tn.NUM_EPOCH, tn.TRAIN_HOLDOUT_KEEP_BEST = 5, True
    for ema in (None, 0.5):
        tn.TRAIN_EMA_DECAY = ema
        run()
        _, curve = hand_loop(two, want_train, want_held, ema)
        best = min(range(5), key=lambda e: (curve[e][0], e))
        print(tag, "KEEP_BEST", "EMA" if ema else "LAST", same_state(LATEST, curve[best][1]), best)
    tn.NUM_EPOCH, tn.TRAIN_HOLDOUT_KEEP_BEST, tn.TRAIN_EMA_DECAY, tn.TRAIN_HOLDOUT_SHARE = 3, False, None, None
    return two, want_train, want_held


# ---- a 6/16/2 network (GeneralTrainer) and the default 6/128/3 (GNNTrainer)
torch.manual_seed(3)
torch.save(GraphPolicyValueNetwork(6, 16, 2, 57, board_size=5).state_dict(), BEST)
two, want_train, want_held = suite("GENERAL")
# the log and the printed lines of one update
tn.TRAIN_HOLDOUT_SHARE, tn.TRAIN_HOLDOUT_EVERY, tn.TRAIN_HOLDOUT_LOG = 0.25, 2, "val.jsonl"
print("LOGGED RUN")
run()
print("")
_, curve = hand_loop(two, want_train, want_held)
record = json.loads(open("val.jsonl").read().splitlines()[-1])
print("LOG", [c["epoch"] for c in record["curve"]] == [2, 3], record["saved_epoch"] == 3,
      record["curve"][1]["policy_loss"] == curve[2][2].policy_loss, record["curve"][0]["value_mse"] == curve[1][2].value_mse,
      record["split"]["held"] == len(want_held), record["split"]["train"] == len(want_train), record["table"]["sums"] == curve[2][2].sums.tolist())
print("LOGLINE", json.dumps(record["curve"][-1]))
tn.TRAIN_HOLDOUT_SHARE, tn.TRAIN_HOLDOUT_EVERY, tn.TRAIN_HOLDOUT_LOG = None, 1, None
# the file route: no window
tn.TRAIN_WINDOW = None
file_off = run()
one = window([rows], 1)
tn.TRAIN_HOLDOUT_SHARE = 0.25
file_on = run()
tn.TRAIN_WINDOW = one
file_train, file_held = holdout_split_reference(one.tensors()[0].cpu().numpy(), one.index().cpu().numpy(), 0.25, SEED)
print("FILE_ROUTE", file_on == on_the_index(one, file_train), file_on != file_off, 0 < len(file_held) < 25)
tn.TRAIN_HOLDOUT_SHARE = None
torch.manual_seed(4)
torch.save(GraphPolicyValueNetwork(6, 128, 3, 57, board_size=5).state_dict(), BEST)
suite("FUSED")
# ---- the residual CNN
torch.manual_seed(5)
torch.save(CNNNetwork(4, 1, board_size=5).state_dict(), BEST)
train, load = tn.train_cnn_network, load_cnn
make = lambda model, max_batch: tn.CNNTrainer(model, max_batch=max_batch)
suite("CNN")
'''


def test_the_loop_with_a_held_out_set(dev, tmp_path):
    """One child process on the 5x5 board, a window of two generations (40 rows, 25 positions).  With every option unset latest.pth is,
    byte for byte, the file of the plain loop run by hand on the trainer's own surface; with share 0.25 it is, byte for byte, the file
    of the option off on a window whose index() is the host-built training index -- also behind the merge, under surprise weighting
    and the mirror, on the file route, and for all three trainers; no held-out slot appears in any epoch's order; with
    TRAIN_HOLDOUT_KEEP_BEST latest.pth is the snapshot a hand-run loop takes at the first minimum of its own validated curve, the
    average's with a weight average; the log line parses and holds the printed numbers."""
    import re
    (tmp_path / "loop.py").write_text(_LOOP)
    env = dict(os.environ, AQG_REPO=REPO, AQG_BOARD_SIZE="5")
    r = subprocess.run([sys.executable, str(tmp_path / "loop.py")], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    shown = [x for x in r.stdout.replace("\r", "\n").splitlines() if x[:1].isupper() and "Epoch" not in x]
    want = [f"{tag} {line}" for tag in ("GENERAL", "FUSED", "CNN")
            for line in ("UNSET_IS_THE_PLAIN_LOOP True True", "SPLIT_IS_THE_HOST_INDEX True True True True True",
                         "BEHIND_THE_MERGE True True", "SURPRISE_AND_MIRROR True True True")]
    for line in want + ["FILE_ROUTE True True True", "LOG True True True True True True True"]:
        assert line in r.stdout, (line, shown)
    kept = re.findall(r"^(\w+) KEEP_BEST (\w+) (\w+) (\d)$", r.stdout, flags=re.M)
    assert len(kept) == 6 and all(k[2] == "True" for k in kept), shown
    assert "held out: " in r.stdout and " distinct positions)" in r.stdout and "kept epoch " in r.stdout
    # the logged run's printed lines hold the log's numbers
    logged = r.stdout.split("LOGGED RUN", 1)[1].replace("\r", "\n")
    last = json.loads(re.search(r"^LOGLINE (.*)$", logged, flags=re.M).group(1))
    epochs = [x for x in logged.splitlines() if x.startswith("Epoch")][:3]
    assert ["Val Loss" in x for x in epochs] == [False, True, True]
    assert (f"| Val Loss: {last['policy_loss']:.4f} / {last['value_mse']:.4f} | Val KL: {last['kl']:.4f} | Top-1: {last['top1']:.3f}"
            in epochs[2])
    assert re.search(r"^ +all +\d+ ", logged, flags=re.M)              # the per-ply table behind the epochs


_RANKS = r'''
import os, sys
sys.path.insert(0, os.environ["AQG_REPO"])
import numpy as np, torch, torch.distributed as dist
from alphaquoridorgnn_amd import constants, train_network as tn
rank = int(os.environ["RANK"])
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:" + os.environ["AQG_PORT"], rank=rank, world_size=2)
tn.NUM_EPOCH, tn.TRAIN_HOLDOUT_SHARE, tn.TRAIN_HOLDOUT_SEED, tn.TRAIN_HOLDOUT_LOG, tn.TRAIN_HOLDOUT_KEEP_BEST = 3, 0.25, 4, "val.jsonl", True
seen = []
validate = tn._Holdout.validate


def recording(self, epoch):
    out = validate(self, epoch)
    seen.append(np.concatenate([out.sums.ravel(), out.counts.ravel().astype(np.float64)]))
    return out


tn._Holdout.validate = recording
torch.manual_seed(11 + rank)            # the shuffle is rank 0's: it is broadcast
tn.train_network()
np.save(f"curve.{rank}.npy", np.stack(seen))
dist.destroy_process_group()
'''


def test_two_ranks_validate_alike(dev, tmp_path):
    """AQG_TRAIN_DATA_PARALLEL=1 on two gloo ranks sharing this GPU: both keep the same validation curve, bit for bit, with no
    collective of its own; rank 0 alone prints, writes latest.pth and appends one line to the log."""
    import pickle
    from alphaquoridorgnn_amd.pv_network_gnn import GraphPolicyValueNetwork
    g = np.load(os.path.join(REPO, "tests", "golden", "cnn_train_5x5.npz"))
    rows = [[[[int(s[0]), int(s[1])], [int(s[2]), int(s[3])], [int(x) for x in s[4:20]]], p.tolist(), int(z)]
            for s, p, z in zip(g["states"], g["pi"], g["z"])]
    os.makedirs(tmp_path / "data")
    with open(tmp_path / "data" / "20260101000001.history", "wb") as f:
        pickle.dump(rows, f)
    from alphaquoridorgnn_amd import constants
    models = tmp_path / "models" / constants.PV_NETWORK_NAME / "5x5"
    os.makedirs(models)
    torch.manual_seed(3)
    torch.save(GraphPolicyValueNetwork(6, 16, 2, 57, board_size=5).state_dict(), models / "best.pth")
    (tmp_path / "worker.py").write_text(_RANKS)
    env = dict(os.environ, AQG_REPO=REPO, AQG_BOARD_SIZE="5", AQG_TRAIN_DATA_PARALLEL="1", AQG_PORT=str(29300 + os.getpid() % 300))
    procs = [subprocess.Popen([sys.executable, str(tmp_path / "worker.py")], cwd=tmp_path, env=dict(env, RANK=str(r)),
                              stdout=subprocess.PIPE, text=True) for r in range(2)]
    outs = [p.communicate(timeout=300)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs)
    curves = [np.load(tmp_path / f"curve.{r}.npy") for r in range(2)]
    assert curves[0].shape[0] == 3 and curves[0].tobytes() == curves[1].tobytes()
    assert "Val Loss" in outs[0] and "held out: " in outs[0] and "kept epoch " in outs[0]
    assert "Val Loss" not in outs[1] and "held out" not in outs[1]
    assert os.path.exists(models / "latest.pth") and len(open(tmp_path / "val.jsonl").read().splitlines()) == 1


def test_command_line_prints_the_table(dev, tmp_path):
    """python -m alphaquoridorgnn_amd.validation NET.pth FILE.history FILE.history on 5x5: the table of a saved 6/16/2 network on the
    rows of both files, every row in bucket 0 (rows read from .history files carry ply 0), no training run."""
    import pickle
    import re
    from alphaquoridorgnn_amd.pv_network_gnn import GraphPolicyValueNetwork
    g = np.load(os.path.join(REPO, "tests", "golden", "cnn_train_5x5.npz"))
    rows = [[[[int(s[0]), int(s[1])], [int(s[2]), int(s[3])], [int(x) for x in s[4:20]]], p.tolist(), int(z)]
            for s, p, z in zip(g["states"], g["pi"], g["z"])]
    for name, part in (("a.history", rows[:25]), ("b.history", rows[25:])):
        with open(tmp_path / name, "wb") as f:
            pickle.dump(part, f)
    torch.manual_seed(3)
    torch.save(GraphPolicyValueNetwork(6, 16, 2, 57, board_size=5).state_dict(), tmp_path / "net.pth")
    env = dict(os.environ, AQG_BOARD_SIZE="5", PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "alphaquoridorgnn_amd.validation", "net.pth", "a.history", "b.history"], cwd=tmp_path, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert f"net.pth: {len(rows)} rows of 2 file(s)" in r.stdout
    assert re.search(r"^ +0-7 +%d " % len(rows), r.stdout, flags=re.M) and re.search(r"^ +all +%d " % len(rows), r.stdout, flags=re.M)
    assert "rejected" not in r.stdout
    bad = subprocess.run([sys.executable, "-m", "alphaquoridorgnn_amd.validation", "net.pth", "a.history", "--buckets", "65"], cwd=tmp_path,
                         env=env, capture_output=True, text=True, timeout=300)
    assert bad.returncode == 2 and "buckets" in bad.stderr
