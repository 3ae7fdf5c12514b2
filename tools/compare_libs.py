"""Bit-identity of two builds of libaqgnn_hip.so on the same inputs (cleanup / refactoring check).

    OUT=/tmp/parent/libaqgnn_hip.so <checkout of the parent commit>/alphaquoridorgnn_amd/csrc/build.sh
    python tools/compare_libs.py /tmp/parent/libaqgnn_hip.so alphaquoridorgnn_amd/libaqgnn_hip.so

Each library runs in its own process (AQG_LIB_PATH): the GNN forward at 300 / 4,096 / 1,001 boards in both guard modes (non-zero GCN
biases), masked engine launches inside 64-game GNN-evaluated generations (history rows; a weight set inside the static fp16 bound and
one outside it: both builds of the evaluation launch), three moves of 640 games with the evaluation cache on for both sets (the
trunk's compact-list builds), three training steps, and then every trainer (GeneralTrainer (6, 32, 2)
and CNNTrainer 8 filters x 1 block on 5x5, GNNTrainer on 9x9 and on 5x5) at max_batch 4 through steps of 4, 4 and 3 positions, a shuffled
epoch of 10, both again with weight decay and clipping on, and a mode-0 then a mode-2 call: parameters, Adam moments, losses, gradient
norms and running statistics.  Prints one line per item; exit code 1 on any difference."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_WORKER = r'''
import sys, os
sys.path.insert(0, sys.argv[1])
import numpy as np, torch
from alphaquoridorgnn_amd import _lib
from alphaquoridorgnn_amd.engine import BatchedSelfPlay
from alphaquoridorgnn_amd.pv_network_cnn import CNNNetwork
from alphaquoridorgnn_amd.pv_network_gnn import GNNNetwork, GraphPolicyValueNetwork
from alphaquoridorgnn_amd.train_network import CNNTrainer, GeneralTrainer, GNNTrainer
from tools.microbench import synth_states
from oracle import gnn as og
dev = torch.device("cuda", 0)
lib = _lib.load()
out = {}
torch.manual_seed(0)
def with_biases(m, scale=1.0):
    # PyG initialises the GCN biases to zero: non-zero ones, so that the trunk's per-degree bias rows matter; `scale` on the trunk's
    # weights takes the set out of the static fp16 bound (the tracking builds serve it)
    sd = m.state_dict()
    for l in range(3):
        sd[f"gcn_layers.{l}.bias"] = torch.linspace(-0.3, 0.5, 128) * (1 + l)
        sd[f"gcn_layers.{l}.lin.weight"] = sd[f"gcn_layers.{l}.lin.weight"] * scale
    m.load_state_dict(sd)
    return m
model = with_biases(GNNNetwork()).to(dev).eval()
pk = model.packed_weights(dev)
for B in (300, 4096, 1001):
    st = synth_states(B, seed=B, dev=dev)
    for flags in (0, 2):
        pooled = torch.zeros((B, 128), device=dev); policy = torch.zeros((B, 209), device=dev); value = torch.zeros((B,), device=dev)
        word = torch.zeros((1,), dtype=torch.int32, device=dev)
        _lib.check(lib.aqg_gcn_forward_boards_guarded(9, _lib.ptr(st), 0, B, _lib.ptr(pk), _lib.ptr(pooled), None, _lib.ptr(policy), None,
                                                      _lib.ptr(value), flags, _lib.ptr(word), _lib.stream_ptr(dev)), "fwd")
        out[f"pooled_{B}_{flags}"] = pooled.cpu().numpy(); out[f"policy_{B}_{flags}"] = policy.cpu().numpy(); out[f"value_{B}_{flags}"] = value.cpu().numpy()
eng = BatchedSelfPlay(model, num_games=64, sims=24, seed=11)
eng.play_generation()
s, v, z = eng.history_tensors()
out["hist_s"], out["hist_v"], out["hist_z"] = s.cpu().numpy(), v.cpu().numpy(), z.cpu().numpy()
# the evaluation launch's tracking build (a 64-game generation of a weight set outside the static bound), and the compact-list builds of
# both guard modes (640 games with the evaluation cache on, three moves)
x3 = with_biases(GNNNetwork(), 3.0).to(dev).eval()
assert model.gnn_flags(dev) == _lib.GNN_RANGE_PROVEN and x3.gnn_flags(dev) == 0
eng = BatchedSelfPlay(x3, num_games=64, sims=24, seed=11)
eng.play_generation()
assert eng.e.gnn_flags == 0
s, v, z = eng.history_tensors()
out["x3_hist_s"], out["x3_hist_v"], out["x3_hist_z"] = s.cpu().numpy(), v.cpu().numpy(), z.cpu().numpy()
for tag, m in (("proven", model), ("x3", x3)):
    eng = BatchedSelfPlay(m, num_games=640, sims=6, seed=5, eval_cache_slots=256)
    for _ in range(3):
        eng.move()
    assert int(eng.t["eval_count"].sum()) > 0 and eng.e.gnn_flags == m.gnn_flags(dev)
    out[f"list_{tag}_pooled"], out[f"list_{tag}_count"] = eng.t["pooled"].cpu().numpy(), eng.t["eval_count"].cpu().numpy()
    s, v, z = eng.history_tensors()
    out[f"list_{tag}_hist_s"], out[f"list_{tag}_hist_v"] = s.cpu().numpy(), v.cpu().numpy()
tm = GNNNetwork()
tm.load_state_dict({k: torch.from_numpy(x.copy()) for k, x in og.init_params(3).items()})
tm = tm.to(dev)
tr = GNNTrainer(tm, max_batch=128)
rng = np.random.RandomState(0)
for i in range(3):
    st = synth_states(128 if i < 2 else 37, seed=50 + i, dev=dev)
    n = st.shape[0]
    pi = torch.softmax(torch.from_numpy(rng.randn(n, 209).astype(np.float32)), 1).to(dev)
    zz = torch.from_numpy(rng.choice([-1.0, 0.0, 1.0], n).astype(np.float32)).to(dev)
    tr.step(st, pi, zz)
for k, t in tm.state_dict().items():
    out["param_" + k] = t.cpu().numpy()
# every trainer at max_batch 4: single steps, an epoch, both again with the controls on, modes 0 and 2
walk5 = torch.from_numpy(np.load(os.path.join(sys.argv[1], "tests", "golden", "walk_5x5.npz"))["states"]).to(dev)
def trainers(controls):
    torch.manual_seed(7)
    yield "general", 5, GeneralTrainer(GraphPolicyValueNetwork(6, 32, 2, 57, board_size=5).to(dev), max_batch=4, **controls)
    yield "cnn", 5, CNNTrainer(CNNNetwork(8, 1, board_size=5).to(dev), max_batch=4, **controls)
    yield "fused9", 9, GNNTrainer(GNNNetwork().to(dev), max_batch=4, **controls)
    yield "fused5", 5, GNNTrainer(GraphPolicyValueNetwork(6, 128, 3, 57, board_size=5).to(dev), max_batch=4, **controls)
def dump(tag, tr):
    for i, tensors in enumerate(zip(tr.params, tr.adam_m, tr.adam_v)):
        for name, t in zip(("param", "adam_m", "adam_v"), tensors):
            out[f"{tag}_{name}{i}"] = t.detach().cpu().numpy()
    for i, t in enumerate(getattr(tr, "buffers", [])):
        out[f"{tag}_running{i}"] = t.cpu().numpy()
    out[tag + "_loss"], out[tag + "_last_norm"], out[tag + "_norms"] = (t.cpu().numpy() for t in (tr.ws["loss"], tr.last_grad_norm, tr.grad_norms))
for ctag, controls in (("plain", {}), ("optim", dict(weight_decay=1e-2, max_grad_norm=0.5))):
    for kind, N, tr in trainers(controls):
        A, tag = N * N + 2 * (N - 1) ** 2, f"{kind}_{ctag}"
        rng = np.random.RandomState(N)
        S = synth_states(10, seed=70, dev=dev) if N == 9 else walk5[::max(1, walk5.shape[0] // 10)][:10].contiguous()
        P = torch.softmax(torch.from_numpy(rng.randn(10, A).astype(np.float32)), 1).to(dev)
        Z = torch.from_numpy(rng.choice([-1.0, 0.0, 1.0], 10).astype(np.float32)).to(dev)
        for lo, hi in ((0, 4), (4, 8), (7, 10)):
            pl, vl = tr.step(S[lo:hi], P[lo:hi], Z[lo:hi])
            out[f"{tag}_step_losses_{lo}"] = torch.stack([pl, vl]).cpu().numpy()
        dump(tag + "_steps", tr)
        out[tag + "_epoch_sums"] = tr.run_epoch(S, P, Z, torch.from_numpy(np.random.RandomState(3).permutation(10))).cpu().numpy()
        dump(tag + "_epoch", tr)
        tr.t.batch, tr.t.step = 4, tr.step_count + 1
        tr._call(S[:4].contiguous(), P[:4].contiguous(), Z[:4].contiguous(), 0)
        out[tag + "_mode0_grads"] = tr.flat_grads.cpu().numpy()
        tr._call(S[:4].contiguous(), P[:4].contiguous(), Z[:4].contiguous(), 2)
        dump(tag + "_modes", tr)
np.savez(sys.argv[2], **out)
'''


def run(libpath, outpath):
    env = dict(os.environ, AQG_LIB_PATH=os.path.abspath(libpath))
    subprocess.run([sys.executable, "-c", _WORKER, ROOT, outpath], check=True, env=env, cwd=ROOT)
    return np.load(outpath)


def main():
    a, b = sys.argv[1:3]
    tmp = os.environ.get("TMPDIR", "/tmp")
    ra, rb = run(a, os.path.join(tmp, "cmp_a.npz")), run(b, os.path.join(tmp, "cmp_b.npz"))
    bad = 0
    for k in ra.files:
        same = np.array_equal(ra[k], rb[k], equal_nan=True)
        d = 0.0 if same else float(np.abs(ra[k].astype(np.float64) - rb[k].astype(np.float64)).max())
        print(f"{k:40s} {'identical' if same else 'DIFFERENT  max |d| = %g' % d}")
        bad += 0 if same else 1
    print("all identical" if not bad else f"{bad} items differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
