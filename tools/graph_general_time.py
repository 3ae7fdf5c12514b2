"""Times the width-generic graph primitives (csrc/gcn_general.hip) at 4,096 9x9 board graphs (331,776 nodes) on one GPU: forward,
and forward + backward, of GraphPolicyValueNetwork at a non-default shape (default 6/256/3; SHAPE=F,H,L).  The default 6/128/3
shape runs the same primitives: tools/graph_autograd_time.py times it (profiles/graph_path_unify_ab.log holds its last
comparison with the fixed-width kernels it replaced).
Prints one line per measurement (median of REPS timed calls after WARMUP)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from alphaquoridorgnn_amd import _lib, pv_network_gnn as P   # noqa: E402

B = int(os.environ.get("BOARDS", "4096"))
REPS, WARMUP = int(os.environ.get("REPS", "20")), int(os.environ.get("WARMUP", "3"))


def timed(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def board_batch(dev):
    """B 9x9 board graphs (random wall-heavy records) as device (x, edge_index, batch) via the board featuriser."""
    from tests.test_gpu_parity import _small_board_states
    recs = _small_board_states(9)
    recs = recs[np.random.RandomState(0).randint(0, recs.shape[0], B)]
    st = torch.from_numpy(recs).to(dev)
    lib = _lib.load()
    R = B * 81
    x = torch.empty((R, 6), dtype=torch.float32, device=dev)
    idx = torch.empty((R, 5), dtype=torch.int32, device=dev)
    w = torch.empty((R, 5), dtype=torch.float32, device=dev)
    _lib.check(lib.aqg_gcn_boards_graph(9, _lib.ptr(st), B, _lib.ptr(x), _lib.ptr(idx), _lib.ptr(w), _lib.stream_ptr(dev)), "featuriser")
    dst = torch.arange(R, device=dev).repeat_interleave(5)
    keep = idx.view(-1) >= 0
    ei = torch.stack([idx.view(-1)[keep].long(), dst[keep]])
    ei = ei[:, ei[0] != ei[1]]                              # _prepare_graph adds the self loops back
    batch = torch.arange(B, device=dev).repeat_interleave(81)
    return st, x, ei, batch


def main():
    dev = _lib.require_gpu()
    torch.manual_seed(0)
    st, x, ei, batch = board_batch(dev)
    shape = tuple(int(v) for v in os.environ.get("SHAPE", "6,256,3").split(","))
    print(f"{B} board graphs, {x.shape[0]} nodes, {ei.shape[1]} edges; shape {shape}")
    net = P.GraphPolicyValueNetwork(*shape, 209).to(dev)
    net.eval()
    with torch.no_grad():
        print(f"  non-default forward(x, edge_index, batch)       {timed(lambda: net(x, ei, batch)):8.3f} ms")
        print(f"  non-default forward_states(records)              {timed(lambda: net.forward_states(st)):8.3f} ms")
    net.train()

    def fwd_bwd():
        p, v = net(x, ei, batch)
        (p.sum() + v.sum()).backward()
    print(f"  non-default train forward + backward             {timed(fwd_bwd):8.3f} ms")


if __name__ == "__main__":
    main()
