"""Times the width-generic graph primitives (csrc/gcn_general.hip) at 4,096 9x9 board graphs (331,776 nodes) on one GPU:
  1. forward, and forward + backward, of GraphPolicyValueNetwork at a non-default shape (default 6/256/3; SHAPE=F,H,L);
  2. at 6/128/3, the same layers composed from the new primitives through the C ABI next to aqg_gcn_forward_graph (the fused
     network's generic path on the VALU graph_linear_kernel), and the two outputs' largest difference.
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

    # 6/128/3: the C ABI primitives against aqg_gcn_forward_graph on the same prepared graph
    lib = _lib.load()
    ref = P.GraphPolicyValueNetwork().to(dev).eval()
    ptr, src, w, gptr, G = P.GraphPolicyValueNetwork._prepare_graph(x, ei, batch)
    pf = [P._param(p, dev) for _, p in ref._ordered_params()]
    n, A = x.shape[0], 209
    f32 = dict(dtype=torch.float32, device=dev)
    w0, w1, pooled = torch.empty((n, 128), **f32), torch.empty((n, 128), **f32), torch.empty((G, 128), **f32)
    logits, policy, vpre, value = torch.empty((G, A), **f32), torch.empty((G, A), **f32), torch.empty((G,), **f32), torch.empty((G,), **f32)
    packed = ref.packed_weights(dev)

    def fused_generic():
        _lib.check(lib.aqg_gcn_forward_graph(6, A, _lib.ptr(x), n, _lib.ptr(ptr), _lib.ptr(src), _lib.ptr(w), _lib.ptr(gptr), G,
                                             _lib.ptr(packed), _lib.ptr(w0), _lib.ptr(w1), _lib.ptr(pooled), _lib.ptr(logits),
                                             _lib.ptr(policy), _lib.ptr(vpre), _lib.ptr(value), _lib.stream_ptr(dev)), "forward_graph")

    def primitives():
        return P._general_forward(lib, dev, ref, x, (ptr, src, w), gptr, G, pf)

    def linears_only():
        h = x
        for l in range(3):
            h = P._linear(lib, dev, h, pf[2 * l])

    print(f"  6/128/3 aqg_gcn_forward_graph (VALU linear)      {timed(fused_generic):8.3f} ms")
    print(f"  6/128/3 gcn_general primitives (MFMA linear)     {timed(primitives):8.3f} ms")
    print(f"  6/128/3 the three MFMA linear maps alone         {timed(linears_only):8.3f} ms")
    fused_generic()
    got = primitives()
    torch.cuda.synchronize()
    print(f"  6/128/3 max |logits diff| {float((got[2] - logits).abs().max()):.3g}, max |value_pre diff| "
          f"{float((got[3] - vpre).abs().max()):.3g}")


if __name__ == "__main__":
    main()
