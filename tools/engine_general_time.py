"""Times the engine's any-shape evaluator (evaluator='general', prior_mode 3) and its fused GCN layer on one GPU (9x9 boards):
  1. per shape (6/64/2, 6/128/3, 6/256/4) and game count (512, 2,048): one network evaluation of all G leaves
     (aqg_gcn_forward_boards_general over 24-byte records), and a self-play move of SIMS simulations -> ms per simulation and
     game-moves/s (games/s = that / plies per game); at 6/128/3 the fused 'gnn' evaluator next to it;
  2. the fused layer against the gen_linear + gen_aggregate composition at 1,024 and 4,096 boards, hidden 64/128/256: the cost
     of one hidden x hidden layer as T(3 layers) - T(2 layers) of each whole forward (median of REPS alternating runs), and the
     weight matrix's L2 traffic (it is re-read by every board tile);
  3. 'external' (model.predict per leaf) against 'general' at 8 games x 16 simulations.
Prints one line per measurement."""
import ctypes
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from alphaquoridorgnn_amd import _lib, pv_network_gnn as P   # noqa: E402
from alphaquoridorgnn_amd.engine import BatchedSelfPlay   # noqa: E402

REPS, WARMUP = int(os.environ.get("REPS", "7")), int(os.environ.get("WARMUP", "2"))
SIMS, MOVES = int(os.environ.get("SIMS", "50")), int(os.environ.get("MOVES", "4"))


def events_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternating(fns):
    """Median ms of each function over REPS rounds in which the functions take turns (after WARMUP rounds)."""
    for _ in range(WARMUP):
        for f in fns:
            f()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(REPS):
        for i, f in enumerate(fns):
            ts[i].append(events_ms(f))
    return [float(np.median(t)) for t in ts]


def records(B, dev):
    from tests.test_gpu_parity import _small_board_states
    recs = _small_board_states(9)
    return torch.from_numpy(recs[np.random.RandomState(0).randint(0, recs.shape[0], B)]).to(dev)


def net_of(shape, dev):
    torch.manual_seed(0)
    return P.GraphPolicyValueNetwork(*shape, 209).to(dev).eval()


def general_forward_fn(net, st, dev, fmt=0):
    lib = _lib.load()
    B, A = st.shape[0], 209
    nws = int(lib.aqg_gcn_boards_general_workspace_floats(9, net.hidden_dim, A, B))
    ws = torch.empty((nws,), dtype=torch.float32, device=dev)
    policy, value = torch.empty((B, A), dtype=torch.float32, device=dev), torch.empty((B,), dtype=torch.float32, device=dev)
    d = net.general_net(dev)

    def run():
        _lib.check(lib.aqg_gcn_forward_boards_general(9, _lib.ptr(st), fmt, B, ctypes.byref(d), None, _lib.ptr(ws), nws, None, None,
                                                      _lib.ptr(policy), None, _lib.ptr(value), _lib.stream_ptr(dev)), "general forward")
    return run


def engine_section(dev):
    print(f"1. evaluation of all leaves and one move ({SIMS} simulations), 9x9")
    for G in (512, 2048):
        st = records(G, dev)
        for shape, ev in (((6, 64, 2), "general"), ((6, 128, 3), "general"), ((6, 128, 3), "gnn"), ((6, 256, 4), "general")):
            net = net_of(shape, dev)
            if ev == "general":
                fwd = general_forward_fn(net, st, dev)
            else:
                fwd = lambda: net.forward_states(st, check_saturation=False)   # noqa: E731
            with torch.no_grad():
                eval_ms = alternating([fwd])[0]
                eng = BatchedSelfPlay(net, num_games=G, sims=SIMS, evaluator=ev, seed=0, record_history=False)
                eng.move()                                    # capture
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(MOVES):
                    eng.move()
                torch.cuda.synchronize()
                mv = (time.perf_counter() - t0) / MOVES
            print(f"  G={G:5d} {'/'.join(map(str, shape)):9s} {ev:8s} eval {eval_ms:7.3f} ms   move {1e3 * mv:8.2f} ms = "
                  f"{1e3 * mv / SIMS:6.3f} ms/sim   {G / mv:9.0f} game-moves/s")
            del eng


def layer_section(dev):
    from tests.test_engine_general import _composition
    print("2. one hidden x hidden GCN layer, T(3 layers) - T(2 layers) of the whole forward (median of alternating runs)")
    for B in (1024, 4096):
        st = records(B, dev)
        for H in (64, 128, 256):
            nets = {L: net_of((6, H, L), dev) for L in (2, 3)}
            fns = []
            for L in (2, 3):
                fns.append(general_forward_fn(nets[L], st, dev))
                fns.append(lambda n=nets[L]: _composition(n, dev, st))
            with torch.no_grad():
                f2, c2, f3, c3 = alternating(fns)
            tiles = -(-H // 64)
            w_l2 = B * tiles * 64 * H * 4 / 1e6
            print(f"  B={B:5d} H={H:4d}  fused layer {f3 - f2:7.3f} ms   linear + aggregate {c3 - c2:7.3f} ms   "
                  f"(whole forward, 3 layers: {f3:7.3f} vs {c3:7.3f} ms)   W re-read from L2 {w_l2:7.1f} MB/layer "
                  f"({w_l2 / max(f3 - f2, 1e-9):6.0f} GB/s)")


def external_section(dev):
    print("3. 'external' vs 'general', 8 games x 16 simulations, one move")
    net = net_of((6, 64, 2), dev)
    for ev in ("external", "general"):
        eng = BatchedSelfPlay(net, num_games=8, sims=16, evaluator=ev, seed=0, record_history=False)
        with torch.no_grad():
            eng.move()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(2):
                eng.move()
            torch.cuda.synchronize()
        print(f"  {ev:8s} {1e3 * (time.perf_counter() - t0) / 2:9.2f} ms per move")


def main():
    dev = _lib.require_gpu()
    which = os.environ.get("SECTIONS", "123")
    if "1" in which:
        engine_section(dev)
    if "2" in which:
        layer_section(dev)
    if "3" in which:
        external_section(dev)


if __name__ == "__main__":
    main()
