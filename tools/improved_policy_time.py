"""Times the completed-Q policy targets on one GPU (include/aqgnn.h, "completed-Q policy targets").

The read-out: one aqg_engine_root_improved_policy launch over READ_ROOTS (2,048) roots of a READ_SIMS (50) simulation search on 9x9 with
the fake evaluator, beside the aqg_engine_root_visits launch over the same roots (the read-out of the visit-count path).

The refresh form: one aqg_replay_refresh_policy launch -- n finished f32 policy rows in legal order written into n scattered slots of a
ring, value blend 0.25 -- against the counts form (aqg_replay_refresh on the visit rows the policy rows were made from) and against
the torch composition of the same rings: the mask by the count, zeros + scatter into an [n, A] f32 array, index_copy_ into the ring,
and the blend.  9x9 at n = 4,000 and 163,840.  The policy form and its composition must leave equal rings.

The stage, 9x9 with the default network: reanalyse() of STAGE_ROWS (4,000) rows at STAGE_SIMS (50) simulations with each policy target,
host wall-clock around a synchronise, the targets taking turns.

Per measurement: WARMUP rounds, then the median, fastest and slowest of ROUNDS (9) rounds, the forms taking turns round by round, a
512 MB fill in front of every timed call (tools/reanalyse_time.py's harness)."""
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import reanalyse_time as rt   # noqa: E402
from alphaquoridorgnn_amd import _lib   # noqa: E402
from alphaquoridorgnn_amd.replay import ReplayWindow   # noqa: E402

E = rt.E
ROUNDS, WARMUP = E("ROUNDS", "9"), E("WARMUP", "2")
READ_ROOTS, READ_SIMS = E("READ_ROOTS", "2048"), E("READ_SIMS", "50")
SIZES = [(9, E("GAMES9", "50") * E("PLIES9", "80")), (9, E("LARGE9", "163840"))]
STAGE_GAMES, STAGE_SIMS, STAGE_ROWS, STAGE_ROUNDS = E("STAGE_GAMES", "50"), E("STAGE_SIMS", "50"), E("STAGE_ROWS", "4000"), E("STAGE_ROUNDS", "3")
BLEND = 0.25
ML = _lib.MAX_LEGAL


def read_out(dev):
    from alphaquoridorgnn_amd.engine import BatchedSelfPlay
    N, G = 9, READ_ROOTS
    eng = BatchedSelfPlay(None, num_games=G, sims=READ_SIMS, board_size=N, evaluator="fake", fake_bias=1, record_history=False, device=dev)
    eng.reset()
    eng.search(eng.root_states72().clone())                    # G times the opening position
    policy = torch.empty((G, ML), dtype=torch.float32, device=dev)
    visits = torch.empty((G, ML), dtype=torch.int32, device=dev)
    actions = torch.empty((G, ML), dtype=torch.uint8, device=dev)
    count = torch.empty((G,), dtype=torch.int32, device=dev)
    vmix = torch.empty((G,), dtype=torch.float32, device=dev)

    def improved():
        _lib.check(eng.lib.aqg_engine_root_improved_policy(ctypes.byref(eng.e), 50.0, 1.0, _lib.ptr(policy), _lib.ptr(actions), _lib.ptr(count),
                                                           _lib.ptr(vmix), eng._stream()), "aqg_engine_root_improved_policy")

    def counts():
        _lib.check(eng.lib.aqg_engine_root_visits(ctypes.byref(eng.e), _lib.ptr(visits), _lib.ptr(actions), _lib.ptr(count), eng._stream()),
                   "aqg_engine_root_visits")

    nbytes = G * (32 * (1 + 131) + 4 * ML + ML + 8)
    times = rt.timed({"root_visits": counts, "root_improved_policy": improved}, ROUNDS, WARMUP)
    rt.report(f"read-out 9x9 {G} roots at {READ_SIMS} simulations", times, "root_visits", nbytes)
    torch.cuda.synchronize()
    print(f"read-out 9x9 rows sum to 1 within {float((policy.double().sum(1) - 1).abs().max()):.2e}; "
          f"non-zero entries per row {float((policy != 0).sum(1).float().mean()):.1f} against {float((visits != 0).sum(1).float().mean()):.1f} "
          f"of the visit rows", flush=True)


def refresh_forms(dev):
    lib = _lib.load()
    for N, n in SIZES:
        A = N * N + 2 * (N - 1) ** 2
        capacity = n + n // 2
        visits, actions, count, q, slots = rt.searched(N, n, capacity, dev)
        j = torch.arange(ML, device=dev)[None, :]
        inside = j < count[:, None]
        policy = torch.where(inside, (visits.float() + 0.25), torch.zeros((), device=dev))
        policy = (policy / policy.sum(1, keepdim=True)).contiguous()                   # non-zero on every legal action, like pi'
        g = torch.Generator(device="cpu").manual_seed(n)
        first = (torch.rand((capacity, A), generator=g).to(dev), (torch.rand((capacity,), generator=g) * 2 - 1).to(dev))
        rings = {k: tuple(x.clone() for x in first) for k in ("torch composition", "counts form", "policy form")}
        keep = torch.tensor(1.0, dtype=torch.float32) - torch.tensor(BLEND, dtype=torch.float32)

        def policy_form():
            rpi, rz = rings["policy form"]
            _lib.check(lib.aqg_replay_refresh_policy(N, A, _lib.ptr(policy), _lib.ptr(actions), _lib.ptr(count), _lib.ptr(q), BLEND,
                                                     _lib.ptr(slots), n, capacity, _lib.ptr(rpi), _lib.ptr(rz), _lib.stream_ptr(dev)),
                       "aqg_replay_refresh_policy")

        def counts_form():
            rpi, rz = rings["counts form"]
            _lib.check(lib.aqg_replay_refresh(N, A, _lib.ptr(visits), _lib.ptr(actions), _lib.ptr(count), _lib.ptr(q), BLEND, _lib.ptr(slots),
                                              n, capacity, _lib.ptr(rpi), _lib.ptr(rz), _lib.stream_ptr(dev)), "aqg_replay_refresh")

        def composition():
            rpi, rz = rings["torch composition"]
            live = j < count[:, None]
            dense = torch.zeros((n, A + 1), dtype=torch.float32, device=dev)
            dense.scatter_(1, torch.where(live, actions.long(), A), torch.where(live, policy, 0.0))
            rpi.index_copy_(0, slots, dense[:, :A])
            rz.index_copy_(0, slots, float(keep) * rz.index_select(0, slots) + BLEND * q)

        nbytes = n * (4 * ML + ML + 16 + 4 * A + 8)
        forms = {"torch composition": composition, "counts form": counts_form, "policy form": policy_form}
        rt.report(f"refresh  {N}x{N} n {n:7d} ({nbytes / 1e6:7.1f} MB read + written)", rt.timed(forms, ROUNDS, WARMUP), "torch composition", nbytes)
        torch.cuda.synchronize()
        same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(rings["policy form"], rings["torch composition"]))
        print(f"refresh  {N}x{N} n {n:7d} the rings of the policy form and of the composition are equal: {same}", flush=True)


def stage(dev):
    from alphaquoridorgnn_amd.engine import MultiSetSelfPlay
    from alphaquoridorgnn_amd.pv_network_gnn import GNNNetwork
    from alphaquoridorgnn_amd.reanalyse import eligible_rows, reanalyse
    N = 9
    torch.manual_seed(1)
    model = GNNNetwork().to(dev).eval()
    model.packed_weights(dev)
    window = ReplayWindow(N, max_generations=2, capacity_rows=200000, device=dev)
    for k in range(2):
        eng = MultiSetSelfPlay(model, num_games=STAGE_GAMES, quota=STAGE_GAMES, sims=STAGE_SIMS, num_sets=1, board_size=N, seed=11 + k, device=dev)
        eng.play_generation()
        window.append_counts(*eng.history_tensors())
        del eng
    eligible = eligible_rows(window)
    done, update = [], [0]

    def one_pass(target):
        def run():
            done.append(reanalyse(window, model, STAGE_ROWS, sims=STAGE_SIMS, seed=3, update=update[0], policy_target=target))
            update[0] += 1
        return run

    times = rt.timed({"visits": one_pass("visits"), "completed_q": one_pass("completed_q")}, STAGE_ROUNDS, 1, wall=True)
    for k, t in times.items():
        print(f"stage    9x9 reanalyse of {done[-1]} of {eligible} rows at {STAGE_SIMS} simulations, policy target {k:12s}: median "
              f"{float(np.median(t)):10.1f} ms  min {min(t):10.1f}  max {max(t):10.1f} host wall-clock", flush=True)


def main():
    dev = torch.device("cuda", torch.cuda.current_device())
    rt.FLUSH.append(torch.zeros((512 << 20,), dtype=torch.uint8, device=dev))
    read_out(dev)
    refresh_forms(dev)
    if STAGE_ROUNDS > 0:
        stage(dev)


if __name__ == "__main__":
    main()
