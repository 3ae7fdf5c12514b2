"""The learning loop, every stage on the MI355X path -- drop-in for the reference's train_cycle.py:10-45.

    create_network()  ->  repeat NUM_TRAIN_CYCLE times:  self_play()  ->  train_network()  ->  evaluate_network()

with the GNN or (--network cnn) the reference's residual CNN: the parameter update dispatches on what best.pth holds.

The reference's commented-out evaluate_best_player stage (the best network against the random, alpha-beta and rollout-MCTS agents,
evaluate_agents.py) is opt-in: --baseline-games K plays K games per agent after each cycle's evaluation stage, on rank 0.
"""
from . import constants
from . import distributed as aqd
from .evaluate_network import evaluate_network
from .pv_network_gnn import create_network
from .self_play import self_play
from .train_network import train_network
from .train_cycle_options import (_parser, check_args, apply_args, _check_start_args, _set_start_options,  # noqa: F401
                                  _check_policy_args, _set_policy_options, _check_reanalyse_args, _check_reanalyse_policy_args,
                                  _set_reanalyse_options, _check_surprise_args, _set_surprise_options, _check_holdout_args,
                                  _set_holdout_options, _set_replay_options, _check_value_lambda_args, _set_target_options,
                                  _set_tree_reuse_options, _set_resign_options, _set_mirror_options, _set_optimiser_options,
                                  _check_average_args, _set_average_options)

NUM_TRAIN_CYCLE = 1000   # train_cycle.py:18


def parameter_update():
    """What the parameter-update stage (train_network in _STAGES) runs: train_network.train_cnn_network() when best.pth holds the
    residual CNN, train_network.train_network() otherwise (both looked up on the module at call time)."""
    import os
    import torch
    from . import train_network as tn
    from .pv_network_cnn import is_cnn_state_dict
    best = constants.PV_NETWORK_PATH + 'best.pth'
    if os.path.exists(best) and is_cnn_state_dict(torch.load(best, map_location="cpu", weights_only=True)):
        return tn.train_cnn_network()
    return tn.train_network()


_STAGES = (("self-play", self_play), ("parameter update", train_network), ("evaluation of the new parameters", evaluate_network))


def _dist():
    """(torch.distributed, whether more than one rank runs, this rank)."""
    import torch.distributed as dist
    rank, world = aqd.rank_world()
    return dist, world > 1, rank


def _create_cnn_network(num_filters=None, num_residual_blocks=None):
    """A CNNNetwork of the given shape (default 128 x 16, pv_network_cnn.py:14-15) written as best.pth at PV_NETWORK_PATH -- where
    self-play, training and evaluation look -- unless a best.pth exists."""
    import os
    import torch
    from . import pv_network_cnn as pc
    path = constants.PV_NETWORK_PATH + 'best.pth'
    if os.path.exists(path):
        return
    model = pc.CNNNetwork(pc.NUM_FILTERS if num_filters is None else num_filters,
                          pc.NUM_RESIDUAL_BLOCKS if num_residual_blocks is None else num_residual_blocks, constants.BOARD_SIZE)
    os.makedirs(constants.PV_NETWORK_PATH, exist_ok=True)
    torch.save(model.state_dict(), path)


def _create_network_once(hidden_dim=None, num_gcn_layers=None, network="gnn", num_filters=None, num_residual_blocks=None):
    """create_network() draws random weights: under torch.distributed only rank 0 may write best.pth (every rank would
    otherwise save a different random init to the same path); the others wait for the file."""
    dist, on, rank = _dist()
    if rank == 0:
        if network == "cnn":
            _create_cnn_network(num_filters, num_residual_blocks)
        else:
            create_network(hidden_dim=hidden_dim, num_gcn_layers=num_gcn_layers)
    if on:
        dist.barrier()


def _evaluate_once():
    """evaluate_network() samples its games from the global numpy RNG: rank 0 plays the match and decides, the decision
    is broadcast, and nobody reads best.pth again before the copy is done."""
    import torch
    dist, on, rank = _dist()
    tag = aqd.next_tag("evaluate")
    if rank == 0:
        with aqd.single_rank_stage(tag):           # the key is published even if the match raises: idle ranks wake up and raise too
            promoted = evaluate_network()
    else:
        promoted = False
        aqd.wait_for_rank0(tag)          # host-side wait: no collective is pending while rank 0 plays the match
    if on:
        t = torch.tensor([1 if promoted else 0], dtype=torch.int64, device=aqd.collective_device())
        dist.broadcast(t, src=0)
        promoted = bool(int(t.item()))
        dist.barrier()
    return promoted


def _baseline_once(games):
    """evaluate_best_player(games) on rank 0, inside a single-rank stage like _evaluate_once; the other ranks wait.  Returns the
    dict of average points on rank 0, None elsewhere."""
    from .evaluate_agents import evaluate_best_player
    dist, on, rank = _dist()
    tag = aqd.next_tag("baseline")
    result = None
    if rank == 0:
        with aqd.single_rank_stage(tag):
            result = evaluate_best_player(games)
    else:
        aqd.wait_for_rank0(tag)
    if on:
        dist.barrier()
    return result


def train_cycle(num_cycles=None, hidden_dim=None, num_gcn_layers=None, network="gnn", num_filters=None, num_residual_blocks=None,
                baseline_games=0, baseline=None):
    """Run the cycle; returns, per iteration, whether `latest` was promoted to `best`.  network 'gnn' (hidden_dim / num_gcn_layers)
    or 'cnn' (num_filters / num_residual_blocks) shapes the best.pth written when none exists; every stage then follows the
    network and shape best.pth holds.  baseline_games K > 0: after each cycle's evaluation stage rank 0 plays best.pth against the
    baseline agents, K games each (evaluate_agents.evaluate_best_player), and appends the dict to the list `baseline`."""
    if network not in ("gnn", "cnn"):
        raise ValueError("network must be 'gnn' or 'cnn'")
    total = NUM_TRAIN_CYCLE if num_cycles is None else int(num_cycles)
    print(f'{constants.PV_NETWORK_NAME} network, {constants.BOARD_SIZE}x{constants.BOARD_SIZE} board, {total} training cycle(s)')
    _create_network_once(hidden_dim, num_gcn_layers, network, num_filters, num_residual_blocks)
    promoted = []
    rank = _dist()[2]
    for cycle in range(1, total + 1):
        outcome = None
        for title, stage in _STAGES:
            if rank == 0:
                print(f'\n[cycle {cycle}/{total}] {title}')
            if stage is evaluate_network:
                outcome = _evaluate_once()
            elif stage is train_network:
                outcome = parameter_update()           # the GNN's stage, or the CNN's when best.pth holds one
            else:
                outcome = stage()
        promoted.append(bool(outcome))
        if baseline_games and baseline_games > 0:
            if rank == 0:
                print(f'\n[cycle {cycle}/{total}] evaluation against the baseline agents')
            points = _baseline_once(int(baseline_games))
            if baseline is not None:
                baseline.append(points)
    return promoted


def main(argv=None):
    """The command line (train_cycle_options: DESCRIPTION is what --help says of it): parse, refuse what can be refused without a
    device, bind this rank to its GPU and join the process group, hand the flags over, run the cycle."""
    import json
    import os
    args = _parser().parse_args(argv)
    check_args(args)                                    # in front of anything that touches a device or the process group
    rank, world = aqd.init_from_env()
    apply_args(args)
    try:
        baseline = []
        promoted = train_cycle(args.cycles, hidden_dim=args.hidden_dim, num_gcn_layers=args.num_gcn_layers, network=args.network,
                               num_filters=args.num_filters, num_residual_blocks=args.num_residual_blocks,
                               baseline_games=args.baseline_games, baseline=baseline)
        if args.result_dir:
            import hashlib
            with open(constants.PV_NETWORK_PATH + 'latest.pth', 'rb') as f:
                digest = hashlib.sha256(f.read()).hexdigest()
            import torch
            with open(os.path.join(args.result_dir, f"train_cycle.rank{rank}.json"), "w") as f:
                result = {"rank": rank, "world": world, "promoted": promoted, "latest_sha256": digest,
                          "device": torch.cuda.current_device()}
                if args.baseline_games > 0:
                    result["baseline"] = baseline
                json.dump(result, f)
    except BaseException:
        aqd.shutdown(ok=False)                      # no barrier on the way out of an exception: the other ranks may never reach one
        raise
    aqd.shutdown()
    return promoted


if __name__ == '__main__':
    main()
