"""The command line of train_cycle.main(): the parser, the checks that need no device (check_args: run in front of anything that
touches a GPU or the process group) and the hand-over of the checked flags onto self_play's, train_network's, pv_mcts's and
evaluate_network's module constants (apply_args), which the stages read at call time."""
import argparse
import math
from pathlib import Path

from . import constants, evaluate_network as en, pv_mcts, self_play as sp, train_network as tn
from . import distributed as aqd
from .openings import check_window_share
from .reanalyse import check_reanalyse_options
from .replay import ReplayWindow, check_holdout_options, check_surprise_options, check_value_blend
from .selfplay_options import (check_gumbel, check_policy_record, check_policy_target, check_resign, check_target_options, check_tree_reuse,
                               check_value_lambda)
from .train_reference import check_average_controls, check_loss_controls

DESCRIPTION = """`python -m alphaquoridorgnn_amd.train_cycle` -- also the per-rank program of
    `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P -m
    alphaquoridorgnn_amd.train_cycle`: every rank binds to GPU LOCAL_RANK and joins the RCCL group (distributed.init_from_env)
    before anything touches a device; self-play is sharded over the ranks, rank 0 trains / evaluates (module docstrings)."""


def _parser():
    """The command line of train_cycle.main()."""
    ap = argparse.ArgumentParser(description=DESCRIPTION)
    ap.add_argument("--cycles", type=int, default=None, help="training cycles (default NUM_TRAIN_CYCLE = 1000, train_cycle.py:18)")
    ap.add_argument("--games", type=int, default=None, help="self-play games per generation over ALL ranks (default SP_GAME_COUNT)")
    ap.add_argument("--sims", type=int, default=None, help="simulations per move (default pv_mcts.PV_EVALUATE_COUNT)")
    ap.add_argument("--epochs", type=int, default=None, help="epochs per parameter update (default train_network.NUM_EPOCH)")
    ap.add_argument("--eval-games", type=int, default=None, help="games per evaluation (default EN_GAME_COUNT)")
    ap.add_argument("--result-dir", default=None, help="every rank writes train_cycle.rank<r>.json (promotions, sha256 of latest.pth) here")
    ap.add_argument("--hidden-dim", type=int, default=None,
                    help="hidden width of the network created when no best.pth exists (default HIDDEN_DIM = 128)")
    ap.add_argument("--num-gcn-layers", type=int, default=None,
                    help="GCN layers of the network created when no best.pth exists (default NUM_GCN_LAYERS = 3)")
    ap.add_argument("--network", choices=("gnn", "cnn"), default="gnn",
                    help="network created when no best.pth exists: the GNN (default) or the reference's residual CNN")
    ap.add_argument("--num-filters", type=int, default=None,
                    help="filters of the CNN created when no best.pth exists (default NUM_FILTERS = 128)")
    ap.add_argument("--num-residual-blocks", type=int, default=None,
                    help="residual blocks of the CNN created when no best.pth exists (default NUM_RESIDUAL_BLOCKS = 16)")
    ap.add_argument("--baseline-games", type=int, default=0,
                    help="games per baseline agent (random, alpha-beta, rollout MCTS) best.pth plays after each cycle's evaluation "
                         "stage, on rank 0 (default 0: no such stage)")
    ap.add_argument("--root-noise-eps", type=float, default=None,
                    help="self-play: weight of the Dirichlet noise mixed into every root's priors (default SP_ROOT_NOISE_EPS = 0: off)")
    ap.add_argument("--root-noise-alpha", type=float, default=None,
                    help="self-play: Dirichlet concentration (default SP_ROOT_NOISE_ALPHA: 10 / the board's action count)")
    ap.add_argument("--temperature-plies", type=int, default=None,
                    help="self-play: plies of a game sampled at SP_TEMPERATURE before the most visited move is taken (default "
                         "SP_TEMPERATURE_PLIES = 0: every ply is sampled)")
    ap.add_argument("--tree-reuse", action="store_true",
                    help="self-play: start each move's search from the chosen child's subtree (default SP_TREE_REUSE = False: a fresh "
                         "tree every move)")
    ap.add_argument("--tree-reuse-visits", type=int, default=None,
                    help="self-play, with --tree-reuse: keep a subtree of at most this many visits (default SP_TREE_REUSE_VISITS: the "
                         "simulation count)")
    ap.add_argument("--resign-threshold", default=None, metavar="T|auto",
                    help="self-play: a mover whose search value and most visited child's value are both below -T resigns the game "
                         "(T in (0, 1]); 'auto': the first generation plays every game out and only collects, and after each "
                         "generation the next T is the one that resigns the most within --resign-max-false-positive (default "
                         "SP_RESIGN_THRESHOLD = None: off)")
    ap.add_argument("--resign-min-ply", type=int, default=None,
                    help="self-play, with --resign-threshold: no resignation before this ply (default SP_RESIGN_MIN_PLY = 0)")
    ap.add_argument("--resign-max-false-positive", type=float, default=None, metavar="F",
                    help="self-play, with --resign-threshold auto: the share of the played-out games' sides that did not lose and "
                         "may still have resigned (default SP_RESIGN_MAX_FALSE_POSITIVE = 0.05)")
    ap.add_argument("--slots", type=int, default=None, metavar="G",
                    help="self-play: play a rank's games on G slots that take the next game when theirs ends (default SP_SLOTS = "
                         "None: one slot per game)")
    ap.add_argument("--value-blend", type=float, default=None,
                    help="self-play: weight L in [0, 1] of the root's search value in the value target, (1 - L) z + L q (default "
                         "SP_VALUE_BLEND = 0: the game outcome alone)")
    ap.add_argument("--value-lambda", type=float, default=None, metavar="X",
                    help="self-play, with --value-blend L > 0: q becomes the lambda-return G of the game's later search values, "
                         "bootstrapped into its outcome -- X in [0, 1], 0 = q, 1 = z (default SP_VALUE_LAMBDA = None: q itself)")
    ap.add_argument("--mirror-augment", action="store_true",
                    help="parameter update: train every epoch on positions mirrored left to right at random (default TRAIN_MIRROR = False: off)")
    ap.add_argument("--mirror-seed", type=int, default=None,
                    help="parameter update: seed of the mirror draws (default TRAIN_MIRROR_SEED = 0)")
    ap.add_argument("--weight-decay", type=float, default=None, metavar="W",
                    help="parameter update: weight decay W on the weight matrices and conv kernels, inside the HIP step (default "
                         "TRAIN_WEIGHT_DECAY = 0: none); decoupled as torch.optim.AdamW unless --coupled-weight-decay")
    ap.add_argument("--coupled-weight-decay", action="store_true",
                    help="parameter update: add W * p to the gradient, as torch.optim.Adam(weight_decay=W) (needs --weight-decay)")
    ap.add_argument("--max-grad-norm", type=float, default=None, metavar="M",
                    help="parameter update: scale every step's gradient to a global L2 norm of at most M, as "
                         "torch.nn.utils.clip_grad_norm_ (default TRAIN_MAX_GRAD_NORM = None: off)")
    ap.add_argument("--policy-loss", choices=("reference", "cross-entropy"), default=None,
                    help="parameter update: the policy loss -- 'reference', CrossEntropyLoss on the already-softmaxed policy, or "
                         "'cross-entropy', the cross-entropy between the target and softmax(logits), taken from the logits inside the "
                         "HIP step (default TRAIN_POLICY_LOSS = 'reference')")
    ap.add_argument("--value-loss-weight", type=_value_loss_weight, default=None, metavar="W",
                    help="parameter update: weight W >= 0 of the value term, the loss minimised being policy + W * value (default "
                         "TRAIN_VALUE_LOSS_WEIGHT = 1)")
    ap.add_argument("--ema-decay", type=float, default=None, metavar="D",
                    help="parameter update: keep an exponential moving average of the parameters with decay D in [0, 1), updated "
                         "inside the HIP steps, and save IT as latest.pth (default TRAIN_EMA_DECAY = None: off, the last iterate)")
    ap.add_argument("--ema-every", type=int, default=None, metavar="K",
                    help="parameter update: update the average at the Adam steps whose number is a multiple of K (default "
                         "TRAIN_EMA_EVERY = 1; needs --ema-decay)")
    ap.add_argument("--replay-generations", type=int, default=0,
                    help="train on a replay window of the newest K self-play generations, resident on the GPU (default 0: off, the "
                         "newest .history file alone); a cycle that finds .history files in ./data resumes from the newest K")
    ap.add_argument("--replay-rows", type=int, default=None,
                    help="rows of the replay window's ring (default: K * 1.5 * the first generation's rows)")
    ap.add_argument("--epoch-rows", type=int, default=None,
                    help="parameter update: rows an epoch trains on, drawn afresh from the window by every epoch's shuffle (default "
                         "TRAIN_EPOCH_ROWS = None: all of them)")
    ap.add_argument("--merge-positions", action="store_true",
                    help="parameter update: merge the rows that hold the same position into one row with the mean policy and value "
                         "target, once per update (default TRAIN_MERGE_POSITIONS = False: one row per occurrence)")
    ap.add_argument("--surprise-weighting", action="store_true",
                    help="parameter update: draw the rows of an update by policy surprise, KL(row's policy target || the network the "
                         "update starts from), once per update and behind --merge-positions (default TRAIN_SURPRISE_WEIGHTING = False: "
                         "every row once)")
    ap.add_argument("--surprise-uniform-share", type=float, default=None, metavar="U",
                    help="parameter update, with --surprise-weighting: the share U in [0, 1] of an update's rows dealt out evenly, the "
                         "rest in proportion to the surprise (default TRAIN_SURPRISE_UNIFORM_SHARE = 0.5)")
    ap.add_argument("--surprise-max-copies", type=int, default=None, metavar="C",
                    help="parameter update, with --surprise-weighting: the most copies of one row, 1..255 (default "
                         "TRAIN_SURPRISE_MAX_COPIES = 8)")
    ap.add_argument("--surprise-seed", type=int, default=None, metavar="S",
                    help="parameter update, with --surprise-weighting: seed of the draws that round a row's expected copies (default "
                         "TRAIN_SURPRISE_SEED = 0)")
    ap.add_argument("--holdout-share", type=float, default=None, metavar="S",
                    help="parameter update: hold a share S in (0, 1) of the POSITIONS out of every update -- a position's side is a "
                         "function of (--holdout-seed, its record) alone -- and validate the network on them after the epochs "
                         "(default TRAIN_HOLDOUT_SHARE = None: off, nothing is launched)")
    ap.add_argument("--holdout-seed", type=int, default=None, metavar="K",
                    help="parameter update, with --holdout-share: seed of the split (default TRAIN_HOLDOUT_SEED = 0); a run that "
                         "changes it between cycles trains on positions it held out before")
    ap.add_argument("--holdout-every", type=int, default=None, metavar="V",
                    help="parameter update, with --holdout-share: validate after every V-th epoch, and always after the last (default "
                         "TRAIN_HOLDOUT_EVERY = 1)")
    ap.add_argument("--keep-best-epoch", action="store_true",
                    help="parameter update, with --holdout-share: save as latest.pth the network of the validated epoch with the "
                         "least held-out policy loss + value MSE (default TRAIN_HOLDOUT_KEEP_BEST = False: the last epoch's)")
    ap.add_argument("--holdout-log", default=None, metavar="PATH",
                    help="parameter update, with --holdout-share: append one JSON line per update to PATH -- the validation curve, the "
                         "per-bucket table of the saved network, the split's counts and the options in force")
    ap.add_argument("--no-history-file", action="store_true",
                    help="self-play: write no .history file (needs --replay-generations; default SP_WRITE_HISTORY = True)")
    ap.add_argument("--reanalyse-rows", type=int, default=None, metavar="R",
                    help="self-play: after each generation, search R of the replay window's older rows again with the network that "
                         "just played and overwrite their policy targets (needs --replay-generations K >= 2; default "
                         "SP_REANALYSE_ROWS = 0: off)")
    ap.add_argument("--reanalyse-sims", type=int, default=None, metavar="S",
                    help="self-play, with --reanalyse-rows: simulations of the fresh searches (default SP_REANALYSE_SIMS: those of a move)")
    ap.add_argument("--reanalyse-value-blend", type=float, default=None, metavar="L",
                    help="self-play, with --reanalyse-rows: weight L in [0, 1] of the fresh search value in a refreshed row's value "
                         "target, (1 - L) z + L q (default SP_REANALYSE_VALUE_BLEND = 0: the value target stays)")
    ap.add_argument("--reanalyse-policy-target", choices=("visits", "completed-q"), default=None,
                    help="self-play, with --reanalyse-rows: a refreshed row's policy target -- the normalised visit counts, or the "
                         "completed-Q improved policy softmax(log p + sigma(completedQ)) of the fresh search (default "
                         "SP_REANALYSE_POLICY_TARGET = visits)")
    ap.add_argument("--reanalyse-c-visit", type=float, default=None, metavar="X",
                    help="self-play, with --reanalyse-policy-target completed-q: c_visit of the transform, >= 0 (default "
                         "SP_REANALYSE_C_VISIT = 50)")
    ap.add_argument("--reanalyse-c-scale", type=float, default=None, metavar="Y",
                    help="self-play, with --reanalyse-policy-target completed-q: c_scale of the transform, >= 0 (default "
                         "SP_REANALYSE_C_SCALE = 1)")
    ap.add_argument("--policy-target", choices=("visits", "completed-q"), default=None,
                    help="self-play: the policy target of the generation's own rows -- the normalised visit counts, or the completed-Q "
                         "improved policy softmax(log p + sigma(completedQ)) of every searched root, recorded move by move (the move "
                         "is still chosen from the visit counts; default SP_POLICY_TARGET = visits)")
    ap.add_argument("--policy-c-visit", type=float, default=None, metavar="X",
                    help="self-play, with --policy-target completed-q: c_visit of the transform, >= 0 (default SP_POLICY_C_VISIT = 50)")
    ap.add_argument("--policy-c-scale", type=float, default=None, metavar="Y",
                    help="self-play, with --policy-target completed-q: c_scale of the transform, >= 0 (default SP_POLICY_C_SCALE = 1)")
    ap.add_argument("--gumbel-considered", type=int, default=None, metavar="M",
                    help="self-play: Gumbel root search -- every root samples M actions without replacement (1..64), spends the "
                         "simulations on them by sequential halving and plays the survivor; needs --policy-target completed-q, the "
                         "matching training target (default SP_GUMBEL_CONSIDERED = 0: off, PUCT at the root and a draw from the visits)")
    ap.add_argument("--gumbel-scale", type=float, default=None, metavar="S",
                    help="self-play, with --gumbel-considered: factor S >= 0 on the Gumbel variates, 0 = a deterministic search "
                         "(default SP_GUMBEL_SCALE = 1)")
    ap.add_argument("--gumbel-seed", type=int, default=None, metavar="K",
                    help="self-play, with --gumbel-considered: seed of the variates (default SP_GUMBEL_SEED = None: derived from the "
                         "generation's seed)")
    ap.add_argument("--eval-opening-plies", type=int, default=None, metavar="K",
                    help="evaluation: play the match from a book of paired openings K random plies deep (K even, an even game count), "
                         "each opening twice with the colours exchanged, and print the paired report (default EN_OPENING_PLIES = 0: off)")
    ap.add_argument("--eval-opening-seed", type=int, default=None, metavar="S",
                    help="evaluation, with --eval-opening-plies: the seed of the book (default EN_OPENING_SEED = 0)")
    ap.add_argument("--start-from-window", type=float, default=None, metavar="S",
                    help="self-play: start a share S in [0, 1] of every generation's games from positions of the replay window instead of "
                         "the opening record (needs --replay-generations; default SP_START_FROM_WINDOW_SHARE = 0: off)")
    return ap


def _check_start_args(args):
    """--eval-opening-plies / --eval-opening-seed / --start-from-window, refused at parse time: an odd depth, an odd game count with a
    depth, a seed without a depth, a share outside [0, 1], a share without a window.  Returns (plies or None, seed or None, share or
    None)."""
    if args.eval_opening_plies is None and args.eval_opening_seed is not None:
        raise ValueError("--eval-opening-seed needs --eval-opening-plies")
    if args.eval_opening_plies is not None:
        games = en.EN_GAME_COUNT if args.eval_games is None else args.eval_games
        try:
            en.check_opening_options(args.eval_opening_plies, games)
        except ValueError as err:
            raise ValueError(f"--eval-opening-plies / --eval-games: {err}") from None
    share = None
    if args.start_from_window is not None:
        try:
            share = check_window_share(args.start_from_window)
        except ValueError as err:
            raise ValueError(f"--start-from-window: {err}") from None
        if args.replay_generations < 1:
            raise ValueError("--start-from-window needs --replay-generations K >= 1: there is no window to start from")
    return args.eval_opening_plies, args.eval_opening_seed, share


def _set_start_options(args):
    """The checked start-position flags onto evaluate_network's and self_play's constants."""
    plies, seed, share = _check_start_args(args)
    if plies is not None:
        en.EN_OPENING_PLIES = plies
    if seed is not None:
        en.EN_OPENING_SEED = seed
    if share is not None:
        sp.SP_START_FROM_WINDOW_SHARE = share


def _check_policy_args(args):
    """--policy-target / --policy-c-visit / --policy-c-scale, refused at parse time: a coefficient without --policy-target completed-q,
    and constants the engine would refuse.  Returns (policy_target, c_visit, c_scale) with the defaults filled in, or None when none
    of the three is given."""
    given = (args.policy_target, args.policy_c_visit, args.policy_c_scale)
    if all(x is None for x in given):
        return None
    if args.policy_target != "completed-q" and (args.policy_c_visit is not None or args.policy_c_scale is not None):
        raise ValueError("--policy-c-visit and --policy-c-scale need --policy-target completed-q")
    try:
        return check_policy_record(*(d if x is None else x for x, d in zip(given, ("visits", sp.SP_POLICY_C_VISIT, sp.SP_POLICY_C_SCALE))))
    except ValueError as err:
        raise ValueError(f"--policy-target / --policy-c-visit / --policy-c-scale: {err}") from None


def _check_gumbel_args(args):
    """--gumbel-considered / --gumbel-scale / --gumbel-seed, refused at parse time: the two dependent flags without the first, the
    option without --policy-target completed-q (a visit row is not a target under sequential halving), and everything the library
    refuses -- M outside 1..64, a bad scale, fewer than two simulations, and the option beside root noise, tree reuse, resignation or
    --temperature-plies.  Returns (considered, scale, seed or None), or None when the option is off."""
    if args.gumbel_considered is None:
        if args.gumbel_scale is not None or args.gumbel_seed is not None:
            raise ValueError("--gumbel-scale and --gumbel-seed need --gumbel-considered")
        return None
    if args.gumbel_considered < 1:
        raise ValueError("--gumbel-considered must be in 1..64")
    target = args.policy_target if args.policy_target is not None else sp.SP_POLICY_TARGET
    if str(target).replace("-", "_") != "completed_q":
        raise ValueError("--gumbel-considered needs --policy-target completed-q: a visit row is not a policy target under sequential halving")
    sims = pv_mcts.PV_EVALUATE_COUNT if args.sims is None else args.sims
    eps = sp.SP_ROOT_NOISE_EPS if args.root_noise_eps is None else args.root_noise_eps
    plies = sp.SP_TEMPERATURE_PLIES if args.temperature_plies is None else args.temperature_plies
    reuse = bool(args.tree_reuse or args.tree_reuse_visits is not None or sp.SP_TREE_REUSE)
    resign = args.resign_threshold if args.resign_threshold is not None else sp.SP_RESIGN_THRESHOLD
    try:
        considered, scale = check_gumbel(args.gumbel_considered, sp.SP_GUMBEL_SCALE if args.gumbel_scale is None else args.gumbel_scale,
                                         sims, eps, reuse, resign, plies)
    except ValueError as err:
        raise ValueError(f"--gumbel-considered / --gumbel-scale: {err}") from None
    return considered, scale, args.gumbel_seed


def _set_gumbel_options(args):
    """The checked Gumbel flags onto self_play's constants."""
    checked = _check_gumbel_args(args)
    if checked is not None:
        sp.SP_GUMBEL_CONSIDERED, sp.SP_GUMBEL_SCALE, sp.SP_GUMBEL_SEED = checked


def _set_policy_options(args):
    """The checked policy-target flags onto self_play's constants."""
    target = _check_policy_args(args)
    if target is not None:
        sp.SP_POLICY_TARGET, sp.SP_POLICY_C_VISIT, sp.SP_POLICY_C_SCALE = target


def _check_reanalyse_args(args):
    """--reanalyse-rows / --reanalyse-sims / --reanalyse-value-blend, refused at parse time: values the stage would refuse, the two
    dependent flags without --reanalyse-rows, and a window that can hold no older generation."""
    if args.reanalyse_rows is None:
        if args.reanalyse_sims is not None or args.reanalyse_value_blend is not None:
            raise ValueError("--reanalyse-sims and --reanalyse-value-blend need --reanalyse-rows")
        return None
    if args.reanalyse_rows < 0:
        raise ValueError("--reanalyse-rows must be >= 0")
    if args.reanalyse_sims is not None and args.reanalyse_sims < 1:
        raise ValueError("--reanalyse-sims must be >= 1")
    blend = 0.0 if args.reanalyse_value_blend is None else args.reanalyse_value_blend
    if not 0.0 <= blend <= 1.0:                             # NaN fails both
        raise ValueError("--reanalyse-value-blend must be in [0, 1]")
    if args.replay_generations < 2:
        raise ValueError("--reanalyse-rows needs --replay-generations K >= 2: the newest generation is never searched again")
    return check_reanalyse_options(args.reanalyse_rows, args.reanalyse_sims, blend)[:3]


def _check_reanalyse_policy_args(args):
    """--reanalyse-policy-target / --reanalyse-c-visit / --reanalyse-c-scale, refused at parse time: any of them without
    --reanalyse-rows, and constants the stage would refuse.  Returns (policy_target, c_visit, c_scale) with the defaults filled in, or
    None when none of the three is given."""
    given = (args.reanalyse_policy_target, args.reanalyse_c_visit, args.reanalyse_c_scale)
    if all(x is None for x in given):
        return None
    if args.reanalyse_rows is None:
        raise ValueError("--reanalyse-policy-target, --reanalyse-c-visit and --reanalyse-c-scale need --reanalyse-rows")
    try:
        return check_policy_target(*(d if x is None else x for x, d in zip(given, ("visits", sp.SP_REANALYSE_C_VISIT, sp.SP_REANALYSE_C_SCALE))))
    except ValueError as err:
        raise ValueError(f"--reanalyse-policy-target / --reanalyse-c-visit / --reanalyse-c-scale: {err}") from None


def _set_reanalyse_options(args):
    """The checked reanalyse flags onto self_play's constants (after _set_replay_options: the window exists)."""
    checked = _check_reanalyse_args(args)
    if checked is not None:
        sp.SP_REANALYSE_ROWS, sp.SP_REANALYSE_SIMS, sp.SP_REANALYSE_VALUE_BLEND = checked
    target = _check_reanalyse_policy_args(args)
    if target is not None:
        sp.SP_REANALYSE_POLICY_TARGET, sp.SP_REANALYSE_C_VISIT, sp.SP_REANALYSE_C_SCALE = target


def _check_surprise_args(args):
    """--surprise-weighting / --surprise-uniform-share / --surprise-max-copies / --surprise-seed, refused at parse time: a coefficient
    without the main flag, and values the stage would refuse.  Returns (uniform_share, max_copies, seed) with the defaults filled in,
    or None when the option is off."""
    given = (args.surprise_uniform_share, args.surprise_max_copies, args.surprise_seed)
    if not args.surprise_weighting:
        if any(x is not None for x in given):
            raise ValueError("--surprise-uniform-share, --surprise-max-copies and --surprise-seed need --surprise-weighting")
        return None
    share, copies, seed = (d if x is None else x for x, d in
                           zip(given, (tn.TRAIN_SURPRISE_UNIFORM_SHARE, tn.TRAIN_SURPRISE_MAX_COPIES, tn.TRAIN_SURPRISE_SEED)))
    try:
        _, share, copies = check_surprise_options(None, share, copies)
    except ValueError as err:
        raise ValueError(f"--surprise-uniform-share / --surprise-max-copies: {err}") from None
    return share, copies, int(seed)


def _set_surprise_options(args):
    """The checked surprise-weighting flags onto train_network's constants (the stage reads them at call time)."""
    checked = _check_surprise_args(args)
    if checked is not None:
        tn.TRAIN_SURPRISE_WEIGHTING = True
        tn.TRAIN_SURPRISE_UNIFORM_SHARE, tn.TRAIN_SURPRISE_MAX_COPIES, tn.TRAIN_SURPRISE_SEED = checked


def _check_holdout_args(args):
    """--holdout-share / --holdout-seed / --holdout-every / --keep-best-epoch / --holdout-log, refused at parse time: a share outside
    (0, 1), V < 1, and any of the others without --holdout-share.  Returns (share, seed, every) with the defaults filled in, or None
    when the option is off."""
    if args.holdout_share is None:
        if args.holdout_seed is not None or args.holdout_every is not None or args.keep_best_epoch or args.holdout_log is not None:
            raise ValueError("--holdout-seed, --holdout-every, --keep-best-epoch and --holdout-log need --holdout-share")
        return None
    seed = tn.TRAIN_HOLDOUT_SEED if args.holdout_seed is None else args.holdout_seed
    every = tn.TRAIN_HOLDOUT_EVERY if args.holdout_every is None else args.holdout_every
    try:
        share, _, every = check_holdout_options(args.holdout_share, seed, every)
    except ValueError as err:
        raise ValueError(f"--holdout-share / --holdout-seed / --holdout-every: {err}") from None
    return share, int(seed), every


def _set_holdout_options(args):
    """The checked hold-out flags onto train_network's constants (the stage reads them at call time)."""
    checked = _check_holdout_args(args)
    if checked is not None:
        tn.TRAIN_HOLDOUT_SHARE, tn.TRAIN_HOLDOUT_SEED, tn.TRAIN_HOLDOUT_EVERY = checked
        tn.TRAIN_HOLDOUT_KEEP_BEST, tn.TRAIN_HOLDOUT_LOG = bool(args.keep_best_epoch), args.holdout_log


def _set_replay_options(args):
    """--replay-generations / --replay-rows / --epoch-rows / --merge-positions / --no-history-file onto self_play's and train_network's hooks: one
    ReplayWindow on this rank's GPU that self-play fills and the parameter update trains on, preloaded from the newest K .history
    files of ./data, oldest first.  Returns the window (None when off)."""
    if args.epoch_rows is not None:
        tn.TRAIN_EPOCH_ROWS = args.epoch_rows
    if args.merge_positions:
        tn.TRAIN_MERGE_POSITIONS = True
    if args.replay_generations < 0:
        raise ValueError("--replay-generations must be >= 0")
    if args.replay_generations == 0:
        if args.no_history_file or args.replay_rows is not None:
            raise ValueError("--no-history-file and --replay-rows need --replay-generations K >= 1")
        return None
    window = ReplayWindow(constants.BOARD_SIZE, max_generations=args.replay_generations, capacity_rows=args.replay_rows,
                          device=aqd.device())
    window.extend_from_files(sorted(Path('./data').glob('*.history'))[-args.replay_generations:])
    sp.SP_REPLAY = tn.TRAIN_WINDOW = window
    if args.no_history_file:
        sp.SP_WRITE_HISTORY = False
    return window


def _check_value_lambda_args(args):
    """--value-lambda, refused at parse time: a value outside [0, 1], and the flag without --value-blend L > 0 (nothing would read
    the lambda-returns).  Returns the lambda as a float, or None when the flag is not given."""
    if args.value_lambda is None:
        return None
    if not 0.0 <= args.value_lambda <= 1.0:                     # NaN fails both
        raise ValueError("--value-lambda must be in [0, 1]")
    if args.value_blend is None or not check_value_blend(args.value_blend) > 0.0:
        raise ValueError("--value-lambda needs --value-blend L > 0: the lambda-return takes the place of q in (1 - L) z + L q")
    return check_value_lambda(args.value_lambda)


def _set_target_options(args):
    """--temperature-plies / --value-blend / --value-lambda onto self_play's constants, refused here if the engine or the append would
    refuse them."""
    plies = None if args.temperature_plies is None else check_target_options(args.temperature_plies)[0]
    blend = None if args.value_blend is None else check_value_blend(args.value_blend)
    lam = _check_value_lambda_args(args)                          # a refused option sets nothing
    if plies is not None:
        sp.SP_TEMPERATURE_PLIES = plies
    if blend is not None:
        sp.SP_VALUE_BLEND = blend
    if lam is not None:
        sp.SP_VALUE_LAMBDA = lam


def _set_tree_reuse_options(args):
    """--tree-reuse / --tree-reuse-visits onto self_play's constants, refused here if the engine would refuse them."""
    if args.tree_reuse or args.tree_reuse_visits is not None:
        check_tree_reuse(args.tree_reuse, args.tree_reuse_visits, pv_mcts.PV_EVALUATE_COUNT)
        sp.SP_TREE_REUSE, sp.SP_TREE_REUSE_VISITS = True, args.tree_reuse_visits


def _set_resign_options(args):
    """--resign-threshold / --resign-min-ply / --resign-max-false-positive / --slots onto self_play's constants, refused here if the
    engine would refuse them."""
    if args.slots is not None:
        if args.slots < 1:
            raise ValueError("--slots must be >= 1")
        sp.SP_SLOTS = args.slots
    if args.resign_threshold is None:
        if args.resign_min_ply is not None or args.resign_max_false_positive is not None:
            raise ValueError("--resign-min-ply and --resign-max-false-positive need --resign-threshold")
        return
    auto = args.resign_threshold == "auto"
    try:
        threshold = 1.0 if auto else float(args.resign_threshold)
    except ValueError:
        raise ValueError(f"--resign-threshold must be a number in (0, 1] or 'auto', not {args.resign_threshold!r}") from None
    min_ply = sp.SP_RESIGN_MIN_PLY if args.resign_min_ply is None else args.resign_min_ply
    threshold, sp.SP_RESIGN_MIN_PLY, _ = check_resign(threshold, min_ply, sp.SP_RESIGN_DISABLE_FRACTION)
    if args.resign_max_false_positive is not None:
        if not auto:
            raise ValueError("--resign-max-false-positive needs --resign-threshold auto")
        if not 0.0 <= args.resign_max_false_positive < 1.0:
            raise ValueError("--resign-max-false-positive must be in [0, 1)")
        sp.SP_RESIGN_MAX_FALSE_POSITIVE = args.resign_max_false_positive
    sp.SP_RESIGN_THRESHOLD = "auto" if auto else threshold
    sp.SP_RESIGN_AUTO = {"threshold": None, "parts": []}


def _set_mirror_options(args):
    """--mirror-augment / --mirror-seed onto train_network's constants (the stages read them at call time)."""
    if args.mirror_augment:
        tn.TRAIN_MIRROR = True
    if args.mirror_seed is not None:
        tn.TRAIN_MIRROR_SEED = args.mirror_seed


def _set_optimiser_options(args):
    """--weight-decay / --coupled-weight-decay / --max-grad-norm onto train_network's constants, refused here if the step would
    refuse them."""
    if args.weight_decay is None and args.coupled_weight_decay:
        raise ValueError("--coupled-weight-decay needs --weight-decay")
    if args.weight_decay is not None:
        if not math.isfinite(args.weight_decay) or args.weight_decay < 0.0:
            raise ValueError("--weight-decay must be finite and >= 0")
        tn.TRAIN_WEIGHT_DECAY, tn.TRAIN_DECOUPLED = args.weight_decay, not args.coupled_weight_decay
    if args.max_grad_norm is not None:
        if not math.isfinite(args.max_grad_norm) or args.max_grad_norm <= 0.0:
            raise ValueError("--max-grad-norm must be finite and > 0")
        tn.TRAIN_MAX_GRAD_NORM = args.max_grad_norm


def _value_loss_weight(text):
    """argparse type of --value-loss-weight: a finite number >= 0, refused at parse time in the library's words."""
    try:
        return check_loss_controls("reference", float(text))[1]
    except ValueError as err:
        raise argparse.ArgumentTypeError(str(err)) from None


def _set_loss_options(args):
    """--policy-loss / --value-loss-weight onto train_network's constants."""
    if args.policy_loss is not None:
        tn.TRAIN_POLICY_LOSS = args.policy_loss.replace("-", "_")
    if args.value_loss_weight is not None:
        tn.TRAIN_VALUE_LOSS_WEIGHT = args.value_loss_weight


def _check_average_args(args):
    """--ema-decay / --ema-every, refused as the library refuses them."""
    if args.ema_decay is None:
        if args.ema_every is not None:
            raise ValueError("--ema-every needs --ema-decay")
        return
    try:
        check_average_controls(args.ema_decay, tn.TRAIN_EMA_EVERY if args.ema_every is None else args.ema_every)
    except ValueError as err:
        raise ValueError(f"--ema-decay / --ema-every: {err}") from None


def _set_average_options(args):
    """--ema-decay / --ema-every onto train_network's constants."""
    _check_average_args(args)
    if args.ema_decay is not None:
        tn.TRAIN_EMA_DECAY = args.ema_decay
    if args.ema_every is not None:
        tn.TRAIN_EMA_EVERY = args.ema_every


def check_args(args):
    """Every check of the parsed flags that needs no device, the first bad flag raising ValueError: what main() runs in front of
    anything that touches a GPU or the process group."""
    for check in (_check_reanalyse_args, _check_reanalyse_policy_args, _check_policy_args, _check_surprise_args, _check_holdout_args,
                  _check_start_args, _check_value_lambda_args, _check_average_args, _check_gumbel_args):
        check(args)


def apply_args(args):
    """The parsed flags onto the module constants the stages read, once this rank has its GPU (the replay window is allocated on
    it).  A flag that is not given leaves its constant alone."""
    if args.games is not None:
        sp.SP_GAME_COUNT = args.games
    if args.sims is not None:
        pv_mcts.PV_EVALUATE_COUNT = args.sims
    if args.root_noise_eps is not None:
        sp.SP_ROOT_NOISE_EPS = args.root_noise_eps
    if args.root_noise_alpha is not None:
        sp.SP_ROOT_NOISE_ALPHA = args.root_noise_alpha
    if args.epochs is not None:
        tn.NUM_EPOCH = args.epochs
    for set_options in (_set_target_options, _set_tree_reuse_options, _set_resign_options, _set_mirror_options, _set_optimiser_options,
                        _set_loss_options, _set_average_options, _set_replay_options, _set_surprise_options, _set_holdout_options,
                        _set_reanalyse_options, _set_policy_options, _set_start_options, _set_gumbel_options):
        set_options(args)
    if args.eval_games is not None:
        en.EN_GAME_COUNT = args.eval_games
